// tables_main.cpp -- the library's table arithmetic (csrc/dmpc_tables.hip) as a plain C++ program, for tests/test_tables_cpu.py.
// stdin: one parameter set per line, "variant h Q1 S1 Qfar Qnear Sfree"; stdout: per set TAB_ALL_DOUBLES doubles, then hsum[3], raw.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dmpc_hip.h"
#define __host__
#define __device__
#include "dmpc_device.h"

using namespace dmpc;
static thread_local std::string g_err;   // what dmpc_tables.hip takes from the context file

#include "dmpc_tables.hip"

int main()
{
    dmpc_params p;
    memset(&p, 0, sizeof(p));
    p.K = K;
    std::vector<double> t(TAB_ALL_DOUBLES);
    double hsum[3];
    while (scanf("%d %lf %lf %lf %lf %lf %lf", &p.variant, &p.h, &p.Q1, &p.S1, &p.Qfar, &p.Qnear, &p.Sfree) == 7) {
        build_tables(p, t.data(), hsum);
        if (fwrite(t.data(), sizeof(double), t.size(), stdout) != t.size() || fwrite(hsum, sizeof(double), 3, stdout) != 3) return 1;
    }
    return 0;
}
