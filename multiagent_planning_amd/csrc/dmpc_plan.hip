// dmpc_plan.hip -- route planning ahead of a transition: which way round the static vehicles every commanded agent goes (dmpc_plan_routes).
//
// There is no reference counterpart (DMPC has no global planner: an agent whose straight line is blocked by a wall of uncommanded vehicles parks
// in front of it).  The rule is pinned in include/dmpc_hip.h and restated in numpy and plain Python by tests/plan.py, which the device must
// equal bit for bit: a cell grid over the workspace, a cell blocked when its centre is inside the collision ellipsoid (rmin + margin) of an
// obstacle, a 6-connected wavefront from the goal's cell, the steepest descent with a fixed neighbour order, and a greedy line-of-sight pruning
// of the cell path.  The only floating-point work is the cell of a point, the centre of a cell and the blocked predicate (fp contraction off);
// everything else is integer arithmetic, so nothing in the result depends on launch geometry, batch size or the order the device visits anything in:
//   plan_block_kernel   the blocked predicate of every cell of a scene, one thread per cell over the obstacles, a wave's 64 answers in one word
//   plan_route_kernel   one workgroup per (scene, agent): the distance field as uint16 per cell in LDS (blocked cells are a sentinel in the same
//                       array), level-synchronous pull sweeps, the descent by one thread into a uint16 path in LDS, the pruning with a lane per
//                       candidate.  Every loop is bounded by a count known on entry: levels <= cells, descent <= hops, emissions <= min(hops, W).
//
// Included into dmpc_api.hip (single translation unit).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pln {

constexpr int MAX_CELLS = DMPC_PLAN_MAX_CELLS;
constexpr unsigned short UNL = 0xffff, BLK = 0xfffe;   // unlabelled / blocked; levels are at most MAX_CELLS - 1
constexpr int SMALL_GRID = 4096;                       // up to this many cells a workgroup has 256 threads, above 1024 (the result is the same)

struct Grid {
    double pmin[3], cell;
    int n[3], ncells;
};

__device__ inline int cell_axis(double p, double pmin, double cell, int n)
{
#pragma clang fp contract(off)
    const double f = floor((p - pmin) / cell);
    return f >= (double)(n - 1) ? n - 1 : (f > 0.0 ? (int)f : 0);
}

__device__ inline double centre_axis(int i, double pmin, double cell)
{
#pragma clang fp contract(off)
    return pmin + ((double)i + 0.5) * cell;
}

// grid (ceil(ncells / 256), S), 256 threads: bit (idx & 63) of mask[s][idx >> 6] = cell idx of scene s is blocked (idx = x + nx (y + ny z))
__global__ __launch_bounds__(256) void plan_block_kernel(Grid g, int M, const double *__restrict__ obst, double cinv, double RR,
                                                         unsigned long long *__restrict__ mask, int words)
{
#pragma clang fp contract(off)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const size_t s = blockIdx.y;
    obst += s * M * 3;
    bool blocked = false;
    if (idx < g.ncells) {
        const int x = idx % g.n[0], y = (idx / g.n[0]) % g.n[1], z = idx / (g.n[0] * g.n[1]);
        const double cx = centre_axis(x, g.pmin[0], g.cell), cy = centre_axis(y, g.pmin[1], g.cell), cz = centre_axis(z, g.pmin[2], g.cell);
        for (int m = 0; m < M; ++m) {
            const double dx = cx - obst[3 * m], dy = cy - obst[3 * m + 1], dz = (cz - obst[3 * m + 2]) * cinv;
            blocked = blocked || (dx * dx + dy * dy) + dz * dz < RR;
        }
    }
    const unsigned long long b = __ballot(blocked);
    if ((threadIdx.x & 63) == 0 && idx < g.ncells) mask[s * words + (idx >> 6)] = b;
}

// clear(a, b) of the rule: the cells (2L a + j (b - a) + L) / (2L), j = 0 .. 2L, per axis as a running quotient and remainder (|b - a| <= L,
// so a step changes a quotient by at most one)
__device__ inline bool los_clear(const unsigned short *field, int ax, int ay, int az, int bx, int by, int bz, int nx, int nxy)
{
    const int dx = bx - ax, dy = by - ay, dz = bz - az;
    const int mx = dx < 0 ? -dx : dx, my = dy < 0 ? -dy : dy, mz = dz < 0 ? -dz : dz;
    const int L = mx > my ? (mx > mz ? mx : mz) : (my > mz ? my : mz), L2 = 2 * L;
    int qx = ax, qy = ay, qz = az, rx = L, ry = L, rz = L;
    for (int j = 0; j <= L2; ++j) {
        if (field[qx + qy * nx + qz * nxy] == BLK) return false;
        rx += dx; if (rx >= L2) { rx -= L2; ++qx; } else if (rx < 0) { rx += L2; --qx; }
        ry += dy; if (ry >= L2) { ry -= L2; ++qy; } else if (ry < 0) { ry += L2; --qy; }
        rz += dz; if (rz >= L2) { rz -= L2; ++qz; } else if (rz < 0) { rz += L2; --qz; }
    }
    return true;
}

// grid S * N_cmd, 256 or 1024 threads, 4 * ncells bytes of dynamic LDS (field, path: uint16 [ncells] each)
__global__ __launch_bounds__(1024) void plan_route_kernel(Grid g, int W, int N_cmd, const double *__restrict__ po, const double *__restrict__ goals,
                                                          const unsigned long long *__restrict__ mask, int words, double *__restrict__ wp,
                                                          int32_t *__restrict__ n_wp, int32_t *__restrict__ plan_status, int32_t *__restrict__ hops)
{
    extern __shared__ unsigned short plan_sh[];
    __shared__ int s_flag[3], s_best;
    const int ncells = g.ncells, nx = g.n[0], ny = g.n[1], nz = g.n[2], nxy = nx * ny;
    unsigned short *field = plan_sh, *path = plan_sh + ncells;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const size_t a = blockIdx.x, s = a / (size_t)N_cmd;
    const double gl[3] = {goals[3 * a], goals[3 * a + 1], goals[3 * a + 2]};
    int sc[3], gc[3];
    for (int k = 0; k < 3; ++k) {
        sc[k] = cell_axis(po[3 * a + k], g.pmin[k], g.cell, g.n[k]);
        gc[k] = cell_axis(gl[k], g.pmin[k], g.cell, g.n[k]);
    }
    const int sidx = sc[0] + sc[1] * nx + sc[2] * nxy, gidx = gc[0] + gc[1] * nx + gc[2] * nxy;

    // free_i: the scene's blocked cells, but for the agent's own start and goal cells
    for (int idx = tid; idx < ncells; idx += nt)
        field[idx] = mask && ((mask[s * words + (idx >> 6)] >> (idx & 63)) & 1ull) ? BLK : UNL;
    if (tid == 0) { s_flag[0] = s_flag[1] = s_flag[2] = 0; s_best = 0; }
    __syncthreads();
    if (tid == 0) { field[sidx] = UNL; field[gidx] = 0; }
    __syncthreads();

    // the field: level L + 1 = the unlabelled free cells with a neighbour at level L.  A thread's cells are tid, tid + nt, ..: their coordinates
    // advance by a fixed step with carries.  Flag of a level (three take turns, so that the one a level sets is cleared two barriers earlier):
    // bit 0 some cell joined, bit 1 the start cell did -- read once behind the barrier, so every wave takes the same exit.
    if (sidx != gidx) {
        const int x0 = tid % nx, y0 = (tid / nx) % ny, z0 = tid / nxy, ax = nt % nx, ay = (nt / nx) % ny, az = nt / nxy;
        int slot = 0;
        for (int L = 0; L < ncells; ++L) {
            const int next = slot == 2 ? 0 : slot + 1;
            if (tid == 0) s_flag[next] = 0;
            const unsigned short lv = (unsigned short)L;
            int x = x0, y = y0, z = z0, got = 0;
            for (int idx = tid; idx < ncells; idx += nt) {
                const int far = (x < gc[0] ? gc[0] - x : x - gc[0]) + (y < gc[1] ? gc[1] - y : y - gc[1]) + (z < gc[2] ? gc[2] - z : z - gc[2]);
                // (a level is at least the cell's city-block distance from the goal: cells beyond L + 1 are not even read.)  Six independent
                // reads; a missing neighbour reads the cell itself, which is no level
                if (far <= L + 1 && field[idx] == UNL) {
                    const unsigned short a0 = field[x > 0 ? idx - 1 : idx], a1 = field[x < nx - 1 ? idx + 1 : idx];
                    const unsigned short a2 = field[y > 0 ? idx - nx : idx], a3 = field[y < ny - 1 ? idx + nx : idx];
                    const unsigned short a4 = field[z > 0 ? idx - nxy : idx], a5 = field[z < nz - 1 ? idx + nxy : idx];
                    if ((a0 == lv) | (a1 == lv) | (a2 == lv) | (a3 == lv) | (a4 == lv) | (a5 == lv)) {
                        field[idx] = (unsigned short)(L + 1);
                        got |= idx == sidx ? 3 : 1;
                    }
                }
                x += ax; if (x >= nx) { x -= nx; ++y; }
                y += ay; if (y >= ny) { y -= ny; ++z; }
                z += az;
            }
            if (got) atomicOr(&s_flag[slot], got);
            __syncthreads();
            const int f = s_flag[slot];
            if (!(f & 1) || (f & 2)) break;
            slot = next;
        }
    }
    const unsigned short ds = field[sidx];             // (nobody writes the field behind the last barrier)
    const bool reachable = ds != UNL;
    const int H = reachable ? (int)ds : 0;

    // the descent: from c_t the first neighbour in the order -x, +x, -y, +y, -z, +z one level down
    if (tid == 0) {
        int x = sc[0], y = sc[1], z = sc[2], idx = sidx;
        path[0] = (unsigned short)idx;
        for (int t = 0; t < H; ++t) {
            const unsigned short want = (unsigned short)(H - t - 1);
            if (x > 0 && field[idx - 1] == want) { idx -= 1; --x; }
            else if (x < nx - 1 && field[idx + 1] == want) { idx += 1; ++x; }
            else if (y > 0 && field[idx - nx] == want) { idx -= nx; --y; }
            else if (y < ny - 1 && field[idx + nx] == want) { idx += nx; ++y; }
            else if (z > 0 && field[idx - nxy] == want) { idx -= nxy; --z; }
            else if (z < nz - 1 && field[idx + nxy] == want) { idx += nxy; ++z; }
            path[t + 1] = (unsigned short)idx;
        }
    }
    __syncthreads();

    // the pruning: from the anchor t0 the largest t that is t0 + 1 or in line of sight.  Candidates from H downwards, a wave per chunk of 64 and
    // a lane per candidate (lane 0 the largest t of its chunk); s_best only ever grows, so "found" is s_best > t0 and it is never set back.
    double *out = wp ? wp + a * (size_t)W * 3 : nullptr;
    int n_em = 0, t0 = 0;
    bool truncated = false;
    while (t0 != H) {
        const int ai = path[t0], az_ = ai / nxy, ay_ = (ai - az_ * nxy) / nx, ax_ = ai - az_ * nxy - ay_ * nx;
        const int nchunks = (H - t0 + 63) >> 6;
        int t1 = t0 + 1;
        for (int c0 = 0; c0 < nchunks; c0 += nw) {
            const int c = c0 + wave, t = H - (c << 6) - lane;
            bool ok = false;
            if (c < nchunks && t > t0) {
                ok = t == t0 + 1;
                if (!ok) {
                    const int bi = path[t], bz = bi / nxy, by = (bi - bz * nxy) / nx, bx = bi - bz * nxy - by * nx;
                    ok = los_clear(field, ax_, ay_, az_, bx, by, bz, nx, nxy);
                }
            }
            const unsigned long long b = __ballot(ok);
            if (b && lane == 0) atomicMax(&s_best, H - (c << 6) - (int)__builtin_ctzll(b));
            __syncthreads();
            t1 = s_best;
            __syncthreads();
            if (t1 > t0) break;
        }
        if (t1 <= t0) t1 = t0 + 1;                     // (t0 + 1 is a candidate of the last chunk: never taken)
        ++n_em;
        if (n_em == W && t1 != H) {                    // more emissions than slots: the goal takes the last one
            truncated = true;
            if (tid == 0 && out) { double *o = out + 3 * (size_t)(W - 1); o[0] = gl[0]; o[1] = gl[1]; o[2] = gl[2]; }
            break;
        }
        if (tid == 0 && out) {
            double *o = out + 3 * (size_t)(n_em - 1);
            if (t1 == H) { o[0] = gl[0]; o[1] = gl[1]; o[2] = gl[2]; }
            else {
                const int bi = path[t1], bz = bi / nxy, by = (bi - bz * nxy) / nx, bx = bi - bz * nxy - by * nx;
                o[0] = centre_axis(bx, g.pmin[0], g.cell); o[1] = centre_axis(by, g.pmin[1], g.cell); o[2] = centre_axis(bz, g.pmin[2], g.cell);
            }
        }
        t0 = t1;
    }
    const int count = n_em > 0 ? n_em : 1;             // no way, or start and goal in one cell: the goal alone
    if (out)
        for (int k = (n_em > 0 ? n_em : 0) + tid; k < W; k += nt) { out[3 * (size_t)k] = gl[0]; out[3 * (size_t)k + 1] = gl[1]; out[3 * (size_t)k + 2] = gl[2]; }
    if (tid == 0) {
        if (n_wp) n_wp[a] = count;
        if (plan_status) plan_status[a] = !reachable ? DMPC_PLAN_UNREACHABLE : (truncated ? DMPC_PLAN_TRUNCATED : DMPC_PLAN_OK);
        if (hops) hops[a] = reachable ? H : -1;
    }
}

}   // namespace pln

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------------
static int plan_check(dmpc_ctx *ctx, const char *who, int S, int N_cmd, int M, int W, const void *po, const void *goals, const void *obst, double cell,
                      double margin, pln::Grid &g)
{
    if (!ctx) { g_err = std::string(who) + ": ctx is NULL"; return -1; }
    if (S < 1 || N_cmd < 1) FAIL(ctx, std::string(who) + ": S and N_cmd must be at least 1");
    if (M < 0) FAIL(ctx, std::string(who) + ": M must not be negative");
    if (W < 1) FAIL(ctx, std::string(who) + ": W must be at least 1");
    if ((size_t)S * (size_t)N_cmd > (size_t)0x7fffffff) FAIL(ctx, std::string(who) + ": S * N_cmd must fit one launch");
    if (!po || !goals) FAIL(ctx, std::string(who) + ": po_cmd and goals must be given");
    if (M > 0 && !obst) FAIL(ctx, std::string(who) + ": obst is NULL with M > 0");
    if (!std::isfinite(cell) || !(cell > 0)) FAIL(ctx, std::string(who) + ": cell must be a finite positive number");
    if (!std::isfinite(margin) || margin < 0) FAIL(ctx, std::string(who) + ": margin must be a finite number, not negative");
    double total = 1.0, na[3];
    for (int k = 0; k < 3; ++k) {
        na[k] = std::max(1.0, std::ceil((ctx->prm.pmax[k] - ctx->prm.pmin[k]) / cell));
        total *= na[k];
    }
    if (!(total <= (double)pln::MAX_CELLS)) {
        char buf[200];
        snprintf(buf, sizeof buf, total < 1e15 ? ": the grid has %.0f x %.0f x %.0f = %.0f cells, more than %d" : ": the grid has %.3g x %.3g x %.3g = %.3g cells, more than %d",
                 na[0], na[1], na[2], total, pln::MAX_CELLS);
        FAIL(ctx, std::string(who) + buf);
    }
    for (int k = 0; k < 3; ++k) { g.pmin[k] = ctx->prm.pmin[k]; g.n[k] = (int)na[k]; }
    g.cell = cell;
    g.ncells = g.n[0] * g.n[1] * g.n[2];
    return 0;
}

// the planner on device arrays, enqueued on st
static int plan_run(dmpc_ctx *ctx, const pln::Grid &g, int S, int N_cmd, int M, int W, const double *po, const double *goals, const double *obst,
                    double margin, double *wp, int32_t *n_wp, int32_t *plan_status, int32_t *hops, hipStream_t st)
{
    const int words = (g.ncells + 63) / 64;
    unsigned long long *mask = nullptr;
    if (M > 0) {
        if (ctx->plan_mask.ensure((size_t)S * words * 8)) FAIL(ctx, "device allocation failed");
        mask = ctx->plan_mask.as<unsigned long long>();
        const double R = ctx->prm.rmin + margin;
        hipLaunchKernelGGL(pln::plan_block_kernel, dim3((unsigned)((g.ncells + 255) / 256), (unsigned)S), dim3(256), 0, st, g, M, obst,
                           1.0 / ctx->prm.c, R * R, mask, words);
    }
    const int lds = 4 * g.ncells;
    if (lds > ctx->max_lds_plan) {
        HIPCHK(ctx, hipFuncSetAttribute((const void *)pln::plan_route_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        ctx->max_lds_plan = lds;
    }
    hipLaunchKernelGGL(pln::plan_route_kernel, dim3((unsigned)((size_t)S * N_cmd)), dim3(g.ncells <= pln::SMALL_GRID ? 256 : 1024), (size_t)lds, st, g,
                       W, N_cmd, po, goals, mask, words, wp, n_wp, plan_status, hops);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

extern "C" int dmpc_plan_routes_device(dmpc_ctx *ctx, int S, int N_cmd, int M, int W, const double *po_cmd, const double *goals, const double *obst,
                                       double cell, double margin, double *waypoints, int32_t *n_wp, int32_t *plan_status, int32_t *hops,
                                       void *stream)
{
    pln::Grid g;
    if (plan_check(ctx, "dmpc_plan_routes_device", S, N_cmd, M, W, po_cmd, goals, obst, cell, margin, g)) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return plan_run(ctx, g, S, N_cmd, M, W, po_cmd, goals, obst, margin, waypoints, n_wp, plan_status, hops, (hipStream_t)stream);
}

extern "C" int dmpc_plan_routes(dmpc_ctx *ctx, int S, int N_cmd, int M, int W, const double *po_cmd, const double *goals, const double *obst,
                                double cell, double margin, double *waypoints, int32_t *n_wp, int32_t *plan_status, int32_t *hops)
{
    pln::Grid g;
    if (plan_check(ctx, "dmpc_plan_routes", S, N_cmd, M, W, po_cmd, goals, obst, cell, margin, g)) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t SN = (size_t)S * N_cmd, SM = (size_t)S * M;
    // po, goals [SN][3] | obst [SM][3] | waypoints [SN][W][3] | n_wp, plan_status, hops [SN]
    if (ctx->plan_io.ensure(SN * 48 + SM * 24 + SN * W * 24 + SN * 12)) FAIL(ctx, "device allocation failed");
    double *d_po = ctx->plan_io.as<double>(), *d_g = d_po + 3 * SN, *d_ob = d_g + 3 * SN, *d_wp = d_ob + 3 * SM;
    int32_t *d_n = (int32_t *)(d_wp + 3 * SN * W), *d_st = d_n + SN, *d_h = d_st + SN;
    HIPCHK(ctx, hipMemcpyAsync(d_po, po_cmd, SN * 24, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_g, goals, SN * 24, hipMemcpyHostToDevice, st));
    if (M > 0) HIPCHK(ctx, hipMemcpyAsync(d_ob, obst, SM * 24, hipMemcpyHostToDevice, st));
    if (plan_run(ctx, g, S, N_cmd, M, W, d_po, d_g, d_ob, margin, waypoints ? d_wp : nullptr, n_wp ? d_n : nullptr, plan_status ? d_st : nullptr,
                 hops ? d_h : nullptr, st))
        return -1;
    if (waypoints) HIPCHK(ctx, hipMemcpyAsync(waypoints, d_wp, SN * W * 24, hipMemcpyDeviceToHost, st));
    if (n_wp) HIPCHK(ctx, hipMemcpyAsync(n_wp, d_n, SN * 4, hipMemcpyDeviceToHost, st));
    if (plan_status) HIPCHK(ctx, hipMemcpyAsync(plan_status, d_st, SN * 4, hipMemcpyDeviceToHost, st));
    if (hops) HIPCHK(ctx, hipMemcpyAsync(hops, d_h, SN * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}
