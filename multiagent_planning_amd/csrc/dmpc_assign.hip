// dmpc_assign.hip -- goal assignment ahead of a transition: which agent takes which point of the next formation (dmpc_assign_goals: N agents,
// N goals; dmpc_assign_rect: N agents, M goals).
//
// There is no reference counterpart (randomTest.m / randomExchange.m hand out labelled goals).  The rule is pinned in include/dmpc_hip.h and
// restated in numpy by tests/assign.py (square) and tests/assign_rect.py, which the device must equal bit for bit: the forward auction with
// eps-scaling in synchronous (Jacobi) rounds over the cost c(i,j) = |E1 (po_i - g_j)|^2, E1 = diag(1,1,1/c); with N != M, reverse rounds
// -- unowned objects offer themselves down to the smallest owned price -- behind the forward rounds of every eps.  Nothing in the result
// depends on launch geometry, batch size or the order the device visits anything in:
//   bidding     one wave per unassigned agent (a compacted list), lanes stride over the goals (SoA in LDS: coordinates + price, 32 B per
//               goal), per-lane top-2 of m = c + price, then a wave butterfly that merges by the total order (m ascending, j ascending)
//   resolution  bids are positive doubles, their bit patterns order as unsigned integers: atomicMax per goal finds the winning bid,
//               atomicMin over the bidders that made it finds the smallest agent
//   no dense cost matrix: costs are recomputed from the 3 + 1 doubles per goal
// Scenes of max(N, M) <= DMPC_ASSIGN_ONE_LAUNCH_MAX run in ONE launch, square or not (assign_one_kernel: one workgroup per scene, everything
// in LDS, workgroup barriers between the stages of a round).  Larger scenes, square only, take two launches per round (assign_bid_kernel
// streams the goals through LDS tile by tile, 16 bidders share a tile; assign_settle_kernel, one workgroup per scene, resolves, applies and
// keeps the phase state) and the host reads the scenes' done flags one window of rounds behind, as dmpc_transition reads its verdicts.
//
// Included into dmpc_api.hip (single translation unit).  Every kernel rounds each operation on its own (fp contraction off).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asg {

constexpr int ONE_MAX = DMPC_ASSIGN_ONE_LAUNCH_MAX;
constexpr int TILE = 2048;          // goals per LDS tile of assign_bid_kernel (64 KB)
constexpr int BID_WAVES = 16;       // bidders that share a tile
constexpr int WINDOW = 64;          // rounds the host launches between two looks at the done flags
constexpr int NONE = 0x7fffffff;
constexpr int DEFAULT_ROUNDS = 1 << 20;

struct Best { double m1, m2; int j1; };   // smallest m, smallest m over j != j1, the goal of m1
struct Top { double g1, g2; int p1; };    // largest g, largest g over p != p1, the person of g1

struct State {                      // of one scene, between the round launches
    unsigned long long cmax_bits;
    double e;
    int cnt, cur, rounds, last;     // bidders of the next round, which half of `list` holds them, rounds so far, this phase runs at eps
};

struct Work {                       // scratch of the round launches, [S][N] each ([S][2][N]: list)
    double *price, *bidv;
    unsigned long long *bidval;
    int *owner, *assigned, *bidwin, *bidj, *list;
    State *state;
    int *done;                      // [S] 0: running, 1: finished, -1: stopped at the round cap
};

__device__ inline double pair_cost(double px, double py, double pz, double gx, double gy, double gz, double cinv)
{
#pragma clang fp contract(off)
    const double dx = px - gx, dy = py - gy, dz = (pz - gz) * cinv;
    return (dx * dx + dy * dy) + dz * dz;
}

// the cost of a person and an object -- the smaller and the larger side of a scene; SWAP, more agents than goals: the persons are the goals.
// The agent goes first into pair_cost.
template <bool SWAP>
__device__ inline double rect_cost(double px, double py, double pz, double ox, double oy, double oz, double cinv)
{
    return SWAP ? pair_cost(ox, oy, oz, px, py, pz, cinv) : pair_cost(px, py, pz, ox, oy, oz, cinv);
}

// lanes stride over goals (objects) jbase .. jbase + n - 1 (ascending per lane: a strict < keeps the smallest j of equal values)
template <bool SWAP = false>
__device__ inline void scan_goals(Best &b, int lane, int n, int jbase, const double *gx, const double *gy, const double *gz, const double *pr,
                                  double px, double py, double pz, double cinv)
{
#pragma clang fp contract(off)
    for (int j = lane; j < n; j += 64) {
        const double m = rect_cost<SWAP>(px, py, pz, gx[j], gy[j], gz[j], cinv) + pr[j];
        if (m < b.m1) { b.m2 = b.m1; b.m1 = m; b.j1 = jbase + j; }
        else if (m < b.m2) b.m2 = m;
    }
}

// the merge is defined by the order (m ascending, j ascending), so every lane ends with the same bits whatever the tree
__device__ inline Best wave_best(Best b)
{
    for (int off = 1; off < 64; off <<= 1) {
        const double o1 = __shfl_xor(b.m1, off), o2 = __shfl_xor(b.m2, off);
        const int oj = __shfl_xor(b.j1, off);
        if (o1 < b.m1 || (o1 == b.m1 && oj < b.j1)) {
            b.m2 = o2 < b.m1 ? o2 : b.m1;
            b.m1 = o1; b.j1 = oj;
        } else {
            b.m2 = b.m2 < o1 ? b.m2 : o1;
        }
    }
    return b;
}

__device__ inline double make_bid(const Best &b, double price_j1, double e, int N)
{
#pragma clang fp contract(off)
    return N == 1 ? price_j1 + e : (price_j1 + (b.m2 - b.m1)) + e;
}

__device__ inline double wave_max(double v)
{
    for (int off = 1; off < 64; off <<= 1) { const double o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}

// e of the first phase / of the phase after one at e: (e, last)
__device__ inline void next_e(double cand, double eps, double &e, int &last)
{
    if (cand > eps) { e = cand; last = 0; } else { e = eps; last = 1; }
}

// The resolution of one round by ONE workgroup, on LDS or global arrays alike: lc[0 .. cnt) bid (bidj, bidv; bidval holds every goal's highest
// bid); the next round's bidders -- losers and displaced owners -- are appended to ln, counted in *n_next (zero on entry).  Leaves bidval / bidwin
// as it found them (0 / NONE).  A previous owner did not bid and a winner owned nothing, so no two threads write one agent's `assigned`.
__device__ inline void resolve_round(int cnt, const int *lc, int *ln, int *n_next, int *bidj, const double *bidv, unsigned long long *bidval,
                                     int *bidwin, int *owner, int *assigned, double *price)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int t = tid; t < cnt; t += nt) {             // the smallest agent among a goal's highest bidders
        const int i = lc[t], j = bidj[i];
        if ((unsigned long long)__double_as_longlong(bidv[i]) == bidval[j]) atomicMin(&bidwin[j], i);
    }
    __syncthreads();
    for (int t = tid; t < cnt; t += nt) {             // losers bid again next round
        const int i = lc[t];
        if (__hip_atomic_load(&bidwin[bidj[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != i) { bidj[i] = -1; ln[atomicAdd(n_next, 1)] = i; }
    }
    __syncthreads();
    for (int t = tid; t < cnt; t += nt) {             // winners take their goals
        const int i = lc[t], j = bidj[i];
        if (j >= 0) {
            const int prev = owner[j];
            if (prev >= 0) { assigned[prev] = -1; ln[atomicAdd(n_next, 1)] = prev; }
            owner[j] = i; assigned[i] = j; price[j] = bidv[i];
            bidval[j] = 0ull; bidwin[j] = NONE;
        }
    }
    __syncthreads();
}

// what a scene stopped at the round cap reports (one workgroup; owner_out: dmpc_assign_rect's, null otherwise; the caller writes the prices,
// as the rounds left them)
__device__ inline void write_capped(int N, int M, size_t s, int32_t *perm, int32_t *owner_out, double *pf, double *cost, int32_t *rounds_out)
{
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        if (perm) perm[s * N + i] = -1;
        if (pf) { pf[(s * N + i) * 3] = 0.0; pf[(s * N + i) * 3 + 1] = 0.0; pf[(s * N + i) * 3 + 2] = 0.0; }
    }
    for (int j = threadIdx.x; j < M; j += blockDim.x)
        if (owner_out) owner_out[s * M + j] = -1;
    if (threadIdx.x == 0) { if (cost) cost[s] = __builtin_nan(""); if (rounds_out) rounds_out[s] = -1; }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// max(N, M) <= ONE_MAX: the whole forward/reverse auction of a scene in one workgroup
// ---------------------------------------------------------------------------------------------------------------------------------------
// The smaller side are the n persons, the larger side the m objects (SWAP: more agents than goals, the goals are the persons; a square scene
// is n == m without SWAP and runs no reverse round).  Forward rounds: one wave per bidding person.  Reverse rounds are their mirror image: one
// wave per offering object (a compacted list), lanes stride over the persons with a per-lane top-2 of g = u - c, a butterfly that merges by
// the total order (g descending, p ascending); offers are positive doubles, so atomicMax on their bit patterns per person finds the winning
// offer and atomicMin over the objects that made it the smallest object.

// The kernel's dynamic LDS: where every column starts, in bytes, and what they take together -- the host sizes the launch from it, the kernel
// carves its pointers from it.  Every 8-byte column lies ahead of every 4-byte column, so odd n, m keep every double and every 64-bit atomic
// 8-byte aligned.  The columns that only reverse rounds use have no rows when n == m: 56 B per object + 40 B per person (96 B per agent) then,
// 76 B per object + 60 B per person otherwise.
struct OneLds {
    unsigned ox, oy, oz, pr, offd, offb, bidval, px, py, pz, bidv, u, offval;   // 8-byte columns
    unsigned owner, bidwin, offp, list, assigned, bidj, offwin;                 // 4-byte columns (list: 2 m rows)
    unsigned bytes;
    __host__ __device__ OneLds(int n, int m)
    {
        const unsigned rm = n < m ? m : 0, rn = n < m ? n : 0;   // rows of the reverse-only columns, per object and per person
        unsigned at = 0;
        auto col = [&at](unsigned rows, unsigned width) { const unsigned o = at; at += rows * width; return o; };
        ox = col(m, 8); oy = col(m, 8); oz = col(m, 8); pr = col(m, 8); offd = col(rm, 8); offb = col(rm, 8); bidval = col(m, 8);
        px = col(n, 8); py = col(n, 8); pz = col(n, 8); bidv = col(n, 8); u = col(rn, 8); offval = col(rn, 8);
        owner = col(m, 4); bidwin = col(m, 4); offp = col(rm, 4); list = col(2 * m, 4);
        assigned = col(n, 4); bidj = col(n, 4); offwin = col(rn, 4);
        bytes = at;
    }
};

struct Scene {                      // of one workgroup of assign_one_kernel
    int n, m, max_rounds;
    double cinv;
    double *ox, *oy, *oz, *pr, *offd, *offb, *px, *py, *pz, *bidv, *u;   // OneLds' columns (offd, offb, offp, u, offval, offwin: n < m only)
    unsigned long long *bidval, *offval;
    int *owner, *bidwin, *offp, *lists, *assigned, *bidj, *offwin;
    int *cnt;                       // [2] the lengths of the two lists
    double *red;                    // [16] one slot per wave
    int rounds, cur;                // rounds so far, forward and reverse; which list holds the bidding persons or offering objects
    __device__ int *list(int k) const { return lists + (size_t)k * m; }
};

// forward(e): everybody unassigned at the prices as they are, then rounds until no person is -- one wave per bidder.  False: the round cap.
template <bool SWAP>
__device__ inline bool forward_rounds(Scene &sc, double e)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int n = sc.n, m = sc.m;
    for (int o = tid; o < m; o += nt) sc.owner[o] = -1;
    for (int p = tid; p < n; p += nt) { sc.assigned[p] = -1; sc.list(sc.cur)[p] = p; }
    int cnt = n;
    __syncthreads();
    while (cnt > 0) {
        if (sc.rounds == sc.max_rounds) return false;
        ++sc.rounds;
        const int *lc = sc.list(sc.cur);
        int *ln = sc.list(sc.cur ^ 1);
        if (tid == 0) sc.cnt[sc.cur ^ 1] = 0;
        for (int t = wave; t < cnt; t += nw) {        // bids
            const int p = lc[t];
            Best b = {__builtin_inf(), __builtin_inf(), NONE};
            scan_goals<SWAP>(b, lane, m, 0, sc.ox, sc.oy, sc.oz, sc.pr, sc.px[p], sc.py[p], sc.pz[p], sc.cinv);
            b = wave_best(b);
            if (lane == 0) {
                const int o1 = b.j1 < m ? b.j1 : 0;   // (no finite value anywhere: a scene of NaNs ends at the round cap, inside the arrays)
                const double bid = make_bid(b, sc.pr[o1], e, m);
                sc.bidj[p] = o1; sc.bidv[p] = bid;
                atomicMax(&sc.bidval[o1], (unsigned long long)__double_as_longlong(bid));
            }
        }
        __syncthreads();
        resolve_round(cnt, lc, ln, &sc.cnt[sc.cur ^ 1], sc.bidj, sc.bidv, sc.bidval, sc.bidwin, sc.owner, sc.assigned, sc.pr);
        sc.cur ^= 1;
        cnt = sc.cnt[sc.cur];
    }
    return true;
}

// the merge is defined by the order (g descending, p ascending), so every lane ends with the same bits whatever the tree
__device__ inline Top wave_top(Top b)
{
    for (int off = 1; off < 64; off <<= 1) {
        const double o1 = __shfl_xor(b.g1, off), o2 = __shfl_xor(b.g2, off);
        const int op = __shfl_xor(b.p1, off);
        if (o1 > b.g1 || (o1 == b.g1 && op < b.p1)) {
            b.g2 = o2 > b.g1 ? o2 : b.g1;
            b.g1 = o1; b.p1 = op;
        } else {
            b.g2 = b.g2 > o1 ? b.g2 : o1;
        }
    }
    return b;
}

__device__ inline double wave_min(double v)
{
    for (int off = 1; off < 64; off <<= 1) { const double o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}

// reverse(e), n < m, behind forward(e): every person owns an object and sc.cnt[sc.cur] is zero on entry.  False: the round cap.
template <bool SWAP>
__device__ inline bool reverse_rounds(Scene &sc, double e)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int n = sc.n, m = sc.m;
    double lo = __builtin_inf();
    for (int p = tid; p < n; p += nt) {
        const int o = sc.assigned[p];
        sc.u[p] = rect_cost<SWAP>(sc.px[p], sc.py[p], sc.pz[p], sc.ox[o], sc.oy[o], sc.oz[o], sc.cinv) + sc.pr[o];
        lo = sc.pr[o] < lo ? sc.pr[o] : lo;
    }
    lo = wave_min(lo);
    if (lane == 0) sc.red[wave] = lo;
    __syncthreads();
    double lam = sc.red[0];                           // the smallest price of an owned object (a minimum: whatever the order)
    for (int w = 1; w < nw; ++w) lam = sc.red[w] < lam ? sc.red[w] : lam;
    for (int o = tid; o < m; o += nt)
        if (sc.owner[o] < 0 && sc.pr[o] > lam) sc.list(sc.cur)[atomicAdd(&sc.cnt[sc.cur], 1)] = o;
    __syncthreads();
    int cnt = sc.cnt[sc.cur];
    while (cnt > 0) {                                 // the list: the unowned objects priced above lam
        if (sc.rounds == sc.max_rounds) return false;
        ++sc.rounds;
        const int *lc = sc.list(sc.cur);
        int *ln = sc.list(sc.cur ^ 1);
        int *n_next = &sc.cnt[sc.cur ^ 1];
        if (tid == 0) *n_next = 0;
        for (int t = wave; t < cnt; t += nw) {        // offers
            const int o = lc[t];
            const double x = sc.ox[o], y = sc.oy[o], z = sc.oz[o];
            Top b = {-__builtin_inf(), -__builtin_inf(), NONE};
            for (int p = lane; p < n; p += 64) {      // (ascending per lane: a strict > keeps the smallest p of equal values)
                const double g = sc.u[p] - rect_cost<SWAP>(sc.px[p], sc.py[p], sc.pz[p], x, y, z, sc.cinv);
                if (g > b.g1) { b.g2 = b.g1; b.g1 = g; b.p1 = p; }
                else if (g > b.g2) b.g2 = g;
            }
            b = wave_top(b);
            if (lane == 0) {
                const int p1 = b.p1 < n ? b.p1 : 0;   // (no finite value anywhere: as in forward_rounds)
                const double beta = b.g1;
                if (lam >= beta - e) { sc.pr[o] = lam; sc.offp[o] = -1; }   // done: nobody wants it above the floor
                else {
                    const double d1 = beta - lam, d2 = (beta - b.g2) + e;   // (n == 1: g2 = -inf, d2 = inf)
                    const double delta = d1 < d2 ? d1 : d2;
                    sc.offp[o] = p1; sc.offd[o] = delta; sc.offb[o] = beta;
                    atomicMax(&sc.offval[p1], (unsigned long long)__double_as_longlong(delta));
                }
            }
        }
        __syncthreads();
        for (int t = tid; t < cnt; t += nt) {         // the smallest object among a person's largest offers
            const int o = lc[t], p = sc.offp[o];
            if (p >= 0 && (unsigned long long)__double_as_longlong(sc.offd[o]) == sc.offval[p]) atomicMin(&sc.offwin[p], o);
        }
        __syncthreads();
        for (int t = tid; t < cnt; t += nt) {         // an offer that was not taken is made again next round
            const int o = lc[t], p = sc.offp[o];
            if (p >= 0 && __hip_atomic_load(&sc.offwin[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != o) { sc.offp[o] = -1; ln[atomicAdd(n_next, 1)] = o; }
        }
        __syncthreads();
        for (int t = tid; t < cnt; t += nt) {         // persons take their offers; what they owned is unowned at its price
            const int o = lc[t], p = sc.offp[o];
            if (p >= 0) {
                const int prev = sc.assigned[p];
                sc.owner[prev] = -1;
                if (sc.pr[prev] > lam) ln[atomicAdd(n_next, 1)] = prev;
                sc.pr[o] = sc.offb[o] - sc.offd[o]; sc.u[p] = sc.u[p] - sc.offd[o];
                sc.owner[o] = p; sc.assigned[p] = o;
                sc.offval[p] = 0ull; sc.offwin[p] = NONE;
            }
        }
        __syncthreads();
        sc.cur ^= 1;
        cnt = sc.cnt[sc.cur];
    }
    return true;
}

template <bool SWAP>
__global__ __launch_bounds__(1024) void assign_one_kernel(int N, int M, const double *__restrict__ po, const double *__restrict__ goals, double cinv,
                                                          double eps, int max_rounds, int32_t *__restrict__ perm,
                                                          int32_t *__restrict__ owner_out, double *__restrict__ pf,
                                                          double *__restrict__ price_out, double *__restrict__ cost,
                                                          int32_t *__restrict__ rounds_out)
{
#pragma clang fp contract(off)
    const int n = SWAP ? M : N, m = SWAP ? N : M;     // persons, objects
    extern __shared__ double sh[];
    __shared__ unsigned long long s_cmax;
    __shared__ int s_cnt[2];
    __shared__ double s_red[16];
    const OneLds at(n, m);
    const auto f64 = [](unsigned off) { return (double *)((char *)sh + off); };
    const auto u64 = [](unsigned off) { return (unsigned long long *)((char *)sh + off); };
    const auto i32 = [](unsigned off) { return (int *)((char *)sh + off); };
    Scene sc = {n, m, max_rounds, cinv,
                f64(at.ox), f64(at.oy), f64(at.oz), f64(at.pr), f64(at.offd), f64(at.offb), f64(at.px), f64(at.py), f64(at.pz), f64(at.bidv), f64(at.u),
                u64(at.bidval), u64(at.offval),
                i32(at.owner), i32(at.bidwin), i32(at.offp), i32(at.list), i32(at.assigned), i32(at.bidj), i32(at.offwin),
                s_cnt, s_red, 0, 0};
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const size_t s = blockIdx.x;
    po += s * N * 3; goals += s * M * 3;
    const double *psrc = SWAP ? goals : po, *osrc = SWAP ? po : goals;

    for (int o = tid; o < m; o += nt) {
        sc.ox[o] = osrc[3 * o]; sc.oy[o] = osrc[3 * o + 1]; sc.oz[o] = osrc[3 * o + 2];
        sc.pr[o] = 0.0; sc.bidval[o] = 0ull; sc.bidwin[o] = NONE;
    }
    for (int p = tid; p < n; p += nt) {
        sc.px[p] = psrc[3 * p]; sc.py[p] = psrc[3 * p + 1]; sc.pz[p] = psrc[3 * p + 2];
        if (n < m) { sc.offval[p] = 0ull; sc.offwin[p] = NONE; }
    }
    if (tid == 0) { s_cmax = 0ull; s_cnt[0] = s_cnt[1] = 0; }
    __syncthreads();
    double mx = 0.0;
    for (int p = wave; p < n; p += nw)
        for (int o = lane; o < m; o += 64) {
            const double c = rect_cost<SWAP>(sc.px[p], sc.py[p], sc.pz[p], sc.ox[o], sc.oy[o], sc.oz[o], cinv);
            mx = c > mx ? c : mx;
        }
    mx = wave_max(mx);
    if (lane == 0) atomicMax(&s_cmax, (unsigned long long)__double_as_longlong(mx));   // non-negative doubles order like their bit patterns
    __syncthreads();
    const double cmax = __longlong_as_double((long long)s_cmax);

    double e; int last;
    next_e(cmax / 4.0, eps, e, last);
    bool capped;
    for (;;) {
        capped = !forward_rounds<SWAP>(sc, e) || (n < m && !reverse_rounds<SWAP>(sc, e));
        if (capped || last) break;
        next_e(e / 4.0, eps, e, last);
    }

    for (int o = tid; o < m; o += nt)
        if (price_out) price_out[s * m + o] = sc.pr[o];
    if (capped) { write_capped(N, M, s, perm, owner_out, pf, cost, rounds_out); return; }
    const int *agent_goal = SWAP ? sc.owner : sc.assigned, *goal_agent = SWAP ? sc.assigned : sc.owner;
    for (int j = tid; j < M; j += nt)
        if (owner_out) owner_out[s * M + j] = goal_agent[j];
    double *term = SWAP ? sc.offd : sc.bidv;          // per agent.  SWAP: the agents are the m objects, and n < m, so offd has its m rows
    const double *ax = SWAP ? sc.ox : sc.px, *ay = SWAP ? sc.oy : sc.py, *az = SWAP ? sc.oz : sc.pz;
    const double *gx = SWAP ? sc.px : sc.ox, *gy = SWAP ? sc.py : sc.oy, *gz = SWAP ? sc.pz : sc.oz;
    for (int i = tid; i < N; i += nt) {
        const int j = agent_goal[i];
        if (perm) perm[s * N + i] = j;
        if (pf) {                                     // an agent without a goal is sent nowhere: its start, bit for bit
            pf[(s * N + i) * 3] = j >= 0 ? gx[j] : ax[i]; pf[(s * N + i) * 3 + 1] = j >= 0 ? gy[j] : ay[i];
            pf[(s * N + i) * 3 + 2] = j >= 0 ? gz[j] : az[i];
        }
        if (j >= 0) term[i] = pair_cost(ax[i], ay[i], az[i], gx[j], gy[j], gz[j], cinv);
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < N; ++i)                   // in increasing i, one addition at a time (without SWAP every agent is a person and has a goal)
            if (!SWAP || agent_goal[i] >= 0) sum = sum + term[i];
        if (cost) cost[s] = sum;
        if (rounds_out) rounds_out[s] = sc.rounds;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// N > ONE_MAX: round launches
// ---------------------------------------------------------------------------------------------------------------------------------------
// grid (G, S), 256 threads: the largest cost of a scene (a maximum: whatever the order)
__global__ __launch_bounds__(256) void assign_cmax_kernel(int N, const double *__restrict__ po, const double *__restrict__ goals, double cinv, Work w)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t s = blockIdx.y;
    po += s * N * 3; goals += s * N * 3;
    double mx = 0.0;
    for (int i = blockIdx.x * 4 + wave; i < N; i += gridDim.x * 4) {
        const double x = po[3 * i], y = po[3 * i + 1], z = po[3 * i + 2];
        for (int j = lane; j < N; j += 64) {
            const double c = pair_cost(x, y, z, goals[3 * j], goals[3 * j + 1], goals[3 * j + 2], cinv);
            mx = c > mx ? c : mx;
        }
    }
    mx = wave_max(mx);
    if (lane == 0) atomicMax(&w.state[s].cmax_bits, (unsigned long long)__double_as_longlong(mx));
}

// every agent unassigned, every goal free, the bidders' list = everybody (one workgroup of a scene; the caller synchronises)
__device__ inline void phase_reset(int N, size_t s, const Work &w, int cur)
{
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        w.assigned[s * N + i] = -1; w.owner[s * N + i] = -1; w.list[(s * 2 + cur) * N + i] = i;
    }
}

// grid S, 1024 threads: prices zero, the first phase
__global__ __launch_bounds__(1024) void assign_begin_kernel(int N, double eps, Work w)
{
    const size_t s = blockIdx.x;
    for (int i = threadIdx.x; i < N; i += blockDim.x) { w.price[s * N + i] = 0.0; w.bidval[s * N + i] = 0ull; w.bidwin[s * N + i] = NONE; }
    phase_reset(N, s, w, 0);
    if (threadIdx.x == 0) {
        State &st = w.state[s];
        next_e(__longlong_as_double((long long)st.cmax_bits) / 4.0, eps, st.e, st.last);
        st.cnt = N; st.cur = 0; st.rounds = 0;
        w.done[s] = 0;
    }
}

// grid (G, S), BID_WAVES waves: one wave per bidder of the scene's list, the goals streamed through LDS in tiles the workgroup's bidders share
__global__ __launch_bounds__(BID_WAVES * 64) void assign_bid_kernel(int N, const double *__restrict__ po, const double *__restrict__ goals,
                                                                    double cinv, Work w)
{
#pragma clang fp contract(off)
    __shared__ double gx[TILE], gy[TILE], gz[TILE], pr[TILE];
    const size_t s = blockIdx.y;
    if (w.done[s]) return;
    const State st = w.state[s];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *lc = w.list + (s * 2 + st.cur) * N;
    const double *price = w.price + s * N;
    po += s * N * 3; goals += s * N * 3;
    for (int chunk = blockIdx.x; chunk * BID_WAVES < st.cnt; chunk += gridDim.x) {
        const int t = chunk * BID_WAVES + wave;
        const bool active = t < st.cnt;
        const int i = active ? lc[t] : 0;
        const double x = po[3 * i], y = po[3 * i + 1], z = po[3 * i + 2];
        Best b = {__builtin_inf(), __builtin_inf(), NONE};
        for (int base = 0; base < N; base += TILE) {
            const int n = N - base < TILE ? N - base : TILE;
            __syncthreads();
            for (int j = tid; j < n; j += BID_WAVES * 64) {
                gx[j] = goals[3 * (size_t)(base + j)]; gy[j] = goals[3 * (size_t)(base + j) + 1]; gz[j] = goals[3 * (size_t)(base + j) + 2];
                pr[j] = price[base + j];
            }
            __syncthreads();
            if (active) scan_goals(b, lane, n, base, gx, gy, gz, pr, x, y, z, cinv);
        }
        if (active) {
            b = wave_best(b);
            if (lane == 0) {
                const int j1 = b.j1 < N ? b.j1 : 0;
                const double bid = make_bid(b, price[j1], st.e, N);
                w.bidj[s * N + i] = j1; w.bidv[s * N + i] = bid;
                atomicMax(&w.bidval[s * N + j1], (unsigned long long)__double_as_longlong(bid));
            }
        }
    }
}

// grid S, 1024 threads: the round's resolution, the next round's bidders, the phase schedule, the round cap and -- once -- the outputs
__global__ __launch_bounds__(1024) void assign_settle_kernel(int N, const double *__restrict__ po, const double *__restrict__ goals, double cinv,
                                                             double eps, int max_rounds, Work w, int32_t *__restrict__ perm,
                                                             double *__restrict__ pf, double *__restrict__ price_out, double *__restrict__ cost,
                                                             int32_t *__restrict__ rounds_out)
{
#pragma clang fp contract(off)
    __shared__ int s_cnt;
    __shared__ double s_part[1024];
    const size_t s = blockIdx.x;
    if (w.done[s]) return;
    const State st = w.state[s];
    const int tid = threadIdx.x;
    const int *lc = w.list + (s * 2 + st.cur) * N;
    int *ln = w.list + (s * 2 + (st.cur ^ 1)) * N;
    double *price = w.price + s * N, *bidv = w.bidv + s * N;
    unsigned long long *bidval = w.bidval + s * N;
    int *owner = w.owner + s * N, *assigned = w.assigned + s * N, *bidwin = w.bidwin + s * N, *bidj = w.bidj + s * N;
    po += s * N * 3; goals += s * N * 3;
    if (tid == 0) s_cnt = 0;                          // (first added to behind resolve_round's first barrier)
    resolve_round(st.cnt, lc, ln, &s_cnt, bidj, bidv, bidval, bidwin, owner, assigned, price);
    const int cnt = s_cnt, rounds = st.rounds + 1;
    if (cnt > 0 || !st.last) {                        // another round
        const bool capped = rounds == max_rounds;
        double e = st.e; int last = st.last, cur = st.cur ^ 1, next_cnt = cnt;
        if (cnt == 0 && !capped) {                    // ... of the next phase
            next_e(st.e / 4.0, eps, e, last);
            phase_reset(N, s, w, cur);
            next_cnt = N;
        }
        if (capped) {
            for (int i = tid; i < N; i += blockDim.x)
                if (price_out) price_out[s * N + i] = price[i];
            write_capped(N, N, s, perm, nullptr, pf, cost, rounds_out);
        }
        if (tid == 0) {
            State &o = w.state[s];
            o.e = e; o.last = last; o.cur = cur; o.cnt = next_cnt; o.rounds = rounds;
            if (capped) w.done[s] = -1;
        }
        return;
    }
    // finished: the outputs; the cost in increasing i, one addition at a time (thread 0, the terms staged 1024 at a time)
    double sum = 0.0;
    for (int base = 0; base < N; base += 1024) {
        const int i = base + tid;
        if (i < N) {
            const int j = assigned[i];
            if (perm) perm[s * N + i] = j;
            if (pf) { pf[(s * N + i) * 3] = goals[3 * j]; pf[(s * N + i) * 3 + 1] = goals[3 * j + 1]; pf[(s * N + i) * 3 + 2] = goals[3 * j + 2]; }
            if (price_out) price_out[s * N + i] = price[i];
            s_part[tid] = pair_cost(po[3 * i], po[3 * i + 1], po[3 * i + 2], goals[3 * j], goals[3 * j + 1], goals[3 * j + 2], cinv);
        }
        __syncthreads();
        if (tid == 0) {
            const int n = N - base < 1024 ? N - base : 1024;
            for (int k = 0; k < n; ++k) sum = sum + s_part[k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        w.state[s].rounds = rounds;
        w.done[s] = 1;
        if (cost) cost[s] = sum;
        if (rounds_out) rounds_out[s] = rounds;
    }
}

}   // namespace asg

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------------
// rect: the dmpc_assign_rect entries (M goals of their own; the one launch only).  The square entries pass M = N.
static int assign_check(dmpc_ctx *ctx, const char *who, int S, int N, int M, const void *po, const void *goals, double eps, bool rect)
{
    if (!ctx) { g_err = std::string(who) + ": ctx is NULL"; return -1; }
    if (S < 1 || N < 1 || M < 1) FAIL(ctx, std::string(who) + (rect ? ": S, N and M must be at least 1" : ": S and N must be at least 1"));
    if (!po || !goals) FAIL(ctx, std::string(who) + ": po and goals must be given");
    if (!(eps > 0) || !std::isfinite(eps)) FAIL(ctx, std::string(who) + ": eps must be a finite positive number");
    if (rect && std::max(N, M) > asg::ONE_MAX)
        FAIL(ctx, std::string(who) + ": N = " + std::to_string(N) + " agents and M = " + std::to_string(M) + " goals: max(N, M) must not exceed " +
                      std::to_string(asg::ONE_MAX) + " (DMPC_ASSIGN_ONE_LAUNCH_MAX; larger square scenes: dmpc_assign_goals)");
    return 0;
}

// agents are the persons when N <= M, goals otherwise (SWAP)
template <bool SWAP>
static int assign_one_launch(dmpc_ctx *ctx, int S, int N, int M, const double *po, const double *goals, double eps, int cap, int32_t *perm,
                             int32_t *owner, double *pf, double *price, double *cost, int32_t *rounds, hipStream_t st)
{
    const int n = std::min(N, M), m = std::max(N, M);
    const int lds = (int)asg::OneLds(n, m).bytes;
    if (lds > ctx->max_lds_assign[SWAP]) {
        HIPCHK(ctx, hipFuncSetAttribute((const void *)asg::assign_one_kernel<SWAP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        ctx->max_lds_assign[SWAP] = lds;
    }
    hipLaunchKernelGGL(asg::assign_one_kernel<SWAP>, dim3((unsigned)S), dim3(m <= 256 ? 256 : 1024), (size_t)lds, st, N, M, po, goals,
                       1.0 / ctx->prm.c, eps, cap, perm, owner, pf, price, cost, rounds);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// the auction on device arrays, enqueued on st (owner: dmpc_assign_rect's output, null otherwise).  Scenes above the one-launch boundary --
// square, assign_check has refused the others --: the host waits for the done flags of each window of rounds while the next window is
// already enqueued, so the call returns with at most the last window's (idle) launches still in flight.
static int assign_run(dmpc_ctx *ctx, int S, int N, int M, const double *po, const double *goals, double eps, int max_rounds, int32_t *perm,
                      int32_t *owner, double *pf, double *price, double *cost, int32_t *rounds, hipStream_t st)
{
    const int cap = max_rounds <= 0 ? asg::DEFAULT_ROUNDS : max_rounds;
    if (std::max(N, M) <= asg::ONE_MAX)
        return N <= M ? assign_one_launch<false>(ctx, S, N, M, po, goals, eps, cap, perm, owner, pf, price, cost, rounds, st)
                      : assign_one_launch<true>(ctx, S, N, M, po, goals, eps, cap, perm, owner, pf, price, cost, rounds, st);
    const double cinv = 1.0 / ctx->prm.c;
    const size_t SN = (size_t)S * N;
    // price, bidv, bidval [SN] x 8 | owner, assigned, bidwin, bidj [SN] x 4, list [2 SN] x 4 | state [S] | done [S]
    const size_t bytes = SN * 48 + (size_t)S * sizeof(asg::State) + (size_t)S * 4;
    if (ctx->asg_work.ensure(bytes)) FAIL(ctx, "device allocation failed");
    asg::Work w;
    w.price = ctx->asg_work.as<double>(); w.bidv = w.price + SN; w.bidval = (unsigned long long *)(w.bidv + SN);
    w.owner = (int *)(w.bidval + SN); w.assigned = w.owner + SN; w.bidwin = w.assigned + SN; w.bidj = w.bidwin + SN; w.list = w.bidj + SN;
    w.state = (asg::State *)(w.list + 2 * SN); w.done = (int *)(w.state + S);
    HIPCHK(ctx, ctx->asg_win.ensure((size_t)2 * S));
    HIPCHK(ctx, hipMemsetAsync(w.state, 0, (size_t)S * sizeof(asg::State), st));
    const unsigned g_rows = (unsigned)std::min((N + 3) / 4, 1024), g_bid = (unsigned)std::min((N + asg::BID_WAVES - 1) / asg::BID_WAVES, 512);
    hipLaunchKernelGGL(asg::assign_cmax_kernel, dim3(g_rows, (unsigned)S), dim3(256), 0, st, N, po, goals, cinv, w);
    hipLaunchKernelGGL(asg::assign_begin_kernel, dim3((unsigned)S), dim3(1024), 0, st, N, eps, w);
    HIPCHK(ctx, hipGetLastError());
    long launched = 0;
    for (int k = 0;; ++k) {
        for (int r = 0; r < asg::WINDOW; ++r) {
            hipLaunchKernelGGL(asg::assign_bid_kernel, dim3(g_bid, (unsigned)S), dim3(asg::BID_WAVES * 64), 0, st, N, po, goals, cinv, w);
            hipLaunchKernelGGL(asg::assign_settle_kernel, dim3((unsigned)S), dim3(1024), 0, st, N, po, goals, cinv, eps, cap, w, perm, pf, price,
                               cost, rounds);
        }
        HIPCHK(ctx, hipGetLastError());
        launched += asg::WINDOW;
        HIPCHK(ctx, hipMemcpyAsync(ctx->asg_win.p + (size_t)(k & 1) * S, w.done, (size_t)S * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipEventRecord(ctx->asg_win.ev[k & 1], st));
        bool over = launched >= (long)cap;            // every scene has finished or met the cap by now
        if (!over && k >= 1) {                        // the window before this one
            HIPCHK(ctx, hipEventSynchronize(ctx->asg_win.ev[(k - 1) & 1]));
            const int32_t *d = ctx->asg_win.p + (size_t)((k - 1) & 1) * S;
            over = true;
            for (int s = 0; s < S; ++s) over = over && d[s] != 0;
        }
        if (over) {
            HIPCHK(ctx, hipEventSynchronize(ctx->asg_win.ev[k & 1]));   // the pinned flags are at rest when the call returns
            if (k >= 1) HIPCHK(ctx, hipEventSynchronize(ctx->asg_win.ev[(k - 1) & 1]));
            break;
        }
    }
    return 0;
}

// the host-pointer entries: po and goals staged into asg_io, the auction, the requested outputs copied back (owner: dmpc_assign_rect's, null
// otherwise), one synchronise
static int assign_staged(dmpc_ctx *ctx, int S, int N, int M, const double *po, const double *goals, double eps, int max_rounds, int32_t *perm,
                         int32_t *owner, double *pf, double *price, double *cost, int32_t *rounds)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t SN = (size_t)S * N, SM = (size_t)S * M, SX = (size_t)S * std::max(N, M);
    const size_t b_po = SN * 3 * sizeof(double), b_goals = SM * 3 * sizeof(double), b_pf = b_po, b_price = SX * sizeof(double),
                 b_cost = S * sizeof(double), b_perm = SN * sizeof(int32_t), b_owner = owner ? SM * sizeof(int32_t) : 0, b_rounds = S * sizeof(int32_t);
    if (ctx->asg_io.ensure(b_po + b_goals + b_pf + b_price + b_cost + b_perm + b_owner + b_rounds)) FAIL(ctx, "device allocation failed");
    char *at = (char *)ctx->asg_io.p;                 // the 8-byte arrays ahead of the 4-byte ones
    auto take = [&at](size_t bytes) { char *p = at; at += bytes; return p; };
    double *d_po = (double *)take(b_po), *d_g = (double *)take(b_goals), *d_pf = (double *)take(b_pf), *d_price = (double *)take(b_price),
           *d_cost = (double *)take(b_cost);
    int32_t *d_perm = (int32_t *)take(b_perm), *d_owner = (int32_t *)take(b_owner), *d_rounds = (int32_t *)take(b_rounds);
    HIPCHK(ctx, hipMemcpyAsync(d_po, po, b_po, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_g, goals, b_goals, hipMemcpyHostToDevice, st));
    if (assign_run(ctx, S, N, M, d_po, d_g, eps, max_rounds, perm ? d_perm : nullptr, owner ? d_owner : nullptr, pf ? d_pf : nullptr,
                   price ? d_price : nullptr, cost ? d_cost : nullptr, rounds ? d_rounds : nullptr, st))
        return -1;
    if (perm) HIPCHK(ctx, hipMemcpyAsync(perm, d_perm, b_perm, hipMemcpyDeviceToHost, st));
    if (owner) HIPCHK(ctx, hipMemcpyAsync(owner, d_owner, b_owner, hipMemcpyDeviceToHost, st));
    if (pf) HIPCHK(ctx, hipMemcpyAsync(pf, d_pf, b_pf, hipMemcpyDeviceToHost, st));
    if (price) HIPCHK(ctx, hipMemcpyAsync(price, d_price, b_price, hipMemcpyDeviceToHost, st));
    if (cost) HIPCHK(ctx, hipMemcpyAsync(cost, d_cost, b_cost, hipMemcpyDeviceToHost, st));
    if (rounds) HIPCHK(ctx, hipMemcpyAsync(rounds, d_rounds, b_rounds, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

extern "C" int dmpc_assign_goals_device(dmpc_ctx *ctx, int S, int N, const double *po, const double *goals, double eps, int max_rounds,
                                        int32_t *perm, double *pf_assigned, double *price, double *cost, int32_t *rounds, void *stream)
{
    if (assign_check(ctx, "dmpc_assign_goals_device", S, N, N, po, goals, eps, false)) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return assign_run(ctx, S, N, N, po, goals, eps, max_rounds, perm, nullptr, pf_assigned, price, cost, rounds, (hipStream_t)stream);
}

extern "C" int dmpc_assign_goals(dmpc_ctx *ctx, int S, int N, const double *po, const double *goals, double eps, int max_rounds, int32_t *perm,
                                 double *pf_assigned, double *price, double *cost, int32_t *rounds)
{
    if (assign_check(ctx, "dmpc_assign_goals", S, N, N, po, goals, eps, false)) return -1;
    return assign_staged(ctx, S, N, N, po, goals, eps, max_rounds, perm, nullptr, pf_assigned, price, cost, rounds);
}

extern "C" int dmpc_assign_rect_device(dmpc_ctx *ctx, int S, int N, int M, const double *po, const double *goals, double eps, int max_rounds,
                                       int32_t *perm, int32_t *owner, double *pf_assigned, double *price, double *cost, int32_t *rounds,
                                       void *stream)
{
    if (assign_check(ctx, "dmpc_assign_rect_device", S, N, M, po, goals, eps, true)) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return assign_run(ctx, S, N, M, po, goals, eps, max_rounds, perm, owner, pf_assigned, price, cost, rounds, (hipStream_t)stream);
}

extern "C" int dmpc_assign_rect(dmpc_ctx *ctx, int S, int N, int M, const double *po, const double *goals, double eps, int max_rounds,
                                int32_t *perm, int32_t *owner, double *pf_assigned, double *price, double *cost, int32_t *rounds)
{
    if (assign_check(ctx, "dmpc_assign_rect", S, N, M, po, goals, eps, true)) return -1;
    return assign_staged(ctx, S, N, M, po, goals, eps, max_rounds, perm, owner, pf_assigned, price, cost, rounds);
}
