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
// Re-planning during a flight (dmpc_transition_replan, dmpc_replan_routes_device; the rule is pinned in include/dmpc_hip.h, tests/replan.py
// restates it) adds three kernels, integer arithmetic behind the same cell of a point and the same blocked predicate:
//   replan_obst_kernel   the obstacle points of column k -- the scripted vehicles' samples k .. k + ahead, or the static vehicles -- gathered from
//                        the resident paths into the point buffer plan_block_kernel reads
//   replan_check_kernel  a lane per (scene, agent): the remaining legs walked on the scene's bitmask in global memory; an agent with a leg that is
//                        not clear is appended to a compacted list (a vector atomicAdd on a device-side count; the list's order is free)
//   replan_route_kernel  plan_route_kernel's body with the agent taken from that list (a workgroup whose index is not below the count returns at
//                        once: the host never reads the count) and an output stage that also restarts the agent's route state
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

// The route state a re-plan restarts (replan_route_kernel).  list / count: the agents replan_check_kernel flagged; list null: every agent, the plan
// before column 0 (replan_count = 0, replan_col = -1).  Everything but cur may be null.
struct Replan {
    const int32_t *list = nullptr, *count = nullptr;
    int k = 0;                                         // the column of the re-plan
    int32_t *cur = nullptr, *since = nullptr;          // [S][N_cmd]
    int32_t *wp_col = nullptr;                         // [S][N_cmd][W]
    double *pf = nullptr;                              // [S][N_cmd][3]: the goal the next step is solved with
    int32_t *replan_count = nullptr, *replan_col = nullptr;
};

// one workgroup per (scene, agent) -- RP: per entry of the list --, 256 or 1024 threads, 4 * ncells bytes of dynamic LDS (field, path: uint16 [ncells] each)
template <bool RP>
__device__ __forceinline__ void plan_route_body(const Grid &g, int W, int N_cmd, const double *__restrict__ po, const double *__restrict__ goals,
                                                const unsigned long long *__restrict__ mask, int words, double *__restrict__ wp,
                                                int32_t *__restrict__ n_wp, int32_t *__restrict__ plan_status, int32_t *__restrict__ hops, const Replan &rp)
{
    extern __shared__ unsigned short plan_sh[];
    __shared__ int s_flag[3], s_best;
    if (RP && rp.list && (int)blockIdx.x >= *rp.count) return;   // (the same for every thread of the workgroup, in front of every barrier)
    const int ncells = g.ncells, nx = g.n[0], ny = g.n[1], nz = g.n[2], nxy = nx * ny;
    unsigned short *field = plan_sh, *path = plan_sh + ncells;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const size_t a = RP && rp.list ? (size_t)rp.list[blockIdx.x] : (size_t)blockIdx.x, s = a / (size_t)N_cmd;
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
    if (RP) {
        // the route starts again: slot 0 -- thread 0 wrote it in every case above -- is the goal of the next step, no waypoint has been left
        if (tid == 0) {
            rp.cur[a] = 0;
            if (rp.since) rp.since[a] = rp.k;
            if (rp.pf) { rp.pf[3 * a] = out[0]; rp.pf[3 * a + 1] = out[1]; rp.pf[3 * a + 2] = out[2]; }
            if (rp.replan_count) rp.replan_count[a] = rp.list ? rp.replan_count[a] + 1 : 0;
            if (rp.replan_col) rp.replan_col[a] = rp.list ? rp.k : -1;
        }
        if (rp.wp_col)
            for (int k = tid; k < W; k += nt) rp.wp_col[a * (size_t)W + k] = -1;
    }
}

// grid S * N_cmd
__global__ __launch_bounds__(1024) void plan_route_kernel(Grid g, int W, int N_cmd, const double *__restrict__ po, const double *__restrict__ goals,
                                                          const unsigned long long *__restrict__ mask, int words, double *__restrict__ wp,
                                                          int32_t *__restrict__ n_wp, int32_t *__restrict__ plan_status, int32_t *__restrict__ hops)
{
    plan_route_body<false>(g, W, N_cmd, po, goals, mask, words, wp, n_wp, plan_status, hops, Replan{});
}

// grid S * N_cmd as well (the list has at most that many entries); po: the agents' current states x_p; wp is never null
__global__ __launch_bounds__(1024) void replan_route_kernel(Grid g, int W, int N_cmd, const double *__restrict__ x_p, const double *__restrict__ goals,
                                                            const unsigned long long *__restrict__ mask, int words, double *__restrict__ wp,
                                                            int32_t *__restrict__ n_wp, int32_t *__restrict__ plan_status, Replan rp)
{
    plan_route_body<true>(g, W, N_cmd, x_p, goals, mask, words, wp, n_wp, plan_status, nullptr, rp);
}

// obst [S][A1][M][3], A1 = ahead + 1: with a path [S][M][P][3] the samples min(k + a, P - 1), a = 0 .. ahead, of every vehicle; without one the
// static vehicles po[s][N_cmd + m] of po [S][N][3] (A1 = 1)
__global__ __launch_bounds__(256) void replan_obst_kernel(int S, int M, int P, int k, int A1, const double *__restrict__ path, const double *__restrict__ po,
                                                          int N, int N_cmd, double *__restrict__ obst)
{
    const size_t total = (size_t)S * A1 * M * 3;
    for (size_t t = blockIdx.x * (size_t)256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int d = (int)(t % 3);
        const size_t u = t / 3, m = u % (size_t)M, v = u / (size_t)M, a = v % (size_t)A1, s = v / (size_t)A1;
        if (path) {
            const long col = (long)k + (long)a;
            const size_t smp = (size_t)(col < (long)P - 1 ? col : (long)P - 1);
            obst[t] = path[((s * M + m) * (size_t)P + smp) * 3 + d];
        } else
            obst[t] = po[(s * (size_t)N + N_cmd + m) * 3 + d];
    }
}

// los_clear on a scene's bitmask, with free_i: the cells f0 and f1 are free whatever the mask says.  A leg inside one cell (L = 0) tests that cell.
__device__ inline bool los_clear_mask(const unsigned long long *__restrict__ mask, int f0, int f1, int ax, int ay, int az, int bx, int by, int bz,
                                      int nx, int nxy)
{
    const int dx = bx - ax, dy = by - ay, dz = bz - az;
    const int mx = dx < 0 ? -dx : dx, my = dy < 0 ? -dy : dy, mz = dz < 0 ? -dz : dz;
    const int L = mx > my ? (mx > mz ? mx : mz) : (my > mz ? my : mz), L2 = 2 * L;
    int qx = ax, qy = ay, qz = az, rx = L, ry = L, rz = L;
    for (int j = 0; j <= L2; ++j) {
        const int q = qx + qy * nx + qz * nxy;
        if (q != f0 && q != f1 && ((mask[q >> 6] >> (q & 63)) & 1ull)) return false;
        if (j == L2) break;                            // (the last cell is b: no step behind it)
        rx += dx; if (rx >= L2) { rx -= L2; ++qx; } else if (rx < 0) { rx += L2; --qx; }
        ry += dy; if (ry >= L2) { ry -= L2; ++qy; } else if (ry < 0) { ry += L2; --qy; }
        rz += dz; if (rz >= L2) { rz -= L2; ++qz; } else if (rz < 0) { rz += L2; --qz; }
    }
    return true;
}

// grid ceil(S * N_cmd / 256), 256 threads, a lane per agent: the legs cell(x_p) -> cell(wp[cur]) -> .. -> cell(wp[n_wp - 1]) on the scene's mask;
// the first leg that is not clear appends the agent to list[atomicAdd(count, 1)].  scene_done (or null): scenes that are over are skipped.
// count is zero on entry.  At most W legs of 2 L + 1 <= 2 max_a n_a - 1 cells each: bounded by counts known on entry.
__global__ __launch_bounds__(256) void replan_check_kernel(Grid g, int W, int N_cmd, int total, const double *__restrict__ x_p, const double *__restrict__ goals,
                                                           const double *__restrict__ wp, const int32_t *__restrict__ n_wp, const int32_t *__restrict__ cur,
                                                           const unsigned long long *__restrict__ mask, int words, const int32_t *__restrict__ scene_done,
                                                           int32_t *__restrict__ list, int32_t *count)
{
    const int ag = blockIdx.x * 256 + threadIdx.x;
    if (ag >= total) return;
    const size_t a = (size_t)ag, s = a / (size_t)N_cmd;
    if (scene_done && scene_done[s]) return;
    const int nx = g.n[0], nxy = g.n[0] * g.n[1];
    int pc[3], gc[3];
    for (int k = 0; k < 3; ++k) {
        pc[k] = cell_axis(x_p[3 * a + k], g.pmin[k], g.cell, g.n[k]);
        gc[k] = cell_axis(goals[3 * a + k], g.pmin[k], g.cell, g.n[k]);
    }
    const int f0 = pc[0] + pc[1] * nx + pc[2] * nxy, f1 = gc[0] + gc[1] * nx + gc[2] * nxy;
    const int n = n_wp[a] < W ? n_wp[a] : W, c0 = cur[a] > 0 ? cur[a] : 0;
    const unsigned long long *m = mask + s * (size_t)words;
    bool ok = true;
    for (int w = c0; w < n && ok; ++w) {
        const double *p = wp + (a * (size_t)W + w) * 3;
        int b[3];
        for (int k = 0; k < 3; ++k) b[k] = cell_axis(p[k], g.pmin[k], g.cell, g.n[k]);
        ok = los_clear_mask(m, f0, f1, pc[0], pc[1], pc[2], b[0], b[1], b[2], nx, nxy);
        pc[0] = b[0]; pc[1] = b[1]; pc[2] = b[2];
    }
    if (!ok) list[atomicAdd(count, 1)] = ag;
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

// ---- re-planning: one step on device arrays (dmpc_replan_routes_device; dmpc_transition_replan's RouteDev drives the same functions) ----
// everything a re-plan step reads and writes, on the device
struct ReplanArgs {
    pln::Grid g;
    int S = 0, N_cmd = 0, W = 0, M = 0;                // M: obstacle points per scene
    double margin = 0.0;
    const double *x_p = nullptr, *goals = nullptr, *obst = nullptr;   // [S][N_cmd][3] twice, [S][M][3]
    double *wp = nullptr;                              // [S][N_cmd][W][3]
    int32_t *n_wp = nullptr, *plan_status = nullptr;
    const int32_t *scene_done = nullptr;               // [S] or null
    pln::Replan rp;                                    // (list and count are set by replan_prepare)
};

// the scratch of a re-plan step in ctx->replan_work -- mask [S][words] | list [S * N_cmd] | count -- and the LDS limit of replan_route_kernel, once
static int replan_prepare(dmpc_ctx *ctx, ReplanArgs &r)
{
    const size_t A = (size_t)r.S * r.N_cmd, words = (size_t)(r.g.ncells + 63) / 64;
    if (ctx->replan_work.ensure((size_t)r.S * words * 8 + (A + 1) * 4)) FAIL(ctx, "device allocation failed");
    int32_t *list = (int32_t *)(ctx->replan_work.as<unsigned long long>() + (size_t)r.S * words);
    r.rp.list = list; r.rp.count = list + A;
    const int lds = 4 * r.g.ncells;
    if (lds > ctx->max_lds_replan) {
        HIPCHK(ctx, hipFuncSetAttribute((const void *)pln::replan_route_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        ctx->max_lds_replan = lds;
    }
    return 0;
}
// the blocked bitmask of every scene from r.obst
static void replan_mask(dmpc_ctx *ctx, const ReplanArgs &r, hipStream_t st)
{
    const double R = ctx->prm.rmin + r.margin;
    hipLaunchKernelGGL(pln::plan_block_kernel, dim3((unsigned)((r.g.ncells + 255) / 256), (unsigned)r.S), dim3(256), 0, st, r.g, r.M, r.obst,
                       1.0 / ctx->prm.c, R * R, ctx->replan_work.as<unsigned long long>(), (r.g.ncells + 63) / 64);
}
// the planner for every agent (flagged false: the plan before column 0) or for the agents the check flags on column k, on the current mask
static int replan_launch(dmpc_ctx *ctx, const ReplanArgs &r, bool flagged, int k, hipStream_t st)
{
    const int words = (r.g.ncells + 63) / 64, total = r.S * r.N_cmd;
    const unsigned long long *mask = r.M > 0 ? ctx->replan_work.as<unsigned long long>() : nullptr;
    pln::Replan rp = r.rp;
    rp.k = k;
    if (flagged) {
        HIPCHK(ctx, hipMemsetAsync((void *)rp.count, 0, 4, st));
        hipLaunchKernelGGL(pln::replan_check_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, r.g, r.W, r.N_cmd, total, r.x_p, r.goals,
                           (const double *)r.wp, (const int32_t *)r.n_wp, (const int32_t *)rp.cur, mask, words, r.scene_done, (int32_t *)rp.list, (int32_t *)rp.count);
    } else
        rp.list = rp.count = nullptr;
    hipLaunchKernelGGL(pln::replan_route_kernel, dim3((unsigned)total), dim3(r.g.ncells <= pln::SMALL_GRID ? 256 : 1024), (size_t)(4 * r.g.ncells), st, r.g,
                       r.W, r.N_cmd, r.x_p, r.goals, mask, words, r.wp, r.n_wp, r.plan_status, rp);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

extern "C" int dmpc_replan_routes_device(dmpc_ctx *ctx, int S, int N_cmd, int M, int W, const double *x_p, const double *goals, const double *obst,
                                         double cell, double margin, int k, double *waypoints, int32_t *n_wp, int32_t *cur, int32_t *since,
                                         int32_t *wp_col, double *pf, int32_t *plan_status, int32_t *replan_count, int32_t *replan_col,
                                         const int32_t *scene_done, void *stream)
{
    const char *who = "dmpc_replan_routes_device";
    ReplanArgs r;
    if (plan_check(ctx, who, S, N_cmd, M, W, x_p, goals, obst, cell, margin, r.g)) return -1;
    if (!waypoints || !n_wp || !cur) FAIL(ctx, std::string(who) + ": waypoints, n_wp and cur must be given");
    if (k < 0) FAIL(ctx, std::string(who) + ": k must not be negative");
    if ((size_t)S * (size_t)N_cmd * (size_t)W > (size_t)0x7fffffff) FAIL(ctx, std::string(who) + ": S * N_cmd * W overflows");
    if (ctx->grp) FAIL(ctx, std::string(who) + ": device pointers belong to ONE GPU; a DMPC_DEVICE_ALL context drives several (use the host-pointer entry points)");
    if (M == 0) return 0;   // nothing is blocked: every leg is clear
    HIPCHK(ctx, hipSetDevice(ctx->device));
    r.S = S; r.N_cmd = N_cmd; r.W = W; r.M = M; r.margin = margin;
    r.x_p = x_p; r.goals = goals; r.obst = obst; r.wp = waypoints; r.n_wp = n_wp; r.plan_status = plan_status; r.scene_done = scene_done;
    r.rp.cur = cur; r.rp.since = since; r.rp.wp_col = wp_col; r.rp.pf = pf; r.rp.replan_count = replan_count; r.rp.replan_col = replan_col;
    if (replan_prepare(ctx, r)) return -1;
    replan_mask(ctx, r, (hipStream_t)stream);
    return replan_launch(ctx, r, true, k, (hipStream_t)stream);
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
