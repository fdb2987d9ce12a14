// dmpc_postcheck.hip -- whole-transition post-checks on the device.
//
// What the reference does after every transition (test/failure_rate.m:136-195, same block in comp_kctr.m,
// comp_hardsoft2.m, dmpc_soft_bound.m:152-190): rescale the MPC solution to the velocity / acceleration limits,
// interpolate at 100 Hz with MATLAB `spline` (not-a-knot cubic), check every agent pair for an ellipsoidal
// collision, and measure path length and trajectory time.  Histories are laid out [S][N][KT_alloc][3] (the
// layout dmpc_transition records), so one (scene, agent, axis) series has stride 3 doubles.
//
// Included into dmpc_api.hip (single translation unit).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pc {

__device__ __forceinline__ double block_min(double v, double *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (t < s) sh[t] = fmin(sh[t], sh[t + s]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
// the tail of every per-scene minimum of squared distances: the minimum is order independent, so an integer atomicMin on the
// (non-negative) double's bit pattern is exact
__device__ __forceinline__ void scene_min(double m, double *sh, unsigned long long *__restrict__ mind2)
{
    m = block_min(m, sh);
    if (threadIdx.x == 0 && m < INFINITY) atomicMin(mind2, (unsigned long long)__double_as_longlong(m));
}

// r_factor = min over agents and knots of min(amax/|a_k|, vmax/|v_k|)   (failure_rate.m:138-145)
__global__ void rfactor_kernel(int N, int KTa, const int *__restrict__ kt_used, const double *__restrict__ vk,
                               const double *__restrict__ ak, double vmax, double amax, double *__restrict__ rf)
{
    __shared__ double sh[256];
    const int s = blockIdx.x, KT = kt_used[s];
    double m = INFINITY;
    for (int e = threadIdx.x; e < N * KT; e += blockDim.x) {
        const int i = e / KT, k = e - i * KT;
        const size_t o = (((size_t)s * N + i) * KTa + k) * 3;
        const double an = sqrt(ak[o] * ak[o] + ak[o + 1] * ak[o + 1] + ak[o + 2] * ak[o + 2]);
        const double vn = sqrt(vk[o] * vk[o] + vk[o + 1] * vk[o + 1] + vk[o + 2] * vk[o + 2]);
        m = fmin(m, fmin(amax / an, vmax / vn));
    }
    m = block_min(m, sh);
    if (threadIdx.x == 0) rf[s] = m;
}

// a_k *= r; v_{k+1} = v_k + hs a_k; p_{k+1} = p_k + hs v_k + hs^2/2 a_k   (failure_rate.m:156-162)
// one thread per (scene, agent, axis); writes the rescaled knots y (and v, a) in place
__global__ void rescale_kernel(int S, int N, int KTa, const int *__restrict__ kt_used, const double *__restrict__ rf,
                               const double *__restrict__ hs, double *__restrict__ pk, double *__restrict__ vk,
                               double *__restrict__ ak)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)S * N * 3) return;
    const int ax = (int)(g % 3);
    const size_t sa = g / 3;
    const int s = (int)(sa / N);
    const int KT = kt_used[s];
    const double r = rf[s], h = hs[s], h22 = h * h / 2;
    const size_t o = sa * (size_t)KTa * 3 + ax;
    double p = pk[o], v = vk[o];
    for (int k = 0; k + 1 < KT; ++k) {
        const double a = ak[o + (size_t)k * 3] * r;
        ak[o + (size_t)k * 3] = a;
        const double vn = v + h * a;
        p = p + h * v + h22 * a;
        v = vn;
        vk[o + (size_t)(k + 1) * 3] = v;
        pk[o + (size_t)(k + 1) * 3] = p;
    }
}

// Not-a-knot cubic spline on uniform knots (MATLAB spline(tk, y)): second derivatives M_k of one series.
//   M0 - 2 M1 + M2 = 0,  M_{k-1} + 4 M_k + M_{k+1} = 6 (y_{k+1} - 2 y_k + y_{k-1}) / h^2,  same at the far end.
// Eliminating the end rows gives M_1 = d_1/6, M_{n-2} = d_{n-2}/6 and a (1,4,1) system for 2..n-3 (Thomas).
// one thread per (scene, agent, axis); `w` is per-series scratch of the same shape as M
__global__ void spline_kernel(int S, int N, int KTa, const int *__restrict__ kt_used, const double *__restrict__ hs,
                              const double *__restrict__ y, double *__restrict__ M, double *__restrict__ w)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)S * N * 3) return;
    const int ax = (int)(g % 3);
    const size_t sa = g / 3;
    const int s = (int)(sa / N);
    const int n = kt_used[s];
    const size_t o = sa * (size_t)KTa * 3 + ax;
    const double *Y = y + o;   // knot k of the series: [3 * k]
    double *MM = M + o, *W = w + o;
    if (n < 4) {   // spline() degenerates to the parabola / line through the points: constant second derivative
        const double h = hs[s];
        const double m = (n == 3) ? (Y[6] - 2 * Y[3] + Y[0]) / (h * h) : 0.0;
        for (int k = 0; k < n; ++k) MM[3 * k] = m;
        return;
    }
    const double s6 = 6.0 / (hs[s] * hs[s]);
    const double m1 = (Y[6] - 2 * Y[3] + Y[0]) * s6 / 6.0;
    const double me = (Y[3 * (n - 1)] - 2 * Y[3 * (n - 2)] + Y[3 * (n - 3)]) * s6 / 6.0;
    MM[3] = m1;
    MM[3 * (n - 2)] = me;
    // forward sweep over 2..n-3
    double cp = 0.0, dp = 0.0;
    for (int k = 2; k <= n - 3; ++k) {
        double d = (Y[3 * (k + 1)] - 2 * Y[3 * k] + Y[3 * (k - 1)]) * s6;
        if (k == 2) d -= m1;
        if (k == n - 3) d -= me;
        const double den = 4.0 - ((k == 2) ? 0.0 : cp);
        cp = 1.0 / den;
        dp = (d - ((k == 2) ? 0.0 : dp)) / den;
        W[3 * k] = cp;
        MM[3 * k] = dp;
    }
    for (int k = n - 4; k >= 2; --k) MM[3 * k] = MM[3 * k] - W[3 * k] * MM[3 * (k + 1)];
    MM[0] = 2 * MM[3] - MM[6];
    MM[3 * (n - 1)] = 2 * MM[3 * (n - 2)] - MM[3 * (n - 3)];
}

// The spline of one series at t: the interval k of t (clamped to the knots, so the end intervals extrapolate) and u = t - t_k once, then the
// cubic of one axis.  `o`: the offset of the series' knot 0, axis included, in y and M.
__device__ __forceinline__ int spline_interval(int n, double h, double t, double &u)
{
    int k = (int)floor(t / h);
    k = k < 0 ? 0 : (k > n - 2 ? n - 2 : k);
    u = t - k * h;
    return k;
}
__device__ __forceinline__ double spline_axis(const double *__restrict__ y, const double *__restrict__ M, size_t o, int k, double h, double u)
{
    const size_t q = o + (size_t)k * 3;
    const double y0 = y[q], y1 = y[q + 3], m0 = M[q], m1 = M[q + 3];
    const double b = (y1 - y0) / h - h * (2 * m0 + m1) / 6.0;
    return y0 + u * (b + u * (m0 / 2 + u * (m1 - m0) / (6.0 * h)));
}
struct P3 { double x, y, z; };
// the three axes of one (scene, vehicle) series [KTa][3] that starts at `o`
__device__ __forceinline__ P3 spline_eval(const double *__restrict__ y, const double *__restrict__ M, size_t o, int n, double h, double t)
{
    double u;
    const int k = spline_interval(n, h, t, u);
    return P3{spline_axis(y, M, o, k, h, u), spline_axis(y, M, o + 1, k, h, u), spline_axis(y, M, o + 2, k, h, u)};
}

// squared ellipsoidal distance |E1 (p_i - p_j)|^2 of one pair (failure_rate.m:172): ONE expression with pinned contractions for
// every kernel that evaluates it, so the brute-force and the cell-grid search return the same bits
__device__ __forceinline__ double pair_d2(double xi, double yi, double zi, double xj, double yj, double zj, double cinv)
{
    const double dx = xi - xj, dy = yi - yj, dz = (zi - zj) * cinv;
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

#define PC_SAMPLES_PER_BLOCK 8
// pairwise ellipsoidal distance at every 100 Hz sample (failure_rate.m:165-181): block = (sample group, scene);
// positions of all agents at one sample are staged in LDS, pairs are strided over the threads (thread per component: one axis each).
__global__ void pairdist_kernel(int N, int KTa, const int *__restrict__ kt_used, const double *__restrict__ hs,
                                const int *__restrict__ ns, double Ts, double cinv, const double *__restrict__ y,
                                const double *__restrict__ M, unsigned long long *__restrict__ mind2,
                                double *__restrict__ p_interp, int ns_alloc)
{
    extern __shared__ double pos[];   // [N][3]
    __shared__ double sh[256];
    const int s = blockIdx.y, n = kt_used[s], nsamp = ns[s];
    const double h = hs[s];
    double m = INFINITY;
    for (int q = 0; q < PC_SAMPLES_PER_BLOCK; ++q) {
        const int smp = blockIdx.x * PC_SAMPLES_PER_BLOCK + q;
        if (smp >= nsamp) break;
        double u;
        const int k = spline_interval(n, h, smp * Ts, u);
        for (int e = threadIdx.x; e < N * 3; e += blockDim.x) {
            const size_t o = ((size_t)s * N + e / 3) * (size_t)KTa * 3 + e % 3;
            const double v = spline_axis(y, M, o, k, h, u);
            pos[e] = v;
            if (p_interp && smp < ns_alloc) p_interp[(((size_t)s * N + e / 3) * ns_alloc + smp) * 3 + e % 3] = v;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < N * N; e += blockDim.x) {
            const int i = e / N, j = e - i * N;
            if (j <= i) continue;
            m = fmin(m, pair_d2(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], cinv));
        }
        __syncthreads();
    }
    scene_min(m, sh, &mind2[s]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Large scenes (N > PC_BRUTE_MAX): the all-pairs search of failure_rate.m:170-181 is O(N^2) per 100 Hz sample -- 5e7 pairs x
// 3 000 samples at N = 10^4.  Per (scene, sample) the agents are binned into a uniform grid whose cells are `edge` wide in
// the metric of the check (x, y, z / c): two agents closer than `edge` lie in the same or in adjacent cells, so testing
// the 27-neighbourhood finds EVERY pair with distance < edge, and each of those is evaluated with the exact fp64 expression
// of the brute-force search.  Hence: if the minimum the grid search returns is <= edge it is the scene's exact minimum
// (bit for bit what the brute force returns: a minimum does not depend on the order of its operands); if it is larger or no
// pair was found at all, no pair is closer than edge >= 2 rmin -- the verdict "no violation" is already proven, and the
// scene is searched again by brute force only to report the exact `min_dist`.  Cell indices are clamped to the grid, which
// keeps adjacency (clamping is monotone and non-expansive), so positions outside the workspace cost candidates, not
// correctness.  A batch of SB samples is processed per pass: evaluate + count, exclusive scan, scatter, search.
struct Grid {
    int nx, ny, nz;
    double x0, y0, z0;      // lower corner
    double inv_e, inv_ez;   // 1 / edge (x, y) and 1 / (edge c) (z)
};
#define PC_BRUTE_MAX 256

// the cell of a point: floor, clamped to the grid
__device__ __forceinline__ int grid_cell(const Grid &g, double x, double y, double z)
{
    int ix = (int)floor((x - g.x0) * g.inv_e), iy = (int)floor((y - g.y0) * g.inv_e), iz = (int)floor((z - g.z0) * g.inv_ez);
    ix = ix < 0 ? 0 : (ix >= g.nx ? g.nx - 1 : ix);
    iy = iy < 0 ? 0 : (iy >= g.ny ? g.ny - 1 : iy);
    iz = iz < 0 ? 0 : (iz >= g.nz ? g.nz - 1 : iz);
    return ix + g.nx * (iy + g.ny * iz);
}

// The table of points of a batch of samples, pts[S][SB][N][3]: thread per (scene, sample smp0 + b of the batch, column).  Columns < Nc are the
// commanded agents' spline (knots y / M [S][Nc][KTa][3]), the others the static positions po_static[S][N-Nc][3] or, with yk, the scripted
// vehicles' spline on the knots yk / Mk [S][N-Nc][KTa][3].  Options: with_grid, the point's cell -> cell_of and its count -> fill; p_interp
// [S][Nc][ns_alloc][3] and p_scripted [S][N-Nc][ns_alloc][3], the interpolated positions of the two kinds of column (null: none).  A sample at or
// beyond the scene's end writes cell_of = -1 with the grid and nothing else.
__global__ void sample_table_kernel(int S, int N, int Nc, int KTa, const int *__restrict__ kt_used, const double *__restrict__ hs,
                                    const int *__restrict__ ns, double Ts, int smp0, int SB, const double *__restrict__ y,
                                    const double *__restrict__ M, const double *__restrict__ po_static, const double *__restrict__ yk,
                                    const double *__restrict__ Mk, int with_grid, Grid g, double *__restrict__ pts, int *__restrict__ cell_of,
                                    int *__restrict__ fill, double *__restrict__ p_interp, double *__restrict__ p_scripted, int ns_alloc)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)S * SB * N) return;
    const int j = (int)(t % N);
    const int b = (int)((t / N) % SB), s = (int)(t / ((size_t)N * SB));
    const int smp = smp0 + b;
    if (smp >= ns[s]) { if (with_grid) cell_of[t] = -1; return; }
    const int n = kt_used[s];
    const double h = hs[s], tt = smp * Ts;
    const size_t v = j < Nc ? (size_t)s * Nc + j : (size_t)s * (N - Nc) + (j - Nc);   // the column's row in its own arrays
    P3 p;
    if (j < Nc) p = spline_eval(y, M, v * (size_t)KTa * 3, n, h, tt);
    else if (yk) p = spline_eval(yk, Mk, v * (size_t)KTa * 3, n, h, tt);
    else p = P3{po_static[3 * v], po_static[3 * v + 1], po_static[3 * v + 2]};
    pts[3 * t] = p.x; pts[3 * t + 1] = p.y; pts[3 * t + 2] = p.z;
    double *out = j < Nc ? p_interp : p_scripted;
    if (out && smp < ns_alloc) {
        double *d = out + (v * ns_alloc + smp) * 3;
        d[0] = p.x; d[1] = p.y; d[2] = p.z;
    }
    if (!with_grid) return;
    const int c = grid_cell(g, p.x, p.y, p.z);
    cell_of[t] = c;
    atomicAdd(&fill[((size_t)s * SB + b) * ((size_t)g.nx * g.ny * g.nz) + c], 1);
}
// (the exclusive prefix of the counts, block per (scene, sample): dmpc::grid_scan_kernel, dmpc_lists.hip)
// thread per (scene, sample, agent): slot of the agent in its cell (the order inside a cell is arbitrary: only a minimum is taken)
__global__ void grid_scatter_kernel(size_t total, int N, int ncell, const int *__restrict__ cell_of, const int *__restrict__ start,
                                    int *__restrict__ fill, int *__restrict__ sorted)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = cell_of[t];
    if (c < 0) return;
    const size_t sb = t / N;
    const int slot = start[sb * (ncell + 1) + c] + atomicAdd(&fill[sb * ncell + c], 1);
    sorted[sb * N + slot] = (int)(t % N);
}
// f(j) for every point j of the 27 cells around cell c, in the order z, y, run of x cells; st / so: `start` and `sorted` of the (scene, sample)
template <class F>
__device__ __forceinline__ void grid_walk(const Grid &g, int c, const int *__restrict__ st, const int *__restrict__ so, F f)
{
    const int ix = c % g.nx, iy = (c / g.nx) % g.ny, iz = c / (g.nx * g.ny);
    const int x_lo = ix > 0 ? ix - 1 : 0, x_hi = ix + 1 < g.nx ? ix + 1 : g.nx - 1;
    for (int dz = -1; dz <= 1; ++dz) {
        const int z = iz + dz;
        if (z < 0 || z >= g.nz) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = iy + dy;
            if (yy < 0 || yy >= g.ny) continue;
            const int base = g.nx * (yy + g.ny * z);
            const int e0 = st[base + x_lo], e1 = st[base + x_hi + 1];   // x is the fastest cell index: three cells = one run
            for (int e = e0; e < e1; ++e) f(so[e]);
        }
    }
}
// f(j, x, y, z) for the points lo .. hi-1 of pp[][3], in ascending order, streamed through LDS in tiles of 256.  Every thread of the block
// takes part in the staging and reaches both barriers; `vi`: the thread owns an agent and f is called for it.
template <class F>
__device__ __forceinline__ void tile_stream(const double *__restrict__ pp, int lo, int hi, bool vi, double *tile, F f)
{
    for (int j0 = lo; j0 < hi; j0 += 256) {
        const int cntj = hi - j0 < 256 ? hi - j0 : 256;
        __syncthreads();
        for (int e = threadIdx.x; e < cntj * 3; e += 256) tile[e] = pp[3 * (size_t)j0 + e];
        __syncthreads();
        if (vi)
            for (int jj = 0; jj < cntj; ++jj) f(j0 + jj, tile[3 * jj], tile[3 * jj + 1], tile[3 * jj + 2]);
    }
}

// block = (tile of 256 agents i, sample, scene): every agent j > i of the 27 cells around i's
__global__ void grid_pairs_kernel(int N, int SB, Grid g, double cinv, const double *__restrict__ pts, const int *__restrict__ cell_of,
                                  const int *__restrict__ start, const int *__restrict__ sorted, unsigned long long *__restrict__ mind2)
{
    __shared__ double sh[256];
    const int s = blockIdx.z, b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const size_t sb = (size_t)s * SB + b, t = sb * N + i;
    double m = INFINITY;
    const int c = i < N ? cell_of[t] : -1;
    if (c >= 0) {
        const double xi = pts[3 * t], yi = pts[3 * t + 1], zi = pts[3 * t + 2];
        const double *pp = pts + sb * (size_t)N * 3;
        grid_walk(g, c, start + sb * ((size_t)g.nx * g.ny * g.nz + 1), sorted + sb * N, [&](int j) {
            if (j > i) m = fmin(m, pair_d2(xi, yi, zi, pp[3 * j], pp[3 * j + 1], pp[3 * j + 2], cinv));
        });
    }
    scene_min(m, sh, &mind2[s]);
}
// brute force over the positions of a batch (fallback of the grid search: scenes without any pair closer than `edge`):
// block = (tile of 256 agents i, sample, scene); the tiles of j >= tile(i) stream through LDS
__global__ void pairs_brute_pts_kernel(int N, int SB, double cinv, const double *__restrict__ pts, const int *__restrict__ cell_of,
                                       const int *__restrict__ scene_on, unsigned long long *__restrict__ mind2)
{
    __shared__ double tile[256 * 3];
    __shared__ double sh[256];
    const int s = blockIdx.z, b = blockIdx.y, it = blockIdx.x;
    if (!scene_on[s]) return;
    const size_t sb = (size_t)s * SB + b;
    if (cell_of[sb * N] < 0) return;   // sample beyond the end of this scene's transition
    const double *pp = pts + sb * (size_t)N * 3;
    const int i = it * 256 + threadIdx.x;
    const bool vi = i < N;
    const double xi = vi ? pp[3 * i] : 0.0, yi = vi ? pp[3 * i + 1] : 0.0, zi = vi ? pp[3 * i + 2] : 0.0;
    double m = INFINITY;
    tile_stream(pp, it * 256, N, vi, tile, [&](int j, double xj, double yj, double zj) {
        if (j > i) m = fmin(m, pair_d2(xi, yi, zi, xj, yj, zj, cinv));
    });
    scene_min(m, sh, &mind2[s]);
}

// Uncommanded vehicles: every (commanded agent, sample) against every static vehicle, all pairs, exact.  block = (tile of 256 (agent, sample)
// items, scene); a thread evaluates its item's spline position once, the static positions po_static[S][M][3] stream through LDS in tiles.
// The same fp64 distance expression as the agent-agent check (pair_d2); a static vehicle has no spline.
__global__ void static_pairs_kernel(int N, int M, int KTa, const int *__restrict__ kt_used, const double *__restrict__ hs,
                                    const int *__restrict__ ns, double Ts, double cinv, const double *__restrict__ y,
                                    const double *__restrict__ Msp, const double *__restrict__ po_static,
                                    unsigned long long *__restrict__ mind2)
{
    __shared__ double tile[256 * 3];
    __shared__ double sh[256];
    const int s = blockIdx.y, n = kt_used[s], nsamp = ns[s];
    if (n < 2 || nsamp < 1) return;   // masked scene
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if ((size_t)blockIdx.x * 256 >= (size_t)N * nsamp) return;   // (uniform per block: the grid is sized for the longest scene)
    const bool vi = e < (size_t)N * nsamp;
    P3 p{0.0, 0.0, 0.0};
    if (vi) {
        const int i = (int)(e / nsamp), smp = (int)(e - (size_t)i * nsamp);
        p = spline_eval(y, Msp, ((size_t)s * N + i) * (size_t)KTa * 3, n, hs[s], smp * Ts);
    }
    double m = INFINITY;
    tile_stream(po_static + (size_t)s * M * 3, 0, M, vi, tile,
                [&](int, double xj, double yj, double zj) { m = fmin(m, pair_d2(p.x, p.y, p.z, xj, yj, zj, cinv)); });
    scene_min(m, sh, &mind2[s]);
}

// Scripted vehicles (dmpc_postcheck_scripted): a vehicle that follows a path over step indices gets the spline the commanded agents get, on
// their time base -- knots t_i = i h_scaled, i = 0 .. K_T_used-1, values sample(j, i) = path[j][min(i, P-1)] (spline_kernel above makes the
// second derivatives of these knots, short histories included).  thread per knot component; yk: [S][M][KTa][3]; path: [S][M][P][3]
__global__ void scripted_knots_kernel(int S, int M, int KTa, int P, const int *__restrict__ kt_used, const double *__restrict__ path,
                                      double *__restrict__ yk)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)S * M * KTa * 3) return;
    const int ax = (int)(g % 3);
    const int i = (int)((g / 3) % KTa);
    const size_t sj = g / ((size_t)3 * KTa);
    const int s = (int)(sj / M);
    yk[g] = i < kt_used[s] ? path[(sj * P + (i < P - 1 ? i : P - 1)) * 3 + ax] : 0.0;
}

// every commanded agent against every scripted vehicle at one sample, all pairs, exact: block = (sample of the batch, scene).  The commanded
// agents' spline positions at the sample are staged in LDS in tiles of 256 (evaluated once each); the pairs (agent of the tile, vehicle) are
// strided over the threads with the vehicle index fastest, so the reads of pts are coalesced.  The distance is pair_d2, the expression of
// static_pairs_kernel, commanded agent first.
__global__ void scripted_pairs_kernel(int N, int M, int KTa, const int *__restrict__ kt_used, const double *__restrict__ hs,
                                      const int *__restrict__ ns, double Ts, int smp0, int SB, double cinv, const double *__restrict__ y,
                                      const double *__restrict__ Msp, const double *__restrict__ pts, unsigned long long *__restrict__ mind2)
{
    __shared__ double tile[256 * 3];
    __shared__ double sh[256];
    const int s = blockIdx.y, b = blockIdx.x, n = kt_used[s], smp = smp0 + b;
    if (n < 2 || smp >= ns[s]) return;   // masked scene, or a sample beyond the end of this scene's transition (uniform per block)
    const double h = hs[s], t = smp * Ts;
    const double *q = pts + ((size_t)s * SB + b) * (size_t)M * 3;
    double m = INFINITY;
    for (int i0 = 0; i0 < N; i0 += 256) {
        const int cnti = N - i0 < 256 ? N - i0 : 256;
        __syncthreads();
        if ((int)threadIdx.x < cnti) {
            const P3 p = spline_eval(y, Msp, ((size_t)s * N + i0 + threadIdx.x) * (size_t)KTa * 3, n, h, t);
            tile[3 * threadIdx.x] = p.x; tile[3 * threadIdx.x + 1] = p.y; tile[3 * threadIdx.x + 2] = p.z;
        }
        __syncthreads();
        for (size_t e = threadIdx.x; e < (size_t)cnti * M; e += 256) {
            const int ii = (int)(e / M), j = (int)(e - (size_t)ii * M);
            m = fmin(m, pair_d2(tile[3 * ii], tile[3 * ii + 1], tile[3 * ii + 2], q[3 * j], q[3 * j + 1], q[3 * j + 2], cinv));
        }
    }
    scene_min(m, sh, &mind2[s]);
}

// per agent: path length sum |p(t_{s+1}) - p(t_s)| (failure_rate.m:183) and the 1-based index after the last
// sample farther than 5 cm from the goal (failure_rate.m:186-193)
__global__ void path_kernel(int S, int N, int KTa, const int *__restrict__ kt_used, const double *__restrict__ hs,
                            const int *__restrict__ ns, double Ts, const double *__restrict__ y, const double *__restrict__ M,
                            const double *__restrict__ pf, double *__restrict__ dist, int *__restrict__ tidx)
{
    const size_t sa = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sa >= (size_t)S * N) return;
    const int s = (int)(sa / N), n = kt_used[s], nsamp = ns[s];
    const double h = hs[s];
    const size_t o = sa * (size_t)KTa * 3;
    const double gx = pf[sa * 3], gy = pf[sa * 3 + 1], gz = pf[sa * 3 + 2];
    double px = 0, py = 0, pz = 0, acc = 0;
    int last = 0;
    for (int smp = 0; smp < nsamp; ++smp) {
        const P3 p = spline_eval(y, M, o, n, h, smp * Ts);
        const double x = p.x, yv = p.y, z = p.z;
        if (smp) acc += sqrt((x - px) * (x - px) + (yv - py) * (yv - py) + (z - pz) * (z - pz));
        px = x; py = yv; pz = z;
        const double dg = sqrt((x - gx) * (x - gx) + (yv - gy) * (yv - gy) + (z - gz) * (z - gz));
        if (dg >= 0.05) last = smp + 2;
    }
    dist[sa] = acc;
    tidx[sa] = last;
}

// fixed-order per-scene reductions of the per-agent results
__global__ void finish_kernel(int N, const double *__restrict__ dist, const int *__restrict__ tidx, double Ts,
                              double *__restrict__ totdist, double *__restrict__ traj_time)
{
    __shared__ double sd[256];
    __shared__ int si[256];
    const int s = blockIdx.x, t = threadIdx.x;
    double a = 0;
    int m = 0;
    for (int i = t; i < N; i += blockDim.x) { a += dist[(size_t)s * N + i]; m = max(m, tidx[(size_t)s * N + i]); }
    sd[t] = a; si[t] = m;
    __syncthreads();
    for (int k = blockDim.x >> 1; k > 0; k >>= 1) {
        if (t < k) { sd[t] += sd[t + k]; si[t] = max(si[t], si[t + k]); }
        __syncthreads();
    }
    if (t == 0) { totdist[s] = sd[0]; traj_time[s] = si[0] * Ts; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Clearance report (dmpc_postcheck_clearance): per commanded agent i the nearest commanded partner (slot 0) and the nearest uncommanded
// vehicle (slot 1) over all 100 Hz samples, with the sample at which it happens.  The searches above reduce the same distances to one number
// per scene; here every thread owns one agent and keeps (d2, sample, partner) per slot in registers.  Ties go to the smallest sample, then the
// smallest partner: samples are walked in ascending order and a later one replaces the best only when it is strictly smaller; within a sample
// the tiled search walks the partners in ascending order (strict <), the cell-grid search, whose order inside a cell is arbitrary, compares
// (d2, partner).  A batch of SB samples is cut into chunks of CH; a block = (tile of 256 agents, chunk, scene) writes its agents' bests of the
// chunk as partials [chunk][S][Nc][2], and clear_finish_kernel folds them, in chunk order, into the running best of the whole transition.

// agent i against the vehicles lo .. hi-1 of one sample, in ascending order: with the strict <, ties go to the smallest partner
__device__ __forceinline__ void clear_scan_tiles(const double *__restrict__ pp, int lo, int hi, int i, bool vi, double xi, double yi, double zi,
                                                 double cinv, int smp, double *tile, double &bd, int &bs, int &bj)
{
    tile_stream(pp, lo, hi, vi, tile, [&](int j, double xj, double yj, double zj) {
        const double d = pair_d2(xi, yi, zi, xj, yj, zj, cinv);
        if (d < bd && j != i) { bd = d; bs = smp; bj = j; }
    });
}
// the partials of one (chunk, scene, agent): part_d2 [chunk][S][Nc][2], part_smp and part_j alike
__device__ __forceinline__ void clear_store(int S, int Nc, int chunk, int s, int i, double *__restrict__ part_d2, int *__restrict__ part_smp,
                                            int *__restrict__ part_j, double d0, int s0, int j0, double d1, int s1, int j1)
{
    const size_t o = (((size_t)chunk * S + s) * Nc + i) * 2;
    part_d2[o] = d0; part_smp[o] = s0; part_j[o] = j0;
    part_d2[o + 1] = d1; part_smp[o + 1] = s1; part_j[o + 1] = j1;
}

// tiled all-pairs: block = (tile of 256 commanded agents i, chunk of CH samples, scene); exact for every agent
__global__ void clear_brute_kernel(int S, int N, int Nc, int SB, int CH, int smp0, const int *__restrict__ ns, double cinv,
                                   const double *__restrict__ pts, double *__restrict__ part_d2, int *__restrict__ part_smp,
                                   int *__restrict__ part_j)
{
    __shared__ double tile[256 * 3];
    const int s = blockIdx.z, chunk = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const bool vi = i < Nc;
    const int nsamp = ns[s];
    double d0 = INFINITY, d1 = INFINITY;
    int s0 = -1, s1 = -1, j0 = -1, j1 = -1;
    for (int q = 0; q < CH; ++q) {
        const int b = chunk * CH + q, smp = smp0 + b;
        if (b >= SB || smp >= nsamp) break;   // (uniform per block)
        const double *pp = pts + ((size_t)s * SB + b) * (size_t)N * 3;
        const double xi = vi ? pp[3 * i] : 0.0, yi = vi ? pp[3 * i + 1] : 0.0, zi = vi ? pp[3 * i + 2] : 0.0;
        clear_scan_tiles(pp, 0, Nc, i, vi, xi, yi, zi, cinv, smp, tile, d0, s0, j0);
        clear_scan_tiles(pp, Nc, N, i, vi, xi, yi, zi, cinv, smp, tile, d1, s1, j1);
    }
    if (vi) clear_store(S, Nc, chunk, s, i, part_d2, part_smp, part_j, d0, s0, j0, d1, s1, j1);
}

// (d2, sample, partner) lexicographically; the samples of a thread ascend, so an equal distance wins only at the same sample with a smaller partner
__device__ __forceinline__ void clear_take(double d, int smp, int j, double &bd, int &bs, int &bj)
{
    if (d < bd || (d == bd && bs == smp && j < bj)) { bd = d; bs = smp; bj = j; }
}
// cell grid: block = (tile of 256 commanded agents i, chunk of CH samples, scene); every vehicle of the 27 cells around i's (grid_walk
// over a grid that holds all N vehicles).  Finds every pair closer than the cell edge; what lies farther is for the caller to discard.
__global__ void clear_grid_kernel(int S, int N, int Nc, int SB, int CH, int smp0, const int *__restrict__ ns, Grid g, double cinv,
                                  const double *__restrict__ pts, const int *__restrict__ cell_of, const int *__restrict__ start,
                                  const int *__restrict__ sorted, double *__restrict__ part_d2, int *__restrict__ part_smp,
                                  int *__restrict__ part_j)
{
    const int s = blockIdx.z, chunk = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Nc) return;
    const int nsamp = ns[s];
    const size_t ncell = (size_t)g.nx * g.ny * g.nz;
    double bd[2] = {INFINITY, INFINITY};   // slot 0: commanded partners, slot 1: the other vehicles
    int bs[2] = {-1, -1}, bj[2] = {-1, -1};
    for (int q = 0; q < CH; ++q) {
        const int b = chunk * CH + q, smp = smp0 + b;
        if (b >= SB || smp >= nsamp) break;
        const size_t sb = (size_t)s * SB + b, t = sb * N + i;
        const int c = cell_of[t];
        if (c < 0) break;
        const double xi = pts[3 * t], yi = pts[3 * t + 1], zi = pts[3 * t + 2];
        const double *pp = pts + sb * (size_t)N * 3;
        grid_walk(g, c, start + sb * (ncell + 1), sorted + sb * N, [&](int j) {
            if (j == i) return;
            const int k = j < Nc ? 0 : 1;
            clear_take(pair_d2(xi, yi, zi, pp[3 * j], pp[3 * j + 1], pp[3 * j + 2], cinv), smp, j, bd[k], bs[k], bj[k]);
        });
    }
    clear_store(S, Nc, chunk, s, i, part_d2, part_smp, part_j, bd[0], bs[0], bj[0], bd[1], bs[1], bj[1]);
}

// thread per (scene, agent, slot): the batch's partials, in chunk order, into the running best run_* [S][Nc][2] (`first`: the batch opens the
// transition), which only its owner touches; `last`: the report -- dist = sqrt(d2), a slot without anything closer than `reach` +inf / -1 / -1,
// a masked scene NaN / -1 / -1
__global__ void clear_finish_kernel(size_t total, int Nc, int nchunk, int first, int last, const int *__restrict__ kt_used, double reach,
                                    const double *__restrict__ part_d2, const int *__restrict__ part_smp, const int *__restrict__ part_j,
                                    double *__restrict__ run_d2, int *__restrict__ run_smp, int *__restrict__ run_j,
                                    double *__restrict__ dist, int *__restrict__ partner, int *__restrict__ sample)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    double bd = first ? INFINITY : run_d2[e];
    int bs = first ? -1 : run_smp[e], bj = first ? -1 : run_j[e];
    for (int c = 0; c < nchunk; ++c) {
        const size_t o = (size_t)c * total + e;
        if (part_d2[o] < bd) { bd = part_d2[o]; bs = part_smp[o]; bj = part_j[o]; }
    }
    run_d2[e] = bd; run_smp[e] = bs; run_j[e] = bj;
    if (!last) return;
    const double d = sqrt(bd);
    const bool masked = !kt_used[e / ((size_t)Nc * 2)], found = d < reach;
    dist[e] = masked ? NAN : (found ? d : INFINITY);
    partner[e] = !masked && found ? bj : -1;
    sample[e] = !masked && found ? bs : -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Flight setpoints (dmpc_postcheck_setpoints): position, velocity and acceleration of every commanded agent at the 100 Hz samples, and per agent
// the largest |v| and |a| over ALL samples with the sample at which it happens.  The reference splines the three histories independently
// (dmpc_soft_bound.m:165-169), so three splines on the same knots are evaluated: y = the rescaled pk / vk / ak as rescale_kernel leaves them,
// M = their second derivatives (spline_kernel).  Sample j has t = j * Ts, the expression of path_kernel / sample_table_kernel.
// A workgroup = (tile of SP_TILE agents, chunk of SP_CHUNK samples, scene): thread t owns sample lo + chunk * SP_CHUNK + t and walks the agents
// of the tile, so the lanes of a wave hold consecutive samples of ONE agent -- the stores into [..][SB][3] are one contiguous run per wave and
// the ~h_scaled / Ts lanes of a spline interval read the same knots.  Peaks: (value, sample) pairs ordered by larger value, then smaller sample
// -- a total order, so the maximum does not depend on how the samples are grouped: per wave by cross-lane exchange, per workgroup through LDS
// in wave order, partials [chunk][S][N], folded in chunk order by setpoint_finish_kernel.
#define SP_TILE 64
#define SP_CHUNK 256

// the norm of every peak, on every path
__device__ __forceinline__ double norm3(double x, double y, double z)
{
    return sqrt(fma(z, z, fma(y, y, x * x)));
}
// (value, sample) lexicographically: the larger value, then the smaller sample; (-1, -1) is "no sample" (norms are >= 0)
__device__ __forceinline__ void peak_take(double v, int smp, double &bv, int &bs)
{
    if (v > bv || (v == bv && smp < bs)) { bv = v; bs = smp; }
}
__device__ __forceinline__ void peak_wave(double &bv, int &bs)
{
    for (int d = 32; d > 0; d >>= 1) {
        const double ov = __shfl_xor(bv, d, 64);
        const int os = __shfl_xor(bs, d, 64);
        peak_take(ov, os, bv, bs);
    }
}

// samples lo .. hi-1 of the transition.  sp / sv / sa: staging arrays [S][N][SB][3] of the samples lo .. lo+SB-1 (hi - lo <= SB) or null; every slot
// below hi is written, zero from the scene's n_samples on.  part_*: [gridDim.y][S][N].
__global__ void __launch_bounds__(SP_CHUNK)
setpoint_kernel(int S, int N, int KTa, const int *__restrict__ kt_used, const double *__restrict__ hs, const int *__restrict__ ns, double Ts,
                int lo, int hi, const double *__restrict__ yp, const double *__restrict__ Mp, const double *__restrict__ yv,
                const double *__restrict__ Mv, const double *__restrict__ ya, const double *__restrict__ Ma, double *__restrict__ sp,
                double *__restrict__ sv, double *__restrict__ sa, int SB, double *__restrict__ part_v, int *__restrict__ part_vs,
                double *__restrict__ part_a, int *__restrict__ part_as)
{
    __shared__ double sh_v[SP_TILE][SP_CHUNK / 64], sh_a[SP_TILE][SP_CHUNK / 64];
    __shared__ int sh_vs[SP_TILE][SP_CHUNK / 64], sh_as[SP_TILE][SP_CHUNK / 64];
    const int s = blockIdx.z, chunk = blockIdx.y, i0 = blockIdx.x * SP_TILE;
    const int cnt = N - i0 < SP_TILE ? N - i0 : SP_TILE;
    const int j0 = lo + chunk * SP_CHUNK, j = j0 + (int)threadIdx.x;
    const int n = kt_used[s], nsamp = ns[s];
    const bool slot = j < hi, live = slot && j < nsamp;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t a0 = (size_t)s * N + i0;
    if (j0 >= nsamp) {   // (uniform per workgroup) nothing to evaluate: zero slots, empty partials
        if (slot)
            for (int a = 0; a < cnt; ++a) {
                const size_t q = ((a0 + a) * (size_t)SB + (size_t)(j - lo)) * 3;
                if (sp) { sp[q] = 0.0; sp[q + 1] = 0.0; sp[q + 2] = 0.0; }
                if (sv) { sv[q] = 0.0; sv[q + 1] = 0.0; sv[q + 2] = 0.0; }
                if (sa) { sa[q] = 0.0; sa[q + 1] = 0.0; sa[q + 2] = 0.0; }
            }
        if ((int)threadIdx.x < cnt) {
            const size_t e = ((size_t)chunk * S + s) * N + i0 + threadIdx.x;
            part_v[e] = -1.0; part_vs[e] = -1; part_a[e] = -1.0; part_as[e] = -1;
        }
        return;
    }
    const double h = hs[s], t = j * Ts;
    for (int a = 0; a < cnt; ++a) {
        const size_t o = (a0 + a) * (size_t)KTa * 3;
        P3 p{0.0, 0.0, 0.0}, v = p, ac = p;
        double bv = -1.0, ba = -1.0;
        int bvs = -1, bas = -1;
        if (live) {
            p = spline_eval(yp, Mp, o, n, h, t); v = spline_eval(yv, Mv, o, n, h, t); ac = spline_eval(ya, Ma, o, n, h, t);
            bv = norm3(v.x, v.y, v.z); bvs = j;
            ba = norm3(ac.x, ac.y, ac.z); bas = j;
        }
        if (slot) {
            const size_t q = ((a0 + a) * (size_t)SB + (size_t)(j - lo)) * 3;
            if (sp) { sp[q] = p.x; sp[q + 1] = p.y; sp[q + 2] = p.z; }
            if (sv) { sv[q] = v.x; sv[q + 1] = v.y; sv[q + 2] = v.z; }
            if (sa) { sa[q] = ac.x; sa[q + 1] = ac.y; sa[q + 2] = ac.z; }
        }
        peak_wave(bv, bvs);
        peak_wave(ba, bas);
        if (lane == 0) { sh_v[a][wave] = bv; sh_vs[a][wave] = bvs; sh_a[a][wave] = ba; sh_as[a][wave] = bas; }
    }
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
        const int a = threadIdx.x;
        double bv = sh_v[a][0], ba = sh_a[a][0];
        int bvs = sh_vs[a][0], bas = sh_as[a][0];
        for (int w = 1; w < SP_CHUNK / 64; ++w) { peak_take(sh_v[a][w], sh_vs[a][w], bv, bvs); peak_take(sh_a[a][w], sh_as[a][w], ba, bas); }
        const size_t e = ((size_t)chunk * S + s) * N + i0 + a;
        part_v[e] = bv; part_vs[e] = bvs; part_a[e] = ba; part_as[e] = bas;
    }
}

// thread per (scene, agent): the partials of one launch, in chunk order, into the running peaks run_* [S][N] (`first`: the launch opens the
// transition); `last`: the report, a masked scene NaN / -1
__global__ void setpoint_finish_kernel(size_t total, int N, int nchunk, int first, int last, const int *__restrict__ kt_used,
                                       const double *__restrict__ part_v, const int *__restrict__ part_vs, const double *__restrict__ part_a,
                                       const int *__restrict__ part_as, double *__restrict__ run_v, int *__restrict__ run_vs,
                                       double *__restrict__ run_a, int *__restrict__ run_as, double *__restrict__ o_v, int *__restrict__ o_vs,
                                       double *__restrict__ o_a, int *__restrict__ o_as)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    double bv = first ? -1.0 : run_v[e], ba = first ? -1.0 : run_a[e];
    int bvs = first ? -1 : run_vs[e], bas = first ? -1 : run_as[e];
    for (int c = 0; c < nchunk; ++c) {
        const size_t o = (size_t)c * total + e;
        peak_take(part_v[o], part_vs[o], bv, bvs);
        peak_take(part_a[o], part_as[o], ba, bas);
    }
    run_v[e] = bv; run_vs[e] = bvs; run_a[e] = ba; run_as[e] = bas;
    if (!last) return;
    const bool masked = !kt_used[e / (size_t)N];
    o_v[e] = masked ? NAN : bv; o_vs[e] = masked ? -1 : bvs;
    o_a[e] = masked ? NAN : ba; o_as[e] = masked ? -1 : bas;
}

}   // namespace pc
