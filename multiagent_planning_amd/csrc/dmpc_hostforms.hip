// dmpc_hostforms.hip -- host-pointer forms of small things (the last part dmpc_api.hip includes): the dense collision-row builders, the start / goal
// generators, and the stand-alone helpers of the path with their four small kernels (hp::).  The host forms share one shape -- ensure the context's
// staging buffers, copy up, launch, copy down, synchronise -- and each writes that order out on the context's stream; the _device forms launch on
// the caller's stream and copy nothing.

// ---------------------------------------------------------------------------------------------
// dense collision-row builders (dec-iSCP/CollConstr.m, dmpc/matlab/CollConstr*DMPC.m, cup-SCP/AddCollConstr.m)
// ---------------------------------------------------------------------------------------------
static size_t strided_extent(int rows, int cols, int64_t rs, int64_t cs)
{
    return (size_t)((rows - 1) * rs + (cols - 1) * cs + 1);
}

extern "C" int dmpc_coll_rows_device(dmpc_ctx *ctx, int K, int n_sel, const int32_t *d_sel, const double *d_l, int k_cmp, int k_blk,
                                     const double *p, const double *a0, double rmin, double c, const double *d_A, int64_t a_rs,
                                     int64_t a_cs, int ncols, double *d_Ain, int64_t o_rs, int64_t o_cs, double *d_bin,
                                     double *d_dist, void *stream)
{
    if (!ctx) { g_err = "dmpc_coll_rows_device: ctx is NULL"; return -1; }
    if (K < 1 || n_sel < 0 || !p || !a0 || k_cmp < 0 || k_cmp >= K || k_blk < 0 || ncols < 1 || !(c > 0) || !d_A || !d_Ain || !d_bin)
        FAIL(ctx, "dmpc_coll_rows_device: bad arguments");
    if (n_sel == 0) return 0;
    if (!d_sel || !d_l) FAIL(ctx, "dmpc_coll_rows_device: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t tot = (size_t)n_sel * ncols;
    hipLaunchKernelGGL(rb::coll_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       n_sel, (const int *)d_sel, K, d_l, k_cmp, k_blk, p[0], p[1], p[2], a0[0], a0[1], a0[2], rmin, 1.0 / c, d_A,
                       (long)a_rs, (long)a_cs, ncols, d_Ain, (long)o_rs, (long)o_cs, d_bin, d_dist, ctx->prm.order == 4 ? 4 : 2);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

extern "C" int dmpc_coll_rows(dmpc_ctx *ctx, int K, int N_obs, int n_sel, const int32_t *sel, const double *l, int k_cmp, int k_blk,
                              const double *p, const double *a0, double rmin, double c, const double *A, int a_rows, int ncols,
                              int64_t a_rs, int64_t a_cs, double *Ain, int64_t o_rs, int64_t o_cs, double *bin, double *dist)
{
    if (!ctx) { g_err = "dmpc_coll_rows: ctx is NULL"; return -1; }
    if (K < 1 || N_obs < 0 || n_sel < 0 || n_sel > N_obs || a_rows < 3 || ncols < 1 || a_rs < 1 || a_cs < 1 || o_rs < 1 || o_cs < 1 ||
        !A || !Ain || !bin || !p || !a0)
        FAIL(ctx, "dmpc_coll_rows: bad arguments");
    if (3 * k_blk + 2 >= a_rows || k_blk < 0) FAIL(ctx, "dmpc_coll_rows: constraint block outside A");
    if (n_sel == 0) return 0;
    if (!sel || !l) FAIL(ctx, "dmpc_coll_rows: bad arguments");
    for (int i = 0; i < n_sel; ++i)
        if (sel[i] < 0 || sel[i] >= N_obs) FAIL(ctx, "dmpc_coll_rows: obstacle index out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t a_ext = strided_extent(a_rows, ncols, a_rs, a_cs), o_ext = strided_extent(n_sel, ncols, o_rs, o_cs);
    if (ctx->rb_A.ensure(a_ext * 8) || ctx->rb_l.ensure((size_t)N_obs * K * 24) || ctx->rb_sel.ensure((size_t)n_sel * 4) ||
        ctx->rb_out.ensure(o_ext * 8) || ctx->rb_bin.ensure((size_t)n_sel * 16))
        FAIL(ctx, "device allocation failed");
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_A.p, A, a_ext * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_l.p, l, (size_t)N_obs * K * 24, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_sel.p, sel, (size_t)n_sel * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->rb_out.p, 0, o_ext * 8, st));
    double *d_bin = ctx->rb_bin.as<double>(), *d_dist = d_bin + n_sel;
    if (dmpc_coll_rows_device(ctx, K, n_sel, ctx->rb_sel.as<int32_t>(), ctx->rb_l.as<double>(), k_cmp, k_blk, p, a0, rmin, c,
                              ctx->rb_A.as<double>(), a_rs, a_cs, ncols, ctx->rb_out.as<double>(), o_rs, o_cs, d_bin, d_dist, st))
        return -1;
    HIPCHK(ctx, hipMemcpyAsync(Ain, ctx->rb_out.p, o_ext * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(bin, d_bin, (size_t)n_sel * 8, hipMemcpyDeviceToHost, st));
    if (dist) HIPCHK(ctx, hipMemcpyAsync(dist, d_dist, (size_t)n_sel * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

extern "C" int dmpc_rows_dense(dmpc_ctx *ctx, int nr, const double *xi, const int32_t *kc, const double *A, int a_rows, int ncols,
                               int64_t a_rs, int64_t a_cs, double *Ain, int64_t o_rs, int64_t o_cs)
{
    if (!ctx) { g_err = "dmpc_rows_dense: ctx is NULL"; return -1; }
    if (nr < 0 || a_rows < 3 || ncols < 1 || a_rs < 1 || a_cs < 1 || o_rs < 1 || o_cs < 1 || !A || !Ain) FAIL(ctx, "dmpc_rows_dense: bad arguments");
    if (nr == 0) return 0;
    if (!xi || !kc) FAIL(ctx, "dmpc_rows_dense: bad arguments");
    for (int r = 0; r < nr; ++r)
        if (kc[r] < 1 || 3 * kc[r] > a_rows) FAIL(ctx, "dmpc_rows_dense: constraint block outside A");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t a_ext = strided_extent(a_rows, ncols, a_rs, a_cs), o_ext = strided_extent(nr, ncols, o_rs, o_cs);
    if (ctx->rb_A.ensure(a_ext * 8) || ctx->rb_l.ensure((size_t)nr * 24) || ctx->rb_sel.ensure((size_t)nr * 4) || ctx->rb_out.ensure(o_ext * 8))
        FAIL(ctx, "device allocation failed");
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_A.p, A, a_ext * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_l.p, xi, (size_t)nr * 24, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_sel.p, kc, (size_t)nr * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->rb_out.p, 0, o_ext * 8, st));
    const size_t tot = (size_t)nr * ncols;
    hipLaunchKernelGGL(rb::xi_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, nr, (const double *)ctx->rb_l.as<double>(),
                       (const int *)ctx->rb_sel.as<int>(), (const double *)ctx->rb_A.as<double>(), (long)a_rs, (long)a_cs, ncols,
                       ctx->rb_out.as<double>(), (long)o_rs, (long)o_cs);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(Ain, ctx->rb_out.p, o_ext * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

extern "C" int dmpc_add_coll_constr_device(dmpc_ctx *ctx, int K, int N, const double *d_p, const double *d_po, double rmin, double c,
                                           const double *d_A, int64_t a_rs, int64_t a_cs, int ncols, double *d_Ain, int64_t o_rs,
                                           int64_t o_cs, double *d_bin, void *stream)
{
    if (!ctx) { g_err = "dmpc_add_coll_constr_device: ctx is NULL"; return -1; }
    if (K < 1 || N < 2 || ncols < 1 || !(c > 0) || !d_p || !d_po || !d_A || !d_Ain || !d_bin)
        FAIL(ctx, "dmpc_add_coll_constr_device: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nrows = (size_t)K * N * (N - 1) / 2, tot = nrows * (size_t)ncols;
    if ((tot + 255) / 256 > 0x7fffffffull) FAIL(ctx, "dmpc_add_coll_constr_device: problem too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    const size_t pch = ((size_t)N * (N - 1) / 2 + RB_PCH - 1) / RB_PCH;
    if (o_cs == 1 && K <= 65535 && pch <= 65535) {   // row-major output: (column tile, k, pair chunk) blocks
        hipLaunchKernelGGL(rb::add_coll_rows_rm_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)K, (unsigned)pch), dim3(256), 0, st,
                           N, K, d_p, d_po, rmin, 1.0 / c, d_A, (long)a_rs, (long)a_cs, ncols, d_Ain, (long)o_rs, d_bin, ctx->prm.order == 4 ? 4 : 2);
    } else if (o_rs == 1 && (ncols + RB_CCH - 1) / RB_CCH <= 65535) {   // column-major output (MATLAB): row-per-thread
        hipLaunchKernelGGL(rb::add_coll_rows_cm_kernel, dim3((unsigned)((nrows + 255) / 256), (unsigned)((ncols + RB_CCH - 1) / RB_CCH)),
                           dim3(256), 0, st, N, K, d_p, d_po, rmin, 1.0 / c, d_A, (long)a_rs, (long)a_cs, ncols, d_Ain, (long)o_cs,
                           d_bin, nrows, ctx->prm.order == 4 ? 4 : 2);
    } else {                                // arbitrary strides: one element per thread
        hipLaunchKernelGGL(rb::add_coll_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, N, K, d_p, d_po, rmin,
                           1.0 / c, d_A, (long)a_rs, (long)a_cs, ncols, d_Ain, (long)o_rs, (long)o_cs, d_bin, nrows, ctx->prm.order == 4 ? 4 : 2);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

extern "C" int dmpc_add_coll_constr(dmpc_ctx *ctx, int K, int N, const double *p, const double *po, double rmin, double c,
                                    const double *A, int ncols, int64_t a_rs, int64_t a_cs, double *Ain, int64_t o_rs, int64_t o_cs,
                                    double *bin)
{
    if (!ctx) { g_err = "dmpc_add_coll_constr: ctx is NULL"; return -1; }
    if (K < 1 || N < 2 || ncols < 1 || a_rs < 1 || a_cs < 1 || o_rs < 1 || o_cs < 1 || !p || !po || !A || !Ain || !bin)
        FAIL(ctx, "dmpc_add_coll_constr: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int a_rows = 3 * K * N;
    const size_t nrows = (size_t)K * N * (N - 1) / 2;
    const size_t a_ext = strided_extent(a_rows, ncols, a_rs, a_cs);
    const size_t o_ext = (size_t)((nrows - 1) * o_rs + (size_t)(ncols - 1) * o_cs + 1);
    if (ctx->rb_A.ensure(a_ext * 8) || ctx->rb_l.ensure((size_t)N * K * 24) || ctx->rb_po.ensure((size_t)N * 24) ||
        ctx->rb_out.ensure(o_ext * 8) || ctx->rb_bin.ensure(nrows * 8))
        FAIL(ctx, "device allocation failed");
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_A.p, A, a_ext * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_l.p, p, (size_t)N * K * 24, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rb_po.p, po, (size_t)N * 24, hipMemcpyHostToDevice, st));
    if (dmpc_add_coll_constr_device(ctx, K, N, ctx->rb_l.as<double>(), ctx->rb_po.as<double>(), rmin, c, ctx->rb_A.as<double>(), a_rs,
                                    a_cs, ncols, ctx->rb_out.as<double>(), o_rs, o_cs, ctx->rb_bin.as<double>(), st))
        return -1;
    HIPCHK(ctx, hipMemcpyAsync(Ain, ctx->rb_out.p, o_ext * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(bin, ctx->rb_bin.p, nrows * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// start / goal generators (randomTest.m, randomExchange.m)
// ---------------------------------------------------------------------------------------------
static int random_sets(dmpc_ctx *ctx, const char *who, int S, int N, const double *pmin, const double *pmax, double rmin, double c,
                       uint64_t seed, int exchange, double *d_out, hipStream_t st)
{
    if (S < 1 || N < 1 || !pmin || !pmax || !(rmin >= 0) || !(c > 0)) FAIL(ctx, std::string(who) + ": bad arguments");
    for (int d = 0; d < 3; ++d) if (!(pmax[d] > pmin[d])) FAIL(ctx, std::string(who) + ": empty box");
    const size_t lds = (size_t)N * 24 + (exchange ? (size_t)N * 8 : 0);
    if (lds > 150 * 1024) FAIL(ctx, std::string(who) + ": at most ~4800 agents per scene");
    HIPCHK(ctx, hipFuncSetAttribute((const void *)gen::random_points_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int waves = exchange ? S : 2 * S;
    hipLaunchKernelGGL(gen::random_points_kernel, dim3((unsigned)waves), dim3(64), lds, st, S, N, 2, exchange, pmin[0], pmin[1], pmin[2],
                       pmax[0], pmax[1], pmax[2], rmin, 1.0 / c, seed, d_out);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

static int random_host(dmpc_ctx *ctx, const char *who, int S, int N, const double *pmin, const double *pmax, double rmin, double c,
                       uint64_t seed, int exchange, double *po, double *pf)
{
    if (!ctx) { g_err = std::string(who) + ": ctx is NULL"; return -1; }
    if (!po || !pf || S < 1 || N < 1) FAIL(ctx, std::string(who) + ": bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t one = (size_t)S * N * 24;
    if (ctx->gen_out.ensure(2 * one)) FAIL(ctx, "device allocation failed");
    if (random_sets(ctx, who, S, N, pmin, pmax, rmin, c, seed, exchange, ctx->gen_out.as<double>(), ctx->stream)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(po, ctx->gen_out.p, one, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(pf, ctx->gen_out.as<char>() + one, one, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int dmpc_random_test(dmpc_ctx *ctx, int S, int N, const double *pmin, const double *pmax, double rmin, double c,
                                uint64_t seed, double *po, double *pf)
{
    return random_host(ctx, "dmpc_random_test", S, N, pmin, pmax, rmin, c, seed, 0, po, pf);
}

extern "C" int dmpc_random_exchange(dmpc_ctx *ctx, int S, int N, const double *pmin, const double *pmax, double rmin, uint64_t seed,
                                    double *po, double *pf)
{
    return random_host(ctx, "dmpc_random_exchange", S, N, pmin, pmax, rmin, 1.0, seed, 1, po, pf);
}

extern "C" int dmpc_random_sets_device(dmpc_ctx *ctx, int S, int N, const double *pmin, const double *pmax, double rmin, double c,
                                       uint64_t seed, int exchange, double *d_po_pf, void *stream)
{
    if (!ctx) { g_err = "dmpc_random_sets_device: ctx is NULL"; return -1; }
    if (!d_po_pf) FAIL(ctx, "dmpc_random_sets_device: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return random_sets(ctx, "dmpc_random_sets_device", S, N, pmin, pmax, rmin, exchange ? 1.0 : c, seed, exchange ? 1 : 0, d_po_pf,
                       (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// standalone forms of the small helpers of the path (propStatedmpc.m, dec-iSCP/propState.m, is_inbounds.m,
// ReachedGoal.m): inside the solvers they are fused into the step kernels; callers that invoke them on their own
// (the reference's scripts do) get the same arithmetic on the device.  Host pointers, synchronous.
// ---------------------------------------------------------------------------------------------
namespace hp {
// p = A_p a + A_initp x0 + tile(off_p), v = A_v a + tile(off_v); one thread per output row
__global__ void prop_state_kernel(int n_rows, int n_cols, const double *__restrict__ A_p, const double *__restrict__ A_v,
                                  const double *__restrict__ A_initp, const double *__restrict__ x0, const double *__restrict__ off,
                                  const double *__restrict__ a, double *__restrict__ p, double *__restrict__ v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    double sp = 0.0, sv = 0.0;
    for (int j = 0; j < n_cols; ++j) {
        sp += A_p[(size_t)i * n_cols + j] * a[j];
        sv += A_v[(size_t)i * n_cols + j] * a[j];
    }
    if (A_initp) {
        double s0 = 0.0;
        for (int u = 0; u < 6; ++u) s0 += A_initp[(size_t)i * 6 + u] * x0[u];
        sp += s0;
    }
    p[i] = sp + off[i % 3];
    v[i] = sv + off[3 + i % 3];
}
// is_inbounds.m:2-5: every coordinate of every point strictly inside [pmin - 5 cm, pmax + 5 cm]
__global__ void inbounds_kernel(int npts, const double *__restrict__ p, const double *__restrict__ lim, int *__restrict__ bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * npts) return;
    const int d = i % 3;
    const double tol = 50e-3;
    if (!(p[i] < lim[3 + d] + tol) || !(p[i] > lim[d] - tol)) atomicOr(bad, 1);
}
// ReachedGoal.m:2-10: max_i |p_i - pf_i| < error_tol
__global__ void reached_kernel(int N, const double *__restrict__ p, const double *__restrict__ pf, double tol, int *__restrict__ bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double dx = p[3 * i] - pf[3 * i], dy = p[3 * i + 1] - pf[3 * i + 1], dz = p[3 * i + 2] - pf[3 * i + 2];
    if (!(sqrt(dx * dx + dy * dy + dz * dz) < tol)) atomicOr(bad, 1);
}
// maxDeviation.m:3-9: per step the distance between the two trajectories (non-negative doubles order like their bit patterns: integer maximum)
__global__ void max_dev_kernel(int nsteps, const double *__restrict__ p, const double *__restrict__ q, unsigned long long *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsteps) return;
    const double dx = p[3 * i] - q[3 * i], dy = p[3 * i + 1] - q[3 * i + 1], dz = p[3 * i + 2] - q[3 * i + 2];
    atomicMax(out, (unsigned long long)__double_as_longlong(sqrt(dx * dx + dy * dy + dz * dz)));
}
}   // namespace hp

extern "C" int dmpc_max_deviation(dmpc_ctx *ctx, int K_cols, const double *p, const double *prev_p, double *tol_out)
{
    if (!ctx) { g_err = "dmpc_max_deviation: ctx is NULL"; return -1; }
    if (K_cols < 1 || !p || !prev_p || !tol_out) FAIL(ctx, "dmpc_max_deviation: bad arguments");
    // `K = length(p)/3; for k = 1:K` on the 3 x K_cols matrix (maxDeviation.m:3-5): length() = max(3, K_cols), the loop visits floor(that / 3) columns
    const int nsteps = (K_cols > 3 ? K_cols : 3) / 3;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (ctx->hp_in.ensure((size_t)6 * nsteps * 8) || ctx->hp_out.ensure(16)) FAIL(ctx, "device allocation failed");
    double *dp = ctx->hp_in.as<double>(), *dq = dp + 3 * nsteps;
    unsigned long long *out = ctx->hp_out.as<unsigned long long>();
    HIPCHK(ctx, hipMemcpyAsync(dp, p, (size_t)3 * nsteps * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dq, prev_p, (size_t)3 * nsteps * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(out, 0, 8, st));
    hipLaunchKernelGGL(hp::max_dev_kernel, dim3((unsigned)((nsteps + 63) / 64)), dim3(64), 0, st, nsteps, (const double *)dp, (const double *)dq, out);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long bits = 0;
    HIPCHK(ctx, hipMemcpyAsync(&bits, out, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    std::memcpy(tol_out, &bits, 8);
    return 0;
}

extern "C" int dmpc_prop_state(dmpc_ctx *ctx, int n_rows, int n_cols, const double *A_p, const double *A_v, const double *A_initp,
                               const double *po, const double *vo, const double *off_p, const double *off_v, const double *a,
                               double *p, double *v)
{
    if (!ctx) { g_err = "dmpc_prop_state: ctx is NULL"; return -1; }
    if (n_rows < 1 || n_cols < 1 || !A_p || !A_v || !a || !p || !v || (A_initp && (!po || !vo))) FAIL(ctx, "dmpc_prop_state: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nA = (size_t)n_rows * n_cols;
    // layout of the staging buffer: A_p | A_v | A_initp | x0(6) | off(6) | a
    const size_t tot = 2 * nA + (size_t)n_rows * 6 + 12 + n_cols;
    if (ctx->hp_in.ensure(tot * 8) || ctx->hp_out.ensure((size_t)n_rows * 16 + 16)) FAIL(ctx, "device allocation failed");
    double *d = ctx->hp_in.as<double>();
    double *dAp = d, *dAv = d + nA, *dA0 = dAv + nA, *dx0 = dA0 + (size_t)n_rows * 6, *doff = dx0 + 6, *da = doff + 6;
    double x0[6] = {0, 0, 0, 0, 0, 0}, off[6] = {0, 0, 0, 0, 0, 0};
    for (int u = 0; u < 3; ++u) {
        if (po) x0[u] = po[u];
        if (vo) x0[3 + u] = vo[u];
        if (off_p) off[u] = off_p[u];
        if (off_v) off[3 + u] = off_v[u];
    }
    HIPCHK(ctx, hipMemcpyAsync(dAp, A_p, nA * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dAv, A_v, nA * 8, hipMemcpyHostToDevice, st));
    if (A_initp) HIPCHK(ctx, hipMemcpyAsync(dA0, A_initp, (size_t)n_rows * 48, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dx0, x0, 48, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(doff, off, 48, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(da, a, (size_t)n_cols * 8, hipMemcpyHostToDevice, st));
    double *dp = ctx->hp_out.as<double>(), *dv = dp + n_rows;
    hipLaunchKernelGGL(hp::prop_state_kernel, dim3((unsigned)((n_rows + 63) / 64)), dim3(64), 0, st, n_rows, n_cols, (const double *)dAp,
                       (const double *)dAv, A_initp ? (const double *)dA0 : (const double *)nullptr, (const double *)dx0,
                       (const double *)doff, (const double *)da, dp, dv);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(p, dp, (size_t)n_rows * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(v, dv, (size_t)n_rows * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

static int flag_kernel_common(dmpc_ctx *ctx, const char *who, int count3, const double *p, int extra_n, const double *extra,
                              int which, double tol, int32_t *out)
{
    if (!ctx) { g_err = std::string(who) + ": ctx is NULL"; return -1; }
    if (count3 < 1 || !p || !extra || !out) FAIL(ctx, std::string(who) + ": bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (ctx->hp_in.ensure(((size_t)count3 + extra_n) * 8) || ctx->hp_out.ensure(16)) FAIL(ctx, "device allocation failed");
    double *dp = ctx->hp_in.as<double>(), *dx = dp + count3;
    int *bad = ctx->hp_out.as<int>();
    HIPCHK(ctx, hipMemcpyAsync(dp, p, (size_t)count3 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dx, extra, (size_t)extra_n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(bad, 0, 4, st));
    if (which == 0)
        hipLaunchKernelGGL(hp::inbounds_kernel, dim3((unsigned)((count3 + 255) / 256)), dim3(256), 0, st, count3 / 3, (const double *)dp,
                           (const double *)dx, bad);
    else
        hipLaunchKernelGGL(hp::reached_kernel, dim3((unsigned)((count3 / 3 + 255) / 256)), dim3(256), 0, st, count3 / 3, (const double *)dp,
                           (const double *)dx, tol, bad);
    HIPCHK(ctx, hipGetLastError());
    int32_t b = 0;
    HIPCHK(ctx, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    *out = b ? 0 : 1;
    return 0;
}

extern "C" int dmpc_is_inbounds(dmpc_ctx *ctx, int npts, const double *p, const double *pmin, const double *pmax, int32_t *inbounds)
{
    if (!pmin || !pmax) { g_err = "dmpc_is_inbounds: bad arguments"; return -1; }
    const double lim[6] = {pmin[0], pmin[1], pmin[2], pmax[0], pmax[1], pmax[2]};
    return flag_kernel_common(ctx, "dmpc_is_inbounds", 3 * npts, p, 6, lim, 0, 0.0, inbounds);
}

extern "C" int dmpc_reached_goal(dmpc_ctx *ctx, int N, const double *p, const double *pf, double error_tol, int32_t *reached)
{
    return flag_kernel_common(ctx, "dmpc_reached_goal", 3 * N, p, 3 * N, pf, 1, error_tol, reached);
}
