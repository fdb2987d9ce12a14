// dmpc_postcheck_host.hip -- the host side of the post-checks (included by dmpc_api.hip; the kernels are in dmpc_postcheck.hip): the record of a
// call, what every post-check starts with (PcPrep), the three checks for the scenes of one context -- postcheck_one, clearance_one,
// setpoints_one --, the runner that sends a call to where its histories live (pc_run), the entries.
//
// The post-checks of S finished transitions (failure_rate.m:136-195) over the N_cmd commanded agents of N vehicles: histories, goals and every
// per-agent output are sized and strided by N_cmd; the M = N - N_cmd other vehicles rest at po_static [S][M][3] (dmpc_postcheck_cmd) or follow
// path [S][M][P][3] (dmpc_postcheck_scripted); dmpc_postcheck_clearance takes either.  pk == null: the histories dmpc_transition left resident
// on the device (no PCIe round trip) -- of a split batch, in the parts' own contexts.
//
// The outputs and options of the three kinds of check; every output may be null unless said otherwise.
struct PcReport {   // dmpc_postcheck, _cmd, _scripted
    const double *pf = nullptr;                                              // [S][N_cmd][3], required
    double *r_factor = nullptr, *h_scaled = nullptr; int32_t *n_samples = nullptr;   // [S], as the four below
    double *min_dist = nullptr; int32_t *violation = nullptr;
    double *totdist = nullptr, *traj_time = nullptr;
    double *p_interp = nullptr; int ns_alloc = 0;                            // [S][N_cmd][ns_alloc][3]
    double *min_dist_other = nullptr; int32_t *violation_other = nullptr;    // [S]: the commanded agents against the static or the scripted vehicles
    double *p_scripted = nullptr;                                            // [S][M][ns_alloc][3]: the scripted vehicles' interpolated positions
};
struct PcClearance {   // dmpc_postcheck_clearance
    double reach = INFINITY;
    double *dist = nullptr; int32_t *partner = nullptr, *sample = nullptr;   // [S][N_cmd][2]
};
struct PcSetpoints {   // dmpc_postcheck_setpoints
    int smp0 = 0, ns_alloc = 0;                                              // the window of samples
    double *p_sp = nullptr, *v_sp = nullptr, *a_sp = nullptr;                // [S][N_cmd][ns_alloc][3]
    double *v_peak = nullptr; int32_t *v_peak_sample = nullptr;              // [S][N_cmd], as the two below
    double *a_peak = nullptr; int32_t *a_peak_sample = nullptr;
    double *r_factor = nullptr, *h_scaled = nullptr; int32_t *n_samples = nullptr;   // [S]
};

// one call of a post-check entry, as the entry filled it (the member of its kind; the other two stay empty)
struct PostcheckCall {
    int S = 0, N = 0, N_cmd = 0, KT_alloc = 0;
    const int32_t *K_T_used = nullptr, *scene_mask = nullptr;
    const double *pk = nullptr, *vk = nullptr, *ak = nullptr;   // all three or none
    double vmax = 0, amax = 0, Ts = 0;
    const double *po_static = nullptr, *path = nullptr; int P = 0;
    PcReport report; PcClearance clearance; PcSetpoints setpoints;
    int M() const { return N - N_cmd; }
    // the same call for scenes [s0, s0 + sn): the one place that knows each array's stride per scene
    PostcheckCall scenes(int s0, int sn) const {
        auto at = [](auto *p, size_t off) { return p ? p + off : nullptr; };
        const size_t z = (size_t)s0, a0 = z * N_cmd, m0 = z * M(), h0 = a0 * (size_t)KT_alloc * 3;
        PostcheckCall c = *this; c.S = sn;
        c.K_T_used = at(K_T_used, z); c.scene_mask = at(scene_mask, z);
        c.pk = at(pk, h0); c.vk = at(vk, h0); c.ak = at(ak, h0);
        c.po_static = at(po_static, m0 * 3); c.path = at(path, m0 * P * 3);
        PcReport &r = c.report; PcClearance &l = c.clearance; PcSetpoints &t = c.setpoints;
        const size_t w0 = a0 * (size_t)r.ns_alloc * 3, t0 = a0 * (size_t)t.ns_alloc * 3;
        r.pf = at(r.pf, a0 * 3);
        r.r_factor = at(r.r_factor, z); r.h_scaled = at(r.h_scaled, z); r.n_samples = at(r.n_samples, z);
        r.min_dist = at(r.min_dist, z); r.violation = at(r.violation, z); r.totdist = at(r.totdist, z); r.traj_time = at(r.traj_time, z);
        r.p_interp = at(r.p_interp, w0); r.p_scripted = at(r.p_scripted, m0 * (size_t)r.ns_alloc * 3);
        r.min_dist_other = at(r.min_dist_other, z); r.violation_other = at(r.violation_other, z);
        l.dist = at(l.dist, a0 * 2); l.partner = at(l.partner, a0 * 2); l.sample = at(l.sample, a0 * 2);
        t.p_sp = at(t.p_sp, t0); t.v_sp = at(t.v_sp, t0); t.a_sp = at(t.a_sp, t0);
        t.v_peak = at(t.v_peak, a0); t.v_peak_sample = at(t.v_peak_sample, a0); t.a_peak = at(t.a_peak, a0); t.a_peak_sample = at(t.a_peak_sample, a0);
        t.r_factor = at(t.r_factor, z); t.h_scaled = at(t.h_scaled, z); t.n_samples = at(t.n_samples, z);
        return c;
    }
};

// What every post-check starts with (failure_rate.m:136-162): the histories on the device (uploaded, or the resident ones copied), r_factor,
// h_scaled and the sample count of every scene, the rescaled knots and their spline.
struct PcPrep {
    std::vector<int32_t> kt, ns;     // K_T_used (0: masked scene), number of 100 Hz samples
    std::vector<double> rf, hs;      // r_factor, h_scaled
    int ns_max = 0;
    // per-scene scalars on the device: kt_used(int) | rf | hs | ns(int) | mind2(u64) | totdist | traj_time
    int *d_kt = nullptr, *d_ns = nullptr;
    double *d_rf = nullptr, *d_hs = nullptr, *d_tot = nullptr, *d_tt = nullptr;
    unsigned long long *d_min = nullptr;
    double *dp = nullptr, *dv = nullptr, *da = nullptr;   // rescaled histories (dp: the knots of the spline, ctx->pc_M its second derivatives)
    // r_factor, h_scaled and n_samples of every scene to the caller: NaN / NaN / 0 for a masked scene
    void scalars_out(double *r_factor, double *h_scaled, int32_t *n_samples) const {
        for (size_t s = 0; s < kt.size(); ++s) {
            if (r_factor) r_factor[s] = rf[s];
            if (h_scaled) h_scaled[s] = hs[s];
            if (n_samples) n_samples[s] = ns[s];
        }
    }
};
// `who`: the entry's name in the messages; pf may be NULL.
static int pc_prepare(dmpc_ctx *ctx, const std::string &who, const PostcheckCall &c, const double *pf, PcPrep &q)
{
    const int S = c.S, N = c.N_cmd, KT_alloc = c.KT_alloc;
    if (S < 1 || N < 1 || KT_alloc < 2 || !c.K_T_used || !(c.vmax > 0) || !(c.amax > 0) || !(c.Ts > 0))
        FAIL(ctx, who + ": bad arguments");
    std::vector<int32_t> &kt = q.kt;
    kt.assign((size_t)S, 0);
    for (int s = 0; s < S; ++s) {
        const bool on = !c.scene_mask || c.scene_mask[s];
        if (on && (c.K_T_used[s] < 2 || c.K_T_used[s] > KT_alloc)) FAIL(ctx, who + ": K_T_used out of range");
        kt[s] = on ? c.K_T_used[s] : 0;   // masked scenes (aborted trials, failure_rate.m:136) are skipped by every kernel
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t A = (size_t)S * N, hist = A * (size_t)KT_alloc * 24;
    if (ctx->pc_p.ensure(hist) || ctx->pc_v.ensure(hist) || ctx->pc_a.ensure(hist) || ctx->pc_M.ensure(hist) ||
        ctx->pc_w.ensure(hist) || ctx->pc_scene.ensure((size_t)S * 64) || ctx->pc_agent.ensure(A * 16) || ctx->pf.ensure(A * 24))
        FAIL(ctx, "device allocation failed");
    if (c.pk) {
        if (!c.vk || !c.ak) FAIL(ctx, who + ": vk/ak missing");
        HIPCHK(ctx, hipMemcpyAsync(ctx->pc_p.p, c.pk, hist, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->pc_v.p, c.vk, hist, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->pc_a.p, c.ak, hist, hipMemcpyHostToDevice, st));
    } else {
        if (ctx->hist_S != S || ctx->hist_N != N || ctx->hist_KT != KT_alloc)
            FAIL(ctx, who + ": no resident histories of this shape (run dmpc_transition first or pass pk/vk/ak)");
        HIPCHK(ctx, hipMemcpyAsync(ctx->pc_p.p, ctx->hist_p.p, hist, hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->pc_v.p, ctx->hist_v.p, hist, hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->pc_a.p, ctx->hist_a.p, hist, hipMemcpyDeviceToDevice, st));
    }
    if (pf) HIPCHK(ctx, hipMemcpyAsync(ctx->pf.p, pf, A * 24, hipMemcpyHostToDevice, st));
    char *sc = ctx->pc_scene.as<char>();
    q.d_kt = (int *)sc;
    q.d_rf = (double *)(sc + (size_t)S * 8); q.d_hs = (double *)(sc + (size_t)S * 16);
    q.d_ns = (int *)(sc + (size_t)S * 24);
    q.d_min = (unsigned long long *)(sc + (size_t)S * 32);
    q.d_tot = (double *)(sc + (size_t)S * 40); q.d_tt = (double *)(sc + (size_t)S * 48);
    HIPCHK(ctx, hipMemcpyAsync(q.d_kt, kt.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(q.d_min, 0x7f, (size_t)S * 8, st));   // 0x7f7f... = a huge finite double
    q.dp = ctx->pc_p.as<double>(); q.dv = ctx->pc_v.as<double>(); q.da = ctx->pc_a.as<double>();
    hipLaunchKernelGGL(pc::rfactor_kernel, dim3((unsigned)S), dim3(256), 0, st, N, KT_alloc, (const int *)q.d_kt, (const double *)q.dv,
                       (const double *)q.da, c.vmax, c.amax, q.d_rf);
    std::vector<double> &rf = q.rf, &hs = q.hs;
    std::vector<int32_t> &ns = q.ns;
    rf.assign((size_t)S, 0.0); hs.assign((size_t)S, 0.0); ns.assign((size_t)S, 0);
    HIPCHK(ctx, hipMemcpyAsync(rf.data(), q.d_rf, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    q.ns_max = 0;
    for (int s = 0; s < S; ++s) {
        if (!kt[s]) { rf[s] = hs[s] = NAN; ns[s] = 0; continue; }
        if (!(std::isfinite(rf[s]) && rf[s] > 0))   // MATLAB: h_scaled = 0, tk = 0:0:T is empty and spline() errors
            FAIL(ctx, who + ": degenerate r_factor (all-zero or non-finite histories)");
        hs[s] = ctx->prm.h / std::sqrt(rf[s]);                                   // failure_rate.m:146
        const double T = (kt[s] - 1) * hs[s];                              // :149
        ns[s] = (std::isfinite(T) && T / c.Ts < 5e7) ? (int)std::floor(T / c.Ts + 1e-10) + 1 : -1;   // :152
        if (ns[s] < 1) FAIL(ctx, who + ": degenerate r_factor (all-zero or non-finite histories)");
        q.ns_max = std::max(q.ns_max, (int)ns[s]);
    }
    HIPCHK(ctx, hipMemcpyAsync(q.d_hs, hs.data(), (size_t)S * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(q.d_ns, ns.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
    const unsigned b3 = (unsigned)((A * 3 + 255) / 256);
    hipLaunchKernelGGL(pc::rescale_kernel, dim3(b3), dim3(256), 0, st, S, N, KT_alloc, (const int *)q.d_kt, (const double *)q.d_rf,
                       (const double *)q.d_hs, q.dp, q.dv, q.da);
    hipLaunchKernelGGL(pc::spline_kernel, dim3(b3), dim3(256), 0, st, S, N, KT_alloc, (const int *)q.d_kt, (const double *)q.d_hs,
                       (const double *)q.dp, ctx->pc_M.as<double>(), ctx->pc_w.as<double>());
    return 0;
}

// the cell grid of the post-checks over the workspace: cells `edge` wide in the metric of the check (z: edge * c) plus a margin of one cell
// per side, at most 32768 of them (`edge` grows until they fit)
static pc::Grid pc_make_grid(const dmpc_params &pr, double &edge)
{
    pc::Grid g{};
    for (;;) {
        g.nx = (int)std::ceil((pr.pmax[0] - pr.pmin[0]) / edge) + 2;
        g.ny = (int)std::ceil((pr.pmax[1] - pr.pmin[1]) / edge) + 2;
        g.nz = (int)std::ceil((pr.pmax[2] - pr.pmin[2]) / (edge * pr.c)) + 2;
        if ((double)g.nx * g.ny * g.nz <= 32768.0) break;
        edge *= 1.25;
    }
    g.x0 = pr.pmin[0] - edge; g.y0 = pr.pmin[1] - edge; g.z0 = pr.pmin[2] - edge * pr.c;
    g.inv_e = 1.0 / edge; g.inv_ez = 1.0 / (edge * pr.c);
    return g;
}

// samples per pass: at most 256 MB at a time, between 1 and `cap`, and no more than there are (ns_max; 1 when there is none)
static int pc_pass_size(double bytes_per_sample, int cap, int ns_max)
{
    const int n = (int)std::min(std::max(std::floor(256.0 * 1048576.0 / bytes_per_sample), 1.0), (double)cap);
    return n > ns_max ? std::max(ns_max, 1) : n;
}

// the buffers of the sample cell grid: `sbn` (scene, sample) pairs of a pass with `tot` points in `ncell` cells each
static bool pc_grid_ensure(dmpc_ctx *ctx, size_t sbn, size_t tot, int ncell)
{
    return ctx->pc_pts.ensure(tot * 24) || ctx->pc_cell.ensure(tot * 4) || ctx->pc_sorted.ensure(tot * 4) || ctx->pc_fill.ensure(sbn * ncell * 4) ||
           ctx->pc_start.ensure(sbn * ((size_t)ncell + 1) * 4);
}
// the grid of one pass from the cells and counts the table kernel left: scan, scatter, counts back to zero for the next pass
static int pc_grid_build(dmpc_ctx *ctx, size_t sbn, size_t tot, int N, int ncell)
{
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(grid_scan_kernel, dim3((unsigned)sbn), dim3(1024), 0, st, ncell, ctx->pc_fill.as<int>(), ctx->pc_start.as<int>());
    hipLaunchKernelGGL(pc::grid_scatter_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, tot, N, ncell,
                       (const int *)ctx->pc_cell.as<int>(), (const int *)ctx->pc_start.as<int>(), ctx->pc_fill.as<int>(), ctx->pc_sorted.as<int>());
    HIPCHK(ctx, hipMemsetAsync(ctx->pc_fill.p, 0, sbn * ncell * 4, st));
    return 0;
}

// One launch of sample_table_kernel for samples [smp0, smp0 + SB) of every scene, and what differs between the tables of the three searches:
// the columns (N of them; the first Nc are the commanded agents' spline and count into the context's cell arrays, the others rest at po_static
// or follow the spline yk / Mk), the cell grid, where the points go and which interpolated positions are kept on the way.
struct PcTable {
    int N = 0, Nc = 0;
    const double *po_static = nullptr, *yk = nullptr, *Mk = nullptr;
    int with_grid = 0; pc::Grid g{};
    double *pts = nullptr, *p_interp = nullptr, *p_scripted = nullptr; int ns_alloc = 0;
};
static void pc_sample_table(dmpc_ctx *ctx, const PostcheckCall &c, const PcPrep &q, const PcTable &t, int smp0, int SB)
{
    const size_t tot = (size_t)c.S * SB * t.N;
    const bool own = t.Nc > 0;
    hipLaunchKernelGGL(pc::sample_table_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, c.S, t.N, t.Nc, c.KT_alloc,
                       (const int *)q.d_kt, (const double *)q.d_hs, (const int *)q.d_ns, c.Ts, smp0, SB, own ? (const double *)q.dp : nullptr,
                       own ? (const double *)ctx->pc_M.as<double>() : nullptr, t.po_static, t.yk, t.Mk, t.with_grid, t.g, t.pts,
                       own ? ctx->pc_cell.as<int>() : nullptr, own ? ctx->pc_fill.as<int>() : nullptr, t.p_interp, t.p_scripted, t.ns_alloc);
}

// the scripted vehicles' splines on the commanded agents' knots: path[S][M][P][3] to the device (with room for S u64 behind it), the knots
// pc_sc_y and their second derivatives pc_sc_M
static int pc_scripted_splines(dmpc_ctx *ctx, const std::string &what, const PostcheckCall &c, const PcPrep &q)
{
    hipStream_t st = ctx->stream;
    const int S = c.S, M = c.M(), KT_alloc = c.KT_alloc, P = c.P;
    const size_t V = (size_t)S * M, knots = V * (size_t)KT_alloc * 24, nk = V * (size_t)KT_alloc * 3;
    if (ctx->pc_sc_path.ensure(V * (size_t)P * 24 + (size_t)S * 8) || ctx->pc_sc_y.ensure(knots) || ctx->pc_sc_M.ensure(knots) || ctx->pc_sc_w.ensure(knots))
        FAIL(ctx, "device allocation failed (" + what + ", scripted vehicles)");
    HIPCHK(ctx, hipMemcpyAsync(ctx->pc_sc_path.p, c.path, V * (size_t)P * 24, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pc::scripted_knots_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, S, M, KT_alloc, P, (const int *)q.d_kt,
                       (const double *)ctx->pc_sc_path.as<double>(), ctx->pc_sc_y.as<double>());
    hipLaunchKernelGGL(pc::spline_kernel, dim3((unsigned)((V * 3 + 255) / 256)), dim3(256), 0, st, S, M, KT_alloc, (const int *)q.d_kt,
                       (const double *)q.d_hs, (const double *)ctx->pc_sc_y.as<double>(), ctx->pc_sc_M.as<double>(), ctx->pc_sc_w.as<double>());
    return 0;
}
// the static vehicles' positions po_static[S][M][3] to the device (pc_static, with room for S u64 behind them)
static int pc_static_upload(dmpc_ctx *ctx, const std::string &what, const PostcheckCall &c)
{
    const size_t bytes = (size_t)c.S * c.M() * 24;
    if (ctx->pc_static.ensure(bytes + (size_t)c.S * 8)) FAIL(ctx, "device allocation failed (" + what + ", static vehicles)");
    HIPCHK(ctx, hipMemcpyAsync(ctx->pc_static.p, c.po_static, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

// The report of dmpc_postcheck[_cmd, _scripted] for the scenes of ONE context (failure_rate.m:136-195): rescale, 100 Hz not-a-knot spline,
// pairwise ellipsoidal collision check, path length, trajectory time; the commanded agents against the static vehicles, or against the
// scripted ones (min_dist_other, violation_other; p_scripted).
static int postcheck_one(dmpc_ctx *ctx, const PostcheckCall &c)
{
    const PcReport &r = c.report;
    PcPrep q;
    if (pc_prepare(ctx, "dmpc_postcheck", c, r.pf, q)) return -1;
    hipStream_t st = ctx->stream;
    const int S = c.S, N = c.N_cmd, M = c.M(), KT_alloc = c.KT_alloc, ns_alloc = r.ns_alloc, ns_max = q.ns_max;
    const size_t A = (size_t)S * N;
    std::vector<double> md(S), tot(S), tt(S);
    double *d_interp = nullptr;
    if (r.p_interp) {
        if (ns_alloc < 1) FAIL(ctx, "dmpc_postcheck: ns_alloc must be positive with p_interp");
        if (ctx->pc_interp.ensure(A * (size_t)ns_alloc * 24)) FAIL(ctx, "device allocation failed");
        d_interp = ctx->pc_interp.as<double>();
        HIPCHK(ctx, hipMemsetAsync(d_interp, 0, A * (size_t)ns_alloc * 24, st));
    }
    // grid search of the large scenes: `grid_pass(scene_on)` runs every sample batch; scene_on = null: cell-grid search of all
    // scenes, else brute force over the same batch positions for the scenes flagged in it
    bool use_grid = N > PC_BRUTE_MAX && ns_max > 0;
    pc::Grid g{};
    double edge = 2.0 * ctx->prm.rmin;
    int SB = 1, ncell = 1;
    if (use_grid) {   // (ns_max > 0)
        g = pc_make_grid(ctx->prm, edge);
        ncell = g.nx * g.ny * g.nz;
        SB = pc_pass_size((double)S * ((double)N * 36.0 + (double)ncell * 8.0 + 4.0), 256, ns_max);
        const size_t sbn = (size_t)S * SB;
        if (pc_grid_ensure(ctx, sbn, sbn * N, ncell) || ctx->pc_on.ensure((size_t)S * 4)) FAIL(ctx, "device allocation failed (post-check cell grid)");
        HIPCHK(ctx, hipMemsetAsync(ctx->pc_fill.p, 0, sbn * ncell * 4, st));
    }
    auto grid_pass = [&](const int *scene_on) -> int {
        const size_t sbn = (size_t)S * SB, tot = sbn * N;
        PcTable t;
        t.N = t.Nc = N; t.with_grid = 1; t.g = g; t.pts = ctx->pc_pts.as<double>(); t.p_interp = scene_on ? nullptr : d_interp; t.ns_alloc = ns_alloc;
        for (int smp0 = 0; smp0 < ns_max; smp0 += SB) {
            pc_sample_table(ctx, c, q, t, smp0, SB);
            if (!scene_on) {
                if (pc_grid_build(ctx, sbn, tot, N, ncell)) return -1;
                hipLaunchKernelGGL(pc::grid_pairs_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)SB, (unsigned)S), dim3(256), 0, st, N, SB, g,
                                   1.0 / ctx->prm.c, (const double *)ctx->pc_pts.as<double>(), (const int *)ctx->pc_cell.as<int>(),
                                   (const int *)ctx->pc_start.as<int>(), (const int *)ctx->pc_sorted.as<int>(), q.d_min);
            } else {
                HIPCHK(ctx, hipMemsetAsync(ctx->pc_fill.p, 0, sbn * ncell * 4, st));   // (the evaluation counted again)
                hipLaunchKernelGGL(pc::pairs_brute_pts_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)SB, (unsigned)S), dim3(256), 0, st, N, SB,
                                   1.0 / ctx->prm.c, (const double *)ctx->pc_pts.as<double>(), (const int *)ctx->pc_cell.as<int>(), scene_on, q.d_min);
            }
            HIPCHK(ctx, hipGetLastError());
        }
        return 0;
    };
    if (use_grid) { if (grid_pass(nullptr)) return -1; }
    else if (ns_max > 0)
    hipLaunchKernelGGL(pc::pairdist_kernel, dim3((unsigned)((ns_max + PC_SAMPLES_PER_BLOCK - 1) / PC_SAMPLES_PER_BLOCK), (unsigned)S),
                       dim3(256), (size_t)N * 24, st, N, KT_alloc, (const int *)q.d_kt, (const double *)q.d_hs, (const int *)q.d_ns, c.Ts,
                       1.0 / ctx->prm.c, (const double *)q.dp, (const double *)ctx->pc_M.as<double>(), q.d_min, d_interp, ns_alloc);
    // scripted vehicles: their splines on the commanded agents' knots, then every (commanded agent, scripted vehicle) pair per sample
    const bool with_scripted = c.path && M > 0 && (r.min_dist_other || r.violation_other || r.p_scripted);
    double *d_sc_interp = nullptr;
    std::vector<double> mdsc(S, 0.0);
    if (with_scripted) {
        const size_t V = (size_t)S * M;
        if (r.p_scripted && ns_alloc < 1) FAIL(ctx, "dmpc_postcheck_scripted: ns_alloc must be positive with p_scripted");
        const int SBs = pc_pass_size((double)V * 24.0, 4096, ns_max);   // (scripted positions)
        if (ctx->pc_sc_pts.ensure(V * (size_t)SBs * 24) || (r.p_scripted && ctx->pc_sc_interp.ensure(V * (size_t)ns_alloc * 24)))
            FAIL(ctx, "device allocation failed (post-check, scripted vehicles)");
        if (pc_scripted_splines(ctx, "post-check", c, q)) return -1;
        unsigned long long *d_min_sc = (unsigned long long *)(ctx->pc_sc_path.as<char>() + V * (size_t)c.P * 24);
        HIPCHK(ctx, hipMemsetAsync(d_min_sc, 0x7f, (size_t)S * 8, st));
        if (r.p_scripted) {
            d_sc_interp = ctx->pc_sc_interp.as<double>();
            HIPCHK(ctx, hipMemsetAsync(d_sc_interp, 0, V * (size_t)ns_alloc * 24, st));
        }
        PcTable t;
        t.N = M; t.yk = ctx->pc_sc_y.as<double>(); t.Mk = ctx->pc_sc_M.as<double>(); t.pts = ctx->pc_sc_pts.as<double>(); t.p_scripted = d_sc_interp; t.ns_alloc = ns_alloc;
        for (int smp0 = 0; smp0 < ns_max; smp0 += SBs) {
            const int nb = ns_max - smp0 < SBs ? ns_max - smp0 : SBs;
            pc_sample_table(ctx, c, q, t, smp0, SBs);
            hipLaunchKernelGGL(pc::scripted_pairs_kernel, dim3((unsigned)nb, (unsigned)S), dim3(256), 0, st, N, M, KT_alloc, (const int *)q.d_kt,
                               (const double *)q.d_hs, (const int *)q.d_ns, c.Ts, smp0, SBs, 1.0 / ctx->prm.c, (const double *)q.dp,
                               (const double *)ctx->pc_M.as<double>(), (const double *)ctx->pc_sc_pts.as<double>(), d_min_sc);
        }
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(mdsc.data(), d_min_sc, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    }
    // uncommanded vehicles: every (commanded agent, sample) against every static vehicle (all pairs, exact)
    const bool with_static = !c.path && M > 0 && (r.min_dist_other || r.violation_other);
    std::vector<double> mds(S, 0.0);
    if (with_static) {
        if (pc_static_upload(ctx, "post-check", c)) return -1;
        unsigned long long *d_min_st = (unsigned long long *)(ctx->pc_static.as<char>() + (size_t)S * M * 24);
        HIPCHK(ctx, hipMemsetAsync(d_min_st, 0x7f, (size_t)S * 8, st));
        if (ns_max > 0)
            hipLaunchKernelGGL(pc::static_pairs_kernel, dim3((unsigned)(((size_t)N * ns_max + 255) / 256), (unsigned)S), dim3(256), 0, st, N, M, KT_alloc,
                               (const int *)q.d_kt, (const double *)q.d_hs, (const int *)q.d_ns, c.Ts, 1.0 / ctx->prm.c, (const double *)q.dp,
                               (const double *)ctx->pc_M.as<double>(), (const double *)ctx->pc_static.as<double>(), d_min_st);
        HIPCHK(ctx, hipMemcpyAsync(mds.data(), d_min_st, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    }
    double *d_dist = ctx->pc_agent.as<double>();
    int *d_tidx = (int *)(ctx->pc_agent.as<char>() + A * 8);
    hipLaunchKernelGGL(pc::path_kernel, dim3((unsigned)((A + 63) / 64)), dim3(64), 0, st, S, N, KT_alloc, (const int *)q.d_kt,
                       (const double *)q.d_hs, (const int *)q.d_ns, c.Ts, (const double *)q.dp, (const double *)ctx->pc_M.as<double>(),
                       (const double *)ctx->pf.as<double>(), d_dist, d_tidx);
    hipLaunchKernelGGL(pc::finish_kernel, dim3((unsigned)S), dim3(256), 0, st, N, (const double *)d_dist, (const int *)d_tidx, c.Ts,
                       q.d_tot, q.d_tt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(md.data(), q.d_min, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    if (use_grid) {
        // scenes in which the grid found no pair closer than its cell edge: nothing is closer than that (no violation); the exact
        // minimum, which the interface reports, takes the brute-force search over the same sample batches
        HIPCHK(ctx, hipStreamSynchronize(st));
        std::vector<int> on(S, 0);
        int n_on = 0;
        for (int s = 0; s < S; ++s)
            if (q.kt[s] && N > 1 && !(md[s] <= edge * edge)) { on[s] = 1; n_on++; }
        ctx->pc_fallback_scenes = n_on;
        if (n_on) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->pc_on.p, on.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
            if (grid_pass(ctx->pc_on.as<int>())) return -1;
            HIPCHK(ctx, hipMemcpyAsync(md.data(), q.d_min, (size_t)S * 8, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(tot.data(), q.d_tot, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(tt.data(), q.d_tt, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    if (r.p_interp) HIPCHK(ctx, hipMemcpyAsync(r.p_interp, d_interp, A * (size_t)ns_alloc * 24, hipMemcpyDeviceToHost, st));
    if (d_sc_interp) HIPCHK(ctx, hipMemcpyAsync(r.p_scripted, d_sc_interp, (size_t)S * M * (size_t)ns_alloc * 24, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    q.scalars_out(r.r_factor, r.h_scaled, r.n_samples);
    for (int s = 0; s < S; ++s) {
        const bool on = q.kt[s] != 0;   // (a masked scene: NaN, no violation)
        const double ds = !on ? NAN : with_scripted ? std::sqrt(mdsc[s]) : with_static ? std::sqrt(mds[s]) : INFINITY;
        const double d = !on ? NAN : (N > 1) ? std::sqrt(md[s]) : INFINITY;
        if (r.min_dist_other) r.min_dist_other[s] = ds;
        if (r.violation_other) r.violation_other[s] = on && ds < ctx->prm.rmin - 0.05;
        if (r.min_dist) r.min_dist[s] = d;
        if (r.violation) r.violation[s] = on && d < ctx->prm.rmin - 0.05;         // failure_rate.m:175
        if (r.totdist) r.totdist[s] = on ? tot[s] : NAN;
        if (r.traj_time) r.traj_time[s] = on ? tt[s] : NAN;
    }
    return 0;
}

// The clearance report of dmpc_postcheck_clearance for the scenes of ONE context: the preamble of every post-check over the Nc commanded
// agents, then per batch of samples one point set of all N vehicles, one search and the fold of its partials (dmpc_postcheck.hip).
static int clearance_one(dmpc_ctx *ctx, const PostcheckCall &c)
{
    const PcClearance &l = c.clearance;
    PcPrep q;
    if (pc_prepare(ctx, "dmpc_postcheck_clearance", c, nullptr, q)) return -1;
    hipStream_t st = ctx->stream;
    const int S = c.S, N = c.N, Nc = c.N_cmd, M = c.M(), ns_max = q.ns_max;
    const double reach = l.reach;
    PcTable t;
    t.N = N; t.Nc = Nc;
    if (M > 0 && c.path) {   // scripted vehicles: their splines on the commanded agents' knots (as dmpc_postcheck_scripted makes them)
        if (pc_scripted_splines(ctx, "clearance", c, q)) return -1;
        t.yk = ctx->pc_sc_y.as<double>(); t.Mk = ctx->pc_sc_M.as<double>();
    } else if (M > 0) {
        if (pc_static_upload(ctx, "clearance", c)) return -1;
        t.po_static = ctx->pc_static.as<double>();
    }
    // The search.  Cell grid: cells at least `reach` wide, so every pair closer than `reach` lies in adjacent cells and is evaluated -- a slot
    // whose best is < reach is exact, any other is reported empty.  Tiled all-pairs: small tables, no bound on the distance, or a bound so
    // wide that the workspace is one cell.
    double edge = 2.0 * ctx->prm.rmin;
    pc::Grid g = pc_make_grid(ctx->prm, edge);   // (the edge dmpc_postcheck chooses)
    bool use_grid = N > PC_BRUTE_MAX && std::isfinite(reach);
    if (use_grid && reach > edge) { edge = reach; g = pc_make_grid(ctx->prm, edge); }
    if (g.nx <= 3 && g.ny <= 3 && g.nz <= 3) use_grid = false;   // (one cell and its margin)
    const int ncell = g.nx * g.ny * g.nz;
    // samples per chunk (= per workgroup) and per batch: at most 256 MB of positions, grid and partials at a time
    int CH = ctx->opt.clear_chunk > 0 ? ctx->opt.clear_chunk : 8;
    const double per_sample = (double)S * ((double)N * 24.0 + (use_grid ? (double)N * 8.0 + (double)ncell * 8.0 + 4.0 : 0.0) + (double)Nc * 32.0 / CH);
    const int SB = pc_pass_size(per_sample, 256, ns_max);
    if (CH > SB) CH = SB;
    const int nchunk = (SB + CH - 1) / CH;
    const size_t sbn = (size_t)S * SB, tot = sbn * N, slots = (size_t)S * Nc * 2;
    if (ctx->pc_pts.ensure(tot * 24) || ctx->pc_cl_part.ensure((size_t)nchunk * slots * 16) || ctx->pc_cl_run.ensure(slots * 16) || ctx->pc_cl_out.ensure(slots * 16) ||
        (use_grid && pc_grid_ensure(ctx, sbn, tot, ncell)))
        FAIL(ctx, "device allocation failed (clearance)");
    t.with_grid = use_grid ? 1 : 0; t.g = g; t.pts = ctx->pc_pts.as<double>();
    double *part_d2 = ctx->pc_cl_part.as<double>(), *run_d2 = ctx->pc_cl_run.as<double>(), *o_dist = ctx->pc_cl_out.as<double>();
    int *part_smp = (int *)(part_d2 + (size_t)nchunk * slots), *part_j = part_smp + (size_t)nchunk * slots;
    int *run_smp = (int *)(run_d2 + slots), *run_j = run_smp + slots;
    int *o_partner = (int *)(o_dist + slots), *o_sample = o_partner + slots;
    const double cinv = 1.0 / ctx->prm.c;
    const dim3 search((unsigned)((Nc + 255) / 256), (unsigned)nchunk, (unsigned)S);
    auto finish = [&](int chunks, int first, int last) {
        hipLaunchKernelGGL(pc::clear_finish_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, slots, Nc, chunks, first, last, (const int *)q.d_kt,
                           reach, (const double *)part_d2, (const int *)part_smp, (const int *)part_j, run_d2, run_smp, run_j, o_dist, o_partner, o_sample);
    };
    if (use_grid) HIPCHK(ctx, hipMemsetAsync(ctx->pc_fill.p, 0, sbn * ncell * 4, st));
    if (ns_max < 1) finish(0, 1, 1);   // (every scene masked)
    for (int smp0 = 0; smp0 < ns_max; smp0 += SB) {
        pc_sample_table(ctx, c, q, t, smp0, SB);
        if (use_grid) {
            if (pc_grid_build(ctx, sbn, tot, N, ncell)) return -1;
            hipLaunchKernelGGL(pc::clear_grid_kernel, search, dim3(256), 0, st, S, N, Nc, SB, CH, smp0, (const int *)q.d_ns, g, cinv,
                               (const double *)ctx->pc_pts.as<double>(), (const int *)ctx->pc_cell.as<int>(), (const int *)ctx->pc_start.as<int>(),
                               (const int *)ctx->pc_sorted.as<int>(), part_d2, part_smp, part_j);
        } else {
            hipLaunchKernelGGL(pc::clear_brute_kernel, search, dim3(256), 0, st, S, N, Nc, SB, CH, smp0, (const int *)q.d_ns, cinv,
                               (const double *)ctx->pc_pts.as<double>(), part_d2, part_smp, part_j);
        }
        finish(nchunk, smp0 == 0, smp0 + SB >= ns_max);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipGetLastError());
    if (l.dist) HIPCHK(ctx, hipMemcpyAsync(l.dist, o_dist, slots * 8, hipMemcpyDeviceToHost, st));
    if (l.partner) HIPCHK(ctx, hipMemcpyAsync(l.partner, o_partner, slots * 4, hipMemcpyDeviceToHost, st));
    if (l.sample) HIPCHK(ctx, hipMemcpyAsync(l.sample, o_sample, slots * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// The setpoints and the limits report of dmpc_postcheck_setpoints for the scenes of ONE context: the preamble of every post-check, the splines
// of the rescaled velocity and acceleration histories next to the position one, then the samples in ascending runs -- what lies in front of
// the window and behind it in one launch each without stores, the window in passes of SB samples that are staged on the device and copied
// out before the next (dmpc_postcheck.hip).
static int setpoints_one(dmpc_ctx *ctx, const PostcheckCall &c)
{
    const PcSetpoints &t = c.setpoints;
    PcPrep q;
    if (pc_prepare(ctx, "dmpc_postcheck_setpoints", c, nullptr, q)) return -1;
    hipStream_t st = ctx->stream;
    const int S = c.S, N = c.N_cmd, KT_alloc = c.KT_alloc, smp0 = t.smp0, ns_alloc = t.ns_alloc, ns_max = q.ns_max;
    const size_t A = (size_t)S * N, hist = A * (size_t)KT_alloc * 24;
    if (ctx->pc_Mv.ensure(hist) || ctx->pc_Ma.ensure(hist)) FAIL(ctx, "device allocation failed (setpoints)");
    const unsigned b3 = (unsigned)((A * 3 + 255) / 256);
    hipLaunchKernelGGL(pc::spline_kernel, dim3(b3), dim3(256), 0, st, S, N, KT_alloc, (const int *)q.d_kt, (const double *)q.d_hs,
                       (const double *)q.dv, ctx->pc_Mv.as<double>(), ctx->pc_w.as<double>());
    hipLaunchKernelGGL(pc::spline_kernel, dim3(b3), dim3(256), 0, st, S, N, KT_alloc, (const int *)q.d_kt, (const double *)q.d_hs,
                       (const double *)q.da, ctx->pc_Ma.as<double>(), ctx->pc_w.as<double>());
    // samples per pass over the window: at most 256 MB of staged setpoints at a time
    double *host[3] = {t.p_sp, t.v_sp, t.a_sp};
    const int n_arr = (host[0] ? 1 : 0) + (host[1] ? 1 : 0) + (host[2] ? 1 : 0);
    int SB = 0;
    if (n_arr) {
        SB = pc_pass_size((double)A * 24.0 * n_arr, ns_alloc, ns_alloc);   // (no cap of its own: the window)
        if (ctx->opt.setpoint_batch > 0) SB = std::min(ctx->opt.setpoint_batch, ns_alloc);
    }
    // the runs: [lo, hi) and whether the run is staged
    struct Run { int lo, hi; bool staged; };
    std::vector<Run> runs;
    const long long w_end = (long long)smp0 + ns_alloc;
    if (!n_arr) { if (ns_max > 0) runs.push_back({0, ns_max, false}); }
    else {
        if (std::min(smp0, ns_max) > 0) runs.push_back({0, std::min(smp0, ns_max), false});
        for (long long lo = smp0; lo < w_end; lo += SB) runs.push_back({(int)lo, (int)std::min(lo + SB, w_end), true});
        if (w_end < ns_max) runs.push_back({(int)w_end, ns_max, false});
    }
    int max_chunks = 1;
    for (const Run &r : runs) max_chunks = std::max(max_chunks, (r.hi - r.lo + SP_CHUNK - 1) / SP_CHUNK);
    const size_t stage = A * (size_t)SB * 24;
    if ((n_arr && ctx->pc_sp_stage.ensure(stage * n_arr)) || ctx->pc_sp_part.ensure((size_t)max_chunks * A * 24) || ctx->pc_sp_run.ensure(A * 24) ||
        ctx->pc_sp_out.ensure(A * 24))
        FAIL(ctx, "device allocation failed (setpoints)");
    double *d_stage[3] = {nullptr, nullptr, nullptr};
    for (int a = 0, u = 0; a < 3; ++a)
        if (host[a]) d_stage[a] = ctx->pc_sp_stage.as<double>() + (size_t)(u++) * A * (size_t)SB * 3;
    // partials [chunk][S][N], running peaks and report [S][N]: values of v, values of a, samples of v, samples of a
    double *part_v = ctx->pc_sp_part.as<double>(), *part_a = part_v + (size_t)max_chunks * A;
    int *part_vs = (int *)(part_a + (size_t)max_chunks * A), *part_as = part_vs + (size_t)max_chunks * A;
    double *run_v = ctx->pc_sp_run.as<double>(), *run_a = run_v + A, *o_v = ctx->pc_sp_out.as<double>(), *o_a = o_v + A;
    int *run_vs = (int *)(run_a + A), *run_as = run_vs + A, *o_vs = (int *)(o_a + A), *o_as = o_vs + A;
    auto finish = [&](int chunks, int first, int last) {
        hipLaunchKernelGGL(pc::setpoint_finish_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, st, A, N, chunks, first, last, (const int *)q.d_kt,
                           (const double *)part_v, (const int *)part_vs, (const double *)part_a, (const int *)part_as, run_v, run_vs, run_a, run_as, o_v,
                           o_vs, o_a, o_as);
    };
    if (runs.empty()) finish(0, 1, 1);   // (every scene masked, no window)
    for (size_t r = 0; r < runs.size(); ++r) {
        const Run &run = runs[r];
        const int len = run.hi - run.lo, chunks = (len + SP_CHUNK - 1) / SP_CHUNK;
        hipLaunchKernelGGL(pc::setpoint_kernel, dim3((unsigned)((N + SP_TILE - 1) / SP_TILE), (unsigned)chunks, (unsigned)S), dim3(SP_CHUNK), 0, st, S, N,
                           KT_alloc, (const int *)q.d_kt, (const double *)q.d_hs, (const int *)q.d_ns, c.Ts, run.lo, run.hi, (const double *)q.dp,
                           (const double *)ctx->pc_M.as<double>(), (const double *)q.dv, (const double *)ctx->pc_Mv.as<double>(), (const double *)q.da,
                           (const double *)ctx->pc_Ma.as<double>(), run.staged ? d_stage[0] : nullptr, run.staged ? d_stage[1] : nullptr,
                           run.staged ? d_stage[2] : nullptr, SB, part_v, part_vs, part_a, part_as);
        finish(chunks, r == 0, r + 1 == runs.size());
        HIPCHK(ctx, hipGetLastError());
        if (!run.staged) continue;
        for (int a = 0; a < 3; ++a)   // rows of `len` samples out of the staging rows of SB, to their place in the rows of ns_alloc
            if (host[a] && len == ns_alloc && SB == ns_alloc)   // (the whole window in one pass: one contiguous block)
                HIPCHK(ctx, hipMemcpyAsync(host[a], d_stage[a], A * (size_t)ns_alloc * 24, hipMemcpyDeviceToHost, st));
            else if (host[a])
                HIPCHK(ctx, hipMemcpy2DAsync(host[a] + (size_t)(run.lo - smp0) * 3, (size_t)ns_alloc * 24, d_stage[a], (size_t)SB * 24, (size_t)len * 24, A,
                                             hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));   // (the next pass overwrites the staging arrays)
    }
    HIPCHK(ctx, hipGetLastError());
    if (t.v_peak) HIPCHK(ctx, hipMemcpyAsync(t.v_peak, o_v, A * 8, hipMemcpyDeviceToHost, st));
    if (t.a_peak) HIPCHK(ctx, hipMemcpyAsync(t.a_peak, o_a, A * 8, hipMemcpyDeviceToHost, st));
    if (t.v_peak_sample) HIPCHK(ctx, hipMemcpyAsync(t.v_peak_sample, o_vs, A * 4, hipMemcpyDeviceToHost, st));
    if (t.a_peak_sample) HIPCHK(ctx, hipMemcpyAsync(t.a_peak_sample, o_as, A * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    q.scalars_out(t.r_factor, t.h_scaled, t.n_samples);   // (what dmpc_postcheck reports)
    return 0;
}

// "the histories of this call are the resident ones of a split batch": dmpc_transition ran the scenes in parts on the child contexts and each
// part's histories stayed where it ran
static bool pc_split_resident(const dmpc_ctx *ctx, const PostcheckCall &c)
{
    const int parts = (int)ctx->split_at.size() - 1;
    return !c.pk && parts >= 2 && ctx->split_at.back() == c.S && ctx->hist_S == c.S && (int)ctx->children.size() >= parts - 1;
}
// A call through `one` (postcheck_one, clearance_one, setpoints_one) where its histories live: here -- or, the resident histories of a split
// batch, every part concurrently on the context that holds it (whose hist_S reads the part's scenes for the call), without host histories;
// part 0 on the calling thread.  The first failed child's message becomes the caller's.  (K_T_used == NULL: here, for its refusal.)
static int pc_run(dmpc_ctx *ctx, const PostcheckCall &c, int (*one)(dmpc_ctx *, const PostcheckCall &))
{
    if (!pc_split_resident(ctx, c) || !c.K_T_used) return one(ctx, c);
    const int parts = (int)ctx->split_at.size() - 1;
    std::vector<int> rc((size_t)parts, 0);
    auto run = [&](int i) {
        dmpc_ctx *ch = i ? ctx->children[(size_t)i - 1] : ctx;
        const int s0 = ctx->split_at[(size_t)i], sn = ctx->split_at[(size_t)i + 1] - s0;
        PostcheckCall part = c.scenes(s0, sn);
        part.pk = part.vk = part.ak = nullptr;
        const int keep = ch->hist_S;
        ch->hist_S = sn;
        rc[(size_t)i] = one(ch, part);
        ch->hist_S = keep;
    };
    std::vector<std::thread> th;
    for (int i = 1; i < parts; ++i) th.emplace_back(run, i);
    run(0);
    for (auto &t : th) t.join();
    for (int i = 1; i < parts; ++i)
        if (rc[(size_t)i]) FAIL(ctx, ctx->children[(size_t)i - 1]->err);
    return rc[0];
}

// The entries.  Every check of an entry's own -- the two "pk, vk, ak must be all given or all NULL" lines, which carry their entry's name,
// among them -- stands beside the entry, in the order the caller has always seen; "vk/ak missing" is pc_prepare's.

// the three report entries: a call without goals is refused as dmpc_postcheck refuses it, whichever entry it came through and wherever its histories live
static int report_run(dmpc_ctx *ctx, const PostcheckCall &c)
{
    if (!c.report.pf) FAIL(ctx, "dmpc_postcheck: bad arguments");
    return pc_run(ctx, c, postcheck_one);
}

extern "C" int dmpc_postcheck(dmpc_ctx *ctx, int S, int N, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                              const double *pk, const double *vk, const double *ak, const double *pf, double vmax, double amax, double Ts,
                              double *r_factor, double *h_scaled, int32_t *n_samples, double *min_dist,
                              int32_t *violation, double *totdist, double *traj_time, double *p_interp, int ns_alloc)
{
    if (!ctx) { g_err = "dmpc_postcheck: ctx is NULL"; return -1; }
    PostcheckCall c;
    c.S = S; c.N = N; c.N_cmd = N; c.KT_alloc = KT_alloc; c.K_T_used = K_T_used; c.scene_mask = scene_mask;
    c.pk = pk; c.vk = vk; c.ak = ak; c.vmax = vmax; c.amax = amax; c.Ts = Ts;
    PcReport &r = c.report;
    r.pf = pf; r.r_factor = r_factor; r.h_scaled = h_scaled; r.n_samples = n_samples; r.min_dist = min_dist; r.violation = violation;
    r.totdist = totdist; r.traj_time = traj_time; r.p_interp = p_interp; r.ns_alloc = ns_alloc;
    return report_run(ctx, c);
}

// the post-checks after a transition with uncommanded vehicles: collision_violation(solution) over the N_cmd trajectories (dmpc.cpp:2052-2086)
// as dmpc_postcheck, plus the commanded-against-static distances the reference leaves out
extern "C" int dmpc_postcheck_cmd(dmpc_ctx *ctx, int S, int N, int N_cmd, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                                  const double *pk, const double *vk, const double *ak, const double *pf, const double *po_static,
                                  double vmax, double amax, double Ts, double *r_factor, double *h_scaled, int32_t *n_samples,
                                  double *min_dist, int32_t *violation, double *totdist, double *traj_time, double *p_interp, int ns_alloc,
                                  double *min_dist_static, int32_t *violation_static)
{
    if (!ctx) { g_err = "dmpc_postcheck_cmd: ctx is NULL"; return -1; }
    if (check_cmd(ctx, "dmpc_postcheck_cmd", S, N, N_cmd)) return -1;
    if (N_cmd < N && !po_static) FAIL(ctx, "dmpc_postcheck_cmd: po_static is NULL with N_cmd < N");
    PostcheckCall c;
    c.S = S; c.N = N; c.N_cmd = N_cmd; c.KT_alloc = KT_alloc; c.K_T_used = K_T_used; c.scene_mask = scene_mask;
    c.pk = pk; c.vk = vk; c.ak = ak; c.vmax = vmax; c.amax = amax; c.Ts = Ts; c.po_static = po_static;
    PcReport &r = c.report;
    r.pf = pf; r.r_factor = r_factor; r.h_scaled = h_scaled; r.n_samples = n_samples; r.min_dist = min_dist; r.violation = violation;
    r.totdist = totdist; r.traj_time = traj_time; r.p_interp = p_interp; r.ns_alloc = ns_alloc;
    r.min_dist_other = min_dist_static; r.violation_other = violation_static;
    return report_run(ctx, c);
}

// the post-checks after dmpc_transition_scripted: the commanded-only outputs are dmpc_postcheck's; the scripted vehicles are splined on the
// commanded agents' knots and every (commanded agent, scripted vehicle) pair is examined at every 100 Hz sample
extern "C" int dmpc_postcheck_scripted(dmpc_ctx *ctx, int S, int N, int N_cmd, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                                       const double *pk, const double *vk, const double *ak, const double *pf, const double *path, int P,
                                       double vmax, double amax, double Ts, double *r_factor, double *h_scaled, int32_t *n_samples,
                                       double *min_dist, int32_t *violation, double *totdist, double *traj_time, double *p_interp, int ns_alloc,
                                       double *min_dist_scripted, int32_t *violation_scripted, double *p_scripted)
{
    if (!ctx) { g_err = "dmpc_postcheck_scripted: ctx is NULL"; return -1; }
    if (check_cmd(ctx, "dmpc_postcheck_scripted", S, N, N_cmd)) return -1;
    if (check_scripted(ctx, "dmpc_postcheck_scripted", S, N_cmd, N - N_cmd, P)) return -1;
    if (!path) FAIL(ctx, "dmpc_postcheck_scripted: path is NULL");
    if (p_scripted && ns_alloc < 1) FAIL(ctx, "dmpc_postcheck_scripted: ns_alloc must be positive with p_scripted");
    PostcheckCall c;
    c.S = S; c.N = N; c.N_cmd = N_cmd; c.KT_alloc = KT_alloc; c.K_T_used = K_T_used; c.scene_mask = scene_mask;
    c.pk = pk; c.vk = vk; c.ak = ak; c.vmax = vmax; c.amax = amax; c.Ts = Ts; c.path = path; c.P = P;
    PcReport &r = c.report;
    r.pf = pf; r.r_factor = r_factor; r.h_scaled = h_scaled; r.n_samples = n_samples; r.min_dist = min_dist; r.violation = violation;
    r.totdist = totdist; r.traj_time = traj_time; r.p_interp = p_interp; r.ns_alloc = ns_alloc;
    r.min_dist_other = min_dist_scripted; r.violation_other = violation_scripted; r.p_scripted = p_scripted;
    return report_run(ctx, c);
}

extern "C" int dmpc_postcheck_clearance(dmpc_ctx *ctx, int S, int N, int N_cmd, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                                        const double *pk, const double *vk, const double *ak, const double *po_static, const double *path, int P,
                                        double vmax, double amax, double Ts, double reach, double *clear_dist, int32_t *clear_partner,
                                        int32_t *clear_sample)
{
    if (!ctx) { g_err = "dmpc_postcheck_clearance: ctx is NULL"; return -1; }
    if (check_cmd(ctx, "dmpc_postcheck_clearance", S, N, N_cmd)) return -1;
    if (po_static && path) FAIL(ctx, "dmpc_postcheck_clearance: po_static and path exclude each other (static vehicles rest, scripted ones move)");
    if (N_cmd < N && !po_static && !path) FAIL(ctx, "dmpc_postcheck_clearance: N_cmd < N needs po_static or path");
    if (!(reach > 0)) FAIL(ctx, "dmpc_postcheck_clearance: reach must be > 0 (+inf: every slot exact)");
    if ((pk || vk || ak) && !(pk && vk && ak)) FAIL(ctx, "dmpc_postcheck_clearance: pk, vk, ak must be all given or all NULL");
    if (path && P < 1) FAIL(ctx, "dmpc_postcheck_clearance: P must be >= 1 (every path has at least its start)");
    PostcheckCall c;
    c.S = S; c.N = N; c.N_cmd = N_cmd; c.KT_alloc = KT_alloc; c.K_T_used = K_T_used; c.scene_mask = scene_mask;
    c.pk = pk; c.vk = vk; c.ak = ak; c.vmax = vmax; c.amax = amax; c.Ts = Ts; c.po_static = po_static; c.path = path; c.P = P;
    PcClearance &l = c.clearance;
    l.reach = reach; l.dist = clear_dist; l.partner = clear_partner; l.sample = clear_sample;
    return pc_run(ctx, c, clearance_one);
}

extern "C" int dmpc_postcheck_setpoints(dmpc_ctx *ctx, int S, int N, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                                        const double *pk, const double *vk, const double *ak, double vmax, double amax, double Ts, int smp0,
                                        int ns_alloc, double *p_sp, double *v_sp, double *a_sp, double *v_peak, int32_t *v_peak_sample,
                                        double *a_peak, int32_t *a_peak_sample, double *r_factor, double *h_scaled, int32_t *n_samples)
{
    if (!ctx) { g_err = "dmpc_postcheck_setpoints: ctx is NULL"; return -1; }
    if (smp0 < 0) FAIL(ctx, "dmpc_postcheck_setpoints: smp0 must be >= 0 (the first sample of the window)");
    if (ns_alloc < 0) FAIL(ctx, "dmpc_postcheck_setpoints: ns_alloc must be >= 0");
    if (ns_alloc == 0 && (p_sp || v_sp || a_sp)) FAIL(ctx, "dmpc_postcheck_setpoints: a setpoint array needs ns_alloc > 0");
    if (ns_alloc > 0 && !p_sp && !v_sp && !a_sp) FAIL(ctx, "dmpc_postcheck_setpoints: ns_alloc > 0 needs p_sp, v_sp or a_sp (the report alone: ns_alloc = 0)");
    if ((pk || vk || ak) && !(pk && vk && ak)) FAIL(ctx, "dmpc_postcheck_setpoints: pk, vk, ak must be all given or all NULL");
    if ((long long)smp0 + ns_alloc > 0x7fff0000LL) FAIL(ctx, "dmpc_postcheck_setpoints: smp0 + ns_alloc overflows the sample index");
    PostcheckCall c;
    c.S = S; c.N = N; c.N_cmd = N; c.KT_alloc = KT_alloc; c.K_T_used = K_T_used; c.scene_mask = scene_mask;
    c.pk = pk; c.vk = vk; c.ak = ak; c.vmax = vmax; c.amax = amax; c.Ts = Ts;
    PcSetpoints &t = c.setpoints;
    t.smp0 = smp0; t.ns_alloc = ns_alloc; t.p_sp = p_sp; t.v_sp = v_sp; t.a_sp = a_sp;
    t.v_peak = v_peak; t.v_peak_sample = v_peak_sample; t.a_peak = a_peak; t.a_peak_sample = a_peak_sample;
    t.r_factor = r_factor; t.h_scaled = h_scaled; t.n_samples = n_samples;
    return pc_run(ctx, c, setpoints_one);
}
