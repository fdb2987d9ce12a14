// dmpc_step.hip -- the single MPC step (host code only; included by dmpc_api.hip behind dmpc_launch.hip): the pieces every caller of launch_step
// shares -- the scratch of a step, the StepIO of that scratch, the mixed-precision rule -- the device-pointer entries and their one body, the
// record of a host-pointer call with its stage / run / fetch path, and the host-pointer entries.  The closed loops (dmpc_transition.hip) and the
// group's and the sharded step (dmpc_multigpu.hip) are built on the same pieces.

// uncommanded vehicles: 1 <= N_cmd <= N (the shared argument check of the *_cmd entries)
static int check_cmd(dmpc_ctx *ctx, const char *entry, int S, int N, int N_cmd)
{
    if (S < 1 || N < 1) FAIL(ctx, std::string(entry) + ": S and N must be >= 1");
    if (N_cmd < 1 || N_cmd > N) FAIL(ctx, std::string(entry) + ": N_cmd must be in 1 .. N (commanded agents first, uncommanded vehicles behind them)");
    return 0;
}

static int ensure_step_scratch(dmpc_ctx *ctx, size_t agents_table, size_t agents_solved)
{
    int rc = 0;
    ctx->end.valid = false;   // the end of the last flight stands in this scratch (dmpc_start.hip); transition_one sets it again
    rc |= ctx->rows.ensure(agents_table * N3 * 8);
    rc |= ctx->lT.ensure(agents_table * N3 * 8);
    rc |= ctx->xp.ensure(agents_solved * 24);
    rc |= ctx->xv.ensure(agents_solved * 24);
    rc |= ctx->xa.ensure(agents_solved * 24);
    rc |= ctx->pf.ensure(agents_solved * 24);
    rc |= ctx->pout.ensure(agents_solved * N3 * 8);
    rc |= ctx->vout.ensure(agents_solved * N3 * 8);
    rc |= ctx->aout.ensure(agents_solved * N3 * 8);
    rc |= ctx->status.ensure(agents_solved * 4);
    rc |= ctx->info.ensure(agents_solved * 32);
    if (rc) FAIL(ctx, "device allocation failed");
    return 0;
}

// the step that reads and writes that scratch: table, states and goals in, predictions, status and info out (packed: [S][c_count] agents)
static StepIO scratch_io(dmpc_ctx *ctx)
{
    StepIO io;
    io.lT = ctx->lT.as<double>(); io.x_p = ctx->xp.as<double>(); io.x_v = ctx->xv.as<double>(); io.x_a = ctx->xa.as<double>(); io.pf = ctx->pf.as<double>();
    io.p_out = ctx->pout.as<double>(); io.v_out = ctx->vout.as<double>(); io.a_out = ctx->aout.as<double>();
    io.status = ctx->status.as<int32_t>(); io.info = ctx->info.as<int32_t>();
    return io;
}

// mixed precision: fp32 copy of a table (n doubles) for the scan
static int table_f32(dmpc_ctx *ctx, const double *src, DevBuf &dst, size_t n, hipStream_t st)
{
    if (dst.ensure(n * 4)) FAIL(ctx, "device allocation failed (fp32 table)");
    hipLaunchKernelGGL(table_to_f32_kernel, dim3(grid_1d(n, 4096)), dim3(256), 0, st, n, src, dst.as<float>());
    return 0;
}
// the rule of a single step: the table io.lT of n entries stays fp64 and a mixed-precision context's scan reads an fp32 copy made here, on the
// stream, into ctx->lTf (half the bytes of the O(N) part; all columns, static ones included).  The closed loops keep copies of their own.
static int mixed_table(dmpc_ctx *ctx, StepIO &io, size_t n, hipStream_t st)
{
    if (!(ctx->precision & DMPC_PREC_MIXED)) return 0;
    if (table_f32(ctx, io.lT, ctx->lTf, n, st)) return -1;
    io.lTf = ctx->lTf.as<float>();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// device-pointer entry points
// ---------------------------------------------------------------------------------------------

// the StepIO of a caller's device arrays, in the order in which the device-pointer entries take them
static StepIO caller_io(const double *lT, const double *x_p, const double *x_v, const double *x_a, const double *pf, double *p_out, double *v_out,
                        double *a_out, double *lT_next, int32_t *status, int32_t *info)
{
    StepIO io;
    io.lT = lT; io.x_p = x_p; io.x_v = x_v; io.x_a = x_a; io.pf = pf;
    io.p_out = p_out; io.v_out = v_out; io.a_out = a_out; io.lT_next = lT_next; io.status = status; io.info = info;
    return io;
}

// the body of both: `who` has checked its shape; the table behind io.lT has table_entries doubles
static int step_device(dmpc_ctx *ctx, const char *who, const StepShape &sh, size_t table_entries, const StepIO &io_in, void *stream)
{
    StepIO io = io_in;
    if (!io.lT || !io.x_p || !io.x_v || !io.x_a || !io.pf || !io.p_out || !io.v_out || !io.a_out || !io.status) FAIL(ctx, std::string(who) + ": NULL pointer");
    if (ctx->grp) FAIL(ctx, std::string(who) + ": device pointers belong to ONE GPU; a DMPC_DEVICE_ALL context drives several (use the host-pointer entry points)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (mixed_table(ctx, io, table_entries, (hipStream_t)stream)) return -1;
    return launch_step(ctx, sh, io, (hipStream_t)stream);
}

extern "C" int dmpc_step_device(dmpc_ctx *ctx, int S, int G, int C, int g_local, const double *lT, const double *x_p,
                                const double *x_v, const double *x_a, const double *pf, double *p_out, double *v_out,
                                double *a_out, double *lT_next, int32_t *status, int32_t *info, void *stream)
{
    if (!ctx) { g_err = "dmpc_step_device: ctx is NULL"; return -1; }
    if (S < 1 || G < 1 || C < 1 || g_local < 0 || g_local >= G) FAIL(ctx, "dmpc_step_device: bad S/G/C/g_local");
    return step_device(ctx, "dmpc_step_device", {S, G, C, g_local, /*c_first*/ 0, /*c_count*/ C}, (size_t)G * S * N3 * C,
                       caller_io(lT, x_p, x_v, x_a, pf, p_out, v_out, a_out, lT_next, status, info), stream);
}

extern "C" int dmpc_step_device_cmd(dmpc_ctx *ctx, int S, int N, int N_cmd, const double *lT, const double *x_p, const double *x_v,
                                    const double *x_a, const double *pf, double *p_out, double *v_out, double *a_out, double *lT_next,
                                    int32_t *status, int32_t *info, void *stream)
{
    if (!ctx) { g_err = "dmpc_step_device_cmd: ctx is NULL"; return -1; }
    if (check_cmd(ctx, "dmpc_step_device_cmd", S, N, N_cmd)) return -1;
    return step_device(ctx, "dmpc_step_device_cmd", {S, /*G*/ 1, /*C*/ N, /*g_local*/ 0, /*c_first*/ 0, /*c_count*/ N_cmd}, (size_t)S * N3 * N,
                       caller_io(lT, x_p, x_v, x_a, pf, p_out, v_out, a_out, lT_next, status, info), stream);
}

extern "C" int dmpc_table_from_rows_device(dmpc_ctx *ctx, int S, int G, int C, const double *rows, double *lT, void *stream)
{
    if (!ctx) { g_err = "dmpc_table_from_rows_device: ctx is NULL"; return -1; }
    if (S < 1 || G < 1 || C < 1 || !rows || !lT) FAIL(ctx, "dmpc_table_from_rows_device: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(table_from_rows_kernel, dim3(grid_1d((size_t)S * G * C * N3, 4096)), dim3(256), 0, (hipStream_t)stream, S, G, C, rows, lT);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

extern "C" int dmpc_advance_device(dmpc_ctx *ctx, int count, const double *p_out, const double *v_out, const double *a_out,
                                   const int32_t *status, double *x_p, double *x_v, double *x_a, void *stream)
{
    if (!ctx) { g_err = "dmpc_advance_device: ctx is NULL"; return -1; }
    if (count < 1 || !p_out || !v_out || !a_out || !status || !x_p || !x_v || !x_a) FAIL(ctx, "dmpc_advance_device: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(advance_kernel, dim3((unsigned)((count * 3 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, count, p_out, v_out, a_out, (const int *)status, x_p, x_v, x_a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// host-pointer entry points
// ---------------------------------------------------------------------------------------------

// one call of a host-pointer step entry: N_cmd agents of every scene, from column `first` of the scene's table on, solved against its N vehicles.
// (The entries fill it with braces: the fields down to `info` stand in the order of the entries' own arguments, and have to stay in it.)
struct StepCall {
    int S, N, N_cmd;
    const double *l;                      // [S][N][3K] predictions of every vehicle, as rows
    const double *x_p, *x_v, *x_a, *pf;   // [S][N_cmd][3]
    double *p_out, *v_out, *a_out;        // [S][N_cmd][3K]
    int32_t *status, *info;               // [S][N_cmd], [S][N_cmd][8] or null
    int first = 0;   // column of the scene's table [3K][N] that the call's first agent has
    int pitch = 0;   // a slice: agents per scene of the arrays it was cut from and still points into (0: the arrays hold the call's agents alone)
    // the same call for agents [lo, lo + cnt) of every scene: the one place that knows each array's stride per agent
    StepCall agents(int lo, int cnt) const {
        auto at = [](auto *p, size_t off) { return p ? p + off : nullptr; };
        StepCall c = *this; c.N_cmd = cnt; c.first = first + lo; c.pitch = pitch ? pitch : N_cmd;
        c.x_p = at(x_p, (size_t)lo * 3); c.x_v = at(x_v, (size_t)lo * 3); c.x_a = at(x_a, (size_t)lo * 3); c.pf = at(pf, (size_t)lo * 3);
        c.p_out = at(p_out, (size_t)lo * N3); c.v_out = at(v_out, (size_t)lo * N3); c.a_out = at(a_out, (size_t)lo * N3);
        c.status = at(status, (size_t)lo); c.info = at(info, (size_t)lo * 8);
        return c;
    }
};

// `per` bytes per agent between an array of the call and its packed copy in the context's scratch: one copy; a slice: one strided copy, a row per scene
static int copy_agents(dmpc_ctx *ctx, const StepCall &c, void *dst, const void *src, size_t per, hipMemcpyKind kind, hipStream_t st)
{
    const size_t row = (size_t)c.N_cmd * per, pitch = (size_t)c.pitch * per;
    const bool up = kind == hipMemcpyHostToDevice;
    if (!c.pitch) HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)c.S * row, kind, st));
    else HIPCHK(ctx, hipMemcpy2DAsync(dst, up ? row : pitch, src, up ? pitch : row, row, (size_t)c.S, kind, st));
    return 0;
}
// the agents' states and goals up, the outputs down (and wait for them)
static int upload_states(dmpc_ctx *ctx, const StepCall &c, hipStream_t st)
{
    const double *src[4] = {c.x_p, c.x_v, c.x_a, c.pf};
    void *dst[4] = {ctx->xp.p, ctx->xv.p, ctx->xa.p, ctx->pf.p};
    for (int u = 0; u < 4; ++u)
        if (copy_agents(ctx, c, dst[u], src[u], 24, hipMemcpyHostToDevice, st)) return -1;
    return 0;
}
static int fetch_step(dmpc_ctx *ctx, const StepCall &c, hipStream_t st)
{
    double *out[3] = {c.p_out, c.v_out, c.a_out};
    const void *dev[3] = {ctx->pout.p, ctx->vout.p, ctx->aout.p};
    for (int u = 0; u < 3; ++u)
        if (copy_agents(ctx, c, out[u], dev[u], N3 * 8, hipMemcpyDeviceToHost, st)) return -1;
    if (copy_agents(ctx, c, c.status, ctx->status.p, 4, hipMemcpyDeviceToHost, st)) return -1;
    if (c.info && copy_agents(ctx, c, c.info, ctx->info.p, 32, hipMemcpyDeviceToHost, st)) return -1;
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// stage on one GPU, first part: the scratch, the rows and the agents' states and goals up, the table [S][3K][N] from the rows
static int upload_step(dmpc_ctx *ctx, const StepCall &c, hipStream_t st)
{
    const size_t T = (size_t)c.S * c.N, A = (size_t)c.S * c.N_cmd;   // table rows, agents solved
    if (ensure_step_scratch(ctx, T, A)) return -1;
    HIPCHK(ctx, hipMemcpyAsync(ctx->rows.p, c.l, T * N3 * 8, hipMemcpyHostToDevice, st));
    if (upload_states(ctx, c, st)) return -1;
    return dmpc_table_from_rows_device(ctx, c.S, 1, c.N, ctx->rows.as<double>(), ctx->lT.as<double>(), st);
}
// stage: that, and the step of the context's scratch in io, with the fp32 copy of the table when the context is mixed
static int stage_step(dmpc_ctx *ctx, const StepCall &c, StepIO &io, hipStream_t st)
{
    if (upload_step(ctx, c, st)) return -1;
    io = scratch_io(ctx);
    return mixed_table(ctx, io, (size_t)c.S * N3 * c.N, st);
}

static int group_step_batch(dmpc_ctx *root, const StepCall &c);   // (dmpc_multigpu.hip, as group_transition: a group's rank stages its own, padded table)

// one MPC step of a call on this context's device: stage, run, fetch
static int step_batch_one(dmpc_ctx *ctx, const StepCall &c)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StepIO io;
    if (stage_step(ctx, c, io, st)) return -1;
    if (launch_step(ctx, {c.S, /*G*/ 1, /*C*/ c.N, /*g_local*/ 0, c.first, c.N_cmd}, io, st)) return -1;
    return fetch_step(ctx, c, st);
}

extern "C" int dmpc_step_batch(dmpc_ctx *ctx, int S, int N, const double *l, const double *x_p, const double *x_v,
                               const double *x_a, const double *pf, double *p_out, double *v_out, double *a_out,
                               int32_t *status, int32_t *info)
{
    if (!ctx) { g_err = "dmpc_step_batch: ctx is NULL"; return -1; }
    if (S < 1 || N < 1) FAIL(ctx, "dmpc_step_batch: S and N must be >= 1");
    if (!l || !x_p || !x_v || !x_a || !pf || !p_out || !v_out || !a_out || !status) FAIL(ctx, "dmpc_step_batch: NULL pointer");
    const StepCall c{S, N, N, l, x_p, x_v, x_a, pf, p_out, v_out, a_out, status, info};
    return (ctx->grp && N >= ctx->grp->G) ? group_step_batch(ctx, c) : step_batch_one(ctx, c);
}

// DMPC::solveParallelDMPCv2's cluster_solvev2 (dmpc.cpp:1792-1841) for the N_cmd = _pf.cols() commanded vehicles of N = _po.cols() (:1572-1573)
extern "C" int dmpc_step_batch_cmd(dmpc_ctx *ctx, int S, int N, int N_cmd, const double *l, const double *x_p, const double *x_v,
                                   const double *x_a, const double *pf, double *p_out, double *v_out, double *a_out,
                                   int32_t *status, int32_t *info)
{
    if (!ctx) { g_err = "dmpc_step_batch_cmd: ctx is NULL"; return -1; }
    if (check_cmd(ctx, "dmpc_step_batch_cmd", S, N, N_cmd)) return -1;
    if (!l || !x_p || !x_v || !x_a || !pf || !p_out || !v_out || !a_out || !status) FAIL(ctx, "dmpc_step_batch_cmd: NULL pointer");
    if (N_cmd == N) return dmpc_step_batch(ctx, S, N, l, x_p, x_v, x_a, pf, p_out, v_out, a_out, status, info);
    return step_batch_one(ctx, {S, N, N_cmd, l, x_p, x_v, x_a, pf, p_out, v_out, a_out, status, info});   // (a DMPC_DEVICE_ALL context: its first GPU)
}

// one scene, one agent: column n of the table, the arrays are that agent's
extern "C" int dmpc_solve_one(dmpc_ctx *ctx, int N, int n, const double *l, const double *po, const double *vo,
                              const double *ao, const double *pf, double *p, double *v, double *a, int32_t *status,
                              int32_t *info)
{
    if (!ctx) { g_err = "dmpc_solve_one: ctx is NULL"; return -1; }
    if (N < 1 || n < 0 || n >= N) FAIL(ctx, "dmpc_solve_one: agent index out of range");
    if (!l || !po || !vo || !ao || !pf || !p || !v || !a || !status) FAIL(ctx, "dmpc_solve_one: NULL pointer");
    StepCall c{/*S*/ 1, N, /*N_cmd*/ 1, l, po, vo, ao, pf, p, v, a, status, info};
    c.first = n;
    return step_batch_one(ctx, c);
}

// the scan + collision rows of ONE agent on one wave, with the step's own parameter block and scan kernel: staged, launched, header and rows
// fetched.  What is this runner's: the exact row capacity and the order of the rows.  `f32_table`: a mixed-precision context's scan reads the
// fp32 copy of the table and runs its float instantiation, as a step's does (mixed_table; an fp64 context stays on the fp64 table either way);
// `prune`: the step's exact pruning instead of every row the reference builds.
struct ScanRowsOne {
    int hdr[8];
    int nrmax = 0;
    bool soft = false;
    std::vector<double> buf;     // the agent's slice of the row scratch: xi [nrmax][3], rhs, then (soft) slack coefficient, cost term, lower bound
    std::vector<int> kbuf, idx;  // constrained step of a row (0-based); the rows in the reference's order
};
static int scan_rows_one(dmpc_ctx *ctx, int N, int n, const double *l, const double *po, const double *vo, bool f32_table, bool prune,
                         bool fetch_rows, ScanRowsOne &R)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const dmpc_params &p = ctx->prm;
    const bool soft = R.soft = variant_soft(p.variant);
    const double zero3[3] = {0, 0, 0};   // (the scan reads no acceleration and no goal)
    StepCall c{};   // (no outputs: the rows come back below)
    c.S = 1; c.N = N; c.N_cmd = 1; c.l = l; c.x_p = po; c.x_v = vo; c.x_a = c.pf = zero3;
    if (upload_step(ctx, c, st)) return -1;
    StepIO io = scratch_io(ctx);
    if (f32_table && mixed_table(ctx, io, (size_t)N3 * N, st)) return -1;
    // the step's own parameter block and scan kernel; what is this entry's: the exact row capacity, one wave
    StepParams P;
    fill_constants(ctx, P);
    P.S = 1; P.G = 1; P.C = N; P.g_local = 0; P.c_first = n; P.c_count = 1;
    const long want = (p.variant == DMPC_VAR_HARD ? (long)K : (p.variant == DMPC_VAR_ALL3 ? 3L : 1L)) * (N > 1 ? N - 1 : 1);
    P.nrmax = R.nrmax = (int)((want + 1) & ~1L);   // the exact worst case: nothing is truncated here
    P.lT = io.lTf ? (const double *)io.lTf : io.lT; P.x_p = io.x_p; P.x_v = io.x_v; P.x_a = io.x_a; P.pf = io.pf;
    P.status = io.status; P.no_prune = prune ? 0 : 1; P.qcap = QMAX; P.qover_bit = ST_CAPACITY;
    const size_t per = (size_t)P.nrmax * (soft ? 7 : 4);
    if (ctx->rowbuf.ensure(per * 8) || ctx->rowkc.ensure((size_t)P.nrmax * 4) || ctx->hdr.ensure(32)) FAIL(ctx, "device allocation failed");
    P.rowbuf = ctx->rowbuf.as<double>(); P.rowkc = ctx->rowkc.as<int>(); P.hdr = ctx->hdr.as<int>();
    P.lds_per_wave = (int)scan_lds_bytes();
    launch_params_kernel(scan_kernel(soft, io.lTf != nullptr, /*fast_exit*/ false, p.order == 4), dim3(1), dim3(64), scan_lds_bytes(), st, P);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(R.hdr, ctx->hdr.p, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const int nr = R.hdr[0];
    if (nr > 0 && fetch_rows) {
        R.buf.resize(per);
        R.kbuf.resize(P.nrmax);
        HIPCHK(ctx, hipMemcpy(R.buf.data(), ctx->rowbuf.p, per * 8, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(R.kbuf.data(), ctx->rowkc.p, (size_t)P.nrmax * 4, hipMemcpyDeviceToHost));
        // reference order: horizon step major, neighbour index minor (the hard variant's rows are emitted
        // neighbour-chunk major on the device): stable sort by constrained step
        R.idx.resize(nr);
        for (int i = 0; i < nr; ++i) R.idx[i] = i;
        if (p.variant == DMPC_VAR_HARD || p.variant == DMPC_VAR_ALL3)
            std::stable_sort(R.idx.begin(), R.idx.end(), [&](int a_, int b_) { return R.kbuf[a_] < R.kbuf[b_]; });
    }
    return 0;
}

// a5/a6 standalone: scan + collision rows of ONE agent in the reference's row order
// (CheckCollSoftDMPC.m + CollConstrSoftDMPC.m and variants), always on the fp64 table, without pruning.  Host pointers.
extern "C" int dmpc_rows_one(dmpc_ctx *ctx, int N, int n, const double *l, const double *po, const double *vo,
                             int max_rows, double *xi, double *rhs, double *slack_coef, int32_t *kc, int32_t *nrows,
                             int32_t *viol_k, int32_t *status)
{
    if (!ctx) { g_err = "dmpc_rows_one: ctx is NULL"; return -1; }
    if (N < 1 || n < 0 || n >= N || max_rows < 0) FAIL(ctx, "dmpc_rows_one: bad arguments");
    if (!l || !po || !vo || !nrows || !viol_k || !status) FAIL(ctx, "dmpc_rows_one: NULL pointer");
    ScanRowsOne R;
    const bool rows = max_rows > 0 && xi && rhs && kc;
    if (scan_rows_one(ctx, N, n, l, po, vo, /*f32_table*/ false, /*prune*/ false, rows, R)) return -1;
    *nrows = R.hdr[1]; *viol_k = R.hdr[2]; *status = R.hdr[3] & (DMPC_ST_COLL | DMPC_ST_CAPACITY);
    const int cnt = R.hdr[0] < max_rows ? R.hdr[0] : max_rows;
    for (int i = 0; rows && i < cnt; ++i) {
        const int j = R.idx[i];
        xi[3 * i] = R.buf[3 * j]; xi[3 * i + 1] = R.buf[3 * j + 1]; xi[3 * i + 2] = R.buf[3 * j + 2];
        rhs[i] = R.buf[(size_t)3 * R.nrmax + j];
        if (slack_coef) slack_coef[i] = R.soft ? R.buf[(size_t)4 * R.nrmax + j] : 0.0;
        kc[i] = R.kbuf[j] + 1;   // 1-based like the reference's k_ctr
    }
    return 0;
}

// development (include/dmpc_hip_dev.h): the scan's own records of ONE agent as a step of this context forms them -- a mixed-precision context
// on the fp32 copy of the table with the float instantiation of the scan and the row builder -- with or without the exact pruning
extern "C" int dmpc_debug_scan_rows(dmpc_ctx *ctx, int N, int n, const double *l, const double *po, const double *vo, int prune,
                                    int max_rows, int32_t *hdr, double *xi, double *rhs, int32_t *kc, double *slack_coef,
                                    double *slack_term, double *slack_lb)
{
    if (!ctx) { g_err = "dmpc_debug_scan_rows: ctx is NULL"; return -1; }
    if (N < 1 || n < 0 || n >= N || max_rows < 0) FAIL(ctx, "dmpc_debug_scan_rows: bad arguments");
    if (!l || !po || !vo || !hdr) FAIL(ctx, "dmpc_debug_scan_rows: NULL pointer");
    if (max_rows > 0 && (!xi || !rhs || !kc || !slack_coef || !slack_term || !slack_lb)) FAIL(ctx, "dmpc_debug_scan_rows: NULL row array");
    if (ctx->prm.order == 4) FAIL(ctx, "dmpc_debug_scan_rows: order 2 only (the context's super-ellipsoid is of order 4)");
    if (ctx->prm.variant == DMPC_VAR_SCP) FAIL(ctx, "dmpc_debug_scan_rows: solveDMPC (DMPC_VAR_SCP) builds its rows inside its own kernel, pass by pass");
    ScanRowsOne R;
    if (scan_rows_one(ctx, N, n, l, po, vo, /*f32_table*/ true, prune != 0, max_rows > 0, R)) return -1;
    for (int i = 0; i < 8; ++i) hdr[i] = R.hdr[i];
    const int cnt = R.hdr[0] < max_rows ? R.hdr[0] : max_rows;
    const size_t m = (size_t)R.nrmax;
    for (int i = 0; i < cnt; ++i) {
        const int j = R.idx[i];
        xi[3 * i] = R.buf[3 * j]; xi[3 * i + 1] = R.buf[3 * j + 1]; xi[3 * i + 2] = R.buf[3 * j + 2];
        rhs[i] = R.buf[3 * m + j];
        kc[i] = R.kbuf[j] + 1;   // 1-based like the reference's k_ctr
        slack_coef[i] = R.soft ? R.buf[4 * m + j] : 0.0;
        slack_term[i] = R.soft ? R.buf[5 * m + j] : 0.0;
        slack_lb[i] = R.soft ? R.buf[6 * m + j] : 0.0;
    }
    return 0;
}

extern "C" int dmpc_init_batch(dmpc_ctx *ctx, int S, int N, const double *po, const double *pf, double *l_out,
                               double *v_out, double *a_out)
{
    if (!ctx) { g_err = "dmpc_init_batch: ctx is NULL"; return -1; }
    if (S < 1 || N < 1 || !po || !pf || !l_out) FAIL(ctx, "dmpc_init_batch: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t A = (size_t)S * N;
    if (ctx->po.ensure(A * 24) || ctx->pf.ensure(A * 24) || ctx->rows.ensure(A * N3 * 8)) FAIL(ctx, "device allocation failed");
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->po.p, po, A * 24, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->pf.p, pf, A * 24, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(init_rows_kernel, dim3((unsigned)((A * N3 + 255) / 256)), dim3(256), 0, st, (int)A, ctx->prm.h,
                       ctx->po.as<double>(), ctx->pf.as<double>(), ctx->rows.as<double>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(l_out, ctx->rows.p, A * N3 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (v_out) memset(v_out, 0, A * N3 * 8);   // initDMPC.m:11-12: v = a = zeros(3,k_hor)
    if (a_out) memset(a_out, 0, A * N3 * 8);
    return 0;
}
