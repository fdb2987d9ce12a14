// dmpc_start.hip -- start in motion (included by dmpc_api.hip behind dmpc_disturb.hip, in front of dmpc_transition.hip): a flight whose column 0
// is a given or carried state and plan instead of initDMPC.  No reference counterpart (the reference flies one leg from rest).  The rule is pinned
// in include/dmpc_hip.h.  Here: the braking plan -- one function, compiled for the device (start_plan_kernel) and the host (dmpc_start_plan) --,
// the gather of a flight's end out of the step scratch (end_gather_kernel), the scripted fill with a column offset per scene, what
// transition_one does on column 0 of a flight with a start (StartDev), and the four entries.

// the braking plan of one agent and axis: entries 0 .. K-1 of p, v, a at stride 3 (any of them null)
__host__ __device__ inline void brake_plan_axis(double h, double alim, double xp, double xv, double xa, double *p, double *v, double *a)
{
#pragma clang fp contract(off)   // every operation rounded on its own: the host, the device and the numpy restatement agree bit for bit
    const double half_hh = (0.5 * h) * h;
    double pk = xp, vk = xv, ak = xa;
    for (int kk = 0; kk < K; ++kk) {
        if (kk) {
            ak = fmin(fmax(-vk / h, -alim), alim);
            const double pn = (pk + h * vk) + half_hh * ak;
            vk = vk + h * ak;
            pk = pn;
        }
        if (p) p[3 * kk] = pk;
        if (v) v[3 * kk] = vk;
        if (a) a[3 * kk] = ak;
    }
}

namespace dmpc {

// one thread per (agent, axis), K - 1 dependent steps; x_p, x_v, x_a [n][3]; p, v, a rows [n][3K] (any of them null)
__global__ __launch_bounds__(256) void start_plan_kernel(int n, double h, double alim, const double *__restrict__ x_p, const double *__restrict__ x_v,
                                                         const double *__restrict__ x_a, double *__restrict__ p, double *__restrict__ v,
                                                         double *__restrict__ a)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * 3) return;
    const size_t ag = t / 3, d = t - ag * 3, o = ag * N3 + d;
    brake_plan_axis(h, alim, x_p[t], x_v[t], x_a[t], p ? p + o : nullptr, v ? v + o : nullptr, a ? a + o : nullptr);
}

// The end of a flight out of the step scratch.  Destination scene s takes source scene src[2 s], which ended on column e = src[2 s + 1]:
//   x_p, x_v, x_a [S][N_cmd][3]   the source's states (the steps behind a scene's end skip it: they are column e's)
//   plan_p [S][N_cmd][3K]         the commanded columns of the table step e wrote -- tab[e & 1], [S_src][3K][N] -- as rows
//   plan_v, plan_a                the rows of the output set step e wrote: vset[e & 1], aset[e & 1] [S_src][N_cmd][3K] (without hold both sets are
//                                 the same rows); zero_e0: a source that ended on column 0 has v = a = 0, nothing wrote its rows
// t enumerates the destination scene and, inside it, [j][c] for the table (the reads run along the agent index, as cmd_cols_from_rows_kernel's
// writes do) and the row order itself for everything else.  Destinations never alias sources.
__global__ __launch_bounds__(256) void end_gather_kernel(int S, int N, int N_cmd, int zero_e0, const int *__restrict__ src, const double *__restrict__ sx_p,
                                                         const double *__restrict__ sx_v, const double *__restrict__ sx_a, const double *__restrict__ tab0,
                                                         const double *__restrict__ tab1, const double *__restrict__ v0, const double *__restrict__ v1,
                                                         const double *__restrict__ a0, const double *__restrict__ a1, double *__restrict__ x_p,
                                                         double *__restrict__ x_v, double *__restrict__ x_a, double *__restrict__ plan_p,
                                                         double *__restrict__ plan_v, double *__restrict__ plan_a)
{
    const size_t per = (size_t)N_cmd * N3, total = (size_t)S * per, st3 = (size_t)N_cmd * 3;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t s = t / per, r = t - s * per;
        const size_t q = (size_t)src[2 * s];
        const int e = src[2 * s + 1];
        const int c = (int)(r % N_cmd), j = (int)(r / N_cmd);
        plan_p[(s * N_cmd + c) * N3 + j] = (e & 1 ? tab1 : tab0)[(q * N3 + j) * N + c];
        const bool zero = zero_e0 && e == 0;
        plan_v[t] = zero ? 0.0 : (e & 1 ? v1 : v0)[q * per + r];
        plan_a[t] = zero ? 0.0 : (e & 1 ? a1 : a0)[q * per + r];
        if (r < st3) { x_p[s * st3 + r] = sx_p[q * st3 + r]; x_v[s * st3 + r] = sx_v[q * st3 + r]; x_a[s * st3 + r] = sx_a[q * st3 + r]; }
    }
}

// scripted_cols_kernel for a flight with a start: the window of scene s starts at column col0[s] + k - 1
__global__ void scripted_cols_from_kernel(int S, int N, int N_cmd, int P, int k, const int *__restrict__ col0, const double *__restrict__ path,
                                          double *__restrict__ lT)
{
    const int M = N - N_cmd;
    const size_t total = (size_t)S * N3 * M;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(t % M);   // t enumerates the destination: [s][j][c - N_cmd]
        const size_t u = t / M;
        const int j = (int)(u % N3), s = (int)(u / N3);
        const long col = (long)col0[s] + k - 1 + j / 3;
        const size_t smp = (size_t)(col < (long)P - 1 ? col : (long)P - 1);
        lT[((size_t)s * N3 + j) * N + N_cmd + m] = path[(((size_t)s * M + m) * P + smp) * 3 + j % 3];
    }
}

}  // namespace dmpc

// ---------------------------------------------------------------------------------------------
// host: the start of a call, the gather
// ---------------------------------------------------------------------------------------------

// the start of one call of a transition entry, as transition_any took it from the context (host form: pointers into the context's copies)
struct Start {
    bool on = false, from_end = false;
    int col0 = 0;
    const double *vo = nullptr, *ao = nullptr, *plan_p = nullptr, *plan_v = nullptr, *plan_a = nullptr;
    explicit operator bool() const { return on; }
};

static bool scene_ended_solved(int32_t status) { return (status & DMPC_ST_SOLVED) && !(status & ~(DMPC_ST_SOLVED | DMPC_ST_REACHED | DMPC_ST_HELD)); }

// the end of pc's last flight for destination scenes 0 .. S-1 (source scene: src_scene[s], null: s) into device arrays of S scenes, on pc's
// stream; the caller has checked the sources and synchronises
static int gather_end(dmpc_ctx *pc, int S, const int32_t *src_scene, double *x, double *plan)
{
    const FlightEnd &e = pc->end;
    const size_t A = (size_t)S * e.N_cmd;
    std::vector<int32_t> &src = pc->start_src_host;
    src.resize((size_t)S * 2);
    for (int s = 0; s < S; ++s) { const int q = src_scene ? src_scene[s] : s; src[2 * s] = q; src[2 * s + 1] = e.last[q]; }
    if (pc->end_src.ensure((size_t)S * 8)) FAIL(pc, "device allocation failed");
    hipStream_t st = pc->stream;
    HIPCHK(pc, hipMemcpyAsync(pc->end_src.p, src.data(), (size_t)S * 8, hipMemcpyHostToDevice, st));
    const double *v[2], *a[2];
    for (int u = 0; u < 2; ++u) {   // (step k writes set k & 1; set 1 is the context's own rows, and without hold so is set 0)
        v[u] = e.hold && !u ? pc->hold_out.as<double>() + (size_t)e.S * e.N_cmd * N3 : pc->vout.as<double>();
        a[u] = e.hold && !u ? pc->hold_out.as<double>() + 2 * (size_t)e.S * e.N_cmd * N3 : pc->aout.as<double>();
    }
    hipLaunchKernelGGL(end_gather_kernel, dim3(grid_1d(A * N3, 4096)), dim3(256), 0, st, S, e.N, e.N_cmd, e.e0_zero ? 1 : 0, (const int *)pc->end_src.as<int>(),
                       (const double *)pc->xp.as<double>(), (const double *)pc->xv.as<double>(), (const double *)pc->xa.as<double>(),
                       (const double *)pc->lT.as<double>(), (const double *)pc->lT2.as<double>(), v[0], v[1], a[0], a[1], x, x + A * 3, x + 2 * A * 3,
                       plan, plan + A * N3, plan + 2 * A * N3);
    HIPCHK(pc, hipGetLastError());
    return 0;
}

// the contexts that hold the end of ctx's last flight and their scenes: `at` as run_parts left it ({0, S}: ctx alone); false: no valid end
static bool end_parts(dmpc_ctx *ctx, std::vector<dmpc_ctx *> &pcs, std::vector<int> &at)
{
    pcs.clear(); at.clear();
    if (ctx->split_at.empty()) { pcs.push_back(ctx); at = {0, ctx->end.S}; return ctx->end.valid; }
    at = ctx->split_at;
    for (size_t i = 0; i + 1 < at.size(); ++i) {
        dmpc_ctx *pc = i ? (i - 1 < ctx->children.size() ? ctx->children[i - 1] : nullptr) : ctx;
        if (!pc || !pc->end.valid || pc->end.S != at[i + 1] - at[i] || pc->end.N_cmd != ctx->end.N_cmd) return false;
        pcs.push_back(pc);
    }
    return true;
}

// what a flight of S scenes and N_cmd commanded agents refuses of the armed start
static int check_start_shape(dmpc_ctx *ctx, const std::string &who, int S, int N_cmd)
{
    const StartState &a = ctx->start;
    if (a.armed && (a.S != S || a.N_cmd != N_cmd)) FAIL(ctx, who + ": the armed start (dmpc_set_start) is for another S or N_cmd");
    return 0;
}

// column 0 of a flight with a start, for transition_one: the start's arrays on the device
struct StartDev {
    dmpc_ctx *ctx; const Start &s; hipStream_t st;
    size_t A = 0;
    std::vector<int32_t> col_host;
    explicit operator bool() const { return s.on; }
    double *x(int u) const { return ctx->start_x.as<double>() + (size_t)u * A * 3; }           // x_p, x_v, x_a
    double *plan(int u) const { return ctx->start_plan.as<double>() + (size_t)u * A * N3; }   // plan_p, plan_v, plan_a
    const int *col0() const { return ctx->start_col.as<int>(); }
    // the buffers; host form: col0 of every scene up (from_end: the snapshot left everything in place)
    int begin(int S, int N_cmd) {
        A = (size_t)S * N_cmd;
        if (ctx->start_x.ensure(3 * A * 24) || ctx->start_plan.ensure(3 * A * N3 * 8) || ctx->start_col.ensure((size_t)S * 4)) FAIL(ctx, "device allocation failed");
        if (s.from_end) return 0;
        col_host.assign((size_t)S, s.col0);
        HIPCHK(ctx, hipMemcpyAsync(ctx->start_col.p, col_host.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
        return 0;
    }
    // x_v, x_a of column 0 (x_p is transition_one's: the call's po packed, or x(0) of a carried start)
    int states(double *xv, double *xa) {
        if (s.from_end) {
            HIPCHK(ctx, hipMemcpyAsync(xv, x(1), A * 24, hipMemcpyDeviceToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(xa, x(2), A * 24, hipMemcpyDeviceToDevice, st));
            return 0;
        }
        if (s.vo) HIPCHK(ctx, hipMemcpyAsync(xv, s.vo, A * 24, hipMemcpyHostToDevice, st)); else HIPCHK(ctx, hipMemsetAsync(xv, 0, A * 24, st));
        if (s.ao) HIPCHK(ctx, hipMemcpyAsync(xa, s.ao, A * 24, hipMemcpyHostToDevice, st)); else HIPCHK(ctx, hipMemsetAsync(xa, 0, A * 24, st));
        return 0;
    }
    // plan_p, plan_v, plan_a rows into the context's buffer: the caller's, or the braking plan from the states of column 0
    int plans(const double *xp, const double *xv, const double *xa) {
        if (s.from_end) return 0;
        if (!s.plan_p) {
            hipLaunchKernelGGL(start_plan_kernel, dim3((unsigned)((A * 3 + 255) / 256)), dim3(256), 0, st, (int)A, ctx->prm.h, ctx->prm.alim, xp, xv, xa, plan(0), plan(1), plan(2));
            return 0;
        }
        HIPCHK(ctx, hipMemcpyAsync(plan(0), s.plan_p, A * N3 * 8, hipMemcpyHostToDevice, st));
        if (s.plan_v) {
            HIPCHK(ctx, hipMemcpyAsync(plan(1), s.plan_v, A * N3 * 8, hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(plan(2), s.plan_a, A * N3 * 8, hipMemcpyHostToDevice, st));
        } else HIPCHK(ctx, hipMemsetAsync(plan(1), 0, 2 * A * N3 * 8, st));
        return 0;
    }
    // the caller's number of every scene's column 0, for the record of the flight's end
    void cols(std::vector<int32_t> &out, int S) const {
        if (!s.on) out.assign((size_t)S, 0);
        else if (s.from_end) out = ctx->start.col;
        else out.assign((size_t)S, s.col0);
    }
};

// ---------------------------------------------------------------------------------------------
// entries
// ---------------------------------------------------------------------------------------------

extern "C" int dmpc_set_start(dmpc_ctx *ctx, const dmpc_start *d)
{
    const std::string who = "dmpc_set_start";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    if (!d) { ctx->start.armed = false; return 0; }
    if (d->S < 1 || d->N_cmd < 1) FAIL(ctx, who + ": S and N_cmd must be >= 1");
    if (d->col0 < 0) FAIL(ctx, who + ": col0 must be >= 0");
    if ((size_t)d->S * (size_t)d->N_cmd > 0x7fffffffu / N3) FAIL(ctx, who + ": S * N_cmd overflows");
    const size_t A = (size_t)d->S * d->N_cmd;
    StartState a;
    a.armed = true; a.from_end = d->from_end != 0; a.S = d->S; a.N_cmd = d->N_cmd; a.col0 = d->col0;
    if (!a.from_end) {
        if (d->src_scene) FAIL(ctx, who + ": src_scene needs from_end");
        if ((d->plan_v != nullptr) != (d->plan_a != nullptr)) FAIL(ctx, who + ": plan_v and plan_a must be both given or both NULL");
        if (d->plan_v && !d->plan_p) FAIL(ctx, who + ": plan_v and plan_a need plan_p");
        const double *src[5] = {d->vo, d->ao, d->plan_p, d->plan_v, d->plan_a};
        std::vector<double> *dst[5] = {&a.vo, &a.ao, &a.plan_p, &a.plan_v, &a.plan_a};
        for (int u = 0; u < 5; ++u) {
            if (!src[u]) continue;
            const size_t n = A * (u < 2 ? 3 : N3);
            for (size_t j = 0; j < n; ++j)
                if (!std::isfinite(src[u][j])) FAIL(ctx, who + ": a vo, ao or plan value is not finite");
            dst[u]->assign(src[u], src[u] + n);
        }
        ctx->start = std::move(a);
        return 0;
    }
    // from_end: the snapshot, now
    if (d->vo || d->ao || d->plan_p || d->plan_v || d->plan_a) FAIL(ctx, who + ": from_end takes no host arrays (vo, ao and the plans must be NULL)");
    std::vector<dmpc_ctx *> pcs; std::vector<int> at;
    if (!end_parts(ctx, pcs, at)) FAIL(ctx, who + ": from_end: the context holds no valid flight end (no flight yet, a sharded one, or the step scratch was used since)");
    if (ctx->end.N_cmd != d->N_cmd) FAIL(ctx, who + ": from_end: N_cmd differs from the last flight's");
    const bool split = pcs.size() > 1;
    const int S_src = at.back();
    if (split && d->src_scene) FAIL(ctx, who + ": from_end: src_scene on the end of a split flight");
    if (!d->src_scene && d->S != S_src) FAIL(ctx, who + ": from_end: S differs from the last flight's (src_scene NULL: identity)");
    for (int s = 0; s < d->S; ++s) {
        const int q = d->src_scene ? d->src_scene[s] : s;
        if (q < 0 || q >= S_src) FAIL(ctx, who + ": from_end: src_scene[" + std::to_string(s) + "] is outside 0 .. S - 1 of the last flight");
        size_t i = 0;
        while (q >= at[i + 1]) ++i;
        if (!scene_ended_solved(pcs[i]->end.status[q - at[i]])) FAIL(ctx, who + ": from_end: source scene " + std::to_string(q) + " did not end DMPC_ST_SOLVED");
    }
    for (size_t i = 0; i < pcs.size(); ++i) {
        dmpc_ctx *pc = pcs[i];
        const int sn = split ? at[i + 1] - at[i] : d->S;
        const size_t An = (size_t)sn * d->N_cmd;
        HIPCHK(ctx, hipSetDevice(pc->device));
        if (pc->start_x.ensure(3 * An * 24) || pc->start_plan.ensure(3 * An * N3 * 8) || pc->start_col.ensure((size_t)sn * 4)) FAIL(ctx, "device allocation failed");
        pc->start.col.resize((size_t)sn);
        for (int s = 0; s < sn; ++s) { const int q = d->src_scene ? d->src_scene[s] : s; pc->start.col[s] = pc->end.col0[q] + pc->end.last[q] + d->col0; }
        if (gather_end(pc, sn, d->src_scene, pc->start_x.as<double>(), pc->start_plan.as<double>())) FAIL(ctx, pc->err);
        HIPCHK(ctx, hipMemcpyAsync(pc->start_col.p, pc->start.col.data(), (size_t)sn * 4, hipMemcpyHostToDevice, pc->stream));
    }
    for (dmpc_ctx *pc : pcs) HIPCHK(ctx, hipStreamSynchronize(pc->stream));
    (void)hipSetDevice(ctx->device);
    a.col = ctx->start.col;   // (part 0's, or the whole batch's)
    if (split) a.at = at;
    ctx->start = std::move(a);
    return 0;
}

extern "C" int dmpc_flight_end(dmpc_ctx *ctx, int S, int N_cmd, double *x_p, double *x_v, double *x_a, double *plan_p, double *plan_v, double *plan_a, int32_t *col)
{
    const std::string who = "dmpc_flight_end";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    if (S < 1 || N_cmd < 1) FAIL(ctx, who + ": S and N_cmd must be >= 1");
    std::vector<dmpc_ctx *> pcs; std::vector<int> at;
    if (!end_parts(ctx, pcs, at)) FAIL(ctx, who + ": the context holds no valid flight end (no flight yet, a sharded one, or the step scratch was used since)");
    if (at.back() != S || ctx->end.N_cmd != N_cmd) FAIL(ctx, who + ": S or N_cmd differs from the last flight's");
    for (size_t i = 0; i < pcs.size(); ++i)
        for (int s = at[i]; s < at[i + 1]; ++s)
            if (!scene_ended_solved(pcs[i]->end.status[s - at[i]])) FAIL(ctx, who + ": scene " + std::to_string(s) + " did not end DMPC_ST_SOLVED: it has no end");
    for (size_t i = 0; i < pcs.size(); ++i) {   // part by part, as the resident histories are gathered
        dmpc_ctx *pc = pcs[i];
        const int sn = at[i + 1] - at[i];
        const size_t An = (size_t)sn * N_cmd, a0 = (size_t)at[i] * N_cmd;
        HIPCHK(ctx, hipSetDevice(pc->device));
        if (pc->end_x.ensure(3 * An * 24) || pc->end_plan.ensure(3 * An * N3 * 8)) FAIL(ctx, "device allocation failed");
        if (gather_end(pc, sn, nullptr, pc->end_x.as<double>(), pc->end_plan.as<double>())) FAIL(ctx, pc->err);
        double *xs[3] = {x_p, x_v, x_a}, *ps[3] = {plan_p, plan_v, plan_a};
        for (int u = 0; u < 3; ++u) {
            if (xs[u]) HIPCHK(ctx, hipMemcpyAsync(xs[u] + a0 * 3, pc->end_x.as<double>() + (size_t)u * An * 3, An * 24, hipMemcpyDeviceToHost, pc->stream));
            if (ps[u]) HIPCHK(ctx, hipMemcpyAsync(ps[u] + a0 * N3, pc->end_plan.as<double>() + (size_t)u * An * N3, An * N3 * 8, hipMemcpyDeviceToHost, pc->stream));
        }
        if (col)
            for (int s = 0; s < sn; ++s) col[at[i] + s] = pc->end.col0[s] + pc->end.last[s];
    }
    for (dmpc_ctx *pc : pcs) HIPCHK(ctx, hipStreamSynchronize(pc->stream));
    (void)hipSetDevice(ctx->device);
    return 0;
}

extern "C" int dmpc_start_plan(const dmpc_params *prm, int n, const double *x_p, const double *x_v, const double *x_a, double *plan_p, double *plan_v, double *plan_a)
{
    const std::string who = "dmpc_start_plan";
    if (!prm || !x_p || !x_v || !x_a) FAIL((dmpc_ctx *)nullptr, who + ": NULL pointer");
    if (n < 1 || prm->K != K || !(prm->h > 0) || !(prm->alim > 0)) FAIL((dmpc_ctx *)nullptr, who + ": n must be >= 1, K = 15, h and alim positive");
    for (size_t t = 0; t < (size_t)n * 3; ++t) {
        const size_t o = (t / 3) * N3 + t % 3;
        brake_plan_axis(prm->h, prm->alim, x_p[t], x_v[t], x_a[t], plan_p ? plan_p + o : nullptr, plan_v ? plan_v + o : nullptr, plan_a ? plan_a + o : nullptr);
    }
    return 0;
}

extern "C" int dmpc_start_plan_device(dmpc_ctx *ctx, int n, const double *x_p, const double *x_v, const double *x_a, double *plan_p, double *plan_v, double *plan_a, void *stream)
{
    const std::string who = "dmpc_start_plan_device";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    if (n < 1 || (size_t)n > 0x7fffffffu / N3) FAIL(ctx, who + ": n must be >= 1");
    if (!x_p || !x_v || !x_a) FAIL(ctx, who + ": NULL pointer");
    if (ctx->grp) FAIL(ctx, who + ": device pointers belong to ONE GPU; a DMPC_DEVICE_ALL context drives several");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(start_plan_kernel, dim3((unsigned)(((size_t)n * 3 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, ctx->prm.h, ctx->prm.alim, x_p, x_v, x_a, plan_p, plan_v, plan_a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}
