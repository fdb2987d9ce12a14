// dmpc_disturb.hip -- disturbed transitions (included by dmpc_api.hip in front of dmpc_transition.hip): a constant wind, bounded noise on position and
// velocity and listed pushes, added to the state of every commanded agent between the state advance and the history record of every column k >= 1.
// No reference counterpart (the reference's loop never sees a state it did not predict).  The rule is pinned in include/dmpc_hip.h; it is one
// function here, disturb_delta, compiled for the device (disturb_kernel, post_step_disturbed_kernel) and for the host (dmpc_disturbance_sample).
//
// The context keeps a copy of the descriptor with the pushes sorted by (scene, agent, column), stable.  A call uploads the wind, the sorted pushes
// and one offset per (scene, agent) of the call into ctx->dist_buf (disturb_upload), so that a thread walks the pushes of its own agent alone.

// what the rule reads, as the device sees it (host: the same, with host pointers)
struct DisturbArgs {
    static constexpr bool on = true;
    uint64_t seed;
    double amp_p, amp_v, h;
    const double *wind;      // [wind_scenes][3] or null
    int wind_all;            // 1: row 0 for every scene
    int s0;                  // the index in the call of scene 0 of this launch (a split batch)
    const dmpc_push *push;   // sorted by (scene, agent, column), list order among equal keys
    const int *off;          // [S * N_cmd + 1]: the pushes of agent a of this launch are push[off[a]] .. push[off[a + 1] - 1]
    const int *col0 = nullptr;   // a flight with a start (dmpc_start.hip): [S] the caller's number of every scene's column 0, added to k; null: 0
    // the hook of post_step_body: scene s and agent i of the launch, column k
    __device__ void operator()(int s, int i, int N, int k, double *xp, double *xv) const;
};

// dp, dv of the rule for agent i of scene s of the launch (a = s * N_cmd + i), column k >= 1
__host__ __device__ inline void disturb_delta(const DisturbArgs &D, int s, int i, size_t a, int k, double *dp, double *dv)
{
#pragma clang fp contract(off)   // every operation rounded on its own: the host, the device and the numpy restatement agree bit for bit
    const uint64_t sc = (uint64_t)(D.s0 + s);
    const uint64_t sid = sc << 32 | (uint64_t)i;
    const double *w = D.wind ? D.wind + (D.wind_all ? 0 : sc * 3) : nullptr;
    const double hh = (0.5 * D.h) * D.h;
    for (int c = 0; c < 3; ++c) {
        const double wc = w ? w[c] : 0.0;
        dp[c] = hh * wc;
        dv[c] = D.h * wc;
        if (D.amp_p > 0.0) dp[c] = dp[c] + D.amp_p * (2.0 * gen::uniform(D.seed, sid, (uint64_t)(6 * (int64_t)k + c)) - 1.0);
        if (D.amp_v > 0.0) dv[c] = dv[c] + D.amp_v * (2.0 * gen::uniform(D.seed, sid, (uint64_t)(6 * (int64_t)k + 3 + c)) - 1.0);
    }
    if (!D.off) return;
    for (int j = D.off[a]; j < D.off[a + 1]; ++j) {
        if (D.push[j].column != k) continue;
        for (int c = 0; c < 3; ++c) { dp[c] = dp[c] + D.push[j].dp[c]; dv[c] = dv[c] + D.push[j].dv[c]; }
    }
}

__device__ inline void DisturbArgs::operator()(int s, int i, int N, int k, double *xp, double *xv) const
{
    double dp[3], dv[3];
    disturb_delta(*this, s, i, (size_t)s * N + i, col0 ? col0[s] + k : k, dp, dv);
    for (int c = 0; c < 3; ++c) { xp[c] = xp[c] + dp[c]; xv[c] = xv[c] + dv[c]; }
}

// dmpc_disturb_device: one thread per (scene, agent); x_p, x_v [S][N_cmd][3]; a scene with scene_done[s] != 0 is left alone
__global__ __launch_bounds__(256) void disturb_kernel(DisturbArgs D, int S, int N_cmd, int k, double *x_p, double *x_v, const int *__restrict__ scene_done)
{
    const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= (size_t)S * N_cmd) return;
    const int s = (int)(a / N_cmd), i = (int)(a - (size_t)s * N_cmd);
    if (scene_done && scene_done[s]) return;
    double xp[3], xv[3];
    for (int c = 0; c < 3; ++c) { xp[c] = x_p[a * 3 + c]; xv[c] = x_v[a * 3 + c]; }
    D(s, i, N_cmd, k, xp, xv);
    for (int c = 0; c < 3; ++c) { x_p[a * 3 + c] = xp[c]; x_v[a * 3 + c] = xv[c]; }
}

// post_step_kernel with the disturbance between the state advance and the history record (one block per scene, the same geometry)
__global__ void post_step_disturbed_kernel(DisturbArgs D, int N, int KT, int k, double tol, const double *__restrict__ p, const double *__restrict__ v,
                                           const double *__restrict__ a, const int *__restrict__ status, double *x_p, double *x_v, double *x_a,
                                           const double *__restrict__ pf, double *pk, double *vk, double *ak, int *flags, int *scene_done,
                                           const int *__restrict__ stopped)
{
    post_step_body(N, KT, k, tol, p, v, a, status, x_p, x_v, x_a, pf, pk, vk, ak, flags, scene_done, stopped, D);
}

// ---------------------------------------------------------------------------------------------
// host: the descriptor's check, the context's copy, the upload of a call
// ---------------------------------------------------------------------------------------------

// what dmpc_set_disturbance and dmpc_disturbance_sample refuse; `why` gets the reason
static bool disturbance_bad(const dmpc_disturbance &d, std::string &why)
{
    if (!(d.amp_p >= 0.0) || !std::isfinite(d.amp_p) || !(d.amp_v >= 0.0) || !std::isfinite(d.amp_v)) { why = "amp_p and amp_v must be finite and >= 0"; return true; }
    if (d.wind_scenes < 0 || d.n_push < 0) { why = "wind_scenes and n_push must be >= 0"; return true; }
    if ((d.wind_scenes > 0 && !d.wind) || (d.n_push > 0 && !d.push)) { why = "a NULL array with a positive count"; return true; }
    for (size_t j = 0; j < (size_t)d.wind_scenes * 3; ++j)
        if (!std::isfinite(d.wind[j])) { why = "a wind value is not finite"; return true; }
    for (int j = 0; j < d.n_push; ++j) {
        const dmpc_push &q = d.push[j];
        if (q.scene < 0 || q.agent < 0 || q.column < 1) { why = "a push needs scene >= 0, agent >= 0 and column >= 1 (column 0 is never disturbed)"; return true; }
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(q.dp[c]) || !std::isfinite(q.dv[c])) { why = "a push value is not finite"; return true; }
    }
    return false;
}

void Disturbance::set(const dmpc_disturbance &d)
{
    on = true; seed = d.seed; amp_p = d.amp_p; amp_v = d.amp_v; wind_scenes = d.wind_scenes;
    wind.assign(d.wind, d.wind + (size_t)d.wind_scenes * 3);
    push.assign(d.push, d.push + d.n_push);
    std::stable_sort(push.begin(), push.end(), [](const dmpc_push &x, const dmpc_push &y) {
        return x.scene != y.scene ? x.scene < y.scene : x.agent != y.agent ? x.agent < y.agent : x.column < y.column;
    });
}

// what a call of S scenes and N_cmd commanded agents refuses of the disturbance in force
static int check_disturb_shape(dmpc_ctx *ctx, const std::string &who, const Disturbance &d, int S, int N_cmd)
{
    if (!d.on) return 0;
    if (d.wind_scenes != 0 && d.wind_scenes != 1 && d.wind_scenes != S) FAIL(ctx, who + ": the disturbance's wind_scenes must be 1 or S");
    for (const dmpc_push &q : d.push)
        if (q.scene >= S || q.agent >= N_cmd) FAIL(ctx, who + ": a push of the disturbance names a scene >= S or an agent >= N_cmd");
    return 0;
}

// offsets [S * N_cmd + 1] into the sorted pushes for scenes [s0, s0 + S) of a call
static void disturb_offsets(const Disturbance &d, int s0, int S, int N_cmd, int32_t *off)
{
    const size_t A = (size_t)S * N_cmd, n = d.push.size();
    size_t j = 0;
    for (size_t a = 0; a <= A; ++a) {
        const int s = s0 + (int)(a / N_cmd), i = (int)(a % N_cmd);
        while (j < n && (d.push[j].scene < s || (d.push[j].scene == s && d.push[j].agent < i))) ++j;
        off[a] = (int32_t)j;
    }
}

// the wind, the sorted pushes and the offsets of scenes [s0, s0 + S) into ctx->dist_buf on `st`; the staging block is the context's and stays as it
// is until the next upload
static int disturb_upload(dmpc_ctx *ctx, int s0, int S, int N_cmd, hipStream_t st)
{
    const Disturbance &d = ctx->dist;
    const size_t A = (size_t)S * N_cmd, wb = d.wind.size() * 8, pb = d.push.size() * sizeof(dmpc_push), ob = pb ? (A + 1) * 4 : 0;
    std::vector<unsigned char> &stage = ctx->dist_stage;
    stage.resize(wb + pb + ob);
    if (wb) std::memcpy(stage.data(), d.wind.data(), wb);
    if (pb) {
        std::memcpy(stage.data() + wb, d.push.data(), pb);
        disturb_offsets(d, s0, S, N_cmd, (int32_t *)(stage.data() + wb + pb));
    }
    if (ctx->dist_buf.ensure(stage.size() + 8)) FAIL(ctx, "device allocation failed");
    if (!stage.empty()) HIPCHK(ctx, hipMemcpyAsync(ctx->dist_buf.p, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
    return 0;
}
// what the kernels take, on the block disturb_upload(ctx, s0, ..) filled
static DisturbArgs disturb_args(dmpc_ctx *ctx, int s0)
{
    const Disturbance &d = ctx->dist;
    const size_t wb = d.wind.size() * 8, pb = d.push.size() * sizeof(dmpc_push);
    const unsigned char *base = ctx->dist_buf.as<unsigned char>();
    return DisturbArgs{d.seed, d.amp_p, d.amp_v, ctx->prm.h, wb ? (const double *)base : nullptr, d.wind_scenes == 1, s0,
                       pb ? (const dmpc_push *)(base + wb) : nullptr, pb ? (const int *)(base + wb + pb) : nullptr};
}

// ---------------------------------------------------------------------------------------------
// entries
// ---------------------------------------------------------------------------------------------

extern "C" int dmpc_set_disturbance(dmpc_ctx *ctx, const dmpc_disturbance *d)
{
    if (!ctx) { g_err = "dmpc_set_disturbance: ctx is NULL"; return -1; }
    std::string why;
    if (d && disturbance_bad(*d, why)) FAIL(ctx, "dmpc_set_disturbance: " + why);
    ctx->dist_key = -1;
    if (!d || (d->seed == 0 && d->amp_p == 0.0 && d->amp_v == 0.0 && d->wind_scenes == 0 && d->n_push == 0)) ctx->dist = Disturbance{};
    else ctx->dist.set(*d);
    return 0;
}

extern "C" int dmpc_disturbance_sample(const dmpc_disturbance *d, double h, int S, int N_cmd, int k, double *dp, double *dv)
{
    const std::string who = "dmpc_disturbance_sample";
    std::string why;
    if (!d || !dp || !dv) FAIL((dmpc_ctx *)nullptr, who + ": NULL pointer");
    if (S < 1 || N_cmd < 1 || k < 0 || !std::isfinite(h) || (size_t)S * (size_t)N_cmd > 0x7fffffffu) FAIL((dmpc_ctx *)nullptr, who + ": S and N_cmd must be >= 1, k >= 0, h finite");
    if (disturbance_bad(*d, why)) FAIL((dmpc_ctx *)nullptr, who + ": " + why);
    Disturbance c; c.set(*d);
    if (check_disturb_shape(nullptr, who, c, S, N_cmd)) return -1;
    const size_t A = (size_t)S * N_cmd;
    std::fill(dp, dp + A * 3, 0.0); std::fill(dv, dv + A * 3, 0.0);
    if (k == 0) return 0;   // column 0 is never disturbed
    std::vector<int32_t> off(A + 1);
    disturb_offsets(c, 0, S, N_cmd, off.data());
    const DisturbArgs D{c.seed, c.amp_p, c.amp_v, h, c.wind.empty() ? nullptr : c.wind.data(), c.wind_scenes == 1, 0, c.push.data(), c.push.empty() ? nullptr : off.data()};
    for (size_t a = 0; a < A; ++a) disturb_delta(D, (int)(a / N_cmd), (int)(a % N_cmd), a, k, dp + a * 3, dv + a * 3);
    return 0;
}

// the disturbance of column k for callers that loop over dmpc_step_device_cmd themselves: behind dmpc_advance_device, in front of whatever records
extern "C" int dmpc_disturb_device(dmpc_ctx *ctx, int S, int N_cmd, int k, double *x_p, double *x_v, const int32_t *scene_done, void *stream)
{
    const std::string who = "dmpc_disturb_device";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    if (S < 1 || N_cmd < 1 || (size_t)S * (size_t)N_cmd > 0x7fffffffu) FAIL(ctx, who + ": S and N_cmd must be >= 1");
    if (k < 1) FAIL(ctx, who + ": k must be >= 1 (column 0 is never disturbed)");
    if (!x_p || !x_v) FAIL(ctx, who + ": NULL pointer");
    if (ctx->grp) FAIL(ctx, who + ": device pointers belong to ONE GPU; a DMPC_DEVICE_ALL context drives several");
    if (check_disturb_shape(ctx, who, ctx->dist, S, N_cmd)) return -1;
    if (!ctx->dist.on) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    // the upload is kept for further columns of the same shape: a change of it waits for the stream, whose earlier launches read the block
    const long key = (long)S * 0x80000000L + N_cmd;
    if (ctx->dist_key != key) {
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (disturb_upload(ctx, 0, S, N_cmd, st)) return -1;
        HIPCHK(ctx, hipStreamSynchronize(st));
        ctx->dist_key = key;
    }
    hipLaunchKernelGGL(disturb_kernel, dim3((unsigned)(((size_t)S * N_cmd + 255) / 256)), dim3(256), 0, st, disturb_args(ctx, 0), S, N_cmd, k, x_p, x_v, (const int *)scene_done);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}
