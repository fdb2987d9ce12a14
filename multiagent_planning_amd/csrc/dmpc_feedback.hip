// dmpc_feedback.hip -- event-triggered feedback (included by dmpc_api.hip behind dmpc_disturb.hip, in front of dmpc_transition.hip): the planning
// state xh apart from the true state x, the tracking error e between them, and the re-anchoring of an agent's plan on an event.  No reference
// counterpart.  The rule is pinned in include/dmpc_hip.h; it is one function here, feedback_rule (and the one store of the re-anchoring,
// reanchor_entry), compiled for the device (post_step_feedback_kernel, feedback_kernel, reanchor_kernel) and for the host
// (dmpc_feedback_apply_host).  A measurement model (dmpc_set_measurement) puts sensor noise and a fixed-gain estimate between the true deviation
// and the rule's decision: estimate_rule beside feedback_rule, compiled for post_step_estimate_kernel, estimate_kernel and
// dmpc_estimate_apply_host; the re-anchoring is the same launch, on the estimate gh that stands in the event record.
//
// Two launches per column, not one.  The rule is per agent and sits where the disturbance sat, in the post step (one block per scene, the verdict's
// reduction behind it).  The re-anchoring is per (plan entry, agent): 3K times as many items, on the [3K][N] table that is contiguous along the
// agent index.  Inside the post step's block a scene of 10 000 agents would walk 450 000 entries with 256 threads; as a launch of its own the walk
// is spread over the device, a wave reads 64 flags with one load and leaves when none is set.  The launch is skipped when reanchor == 0.

// one agent, one column.  advanced: plan_p / plan_v are entry 0 of its p and v rows; else they are not read.  In/out: xh, e.  Out: the true
// x_p, x_v (may alias plan_p, plan_v), g = (g_p, g_v) [6], n = (n_p, n_v).  Returns the event.
__host__ __device__ inline bool feedback_rule(double trigger_p, double trigger_v, double h, bool advanced, const double *plan_p, const double *plan_v,
                                              const double *dp, const double *dv, double *xh_p, double *xh_v, double *e_p, double *e_v, double *x_p,
                                              double *x_v, double *g, double *n)
{
#pragma clang fp contract(off)   // every operation rounded on its own: the host, the device and the numpy restatement agree bit for bit
    double q_p[3], q_v[3];
    for (int c = 0; c < 3; ++c) {
        if (advanced) {
            q_p[c] = plan_p[c]; q_v[c] = plan_v[c];
            g[c] = (e_p[c] + h * e_v[c]) + dp[c];
        } else {
            q_p[c] = xh_p[c]; q_v[c] = xh_v[c];
            g[c] = e_p[c] + dp[c];
        }
        g[3 + c] = e_v[c] + dv[c];
        x_p[c] = q_p[c] + g[c];
        x_v[c] = q_v[c] + g[3 + c];
    }
    n[0] = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    n[1] = sqrt((g[3] * g[3] + g[4] * g[4]) + g[5] * g[5]);
    const bool event = n[0] > trigger_p || n[1] > trigger_v;
    for (int c = 0; c < 3; ++c) {
        xh_p[c] = event ? x_p[c] : q_p[c]; xh_v[c] = event ? x_v[c] : q_v[c];
        e_p[c] = event ? 0.0 : g[c];       e_v[c] = event ? 0.0 : g[3 + c];
    }
    return event;
}

// sqrt((x*x + y*y) + z*z), every operation rounded on its own
__host__ __device__ inline double norm3_plain(const double *g)
{
#pragma clang fp contract(off)
    return sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
}

// the measurement noise of agent i of scene sc OF THE CALL on the caller's column col >= 1: m_p = amp_p * u, m_v = amp_v * u, a stream of its
// own (bit 63 of the stream id: never the disturbance's, whatever the seeds)
__host__ __device__ inline void measure_noise(uint64_t seed, double amp_p, double amp_v, int sc, int i, int col, double *mp, double *mv)
{
#pragma clang fp contract(off)
    const uint64_t sid = (uint64_t)1 << 63 | (uint64_t)sc << 32 | (uint64_t)i;
    for (int c = 0; c < 3; ++c) {
        mp[c] = amp_p * (2.0 * gen::uniform(seed, sid, (uint64_t)(6 * (int64_t)col + c)) - 1.0);
        mv[c] = amp_v * (2.0 * gen::uniform(seed, sid, (uint64_t)(6 * (int64_t)col + 3 + c)) - 1.0);
    }
}

// feedback_rule with a measurement between the true deviation g and the decision: the rule decides on the estimate gh = b + gain * ((g + m) - b),
// b the belief eh propagated as e is; on an event the planner is set to q + gh and e keeps what the estimate missed.  The vehicle (x_p, x_v) is
// feedback_rule's, untouched by m.  In/out: xh, e, eh.  Out: x_p, x_v (may alias plan_p, plan_v), g, gh [6], d = g - gh [6], n = (|gh_p|, |gh_v|).
__host__ __device__ inline bool estimate_rule(double trigger_p, double trigger_v, double h, bool advanced, const double *plan_p, const double *plan_v,
                                              const double *dp, const double *dv, const double *mp, const double *mv, double amp_p, double amp_v,
                                              double gain_p, double gain_v, double *xh_p, double *xh_v, double *e_p, double *e_v, double *eh_p,
                                              double *eh_v, double *x_p, double *x_v, double *g, double *gh, double *d, double *n)
{
#pragma clang fp contract(off)   // every operation rounded on its own: the host, the device and the numpy restatement agree bit for bit
    double q_p[3], q_v[3];
    for (int c = 0; c < 3; ++c) {
        double b_p;
        if (advanced) {
            q_p[c] = plan_p[c]; q_v[c] = plan_v[c];
            g[c] = (e_p[c] + h * e_v[c]) + dp[c];
            b_p = eh_p[c] + h * eh_v[c];
        } else {
            q_p[c] = xh_p[c]; q_v[c] = xh_v[c];
            g[c] = e_p[c] + dp[c];
            b_p = eh_p[c];
        }
        const double b_v = eh_v[c];
        g[3 + c] = e_v[c] + dv[c];
        x_p[c] = q_p[c] + g[c];
        x_v[c] = q_v[c] + g[3 + c];
        const double y_p = amp_p > 0.0 ? g[c] + mp[c] : g[c], y_v = amp_v > 0.0 ? g[3 + c] + mv[c] : g[3 + c];
        gh[c] = gain_p == 1.0 ? y_p : b_p + gain_p * (y_p - b_p);
        gh[3 + c] = gain_v == 1.0 ? y_v : b_v + gain_v * (y_v - b_v);
        d[c] = g[c] - gh[c];
        d[3 + c] = g[3 + c] - gh[3 + c];
    }
    n[0] = norm3_plain(gh);
    n[1] = norm3_plain(gh + 3);
    const bool event = n[0] > trigger_p || n[1] > trigger_v;
    for (int c = 0; c < 3; ++c) {
        xh_p[c] = event ? q_p[c] + gh[c] : q_p[c]; xh_v[c] = event ? q_v[c] + gh[3 + c] : q_v[c];
        e_p[c] = event ? d[c] : g[c];              e_v[c] = event ? d[3 + c] : g[3 + c];
        eh_p[c] = event ? 0.0 : gh[c];             eh_v[c] = event ? 0.0 : gh[3 + c];
    }
    return event;
}

// the re-anchoring of plan entry kk, one component: the agent's entry of the next table and of its v row
__host__ __device__ inline void reanchor_entry(double h, int kk, double g_p, double g_v, double *table, double *v_row)
{
#pragma clang fp contract(off)
    *table = *table + (g_p + ((double)kk * h) * g_v);
    *v_row = *v_row + g_v;
}

// The hook of post_step_body for a flight with a policy and a disturbance.  post_step_body hands it (xp, xv) = entry 0 of the plan of an agent that
// advanced, else the stored true state (not read here: q is xh then), and records what it leaves there.
struct FeedbackArgs {
    static constexpr bool on = true;
    DisturbArgs D;
    double trigger_p, trigger_v;
    const int *status;                  // [S][N_cmd], behind the hold rule
    double *xh_p, *xh_v, *e_p, *e_v;    // [S][N_cmd][3]
    double *g;                          // [S][N_cmd][6]: the event record
    int *event;                         // [S][N_cmd]: the column of the agent's last event (0: none yet) -- reanchor_kernel's flag of column k is `== k`
    int *count, *first, *last, *p_col, *v_col;   // the log, [S][N_cmd] each
    double *p_max, *v_max;
    __device__ void operator()(int s, int i, int N, int k, double *xp, double *xv) const
    {
        const size_t a = (size_t)s * N + i, b = a * 3;
        double dp[3], dv[3], hp[3], hv[3], ep[3], ev[3], gg[6], n[2];
        disturb_delta(D, s, i, a, D.col0 ? D.col0[s] + k : k, dp, dv);
        for (int c = 0; c < 3; ++c) { hp[c] = xh_p[b + c]; hv[c] = xh_v[b + c]; ep[c] = e_p[b + c]; ev[c] = e_v[b + c]; }
        const bool hit = feedback_rule(trigger_p, trigger_v, D.h, (status[a] & ST_SOLVED) != 0, xp, xv, dp, dv, hp, hv, ep, ev, xp, xv, gg, n);
        for (int c = 0; c < 3; ++c) { xh_p[b + c] = hp[c]; xh_v[b + c] = hv[c]; e_p[b + c] = ep[c]; e_v[b + c] = ev[c]; }
        for (int c = 0; c < 6; ++c) g[a * 6 + c] = gg[c];
        if (hit) {
            event[a] = k;
            count[a] += 1;
            if (first[a] < 0) first[a] = k;
            last[a] = k;
        }
        if (n[0] > p_max[a]) { p_max[a] = n[0]; p_col[a] = k; }   // (columns come in order: ties stay with the smallest)
        if (n[1] > v_max[a]) { v_max[a] = n[1]; v_col[a] = k; }
    }
};

// post_step_kernel with the feedback rule (the disturbance inside it) between the state advance and the history record: one block per scene, the
// geometry of post_step_disturbed_kernel
__global__ void post_step_feedback_kernel(FeedbackArgs F, int N, int KT, int k, double tol, const double *__restrict__ p, const double *__restrict__ v,
                                          const double *__restrict__ a, double *x_p, double *x_v, double *x_a, const double *__restrict__ pf, double *pk,
                                          double *vk, double *ak, int *flags, int *scene_done, const int *__restrict__ stopped)
{
    post_step_body(N, KT, k, tol, p, v, a, F.status, x_p, x_v, x_a, pf, pk, vk, ak, flags, scene_done, stopped, F);
}

// dmpc_feedback_device: one thread per (scene, agent); a scene with scene_done[s] != 0 is left alone.  use_d == 0: no disturbance (D is not read)
__global__ __launch_bounds__(256) void feedback_kernel(DisturbArgs D, int use_d, double trigger_p, double trigger_v, double h, int S, int N_cmd, int k,
                                                       const double *__restrict__ p, const double *__restrict__ v, const double *__restrict__ a,
                                                       const int *__restrict__ status, double *x_p, double *x_v, double *x_a, double *xh_p, double *xh_v,
                                                       double *e_p, double *e_v, double *g, int *event, const int *__restrict__ scene_done)
{
    const size_t ag = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ag >= (size_t)S * N_cmd) return;
    const int s = (int)(ag / N_cmd), i = (int)(ag - (size_t)s * N_cmd);
    if (scene_done && scene_done[s]) return;
    const size_t b = ag * 3;
    const bool advanced = (status[ag] & ST_SOLVED) != 0;
    double dp[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, hp[3], hv[3], ep[3], ev[3], xp[3], xv[3], gg[6], n[2];
    if (use_d) disturb_delta(D, s, i, ag, k, dp, dv);
    for (int c = 0; c < 3; ++c) { hp[c] = xh_p[b + c]; hv[c] = xh_v[b + c]; ep[c] = e_p[b + c]; ev[c] = e_v[b + c]; }
    const bool hit = feedback_rule(trigger_p, trigger_v, h, advanced, p + ag * N3, v + ag * N3, dp, dv, hp, hv, ep, ev, xp, xv, gg, n);
    for (int c = 0; c < 3; ++c) {
        x_p[b + c] = xp[c]; x_v[b + c] = xv[c];
        if (advanced) x_a[b + c] = a[ag * N3 + c];
        xh_p[b + c] = hp[c]; xh_v[b + c] = hv[c]; e_p[b + c] = ep[c]; e_v[b + c] = ev[c];
    }
    for (int c = 0; c < 6; ++c) g[ag * 6 + c] = gg[c];
    event[ag] = hit ? 1 : 0;
}

// The hook of post_step_body for a flight with a policy and a measurement (a disturbance or none: use_d).  As FeedbackArgs, and: the belief, the
// measurement's stream, gh in the event record (what reanchor_kernel shifts by), dmpc_feedback_log's log on the norms of gh, dmpc_estimate_log's
// log.  One thread owns an agent: no atomics.
struct EstimateArgs {
    static constexpr bool on = true;
    DisturbArgs D; int use_d;
    uint64_t seed; double amp_p, amp_v, gain_p, gain_v;
    int s0; const int *col0;            // the index in the call of scene 0 of this launch; a start's column 0 per scene, or null
    double h, trigger_p, trigger_v;
    const int *status;                  // [S][N_cmd], behind the hold rule
    size_t A;                           // S * N_cmd: the stride of every block below
    double *x;                          // xh_p | xh_v | e_p | e_v, [A][3] each
    double *eh;                         // eh_p | eh_v, [A][3] each
    double *g;                          // [A][6]: the event record, gh
    int *event;                         // [A]: the column of the agent's last event
    int *fli; double *fld;              // dmpc_feedback_log's: count, first, last, p_col, v_col [A] each; p_max, v_max [A] each
    int *eli; double *eld;              // dmpc_estimate_log's: err_p_col, err_v_col, dev_p_col, dev_v_col; err_p_max, err_v_max, dev_p_max, dev_v_max
    __device__ void operator()(int s, int i, int N, int k, double *xp, double *xv) const
    {
        const size_t a = (size_t)s * N + i, b = a * 3;
        const int col = col0 ? col0[s] + k : k;
        double dp[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, mp[3], mv[3], hp[3], hv[3], ep[3], ev[3], bp[3], bv[3], gg[6], gh[6], dd[6], n[2];
        if (use_d) disturb_delta(D, s, i, a, col, dp, dv);
        measure_noise(seed, amp_p, amp_v, s0 + s, i, col, mp, mv);
        double *xh_p = x, *xh_v = x + A * 3, *e_p = x + A * 6, *e_v = x + A * 9, *eh_p = eh, *eh_v = eh + A * 3;
        for (int c = 0; c < 3; ++c) {
            hp[c] = xh_p[b + c]; hv[c] = xh_v[b + c]; ep[c] = e_p[b + c]; ev[c] = e_v[b + c]; bp[c] = eh_p[b + c]; bv[c] = eh_v[b + c];
        }
        const bool hit = estimate_rule(trigger_p, trigger_v, h, (status[a] & ST_SOLVED) != 0, xp, xv, dp, dv, mp, mv, amp_p, amp_v, gain_p, gain_v, hp, hv, ep,
                                       ev, bp, bv, xp, xv, gg, gh, dd, n);
        for (int c = 0; c < 3; ++c) {
            xh_p[b + c] = hp[c]; xh_v[b + c] = hv[c]; e_p[b + c] = ep[c]; e_v[b + c] = ev[c]; eh_p[b + c] = bp[c]; eh_v[b + c] = bv[c];
        }
        for (int c = 0; c < 6; ++c) g[a * 6 + c] = gh[c];
        if (hit) {
            event[a] = k;
            fli[a] += 1;
            if (fli[A + a] < 0) fli[A + a] = k;
            fli[2 * A + a] = k;
        }
        if (n[0] > fld[a]) { fld[a] = n[0]; fli[3 * A + a] = k; }   // (columns come in order: ties stay with the smallest)
        if (n[1] > fld[A + a]) { fld[A + a] = n[1]; fli[4 * A + a] = k; }
        const double m4[4] = {norm3_plain(dd), norm3_plain(dd + 3), norm3_plain(gg), norm3_plain(gg + 3)};
        for (int u = 0; u < 4; ++u)
            if (m4[u] > eld[u * A + a]) { eld[u * A + a] = m4[u]; eli[u * A + a] = k; }
    }
};

// post_step_feedback_kernel with the measurement between the true deviation and the rule's decision: the same geometry (128 or 256 threads; the
// bound lets the compiler keep the hook's state in registers -- at the default 1024 it left 16 bytes of scratch per lane)
__global__ __launch_bounds__(256) void post_step_estimate_kernel(EstimateArgs E, int N, int KT, int k, double tol, const double *__restrict__ p, const double *__restrict__ v,
                                          const double *__restrict__ a, double *x_p, double *x_v, double *x_a, const double *__restrict__ pf, double *pk,
                                          double *vk, double *ak, int *flags, int *scene_done, const int *__restrict__ stopped)
{
    post_step_body(N, KT, k, tol, p, v, a, E.status, x_p, x_v, x_a, pf, pk, vk, ak, flags, scene_done, stopped, E);
}

// what estimate_kernel takes of the context's settings
struct EstimateCol {
    DisturbArgs D; int use_d;
    uint64_t seed; double amp_p, amp_v, gain_p, gain_v;
    double h, trigger_p, trigger_v;
};

// dmpc_estimate_device: one thread per (scene, agent); a scene with scene_done[s] != 0 is left alone.  g gets gh: what reanchor_kernel shifts by
__global__ __launch_bounds__(256) void estimate_kernel(EstimateCol E, int S, int N_cmd, int k, const double *__restrict__ p, const double *__restrict__ v,
                                                       const double *__restrict__ a, const int *__restrict__ status, double *x_p, double *x_v, double *x_a,
                                                       double *xh_p, double *xh_v, double *e_p, double *e_v, double *eh_p, double *eh_v, double *g, int *event,
                                                       const int *__restrict__ scene_done)
{
    const size_t ag = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ag >= (size_t)S * N_cmd) return;
    const int s = (int)(ag / N_cmd), i = (int)(ag - (size_t)s * N_cmd);
    if (scene_done && scene_done[s]) return;
    const size_t b = ag * 3;
    const bool advanced = (status[ag] & ST_SOLVED) != 0;
    double dp[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, mp[3], mv[3], hp[3], hv[3], ep[3], ev[3], bp[3], bv[3], xp[3], xv[3], gg[6], gh[6], dd[6], n[2];
    if (E.use_d) disturb_delta(E.D, s, i, ag, k, dp, dv);
    measure_noise(E.seed, E.amp_p, E.amp_v, s, i, k, mp, mv);
    for (int c = 0; c < 3; ++c) {
        hp[c] = xh_p[b + c]; hv[c] = xh_v[b + c]; ep[c] = e_p[b + c]; ev[c] = e_v[b + c]; bp[c] = eh_p[b + c]; bv[c] = eh_v[b + c];
    }
    const bool hit = estimate_rule(E.trigger_p, E.trigger_v, E.h, advanced, p + ag * N3, v + ag * N3, dp, dv, mp, mv, E.amp_p, E.amp_v, E.gain_p, E.gain_v, hp, hv,
                                   ep, ev, bp, bv, xp, xv, gg, gh, dd, n);
    for (int c = 0; c < 3; ++c) {
        x_p[b + c] = xp[c]; x_v[b + c] = xv[c];
        if (advanced) x_a[b + c] = a[ag * N3 + c];
        xh_p[b + c] = hp[c]; xh_v[b + c] = hv[c]; e_p[b + c] = ep[c]; e_v[b + c] = ev[c]; eh_p[b + c] = bp[c]; eh_v[b + c] = bv[c];
    }
    for (int c = 0; c < 6; ++c) g[ag * 6 + c] = gh[c];
    event[ag] = hit ? 1 : 0;
}

// The re-anchoring of the agents whose flag is `mark`: one thread per (scene, plan entry, agent), the agent index fastest -- a wave covers 64
// neighbouring agents of one table line [s][j][.], so its loads and stores of lT_next are whole lines where the agents had events together (the v
// rows [S][N_cmd][3K] are strided by 3K; events are rare).  `stopped` (or null): scenes with a non-zero word are left alone.
__global__ __launch_bounds__(256) void reanchor_kernel(int S, int N, int N_cmd, int mark, double h, const int *__restrict__ event,
                                                       const double *__restrict__ g, const int *__restrict__ stopped, double *lT_next, double *v_rows)
{
    const size_t total = (size_t)S * N3 * N_cmd;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(t % N_cmd);
        const size_t u = t / N_cmd;
        const int j = (int)(u % N3), s = (int)(u / N3);
        const size_t ag = (size_t)s * N_cmd + i;
        if (event[ag] != mark || (stopped && stopped[s])) continue;
        const int c = j % 3;
        reanchor_entry(h, j / 3, g[ag * 6 + c], g[ag * 6 + 3 + c], lT_next + ((size_t)s * N3 + j) * N + i, v_rows + ag * N3 + j);
    }
}

// ---------------------------------------------------------------------------------------------
// host: the policy's check, the entries
// ---------------------------------------------------------------------------------------------

// what dmpc_set_feedback and dmpc_feedback_apply_host refuse; `why` gets the reason
static bool feedback_bad(const dmpc_feedback &f, std::string &why)
{
    if (!(f.trigger_p >= 0.0) || !(f.trigger_v >= 0.0)) { why = "trigger_p and trigger_v must be >= 0 (+inf allowed, NaN not)"; return true; }
    if (f.reanchor != 0 && f.reanchor != 1) { why = "reanchor must be 0 or 1"; return true; }
    return false;
}

extern "C" int dmpc_set_feedback(dmpc_ctx *ctx, const dmpc_feedback *fb)
{
    std::string why;
    if (fb && feedback_bad(*fb, why)) FAIL(ctx, "dmpc_set_feedback: " + why);   // (the policy first: its refusals need no context to be seen)
    if (!ctx) { g_err = "dmpc_set_feedback: ctx is NULL"; return -1; }
    ctx->fb = fb ? Feedback{true, fb->trigger_p, fb->trigger_v, fb->reanchor} : Feedback{};
    return 0;
}

// the shape and pointer check of dmpc_feedback_device and dmpc_feedback_apply_host
static int check_feedback_column(dmpc_ctx *ctx, const std::string &who, int S, int N, int N_cmd, int k, bool null_array)
{
    if (S < 1 || N_cmd < 1 || N_cmd > N || (size_t)S * (size_t)N > 0x7fffffffu / N3) FAIL(ctx, who + ": S and N_cmd must be >= 1, N_cmd <= N");
    if (k < 1) FAIL(ctx, who + ": k must be >= 1 (column 0 has xh = x, e = 0)");
    if (null_array) FAIL(ctx, who + ": NULL pointer");
    return 0;
}

extern "C" int dmpc_feedback_device(dmpc_ctx *ctx, int S, int N, int N_cmd, int k, const double *p_rows, double *v_rows, const double *a_rows,
                                    const int32_t *status, double *x_p, double *x_v, double *x_a, double *xh_p, double *xh_v, double *e_p, double *e_v,
                                    double *lT_next, int32_t *event, const int32_t *scene_done, void *stream)
{
    const std::string who = "dmpc_feedback_device";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    if (check_feedback_column(ctx, who, S, N, N_cmd, k, !p_rows || !v_rows || !a_rows || !status || !x_p || !x_v || !x_a || !xh_p || !xh_v || !e_p || !e_v || !lT_next || !event))
        return -1;
    if (ctx->grp) FAIL(ctx, who + ": device pointers belong to ONE GPU; a DMPC_DEVICE_ALL context drives several");
    if (check_disturb_shape(ctx, who, ctx->dist, S, N_cmd)) return -1;
    if (!ctx->fb.on) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t A = (size_t)S * N_cmd;
    if (ctx->fb_g.cap < A * 48) {   // (a larger record: the stream's earlier launches read the old one)
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (ctx->fb_g.ensure(A * 48)) FAIL(ctx, "device allocation failed");
    }
    DisturbArgs D{};
    if (ctx->dist.on) {   // the upload is kept for further columns of the same shape, as dmpc_disturb_device keeps it
        const long key = (long)S * 0x80000000L + N_cmd;
        if (ctx->dist_key != key) {
            HIPCHK(ctx, hipStreamSynchronize(st));
            if (disturb_upload(ctx, 0, S, N_cmd, st)) return -1;
            HIPCHK(ctx, hipStreamSynchronize(st));
            ctx->dist_key = key;
        }
        D = disturb_args(ctx, 0);
    }
    const Feedback &f = ctx->fb;
    hipLaunchKernelGGL(feedback_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, st, D, ctx->dist.on ? 1 : 0, f.trigger_p, f.trigger_v, ctx->prm.h, S, N_cmd, k,
                       p_rows, (const double *)v_rows, a_rows, (const int *)status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, ctx->fb_g.as<double>(), (int *)event,
                       (const int *)scene_done);
    if (f.reanchor)
        hipLaunchKernelGGL(reanchor_kernel, dim3(grid_1d(A * N3, 4096)), dim3(256), 0, st, S, N, N_cmd, 1, ctx->prm.h, (const int *)event,
                           (const double *)ctx->fb_g.as<double>(), (const int *)scene_done, lT_next, v_rows);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

extern "C" int dmpc_feedback_apply_host(const dmpc_feedback *fb, const dmpc_disturbance *d, double h, int S, int N, int N_cmd, int k,
                                        const double *p_rows, double *v_rows, const double *a_rows, const int32_t *status, double *x_p, double *x_v,
                                        double *x_a, double *xh_p, double *xh_v, double *e_p, double *e_v, double *lT_next, int32_t *event,
                                        const int32_t *scene_done)
{
    const std::string who = "dmpc_feedback_apply_host";
    dmpc_ctx *const none = nullptr;
    std::string why;
    if (!fb) FAIL(none, who + ": fb is NULL");
    if (feedback_bad(*fb, why)) FAIL(none, who + ": " + why);
    if (!std::isfinite(h)) FAIL(none, who + ": h must be finite");
    if (check_feedback_column(none, who, S, N, N_cmd, k, !p_rows || !v_rows || !a_rows || !status || !x_p || !x_v || !x_a || !xh_p || !xh_v || !e_p || !e_v || !lT_next || !event))
        return -1;
    const size_t A = (size_t)S * N_cmd;
    Disturbance dist;
    std::vector<int32_t> off;
    DisturbArgs D{};
    if (d) {
        if (disturbance_bad(*d, why)) FAIL(none, who + ": " + why);
        dist.set(*d);
        if (check_disturb_shape(none, who, dist, S, N_cmd)) return -1;
        off.resize(A + 1);
        disturb_offsets(dist, 0, S, N_cmd, off.data());
        D = DisturbArgs{dist.seed, dist.amp_p, dist.amp_v, h, dist.wind.empty() ? nullptr : dist.wind.data(), dist.wind_scenes == 1, 0, dist.push.data(),
                        dist.push.empty() ? nullptr : off.data()};
    }
    for (size_t ag = 0; ag < A; ++ag) {
        const int s = (int)(ag / N_cmd), i = (int)(ag % N_cmd);
        if (scene_done && scene_done[s]) continue;
        const size_t b = ag * 3;
        const bool advanced = (status[ag] & DMPC_ST_SOLVED) != 0;
        double dp[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, g[6], n[2];
        if (d) disturb_delta(D, s, i, ag, k, dp, dv);
        const bool hit = feedback_rule(fb->trigger_p, fb->trigger_v, h, advanced, p_rows + ag * N3, v_rows + ag * N3, dp, dv, xh_p + b, xh_v + b, e_p + b, e_v + b,
                                       x_p + b, x_v + b, g, n);
        if (advanced)
            for (int c = 0; c < 3; ++c) x_a[b + c] = a_rows[ag * N3 + c];
        event[ag] = hit ? 1 : 0;
        if (!hit || !fb->reanchor) continue;
        for (int j = 0; j < N3; ++j) reanchor_entry(h, j / 3, g[j % 3], g[3 + j % 3], lT_next + ((size_t)s * N3 + j) * N + i, v_rows + ag * N3 + j);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// the measurement model: its check, the entries
// ---------------------------------------------------------------------------------------------

// what dmpc_set_measurement, dmpc_measurement_sample and dmpc_estimate_apply_host refuse; `why` gets the reason
static bool measurement_bad(const dmpc_measurement &m, std::string &why)
{
    if (!(m.amp_p >= 0.0) || !std::isfinite(m.amp_p)) { why = "amp_p must be finite and >= 0"; return true; }
    if (!(m.amp_v >= 0.0) || !std::isfinite(m.amp_v)) { why = "amp_v must be finite and >= 0"; return true; }
    if (!(m.gain_p > 0.0) || !(m.gain_p <= 1.0)) { why = "gain_p must be in (0, 1]"; return true; }
    if (!(m.gain_v > 0.0) || !(m.gain_v <= 1.0)) { why = "gain_v must be in (0, 1]"; return true; }
    return false;
}

extern "C" int dmpc_set_measurement(dmpc_ctx *ctx, const dmpc_measurement *m)
{
    std::string why;
    if (m && measurement_bad(*m, why)) FAIL(ctx, "dmpc_set_measurement: " + why);   // (the descriptor first, as dmpc_set_feedback)
    if (!ctx) { g_err = "dmpc_set_measurement: ctx is NULL"; return -1; }
    ctx->meas = m ? Measurement{true, m->seed, m->amp_p, m->amp_v, m->gain_p, m->gain_v} : Measurement{};
    return 0;
}

extern "C" int dmpc_measurement_sample(const dmpc_measurement *m, int S, int N_cmd, int k, double *mp, double *mv)
{
    const std::string who = "dmpc_measurement_sample";
    dmpc_ctx *const none = nullptr;
    std::string why;
    if (!m || !mp || !mv) FAIL(none, who + ": NULL pointer");
    if (S < 1 || N_cmd < 1 || k < 0 || (size_t)S * (size_t)N_cmd > 0x7fffffffu) FAIL(none, who + ": S and N_cmd must be >= 1, k >= 0");
    if (measurement_bad(*m, why)) FAIL(none, who + ": " + why);
    const size_t A = (size_t)S * N_cmd;
    std::fill(mp, mp + A * 3, 0.0); std::fill(mv, mv + A * 3, 0.0);
    if (k == 0) return 0;   // column 0 is never measured: xh = x there
    for (size_t a = 0; a < A; ++a) measure_noise(m->seed, m->amp_p, m->amp_v, (int)(a / N_cmd), (int)(a % N_cmd), k, mp + a * 3, mv + a * 3);
    return 0;
}

extern "C" int dmpc_estimate_device(dmpc_ctx *ctx, int S, int N, int N_cmd, int k, const double *p_rows, double *v_rows, const double *a_rows,
                                    const int32_t *status, double *x_p, double *x_v, double *x_a, double *xh_p, double *xh_v, double *e_p, double *e_v,
                                    double *eh_p, double *eh_v, double *lT_next, int32_t *event, const int32_t *scene_done, void *stream)
{
    const std::string who = "dmpc_estimate_device";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    if (check_feedback_column(ctx, who, S, N, N_cmd, k,
                              !p_rows || !v_rows || !a_rows || !status || !x_p || !x_v || !x_a || !xh_p || !xh_v || !e_p || !e_v || !eh_p || !eh_v || !lT_next || !event))
        return -1;
    if (ctx->grp) FAIL(ctx, who + ": device pointers belong to ONE GPU; a DMPC_DEVICE_ALL context drives several");
    if (check_disturb_shape(ctx, who, ctx->dist, S, N_cmd)) return -1;
    if (!ctx->fb.on || !ctx->meas.on) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t A = (size_t)S * N_cmd;
    if (ctx->fb_g.cap < A * 48) {   // (a larger record: the stream's earlier launches read the old one)
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (ctx->fb_g.ensure(A * 48)) FAIL(ctx, "device allocation failed");
    }
    DisturbArgs D{};
    if (ctx->dist.on) {   // the upload is kept for further columns of the same shape, as dmpc_disturb_device keeps it
        const long key = (long)S * 0x80000000L + N_cmd;
        if (ctx->dist_key != key) {
            HIPCHK(ctx, hipStreamSynchronize(st));
            if (disturb_upload(ctx, 0, S, N_cmd, st)) return -1;
            HIPCHK(ctx, hipStreamSynchronize(st));
            ctx->dist_key = key;
        }
        D = disturb_args(ctx, 0);
    }
    const Feedback &f = ctx->fb;
    const Measurement &m = ctx->meas;
    const EstimateCol E{D, ctx->dist.on ? 1 : 0, m.seed, m.amp_p, m.amp_v, m.gain_p, m.gain_v, ctx->prm.h, f.trigger_p, f.trigger_v};
    hipLaunchKernelGGL(estimate_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, st, E, S, N_cmd, k, p_rows, (const double *)v_rows, a_rows,
                       (const int *)status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v, ctx->fb_g.as<double>(), (int *)event, (const int *)scene_done);
    if (f.reanchor)
        hipLaunchKernelGGL(reanchor_kernel, dim3(grid_1d(A * N3, 4096)), dim3(256), 0, st, S, N, N_cmd, 1, ctx->prm.h, (const int *)event,
                           (const double *)ctx->fb_g.as<double>(), (const int *)scene_done, lT_next, v_rows);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

extern "C" int dmpc_estimate_apply_host(const dmpc_feedback *fb, const dmpc_measurement *m, const dmpc_disturbance *d, double h, int S, int N, int N_cmd,
                                        int k, const double *p_rows, double *v_rows, const double *a_rows, const int32_t *status, double *x_p, double *x_v,
                                        double *x_a, double *xh_p, double *xh_v, double *e_p, double *e_v, double *eh_p, double *eh_v, double *lT_next,
                                        int32_t *event, const int32_t *scene_done)
{
    const std::string who = "dmpc_estimate_apply_host";
    dmpc_ctx *const none = nullptr;
    std::string why;
    if (!fb) FAIL(none, who + ": fb is NULL");
    if (!m) FAIL(none, who + ": m is NULL");
    if (feedback_bad(*fb, why)) FAIL(none, who + ": " + why);
    if (measurement_bad(*m, why)) FAIL(none, who + ": " + why);
    if (!std::isfinite(h)) FAIL(none, who + ": h must be finite");
    if (check_feedback_column(none, who, S, N, N_cmd, k,
                              !p_rows || !v_rows || !a_rows || !status || !x_p || !x_v || !x_a || !xh_p || !xh_v || !e_p || !e_v || !eh_p || !eh_v || !lT_next || !event))
        return -1;
    const size_t A = (size_t)S * N_cmd;
    Disturbance dist;
    std::vector<int32_t> off;
    DisturbArgs D{};
    if (d) {
        if (disturbance_bad(*d, why)) FAIL(none, who + ": " + why);
        dist.set(*d);
        if (check_disturb_shape(none, who, dist, S, N_cmd)) return -1;
        off.resize(A + 1);
        disturb_offsets(dist, 0, S, N_cmd, off.data());
        D = DisturbArgs{dist.seed, dist.amp_p, dist.amp_v, h, dist.wind.empty() ? nullptr : dist.wind.data(), dist.wind_scenes == 1, 0, dist.push.data(),
                        dist.push.empty() ? nullptr : off.data()};
    }
    for (size_t ag = 0; ag < A; ++ag) {
        const int s = (int)(ag / N_cmd), i = (int)(ag % N_cmd);
        if (scene_done && scene_done[s]) continue;
        const size_t b = ag * 3;
        const bool advanced = (status[ag] & DMPC_ST_SOLVED) != 0;
        double dp[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, mp[3], mv[3], g[6], gh[6], dd[6], n[2];
        if (d) disturb_delta(D, s, i, ag, k, dp, dv);
        measure_noise(m->seed, m->amp_p, m->amp_v, s, i, k, mp, mv);
        const bool hit = estimate_rule(fb->trigger_p, fb->trigger_v, h, advanced, p_rows + ag * N3, v_rows + ag * N3, dp, dv, mp, mv, m->amp_p, m->amp_v, m->gain_p,
                                       m->gain_v, xh_p + b, xh_v + b, e_p + b, e_v + b, eh_p + b, eh_v + b, x_p + b, x_v + b, g, gh, dd, n);
        if (advanced)
            for (int c = 0; c < 3; ++c) x_a[b + c] = a_rows[ag * N3 + c];
        event[ag] = hit ? 1 : 0;
        if (!hit || !fb->reanchor) continue;
        for (int j = 0; j < N3; ++j) reanchor_entry(h, j / 3, gh[j % 3], gh[3 + j % 3], lT_next + ((size_t)s * N3 + j) * N + i, v_rows + ag * N3 + j);
    }
    return 0;
}

// the contexts that hold the log of ctx's last flight and their scenes, as end_parts finds a flight's end; false: no flight with a policy
static bool feedback_parts(dmpc_ctx *ctx, std::vector<dmpc_ctx *> &pcs, std::vector<int> &at)
{
    pcs.clear(); at.clear();
    if (ctx->split_at.empty()) { pcs.push_back(ctx); at = {0, ctx->fb_flight.S}; return ctx->fb_flight.valid; }
    at = ctx->split_at;
    for (size_t i = 0; i + 1 < at.size(); ++i) {
        dmpc_ctx *pc = i ? (i - 1 < ctx->children.size() ? ctx->children[i - 1] : nullptr) : ctx;
        if (!pc || !pc->fb_flight.valid || pc->fb_flight.S != at[i + 1] - at[i] || pc->fb_flight.N_cmd != ctx->fb_flight.N_cmd) return false;
        pcs.push_back(pc);
    }
    return true;
}

extern "C" int dmpc_feedback_log(dmpc_ctx *ctx, int S, int N_cmd, int32_t *event_count, int32_t *event_first, int32_t *event_last, double *dev_p_max,
                                 int32_t *dev_p_col, double *dev_v_max, int32_t *dev_v_col, double *xh_p, double *xh_v, double *e_p, double *e_v)
{
    const std::string who = "dmpc_feedback_log";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    if (S < 1 || N_cmd < 1) FAIL(ctx, who + ": S and N_cmd must be >= 1");
    std::vector<dmpc_ctx *> pcs; std::vector<int> at;
    if (!feedback_parts(ctx, pcs, at)) FAIL(ctx, who + ": the context holds no log (no flight yet, a sharded one, or a flight with no policy set)");
    if (at.back() != S || ctx->fb_flight.N_cmd != N_cmd) FAIL(ctx, who + ": S or N_cmd differs from the last flight's");
    for (size_t i = 0; i < pcs.size(); ++i) {   // part by part, as dmpc_flight_end gathers a flight's end
        dmpc_ctx *pc = pcs[i];
        const size_t An = (size_t)(at[i + 1] - at[i]) * N_cmd, a0 = (size_t)at[i] * N_cmd;
        int32_t *ints[5] = {event_count, event_first, event_last, dev_p_col, dev_v_col};
        double *maxs[2] = {dev_p_max, dev_v_max}, *xs[4] = {xh_p, xh_v, e_p, e_v};
        if (!pc->fb_flight.live) {   // the policy was inert: xh is the true state the scratch still holds, e = 0, no event, no deviation
            if ((xh_p || xh_v) && !pc->end.valid) FAIL(ctx, who + ": the policy was inert (no disturbance) and the step scratch that holds the states was used since the flight");
            HIPCHK(ctx, hipSetDevice(pc->device));
            for (int u = 0; u < 5; ++u) if (ints[u]) std::fill(ints[u] + a0, ints[u] + a0 + An, u == 1 || u == 2 ? -1 : 0);
            for (int u = 0; u < 2; ++u) if (maxs[u]) std::fill(maxs[u] + a0, maxs[u] + a0 + An, 0.0);
            for (int u = 2; u < 4; ++u) if (xs[u]) std::fill(xs[u] + a0 * 3, xs[u] + (a0 + An) * 3, 0.0);
            if (xh_p) HIPCHK(ctx, hipMemcpyAsync(xh_p + a0 * 3, pc->xp.p, An * 24, hipMemcpyDeviceToHost, pc->stream));
            if (xh_v) HIPCHK(ctx, hipMemcpyAsync(xh_v + a0 * 3, pc->xv.p, An * 24, hipMemcpyDeviceToHost, pc->stream));
            continue;
        }
        HIPCHK(ctx, hipSetDevice(pc->device));
        for (int u = 0; u < 5; ++u) if (ints[u]) HIPCHK(ctx, hipMemcpyAsync(ints[u] + a0, pc->fb_logi.as<int32_t>() + (size_t)u * An, An * 4, hipMemcpyDeviceToHost, pc->stream));
        for (int u = 0; u < 2; ++u) if (maxs[u]) HIPCHK(ctx, hipMemcpyAsync(maxs[u] + a0, pc->fb_logd.as<double>() + (size_t)u * An, An * 8, hipMemcpyDeviceToHost, pc->stream));
        for (int u = 0; u < 4; ++u) if (xs[u]) HIPCHK(ctx, hipMemcpyAsync(xs[u] + a0 * 3, pc->fb_x.as<double>() + (size_t)u * An * 3, An * 24, hipMemcpyDeviceToHost, pc->stream));
    }
    for (dmpc_ctx *pc : pcs) HIPCHK(ctx, hipStreamSynchronize(pc->stream));
    (void)hipSetDevice(ctx->device);
    return 0;
}

extern "C" int dmpc_estimate_log(dmpc_ctx *ctx, int S, int N_cmd, double *err_p_max, int32_t *err_p_col, double *err_v_max, int32_t *err_v_col, double *dev_p_max,
                                 int32_t *dev_p_col, double *dev_v_max, int32_t *dev_v_col, double *eh_p, double *eh_v)
{
    const std::string who = "dmpc_estimate_log";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    if (S < 1 || N_cmd < 1) FAIL(ctx, who + ": S and N_cmd must be >= 1");
    std::vector<dmpc_ctx *> pcs; std::vector<int> at;
    bool ok = feedback_parts(ctx, pcs, at);
    for (size_t i = 0; ok && i < pcs.size(); ++i) ok = pcs[i]->fb_flight.measured;
    if (!ok) FAIL(ctx, who + ": the context holds no log (no flight yet, a sharded one, or a flight with no measurement set: dmpc_set_measurement)");
    if (at.back() != S || ctx->fb_flight.N_cmd != N_cmd) FAIL(ctx, who + ": S or N_cmd differs from the last flight's");
    for (size_t i = 0; i < pcs.size(); ++i) {   // part by part, as dmpc_feedback_log
        dmpc_ctx *pc = pcs[i];
        const size_t An = (size_t)(at[i + 1] - at[i]) * N_cmd, a0 = (size_t)at[i] * N_cmd;
        int32_t *cols[4] = {err_p_col, err_v_col, dev_p_col, dev_v_col};
        double *maxs[4] = {err_p_max, err_v_max, dev_p_max, dev_v_max}, *xs[2] = {eh_p, eh_v};
        HIPCHK(ctx, hipSetDevice(pc->device));
        for (int u = 0; u < 4; ++u) if (cols[u]) HIPCHK(ctx, hipMemcpyAsync(cols[u] + a0, pc->est_logi.as<int32_t>() + (size_t)u * An, An * 4, hipMemcpyDeviceToHost, pc->stream));
        for (int u = 0; u < 4; ++u) if (maxs[u]) HIPCHK(ctx, hipMemcpyAsync(maxs[u] + a0, pc->est_logd.as<double>() + (size_t)u * An, An * 8, hipMemcpyDeviceToHost, pc->stream));
        for (int u = 0; u < 2; ++u) if (xs[u]) HIPCHK(ctx, hipMemcpyAsync(xs[u] + a0 * 3, pc->est_x.as<double>() + (size_t)u * An * 3, An * 24, hipMemcpyDeviceToHost, pc->stream));
    }
    for (dmpc_ctx *pc : pcs) HIPCHK(ctx, hipStreamSynchronize(pc->stream));
    (void)hipSetDevice(ctx->device);
    return 0;
}
