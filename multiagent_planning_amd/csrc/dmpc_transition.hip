// dmpc_transition.hip -- the closed loop on one GPU (included by dmpc_api.hip; the sharded loop is in dmpc_multigpu.hip): the record of a call and
// its argument check, the MPC loop (transition_one), the split of a batch over contexts (batch_parts, transition_any), the entries.
//
// The whole `for k = 1:K_T` loop on the device (dmpc_soft_bound.m:115-148, failure_rate.m:99-127) for the N_cmd commanded agents of N vehicles
// (DMPC::solveParallelDMPCv2, dmpc.cpp:1570-1730: N = _po.cols(), N_cmd = _pf.cols()).  State, goals, outputs, histories, status and the
// scene verdict are sized and strided by N_cmd (A agents); the tables and neighbour structures by N (T columns).  N_cmd == N: dmpc_transition.
// path != null (dmpc_transition_scripted): the N - N_cmd vehicles behind the commanded ones follow path[S][N - N_cmd][P][3]; po is then
// [S][N_cmd][3], and one launch before every step writes their columns of the current table (scripted_cols_kernel).
//
// A mission (dmpc_transition_mission; Q = 0: none): pf is ignored, the goal sets are goals [S][Q][N_cmd][3], resident for the call; stage 0's go
// into ctx->pf, and one launch after the verdict of every column (mission_stage_kernel) applies the stage rule there.
struct Mission {
    int Q = 0;
    const double *goals = nullptr;       // [S][Q][N_cmd][3]
    const int32_t *deadline = nullptr;   // [S][Q] or null
    int32_t *stage_col = nullptr;        // [S][Q] or null
    explicit operator bool() const { return Q > 0; }
};
// Hold (dmpc_transition_hold; max_hold < 0: none): an agent whose solve failed flies its previous plan, shifted, for up to max_hold consecutive
// columns (hold_kernel, between the solve and the post step of every column).  The post step is never fused into the solve launch then: the held
// plan has to be in place before the state advances.  The step's output rows alternate between two sets, so that the previous plan's v and a still
// stand in the other set after the solve; the previous positions are the agent's column of the table the step read.
struct Hold {
    int max_hold = -1;
    int32_t *hold_count = nullptr, *hold_first = nullptr;   // [S][N_cmd] or null
    int32_t *agent_status = nullptr;                        // [S][N_cmd][K_T_max] or null
    explicit operator bool() const { return max_hold >= 0; }
};

// A route (dmpc_transition_route; W = 0: none): pf is ignored, every commanded agent has waypoints of its own, resident for the call; waypoint 0 of
// every agent goes into ctx->pf, and one launch after the verdict of every column (route_kernel) applies the waypoint rule there, per agent.
// Route and mission are never both set.
// A re-planned route (dmpc_transition_replan; goals != null): no waypoints are passed; they are planned on the device before column 0 (dmpc_plan.hip)
// and, every `every` columns, planned again for the agents whose remaining legs are no longer clear, behind the waypoint rule of that column.
struct Route {
    int W = 0;
    const double *waypoints = nullptr;   // [S][N_cmd][W][3]
    const int32_t *n_wp = nullptr;       // [S][N_cmd] or null: every agent has W
    double capture = 0.0; int timeout = 0;
    int32_t *wp_col = nullptr;           // [S][N_cmd][W] or null
    int32_t *wp_index = nullptr;         // [S][N_cmd] or null
    const double *goals = nullptr;       // [S][N_cmd][3]: a re-planned route
    pln::Grid grid{}; double margin = 0.0; int every = 0, ahead = 0;   // (the grid of `cell` metres, as the entry's check made it)
    double *waypoints_out = nullptr;     // [S][N_cmd][W][3] or null: the plan in force when the scene ended
    int32_t *n_wp_out = nullptr, *plan_status = nullptr, *replan_count = nullptr, *replan_col = nullptr;   // [S][N_cmd] or null
    explicit operator bool() const { return W > 0; }
};

// one call of a transition entry, as the entry filled it
struct TransitionCall {
    int S, N, N_cmd;
    const double *po, *pf;   // (a mission: pf is its goals; a route: its waypoints)
    int K_T_max; double error_tol;
    double *pk, *vk, *ak;    // all three or none
    int32_t *K_T_used, *scene_status;
    const double *path = nullptr; int P = 0;
    Mission mission; Hold hold; Route route;
    Start start;             // the armed start, as transition_any took it from the context (dmpc_start.hip)
    int s0 = 0;              // the index in the caller's batch of scene 0 (a part of a split batch; the disturbance rule counts scenes of the call)
    // the same call for scenes [s0, s0 + sn): the one place that knows each array's stride per scene
    TransitionCall scenes(int s0, int sn) const {
        auto at = [](auto *p, size_t off) { return p ? p + off : nullptr; };
        const size_t a0 = (size_t)s0 * N_cmd, q0 = (size_t)s0 * mission.Q, h0 = a0 * (size_t)K_T_max, w0 = a0 * (size_t)route.W;
        TransitionCall c = *this; c.S = sn; c.s0 = this->s0 + s0;
        c.po = at(po, (path ? a0 : (size_t)s0 * N) * 3);   // (scripted vehicles: po covers the commanded agents)
        c.path = at(path, (size_t)s0 * (N - N_cmd) * P * 3);
        c.pk = at(pk, h0 * 3); c.vk = at(vk, h0 * 3); c.ak = at(ak, h0 * 3);
        c.K_T_used = at(K_T_used, s0); c.scene_status = at(scene_status, s0);
        c.mission.goals = at(mission.goals, q0 * N_cmd * 3); c.mission.deadline = at(mission.deadline, q0); c.mission.stage_col = at(mission.stage_col, q0);
        c.route.waypoints = at(route.waypoints, w0 * 3); c.route.n_wp = at(route.n_wp, a0); c.route.wp_col = at(route.wp_col, w0); c.route.wp_index = at(route.wp_index, a0);
        c.route.goals = at(route.goals, a0 * 3); c.route.waypoints_out = at(route.waypoints_out, w0 * 3); c.route.n_wp_out = at(route.n_wp_out, a0);
        c.route.plan_status = at(route.plan_status, a0); c.route.replan_count = at(route.replan_count, a0); c.route.replan_col = at(route.replan_col, a0);
        c.pf = mission ? c.mission.goals : route ? (route.goals ? c.route.goals : c.route.waypoints) : at(pf, a0 * 3);
        c.hold.hold_count = at(hold.hold_count, a0); c.hold.hold_first = at(hold.hold_first, a0); c.hold.agent_status = at(hold.agent_status, h0);
        c.start.vo = at(start.vo, a0 * 3); c.start.ao = at(start.ao, a0 * 3);
        c.start.plan_p = at(start.plan_p, a0 * N3); c.start.plan_v = at(start.plan_v, a0 * N3); c.start.plan_a = at(start.plan_a, a0 * N3);
        return c;
    }
};

static int group_transition(dmpc_ctx *root, const TransitionCall &c);   // (dmpc_multigpu.hip)
// what every transition entry refuses (each entry's own extras -- check_cmd, check_scripted, check_mission, max_hold -- are checked beside it)
static int check_call(dmpc_ctx *ctx, const std::string &who, const TransitionCall &c)
{
    if (c.S < 1 || c.N < 1 || c.N_cmd < 1 || c.N_cmd > c.N || c.K_T_max < 2 || !c.po || !c.pf || !c.K_T_used || !c.scene_status || ((c.pk || c.vk || c.ak) && !(c.pk && c.vk && c.ak)))
        FAIL(ctx, who + ": bad arguments");
    if (check_start_shape(ctx, who, c.S, c.N_cmd)) return -1;
    if (ctx->meas.on && !ctx->fb.on)
        FAIL(ctx, who + ": a measurement is set (dmpc_set_measurement) and no feedback policy: set one with dmpc_set_feedback (trigger (0, 0) feeds the measurement back on every column)");
    return check_disturb_shape(ctx, who, ctx->dist, c.S, c.N_cmd);
}

// The verdicts of every column and scene -- flags [K_T_max][S][2]: (reached, OR of the status bits) -- folded into what the caller gets.  The host
// looks at them in windows of `chunk` MPC steps; the first window includes the initDMPC column.
struct VerdictFold {
    static constexpr int chunk = 8;
    int S = 0, ndone = 0;
    int32_t *K_T_used = nullptr, *scene_status = nullptr;
    std::vector<int> done;
    void init(const TransitionCall &c) {
        S = c.S; ndone = 0; K_T_used = c.K_T_used; scene_status = c.scene_status; done.assign((size_t)S, 0);
        for (int s = 0; s < S; ++s) { K_T_used[s] = c.K_T_max; scene_status[s] = DMPC_ST_SOLVED; }
    }
    static bool window_ends(int k, int K_T_max) { return k % chunk == 0 || k == K_T_max - 1; }
    static int window_start(int k) { return k <= chunk ? 0 : ((k - 1) / chunk) * chunk + 1; }
    void fold(const int32_t *flags, int k0, int k1) {
        for (int kk = k0; kk <= k1; ++kk)
            for (int s = 0; s < S; ++s) {
                const int32_t reached = flags[((size_t)kk * S + s) * 2], stbits = flags[((size_t)kk * S + s) * 2 + 1];
                // some agent failed: the reference aborts the trial; else ReachedGoal.m (failure_rate.m:125)
                const int32_t over = (stbits & ~DMPC_ST_SOLVED) ? stbits : (reached ? DMPC_ST_SOLVED | DMPC_ST_REACHED : 0);
                if (over && !done[s]) { done[s] = 1; ndone++; K_T_used[s] = kk + 1; scene_status[s] = over; }
            }
    }
};

// what every transition starts from: no verdicts, no scene over, empty histories (`hist` bytes each)
static int reset_run_buffers(dmpc_ctx *ctx, int S, int K_T_max, size_t hist, hipStream_t st)
{
    HIPCHK(ctx, hipMemsetAsync(ctx->flags.p, 0, (size_t)K_T_max * S * 8, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->scene_done.p, 0, (size_t)S * 4, st));
    for (DevBuf *h : {&ctx->hist_p, &ctx->hist_v, &ctx->hist_a}) HIPCHK(ctx, hipMemsetAsync(h->p, 0, hist, st));
    return 0;
}
// the histories stay resident for dmpc_postcheck either way; the download is optional
static int download_histories(dmpc_ctx *ctx, const TransitionCall &c, size_t hist, hipStream_t st)
{
    if (!c.pk) return 0;
    HIPCHK(ctx, hipMemcpyAsync(c.pk, ctx->hist_p.p, hist, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(c.vk, ctx->hist_v.p, hist, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(c.ak, ctx->hist_a.p, hist, hipMemcpyDeviceToHost, st));
    return 0;
}

// the device side of the goals: one leg's pf (a route's waypoints: RouteDev), or a mission's goal sets and, in ctx->mis_state, every scene's stage, its first column, stage_col, deadlines
struct MissionDev {
    dmpc_ctx *ctx; const TransitionCall &c; hipStream_t st;
    int *stage_of = nullptr, *k_start = nullptr, *col = nullptr, *dl = nullptr;   // [S], [S], [S][Q], [S][Q] (null: no deadlines)
    int begin() {   // the goal sets and the deadlines go up once per call; stage 0's goals into ctx->pf; stage = k_start = 0, stage_col = -1
        if (c.route) return 0;   // (RouteDev::begin fills ctx->pf)
        const Mission &m = c.mission;
        const size_t S = (size_t)c.S, SQ = S * m.Q, set = (size_t)c.N_cmd * 24;
        if (!m) { HIPCHK(ctx, hipMemcpyAsync(ctx->pf.p, c.pf, S * set, hipMemcpyHostToDevice, st)); return 0; }
        if (ctx->pf.ensure(S * set) || ctx->mis_goals.ensure(SQ * set) || ctx->mis_state.ensure((2 * S + 2 * SQ) * 4)) FAIL(ctx, "device allocation failed");
        stage_of = ctx->mis_state.as<int>(); k_start = stage_of + S; col = k_start + S; dl = m.deadline ? col + SQ : nullptr;
        HIPCHK(ctx, hipMemcpyAsync(ctx->mis_goals.p, m.goals, SQ * set, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->pf.p, set, ctx->mis_goals.p, m.Q * set, set, S, hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemsetAsync(stage_of, 0, 2 * S * 4, st));
        HIPCHK(ctx, hipMemsetAsync(col, 0xff, SQ * 4, st));
        if (dl) HIPCHK(ctx, hipMemcpyAsync(dl, m.deadline, SQ * 4, hipMemcpyHostToDevice, st));
        return 0;
    }
    void stage(int k) {   // the stage rule on column k, behind its verdict (a first stage that is reached on the initDMPC column ends there)
        if (!c.mission) return;
        hipLaunchKernelGGL(mission_stage_kernel, dim3((unsigned)c.S), dim3(c.N_cmd * 3 >= 256 ? 256u : 64u), 0, st, c.N_cmd, c.mission.Q, k,
                           (const double *)ctx->mis_goals.as<double>(), (const int *)dl, ctx->flags.as<int>() + (size_t)k * c.S * 2,
                           ctx->scene_done.as<int>(), stage_of, k_start, col, ctx->pf.as<double>());
    }
    int finish() {
        if (c.mission.stage_col) HIPCHK(ctx, hipMemcpyAsync(c.mission.stage_col, col, (size_t)c.S * c.mission.Q * 4, hipMemcpyDeviceToHost, st));
        return 0;
    }
};

// the device side of a route: the waypoints in ctx->route_wp and, in ctx->route_state, n_wp, every agent's current waypoint, the column it became
// current on, and wp_col
struct RouteDev {
    dmpc_ctx *ctx; const TransitionCall &c; hipStream_t st;
    int *n_wp = nullptr, *cur = nullptr, *since = nullptr, *col = nullptr;   // [S][N_cmd] each, [S][N_cmd][W]
    std::vector<double> first; std::vector<int32_t> count;                    // waypoint 0 of every agent; n_wp where the caller passed none (alive until the call's last synchronisation)
    ReplanArgs rp;                                                            // a re-planned route: what its launches take (plan_status, replan_count, replan_col [S][N_cmd] behind wp_col)
    int obst_cols = 0;                                                        // ... and the columns of every path its obstacle set holds (0: static vehicles)
    void gather_obst(int k) {   // obst(k) of the rule into ctx->replan_obst
        const int M = c.N - c.N_cmd, A1 = obst_cols ? obst_cols : 1;
        hipLaunchKernelGGL(pln::replan_obst_kernel, dim3(grid_1d((size_t)c.S * A1 * M * 3, 4096)), dim3(256), 0, st, c.S, M, c.P, k, A1,
                           (const double *)(obst_cols ? ctx->path.as<double>() : nullptr), (const double *)ctx->po.as<double>(), c.N, c.N_cmd, ctx->replan_obst.as<double>());
    }
    // a re-planned route: the goals go up once per call; the plan before column 0 -- from the commanded agents' starts, packed in ctx->xp as
    // column 0 has them, round obst(0) -- writes the waypoints, n_wp, cur = since = 0, wp_col = -1 and waypoint 0 of every agent into ctx->pf
    int begin_replan() {
        const Route &r = c.route;
        const size_t A = (size_t)c.S * c.N_cmd, AW = A * r.W;
        const int M = c.N - c.N_cmd;
        obst_cols = c.path ? r.ahead + 1 : 0;
        const size_t pts = (size_t)M * (obst_cols ? obst_cols : 1);
        if (ctx->pf.ensure(A * 24) || ctx->route_wp.ensure(AW * 24) || ctx->route_state.ensure((6 * A + AW) * 4) || ctx->replan_goals.ensure(A * 24) ||
            ctx->replan_obst.ensure((size_t)c.S * pts * 24))
            FAIL(ctx, "device allocation failed");
        n_wp = ctx->route_state.as<int>(); cur = n_wp + A; since = cur + A; col = since + A;
        HIPCHK(ctx, hipMemcpyAsync(ctx->replan_goals.p, r.goals, A * 24, hipMemcpyHostToDevice, st));
        double *xp = ctx->xp.as<double>();
        if (c.start.from_end) ;   // (the carried positions stand in ctx->xp already: the commanded rows of po are ignored)
        else if (c.N_cmd == c.N || c.path) HIPCHK(ctx, hipMemcpyAsync(xp, ctx->po.p, A * 24, hipMemcpyDeviceToDevice, st));
        else HIPCHK(ctx, hipMemcpy2DAsync(xp, (size_t)c.N_cmd * 24, ctx->po.p, (size_t)c.N * 24, (size_t)c.N_cmd * 24, (size_t)c.S, hipMemcpyDeviceToDevice, st));
        rp.g = r.grid; rp.S = c.S; rp.N_cmd = c.N_cmd; rp.W = r.W; rp.M = (int)pts; rp.margin = r.margin;
        rp.x_p = xp; rp.goals = ctx->replan_goals.as<double>(); rp.obst = ctx->replan_obst.as<double>(); rp.wp = ctx->route_wp.as<double>();
        rp.n_wp = n_wp; rp.plan_status = col + AW; rp.scene_done = ctx->scene_done.as<int>();
        rp.rp.cur = cur; rp.rp.since = since; rp.rp.wp_col = col; rp.rp.pf = ctx->pf.as<double>(); rp.rp.replan_count = col + AW + A; rp.rp.replan_col = col + AW + 2 * A;
        if (replan_prepare(ctx, rp)) return -1;
        if (pts) { gather_obst(0); replan_mask(ctx, rp, st); }   // (static vehicles: the mask of the whole call)
        return replan_launch(ctx, rp, false, 0, st);
    }
    int begin() {   // the waypoints and n_wp go up once per call; waypoint 0 of every agent into ctx->pf; cur = since = 0, wp_col = -1
        const Route &r = c.route;
        if (!r) return 0;
        if (r.goals) return begin_replan();
        const size_t A = (size_t)c.S * c.N_cmd, AW = A * r.W;
        if (ctx->pf.ensure(A * 24) || ctx->route_wp.ensure(AW * 24) || ctx->route_state.ensure((3 * A + AW) * 4)) FAIL(ctx, "device allocation failed");
        n_wp = ctx->route_state.as<int>(); cur = n_wp + A; since = cur + A; col = since + A;
        first.resize(A * 3);
        for (size_t a = 0; a < A; ++a) std::memcpy(&first[a * 3], r.waypoints + a * r.W * 3, 24);
        if (!r.n_wp) count.assign(A, r.W);
        HIPCHK(ctx, hipMemcpyAsync(ctx->route_wp.p, r.waypoints, AW * 24, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->pf.p, first.data(), A * 24, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(n_wp, r.n_wp ? r.n_wp : count.data(), A * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemsetAsync(cur, 0, 2 * A * 4, st));
        HIPCHK(ctx, hipMemsetAsync(col, 0xff, AW * 4, st));
        return 0;
    }
    int rule(int k) {   // the waypoint rule on column k, behind its verdict
        if (!c.route) return 0;
        hipLaunchKernelGGL(route_kernel, dim3((unsigned)c.S), dim3(c.N_cmd * 3 >= 256 ? 256u : 64u), 0, st, c.N_cmd, c.route.W, k,
                           c.route.capture * c.route.capture, c.route.timeout, (const double *)ctx->route_wp.as<double>(), (const int *)n_wp,
                           (const double *)ctx->xp.as<double>(), ctx->flags.as<int>() + (size_t)k * c.S * 2, ctx->scene_done.as<int>(), cur, since, col,
                           ctx->pf.as<double>());
        const Route &r = c.route;
        if (!r.goals || r.every < 1 || k < 1 || k >= c.K_T_max - 1 || k % r.every || !rp.M) return 0;
        // a re-plan column: the agents of running scenes whose remaining legs are not clear on blocked(k) are planned again from where they are
        if (obst_cols) { gather_obst(k); replan_mask(ctx, rp, st); }
        return replan_launch(ctx, rp, true, k, st);
    }
    int finish() {
        const size_t A = (size_t)c.S * c.N_cmd;
        if (const Route &r = c.route; r.goals) {
            if (r.waypoints_out) HIPCHK(ctx, hipMemcpyAsync(r.waypoints_out, rp.wp, A * r.W * 24, hipMemcpyDeviceToHost, st));
            if (r.n_wp_out) HIPCHK(ctx, hipMemcpyAsync(r.n_wp_out, n_wp, A * 4, hipMemcpyDeviceToHost, st));
            if (r.plan_status) HIPCHK(ctx, hipMemcpyAsync(r.plan_status, rp.plan_status, A * 4, hipMemcpyDeviceToHost, st));
            if (r.replan_count) HIPCHK(ctx, hipMemcpyAsync(r.replan_count, rp.rp.replan_count, A * 4, hipMemcpyDeviceToHost, st));
            if (r.replan_col) HIPCHK(ctx, hipMemcpyAsync(r.replan_col, rp.rp.replan_col, A * 4, hipMemcpyDeviceToHost, st));
        }
        if (c.route.wp_col) HIPCHK(ctx, hipMemcpyAsync(c.route.wp_col, col, A * c.route.W * 4, hipMemcpyDeviceToHost, st));
        if (c.route.wp_index) HIPCHK(ctx, hipMemcpyAsync(c.route.wp_index, cur, A * 4, hipMemcpyDeviceToHost, st));
        return 0;
    }
};

// the device side of hold: run, hold_count, hold_first [S][N_cmd] and the agent_status log [S][N_cmd][K_T_max] in ctx->hold_state, and the two
// sets of p / v / a output rows that the steps alternate between (step k writes set k & 1).  Without hold both sets are the context's own rows.
struct HoldDev {
    dmpc_ctx *ctx; const TransitionCall &c; hipStream_t st;
    size_t A = 0;   // S * N_cmd
    double *outs[2][3] = {};
    int *run = nullptr, *cnt = nullptr, *first = nullptr, *log = nullptr;
    std::vector<int32_t> held;
    const double *start_va = nullptr;   // a start: its plan_v | plan_a rows, the "previous plan" of column 1
    int begin() {
        for (auto &set : outs) { set[0] = ctx->pout.as<double>(); set[1] = ctx->vout.as<double>(); set[2] = ctx->aout.as<double>(); }
        if (!c.hold) return 0;
        A = (size_t)c.S * c.N_cmd;
        if (A > 0x7fffffffu) FAIL(ctx, "dmpc_transition_hold: S * N_cmd overflows");
        const size_t row_bytes = A * N3 * 8;
        if (ctx->hold_out.ensure(3 * row_bytes) || ctx->hold_state.ensure((3 * A + A * (size_t)c.K_T_max) * 4)) FAIL(ctx, "device allocation failed");
        for (int j = 0; j < 3; ++j) outs[0][j] = ctx->hold_out.as<double>() + (size_t)j * A * N3;   // (the first step writes the context's own rows)
        run = ctx->hold_state.as<int>(); cnt = run + A; first = cnt + A; log = first + A;
        if (start_va) HIPCHK(ctx, hipMemcpyAsync(outs[0][1], start_va, 2 * row_bytes, hipMemcpyDeviceToDevice, st));
        else HIPCHK(ctx, hipMemsetAsync(outs[0][1], 0, 2 * row_bytes, st));   // the initDMPC plan: v = a = 0 (its positions are the first table)
        HIPCHK(ctx, hipMemsetAsync(cnt, 0, A * 4, st));
        HIPCHK(ctx, hipMemsetAsync(first, 0xff, A * 4, st));
        HIPCHK(ctx, hipMemsetAsync(log, 0, A * (size_t)c.K_T_max * 4, st));
        return 0;
    }
    // the hold rule on column k of the step that read `cur` and wrote `nxt`.  Column 0: every status is DMPC_ST_SOLVED -- run = 0 and the log's
    // first column, also of a scene that is over already; it stands in the set the first step writes
    void apply(int k, const double *cur, double *nxt) {
        if (!c.hold) return;
        const int set = k ? k & 1 : 1;
        double **out = outs[set], **prev = outs[set ^ 1];   // the previous plan's v, a stand in the other set
        hipLaunchKernelGGL(hold_kernel, dim3((unsigned)((A + 63) / 64)), dim3(64), 0, st, (int)A, c.N_cmd, c.N, c.K_T_max, k, c.hold.max_hold, ctx->prm.h,
                           ctx->prm.alim, cur, nxt, (const double *)prev[1], (const double *)prev[2], out[0], out[1], out[2], ctx->status.as<int>(),
                           (const int *)ctx->scene_done.as<int>(), run, log, cnt, first);
    }
    int finish() {   // the downloads, in front of the call's last synchronisation ...
        if (!c.hold) return 0;
        held.resize(A);
        HIPCHK(ctx, hipMemcpyAsync(held.data(), cnt, A * 4, hipMemcpyDeviceToHost, st));
        if (c.hold.hold_first) HIPCHK(ctx, hipMemcpyAsync(c.hold.hold_first, first, A * 4, hipMemcpyDeviceToHost, st));
        if (c.hold.agent_status) HIPCHK(ctx, hipMemcpyAsync(c.hold.agent_status, log, A * (size_t)c.K_T_max * 4, hipMemcpyDeviceToHost, st));
        return 0;
    }
    void report() {   // ... and behind it (every hold the device recorded stands on a column < K_T_used: the steps behind a scene's end skip it)
        for (size_t a = 0; a < A; ++a)
            if (held[a] > 0) c.scene_status[a / (size_t)c.N_cmd] |= DMPC_ST_HELD;
        if (c.hold.hold_count) std::memcpy(c.hold.hold_count, held.data(), A * 4);
    }
};

// the device side of a disturbance (dmpc_disturb.hip): the wind, the sorted pushes and the offsets of this call's scenes go up once per call
struct DisturbDev {
    dmpc_ctx *ctx; const TransitionCall &c; hipStream_t st;
    DisturbArgs args{};
    explicit operator bool() const { return ctx->dist.on; }
    int begin() {
        if (!ctx->dist.on) return 0;
        ctx->dist_key = -1;   // (dmpc_disturb_device's upload does not survive this one)
        if (disturb_upload(ctx, c.s0, c.S, c.N_cmd, st)) return -1;
        args = disturb_args(ctx, c.s0);
        return 0;
    }
};

// the device side of a feedback policy (dmpc_feedback.hip), live only next to a disturbance or a measurement (without either e stays 0 and the
// flight is the plain one): the planning state and the error in ctx->fb_x, the event record, the log; with a measurement also the belief in
// ctx->est_x and dmpc_estimate_log's log.  The solver's io.x_p / x_v point at xh; everything else keeps
// reading the true state in ctx->xp / xv / xa.
struct FeedbackDev {
    dmpc_ctx *ctx; const TransitionCall &c; hipStream_t st;
    size_t A = 0;
    const int *col0 = nullptr;   // a start: the caller's number of every scene's column 0 (the measurement's stream counts from it, as the disturbance's does)
    explicit operator bool() const { return ctx->fb.on && (ctx->dist.on || ctx->meas.on); }
    bool measured() const { return ctx->fb.on && ctx->meas.on; }
    double *x(int u) const { return ctx->fb_x.as<double>() + (size_t)u * A * 3; }   // xh_p, xh_v, e_p, e_v
    // column 0, behind whatever set its true state: xh = x, e = 0; no event yet; the log's column 0 (deviation 0)
    int begin(const double *xp, const double *xv) {
        ctx->fb_flight = FeedbackFlight{ctx->fb.on, (bool)*this, c.S, c.N_cmd, measured()};
        if (!*this) return 0;
        A = (size_t)c.S * c.N_cmd;
        if (ctx->fb_x.ensure(4 * A * 24) || ctx->fb_g.ensure(A * 48) || ctx->fb_ev.ensure(A * 4) || ctx->fb_logi.ensure(5 * A * 4) || ctx->fb_logd.ensure(2 * A * 8))
            FAIL(ctx, "device allocation failed");
        HIPCHK(ctx, hipMemcpyAsync(x(0), xp, A * 24, hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(x(1), xv, A * 24, hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemsetAsync(x(2), 0, 2 * A * 24, st));
        HIPCHK(ctx, hipMemsetAsync(ctx->fb_ev.p, 0, A * 4, st));
        int *li = ctx->fb_logi.as<int>();
        HIPCHK(ctx, hipMemsetAsync(li, 0, 5 * A * 4, st));             // count, (first, last), p_col, v_col
        HIPCHK(ctx, hipMemsetAsync(li + A, 0xff, 2 * A * 4, st));      // first = last = -1
        HIPCHK(ctx, hipMemsetAsync(ctx->fb_logd.p, 0, 2 * A * 8, st));
        if (!measured()) return 0;
        if (ctx->est_x.ensure(2 * A * 24) || ctx->est_logi.ensure(4 * A * 4) || ctx->est_logd.ensure(4 * A * 8)) FAIL(ctx, "device allocation failed");
        HIPCHK(ctx, hipMemsetAsync(ctx->est_x.p, 0, 2 * A * 24, st));   // eh = 0; the log's column 0 (error 0, deviation 0)
        HIPCHK(ctx, hipMemsetAsync(ctx->est_logi.p, 0, 4 * A * 4, st));
        HIPCHK(ctx, hipMemsetAsync(ctx->est_logd.p, 0, 4 * A * 8, st));
        return 0;
    }
    // the post step of column k on the step's rows `out`, then the re-anchoring of `nxt` and of the v rows
    void post(const DisturbArgs &D, int k, double **out, double *nxt, double *xp, double *xv, double *xa, int *verdict_k) {
        const Feedback &f = ctx->fb;
        int *li = ctx->fb_logi.as<int>(); double *ld = ctx->fb_logd.as<double>();
        if (measured()) {   // the rule decides on the estimate; gh stands in the event record
            const Measurement &m = ctx->meas;
            const EstimateArgs E{D, ctx->dist.on ? 1 : 0, m.seed, m.amp_p, m.amp_v, m.gain_p, m.gain_v, c.s0, col0, ctx->prm.h, f.trigger_p, f.trigger_v,
                                 (const int *)ctx->status.as<int32_t>(), A, x(0), ctx->est_x.as<double>(), ctx->fb_g.as<double>(), ctx->fb_ev.as<int>(), li, ld,
                                 ctx->est_logi.as<int>(), ctx->est_logd.as<double>()};
            hipLaunchKernelGGL(post_step_estimate_kernel, dim3((unsigned)c.S), dim3(c.N_cmd >= 256 ? 256 : 128), 0, st, E, c.N_cmd, c.K_T_max, k, c.error_tol,
                               (const double *)out[0], (const double *)out[1], (const double *)out[2], xp, xv, xa, (const double *)ctx->pf.as<double>(),
                               ctx->hist_p.as<double>(), ctx->hist_v.as<double>(), ctx->hist_a.as<double>(), verdict_k, ctx->scene_done.as<int>(),
                               (const int *)ctx->scene_done.as<int>());
        } else {
            const FeedbackArgs F{D, f.trigger_p, f.trigger_v, (const int *)ctx->status.as<int32_t>(), x(0), x(1), x(2), x(3), ctx->fb_g.as<double>(), ctx->fb_ev.as<int>(),
                                 li, li + A, li + 2 * A, li + 3 * A, li + 4 * A, ld, ld + A};
            hipLaunchKernelGGL(post_step_feedback_kernel, dim3((unsigned)c.S), dim3(c.N_cmd >= 256 ? 256 : 128), 0, st, F, c.N_cmd, c.K_T_max, k, c.error_tol,
                               (const double *)out[0], (const double *)out[1], (const double *)out[2], xp, xv, xa, (const double *)ctx->pf.as<double>(),
                               ctx->hist_p.as<double>(), ctx->hist_v.as<double>(), ctx->hist_a.as<double>(), verdict_k, ctx->scene_done.as<int>(),
                               (const int *)ctx->scene_done.as<int>());
        }
        if (f.reanchor)   // (a scene that stopped before this column kept the flag of an earlier one: no scene_done here, which column k has just set)
            hipLaunchKernelGGL(reanchor_kernel, dim3(grid_1d(A * N3, 4096)), dim3(256), 0, st, c.S, c.N, c.N_cmd, k, ctx->prm.h, (const int *)ctx->fb_ev.as<int>(),
                               (const double *)ctx->fb_g.as<double>(), (const int *)nullptr, nxt, out[1]);
    }
};

static int transition_one(dmpc_ctx *ctx, const TransitionCall &c)
{
    const int S = c.S, N = c.N, N_cmd = c.N_cmd, K_T_max = c.K_T_max;
    const bool scripted = c.path != nullptr, mixed = (ctx->precision & DMPC_PREC_MIXED) != 0;   // mixed: the scan of every step reads an fp32 copy of the current table
    // ---- begin: allocation, uploads, resets
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t A = (size_t)S * N_cmd, T = (size_t)S * N, hist = A * (size_t)K_T_max * 24;
    if (ensure_step_scratch(ctx, T, A)) return -1;
    if (ctx->lT2.ensure(T * N3 * 8) || ctx->po.ensure(T * 24) || ctx->hist_p.ensure(hist) || ctx->hist_v.ensure(hist) ||
        ctx->hist_a.ensure(hist) || ctx->flags.ensure((size_t)K_T_max * S * 8) || ctx->scene_done.ensure((size_t)S * 4))
        FAIL(ctx, "device allocation failed");
    hipStream_t st = ctx->stream;
    double *xp = ctx->xp.as<double>(), *xv = ctx->xv.as<double>(), *xa = ctx->xa.as<double>();
    if (scripted) {   // the paths go up once per call
        const size_t path_bytes = (T - A) * (size_t)c.P * 24;
        if (ctx->path.ensure(path_bytes)) FAIL(ctx, "device allocation failed");
        HIPCHK(ctx, hipMemcpyAsync(ctx->path.p, c.path, path_bytes, hipMemcpyHostToDevice, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->po.p, c.po, (scripted ? A : T) * 24, hipMemcpyHostToDevice, st));
    MissionDev mission{ctx, c, st}; HoldDev hold{ctx, c, st}; RouteDev route{ctx, c, st}; DisturbDev disturb{ctx, c, st}; FeedbackDev feedback{ctx, c, st};
    StartDev start{ctx, c.start, st};
    if (start && start.begin(S, N_cmd)) return -1;
    if (c.start.from_end) HIPCHK(ctx, hipMemcpyAsync(xp, start.x(0), A * 24, hipMemcpyDeviceToDevice, st));   // (in front of a re-planned route's first plan)
    if (mission.begin() || route.begin() || disturb.begin()) return -1;
    if (start && disturb) disturb.args.col0 = start.col0();
    if (start) feedback.col0 = start.col0();
    if (reset_run_buffers(ctx, S, K_T_max, hist, st)) return -1;
    // ---- column 0: initDMPC (dmpc_soft_bound.m:117-121): state = (po, 0, 0), table = straight lines
    // (a start, dmpc_start.hip: state = (po, vo, ao) or the carried one, the commanded columns of the table = the start's plan rows)
    if (c.start.from_end) ;   // (the carried positions: copied above)
    else if (N_cmd == N || scripted) HIPCHK(ctx, hipMemcpyAsync(xp, ctx->po.p, A * 24, hipMemcpyDeviceToDevice, st));
    else HIPCHK(ctx, hipMemcpy2DAsync(xp, (size_t)N_cmd * 24, ctx->po.p, (size_t)N * 24, (size_t)N_cmd * 24, (size_t)S, hipMemcpyDeviceToDevice, st));   // the commanded agents' starts, packed
    const double *rows0 = ctx->rows.as<double>();
    if (start) {
        if (start.states(xv, xa) || start.plans(xp, xv, xa)) return -1;
        rows0 = start.plan(0);
        if (c.hold) hold.start_va = start.plan(1);
        else {   // the plan column 0 was built from, where a step's would stand: the end of a scene that ends here
            HIPCHK(ctx, hipMemcpyAsync(ctx->vout.p, start.plan(1), A * N3 * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(ctx->aout.p, start.plan(2), A * N3 * 8, hipMemcpyDeviceToDevice, st));
        }
    } else {
        for (double *x : {xv, xa}) HIPCHK(ctx, hipMemsetAsync(x, 0, A * 24, st));
        hipLaunchKernelGGL(init_rows_kernel, dim3((unsigned)((A * N3 + 255) / 256)), dim3(256), 0, st, (int)A, ctx->prm.h,
                           (const double *)(N_cmd == N ? ctx->po.as<double>() : xp), ctx->pf.as<double>(), ctx->rows.as<double>());
    }
    if (N_cmd == N) {
        if (dmpc_table_from_rows_device(ctx, S, 1, N, rows0, ctx->lT.as<double>(), st)) return -1;
    } else {
        // the commanded columns of the first table from the initDMPC rows; the static columns -- po replicated over the horizon (dmpc.cpp:1633-1649)
        // -- into BOTH tables of the ping-pong pair, once: the solve kernels write the columns of the agents they solved and nothing else
        hipLaunchKernelGGL(cmd_cols_from_rows_kernel, dim3(grid_1d(A * N3, 4096)), dim3(256), 0, st, S, N, N_cmd, rows0, ctx->lT.as<double>());
        if (!scripted)   // (scripted vehicles: their columns are written before every step, the first included -- window k = 1 of the first table)
            hipLaunchKernelGGL(static_cols_kernel, dim3(grid_1d((T - A) * N3, 4096)), dim3(256), 0, st, S, N, N_cmd, (const double *)ctx->po.as<double>(),
                               ctx->lT.as<double>(), ctx->lT2.as<double>());
    }
    if (feedback.begin(xp, xv)) return -1;
    hipLaunchKernelGGL(record_kernel, dim3((unsigned)((A * 3 + 255) / 256)), dim3(256), 0, st, S, N_cmd, K_T_max, 0, xp, xv, xa, ctx->hist_p.as<double>(),
                       ctx->hist_v.as<double>(), ctx->hist_a.as<double>());
    // ReachedGoal is also evaluated on the initDMPC column (failure_rate.m:125 runs after k = 1 as well)
    HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->status.p, DMPC_ST_SOLVED, A, st));
    hipLaunchKernelGGL(scene_reduce_kernel, dim3((unsigned)S), dim3(256), 0, st, N_cmd, c.error_tol, xp, ctx->pf.as<double>(),
                       (const int *)ctx->status.as<int32_t>(), ctx->flags.as<int>(), ctx->scene_done.as<int>());
    mission.stage(0);
    if (route.rule(0)) return -1;
    double *cur = ctx->lT.as<double>(), *nxt = ctx->lT2.as<double>();
    if (hold.begin()) return -1;
    hold.apply(0, cur, nxt);
    ctx->post_acc_S = 0;   // the scene accumulators of the fused post-step start from zero in every transition
    // The host looks at the per-step verdicts every VerdictFold::chunk MPC steps -- one window BEHIND the steps it enqueues: the verdicts of
    // window c are copied to pinned host memory behind an event, the steps of window c+1 are enqueued, and only then the host waits for the
    // event of window c.  The device never idles while the host reads flags (a stream synchronisation per window cost 40-45 us of idle GPU per
    // 8 steps: 8 % of a single-scene transition); the steps enqueued past the end of a trial are skipped on the device (scene_done), so
    // what a scene records and reports does not change.
    HIPCHK(ctx, ctx->flag_win.ensure((size_t)K_T_max * S * 2));
    VerdictFold verdict; verdict.init(c);
    int pend_k0 = -1, pend_k1 = -1, pend_ev = 0, nwin = 0;   // the window whose verdicts are in flight to the host
    auto digest = [&]() -> int {   // wait for the pending window and fold its verdicts
        if (pend_k0 < 0) return 0;
        HIPCHK(ctx, hipEventSynchronize(ctx->flag_win.ev[pend_ev]));
        verdict.fold(ctx->flag_win.p, pend_k0, pend_k1); pend_k0 = -1;
        return 0;
    };
    // ---- columns 1 .. K_T_max - 1
    for (int k = 1; k < K_T_max && verdict.ndone < S; ++k) {
        if (scripted && start)   // (a start: the window of scene s begins at its column col0[s] + k-1)
            hipLaunchKernelGGL(scripted_cols_from_kernel, dim3(grid_1d((T - A) * N3, 4096)), dim3(256), 0, st, S, N, N_cmd, c.P, k, start.col0(), (const double *)ctx->path.as<double>(), cur);
        else if (scripted)   // the scripted columns of the current table: window k-1 .. k+K-2 of every path (before the fp32 copy, which then covers them)
            hipLaunchKernelGGL(scripted_cols_kernel, dim3(grid_1d((T - A) * N3, 4096)), dim3(256), 0, st, S, N, N_cmd, c.P, k, (const double *)ctx->path.as<double>(), cur, (float *)nullptr);
        if (mixed && table_f32(ctx, cur, ctx->lTf, T * N3, st)) return -1;   // (all N columns, the static ones included)
        int *const verdict_k = ctx->flags.as<int>() + (size_t)k * S * 2;
        const PostStep post{K_T_max, k, c.error_tol, xp, xv, xa, ctx->hist_p.as<double>(), ctx->hist_v.as<double>(), ctx->hist_a.as<double>(), verdict_k, ctx->scene_done.as<int>()};
        double **out = hold.outs[k & 1];
        StepIO io = scratch_io(ctx);   // (xp, xv, xa, the goals and the status are the scratch's; a closed loop takes no info)
        io.lT = cur; io.lT_next = nxt; io.info = nullptr;
        if (feedback) { io.x_p = feedback.x(0); io.x_v = feedback.x(1); }   // (the solver starts from the planning state)
        io.p_out = out[0]; io.v_out = out[1]; io.a_out = out[2];
        io.scene_done = ctx->scene_done.as<int>(); io.lTf = mixed ? ctx->lTf.as<float>() : nullptr; io.post = c.hold || disturb || feedback ? nullptr : &post;   // (hold, a disturbance, a live policy: the post step is a launch of its own)
        const StepShape sh{S, /*G*/ 1, /*C*/ N, /*g_local*/ 0, /*c_first*/ 0, /*c_count*/ N_cmd};
        if (launch_step(ctx, sh, io, st)) return -1;
        hold.apply(k, cur, nxt);
        // state advance + history column + scene verdict in one launch (unless the solve kernel did them: tiny launches)
        if (feedback)   // ... with the feedback rule, the disturbance of column k inside it, between the advance and the record
            feedback.post(disturb.args, k, out, nxt, xp, xv, xa, verdict_k);
        else if (disturb)   // ... with the disturbance of column k between the advance and the record
            hipLaunchKernelGGL(post_step_disturbed_kernel, dim3((unsigned)S), dim3(N_cmd >= 256 ? 256 : 128), 0, st, disturb.args, N_cmd, K_T_max, k, c.error_tol,
                               (const double *)out[0], (const double *)out[1], (const double *)out[2],
                               (const int *)ctx->status.as<int32_t>(), xp, xv, xa, (const double *)ctx->pf.as<double>(), ctx->hist_p.as<double>(),
                               ctx->hist_v.as<double>(), ctx->hist_a.as<double>(), verdict_k, ctx->scene_done.as<int>(), (const int *)ctx->scene_done.as<int>());
        else if (!ctx->post_fused)
            hipLaunchKernelGGL(post_step_kernel, dim3((unsigned)S), dim3(N_cmd >= 256 ? 256 : 128), 0, st, N_cmd, K_T_max, k, c.error_tol,
                               (const double *)out[0], (const double *)out[1], (const double *)out[2],
                               (const int *)ctx->status.as<int32_t>(), xp, xv, xa, (const double *)ctx->pf.as<double>(), ctx->hist_p.as<double>(),
                               ctx->hist_v.as<double>(), ctx->hist_a.as<double>(), verdict_k, ctx->scene_done.as<int>(), (const int *)ctx->scene_done.as<int>());
        mission.stage(k);
        if (route.rule(k)) return -1;
        HIPCHK(ctx, hipGetLastError());
        std::swap(cur, nxt);   // l = new_l (dmpc_soft_bound.m:146)
        if (VerdictFold::window_ends(k, K_T_max)) {
            if (digest()) return -1;   // the window before this one (its steps ran while this one was enqueued)
            const int k0 = VerdictFold::window_start(k);
            HIPCHK(ctx, hipMemcpyAsync(&ctx->flag_win.p[(size_t)k0 * S * 2], ctx->flags.as<int>() + (size_t)k0 * S * 2, (size_t)(k - k0 + 1) * S * 8, hipMemcpyDeviceToHost, st));
            pend_ev = nwin++ & 1;
            HIPCHK(ctx, hipEventRecord(ctx->flag_win.ev[pend_ev], st));
            pend_k0 = k0; pend_k1 = k;
        }
    }
    // ---- end: the last window, the downloads
    if (digest()) return -1;
    if (download_histories(ctx, c, hist, st) || mission.finish() || route.finish() || hold.finish()) return -1;
    HIPCHK(ctx, hipStreamSynchronize(st));
    hold.report();
    ctx->hist_S = S; ctx->hist_N = N_cmd; ctx->hist_KT = K_T_max;   // (the resident histories are the commanded agents')
    // the end of this flight stands in the step scratch until something else uses it (dmpc_flight_end, a from_end start)
    FlightEnd &end = ctx->end;
    end.S = S; end.N = N; end.N_cmd = N_cmd; end.hold = (bool)c.hold; end.e0_zero = !c.hold && !start;
    end.last.resize((size_t)S); end.status.assign(c.scene_status, c.scene_status + S); start.cols(end.col0, S);
    for (int s = 0; s < S; ++s) end.last[s] = c.K_T_used[s] - 1;
    end.valid = true;
    return 0;
}

// development options of a context handed to a context it creates for itself (further parts of a split batch, the second group)
static void copy_debug_options(dmpc_ctx *dst, const dmpc_ctx *src)
{
    for (const DevOptionEntry &t : dev_options)
        if (t.inherited) dst->opt.*(t.member) = src->opt.*(t.member);   // (each member as its own value: grid_min_part too)
    for (dmpc_ctx *pc : dst->peers) copy_debug_options(pc, src);
    for (dmpc_ctx *ch : dst->children) copy_debug_options(ch, src);
}

// children[i] of ctx, ready to run a part of a split batch: created on `device` if it is not there yet (DMPC_DEVICE_ALL: a second set of rank contexts,
// threads and streams on the same GPUs), with ctx's development options (its rank contexts too), never splitting itself, with ctx's current parameters
static int part_context(dmpc_ctx *ctx, size_t i, int device)
{
    const bool group = device == DMPC_DEVICE_ALL;
    const std::string what = group ? "dmpc_transition: second group: " : "dmpc_transition: further context: ";
    while (ctx->children.size() <= i) {
        const int keep = g_emulate_devices.load();
        if (group && ctx->grp_emulated) g_emulate_devices.store(ctx->grp->G);
        dmpc_ctx *ch = dmpc_create(&ctx->prm, device, ctx->precision);
        if (group) g_emulate_devices.store(keep);
        if (ch && group && (!ch->grp || ch->grp->G != ctx->grp->G)) { dmpc_destroy(ch); ch = nullptr; }
        if (!ch) FAIL(ctx, what + g_err);
        copy_debug_options(ch, ctx);
        ch->opt.no_split = 1; ctx->children.push_back(ch);
    }
    dmpc_ctx *ch = ctx->children[i];
    ch->dist = ctx->dist; ch->fb = ctx->fb; ch->meas = ctx->meas;
    if (std::memcmp(&ch->prm, &ctx->prm, sizeof(dmpc_params)) != 0 && dmpc_set_params(ch, &ctx->prm)) FAIL(ctx, what + ch->err);
    return 0;
}

// part i of a split batch -- scenes [at[i], at[i + 1]) -- through `body` on its own context (0: ctx, i > 0: children[i - 1]) and host thread
static int run_parts(dmpc_ctx *ctx, const TransitionCall &c, const std::vector<int> &at, int (*body)(dmpc_ctx *, const TransitionCall &))
{
    const size_t parts = at.size() - 1;
    std::vector<int> rc(parts, 0);
    auto run = [&](size_t i) { rc[i] = body(i ? ctx->children[i - 1] : ctx, c.scenes(at[i], at[i + 1] - at[i])); };
    std::vector<std::thread> th;
    for (size_t i = 1; i < parts; ++i) th.emplace_back(run, i);
    run(0);
    for (auto &t : th) t.join();
    (void)hipSetDevice(ctx->device);
    for (size_t i = 1; i < parts; ++i)
        if (rc[i]) FAIL(ctx, ctx->children[i - 1]->err);
    if (rc[0]) return -1;
    ctx->split_at = at; ctx->hist_S = c.S;   // the resident histories are split over the contexts (dmpc_postcheck knows)
    return 0;
}

// Batched transitions are bound, MPC step by MPC step, by the slowest agent of the whole batch while most of the GPU idles.  Scenes are independent,
// so a large batch is run in parts side by side: the tail of one part overlaps the bulk of another (512 transitions of 100 agents, two halves: 103 ->
// 60 ms).  Launches of fewer than ~2000 agents are one-agent workgroups, which the hardware interleaves across streams freely (persistent launches
// hold a CU's whole LDS), so many small parts overlap best.  sharded (a DMPC_DEVICE_ALL context): batches of 64 or more scenes as TWO groups -- while
// one half's ranks exchange their predictions the other half's solve kernels keep the GPUs busy.  want: option split_parts.  Returns every part's first scene, and S.
static std::vector<int> batch_parts(int S, int want, bool sharded)
{
    const int parts = sharded ? (want > 0 ? std::min(want, 2) : (S >= 64 ? 2 : 1)) : std::min(S, want > 0 ? want : (S >= 128 ? 4 : (S >= 32 ? 2 : 1)));
    std::vector<int> at((size_t)parts + 1);
    for (int i = 0; i <= parts; ++i) at[(size_t)i] = (int)((long)S * i / parts);
    return at;
}

// A batch in parts (batch_parts), each on a context, HIP stream and host thread of its own.  A DMPC_DEVICE_ALL context shards the agents of each scene
// over every visible GPU (dmpc_multigpu.hip) -- unless there are uncommanded vehicles, a mission, a route, a disturbance, a feedback policy or a start, or fewer agents than twice the GPUs (the
// reference's small swarms on an 8-GPU node: sharding N = 4 agents over 8 GPUs is impossible and over 2-3 of them nothing but barriers and peer
// copies): the first GPU alone then, unsplit, as dmpc_step_batch does.
static int transition_any(dmpc_ctx *ctx, const TransitionCall &call)
{
    ctx->split_at.clear();
    ctx->end.valid = false;   // (transition_one sets it again; a sharded flight leaves no end)
    ctx->fb_flight.valid = false;   // (likewise: dmpc_feedback_log)
    TransitionCall c = call;
    // the armed start is consumed here: every entry has passed its own checks (a from_end start was snapshotted in the parts of the flight it
    // continues, so it is flown in those parts -- or, snapshotted whole, unsplit)
    StartState &a = ctx->start;
    std::vector<int> start_at;
    if (a.armed) {
        auto ptr = [](const std::vector<double> &v) { return v.empty() ? nullptr : v.data(); };
        c.start = Start{true, a.from_end, a.col0, ptr(a.vo), ptr(a.ao), ptr(a.plan_p), ptr(a.plan_v), ptr(a.plan_a)};
        if (a.from_end) start_at = a.at.empty() ? std::vector<int>{0, c.S} : a.at;
        a.armed = false;
    }
    const bool sharded = ctx->grp && c.N_cmd == c.N && !c.mission && !c.route && !ctx->dist.on && !ctx->fb.on && !c.start;
    if (sharded && c.N < 2 * ctx->grp->G) return transition_one(ctx, c);
    int (*const body)(dmpc_ctx *, const TransitionCall &) = sharded ? group_transition : transition_one;
    const std::vector<int> at = start_at.empty() ? batch_parts(c.S, ctx->opt.split_parts, sharded) : start_at;
    if (at.size() < 3 || (ctx->opt.no_split && start_at.empty()) || (ctx->grp && !sharded)) return body(ctx, c);
    for (size_t i = 0; i + 2 < at.size(); ++i)
        if (part_context(ctx, i, sharded ? DMPC_DEVICE_ALL : ctx->device)) return -1;
    if (run_parts(ctx, c, at, body)) { ctx->end.valid = false; return -1; }
    return 0;
}

extern "C" int dmpc_transition(dmpc_ctx *ctx, int S, int N, const double *po, const double *pf, int K_T_max, double error_tol, double *pk, double *vk,
                               double *ak, int32_t *K_T_used, int32_t *scene_status)
{
    if (!ctx) { g_err = "dmpc_transition: ctx is NULL"; return -1; }
    const TransitionCall c{S, N, N, po, pf, K_T_max, error_tol, pk, vk, ak, K_T_used, scene_status};
    return check_call(ctx, "dmpc_transition", c) ? -1 : transition_any(ctx, c);
}

// DMPC::solveParallelDMPCv2 (dmpc.cpp:1570-1730) with N_cmd = _pf.cols() < N = _po.cols(): the uncommanded vehicles are static columns of the table
extern "C" int dmpc_transition_cmd(dmpc_ctx *ctx, int S, int N, int N_cmd, const double *po, const double *pf, int K_T_max, double error_tol,
                                   double *pk, double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status)
{
    if (!ctx) { g_err = "dmpc_transition_cmd: ctx is NULL"; return -1; }
    if (check_cmd(ctx, "dmpc_transition_cmd", S, N, N_cmd)) return -1;
    const TransitionCall c{S, N, N_cmd, po, pf, K_T_max, error_tol, pk, vk, ak, K_T_used, scene_status};
    return check_call(ctx, "dmpc_transition_cmd", c) ? -1 : transition_any(ctx, c);
}

// Scripted vehicles: the uncommanded vehicles of dmpc_transition_cmd MOVE along paths the caller knows.  No reference counterpart
// (DMPC::solveParallelDMPCv2 freezes uncommanded vehicles, dmpc.cpp:1633-1649); a commanded agent sees such a column as it sees any neighbour.
static int check_scripted(dmpc_ctx *ctx, const char *entry, int S, int N_cmd, int M, int P)
{
    if (S < 1) FAIL(ctx, std::string(entry) + ": S must be >= 1");
    if (N_cmd < 1) FAIL(ctx, std::string(entry) + ": N_cmd must be >= 1 (commanded agents first, scripted vehicles behind them)");
    if (M < 1) FAIL(ctx, std::string(entry) + ": M must be >= 1 (no scripted vehicle: use the entry without them)");
    if (P < 1) FAIL(ctx, std::string(entry) + ": P must be >= 1 (every path has at least its start)");
    if ((long)N_cmd + M > 0x7fffffffL) FAIL(ctx, std::string(entry) + ": N_cmd + M overflows");
    return 0;
}

extern "C" int dmpc_transition_scripted(dmpc_ctx *ctx, int S, int N_cmd, int M, int P, const double *po, const double *pf, const double *path,
                                        int K_T_max, double error_tol, double *pk, double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status)
{
    if (!ctx) { g_err = "dmpc_transition_scripted: ctx is NULL"; return -1; }
    if (check_scripted(ctx, "dmpc_transition_scripted", S, N_cmd, M, P)) return -1;
    if (!path) FAIL(ctx, "dmpc_transition_scripted: path is NULL");
    if ((pk || vk || ak) && !(pk && vk && ak)) FAIL(ctx, "dmpc_transition_scripted: pk, vk, ak must be all given or all NULL");
    const TransitionCall c{S, N_cmd + M, N_cmd, po, pf, K_T_max, error_tol, pk, vk, ak, K_T_used, scene_status, path, P};
    return check_call(ctx, "dmpc_transition_scripted", c) ? -1 : transition_any(ctx, c);   // (a DMPC_DEVICE_ALL context: N_cmd < N, its first GPU)
}

// Missions: a transition through a sequence of goal sets.  No reference counterpart (the reference flies one leg); the step is the
// reference's, the stage rule the loop a caller of dmpc_step_batch[_cmd] could write on the host -- applied on the device after the verdict of
// every column (mission_stage_kernel), so that the host keeps reading the verdicts one window behind.
// the shared argument check of dmpc_transition_mission and dmpc_transition_hold
static int check_mission(dmpc_ctx *ctx, const std::string &who, const TransitionCall &c)
{
    const int S = c.S, Q = c.mission.Q;
    if (check_cmd(ctx, who.c_str(), S, c.N, c.N_cmd)) return -1;
    if (Q < 1) FAIL(ctx, who + ": Q must be >= 1 (a mission has at least one stage)");
    if (!c.mission.goals) FAIL(ctx, who + ": goals is NULL");
    if (c.path && check_scripted(ctx, who.c_str(), S, c.N_cmd, c.N - c.N_cmd, c.P)) return -1;
    if ((c.pk || c.vk || c.ak) && !(c.pk && c.vk && c.ak)) FAIL(ctx, who + ": pk, vk, ak must be all given or all NULL");
    if (check_call(ctx, who, c)) return -1;
    if ((size_t)S * (size_t)Q > 0x7fffffffu) FAIL(ctx, who + ": S * Q overflows");
    if (const int32_t *deadline = c.mission.deadline)
        for (int s = 0; s < S; ++s) {
            for (int q = 0; q < Q; ++q)
                if (deadline[(size_t)s * Q + q] < 0) FAIL(ctx, who + ": a deadline is negative (0: none)");
            if (deadline[(size_t)s * Q + Q - 1] != 0) FAIL(ctx, who + ": the last stage's deadline must be 0 (the last stage ends the trial when it is reached)");
        }
    return 0;
}

extern "C" int dmpc_transition_mission(dmpc_ctx *ctx, int S, int N, int N_cmd, int Q, const double *po, const double *goals, const int32_t *deadline,
                                       const double *path, int P, int K_T_max, double error_tol, double *pk, double *vk, double *ak,
                                       int32_t *K_T_used, int32_t *scene_status, int32_t *stage_col)
{
    if (!ctx) { g_err = "dmpc_transition_mission: ctx is NULL"; return -1; }
    const TransitionCall c{S, N, N_cmd, po, goals, K_T_max, error_tol, pk, vk, ak, K_T_used, scene_status, path, path ? P : 0, Mission{Q, goals, deadline, stage_col}};
    return check_mission(ctx, "dmpc_transition_mission", c) ? -1 : transition_any(ctx, c);   // (a DMPC_DEVICE_ALL context: its first GPU)
}

// Hold policy: dmpc_transition_mission in which an agent whose solve failed flies its previous plan while the scene goes on.  No reference
// counterpart (the reference's failure-rate experiment stops the trial); the rule is in include/dmpc_hip.h, the device side is hold_kernel.
extern "C" int dmpc_transition_hold(dmpc_ctx *ctx, int S, int N, int N_cmd, int Q, const double *po, const double *goals, const int32_t *deadline,
                                    const double *path, int P, int K_T_max, double error_tol, int max_hold, double *pk, double *vk, double *ak, int32_t *K_T_used,
                                    int32_t *scene_status, int32_t *stage_col, int32_t *hold_count, int32_t *hold_first, int32_t *agent_status)
{
    if (!ctx) { g_err = "dmpc_transition_hold: ctx is NULL"; return -1; }
    const TransitionCall c{S, N, N_cmd, po, goals, K_T_max, error_tol, pk, vk, ak, K_T_used, scene_status, path, path ? P : 0,
                           Mission{Q, goals, deadline, stage_col}, Hold{max_hold, hold_count, hold_first, agent_status}};
    if (check_mission(ctx, "dmpc_transition_hold", c)) return -1;
    if (max_hold < 0) FAIL(ctx, "dmpc_transition_hold: max_hold must be >= 0 (0: no agent is ever held, dmpc_transition_mission)");
    return transition_any(ctx, c);   // (a DMPC_DEVICE_ALL context: its first GPU)
}

// Routes: every commanded agent through waypoints of its own, switched per agent on the device.  No reference counterpart (DMPC has no global
// planner: an agent whose straight line is blocked by uncommanded vehicles parks in front of them); the step is the reference's, the rule -- pinned
// in include/dmpc_hip.h -- the loop a caller of dmpc_step_batch[_cmd] could write on the host, applied after the verdict of every column (route_kernel).
extern "C" int dmpc_transition_route(dmpc_ctx *ctx, int S, int N, int N_cmd, int W, const double *po, const double *waypoints, const int32_t *n_wp,
                                     double capture, int timeout, const double *path, int P, int K_T_max, double error_tol, int max_hold, double *pk,
                                     double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status, int32_t *wp_col, int32_t *wp_index,
                                     int32_t *hold_count, int32_t *hold_first, int32_t *agent_status)
{
    const std::string who = "dmpc_transition_route";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    TransitionCall c{S, N, N_cmd, po, waypoints, K_T_max, error_tol, pk, vk, ak, K_T_used, scene_status, path, path ? P : 0, Mission{},
                     Hold{max_hold, hold_count, hold_first, agent_status}};
    c.route = Route{W, waypoints, n_wp, capture, timeout, wp_col, wp_index};
    if (check_cmd(ctx, who.c_str(), S, N, N_cmd)) return -1;
    if (W < 1) FAIL(ctx, who + ": W must be >= 1 (every agent has at least its goal)");
    if (!waypoints) FAIL(ctx, who + ": waypoints is NULL");
    if (path && check_scripted(ctx, who.c_str(), S, N_cmd, N - N_cmd, P)) return -1;
    if ((pk || vk || ak) && !(pk && vk && ak)) FAIL(ctx, who + ": pk, vk, ak must be all given or all NULL");
    if (check_call(ctx, who, c)) return -1;
    if ((size_t)S * (size_t)N_cmd * (size_t)W > 0x7fffffffu) FAIL(ctx, who + ": S * N_cmd * W overflows");
    if (!(capture > 0.0)) FAIL(ctx, who + ": capture must be > 0 (metres)");
    if (timeout < 0) FAIL(ctx, who + ": timeout is negative (0: none)");
    if (max_hold < 0) FAIL(ctx, who + ": max_hold must be >= 0 (0: no agent is ever held)");
    if (n_wp)
        for (size_t a = 0; a < (size_t)S * N_cmd; ++a)
            if (n_wp[a] < 1 || n_wp[a] > W) FAIL(ctx, who + ": an n_wp entry is outside 1 .. W");
    return transition_any(ctx, c);   // (a DMPC_DEVICE_ALL context: its first GPU)
}

// Re-planned routes: dmpc_plan_routes before column 0, dmpc_transition_route from there, and every `every` columns the agents whose remaining legs are
// no longer clear planned again on the device, from where they are, round the vehicles where they are (the rule is pinned in include/dmpc_hip.h;
// the kernels are dmpc_plan.hip's).  No reference counterpart.
extern "C" int dmpc_transition_replan(dmpc_ctx *ctx, int S, int N, int N_cmd, int W, const double *po, const double *goals, double cell, double margin,
                                      int every, int ahead, double capture, int timeout, const double *path, int P, int K_T_max, double error_tol,
                                      int max_hold, double *pk, double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status, double *waypoints_out,
                                      int32_t *n_wp_out, int32_t *plan_status, int32_t *wp_col, int32_t *wp_index, int32_t *replan_count,
                                      int32_t *replan_col, int32_t *hold_count, int32_t *hold_first, int32_t *agent_status)
{
    const std::string who = "dmpc_transition_replan";
    if (!ctx) { g_err = who + ": ctx is NULL"; return -1; }
    TransitionCall c{S, N, N_cmd, po, goals, K_T_max, error_tol, pk, vk, ak, K_T_used, scene_status, path, path ? P : 0, Mission{},
                     Hold{max_hold, hold_count, hold_first, agent_status}};
    c.route = Route{W, nullptr, nullptr, capture, timeout, wp_col, wp_index, goals, pln::Grid{}, margin, every, ahead, waypoints_out, n_wp_out, plan_status,
                    replan_count, replan_col};
    if (check_cmd(ctx, who.c_str(), S, N, N_cmd)) return -1;
    if (W < 1) FAIL(ctx, who + ": W must be >= 1 (every agent has at least its goal)");
    if (!goals) FAIL(ctx, who + ": goals is NULL");
    if (path && check_scripted(ctx, who.c_str(), S, N_cmd, N - N_cmd, P)) return -1;
    if ((pk || vk || ak) && !(pk && vk && ak)) FAIL(ctx, who + ": pk, vk, ak must be all given or all NULL");
    if (check_call(ctx, who, c)) return -1;
    if ((size_t)S * (size_t)N_cmd * (size_t)W > 0x7fffffffu) FAIL(ctx, who + ": S * N_cmd * W overflows");
    if (!(capture > 0.0)) FAIL(ctx, who + ": capture must be > 0 (metres)");
    if (timeout < 0) FAIL(ctx, who + ": timeout is negative (0: none)");
    if (max_hold < 0) FAIL(ctx, who + ": max_hold must be >= 0 (0: no agent is ever held)");
    if (every < 0) FAIL(ctx, who + ": every is negative (0: the plan of column 0 is flown to the end)");
    if (ahead < 0) FAIL(ctx, who + ": ahead is negative (0: the vehicles where they are on the column)");
    if ((double)(N - N_cmd) * ((double)ahead + 1.0) * (double)S > (double)0x7fffffff / 3) FAIL(ctx, who + ": S * (N - N_cmd) * (ahead + 1) overflows");
    if (plan_check(ctx, who.c_str(), S, N_cmd, 0, W, po, goals, nullptr, cell, margin, c.route.grid)) return -1;
    return transition_any(ctx, c);   // (a DMPC_DEVICE_ALL context: its first GPU)
}

// the fill of dmpc_transition_scripted for callers that loop over dmpc_step_device_cmd themselves
extern "C" int dmpc_scripted_cols_device(dmpc_ctx *ctx, int S, int N, int N_cmd, int P, const double *path_dev, int k, double *lT, float *lTf, void *stream)
{
    if (!ctx) { g_err = "dmpc_scripted_cols_device: ctx is NULL"; return -1; }
    if (check_cmd(ctx, "dmpc_scripted_cols_device", S, N, N_cmd)) return -1;
    if (check_scripted(ctx, "dmpc_scripted_cols_device", S, N_cmd, N - N_cmd, P)) return -1;
    if (k < 1) FAIL(ctx, "dmpc_scripted_cols_device: k must be >= 1 (the MPC step that produces history column k)");
    if (!path_dev || !lT) FAIL(ctx, "dmpc_scripted_cols_device: NULL pointer");
    if (ctx->grp) FAIL(ctx, "dmpc_scripted_cols_device: device pointers belong to ONE GPU; a DMPC_DEVICE_ALL context drives several (use the host-pointer entry points)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(scripted_cols_kernel, dim3(grid_1d((size_t)S * (N - N_cmd) * N3, 4096)), dim3(256), 0, (hipStream_t)stream, S, N, N_cmd, P, k, path_dev, lT, lTf);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}
