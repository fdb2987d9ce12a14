// dmpc_context.hip -- a context and its life (host code only; the first part dmpc_api.hip includes behind the kernels): the owner types, the group's
// shared block, the development options and their table, dmpc_ctx, FAIL / HIPCHK, create, destroy, set_params, the profile and the error and count
// readers.  There is deliberately NO CPU fallback anywhere in the library: without a HIP device every compute entry point fails with an error.
// One ownership rule: whatever a context holds on a device or pinned is a member that frees itself (DevBuf, PinnedInts, EvList), and dmpc_destroy
// selects the context's device before it deletes the context.  A new resource is a new member of one of these types, never a line in dmpc_destroy.

using namespace dmpc;

static thread_local std::string g_err;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) return -1;
        cap = bytes;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    ~DevBuf() { release(); }   // every buffer of a context goes with it (dmpc_destroy selects the device first)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    template <class T> T *as() const { return (T *)p; }
};

// A pinned int32 array and a pair of untimed events: the window through which a loop on the host reads what the device decided, one window behind
// the launches it enqueues (transition_one's verdicts, the auction's done flags).  Goes with its context, under DevBuf's rule: the device is current
struct PinnedInts {
    int32_t *p = nullptr; size_t cap = 0;   // cap: ints
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t ensure(size_t ints)
    {
        if (cap < ints) {
            if (p) (void)hipHostFree(p);
            p = nullptr; cap = 0;
            const hipError_t e = hipHostMalloc((void **)&p, ints * 4, hipHostMallocDefault);
            if (e != hipSuccess) return e;
            cap = ints;
        }
        for (hipEvent_t &e : ev) {
            const hipError_t r = e ? hipSuccess : hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    ~PinnedInts() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); if (p) (void)hipHostFree(p); }
    PinnedInts() = default;
    PinnedInts(const PinnedInts &) = delete;
    PinnedInts &operator=(const PinnedInts &) = delete;
};

// The profile's event triples (step start | scan+order done | solve tiers done), in flight or pooled; same rule
struct Ev { hipEvent_t t0, t1, t2; };
struct EvList : std::vector<Ev> {
    ~EvList() { for (Ev &ev : *this) { (void)hipEventDestroy(ev.t0); (void)hipEventDestroy(ev.t1); (void)hipEventDestroy(ev.t2); } }
};

// One process, several GPUs (dmpc_create(prm, DMPC_DEVICE_ALL, ..)): what the sub-contexts of a group share -- a host barrier for
// their threads, the pointers each rank publishes for the per-step exchange, and the events that order the peer copies.
struct GroupShared {
    int G = 1;
    std::atomic<int> arrived{0};
    std::atomic<int> phase{0};
    std::atomic<int> abort{0};          // a rank failed: everybody leaves the barriers with an error instead of waiting forever
    std::vector<double *> next_ptr;     // [G] table the rank reads in the NEXT step (peers write their chunks into it)
    std::vector<int *> fall_ptr;        // [G] the rank's gathered scene verdicts
    std::vector<int> dev;               // [G] HIP device of the rank
    std::vector<hipEvent_t> ev;         // [G][2] "rank's copies of this step are enqueued", alternating
    double *hist_dst[3] = {nullptr, nullptr, nullptr};   // rank 0's scene-wide history arrays (gather_histories)
    ~GroupShared() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }   // (dmpc_destroy deletes it with the root's device current)
    // sense-reversing spin barrier of the G rank threads; false: the group was aborted
    bool wait()
    {
        const int ph = phase.load(std::memory_order_acquire);
        if (arrived.fetch_add(1, std::memory_order_acq_rel) == G - 1) {
            arrived.store(0, std::memory_order_relaxed);
            phase.store(ph + 1, std::memory_order_release);
        } else {
            int spins = 0;
            while (phase.load(std::memory_order_acquire) == ph) {
                if (abort.load(std::memory_order_relaxed)) return false;
                if (++spins > 256) std::this_thread::yield();
            }
        }
        return !abort.load(std::memory_order_relaxed);
    }
};

// Development / test options of a context (dmpc_debug_option; the table of their names is dev_options below).  They select launch forms and
// tiers, never arithmetic.
struct DevOptions {
    int no_fuse = 0;         // development option no_fuse: always launch post_step_kernel
    int no_persist = 0;      // development option no_persist: one-agent-per-workgroup solve launches
    int force_persist = 0;   // development option force_persist (tests): the persistent kernel on small launches
    int cull_min = 256;      // development option cull_min: neighbour lists from this many agents per scene on
    int order_slices = 0;    // development option order_slices: workgroups of the order kernel (0: by launch size)
    int no_cull = 0;         // development option no_cull: no neighbour lists in the scan of large scenes (A/B runs, tests)
    int no_lpt = 0;          // development option no_lpt: no heaviest-first solve order
    int order_hint = 0;      // option order_hint = 1: the launch order also uses the agents' work estimates of the context's previous step (measured: no gain in
                             // closed loops -- the heavy agents of a step are not the heavy agents of the step before -- so off; a replay of ONE step would flatter it)
    int crash_min = CRASH_MIN_DEFAULT;   // see StepParams::crash_min (development option crash_min; crash_any: also for the slack-free variants)
    int crash_any = 0;
    int pivot_explore = 0;   // development option pivot_explore (DMPC_PIVOT_EXPLORE builds)
    int no_fast_exit = 0;    // development option no_fast_exit (tests): every agent through the solve kernel (the unconstrained exit of the scan off)
    int iter_cap = ITER_CAP; // development option iter_cap: cap of the active-set iterations (agents beyond it end DMPC_ST_ITERCAP)
    int tier1_env = 0;       // development option tier1_qcap (tests): 32 = two tiers for the slack variants (any value: no shallow-launch shortcut)
    int split_parts = 0;     // development option split_parts: number of parts (0: the built-in rule)
    int no_split = 0;        // development option no_split
    int reduced_solver = 1;  // solveSoftDMPCbound: the reduced solver (dmpc_rsolve.hip) in front of the general one; 0: the general solver alone (A/B runs, tests)
    int rsolve_cap = 0;      // development option rsolve_cap: the reduced solver hands an agent over after this many equality solves of a ladder level (0: its default; tests of the hand-over)
    int no_split_t = 0;      // development option no_split_t: slack-free persistent solve with the whole inverse factor in every wave's block (nine waves per CU; A/B runs, tests)
    int grid_min = 768;      // development option grid_min: cell-grid neighbour lists from this many agents per scene on (below: nbr_kernel) ...
    int grid_min_part = 2048; // ... and when the query covers only a PART of the scene's agents (a rank's chunk: the grid is still built over all of them)
    int prep_fuse = 1;       // development option prep_fuse: 0 = the cell grid of a single scene by the five kernels of round 4 instead of grid_prep_kernel + grid_fill2_kernel
    int grid_cells = -1;     // development option grid_cells: row of plan_lists' cell geometries (0 = the cells of rounds 4-6: R x 1.5 R x 1.5 R c, at most 32 per axis; 1, 2, 3 finer; other values: the default row)
    int list_cap = 0;        // development option list_cap (tests): at most this many entries per neighbour list, in multiples of 64 (0: the built-in rule -- which never goes below the scene's agent count, so a full list needs this option)
    int nbr_grid = 1;        // development option nbr_grid: 0 = neighbour lists of large scenes from the all-pairs box test of round 3 (nbr_kernel) instead of the cell grid + distance filter
    int no_level_skip = 0;   // development option no_level_skip (see StepParams)
    int no_level_check = 0;  // development option no_level_check (see StepParams)
    int lds_pad_kb = 0;      // development option lds_pad_kb: KB of unused LDS per one-agent solve workgroup (occupancy experiments: fewer resident agents per CU)
    int f32_dep_exp = 8;     // development option f32_dep_exp: fp32-factor kernels treat a pivot as dependent below delta / s_pp = 10^-n
    int ext_cap = 0;         // development option ext_cap (tests): at most this many T extensions per workgroup (1: every agent that needs one waits for the same slot)
    int queue_chunk = 0;     // development option queue_chunk: positions per ticket of the persistent queue's light bulk (0: chosen per launch)
    int static_queue = 0;    // development option static_queue: persistent waves take queue positions round-robin instead of by ticket
    int close_pairs = 1;     // development option close_pairs: 0 = the scan walks its neighbour list for the pairs inside rmin instead of taking them from the grid query (A/B runs, tests)
    int close_cap = 64;      // development option close_cap: (neighbour, step) pairs the query records per agent; an agent with more falls back to the walk (tests)
    int clear_chunk = 8;     // development option clear_chunk: 100 Hz samples per workgroup of the clearance searches (dmpc_postcheck_clearance; tests)
    int setpoint_batch = 0;  // development option setpoint_batch: 100 Hz samples per staging pass of dmpc_postcheck_setpoints (0: the 256 MB rule; tests)
};

// dmpc_set_disturbance's copy of the descriptor (dmpc_disturb.hip); the pushes sorted by (scene, agent, column), stable
struct Disturbance {
    bool on = false;
    uint64_t seed = 0;
    double amp_p = 0.0, amp_v = 0.0;
    int wind_scenes = 0;
    std::vector<double> wind;      // [wind_scenes][3]
    std::vector<dmpc_push> push;
    void set(const dmpc_disturbance &d);
};

// dmpc_set_feedback's copy of the policy (dmpc_feedback.hip), and what the last flight left for dmpc_feedback_log
struct Feedback {
    bool on = false;
    double trigger_p = 0.0, trigger_v = 0.0;
    int reanchor = 0;
};
struct FeedbackFlight {
    bool valid = false, live = false;   // valid: the flight had a policy; live: ... and a disturbance or a measurement, so the loop kept xh, e and the log (else xh = x, e = 0, no event)
    int S = 0, N_cmd = 0;
    bool measured = false;              // ... and a measurement: the loop also kept the belief and dmpc_estimate_log's log
};
// dmpc_set_measurement's copy of the measurement model (dmpc_feedback.hip)
struct Measurement {
    bool on = false;
    uint64_t seed = 0;
    double amp_p = 0.0, amp_v = 0.0, gain_p = 1.0, gain_v = 1.0;
};

// dmpc_set_start's armed start (dmpc_start.hip).  Host form: copies of the caller's arrays, uploaded by the flight that consumes it.  from_end: the
// snapshot stands in the context's start_x / start_plan already (a split flight: in every part's context), `col` is each scene's column 0
struct StartState {
    bool armed = false, from_end = false;
    int S = 0, N_cmd = 0, col0 = 0;
    std::vector<double> vo, ao, plan_p, plan_v, plan_a;   // [S][N_cmd][3], [S][N_cmd][3K]; empty: absent
    std::vector<int32_t> col;                             // from_end: [S] of this context's scenes
    std::vector<int> at;                                  // from_end of a split flight: the parts it was snapshotted in
};
// the end of the context's last flight (transition_one): what dmpc_flight_end and a from_end start read of the step scratch
struct FlightEnd {
    bool valid = false, hold = false, e0_zero = false;    // e0_zero: a scene that ended on column 0 has the initDMPC plan's v = a = 0 (nothing wrote them)
    int S = 0, N = 0, N_cmd = 0;
    std::vector<int32_t> last, status, col0;              // [S]: K_T_used - 1, scene_status, the caller's number of column 0
};

struct dmpc_ctx {
    int device = 0;
    int precision = DMPC_PREC_F64;   // DMPC_PREC_MIXED: fp32 table / scan / rows, fp64 QP (host-pointer entry points)
    hipStream_t stream = nullptr;
    dmpc_params prm{};
    DevBuf d_tables;              // [3][900] Gram tables + [225] Lambda' table (dmpc_device.h: TAB_DOUBLES), then the inverse factors (upload_tables)
    double hsum[3] = {0, 0, 0};   // per cost case: sum of |H1(i,j)| (dual-bound certificate of the slack-free variants)
    std::string err;
    int num_cu = 0;
    DevOptions opt;          // development options (dmpc_debug_option)
    // the step (dmpc_launch.hip, dmpc_step.hip): launch limits and records, the scan -> solve hand-off, scratch of the host-pointer entry points
    int64_t solves = 0;
    int max_lds_scp = 0;
    int max_lds_set = 0;
    int max_lds_persist = 0;
    DevBuf post_acc; int post_acc_S = 0, post_fused = 0;
    DevBuf rowbuf, rowkc, hdr, order, counter, flag_list, scene_done;
    DevBuf prev_cost;        // [S * c_count] work estimates of the previous step (solve kernel -> order kernel)
    long prev_cost_shape = -1;
    int single_tier = 0;         // 1: solve with the full working-set capacity in one launch
    DevBuf lTf, lTf2;            // mixed precision: fp32 copies of the tables the scan reads
    DevBuf rows, lT, lT2, xp, xv, xa, pf, po, pout, vout, aout, status, info;
    std::string last_kernel; // the solve kernel the last step launched for the bulk of its agents (dmpc_last_solve_kernel)
    int rsolve_blocks = 0;   // workgroups of dmpc_rsolve_persist_kernel a CU holds (occupancy query, once per context)
    // neighbour lists (dmpc_lists.hip)
    DevBuf bbox, bbox_nm, nbr_list, nbr_cnt, lrow;
    DevBuf close_list, close_cnt;   // the query's close pairs (StepParams::close_list)
    int max_lds_fill2 = 0;   // dynamic-LDS limit grid_fill2_kernel was last raised to (build_neighbour_lists)
    bool grid_clean = false; // the cell grid's counters were left zero by the last scan launch (grid_clean_key: for which buffer / size)
    unsigned long long grid_clean_key = 0;
    DevBuf grid;             // cell grid of the neighbour lists (counts, starts, entries)
    struct ListsBuilt {      // the last list build, for dmpc_debug_read_grid (S = 0: none yet)
        int S = 0, G = 0, C = 0, n[3] = {0, 0, 0}, ncell = 0, build = 0, cap = 0, close_cap = 0, agents = 0, parts = 0;
        const int *maxhalf = nullptr, *start = nullptr; const void *ent = nullptr;   // inside `grid`
        bool armed = false;      // dmpc_debug_read_grid was called on this context: builds from now on keep a copy of their half extents
        bool kept = false;       // ... and the last one did (the two-launch build's are set back to zero by the step's scan kernel)
    } lists_built;
    DevBuf maxhalf_kept;     // [S][3][3], filled right after grid_prep_kernel / grid_bin_kernel on an armed context
    // the transition and its modes (dmpc_transition.hip, dmpc_disturb.hip)
    DevBuf hist_p, hist_v, hist_a, flags;
    int hist_S = 0, hist_N = 0, hist_KT = 0;   // shape of the histories left resident by the last dmpc_transition
    PinnedInts flag_win;                        // the per-step verdicts of dmpc_transition, a window behind the steps
    std::vector<dmpc_ctx *> children;   // further contexts (own stream and buffers) for the other parts of a split batch of transitions
    std::vector<int> split_at;          // non-empty: the last dmpc_transition left scenes [split_at[i], split_at[i+1]) in part i (0: here, i > 0: children[i-1])
    DevBuf path;                                                           // dmpc_transition_scripted: the scripted vehicles' paths [S][M][P][3], resident for the call
    DevBuf hold_out, hold_state;                                           // dmpc_transition_hold: the second set of p / v / a output rows 3 x [S][N_cmd][3K]; ints: run, hold_count, hold_first [S][N_cmd] each, agent_status [S][N_cmd][K_T_max]
    DevBuf mis_goals, mis_state;                                           // dmpc_transition_mission: goal sets [S][Q][N_cmd][3]; ints: stage [S], k_start [S], stage_col [S][Q], deadline [S][Q]
    DevBuf route_wp, route_state;                                          // dmpc_transition_route: waypoints [S][N_cmd][W][3]; ints: n_wp, cur, since [S][N_cmd] each, wp_col [S][N_cmd][W]
    Disturbance dist;                                                      // dmpc_set_disturbance: the disturbance in force (children of a split batch get a copy per call)
    DevBuf dist_buf; std::vector<unsigned char> dist_stage; long dist_key = -1;   // ... of a call on the device: wind | sorted pushes | offsets [S * N_cmd + 1]; its host staging; the shape dmpc_disturb_device uploaded for
    // event-triggered feedback (dmpc_feedback.hip)
    Feedback fb;                                                           // dmpc_set_feedback: the policy in force (children of a split batch get a copy per call)
    FeedbackFlight fb_flight;                                              // what dmpc_feedback_log reads of the last flight
    Measurement meas;                                                      // dmpc_set_measurement: the measurement model in force (children of a split batch get a copy per call)
    DevBuf est_x, est_logi, est_logd;                                      // of a measured flight: the belief eh_p | eh_v [S][N_cmd][3] each; dmpc_estimate_log's log: err_p_col, err_v_col, dev_p_col, dev_v_col [S][N_cmd] each; err_p_max, err_v_max, dev_p_max, dev_v_max [S][N_cmd] each
    DevBuf fb_x, fb_g, fb_ev, fb_logi, fb_logd;                            // of a flight: xh_p | xh_v | e_p | e_v [S][N_cmd][3] each; the event record g_p | g_v [S][N_cmd][6] (also dmpc_feedback_device's) and its flag [S][N_cmd]; the log: count, first, last, p_col, v_col [S][N_cmd] each; p_max, v_max [S][N_cmd] each
    // a flight's start and end (dmpc_start.hip)
    StartState start; FlightEnd end; std::vector<int32_t> start_src_host;                                       // dmpc_set_start: the armed start; the end of the last flight, valid until the step scratch is used again
    DevBuf start_x, start_plan, start_col, end_x, end_plan, end_src;       // a start on the device: x_p | x_v | x_a, plan_p | plan_v | plan_a rows, col0 [S]; dmpc_flight_end's gather; (source scene, last column) [S][2]
    // goal assignment (dmpc_assign.hip)
    DevBuf asg_io, asg_work;                                               // dmpc_assign_goals / _rect: staged inputs / outputs of the host forms; scratch of the round launches
    PinnedInts asg_win;                                                    // the scenes' done flags of two windows of rounds
    int max_lds_assign[2] = {0, 0};   // dynamic-LDS limit assign_one_kernel<SWAP> was last raised to
    // route planning (dmpc_plan.hip)
    DevBuf plan_io, plan_mask;                                             // dmpc_plan_routes: staged inputs / outputs of the host form; the scenes' blocked bitmasks
    int max_lds_plan = 0;    // dynamic-LDS limit plan_route_kernel was last raised to
    DevBuf replan_work, replan_obst, replan_goals;                         // re-planning: blocked bitmasks | flagged list | count; the obstacle points of a column; dmpc_transition_replan's goals
    int max_lds_replan = 0;  // dynamic-LDS limit replan_route_kernel was last raised to
    // the post-checks (dmpc_postcheck_host.hip)
    int pc_fallback_scenes = 0;   // last dmpc_postcheck: scenes of a cell-grid search that were searched again by brute force
    DevBuf pc_p, pc_v, pc_a, pc_M, pc_w, pc_scene, pc_agent, pc_interp;   // post-check work buffers
    DevBuf pc_static;                                                      // post-check: positions of the uncommanded vehicles + their per-scene minimum
    DevBuf pc_sc_path, pc_sc_y, pc_sc_M, pc_sc_w, pc_sc_pts, pc_sc_interp; // dmpc_postcheck_scripted: paths, knots, second derivatives, scratch, sample batch, p_scripted
    DevBuf pc_pts, pc_cell, pc_fill, pc_start, pc_sorted, pc_on;           // post-check, large scenes: cell grid of a batch of samples
    DevBuf pc_cl_part, pc_cl_run, pc_cl_out;                               // dmpc_postcheck_clearance: partials of a sample batch, running best, report
    DevBuf pc_Mv, pc_Ma, pc_sp_stage, pc_sp_part, pc_sp_run, pc_sp_out;    // dmpc_postcheck_setpoints: second derivatives of the v / a splines, staged setpoints of a pass, peak partials, running peaks, report
    // multi-GPU (dmpc_multigpu.hip): RCCL communicator of this rank, exchange buffers
    void *comm = nullptr;
    int nranks = 1, rank = 0;
    DevBuf sendbuf, sendbuf32, own64, mg_pf, mg_floc, mg_fall, full_p, full_v, full_a, gath;
    // one process, several GPUs: this context is rank `rank` of the group `grp`; the context the caller holds (rank 0) owns
    // the others (`peers`, ranks 1..G-1) and the shared block
    GroupShared *grp = nullptr;
    std::vector<dmpc_ctx *> peers;
    long grp_steps = 0;      // exchanges of this rank so far (parity of the event pair)
    int grp_emulated = 0;    // the group's ranks share one device (dmpc_debug_emulate_devices): a second group is built the same way
    int debug_rank = 0;      // dmpc_debug_set_rank: emulated rank without a transport (tests)
    // dense row builders, generators and helpers (dmpc_hostforms.hip): staging of the host-pointer entries
    DevBuf rb_A, rb_l, rb_sel, rb_out, rb_bin, rb_po, gen_out, hp_in, hp_out;
    // development aids (dmpc_debug.hip)
    DevBuf dbg; int dbg_agent = -1, dbg_cap = 0;              // development trace (dmpc_debug_trace); null unless armed
    DevBuf forced_order; int forced_n = 0;                    // development aid (dmpc_debug_set_order)
    // the profile (dmpc_profile, launch_step)
    int profile = 0;
    EvList events, ev_pool;
    double prof_scan_ms_sum = 0.0;
    double prof_ms_sum = 0.0;
    int64_t prof_n = 0;
};

// workgroups of 256 threads for n elements of a grid-stride kernel, at most cap
static unsigned grid_1d(size_t n, size_t cap) { return (unsigned)std::min((n + 255) / 256, cap); }

#define FAIL(ctx, msg)                                   \
    do {                                                 \
        std::string m_ = (msg);                          \
        if (ctx) (ctx)->err = m_;                        \
        g_err = m_;                                      \
        return -1;                                       \
    } while (0)
#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) FAIL(ctx, std::string(#call) + ": " + hipGetErrorString(e_));       \
    } while (0)

static int check_params(const dmpc_params *p, std::string &why)
{
    if (!p) { why = "params is NULL"; return -1; }
    if (p->K != K) { why = "only K = k_hor = 15 is supported (the value every reference script uses)"; return -1; }
    if (p->order != 2 && !(p->order == 4 && (p->variant == DMPC_VAR_SOFTALL || p->variant == DMPC_VAR_SOFTALL_C || p->variant == DMPC_VAR_ELLIP || p->variant == DMPC_VAR_REPAIR || p->variant == DMPC_VAR_CPP1))) {
        why = "ellipsoid order must be 2, or 4 with solveSoftDMPC / solveEllipDMPC / solveSoftDMPCrepair / DMPC::solveQP (test/comp_test_ellipconstr.m:158)"; return -1;
    }
    if (p->variant < 0 || p->variant > DMPC_VAR_SCP) { why = "unknown variant"; return -1; }
    if (p->variant == DMPC_VAR_SCP && !(p->tol >= 0)) { why = "solveDMPC: tol must be >= 0"; return -1; }
    if (!(p->h > 0) || !(p->rmin > 0) || !(p->c > 0) || !(p->alim > 0)) { why = "h, rmin, c, alim must be positive"; return -1; }
    for (int d = 0; d < 3; ++d)
        if (!(p->pmax[d] > p->pmin[d])) { why = "pmax must exceed pmin"; return -1; }
    return 0;
}

static void build_tables(const dmpc_params &p, double *t, double hsum[3]);   // dmpc_tables.hip

// the device tables of the context's parameters (the layout: dmpc_device.h)
static int upload_tables(dmpc_ctx *ctx)
{
    std::vector<double> t(TAB_ALL_DOUBLES);
    build_tables(ctx->prm, t.data(), ctx->hsum);
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_tables.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" const char *dmpc_last_error(const dmpc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }
extern "C" int dmpc_abi_version(void) { return DMPC_ABI_VERSION; }
extern "C" const char *dmpc_last_solve_kernel(const dmpc_ctx *ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }

static std::atomic<int> g_emulate_devices{0};
// development / tests (not in the public header): DMPC_DEVICE_ALL then builds a group of n ranks that all sit on the calling thread's
// current device -- the single-process multi-GPU path (threads, peer copies, events) on a box with ONE GPU.  n = 0: off.
extern "C" int dmpc_debug_emulate_devices(int n)
{
    if (n < 0 || n > 64) return -1;
    g_emulate_devices.store(n);
    return 0;
}

// Development / test options of a context (not in the public header; nothing in the library reads the environment per call).  They select
// launch forms and tiers, never arithmetic: every combination returns the same bits (tests/test_gpu_paths.py).  A process can preset them for
// the contexts it creates with ONE environment variable, DMPC_DEBUG_OPTIONS="name=value,name=value" (the probes under tools/).
// One table of the options: the name dmpc_debug_option takes, the member, and whether a context hands its value to the contexts it creates for
// itself (copy_debug_options).  split_parts and no_split describe the splitting itself and stay with their context.
struct DevOptionEntry { const char *name; int DevOptions::*member; bool inherited; };
static const DevOptionEntry dev_options[] = {
    {"no_fuse", &DevOptions::no_fuse, true}, {"no_persist", &DevOptions::no_persist, true}, {"force_persist", &DevOptions::force_persist, true}, {"no_cull", &DevOptions::no_cull, true},
    {"order_slices", &DevOptions::order_slices, true}, {"cull_min", &DevOptions::cull_min, true}, {"no_lpt", &DevOptions::no_lpt, true}, {"order_hint", &DevOptions::order_hint, true},
    {"crash_min", &DevOptions::crash_min, true}, {"crash_any", &DevOptions::crash_any, true}, {"no_fast_exit", &DevOptions::no_fast_exit, true}, {"pivot_explore", &DevOptions::pivot_explore, true},
    {"iter_cap", &DevOptions::iter_cap, true}, {"tier1_qcap", &DevOptions::tier1_env, true}, {"split_parts", &DevOptions::split_parts, false}, {"no_split", &DevOptions::no_split, false},
    {"no_level_skip", &DevOptions::no_level_skip, true}, {"prep_fuse", &DevOptions::prep_fuse, true}, {"static_queue", &DevOptions::static_queue, true}, {"queue_chunk", &DevOptions::queue_chunk, true},
    {"no_split_t", &DevOptions::no_split_t, true}, {"ext_cap", &DevOptions::ext_cap, true}, {"nbr_grid", &DevOptions::nbr_grid, true}, {"f32_dep_exp", &DevOptions::f32_dep_exp, true},
    {"grid_min", &DevOptions::grid_min, true}, {"grid_min_part", &DevOptions::grid_min_part, true}, {"no_level_check", &DevOptions::no_level_check, true}, {"lds_pad_kb", &DevOptions::lds_pad_kb, true},
    {"reduced_solver", &DevOptions::reduced_solver, true}, {"rsolve_cap", &DevOptions::rsolve_cap, true}, {"clear_chunk", &DevOptions::clear_chunk, true},
    {"setpoint_batch", &DevOptions::setpoint_batch, true},
    {"close_pairs", &DevOptions::close_pairs, true}, {"close_cap", &DevOptions::close_cap, true}, {"grid_cells", &DevOptions::grid_cells, true}, {"list_cap", &DevOptions::list_cap, true}};

extern "C" int dmpc_debug_option(dmpc_ctx *ctx, const char *name, int value)
{
    if (!ctx || !name) return -1;
    for (const DevOptionEntry &t : dev_options)
        if (!std::strcmp(t.name, name)) {
            ctx->opt.*(t.member) = value;
            if (t.member == &DevOptions::grid_min) ctx->opt.grid_min_part = value;   // (the option forces the grid for every query from that size on; grid_min_part after it: that threshold alone)
            for (dmpc_ctx *pc : ctx->peers) (void)dmpc_debug_option(pc, name, value);
            for (dmpc_ctx *ch : ctx->children) (void)dmpc_debug_option(ch, name, value);
            return 0;
        }
    ctx->err = std::string("dmpc_debug_option: unknown option ") + name;
    return -1;
}
static void options_from_env(dmpc_ctx *ctx)
{
    const char *e = getenv("DMPC_DEBUG_OPTIONS");
    if (!e) return;
    std::string all(e);
    size_t pos = 0;
    while (pos < all.size()) {
        size_t end = all.find(',', pos);
        if (end == std::string::npos) end = all.size();
        const std::string item = all.substr(pos, end - pos);
        const size_t eq = item.find('=');
        if (eq != std::string::npos) (void)dmpc_debug_option(ctx, item.substr(0, eq).c_str(), atoi(item.c_str() + eq + 1));
        pos = end + 1;
    }
}

static dmpc_ctx *create_one(const dmpc_params *prm, int device, int precision)
{
    if (hipSetDevice(device) != hipSuccess) { g_err = "dmpc_create: hipSetDevice failed"; return nullptr; }
    dmpc_ctx *ctx = new dmpc_ctx();
    ctx->device = device;
    ctx->precision = precision;
    ctx->prm = *prm;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        ctx->d_tables.ensure(sizeof(double) * TAB_ALL_DOUBLES) != 0 || upload_tables(ctx) != 0) {
        g_err = "dmpc_create: device initialisation failed: " + ctx->err;
        dmpc_destroy(ctx);
        return nullptr;
    }
    if (hipDeviceGetAttribute(&ctx->num_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ctx->num_cu = 0;
    options_from_env(ctx);
    return ctx;
}

// every GPU of devs, one process: rank r of the group on device devs[r] (the reference's thread clusters, dmpc.cpp:1600-1625, one GPU each)
static dmpc_ctx *create_group(const dmpc_params *prm, const std::vector<int> &devs, int precision, bool emulated)
{
    const int G = (int)devs.size();
    GroupShared *sh = new GroupShared();
    sh->G = G; sh->dev = devs;
    sh->next_ptr.assign((size_t)G, nullptr); sh->fall_ptr.assign((size_t)G, nullptr);
    sh->ev.assign((size_t)G * 2, nullptr);
    dmpc_ctx *root = nullptr;
    bool ok = true;
    for (int r = 0; r < G && ok; ++r) {
        dmpc_ctx *c = create_one(prm, devs[(size_t)r], precision);
        if (!c) { ok = false; break; }
        c->grp = sh; c->nranks = G; c->rank = r; c->grp_emulated = emulated;
        if (r == 0) root = c; else root->peers.push_back(c);
        for (int u = 0; u < 2 && ok; ++u) ok = hipEventCreateWithFlags(&sh->ev[(size_t)r * 2 + u], hipEventDisableTiming) == hipSuccess;
        // direct loads / stores and copies between the GPUs of the group over xGMI
        for (int q = 0; q < G && ok; ++q)
            if (devs[(size_t)q] != devs[(size_t)r]) {
                const hipError_t pe = hipDeviceEnablePeerAccess(devs[(size_t)q], 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();   // copies still work (staged)
            }
    }
    if (!ok) {
        if (g_err.empty()) g_err = "dmpc_create: group initialisation failed";
        if (root) dmpc_destroy(root); else delete sh;
        return nullptr;
    }
    (void)hipSetDevice(devs[0]);
    return root;
}

extern "C" dmpc_ctx *dmpc_create(const dmpc_params *prm, int device, int precision)
{
    std::string why;
    if (check_params(prm, why)) { g_err = "dmpc_create: " + why; return nullptr; }
    if (precision < DMPC_PREC_F64 || precision > DMPC_PREC_LOW) { g_err = "dmpc_create: precision must be DMPC_PREC_F64, _MIXED, _F32FACTOR or _LOW"; return nullptr; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_err = std::string("dmpc_create: no HIP device available (") + hipGetErrorString(e) +
                "); this library has no CPU fallback";
        return nullptr;
    }
    if (device == DMPC_DEVICE_CURRENT && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device < 0 && device != DMPC_DEVICE_ALL) { g_err = "dmpc_create: device must be a HIP device index, DMPC_DEVICE_CURRENT or DMPC_DEVICE_ALL"; return nullptr; }
    if (device == DMPC_DEVICE_ALL) {   // every visible GPU; one visible GPU: a plain context
        std::vector<int> devs;
        const int emu = g_emulate_devices.load();
        if (emu > 0) {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess) cur = 0;
            devs.assign((size_t)emu, cur);
        } else
            for (int d = 0; d < ndev; ++d) devs.push_back(d);
        return devs.size() == 1 ? create_one(prm, devs[0], precision) : create_group(prm, devs, precision, emu > 0);
    }
    if (device < 0 || device >= ndev) { g_err = "dmpc_create: device index out of range"; return nullptr; }
    return create_one(prm, device, precision);
}

extern "C" int dmpc_group_size(const dmpc_ctx *ctx) { return ctx ? (ctx->grp ? ctx->grp->G : 1) : 0; }

// Only what is ordering stands here; every resource goes in `delete ctx`, by its member's destructor, with the context's device current
extern "C" void dmpc_destroy(dmpc_ctx *ctx)
{
    if (!ctx) return;
    for (dmpc_ctx *pc : ctx->peers) dmpc_destroy(pc);
    ctx->peers.clear();
    for (dmpc_ctx *ch : ctx->children) dmpc_destroy(ch);
    ctx->children.clear();
    if (ctx->comm) (void)dmpc_comm_destroy(ctx);
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->grp && ctx->rank == 0) delete ctx->grp;   // the root goes last: the shared block with it
    ctx->grp = nullptr;
    hipStream_t st = ctx->stream;
    delete ctx;
    if (st) (void)hipStreamDestroy(st);
}

extern "C" int dmpc_set_params(dmpc_ctx *ctx, const dmpc_params *prm)
{
    if (!ctx) { g_err = "dmpc_set_params: ctx is NULL"; return -1; }
    std::string why;
    if (check_params(prm, why)) FAIL(ctx, "dmpc_set_params: " + why);
    for (dmpc_ctx *pc : ctx->peers)
        if (dmpc_set_params(pc, prm)) FAIL(ctx, pc->err);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->prm = *prm;
    return upload_tables(ctx);
}

extern "C" int64_t dmpc_solve_count(const dmpc_ctx *ctx)
{
    if (!ctx) return 0;
    int64_t n = ctx->solves;
    for (const dmpc_ctx *ch : ctx->children) n += ch->solves;
    for (const dmpc_ctx *pc : ctx->peers) n += dmpc_solve_count(pc);
    return n;
}

extern "C" int dmpc_profile(dmpc_ctx *ctx, int enable)
{
    if (!ctx) return -1;
    ctx->profile = enable;
    if (enable && ctx->ev_pool.size() < 64) {   // a pool for the next steps, created outside any timed loop
        HIPCHK(ctx, hipSetDevice(ctx->device));
        while (ctx->ev_pool.size() < 64) {
            Ev ev{nullptr, nullptr, nullptr};
            HIPCHK(ctx, hipEventCreate(&ev.t0)); HIPCHK(ctx, hipEventCreate(&ev.t1)); HIPCHK(ctx, hipEventCreate(&ev.t2));
            ctx->ev_pool.push_back(ev);
        }
    }
    return 0;
}

extern "C" int dmpc_profile_read2(dmpc_ctx *ctx, double *solve_avg_ms, double *scan_avg_ms, int64_t *n_steps)
{
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (auto &ev : ctx->events) {
        HIPCHK(ctx, hipEventSynchronize(ev.t2));
        float ms_scan = 0.f, ms_solve = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms_scan, ev.t0, ev.t1));
        HIPCHK(ctx, hipEventElapsedTime(&ms_solve, ev.t1, ev.t2));
        ctx->prof_scan_ms_sum += ms_scan;
        ctx->prof_ms_sum += ms_solve;
        ctx->prof_n += 1;
        ctx->ev_pool.push_back(ev);
    }
    ctx->events.clear();
    if (solve_avg_ms) *solve_avg_ms = ctx->prof_n ? ctx->prof_ms_sum / (double)ctx->prof_n : 0.0;
    if (scan_avg_ms) *scan_avg_ms = ctx->prof_n ? ctx->prof_scan_ms_sum / (double)ctx->prof_n : 0.0;
    if (n_steps) *n_steps = ctx->prof_n;
    ctx->prof_ms_sum = ctx->prof_scan_ms_sum = 0.0;
    ctx->prof_n = 0;
    return 0;
}

// average duration (ms) of the step's kernels (scan + order + solve tiers) since the previous read
extern "C" int dmpc_profile_read(dmpc_ctx *ctx, double *avg_ms, int64_t *n_launches)
{
    double a = 0.0, b = 0.0;
    const int rc = dmpc_profile_read2(ctx, &a, &b, n_launches);
    if (avg_ms) *avg_ms = a + b;
    return rc;
}
