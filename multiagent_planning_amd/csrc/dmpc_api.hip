// dmpc_api.hip -- host side of libdmpc_hip.so: the C ABI declared in include/dmpc_hip.h.
//
// Owns the HIP context state (stream, precomputed per-case tables, scratch buffers) and launches
// the kernels of dmpc_kernels.hip.  There is deliberately NO CPU fallback anywhere in this file:
// without a HIP device every compute entry point fails with an error.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dmpc_hip.h"
#include "../../include/dmpc_hip_dev.h"
#include "dmpc_device.h"

#include "dmpc_kernels.hip"
#include "dmpc_postcheck.hip"
#include "dmpc_rowbuild.hip"
#include "dmpc_generators.hip"   // single translation unit: kernels + host ABI

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
    template <class T> T *as() { return (T *)p; }
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
    double *d_tables = nullptr;   // [3][900] Gram tables + [225] Lambda' table (dmpc_device.h: TAB_DOUBLES)
    double hsum[3] = {0, 0, 0};   // per cost case: sum of |H1(i,j)| (dual-bound certificate of the slack-free variants)
    std::string err;
    int64_t solves = 0;
    int max_lds_scp = 0;
    int max_lds_set = 0;
    // scratch for the host-pointer entry points
    DevBuf post_acc; int post_acc_S = 0, post_fused = 0;
    DevBuf rowbuf, rowkc, hdr, order, bbox, bbox_nm, nbr_list, nbr_cnt, lrow, counter, flag_list, scene_done;
    DevBuf close_list, close_cnt;   // the query's close pairs (StepParams::close_list)
    int num_cu = 0;
    DevOptions opt;          // development options (dmpc_debug_option)
    int max_lds_persist = 0;
    int max_lds_fill2 = 0;   // dynamic-LDS limit grid_fill2_kernel was last raised to (build_neighbour_lists)
    DevBuf prev_cost;        // [S * c_count] work estimates of the previous step (solve kernel -> order kernel)
    long prev_cost_shape = -1;
    int single_tier = 0;         // 1: solve with the full working-set capacity in one launch
    DevBuf lTf, lTf2;            // mixed precision: fp32 copies of the tables the scan reads
    DevBuf rows, lT, lT2, xp, xv, xa, pf, po, pout, vout, aout, status, info, hist_p, hist_v, hist_a, flags;
    int hist_S = 0, hist_N = 0, hist_KT = 0;   // shape of the histories left resident by the last dmpc_transition
    int32_t *flags_host = nullptr; size_t flags_host_cap = 0;   // pinned: per-step verdicts of dmpc_transition
    hipEvent_t flag_ev[2] = {nullptr, nullptr};
    DevBuf asg_io, asg_work;                                               // dmpc_assign_goals / _rect: staged inputs / outputs of the host forms; scratch of the round launches
    int32_t *asg_host = nullptr; size_t asg_host_cap = 0;                  // pinned: the scenes' done flags of two windows of rounds
    hipEvent_t asg_ev[2] = {nullptr, nullptr};
    int max_lds_assign[2] = {0, 0};   // dynamic-LDS limit assign_one_kernel<SWAP> was last raised to
    DevBuf plan_io, plan_mask;                                             // dmpc_plan_routes: staged inputs / outputs of the host form; the scenes' blocked bitmasks
    int max_lds_plan = 0;    // dynamic-LDS limit plan_route_kernel was last raised to
    DevBuf replan_work, replan_obst, replan_goals;                         // re-planning: blocked bitmasks | flagged list | count; the obstacle points of a column; dmpc_transition_replan's goals
    int max_lds_replan = 0;  // dynamic-LDS limit replan_route_kernel was last raised to
    int pc_fallback_scenes = 0;   // last dmpc_postcheck: scenes of a cell-grid search that were searched again by brute force
    std::vector<dmpc_ctx *> children;   // further contexts (own stream and buffers) for the other parts of a split batch of transitions
    std::vector<int> split_at;          // non-empty: the last dmpc_transition left scenes [split_at[i], split_at[i+1]) in part i (0: here, i > 0: children[i-1])
    std::string last_kernel; // the solve kernel the last step launched for the bulk of its agents (dmpc_last_solve_kernel)
    int rsolve_blocks = 0;   // workgroups of dmpc_rsolve_persist_kernel a CU holds (occupancy query, once per context)
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
    DevBuf pc_p, pc_v, pc_a, pc_M, pc_w, pc_scene, pc_agent, pc_interp;   // post-check work buffers
    DevBuf pc_static;                                                      // post-check: positions of the uncommanded vehicles + their per-scene minimum
    DevBuf path;                                                           // dmpc_transition_scripted: the scripted vehicles' paths [S][M][P][3], resident for the call
    DevBuf hold_out, hold_state;                                           // dmpc_transition_hold: the second set of p / v / a output rows 3 x [S][N_cmd][3K]; ints: run, hold_count, hold_first [S][N_cmd] each, agent_status [S][N_cmd][K_T_max]
    DevBuf mis_goals, mis_state;                                           // dmpc_transition_mission: goal sets [S][Q][N_cmd][3]; ints: stage [S], k_start [S], stage_col [S][Q], deadline [S][Q]
    Disturbance dist;                                                      // dmpc_set_disturbance: the disturbance in force (children of a split batch get a copy per call)
    DevBuf dist_buf; std::vector<unsigned char> dist_stage; long dist_key = -1;   // ... of a call on the device: wind | sorted pushes | offsets [S * N_cmd + 1]; its host staging; the shape dmpc_disturb_device uploaded for
    StartState start; FlightEnd end; std::vector<int32_t> start_src_host;                                       // dmpc_set_start: the armed start; the end of the last flight, valid until the step scratch is used again
    DevBuf start_x, start_plan, start_col, end_x, end_plan, end_src;       // a start on the device: x_p | x_v | x_a, plan_p | plan_v | plan_a rows, col0 [S]; dmpc_flight_end's gather; (source scene, last column) [S][2]
    DevBuf route_wp, route_state;                                          // dmpc_transition_route: waypoints [S][N_cmd][W][3]; ints: n_wp, cur, since [S][N_cmd] each, wp_col [S][N_cmd][W]
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
    DevBuf rb_A, rb_l, rb_sel, rb_out, rb_bin, rb_po, gen_out, hp_in, hp_out;                     // dense row builders (host-pointer entries)
    // profiling
    int profile = 0;
    double *dbg = nullptr; int dbg_agent = -1, dbg_cap = 0;   // development trace (dmpc_debug_trace)
    DevBuf forced_order; int forced_n = 0;                    // development aid (dmpc_debug_set_order)
    struct Ev { hipEvent_t t0, t1, t2; };   // step start | scan+order done | solve tiers done
    std::vector<Ev> events, ev_pool;
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

// ---------------------------------------------------------------------------------------------
// host math: model matrices (a1-a3) and the per-case tables
// ---------------------------------------------------------------------------------------------

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

extern "C" int dmpc_model_matrices(const dmpc_params *prm, double *Lambda, double *Av, double *A0, double *Delta)
{
    if (!prm || prm->K < 1 || prm->K > 64) { g_err = "dmpc_model_matrices: bad params"; return -1; }
    const int Kh = prm->K, n = 3 * Kh;
    const double h = prm->h;
    // Same floating-point recurrences as the reference so the matrices agree bit for bit:
    //   row_k = Aux*row_{k-1} + [0 .. b .. 0]  (getPosMat.m:18-23, dmpc_soft_bound.m:100-105)
    //   A_init = Aux*A_init                     (dmpc_soft_bound.m:106-107)
    // with Aux = [I3 h*I3; 0 I3], b = [h^2/2*I3; h*I3].  Per axis the state is (pos,vel) so only the
    // two scalar sequences pr[j], vr[j] (coefficients of a_j) are needed.
    std::vector<double> pr(Kh, 0.0), vr(Kh, 0.0);
    double a0p = 1.0, a0v = 0.0;   // A_init(1,1), A_init(1,4) of the current power of Aux
    if (Lambda) memset(Lambda, 0, sizeof(double) * n * n);
    if (Av) memset(Av, 0, sizeof(double) * n * n);
    if (A0) memset(A0, 0, sizeof(double) * n * 6);
    for (int k = 0; k < Kh; ++k) {
        for (int j = 0; j < Kh; ++j) {
            const double np_ = 1.0 * pr[j] + h * vr[j];   // Aux rows 1:3
            const double nv_ = 1.0 * vr[j];               // Aux rows 4:6
            pr[j] = np_; vr[j] = nv_;
        }
        pr[k] += h * h / 2; vr[k] += h;
        a0v = 1.0 * a0v + h * 1.0;   // (Aux*A_init)(1,4) = A_init(1,4) + h*A_init(4,4)
        for (int j = 0; j < Kh; ++j)
            for (int a = 0; a < 3; ++a) {
                if (Lambda) Lambda[(size_t)(3 * k + a) * n + 3 * j + a] = pr[j];
                if (Av) Av[(size_t)(3 * k + a) * n + 3 * j + a] = vr[j];
            }
        if (A0)
            for (int a = 0; a < 3; ++a) { A0[(size_t)(3 * k + a) * 6 + a] = a0p; A0[(size_t)(3 * k + a) * 6 + 3 + a] = a0v; }
    }
    if (Delta) {   // getDeltaMat.m:2-8: [I 0 ..; -I I 0 ..; ...]
        memset(Delta, 0, sizeof(double) * n * n);
        for (int k = 0; k < Kh; ++k)
            for (int a = 0; a < 3; ++a) {
                Delta[(size_t)(3 * k + a) * n + 3 * k + a] = 1.0;
                if (k > 0) Delta[(size_t)(3 * k + a) * n + 3 * (k - 1) + a] = -1.0;
            }
    }
    return 0;
}

extern "C" int dmpc_posvel_matrix(double h, int Kh, double *Aaug)
{
    // getPosVelMat.m:24: Aaug = [new_row(K); [0 .. I3]; [I3 0 ..]]  (12 x 3K): final position and
    // velocity rows, then the selectors of the last and first acceleration
    if (!Aaug || Kh < 1) { g_err = "dmpc_posvel_matrix: bad arguments"; return -1; }
    const int n = 3 * Kh;
    memset(Aaug, 0, sizeof(double) * 12 * n);
    for (int j = 0; j < Kh; ++j)
        for (int a = 0; a < 3; ++a) {
            Aaug[(size_t)a * n + 3 * j + a] = h * h / 2 + (double)(Kh - 1 - j) * h * h;
            Aaug[(size_t)(3 + a) * n + 3 * j + a] = h;
        }
    for (int a = 0; a < 3; ++a) {
        Aaug[(size_t)(6 + a) * n + 3 * (Kh - 1) + a] = 1.0;
        Aaug[(size_t)(9 + a) * n + a] = 1.0;
    }
    return 0;
}

// H1 = 2(q l_K l_K' + s D1'D1 + I)  (per-axis block of solveSoftDMPCbound.m:98); returns
// H1^-1, M1 = H1^-1 L', P1 = L H1^-1 L' (row-major 15x15 each)
static void build_case_tables(double h, double q, double s, double *out /*675*/, double *hsum = nullptr)
{
    long double L[K][K], H[K][K], Hi[K][K], C[K][K];
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) L[i][j] = (j <= i) ? ((long double)h * h / 2 + (long double)(i - j) * h * h) : 0.0L;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            long double dd = 0.0L;   // (D1'D1)_{ij}: tridiagonal [.. -1 2 -1 ..], last diagonal entry 1
            if (i == j) dd = (i == K - 1) ? 1.0L : 2.0L;
            else if (i == j + 1 || j == i + 1) dd = -1.0L;
            H[i][j] = 2.0L * ((long double)q * L[K - 1][i] * L[K - 1][j] + (long double)s * dd + (i == j ? 1.0L : 0.0L));
        }
    if (hsum) {   // sum of |H(i,j)|, rounded up: max over |a| <= alim of a'Ha/2 is at most alim^2/2 times this
        long double t = 0.0L;
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) t += fabsl(H[i][j]);
        *hsum = (double)(t * (1.0L + 1e-12L));
    }
    // Cholesky H = C C'
    memset(C, 0, sizeof(C));
    for (int j = 0; j < K; ++j) {
        long double d = H[j][j];
        for (int k = 0; k < j; ++k) d -= C[j][k] * C[j][k];
        C[j][j] = sqrtl(d);
        for (int i = j + 1; i < K; ++i) {
            long double t = H[i][j];
            for (int k = 0; k < j; ++k) t -= C[i][k] * C[j][k];
            C[i][j] = t / C[j][j];
        }
    }
    // Hi = H^-1 column by column
    for (int c = 0; c < K; ++c) {
        long double y[K], x[K];
        for (int i = 0; i < K; ++i) {
            long double t = (i == c) ? 1.0L : 0.0L;
            for (int k = 0; k < i; ++k) t -= C[i][k] * y[k];
            y[i] = t / C[i][i];
        }
        for (int i = K - 1; i >= 0; --i) {
            long double t = y[i];
            for (int k = i + 1; k < K; ++k) t -= C[k][i] * x[k];
            x[i] = t / C[i][i];
        }
        for (int i = 0; i < K; ++i) Hi[i][c] = x[i];
    }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            long double sym = 0.5L * (Hi[i][j] + Hi[j][i]);
            out[i * K + j] = (double)sym;
        }
    long double M[K][K];
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            long double t = 0.0L;
            for (int k = 0; k < K; ++k) t += 0.5L * (Hi[i][k] + Hi[k][i]) * L[j][k];
            M[i][j] = t;
            out[225 + i * K + j] = (double)t;
        }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            long double t = 0.0L;
            for (int k = 0; k < K; ++k) t += L[i][k] * M[k][j];
            out[450 + i * K + j] = (double)t;
        }
    // P1 is symmetric in exact arithmetic: symmetrise the rounded table
    for (int i = 0; i < K; ++i)
        for (int j = i + 1; j < K; ++j) {
            double m = 0.5 * (out[450 + i * K + j] + out[450 + j * K + i]);
            out[450 + i * K + j] = out[450 + j * K + i] = m;
        }
}

// the device tables: per cost case the symmetric 30x30 Gram table over (space, step) -- G[A i][A j] = H1^-1, G[A i][W j] =
// (H1^-1 L')(i,j), G[W i][W j] = L H1^-1 L' -- then Lt[k][kk] = Lambda(kk,k)
static int upload_tables(dmpc_ctx *ctx)
{
    std::vector<double> t(TAB_ALL_DOUBLES, 0.0);
    const dmpc_params &p = ctx->prm;
    const double sfree = p.Sfree > 0 ? p.Sfree : 10.0;
    const double qs[3] = {p.Qfar > 0 ? p.Qfar : 1000.0, p.Qnear > 0 ? p.Qnear : 10000.0, p.Q1};   // far (:44-47), near (:49-52), coll (:54-57)
    const double ss[3] = {sfree, sfree, (p.variant == DMPC_VAR_ALL3) ? 10.0 : p.S1};             // all:71
    for (int c = 0; c < 3; ++c) {
        double hmp[675];
        build_case_tables(p.h, qs[c], ss[c], hmp, &ctx->hsum[c]);
        double *G = &t[(size_t)c * TAB_CASE_DOUBLES];
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) {
                G[i * 30 + j] = hmp[i * K + j];
                G[i * 30 + 15 + j] = hmp[225 + i * K + j];
                G[(15 + j) * 30 + i] = hmp[225 + i * K + j];
                G[(15 + i) * 30 + 15 + j] = hmp[450 + i * K + j];
            }
        // Tp = C^-T with H1^-1 = C C' (the ROUNDED table above: the numbers the solver's Schur complement is made of).  The leading
        // m x m block of Tp is the inverse factor of the leading block of H1^-1: S^-1 = Tp Tp' for the bounds of steps 0..m-1 of one axis.
        // Second table: the same for the steps in FALLING order (14, 13, ..): H1^-1 with rows and columns reversed.
        for (int rev = 0; rev < 2; ++rev) {
            long double C[K][K], Ci[K][K];
            memset(C, 0, sizeof(C)); memset(Ci, 0, sizeof(Ci));
            auto hi = [&](int i, int j) -> long double { return rev ? hmp[(K - 1 - i) * K + (K - 1 - j)] : hmp[i * K + j]; };
            for (int j = 0; j < K; ++j) {
                long double d = hi(j, j);
                for (int k = 0; k < j; ++k) d -= C[j][k] * C[j][k];
                C[j][j] = sqrtl(d);
                for (int i = j + 1; i < K; ++i) {
                    long double v = hi(i, j);
                    for (int k = 0; k < j; ++k) v -= C[i][k] * C[j][k];
                    C[i][j] = v / C[j][j];
                }
            }
            for (int c2 = 0; c2 < K; ++c2)   // C^-1 column by column (forward substitution)
                for (int i = c2; i < K; ++i) {
                    long double v = (i == c2) ? 1.0L : 0.0L;
                    for (int k = c2; k < i; ++k) v -= C[i][k] * Ci[k][c2];
                    Ci[i][c2] = v / C[i][i];
                }
            double *Tp = &t[(size_t)TAB_DOUBLES + (size_t)(2 * c + rev) * TAB_TP_CASE];
            for (int i = 0; i < K; ++i)
                for (int j = i; j < K; ++j) Tp[i * (31 - i) / 2 + j - i] = (double)Ci[j][i];
        }
    }
    for (int k = 0; k < K; ++k)
        for (int kk = k; kk < K; ++kk) t[3 * TAB_CASE_DOUBLES + k * K + kk] = p.h * p.h / 2 + (double)(kk - k) * p.h * p.h;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_tables, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------

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
        hipMalloc((void **)&ctx->d_tables, sizeof(double) * TAB_ALL_DOUBLES) != hipSuccess || upload_tables(ctx) != 0) {
        g_err = "dmpc_create: device initialisation failed: " + ctx->err;
        dmpc_destroy(ctx);
        return nullptr;
    }
    if (hipDeviceGetAttribute(&ctx->num_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ctx->num_cu = 0;
    options_from_env(ctx);
    return ctx;
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
    if (device == DMPC_DEVICE_ALL) {
        // every visible GPU, one process: rank r of the group on device r (the reference's thread clusters, dmpc.cpp:1600-1625,
        // one GPU each).  One visible GPU: a plain context.
        std::vector<int> devs;
        const int emu = g_emulate_devices.load();
        if (emu > 0) {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess) cur = 0;
            devs.assign((size_t)emu, cur);
        } else
            for (int d = 0; d < ndev; ++d) devs.push_back(d);
        if (devs.size() == 1) return create_one(prm, devs[0], precision);
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
            c->grp = sh; c->nranks = G; c->rank = r; c->grp_emulated = emu > 0;
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
    if (device < 0 || device >= ndev) { g_err = "dmpc_create: device index out of range"; return nullptr; }
    return create_one(prm, device, precision);
}

extern "C" int dmpc_group_size(const dmpc_ctx *ctx) { return ctx ? (ctx->grp ? ctx->grp->G : 1) : 0; }

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
    if (ctx->grp && ctx->rank == 0) {   // the root goes last: the shared block with it
        for (hipEvent_t ev : ctx->grp->ev) if (ev) (void)hipEventDestroy(ev);
        delete ctx->grp;
    }
    ctx->grp = nullptr;
    for (auto &ev : ctx->events) { (void)hipEventDestroy(ev.t0); (void)hipEventDestroy(ev.t1); (void)hipEventDestroy(ev.t2); }
    for (auto &ev : ctx->ev_pool) { (void)hipEventDestroy(ev.t0); (void)hipEventDestroy(ev.t1); (void)hipEventDestroy(ev.t2); }
    for (int u = 0; u < 2; ++u) if (ctx->flag_ev[u]) (void)hipEventDestroy(ctx->flag_ev[u]);
    if (ctx->flags_host) (void)hipHostFree(ctx->flags_host);
    for (int u = 0; u < 2; ++u) if (ctx->asg_ev[u]) (void)hipEventDestroy(ctx->asg_ev[u]);
    if (ctx->asg_host) (void)hipHostFree(ctx->asg_host);
    if (ctx->dbg) (void)hipFree(ctx->dbg);
    if (ctx->d_tables) (void)hipFree(ctx->d_tables);
    hipStream_t st = ctx->stream;
    delete ctx;   // releases every DevBuf
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
            dmpc_ctx::Ev ev{nullptr, nullptr, nullptr};
            HIPCHK(ctx, hipEventCreate(&ev.t0)); HIPCHK(ctx, hipEventCreate(&ev.t1)); HIPCHK(ctx, hipEventCreate(&ev.t2));
            ctx->ev_pool.push_back(ev);
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------

#include "dmpc_launch.hip"   // plan_step, the five stages, launch_step
#include "dmpc_step.hip"     // the single step: scratch, StepIO and mixed-precision helpers, the record of a host-pointer call, the step entries

// ---------------------------------------------------------------------------------------------
// development aids, the profile's readers
// ---------------------------------------------------------------------------------------------

// development aid (not part of the public header): trace the active-set iterations of one agent
extern "C" int dmpc_debug_trace(dmpc_ctx *ctx, int agent, int cap, double *host_out)
{
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (host_out && ctx->dbg) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(host_out, ctx->dbg, sizeof(double) * 8 * ctx->dbg_cap, hipMemcpyDeviceToHost));
        return 0;
    }
    if (ctx->dbg) { (void)hipFree(ctx->dbg); ctx->dbg = nullptr; }
    ctx->dbg_agent = agent; ctx->dbg_cap = cap;
    if ((agent >= 0 || agent == -2 || agent == -3 || agent == -5 || agent == -7) && cap > 0) {
        HIPCHK(ctx, hipMalloc((void **)&ctx->dbg, sizeof(double) * 8 * cap));
        HIPCHK(ctx, hipMemset(ctx->dbg, 0, sizeof(double) * 8 * cap));
    }
    return 0;
}

// development aid (not part of the public header): a coalesced streaming read of `bytes` bytes at lane_bytes (8 | 16) per lane, `reps`
// launches -- the known byte count the FETCH_SIZE counter is calibrated on (tools/gpu_fetch_calib.py under rocprofv3 --pmc FETCH_SIZE)
extern "C" int dmpc_debug_read_probe(dmpc_ctx *ctx, size_t bytes, int lane_bytes, int reps)
{
    if (!ctx || (lane_bytes != 8 && lane_bytes != 16) || bytes < 4096) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *buf = nullptr; double *sink = nullptr;
    HIPCHK(ctx, hipMalloc(&buf, bytes));
    HIPCHK(ctx, hipMalloc((void **)&sink, 64));
    HIPCHK(ctx, hipMemsetAsync(buf, 0, bytes, ctx->stream));
    for (int r = 0; r < reps; ++r) {
        if (lane_bytes == 8) hipLaunchKernelGGL(read_probe_kernel<double>, dim3(256 * 16), dim3(256), 0, ctx->stream, bytes / 8, (const double *)buf, sink);
        else hipLaunchKernelGGL(read_probe_kernel<double2>, dim3(256 * 16), dim3(256), 0, ctx->stream, bytes / 16, (const double2 *)buf, sink);
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(buf); (void)hipFree(sink);
    return 0;
}

// development aid (not part of the public header): the scan's hand-off headers of the last step (8 ints per agent: rows, reference row count,
// violating step, status, flags, rows exist, ladder start, launch-order key)
extern "C" int dmpc_debug_read_hdr(dmpc_ctx *ctx, int *host_out, int n_agents)
{
    if (!ctx || !host_out) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if ((size_t)n_agents * 32 > ctx->hdr.cap) { ctx->err = "dmpc_debug_read_hdr: more agents than the last step had"; return -1; }
    HIPCHK(ctx, hipMemcpy(host_out, ctx->hdr.p, (size_t)n_agents * 32, hipMemcpyDeviceToHost));
    return 0;
}

// development aid (not part of the public header): what the last list build of a step left on the device (include/dmpc_hip_dev.h has the layout)
extern "C" int dmpc_debug_read_grid(dmpc_ctx *ctx, int *shape, void *out, size_t out_bytes)
{
    if (!ctx || !shape) return -1;
    dmpc_ctx::ListsBuilt &b = ctx->lists_built;
    b.armed = true;
    if (b.S == 0) { ctx->err = "dmpc_debug_read_grid: no step of this context has built neighbour lists"; return -1; }
    const int sh[12] = {b.S, b.G, b.C, b.n[0], b.n[1], b.n[2], b.ncell, b.build, b.cap, b.close_cap, b.agents, b.parts};
    memcpy(shape, sh, sizeof(sh));
    if (!out) return 0;
    const size_t nag = (size_t)b.G * b.C, grid = b.build ? 1 : 0, agents = (size_t)b.agents;
    const struct { const void *src; size_t words; } part[] = {
        {ctx->bbox.p, nag * b.S * 6 * NSEG}, {b.kept ? ctx->maxhalf_kept.p : b.maxhalf, grid * b.S * NSEG * 3}, {b.start, grid * b.S * NSEG * ((size_t)b.ncell + 1)},
        {b.ent, grid * 2 * b.S * NSEG * nag * 4}, {ctx->nbr_cnt.p, agents * b.parts}, {ctx->nbr_list.p, agents * b.cap},
        {ctx->close_cnt.p, b.close_cap ? agents : 0}, {ctx->close_list.p, agents * b.close_cap * 2}};
    size_t words = 0;
    for (const auto &q : part) words += q.words;
    if (out_bytes < words * 4) { ctx->err = "dmpc_debug_read_grid: the buffer is too small (" + std::to_string(words * 4) + " bytes)"; return -1; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    char *dst = (char *)out;
    for (const auto &q : part) {
        if (q.words) HIPCHK(ctx, hipMemcpy(dst, q.src, q.words * 4, hipMemcpyDeviceToHost));
        dst += q.words * 4;
    }
    return 0;
}

// development aid (not part of the public header): force the solve launch order (a permutation of the S*c_count agents
// of the next launches; n = 0 returns to the built-in policy).  Used to measure what an ideal order would give.
extern "C" int dmpc_debug_set_order(dmpc_ctx *ctx, const int *host_order, int n)
{
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->forced_n = 0;
    if (n > 0 && host_order) {
        if (ctx->forced_order.ensure(sizeof(int) * (size_t)n)) { ctx->err = "dmpc_debug_set_order: out of device memory"; return -1; }
        HIPCHK(ctx, hipMemcpy(ctx->forced_order.p, host_order, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
        ctx->forced_n = n;
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

#include "dmpc_plan.hip"     // route planning round static vehicles, before and during a flight: the wavefront planner's kernels, the three entries
#include "dmpc_disturb.hip"  // disturbed transitions: the rule on the host and the device, the descriptor's check and upload, the three entries
#include "dmpc_start.hip"    // a flight from a given or carried state and plan: the braking plan, the gather of a flight's end, the four entries
#include "dmpc_transition.hip"   // the closed loop: the record of a call, transition_one, transition_any, the seven entries

#include "dmpc_postcheck_host.hip"   // the post-checks on the host: the record of a call, PcPrep, the three checks, pc_run, the five entries

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

#include "dmpc_fileio.hip"
#include "dmpc_multigpu.hip"


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

#include "dmpc_assign.hip"   // goal assignment: the auction's kernels and the four entries


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
