/*
 * dmpc_hip.h -- C ABI of libdmpc_hip.so: the MI355X (gfx950) implementation of the DMPC
 * per-agent horizon-QP hot path of carlosluis/multiagent_planning.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository root).  Plain C, plain pointers and sizes: this is what a MEX gateway,
 * a cgo/ctypes stub or the C++ DMPC class would bind.
 *
 * Conventions
 *   - all real data is IEEE fp64 (MATLAB double / C++ double), K = k_hor = 15
 *   - "table" l: the previous MPC step's predicted position horizons of all agents.
 *     Host layout == MATLAB l(3,K,N) column-major == row-major [N][3K] with the stacked
 *     [x1 y1 z1 x2 ...] order (dmpc/matlab/dmpc_soft_bound.m:131,146).
 *   - S independent scenes ("trials", test/failure_rate.m:65) may be batched: arrays are
 *     [S][N][...]; agents only see neighbours of their own scene.  S = 1 is the reference case.
 *   - return value: 0 = ok, <0 = API/runtime error (text via dmpc_last_error); numerical
 *     outcomes are reported per agent in status[] (DMPC_ST_* bits) and info[] (DMPC_I_*).
 *   - entry points are synchronous unless noted; one HIP stream per context; a context may be
 *     used from one host thread at a time and has ONE step in flight at a time (the *_device entry
 *     points share per-context scratch: do not issue them on two streams of one context
 *     concurrently); distinct contexts are independent (dmpc/cpp/cluster_test.cpp:40 runs up to
 *     10 solver threads).
 */
#ifndef DMPC_HIP_H
#define DMPC_HIP_H

#include <stdint.h>

/* the library is built with hidden visibility: the entry points declared here (and the development interface of
 * dmpc_hip_dev.h) are all it exports */
#define DMPC_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

/* solver variants == reference functions under dmpc/matlab/ */
enum {
    DMPC_VAR_BOUND = 0,    /* solveSoftDMPCbound.m:1        (primary; test/failure_rate.m:110)  */
    DMPC_VAR_BOUND2 = 1,   /* solveSoftDMPCbound2.m:1       (test/comp_kctr.m:248)              */
    DMPC_VAR_ALL3 = 2,     /* solveSoftDMPCall.m:1                                              */
    DMPC_VAR_HARD = 3,     /* solveHardDMPC.m:1             (test/comp_hardsoft2.m)             */
    DMPC_VAR_ONDEMAND = 4, /* solveHardDMPCOnDemand.m:1                                         */
    DMPC_VAR_ELLIP = 5,    /* solveEllipDMPC.m:1                                                */
    DMPC_VAR_SOFTALL = 6,  /* solveSoftDMPC.m:1             (test/success_test_softdmpc.m:90)   */
    DMPC_VAR_REPAIR = 7,   /* solveSoftDMPCrepair.m:1       (test/comp_repair.m:93)             */
    /* the C++ flavour, DMPC::solveQPv2 (dmpc/cpp/dmpc.cpp:803-1287) with _k_factor = 0 / -1 (main.cpp:37-38):
     * bound / bound2 with the near-neighbour radius rmin*(1+(float)k/k_hor) (:418), slack bounds [-0.01f, 0] doubled on
     * retry together with term (<= 20 retries, :1079-1088), no early return on a first-step collision (DMPC_ST_COLL is
     * reported NEXT TO a solution, :419-424) and no in-bounds test.  All members of the C++ class are floats
     * (dmpc.h:191-205): pass h, rmin, c, alim as (double)(float) values and term = -1e6, Q1 = 1000, S1 = 100 (:846,942-945)
     * to reproduce its arithmetic. */
    DMPC_VAR_CPP = 8,
    DMPC_VAR_CPP2 = 9,
    /* the FIRST C++ version, DMPC::solveQP (dmpc/cpp/dmpc.cpp:554-801; callers solveDMPC :1367, cluster_solve :1776): at the first
     * horizon step k (0-based) where check_collisions (:378-396) finds a neighbour inside rmin, rows for ALL N-1 neighbours
     * (build_collconstraint :450-498) on step k-1, each with its own slack: [A I; 0 I] x <= [b; 0] (:629-633), linear slack cost -1e6
     * (:715), quadratic slack weight 1 (:719); cost cases by `violation` (:640-661); ONE QuadProgDense solve, no retry, no in-bounds
     * test, no first-step collision test.  A violation at k = 0 makes the reference index row -3 of A0 (undefined behaviour): reported
     * as DMPC_ST_COLL without a solve.  Float members as for DMPC_VAR_CPP. */
    DMPC_VAR_CPP1 = 10,
    /* solveSoftDMPC_c.m:1-96 (test/comp_confidence.m:184): solveSoftDMPC with the slack penalties of :60-63 -- linear -1e4 (K/k)^2, quadratic
     * 1e6 (K/k)^2, k the first violating horizon step (1-based) -- and no outbound output.  order 2 or 4. */
    DMPC_VAR_SOFTALL_C = 11,
    /* solveDMPC.m:1-74, the legacy SCP loop (dmpc/matlab/dmpc.m:79, test/success_test_dmpc.m:80, test/comp_heuristics.m:76): up to k_hor
     * passes; every pass re-linearises HARD spherical rows (CheckCollDMPC.m:6-8: plain Euclidean norm, no E1; CollConstrDMPC.m:8-30) for ALL
     * N-1 neighbours at every horizon step of `addConstr` about the previous pass's prediction, adds at most ONE new step per pass (the first
     * violating step not yet in the set, :28-33), solves the QP (cost case by `isempty(Ain_total)` only, :38-48) and stops when
     * maxDeviation(p, prev_p) <= dmpc_params.tol (:17,69; maxDeviation.m:3 looks at the first length(p)/3 = 5 steps of the 3 x 15 matrix).
     * The whole loop of an agent runs inside ONE kernel launch.  info: VIOLK = smallest step of addConstr, NROWS = rows of the last pass,
     * TRIES = passes made, CASE = 0 / 2 of the last pass; an infeasible pass ends the loop with DMPC_ST_INFEAS (`success = 0`, :58-63).
     * c and order are not used (sphere); no in-bounds test, no first-step collision test.
     * Row capacity: N-1 rows per step added to addConstr, at most 4096 rows over all passes, counted after exact pruning.  An agent can
     * overflow from N = 275 on (15 * 274 > 4096), and only when more than 4096 of its rows can become active; it then gets
     * DMPC_ST_CAPACITY with zero outputs. */
    DMPC_VAR_SCP = 12
};

/* per-agent status bits (the reference's feasible/success, outbound, coll flags) */
enum {
    DMPC_ST_SOLVED = 1,    /* p,v,a valid                                                        */
    DMPC_ST_OUTBOUND = 2,  /* is_inbounds.m:2-5 failed for the first predicted position          */
    DMPC_ST_COLL = 4,      /* already collided at horizon step 1 (solveSoftDMPCbound.m:25-31)    */
    DMPC_ST_INFEAS = 8,    /* QP infeasible after the retry ladder (solveSoftDMPCbound.m:102-155) */
    DMPC_ST_CAPACITY = 16, /* internal capacity exceeded (rows / active set): result NOT valid   */
    DMPC_ST_ITERCAP = 32,  /* iteration cap hit: result NOT valid                                */
    DMPC_ST_HELD = 64,     /* dmpc_transition_hold only: the agent flew its previous plan on this column */
    DMPC_ST_REACHED = 256  /* scene_status of dmpc_transition only: all agents reached their goals */
};

/* info[] : 8 int32 per agent */
enum {
    DMPC_I_VIOLK = 0,   /* 1-based first violating horizon step handled (0 = none)              */
    DMPC_I_NROWS = 1,   /* number of collision rows built (Nv)                                  */
    DMPC_I_TRIES = 2,   /* QP attempts (retry ladder)                                           */
    DMPC_I_CASE = 3,    /* cost case 0 far / 1 near / 2 collision (solveSoftDMPCbound.m:43-58)  */
    DMPC_I_ITERS = 4,   /* active-set iterations (all tries)                                    */
    DMPC_I_NSLACK = 5,  /* slack variables < 0 at the solution                                  */
    DMPC_I_NACTIVE = 6, /* active constraints at the solution                                   */
    DMPC_I_MAXQ = 7,    /* peak working-set size                                                */
    DMPC_INFO_LEN = 8
};

/* mirrors the reference's constants block (dmpc/matlab/dmpc_soft_bound.m:7-78;
 * dmpc/cpp/dmpc.h:50-63 `struct Params`) */
typedef struct {
    int32_t K;         /* horizon length k_hor; must be 15                                   */
    int32_t variant;   /* DMPC_VAR_*                                                         */
    int32_t order;     /* ellipsoid order: 2; or 4 (super-ellipsoid of test/comp_test_ellipconstr.m:158-187: dist = |E1 d|_4, E2 = E^-4) with
                        * the all-neighbour variants DMPC_VAR_SOFTALL / _SOFTALL_C / _ELLIP / _REPAIR / _CPP1; refused otherwise */
    int32_t max_tries; /* <=0: reference default (30)                                        */
    double h;          /* time step                                                          */
    double rmin;       /* collision radius                                                   */
    double c;          /* E = diag(1,1,c)                                                    */
    double alim;       /* |a| limit                                                          */
    double Q1, S1;     /* collision-case weights                                             */
    double term;       /* linear slack penalty (negative)                                    */
    double pmin[3], pmax[3];
    /* Weights of the two collision-free cost cases.  0 = the constants hard-coded at the reference's HEAD
     * (solveSoftDMPCbound.m:44-52, dmpc.cpp:922-938): far from the goal Q = 1000, within 1 m Q = 10000, S = 10 in both.
     * Earlier revisions of dmpc/cpp used other values: the recorded dmpc/cpp_results/trajectories (200-agents).txt is
     * reproduced to its 6 printed digits with Qfar = 100, Qnear = 1000 (tests/test_oracle_golden.py). */
    double Qfar, Qnear, Sfree;
    double tol;        /* DMPC_VAR_SCP only: `tol` of solveDMPC(..., Delta, tol, Q1, S1) (solveDMPC.m:1): the SCP loop ends when the largest
                        * position change of a pass falls to tol or below.  Ignored by every other variant.  (new in ABI revision 6) */
} dmpc_params;

typedef struct dmpc_ctx dmpc_ctx;

/* arithmetic of a context */
enum {
    DMPC_PREC_F64 = 0,   /* everything fp64 (the reference is MATLAB double)                                          */
    DMPC_PREC_MIXED = 1, /* the prediction table is kept in fp32 and the scan + collision rows (a5/a6) are computed in
                          * fp32; the QP itself (cost, factor, multipliers, propagation) and all inputs / outputs stay
                          * fp64.  Every entry point takes such a context: the host-pointer ones, the device-pointer steps (they
                          * make the fp32 copy of the caller's fp64 table themselves) and the sharded transitions, where the table
                          * the ranks exchange per step is the fp32 one (half the payload).  BASELINE configs[4].  The exact pruning,
                          * the infeasibility certificate and the ladder start keep a margin of 2e-5 that covers the fp32 rounding for
                          * coordinates up to about 8 m per axis: DESIGN.md section 6 has the bounds and the domain.          */
    DMPC_PREC_F32FACTOR = 2, /* the QP below fp64 (BASELINE configs[4], "fp32 vs fp64 tolerance sweep"): the inverse factor of the
                          * active-set solver -- its largest object, what every iteration multiplies with -- is STORED in fp32; cost,
                          * multipliers, residuals and the refinement of the result stay fp64 (lambda += T T' rho until the active-set
                          * residual is at 1e-13 or stops contracting).  Scan and rows fp64.  Not bit-compatible with DMPC_PREC_F64:
                          * the sweep (tests/test_gpu_precision.py) reports status agreement and l_inf per variant. */
    DMPC_PREC_LOW = 3    /* DMPC_PREC_MIXED | DMPC_PREC_F32FACTOR: fp32 table / scan / rows AND fp32 factor                      */
    /* DMPC_VAR_ALL3 keeps the fp64 factor whatever the context's precision says: its three nearly parallel rows per neighbour are the
     * one case the sweep found the fp32 factor unfit for (1 % of its agent-steps on another retry-ladder level). */
};

/* Create a solver context.  Replaces the constants/precompute preamble of dmpc/matlab/dmpc_soft_bound.m:80-108 and the DMPC ctor
 * dmpc/cpp/dmpc.cpp:19-75.  precision: DMPC_PREC_*.
 *   device >= 0           one HIP device.
 *   DMPC_DEVICE_ALL (-100) EVERY visible GPU, from this one process: the agents of each scene are sharded over the GPUs in the
 *                         reference's contiguous thread clusters (DMPC::solveParallelDMPCv2, dmpc/cpp/dmpc.cpp:1600-1625: N/G each,
 *                         the first N mod G one more), one internal host thread + stream + sub-context per GPU, and the join of
 *                         every MPC step (`prev_obs = obs`, :1671-1681; `l = new_l`, dmpc_soft_bound.m:146) is a set of direct
 *                         peer copies over xGMI, each rank writing its chunk of new predictions into every GPU's next table
 *                         (one address space: no collective library involved; the one-process-per-GPU form below uses RCCL).
 *                         The host-pointer entry points a MATLAB / C++ caller uses -- dmpc_transition, dmpc_step_batch,
 *                         dmpc_postcheck on the resident histories -- work unchanged on such a context; the per-agent and helper
 *                         entry points run on its first GPU; the device-pointer entry points (one device's memory) refuse it.
 *                         With one visible GPU this is a plain context.  Results do not depend on the number of GPUs, bit for bit.
 *   DMPC_DEVICE_CURRENT (-1) the calling thread's current HIP device (one process per GPU: "this rank's GPU").
 *   Any other negative value is refused.
 * Returns NULL on failure (no device, bad parameters); dmpc_last_error(NULL) has the text. */
#define DMPC_DEVICE_CURRENT (-1)   /* (the value "current device" has had since the first version of this header) */
#define DMPC_DEVICE_ALL (-100)
/* ABI revision of this header.  The special device values changed once (the round-3 header had DMPC_DEVICE_ALL = -1, DMPC_DEVICE_CURRENT = -2;
 * since revision 4 they are the two values above and any other negative device is refused), so a binding compiled against another header
 * should compare dmpc_abi_version() with the DMPC_ABI_VERSION it was built with before its first dmpc_create. */
#define DMPC_ABI_VERSION 8
DMPC_API int dmpc_abi_version(void);
DMPC_API dmpc_ctx *dmpc_create(const dmpc_params *prm, int device, int precision);
/* number of GPUs the context drives (1 unless created with DMPC_DEVICE_ALL on a multi-GPU node) */
DMPC_API int dmpc_group_size(const dmpc_ctx *ctx);
DMPC_API void dmpc_destroy(dmpc_ctx *ctx);
DMPC_API const char *dmpc_last_error(const dmpc_ctx *ctx);

/* Change parameters (variant, weights, bounds ...) of an existing context.  Every later call answers, bit for bit, as on a context
 * created with `prm` (same device and precision); what survives is what is not a parameter: development options, the disturbance of
 * dmpc_set_disturbance and the resident histories of the last transition.  A refused block (-1) leaves the context as it was. */
DMPC_API int dmpc_set_params(dmpc_ctx *ctx, const dmpc_params *prm);

/* a1-a3: getPosMat.m:1 (Lambda = A = A_p), A_v / A_initp loop dmpc_soft_bound.m:92-108,
 * getDeltaMat.m:1.  Host computation, row-major; any pointer may be NULL.
 * Lambda, Av, Delta: 3K x 3K; A0: 3K x 6. */
DMPC_API int dmpc_model_matrices(const dmpc_params *prm, double *Lambda, double *Av, double *A0, double *Delta);

/* getPosVelMat.m:1 (dec-iSCP/cup-SCP helper kept for signature parity): Aaug (12 x 3K). */
DMPC_API int dmpc_posvel_matrix(double h, int K, double *Aaug);

/* a4: initDMPC.m:1 for S*N agents (MPC step k = 1).  Host pointers.
 * po, pf: [S][N][3]; l_out, v_out, a_out: [S][N][3K]. */
DMPC_API int dmpc_init_batch(dmpc_ctx *ctx, int S, int N, const double *po, const double *pf, double *l_out,
                    double *v_out, double *a_out);

/* a11: ONE MPC step for all agents of S scenes == the body of `for n = 1:N`
 * (dmpc_soft_bound.m:116-135 / cluster_solvev2 dmpc/cpp/dmpc.cpp:1792-1841) with the solver
 * selected by prm.variant.  Host pointers; copies in, launches, copies out, synchronises.
 * l: [S][N][3K]; x_p,x_v,x_a (= pk,vk,ak(:,k-1,n)), pf: [S][N][3];
 * p_out,v_out,a_out: [S][N][3K] (rows of agents without DMPC_ST_SOLVED are zero);
 * status: [S][N]; info: [S][N][8] (may be NULL). */
DMPC_API int dmpc_step_batch(dmpc_ctx *ctx, int S, int N, const double *l, const double *x_p, const double *x_v,
                    const double *x_a, const double *pf, double *p_out, double *v_out, double *a_out,
                    int32_t *status, int32_t *info);

/* Uncommanded vehicles (ABI revision 8).  The C++ class plans for N vehicles of which only N_cmd are commanded: N = _po.cols(),
 * N_cmd = _pf.cols() (DMPC::solveParallelDMPCv2 dmpc/cpp/dmpc.cpp:1572-1573, solveDMPC :1295-1430, solveParallelDMPC :1435-1565).
 * Agents 0 .. N_cmd-1 are commanded; agents N_cmd .. N-1 stay where they are, and their "prediction" is their start position
 * replicated over the horizon at every MPC step (:1633-1649, :1320-1330).  A commanded agent treats such a column like any
 * neighbour -- same ellipsoid, same thresholds, same row order by neighbour index (check_collisionsv2 loops over all N, :395-448);
 * static agents are never solved, never advanced, have no status and do not enter ReachedGoal or the scene verdict
 * (reached_goalv2 and the recorded solution cover the N_cmd commanded ones, :1600, :1684, :1691).
 * The *_cmd entries below take 1 <= N_cmd <= N (anything else: -1 and a message, nothing launched); with N_cmd == N each returns
 * bit for bit what the entry without the suffix returns.  On a DMPC_DEVICE_ALL context a call with N_cmd < N runs on the first GPU
 * (the rule for N < 2 G).  The RCCL entries (dmpc_step_sharded_device, dmpc_transition_sharded*) have NO *_cmd form: a fleet with
 * uncommanded vehicles is planned by one process.
 *
 * dmpc_step_batch_cmd: dmpc_step_batch for the commanded agents against the caller's table of all N vehicles (the caller keeps
 * the static rows constant).  l: [S][N][3K]; x_p, x_v, x_a, pf: [S][N_cmd][3]; p_out, v_out, a_out: [S][N_cmd][3K];
 * status: [S][N_cmd]; info: [S][N_cmd][8] or NULL. */
DMPC_API int dmpc_step_batch_cmd(dmpc_ctx *ctx, int S, int N, int N_cmd, const double *l, const double *x_p, const double *x_v,
                        const double *x_a, const double *pf, double *p_out, double *v_out, double *a_out,
                        int32_t *status, int32_t *info);

/* a7/a8: one agent (0-based n) of one scene: the per-call entry the signature-preserving MATLAB
 * wrappers use ([p,v,a,feasible,outbound,coll] = solveSoftDMPCbound(...), solveSoftDMPCbound.m:1).
 * Host pointers.  l: [N][3K]; po,vo,ao,pf: [3]; p,v,a: [3K]; info: [8] or NULL. */
DMPC_API int dmpc_solve_one(dmpc_ctx *ctx, int N, int n, const double *l, const double *po, const double *vo,
                   const double *ao, const double *pf, double *p, double *v, double *a, int32_t *status,
                   int32_t *info);

/* a5/a6 standalone: the scan and the collision rows of ONE agent (0-based n) exactly as the selected
 * solver variant builds them -- [violation,min_dist,viol_constr] = CheckCollSoftDMPC(...) (CheckCollSoftDMPC.m:1)
 * followed by [Ain,bin,prev_dist] = CollConstrSoftDMPC(...) (CollConstrSoftDMPC.m:1; ...2 / Hard / HardOnDemand /
 * Ellip variants) -- in structured form, reference row order, no pruning.  Host pointers.
 *   row i:  -xi_i' * Lambda(3kc_i-2:3kc_i, :) * a  [+ slack_coef_i * eps_i]  <=  rhs_i
 *   xi: [max_rows][3] = E2*(p - p_j); kc: 1-based constrained horizon step; rhs = bin; slack_coef = prev_dist
 *   (1 for solveSoftDMPC, 0 for the hard variants); nrows = number of rows built (may exceed max_rows);
 *   viol_k = 1-based first violating horizon step (0 none); status = DMPC_ST_COLL or 0. */
DMPC_API int dmpc_rows_one(dmpc_ctx *ctx, int N, int n, const double *l, const double *po, const double *vo, int max_rows,
                  double *xi, double *rhs, double *slack_coef, int32_t *kc, int32_t *nrows, int32_t *viol_k,
                  int32_t *status);

/* Device-resident form of a11 for callers that keep state in HBM (bench, multi-GPU driver).
 * The table is in the chunked transposed layout lT[G][S][3K][C]: G chunks (= ranks) of C agents
 * each, N = G*C agents per scene; this call solves the C agents of chunk g_local of every scene
 * against the whole table (the per-step all-gather concatenates the ranks' lT_next chunks).
 * All pointers are DEVICE pointers; `stream` is the caller's hipStream_t and is used as given (NULL = HIP's
 * default stream, which is also PyTorch's default current stream), so the launches are ordered with the caller's
 * other work on that stream (e.g. the RCCL all-gather of lT_next); asynchronous: returns after enqueueing.
 *   x_p,x_v,x_a,pf : [S][C][3]          p_out,v_out,a_out : [S][C][3K]
 *   lT_next        : [S][3K][C] (this chunk, may be NULL)   status [S][C], info [S][C][8] */
DMPC_API int dmpc_step_device(dmpc_ctx *ctx, int S, int G, int C, int g_local, const double *lT, const double *x_p,
                     const double *x_v, const double *x_a, const double *pf, double *p_out, double *v_out,
                     double *a_out, double *lT_next, int32_t *status, int32_t *info, void *stream);

/* dmpc_step_device for N_cmd commanded agents of a table of N vehicles, one chunk (G = 1): lT, lT_next: [S][3K][N];
 * x_p, x_v, x_a, pf: [S][N_cmd][3]; p_out, v_out, a_out: [S][N_cmd][3K]; status [S][N_cmd], info [S][N_cmd][8] or NULL.
 * Only columns < N_cmd of lT_next are written: its static columns (N_cmd .. N-1) are the CALLER'S -- fill them once, in both
 * tables of a ping-pong pair (dmpc_table_from_rows_device builds either table from rows [S][N][3K]). */
DMPC_API int dmpc_step_device_cmd(dmpc_ctx *ctx, int S, int N, int N_cmd, const double *lT, const double *x_p, const double *x_v,
                         const double *x_a, const double *pf, double *p_out, double *v_out, double *a_out, double *lT_next,
                         int32_t *status, int32_t *info, void *stream);

/* layout helpers (device pointers, asynchronous on `stream`):
 * rows [S][N][3K] -> lT [G][S][3K][C] with N = G*C, and first columns x_next = out(:,1). */
DMPC_API int dmpc_table_from_rows_device(dmpc_ctx *ctx, int S, int G, int C, const double *rows, double *lT, void *stream);

/* Fused state advance on device: x_p,x_v,x_a <- first horizon column of p_out,v_out,a_out for
 * SOLVED agents (dmpc_soft_bound.m:132-134).  [S][C] agents. */
DMPC_API int dmpc_advance_device(dmpc_ctx *ctx, int count, const double *p_out, const double *v_out, const double *a_out,
                        const int32_t *status, double *x_p, double *x_v, double *x_a, void *stream);

/* Whole transition on one device: the `for k = 1:K_T` loop of dmpc_soft_bound.m:115-148 /
 * DMPC::solveParallelDMPCv2 (dmpc/cpp/dmpc.cpp:1656-1686) with every vehicle commanded (N_cmd == N; dmpc_transition_cmd below
 * covers N_cmd < N) incl. initDMPC at k = 1, the table
 * swap l = new_l and the ReachedGoal.m test.  Host pointers.
 * K_T_max = number of history COLUMNS, the initial state (k = 1, initDMPC) included: at most K_T_max - 1 solves per agent.
 * `for k = 1:K_T` of dmpc_soft_bound.m:115 is K_T_max = K_T; `while ~reached_goal && k < max_K` of test/failure_rate.m:99
 * records max_K - 1 columns: pass K_T_max = max_K - 1.  ReachedGoal.m is evaluated on every column, the first included.
 * A scene stops at the first step where any agent's status is not exactly DMPC_ST_SOLVED (infeasible, collided, out of
 * the workspace): stricter than failure_rate.m, which only aborts on `~feasible` and -- solveSoftDMPCbound keeping
 * feasible = 1 on outbound -- carries on with a partially updated table after an outbound first step (:112-126).
 * A QP that is infeasible without any collision row is reported DMPC_ST_INFEAS at once: the reference retries it up to 30
 * times with quadprog's ConstraintTolerance doubled each time (solveSoftDMPCbound.m:140-146) and may end up accepting a
 * bound-violating point, typically reported `outbound` instead.
 * po,pf: [S][N][3]; pk,vk,ak: [S][N][K_T_max][3] (written up to K_T_used[s]; the columns a scene never reached stay zero, like the preallocated arrays of the reference) or all three NULL: the histories
 * then only stay on the device (for dmpc_postcheck) and the 3 x S*N*K_T_max*24-byte download is skipped;
 * K_T_used[S]: number of MPC steps taken per scene; scene_status[S]: OR of agent status bits at
 * the step where the scene stopped; DMPC_ST_SOLVED | DMPC_ST_REACHED = every agent within error_tol of its goal
 * (ReachedGoal.m), DMPC_ST_SOLVED alone = ran to K_T_max without reaching (failed_goal, failure_rate.m:131-134).
 * Batches of 32 or more scenes are run in parts (2; 4 from 128 scenes on) on internal contexts of their own (a HIP stream and a
 * helper host thread each for the duration of the call) so that the slow tail of one part overlaps the others; scenes are independent,
 * results do not depend on the split.  On a DMPC_DEVICE_ALL context the agents of every scene are sharded over the GPUs instead
 * (see dmpc_create), and batches of 64 or more scenes run as two such groups side by side. */
DMPC_API int dmpc_transition(dmpc_ctx *ctx, int S, int N, const double *po, const double *pf, int K_T_max,
                    double error_tol, double *pk, double *vk, double *ak, int32_t *K_T_used,
                    int32_t *scene_status);

/* dmpc_transition with uncommanded vehicles: DMPC::solveParallelDMPCv2 (dmpc/cpp/dmpc.cpp:1570-1730; solveDMPC :1295-1430 and
 * solveParallelDMPC :1435-1565 plan the same problem) for N = _po.cols() vehicles of which N_cmd = _pf.cols() are commanded.
 * po: [S][N][3], pf: [S][N_cmd][3]; pk, vk, ak: [S][N_cmd][K_T_max][3] or all NULL; the columns N_cmd .. N-1 of the table hold
 * po replicated K times at every MPC step, the first included.  Stopping rule, verdict read-back, batch split, K_T_used and
 * scene_status as for dmpc_transition, over the commanded agents only; the histories of the commanded agents stay resident for
 * dmpc_postcheck_cmd (or dmpc_postcheck with N = N_cmd). */
DMPC_API int dmpc_transition_cmd(dmpc_ctx *ctx, int S, int N, int N_cmd, const double *po, const double *pf, int K_T_max,
                        double error_tol, double *pk, double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status);

/* Scripted vehicles: uncommanded vehicles that MOVE along a path the caller knows (a piloted craft, a vehicle run by another planner).
 * NO REFERENCE COUNTERPART: DMPC::solveParallelDMPCv2 freezes uncommanded vehicles at their start (dmpc/cpp/dmpc.cpp:1633-1649, what
 * dmpc_transition_cmd does).  What the reference does define is one MPC step of a commanded agent against a table of N rows (cluster_solvev2,
 * :1792-1841); the three entries below are that step applied to a table whose uncommanded rows are rewritten before every step -- the loop a
 * caller of dmpc_step_batch_cmd could write on the host -- with everything dmpc_transition_cmd keeps on the device.  Additive: the ABI
 * revision stays 8.
 *   scene     N_cmd >= 1 commanded agents first, M >= 1 scripted vehicles behind them; the table has N = N_cmd + M columns.
 *   path      [S][M][P][3], P >= 1: sample t of a vehicle is its position at history column t (column 0 = the start, the initDMPC column);
 *             sample(j, t) = path[j][min(t, P-1)] -- a vehicle whose path has ended stays at its last sample.
 *   alignment at the MPC step that produces history column k (k = 1 .. K_T_max-1), horizon entry kk = 0 .. K-1 of scripted vehicle j is
 *             sample(j, k-1+kk): the window covers columns k-1 .. k+K-2, NOT k .. k+K-1.  A commanded neighbour's row has the same alignment
 *             (it is the output of step k-1, whose first column is history column k-1; the first table starts at po, column 0), and the scan
 *             compares the agent's own previous horizon with these rows column by column.
 * Scripted vehicles are never solved, have no status and do not enter ReachedGoal or the scene verdict.
 *
 * dmpc_transition_scripted: dmpc_transition_cmd with moving uncommanded vehicles.  Host pointers.  po, pf: [S][N_cmd][3]; pk, vk, ak:
 * [S][N_cmd][K_T_max][3] or all three NULL.  The path is uploaded once per call; before EVERY step (the first included) one launch writes the
 * scripted columns of the current table from it (in mixed precision before the fp32 copy of the table is made).  Stopping rule, K_T_used,
 * scene_status, histories, verdict read-back, batch split (each part gets its scenes' paths) and resident histories as for
 * dmpc_transition_cmd; on a DMPC_DEVICE_ALL context the call runs on the first GPU (the rule for N_cmd < N); there is no RCCL form.
 * With P == 1 the result is dmpc_transition_cmd on po = [po; path[:, :, 0]], byte for byte.
 * M < 1, P < 1, N_cmd < 1, a NULL path or only some of pk / vk / ak: -1 and a message that starts with the entry's name, nothing launched. */
DMPC_API int dmpc_transition_scripted(dmpc_ctx *ctx, int S, int N_cmd, int M, int P, const double *po, const double *pf, const double *path,
                             int K_T_max, double error_tol, double *pk, double *vk, double *ak, int32_t *K_T_used,
                             int32_t *scene_status);

/* The same fill for device-resident callers that loop over dmpc_step_device_cmd: writes columns N_cmd .. N-1 of lT[S][3K][N] for MPC step
 * k >= 1 (the step that produces history column k) from path_dev [S][N - N_cmd][P][3]; lTf non-NULL: also the same columns of an fp32 table
 * of the same layout.  Device pointers, asynchronous on `stream`.  Call it on the table a step is about to READ, before that step. */
DMPC_API int dmpc_scripted_cols_device(dmpc_ctx *ctx, int S, int N, int N_cmd, int P, const double *path_dev, int k, double *lT, float *lTf,
                              void *stream);

/* Missions: one transition through a SEQUENCE of goal sets (formations A -> B -> C flown as one trajectory, a retarget at a known time, a
 * formation that is only passed through).  NO REFERENCE COUNTERPART: the reference flies one leg (one pf, every agent at rest at the start,
 * the trial over when pf is reached).  What it defines is the MPC step; this entry is that step in the loop a caller of
 * dmpc_step_batch[_cmd] could write on the host, with the rule below applied between two steps -- on the device, so that the verdicts
 * are still read one window behind the steps.  Additive: the ABI revision stays 8.
 *   goals     [S][Q][N_cmd][3], Q >= 1 stages per scene; deadline [S][Q] (int32) or NULL = none: 0 = none, negative values are refused,
 *             the last stage's entry must be 0.
 *   stage 0   starts at history column 0, the initDMPC column: its straight lines run from po to goals[s][0], as in dmpc_transition.
 *   a stage q < Q-1 ENDS AT THE FIRST COLUMN k at which (a) ReachedGoal holds on column k against goals[s][q] (max_i |p_i - pf_i| < error_tol,
 *             the verdict of that column as dmpc_transition computes it) or (b) deadline[s][q] > 0 and k - k_start(q) >= deadline[s][q].
 *             Then stage_col[s][q] = k, k_start(q+1) = k, and the step that produces column k+1 is the first one solved with goals[s][q+1].
 *             THE TABLE IS NOT REWRITTEN: for that one step the neighbours see the plans made for the old goals, as a host loop's would.
 *             AT MOST ONE STAGE ENDS PER COLUMN: stage q+1 is first examined on column k+1, also when its goals are stage q's (or are met
 *             already) -- two stages with the same goals end on consecutive columns.
 *   stage Q-1 reached on column k ends the trial: DMPC_ST_SOLVED | DMPC_ST_REACHED, K_T_used = k+1, stage_col[s][Q-1] = k (dmpc_transition's
 *             rules).  Reaching an earlier stage never ends the trial and never sets DMPC_ST_REACHED.
 *   failure   an agent whose status is not exactly DMPC_ST_SOLVED stops the scene as in dmpc_transition, in whatever stage; no stage ends on
 *             that column.  stage_col of a stage that never ended is -1.
 * K_T_max counts the columns of the whole mission.  pk, vk, ak: ONE [S][N_cmd][K_T_max][3] array each (or all three NULL), resident afterwards:
 * dmpc_postcheck*, dmpc_postcheck_clearance with pf = goals[:, Q-1] work on them unchanged.  stage_col: [S][Q] or NULL.
 * po: [S][N][3] without a path (N_cmd < N: static vehicles, as dmpc_transition_cmd); with path [S][N-N_cmd][P][3]: [S][N_cmd][3] and scripted
 * vehicles, as dmpc_transition_scripted.  Q == 1 without deadline is dmpc_transition / _cmd / _scripted byte for byte.  Batch split as
 * dmpc_transition (each part gets its scenes' goals, deadlines and stage_col); a DMPC_DEVICE_ALL context runs the call on its first GPU;
 * there is no RCCL form.  Q < 1, a NULL goals, a negative deadline, a non-zero last deadline, or what the entries above refuse: -1 and a
 * message that starts with the entry's name, nothing launched. */
DMPC_API int dmpc_transition_mission(dmpc_ctx *ctx, int S, int N, int N_cmd, int Q, const double *po, const double *goals, const int32_t *deadline,
                            const double *path, int P, int K_T_max, double error_tol, double *pk, double *vk, double *ak,
                            int32_t *K_T_used, int32_t *scene_status, int32_t *stage_col);

/* Hold policy: dmpc_transition_mission in which AN AGENT WHOSE SOLVE FAILED FLIES ITS PREVIOUS PLAN WHILE THE SCENE GOES ON.  NO REFERENCE
 * COUNTERPART: the reference's failure-rate experiment -- and every other closed loop of this header -- stops the whole scene at the first
 * column on which any agent's status is not exactly DMPC_ST_SOLVED.  Additive: the ABI revision stays 8.  The arguments up to stage_col are
 * dmpc_transition_mission's, with the same meaning, the same refusals and the same batch split (Q == 1 without a deadline: the one-leg, static
 * and scripted forms).  The rule, per commanded agent, after the solve of the step that produces history column k:
 *   fail      the agent's status is not exactly DMPC_ST_SOLVED -- the predicate that stops a scene elsewhere; it includes
 *             DMPC_ST_SOLVED | DMPC_ST_OUTBOUND and the DMPC_ST_SOLVED | DMPC_ST_COLL of the cpp variants, whose solution is then discarded.
 *   run       the number of consecutive columns up to and including k on which the agent failed; 0 after a column on which it did not.
 *   held      fail and run <= max_hold: the agent's plan of this step is its previous plan shifted by one entry,
 *               p'[kk] = p[kk+1], v'[kk] = v[kk+1], a'[kk] = a[kk+1]   (kk = 0 .. K-2, copies)
 *             with a braking tail as the last entry, per axis, every operation rounded on its own (no fused multiply-add):
 *               a'[K-1] = a_t = min(max(-v[K-1] / h, -alim), alim)
 *               v'[K-1] = v[K-1] + h * a_t
 *               p'[K-1] = (p[K-1] + h * v[K-1]) + (0.5 * h * h) * a_t
 *             "Previous plan" is the agent's plan of step k-1, solved or held; for k = 1 the initDMPC plan (the straight-line positions,
 *             v = a = 0).  A held plan is treated exactly as a solved one: its column goes into the next table, its first entry becomes the
 *             state and history column k, and it counts as solved in the scene verdict, in ReachedGoal and in the mission stage rule.
 *   over      fail and run > max_hold: the agent is not held, and the column ends the scene exactly as in dmpc_transition_mission -- the
 *             same recorded column, K_T_used = k+1, scene_status = the OR of the raw bits (of the agents not held on that column).
 * max_hold >= 0.  max_hold == 0: every output of the common arguments is dmpc_transition_mission's byte for byte, on failing scenes too.
 * Outputs, each or all NULL:
 *   hold_count   [S][N_cmd]            the columns on which the agent was held
 *   hold_first   [S][N_cmd]            the first such column, or -1
 *   agent_status [S][N_cmd][K_T_max]   column 0: DMPC_ST_SOLVED; column k: the solver's raw status of that step, DMPC_ST_HELD OR-ed in where
 *                                      the agent was held; columns the scene never reached: 0
 * scene_status[s] carries DMPC_ST_HELD in addition when any agent of the scene was held on a column < K_T_used[s], and is as in
 * dmpc_transition_mission otherwise: DMPC_ST_SOLVED | DMPC_ST_REACHED | DMPC_ST_HELD is a transition that arrived with holds.  Whether a flown
 * transition kept its clearance is what dmpc_postcheck* and dmpc_postcheck_clearance answer on the resident histories, unchanged.
 * A DMPC_DEVICE_ALL context runs the call on its first GPU; there is no RCCL form.  max_hold < 0, or what dmpc_transition_mission refuses:
 * -1 and a message that starts with the entry's name, nothing launched. */
DMPC_API int dmpc_transition_hold(dmpc_ctx *ctx, int S, int N, int N_cmd, int Q, const double *po, const double *goals, const int32_t *deadline,
                         const double *path, int P, int K_T_max, double error_tol, int max_hold, double *pk, double *vk, double *ak,
                         int32_t *K_T_used, int32_t *scene_status, int32_t *stage_col, int32_t *hold_count, int32_t *hold_first,
                         int32_t *agent_status);

/* Routes: EVERY COMMANDED AGENT THROUGH WAYPOINTS OF ITS OWN, switched per agent on the device.  NO REFERENCE COUNTERPART: DMPC has no global
 * planner -- an agent whose straight line is blocked by a wall of uncommanded vehicles parks in front of it -- and a mission switches a whole
 * scene at once, every agent braking at every intermediate formation.  The step is the reference's; this entry is that step in the loop a caller
 * of dmpc_step_batch[_cmd] could write on the host, with the rule below applied between two steps, on the device.  Additive: the ABI revision stays 8.
 *   waypoints [S][N_cmd][W][3], W >= 1; n_wp [S][N_cmd] (int32, each 1 .. W) or NULL = every agent has W.  An agent's last waypoint,
 *             waypoints[s][i][n_wp-1], is its goal; entries behind it are never read.
 *   capture   > 0, metres; timeout >= 0, columns, 0 = none.
 *   state     per commanded agent: cur[i], the index of its current waypoint, and since[i], the column on which that waypoint became current; both
 *             start at 0.  The goal the QP of agent i sees is waypoints[s][i][cur[i]].  Column 0 is the initDMPC column: its straight lines run
 *             from po to every agent's waypoint 0.
 *   the rule  after the post step of history column k (column 0 included), with bits = the OR of the status words and the states as that column
 *             recorded them, in this order:
 *             1. bits & ~DMPC_ST_SOLVED: the scene stops exactly as in dmpc_transition; no waypoint switches on that column.
 *             2. all_last = every agent has cur[i] == n_wp[i]-1, evaluated BEFORE any switch of this column.  all_last and ReachedGoal on
 *                column k (the post step's verdict: max_i |p_i - goal_i| < error_tol): the trial ends, DMPC_ST_SOLVED | DMPC_ST_REACHED,
 *                K_T_used = k+1.  While all_last is false a column never reports DMPC_ST_REACHED and never ends the trial, also when every agent
 *                happens to be within error_tol of its current waypoint.
 *             3. otherwise every agent with cur[i] < n_wp[i]-1 switches when (a) d2 < capture * capture, d2 = (dx*dx + dy*dy) + dz*dz,
 *                d = p_i(k) - waypoints[s][i][cur[i]], in fp64 with every operation rounded on its own (no fused multiply-add), or
 *                (b) timeout > 0 and k - since[i] >= timeout.  On a switch wp_col[s][i][cur[i]] = k, cur[i] += 1, since[i] = k, and the step that
 *                produces column k+1 is the first one solved with the new waypoint.
 *             AT MOST ONE WAYPOINT PER AGENT AND COLUMN: the next waypoint is first examined on column k+1, also when it is met already.
 *             THE TABLE IS NOT REWRITTEN: for that one step the neighbours see the plan made for the old waypoint, as a host loop's would.
 *             The rule reads the fp64 states in every precision mode.
 *   failure   max_hold >= 0, the policy of dmpc_transition_hold: 0 stops the scene at the first failed agent; a held plan counts as a solved one
 *             in the rule above.  hold_count, hold_first, agent_status and DMPC_ST_HELD are dmpc_transition_hold's.
 * po, path, P, pk / vk / ak (resident afterwards; dmpc_postcheck* and dmpc_postcheck_clearance take pf = the last waypoints), K_T_used and
 * scene_status are dmpc_transition_hold's: static vehicles with N_cmd < N and no path, scripted ones with a path.  Outputs, each or both NULL:
 *   wp_col    [S][N_cmd][W]   the column on which the agent left waypoint w; -1 where it never did, for its last waypoint and for w >= n_wp
 *   wp_index  [S][N_cmd]      cur[i] when the scene ended
 * W == 1 with timeout == 0: every common output is dmpc_transition_hold's with Q == 1 byte for byte (max_hold == 0: dmpc_transition / _cmd /
 * _scripted).  Every n_wp == W, a capture too small to fire and timeout == T: dmpc_transition_mission on goals[q][i] = waypoints[i][q] with
 * deadline = [T, .., T, 0] byte for byte, wherever no intermediate stage is reached before its deadline.  Batch split as dmpc_transition (each
 * part gets its scenes' waypoints, n_wp and outputs); a DMPC_DEVICE_ALL context runs the call on its first GPU; there is no RCCL form.
 * W < 1, a NULL waypoints, an n_wp entry outside 1 .. W, a capture that is not > 0 (NaN included), timeout < 0, max_hold < 0, or what
 * dmpc_transition_hold refuses of the common arguments: -1 and a message that starts with the entry's name, nothing launched. */
DMPC_API int dmpc_transition_route(dmpc_ctx *ctx, int S, int N, int N_cmd, int W, const double *po, const double *waypoints, const int32_t *n_wp,
                          double capture, int timeout, const double *path, int P, int K_T_max, double error_tol, int max_hold, double *pk,
                          double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status, int32_t *wp_col, int32_t *wp_index,
                          int32_t *hold_count, int32_t *hold_first, int32_t *agent_status);

/* Multi-GPU: the agents of every scene sharded over the GPUs of one node, ONE PROCESS (rank) PER GPU, each with its own
 * context.  Replaces the thread clusters of DMPC::solveParallelDMPCv2 (dmpc/cpp/dmpc.cpp:1570-1686): contiguous agent ranges,
 * N/G each, the first N mod G one more (:1600-1625; dmpc_partition), every cluster reading the previous predictions of all
 * agents (`prev_obs = obs` after the join, :1671-1681; `l = new_l`, dmpc/matlab/dmpc_soft_bound.m:146).  The join is one
 * RCCL all-gather over xGMI per MPC step on the context's stream, the termination test (ReachedGoal.m / the abort of
 * test/failure_rate.m:112-125) a second tiny one grouped with it.
 *   dmpc_comm_unique_id   rank 0: a 128-byte id (ncclGetUniqueId) to hand to every rank by any out-of-band means
 *   dmpc_comm_init        every rank: joins the communicator (ncclCommInitRank on the context's device); nranks = 1 works
 *   dmpc_comm_destroy     leaves it (dmpc_destroy does this too)
 * A context without a communicator behaves as rank 0 of 1 (the exchange is a device copy).
 * Table layout for N agents on G ranks: lT[G][S][3K][Cmax], Cmax = ceil(N/G); the last column of the chunks of the short
 * ranks is padding that is never read. */
DMPC_API int dmpc_partition(int N, int G, int rank, int32_t *lo, int32_t *count, int32_t *cmax);
DMPC_API int dmpc_comm_unique_id(char *id128);
DMPC_API int dmpc_comm_init(dmpc_ctx *ctx, const char *id128, int nranks, int rank);
DMPC_API int dmpc_comm_destroy(dmpc_ctx *ctx);
/* ranks of the context's communicator as RCCL itself counts them (ncclCommCount); the group size of a DMPC_DEVICE_ALL context; 1 otherwise */
DMPC_API int dmpc_comm_size(const dmpc_ctx *ctx);

/* One MPC step of this rank's agents + the exchange (cluster_solvev2 + the join, dmpc.cpp:1656-1686,1792-1841).  Device
 * pointers, asynchronous on `stream`: x_p, x_v, x_a, pf: [S][count][3] and p_out, v_out, a_out: [S][count][3K] of this
 * rank's `count` agents (dmpc_partition); lT, lT_next: the whole table [G][S][3K][Cmax] before / after the step -- every
 * rank's new predictions arrive in its slot of lT_next by the all-gather.  status [S][count], info [S][count][8] or NULL. */
DMPC_API int dmpc_step_sharded_device(dmpc_ctx *ctx, int S, int N, const double *lT, const double *x_p, const double *x_v,
                             const double *x_a, const double *pf, double *p_out, double *v_out, double *a_out,
                             double *lT_next, int32_t *status, int32_t *info, void *stream);

/* The whole transition (dmpc_transition) sharded: every rank passes the SAME start/goal sets po, pf [S][N][3] (host) and gets
 * the histories pk, vk, ak [S][count][K_T_max][3] of ITS agents (or NULL), and the same K_T_used[S] / scene_status[S] as the
 * other ranks (a scene stops on every rank at the step where any agent of any rank fails or all agents reached their
 * goals: the rule of dmpc_transition).  Results do not depend on the number of ranks (bit for bit). */
DMPC_API int dmpc_transition_sharded(dmpc_ctx *ctx, int S, int N, const double *po, const double *pf, int K_T_max, double error_tol,
                            double *pk, double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status);

/* The same, followed by ONE all-gather per history array: every rank then also holds the scene-wide histories [S][N][K_T_max][3]
 * on its device, which is what dmpc_postcheck(.., pk = NULL, ..) checks -- the post-checks of test/failure_rate.m:136-195 after a
 * sharded transition, on any rank (pk, vk, ak still return the rank's own agents).  A DMPC_DEVICE_ALL context does this inside
 * dmpc_transition. */
DMPC_API int dmpc_transition_sharded_gather(dmpc_ctx *ctx, int S, int N, const double *po, const double *pf, int K_T_max, double error_tol,
                                   double *pk, double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status);

/* f-1: the post-checks the reference runs after every transition -- test/failure_rate.m:136-195 (identical
 * blocks: test/comp_kctr.m:141-205, test/comp_hardsoft2.m:140-204, dmpc/matlab/dmpc_soft_bound.m:152-190):
 *   r_factor = min_{i,k} min(amax/|a_k|, vmax/|v_k|), h_scaled = h/sqrt(r_factor)       (:138-146)
 *   rescale  a_k *= r_factor; v,p re-integrated with h_scaled                           (:156-162)
 *   p(t) = spline(tk, pk, 0:Ts:T) (MATLAB not-a-knot cubic), T = (K_T_used-1) h_scaled  (:149-167)
 *   violation = any pair with |E1 (p_i - p_j)| < rmin - 0.05 at any sample              (:170-181)
 *   totdist = sum of sample-to-sample path lengths over all agents                      (:183)
 *   traj_time = Ts * max_i (1 + last sample index with |p_i - pf_i| >= 0.05)            (:186-194)
 * pk, vk, ak: [S][N][KT_alloc][3] un-rescaled histories exactly as dmpc_transition returns them, K_T_used[S]
 * valid columns per scene; pass pk = vk = ak = NULL to use the histories the last dmpc_transition of this
 * context left resident on the device.  Inputs are not modified.  Any output pointer may be NULL.
 * scene_mask (optional, [S]): 0 skips a scene (the reference only post-checks trials that stayed feasible and
 * reached their goals, failure_rate.m:136); skipped scenes report NaN / 0.  A checked scene whose histories are
 * all zero is an error (MATLAB: h_scaled = 0 makes tk empty and spline() fails).
 * p_interp (optional): [S][N][ns_alloc][3] interpolated positions (samples >= n_samples[s] are zero).
 * Any number of agents per scene: up to 256 the pairwise check is the literal all-pairs search; larger scenes bin the agents of every
 * sample into a uniform cell grid (cell = 2 rmin in the metric of the check), test the 27-neighbourhood with the same fp64 expression and
 * fall back to a tiled all-pairs pass for scenes without any pair that close -- min_dist and violation are exact either way.
 * After dmpc_transition on a DMPC_DEVICE_ALL context, or dmpc_transition_sharded_gather, the resident histories are the scene-wide ones. */
DMPC_API int dmpc_postcheck(dmpc_ctx *ctx, int S, int N, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                   const double *pk, const double *vk, const double *ak, const double *pf, double vmax, double amax, double Ts,
                   double *r_factor, double *h_scaled, int32_t *n_samples, double *min_dist, int32_t *violation,
                   double *totdist, double *traj_time, double *p_interp, int ns_alloc);

/* dmpc_postcheck after a transition with uncommanded vehicles.  r_factor, h_scaled, the spline, totdist, traj_time and
 * min_dist / violation are computed over the N_cmd commanded agents exactly as dmpc_postcheck does for N = N_cmd -- what the
 * reference checks: collision_violation(solution) sees the N_cmd trajectories only (dmpc/cpp/dmpc.cpp:2052-2086).  Two more
 * outputs cover what it leaves out: min_dist_static[S] = the smallest |E1 (p_i(t) - po_j)| over every 100 Hz sample of every
 * commanded agent i and every static vehicle j (the same fp64 expression; a static vehicle has no spline, its position is po_j),
 * violation_static[S] = min_dist_static < rmin - 0.05.  Static-static pairs are not examined.
 * pk, vk, ak, pf: [S][N_cmd][..] as for dmpc_postcheck (NULL histories: the resident ones of dmpc_transition_cmd);
 * po_static: [S][N - N_cmd][3], required when N_cmd < N; with N_cmd == N the two outputs are +inf / 0 and everything else is
 * dmpc_postcheck bit for bit.  Either new output may be NULL; masked scenes report NaN / 0. */
DMPC_API int dmpc_postcheck_cmd(dmpc_ctx *ctx, int S, int N, int N_cmd, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                       const double *pk, const double *vk, const double *ak, const double *pf, const double *po_static,
                       double vmax, double amax, double Ts, double *r_factor, double *h_scaled, int32_t *n_samples,
                       double *min_dist, int32_t *violation, double *totdist, double *traj_time, double *p_interp, int ns_alloc,
                       double *min_dist_static, int32_t *violation_static);

/* dmpc_postcheck after dmpc_transition_scripted (no reference counterpart, see there): the arguments of dmpc_postcheck_cmd with po_static
 * replaced by path [S][N - N_cmd][P][3] and P, and the two static outputs by min_dist_scripted[S] / violation_scripted[S]; p_scripted
 * (optional): [S][N - N_cmd][ns_alloc][3], the interpolated positions of the scripted vehicles (samples >= n_samples[s] are zero).
 * All commanded-only outputs are dmpc_postcheck on the N_cmd histories, bit for bit.  A scripted vehicle's position at a 100 Hz sample is
 * the same not-a-knot spline the commanded agents get, on THEIR knots: t_i = i h_scaled, i = 0 .. K_T_used-1, with values sample(j, i) --
 * the path is a path over step indices and is rescaled in time with the fleet; short histories (K_T_used < 4) degenerate as the commanded
 * spline does.  min_dist_scripted = the smallest |E1 (p_i(t) - q_j(t))| over commanded agents i, scripted vehicles j and samples t (the fp64
 * expression of the static check), violation_scripted = min_dist_scripted < rmin - 0.05.  Scripted-scripted pairs are not examined.
 * Requires 1 <= N_cmd < N, P >= 1 and a path; masked scenes report NaN / 0; any output may be NULL. */
DMPC_API int dmpc_postcheck_scripted(dmpc_ctx *ctx, int S, int N, int N_cmd, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                            const double *pk, const double *vk, const double *ak, const double *pf, const double *path, int P,
                            double vmax, double amax, double Ts, double *r_factor, double *h_scaled, int32_t *n_samples,
                            double *min_dist, int32_t *violation, double *totdist, double *traj_time, double *p_interp, int ns_alloc,
                            double *min_dist_scripted, int32_t *violation_scripted, double *p_scripted);

/* Clearance report (no reference counterpart; additive, the ABI revision stays 8): WHICH agent came closest to WHICH vehicle, and WHEN -- what
 * min_dist / violation of the three post-checks above reduce to one number per scene.  Same rescale, same not-a-knot spline, same 100 Hz samples
 * and the same fp64 distance expression; the scripted vehicles of `path` are splined as dmpc_postcheck_scripted does.  Every commanded agent
 * i < N_cmd gets two slots:
 *   slot 0  its nearest commanded partner j != i, j < N_cmd
 *   slot 1  its nearest uncommanded vehicle N_cmd <= j < N: at rest at po_static [S][N-N_cmd][3], or scripted along path [S][N-N_cmd][P][3]
 *           (one of the two, never both; both may be NULL when N_cmd == N)
 * and per slot, in arrays [S][N_cmd][2] (any of them may be NULL):
 *   clear_dist     the smallest |E1 (p_i(t) - p_j(t))| over all samples t < n_samples[s] and all j of the slot's kind
 *   clear_partner  that j, 0-based in the numbering of the table (0 .. N-1)
 *   clear_sample   the 0-based sample; the time is clear_sample * Ts
 * Ties go to the smallest sample, then the smallest partner; the result does not depend on the batch size S, the launch geometry or the order
 * in which the device visits pairs.  Hence min_i clear_dist[s][i][0] == min_dist[s] of dmpc_postcheck, and min_i clear_dist[s][i][1] ==
 * min_dist_static[s] / min_dist_scripted[s], bit for bit.
 * reach (> 0, +inf allowed): a distance in the metric of the check that bounds the search.  A slot whose distance is < reach is exact; a slot
 * with nothing inside reach reports +inf / -1 / -1 (so does slot 1 when N_cmd == N, and slot 0 of an only agent).  With reach = +inf every
 * slot is exact and tables of more than 256 vehicles are searched all-pairs; a finite reach lets them use the cell grid of dmpc_postcheck with
 * cells at least reach wide.  Masked scenes report NaN / -1 / -1 in both slots, whatever N_cmd is.
 * pk, vk, ak: [S][N_cmd][KT_alloc][3] or all three NULL (the resident histories, with dmpc_postcheck's rule on a DMPC_DEVICE_ALL context).
 * po_static together with path, N_cmd < N with neither, reach <= 0 or NaN, only some of pk / vk / ak, P < 1 with a path: -1 and a message
 * that starts with the entry's name, nothing launched.  Static-static and scripted-scripted pairs are not examined. */
DMPC_API int dmpc_postcheck_clearance(dmpc_ctx *ctx, int S, int N, int N_cmd, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                             const double *pk, const double *vk, const double *ak, const double *po_static, const double *path, int P,
                             double vmax, double amax, double Ts, double reach, double *clear_dist, int32_t *clear_partner,
                             int32_t *clear_sample);

/* Flight setpoints and limits report (additive, the ABI revision stays 8): position, velocity AND acceleration of the N commanded agents at the
 * 100 Hz samples of the post-check -- what DMPC::interp_trajectory (dmpc/cpp/dmpc.cpp:1938-2050) returns as pos / vel / acc, what
 * dmpc_soft_bound.m:165-169 computes as spline(tk,pk,t), spline(tk,vk,t), spline(tk,ak,t) and what dmpc_trajectories2file takes -- and, per
 * agent, the largest |v| and |a| over the whole transition with the sample at which it happens.
 * The preamble is dmpc_postcheck's: r_factor, h_scaled, n_samples, the rescaled histories and the position spline are the same bits.  v and a
 * are the same not-a-knot spline on the same knots i * h_scaled through the velocity and acceleration histories AS THE RESCALE LEAVES THEM --
 * including the last acceleration column, which the reference's loop `for k = 1:K-1` (failure_rate.m:156-162) never multiplies by r_factor.
 * v is deliberately NOT the derivative of the position spline (nor a of the velocity spline): the reference interpolates three series
 * independently, and on a recorded transition (tests/golden/postcheck_comp_kctr_2.npz) the two velocities differ by up to 5.3e-2 m/s.
 * Histories with K_T_used < 4 degenerate as the position spline does (parabola / line through the points).
 * pk, vk, ak: [S][N][KT_alloc][3], un-rescaled, or all three NULL (the resident histories under dmpc_postcheck's rules: a split batch is
 * handled part by part where the histories live; a DMPC_DEVICE_ALL context holds the scene-wide ones).  Inputs are never modified.
 * Setpoints: p_sp, v_sp, a_sp [S][N][ns_alloc][3], any of them NULL.  Global sample j (t = j * Ts) with smp0 <= j < min(smp0 + ns_alloc,
 * n_samples[s]) goes to index j - smp0; every other slot is zero.  p_sp with smp0 = 0 is p_interp of dmpc_postcheck byte for byte, and any
 * window is a slice of the full call byte for byte.  Windows that would need more than 256 MB of device memory are produced in several
 * passes.  ns_alloc = 0 with all three NULL is the report alone: no setpoint is stored anywhere and 4 S N numbers come back.
 * Report, arrays [S][N], any of them NULL:
 *   v_peak         max_j |v_i(t_j)| over ALL samples j < n_samples[s] (the window does not restrict it); |x| = sqrt(fma(z, z, fma(y, y, x * x)))
 *   v_peak_sample  the 0-based sample of that maximum; ties go to the smallest sample
 *   a_peak, a_peak_sample   the same for the acceleration
 * The report does not depend on S, the window, the passes, the launch geometry or which outputs are NULL.  The rescale enforces vmax / amax
 * at the knots only; the spline may exceed them in between (on the recorded transition above a_peak of one agent is 1.0044 at amax = 1).
 * Comparing the peaks with the limits is the caller's job.  Masked scenes report NaN / -1 and zero setpoints.
 * -1 with a message that starts with the entry's name and nothing launched: what dmpc_postcheck refuses of the common arguments, smp0 < 0,
 * ns_alloc < 0, a setpoint array with ns_alloc = 0, ns_alloc > 0 without one, only some of pk / vk / ak. */
DMPC_API int dmpc_postcheck_setpoints(dmpc_ctx *ctx, int S, int N, int KT_alloc, const int32_t *K_T_used, const int32_t *scene_mask,
                             const double *pk, const double *vk, const double *ak, double vmax, double amax, double Ts,
                             int smp0, int ns_alloc, double *p_sp, double *v_sp, double *a_sp,
                             double *v_peak, int32_t *v_peak_sample, double *a_peak, int32_t *a_peak_sample,
                             double *r_factor, double *h_scaled, int32_t *n_samples);

/* f-3: dense collision rows behind the CollConstr / AddCollConstr helpers named in the north star.  All of them
 * compute, per neighbour j (E1 = diag(1,1,1/c), E2 = E1^order; the ORDER is the context's, dmpc_params.order: 2, or 4 on a context of an
 * all-neighbour variant -- the helpers are generic in it, CollConstrSoftDMPC.m:16-21, and test/comp_test_ellipconstr.m:158 sets 4):
 *     dist = |E1 (p - p_j)|_order,  diff = E2 (p - p_j).^(order-1),  pd = dist^(order-1),
 *     r = pd (rmin - dist + diff.p/pd) - diff.a0,   Ain(row,:) = -diff_mat * A = -(diff . A(3 k_blk + 1..3, :)),  bin(row) = -r
 * (`dist` below returns pd = prev_dist, what CollConstrSoftDMPC.m:19 hands back: the distance itself for order 2)
 * replacing (file:line)
 *     dec-iSCP/CollConstr.m:1-24                (k_cmp = k-1, k_blk = k-2, a0 = po; all obstacles of `l`)
 *     dmpc/matlab/CollConstrSoftDMPC.m:1-32     (k_cmp = k_blk = k-1, a0 = A_initp(3k-2:3k,:)[po;vo]; `violation` mask)
 *     dmpc/matlab/CollConstrSoftDMPC2.m:8       (k_blk = k-2)     CollConstrHardDMPC.m:19 (all j != n, dist < 1)
 *     CollConstrHardDMPCOnDemand.m, CollConstrEllipDMPC.m, CollConstrSoftDMPCall.m
 * l: [N_obs][K][3] (== MATLAB l(3,K,N_obs)); sel: the n_sel 0-based obstacle indices to build rows for, in output
 * order; k_cmp / k_blk: 0-based horizon column compared / 3-row block of A used; A: a_rows x ncols with element
 * (i,j) at A[i*a_rs + j*a_cs] (MATLAB column-major: a_rs = 1, a_cs = a_rows); Ain: n_sel x ncols with strides
 * o_rs / o_cs; bin, dist (optional): [n_sel].  The *_device form takes device pointers and a HIP stream. */
DMPC_API int dmpc_coll_rows(dmpc_ctx *ctx, int K, int N_obs, int n_sel, const int32_t *sel, const double *l, int k_cmp, int k_blk,
                   const double *p, const double *a0, double rmin, double c, const double *A, int a_rows, int ncols,
                   int64_t a_rs, int64_t a_cs, double *Ain, int64_t o_rs, int64_t o_cs, double *bin, double *dist);
DMPC_API int dmpc_coll_rows_device(dmpc_ctx *ctx, int K, int n_sel, const int32_t *d_sel, const double *d_l, int k_cmp, int k_blk,
                          const double *p, const double *a0, double rmin, double c, const double *d_A, int64_t a_rs,
                          int64_t a_cs, int ncols, double *d_Ain, int64_t o_rs, int64_t o_cs, double *d_bin, double *d_dist,
                          void *stream);

/* dense form of structured rows as dmpc_rows_one returns them: Ain(r,:) = -(xi_r . A(3 kc_r - 2 .. 3 kc_r, :)), kc 1-based
 * (`Ain_total(idx,:) = -diff_mat*Ain`, CollConstrSoftDMPC.m:24-27).  xi [nr][3], kc [nr]; A / Ain strided as above. */
DMPC_API int dmpc_rows_dense(dmpc_ctx *ctx, int nr, const double *xi, const int32_t *kc, const double *A, int a_rows, int ncols,
                    int64_t a_rs, int64_t a_cs, double *Ain, int64_t o_rs, int64_t o_cs);

/* cup-SCP/AddCollConstr.m:1-31: the K N(N-1)/2 pairwise rows (pairs i<j in order, k fastest) of the coupled QP
 *     r = dist (rmin - dist) + diff.(p_i,k - p_j,k) - diff.(po_i - po_j)
 *     Ain(row,:) = -(diff . A(blk(i,k),:) - diff . A(blk(j,k),:)),  blk(i,k) = rows 3K(i-1)+3(k-1)+1..3;  bin = -r
 * p: [N][K][3] (== MATLAB p(3,K,N)); po: [N][3]; A: 3KN x ncols (strided as above); Ain: K N(N-1)/2 x ncols. */
DMPC_API int dmpc_add_coll_constr(dmpc_ctx *ctx, int K, int N, const double *p, const double *po, double rmin, double c,
                         const double *A, int ncols, int64_t a_rs, int64_t a_cs, double *Ain, int64_t o_rs, int64_t o_cs,
                         double *bin);
DMPC_API int dmpc_add_coll_constr_device(dmpc_ctx *ctx, int K, int N, const double *d_p, const double *d_po, double rmin, double c,
                                const double *d_A, int64_t a_rs, int64_t a_cs, int ncols, double *d_Ain, int64_t o_rs,
                                int64_t o_cs, double *d_bin, void *stream);

/* f-2: the reference's on-disk result formats (host code, no context needed; return 0 / -1 + dmpc_last_error(NULL)).
 * dmpc_trajectories2file == DMPC::trajectories2file (dmpc/cpp/dmpc.cpp:2088-2126), the text file
 * dmpc/cpp_results/read_result.m:4-44 reads: header `N N_cmd h_scaled pmin' pmax'`, then po (3 x N), pf (3 x N_cmd),
 * then the 3 x T position block of every trajectory, then the velocity blocks, then the acceleration blocks -- each
 * matrix in Eigen's default stream format (6 significant digits, columns aligned per matrix), byte for byte.
 * po [N][3], pf [N_cmd][3], pos/vel/acc [N_cmd][T][3] (== MATLAB pk(3,T,N_cmd)). */
DMPC_API int dmpc_trajectories2file(const char *path, int N, int N_cmd, int T, double h_scaled, const double *pmin,
                           const double *pmax, const double *po, const double *pf, const double *pos,
                           const double *vel, const double *acc);
/* test2file (dmpc/cpp/cluster_test.cpp:9-33; read by dmpc/cpp_results/cluster_test.m): header
 * `n_cluster n_vehicles n_trials`, the cluster sizes and vehicle counts, then one n_vehicles x n_trials block of
 * wall times per cluster size.  times [n_cluster][n_vehicles][n_trials]. */
DMPC_API int dmpc_test2file(const char *path, int n_cluster, int n_vehicles, int n_trials, const double *cluster_size,
                   const double *num_vehicles, const double *times);

/* f-2: the reference's start/goal generators for S scenes at once.
 * dmpc_random_test     == randomTest.m:1-60: N starts and, independently, N goals uniform in [pmin, pmax], each
 *                         farther than rmin (|E1 (p_i - p_j)|_2, E1 = diag(1,1,1/c)) from the earlier points of its
 *                         set; rejection sampling, <= 200000 tries per point, else the set restarts.
 * dmpc_random_exchange == randomExchange.m:1-57: starts as above with the Euclidean distance, goals = starts
 *                         permuted by the .m's draw-without-replacement rule (no agent keeps its own start).
 * po, pf: [S][N][3].  MATLAB's global rand stream cannot be reproduced: draws come from a counter-based stream
 * (splitmix64 of seed, scene, set, draw index), so a (seed, S, N, box, rmin) tuple always gives the same scenes.
 * The _device form writes [2][S][N][3] (starts, then goals) to device memory on the caller's stream. */
DMPC_API int dmpc_random_test(dmpc_ctx *ctx, int S, int N, const double *pmin, const double *pmax, double rmin, double c,
                     uint64_t seed, double *po, double *pf);
DMPC_API int dmpc_random_exchange(dmpc_ctx *ctx, int S, int N, const double *pmin, const double *pmax, double rmin, uint64_t seed,
                         double *po, double *pf);
DMPC_API int dmpc_random_sets_device(dmpc_ctx *ctx, int S, int N, const double *pmin, const double *pmax, double rmin, double c,
                            uint64_t seed, int exchange, double *d_po_pf, void *stream);

/* Goal assignment ahead of a transition: S scenes of N agents at po and N goals, both [S][N][3]; which agent takes which goal is the
 * library's choice: the permutation that minimises sum_i c(i, perm[i]), c(i,j) = |E1 (po_i - g_j)|^2 with E1 = diag(1,1,1/c) of the context's
 * parameters -- the metric of the collision ellipsoid.  For that labelling (po_i - po_j)' E1^2 (g_i - g_j) >= 0 for every pair, so two agents
 * on initDMPC's straight lines never come closer than min(|po_i - po_j|, |g_i - g_j|) / sqrt(2) in that metric.  No reference counterpart.
 * The rule is pinned so that the result depends on nothing but the inputs (tests/assign.py restates it; the device equals it bit for bit):
 *   cost      cinv = 1.0 / c; dx, dy = po_i - g_j; dz = (po_i - g_j)_z * cinv; c(i,j) = (dx*dx + dy*dy) + dz*dz, each operation rounded on its own
 *   solver    forward auction with eps-scaling in synchronous (Jacobi) rounds: cmax = max c(i,j); price = 0;
 *             e = cmax / 4; while (e > eps) { phase(e); e = e / 4; } phase(eps).  A phase unassigns every agent, keeps the prices, and runs
 *             rounds until no agent is unassigned.
 *   round     every agent i unassigned at its start takes m_j = c(i,j) + price[j] over all goals; j1 = the smallest m_j (ties: the smallest j),
 *             m2 = the smallest over j != j1; it bids (price[j1] + (m2 - m_j1)) + e for j1 (N == 1: price[0] + e).  After all bids every goal that
 *             received one goes to the highest bidder (ties: the smallest i), its price becomes that bid, its previous owner is unassigned.
 *   cap       rounds counts the rounds of all phases; a scene that would need more than max_rounds (<= 0: 1 << 20) stops and reports
 *             rounds = -1, perm = -1 everywhere, cost = NaN and pf_assigned zero (price: as the rounds left it); the other scenes are unaffected.
 * On return m_perm[i] - min_j m_j <= eps for every agent up to rounding, hence a total within N eps of the optimum.
 * perm [S][N] (the goal of agent i), pf_assigned [S][N][3] = goals[perm[i]], price [S][N] (per goal), cost [S] = sum of c(i, perm[i]) in
 * increasing i, rounds [S]; any output may be NULL.  fp64 whatever the context's precision; a DMPC_DEVICE_ALL context runs the call on its
 * first GPU; a fleet with uncommanded vehicles passes its commanded agents only.  Refused (-1, nothing launched): S < 1, N < 1, po or goals
 * NULL, eps not a finite positive number.
 * The _device form takes device pointers and enqueues on the caller's stream; scenes of more than 1024 agents take round launches, whose
 * done flags the host reads window by window, so for them the call returns only once every scene has finished. */
DMPC_API int dmpc_assign_goals(dmpc_ctx *ctx, int S, int N, const double *po, const double *goals, double eps, int max_rounds,
                      int32_t *perm, double *pf_assigned, double *price, double *cost, int32_t *rounds);
DMPC_API int dmpc_assign_goals_device(dmpc_ctx *ctx, int S, int N, const double *po, const double *goals, double eps, int max_rounds,
                             int32_t *perm, double *pf_assigned, double *price, double *cost, int32_t *rounds, void *stream);

/* Rectangular goal assignment (additive, the ABI revision stays 8): S scenes of N agents at po [S][N][3] and M goals [S][M][3], N, M >= 1.
 * More goals than agents (a formation with spare slots, a field of landing pads): the library chooses the cheapest N of the M points and says
 * which stay empty.  Fewer goals than agents (the next figure needs 80 of the 100 drones): it chooses which M fly; the others are sent nowhere
 * (pf_assigned = po) and stay commanded agents, so they still dodge.  The total sum of c(i, perm[i]) over the n = min(N, M) matched pairs
 * is minimised over all ways to match n pairs; c as dmpc_assign_goals.  No reference counterpart.  dmpc_assign_goals itself is unchanged.
 * The rule -- a forward/reverse auction with eps-scaling in synchronous (Jacobi) rounds -- is pinned so that the result depends on nothing but
 * the inputs (tests/assign_rect.py restates it; the device equals it bit for bit).  m = max(N, M).
 *   persons   the smaller side are the persons, the larger side the objects: agents are persons when N <= M, goals are persons when N > M;
 *             p and o are agent or goal indices.
 *   cost      c(p,o) is always computed from the agent-goal pair: cinv = 1.0 / c; dx, dy = po_i - g_j; dz = (po_i - g_j)_z * cinv;
 *             (dx*dx + dy*dy) + dz*dz, each operation rounded on its own; no fused multiply-add anywhere in the rule.
 *   schedule  cmax = max c over all N M pairs; price[o] = 0 for every object;
 *             e = cmax / 4; while (e > eps) { forward(e); reverse(e); e = e / 4; } forward(eps); reverse(eps).
 *   forward   dmpc_assign_goals' phase with objects in the place of goals: every person unassigned and every object unowned, prices kept; rounds
 *             until no person is unassigned.  In a round every person p unassigned at its start takes v_o = c(p,o) + price[o] over all objects;
 *             o1 = the smallest v (ties: the smallest o), v2 = the smallest over o != o1; it bids (price[o1] + (v2 - v1)) + e (m == 1:
 *             price[0] + e).  Every object with bids goes to its highest bidder (ties: the smallest p), its price becomes that bid, its previous
 *             owner is unassigned.
 *   reverse   nothing when n == m.  Setup: u[p] = c(p, o_p) + price[o_p] for every person and its object o_p; lambda = the smallest price over
 *             the owned objects, fixed for this call.  Rounds until no object is unowned with price > lambda.  In a round every such object o,
 *             from the state at the round's start, takes g_p = u[p] - c(p,o) over all persons; p1 = the largest g (ties: the smallest p),
 *             beta = g_p1, omega = the largest over p != p1 (n == 1: -inf).  lambda >= beta - e: price[o] = lambda and the object is done.
 *             Otherwise it offers delta = min(beta - lambda, (beta - omega) + e) > 0 to p1.  Then every person with offers takes the largest
 *             delta (ties: the smallest o): price[o] = beta_o - delta, u[p] = u[p] - delta, the person's previous object becomes unowned with
 *             its price as it is, the person owns o.  An object whose offer was not taken changes nothing and offers again next round.
 *   cap       rounds counts forward and reverse rounds alike; a scene that would need more than max_rounds (<= 0: 1 << 20) reports
 *             rounds = -1, perm = -1, owner = -1, cost = NaN, pf_assigned zero and price as the rounds left it; the other scenes are unaffected.
 * On return every person's object is within eps of its best in c + price, up to rounding, and no unowned object is priced above an owned one,
 * up to rounding: hence a total within n eps of the optimum over all ways to match n pairs.  With N == M every output equals dmpc_assign_goals'
 * on the same inputs bit for bit (no reverse round runs) and owner is the inverse of perm.
 * perm [S][N] (the goal of agent i, or -1), owner [S][M] (the agent of goal j, or -1), pf_assigned [S][N][3] = goals[perm[i]], or po_i bit for
 * bit where perm[i] = -1, price [S][max(N, M)] per object (per goal when N <= M, per agent otherwise), cost [S] = the sum of c(i, perm[i])
 * over the assigned agents in increasing i, rounds [S]; any output may be NULL.  fp64 whatever the context's precision; a DMPC_DEVICE_ALL
 * context runs the call on its first GPU.  Refused (-1, nothing launched, a message that starts with the entry's name): S, N or M < 1; po or
 * goals NULL; eps not a finite positive number; max(N, M) > DMPC_ASSIGN_ONE_LAUNCH_MAX (1024; the message has both counts).  The whole auction
 * of a scene runs in one workgroup's LDS; a round-launch path for larger rectangular scenes does not exist (larger SQUARE scenes go through
 * dmpc_assign_goals).  The _device form takes device pointers and enqueues one launch on the caller's stream. */
DMPC_API int dmpc_assign_rect(dmpc_ctx *ctx, int S, int N, int M, const double *po, const double *goals, double eps, int max_rounds,
                     int32_t *perm, int32_t *owner, double *pf_assigned, double *price, double *cost, int32_t *rounds);
DMPC_API int dmpc_assign_rect_device(dmpc_ctx *ctx, int S, int N, int M, const double *po, const double *goals, double eps, int max_rounds,
                            int32_t *perm, int32_t *owner, double *pf_assigned, double *price, double *cost, int32_t *rounds, void *stream);

/* Route planning ahead of a transition (additive, the ABI revision stays 8): which way round the static vehicles every commanded agent goes.
 * DMPC has no global planner -- an agent whose straight line is blocked by a wall of uncommanded vehicles parks in front of it -- and
 * dmpc_transition_route flies waypoints somebody has to supply; this entry supplies them.  No reference counterpart.
 * S scenes; po_cmd and goals [S][N_cmd][3]: the commanded agents' starts and goals; obst [S][M][3], M >= 0 (NULL allowed when M == 0): the
 * vehicles to go round (the rows of po behind the commanded ones; a caller may add a snapshot of scripted vehicles).  Commanded agents do not
 * block each other: keeping them apart is DMPC's job.  rmin, c, pmin and pmax are the context's.
 * The rule is pinned so that the result depends on nothing but the inputs (tests/plan.py restates it; the device equals it bit for bit).  Every
 * fp64 operation is rounded on its own, no fused multiply-add; everything after the blocked predicate is integer arithmetic:
 *   grid      n_a = max(1, (int)ceil((pmax_a - pmin_a) / cell)) cells per axis; the cell of a point is clamp((int)floor((p_a - pmin_a) / cell),
 *             0, n_a - 1) -- points outside the box are clamped --, its centre pmin_a + (i_a + 0.5) * cell.  n_x n_y n_z <= DMPC_PLAN_MAX_CELLS.
 *   blocked   a cell is blocked if for some obstacle m (dx*dx + dy*dy) + dz*dz < R*R with dx, dy = centre - obst_m, dz = (centre - obst_m)_z * cinv,
 *             cinv = 1.0 / c, R = rmin + margin.  For agent i with start cell s_i (of po_cmd) and goal cell g_i:
 *             free_i(q) = !blocked(q) || q == s_i || q == g_i.
 *   field     D(g_i) = 0; level L+1 is every unlabelled cell with free_i that has a 6-neighbour at level L; the sweep stops once s_i is labelled
 *             or a level adds nothing.  s_i unlabelled: DMPC_PLAN_UNREACHABLE, n_wp = 1, every slot the goal, hops = -1.  Else hops = D(s_i).
 *   descent   the path c_0 = s_i .. c_H = g_i: from c_t the first neighbour in the order -x, +x, -y, +y, -z, +z with D = D(c_t) - 1.
 *   clear     clear(a, b) with L = max_axis |b - a|: for j = 0 .. 2L the cell q_axis = (2L a_axis + j (b_axis - a_axis) + L) / (2L) (integer
 *             division) must be free_i.
 *   pruning   anchor t0 = 0; until t0 == H: t1 = the largest t > t0 that is t0 + 1 or has clear(c_t0, c_t); emit t1; t0 = t1.  A waypoint is
 *             the centre of c_t, except that an emitted t == H is the goal itself, bit for bit.  H == 0: n_wp = 1.  More than W emissions: the
 *             first W - 1 are kept, the goal takes slot W - 1, DMPC_PLAN_TRUNCATED.  Slots from n_wp on hold the goal.
 * waypoints [S][N_cmd][W][3], n_wp, plan_status, hops [S][N_cmd] int32; any output may be NULL.  waypoints and n_wp are laid out as
 * dmpc_transition_route takes them.  fp64 whatever the context's precision; a DMPC_DEVICE_ALL context runs the call on its first GPU; there
 * is no RCCL form.  Refused (-1, nothing launched, a message that starts with the entry's name): S < 1, N_cmd < 1, M < 0, W < 1; po_cmd or goals
 * NULL, obst NULL with M > 0; cell or margin not finite, cell <= 0, margin < 0; more than DMPC_PLAN_MAX_CELLS cells (the message has the count).
 * The _device form takes device pointers and enqueues on the caller's stream. */
#define DMPC_PLAN_MAX_CELLS 32768
#define DMPC_PLAN_OK 0
#define DMPC_PLAN_TRUNCATED 1
#define DMPC_PLAN_UNREACHABLE 2
DMPC_API int dmpc_plan_routes(dmpc_ctx *ctx, int S, int N_cmd, int M, int W, const double *po_cmd, const double *goals, const double *obst,
                     double cell, double margin, double *waypoints, int32_t *n_wp, int32_t *plan_status, int32_t *hops);
DMPC_API int dmpc_plan_routes_device(dmpc_ctx *ctx, int S, int N_cmd, int M, int W, const double *po_cmd, const double *goals, const double *obst,
                            double cell, double margin, double *waypoints, int32_t *n_wp, int32_t *plan_status, int32_t *hops, void *stream);

/* Re-planned routes (additive, the ABI revision stays 8): dmpc_plan_routes before column 0, dmpc_transition_route from there, and DURING THE FLIGHT
 * the route of every agent whose remaining legs are no longer clear is planned again, on the device, between two steps.  dmpc_plan_routes plans
 * once against points that do not move; with scripted vehicles that is a guess, and dmpc_transition_route flies the guess to the end.  No reference
 * counterpart.  po, path, P, K_T_max, error_tol, max_hold, capture, timeout, pk / vk / ak, K_T_used, scene_status, wp_col, wp_index and the hold
 * outputs are dmpc_transition_route's; W, cell and margin dmpc_plan_routes'; goals [S][N_cmd][3]; every >= 0 columns (0: never re-planned);
 * ahead >= 0 columns.  tests/replan.py restates the rule; the device equals it bit for bit:
 *   obst(k)   the obstacle set on column k.  With a path: the points sample(j, k + a), a = 0 .. ahead, of every scripted vehicle j -- M (ahead + 1)
 *             points, sample(j, t) = path[s][j][min(t, P - 1)].  Without one: po[s][N_cmd ..], the same on every column.
 *   blocked(k) dmpc_plan_routes' blocked predicate over obst(k), on the same grid.
 *   column 0  waypoints, n_wp, plan_status = dmpc_plan_routes(po_cmd, goals, obst(0)); cur = since = 0; the flight is dmpc_transition_route's.
 *   checked   after the route rule of column k, the waypoint switches of that column included, when every > 0, 0 < k < K_T_max - 1,
 *             k % every == 0 and the scene is still running behind that rule (it has neither failed nor reached).
 *   legs      of agent i: between the cells of x_p_i(k) (the fp64 state in every precision mode), wp[i][cur], .., wp[i][n_wp - 1].  A leg a -> b
 *             is clear when clear(a, b) of the plan rule holds on blocked(k) with free_i = !blocked(k) or the agent's current cell or its goal's
 *             cell; a leg with a == b when that one cell is free_i.
 *   re-plan   some leg not clear: the agent's row of waypoints, n_wp and plan_status become the plan rule's output for start x_p_i(k), goal_i and
 *             blocked(k) (DMPC_PLAN_UNREACHABLE: the goal alone, as it is); cur = 0, since = k, the next step is solved with the new waypoint 0,
 *             which is first examined on column k + 1; the agent's wp_col row goes back to -1; replan_count[i] += 1, replan_col[i] = k.
 *             The table is not rewritten.  A held agent counts as solved, as in the route rule.
 * All floating point ends with the cell of a point and the blocked predicate, so nothing depends on launch geometry, the batch split or the order
 * in which the device visits agents.  Outputs, each may be NULL: waypoints_out [S][N_cmd][W][3], n_wp_out, plan_status [S][N_cmd]: the plan in
 * force when the scene ended (wp_col and wp_index refer to it); replan_count [S][N_cmd]; replan_col [S][N_cmd]: the last re-plan's column, -1 if
 * the agent never was re-planned.  every == 0: every common output is dmpc_plan_routes on obst(0) followed by dmpc_transition_route, byte for
 * byte.  Commanded agents do not block each other; a re-plan sees `ahead` columns and no further; there is no hysteresis beyond `every`.
 * Batch split as dmpc_transition_route; a DMPC_DEVICE_ALL context runs the call on its first GPU; there is no RCCL form.  Refused (-1, nothing
 * launched, a message that starts with the entry's name): what dmpc_plan_routes and dmpc_transition_route refuse of the common arguments,
 * every < 0, ahead < 0, a NULL goals.
 * dmpc_replan_routes_device is ONE re-plan step (check, then plan the flagged agents) on device arrays, enqueued on the caller's stream, for
 * callers that loop over dmpc_step_device_cmd themselves: x_p, goals [S][N_cmd][3]; obst [S][M][3] = obst(k), gathered by the caller; waypoints
 * [S][N_cmd][W][3], n_wp, cur [S][N_cmd] are read and, for a re-planned agent, rewritten; since, wp_col [S][N_cmd][W], pf [S][N_cmd][3] (the goal the
 * next step takes), plan_status, replan_count, replan_col may be NULL; scene_done [S] or NULL: scenes with a non-zero word are skipped.  k is
 * the column written into since and replan_col.  M == 0: nothing is blocked, nothing is launched.  It refuses what dmpc_plan_routes_device
 * refuses, a NULL waypoints, n_wp or cur, k < 0 and a DMPC_DEVICE_ALL context. */
DMPC_API int dmpc_transition_replan(dmpc_ctx *ctx, int S, int N, int N_cmd, int W, const double *po, const double *goals, double cell, double margin,
                           int every, int ahead, double capture, int timeout, const double *path, int P, int K_T_max, double error_tol,
                           int max_hold, double *pk, double *vk, double *ak, int32_t *K_T_used, int32_t *scene_status, double *waypoints_out,
                           int32_t *n_wp_out, int32_t *plan_status, int32_t *wp_col, int32_t *wp_index, int32_t *replan_count,
                           int32_t *replan_col, int32_t *hold_count, int32_t *hold_first, int32_t *agent_status);
DMPC_API int dmpc_replan_routes_device(dmpc_ctx *ctx, int S, int N_cmd, int M, int W, const double *x_p, const double *goals, const double *obst,
                              double cell, double margin, int k, double *waypoints, int32_t *n_wp, int32_t *cur, int32_t *since,
                              int32_t *wp_col, double *pf, int32_t *plan_status, int32_t *replan_count, int32_t *replan_col,
                              const int32_t *scene_done, void *stream);

/* Disturbed transitions (additive, the ABI revision stays 8): WIND, NOISE AND PUSHES ON THE STATE, IN THE LOOP.  NO REFERENCE COUNTERPART: in
 * every closed loop of this header the state of column k is, bit for bit, entry 0 of the plan solved on column k-1 -- the vehicle is never
 * anywhere but where the model put it.  A disturbance is a SETTING OF THE CONTEXT: while one is set, dmpc_transition, _cmd, _scripted, _mission,
 * _hold, _route and _replan add it to the state of every commanded agent between the state advance and the history record of every column
 * k >= 1; with none set every entry launches what it launched before and returns the same bytes.  tests/disturb.py restates the rule; the
 * device, dmpc_disturbance_sample on the host and that restatement agree bit for bit.
 *   the rule  for scene s (its index IN THE CALL, also when the batch is split over contexts), commanded agent i, column k >= 1, component
 *             c = 0, 1, 2, in fp64, every operation rounded on its own (no fused multiply-add); uniform(seed, sid, ctr) is the counter-based
 *             stream of dmpc_random_test (53 bits in [0, 1)), h the context's step:
 *               sid  = (uint64) s << 32 | i
 *               u_j  = 2.0 * uniform(seed, sid, 6 * k + j) - 1.0                      j = 0 .. 5
 *               w    = wind[s] (wind_scenes == 1: wind[0]; no wind: 0)
 *               dp_c = ((0.5 * h) * h) * w_c;  if amp_p > 0: dp_c = dp_c + amp_p * u_c;
 *                      then, in list order, every push with (scene, agent, column) == (s, i, k): dp_c = dp_c + push.dp[c]
 *               dv_c = h * w_c;                if amp_v > 0: dv_c = dv_c + amp_v * u_(3+c);   then the same pushes' dv[c]
 *               x_p_c = x_p_c + dp_c;   x_v_c = x_v_c + dv_c
 *             Column 0 is never disturbed; x_a never is.  Nothing depends on launch geometry or on the batch split.
 *   the place in column k >= 1: solve; hold rule; state advance; DISTURBANCE; history record; verdict; mission / route / re-plan rule.  So the
 *             histories hold the disturbed state, ReachedGoal and the waypoint rule are evaluated on it, and the next solve starts from it.  THE
 *             PREDICTION TABLE IS NOT TOUCHED: a neighbour's view of the agent is stale for one column.  Every commanded agent of a scene that
 *             was running when the column began is disturbed, whether its solve succeeded, was held or failed (a failed agent's state is the
 *             previous column's, plus the disturbance); scenes that are over are skipped.
 *   dmpc_set_disturbance copies everything (the pushes sorted by scene, agent and column, list order kept among equal keys); d == NULL, or a
 *             descriptor that is all zero, clears.  A push on a column at or behind K_T_max is legal and never applied.
 *   dmpc_disturbance_sample: dp, dv [S][N_cmd][3] of column k by the rule, on the host -- no context, no GPU; k == 0 gives zeros.
 *   dmpc_disturb_device: the disturbance of column k on device arrays x_p, x_v [S][N_cmd][3], enqueued on the caller's stream, for callers that
 *             loop over dmpc_step_device_cmd themselves (behind dmpc_advance_device); scene_done [S] or NULL: scenes with a non-zero word are
 *             skipped.  With no disturbance set it returns 0 and launches nothing.
 * Batch split as dmpc_transition.  A DMPC_DEVICE_ALL context with a disturbance set runs the call unsharded on its first GPU;
 * dmpc_transition_sharded[_gather] refuse while one is set; there is no RCCL form.  Not modelled here: disturbed uncommanded or scripted
 * vehicles.  A planning state apart from the true one and re-anchoring of the agent's table column: dmpc_set_feedback, below.
 * Refused (-1, nothing launched, a message that starts with the entry's name) by dmpc_set_disturbance and dmpc_disturbance_sample: a negative or
 * non-finite amp_p or amp_v, a non-finite wind or push value, n_push < 0, wind_scenes < 0, a NULL array with a positive count, a push with
 * scene < 0, agent < 0 or column < 1.  By a transition entry, dmpc_disturbance_sample and dmpc_disturb_device: wind_scenes neither 0, 1 nor S, a
 * push with scene >= S or agent >= N_cmd.  dmpc_disturb_device also: k < 1, a NULL x_p or x_v, a DMPC_DEVICE_ALL context. */
typedef struct dmpc_push { int32_t scene, agent, column; double dp[3], dv[3]; } dmpc_push;
typedef struct dmpc_disturbance {
    uint64_t seed;
    double amp_p, amp_v;                   /* half-widths of the uniform noise on position (m) and velocity (m/s); >= 0, finite */
    const double *wind; int wind_scenes;   /* acceleration [wind_scenes][3] (m/s^2) or NULL / 0; 1: the same for every scene, else == S of the call */
    const dmpc_push *push; int n_push;     /* listed impulses or NULL / 0 */
} dmpc_disturbance;
DMPC_API int dmpc_set_disturbance(dmpc_ctx *ctx, const dmpc_disturbance *d);
DMPC_API int dmpc_disturbance_sample(const dmpc_disturbance *d, double h, int S, int N_cmd, int k, double *dp, double *dv);
DMPC_API int dmpc_disturb_device(dmpc_ctx *ctx, int S, int N_cmd, int k, double *x_p, double *x_v, const int32_t *scene_done, void *stream);

/* Start in motion (additive, the ABI revision stays 8): A FLIGHT FROM A GIVEN OR CARRIED STATE AND PLAN.  NO REFERENCE COUNTERPART: the
 * reference flies one leg, every agent at rest at the start.  A start is a one-shot SETTING OF THE CONTEXT.
 * THE START IS CONSUMED BY ONE FLIGHT: the next of dmpc_transition, _cmd, _scripted, _mission, _hold, _route, _replan that passes its own
 * argument checks uses it and clears it; a refused call leaves it armed; with none armed every entry launches what it launched before and
 * returns the same bytes.
 *   column 0  of that flight, instead of initDMPC: for every commanded agent x_p = its row of the call's po, x_v = vo, x_a = ao (history column
 *             0 records these); its column of the first table = plan_p [3K], entry kk where it expects to be on column kk (entry 0 is not
 *             checked against x_p: a disturbed state is not on its plan).  Hold mode: the "previous plan" of column 1 is (plan_p, plan_v,
 *             plan_a); plan_v / plan_a absent: zeros; the run counters start at 0.  Uncommanded vehicles as ever.
 *   no plan   (plan_p NULL): THE BRAKING PLAN, made on the device, per agent and axis, in fp64, every operation rounded on its own (no fused
 *             multiply-add) -- the hold policy's braking tail K-1 times:
 *               p[0] = x_p, v[0] = x_v, a[0] = x_a;   for kk = 1 .. K-1:
 *               a[kk] = min(max(-v[kk-1] / h, -alim), alim);  v[kk] = v[kk-1] + h * a[kk];  p[kk] = (p[kk-1] + h * v[kk-1]) + ((0.5 * h) * h) * a[kk]
 *             dmpc_start_plan is the rule on the host (no context, no GPU), dmpc_start_plan_device its kernel on device rows [n][3K] for
 *             callers of dmpc_step_device_cmd; tests/start.py restates it; the three agree bit for bit.  n states [n][3]; any output NULL.
 *   col0      COLUMN 0 IS THE CALLER'S COLUMN col0: local column k is the caller's column col0 + k in exactly two places -- the scripted window
 *             is sample(j, col0 + k-1+kk), and the disturbance rule uses col0 + k for the stream counter and for a push's column.  Local column
 *             0 is never disturbed.  Deadlines, timeouts, K_T_used, stage_col, wp_col, hold_first and the histories count local columns.
 *   behind column 0 everything is the entry's own loop: ReachedGoal on column 0 against the new goals (a scene can end there), the stop rule,
 *             the mission / route / re-plan rules (dmpc_transition_replan plans its first routes from the start's positions), hold, disturbance.
 *   the end   of a flight: scene s ends on column e = K_T_used[s] - 1; its end is x_p, x_v, x_a of column e, every commanded agent's plan of
 *             the step that produced column e (e = 0: the plan column 0 was built from) and col = col0 + e.  Kept for scenes that ended
 *             DMPC_ST_SOLVED (with or without _REACHED, _HELD), until the next call on the context that uses the step scratch (any step or
 *             transition entry; not the post-checks).  dmpc_flight_end copies it to the host ([S][N_cmd][3],
 *             [S][N_cmd][3K], [S]; any output NULL).
 *   from_end  = 1: the start is the end of this context's last flight, gathered ON THE DEVICE when dmpc_set_start is called (so later calls may
 *             reuse the scratch): scene s starts where scene src_scene[s] of that flight ended (NULL: identity, S equal), col0 is added to
 *             that end's col.  vo, ao and the plans must be NULL; the commanded rows of the flight's po are ignored (they must still be
 *             passed), the uncommanded rows are read as ever.
 * Batch split as dmpc_transition (results do not depend on it); src_scene on the end of a split flight is refused.  A DMPC_DEVICE_ALL context
 * runs a flight with a start on its first GPU; from_end and dmpc_flight_end after a sharded flight are refused;
 * dmpc_transition_sharded[_gather] refuse while a start is armed; there is no RCCL form.
 * Refused (-1, nothing launched, a message that starts with the entry's name): S or N_cmd < 1, col0 < 0, plan_v without plan_a or without
 * plan_p, host arrays together with from_end, src_scene without from_end or with an entry out of range, a source scene that did not end
 * SOLVED (named by index), no valid flight end on the context, a non-finite value; by a flight: S / N_cmd other than the armed start's. */
typedef struct dmpc_start {
    int32_t S, N_cmd;                        /* of the flight it arms; that flight must match or is refused */
    int32_t from_end;                        /* 0: the host arrays below; 1: the end of this context's last flight, on the device */
    const int32_t *src_scene;                /* from_end only, [S]: scene s starts where scene src_scene[s] of that flight ended; NULL: identity, S equal */
    const double *vo, *ao;                   /* [S][N_cmd][3] or NULL = zeros                                  (from_end: must be NULL) */
    const double *plan_p, *plan_v, *plan_a;  /* [S][N_cmd][3K]; plan_p NULL: the braking plan; plan_v and plan_a both or neither, only with plan_p */
    int32_t col0;                            /* >= 0; from_end: added to the end's col */
} dmpc_start;
DMPC_API int dmpc_set_start(dmpc_ctx *ctx, const dmpc_start *start);   /* NULL clears */
DMPC_API int dmpc_flight_end(dmpc_ctx *ctx, int S, int N_cmd, double *x_p, double *x_v, double *x_a, double *plan_p, double *plan_v, double *plan_a,
                    int32_t *col);
DMPC_API int dmpc_start_plan(const dmpc_params *prm, int n, const double *x_p, const double *x_v, const double *x_a, double *plan_p, double *plan_v,
                    double *plan_a);
DMPC_API int dmpc_start_plan_device(dmpc_ctx *ctx, int n, const double *x_p, const double *x_v, const double *x_a, double *plan_p, double *plan_v,
                           double *plan_a, void *stream);

/* Event-triggered feedback (additive, the ABI revision stays 8): THE PLANNING STATE APART FROM THE TRUE STATE.  NO REFERENCE COUNTERPART (the rule
 * is the one the reference author's follow-up describes: plan from your own prediction while the vehicle tracks it, re-initialise from the
 * vehicle's state only when the tracking error passes a threshold).  A feedback policy is a SETTING OF THE CONTEXT, persistent like the
 * disturbance: dmpc_set_feedback(ctx, fb); NULL clears.  It is honoured by dmpc_transition, _cmd, _scripted, _mission, _hold, _route and
 * _replan.  WITHOUT A DISTURBANCE THE POLICY IS INERT (e == 0 for ever): such a flight, like one with no policy, enqueues what it enqueued before
 * and returns the same bytes.  tests/feedback.py restates the rule; the loop, dmpc_feedback_device, dmpc_feedback_apply_host and that
 * restatement agree bit for bit.
 *   per commanded agent: the TRUE state x = (x_p, x_v) -- recorded in the histories, judged by ReachedGoal, read by the route, re-plan and mission
 *             rules, exactly as before; the PLANNING state xh the solver starts from; the tracking error e = (e_p, e_v).
 *   column 0: xh = x, e = 0 -- also in a flight with a start (dmpc_set_start), WHATEVER THE PREVIOUS FLIGHT ENDED WITH: e is not carried
 *             across dmpc_flight_end.  So with trigger = (0, 0) every column ends with e == 0 and cut-and-continue stays bit-identical; with other
 *             thresholds it need not.
 *   column k >= 1, for every commanded agent of a scene that was running when the column began, behind the solve and the hold rule.  Its plan
 *             rows are p, v, a [3K]; d = (dp, dv) is the disturbance of the column by the rule above (none set: 0).  fp64, every operation
 *             rounded on its own (no fused multiply-add), per component c:
 *               advanced (its status after the hold rule has DMPC_ST_SOLVED):
 *                     q_p = p[c], q_v = v[c];   g_p = (e_p + h * e_v) + dp;   g_v = e_v + dv
 *               not advanced:
 *                     q = xh unchanged;         g_p = e_p + dp;               g_v = e_v + dv
 *               x_p = q_p + g_p;   x_v = q_v + g_v;   x_a = a[c] (advanced only)
 *               n_p = sqrt((g_px*g_px + g_py*g_py) + g_pz*g_pz);   n_v likewise
 *               event = (n_p > trigger_p) || (n_v > trigger_v)
 *               event:    xh = x;  e = 0;  and if reanchor, for kk = 0 .. K-1:
 *                             table_next[3kk+c] = table_next[3kk+c] + (g_p + ((double)kk * h) * g_v)        (the agent's column of the next table)
 *                             v[3kk+c]          = v[3kk+c] + g_v
 *               no event: xh = q;  e = g
 *             With e == 0 the state is q + d: trigger = (0, 0), reanchor = 0 is the disturbed loop of before, byte for byte.  trigger = +inf
 *             never feeds back (open loop).  Entry 0 of a re-anchored column is x_p.  The v rows are re-anchored too: they are what the hold
 *             rule and dmpc_flight_end read as "the previous plan's velocities", so a held or carried plan continues the re-anchored one.
 *             Nothing depends on launch geometry, batch split or visiting order.
 *   dmpc_feedback_device: one column on device arrays, enqueued on the caller's stream, for callers that loop over dmpc_step_device_cmd themselves
 *             (INSTEAD of dmpc_advance_device and dmpc_disturb_device): p_rows, v_rows, a_rows [S][N_cmd][3K] and status [S][N_cmd] of the step;
 *             x_p, x_v, x_a, xh_p, xh_v, e_p, e_v [S][N_cmd][3]; lT_next [S][3K][N] the table the step wrote; event [S][N_cmd] (out: 0 | 1).
 *             v_rows and lT_next are in/out.  It applies the context's disturbance of column k, if one is set, and the policy; with no policy
 *             set it launches nothing.  Scenes with scene_done[s] != 0 (scene_done [S] or NULL) are left alone.
 *   dmpc_feedback_apply_host: the same column on host arrays with an explicit policy `fb`, an optional disturbance `d` (NULL: none) and the step
 *             h -- no context, no GPU.
 *   dmpc_feedback_log: a report on the context's last flight, resident until the next one (a split batch: gathered part by part); any output
 *             NULL.  event_count, event_first, event_last [S][N_cmd]: first and last are local columns, -1 when there was none.  dev_p_max,
 *             dev_v_max [S][N_cmd]: the largest n_p / n_v seen, events included (column 0 counts with 0); dev_p_col, dev_v_col their columns,
 *             ties to the smallest.  xh_p, xh_v, e_p, e_v [S][N_cmd][3]: the planning state and the error at the scene's last column.
 * Batch split as dmpc_transition (results do not depend on it).  A DMPC_DEVICE_ALL context with a policy set runs the call unsharded on its
 * first GPU; dmpc_transition_sharded[_gather] refuse while one is set; there is no RCCL form.  Measurement noise apart from process noise (an
 * estimate that does not move the vehicle): dmpc_set_measurement, below.  Not modelled: e carried across dmpc_flight_end, events forced by the
 * caller.
 * Refused (-1, nothing launched, a message that starts with the entry's name) by dmpc_set_feedback and dmpc_feedback_apply_host: a NaN or
 * negative trigger_p or trigger_v, reanchor outside {0, 1}; by dmpc_feedback_device and dmpc_feedback_apply_host: S, N_cmd < 1, N_cmd > N,
 * k < 1, a NULL array other than scene_done, a disturbance that does not fit the call; dmpc_feedback_device: a DMPC_DEVICE_ALL context;
 * dmpc_feedback_log: no flight on the context yet, a flight without a policy, a sharded one, S or N_cmd other than the flight's. */
typedef struct dmpc_feedback {
    double  trigger_p, trigger_v;   /* thresholds on |g_p| (m) and |g_v| (m/s); >= 0, +inf allowed, NaN refused */
    int32_t reanchor;               /* 0 | 1: on an event, shift the agent's column of the next table and its v rows onto the true state */
} dmpc_feedback;
DMPC_API int dmpc_set_feedback(dmpc_ctx *ctx, const dmpc_feedback *fb);   /* NULL clears */
DMPC_API int dmpc_feedback_device(dmpc_ctx *ctx, int S, int N, int N_cmd, int k, const double *p_rows, double *v_rows, const double *a_rows,
                         const int32_t *status, double *x_p, double *x_v, double *x_a, double *xh_p, double *xh_v, double *e_p, double *e_v,
                         double *lT_next, int32_t *event, const int32_t *scene_done, void *stream);
DMPC_API int dmpc_feedback_apply_host(const dmpc_feedback *fb, const dmpc_disturbance *d, double h, int S, int N, int N_cmd, int k,
                             const double *p_rows, double *v_rows, const double *a_rows, const int32_t *status, double *x_p, double *x_v,
                             double *x_a, double *xh_p, double *xh_v, double *e_p, double *e_v, double *lT_next, int32_t *event,
                             const int32_t *scene_done);
DMPC_API int dmpc_feedback_log(dmpc_ctx *ctx, int S, int N_cmd, int32_t *event_count, int32_t *event_first, int32_t *event_last, double *dev_p_max,
                      int32_t *dev_p_col, double *dev_v_max, int32_t *dev_v_col, double *xh_p, double *xh_v, double *e_p, double *e_v);

/* Measured state (additive, the ABI revision stays 8): SENSOR NOISE AND A FIXED-GAIN ESTIMATE IN THE LOOP.  NO REFERENCE COUNTERPART.  In the
 * feedback rule above the planner knows the true deviation g exactly; here it sees g through a noisy measurement and keeps an estimate of it.  A
 * measurement model is a SETTING OF THE CONTEXT, persistent like the disturbance and the policy: dmpc_set_measurement(ctx, m); NULL clears.  IT
 * CHANGES WHAT THE FEEDBACK RULE DECIDES ON AND WHAT THE PLANNER IS RE-INITIALISED TO; IT NEVER MOVES THE VEHICLE.  It is honoured only under a
 * feedback policy: dmpc_transition, _cmd, _scripted, _mission, _hold, _route and _replan refuse a flight with a measurement set and no policy
 * (set one with dmpc_set_feedback; trigger (0, 0) is "feed the measurement back on every column").  A disturbance is not required: the policy is
 * live when a disturbance OR a measurement is set; with a measurement alone dp = dv = 0.  With no measurement set every entry enqueues what it
 * enqueued before and returns the same bytes.  tests/estimate.py restates the rule; the loop, dmpc_estimate_device, dmpc_estimate_apply_host and
 * that restatement agree bit for bit.
 *   per commanded agent one more pair of state, beside the true error e: the BELIEF eh = (eh_p, eh_v), the planner's estimate of e.
 *   column 0: eh = 0 -- also in a flight with a start; like e, it is not carried across dmpc_flight_end.
 *   column k >= 1: the same agents and the same place in the column as the feedback rule.  fp64, every operation rounded on its own (no fused
 *             multiply-add), per component c; uniform as in the disturbance rule, col0 the start's (none: 0), s the scene's index in the call:
 *               sid   = (uint64) 1 << 63 | (uint64) s << 32 | i          (a stream of its own: never the disturbance's, even with equal seeds)
 *               u_j   = 2.0 * uniform(seed, sid, 6 * (col0 + k) + j) - 1.0          j = 0 .. 5
 *               m_p   = amp_p * u_c;   m_v = amp_v * u_(3+c)
 *               q, g_p, g_v, x_p = q_p + g_p, x_v = q_v + g_v, x_a: exactly the feedback rule's (the vehicle: unchanged by the measurement)
 *               b_p   = advanced ? eh_p + h * eh_v : eh_p;   b_v = eh_v
 *               y_p   = amp_p > 0 ? g_p + m_p : g_p;         y_v likewise with amp_v          (amp == 0: no addition, -0.0 stays -0.0)
 *               gh_p  = gain_p == 1.0 ? y_p : b_p + gain_p * (y_p - b_p);   gh_v likewise with gain_v
 *               n_p   = sqrt((gh_px*gh_px + gh_py*gh_py) + gh_pz*gh_pz);   n_v likewise;   event = (n_p > trigger_p) || (n_v > trigger_v)
 *               event:    xh = q + gh;  e = g - gh;  eh = 0;  and if reanchor: the re-anchoring above with (gh_p, gh_v) in the place of (g_p, g_v)
 *               no event: xh = q;       e = g;       eh = gh
 *             With amp = (0, 0) and gain = (1, 1) this is the feedback rule bit for bit: gh = g, q + g is the expression of x, g - g = +0.
 *   dmpc_measurement_sample: m_p, m_v [S][N_cmd][3] of column k (col0 = 0) on the host -- no context, no GPU; k == 0 gives zeros.
 *   dmpc_estimate_device: dmpc_feedback_device with the belief eh_p, eh_v [S][N_cmd][3] (in/out) behind e_v.  It applies the context's
 *             disturbance of column k if one is set, its measurement and its policy; with no policy or no measurement set it launches nothing.
 *             dmpc_feedback_device itself never reads the measurement.
 *   dmpc_estimate_apply_host: the same column on host arrays with an explicit policy `fb`, measurement `m` and optional disturbance `d` (NULL:
 *             none) -- no context, no GPU.
 *   dmpc_estimate_log: a report on the context's last flight, on dmpc_feedback_log's model (resident until the next flight, a split batch
 *             gathered part by part, any output NULL).  err_p_max, err_v_max [S][N_cmd]: the largest estimation error |g_p - gh_p|, |g_v - gh_v|
 *             (the norm as n_p, of the differences rounded once); dev_p_max, dev_v_max: the largest TRUE |g_p|, |g_v|; *_col their local
 *             columns, ties to the smallest, column 0 counts with 0.  eh_p, eh_v [S][N_cmd][3]: the belief at the scene's last column.
 *             ON SUCH A FLIGHT dmpc_feedback_log's dev_* ARE THE NORMS THE EVENTS WERE DECIDED ON (of gh, not of g), and its xh, e are as stored
 *             by the rule above (e need not be 0 after an event).
 * Batch split, DMPC_DEVICE_ALL and the sharded entries as for the policy: a DMPC_DEVICE_ALL context flies such a flight on its first GPU,
 * dmpc_transition_sharded[_gather] refuse while a measurement is set; there is no RCCL form.  Not modelled: a Kalman filter with a covariance
 * (the gains are fixed), e or eh carried across dmpc_flight_end, events forced by the caller, noisy knowledge of uncommanded or scripted vehicles.
 * Refused (-1, nothing launched, a message that starts with the entry's name) by dmpc_set_measurement (the descriptor is checked before the
 * context), dmpc_measurement_sample and dmpc_estimate_apply_host, by the field's name: a negative or non-finite amp_p or amp_v, a gain_p or
 * gain_v outside (0, 1] or NaN; by dmpc_estimate_device and dmpc_estimate_apply_host what dmpc_feedback_device / _apply_host refuse, and a NULL
 * eh_p, eh_v or m; by dmpc_estimate_log: no flight yet, a sharded one, a flight without a policy or without a measurement, S or N_cmd other than
 * the flight's. */
typedef struct dmpc_measurement {
    uint64_t seed;
    double amp_p, amp_v;     /* half-widths of the uniform sensor noise on position (m) and velocity (m/s); >= 0, finite */
    double gain_p, gain_v;   /* fixed gains of the estimate, in (0, 1]; 1: the estimate is the measurement */
} dmpc_measurement;          /* 40 bytes, offsets 0 8 16 24 32 */
DMPC_API int dmpc_set_measurement(dmpc_ctx *ctx, const dmpc_measurement *m);   /* NULL clears */
DMPC_API int dmpc_measurement_sample(const dmpc_measurement *m, int S, int N_cmd, int k, double *mp, double *mv);
DMPC_API int dmpc_estimate_device(dmpc_ctx *ctx, int S, int N, int N_cmd, int k, const double *p_rows, double *v_rows, const double *a_rows,
                         const int32_t *status, double *x_p, double *x_v, double *x_a, double *xh_p, double *xh_v, double *e_p, double *e_v,
                         double *eh_p, double *eh_v, double *lT_next, int32_t *event, const int32_t *scene_done, void *stream);
DMPC_API int dmpc_estimate_apply_host(const dmpc_feedback *fb, const dmpc_measurement *m, const dmpc_disturbance *d, double h, int S, int N,
                             int N_cmd, int k, const double *p_rows, double *v_rows, const double *a_rows, const int32_t *status, double *x_p,
                             double *x_v, double *x_a, double *xh_p, double *xh_v, double *e_p, double *e_v, double *eh_p, double *eh_v,
                             double *lT_next, int32_t *event, const int32_t *scene_done);
DMPC_API int dmpc_estimate_log(dmpc_ctx *ctx, int S, int N_cmd, double *err_p_max, int32_t *err_p_col, double *err_v_max, int32_t *err_v_col,
                      double *dev_p_max, int32_t *dev_p_col, double *dev_v_max, int32_t *dev_v_col, double *eh_p, double *eh_v);

/* Standalone forms of the path's small helpers (fused into the step kernels inside the solvers), for callers that
 * invoke them on their own as the reference's scripts do.  Host pointers, synchronous.
 *   dmpc_prop_state   propStatedmpc.m:1-8 (A_initp given): p = A_p a + A_initp [po;vo], v = A_v a + 1 (x) vo  -> pass
 *                     off_v = vo; dec-iSCP/propState.m:1-10 (A_initp = NULL): new_p + repmat(po) -> pass off_p = po.
 *                     A_p, A_v: [n_rows][n_cols] row-major, A_initp: [n_rows][6] or NULL; off_p/off_v: 3-vectors tiled
 *                     over the rows (or NULL).
 *   dmpc_is_inbounds  is_inbounds.m:1-6 on npts points [npts][3] (5 cm tolerance)
 *   dmpc_reached_goal ReachedGoal.m:1-11: max_i |p_i - pf_i| < error_tol, p, pf [N][3]
 *   dmpc_max_deviation maxDeviation.m:1-11 (the stopping measure of solveDMPC.m:69): p, prev_p [K_cols][3] (== MATLAB 3 x K_cols); the
 *                     largest per-step distance over the steps the .m looks at -- `K = length(p)/3` of the MATRIX p is max(3, K_cols)/3,
 *                     i.e. the first 5 of 15 horizon steps, restated as written */
DMPC_API int dmpc_prop_state(dmpc_ctx *ctx, int n_rows, int n_cols, const double *A_p, const double *A_v, const double *A_initp,
                    const double *po, const double *vo, const double *off_p, const double *off_v, const double *a,
                    double *p, double *v);
DMPC_API int dmpc_is_inbounds(dmpc_ctx *ctx, int npts, const double *p, const double *pmin, const double *pmax, int32_t *inbounds);
DMPC_API int dmpc_reached_goal(dmpc_ctx *ctx, int N, const double *p, const double *pf, double error_tol, int32_t *reached);
DMPC_API int dmpc_max_deviation(dmpc_ctx *ctx, int K_cols, const double *p, const double *prev_p, double *tol_out);

/* Agent-steps LAUNCHED by this context so far (incl. the half of a split dmpc_transition batch that runs on the internal
 * second context).  An upper bound of the QPs actually solved: agents of scenes that already stopped are skipped on the
 * device, and agents the scan certifies infeasible never enter the solver; per-agent outcomes are in status[]. */
DMPC_API int64_t dmpc_solve_count(const dmpc_ctx *ctx);

/* Roofline instrumentation: with dmpc_profile(ctx,1) every step-kernel launch is bracketed by HIP
 * events on the stream it is launched on; dmpc_profile_read drains them and returns the average
 * duration (ms) of the step's kernels and the step count since the previous read. */
DMPC_API int dmpc_profile(dmpc_ctx *ctx, int enable);
DMPC_API int dmpc_profile_read(dmpc_ctx *ctx, double *avg_ms, int64_t *n_launches);
/* same, split into the solve kernel(s) (dmpc_solve_kernel, the dominant kernel) and scan + ordering */
DMPC_API int dmpc_profile_read2(dmpc_ctx *ctx, double *solve_avg_ms, double *scan_avg_ms, int64_t *n_steps);
/* the solve kernel the context's last MPC step launched for the bulk of its agents, as a profiler names it (e.g. "dmpc_rsolve_persist_kernel",
 * "dmpc_solve_persist_kernel<true, 56, 48, double>"): the launch form is picked per step from the variant and the depth of the launch, and whoever
 * reports the measured duration of "the dominant kernel" (bench.py's roofline block) names the kernel from here, not from a copy of that rule.
 * The string lives in the context; empty before the first step.  (ABI revision 7) */
DMPC_API const char *dmpc_last_solve_kernel(const dmpc_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* DMPC_HIP_H */
