// dmpc_mex.cpp -- MEX gateway binding libdmpc_hip.so (include/dmpc_hip.h) into MATLAB.
//
// Build on a MATLAB host:   mex -I../../include dmpc_mex.cpp -L.. -ldmpc_hip
// (MATLAB's mex.h is not in the build container; there the gateway is compiled and EXECUTED against the mock MEX runtime
// of tests/mock_mex/ -- tests/test_mex_gateway.py.)
//
// One gateway, dispatched on a command string, keeps ONE persistent context per parameter set:
//   [p,v,a,status,info] = dmpc_mex('solve_one', params, l, n, po, vo, ao, pf)
//   [P,V,A,status,info] = dmpc_mex('step_batch', params, l, x_p, x_v, x_a, pf)          states / pf 3 x N_cmd, N_cmd <= N: see below
//   [r_factor,h_scaled,violation,totdist,traj_time,p] = dmpc_mex('postcheck', params, pk, vk, ak, pf, vmax, amax, Ts)
//   [r_factor,h_scaled,violation,totdist,traj_time,p,violation_static,min_dist_static] = dmpc_mex('postcheck', ..., Ts, po_static)
//   [dist,partner,time] = dmpc_mex('clearance', params, pk, vk, ak, pf, vmax, amax, Ts[, po_static|[][, reach]])   2 x N each; partner 1-based, 0 = none
//   [p,v,a,peaks] = dmpc_mex('setpoints', params, pk, vk, ak, vmax, amax, Ts[, first[, count]])   100 Hz setpoints 3 x count x N from sample `first` (1-based) on;
//                                                                                    peaks 4 x N: v_peak; its sample (1-based); a_peak; its sample
//   [Lambda,Av,A0,Delta] = dmpc_mex('model_matrices', params)
//   [Ain,bin,dist] = dmpc_mex('coll_rows', params, l, sel0, k_cmp0, k_blk0, p, a0, rmin, c, A)     (0-based indices)
//   [Ain,bin]      = dmpc_mex('add_coll_constr', params, p, po, rmin, c, A)
//   Aaug           = dmpc_mex('posvel_matrix', params)                                  getPosVelMat.m (12 x 3K)
//   [p,v,a]        = dmpc_mex('init_batch', params, po, pf)                             initDMPC.m for N agents (3 x K x N each)
//   [p,v]          = dmpc_mex('prop_state', params, A_p, A_v, A_initp|[], po, vo, a)    propStatedmpc.m / dec-iSCP propState.m
//   [xi,rhs,dist,kc,viol_k,coll] = dmpc_mex('rows_one', params, l, n, po, vo)           CheckCollSoftDMPC + CollConstr*DMPC rows
//   Ain            = dmpc_mex('rows_dense', params, xi, kc, A)                          -diff_mat*A of structured rows
//   [pk,vk,ak,K_T_used,scene_status] = dmpc_mex('transition', params, po, pf, K_T_max, error_tol)   the whole k-loop on the GPU
//   [pk,vk,ak,K_T_used,scene_status] = dmpc_mex('transition_disturbed', params, po, pf, K_T_max, error_tol, noise_p, noise_v, seed, wind, pushes)   see below
//   [pk,vk,ak,K_T_used,scene_status,event_count,event_first,event_last,dev_p_max,dev_p_col,dev_v_max,dev_v_col,xh_p,xh_v,e_p,e_v] = dmpc_mex('transition_feedback',
//                    params, po, pf, K_T_max, error_tol, trigger_p, trigger_v, reanchor, noise_p, noise_v, seed, wind, pushes)   see below
//   [pk,vk,ak,K_T_used,scene_status,<'transition_feedback's log>,err_p_max,err_p_col,err_v_max,err_v_col,dev_p_max,dev_p_col,dev_v_max,dev_v_col,eh_p,eh_v] =
//                    dmpc_mex('transition_estimated', <'transition_feedback's arguments>, meas_p, meas_v, gain_p, gain_v, meas_seed)   see below
//   [pk,vk,ak,K_T_used,scene_status,stage_col] = dmpc_mex('mission', params, po, goals, K_T_max, error_tol[, deadline])   goals 3 x N_cmd x Q: see below
//   [pk,vk,ak,K_T_used,scene_status,wp_col] = dmpc_mex('route', params, po, waypoints, K_T_max, error_tol, capture[, n_wp[, timeout]])   waypoints 3 x W x N_cmd: see below
//   [perm,pf,cost,rounds] = dmpc_mex('assign', params, po, goals[, eps[, max_rounds]])  goal assignment (dmpc_assign_goals): po, goals 3 x N; perm 1 x N, 1-based:
//                                                                                    agent i takes goals(:,perm(i)) = pf(:,i); eps default 1e-4 / N
//   [perm,pf,owner,cost,rounds] = dmpc_mex('assign_rect', params, po, goals[, eps[, max_rounds]])  N agents, M goals (dmpc_assign_rect): po 3 x N, goals 3 x M;
//                                                                                    perm 1 x N, owner 1 x M, 1-based, 0: none (pf(:,i) = po(:,i) then); eps default 1e-4 / max(N,M)
//   [waypoints,n_wp,plan_status,hops] = dmpc_mex('plan', params, po, goals, cell[, margin[, W[, obstacles]]])   route planning (dmpc_plan_routes): see below
//   [pk,vk,ak,K_T_used,scene_status,waypoints,n_wp,replan_count,replan_col,wp_col,plan_status] = dmpc_mex('replan', params, po, goals, K_T_max, error_tol, cell,
//                    capture[, margin[, W[, every[, ahead[, path[, timeout]]]]]])        re-planned routes (dmpc_transition_replan): see below
//   inbounds       = dmpc_mex('is_inbounds', params, p, pmin, pmax)                    is_inbounds.m
//   pass           = dmpc_mex('reached_goal', params, p, pf, error_tol)                ReachedGoal.m
//   tol            = dmpc_mex('max_deviation', params, p, prev_p)                      maxDeviation.m (p, prev_p: 3 x K)
//   [po,pf]        = dmpc_mex('random_test', params, N, pmin, pmax, rmin, c, seed)      randomTest.m
//   [po,pf]        = dmpc_mex('random_exchange', params, N, pmin, pmax, rmin, seed)     randomExchange.m
//   [x_p,x_v,x_a,plan_p,plan_v,plan_a,col] = dmpc_mex('flight_end', params, N_cmd)
//   [pk,vk,ak,K_T_used,status] = dmpc_mex('transition_from', params, po, pf, K_T_max, error_tol, vo, ao, plan_p, plan_v, plan_a, col0[, from_end])
// Uncommanded vehicles (DMPC::solveParallelDMPCv2, dmpc/cpp/dmpc.cpp:1572-1573: N = _po.cols(), N_cmd = _pf.cols()): 'transition' and
// 'step_batch' take pf (and the states) with FEWER columns than po / l -- the first N_cmd vehicles are commanded, the others stay at po as
// static obstacles, and the outputs cover the commanded ones; 'postcheck' takes po_static (3 x M) behind Ts.
// Missions (dmpc_transition_mission, no reference counterpart): 'mission' is 'transition' through the Q goal sets goals(:,:,q) one after the
// other -- a stage ends at the first column where its goals are reached or its deadline (1 x Q, 0 = none, the last 0) has passed; stage_col
// (1 x Q) holds the 0-based history column each stage ended on, -1 for a stage that never did.  N_cmd < N: static vehicles, as 'transition'.
// Routes (dmpc_transition_route, no reference counterpart): 'route' is 'transition' with waypoints of its own for every commanded agent,
// waypoints(:,w,i) -- agent i leaves a waypoint that is not its last when it is closer to it than capture (metres) or has flown towards it for
// timeout columns (0 = none); n_wp (1 x N_cmd, default W each) counts an agent's waypoints, the last of them is its goal; wp_col (W x N_cmd) holds
// the 0-based history column on which the agent left each waypoint, -1 where it never did.  A failed agent stops the scene (max_hold = 0).
// Route planning (dmpc_plan_routes, no reference counterpart): 'plan' finds the waypoints 'route' flies -- po 3 x N, goals 3 x N_cmd, N_cmd <= N: the
// vehicles behind the commanded ones are the obstacles to go round, obstacles (3 x M) adds further points; cell (metres) is the planning grid's,
// margin (default 0) widens rmin, W (default 4) is the number of waypoint slots.  waypoints 3 x W x N_cmd and n_wp 1 x N_cmd go into 'route' as they
// are; plan_status 1 x N_cmd: 0 ok, 1 truncated (more corners than W: the goal took the last slot), 2 no way (the goal alone); hops 1 x N_cmd: cells
// of the path, -1 for no way.
// Re-planned routes (dmpc_transition_replan, no reference counterpart): 'replan' is 'plan' before column 0, 'route' from there, and every `every`
// columns (default 5, 0 = never) the agents whose remaining legs are no longer clear are planned again on the device, round the vehicles where they
// are on that column and on the `ahead` (default 0) columns behind it.  path (3 x P x M, optional): scripted vehicles, po is then 3 x N_cmd; without
// it the vehicles of po behind the goals are static obstacles.  waypoints, n_wp, plan_status: the plan in force at the end; replan_count, replan_col
// (1 x N_cmd): re-plans per agent and the 0-based column of the last one, -1 for none; wp_col refers to the last plan.
// Disturbed transitions (dmpc_set_disturbance, no reference counterpart): 'transition_disturbed' is 'transition' with a disturbance added to the state
// of every commanded agent on every column from 1 on, by the rule include/dmpc_hip.h pins: uniform noise of half-width noise_p (metres) on the
// position and noise_v (m/s) on the velocity from the stream `seed` (an integer below 2^53), a constant wind (3 x 1, m/s^2, or []) and pushes
// (8 x n or []: agent, 1-based; history column, 0-based, >= 1; dp (3); dv (3)).  The command sets the disturbance, flies and clears it.
// Event-triggered feedback (dmpc_set_feedback, no reference counterpart): 'transition_feedback' is 'transition_disturbed' under a feedback policy --
// the solver starts from its own prediction and from the true state again only on an event, a tracking error above trigger_p (metres) or trigger_v
// (m/s; Inf: never, 0: on every column); reanchor (0 | 1): an event shifts the agent's announced plan onto the true state.  Behind the flight's
// outputs come dmpc_feedback_log's, in the order of the list above: event_count, event_first, event_last, dev_p_col, dev_v_col (1 x N_cmd; 0-based history columns,
// -1: none), dev_p_max, dev_v_max (1 x N_cmd) and xh_p, xh_v, e_p, e_v (3 x N_cmd).  The command sets the policy and the disturbance, flies, reads the log and clears both.
// Measured state (dmpc_set_measurement, no reference counterpart): 'transition_estimated' is 'transition_feedback' in which the rule decides on an
// estimate of the tracking error -- the true deviation plus uniform sensor noise of half-widths meas_p (metres), meas_v (m/s) from the stream
// meas_seed, blended into the planner's belief with the fixed gains gain_p, gain_v in (0, 1] -- and re-initialises the planner to it; the vehicle is
// never moved by it.  Behind 'transition_feedback's outputs (whose dev_* are then the norms the events were decided on) come dmpc_estimate_log's:
// err_p_max, err_p_col, err_v_max, err_v_col (1 x N_cmd: the largest estimation error and its 0-based column), dev_p_max, dev_p_col, dev_v_max,
// dev_v_col (the largest TRUE tracking error) and eh_p, eh_v (3 x N_cmd: the belief at the last column).  The command sets all three, flies, reads
// both logs and clears all three.
// Start in motion (dmpc_set_start, no reference counterpart): 'flight_end' returns where the last 'transition*' of the context ended -- x_p, x_v,
// x_a (3 x N_cmd), every agent's plan of the step that produced the last column, plan_p, plan_v, plan_a (3 x K x N_cmd), and col, that column in the
// caller's count; 'transition_from' is 'transition' whose column 0 is the state (po, vo, ao) and the plan given instead of initDMPC: vo, ao
// (3 x N_cmd or [] = zeros), plan_p ([]: the braking plan), plan_v, plan_a (both or []), col0 (the caller's number of column 0: scripted windows,
// the disturbance's counter); from_end = 1 (all five arrays []): the end of the context's last flight, carried on the device, col0 added to its col.
// The command sets the start, flies dmpc_transition_cmd and clears the start on any error.
// `params` is a struct with the fields of dmpc_params (variant as the DMPC_VAR_* integer).
// The signature-preserving wrappers (solveSoftDMPCbound.m, ...) in this directory call 'solve_one'
// and convert status bits into the reference's [] + flag conventions.
#include "mex.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dmpc_hip.h"

// A few persistent contexts keyed by their parameters (most recently used first): scripts of the reference alternate helpers that
// carry their own constants (initDMPC, CheckCollSoftDMPC, propStatedmpc ...) with the solver inside one loop -- one context re-tuned on
// every call would rebuild and upload its tables twice per agent and MPC step.
struct CtxSlot { dmpc_params prm; dmpc_ctx *ctx; };
static CtxSlot g_slots[4] = {};
static int g_nslots = 0;
static bool g_registered = false;

static void cleanup()
{
    for (int i = 0; i < g_nslots; ++i) if (g_slots[i].ctx) dmpc_destroy(g_slots[i].ctx);
    g_nslots = 0;
}

static double field(const mxArray *s, const char *name)
{
    const mxArray *f = mxGetField(s, 0, name);
    if (!f) mexErrMsgIdAndTxt("dmpc:params", "missing field %s", name);
    return mxGetScalar(f);
}

static dmpc_params read_params(const mxArray *s)
{
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("dmpc:params", "params must be a struct");
    dmpc_params p{};   // value-initialised: the struct is compared bytewise (context cache)
    p.K = (int32_t)field(s, "K"); p.variant = (int32_t)field(s, "variant");
    p.order = (int32_t)field(s, "order"); p.max_tries = 0;
    p.h = field(s, "h"); p.rmin = field(s, "rmin"); p.c = field(s, "c"); p.alim = field(s, "alim");
    p.Q1 = field(s, "Q1"); p.S1 = field(s, "S1"); p.term = field(s, "term");
    const double *pmin = mxGetPr(mxGetField(s, 0, "pmin")), *pmax = mxGetPr(mxGetField(s, 0, "pmax"));
    for (int d = 0; d < 3; ++d) { p.pmin[d] = pmin[d]; p.pmax[d] = pmax[d]; }
    // optional: weights of the collision-free cost cases (0 = the reference's HEAD constants)
    const mxArray *qf = mxGetField(s, 0, "Qfar"), *qn = mxGetField(s, 0, "Qnear"), *sf = mxGetField(s, 0, "Sfree");
    p.Qfar = qf ? mxGetScalar(qf) : 0.0; p.Qnear = qn ? mxGetScalar(qn) : 0.0; p.Sfree = sf ? mxGetScalar(sf) : 0.0;
    // optional: `tol` of solveDMPC.m:1 (DMPC_VAR_SCP)
    const mxArray *tl = mxGetField(s, 0, "tol");
    p.tol = tl ? mxGetScalar(tl) : 0.0;
    return p;
}

static dmpc_ctx *context(const dmpc_params &p)
{
    for (int i = 0; i < g_nslots; ++i)
        if (std::memcmp(&p, &g_slots[i].prm, sizeof(p)) == 0) {
            const CtxSlot hit = g_slots[i];
            for (int j = i; j > 0; --j) g_slots[j] = g_slots[j - 1];
            g_slots[0] = hit;
            return hit.ctx;
        }
    // every visible GPU (DMPC_DEVICE_ALL): on a multi-GPU node the agents of a scene are sharded over the GPUs inside the library,
    // like the thread clusters of DMPC::solveParallelDMPCv2; with one GPU this is a plain context
    dmpc_ctx *c = nullptr;
    if (g_nslots == 4) {   // re-tune the least recently used context
        c = g_slots[3].ctx;
        if (dmpc_set_params(c, &p)) mexErrMsgIdAndTxt("dmpc:params", "%s", dmpc_last_error(c));
        g_nslots = 3;
    } else {
        // (the library found at run time must speak the header this gateway was compiled with: the special device values changed once)
        if (dmpc_abi_version() != DMPC_ABI_VERSION) mexErrMsgIdAndTxt("dmpc:abi", "libdmpc_hip.so has ABI revision %d, this gateway was compiled for %d", dmpc_abi_version(), DMPC_ABI_VERSION);
        c = dmpc_create(&p, DMPC_DEVICE_ALL, DMPC_PREC_F64);
        if (!c) mexErrMsgIdAndTxt("dmpc:create", "%s", dmpc_last_error(nullptr));
    }
    for (int j = g_nslots; j > 0; --j) g_slots[j] = g_slots[j - 1];
    g_slots[0].prm = p; g_slots[0].ctx = c;
    g_nslots++;
    if (!g_registered) { mexAtExit(cleanup); mexLock(); g_registered = true; }
    return c;
}

static void need(bool ok, const char *what) { if (!ok) mexErrMsgIdAndTxt("dmpc:shape", "%s", what); }

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    need(nrhs >= 2 && mxIsChar(prhs[0]), "usage: dmpc_mex(cmd, params, ...)");
    char cmd[32];
    mxGetString(prhs[0], cmd, sizeof(cmd));
    dmpc_params p = read_params(prhs[1]);
    const int n3 = 3 * p.K;
    if (!std::strcmp(cmd, "model_matrices")) {
        plhs[0] = mxCreateDoubleMatrix(n3, n3, mxREAL);
        mxArray *Av = mxCreateDoubleMatrix(n3, n3, mxREAL), *A0 = mxCreateDoubleMatrix(6, n3, mxREAL),
                *Dl = mxCreateDoubleMatrix(n3, n3, mxREAL);
        // the C ABI is row-major: the returned column-major MATLAB arrays hold the TRANSPOSES, which the
        // .m wrappers undo (Lambda, A_v, Delta) / A0 is created 6 x 3K and transposed there
        dmpc_model_matrices(&p, mxGetPr(plhs[0]), mxGetPr(Av), mxGetPr(A0), mxGetPr(Dl));
        if (nlhs > 1) plhs[1] = Av; if (nlhs > 2) plhs[2] = A0; if (nlhs > 3) plhs[3] = Dl;
        return;
    }
    if (!std::strcmp(cmd, "posvel_matrix")) {   // getPosVelMat.m:24 (host computation)
        mxArray *t = mxCreateDoubleMatrix(n3, 12, mxREAL);   // row-major 12 x 3K == column-major 3K x 12
        dmpc_posvel_matrix(p.h, p.K, mxGetPr(t));
        plhs[0] = mxCreateDoubleMatrix(12, n3, mxREAL);
        for (int i = 0; i < 12; ++i) for (int j = 0; j < n3; ++j) mxGetPr(plhs[0])[i + 12 * j] = mxGetPr(t)[(size_t)i * n3 + j];
        return;
    }
    dmpc_ctx *ctx = context(p);
    if (!std::strcmp(cmd, "solve_one")) {
        need(nrhs == 8, "solve_one: (cmd, params, l, n, po, vo, ao, pf)");
        const mwSize *dl = mxGetDimensions(prhs[2]);
        need(mxGetNumberOfDimensions(prhs[2]) == 3 && dl[0] == 3 && (int)dl[1] == p.K, "l must be 3 x K x N");
        const int N = (int)dl[2], n = (int)mxGetScalar(prhs[3]);
        for (int i = 4; i < 8; ++i) need(mxGetNumberOfElements(prhs[i]) == 3, "po, vo, ao, pf must have 3 elements");
        plhs[0] = mxCreateDoubleMatrix(3, p.K, mxREAL);   // column-major 3 x K == stacked [x1 y1 z1 x2 ...]
        mxArray *v = mxCreateDoubleMatrix(3, p.K, mxREAL), *a = mxCreateDoubleMatrix(3, p.K, mxREAL);
        mxArray *st = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL), *inf = mxCreateNumericMatrix(1, 8, mxINT32_CLASS, mxREAL);
        // MATLAB l(3,K,N) column-major IS the [N][3K] row-major table: passed without copying
        if (dmpc_solve_one(ctx, N, n - 1, mxGetPr(prhs[2]), mxGetPr(prhs[4]), mxGetPr(prhs[5]), mxGetPr(prhs[6]), mxGetPr(prhs[7]),
                           mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a), (int32_t *)mxGetData(st), (int32_t *)mxGetData(inf)))
            mexErrMsgIdAndTxt("dmpc:solve", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a; if (nlhs > 3) plhs[3] = st; if (nlhs > 4) plhs[4] = inf;
        return;
    }
    if (!std::strcmp(cmd, "step_batch")) {
        need(nrhs == 7, "step_batch: (cmd, params, l, x_p, x_v, x_a, pf)");
        const mwSize *dl = mxGetDimensions(prhs[2]);
        need(mxGetNumberOfDimensions(prhs[2]) == 3 && dl[0] == 3 && (int)dl[1] == p.K, "l must be 3 x K x N");
        const int N = (int)dl[2], Nc = (int)(mxGetNumberOfElements(prhs[6]) / 3);   // N_cmd = columns of pf
        need(Nc >= 1 && Nc <= N, "pf must be 3 x N_cmd with 1 <= N_cmd <= N");
        for (int i = 3; i < 7; ++i) need(mxGetNumberOfElements(prhs[i]) == (size_t)3 * Nc, "states and pf must be 3 x N_cmd");
        const mwSize d3[3] = {3, (mwSize)p.K, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *st = mxCreateNumericMatrix(1, Nc, mxINT32_CLASS, mxREAL), *inf = mxCreateNumericMatrix(8, Nc, mxINT32_CLASS, mxREAL);
        const int rc = Nc == N ? dmpc_step_batch(ctx, 1, N, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), mxGetPr(prhs[5]), mxGetPr(prhs[6]),
                                                 mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a), (int32_t *)mxGetData(st), (int32_t *)mxGetData(inf))
                                 : dmpc_step_batch_cmd(ctx, 1, N, Nc, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), mxGetPr(prhs[5]), mxGetPr(prhs[6]),
                                                       mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a), (int32_t *)mxGetData(st), (int32_t *)mxGetData(inf));
        if (rc)
            mexErrMsgIdAndTxt("dmpc:step", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a; if (nlhs > 3) plhs[3] = st; if (nlhs > 4) plhs[4] = inf;
        return;
    }
    if (!std::strcmp(cmd, "postcheck")) {   // failure_rate.m:136-195 for one trial
        need(nrhs == 9 || nrhs == 10, "postcheck: (cmd, params, pk, vk, ak, pf, vmax, amax, Ts[, po_static])");
        const mwSize *dh = mxGetDimensions(prhs[2]);
        need(mxGetNumberOfDimensions(prhs[2]) == 3 && dh[0] == 3, "pk must be 3 x KT x N");
        const int KT = (int)dh[1], N = (int)dh[2];
        for (int i = 3; i < 5; ++i) need(mxGetNumberOfElements(prhs[i]) == (size_t)3 * KT * N, "vk, ak must match pk");
        need(mxGetNumberOfElements(prhs[5]) == (size_t)3 * N, "pf must be 1 x 3 x N");
        const double vmax = mxGetScalar(prhs[6]), amax = mxGetScalar(prhs[7]), Ts = mxGetScalar(prhs[8]);
        double rf = 0, hs = 0, tot = 0, tt = 0, mds = 0;
        int32_t ns = 0, viol = 0, kt = KT, viol_st = 0;
        // uncommanded vehicles: po_static is 3 x M; the histories and pf are the N commanded agents'
        const int M = nrhs == 10 ? (int)(mxGetNumberOfElements(prhs[9]) / 3) : 0;
        if (nrhs == 10) need(mxGetNumberOfElements(prhs[9]) == (size_t)3 * M, "po_static must be 3 x M");
        // MATLAB pk(3,KT,N) column-major IS the [N][KT][3] history layout
        if (M > 0 ? dmpc_postcheck_cmd(ctx, 1, N + M, N, KT, &kt, nullptr, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), mxGetPr(prhs[5]),
                                       mxGetPr(prhs[9]), vmax, amax, Ts, &rf, &hs, &ns, nullptr, &viol, &tot, &tt, nullptr, 0, &mds, &viol_st)
                  : dmpc_postcheck(ctx, 1, N, KT, &kt, nullptr, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), mxGetPr(prhs[5]), vmax,
                                   amax, Ts, &rf, &hs, &ns, nullptr, &viol, &tot, &tt, nullptr, 0))
            mexErrMsgIdAndTxt("dmpc:postcheck", "%s", dmpc_last_error(ctx));
        if (nlhs > 6) plhs[6] = mxCreateDoubleScalar((double)viol_st);
        if (nlhs > 7) plhs[7] = mxCreateDoubleScalar(M > 0 ? mds : (double)INFINITY);
        plhs[0] = mxCreateDoubleScalar(rf);
        if (nlhs > 1) plhs[1] = mxCreateDoubleScalar(hs);
        if (nlhs > 2) plhs[2] = mxCreateDoubleScalar((double)viol);
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar(tot);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar(tt);
        if (nlhs > 5) {   // the interpolated positions p(3, length(t), N), second pass now that length(t) is known
            const mwSize d3[3] = {3, (mwSize)ns, (mwSize)N};
            plhs[5] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
            if (dmpc_postcheck(ctx, 1, N, KT, &kt, nullptr, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), mxGetPr(prhs[5]),
                               vmax, amax, Ts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, mxGetPr(plhs[5]), ns))
                mexErrMsgIdAndTxt("dmpc:postcheck", "%s", dmpc_last_error(ctx));
        }
        return;
    }
    if (!std::strcmp(cmd, "clearance")) {   // dmpc_postcheck_clearance for one trial: nearest commanded partner (row 1) / uncommanded vehicle (row 2) per agent
        need(nrhs >= 9 && nrhs <= 11, "clearance: (cmd, params, pk, vk, ak, pf, vmax, amax, Ts[, po_static[, reach]])");
        const mwSize *dh = mxGetDimensions(prhs[2]);
        need(mxGetNumberOfDimensions(prhs[2]) == 3 && dh[0] == 3, "pk must be 3 x KT x N");
        const int KT = (int)dh[1], N = (int)dh[2];
        for (int i = 3; i < 5; ++i) need(mxGetNumberOfElements(prhs[i]) == (size_t)3 * KT * N, "vk, ak must match pk");
        need(mxGetNumberOfElements(prhs[5]) == (size_t)3 * N, "pf must be 1 x 3 x N");
        const double vmax = mxGetScalar(prhs[6]), amax = mxGetScalar(prhs[7]), Ts = mxGetScalar(prhs[8]);
        const int M = nrhs >= 10 ? (int)(mxGetNumberOfElements(prhs[9]) / 3) : 0;
        if (nrhs >= 10) need(mxGetNumberOfElements(prhs[9]) == (size_t)3 * M, "po_static must be 3 x M (or [])");
        const double reach = nrhs == 11 ? mxGetScalar(prhs[10]) : (double)INFINITY;
        int32_t kt = KT;
        std::vector<int32_t> partner((size_t)2 * N), sample((size_t)2 * N);
        plhs[0] = mxCreateDoubleMatrix(2, N, mxREAL);   // MATLAB (2, N) column-major IS the [N][2] slot layout
        if (dmpc_postcheck_clearance(ctx, 1, N + M, N, KT, &kt, nullptr, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), M > 0 ? mxGetPr(prhs[9]) : nullptr,
                                     nullptr, 0, vmax, amax, Ts, reach, mxGetPr(plhs[0]), partner.data(), sample.data()))
            mexErrMsgIdAndTxt("dmpc:clearance", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) {   // 1-based vehicle of the table (commanded agents first); 0: nothing inside reach
            plhs[1] = mxCreateDoubleMatrix(2, N, mxREAL);
            for (size_t e = 0; e < (size_t)2 * N; ++e) mxGetPr(plhs[1])[e] = (double)(partner[e] + 1);
        }
        if (nlhs > 2) {   // seconds from the start of the rescaled transition; NaN: nothing inside reach
            plhs[2] = mxCreateDoubleMatrix(2, N, mxREAL);
            for (size_t e = 0; e < (size_t)2 * N; ++e) mxGetPr(plhs[2])[e] = sample[e] >= 0 ? sample[e] * Ts : (double)NAN;
        }
        return;
    }
    if (!std::strcmp(cmd, "setpoints")) {   // dmpc_postcheck_setpoints for one trial: spline(tk,pk,t), spline(tk,vk,t), spline(tk,ak,t) (dmpc_soft_bound.m:165-169) and the peaks of |v|, |a|
        need(nrhs >= 8 && nrhs <= 10, "setpoints: (cmd, params, pk, vk, ak, vmax, amax, Ts[, first[, count]])");
        const mwSize *dh = mxGetDimensions(prhs[2]);
        need(mxGetNumberOfDimensions(prhs[2]) == 3 && dh[0] == 3, "pk must be 3 x KT x N");
        const int KT = (int)dh[1], N = (int)dh[2];
        for (int i = 3; i < 5; ++i) need(mxGetNumberOfElements(prhs[i]) == (size_t)3 * KT * N, "vk, ak must match pk");
        const double vmax = mxGetScalar(prhs[5]), amax = mxGetScalar(prhs[6]), Ts = mxGetScalar(prhs[7]);
        const double first = nrhs >= 9 ? mxGetScalar(prhs[8]) : 1.0;
        need(first >= 1 && first == std::floor(first) && first < 2147483647.0, "first must be a sample number >= 1");
        const int smp0 = (int)first - 1;
        int32_t kt = KT, ns = 0;
        int count = 0;
        if (nrhs == 10) {
            const double c = mxGetScalar(prhs[9]);
            need(c >= 1 && c == std::floor(c) && c < 2147483647.0, "count must be an integer >= 1");
            count = (int)c;
        } else {   // from `first` to the end of the trajectory: the report alone says how long it is
            if (dmpc_postcheck_setpoints(ctx, 1, N, KT, &kt, nullptr, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), vmax, amax, Ts, 0, 0, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ns))
                mexErrMsgIdAndTxt("dmpc:setpoints", "%s", dmpc_last_error(ctx));
            count = ns - smp0 > 1 ? ns - smp0 : 1;
        }
        const mwSize d3[3] = {3, (mwSize)count, (mwSize)N};   // MATLAB (3, count, N) column-major IS the [N][count][3] layout
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        std::vector<double> vp((size_t)N), ap((size_t)N);
        std::vector<int32_t> vs((size_t)N), as((size_t)N);
        if (dmpc_postcheck_setpoints(ctx, 1, N, KT, &kt, nullptr, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), vmax, amax, Ts, smp0, count,
                                     mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a), vp.data(), vs.data(), ap.data(), as.data(), nullptr, nullptr, nullptr))
            mexErrMsgIdAndTxt("dmpc:setpoints", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) {   // rows: v_peak, its 1-based sample, a_peak, its 1-based sample
            plhs[3] = mxCreateDoubleMatrix(4, N, mxREAL);
            for (int i = 0; i < N; ++i) {
                double *col = mxGetPr(plhs[3]) + (size_t)4 * i;
                col[0] = vp[(size_t)i]; col[1] = (double)(vs[(size_t)i] + 1); col[2] = ap[(size_t)i]; col[3] = (double)(as[(size_t)i] + 1);
            }
        }
        return;
    }
    if (!std::strcmp(cmd, "coll_rows")) {   // dec-iSCP/CollConstr.m, dmpc/matlab/CollConstr*DMPC.m
        need(nrhs == 11, "coll_rows: (cmd, params, l, sel0, k_cmp0, k_blk0, p, a0, rmin, c, A)");
        const mwSize *dl = mxGetDimensions(prhs[2]);
        need(mxGetNumberOfDimensions(prhs[2]) >= 2 && dl[0] == 3, "l must be 3 x K x N_obs");
        const int K = (int)dl[1], N_obs = mxGetNumberOfDimensions(prhs[2]) == 3 ? (int)dl[2] : 1;
        const int n_sel = (int)mxGetNumberOfElements(prhs[3]);
        std::string selbuf((size_t)n_sel * sizeof(int32_t) + 1, '\0');
        int32_t *sel = (int32_t *)&selbuf[0];
        for (int i = 0; i < n_sel; ++i) sel[i] = (int32_t)mxGetPr(prhs[3])[i];
        need(mxGetNumberOfElements(prhs[6]) == 3 && mxGetNumberOfElements(prhs[7]) == 3, "p, a0 must have 3 elements");
        const int a_rows = (int)mxGetM(prhs[10]), ncols = (int)mxGetN(prhs[10]);
        plhs[0] = mxCreateDoubleMatrix(n_sel, ncols, mxREAL);
        mxArray *b = mxCreateDoubleMatrix(n_sel, 1, mxREAL), *d = mxCreateDoubleMatrix(n_sel, 1, mxREAL);
        // column-major operands bind through the strides: A(i,j) at i + j*a_rows, Ain(r,c) at r + c*n_sel
        if (dmpc_coll_rows(ctx, K, N_obs, n_sel, sel, mxGetPr(prhs[2]), (int)mxGetScalar(prhs[4]), (int)mxGetScalar(prhs[5]),
                           mxGetPr(prhs[6]), mxGetPr(prhs[7]), mxGetScalar(prhs[8]), mxGetScalar(prhs[9]), mxGetPr(prhs[10]), a_rows,
                           ncols, 1, a_rows, mxGetPr(plhs[0]), 1, n_sel > 0 ? n_sel : 1, mxGetPr(b), mxGetPr(d)))
            mexErrMsgIdAndTxt("dmpc:coll_rows", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = b; if (nlhs > 2) plhs[2] = d;
        return;
    }
    if (!std::strcmp(cmd, "add_coll_constr")) {   // cup-SCP/AddCollConstr.m
        need(nrhs == 7, "add_coll_constr: (cmd, params, p, po, rmin, c, A)");
        const mwSize *dp_ = mxGetDimensions(prhs[2]);
        need(mxGetNumberOfDimensions(prhs[2]) == 3 && dp_[0] == 3, "p must be 3 x K x N");
        const int K = (int)dp_[1], N = (int)dp_[2];
        need(mxGetNumberOfElements(prhs[3]) == (size_t)3 * N, "po must be 1 x 3 x N");
        need((int)mxGetM(prhs[6]) == 3 * K * N, "A must have 3*K*N rows");
        const int ncols = (int)mxGetN(prhs[6]);
        const mwSize nrows = (mwSize)K * N * (N - 1) / 2;
        plhs[0] = mxCreateDoubleMatrix(nrows, ncols, mxREAL);
        mxArray *b = mxCreateDoubleMatrix(nrows, 1, mxREAL);
        if (dmpc_add_coll_constr(ctx, K, N, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetScalar(prhs[4]), mxGetScalar(prhs[5]),
                                 mxGetPr(prhs[6]), ncols, 1, 3 * K * N, mxGetPr(plhs[0]), 1, (int64_t)nrows, mxGetPr(b)))
            mexErrMsgIdAndTxt("dmpc:add_coll_constr", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = b;
        return;
    }
    if (!std::strcmp(cmd, "init_batch")) {   // initDMPC.m:1-13 for every agent of one scene
        need(nrhs == 4, "init_batch: (cmd, params, po, pf)");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3);
        need(N >= 1 && mxGetNumberOfElements(prhs[2]) == (size_t)3 * N && mxGetNumberOfElements(prhs[3]) == (size_t)3 * N, "po, pf must be 3 x N");
        const mwSize d3[3] = {3, (mwSize)p.K, (mwSize)N};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        if (dmpc_init_batch(ctx, 1, N, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a)))
            mexErrMsgIdAndTxt("dmpc:init", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        return;
    }
    if (!std::strcmp(cmd, "prop_state")) {   // propStatedmpc.m:1-8 (A_initp given) / dec-iSCP/propState.m:1-10 (A_initp = [])
        need(nrhs == 8, "prop_state: (cmd, params, A_p, A_v, A_initp, po, vo, a)");
        const int rows = (int)mxGetM(prhs[2]), cols = (int)mxGetN(prhs[2]);
        need((int)mxGetM(prhs[3]) == rows && (int)mxGetN(prhs[3]) == cols, "A_p, A_v must have the same shape");
        need((int)mxGetNumberOfElements(prhs[7]) == cols, "a must have one element per column of A_p");
        const bool with_init = mxGetNumberOfElements(prhs[4]) > 0;
        if (with_init) need((int)mxGetM(prhs[4]) == rows && (int)mxGetN(prhs[4]) == 6, "A_initp must be rows x 6");
        // the C ABI takes row-major matrices: transpose the column-major MATLAB operands
        std::string buf((size_t)(2 * rows * cols + rows * 6) * sizeof(double), '\0');
        double *Ap = (double *)&buf[0], *Av = Ap + (size_t)rows * cols, *A0 = Av + (size_t)rows * cols;
        const double *mp = mxGetPr(prhs[2]), *mv = mxGetPr(prhs[3]);
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j) { Ap[(size_t)i * cols + j] = mp[i + (size_t)j * rows]; Av[(size_t)i * cols + j] = mv[i + (size_t)j * rows]; }
        if (with_init) { const double *m0 = mxGetPr(prhs[4]); for (int i = 0; i < rows; ++i) for (int j = 0; j < 6; ++j) A0[i * 6 + j] = m0[i + (size_t)j * rows]; }
        plhs[0] = mxCreateDoubleMatrix(rows, 1, mxREAL);
        mxArray *v = mxCreateDoubleMatrix(rows, 1, mxREAL);
        const double *po = mxGetPr(prhs[5]), *vo = mxGetPr(prhs[6]);
        // propStatedmpc: v = A_v a + repmat(vo); propState: p = A_p a + repmat(po), v = A_v a
        if (dmpc_prop_state(ctx, rows, cols, Ap, Av, with_init ? A0 : nullptr, with_init ? po : nullptr, with_init ? vo : nullptr,
                            with_init ? nullptr : po, with_init ? vo : nullptr, mxGetPr(prhs[7]), mxGetPr(plhs[0]), mxGetPr(v)))
            mexErrMsgIdAndTxt("dmpc:prop_state", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v;
        return;
    }
    if (!std::strcmp(cmd, "is_inbounds")) {   // is_inbounds.m:1-6: p is 3 x n (column-major = [n][3] points)
        need(nrhs == 5 && mxGetM(prhs[2]) == 3 && mxGetNumberOfElements(prhs[3]) == 3 && mxGetNumberOfElements(prhs[4]) == 3, "is_inbounds: (cmd, params, p(3 x n), pmin, pmax)");
        int32_t ok = 0;
        if (dmpc_is_inbounds(ctx, (int)mxGetN(prhs[2]), mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), &ok))
            mexErrMsgIdAndTxt("dmpc:is_inbounds", "%s", dmpc_last_error(ctx));
        plhs[0] = mxCreateDoubleScalar(ok ? 1.0 : 0.0);   // (a double 0/1: `if (...)` and `&&` in the scripts take it like the logical of the .m file)
        return;
    }
    if (!std::strcmp(cmd, "reached_goal")) {   // ReachedGoal.m:1-11 on the positions of ONE time index: p, pf are 3 x N
        need(nrhs == 5 && mxGetM(prhs[2]) == 3 && mxGetNumberOfElements(prhs[3]) == mxGetNumberOfElements(prhs[2]), "reached_goal: (cmd, params, p(3 x N), pf(3 x N), error_tol)");
        int32_t ok = 0;
        if (dmpc_reached_goal(ctx, (int)mxGetN(prhs[2]), mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetScalar(prhs[4]), &ok))
            mexErrMsgIdAndTxt("dmpc:reached_goal", "%s", dmpc_last_error(ctx));
        plhs[0] = mxCreateDoubleScalar(ok ? 1.0 : 0.0);   // (a double 0/1: `if (...)` and `&&` in the scripts take it like the logical of the .m file)
        return;
    }
    if (!std::strcmp(cmd, "max_deviation")) {   // maxDeviation.m:1-11: p, prev_p are 3 x K (column-major = [K][3])
        need(nrhs == 4 && mxGetM(prhs[2]) == 3 && mxGetNumberOfElements(prhs[3]) == mxGetNumberOfElements(prhs[2]), "max_deviation: (cmd, params, p(3 x K), prev_p(3 x K))");
        double tol = 0.0;
        if (dmpc_max_deviation(ctx, (int)mxGetN(prhs[2]), mxGetPr(prhs[2]), mxGetPr(prhs[3]), &tol))
            mexErrMsgIdAndTxt("dmpc:max_deviation", "%s", dmpc_last_error(ctx));
        plhs[0] = mxCreateDoubleScalar(tol);
        return;
    }
    if (!std::strcmp(cmd, "rows_one")) {   // CheckCollSoftDMPC.m + CollConstr*DMPC.m of the context's variant, structured rows
        need(nrhs == 6, "rows_one: (cmd, params, l, n, po, vo)");
        const mwSize *dl = mxGetDimensions(prhs[2]);
        need(mxGetNumberOfDimensions(prhs[2]) == 3 && dl[0] == 3 && (int)dl[1] == p.K, "l must be 3 x K x N");
        const int N = (int)dl[2], n = (int)mxGetScalar(prhs[3]);
        const int cap = (p.variant == DMPC_VAR_HARD ? p.K : (p.variant == DMPC_VAR_ALL3 ? 3 : 1)) * (N > 1 ? N - 1 : 1);
        std::string buf((size_t)cap * (5 * sizeof(double) + sizeof(int32_t)) + 8, '\0');
        double *xi = (double *)&buf[0], *rhs = xi + (size_t)3 * cap, *sc = rhs + cap;
        int32_t *kc = (int32_t *)(sc + cap), nr = 0, vk = 0, st = 0;
        if (dmpc_rows_one(ctx, N, n - 1, mxGetPr(prhs[2]), mxGetPr(prhs[4]), mxGetPr(prhs[5]), cap, xi, rhs, sc, kc, &nr, &vk, &st))
            mexErrMsgIdAndTxt("dmpc:rows", "%s", dmpc_last_error(ctx));
        const int m = nr < cap ? nr : cap;
        plhs[0] = mxCreateDoubleMatrix(3, m, mxREAL);
        std::memcpy(mxGetPr(plhs[0]), xi, (size_t)3 * m * sizeof(double));
        mxArray *b = mxCreateDoubleMatrix(m, 1, mxREAL), *d = mxCreateDoubleMatrix(m, 1, mxREAL), *k = mxCreateDoubleMatrix(m, 1, mxREAL);
        for (int i = 0; i < m; ++i) { mxGetPr(b)[i] = rhs[i]; mxGetPr(d)[i] = sc[i]; mxGetPr(k)[i] = (double)kc[i]; }
        if (nlhs > 1) plhs[1] = b; if (nlhs > 2) plhs[2] = d; if (nlhs > 3) plhs[3] = k;
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)vk);
        if (nlhs > 5) plhs[5] = mxCreateDoubleScalar((double)((st & DMPC_ST_COLL) != 0));
        return;
    }
    if (!std::strcmp(cmd, "rows_dense")) {   // Ain_total(idx,:) = -diff_mat*Ain (CollConstrSoftDMPC.m:24-27)
        need(nrhs == 5, "rows_dense: (cmd, params, xi, kc, A)");
        const int nr = (int)mxGetNumberOfElements(prhs[3]);
        need((int)mxGetNumberOfElements(prhs[2]) == 3 * nr, "xi must be 3 x nr");
        const int a_rows = (int)mxGetM(prhs[4]), ncols = (int)mxGetN(prhs[4]);
        std::string kb((size_t)nr * sizeof(int32_t) + 4, '\0');
        int32_t *kc = (int32_t *)&kb[0];
        for (int i = 0; i < nr; ++i) kc[i] = (int32_t)mxGetPr(prhs[3])[i];
        plhs[0] = mxCreateDoubleMatrix(nr, ncols, mxREAL);
        if (nr > 0 && dmpc_rows_dense(ctx, nr, mxGetPr(prhs[2]), kc, mxGetPr(prhs[4]), a_rows, ncols, 1, a_rows, mxGetPr(plhs[0]), 1, nr))
            mexErrMsgIdAndTxt("dmpc:rows_dense", "%s", dmpc_last_error(ctx));
        return;
    }
    if (!std::strcmp(cmd, "transition")) {   // the whole `for k = 1:K_T` loop (dmpc_soft_bound.m:115-148) of one trial
        need(nrhs == 6, "transition: (cmd, params, po, pf, K_T_max, error_tol)");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), Nc = (int)(mxGetNumberOfElements(prhs[3]) / 3), KT = (int)mxGetScalar(prhs[4]);
        need(N >= 1 && Nc >= 1 && Nc <= N && mxGetNumberOfElements(prhs[3]) == (size_t)3 * Nc && KT >= 2, "po must be 3 x N, pf 3 x N_cmd (N_cmd <= N), K_T_max >= 2");
        const mwSize d3[3] = {3, (mwSize)KT, (mwSize)Nc};   // the histories of the commanded agents (_pf.cols(), dmpc.cpp:1573)
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        int32_t used = 0, sst = 0;
        if (Nc == N ? dmpc_transition(ctx, 1, N, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v),
                                      mxGetPr(a), &used, &sst)
                    : dmpc_transition_cmd(ctx, 1, N, Nc, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v),
                                          mxGetPr(a), &used, &sst))
            mexErrMsgIdAndTxt("dmpc:transition", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)used);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)sst);
        return;
    }
    if (!std::strcmp(cmd, "transition_disturbed")) {   // 'transition' with wind, noise and pushes on the state (dmpc_set_disturbance): set, fly, clear
        need(nrhs == 11, "transition_disturbed: (cmd, params, po, pf, K_T_max, error_tol, noise_p, noise_v, seed, wind, pushes)");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), Nc = (int)(mxGetNumberOfElements(prhs[3]) / 3), KT = (int)mxGetScalar(prhs[4]);
        need(N >= 1 && Nc >= 1 && Nc <= N && mxGetNumberOfElements(prhs[3]) == (size_t)3 * Nc && KT >= 2, "po must be 3 x N, pf 3 x N_cmd (N_cmd <= N), K_T_max >= 2");
        const size_t nw = mxGetNumberOfElements(prhs[9]), np8 = mxGetNumberOfElements(prhs[10]);
        need(nw == 0 || nw == 3, "wind must have 3 elements (or be empty)");
        need(np8 == 0 || (mxGetM(prhs[10]) == 8 && np8 % 8 == 0), "pushes must be 8 x n: agent (1-based), column (0-based), dp (3), dv (3) (or empty)");
        std::vector<dmpc_push> push(np8 / 8);
        for (size_t j = 0; j < push.size(); ++j) {
            const double *q = mxGetPr(prhs[10]) + 8 * j;
            push[j].scene = 0; push[j].agent = (int32_t)q[0] - 1; push[j].column = (int32_t)q[1];
            for (int c = 0; c < 3; ++c) { push[j].dp[c] = q[2 + c]; push[j].dv[c] = q[5 + c]; }
        }
        const dmpc_disturbance dist{(uint64_t)mxGetScalar(prhs[8]), mxGetScalar(prhs[6]), mxGetScalar(prhs[7]), nw ? mxGetPr(prhs[9]) : nullptr, nw ? 1 : 0,
                                    push.empty() ? nullptr : push.data(), (int)push.size()};
        const mwSize d3[3] = {3, (mwSize)KT, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        int32_t used = 0, sst = 0;
        if (dmpc_set_disturbance(ctx, &dist)) mexErrMsgIdAndTxt("dmpc:transition_disturbed", "%s", dmpc_last_error(ctx));
        const int rc = Nc == N ? dmpc_transition(ctx, 1, N, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v),
                                                 mxGetPr(a), &used, &sst)
                               : dmpc_transition_cmd(ctx, 1, N, Nc, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v),
                                                     mxGetPr(a), &used, &sst);
        const std::string why = rc ? dmpc_last_error(ctx) : "";
        dmpc_set_disturbance(ctx, nullptr);   // the contexts are kept between calls: the setting must not outlive this one
        if (rc) mexErrMsgIdAndTxt("dmpc:transition_disturbed", "%s", why.c_str());
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)used);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)sst);
        return;
    }
    if (!std::strcmp(cmd, "transition_feedback")) {   // 'transition_disturbed' under a feedback policy (dmpc_set_feedback): set both, fly, read the log, clear both
        need(nrhs == 14, "transition_feedback: (cmd, params, po, pf, K_T_max, error_tol, trigger_p, trigger_v, reanchor, noise_p, noise_v, seed, wind, pushes)");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), Nc = (int)(mxGetNumberOfElements(prhs[3]) / 3), KT = (int)mxGetScalar(prhs[4]);
        need(N >= 1 && Nc >= 1 && Nc <= N && mxGetNumberOfElements(prhs[3]) == (size_t)3 * Nc && KT >= 2, "po must be 3 x N, pf 3 x N_cmd (N_cmd <= N), K_T_max >= 2");
        const size_t nw = mxGetNumberOfElements(prhs[12]), np8 = mxGetNumberOfElements(prhs[13]);
        need(nw == 0 || nw == 3, "wind must have 3 elements (or be empty)");
        need(np8 == 0 || (mxGetM(prhs[13]) == 8 && np8 % 8 == 0), "pushes must be 8 x n: agent (1-based), column (0-based), dp (3), dv (3) (or empty)");
        std::vector<dmpc_push> push(np8 / 8);
        for (size_t j = 0; j < push.size(); ++j) {
            const double *q = mxGetPr(prhs[13]) + 8 * j;
            push[j].scene = 0; push[j].agent = (int32_t)q[0] - 1; push[j].column = (int32_t)q[1];
            for (int c = 0; c < 3; ++c) { push[j].dp[c] = q[2 + c]; push[j].dv[c] = q[5 + c]; }
        }
        const dmpc_disturbance dist{(uint64_t)mxGetScalar(prhs[11]), mxGetScalar(prhs[9]), mxGetScalar(prhs[10]), nw ? mxGetPr(prhs[12]) : nullptr, nw ? 1 : 0,
                                    push.empty() ? nullptr : push.data(), (int)push.size()};
        const dmpc_feedback fbk{mxGetScalar(prhs[6]), mxGetScalar(prhs[7]), (int32_t)mxGetScalar(prhs[8])};
        const mwSize d3[3] = {3, (mwSize)KT, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        int32_t used = 0, sst = 0;
        if (dmpc_set_feedback(ctx, &fbk)) mexErrMsgIdAndTxt("dmpc:transition_feedback", "%s", dmpc_last_error(ctx));
        if (dmpc_set_disturbance(ctx, &dist)) {
            const std::string why = dmpc_last_error(ctx);
            dmpc_set_feedback(ctx, nullptr);
            mexErrMsgIdAndTxt("dmpc:transition_feedback", "%s", why.c_str());
        }
        int rc = Nc == N ? dmpc_transition(ctx, 1, N, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a),
                                           &used, &sst)
                         : dmpc_transition_cmd(ctx, 1, N, Nc, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v),
                                               mxGetPr(a), &used, &sst);
        mxArray *f[11];   // event_count, event_first, event_last, dev_p_col, dev_v_col | dev_p_max, dev_v_max | xh_p, xh_v, e_p, e_v
        for (int u = 0; u < 11; ++u) f[u] = mxCreateDoubleMatrix(u < 7 ? 1 : 3, Nc, mxREAL);
        std::vector<int32_t> li((size_t)5 * Nc);
        if (!rc) rc = dmpc_feedback_log(ctx, 1, Nc, &li[0], &li[Nc], &li[2 * (size_t)Nc], mxGetPr(f[5]), &li[3 * (size_t)Nc], mxGetPr(f[6]), &li[4 * (size_t)Nc],
                                        mxGetPr(f[7]), mxGetPr(f[8]), mxGetPr(f[9]), mxGetPr(f[10]));
        const std::string why = rc ? dmpc_last_error(ctx) : "";
        dmpc_set_disturbance(ctx, nullptr);   // the contexts are kept between calls: the settings must not outlive this one
        dmpc_set_feedback(ctx, nullptr);
        if (rc) mexErrMsgIdAndTxt("dmpc:transition_feedback", "%s", why.c_str());
        for (int u = 0; u < 5; ++u)
            for (int i = 0; i < Nc; ++i) mxGetPr(f[u])[i] = (double)li[(size_t)u * Nc + i];
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)used);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)sst);
        static const int order[11] = {0, 1, 2, 5, 3, 6, 4, 7, 8, 9, 10};   // dmpc_feedback_log's order of outputs
        for (int u = 0; u < 11; ++u) if (nlhs > 5 + u) plhs[5 + u] = f[order[u]];
        return;
    }
    if (!std::strcmp(cmd, "transition_estimated")) {   // 'transition_feedback' behind a measurement (dmpc_set_measurement): set all three, fly, read both logs, clear all three
        need(nrhs == 19, "transition_estimated: (cmd, params, po, pf, K_T_max, error_tol, trigger_p, trigger_v, reanchor, noise_p, noise_v, seed, wind, pushes, meas_p, meas_v, gain_p, gain_v, meas_seed)");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), Nc = (int)(mxGetNumberOfElements(prhs[3]) / 3), KT = (int)mxGetScalar(prhs[4]);
        need(N >= 1 && Nc >= 1 && Nc <= N && mxGetNumberOfElements(prhs[3]) == (size_t)3 * Nc && KT >= 2, "po must be 3 x N, pf 3 x N_cmd (N_cmd <= N), K_T_max >= 2");
        const size_t nw = mxGetNumberOfElements(prhs[12]), np8 = mxGetNumberOfElements(prhs[13]);
        need(nw == 0 || nw == 3, "wind must have 3 elements (or be empty)");
        need(np8 == 0 || (mxGetM(prhs[13]) == 8 && np8 % 8 == 0), "pushes must be 8 x n: agent (1-based), column (0-based), dp (3), dv (3) (or empty)");
        std::vector<dmpc_push> push(np8 / 8);
        for (size_t j = 0; j < push.size(); ++j) {
            const double *q = mxGetPr(prhs[13]) + 8 * j;
            push[j].scene = 0; push[j].agent = (int32_t)q[0] - 1; push[j].column = (int32_t)q[1];
            for (int c = 0; c < 3; ++c) { push[j].dp[c] = q[2 + c]; push[j].dv[c] = q[5 + c]; }
        }
        const dmpc_disturbance dist{(uint64_t)mxGetScalar(prhs[11]), mxGetScalar(prhs[9]), mxGetScalar(prhs[10]), nw ? mxGetPr(prhs[12]) : nullptr, nw ? 1 : 0,
                                    push.empty() ? nullptr : push.data(), (int)push.size()};
        const dmpc_feedback fbk{mxGetScalar(prhs[6]), mxGetScalar(prhs[7]), (int32_t)mxGetScalar(prhs[8])};
        const dmpc_measurement meas{(uint64_t)mxGetScalar(prhs[18]), mxGetScalar(prhs[14]), mxGetScalar(prhs[15]), mxGetScalar(prhs[16]), mxGetScalar(prhs[17])};
        const mwSize d3[3] = {3, (mwSize)KT, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        int32_t used = 0, sst = 0;
        auto clear = [&]() { dmpc_set_disturbance(ctx, nullptr); dmpc_set_feedback(ctx, nullptr); dmpc_set_measurement(ctx, nullptr); };   // the contexts are kept between calls: the settings must not outlive this one
        if (dmpc_set_feedback(ctx, &fbk) || dmpc_set_measurement(ctx, &meas) || dmpc_set_disturbance(ctx, &dist)) {
            const std::string why = dmpc_last_error(ctx);
            clear();
            mexErrMsgIdAndTxt("dmpc:transition_estimated", "%s", why.c_str());
        }
        int rc = Nc == N ? dmpc_transition(ctx, 1, N, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a),
                                           &used, &sst)
                         : dmpc_transition_cmd(ctx, 1, N, Nc, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v),
                                               mxGetPr(a), &used, &sst);
        mxArray *f[11];   // event_count, event_first, event_last, dev_p_col, dev_v_col | dev_p_max, dev_v_max | xh_p, xh_v, e_p, e_v
        for (int u = 0; u < 11; ++u) f[u] = mxCreateDoubleMatrix(u < 7 ? 1 : 3, Nc, mxREAL);
        mxArray *g[10];   // err_p_col, err_v_col, dev_p_col, dev_v_col | err_p_max, err_v_max, dev_p_max, dev_v_max | eh_p, eh_v
        for (int u = 0; u < 10; ++u) g[u] = mxCreateDoubleMatrix(u < 8 ? 1 : 3, Nc, mxREAL);
        std::vector<int32_t> li((size_t)5 * Nc), gi((size_t)4 * Nc);
        if (!rc) rc = dmpc_feedback_log(ctx, 1, Nc, &li[0], &li[Nc], &li[2 * (size_t)Nc], mxGetPr(f[5]), &li[3 * (size_t)Nc], mxGetPr(f[6]), &li[4 * (size_t)Nc],
                                        mxGetPr(f[7]), mxGetPr(f[8]), mxGetPr(f[9]), mxGetPr(f[10]));
        if (!rc) rc = dmpc_estimate_log(ctx, 1, Nc, mxGetPr(g[4]), &gi[0], mxGetPr(g[5]), &gi[Nc], mxGetPr(g[6]), &gi[2 * (size_t)Nc], mxGetPr(g[7]), &gi[3 * (size_t)Nc],
                                        mxGetPr(g[8]), mxGetPr(g[9]));
        const std::string why = rc ? dmpc_last_error(ctx) : "";
        clear();
        if (rc) mexErrMsgIdAndTxt("dmpc:transition_estimated", "%s", why.c_str());
        for (int u = 0; u < 5; ++u)
            for (int i = 0; i < Nc; ++i) mxGetPr(f[u])[i] = (double)li[(size_t)u * Nc + i];
        for (int u = 0; u < 4; ++u)
            for (int i = 0; i < Nc; ++i) mxGetPr(g[u])[i] = (double)gi[(size_t)u * Nc + i];
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)used);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)sst);
        static const int order[11] = {0, 1, 2, 5, 3, 6, 4, 7, 8, 9, 10};   // dmpc_feedback_log's order of outputs
        for (int u = 0; u < 11; ++u) if (nlhs > 5 + u) plhs[5 + u] = f[order[u]];
        static const int eorder[10] = {4, 0, 5, 1, 6, 2, 7, 3, 8, 9};      // dmpc_estimate_log's
        for (int u = 0; u < 10; ++u) if (nlhs > 16 + u) plhs[16 + u] = g[eorder[u]];
        return;
    }
    if (!std::strcmp(cmd, "flight_end")) {   // where the last 'transition*' of this context ended (dmpc_flight_end): what 'transition_from' takes
        need(nrhs == 3, "flight_end: (cmd, params, N_cmd)");
        const int Nc = (int)mxGetScalar(prhs[2]);
        need(Nc >= 1, "N_cmd must be >= 1");
        const mwSize d3[3] = {3, (mwSize)p.K, (mwSize)Nc};
        mxArray *o[6];
        for (int u = 0; u < 6; ++u) o[u] = u < 3 ? mxCreateDoubleMatrix(3, Nc, mxREAL) : mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        int32_t col = 0;
        if (dmpc_flight_end(ctx, 1, Nc, mxGetPr(o[0]), mxGetPr(o[1]), mxGetPr(o[2]), mxGetPr(o[3]), mxGetPr(o[4]), mxGetPr(o[5]), &col))
            mexErrMsgIdAndTxt("dmpc:flight_end", "%s", dmpc_last_error(ctx));
        plhs[0] = o[0];
        for (int u = 1; u < 6; ++u) if (nlhs > u) plhs[u] = o[u];
        if (nlhs > 6) plhs[6] = mxCreateDoubleScalar((double)col);
        return;
    }
    if (!std::strcmp(cmd, "transition_from")) {   // 'transition' from a given or carried state and plan (dmpc_set_start): set, fly, clear on any error
        need(nrhs == 12 || nrhs == 13, "transition_from: (cmd, params, po, pf, K_T_max, error_tol, vo, ao, plan_p, plan_v, plan_a, col0[, from_end])");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), Nc = (int)(mxGetNumberOfElements(prhs[3]) / 3), KT = (int)mxGetScalar(prhs[4]);
        need(N >= 1 && Nc >= 1 && Nc <= N && mxGetNumberOfElements(prhs[3]) == (size_t)3 * Nc && KT >= 2, "po must be 3 x N, pf 3 x N_cmd (N_cmd <= N), K_T_max >= 2");
        const double *arr[5];
        for (int u = 0; u < 5; ++u) {   // vo, ao: 3 x N_cmd; plan_p, plan_v, plan_a: 3 x K x N_cmd; or []
            const size_t n = mxGetNumberOfElements(prhs[6 + u]), want = (size_t)(u < 2 ? 3 : n3) * Nc;
            need(n == 0 || n == want, "vo, ao must be 3 x N_cmd, plan_p, plan_v, plan_a 3 x K x N_cmd (or empty)");
            arr[u] = n ? mxGetPr(prhs[6 + u]) : nullptr;
        }
        const dmpc_start start{1, Nc, nrhs == 13 && mxGetScalar(prhs[12]) != 0.0, nullptr, arr[0], arr[1], arr[2], arr[3], arr[4], (int32_t)mxGetScalar(prhs[11])};
        const mwSize d3[3] = {3, (mwSize)KT, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        int32_t used = 0, sst = 0;
        if (dmpc_set_start(ctx, &start)) mexErrMsgIdAndTxt("dmpc:transition_from", "%s", dmpc_last_error(ctx));
        const int rc = dmpc_transition_cmd(ctx, 1, N, Nc, mxGetPr(prhs[2]), mxGetPr(prhs[3]), KT, mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a),
                                           &used, &sst);
        const std::string why = rc ? dmpc_last_error(ctx) : "";
        if (rc) dmpc_set_start(ctx, nullptr);   // the contexts are kept between calls: a start that was not consumed must not outlive this one
        if (rc) mexErrMsgIdAndTxt("dmpc:transition_from", "%s", why.c_str());
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)used);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)sst);
        return;
    }
    if (!std::strcmp(cmd, "mission")) {   // one trial through a sequence of goal sets (dmpc_transition_mission)
        need(nrhs == 6 || nrhs == 7, "mission: (cmd, params, po, goals, K_T_max, error_tol[, deadline])");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), KT = (int)mxGetScalar(prhs[4]);
        const mwSize *gd = mxGetDimensions(prhs[3]);
        const int Nc = mxGetNumberOfDimensions(prhs[3]) >= 2 ? (int)gd[1] : 0;
        const int Q = Nc >= 1 ? (int)(mxGetNumberOfElements(prhs[3]) / ((size_t)3 * Nc)) : 0;
        need(N >= 1 && Nc >= 1 && Nc <= N && Q >= 1 && gd[0] == 3 && mxGetNumberOfElements(prhs[3]) == (size_t)3 * Nc * Q && KT >= 2,
             "po must be 3 x N, goals 3 x N_cmd x Q (N_cmd <= N, Q >= 1), K_T_max >= 2");
        const bool with_dl = nrhs == 7 && mxGetNumberOfElements(prhs[6]) > 0;
        need(!with_dl || mxGetNumberOfElements(prhs[6]) == (size_t)Q, "deadline must have Q elements (or be empty)");
        std::vector<int32_t> dl((size_t)Q, 0), col((size_t)Q, -1);
        for (int q = 0; with_dl && q < Q; ++q) dl[(size_t)q] = (int32_t)mxGetPr(prhs[6])[q];
        const mwSize d3[3] = {3, (mwSize)KT, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        int32_t used = 0, sst = 0;
        if (dmpc_transition_mission(ctx, 1, N, Nc, Q, mxGetPr(prhs[2]), mxGetPr(prhs[3]), with_dl ? dl.data() : nullptr, nullptr, 0, KT,
                                    mxGetScalar(prhs[5]), mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a), &used, &sst, col.data()))
            mexErrMsgIdAndTxt("dmpc:mission", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)used);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)sst);
        if (nlhs > 5) {
            plhs[5] = mxCreateDoubleMatrix(1, (mwSize)Q, mxREAL);
            for (int q = 0; q < Q; ++q) mxGetPr(plhs[5])[q] = (double)col[(size_t)q];
        }
        return;
    }
    if (!std::strcmp(cmd, "route")) {   // one trial with waypoints of its own for every commanded agent (dmpc_transition_route)
        need(nrhs >= 7 && nrhs <= 9, "route: (cmd, params, po, waypoints, K_T_max, error_tol, capture[, n_wp[, timeout]])");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), KT = (int)mxGetScalar(prhs[4]);
        const mwSize *wd = mxGetDimensions(prhs[3]);
        const int W = mxGetNumberOfDimensions(prhs[3]) >= 2 ? (int)wd[1] : 0;
        const int Nc = W >= 1 ? (int)(mxGetNumberOfElements(prhs[3]) / ((size_t)3 * W)) : 0;
        need(N >= 1 && W >= 1 && Nc >= 1 && Nc <= N && wd[0] == 3 && mxGetNumberOfElements(prhs[3]) == (size_t)3 * W * Nc && KT >= 2,
             "po must be 3 x N, waypoints 3 x W x N_cmd (N_cmd <= N, W >= 1), K_T_max >= 2");
        const bool with_n = nrhs >= 8 && mxGetNumberOfElements(prhs[7]) > 0;
        need(!with_n || mxGetNumberOfElements(prhs[7]) == (size_t)Nc, "n_wp must have N_cmd elements (or be empty)");
        std::vector<int32_t> n_wp((size_t)Nc, W), col((size_t)Nc * W, -1);
        for (int i = 0; with_n && i < Nc; ++i) n_wp[(size_t)i] = (int32_t)mxGetPr(prhs[7])[i];
        const int timeout = nrhs >= 9 ? (int)mxGetScalar(prhs[8]) : 0;
        const mwSize d3[3] = {3, (mwSize)KT, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        int32_t used = 0, sst = 0;
        if (dmpc_transition_route(ctx, 1, N, Nc, W, mxGetPr(prhs[2]), mxGetPr(prhs[3]), with_n ? n_wp.data() : nullptr, mxGetScalar(prhs[6]), timeout,
                                  nullptr, 0, KT, mxGetScalar(prhs[5]), 0, mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a), &used, &sst, col.data(), nullptr,
                                  nullptr, nullptr, nullptr))
            mexErrMsgIdAndTxt("dmpc:route", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)used);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)sst);
        if (nlhs > 5) {
            plhs[5] = mxCreateDoubleMatrix((mwSize)W, (mwSize)Nc, mxREAL);
            for (size_t j = 0; j < col.size(); ++j) mxGetPr(plhs[5])[j] = (double)col[j];
        }
        return;
    }
    if (!std::strcmp(cmd, "assign")) {   // which agent takes which goal (dmpc_assign_goals); a scene that met the round cap: perm 0, cost NaN, rounds -1
        need(nrhs >= 4 && nrhs <= 6, "assign: (cmd, params, po, goals[, eps[, max_rounds]])");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3);
        need(N >= 1 && mxGetM(prhs[2]) == 3 && mxGetM(prhs[3]) == 3 && mxGetNumberOfElements(prhs[2]) == (size_t)3 * N &&
             mxGetNumberOfElements(prhs[3]) == (size_t)3 * N, "po and goals must both be 3 x N");
        const double eps = nrhs > 4 && mxGetNumberOfElements(prhs[4]) > 0 ? mxGetScalar(prhs[4]) : 1e-4 / N;
        const int max_rounds = nrhs > 5 ? (int)mxGetScalar(prhs[5]) : 0;
        std::vector<int32_t> perm((size_t)N, 0);
        mxArray *pf = mxCreateDoubleMatrix(3, (mwSize)N, mxREAL);
        double cost = 0.0;
        int32_t rounds = 0;
        if (dmpc_assign_goals(ctx, 1, N, mxGetPr(prhs[2]), mxGetPr(prhs[3]), eps, max_rounds, perm.data(), mxGetPr(pf), nullptr, &cost, &rounds))
            mexErrMsgIdAndTxt("dmpc:assign", "%s", dmpc_last_error(ctx));
        plhs[0] = mxCreateDoubleMatrix(1, (mwSize)N, mxREAL);
        for (int i = 0; i < N; ++i) mxGetPr(plhs[0])[i] = (double)(perm[(size_t)i] + 1);
        if (nlhs > 1) plhs[1] = pf;
        if (nlhs > 2) plhs[2] = mxCreateDoubleScalar(cost);
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)rounds);
        return;
    }
    if (!std::strcmp(cmd, "assign_rect")) {   // N agents, M goals (dmpc_assign_rect); 0: "none"; a scene that met the round cap: perm and owner 0, cost NaN, rounds -1
        need(nrhs >= 4 && nrhs <= 6, "assign_rect: (cmd, params, po, goals[, eps[, max_rounds]])");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), M = (int)(mxGetNumberOfElements(prhs[3]) / 3);
        need(N >= 1 && M >= 1 && mxGetM(prhs[2]) == 3 && mxGetM(prhs[3]) == 3 && mxGetNumberOfElements(prhs[2]) == (size_t)3 * N &&
             mxGetNumberOfElements(prhs[3]) == (size_t)3 * M, "po must be 3 x N and goals 3 x M");
        const double eps = nrhs > 4 && mxGetNumberOfElements(prhs[4]) > 0 ? mxGetScalar(prhs[4]) : 1e-4 / (N > M ? N : M);
        const int max_rounds = nrhs > 5 ? (int)mxGetScalar(prhs[5]) : 0;
        std::vector<int32_t> perm((size_t)N, 0), owner((size_t)M, 0);
        mxArray *pf = mxCreateDoubleMatrix(3, (mwSize)N, mxREAL);
        double cost = 0.0;
        int32_t rounds = 0;
        if (dmpc_assign_rect(ctx, 1, N, M, mxGetPr(prhs[2]), mxGetPr(prhs[3]), eps, max_rounds, perm.data(), owner.data(), mxGetPr(pf), nullptr, &cost,
                             &rounds))
            mexErrMsgIdAndTxt("dmpc:assign_rect", "%s", dmpc_last_error(ctx));
        plhs[0] = mxCreateDoubleMatrix(1, (mwSize)N, mxREAL);
        for (int i = 0; i < N; ++i) mxGetPr(plhs[0])[i] = (double)(perm[(size_t)i] + 1);
        if (nlhs > 1) plhs[1] = pf;
        if (nlhs > 2) {
            plhs[2] = mxCreateDoubleMatrix(1, (mwSize)M, mxREAL);
            for (int j = 0; j < M; ++j) mxGetPr(plhs[2])[j] = (double)(owner[(size_t)j] + 1);
        }
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar(cost);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)rounds);
        return;
    }
    if (!std::strcmp(cmd, "plan")) {   // which way round the static vehicles (dmpc_plan_routes): the waypoints 'route' takes
        need(nrhs >= 5 && nrhs <= 8, "plan: (cmd, params, po, goals, cell[, margin[, W[, obstacles]]])");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), Nc = (int)(mxGetNumberOfElements(prhs[3]) / 3);
        need(N >= 1 && Nc >= 1 && Nc <= N && mxGetM(prhs[2]) == 3 && mxGetM(prhs[3]) == 3 && mxGetNumberOfElements(prhs[2]) == (size_t)3 * N &&
             mxGetNumberOfElements(prhs[3]) == (size_t)3 * Nc, "po must be 3 x N, goals 3 x N_cmd (N_cmd <= N)");
        const double margin = nrhs > 5 && mxGetNumberOfElements(prhs[5]) > 0 ? mxGetScalar(prhs[5]) : 0.0;
        const int W = nrhs > 6 && mxGetNumberOfElements(prhs[6]) > 0 ? (int)mxGetScalar(prhs[6]) : 4;
        const int Mx = nrhs > 7 ? (int)(mxGetNumberOfElements(prhs[7]) / 3) : 0;
        need(Mx == 0 || (mxGetM(prhs[7]) == 3 && mxGetNumberOfElements(prhs[7]) == (size_t)3 * Mx), "obstacles must be 3 x M");
        need(W >= 1, "W must be at least 1");
        const int M = N - Nc + Mx;
        std::vector<double> obst(mxGetPr(prhs[2]) + (size_t)3 * Nc, mxGetPr(prhs[2]) + (size_t)3 * N);
        if (Mx) obst.insert(obst.end(), mxGetPr(prhs[7]), mxGetPr(prhs[7]) + (size_t)3 * Mx);
        std::vector<int32_t> n_wp((size_t)Nc, 0), st((size_t)Nc, 0), hops((size_t)Nc, 0);
        const mwSize d3[3] = {3, (mwSize)W, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        if (dmpc_plan_routes(ctx, 1, Nc, M, W, mxGetPr(prhs[2]), mxGetPr(prhs[3]), M ? obst.data() : nullptr, mxGetScalar(prhs[4]), margin,
                             mxGetPr(plhs[0]), n_wp.data(), st.data(), hops.data()))
            mexErrMsgIdAndTxt("dmpc:plan", "%s", dmpc_last_error(ctx));
        const std::vector<int32_t> *outs[3] = {&n_wp, &st, &hops};
        for (int o = 0; o < 3 && nlhs > o + 1; ++o) {
            plhs[o + 1] = mxCreateDoubleMatrix(1, (mwSize)Nc, mxREAL);
            for (int i = 0; i < Nc; ++i) mxGetPr(plhs[o + 1])[i] = (double)(*outs[o])[(size_t)i];
        }
        return;
    }
    if (!std::strcmp(cmd, "replan")) {   // plan, route and re-plans during the flight (dmpc_transition_replan)
        need(nrhs >= 8 && nrhs <= 14, "replan: (cmd, params, po, goals, K_T_max, error_tol, cell, capture[, margin[, W[, every[, ahead[, path[, timeout]]]]]])");
        const int N = (int)(mxGetNumberOfElements(prhs[2]) / 3), Nc = (int)(mxGetNumberOfElements(prhs[3]) / 3), KT = (int)mxGetScalar(prhs[4]);
        need(N >= 1 && Nc >= 1 && Nc <= N && mxGetM(prhs[2]) == 3 && mxGetM(prhs[3]) == 3 && mxGetNumberOfElements(prhs[2]) == (size_t)3 * N &&
             mxGetNumberOfElements(prhs[3]) == (size_t)3 * Nc && KT >= 2, "po must be 3 x N, goals 3 x N_cmd (N_cmd <= N), K_T_max >= 2");
        auto opt = [&](int i, double dflt) { return nrhs > i && mxGetNumberOfElements(prhs[i]) > 0 ? mxGetScalar(prhs[i]) : dflt; };
        const double margin = opt(8, 0.0);
        const int W = (int)opt(9, 4.0), every = (int)opt(10, 5.0), ahead = (int)opt(11, 0.0), timeout = (int)opt(13, 0.0);
        need(W >= 1, "W must be at least 1");
        const bool scripted = nrhs > 12 && mxGetNumberOfElements(prhs[12]) > 0;
        int M = 0, P = 0;
        if (scripted) {
            const mwSize *pd = mxGetDimensions(prhs[12]);
            P = mxGetNumberOfDimensions(prhs[12]) >= 2 ? (int)pd[1] : 0;
            M = P >= 1 ? (int)(mxGetNumberOfElements(prhs[12]) / ((size_t)3 * P)) : 0;
            need(pd[0] == 3 && P >= 1 && M >= 1 && mxGetNumberOfElements(prhs[12]) == (size_t)3 * P * M && N == Nc,
                 "path must be 3 x P x M, and po then covers the commanded agents (3 x N_cmd)");
        }
        const mwSize d3[3] = {3, (mwSize)KT, (mwSize)Nc}, w3[3] = {3, (mwSize)W, (mwSize)Nc};
        plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *v = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *a = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
        mxArray *wp = mxCreateNumericArray(3, w3, mxDOUBLE_CLASS, mxREAL);
        std::vector<int32_t> n_wp((size_t)Nc, 0), st((size_t)Nc, 0), cnt((size_t)Nc, 0), rcol((size_t)Nc, -1), col((size_t)Nc * W, -1);
        int32_t used = 0, sst = 0;
        if (dmpc_transition_replan(ctx, 1, N + M, Nc, W, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetScalar(prhs[6]), margin, every, ahead, mxGetScalar(prhs[7]),
                                   timeout, scripted ? mxGetPr(prhs[12]) : nullptr, P, KT, mxGetScalar(prhs[5]), 0, mxGetPr(plhs[0]), mxGetPr(v), mxGetPr(a),
                                   &used, &sst, mxGetPr(wp), n_wp.data(), st.data(), col.data(), nullptr, cnt.data(), rcol.data(), nullptr, nullptr, nullptr))
            mexErrMsgIdAndTxt("dmpc:replan", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = v; if (nlhs > 2) plhs[2] = a;
        if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)used);
        if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)sst);
        if (nlhs > 5) plhs[5] = wp;
        const std::vector<int32_t> *rows[3] = {&n_wp, &cnt, &rcol};
        for (int o = 0; o < 3 && nlhs > o + 6; ++o) {
            plhs[o + 6] = mxCreateDoubleMatrix(1, (mwSize)Nc, mxREAL);
            for (int i = 0; i < Nc; ++i) mxGetPr(plhs[o + 6])[i] = (double)(*rows[o])[(size_t)i];
        }
        if (nlhs > 9) {
            plhs[9] = mxCreateDoubleMatrix((mwSize)W, (mwSize)Nc, mxREAL);
            for (size_t j = 0; j < col.size(); ++j) mxGetPr(plhs[9])[j] = (double)col[j];
        }
        if (nlhs > 10) {
            plhs[10] = mxCreateDoubleMatrix(1, (mwSize)Nc, mxREAL);
            for (int i = 0; i < Nc; ++i) mxGetPr(plhs[10])[i] = (double)st[(size_t)i];
        }
        return;
    }
    if (!std::strcmp(cmd, "random_test") || !std::strcmp(cmd, "random_exchange")) {   // randomTest.m / randomExchange.m
        const bool ex = cmd[7] == 'e';
        need(nrhs == (ex ? 7 : 8), ex ? "random_exchange: (cmd, params, N, pmin, pmax, rmin, seed)" : "random_test: (cmd, params, N, pmin, pmax, rmin, c, seed)");
        const int N = (int)mxGetScalar(prhs[2]);
        need(N >= 1 && mxGetNumberOfElements(prhs[3]) == 3 && mxGetNumberOfElements(prhs[4]) == 3, "pmin, pmax must have 3 elements");
        plhs[0] = mxCreateDoubleMatrix(3, N, mxREAL);
        mxArray *pf = mxCreateDoubleMatrix(3, N, mxREAL);
        const int rc = ex ? dmpc_random_exchange(ctx, 1, N, mxGetPr(prhs[3]), mxGetPr(prhs[4]), mxGetScalar(prhs[5]), (uint64_t)mxGetScalar(prhs[6]),
                                                 mxGetPr(plhs[0]), mxGetPr(pf))
                          : dmpc_random_test(ctx, 1, N, mxGetPr(prhs[3]), mxGetPr(prhs[4]), mxGetScalar(prhs[5]), mxGetScalar(prhs[6]),
                                             (uint64_t)mxGetScalar(prhs[7]), mxGetPr(plhs[0]), mxGetPr(pf));
        if (rc) mexErrMsgIdAndTxt("dmpc:random", "%s", dmpc_last_error(ctx));
        if (nlhs > 1) plhs[1] = pf;
        return;
    }
    mexErrMsgIdAndTxt("dmpc:cmd", "unknown command %s", cmd);
}
