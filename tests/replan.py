"""Test helper: re-planned routes (dmpc_transition_replan, dmpc_replan_routes_device) -- the pinned rule of include/dmpc_hip.h as a host loop over an
MPC step, composed from tests/plan.py (the plan rule) and tests/route.py (the waypoint rule, whose loop is repeated here because the re-plan stands
inside it), the scenes the tests use, and raw ctypes calls of the entries.

There is no reference counterpart.  The rule, per scene, on top of route.route_loop's:
  obst(k)    with a path: sample(j, k + a), a = 0 .. ahead, of every scripted vehicle j (scripted.sample: clamped at P - 1); without: po[N_cmd:]
  column 0   waypoints, n_wp, plan_status = plan.plan(po_cmd, goals, obst(0)); cur = since = 0
  checked    after the route rule of column k, its switches included, when every > 0, 0 < k < K_T_max - 1, k % every == 0 and the trial is not over
  legs       of agent i: the cells of x_p_i(k), wp[i][cur], .., wp[i][n_wp - 1]; a leg a -> b is clear when plan.clear(free_i, a, b) holds on
             blocked(k) with free_i = not blocked, or the agent's current cell, or its goal's cell; a leg with a == b when that one cell is free_i
  re-plan    some leg not clear: wp[i], n_wp[i], plan_status[i] = plan.plan_agent(blocked(k), x_p_i(k), goal_i); cur = 0, since = k, the agent's
             wp_col row = -1, replan_count[i] += 1, replan_col[i] = k; the new waypoint 0 is first examined on column k + 1
"""
import ctypes as C
import functools

import numpy as np

import hold as hd
import mission as ms
import obstacles as ob
import plan as pl
import route as rt
import scripted as sc
from obstacles import KW, _dp, _ip, _f   # noqa: F401

REACHED = rt.REACHED
HELD = rt.HELD


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------
def leg_clear(free, a, b):
    """plan.clear, and a leg inside one cell (plan.clear divides by zero there): that cell must be free"""
    return bool(free[a]) if a == b else pl.clear(free, a, b)


def legs_clear(blocked, xp, wp, cur, n_wp, goal, pmin, cell):
    """the remaining legs of one agent on a scene's blocked grid"""
    n = blocked.shape
    c = lambda p: tuple(int(v) for v in pl.cell_of(p, pmin, cell, n))
    free = ~blocked
    free[c(xp)] = True
    free[c(goal)] = True
    cs = [c(xp)] + [c(wp[q]) for q in range(int(cur), int(n_wp))]
    return all(leg_clear(free, a, b) for a, b in zip(cs, cs[1:]))


def replan_step(blocked, xp, goals, wp, n_wp, cur, pmin, cell, skip=None):
    """ONE re-plan step on one scene (what dmpc_replan_routes_device does per scene): blocked [nx,ny,nz], xp, goals [nc,3], wp [nc,W,3], n_wp, cur
    [nc]; skip: the scene is over, nobody is looked at.  Returns [(i, waypoints [W,3], n_wp, status)] of the agents that are planned again."""
    out = []
    if skip:
        return out
    W = wp.shape[1]
    for i in range(wp.shape[0]):
        if legs_clear(blocked, xp[i], wp[i], cur[i], n_wp[i], goals[i], pmin, cell):
            continue
        w2, n2, st, _, _ = pl.plan_agent(blocked, xp[i], goals[i], pmin, cell, W)
        out.append((i, w2, int(n2), int(st)))
    return out


def boundary_distance(xp, pmin, cell):
    """the smallest distance [m] of a coordinate of xp [..,3] from a face of the grid's cells"""
    u = (np.asarray(xp, float) - np.asarray(pmin, float)) / cell
    return float((np.abs(u - np.round(u)) * cell).min())


def replan_loop(step, po, goals, cell, margin, W=4, every=5, ahead=0, capture=0.5, timeout=0, path=None, K_T_max=100, error_tol=0.05, max_hold=None,
                kw=KW):
    """The rule as a host loop.  step: as route.route_loop's.  po [N,3] (with a path: [nc,3]), goals [nc,3].  Returns route_loop's dict and
    waypoints [nc,W,3], n_wp, plan_status, replan_count, replan_col [nc] (the plan in force at the end), replans: [(column, agent, status, n_wp)],
    checked: the columns a re-plan was checked on, boundary_margin: the smallest distance of any x_p from a cell face on those columns."""
    po, goals = np.asarray(po, float), np.asarray(goals, float)
    nc = goals.shape[0]
    M = path.shape[0] if path is not None else po.shape[0] - nc
    pmin, pmax, h, alim = kw["pmin"], kw["pmax"], kw["h"], kw["alim"]

    def obst(k):
        if path is None:
            return po[nc:]
        return np.concatenate([sc.sample(path, k + a) for a in range(ahead + 1)])

    def grid(k):
        return pl.blocked_grid(obst(k), pmin, pmax, cell, margin, kw["rmin"], kw["c"])

    first = pl.plan(po[None, :nc], goals[None], obst(0)[None], cell, margin, W, kw)
    wp, n, pst = first["waypoints"][0].copy(), first["n_wp"][0].astype(int), first["plan_status"][0].copy()
    static_grid = grid(0) if path is None else None
    cur, since, col = np.zeros(nc, dtype=int), np.zeros(nc, dtype=int), np.full((nc, W), -1, dtype=np.int32)
    rcnt, rcol = np.zeros(nc, dtype=np.int32), np.full(nc, -1, dtype=np.int32)
    idx = np.arange(nc)
    goal = wp[idx, cur].copy()
    l = np.zeros((nc + M, 45))
    l[:nc] = ob.init_table(po[:nc], goal)
    xp, xv, xa = po[:nc].copy(), np.zeros((nc, 3)), np.zeros((nc, 3))
    pk, vk, ak = (np.zeros((nc, K_T_max, 3)) for _ in range(3))
    pk[:, 0] = xp
    used, sst = K_T_max, 1
    speeds, cap_margin, reach_margin, replans, checked, bmargin = [], [np.inf], {}, [], [], [np.inf]
    cap2 = capture * capture
    hold = max_hold is not None
    Pp, V, A = l[:nc].copy(), np.zeros((nc, 45)), np.zeros((nc, 45))
    run, cnt, hfirst = np.zeros(nc, dtype=int), np.zeros(nc, dtype=np.int32), np.full(nc, -1, dtype=np.int32)
    ast = np.zeros((nc, K_T_max), dtype=np.int32)
    ast[:, 0] = 1

    def route_rule(k, bits):
        """route.route_loop's rule of column k; True: the trial is over"""
        nonlocal used, sst
        if bits & ~1:
            used, sst = k + 1, bits
            return True
        d = xp - goal
        if (cur == n - 1).all():
            dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).max()
            reach_margin[k] = abs(float(dist) - error_tol)
            if ms.reached_goal(xp, goal, error_tol):
                used, sst = k + 1, REACHED
                return True
            return False
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        cand = cur < n - 1
        cap_margin.append(float(np.abs(np.sqrt(d2[cand]) - capture).min()))
        sw = cand & ((d2 < cap2) | ((timeout > 0) & (k - since >= timeout)))
        for i in np.nonzero(sw)[0]:
            col[i, cur[i]] = k
            speeds.append(float(np.linalg.norm(xv[i])))
        cur[sw] += 1
        since[sw] = k
        goal[sw] = wp[idx[sw], cur[sw]]
        return False

    def rule(k, bits):
        if route_rule(k, bits):
            return True
        if every > 0 and 0 < k < K_T_max - 1 and k % every == 0:
            checked.append(k)
            bmargin.append(boundary_distance(xp, pmin, cell))
            blocked = static_grid if path is None else grid(k)
            for i, w2, n2, st in replan_step(blocked, xp, goals, wp, n, cur, pmin, cell):
                wp[i], n[i], pst[i] = w2, n2, st
                cur[i], since[i], col[i] = 0, k, -1
                goal[i] = wp[i, 0]
                rcnt[i] += 1
                rcol[i] = k
                replans.append((k, int(i), st, n2))
        return False

    over = rule(0, 1)
    for k in range(1, K_T_max):
        if over:
            break
        if M:
            l[nc:] = sc.window(path, k) if path is not None else np.tile(po[nc:], (1, 15))
        here = (sc.sample(path, k - 1) if path is not None else po[nc:]) if M else np.zeros((0, 3))
        p, v, a, st = step(l, xp, xv, xa, goal, here)
        p, v, a, st = p.copy(), v.copy(), a.copy(), np.asarray(st).astype(np.int32)
        eff = st
        if hold:
            fail = st != 1
            run = np.where(fail, run + 1, 0)
            held = fail & (run <= max_hold)
            ast[:, k] = np.where(held, st | HELD, st)
            if held.any():
                p[held], v[held], a[held] = hd.shift_plan(Pp[held], V[held], A[held], h, alim)
                cnt[held] += 1
                hfirst[held & (hfirst < 0)] = k
            eff = np.where(held, 1, st)
        ok = (eff & 1) == 1
        l[:nc][ok] = p[ok]
        xp[ok], xv[ok], xa[ok] = p[ok, :3], v[ok, :3], a[ok, :3]
        Pp[ok], V[ok], A[ok] = p[ok], v[ok], a[ok]
        pk[:, k], vk[:, k], ak[:, k] = xp, xv, xa
        over = rule(k, int(np.bitwise_or.reduce(eff)))
    out = dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, wp_col=col, wp_index=cur.astype(np.int32), switch_speed=speeds,
               capture_margin=min(cap_margin), reach_margin=reach_margin, waypoints=wp, n_wp=n.astype(np.int32), plan_status=pst.astype(np.int32),
               replan_count=rcnt, replan_col=rcol, replans=replans, checked=checked, boundary_margin=min(bmargin))
    if hold:
        if cnt.any():
            out["scene_status"] = sst | HELD
        out.update(hold_count=cnt, hold_first=hfirst, agent_status=ast)
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
DOOR_P = 113
DOOR_START = np.array([(1.6, y, z) for z in (0.5, 1.2, 1.9) for y in (1.6, 2.0, 2.4)])     # nine scripted vehicles beside the wall's +y end
DOOR_PO = np.array([(-1.5, 0.6, 1.2), (-1.5, -0.7, 1.2)])
DOOR_CALL = dict(cell=0.25, margin=0.2, W=4, capture=0.5, timeout=0, error_tol=0.05, K_T_max=140)


def door(seed=0, moves=True):
    """route.WALL as paths that do not move, and a door of nine vehicles that moves from x = 1.6 to x = 0 at 0.2 m per column and stays: it shuts
    the wall's +y end by column 8.  Two agents from x = -1.5 to x = +1.5; seed > 0 jitters the starts by up to 3 cm; moves False: the door
    never moves.  dict(po [2,3], goals [2,3], path [30,P,3], kw) and DOOR_CALL's settings"""
    t = np.arange(DOOR_P)
    dr = np.repeat(DOOR_START[:, None, :], DOOR_P, axis=1)
    if moves:
        dr[:, :, 0] = np.maximum(0.0, 1.6 - 0.2 * t)[None, :]
    path = np.concatenate([np.repeat(rt.WALL[:, None, :], DOOR_P, axis=1), dr])
    po = DOOR_PO.copy()
    if seed:
        po += np.random.default_rng(7100 + seed).uniform(-0.03, 0.03, po.shape)
    return dict(DOOR_CALL, po=po, goals=DOOR_PO * np.array([-1.0, 1.0, 1.0]), path=path, kw=KW)


def loop_on(step, s, every, ahead=0, max_hold=None, **over):
    """replan_loop on a scene dict"""
    a = dict(s)
    a.update(over)
    return replan_loop(step, a["po"], a["goals"], a["cell"], a["margin"], a["W"], every, ahead, a["capture"], a["timeout"], a.get("path"), a["K_T_max"],
                       a["error_tol"], max_hold, a["kw"])


@functools.lru_cache(maxsize=None)
def oracle_result(name, every, ahead=0, seed=0):
    """the oracle's re-plan loop (solveSoftDMPCbound) on a named scene, computed once per session (shared by the tests: do not modify)"""
    from oracle import oracle as orc
    s = {"door": door, "wall": wall}[name](seed)
    return loop_on(ms.oracle_step(orc, orc.make_params("bound", **s["kw"])), s, every, ahead)


def wall(seed=0):
    """plan.wall() -- three agents round 21 static vehicles, no path -- with the settings of a re-planned flight"""
    s = pl.wall()
    po = s["po"].copy()
    if seed:
        po[:3] += np.random.default_rng(5000 + seed).uniform(-0.1, 0.1, (3, 3))
    return dict(po=po, goals=s["goals"], path=None, kw=KW, cell=0.25, margin=0.2, W=4, capture=s["capture"], timeout=0, error_tol=s["error_tol"],
                K_T_max=s["K_T_max"])


# ---- comparisons --------------------------------------------------------------------------------------------------------------------------------
ROUTE_KEYS = ("K_T_used", "scene_status", "wp_col", "wp_index")
PLAN_KEYS = ("waypoints", "n_wp", "plan_status", "replan_count", "replan_col")
HIST = ("pk", "vk", "ak")
HOLD = ("hold_count", "hold_first", "agent_status")


def same_as_loop(res, host, s=0, hold=False, hist=True):
    """scene s of an entry's result against a loop's dict, bit for bit"""
    assert int(res["K_T_used"][s]) == host["K_T_used"] and int(res["scene_status"][s]) == host["scene_status"], \
        (res["K_T_used"][s], host["K_T_used"], res["scene_status"][s], host["scene_status"])
    for k in ("wp_col", "wp_index") + PLAN_KEYS + (HIST if hist else ()) + (HOLD if hold else ()):
        a, b = np.asarray(res[k][s]), np.asarray(host[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a.tolist() if a.size < 40 else "", b.tolist() if b.size < 40 else "")


# ---- raw calls ----------------------------------------------------------------------------------------------------------------------------------
def raw_replan(d, po, goals, cell=0.25, margin=0.2, W=4, every=5, ahead=0, capture=0.5, timeout=0, path=None, K_T_max=100, error_tol=0.05, max_hold=0,
               n_cmd=None, P=None, histories=(1, 1, 1), outputs=True, ctx="own"):
    """dmpc_transition_replan on po [S,N,3] (with a path [S,M,P,3]: [S,N_cmd,3]), goals [S,N_cmd,3] (None: a NULL pointer; then n_cmd must be
    given); n_cmd, P override the shapes; histories: which of pk, vk, ak are passed; outputs False: every optional output NULL.  Returns (rc, dict)."""
    po = _f(po)
    goals = _f(goals) if goals is not None else None
    S = po.shape[0]
    nc = goals.shape[1] if n_cmd is None else n_cmd
    path = _f(path) if path is not None else None
    N = po.shape[1] + (path.shape[1] if path is not None else 0)
    P = (path.shape[2] if path is not None else 0) if P is None else P
    m, w = max(nc, 1), max(W, 1)
    pk, vk, ak = (np.zeros((S, m, K_T_max, 3)) for _ in range(3))
    used, sst = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    wp, col = np.zeros((S, m, w, 3)), np.zeros((S, m, w), dtype=np.int32)
    n_wp, pst, index, rcnt, rcol, cnt, first = (np.zeros((S, m), dtype=np.int32) for _ in range(7))
    ast = np.zeros((S, m, K_T_max), dtype=np.int32)
    hp = [_dp(a if on else None) for a, on in zip((pk, vk, ak), histories)]
    o = lambda a: (_dp if a.dtype == np.float64 else _ip)(a if outputs else None)
    rc = d._L.dmpc_transition_replan(d._ctx if ctx == "own" else ctx, S, N, nc, int(W), _dp(po), _dp(goals), C.c_double(cell), C.c_double(margin), int(every),
                                     int(ahead), C.c_double(capture), int(timeout), _dp(path), P, int(K_T_max), C.c_double(error_tol), int(max_hold), hp[0], hp[1],
                                     hp[2], _ip(used), _ip(sst), o(wp), o(n_wp), o(pst), o(col), o(index), o(rcnt), o(rcol), o(cnt), o(first), o(ast))
    return rc, dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, waypoints=wp, n_wp=n_wp, plan_status=pst, wp_col=col, wp_index=index,
                    replan_count=rcnt, replan_col=rcol, hold_count=cnt, hold_first=first, agent_status=ast)


STEP_KEYS = ("waypoints", "n_wp", "cur", "since", "wp_col", "pf", "plan_status", "replan_count", "replan_col")


def step_state(xp, goals, wp, n_wp, cur, fill=-7):
    """the arrays one re-plan step reads and writes, [S,nc,..]: the outputs it may leave alone are filled with a value no re-plan writes"""
    S, nc, W = wp.shape[:3]
    return dict(x_p=_f(xp), goals=_f(goals), waypoints=_f(wp).copy(), n_wp=np.ascontiguousarray(n_wp, dtype=np.int32).copy(),
                cur=np.ascontiguousarray(cur, dtype=np.int32).copy(), since=np.full((S, nc), fill, dtype=np.int32),
                wp_col=np.full((S, nc, W), fill, dtype=np.int32), pf=np.full((S, nc, 3), float(fill)), plan_status=np.full((S, nc), fill, dtype=np.int32),
                replan_count=np.full((S, nc), 3, dtype=np.int32), replan_col=np.full((S, nc), fill, dtype=np.int32))


def step_expected(state, obst, cell, margin, k, kw=KW, scene_done=None):
    """what one re-plan step on column k leaves of step_state's arrays, by the restatement; returns (dict, flagged [(s, i)])"""
    out = {key: state[key].copy() for key in STEP_KEYS}
    flagged = []
    for s in range(state["waypoints"].shape[0]):
        blocked = pl.blocked_grid(obst[s], kw["pmin"], kw["pmax"], cell, margin, kw["rmin"], kw["c"])
        done = scene_done is not None and scene_done[s]
        for i, w2, n2, st in replan_step(blocked, state["x_p"][s], state["goals"][s], state["waypoints"][s], state["n_wp"][s], state["cur"][s], kw["pmin"],
                                         cell, skip=done):
            out["waypoints"][s, i], out["n_wp"][s, i], out["plan_status"][s, i] = w2, n2, st
            out["cur"][s, i], out["since"][s, i], out["wp_col"][s, i], out["pf"][s, i] = 0, k, -1, w2[0]
            out["replan_count"][s, i] += 1
            out["replan_col"][s, i] = k
            flagged.append((s, i))
    return out, flagged


def device_step_call(d, state, obst, cell, margin, k, scene_done=None, stream=None, optional=True):
    """dmpc_replan_routes_device on step_state's arrays through torch tensors; returns the arrays afterwards (optional False: the optional ones
    are not passed and come back as they went)"""
    import torch
    dev = torch.device("cuda")
    t = {key: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for key, v in state.items()}
    tob = torch.from_numpy(_f(obst)).to(dev)
    tdone = torch.from_numpy(np.ascontiguousarray(scene_done, dtype=np.int32)).to(dev) if scene_done is not None else None
    S, nc, W = state["waypoints"].shape[:3]
    torch.cuda.synchronize()
    opt = lambda key: t[key].data_ptr() if optional else 0
    d.replan_routes_device(S, nc, tob.shape[1], W, t["x_p"].data_ptr(), t["goals"].data_ptr(), tob.data_ptr(), cell, margin, k, t["waypoints"].data_ptr(),
                           t["n_wp"].data_ptr(), t["cur"].data_ptr(), opt("since"), opt("wp_col"), opt("pf"), opt("plan_status"), opt("replan_count"),
                           opt("replan_col"), tdone.data_ptr() if tdone is not None else 0, stream.cuda_stream if stream is not None else 0)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return {key: t[key].cpu().numpy() for key in STEP_KEYS}


def same_step(out, ref, what=""):
    for key in STEP_KEYS:
        a, b = out[key], ref[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)[:4].tolist()
            raise AssertionError(f"{what}: {key} differs at {bad}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}")
