"""Test helper: the hold policy (dmpc_transition_hold) -- an agent whose solve failed flies its previous plan while the scene goes on -- as a
Python loop over an MPC step, the scenes the tests use, and a raw ctypes call of the entry.

There is no reference counterpart (the reference's failure-rate experiment stops the trial at the first failed agent).  The truth is the
reference's own MPC step (oracle.step) in mission.mission_loop with one rule added behind every step (hold_loop), per commanded agent:
  fail   the status is not exactly SOLVED (= 1): the predicate that stops a scene in every other loop;
  run    the consecutive columns up to and including this one on which the agent failed;
  held   fail and run <= max_hold: the plan of this step is the previous plan (of step k-1, solved or held; for k = 1 the initDMPC plan:
         straight-line positions, v = a = 0) shifted by one entry, with the braking tail of `shift_plan` as its last entry.  The held plan is a
         solved one from there on: table row, state, history column, scene verdict, ReachedGoal, stage rule;
  over   fail and run > max_hold: the column ends the scene as in mission_loop, with the OR of the raw bits.
"""
import numpy as np

import mission as mi
import obstacles as ob
import scripted as sc
from obstacles import KW, _dp, _ip, _f   # noqa: F401

HELD = 64
REACHED = 1 | 256
MAX_HOLD = 14           # the default budget of Dmpc.transition(on_fail="hold"): a whole horizon less one entry
KT = sc.KT              # K_T_max of every scene here (100)
ERROR_TOL = ob.ERROR_TOL


def shift_plan(p, v, a, h=KW["h"], alim=KW["alim"]):
    """the held plan of rows p, v, a [n,45]: entries 1 .. K-1 moved to 0 .. K-2 (copies), and the braking tail as entry K-1 -- written operation by
    operation: numpy rounds each of them on its own, as the device does (no fused multiply-add)"""
    p, v, a = np.asarray(p, float), np.asarray(v, float), np.asarray(a, float)
    pn, vn, an = np.empty_like(p), np.empty_like(v), np.empty_like(a)
    pn[:, :42], vn[:, :42], an[:, :42] = p[:, 3:], v[:, 3:], a[:, 3:]
    pl, vl = p[:, 42:], v[:, 42:]
    q = -vl
    q = q / h
    a_t = np.minimum(np.maximum(q, -alim), alim)
    hv = h * vl
    ha = h * a_t
    c = 0.5 * h
    c = c * h
    ca = c * a_t
    s = pl + hv
    an[:, 42:] = a_t
    vn[:, 42:] = vl + ha
    pn[:, 42:] = s + ca
    return pn, vn, an


def hold_loop(step, po, goals, deadline=None, path=None, K_T_max=KT, error_tol=ERROR_TOL, max_hold=MAX_HOLD, h=KW["h"], alim=KW["alim"]):
    """mission.mission_loop with the hold rule: same arguments (goals [Q,nc,3]; one leg: goals = pf[None]), same `step`.  Returns its dict (pk, vk, ak,
    K_T_used, scene_status -- with HELD --, stage_col) and hold_count, hold_first [nc], agent_status [nc,K_T_max], log: [(column, agent, raw status)]
    of every hold in order."""
    po, goals = np.asarray(po, float), np.asarray(goals, float)
    Q, nc = goals.shape[0], goals.shape[1]
    dl = np.zeros(Q, dtype=int) if deadline is None else np.asarray(deadline, dtype=int)
    M = path.shape[0] if path is not None else po.shape[0] - nc
    l = np.zeros((nc + M, 45))
    l[:nc] = ob.init_table(po[:nc], goals[0])
    xp, xv, xa = po[:nc].copy(), np.zeros((nc, 3)), np.zeros((nc, 3))
    pk, vk, ak = (np.zeros((nc, K_T_max, 3)) for _ in range(3))
    pk[:, 0] = xp
    stage, k0, col = 0, 0, np.full(Q, -1, dtype=np.int32)
    used, sst = K_T_max, 1
    P, V, A = l[:nc].copy(), np.zeros((nc, 45)), np.zeros((nc, 45))   # the previous plan of every agent: initDMPC's
    run = np.zeros(nc, dtype=int)
    cnt, first = np.zeros(nc, dtype=np.int32), np.full(nc, -1, dtype=np.int32)
    ast = np.zeros((nc, K_T_max), dtype=np.int32)
    ast[:, 0] = 1
    log = []

    def rule(k, bits):
        """the verdict of column k; True: the trial is over"""
        nonlocal stage, k0, used, sst
        if bits & ~1:
            used, sst = k + 1, bits
            return True
        hit = mi.reached_goal(xp, goals[stage], error_tol)
        if stage == Q - 1:
            if hit:
                col[stage] = k
                used, sst = k + 1, REACHED
            return hit
        if hit or (dl[stage] > 0 and k - k0 >= dl[stage]):
            col[stage] = k
            stage, k0 = stage + 1, k
        return False

    over = rule(0, 1)
    for k in range(1, K_T_max):
        if over:
            break
        if M:
            l[nc:] = sc.window(path, k) if path is not None else np.tile(po[nc:], (1, 15))
        here = (sc.sample(path, k - 1) if path is not None else po[nc:]) if M else np.zeros((0, 3))
        p, v, a, st = step(l, xp, xv, xa, goals[stage], here)
        p, v, a, st = p.copy(), v.copy(), a.copy(), np.asarray(st).astype(np.int32)
        fail = st != 1
        run = np.where(fail, run + 1, 0)
        held = fail & (run <= max_hold)
        ast[:, k] = np.where(held, st | HELD, st)
        if held.any():
            p[held], v[held], a[held] = shift_plan(P[held], V[held], A[held], h, alim)
            cnt[held] += 1
            first[held & (first < 0)] = k
            log += [(k, int(i), int(st[i])) for i in np.nonzero(held)[0]]
        eff = np.where(held, 1, st)
        ok = (eff & 1) == 1
        l[:nc][ok] = p[ok]
        xp[ok], xv[ok], xa[ok] = p[ok, :3], v[ok, :3], a[ok, :3]
        P[ok], V[ok], A[ok] = p[ok], v[ok], a[ok]
        pk[:, k], vk[:, k], ak[:, k] = xp, xv, xa
        over = rule(k, int(np.bitwise_or.reduce(eff)))
    if cnt.any():
        sst |= HELD
    return dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, stage_col=col, hold_count=cnt, hold_first=first, agent_status=ast, log=log)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def scene(kind, seed):
    """dict(po, goals [1,nc,3], deadline None, path) of a one-leg scene: kind "A" / "B" = scripted.scene (moving wall), "wall" = obstacles.wall_scene
    (static wall), 8 commanded agents and 10 vehicles each"""
    if kind in ("A", "B"):
        po, pf, path = sc.scene(kind, seed)
        return dict(po=po, goals=pf[None], deadline=None, path=path)
    assert kind == "wall"
    po, pf = ob.wall_scene(8, seed)
    return dict(po=po, goals=pf[None], deadline=None, path=None)


# the four failing rows of the issue's table: (solver, kind, seed)
FAILING = (("hard", "A", 0), ("ondemand", "wall", 1), ("bound", "A", 0), ("bound2", "A", 2))
# bound flies these without a failure
CLEAN = tuple(("B", s) for s in (0, 1, 2)) + tuple(("wall", s) for s in (0, 1, 2))


def batch(scenes, P=sc.P_A):
    """scenes [(kind, seed)] of kinds A / B (paths padded to P samples), or all of kind wall, as one batch: dict(po, goals [S,1,nc,3], path or None)"""
    s_ = [scene(k, s) for k, s in scenes]
    path = np.stack([sc.pad_path(x["path"], P) for x in s_]) if s_[0]["path"] is not None else None
    return dict(po=np.stack([x["po"] for x in s_]), goals=np.stack([x["goals"] for x in s_]), path=path)


_oracle_cache = {}


def oracle_result(solver, kind, seed, max_hold=MAX_HOLD, K_T_max=KT):
    """the oracle's hold loop on scene(kind, seed), computed once per session (shared by the tests: do not modify)"""
    key = (solver, kind, seed, max_hold, K_T_max)
    if key not in _oracle_cache:
        from oracle import oracle as orc
        s = scene(kind, seed)
        _oracle_cache[key] = hold_loop(mi.oracle_step(orc, orc.make_params(solver, **KW)), s["po"], s["goals"], None, s["path"], K_T_max=K_T_max,
                                       max_hold=max_hold)
    return _oracle_cache[key]


# ---- raw call of the entry ------------------------------------------------------------------------------------------------------------------
def raw_hold(d, po, goals, deadline=None, path=None, K_T_max=KT, error_tol=ERROR_TOL, max_hold=MAX_HOLD, Q=None, n_cmd=None, P=None, histories=(1, 1, 1),
             outputs=(1, 1, 1)):
    """dmpc_transition_hold on po [S,N,3] (with a path [S,M,P,3]: [S,N_cmd,3]), goals [S,Q,N_cmd,3] (None: a NULL pointer; then Q and n_cmd must be
    given), deadline [S,Q] or None; Q, n_cmd, P override the shapes; histories: which of pk, vk, ak are passed; outputs: which of hold_count,
    hold_first, agent_status.  Returns (rc, dict)."""
    po = _f(po)
    goals = _f(goals) if goals is not None else None
    S = po.shape[0]
    Q = goals.shape[1] if Q is None else Q
    nc = goals.shape[2] if n_cmd is None else n_cmd
    path = _f(path) if path is not None else None
    N = po.shape[1] + (path.shape[1] if path is not None else 0)
    P = (path.shape[2] if path is not None else 0) if P is None else P
    deadline = np.ascontiguousarray(deadline, dtype=np.int32) if deadline is not None else None
    m, q = max(nc, 1), max(Q, 1)
    pk, vk, ak = (np.zeros((S, m, K_T_max, 3)) for _ in range(3))
    used, sst, col = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32), np.zeros((S, q), dtype=np.int32)
    cnt, first, ast = np.zeros((S, m), dtype=np.int32), np.zeros((S, m), dtype=np.int32), np.zeros((S, m, K_T_max), dtype=np.int32)
    hp = [_dp(a if on else None) for a, on in zip((pk, vk, ak), histories)]
    op = [_ip(a if on else None) for a, on in zip((cnt, first, ast), outputs)]
    rc = d._L.dmpc_transition_hold(d._ctx, S, N, nc, Q, _dp(po), _dp(goals), _ip(deadline), _dp(path), P, int(K_T_max), float(error_tol), int(max_hold),
                                   hp[0], hp[1], hp[2], _ip(used), _ip(sst), _ip(col), op[0], op[1], op[2])
    return rc, dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, stage_col=col, hold_count=cnt, hold_first=first, agent_status=ast)


OUTPUTS = ("pk", "vk", "ak", "K_T_used", "scene_status", "stage_col", "hold_count", "hold_first", "agent_status")
