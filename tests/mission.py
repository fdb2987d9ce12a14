"""Test helper: missions -- a transition through a sequence of goal sets (dmpc_transition_mission) -- the stage rule as a Python loop over an
MPC step, the scenes the GPU tests use, and a raw ctypes call of the entry.

There is no reference counterpart (the reference flies one leg).  The truth is the reference's own MPC step (oracle.step) in the loop a caller
could write on the host (mission_loop):
  stage 0 starts at history column 0 (the initDMPC column, straight lines from po to goals[0]);
  a stage q < Q-1 ends at the first column k where goals[q] are reached on column k, or deadline[q] > 0 and k - k_start(q) >= deadline[q];
  then stage_col[q] = k, k_start(q+1) = k, and the step that produces column k+1 is the first one solved with goals[q+1]; the table is left alone;
  at most one stage ends per column; the last stage reached ends the trial; a failed agent stops the scene in whatever stage.

Scenes: four commanded agents on the corners of a square of side 0.7 m (z = 1.2) that turn a quarter at a time -- every leg is 0.7 m along an edge,
24 columns -- alone, next to two static vehicles, or next to two scripted ones that cross above and below the square.  The scene that
fails is scripted.scene("A", 0), the wall crossing most solvers abort with a collision.
"""
import functools

import numpy as np

import obstacles as ob
import scripted as sc
from obstacles import KW, _dp, _ip, _f   # noqa: F401  (KW: the scenes' solver parameters, re-exported)

KT = 80                 # K_T_max of every mission here: the columns of the whole mission
ERROR_TOL = 0.1         # m: a formation counts as reached -- passed through -- within 10 cm; the last centimetres of a leg are the slow ones (a 0.6 m leg
                        # takes 23 columns to 0.1 m and 34 to 0.01 m), and three legs have to fit K_T_max = 80
SPEED_FLOOR = 0.2       # m/s: the deadline scene must switch at least once while some agent is faster than this (a tenth of the 2 m/s the post-check
                        # allows, twenty times what an agent within error_tol of its goal still does)
REACHED = 1 | 256


def square(turn, jitter=0.0, seed=0):
    """the four corners of the square, turned by `turn` quarters: agent i stands on corner i + turn; [4,3]"""
    c = np.array([(-0.35, -0.35, 1.2), (0.35, -0.35, 1.2), (0.35, 0.35, 1.2), (-0.35, 0.35, 1.2)])
    out = np.roll(c, -turn, axis=0)
    if jitter:
        out = out + np.random.default_rng(4000 + 10 * seed + turn).uniform(-jitter, jitter, out.shape)
    return out


STATIC = np.array([(0.0, -0.68, 1.2), (0.68, 0.0, 1.2)])      # two vehicles that rest beside two edges of the square, 0.33 m < rmin from the agents' lines


def crossing_paths(P=KT + 14, seed=0):
    """two scripted vehicles [2,P,3] that shuttle along x just above and just below the square, 0.05 m per step, outside the edges y = -+0.35"""
    t = np.arange(P)
    x = -1.0 + 0.05 * np.abs((t + 7 * seed) % 80 - 40)
    return np.stack([np.stack([x, np.full(P, 0.65), np.full(P, 1.4)], axis=1), np.stack([-x, np.full(P, -0.65), np.full(P, 1.0)], axis=1)])


def scene(name, seed=0):
    """dict(po [N,3] (with a path: [N_cmd,3]), goals [Q,N_cmd,3], deadline [Q] or None, path [M,P,3] or None) of one scene:
      reached     Q = 3, every stage ends because it is reached
      static      the same next to two static vehicles (po has six rows)
      path        the same next to two scripted vehicles
      deadline    Q = 3 on a square of side 1 m, the first two stages end on their deadlines (8 and 10 columns), in flight
      column0     po == goals[0]: the first stage is reached on the initDMPC column
      coincident  goals[1] == goals[0]: two stages end on consecutive columns
      failure     scripted.scene("A", 0) (8 agents, 10 scripted vehicles): a third of the way for 5 columns, then the far side, then back: an agent
                  collides in stage 1 of 3
    """
    j = 0.02
    po = square(0, j, seed)
    g = np.stack([square(1, j, seed), square(2, j, seed), square(3, j, seed)])
    out = dict(po=po, goals=g, deadline=None, path=None)
    if name == "reached":
        pass
    elif name == "static":
        out["po"] = np.vstack([po, STATIC])
    elif name == "path":
        out["path"] = crossing_paths(seed=seed)
    elif name == "deadline":
        grow = np.array([1.0 / 0.7, 1.0 / 0.7, 1.0])      # legs of 1 m: eight columns into one an agent flies at a quarter of a metre per second
        out = dict(po=po * grow, goals=g * grow, deadline=np.array([8, 10, 0], dtype=np.int32), path=None)
    elif name == "column0":
        out["goals"] = np.stack([po, g[0], g[1]])
    elif name == "coincident":
        out["goals"] = np.stack([g[0], g[0], g[1]])
    elif name == "failure":
        wpo, wpf, wpath = sc.scene("A", seed)
        out = dict(po=wpo, goals=np.stack([wpo + 0.2 * (wpf - wpo), wpf, wpo]), deadline=np.array([5, 0, 0], dtype=np.int32), path=wpath)
    else:
        raise KeyError(name)
    return out


SCENES = ("reached", "static", "path", "deadline", "column0", "coincident", "failure")


def reached_goal(xp, pf, error_tol):
    """ReachedGoal as the post step evaluates it: max_i sqrt(dx^2 + dy^2 + dz^2) < error_tol"""
    d = xp - pf
    return bool(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).max() < error_tol)


def mission_loop(step, po, goals, deadline=None, path=None, K_T_max=KT, error_tol=ERROR_TOL):
    """The stage rule as a host loop.  step(l [N,45], xp, xv, xa [nc,3], pf [nc,3], here [M,3]) -> (p, v, a [nc,45], status [nc]) is one MPC
    step of the nc commanded agents on the N-row table.  po [N,3] (with a path: [nc,3]), goals [Q,nc,3].  Returns dict(pk, vk, ak [nc,K_T_max,3],
    K_T_used, scene_status, stage_col [Q], switch_speed: the largest |v| of any agent on every column where a stage q < Q-1 ended)."""
    po, goals = np.asarray(po, float), np.asarray(goals, float)
    Q, nc = goals.shape[0], goals.shape[1]
    dl = np.zeros(Q, dtype=int) if deadline is None else np.asarray(deadline, dtype=int)
    M = path.shape[0] if path is not None else po.shape[0] - nc
    l = np.zeros((nc + M, 45))
    l[:nc] = ob.init_table(po[:nc], goals[0])
    xp, xv, xa = po[:nc].copy(), np.zeros((nc, 3)), np.zeros((nc, 3))
    pk, vk, ak = (np.zeros((nc, K_T_max, 3)) for _ in range(3))
    pk[:, 0] = xp
    stage, k0, col, speeds = 0, 0, np.full(Q, -1, dtype=np.int32), []
    used, sst = K_T_max, 1

    def rule(k, bits):
        """the verdict of column k; True: the trial is over"""
        nonlocal stage, k0, used, sst
        if bits & ~1:
            used, sst = k + 1, bits
            return True
        hit = reached_goal(xp, goals[stage], error_tol)
        if stage == Q - 1:
            if hit:
                col[stage] = k
                used, sst = k + 1, REACHED
            return hit
        if hit or (dl[stage] > 0 and k - k0 >= dl[stage]):
            col[stage] = k
            speeds.append(float(np.linalg.norm(xv, axis=1).max()))
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
        ok = (st & 1) == 1
        l[:nc][ok] = p[ok]
        xp[ok], xv[ok], xa[ok] = p[ok, :3], v[ok, :3], a[ok, :3]
        pk[:, k], vk[:, k], ak[:, k] = xp, xv, xa
        over = rule(k, int(np.bitwise_or.reduce(st)))
    return dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, stage_col=col, switch_speed=speeds)


def oracle_step(orc, prm, nthreads=ob.NTHREADS):
    """mission_loop's step over oracle.step: the uncommanded vehicles are rows of the table with themselves as goals, their outputs are discarded"""
    def step(l, xp, xv, xa, pf, here):
        nc, z = xp.shape[0], np.zeros_like(here)
        o = orc.step(prm, l, np.vstack([xp, here]), np.vstack([xv, z]), np.vstack([xa, z]), np.vstack([pf, here]), nthreads=nthreads)
        return o["p"][:nc], o["v"][:nc], o["a"][:nc], o["status"][:nc]
    return step


def device_step(d):
    """mission_loop's step over dmpc_step_batch (every vehicle commanded) / dmpc_step_batch_cmd, one scene at a time"""
    def step(l, xp, xv, xa, pf, here):
        if here.shape[0] == 0:
            o = d.step_batch(l, xp, xv, xa, pf)
        else:
            rc, o = ob.raw_step_batch_cmd(d, l[None], xp[None], xv[None], xa[None], pf[None], xp.shape[0])
            assert rc == 0
            o = {k: o[k][0] for k in o}
        return o["p"], o["v"], o["a"], o["status"]
    return step


@functools.lru_cache(maxsize=None)
def oracle_result(solver, name, seed=0):
    """the oracle's mission loop on scene(name, seed), computed once per session (shared by the tests: do not modify)"""
    from oracle import oracle as orc
    s = scene(name, seed)
    return mission_loop(oracle_step(orc, orc.make_params(solver, **KW)), s["po"], s["goals"], s["deadline"], s["path"])


def batch(names, seeds=None):
    """the scenes scene(name, seed) of one shape as one batch: dict(po [S,..], goals [S,Q,nc,3], deadline [S,Q] (zeros where a scene has none),
    path [S,M,P,3] or None)"""
    seeds = [0] * len(names) if seeds is None else seeds
    sc_ = [scene(n, s) for n, s in zip(names, seeds)]
    Q = sc_[0]["goals"].shape[0]
    dl = np.stack([x["deadline"] if x["deadline"] is not None else np.zeros(Q, dtype=np.int32) for x in sc_]).astype(np.int32)
    path = np.stack([x["path"] for x in sc_]) if sc_[0]["path"] is not None else None
    return dict(po=np.stack([x["po"] for x in sc_]), goals=np.stack([x["goals"] for x in sc_]), deadline=dl, path=path)


# ---- raw call of the entry ------------------------------------------------------------------------------------------------------------
def raw_mission(d, po, goals, deadline=None, path=None, K_T_max=KT, error_tol=ERROR_TOL, Q=None, n_cmd=None, P=None, histories=(1, 1, 1),
                stage_col=True):
    """dmpc_transition_mission on po [S,N,3] (with a path [S,M,P,3]: [S,N_cmd,3]), goals [S,Q,N_cmd,3] (None: a NULL pointer; then Q and n_cmd
    must be given), deadline [S,Q] or None; Q, n_cmd, P override the shapes; histories: which of pk, vk, ak are passed.  Returns (rc, dict)."""
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
    hp = [_dp(a if on else None) for a, on in zip((pk, vk, ak), histories)]
    rc = d._L.dmpc_transition_mission(d._ctx, S, N, nc, Q, _dp(po), _dp(goals), _ip(deadline), _dp(path), P, int(K_T_max), float(error_tol),
                                      hp[0], hp[1], hp[2], _ip(used), _ip(sst), _ip(col if stage_col else None))
    return rc, dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, stage_col=col)
