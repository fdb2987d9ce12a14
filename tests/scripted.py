"""Test helper: scenes with SCRIPTED vehicles -- uncommanded vehicles that follow a known path (dmpc_transition_scripted,
dmpc_scripted_cols_device, dmpc_postcheck_scripted) -- the oracle's closed loop over them, and raw ctypes calls of the three entries.

There is no reference counterpart (DMPC::solveParallelDMPCv2 freezes uncommanded vehicles).  The truth is the reference's own MPC step
(oracle.step) applied to a table whose uncommanded rows are rewritten before every step: at the step that produces history column k,
horizon entry kk of vehicle j is sample(j, k-1+kk), sample(j, t) = path[j][min(t, P-1)].

Scenes are built on obstacles.wall_scene / obstacles.KW: 8 commanded agents cross the plane x = 0, on which the 10 wall vehicles now move
along y at 0.5 m/s = 0.1 m per step, the two rows (z = 0.75, z = 1.65) in opposite directions.  The wall is 4 m wide in a 5 m workspace,
so a vehicle cannot run on for a whole transition: each one shuttles +-0.4 m about its place (a triangle wave of period 16 steps), which
keeps every sample inside the workspace.
  variant A   P = K_T_max + 13: the path outlasts every horizon window, the clamp is never hit
  variant B   P = 12: the vehicles stop mid-transition (at sample 11, 0.3 m past their place on the way back), every later window is clamped
  variant C   N_cmd = 1, M = 1, head-on: the vehicle flies the agent's line in the opposite direction, then rests where the agent started
"""
import functools

import numpy as np

import obstacles as ob
from obstacles import KW, ERROR_TOL, _dp, _ip, _f   # noqa: F401  (KW, ERROR_TOL: the scenes' solver parameters, re-exported)

KT = 100                # K_T_max of every scene here
STEP = 0.1              # m per MPC step: 0.5 m/s at h = 0.2 s
SWING = 4               # steps from the middle of a vehicle's shuttle to its turning point (0.4 m)
P_A, P_B, P_C = KT + 13, 12, 31
WALL_SHIFT = 0.002      # m along y per seed, from seed 1 on which the wall stands at obstacles.wall_scene's places: no two scenes of a batch share a
                        # path (seeds up to 35 stay inside the workspace: 2 + 0.4 + 0.07 < 2.5)


def sample(path, t):
    """sample(j, t) = path[j][min(t, P-1)] for all vehicles; path [M,P,3] -> [M,3]"""
    return path[:, min(int(t), path.shape[1] - 1)]


def window(path, k, shift=0):
    """table rows [M,45] of the scripted vehicles at the MPC step that produces history column k: entries sample(j, k-1+kk+shift), kk = 0..14
    (shift = 0 is the rule; shift = +1 is the off-by-one a window starting at column k would be)"""
    return np.stack([sample(path, k - 1 + kk + shift) for kk in range(15)], axis=1).reshape(path.shape[0], 45)


def _shuttle(t):
    """triangle wave of slope +-1 and amplitude SWING, 0 at t = 0 and rising first"""
    u = (np.asarray(t) + SWING) % (4 * SWING)
    return np.where(u <= 2 * SWING, u - SWING, 3 * SWING - u)


def wall_paths(start, P):
    """paths [M,P,3] of the wall vehicles from their places `start` [M,3]: along y, 0.1 m per step, the rows (z) in opposite directions"""
    t = np.arange(P)
    sign = np.where(start[:, 2] < 1.2, 1.0, -1.0)
    path = np.repeat(start[:, None, :], P, axis=1)
    path[:, :, 1] += sign[:, None] * STEP * _shuttle(t)[None, :]
    return path


def scene(variant, seed=0):
    """(po [N_cmd,3], pf [N_cmd,3], path [M,P,3]) of one scene"""
    if variant in ("A", "B"):
        po, pf = ob.wall_scene(8, seed)
        start = po[8:].copy()
        start[:, 1] += WALL_SHIFT * (seed - 1)                 # wall_scene jitters the commanded agents only: the wall itself differs by scene here
        return po[:8].copy(), pf, wall_paths(start, P_A if variant == "A" else P_B)
    assert variant == "C"
    po = np.array([[-1.5, 0.0 + 0.02 * seed, 1.2]])
    pf = np.array([[1.5, 0.0, 1.2]])
    x = np.maximum(1.5 - STEP * np.arange(P_C), -1.5)          # 30 steps from x = +1.5 to the agent's start, then at rest
    path = np.stack([x, np.full(P_C, 0.05), np.full(P_C, 1.25)], axis=1)[None]
    return po, pf, path


def pad_path(path, P):
    """the same motion as a longer array: the last sample repeated -- what the clamp says a path that has ended means"""
    extra = P - path.shape[-2]
    return path if extra <= 0 else np.concatenate([path, np.repeat(path[..., -1:, :], extra, axis=-2)], axis=-2)


# the seeds of the closed-loop tests, picked with the oracle on the CPU: with each of the four solver variants those tests use, at least one scene
# of every variant ends SOLVED | REACHED (tests/test_scripted_cpu.py asserts it); A/0 is a scene most solvers abort with a collision
SEEDS = {"A": (0, 1), "B": (0, 3), "C": (0,)}


def batch(variant, seeds=None):
    """(po [S,N_cmd,3], pf, path [S,M,P,3]) of the scenes scene(variant, seed)"""
    sc = [scene(variant, s) for s in (SEEDS[variant] if seeds is None else seeds)]
    return tuple(np.stack([x[i] for x in sc]) for i in range(3))


def mixed_batch(n):
    """n scenes of variants A and B alternating in ONE batch: the paths of B padded to P_A by their last sample"""
    sc = [scene("AB"[i % 2], i) for i in range(n)]
    return np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc]), np.stack([pad_path(x[2], P_A) for x in sc])


def oracle_loop_scripted(orc, prm, po, pf, path, K_T_max=KT, shift=0, error_tol=ERROR_TOL, nthreads=ob.NTHREADS):
    """obstacles.oracle_loop with the uncommanded rows set to window(path, k, shift) before the step that produces column k: po, pf [N_cmd,3],
    path [M,P,3].  The scripted vehicles' own outputs are discarded.  Returns dict(pk, vk, ak [N_cmd,K_T_max,3], K_T_used, scene_status,
    nrows [K_T_used-1, N_cmd])."""
    po, pf, path = np.asarray(po, float), np.asarray(pf, float), np.asarray(path, float)
    nc, M = po.shape[0], path.shape[0]
    l = np.zeros((nc + M, 45))
    l[:nc] = ob.init_table(po, pf)
    xp, xv, xa = po.copy(), np.zeros((nc, 3)), np.zeros((nc, 3))
    z = np.zeros((M, 3))
    pk, vk, ak = (np.zeros((nc, K_T_max, 3)) for _ in range(3))
    pk[:, 0] = po
    used, sst, nrows = K_T_max, 1, []
    if np.linalg.norm(po - pf, axis=1).max() < error_tol:
        return dict(pk=pk, vk=vk, ak=ak, K_T_used=1, scene_status=1 | 256, nrows=np.zeros((0, nc), int))
    for k in range(1, K_T_max):
        l[nc:] = window(path, k, shift)
        here = sample(path, k - 1)
        o = orc.step(prm, l, np.vstack([xp, here]), np.vstack([xv, z]), np.vstack([xa, z]), np.vstack([pf, here]), nthreads=nthreads)
        st = o["status"][:nc]
        nrows.append(o["info"][:nc, 7].copy())
        ok = (st & 1) == 1
        l[:nc][ok] = o["p"][:nc][ok]
        xp[ok], xv[ok], xa[ok] = o["p"][:nc, :3][ok], o["v"][:nc, :3][ok], o["a"][:nc, :3][ok]
        pk[:, k], vk[:, k], ak[:, k] = xp, xv, xa
        bits = int(np.bitwise_or.reduce(st))
        if bits & ~1:
            used, sst = k + 1, bits
            break
        if np.linalg.norm(xp - pf, axis=1).max() < error_tol:
            used, sst = k + 1, 1 | 256
            break
    return dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, nrows=np.array(nrows))


@functools.lru_cache(maxsize=None)
def oracle_result(solver, variant, seed, shift=0, frozen=False):
    """the oracle's closed loop on scene(variant, seed), computed once per session (shared by the tests: do not modify);
    frozen: the vehicles stay at their starts (P = 1)"""
    from oracle import oracle as orc
    po, pf, path = scene(variant, seed)
    return oracle_loop_scripted(orc, orc.make_params(solver, **KW), po, pf, path[:, :1] if frozen else path, shift=shift)


@functools.lru_cache(maxsize=None)
def oracle_min_dist_scripted(solver, variant, seed):
    """the smallest |E1 (p_i(t) - q_j(t))| at 100 Hz of the oracle's closed loop on scene(variant, seed): oracle/postcheck.py on the commanded
    histories, scipy's not-a-knot spline through sample(j, i) on the same knots.  None unless the loop ended SOLVED | REACHED."""
    from scipy.interpolate import CubicSpline
    from oracle import postcheck as PC
    r = oracle_result(solver, variant, seed)
    if r["scene_status"] != (1 | 256):
        return None
    _, pf, path = scene(variant, seed)
    u = r["K_T_used"]
    o = PC.postcheck(r["pk"][:, :u], r["vk"][:, :u], r["ak"][:, :u], pf, KW["h"], KW["rmin"], KW["c"])
    tk, t = PC.sample_times(u, o["h_scaled"])
    knots = np.stack([sample(path, i) for i in range(u)], axis=1)
    q = np.stack([CubicSpline(tk, knots[j], axis=0, bc_type="not-a-knot")(t) for j in range(path.shape[0])])
    e1 = np.array([1.0, 1.0, 1.0 / KW["c"]])
    return float(np.sqrt((((o["p"][:, None] - q[None]) * e1) ** 2).sum(-1)).min())


# ---- raw calls of the three entries --------------------------------------------------------------------------------------------------
def raw_transition_scripted(d, po, pf, path, K_T_max=KT, error_tol=ERROR_TOL, M=None, P=None, n_cmd=None, histories=(1, 1, 1)):
    """dmpc_transition_scripted on po, pf [S,N_cmd,3], path [S,M,P,3] (None: a NULL pointer; M, P, n_cmd override the shapes; histories: which
    of pk, vk, ak are passed); returns (rc, dict)"""
    po, pf = _f(po), _f(pf)
    S, nc = po.shape[0], po.shape[1]
    path = _f(path) if path is not None else None
    M = (path.shape[1] if path is not None else 1) if M is None else M
    P = (path.shape[2] if path is not None else 1) if P is None else P
    pk, vk, ak = (np.zeros((S, nc, K_T_max, 3)) for _ in range(3))
    used, sst = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    hp = [_dp(a if on else None) for a, on in zip((pk, vk, ak), histories)]
    rc = d._L.dmpc_transition_scripted(d._ctx, S, nc if n_cmd is None else n_cmd, M, P, _dp(po), _dp(pf), _dp(path), int(K_T_max), float(error_tol),
                                       hp[0], hp[1], hp[2], _ip(used), _ip(sst))
    return rc, dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst)


def raw_postcheck_scripted(d, K_T_used, pk, vk, ak, pf, path, vmax=2.0, amax=1.0, Ts=0.01, ns_alloc=0, M=None, P=None):
    """dmpc_postcheck_scripted on [S,N_cmd,KT,3] histories (pk an int: the resident ones, pk = KT_alloc), path [S,M,P,3]; returns (rc, dict)"""
    pf = _f(pf)
    S, nc = pf.shape[0], pf.shape[1]
    used = np.ascontiguousarray(K_T_used, dtype=np.int32)
    if isinstance(pk, int):
        KTa, pk, vk, ak = pk, None, None, None
    else:
        pk, vk, ak = _f(pk), _f(vk), _f(ak)
        KTa = pk.shape[2]
    path = _f(path) if path is not None else None
    M = (path.shape[1] if path is not None else 1) if M is None else M
    P = (path.shape[2] if path is not None else 1) if P is None else P
    out = dict(r_factor=np.zeros(S), h_scaled=np.zeros(S), n_samples=np.zeros(S, dtype=np.int32), min_dist=np.zeros(S),
               violation=np.zeros(S, dtype=np.int32), totdist=np.zeros(S), traj_time=np.zeros(S), min_dist_scripted=np.zeros(S),
               violation_scripted=np.zeros(S, dtype=np.int32))
    p_i = np.zeros((S, nc, ns_alloc, 3)) if ns_alloc else None
    p_s = np.zeros((S, max(M, 1), ns_alloc, 3)) if ns_alloc else None
    rc = d._L.dmpc_postcheck_scripted(d._ctx, S, nc + M, nc, KTa, _ip(used), _ip(None), _dp(pk), _dp(vk), _dp(ak), _dp(pf), _dp(path), P,
                                      float(vmax), float(amax), float(Ts), _dp(out["r_factor"]), _dp(out["h_scaled"]), _ip(out["n_samples"]),
                                      _dp(out["min_dist"]), _ip(out["violation"]), _dp(out["totdist"]), _dp(out["traj_time"]), _dp(p_i), int(ns_alloc),
                                      _dp(out["min_dist_scripted"]), _ip(out["violation_scripted"]), _dp(p_s))
    if p_i is not None:
        out["p"], out["p_scripted"] = p_i, p_s
    return rc, out
