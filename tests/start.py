"""Test helper: start in motion (dmpc_set_start) -- a flight whose column 0 is a given or carried state and plan instead of initDMPC -- the braking
plan in numpy, the one-leg loop from such a start over an MPC step, the head-on scene, and raw ctypes calls of the four entries.

There is no reference counterpart (the reference flies one leg from rest).  The truth is the reference's own MPC step (oracle.step) in the loop a
caller could write on the host (start_loop): column 0 is (x_p, x_v, x_a), the commanded rows of the first table are plan_p, and everything behind
column 0 is dmpc_transition's loop.  A flight cut at column c and continued from its end -- state and plan of the step that produced column c --
is the same sequence of steps, so it gives columns c .. of the whole flight bit for bit."""
import ctypes as C

import numpy as np

import mission as mi
import obstacles as ob
from multiagent_planning_amd import _lib
from obstacles import KW, _dp, _ip, _f   # noqa: F401

K = 15
ERROR_TOL = mi.ERROR_TOL   # 0.1 m, as the missions: the fleet is retasked when it has passed through a formation, not when it has settled there
REACHED = 1 | 256
KT = 60                 # K_T_max of the head-on flights


def brake_plan(x_p, x_v, x_a, h=KW["h"], alim=KW["alim"]):
    """the braking plan of include/dmpc_hip.h for states [..,3] -> (p, v, a) [..,45], written operation by operation: numpy rounds each of them on
    its own, as the device does (no fused multiply-add)"""
    x_p, x_v, x_a = (np.asarray(x, float) for x in (x_p, x_v, x_a))
    p, v, a = (np.empty(x_p.shape[:-1] + (3 * K,)) for _ in range(3))
    pk, vk, ak = x_p.copy(), x_v.copy(), x_a.copy()
    c = 0.5 * h
    c = c * h
    for kk in range(K):
        if kk:
            q = -vk
            q = q / h
            ak = np.minimum(np.maximum(q, -alim), alim)
            hv = h * vk
            ha = h * ak
            ca = c * ak
            s = pk + hv
            pk = s + ca
            vk = vk + ha
        p[..., 3 * kk:3 * kk + 3], v[..., 3 * kk:3 * kk + 3], a[..., 3 * kk:3 * kk + 3] = pk, vk, ak
    return p, v, a


def head_on():
    """two agents that fly at each other, (-1, 0, 1.2) <-> (1, 0.01, 1.2): each to the other's x on its own y, one centimetre apart; po, pf [2,3]"""
    po = np.array([(-1.0, 0.0, 1.2), (1.0, 0.01, 1.2)])
    return po, po * [-1.0, 1.0, 1.0]


def start_loop(step, x_p, x_v, x_a, plan_p, pf, K_T_max, error_tol=ERROR_TOL, static=None, plan_v=None, plan_a=None):
    """One leg from a start, as a host loop.  step: mission.oracle_step / mission.device_step.  x_p, x_v, x_a [nc,3], plan_p [nc,45], pf [nc,3];
    static [M,3]: uncommanded vehicles behind the commanded ones.  Returns dict(pk, vk, ak [nc,K_T_max,3], K_T_used, scene_status, and the end:
    x_p, x_v, x_a [nc,3], plan_p, plan_v, plan_a [nc,45] -- the plan of the step that produced the last column; none ran: the start's)."""
    xp, xv, xa = (np.array(x, float) for x in (x_p, x_v, x_a))
    nc = xp.shape[0]
    static = np.zeros((0, 3)) if static is None else np.asarray(static, float)
    l = np.zeros((nc + static.shape[0], 45))
    l[:nc] = plan_p
    l[nc:] = np.tile(static, (1, K))
    P = np.array(plan_p, float)
    V = np.zeros((nc, 45)) if plan_v is None else np.array(plan_v, float)
    A = np.zeros((nc, 45)) if plan_a is None else np.array(plan_a, float)
    pk, vk, ak = (np.zeros((nc, K_T_max, 3)) for _ in range(3))
    pk[:, 0], vk[:, 0], ak[:, 0] = xp, xv, xa
    used, sst = K_T_max, 1
    if mi.reached_goal(xp, pf, error_tol):
        used, sst = 1, REACHED
    else:
        for k in range(1, K_T_max):
            p, v, a, st = step(l, xp, xv, xa, pf, static)
            ok = (st & 1) == 1
            l[:nc][ok] = p[ok]
            xp[ok], xv[ok], xa[ok] = p[ok, :3], v[ok, :3], a[ok, :3]
            P[ok], V[ok], A[ok] = p[ok], v[ok], a[ok]
            pk[:, k], vk[:, k], ak[:, k] = xp, xv, xa
            bits = int(np.bitwise_or.reduce(st))
            if bits & ~1:
                used, sst = k + 1, bits
                break
            if mi.reached_goal(xp, pf, error_tol):
                used, sst = k + 1, REACHED
                break
    return dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, x_p=xp, x_v=xv, x_a=xa, plan_p=P, plan_v=V, plan_a=A)


def rest_loop(step, po, pf, K_T_max, error_tol=ERROR_TOL):
    """dmpc_transition's loop (every vehicle commanded) as start_loop from rest on the initDMPC table"""
    z = np.zeros_like(po)
    return start_loop(step, po, z, z, ob.init_table(po, pf), pf, K_T_max, error_tol)


def continue_loop(step, end, pf, K_T_max, error_tol=ERROR_TOL):
    """start_loop from the end of another start_loop"""
    return start_loop(step, end["x_p"], end["x_v"], end["x_a"], end["plan_p"], pf, K_T_max, error_tol, plan_v=end["plan_v"], plan_a=end["plan_a"])


# ---- raw calls of the entries ---------------------------------------------------------------------------------------------------------------
def raw_set_start(d, S, n_cmd, vo=None, ao=None, plan_p=None, plan_v=None, plan_a=None, col0=0, from_end=0, src_scene=None, ctx="own"):
    """dmpc_set_start with exactly these fields (arrays as given, None: NULL); returns rc"""
    keep = [_f(a) if a is not None else None for a in (vo, ao, plan_p, plan_v, plan_a)]
    src = np.ascontiguousarray(src_scene, dtype=np.int32) if src_scene is not None else None
    s = _lib.DmpcStart(int(S), int(n_cmd), int(from_end), _ip(src), *[_dp(a) for a in keep], int(col0))
    return d._L.dmpc_set_start(d._ctx if ctx == "own" else ctx, C.byref(s))


def raw_flight_end(d, S, n_cmd, outputs=(1,) * 7, ctx="own"):
    """dmpc_flight_end; outputs: which of x_p, x_v, x_a, plan_p, plan_v, plan_a, col are passed.  Returns (rc, dict)."""
    m, s = max(n_cmd, 1), max(S, 1)
    o = dict(x_p=np.zeros((s, m, 3)), x_v=np.zeros((s, m, 3)), x_a=np.zeros((s, m, 3)), plan_p=np.zeros((s, m, 45)), plan_v=np.zeros((s, m, 45)),
             plan_a=np.zeros((s, m, 45)), col=np.zeros(s, dtype=np.int32))
    ptr = [(_ip if k == "col" else _dp)(o[k] if on else None) for k, on in zip(o, outputs)]
    rc = d._L.dmpc_flight_end(d._ctx if ctx == "own" else ctx, int(S), int(n_cmd), *ptr)
    return rc, o


def raw_start_plan(d, x_p, x_v, x_a, n=None, prm="own"):
    """dmpc_start_plan on states [n,3]; returns (rc, (p, v, a) [n,45])"""
    x_p, x_v, x_a = _f(x_p), _f(x_v), _f(x_a)
    n = x_p.shape[0] if n is None else n
    out = [np.zeros((max(n, 1), 45)) for _ in range(3)]
    rc = d._L.dmpc_start_plan(C.byref(d.prm) if prm == "own" else prm, int(n), _dp(x_p), _dp(x_v), _dp(x_a), *[_dp(a) for a in out])
    return rc, tuple(out)
