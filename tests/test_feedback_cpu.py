"""CPU: event-triggered feedback (dmpc_set_feedback) on the host -- the entries and their refusals, dmpc_feedback_apply_host (no context, no GPU)
against the numpy restatement of tests/feedback.py byte for byte, and the conditions of the head-on scene that the GPU tests
(tests/test_gpu_feedback.py) rely on, by the oracle's MPC step in the restated loop."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import disturb as di
import feedback as fb
import obstacles as ob
import start as stt
from helpers import ROOT
from multiagent_planning_amd import _lib

H = ob.KW["h"]
INF = float("inf")
NAMES = ("dmpc_set_feedback", "dmpc_feedback_device", "dmpc_feedback_apply_host", "dmpc_feedback_log")
OUT = ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "event", "lT_next", "v_rows")


# ---- 1. the entries -------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()
    for name, nargs in zip(NAMES, (2, 20, 21, 14)):
        assert re.search(r"DMPC_API int " + name + r"\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == nargs, name
    for method in ("set_feedback", "clear_feedback", "feedback_log", "feedback_device"):
        assert callable(getattr(_lib.Dmpc, method)), method
    assert callable(_lib.feedback_apply)


def test_struct_layout_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()
    body = re.search(r"typedef struct dmpc_feedback \{(.*?)\} dmpc_feedback;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("trigger_p", "double"), ("trigger_v", "double"), ("reanchor", "int32_t")]
    ct = {"double": C.c_double, "int32_t": C.c_int32}
    assert [(n, t) for n, t in _lib.DmpcFeedback._fields_] == [(n, ct[t]) for n, t in fields]
    assert (_lib.DmpcFeedback.trigger_p.offset, _lib.DmpcFeedback.trigger_v.offset, _lib.DmpcFeedback.reanchor.offset) == (0, 8, 16)
    assert C.sizeof(_lib.DmpcFeedback) == 24


def test_a_null_context_is_refused_by_name():
    L = _lib.load()
    f = _lib.DmpcFeedback(0.0, 0.0, 0)
    z = C.c_void_p(0)
    nd, ni = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
    calls = {"dmpc_set_feedback": lambda: L.dmpc_set_feedback(None, C.byref(f)),
             "dmpc_feedback_device": lambda: L.dmpc_feedback_device(None, 1, 1, 1, 1, *[z] * 15),
             "dmpc_feedback_log": lambda: L.dmpc_feedback_log(None, 1, 1, ni, ni, ni, nd, ni, nd, ni, nd, nd, nd, nd)}
    for name, call in calls.items():
        assert call() == -1 and L.dmpc_last_error(None).decode() == f"{name}: ctx is NULL", name


BAD_POLICIES = [(float("nan"), 0.0, 0), (0.0, float("nan"), 1), (-1e-9, 0.0, 0), (0.0, -INF, 0), (0.05, 0.25, 2), (0.05, 0.25, -1)]


def test_apply_host_refuses_bad_policies_and_shapes():
    c = fb.random_column(2, 3, 3, 1)
    args = [c[k] for k in ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next")]
    for bad in BAD_POLICIES:
        rc, msg, o = fb.raw_apply(bad, H, 1, *args)
        assert rc == -1 and msg.startswith("dmpc_feedback_apply_host: "), (bad, msg)
        assert all(o[k].tobytes() == np.asarray(c["v" if k == "v_rows" else k]).tobytes() for k in OUT if k != "event"), bad   # nothing written
    for good in ((0.0, 0.0, 0), (INF, INF, 1), (0.05, INF, 1)):
        assert fb.raw_apply(good, H, 1, *args)[0] == 0, good
    for kw in (dict(k=0), dict(S=0), dict(n=0), dict(n=4), dict(dist=dict(pushes=[di.push(2, 0, 1)])), dict(dist=dict(noise_p=-1.0))):
        k = kw.pop("k", 1)
        rc, msg, _ = fb.raw_apply((0.05, 0.25, 1), H, k, *args, **kw)
        assert rc == -1 and msg.startswith("dmpc_feedback_apply_host: "), (kw, msg)
    L = _lib.load()
    assert L.dmpc_feedback_apply_host(None, None, H, 1, 1, 1, 1, *[None] * 14) == -1 and L.dmpc_last_error(None).decode().startswith("dmpc_feedback_apply_host: ")
    # the Python layer's own shape checks, and its pass-through of the library's message
    with pytest.raises(_lib.DmpcError, match="^feedback_apply: "):
        _lib.feedback_apply(0.05, 0.25, 1, H, 1, c["p"][:, :, :44], *args[1:])
    with pytest.raises(_lib.DmpcError, match="^dmpc_feedback_apply_host: "):
        _lib.feedback_apply(-1.0, 0.25, 1, H, 1, *args)


def test_set_feedback_refuses_bad_policies_by_name():
    """dmpc_set_feedback checks the policy before it looks at the context, so its refusals show without a GPU (on a live context:
    tests/test_gpu_feedback.py); a good policy then meets the NULL context"""
    for bad in BAD_POLICIES:
        rc, msg = fb.raw_set_feedback(None, *bad, ctx=None)
        assert rc == -1 and msg.startswith("dmpc_set_feedback: ") and "ctx" not in msg, (bad, msg)
    for good in ((0.0, 0.0, 0), (INF, INF, 1), (0.05, 0.25, 1)):
        rc, msg = fb.raw_set_feedback(None, *good, ctx=None)
        assert rc == -1 and msg == "dmpc_set_feedback: ctx is NULL", (good, msg)


# ---- 2. the rule ----------------------------------------------------------------------------------------------------------------------------
def _dists(S, n):
    return {"none": None,
            "wind, noise, push": dict(noise_p=2e-3, noise_v=1e-2, seed=7, wind=np.arange(3.0 * S).reshape(S, 3) * 0.1 - 0.2,
                                      pushes=[di.push(S - 1, n - 1, 2, dp=(0.1, 0.0, -0.1), dv=(0.0, 0.3, 0.0)), di.push(0, 0, 3, dp=(0.0, 0.2, 0.0))])}


def _same(got, want, what):
    for key in OUT:
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), (what, key)


@pytest.mark.parametrize("S,n", [(1, 1), (2, 64), (2, 65)])
def test_apply_host_equals_the_restatement_byte_for_byte(S, n):
    N = n + (5 if n == 65 else 0)   # (a table wider than the commanded agents: the stride is N)
    c = fb.random_column(S, n, N, 100 * S + n)
    assert (c["status"] & 1).any() or n == 1
    args = [c[k] for k in ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next")]
    done = np.zeros(S, dtype=np.int32)
    done[S - 1] = S > 1   # a finished scene
    seen = set()
    for dname, dist in _dists(S, n).items():
        for pol in ((0.0, 0.0, 0), (0.0, 0.0, 1), (0.05, 0.25, 1), (0.05, 0.25, 0), (INF, INF, 1), (INF, 0.25, 1), (0.05, INF, 0)):
            for k in (2, 3):
                for sd in (None, done):
                    dp, dv = di.sample(H, S, n, k, **dist) if dist else (None, None)
                    want = fb.column(*pol, H, *args, dp, dv, sd)
                    rc, msg, got = fb.raw_apply(pol, H, k, *args, dist=dist, scene_done=sd)
                    assert rc == 0, msg
                    _same(got, want, (dname, pol, k, sd is not None))
                    seen.add((int(want["event"].sum()) > 0, int((want["event"] == 0).sum()) > 0))
                    if sd is not None and S > 1:   # the finished scene: nothing of it moved
                        assert all(np.array_equal(got[key][S - 1], np.asarray(c["v" if key == "v_rows" else key])[S - 1]) for key in OUT if key != "event")
        # the Python form returns the same
        got = _lib.feedback_apply(0.05, 0.25, 1, H, 2, *args, scene_done=done, disturb=dist)
        dp, dv = di.sample(H, S, n, 2, **dist) if dist else (None, None)
        _same(got, fb.column(0.05, 0.25, 1, H, *args, dp, dv, done), dname)
    assert (True, True) in seen or n == 1   # columns with events and columns with agents that had none


def test_a_deviation_equal_to_the_threshold_is_no_event():
    """the test is `>`: 3-4-0 triangles whose norms are exact in fp64, advanced and not advanced, on either threshold"""
    c = fb.random_column(1, 4, 4, 9, e_zero=True)
    c["status"][:] = [[1, 2, 1, 2]]
    g = np.array([0.1875, 0.25, 0.0])   # |g| = 0.3125, every product and sum exact
    dp, dv = np.zeros((1, 4, 3)), np.zeros((1, 4, 3))
    dp[0, :2], dv[0, 2:] = g, g
    pushes = [di.push(0, i, 1, dp=dp[0, i], dv=dv[0, i]) for i in range(4)]
    args = [c[k] for k in ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next")]
    assert fb.norm3(g) == 0.3125
    for pol, events in (((0.3125, 0.3125, 1), 0), ((np.nextafter(0.3125, 0), INF, 1), 2), ((INF, np.nextafter(0.3125, 0), 1), 2), ((0.3125, INF, 1), 0)):
        rc, msg, got = fb.raw_apply(pol, H, 1, *args, dist=dict(pushes=pushes))
        assert rc == 0 and int(got["event"].sum()) == events, (pol, got["event"])
        _same(got, fb.column(*pol, H, *args, dp, dv), pol)
        if not events:   # no event: the error is kept, the plan is not touched
            assert np.array_equal(got["e_p"], dp) and np.array_equal(got["e_v"], dv) and np.array_equal(got["lT_next"], c["lT_next"])


def test_trigger_zero_without_reanchor_is_state_plus_disturbance():
    """with e = 0 the state is q + d: today's disturbed loop -- and xh = x, e = 0 afterwards, whatever d was"""
    S, n = 2, 7
    c = fb.random_column(S, n, n, 5, e_zero=True)
    c["xh_p"], c["xh_v"] = c["x_p"].copy(), c["x_v"].copy()
    dist = _dists(S, n)["wind, noise, push"]
    dp, dv = di.sample(H, S, n, 2, **dist)
    args = [c[k] for k in ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next")]
    rc, _, got = fb.raw_apply((0.0, 0.0, 0), H, 2, *args, dist=dist)
    adv = ((c["status"] & 1) == 1)[..., None]
    assert rc == 0
    assert np.array_equal(got["x_p"], np.where(adv, c["p"][..., :3], c["x_p"]) + dp) and np.array_equal(got["x_v"], np.where(adv, c["v"][..., :3], c["x_v"]) + dv)
    assert np.array_equal(got["xh_p"], got["x_p"]) and np.array_equal(got["xh_v"], got["x_v"]) and not got["e_p"].any() and not got["e_v"].any()
    assert np.array_equal(got["lT_next"], c["lT_next"]) and np.array_equal(got["v_rows"], c["v"])
    # re-anchored: entry 0 of an advanced agent's column is x_p, and its v rows moved by g_v = dv
    rc, _, re_ = fb.raw_apply((0.0, 0.0, 1), H, 2, *args, dist=dist)
    lT0 = np.where(adv, c["p"], 0.0).transpose(0, 2, 1)   # (the step wrote the advanced agents' columns of the table)
    args[-1] = lT0
    rc, _, re_ = fb.raw_apply((0.0, 0.0, 1), H, 2, *args, dist=dist)
    a3 = np.broadcast_to(adv, (S, n, 3))
    assert np.array_equal(re_["lT_next"][:, :3, :].transpose(0, 2, 1)[a3], re_["x_p"][a3])
    assert np.array_equal(re_["v_rows"][..., 3:6], c["v"][..., 3:6] + dv)


# ---- 3. the head-on scene with the oracle's step --------------------------------------------------------------------------------------------
KT, TOL = 60, 0.1
PUSH = dict(pushes=[di.push(0, 0, 5, dp=(0.0, 0.15, 0.0))])


@functools.lru_cache(maxsize=None)
def _oracle_loop(policy, dist_key):
    """the restated loop over oracle.step on start.head_on() (shared: do not modify)"""
    from oracle import oracle as orc
    po, pf = stt.head_on()
    dist = PUSH if dist_key == "push" else dict(noise_p=2e-3, noise_v=1e-2, seed=dist_key)
    return fb.loop(fb.oracle_batch_step(orc, orc.make_params("bound", **ob.KW)), po[None], pf[None], KT, TOL, H, policy, dist)


def min_distance(res, s=0):
    """the smallest collision-metric distance |E1 (p_i - p_j)| of scene s over the columns it flew"""
    pk, used = res["pk"][s], int(res["K_T_used"][s])
    e1 = np.array([1.0, 1.0, 1.0 / ob.KW["c"]])
    n = pk.shape[0]
    return min(float(np.sqrt((((pk[i, k] - pk[j, k]) * e1) ** 2).sum())) for k in range(used) for i in range(n) for j in range(i))


def test_head_on_push_tells_the_three_policies_apart():
    cut = ob.KW["rmin"] - 0.05
    open_loop, trig = _oracle_loop((INF, INF, 0), "push"), _oracle_loop((0.05, 0.25, 1), "push")
    z0, z1 = _oracle_loop((0.0, 0.0, 0), "push"), _oracle_loop((0.0, 0.0, 1), "push")
    d_open, d_trig = min_distance(open_loop), min_distance(trig)
    both = min(int(z0["K_T_used"][0]), int(z1["K_T_used"][0]))
    diff = float(np.abs(z0["pk"][:, :, :both] - z1["pk"][:, :, :both]).max())
    print(f"open loop {d_open:.4f} m, triggered {d_trig:.4f} m (cut {cut:.2f}), events {trig['events']}, reanchor 0 vs 1: {diff:.3e} m")
    assert open_loop["events"] == [] and d_open < cut
    assert trig["events"] == [(5, 0, 0)] and d_trig >= cut
    assert trig["log"]["event_count"].tolist() == [[1, 0]] and trig["log"]["event_first"].tolist() == [[5, -1]] and trig["log"]["dev_p_col"][0, 0] == 5
    assert diff > 1e-3
    # a push along x on column 7, where no collision row is active: re-anchoring changes nothing the solver reads differently
    from oracle import oracle as orc
    po, pf = stt.head_on()
    step = fb.oracle_batch_step(orc, orc.make_params("bound", **ob.KW))
    xpush = dict(pushes=[di.push(0, 0, 7, dp=(0.15, 0.0, 0.0))])
    x0, x1 = (fb.loop(step, po[None], pf[None], KT, TOL, H, (0.0, 0.0, r), xpush) for r in (0, 1))
    assert x0["events"] == x1["events"] == [(7, 0, 0)] and x0["pk"].tobytes() == x1["pk"].tobytes()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bounded_noise_triggers_rarely_and_every_quiet_column_is_within_the_thresholds(seed):
    tp, tv = 0.05, 0.25
    res = _oracle_loop((tp, tv, 1), seed)
    cols = 2 * (int(res["K_T_used"][0]) - 1)
    print(f"seed {seed}: {len(res['events'])} events on {cols} agent-columns, largest deviation {res['log']['dev_p_max'].max():.4f} m, {res['log']['dev_v_max'].max():.4f} m/s")
    assert 0 < len(res["events"]) < cols / 4
    # the property: a column without an event left a deviation inside both thresholds (and that deviation is the error the next column starts with)
    quiet = 0
    for k, n_p, n_v, event in res["columns"]:
        calm = event[0] == 0
        quiet += int(calm.sum())
        assert (n_p[0][calm] <= tp).all() and (n_v[0][calm] <= tv).all(), k
        assert ((n_p[0] > tp) | (n_v[0] > tv))[~calm].all(), k
    assert quiet == cols - len(res["events"])
    assert res["log"]["dev_p_max"].max() == max(c[1].max() for c in res["columns"])
