"""GPU: routes -- every commanded agent through waypoints of its own -- through dmpc_transition_route.  There is no reference counterpart; the
truth is the reference's own MPC step in the loop a caller could write on the host (route.route_loop), over the oracle's step and over
dmpc_step_batch / dmpc_step_batch_cmd.

Bars are the ones the existing files use for the same comparisons: bit identity against the one-leg entries, the hold entry and missions,
against the host loop and between batch shapes; the closed loop against the oracle's at 1e-7 (tests/test_gpu_mission.py)."""
import os

import numpy as np
import pytest

import multiagent_planning_amd as mp
from helpers import ROOT, lib_source
import mission as ms
import route as rt

pytestmark = pytest.mark.gpu

REACHED = mp.ST_SOLVED | mp.ST_REACHED
HIST = ("pk", "vk", "ak")
HOLD = ("hold_count", "hold_first", "agent_status")


def _err(d):
    return d._L.dmpc_last_error(d._ctx).decode()


def _same(a, b, keys, what):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _route(d, s, **kw):
    """Dmpc.route on one scene dict of route.py, as a batch of one"""
    return d.route(s["po"][None], s["wp"][None], s["K_T_max"], s["capture"], n_wp=None if s["n_wp"] is None else s["n_wp"][None], timeout=s["timeout"],
                   error_tol=s["error_tol"], path=None if s["path"] is None else s["path"][None], **kw)


# ---- 1. W == 1: the one-leg entries and the hold entry byte for byte ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tiny", "split40"])
def test_one_waypoint_equals_transition_and_hold_byte_for_byte(shape):
    """one tiny scene, one with static and one with scripted vehicles, and 40 scenes (two parts on contexts of their own), against Dmpc.transition
    with on_fail "stop" and "hold"; nobody ever leaves a waypoint.  K_T_max = 30 columns in the batch of 40 with one scene's goals out of reach."""
    n = 40 if shape == "split40" else 1
    kt, tol = 30, ms.ERROR_TOL
    batches = [ms.batch([name] * n, list(range(n))) for name in ("reached", "static", "path")]
    if n == 40:
        src = lib_source()
        assert "(S >= 128 ? 4 : (S >= 32 ? 2 : 1))" in src
        for b in batches:
            b["goals"][7, 0, :, 0] += 2.0                                             # too far for 30 columns
    d = mp.Dmpc("bound", **ms.KW)
    for b, name in zip(batches, ("dmpc_transition", "dmpc_transition_cmd", "dmpc_transition_scripted")):
        pf = b["goals"][:, 0]
        for on_fail in ("stop", "hold"):
            leg = d.transition(b["po"], pf, kt, tol, path=b["path"], on_fail=on_fail)
            res = d.route(b["po"], pf[:, :, None], kt, 0.5, error_tol=tol, path=b["path"], on_fail=on_fail)
            _same(res, leg, HIST + ("K_T_used", "scene_status") + (HOLD if on_fail == "hold" else ()), f"{shape} / {name} / {on_fail}")
            assert res["wp_col"].shape == (n, 4, 1) and (res["wp_col"] == -1).all() and not res["wp_index"].any()
            assert (leg["scene_status"] == REACHED).any() and (n != 40 or leg["scene_status"][7] == mp.ST_SOLVED)


# ---- 2. timeout-only routes: missions with equal deadlines, byte for byte -----------------------------------------------------------------------
@pytest.mark.parametrize("name,T", [("deadline", 8), ("failure", 5)])
def test_timeout_only_routes_equal_missions_with_equal_deadlines(name, T):
    s = rt.timeout_route(name, T)
    d = mp.Dmpc("bound", **ms.KW)
    path = None if s["path"] is None else s["path"][None]
    mis = d.mission(s["po"][None], s["goals"][None], ms.KT, ms.ERROR_TOL, deadline=s["deadline"][None], path=path)
    res = d.route(s["po"][None], s["wp"][None], ms.KT, s["capture"], timeout=T, error_tol=ms.ERROR_TOL, path=path)
    print(name, "K_T_used", res["K_T_used"], mis["K_T_used"], "status", res["scene_status"], mis["scene_status"], "stage_col", mis["stage_col"])
    _same(res, mis, HIST + ("K_T_used", "scene_status"), name)
    Q = s["goals"].shape[0]
    assert list(mis["stage_col"][0, :Q - 1]) == [T, 2 * T] and int(mis["K_T_used"][0]) > 2 * T + 1
    for q in range(Q - 1):
        assert (res["wp_col"][:, :, q] == mis["stage_col"][:, q, None]).all(), q
    assert (res["wp_col"][:, :, Q - 1] == -1).all() and (res["wp_index"] == Q - 1).all()


# ---- 3. the scenes against the host loop (bit for bit) and the oracle's loop (1e-7) -------------------------------------------------------------
def _equals_loop(res, host, hold=False):
    u = host["K_T_used"]
    assert int(res["K_T_used"][0]) == u and int(res["scene_status"][0]) == host["scene_status"]
    assert np.array_equal(res["wp_col"][0], host["wp_col"]) and np.array_equal(res["wp_index"][0], host["wp_index"])
    for k in HIST + (HOLD if hold else ()):
        assert np.array_equal(res[k][0], host[k]), k


@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("name", ["wall", "capture-failure"])
def test_route_vs_host_loop_and_oracle_loop(name, precision):
    s, o = rt.scene(name), rt.oracle_result(name)
    d = mp.Dmpc("bound", precision=precision, **s["kw"])
    res = _route(d, s)
    host = rt.route_loop(ms.device_step(d), s["po"], s["wp"], s["n_wp"], s["capture"], s["timeout"], s["path"], s["K_T_max"], s["error_tol"])
    u = o["K_T_used"]
    errs = {k: float(np.abs(res[k][0] - o[k]).max()) for k in HIST}
    print(f"{name} {precision}: K_T_used {res['K_T_used'][0]} / host {host['K_T_used']} / oracle {u}, status {res['scene_status'][0]}, "
          f"wp_col {res['wp_col'][0].tolist()}, l_inf vs the oracle's loop {errs}")
    _equals_loop(res, host)
    assert host["K_T_used"] == u and host["scene_status"] == o["scene_status"]
    assert np.array_equal(host["wp_col"], o["wp_col"]) and np.array_equal(host["wp_index"], o["wp_index"])
    # f64: the bar of tests/test_gpu_mission.py.  mixed: the table the scan and the collision rows read is fp32 -- half an ulp of a coordinate of
    # 2 m is 1.2e-7 m on every step of the loop -- so the decisions must be the oracle's, the histories within the 1e-4 m that
    # tests/test_gpu_precision.py allows a mixed context against fp64 (seen: wall 1.2e-7 in pk, 2.1e-7 in ak; capture-failure 8.3e-7 and 3.0e-6)
    for k in HIST:
        assert errs[k] < (1e-7 if precision == "f64" else 1e-4), k
    assert not res["pk"][0][:, u:].any()


@pytest.mark.parametrize("on_fail", ["stop", "hold"])
def test_crowd300_vs_host_loop(on_fail):
    """300 agents: a block of 256 threads passes over the agents twice.  on_fail "hold": the host loop with tests/hold.py's rule, max_hold = 14"""
    s = rt.crowd300()
    hold = on_fail == "hold"
    d = mp.Dmpc("bound", **s["kw"])
    res = _route(d, s, on_fail=on_fail, max_hold=14)
    host = rt.route_loop(ms.device_step(d), s["po"], s["wp"], s["n_wp"], s["capture"], s["timeout"], s["path"], s["K_T_max"], s["error_tol"],
                         max_hold=14 if hold else None, h=s["kw"]["h"], alim=s["kw"]["alim"])
    col = res["wp_col"][0][:, 0]
    print(f"crowd300 {on_fail}: K_T_used {res['K_T_used'][0]}, status {res['scene_status'][0]}, switched {(col >= 0).sum()}, columns {sorted(set(col[col >= 0]))}, "
          f"index >= 256: {(col[256:] >= 0).sum()}" + (f", held {int((res['hold_count'][0] > 0).sum())}" if hold else ""))
    _equals_loop(res, host, hold)
    assert (col[256:] >= 0).sum() >= 1 and len(set(col[col >= 0])) >= 5
    assert (col[s["n_wp"] == 1] == -1).all() and (res["wp_col"][0][:, 1] == -1).all() and np.array_equal(res["wp_index"][0], (col >= 0).astype(np.int32))
    if not hold:
        assert int(res["scene_status"][0]) == 5 and int(res["K_T_used"][0]) == 24 and (col >= 0).sum() == 85 and 0 in col
    else:
        assert res["hold_count"].any() and int(res["scene_status"][0]) & mp.ST_HELD and int(res["K_T_used"][0]) > 24


# ---- 4. batch independence ------------------------------------------------------------------------------------------------------------------------
def test_scenes_of_a_split_batch_switch_on_their_own():
    """wall with seeds and capture-failure, embedded in one shape (route.embedded: their own shapes differ), as one batch of 32 scenes in two
    parts: every scene as when it runs alone"""
    kinds = [("wall", i // 2) if i % 2 == 0 else ("capture-failure", i // 2) for i in range(32)]
    b, c = rt.batch(kinds), rt.BATCH_CALL
    call = lambda d, sl: d.route(b["po"][sl], b["wp"][sl], c["K_T_max"], c["capture"], n_wp=b["n_wp"][sl], timeout=c["timeout"], error_tol=c["error_tol"],
                                 path=b["path"][sl])
    res = call(mp.Dmpc("bound", **rt.KW), slice(None))
    print("K_T_used", res["K_T_used"].tolist(), "status", res["scene_status"].tolist())
    assert (res["scene_status"][0::2] == REACHED).all() and (res["scene_status"][1::2] & ~mp.ST_SOLVED).all()
    assert len({c.tobytes() for c in res["wp_col"]}) >= 8 and len(set(res["K_T_used"].tolist())) >= 4
    one = mp.Dmpc("bound", **rt.KW)
    for s in range(32):
        alone = call(one, slice(s, s + 1))
        for k in rt.OUTPUTS:
            assert alone[k][0].tobytes() == res[k][s].tobytes(), (s, k)
        assert not res["pk"][s][:, res["K_T_used"][s]:].any()


# ---- 5. no REACHED while some agent is not on its last waypoint ----------------------------------------------------------------------------------
def test_a_column_never_reports_reached_before_every_agent_is_on_its_last_waypoint():
    """every agent starts within error_tol of its waypoint 0: the verdict of column 0 says "reached" while nobody is on its last waypoint.  The column
    must not end the trial; every agent leaves waypoint 0 there instead (agent 3 has a third waypoint, the second at its start, which it leaves on
    column 1) and the trial ends at the goals."""
    po = ms.square(0)
    side = np.array([0.3, 0.0, 0.0])
    wp = np.stack([po + 0.004, po + side, po + side], axis=1)
    wp[3, 1] = po[3]
    n_wp = np.array([2, 2, 2, 3], dtype=np.int32)
    tol = 0.02
    assert np.linalg.norm(po - wp[:, 0], axis=1).max() < tol
    d = mp.Dmpc("bound", **ms.KW)
    res = d.route(po, wp, 60, 0.1, n_wp=n_wp, error_tol=tol)
    host = rt.route_loop(ms.device_step(d), po, wp, n_wp, 0.1, 0, None, 60, tol)
    print("K_T_used", res["K_T_used"], "status", res["scene_status"], "wp_col", res["wp_col"].tolist())
    _equals_loop({k: v if k in ("K_T_used", "scene_status") else v[None] for k, v in res.items()}, host)
    assert (res["wp_col"][:, 0] == 0).all() and res["wp_col"][3, 1] == 1 and int(res["scene_status"][0]) == REACHED
    u = int(res["K_T_used"][0])
    assert u > 10 and np.linalg.norm(res["pk"][:, u - 1] - wp[np.arange(4), n_wp - 1], axis=1).max() < tol


# ---- 6. resident histories -------------------------------------------------------------------------------------------------------------------------
def test_postcheck_and_clearance_on_the_resident_histories():
    s = rt.wall()
    d = mp.Dmpc("bound", **rt.KW)
    res = _route(d, s)
    assert int(res["scene_status"][0]) == REACHED
    pf, pos, kt = s["wp"][np.arange(3), s["n_wp"] - 1][None], s["po"][None, 3:], s["K_T_max"]
    down = d.postcheck(res["K_T_used"], pf, res["pk"], res["vk"], res["ak"], po_static=pos)
    cd = d.clearance(res["K_T_used"], pf, res["pk"], res["vk"], res["ak"], po_static=pos)
    again = _route(d, s, histories=False)
    assert again["pk"] is None and np.array_equal(again["wp_col"], res["wp_col"])
    here = d.postcheck(res["K_T_used"], pf, KT_alloc=kt, po_static=pos)
    assert sorted(down) == sorted(here) and all(np.array_equal(down[k], here[k]) for k in down)
    ch = d.clearance(res["K_T_used"], pf, KT_alloc=kt, po_static=pos)
    assert all(np.array_equal(cd[k], ch[k], equal_nan=True) for k in cd) and np.isfinite(cd["dist"]).all()
    # the route is ONE flight round the wall: longer than the straight lines through it
    assert (down["totdist"] > 1.2 * np.linalg.norm(pf - s["po"][None, :3], axis=-1).sum(-1)).all()


# ---- 7. argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name_and_launch_nothing():
    s = rt.capture_failure()
    po, wp, path = s["po"][None], s["wp"][None], s["path"][None]
    d = mp.Dmpc("bound", **rt.KW)
    n0 = d.solve_count
    ok = np.full((1, 8), 3, dtype=np.int32)
    low, high = ok.copy(), ok.copy()
    low[0, 5], high[0, 2] = 0, 4
    cases = [(dict(W=0), "W must"), (dict(W=-2), "W must"), (dict(wp=None, W=3, n_cmd=8), "waypoints is NULL"),
             (dict(n_wp=low), "n_wp"), (dict(n_wp=high), "n_wp"),
             (dict(capture=0.0), "capture"), (dict(capture=-0.5), "capture"), (dict(capture=float("nan")), "capture"),
             (dict(timeout=-1), "timeout"), (dict(max_hold=-1), "max_hold"),
             (dict(n_cmd=0), "N_cmd must"), (dict(n_cmd=19), "N_cmd must"), (dict(P=0), "P must"), (dict(K_T_max=1), "bad arguments"),
             (dict(histories=(1, 0, 1)), "pk, vk, ak")]
    for kw, word in cases:
        args = dict(po=po, wp=wp, n_wp=ok, capture=0.3, path=path, K_T_max=20, error_tol=0.1); args.update(kw)
        rc, _ = rt.raw_route(d, **args)
        assert rc == -1 and _err(d).startswith("dmpc_transition_route: ") and word in _err(d), (kw, _err(d))
    assert d.solve_count == n0
    b = ms.scene("path")
    leg = d.transition(b["po"][None], b["goals"][None, 0], 30, ms.ERROR_TOL, path=b["path"][None])   # the context still runs a normal transition
    assert int(leg["scene_status"][0]) == REACHED and d.solve_count > n0
    rc, res = rt.raw_route(d, po, wp, None, 0.3, 0, path, 80, 0.1, outputs=(0, 0), hold_outputs=(0, 0, 0))   # ... and a route, without its optional outputs
    o = rt.oracle_result("capture-failure")
    assert rc == 0 and int(res["scene_status"][0]) == o["scene_status"] and int(res["K_T_used"][0]) == o["K_T_used"]
