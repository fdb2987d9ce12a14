"""CPU: routes (dmpc_transition_route) without a device -- declared, exported and bound, the ABI revision still 8, a NULL context refused by
name, the binding's argument rules -- and the conditions the scenes of tests/route.py must meet for the GPU tests (tests/test_gpu_route.py)
to be worth running, checked with the oracle's loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from multiagent_planning_amd import _lib
from helpers import ROOT
import mission as ms
import route as rt

NAME = "dmpc_transition_route"


def test_route_entry_is_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load()
    assert re.search(r"DMPC_API int " + NAME + r"\s*\(", hdr)
    assert NAME in _lib.ABI_SYMBOLS and hasattr(L, NAME) and getattr(L, NAME).argtypes is not None and len(L.dmpc_transition_route.argtypes) == 25
    assert re.search(r"#define DMPC_ABI_VERSION 8\b", hdr) and _lib.ABI_VERSION == 8 and L.dmpc_abi_version() == 8
    assert not re.findall(r"dmpc_[a-z_]*sharded[a-z_]*_route|dmpc_[a-z_]*route[a-z_]*sharded", hdr)
    # the header states the two rules a caller could not guess
    assert "AT MOST ONE WAYPOINT PER AGENT AND COLUMN" in raw and raw.count("THE TABLE IS NOT REWRITTEN") == 2
    assert hasattr(_lib.Dmpc, "route")


def test_null_context_is_refused_by_name():
    L = _lib.load()
    nd, ni = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
    assert L.dmpc_transition_route(None, 1, 2, 2, 1, nd, nd, ni, 0.5, 0, nd, 0, 10, 0.01, 0, nd, nd, nd, ni, ni, ni, ni, ni, ni, ni) == -1
    assert L.dmpc_last_error(None).decode().startswith(NAME + ":")


def test_argument_rules_of_the_binding():
    """checked before anything reaches the library (no context needed: the method is called unbound)"""
    s = rt.capture_failure()
    po, wp, path = s["po"], s["wp"], s["path"]
    route = _lib.Dmpc.route
    with pytest.raises(_lib.DmpcError, match="waypoints"):
        route(None, po, wp[:, 0], 10, 0.3)                                            # one waypoint per agent without the waypoint axis
    with pytest.raises(_lib.DmpcError, match="waypoints"):
        route(None, po[None], wp, 10, 0.3)                                            # batched po, unbatched waypoints
    with pytest.raises(_lib.DmpcError, match="same commanded agents"):
        route(None, np.vstack([po, ms.STATIC]), wp, 10, 0.3, path=path)
    with pytest.raises(_lib.DmpcError, match="FIRST N_cmd"):
        route(None, po[:3], wp, 10, 0.3)
    for bad in (np.zeros(8, dtype=int), np.full(8, 4), np.ones(7, dtype=int), np.ones(8)):
        with pytest.raises(_lib.DmpcError, match="n_wp"):
            route(None, po, wp, 10, 0.3, n_wp=bad, path=path)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(_lib.DmpcError, match="capture"):
            route(None, po, wp, 10, bad, path=path)
    with pytest.raises(_lib.DmpcError, match="timeout"):
        route(None, po, wp, 10, 0.3, timeout=-1, path=path)
    with pytest.raises(_lib.DmpcError, match="on_fail"):
        route(None, po, wp, 10, 0.3, path=path, on_fail="go on")


def test_scenes_lie_inside_the_workspace():
    for s in (rt.wall(), rt.wall(3), rt.capture_failure(), rt.crowd300(), rt.embedded("wall", 2), rt.embedded("capture-failure", 1)):
        lo, hi = np.array(s.get("kw", rt.KW)["pmin"]), np.array(s.get("kw", rt.KW)["pmax"])
        pts = [s["po"], s["wp"].reshape(-1, 3)] + ([s["path"].reshape(-1, 3)] if s["path"] is not None else [])
        for p in pts:
            assert (p >= lo).all() and (p <= hi).all()
    w = rt.wall()
    assert w["po"].shape == (24, 3) and w["wp"].shape == (3, 3, 3) and list(w["n_wp"]) == [3, 3, 2]
    c = rt.crowd300()
    assert c["po"].shape == (300, 3) and c["wp"].shape == (300, 2, 3) and (c["n_wp"] == 2).sum() == 257 and (c["n_wp"][::7] == 1).all()


def test_the_wall_parks_the_agents_and_the_routes_lead_them_round_it():
    """flown directly the oracle's loop (solveSoftDMPCbound) runs all 100 columns, never reaches and leaves every agent more than 1 m from its goal;
    over its waypoints it arrives in 68 columns, the agents switch on different columns, in flight, and no decision is closer to its threshold than
    1e-5 -- a hundred times the 1e-7 the device's loop agrees with the oracle's to"""
    s = rt.wall()
    goal = s["wp"][np.arange(3), s["n_wp"] - 1]
    d = rt.oracle_result("wall", 0, True)
    assert d["K_T_used"] == 100 and d["scene_status"] == 1 and (d["wp_col"] == -1).all()
    assert np.linalg.norm(d["pk"][:, -1] - goal, axis=1).min() > 1.0
    r = rt.oracle_result("wall")
    print("wall:", r["K_T_used"], r["wp_col"].tolist(), r["switch_speed"], r["capture_margin"], sorted(r["reach_margin"].items())[-2:])
    assert r["scene_status"] == rt.REACHED and r["K_T_used"] == 68
    assert r["wp_col"].tolist() == [[20, 35, -1], [19, 33, -1], [21, -1, -1]] and list(r["wp_index"]) == [2, 2, 1]
    assert len(r["switch_speed"]) == 5 and min(r["switch_speed"]) > ms.SPEED_FLOOR
    last = sorted(r["reach_margin"])[-2:]
    assert last == [66, 67] and r["capture_margin"] > 1e-5 and min(r["reach_margin"][k] for k in last) > 1e-5
    assert np.linalg.norm(r["pk"][:, 67] - goal, axis=1).max() < s["error_tol"] and not r["pk"][:, 68:].any()


def test_capture_failure_stops_after_every_agent_has_switched_once():
    r = rt.oracle_result("capture-failure")
    print("capture-failure:", r["K_T_used"], r["scene_status"], r["wp_col"][:, 0], r["capture_margin"])
    assert r["scene_status"] == 5 and r["K_T_used"] == 32 and r["capture_margin"] > 1e-5
    assert (r["wp_index"] == 1).all() and (r["wp_col"][:, 1:] == -1).all()
    assert r["wp_col"][:, 0].min() == 18 and r["wp_col"][:, 0].max() == 25 and len(set(r["wp_col"][:, 0])) > 1


def test_crowd300_switches_on_many_columns_and_past_the_first_256_agents():
    r, s = rt.oracle_result("crowd300"), rt.crowd300()
    col = r["wp_col"][:, 0]
    print("crowd300:", r["K_T_used"], r["scene_status"], (col >= 0).sum(), sorted(set(col[col >= 0])), (col[256:] >= 0).sum())
    assert r["scene_status"] == 5 and r["K_T_used"] == 24
    assert (col[s["n_wp"] == 1] == -1).all() and np.array_equal(r["wp_index"], (col >= 0).astype(np.int32))
    assert (col >= 0).sum() == 85 and (col[256:] >= 0).sum() >= 1 and len(set(col[col >= 0])) >= 5 and 0 in col


@pytest.mark.parametrize("name,T,used", [("deadline", 8, 61), ("failure", 5, 45)])
def test_timeout_only_routes_are_missions_with_equal_deadlines(name, T, used):
    """every n_wp == W, a capture too small to fire, timeout = T: the oracle's route loop equals its mission loop with deadline = [T, T, 0]"""
    from oracle import oracle as orc
    s = rt.timeout_route(name, T)
    step = ms.oracle_step(orc, orc.make_params("bound", **ms.KW))
    m = ms.mission_loop(step, s["po"], s["goals"], s["deadline"], s["path"])
    r = rt.route_loop(step, s["po"], s["wp"], None, s["capture"], T, s["path"], ms.KT, ms.ERROR_TOL)
    print(name, m["K_T_used"], m["scene_status"], m["stage_col"], r["wp_col"][0])
    assert r["K_T_used"] == m["K_T_used"] == used and r["scene_status"] == m["scene_status"]
    assert list(m["stage_col"][:2]) == [T, 2 * T]                                     # no intermediate stage is reached before its deadline
    assert all(np.array_equal(r[k], m[k]) for k in ("pk", "vk", "ak"))
    assert (r["wp_col"][:, :2] == m["stage_col"][:2]).all() and (r["wp_col"][:, 2] == -1).all()


def test_loop_with_one_waypoint_is_the_one_leg_loop():
    """W = 1: the rule leaves obstacles.oracle_loop / scripted.oracle_loop_scripted as they are"""
    from oracle import oracle as orc
    import obstacles as ob
    import scripted as sc
    prm = orc.make_params("bound", **ms.KW)
    for name in ("static", "path"):
        s = ms.scene(name)
        pf = s["goals"][0]
        r = rt.route_loop(ms.oracle_step(orc, prm), s["po"], pf[:, None], None, 0.5, 0, s["path"], 40, ms.ERROR_TOL)
        o = (sc.oracle_loop_scripted(orc, prm, s["po"], pf, s["path"], K_T_max=40, error_tol=ms.ERROR_TOL) if s["path"] is not None
             else ob.oracle_loop(orc, prm, s["po"], pf, 40, error_tol=ms.ERROR_TOL))
        assert r["K_T_used"] == o["K_T_used"] and r["scene_status"] == o["scene_status"] == rt.REACHED
        assert all(np.array_equal(r[k], o[k]) for k in ("pk", "vk", "ak"))
        assert (r["wp_col"] == -1).all() and (r["wp_index"] == 0).all()


def test_the_batch_scenes_keep_their_character_in_the_batch_shape():
    """wall and capture-failure embedded in one shape (route.embedded) under the batch's call parameters: the wall still arrives over its waypoints,
    on columns of its own per seed; the crossing still stops with a failed agent after switches"""
    from oracle import oracle as orc
    step = ms.oracle_step(orc, orc.make_params("bound", **rt.KW))
    c = rt.BATCH_CALL
    res = {}
    for kind, seed in (("wall", 0), ("wall", 1), ("capture-failure", 0)):
        e = rt.embedded(kind, seed)
        res[kind, seed] = r = rt.route_loop(step, e["po"], e["wp"], e["n_wp"], c["capture"], c["timeout"], e["path"], c["K_T_max"], c["error_tol"])
        print(kind, seed, r["K_T_used"], r["scene_status"], r["wp_col"].tolist())
    w0, w1, f = res["wall", 0], res["wall", 1], res["capture-failure", 0]
    assert w0["scene_status"] == w1["scene_status"] == rt.REACHED and (w0["wp_col"][:3, 0] > 0).all() and (w0["wp_col"][3:] == -1).all()
    assert not np.array_equal(w0["pk"], w1["pk"])
    assert f["scene_status"] & ~1 and (f["wp_col"][:, 0] > 0).any()
