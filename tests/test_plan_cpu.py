"""CPU: route planning (dmpc_plan_routes) without a device -- declared, exported and bound, the ABI revision still 8, a NULL context refused by
name, the binding's argument rules -- and the restatement of the pinned rule (tests/plan.py) itself: its hops against an independent queue BFS,
every emitted leg in line of sight, the slot rules, and, with the oracle's step in the route loop, that the planned waypoints lead the agents
round the wall that parks them when they fly straight."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from multiagent_planning_amd import _lib
from helpers import ROOT
import mission as ms
import plan as pl
import route as rt

NAMES = ("dmpc_plan_routes", "dmpc_plan_routes_device")


def test_plan_entries_are_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load()
    for name, nargs in zip(NAMES, (14, 15)):
        assert re.search(r"DMPC_API int " + name + r"\s*\(", hdr)
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    assert re.search(r"#define DMPC_ABI_VERSION 8\b", hdr) and _lib.ABI_VERSION == 8 and L.dmpc_abi_version() == 8
    for word, value in (("DMPC_PLAN_OK", pl.OK), ("DMPC_PLAN_TRUNCATED", pl.TRUNCATED), ("DMPC_PLAN_UNREACHABLE", pl.UNREACHABLE),
                        ("DMPC_PLAN_MAX_CELLS", pl.MAX_CELLS)):
        assert re.search(r"#define " + word + r" " + str(value) + r"\b", hdr), word
    assert (_lib.PLAN_OK, _lib.PLAN_TRUNCATED, _lib.PLAN_UNREACHABLE) == (pl.OK, pl.TRUNCATED, pl.UNREACHABLE)
    assert hasattr(_lib.Dmpc, "plan") and hasattr(_lib.Dmpc, "plan_routes_device")


def test_null_context_is_refused_by_name():
    L = _lib.load()
    nd, ni = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
    assert L.dmpc_plan_routes(None, 1, 1, 0, 4, nd, nd, nd, 0.25, 0.0, nd, ni, ni, ni) == -1
    assert L.dmpc_last_error(None).decode().startswith("dmpc_plan_routes:")
    assert L.dmpc_plan_routes_device(None, 1, 1, 0, 4, None, None, None, 0.25, 0.0, None, None, None, None, None) == -1
    assert L.dmpc_last_error(None).decode().startswith("dmpc_plan_routes_device:")


def test_argument_rules_of_the_binding():
    """checked before anything reaches the library (no context needed: the method is called unbound)"""
    s = pl.wall()
    plan = _lib.Dmpc.plan
    with pytest.raises(_lib.DmpcError, match="goals"):
        plan(None, s["po"][None], s["goals"], 0.25)                                   # batched po, unbatched goals
    with pytest.raises(_lib.DmpcError, match="N_cmd <= N"):
        plan(None, s["po"][:2], s["goals"], 0.25)
    with pytest.raises(_lib.DmpcError, match="goals"):
        plan(None, s["po"], s["goals"][:, :2], 0.25)
    with pytest.raises(_lib.DmpcError, match="obstacles"):
        plan(None, s["po"], s["goals"], 0.25, obstacles=np.zeros((2, 4, 3)))


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------------------
def _scenes():
    """(name, result with detail, po_cmd [S,nc,3], goals, W)"""
    w = pl.wall()
    out = [(f"wall {cm}", pl.result("wall", *cm), w["po"][None, :3], w["goals"][None], 4) for cm in pl.WALL_GRIDS]
    cs = pl.small_cases()
    out.append(("small", pl.result("small"), np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs]), pl.SMALL["W"]))
    f, m = pl.flat(), pl.maze()
    out.append(("flat", pl.result("flat"), f["po"][None], f["goals"][None], 4))
    out.append(("maze 32", pl.result("maze", 32), m["po"][None], m["goals"][None], 32))
    out.append(("maze 4", pl.result("maze", 4), m["po"][None], m["goals"][None], 4))
    return out


def test_hops_equal_an_independent_queue_bfs():
    for name, r, po, goals, W in _scenes():
        for s in range(po.shape[0]):
            for i in range(po.shape[1]):
                d = r["info"][s][i]
                n = d["free"].shape
                kw = pl.MAZE_KW if name.startswith("maze") else (pl.FLAT_KW if name == "flat" else pl.KW)
                a = tuple(int(v) for v in pl.cell_of(po[s, i], kw["pmin"], _cell(name), n))
                b = tuple(int(v) for v in pl.cell_of(goals[s, i], kw["pmin"], _cell(name), n))
                assert pl.bfs_hops(d["free"], a, b) == int(r["hops"][s, i]), (name, s, i)


def _cell(name):
    if name.startswith("wall"):
        return float(name.split("(")[1].split(",")[0])
    return {"small": pl.SMALL["cell"], "flat": 0.25}.get(name, 0.125)


def test_every_emitted_leg_is_clear_and_the_slots_follow_the_rule():
    seen = set()
    for name, r, po, goals, W in _scenes():
        for s in range(po.shape[0]):
            for i in range(po.shape[1]):
                d, n_wp, st, hops = r["info"][s][i], int(r["n_wp"][s, i]), int(r["plan_status"][s, i]), int(r["hops"][s, i])
                wp = r["waypoints"][s, i]
                seen.add(st)
                assert 1 <= n_wp <= W and wp.shape == (W, 3)
                assert wp[n_wp - 1].tobytes() == goals[s, i].tobytes()                # the last waypoint is the goal, bitwise
                assert all(wp[k].tobytes() == goals[s, i].tobytes() for k in range(n_wp, W))
                if st == pl.UNREACHABLE:
                    assert hops == -1 and n_wp == 1 and d["path"] is None
                    continue
                path, em = d["path"], d["emitted"]
                assert hops == len(path) - 1 and all(sum(abs(a - b) for a, b in zip(p, q)) == 1 for p, q in zip(path, path[1:]))
                assert all(d["free"][q] for q in path)
                if hops == 0:
                    assert n_wp == 1 and st == pl.OK and not em
                    continue
                assert em[-1] == hops and all(b > a for a, b in zip([0] + em, em))
                for a, b in zip([0] + em, em):
                    assert b == a + 1 or pl.clear(d["free"], path[a], path[b]), (name, s, i, a, b)
                    assert all(not pl.clear(d["free"], path[a], path[t]) for t in range(b + 1, hops + 1))   # ... and the farthest one
                assert (st == pl.TRUNCATED) == (len(em) > W) and n_wp == min(len(em), W)
    assert seen == {pl.OK, pl.TRUNCATED, pl.UNREACHABLE}


def test_the_scenes_are_what_the_gpu_tests_take_them_for():
    r = pl.result("maze", 32)
    assert int(r["hops"][0, 0]) == 350 and int(r["n_wp"][0, 0]) == 18 and int(r["plan_status"][0, 0]) == pl.OK
    r4 = pl.result("maze", 4)
    assert int(r4["n_wp"][0, 0]) == 4 and int(r4["plan_status"][0, 0]) == pl.TRUNCATED
    assert np.array_equal(r4["waypoints"][0, 0, :3], r["waypoints"][0, 0, :3])
    assert pl.grid_shape(pl.MAZE_KW["pmin"], pl.MAZE_KW["pmax"], 0.125) == (40, 40, 1)
    assert pl.grid_shape(pl.KW["pmin"], pl.KW["pmax"], 0.3) == (17, 17, 7)
    assert pl.grid_shape(pl.CAP_KW["pmin"], pl.CAP_KW["pmax"], 0.25) == (32, 32, 32)
    assert pl.grid_shape(pl.FLAT_KW["pmin"], pl.FLAT_KW["pmax"], 0.25) == (20, 20, 1)
    for cm in pl.WALL_GRIDS:
        w = pl.result("wall", *cm)
        assert w["n_wp"].tolist() == [[3, 3, 3]] and not w["plan_status"].any()
    names = [c[0] for c in pl.small_cases()]
    s = pl.result("small")
    row = lambda name: names.index(name)
    assert (s["hops"][row("same-cell")] == 0).all() and (s["n_wp"][row("same-cell")] == 1).all()
    assert (s["plan_status"][row("enclosed")] == pl.UNREACHABLE).all() and (s["hops"][row("enclosed")] == -1).all()
    for name in ("start-blocked", "goal-blocked", "outside"):
        assert (s["plan_status"][row(name)] == pl.OK).all() and (s["hops"][row(name)] > 0).all(), name
    cs = pl.small_cases()
    for name, which in (("start-blocked", 1), ("goal-blocked", 2)):                    # the cell really is blocked
        c = cs[row(name)]
        b = pl.blocked_grid(c[3], pl.KW["pmin"], pl.KW["pmax"], pl.SMALL["cell"], pl.SMALL["margin"], pl.KW["rmin"], pl.KW["c"])
        for p in c[which]:
            assert b[tuple(pl.cell_of(p, pl.KW["pmin"], pl.SMALL["cell"], b.shape))], name
    lo, hi = np.array(pl.KW["pmin"]), np.array(pl.KW["pmax"])
    out = cs[row("outside")]
    assert all(((p < lo) | (p > hi)).any() for p in np.vstack([out[1], out[2]]))


def test_the_planned_waypoints_lead_round_the_wall_that_parks_the_straight_flight():
    """wall, cell 0.25, margin 0.2, W = 4: route_loop over the oracle's step (solveSoftDMPCbound) reaches the goals over the planned waypoints;
    flown straight the same agents run all 100 columns and never reach"""
    from oracle import oracle as orc
    s = pl.wall()
    r = pl.result("wall", 0.25, 0.2)
    step = ms.oracle_step(orc, orc.make_params("bound", **s["kw"]))
    res = rt.route_loop(step, s["po"], r["waypoints"][0], r["n_wp"][0], s["capture"], 0, None, s["K_T_max"], s["error_tol"])
    print("wall over the planned waypoints:", res["K_T_used"], res["scene_status"], res["wp_col"].tolist())
    assert res["scene_status"] == rt.REACHED == 257 and res["K_T_used"] < s["K_T_max"]
    direct = rt.oracle_result("wall", 0, True)
    assert direct["scene_status"] == 1 and direct["K_T_used"] == 100
