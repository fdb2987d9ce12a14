"""GPU: route planning round static vehicles (dmpc_plan_routes) against the restatement of its pinned rule (tests/plan.py), byte for byte in
waypoints, n_wp, plan_status and hops; the planned waypoints flown by dmpc_transition_route against the host loop over the device's step."""
import numpy as np
import pytest

import multiagent_planning_amd as mp
import mission as ms
import plan as pl
import route as rt

pytestmark = pytest.mark.gpu

REACHED = mp.ST_SOLVED | mp.ST_REACHED


@pytest.fixture(scope="module")
def d():
    ctx = mp.Dmpc("bound", **pl.KW)
    yield ctx
    ctx.close()


def _ctx(kw, **more):
    return mp.Dmpc("bound", **kw, **more)


def _plan_scene(s, W, ctx=None):
    """Dmpc.plan on a scene dict of plan.py with an explicit obstacle set, as a batch of one"""
    own = ctx is None
    ctx = _ctx(s["kw"]) if own else ctx
    try:
        return ctx.plan(s["po"][None], s["goals"][None], s["cell"], s["margin"], W, obstacles=s["obst"][None])
    finally:
        if own:
            ctx.close()


# ---- 1. the wall ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,margin", pl.WALL_GRIDS)
def test_wall_equals_the_restatement(d, cell, margin):
    s = pl.wall()
    out = d.plan(s["po"][None], s["goals"][None], cell, margin, W=4)
    print(cell, margin, pl.grid_shape(pl.KW["pmin"], pl.KW["pmax"], cell), out["n_wp"].tolist(), out["hops"].tolist(), out["waypoints"][0].tolist())
    pl.same(out, pl.result("wall", cell, margin), f"wall {cell} {margin}")
    assert out["n_wp"].tolist() == [[3, 3, 3]]


# ---- 2. the table of small cases ------------------------------------------------------------------------------------------------------------------
def test_small_cases_as_one_call_and_each_on_its_own(d):
    cs, ref = pl.small_cases(), pl.result("small")
    po, goals, obst = (np.stack([c[k] for c in cs]) for k in (1, 2, 3))
    out = d.plan(po, goals, obstacles=obst, **pl.SMALL)
    print({c[0]: (out["n_wp"][k].tolist(), out["plan_status"][k].tolist(), out["hops"][k].tolist()) for k, c in enumerate(cs)})
    pl.same(out, ref, "small cases, one call")
    for k, c in enumerate(cs):
        alone = d.plan(po[k:k + 1], goals[k:k + 1], obstacles=obst[k:k + 1], **pl.SMALL)
        pl.same(alone, {key: ref[key][k:k + 1] for key in pl.KEYS}, c[0])
    names = [c[0] for c in cs]
    assert (out["plan_status"][names.index("enclosed")] == mp.PLAN_UNREACHABLE).all() and (out["hops"][names.index("enclosed")] == -1).all()
    assert (out["hops"][names.index("same-cell")] == 0).all()


def test_no_obstacles_gives_the_goals_and_route_on_them_is_transition(d):
    """M = 0, obst NULL: every n_wp == 1, the waypoints are the goals bitwise, and route() on them is transition() byte for byte"""
    b = ms.batch(["reached"] * 3, [0, 1, 2])
    po, pf = b["po"], b["goals"][:, 0]
    rc, msg, raw = pl.raw_plan(d, po.shape[0], po.shape[1], 0, 4, po, pf, None, 0.25, 0.2)
    assert rc == 0, msg
    out = d.plan(po, pf, 0.25, 0.2, W=4)
    pl.same(out, raw, "binding against the raw call")
    pl.same(out, pl.plan(po, pf, None, 0.25, 0.2, 4), "no obstacles")
    assert (out["n_wp"] == 1).all() and not out["plan_status"].any() and (out["hops"] >= 0).all()
    assert out["waypoints"].tobytes() == np.repeat(pf[:, :, None, :], 4, axis=2).tobytes()
    leg = d.transition(po, pf, 30, ms.ERROR_TOL)
    res = d.route(po, out["waypoints"], 30, 0.5, n_wp=out["n_wp"], error_tol=ms.ERROR_TOL)
    for k in ("pk", "vk", "ak", "K_T_used", "scene_status"):
        assert res[k].tobytes() == leg[k].tobytes(), k
    assert (leg["scene_status"] == REACHED).any()


def test_a_box_thinner_than_one_cell(d):
    s = pl.flat()
    out = _plan_scene(s, 4)
    print("flat", out["n_wp"].tolist(), out["hops"].tolist(), out["waypoints"][0].tolist())
    pl.same(out, pl.result("flat"), "flat")
    assert (out["hops"] > 0).all() and (out["n_wp"] > 1).all()


# ---- 3. serpentine maze: more levels and path cells than a workgroup has threads --------------------------------------------------------------------
@pytest.mark.parametrize("W", [32, 4])
def test_serpentine_maze(W):
    out = _plan_scene(pl.maze(), W)
    print("maze", W, out["n_wp"].tolist(), out["plan_status"].tolist(), out["hops"].tolist())
    pl.same(out, pl.result("maze", W), f"maze W = {W}")
    assert int(out["hops"][0, 0]) == 350
    assert (int(out["n_wp"][0, 0]), int(out["plan_status"][0, 0])) == ((18, mp.PLAN_OK) if W == 32 else (4, mp.PLAN_TRUNCATED))


# ---- 4. the grid at its cap -------------------------------------------------------------------------------------------------------------------------
def test_grid_at_the_cap_and_one_cell_more():
    s = pl.cap()
    assert pl.grid_shape(s["kw"]["pmin"], s["kw"]["pmax"], s["cell"]) == (32, 32, 32)
    ctx = _ctx(s["kw"])
    try:
        out = _plan_scene(s, 4, ctx)
        print("cap", out["n_wp"].tolist(), out["plan_status"].tolist(), out["hops"].tolist())
        pl.same(out, pl.result("cap"), "cap")
        assert (out["hops"] > 32).all() and (out["n_wp"] > 1).all()
    finally:
        ctx.close()
    big = _ctx(dict(s["kw"], pmax=(8.25, 8.0, 8.0)))                                 # 33 x 32 x 32
    try:
        n0 = big.solve_count
        rc, msg, _ = pl.raw_plan(big, 1, 2, 1, 4, s["po"][None], s["goals"][None], s["obst"][None], s["cell"], s["margin"])
        assert rc == -1 and msg.startswith("dmpc_plan_routes: ") and "33792" in msg and "32768" in msg, msg
        assert big.solve_count == n0
    finally:
        big.close()


# ---- 5. batching, the device form, the context's precision -------------------------------------------------------------------------------------------
def test_a_scene_does_not_depend_on_its_batch(d):
    b, ref = pl.batch5(), pl.result("batch5")
    call = lambda sl: d.plan(b["po"][sl], b["goals"][sl], b["cell"], b["margin"], W=4, obstacles=b["obst"][sl])
    out = call(slice(None))
    print("batch5: n_wp counts", np.bincount(out["n_wp"].ravel()).tolist(), "status counts", np.bincount(out["plan_status"].ravel(), minlength=3).tolist())
    pl.same(out, ref, "batch of 5")
    for s in range(5):
        alone = call(slice(s, s + 1))
        for k in pl.KEYS:
            assert alone[k][0].tobytes() == out[k][s].tobytes(), (s, k)
    assert (out["n_wp"] > 1).sum() >= 20 and len({out["n_wp"][s].tobytes() for s in range(5)}) == 5


def test_device_form_on_another_stream_equals_the_host_form(d):
    import torch
    b = pl.batch5()
    S, nc, M, W = 5, b["po"].shape[1], b["obst"].shape[1], 4
    host = d.plan(b["po"], b["goals"], b["cell"], b["margin"], W=W, obstacles=b["obst"])
    dev = torch.device("cuda")
    tpo, tg, tob = (torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("po", "goals", "obst"))
    wp = torch.full((S, nc, W, 3), -7.0, dtype=torch.float64, device=dev)
    n_wp, st, hops = (torch.full((S, nc), -7, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    d.plan_routes_device(S, nc, M, W, tpo.data_ptr(), tg.data_ptr(), tob.data_ptr(), b["cell"], b["margin"], wp.data_ptr(), n_wp.data_ptr(),
                         st.data_ptr(), hops.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    for k, t in (("waypoints", wp), ("n_wp", n_wp), ("plan_status", st), ("hops", hops)):
        assert t.cpu().numpy().tobytes() == host[k].tobytes(), k
    # outputs are optional
    n_wp.fill_(-7)
    torch.cuda.synchronize()
    d.plan_routes_device(S, nc, M, W, tpo.data_ptr(), tg.data_ptr(), tob.data_ptr(), b["cell"], b["margin"], n_wp=n_wp.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert n_wp.cpu().numpy().tobytes() == host["n_wp"].tobytes()


def test_context_precision_does_not_change_a_bit(d):
    b = pl.batch5()
    m = _ctx(pl.KW, precision="mixed")
    try:
        got = m.plan(b["po"], b["goals"], b["cell"], b["margin"], W=4, obstacles=b["obst"])
    finally:
        m.close()
    pl.same(got, pl.result("batch5"), "mixed-precision context")


# ---- 6. end to end on the device ---------------------------------------------------------------------------------------------------------------------
def test_plan_then_route_crosses_the_wall(d):
    """plan() then route() on the wall: the scene arrives, and K_T_used, wp_col and the histories equal route_loop over the device's step on the
    same waypoints bit for bit; transition() straight to the goals ends without ST_REACHED"""
    s = pl.wall()
    p = d.plan(s["po"][None], s["goals"][None], 0.25, 0.2, W=4)
    res = d.route(s["po"][None], p["waypoints"], s["K_T_max"], s["capture"], n_wp=p["n_wp"], error_tol=s["error_tol"])
    host = rt.route_loop(ms.device_step(d), s["po"], p["waypoints"][0], p["n_wp"][0], s["capture"], 0, None, s["K_T_max"], s["error_tol"])
    print("wall: K_T_used", res["K_T_used"], "status", res["scene_status"], "wp_col", res["wp_col"][0].tolist())
    assert int(res["scene_status"][0]) == REACHED
    assert int(res["K_T_used"][0]) == host["K_T_used"] and int(res["scene_status"][0]) == host["scene_status"]
    assert np.array_equal(res["wp_col"][0], host["wp_col"]) and np.array_equal(res["wp_index"][0], host["wp_index"])
    for k in ("pk", "vk", "ak"):
        assert res[k][0].tobytes() == host[k].tobytes(), k
    straight = d.transition(s["po"][None], s["goals"][None], s["K_T_max"], s["error_tol"])
    print("straight: K_T_used", straight["K_T_used"], "status", straight["scene_status"])
    assert not int(straight["scene_status"][0]) & mp.ST_REACHED
    down = d.postcheck(res["K_T_used"], s["goals"][None], res["pk"], res["vk"], res["ak"], po_static=s["po"][None, 3:])
    print("postcheck over the planned route: static clearance", {k: v.tolist() for k, v in down.items() if "static" in k})   # (reported, not asserted)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name_and_launch_nothing():
    s = pl.wall()
    po, goals, obst = s["po"][None, :3], s["goals"][None], s["po"][None, 3:]
    d = _ctx(pl.KW)
    try:
        n0 = d.solve_count
        ok = dict(S=1, nc=3, M=21, W=4, po=po, goals=goals, obst=obst, cell=0.25, margin=0.2)
        nan, inf = float("nan"), float("inf")
        cases = [(dict(S=0), "S and N_cmd"), (dict(S=-1), "S and N_cmd"), (dict(nc=0), "S and N_cmd"), (dict(M=-1), "M must"), (dict(W=0), "W must"),
                 (dict(W=-3), "W must"), (dict(po=None), "po_cmd and goals"), (dict(goals=None), "po_cmd and goals"), (dict(obst=None), "obst is NULL"),
                 (dict(cell=0.0), "cell"), (dict(cell=-0.25), "cell"), (dict(cell=nan), "cell"), (dict(cell=inf), "cell"),
                 (dict(margin=-0.1), "margin"), (dict(margin=nan), "margin"), (dict(margin=inf), "margin"),
                 (dict(cell=0.05), f"{int(np.prod(pl.grid_shape(pl.KW['pmin'], pl.KW['pmax'], 0.05)))} cells"), (dict(cell=1e-300), "cells")]
        for kw, word in cases:
            args = dict(ok); args.update(kw)
            rc, msg, _ = pl.raw_plan(d, **args)
            assert rc == -1 and msg.startswith("dmpc_plan_routes: ") and word in msg, (kw, msg)
        assert d.solve_count == n0
        # the context still plans (without its optional outputs, too) and flies afterwards
        rc, msg, out = pl.raw_plan(d, **ok)
        assert rc == 0, msg
        pl.same(out, pl.result("wall", 0.25, 0.2), "after the refusals")
        rc, msg, part = pl.raw_plan(d, **ok, outputs=(0, 1, 0, 0))
        assert rc == 0 and np.array_equal(part["n_wp"], out["n_wp"]) and not part["waypoints"].any()
        res = d.route(s["po"][None], out["waypoints"], s["K_T_max"], s["capture"], n_wp=out["n_wp"], error_tol=s["error_tol"])
        assert int(res["scene_status"][0]) == REACHED and d.solve_count > n0
    finally:
        d.close()
