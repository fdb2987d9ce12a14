"""GPU: re-planned routes -- dmpc_transition_replan against the host loop of tests/replan.py over the device's own step (bit for bit) and over the
oracle's step (decisions identical, histories at the bars tests/test_gpu_route.py uses), and one re-plan step through dmpc_replan_routes_device
against the restatement, byte for byte.  There is no reference counterpart."""
import numpy as np
import pytest

import multiagent_planning_amd as mp
import mission as ms
import plan as pl
import replan as rp

pytestmark = pytest.mark.gpu

REACHED = mp.ST_SOLVED | mp.ST_REACHED
COMMON = rp.HIST + rp.ROUTE_KEYS


def _err(d):
    return d._L.dmpc_last_error(d._ctx).decode()


@pytest.fixture(scope="module")
def d():
    ctx = mp.Dmpc("bound", **rp.KW)
    yield ctx
    ctx.close()


def _replan(d, s, every, ahead=0, sl=None, **kw):
    """Dmpc.replan on a scene dict of replan.py as a batch of one, or (sl) on a slice of a batch dict"""
    pick = (lambda a: a[None]) if sl is None else (lambda a: a[sl])
    return d.replan(pick(s["po"]), pick(s["goals"]), s["K_T_max"], s["cell"], s["capture"], margin=s["margin"], W=s["W"], every=every, ahead=ahead,
                    timeout=s["timeout"], error_tol=s["error_tol"], path=None if s["path"] is None else pick(s["path"]), **kw)


# ---- 1. every == 0: plan + route, byte for byte ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wall", "door"])
def test_every_0_equals_plan_then_route_byte_for_byte(d, name):
    s = rp.wall() if name == "wall" else rp.door()
    nc = len(s["goals"])
    res = _replan(d, s, 0, ahead=2)
    obst = None if s["path"] is None else np.concatenate([s["path"][:, a] for a in range(3)])[None]     # obst(0) with ahead = 2
    p = d.plan(s["po"][None], s["goals"][None], s["cell"], s["margin"], W=s["W"], obstacles=obst)
    ref = d.route(s["po"][None], p["waypoints"], s["K_T_max"], s["capture"], n_wp=p["n_wp"], timeout=s["timeout"], error_tol=s["error_tol"],
                  path=None if s["path"] is None else s["path"][None])
    print(name, "K_T_used", res["K_T_used"], "status", res["scene_status"], "n_wp", res["n_wp"].tolist(), "wp_col", res["wp_col"].tolist())
    for k in COMMON:
        assert res[k].dtype == ref[k].dtype and res[k].tobytes() == ref[k].tobytes(), k
    for k in ("waypoints", "n_wp", "plan_status"):
        assert res[k].tobytes() == p[k].tobytes(), k
    assert not res["replan_count"].any() and (res["replan_col"] == -1).all() and (res["n_wp"] > 1).any()
    # what the parent's pipeline does with the door: it never arrives
    if name == "wall":
        assert int(res["scene_status"][0]) == REACHED
    else:
        assert int(res["scene_status"][0]) == mp.ST_SOLVED and int(res["K_T_used"][0]) == 140
    assert res["pk"].shape == (1, nc, s["K_T_max"], 3)


# ---- 2. the door: the host loop over the device's step (bit for bit), the oracle's loop -------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("every,ahead", [(5, 0), (5, 3)])
def test_door_vs_host_loop_and_oracle_loop(every, ahead, precision):
    s, o = rp.door(), rp.oracle_result("door", every, ahead)
    ctx = mp.Dmpc("bound", precision=precision, **s["kw"])
    try:
        res = _replan(ctx, s, every, ahead)
        host = rp.loop_on(ms.device_step(ctx), s, every, ahead)
    finally:
        ctx.close()
    u = o["K_T_used"]
    errs = {k: float(np.abs(res[k][0] - o[k]).max()) for k in rp.HIST}
    print(f"door every={every} ahead={ahead} {precision}: K_T_used {res['K_T_used'][0]} / host {host['K_T_used']} / oracle {u}, status {res['scene_status'][0]}, "
          f"re-plans {host['replans']}, count {res['replan_count'][0].tolist()}, col {res['replan_col'][0].tolist()}, l_inf vs the oracle's loop {errs}, "
          f"boundary_margin {o['boundary_margin']:.2e}, capture_margin {o['capture_margin']:.2e}")
    rp.same_as_loop(res, host)
    # the decisions are the oracle's: the end, every switch, every re-plan and the plans they made
    assert host["K_T_used"] == u and host["scene_status"] == o["scene_status"] == REACHED and host["replans"] == o["replans"] and host["checked"] == o["checked"]
    for k in ("wp_col", "wp_index") + rp.PLAN_KEYS:
        assert np.array_equal(host[k], o[k]), k
    assert res["replan_count"][0, 0] >= 1
    # f64: the bar of tests/test_gpu_mission.py.  mixed: the 1e-4 m of tests/test_gpu_precision.py, as tests/test_gpu_route.py argues; the decisions
    # can be the oracle's because no x_p is within 1e-4 m of a cell face on a re-plan column and no capture test within 1e-4 m (tests/test_replan_cpu.py)
    for k in rp.HIST:
        assert errs[k] < (1e-7 if precision == "f64" else 1e-4), k
    assert not res["pk"][0][:, u:].any()


def test_door_with_holds_equals_the_host_loop_with_holds(d):
    s = rp.door()
    res = _replan(d, s, 5, on_fail="hold", max_hold=14)
    host = rp.loop_on(ms.device_step(d), s, 5, max_hold=14)
    print("door hold: K_T_used", res["K_T_used"], "status", res["scene_status"], "held", res["hold_count"].tolist(), "re-plans", host["replans"])
    rp.same_as_loop(res, host, hold=True)
    # a scene in which an agent fails on column 5, a re-plan column: held, the scene goes on and is re-planned as the loop with holds says
    f = _failing()
    res = _replan(d, f, 5, on_fail="hold", max_hold=14)
    host = rp.loop_on(ms.device_step(d), f, 5, max_hold=14, K_T_max=f["K_T_max"])
    print("failing door, hold: K_T_used", res["K_T_used"], "status", res["scene_status"], "held", res["hold_count"].tolist(), "re-plans", host["replans"])
    rp.same_as_loop(res, host, hold=True)
    assert res["hold_count"].any()


# ---- 3. a batch in one shape ------------------------------------------------------------------------------------------------------------------------
def _failing():
    """the door with agent 1 in the door's way: its solve fails on column 5, a re-plan column (the oracle's loop: K_T_used 6, status 5)"""
    s = rp.door()
    s["po"] = s["po"].copy()
    s["po"][1] = (0.6, 2.0, 1.2)
    s["K_T_max"] = 40
    return s


def test_scenes_of_a_split_batch_replan_on_their_own(d):
    """32 doors (two parts on contexts of their own): jittered starts, one door that never moves, one scene that fails on a re-plan column; every
    scene byte for byte itself run alone, and the failed scene stops re-planning as the host loop does"""
    scenes = [rp.door(seed) for seed in range(30)] + [rp.door(0, moves=False), _failing()]
    b = dict(rp.DOOR_CALL, **{k: np.stack([s[k] for s in scenes]) for k in ("po", "goals", "path")})
    res = _replan(d, b, 5, sl=slice(None))
    print("K_T_used", res["K_T_used"].tolist(), "status", res["scene_status"].tolist(), "re-plans", res["replan_count"].sum(axis=1).tolist())
    assert (res["scene_status"][:31] == REACHED).all() and res["scene_status"][31] & ~mp.ST_SOLVED and len(set(res["K_T_used"].tolist())) >= 4
    assert len({c.tobytes() for c in res["replan_col"]}) >= 3 and (res["replan_count"][:30, 0] >= 1).all()
    one = mp.Dmpc("bound", **rp.KW)
    try:
        for s in range(32):
            alone = _replan(one, b, 5, sl=slice(s, s + 1))
            for k in COMMON + rp.PLAN_KEYS:
                assert alone[k][0].tobytes() == res[k][s].tobytes(), (s, k)
            assert not res["pk"][s][:, res["K_T_used"][s]:].any()
        host = rp.loop_on(ms.device_step(one), scenes[31], 5, K_T_max=140)
    finally:
        one.close()
    rp.same_as_loop(res, host, s=31)
    u = int(res["K_T_used"][31])
    assert (u - 1) % 5 == 0 and not res["replan_count"][31].any()            # it failed ON a re-plan column: nobody was planned again there


# ---- 4. one re-plan step: dmpc_replan_routes_device against the restatement ---------------------------------------------------------------------------
def _straight(po, goals, W=4):
    """every agent straight to its goal: waypoints [S,nc,W,3], n_wp = 1, cur = 0"""
    S, nc = goals.shape[:2]
    return np.repeat(goals[:, :, None, :], W, axis=2), np.ones((S, nc), dtype=np.int32), np.zeros((S, nc), dtype=np.int32)


def _check_step(ctx, state, obst, cell, margin, k, kw, what, **more):
    ref, flagged = rp.step_expected(state, obst, cell, margin, k, kw, more.get("scene_done"))
    out = rp.device_step_call(ctx, state, obst, cell, margin, k, **more)
    rp.same_step(out, ref, what)
    return out, flagged


def test_step_nobody_and_everybody_flagged(d):
    s = rp.wall()
    po, goals, obst = s["po"][None, :3], s["goals"][None], s["po"][None, 3:]
    p = pl.result("wall", 0.25, 0.2)
    state = rp.step_state(po, goals, p["waypoints"], p["n_wp"], np.zeros((1, 3)))
    out, flagged = _check_step(d, state, obst, 0.25, 0.2, 9, rp.KW, "the planned routes")
    assert not flagged
    for k in rp.STEP_KEYS:                                                   # every buffer is untouched
        assert out[k].tobytes() == state[k].tobytes(), k
    wp, n_wp, cur = _straight(po, goals)
    state = rp.step_state(po, goals, wp, n_wp, cur)
    out, flagged = _check_step(d, state, obst, 0.25, 0.2, 9, rp.KW, "straight through the wall")
    assert len(flagged) == 3 and out["waypoints"].tobytes() == p["waypoints"].tobytes() and (out["replan_count"] == 4).all() and (out["since"] == 9).all()
    # a scene that is over is skipped; the optional outputs are optional
    out, flagged = _check_step(d, state, obst, 0.25, 0.2, 9, rp.KW, "a scene that is over", scene_done=np.array([1]))
    assert not flagged
    out = rp.device_step_call(d, state, obst, 0.25, 0.2, 9, optional=False)
    ref, _ = rp.step_expected(state, obst, 0.25, 0.2, 9)
    for k in rp.STEP_KEYS:
        assert out[k].tobytes() == (ref if k in ("waypoints", "n_wp", "cur") else state)[k].tobytes(), k


def test_step_300_agents_some_flagged_on_another_stream(d):
    """two of plan.batch5's scenes with 300 agents each -- more than one block of 256 lanes in the check, more than 64 agents per wave --, a third of
    the agents on the second of two waypoints; on a stream of the caller's"""
    import torch
    b = pl.batch5(nc=300)
    po, goals, obst = b["po"][1:3], b["goals"][1:3], b["obst"][1:3]
    wp, n_wp, cur = _straight(po, goals)
    mid = 0.5 * (po + goals)
    two = np.arange(300) % 3 == 0
    wp[:, two, 0] = mid[:, two]
    n_wp[:, two] = 2
    cur[:, np.arange(300) % 6 == 0] = 1
    state = rp.step_state(po, goals, wp, n_wp, cur)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    out, flagged = _check_step(d, state, obst, b["cell"], b["margin"], 12, rp.KW, "300 agents", stream=stream)
    n = [sum(1 for s, _ in flagged if s == q) for q in (0, 1)]
    print("300 agents: flagged per scene", n, "beyond 256:", sum(1 for _, i in flagged if i >= 256), "n_wp", np.bincount(out["n_wp"].ravel()).tolist())
    assert all(20 <= q <= 280 for q in n) and sum(1 for _, i in flagged if i >= 256) >= 2


@pytest.mark.parametrize("case", ["2023-cells", "cap", "one-cell-leg", "unreachable", "truncated"])
def test_step_edge_grids_and_plans(case):
    kw, k, margin = rp.KW, 5, 0.0
    if case == "2023-cells":                                                 # 17 x 17 x 7: the last mask word is not full
        s, cell, margin = rp.wall(), 0.3, 0.2
        assert pl.grid_shape(kw["pmin"], kw["pmax"], cell) == (17, 17, 7)
        po, goals, obst = s["po"][None, :3], s["goals"][None], s["po"][None, 3:]
        wp, n_wp, cur = _straight(po, goals)
    elif case == "cap":                                                      # 32 x 32 x 32 cells, the workgroup of 1024 threads and 128 KiB of LDS
        s = pl.cap()
        kw, cell, margin = s["kw"], s["cell"], s["margin"]
        po = np.vstack([s["po"], [(0.3, 0.3, 0.3)]])[None]
        goals = np.vstack([s["goals"], [(0.4, 7.7, 0.2)]])[None]             # the third agent passes the obstacle at a distance: not flagged
        obst = s["obst"][None]
        wp, n_wp, cur = _straight(po, goals)
    elif case == "one-cell-leg":                                             # waypoint 0 in the agent's own cell, which an obstacle blocks; the second leg decides
        cell = 0.5
        po = np.array([[(-1.2, 0.3, 1.2), (-1.2, 0.3, 1.2)]])
        goals = np.array([[(1.2, 0.2, 1.2), (-1.2, 2.2, 1.2)]])
        obst = np.array([[(-1.25, 0.25, 1.2), (0.0, 0.25, 1.2)]])
        wp, n_wp, cur = _straight(po, goals)
        wp[0, :, 0] = (-1.1, 0.1, 1.3)
        n_wp[:] = 2
    elif case == "unreachable":
        cell = pl.SMALL["cell"]
        _, p, g, ob_ = pl.small_cases()[3]
        po, goals, obst = p[None], g[None], ob_[None]
        wp, n_wp, cur = _straight(po, goals)
    else:                                                                    # the maze with W = 4: the re-plan is truncated
        s = pl.maze()
        kw, cell = s["kw"], s["cell"]
        po, goals, obst = s["po"][None], s["goals"][None], s["obst"][None]
        wp, n_wp, cur = _straight(po, goals)
    state = rp.step_state(po, goals, wp, n_wp, cur)
    ctx = mp.Dmpc("bound", **kw)
    try:
        out, flagged = _check_step(ctx, state, obst, cell, margin, k, kw, case)
    finally:
        ctx.close()
    print(case, "flagged", flagged, "n_wp", out["n_wp"].tolist(), "status", out["plan_status"].tolist())
    if case == "2023-cells":
        assert len(flagged) == 3
    elif case == "cap":
        assert flagged == [(0, 0), (0, 1)] and out["plan_status"][0, 2] == -7
    elif case == "one-cell-leg":
        assert flagged == [(0, 0)]
    elif case == "unreachable":
        assert (0, 0) in flagged and out["plan_status"][0, 0] == mp.PLAN_UNREACHABLE and out["n_wp"][0, 0] == 1
    else:
        assert flagged == [(0, 0)] and out["plan_status"][0, 0] == mp.PLAN_TRUNCATED and out["n_wp"][0, 0] == 4


# ---- 5. argument checks -------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name_and_launch_nothing(d):
    s = rp.door()
    po, goals, path = s["po"][None], s["goals"][None], s["path"][None]
    n0 = d.solve_count
    cases = [(dict(every=-1), "every"), (dict(ahead=-1), "ahead"), (dict(goals=None, n_cmd=2), "goals is NULL"), (dict(W=0), "W must"),
             (dict(cell=0.0), "cell"), (dict(cell=float("nan")), "cell"), (dict(margin=-0.1), "margin"), (dict(cell=0.05), "more than 32768"),
             (dict(capture=0.0), "capture"), (dict(timeout=-1), "timeout"), (dict(max_hold=-1), "max_hold"), (dict(n_cmd=0), "N_cmd must"),
             (dict(P=0), "P must"), (dict(K_T_max=1), "bad arguments"), (dict(histories=(1, 0, 1)), "pk, vk, ak")]
    for kw, word in cases:
        args = dict(po=po, goals=goals, path=path, K_T_max=20); args.update(kw)
        rc, _ = rp.raw_replan(d, **args)
        assert rc == -1 and _err(d).startswith("dmpc_transition_replan: ") and word in _err(d), (kw, _err(d))
    assert d.solve_count == n0
    import torch
    z = torch.zeros(64, dtype=torch.float64, device="cuda").data_ptr()
    for kw, word in [(dict(waypoints=0), "waypoints, n_wp and cur"), (dict(k=-1), "k must"), (dict(cell=0.0), "cell"), (dict(W=0), "W must")]:
        a = dict(S=1, n_cmd=2, M=1, W=4, x_p=z, goals=z, obst=z, cell=0.25, margin=0.2, k=3, waypoints=z, n_wp=z, cur=z); a.update(kw)
        with pytest.raises(mp.DmpcError, match="dmpc_replan_routes_device: .*" + word):
            d.replan_routes_device(**a)
    # the context still runs: the entry without its optional outputs and histories
    rc, res = rp.raw_replan(d, po, goals, path=path, K_T_max=140, histories=(0, 0, 0), outputs=False)
    o = rp.oracle_result("door", 5)
    assert rc == 0 and int(res["scene_status"][0]) == o["scene_status"] and int(res["K_T_used"][0]) == o["K_T_used"] and d.solve_count > n0
