"""CPU: the re-plan rule of tests/replan.py over the oracle's step (solveSoftDMPCbound) -- what the scene "door" does with and without re-plans, the
margins the mixed-precision GPU test relies on, and the rule's corner cases.  No GPU."""
import numpy as np
import pytest

import mission as ms
import plan as pl
import replan as rp
import route as rt

KW = rp.KW


@pytest.fixture(scope="module")
def step():
    from oracle import oracle as orc
    return ms.oracle_step(orc, orc.make_params("bound", **KW))


def _figures(tag, r):
    print(f"{tag}: K_T_used {r['K_T_used']}, status {r['scene_status']}, re-plans {[(k, i) for k, i, _, _ in r['replans']]}, "
          f"final {r['pk'][:, r['K_T_used'] - 1].round(2).tolist()}, boundary_margin {r['boundary_margin']:.3e}, capture_margin {r['capture_margin']:.3e}")


def test_door_flown_as_planned_never_arrives():
    """every = 0: the plan of column 0 sends agent 0 round the +y end, which the door shuts by column 8 (the rule's first prototype: 140 columns, agent 0 at
    (-1.50, 1.42, 1.70))"""
    r = rp.oracle_result("door", 0)
    _figures("door every=0", r)
    assert r["K_T_used"] == 140 and r["scene_status"] == 1 and not r["replans"] and not r["checked"]
    assert r["pk"][0, -1, 0] < 0.0 and np.linalg.norm(r["pk"][0, -1] - rp.door()["goals"][0]) > 1.0


@pytest.mark.parametrize("every,ahead", [(5, 0), (10, 0), (5, 3)])
def test_door_with_replans_arrives(every, ahead):
    """the rule's first prototype: every 5 -> 98 columns, re-plans of agent 0 on 5, 10, 30, 35, 40 and of agent 1 on 20, 25; every 10 -> 103 columns, two
    re-plans; every 5, ahead 3 -> 93 columns, four re-plans"""
    r = rp.oracle_result("door", every, ahead)
    _figures(f"door every={every} ahead={ahead}", r)
    assert r["scene_status"] == rp.REACHED and r["K_T_used"] < 140
    shut = 8 - ahead                                   # the column from which obst(k) holds the door at x = 0
    assert any(i == 0 and k >= shut for k, i, _, _ in r["replans"])
    assert r["replan_count"][0] >= 1 and r["replan_col"][0] >= shut and r["replan_count"].sum() == len(r["replans"])
    assert all(k % every == 0 and 0 < k < 139 for k in r["checked"])
    # the margins the mixed-precision GPU test needs: no x_p within 0.1 mm of a cell face on a re-plan column, no capture test within 0.1 mm
    assert r["boundary_margin"] > 1e-4 and r["capture_margin"] > 1e-4


def test_every_0_is_plan_then_route_loop(step):
    for s in (rp.door(), rp.wall()):
        r = rp.loop_on(step, s, 0, K_T_max=40)
        obst = s["path"][:, 0] if s["path"] is not None else s["po"][len(s["goals"]):]
        p = pl.plan(s["po"][None, :len(s["goals"])], s["goals"][None], obst[None], s["cell"], s["margin"], s["W"], KW)
        ref = rt.route_loop(step, s["po"], p["waypoints"][0], p["n_wp"][0], s["capture"], s["timeout"], s["path"], 40, s["error_tol"])
        for k in ("pk", "vk", "ak", "wp_col", "wp_index"):
            assert np.array_equal(r[k], ref[k]), k
        assert r["K_T_used"] == ref["K_T_used"] and r["scene_status"] == ref["scene_status"]
        for k in ("waypoints", "n_wp", "plan_status"):
            assert np.array_equal(r[k], p[k][0]), k
        assert not r["replan_count"].any() and (r["replan_col"] == -1).all()


def test_a_leg_inside_one_cell():
    """x_p and the current waypoint in one cell: the leg is that cell (plan.clear would divide by zero) -- free as the agent's own cell even when an
    obstacle blocks it; the next leg decides"""
    pmin, cell = KW["pmin"], 0.5
    free = np.ones((3, 3, 3), dtype=bool)
    assert rp.leg_clear(free, (1, 1, 1), (1, 1, 1))
    free[1, 1, 1] = False
    assert not rp.leg_clear(free, (1, 1, 1), (1, 1, 1))
    xp, goal = np.array([-1.2, 0.3, 1.2]), np.array([1.2, 0.2, 1.2])
    wp = np.array([[-1.1, 0.1, 1.3], goal])                                  # waypoint 0 in the agent's cell
    own = pl.blocked_grid(np.array([[-1.25, 0.25, 1.2]]), pmin, KW["pmax"], cell, 0.0, KW["rmin"], KW["c"])
    assert own[tuple(pl.cell_of(xp, pmin, cell, own.shape))] and rp.legs_clear(own, xp, wp, 0, 2, goal, pmin, cell)
    mid = pl.blocked_grid(np.array([[0.0, 0.25, 1.2]]), pmin, KW["pmax"], cell, 0.0, KW["rmin"], KW["c"])
    assert not rp.legs_clear(mid, xp, wp, 0, 2, goal, pmin, cell) and rp.legs_clear(mid, xp, wp, 0, 1, wp[0], pmin, cell)


def test_an_enclosed_agent_replans_to_the_goal_alone_and_the_loop_goes_on(step):
    """plan.small_cases' "enclosed" goal (a shell of six obstacles round its cell) as a flight: the plan of column 0 and every re-plan are
    UNREACHABLE -- the goal alone -- on every re-plan column, and the loop runs on to K_T_max"""
    name, po, goals, obst = pl.small_cases()[3]
    assert name == "enclosed"
    r = rp.replan_loop(step, np.vstack([po[:1], obst[:6]]), goals[:1], 0.5, 0.0, 4, 3, 0, 0.5, 0, None, 14, 0.05)
    print("enclosed:", r["replans"], r["K_T_used"], r["scene_status"])
    assert r["plan_status"][0] == pl.UNREACHABLE and r["n_wp"][0] == 1 and np.array_equal(r["waypoints"][0], np.tile(goals[0], (4, 1)))
    assert r["scene_status"] == 1 and r["K_T_used"] == 14                    # (the step solves every column: the agent parks in front of the shell)
    assert [k for k, _, _, _ in r["replans"]] == r["checked"] == [3, 6, 9, 12] and all(st == pl.UNREACHABLE for _, _, st, _ in r["replans"])
    assert r["replan_count"][0] == 4 and r["replan_col"][0] == 12


def test_no_replan_on_column_0_or_on_the_last_column(step):
    """every = 1 and K_T_max = 6: checked on columns 1 .. 4; every = 5 with K_T_max = 6: column 5 is the last one, nothing is checked"""
    s = rp.door()
    r = rp.loop_on(step, s, 1, K_T_max=6)
    assert r["K_T_used"] == 6 and r["checked"] == [1, 2, 3, 4]
    r = rp.loop_on(step, s, 5, K_T_max=6)
    assert r["checked"] == [] and not r["replans"]
    r = rp.loop_on(step, s, 5, K_T_max=7)
    assert r["checked"] == [5]
