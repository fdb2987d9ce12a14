"""CPU: the hold policy (hold.hold_loop) over the oracle's MPC step -- which agents are held on which columns of the wall crossings that stop
today, the budget, and the braking tail of a held plan.  The GPU side (tests/test_gpu_hold.py) compares dmpc_transition_hold with these loops."""
import math

import numpy as np
import pytest

import hold as ho
import mission as mi
import obstacles as ob

K, H, ALIM = 15, ob.KW["h"], ob.KW["alim"]
VMAX = 2.0              # m/s: the speed the post-check allows (dmpc_postcheck's vmax)
INFEAS, COLL = 8, 4


def _by_column(log):
    out = {}
    for k, i, st in log:
        out.setdefault(k, []).append((i, st))
    return out


def _stop(solver, kind, seed):
    from oracle import oracle as orc
    s = ho.scene(kind, seed)
    return mi.mission_loop(mi.oracle_step(orc, orc.make_params(solver, **ho.KW)), s["po"], s["goals"], None, s["path"], K_T_max=ho.KT, error_tol=ho.ERROR_TOL)


# (solver, kind, seed): (column and status at which the scene stops today, the hold log {column: [(agent, raw status)]}, the column reached)
EXPECTED = {
    ("hard", "A", 0): ((3, 9), {3: [(5, INFEAS)], 5: [(4, INFEAS)]}, 83),
    ("ondemand", "wall", 1): ((6, 9), {6: [(1, INFEAS), (2, INFEAS), (3, INFEAS), (5, INFEAS)], 7: [(2, INFEAS), (7, INFEAS)],
                                       **{k: [(2, INFEAS)] for k in range(8, 15)}}, 72),
    ("bound", "A", 0): ((19, 5), {19: [(3, COLL)], 23: [(0, COLL), (2, COLL)]}, 80),
    ("bound2", "A", 2): ((15, 5), {15: [(4, COLL), (6, COLL)], 16: [(0, COLL), (6, COLL)], 17: [(0, COLL), (6, COLL)]}, 72),
}


@pytest.mark.parametrize("case", ho.FAILING, ids=lambda c: "-".join(map(str, c)))
def test_scenes_that_stop_today_reach_their_goals_with_hold(case):
    """The oracle's loop with max_hold = 14 (K_T_max = 100, error_tol = 0.01), as computed -- (column, agent, raw status) of every hold:
      hard, scripted A 0        stops on column 3 (status 9); holds (3, 5, INFEAS), (5, 4, INFEAS); reached on column 83
      ondemand, wall_scene(8,1) stops on column 6 (9); 13 holds: column 6 agents 1, 2, 3, 5; column 7 agents 2, 7; columns 8 .. 14 agent 2
                                (nine consecutive columns, 6 .. 14); all INFEAS; reached on column 72
      bound, scripted A 0       stops on column 19 (5); holds (19, 3, COLL), (23, 0, COLL), (23, 2, COLL); reached on column 80
      bound2, scripted A 2      stops on column 15 (5); 6 holds: (15, 4), (15, 6), (16, 0), (16, 6), (17, 0), (17, 6), all COLL: agents 0 and 6 on
                                the same columns; reached on column 72"""
    (stop_col, stop_st), holds, reached_col = EXPECTED[case]
    m = _stop(*case)
    assert (m["K_T_used"] - 1, m["scene_status"]) == (stop_col, stop_st)
    r = ho.oracle_result(*case)
    print(case, r["log"], r["K_T_used"], r["scene_status"])
    assert _by_column(r["log"]) == holds
    assert r["K_T_used"] == reached_col + 1 and r["scene_status"] == (ho.REACHED | ho.HELD) and r["stage_col"][0] == reached_col
    # the record agrees with the log, and a held column of the histories is the second entry of the plan before it: nothing stands still
    n = sum(len(v) for v in holds.values())
    assert r["hold_count"].sum() == n and ((r["agent_status"] & ho.HELD) != 0).sum() == n
    for k, lst in holds.items():
        for i, st in lst:
            assert r["agent_status"][i, k] == (st | ho.HELD)
    first = {}
    for k, i, _ in r["log"]:
        first.setdefault(i, k)
    assert all(r["hold_first"][i] == first.get(i, -1) for i in range(8))
    u = r["K_T_used"]
    assert (r["agent_status"][:, 0] == 1).all() and (r["agent_status"][:, u:] == 0).all() and (r["agent_status"][:, 1:u] != 0).all()
    # up to the first hold the loop is the one that stops today
    assert np.array_equal(r["pk"][:, :stop_col], m["pk"][:, :stop_col])


def test_scenes_without_a_failure_are_untouched():
    for kind, seed in ho.CLEAN:
        r = ho.oracle_result("bound", kind, seed)
        m = _stop("bound", kind, seed)
        assert r["log"] == [] and r["scene_status"] == ho.REACHED and not r["hold_count"].any() and (r["hold_first"] == -1).all()
        for k in ("pk", "vk", "ak"):
            assert np.array_equal(r[k], m[k])
        assert r["K_T_used"] == m["K_T_used"]


@pytest.mark.parametrize("case", [("hard", "A", 0), ("bound", "A", 0)], ids=lambda c: "-".join(map(str, c)))
def test_max_hold_zero_is_the_loop_that_stops(case):
    r = ho.oracle_result(*case, max_hold=0)
    m = _stop(*case)
    for k in ("pk", "vk", "ak"):
        assert np.array_equal(r[k], m[k])
    assert r["K_T_used"] == m["K_T_used"] and r["scene_status"] == m["scene_status"] and m["scene_status"] & ~1
    assert r["log"] == [] and not r["hold_count"].any()
    u = r["K_T_used"]
    assert int(np.bitwise_or.reduce(r["agent_status"][:, u - 1])) == m["scene_status"] and not (r["agent_status"] & ho.HELD).any()


def test_budget_of_three_ends_on_the_fourth_consecutive_failure():
    """ondemand / wall_scene(8,1), max_hold = 3, as computed: holds on columns 6 (agents 1, 2, 3, 5), 7 (agents 2, 7) and 8 (agent 2); agent 2 fails a
    fourth time in a row on column 9, which ends the scene: K_T_used = 10, scene_status = SOLVED | INFEAS | HELD, not reached"""
    r = ho.oracle_result("ondemand", "wall", 1, max_hold=3)
    print(r["log"], r["K_T_used"], r["scene_status"])
    assert _by_column(r["log"]) == {6: [(1, 8), (2, 8), (3, 8), (5, 8)], 7: [(2, 8), (7, 8)], 8: [(2, 8)]}
    assert r["K_T_used"] == 10 and r["scene_status"] == (1 | INFEAS | ho.HELD) and r["stage_col"][0] == -1
    last = r["agent_status"][:, 9]
    assert last[2] == INFEAS and (np.delete(last, 2) == 1).all()                   # raw bits, no HELD on the over-budget column
    assert (r["agent_status"][2, 6:9] == (INFEAS | ho.HELD)).all()
    assert np.array_equal(r["pk"][2, 9], r["pk"][2, 8])                           # the over-budget agent stands where it was, as in every loop that stops
    full = ho.oracle_result("ondemand", "wall", 1)
    assert np.array_equal(r["pk"][:, :9], full["pk"][:, :9])


# ---- the tail ---------------------------------------------------------------------------------------------------------------------------------
def _plans():
    """plans [n,45] x 3 whose speeds stay within VMAX: random ones, and last entries on a grid over [-VMAX, VMAX] with both ends and their neighbours"""
    rng = np.random.default_rng(7)
    n = 2000
    p, v, a = rng.uniform(-2, 2, (n, 45)), rng.uniform(-VMAX, VMAX, (n, 45)), rng.uniform(-ALIM, ALIM, (n, 45))
    v[:600, 42:] = np.linspace(-VMAX, VMAX, 1800).reshape(600, 3)
    v[600, 42:], v[601, 42:] = np.nextafter(VMAX, 0), -np.nextafter(VMAX, 0)
    return p, v, a


def test_tail_brakes_within_alim_and_comes_to_rest():
    """A plan held again and again: the appended accelerations never exceed alim, a tail entry continues the one before it under that acceleration,
    and after K + ceil(vmax / (alim h)) = 25 holds every velocity of the plan is exactly zero and the positions no longer move.  The count: the
    tail brakes |v| <= vmax at alim h per entry, so after ceil(vmax / (alim h)) = 10 entries |v| <= alim h and the next entry's a_t = -v / h is
    unclamped; K - 1 further holds move that entry to the front.  It leaves v + h * (-v / h) == 0 exactly for h = 0.2 (asserted below on 10^6 values:
    the quotient by 0.2 is the product by 5 up to one rounding, which the product by 0.2 undoes)."""
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.uniform(-ALIM * H, ALIM * H, 10**6), [ALIM * H, -ALIM * H, 0.0, 5e-324, 1e-300]])
    q = -x
    q = q / H
    assert (np.abs(q) <= ALIM).all() and (x + H * q == 0).all()
    p, v, a = _plans()
    n_rest = K + math.ceil(VMAX / (ALIM * H))
    assert n_rest == 25
    for n in range(1, n_rest + 6):
        pn, vn, an = ho.shift_plan(p, v, a)
        assert np.array_equal(pn[:, :42], p[:, 3:]) and np.array_equal(vn[:, :42], v[:, 3:]) and np.array_equal(an[:, :42], a[:, 3:])
        at, vl, pl = an[:, 42:], v[:, 42:], p[:, 42:]
        assert (np.abs(at) <= ALIM).all()
        assert (np.abs(vn[:, 42:]) <= np.abs(vl)).all()                            # braking: never faster, never through zero and beyond
        assert (vn[:, 42:] * vl >= 0).all()
        assert np.abs(pn[:, 42:] - (pl + H * vl + 0.5 * H * H * at)).max() <= 4e-15   # the double integrator, up to the roundings of three sums near 4
        p, v, a = pn, vn, an
        if n == K:
            assert (np.abs(a) <= ALIM).all()                                       # the whole plan is tail now
        if n >= n_rest:
            p3 = p.reshape(-1, K, 3)
            assert (v == 0).all() and (a[:, 3:] == 0).all() and (p3 == p3[:, :1]).all()


def test_tail_of_the_initdmpc_plan_stands_still():
    """k = 1: the previous plan is initDMPC's (v = a = 0), so a hold on the first step repeats the straight line's last position"""
    po, pf = ob.wall_scene(8, 0)
    l = ob.init_table(po[:8], pf)
    z = np.zeros_like(l)
    p, v, a = ho.shift_plan(l, z, z)
    assert np.array_equal(p[:, :42], l[:, 3:]) and np.array_equal(p[:, 42:], l[:, 42:]) and not v.any() and not a.any()
