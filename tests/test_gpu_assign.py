"""GPU: goal assignment (dmpc_assign_goals) against the numpy restatement of its pinned rule (tests/assign.py), bit for bit in perm, price,
rounds, cost and pf_assigned -- on both sides of the one-launch boundary -- and, independently of the restatement, against
scipy.optimize.linear_sum_assignment and the eps-complementary-slackness certificate the prices carry."""
import re

import numpy as np
import pytest

import assign as asg
from helpers import ROOT

pytestmark = pytest.mark.gpu

PMIN, PMAX, RMIN, C = (-2.5, -2.5, 0.2), (2.5, 2.5, 2.2), 0.35, 2.0


def _one_launch_max():
    txt = open(ROOT + "/include/dmpc_hip_dev.h").read()
    return int(re.search(r"#define\s+DMPC_ASSIGN_ONE_LAUNCH_MAX\s+(\d+)", txt).group(1))


ONE_MAX = _one_launch_max()


@pytest.fixture(scope="module")
def d():
    import multiagent_planning_amd as mp
    ctx = mp.Dmpc("bound", c=asg.C_LATTICE)
    yield ctx
    ctx.close()


def _lattice_batch(N, seeds):
    sc = [asg.lattice(N, s) for s in seeds]
    return np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc])


@pytest.mark.parametrize("N,S", [(1, 3), (2, 3), (3, 3), (64, 3), (65, 3), (300, 3), (ONE_MAX, 1), (ONE_MAX + 76, 1)])
def test_device_equals_the_restatement_bit_for_bit(d, N, S):
    po, g = _lattice_batch(N, range(S))
    out = d.assign(po, g, eps=asg.lattice_eps(N))
    for s in range(S):
        ref = asg.lattice_result(N, s)
        assert ref["rounds"] > 0
        assert asg.same(out, ref, s) is None, (N, s, asg.same(out, ref, s), int(out["rounds"][s]), ref["rounds"])


def _tie_scene(name):
    if name == "equal":        # every c(i,j) equal, cmax > 0
        return np.tile([0.25, 0.5, 1.0], (8, 1)), np.tile([1.0, -0.75, 1.5], (8, 1))
    if name == "zero":         # cmax == 0
        return np.tile([0.25, 0.5, 1.0], (8, 1)), np.tile([0.25, 0.5, 1.0], (8, 1))
    sq = np.array([(1.0, 1.0, 1.0), (-1.0, 1.0, 1.0), (-1.0, -1.0, 1.0), (1.0, -1.0, 1.0)])
    r = np.sqrt(2.0)           # the same square turned by 45 degrees: every corner has two nearest goals
    return sq, np.array([(r, 0.0, 1.0), (0.0, r, 1.0), (-r, 0.0, 1.0), (0.0, -r, 1.0)])


@pytest.mark.parametrize("name", ["equal", "zero", "square"])
def test_ties_everywhere_equal_the_restatement(d, name):
    po, g = _tie_scene(name)
    eps = 1e-4 / len(po)
    ref = asg.auction(po, g, asg.C_LATTICE, eps)
    assert ref["rounds"] > 0 and (ref["cmax"] == 0) == (name == "zero")
    out = d.assign(po[None], g[None], eps=eps)
    assert asg.same(out, ref, 0) is None, asg.same(out, ref, 0)
    assert sorted(out["perm"][0].tolist()) == list(range(len(po)))


@pytest.mark.parametrize("N", [300, ONE_MAX + 76])
def test_a_scene_does_not_depend_on_its_batch(d, N):
    """a scene that finishes after a dozen rounds next to one that takes thousands: early exits, idle rounds and the host's windows"""
    ex, lat, eps = asg.exchange(N), asg.lattice(N), asg.lattice_eps(N)
    short, long_ = asg.auction(ex[0], ex[1], asg.C_LATTICE, eps), asg.lattice_result(N)
    assert 0 < short["rounds"] < 64 and long_["rounds"] > 2000
    po, g = np.stack([ex[0], lat[0], ex[0]]), np.stack([ex[1], lat[1], ex[1]])
    both = d.assign(po, g, eps=eps)
    for s in range(3):
        alone = d.assign(po[s:s + 1], g[s:s + 1], eps=eps)
        for k in ("perm", "pf", "price", "cost", "rounds"):
            assert both[k][s].tobytes() == alone[k][0].tobytes(), (s, k)
    assert asg.same(both, short, 0) is None and asg.same(both, long_, 1) is None and asg.same(both, short, 2) is None


@pytest.mark.parametrize("N", [64, ONE_MAX + 76])
def test_round_cap_stops_one_scene_and_leaves_the_other(d, N):
    ex, lat, eps, cap = asg.exchange(N), asg.lattice(N), asg.lattice_eps(N), 50
    short = asg.auction(ex[0], ex[1], asg.C_LATTICE, eps, max_rounds=cap)
    assert 0 < short["rounds"] < cap and asg.lattice_result(N)["rounds"] > cap
    capped = asg.auction(lat[0], lat[1], asg.C_LATTICE, eps, max_rounds=cap)
    assert capped["rounds"] == -1
    out = d.assign(np.stack([ex[0], lat[0]]), np.stack([ex[1], lat[1]]), eps=eps, max_rounds=cap)
    assert asg.same(out, short, 0) is None
    assert out["rounds"][1] == -1 and (out["perm"][1] == -1).all() and np.isnan(out["cost"][1]) and not out["pf"][1].any()
    assert np.array_equal(out["price"][1], capped["price"])
    # exactly as many rounds as the scene needs are enough
    need = asg.lattice_result(64)
    po, g = asg.lattice(64)
    assert asg.same(d.assign(po[None], g[None], eps=asg.lattice_eps(64), max_rounds=need["rounds"]), need, 0) is None


def test_random_scenes_against_scipy_and_the_price_certificate(d):
    S, N = 8, 100
    po, g = d.random_test(S, N, PMIN, PMAX, RMIN, C, 11)
    out = d.assign(po, g)
    eps = 1e-4 / N
    for s in range(S):
        perm = out["perm"][s]
        assert sorted(perm.tolist()) == list(range(N)) and out["rounds"][s] > 0
        opt, _ = asg.optimum(po[s], g[s], C)
        print(f"scene {s}: rounds {out['rounds'][s]}, cost - optimum = {out['cost'][s] - opt:.3e}")
        assert out["cost"][s] <= opt + 1e-4
        sl, cmax = asg.slack(po[s], g[s], C, perm, out["price"][s])
        assert sl.max() <= eps + 1e-12 * max(1.0, cmax + out["price"][s].max())
        assert np.array_equal(out["pf"][s], g[s][perm])


@pytest.mark.parametrize("S,N", [(4, 12), (2, 200)])
def test_exchange_scenes_send_every_agent_home(d, S, N):
    po, pf = d.random_exchange(S, N, PMIN, PMAX, RMIN, 5)
    assert not np.array_equal(po, pf)
    out = d.assign(po, pf)
    assert out["pf"].tobytes() == po.tobytes() and (out["cost"] == 0.0).all() and (out["rounds"] > 0).all()


@pytest.mark.parametrize("N", [65, ONE_MAX + 76])
def test_device_form_equals_the_host_form(d, N):
    import torch
    po, g = _lattice_batch(N, range(2))
    eps = asg.lattice_eps(N)
    host = d.assign(po, g, eps=eps)
    dev = torch.device("cuda")
    tpo, tg = torch.from_numpy(po).to(dev), torch.from_numpy(g).to(dev)
    perm = torch.full((2, N), -7, dtype=torch.int32, device=dev)
    rounds = torch.full((2,), -7, dtype=torch.int32, device=dev)
    pf, price, cost = torch.zeros((2, N, 3), dtype=torch.float64, device=dev), torch.zeros((2, N), dtype=torch.float64, device=dev), \
        torch.zeros((2,), dtype=torch.float64, device=dev)
    d.assign_goals_device(2, N, tpo.data_ptr(), tg.data_ptr(), eps, 0, perm.data_ptr(), pf.data_ptr(), price.data_ptr(), cost.data_ptr(),
                          rounds.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, t in (("perm", perm), ("pf", pf), ("price", price), ("cost", cost), ("rounds", rounds)):
        assert t.cpu().numpy().tobytes() == host[k].tobytes(), k
    # outputs are optional
    d.assign_goals_device(2, N, tpo.data_ptr(), tg.data_ptr(), eps, 0, perm=perm.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert perm.cpu().numpy().tobytes() == host["perm"].tobytes()


def test_context_precision_does_not_change_a_bit(d):
    import multiagent_planning_amd as mp
    po, g = d.random_test(2, 100, PMIN, PMAX, RMIN, C, 3)
    want = d.assign(po, g)
    m = mp.Dmpc("bound", precision="mixed", c=asg.C_LATTICE)
    try:
        got = m.assign(po, g)
    finally:
        m.close()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_refusals(d):
    po, g = asg.lattice(3)
    po, g = po[None], g[None]
    bad = [(0, 3, po, g, 1e-3), (1, 0, po, g, 1e-3), (-1, 3, po, g, 1e-3), (1, 3, None, g, 1e-3), (1, 3, po, None, 1e-3), (1, 3, po, g, 0.0),
           (1, 3, po, g, -1e-3), (1, 3, po, g, float("nan")), (1, 3, po, g, float("inf"))]
    for S, N, a, b, eps in bad:
        rc, msg = asg.raw_assign(d, S, N, a, b, eps)
        assert rc == -1 and msg.startswith("dmpc_assign_goals: "), (S, N, eps, rc, msg)
    rc, _ = asg.raw_assign(d, 1, 3, po, g, 1e-3)
    assert rc == 0


def test_transition_with_assign_flies_an_exchange_scene_home(d):
    import multiagent_planning_amd as mp
    po, pf = d.random_exchange(1, 12, PMIN, PMAX, RMIN, 9)
    out = d.transition(po, pf, 8, assign=True)
    assert out["K_T_used"][0] == 1 and out["scene_status"][0] == (mp.ST_SOLVED | mp.ST_REACHED)
    assert np.array_equal(pf[0][out["perm"][0]], po[0])
    plain, off = d.transition(po, pf, 8), d.transition(po, pf, 8, assign=False)
    assert list(plain) == list(off) and "perm" not in plain
    for k in plain:
        assert plain[k].tobytes() == off[k].tobytes(), k
    assert plain["K_T_used"][0] > 1


def test_mission_with_assign_chains_the_stages(d):
    po, g1 = d.random_test(2, 8, PMIN, PMAX, RMIN, C, 21)
    g2, _ = d.random_test(2, 8, PMIN, PMAX, RMIN, C, 22)
    goals = np.stack([g1, g2], axis=1)
    out = d.mission(po, goals, 4, assign=True)
    a1 = d.assign(po, g1)
    a2 = d.assign(a1["pf"], g2)
    assert out["perm"].shape == (2, 2, 8)
    assert np.array_equal(out["perm"][:, 0], a1["perm"]) and np.array_equal(out["perm"][:, 1], a2["perm"])
    flown = d.mission(po, np.stack([a1["pf"], a2["pf"]], axis=1), 4)
    plain = d.mission(po, goals, 4)
    assert "perm" not in plain and sorted(out) == sorted(list(plain) + ["perm"])
    for k in flown:
        assert out[k].tobytes() == flown[k].tobytes(), k
