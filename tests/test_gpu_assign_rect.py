"""GPU: rectangular goal assignment (dmpc_assign_rect: N agents, M goals) against the numpy restatement of its pinned rule (tests/assign_rect.py),
bit for bit in perm, owner, price, rounds, cost and pf_assigned; against dmpc_assign_goals on square scenes; and through transition() and
mission() with assign="rect"."""
import re

import numpy as np
import pytest

import assign as asg
import assign_rect as ar
from helpers import ROOT

pytestmark = pytest.mark.gpu

PMIN, PMAX, RMIN = (-2.5, -2.5, 0.2), (2.5, 2.5, 2.2), 0.35
ONE_MAX = int(re.search(r"#define\s+DMPC_ASSIGN_ONE_LAUNCH_MAX\s+(\d+)", open(ROOT + "/include/dmpc_hip_dev.h").read()).group(1))
# one person; one object; one more object than persons; both orientations; a wave boundary on each side; the 256 -> 1024-thread switch with the
# reverse columns in LDS; the LDS cap; one short of square at the cap: the largest launch there is (76 * 1024 + 60 * 1023 = 139 204 B)
SHAPES = [(1, 1), (1, 4), (4, 1), (2, 3), (3, 2), (63, 64), (64, 65), (65, 64), (60, 100), (100, 60), (256, 257), (257, 256), (1, 1024), (1024, 1),
          (900, 1024), (1023, 1024), (1024, 1023)]


@pytest.fixture(scope="module")
def d():
    import multiagent_planning_amd as mp
    ctx = mp.Dmpc("bound", c=asg.C_LATTICE)
    yield ctx
    ctx.close()


def test_the_shapes_reach_the_one_launch_boundary():
    assert ONE_MAX == 1024 and max(max(s) for s in SHAPES) == ONE_MAX


@pytest.mark.parametrize("N,M", SHAPES)
def test_device_equals_the_restatement_bit_for_bit(d, N, M):
    S = 3
    po, g = ar.lattice_batch(N, M, range(S))
    out = d.assign_rect(po, g, eps=ar.lattice_eps(N, M))
    assert out["perm"].shape == (S, N) and out["owner"].shape == (S, M) and out["price"].shape == (S, max(N, M)) and out["pf"].shape == (S, N, 3)
    for s in range(S):
        ref = ar.lattice_result(N, M, s)
        assert ref["rounds"] > 0 and (ref["rev"] > 0 or N == M)
        assert ar.same(out, ref, s) is None, (N, M, s, ar.same(out, ref, s), int(out["rounds"][s]), ref["rounds"])
        assert ar.consistent(po[s], {k: out[k][s] for k in out}, N, M)


@pytest.mark.parametrize("name", ["equal", "equalT", "zero", "zeroT", "grid", "gridT", "duplicates", "subsetT"])
def test_ties_everywhere_equal_the_restatement(d, name):
    po, g = ar.tie_scene(name)
    eps = 1e-4 / max(len(po), len(g))
    ref = ar.auction_rect(po, g, asg.C_LATTICE, eps)
    assert ref["rounds"] > 0
    out = d.assign_rect(po[None], g[None], eps=eps)
    assert ar.same(out, ref, 0) is None, ar.same(out, ref, 0)


@pytest.mark.parametrize("N", [3, 65, 300])
def test_square_scenes_equal_dmpc_assign_goals_bit_for_bit(d, N):
    sc = [asg.lattice(N, s) for s in range(2)]
    po, g = np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc])
    eps = asg.lattice_eps(N)
    sq, re_ = d.assign(po, g, eps=eps), d.assign_rect(po, g, eps=eps)
    assert (sq["rounds"] > 0).all()
    for k in sq:
        assert re_[k].tobytes() == sq[k].tobytes(), k
    for s in range(2):
        inv = np.empty(N, dtype=np.int32)
        inv[sq["perm"][s]] = np.arange(N)
        assert np.array_equal(re_["owner"][s], inv)


def _square_batch(N, seeds):
    sc = [asg.lattice(N, s) for s in seeds]
    return np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc])


@pytest.mark.parametrize("N", [1, 64, 257, ONE_MAX])
def test_square_scenes_equal_the_square_restatement_bit_for_bit(d, N):
    """N == M leaves the reverse-only columns out of LDS; against tests/assign.py, which knows no reverse round: one agent, a full wave, the
    256 -> 1024-thread switch, the cap"""
    po, g = _square_batch(N, range(2))
    out = d.assign_rect(po, g, eps=asg.lattice_eps(N))
    for s in range(2):
        ref = asg.lattice_result(N, s)
        assert ref["rounds"] > 0
        assert asg.same(out, ref, s) is None, (N, s, asg.same(out, ref, s), int(out["rounds"][s]), ref["rounds"])
        inv = np.empty(N, dtype=np.int32)
        inv[ref["perm"]] = np.arange(N)
        assert np.array_equal(out["owner"][s], inv)


def test_the_lds_limit_is_raised_whatever_the_order_of_the_calls():
    """both entries share one limit per instantiation of the kernel: on a fresh context every launch is larger or smaller than what was set before"""
    import multiagent_planning_amd as mp
    ctx = mp.Dmpc("bound", c=asg.C_LATTICE)
    try:
        for N, M in ((900, 1024), (3, None), (ONE_MAX, None), (100, 60), (1024, 1023), (300, None)):
            if M is None:
                po, g = asg.lattice(N)
                assert asg.same(ctx.assign(po[None], g[None], eps=asg.lattice_eps(N)), asg.lattice_result(N), 0) is None, N
            else:
                po, g = ar.lattice_batch(N, M, [0])
                assert ar.same(ctx.assign_rect(po, g, eps=ar.lattice_eps(N, M)), ar.lattice_result(N, M), 0) is None, (N, M)
    finally:
        ctx.close()


def test_round_cap_on_a_square_scene_is_the_same_through_both_entries(d):
    """a cap of exactly the rounds the first scene needs, next to a scene that needs many more"""
    N = 64
    ex, lat, eps = asg.exchange(N), asg.lattice(N), asg.lattice_eps(N)
    cap = asg.auction(ex[0], ex[1], asg.C_LATTICE, eps)["rounds"]
    assert 0 < cap < 16 and asg.lattice_result(N)["rounds"] > cap
    po, g = np.stack([ex[0], lat[0]]), np.stack([ex[1], lat[1]])
    sq, re_ = d.assign(po, g, eps=eps, max_rounds=cap), d.assign_rect(po, g, eps=eps, max_rounds=cap)
    for k in sq:
        assert re_[k].tobytes() == sq[k].tobytes(), k
    for out in (sq, re_):
        assert out["rounds"][0] == cap and sorted(out["perm"][0].tolist()) == list(range(N))
        assert out["rounds"][1] == -1 and (out["perm"][1] == -1).all() and np.isnan(out["cost"][1]) and not out["pf"][1].any()
        assert out["price"][1].tobytes() == asg.auction(lat[0], lat[1], asg.C_LATTICE, eps, max_rounds=cap)["price"].tobytes()
    assert (re_["owner"][1] == -1).all() and sorted(re_["owner"][0].tolist()) == list(range(N))


@pytest.mark.parametrize("N,M", [(60, 100), (100, 60)])
def test_a_scene_does_not_depend_on_its_batch(d, N, M):
    po, g = ar.lattice_batch(N, M, range(3))
    eps = ar.lattice_eps(N, M)
    both = d.assign_rect(po, g, eps=eps)
    alone = d.assign_rect(po[1:2], g[1:2], eps=eps)
    for k in both:
        assert both[k][1].tobytes() == alone[k][0].tobytes(), k
    assert len({int(r) for r in both["rounds"]}) > 1        # (next to scenes that run for another number of rounds)


@pytest.mark.parametrize("N,M", [(12, 20), (20, 12)])
@pytest.mark.parametrize("kind", ["f", "r"])
def test_round_cap_stops_one_scene_and_leaves_the_other(d, N, M, kind):
    """max_rounds one below what a scene needs -- its last round a forward one or a reverse one, by the restatement -- next to a scene that finishes"""
    res = [ar.lattice_result(N, M, s) for s in range(8)]
    hit = next(s for s in range(8) if res[s]["kinds"][-1] == kind)
    cap = res[hit]["rounds"] - 1
    short = next(s for s in range(8) if res[s]["rounds"] <= cap)
    eps = ar.lattice_eps(N, M)
    po, g = ar.lattice_batch(N, M, (short, hit))
    capped = ar.auction_rect(po[1], g[1], asg.C_LATTICE, eps, max_rounds=cap)
    assert capped["rounds"] == -1 and capped["kinds"] == res[hit]["kinds"][:-1]
    out = d.assign_rect(po, g, eps=eps, max_rounds=cap)
    assert ar.same(out, res[short], 0) is None
    assert out["rounds"][1] == -1 and (out["perm"][1] == -1).all() and (out["owner"][1] == -1).all() and np.isnan(out["cost"][1])
    assert not out["pf"][1].any()
    assert out["price"][1].tobytes() == capped["price"].tobytes()
    # exactly as many rounds as the scene needs are enough
    assert ar.same(d.assign_rect(po[1:], g[1:], eps=eps, max_rounds=cap + 1), res[hit], 0) is None


@pytest.mark.parametrize("N,M", [(65, 64), (60, 100)])
def test_device_form_equals_the_host_form(d, N, M):
    import torch
    po, g = ar.lattice_batch(N, M, range(2))
    eps = ar.lattice_eps(N, M)
    host = d.assign_rect(po, g, eps=eps)
    dev = torch.device("cuda")
    tpo, tg = torch.from_numpy(po).to(dev), torch.from_numpy(g).to(dev)
    t = dict(perm=torch.full((2, N), -7, dtype=torch.int32, device=dev), owner=torch.full((2, M), -7, dtype=torch.int32, device=dev),
             pf=torch.zeros((2, N, 3), dtype=torch.float64, device=dev), price=torch.zeros((2, max(N, M)), dtype=torch.float64, device=dev),
             cost=torch.zeros((2,), dtype=torch.float64, device=dev), rounds=torch.full((2,), -7, dtype=torch.int32, device=dev))
    st = torch.cuda.current_stream().cuda_stream
    d.assign_rect_device(2, N, M, tpo.data_ptr(), tg.data_ptr(), eps, 0, stream=st, **{k: v.data_ptr() for k, v in t.items()})
    torch.cuda.synchronize()
    for k, v in t.items():
        assert v.cpu().numpy().tobytes() == host[k].tobytes(), k
    # outputs are optional
    t["owner"].fill_(-7)
    d.assign_rect_device(2, N, M, tpo.data_ptr(), tg.data_ptr(), eps, 0, owner=t["owner"].data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert t["owner"].cpu().numpy().tobytes() == host["owner"].tobytes()


def test_context_precision_does_not_change_a_bit(d):
    import multiagent_planning_amd as mp
    po, g = ar.lattice_batch(60, 100, range(2))
    want = d.assign_rect(po, g)
    m = mp.Dmpc("bound", precision="mixed", c=asg.C_LATTICE)
    try:
        got = m.assign_rect(po, g)
    finally:
        m.close()
    assert (want["rounds"] > 0).all()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_refusals_launch_nothing_and_leave_the_next_call_correct(d):
    po, g = ar.lattice_batch(3, 5, [0])
    bad = [(0, 3, 5, po, g, 1e-3), (-1, 3, 5, po, g, 1e-3), (1, 0, 5, po, g, 1e-3), (1, 3, 0, po, g, 1e-3), (1, -2, 5, po, g, 1e-3),
           (1, 3, 5, None, g, 1e-3), (1, 3, 5, po, None, 1e-3), (1, 3, 5, po, g, 0.0), (1, 3, 5, po, g, -1e-3), (1, 3, 5, po, g, float("nan")),
           (1, 3, 5, po, g, float("inf"))]
    for S, N, M, a, b, eps in bad:
        rc, msg, out = ar.raw_assign_rect(d, S, N, M, a, b, eps)
        assert rc == -1 and msg.startswith("dmpc_assign_rect: "), (S, N, M, eps, rc, msg)
        assert not any(v.any() for v in out.values()), (S, N, M, eps)      # nothing was written
    big = np.zeros((1, ONE_MAX + 1, 3))
    for N, M, a, b in ((3, ONE_MAX + 1, po, big), (ONE_MAX + 1, 5, big, g), (ONE_MAX + 1, ONE_MAX + 1, big, big)):
        rc, msg, out = ar.raw_assign_rect(d, 1, N, M, a, b, 1e-3)
        assert rc == -1 and msg.startswith("dmpc_assign_rect: ") and re.search(rf"\b{N}\b", msg) and re.search(rf"\b{M}\b", msg), msg
        assert not any(v.any() for v in out.values())
    import torch
    with pytest.raises(RuntimeError, match="^dmpc_assign_rect_device: "):
        d.assign_rect_device(1, 3, ONE_MAX + 1, 0, 0, 1e-3)
    with pytest.raises(RuntimeError, match="^dmpc_assign_rect_device: "):
        d.assign_rect_device(1, 3, 5, torch.zeros(9, dtype=torch.float64, device="cuda").data_ptr(), 0, 1e-3)
    eps = ar.lattice_eps(3, 5)
    rc, _, out = ar.raw_assign_rect(d, 1, 3, 5, po, g, eps)
    assert rc == 0 and ar.same(out, ar.lattice_result(3, 5), 0) is None
    with pytest.raises(RuntimeError, match="assign: "):     # assign() keeps refusing unequal shapes
        d.assign(po, g)


# ---- transition() and mission() ----------------------------------------------------------------------------------------------------------
def _rows(z, y, xs):
    return np.array([(x, y, z) for x in xs], dtype=np.float64)


FLEET6 = np.concatenate([_rows(1.0, -0.5, (-1.0, 0.0, 1.0)), _rows(1.0, 0.5, (-1.0, 0.0, 1.0))])      # a small lattice, 1 m apart
SPOTS4 = _rows(1.5, 1.5, (-1.5, -0.5, 0.5, 1.5))
KT, TOL = 60, 0.01


@pytest.mark.parametrize("po,goals", [(FLEET6, SPOTS4), (SPOTS4, FLEET6)], ids=["6_agents_4_goals", "4_agents_6_goals"])
def test_transition_with_rect_assignment(d, po, goals):
    import multiagent_planning_amd as mp
    N, M = len(po), len(goals)
    ref = ar.auction_rect(po, goals, asg.C_LATTICE, 1e-4 / max(N, M))
    out = d.transition(po[None], goals[None], KT, TOL, assign="rect")
    assert np.array_equal(out["perm"][0], ref["perm"]) and np.array_equal(out["owner"][0], ref["owner"])
    assert (out["perm"][0] >= 0).sum() == min(N, M) and (out["owner"][0] == -1).sum() == max(M - N, 0)
    a = d.assign_rect(po[None], goals[None])
    assert a["pf"][0].tobytes() == ref["pf"].tobytes()
    plain = d.transition(po[None], a["pf"], KT, TOL)
    assert sorted(out) == sorted(list(plain) + ["perm", "owner"])
    for k in plain:
        assert out[k].tobytes() == plain[k].tobytes(), k
    used = int(out["K_T_used"][0])
    assert out["scene_status"][0] == (mp.ST_SOLVED | mp.ST_REACHED) and 1 < used <= KT
    end = out["pk"][0][:, used - 1]
    assert np.abs(end - ref["pf"]).max() < TOL                    # the chosen agents arrive ...
    stay = ref["perm"] < 0
    assert stay.sum() == max(N - M, 0) and (np.abs(end[stay] - po[stay]).max() < TOL if stay.any() else True)   # ... the others end where they began


def test_transition_refuses_another_assign_value(d):
    import multiagent_planning_amd as mp
    for bad in ("square", "Rect", 2, None):
        with pytest.raises(mp.DmpcError, match="transition: assign"):
            d.transition(FLEET6[None], SPOTS4[None], 4, assign=bad)
        with pytest.raises(mp.DmpcError, match="mission: assign"):
            d.mission(FLEET6[None], SPOTS4[None, None], 4, assign=bad)


def test_mission_with_rect_assignment_chains_the_stages(d):
    po = FLEET6[None]
    goals = np.stack([SPOTS4, _rows(1.0, -1.5, (-1.5, -0.5, 0.5, 1.5))])[None]      # [S,Q,M,3]: two stages of 4 goals for 6 agents
    a1 = d.assign_rect(po, goals[:, 0])
    a2 = d.assign_rect(a1["pf"], goals[:, 1])
    out = d.mission(po, goals, 6, assign="rect")
    assert out["perm"].shape == (1, 2, 6) and out["owner"].shape == (1, 2, 4)
    assert np.array_equal(out["perm"][:, 0], a1["perm"]) and np.array_equal(out["perm"][:, 1], a2["perm"])
    assert np.array_equal(out["owner"][:, 0], a1["owner"]) and np.array_equal(out["owner"][:, 1], a2["owner"])
    # an agent without a goal in a stage keeps its previous target (po in stage 0)
    idle1, idle2 = a1["perm"][0] < 0, a2["perm"][0] < 0
    assert idle1.sum() == idle2.sum() == 2
    assert a1["pf"][0][idle1].tobytes() == po[0][idle1].tobytes() and a2["pf"][0][idle2].tobytes() == a1["pf"][0][idle2].tobytes()
    flown = d.mission(po, np.stack([a1["pf"], a2["pf"]], axis=1), 6)
    assert sorted(out) == sorted(list(flown) + ["perm", "owner"])
    for k in flown:
        assert out[k].tobytes() == flown[k].tobytes(), k


def test_assign_true_on_a_square_scene_returns_what_it_returned_before(d):
    po, pf = d.random_exchange(1, 12, PMIN, PMAX, RMIN, 9)
    out = d.transition(po, pf, 8, assign=True)
    a = d.assign(po, pf)
    plain = d.transition(po, a["pf"], 8)
    assert sorted(out) == sorted(list(plain) + ["perm"]) and np.array_equal(out["perm"], a["perm"])
    for k in plain:
        assert out[k].tobytes() == plain[k].tobytes(), k
