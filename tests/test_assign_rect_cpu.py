"""CPU: the numpy restatement of the rectangular forward/reverse auction (tests/assign_rect.py) against the square restatement (tests/assign.py),
against scipy.optimize.linear_sum_assignment on the rectangular cost matrix, and against its own certificates.  Lattice scenes (points on a
0.25 m lattice, c = 2: every cost is a multiple of 1/64, every sum exact) at eps = 1/(128 max(N, M)): min(N, M) eps < 1/64, so a total within
min(N, M) eps of the optimum IS the optimum."""
import numpy as np
import pytest

import assign as asg
import assign_rect as ar

LATTICE = [(1, 4), (4, 1), (2, 3), (3, 2), (3, 5), (5, 3), (64, 65), (65, 64), (60, 100), (100, 60), (100, 200), (300, 1000), (1000, 300)]
TIES = ["equal", "duplicates", "subset", "subsetT", "grid", "gridT"]


@pytest.mark.parametrize("N", (1, 2, 3, 65))
def test_square_scenes_equal_the_square_restatement_bit_for_bit(N):
    po, g = asg.lattice(N)
    want = asg.lattice_result(N)
    got = ar.auction_rect(po, g, asg.C_LATTICE, asg.lattice_eps(N))
    assert asg.same(got, want) is None, asg.same(got, want)
    assert got["rev"] == 0 and got["fwd"] == want["rounds"]
    inv = np.empty(N, dtype=np.int32)
    inv[got["perm"]] = np.arange(N)
    assert np.array_equal(got["owner"], inv)


@pytest.mark.parametrize("N,M", LATTICE)
def test_lattice_scene_is_solved_to_the_rectangular_optimum(N, M):
    po, g = ar.lattice(N, M)
    r = ar.lattice_result(N, M)
    print(f"{N} x {M}: rounds {r['rounds']} = {r['fwd']} forward + {r['rev']} reverse")
    assert r["rounds"] == r["fwd"] + r["rev"] > 0 and r["rev"] > 0
    assert ar.consistent(po, r, N, M)
    assert r["cost"] == ar.optimum_rect(po, g, asg.C_LATTICE)
    assert r["price"].shape == (max(N, M),)
    assert np.array_equal(r["pf"][r["perm"] >= 0], g[r["perm"][r["perm"] >= 0]])


@pytest.mark.parametrize("seed", range(12))
def test_uniform_scenes_carry_the_certificate(seed):
    """every person's object is within eps of its best in c + price, and no unowned object is priced above an owned one.  Rounding allowance:
    a slack is the difference of two sums c + price of magnitude at most cmax + max price, each rounded once, and u is carried through at most
    `rounds` subtractions of the same magnitude: (4 + rounds) ulps of that magnitude, 2^-52 each, bounds both."""
    rng = np.random.default_rng(400 + seed)
    n, m = int(rng.integers(1, 41)), int(rng.integers(1, 61))
    n, m = min(n, m), max(n, m)
    N, M = (n, m) if seed % 2 == 0 else (m, n)
    po, g = ar.uniform(N, M, seed)
    eps = 1e-6
    r = ar.auction_rect(po, g, 2.0, eps)
    assert r["rounds"] > 0 and ar.consistent(po, r, N, M)
    sl, over, cmax = ar.certificate(po, g, 2.0, r)
    allow = (4 + r["rounds"]) * 2.0 ** -52 * max(1.0, cmax + r["price"].max())
    print(f"{N} x {M}: rounds {r['rounds']}, slack - eps = {sl - eps:.3e}, unowned - owned = {over:.3e}, allowance {allow:.3e}")
    assert sl <= eps + allow
    assert over <= allow
    assert r["cost"] <= ar.optimum_rect(po, g, 2.0) + n * eps + allow


@pytest.mark.parametrize("name", TIES + ["equalT", "duplicatesT", "zero", "zeroT"])
def test_scenes_full_of_ties_terminate_within_the_default_cap(name):
    po, g = ar.tie_scene(name)
    N, M = len(po), len(g)
    r = ar.auction_rect(po, g, asg.C_LATTICE, 1e-4 / max(N, M))
    assert 0 < r["rounds"] < ar.DEFAULT_ROUNDS and ar.consistent(po, r, N, M)
    assert abs(r["cost"] - ar.optimum_rect(po, g, asg.C_LATTICE)) <= 1e-4
    if name.startswith(("equal", "zero")):
        assert r["cmax"] == 0.0 and r["cost"] == 0.0


def test_perm_and_owner_are_consistent_and_unassigned_agents_stay():
    for N, M in ((5, 3), (3, 5), (100, 60)):
        po, g = ar.lattice(N, M)
        r = ar.lattice_result(N, M)
        assert ar.consistent(po, r, N, M)
        assert (r["perm"] >= 0).sum() == min(N, M) == (r["owner"] >= 0).sum()
        for i in np.flatnonzero(r["perm"] >= 0):
            assert r["owner"][r["perm"][i]] == i
        assert np.array_equal(r["pf"][r["perm"] < 0], po[r["perm"] < 0])


def test_round_cap_reports_the_scene_as_unsolved_in_either_kind_of_round():
    po, g = ar.lattice(60, 100)
    full = ar.lattice_result(60, 100)
    eps = ar.lattice_eps(60, 100)
    for kind in "fr":
        k = full["kinds"].rindex(kind)            # the scene needs round k + 1, of this kind
        r = ar.auction_rect(po, g, asg.C_LATTICE, eps, max_rounds=k)
        assert r["rounds"] == -1 and (r["perm"] == -1).all() and (r["owner"] == -1).all() and np.isnan(r["cost"]) and not r["pf"].any()
        assert r["kinds"] == full["kinds"][:k]
    assert ar.same(ar.auction_rect(po, g, asg.C_LATTICE, eps, max_rounds=full["rounds"]), full) is None
