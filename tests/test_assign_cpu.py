"""CPU: the numpy restatement of the goal-assignment auction (tests/assign.py) against scipy.optimize.linear_sum_assignment and against its
own certificates.  Lattice scenes (points on a 0.25 m lattice, c = 2: every cost is a multiple of 1/64, every sum exact) at eps = 1/(128 N):
N eps < 1/64, so a total within N eps of the optimum IS the optimum."""
import numpy as np
import pytest

import assign as asg

LATTICE_N = (1, 2, 3, 64, 65, 300, 1100)


@pytest.mark.parametrize("N", LATTICE_N)
def test_lattice_scene_is_solved_to_the_optimum_with_its_certificates(N):
    po, g = asg.lattice(N)
    eps = asg.lattice_eps(N)
    r = asg.lattice_result(N)
    perm = r["perm"]
    assert sorted(perm.tolist()) == list(range(N))
    opt, _ = asg.optimum(po, g, asg.C_LATTICE)
    assert r["cost"] == opt
    sl, cmax = asg.slack(po, g, asg.C_LATTICE, perm, r["price"])
    print(f"N={N} rounds={r['rounds']} phases={r['phases']} worst slack - eps = {sl.max() - eps:.3e}")
    assert sl.max() <= eps + 1e-12 * max(1.0, cmax + r["price"].max())
    # the swap inequality (po_i - po_j)' E1^2 (g_perm[i] - g_perm[j]) >= 0, exact on the lattice
    e2 = np.array([1.0, 1.0, 1.0 / asg.C_LATTICE ** 2])
    a, b = po * e2, g[perm]
    G = a @ b.T                                   # G[i,j] = po_i' E1^2 g_perm[j]
    d = np.diag(G)
    assert ((d[:, None] + d[None, :]) - (G + G.T) >= 0).all()
    assert np.array_equal(r["pf"], g[perm]) and r["rounds"] > 0


@pytest.mark.parametrize("N", (100, 300))
def test_uniform_scene_is_within_n_eps_of_the_optimum(N):
    po, g = asg.uniform(N)
    eps = 1e-4 / N
    r = asg.auction(po, g, 2.0, eps)
    assert sorted(r["perm"].tolist()) == list(range(N))
    opt, _ = asg.optimum(po, g, 2.0)
    assert r["cost"] <= opt + N * eps


@pytest.mark.parametrize("N", (100, 300))
def test_exchange_scene_sends_every_agent_home_at_no_cost(N):
    po, g = asg.exchange(N)
    r = asg.auction(po, g, 2.0, 1e-4 / N)
    assert r["cost"] == 0.0 and np.array_equal(g[r["perm"]], po)


def test_round_cap_reports_the_scene_as_unsolved():
    po, g = asg.lattice(64)
    full = asg.lattice_result(64)
    r = asg.auction(po, g, asg.C_LATTICE, asg.lattice_eps(64), max_rounds=full["rounds"] - 1)
    assert r["rounds"] == -1 and (r["perm"] == -1).all() and np.isnan(r["cost"]) and not r["pf"].any()
    r = asg.auction(po, g, asg.C_LATTICE, asg.lattice_eps(64), max_rounds=full["rounds"])
    assert asg.same(r, full) is None
