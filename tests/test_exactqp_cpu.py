"""CPU: the extended-precision minimiser of tests/exactqp.py on the oracle's own answers (no GPU), and its negative controls.

The helper is the reference of tests/test_gpu_exact.py; what is shown here is that it (1) resolves every solved agent of the recorded
congested scenes from the oracle's answer, within 1e-10 of it (measured worst 7e-13; 1e-10 is the margin for another host's BLAS),
(2) agrees with the MATLAB/quadprog record as closely as the oracle does, (3) finds the same x* from an answer 1e-7 off and reports
that distance, and (4) does not follow an answer that is a KKT point of the WRONG active set."""
import numpy as np
import pytest

from oracle import oracle as orc
from helpers import load_golden, step14_inputs
import certificates as cert
import exactqp as ex

CASES = [("failure_rate2_bound", "bound"), ("failure_rate2_bound", "cpp"), ("comp_kctr_3_bound2", "bound2"), ("comp_kctr_3_bound2", "cpp2")]
RECORDED = {("failure_rate2_bound", "bound"), ("comp_kctr_3_bound2", "bound2")}      # the variant the MATLAB record was produced by
_cache = {}


def _scene(name, variant):
    """oracle step and exact minimisers of a recorded scene at MPC step 14, computed once and shared (read-only)"""
    if (name, variant) not in _cache:
        g, kw = load_golden(name)
        sc = step14_inputs(g)
        prm = orc.make_params(variant, **kw)
        ref = orc.step(prm, *sc, nthreads=8)
        X, lam, res, cmp_ = ex.exact_batch(orc, prm, *sc, ref["a"], ref["status"], ref["info"][:, orc.I_TRIES])
        for v in (X, lam, res, cmp_, ref["a"]):
            v.setflags(write=False)
        _cache[(name, variant)] = (g, kw, sc, prm, ref, X, lam, res, cmp_)
    return _cache[(name, variant)]


@pytest.mark.parametrize("name,variant", CASES)
def test_oracle_answers_resolve_to_the_exact_minimiser(name, variant):
    g, kw, sc, prm, ref, X, lam, res, cmp_ = _scene(name, variant)
    ok = (ref["status"] & 1) == 1
    assert ok.sum() > 30 and np.array_equal(cmp_, ok)
    assert res[ok].all(), f"unresolved agents {np.where(ok & ~res)[0]}"
    e = np.abs(ref["a"][ok] - X[ok]).max(axis=1)
    print(f"{name}/{variant}: {int(ok.sum())} agents resolved, worst |a_oracle - x*| {e.max():.2e}, ladder levels up to "
          f"{int(ref['info'][ok, orc.I_TRIES].max())}, lam_max up to {lam[ok].max():.2e}")
    assert e.max() <= 1e-10
    if (name, variant) in RECORDED:
        # the MATLAB/quadprog record of the step (new_l: the positions of the horizon): x* is as close to it as the oracle's answer is
        l, xp, xv, xa, pf = sc
        Lam, Av, A0, Dl = orc.model_matrices(kw["h"], 15)
        nd = int(g["n_done"])
        p_star = X[:nd] @ Lam.T + np.hstack([xp[:nd], xv[:nd]]) @ A0.T
        e_star = np.abs(p_star - g["new_l"][:nd]).max(axis=1)
        e_orc = np.abs(ref["p"][:nd] - g["new_l"][:nd]).max(axis=1)
        assert np.abs(e_star - e_orc).max() <= 1e-10
        assert ((e_star <= 2e-6) == (e_orc <= 2e-6)).all() and (e_orc <= 2e-6).sum() >= int(0.75 * nd)


def _constrained_agent(name, variant):
    """an agent of the scene whose minimiser has active rows with multipliers well away from zero (the first such)"""
    g, kw, sc, prm, ref, X, lam, res, cmp_ = _scene(name, variant)
    l, xp, xv, xa, pf = sc
    for n in np.where(res & (lam > 1.0))[0]:
        qp = orc.assemble_one(prm, l, int(n), xp[n], xv[n], xa[n], pf[n], level=max(int(ref["info"][n, orc.I_TRIES]) - 1, 0))
        W = ex.working_set(qp, ref["a"][n])
        x, lm, singular = ex.kkt_point(qp, W)
        if not singular and len(W) >= 2 and lm.min() > 1e-3:
            return int(n), qp, W, lm, ref["a"][n], X[n]
    raise AssertionError("no constrained agent in the scene")


@pytest.mark.parametrize("name,variant", [("failure_rate2_bound", "bound"), ("comp_kctr_3_bound2", "cpp2")])
def test_an_answer_1e7_off_resolves_to_the_same_minimiser(name, variant):
    """negative control 1: the oracle's answer moved 1e-7 (2-norm) toward a = 0 -- a feasible direction: the acceleration box and the
    workspace are convex and hold a = 0 here (asserted), the slack rows are completed -- names the same working set: the helper returns
    the same x* and so reports the distance of the perturbed answer, 1e-7-ish, not zero"""
    n, qp, W, lm, a, xs = _constrained_agent(name, variant)
    u = -a / np.linalg.norm(a)
    a_off = a + 1e-7 * u
    assert (qp["C"] @ cert.complete_slack(qp, a_off) - qp["d"]).max() <= 1e-12, "the direction must be feasible"
    r = ex.exact_minimiser(qp, a_off)
    assert r["resolved"], r["why"]
    assert np.abs(r["x"] - xs).max() <= 1e-13
    dist = float(np.abs(a_off - r["x"]).max())
    want = float(np.abs(1e-7 * u).max())
    print(f"{name}/{variant} agent {n}: perturbed by {want:.3e} (l_inf), reported distance {dist:.3e}")
    assert abs(dist - want) <= 1e-10 and 1e-8 < dist <= 1e-7


@pytest.mark.parametrize("name,variant", [("failure_rate2_bound", "bound"), ("comp_kctr_3_bound2", "cpp2")])
def test_a_kkt_point_of_the_wrong_active_set_is_not_followed(name, variant):
    """negative control 2: the stationary point of the working set WITHOUT the row of largest multiplier among those that act on the
    accelerations (a solver that lost a constraint; a slack's own bound row would leave `a` where it is).  Either verdict is right:
    `unresolved`, or resolved at a distance above 1e-6.  What occurs on both scenes is UNRESOLVED: the dropped row is a collision row
    (multipliers 58.5 and 61.3); the candidate rows at the wrong point name a working set that is not the minimiser's, and its
    stationary point violates a row by about 2e2.  A wrong active set thus never yields an
    x* that vouches for the wrong answer; were it resolved, x* would be the true minimiser (asserted) and the distance would show."""
    n, qp, W, lm, a, xs = _constrained_agent(name, variant)
    on_a = np.abs(qp["C"][W, :45]).max(axis=1) > 0
    drop = int(np.argmax(np.where(on_a, lm, -1.0)))
    x_wrong, lm_wrong, singular = ex.kkt_point(qp, np.delete(W, drop))
    assert not singular
    r = ex.exact_minimiser(qp, x_wrong[:45])
    dist = float(np.abs(x_wrong[:45] - r["x"]).max()) if r["resolved"] else float("nan")
    print(f"{name}/{variant} agent {n}: row {int(W[drop])} (multiplier {lm[drop]:.3g}) dropped: " +
          (f"resolved, distance {dist:.3e}" if r["resolved"] else f"unresolved ({r['why']})"))
    assert (not r["resolved"]) or dist > 1e-6
    if r["resolved"]:
        assert np.abs(r["x"] - xs).max() <= 1e-13, "a resolved answer is THE minimiser, whatever the candidate was"


def test_a_dependent_working_set_is_unresolved():
    """the helper's `singular` verdict: a working set with a repeated row"""
    n, qp, W, lm, a, xs = _constrained_agent("failure_rate2_bound", "bound")
    x, lam, singular = ex.kkt_point(qp, np.r_[W, W[:1]])
    assert singular and x is None
