"""The synthetic crowd scenes of tests/crowds.py against the oracle alone (no GPU): every probe has the row count, first violating
step and status the GPU capacity tests (tests/test_gpu_capacity.py) rely on."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
import crowds as cr

NT = min(os.cpu_count() or 1, 16)
KW = cr.solver_kw()


def _probe(variant, sc, kw=KW):
    l, xp, xv, xa, pf = sc
    return orc.rows_one(orc.make_params(variant, **kw), l, 0, xp[0], xv[0])


@pytest.mark.parametrize("variant,rows,kc", [(v, r, 10) for v in ("bound", "cpp") for r in (63, 64, 65)] +
                         [(v, r, 11) for v in ("bound2", "cpp2") for r in (63, 64, 65)] +
                         [("bound", 128, 10), ("bound", 129, 10), ("all3", 384, 10), ("all3", 387, 10), ("bound", 5, 10), ("bound", 9, 10)])
def test_soft_crowd_has_the_intended_rows(variant, rows, kc):
    sc = cr.soft_crowd(variant, rows, kc=kc)
    r = _probe(variant, sc)
    assert r["nrows"] == rows and r["viol_k"] == kc and r["status"] == 0, (r["nrows"], r["viol_k"], r["status"])
    l = sc[0].reshape(len(sc[0]), 15, 3)
    d1 = np.sqrt(((l[1:, 0] - l[0, 0]) ** 2 * [1, 1, 0.25]).sum(1))
    assert d1.min() >= KW["rmin"] - 0.05                   # nobody near the probe's first step: no ST_COLL
    dk = np.sqrt(((l[1:, kc - 1] - l[0, kc - 1]) ** 2 * [1, 1, 0.25]).sum(1))
    assert (dk < KW["rmin"]).sum() == 1                    # exactly one violator


@pytest.mark.parametrize("variant", ["bound", "bound2", "cpp", "cpp2"])
def test_ladder_crowd_climbs(variant):
    """the 64-row probe of the ladder test: the oracle's solve needs at least three tries (ladder levels)"""
    sc = cr.ladder_crowd(variant, 64)
    ref = orc.solve_one(orc.make_params(variant, **KW), sc[0], 0, sc[1][0], sc[2][0], sc[3][0], sc[4][0])
    assert ref["status"] & 1 and ref["info"][orc.I_NROWS] == 64 and ref["info"][orc.I_TRIES] >= 3, ref["info"]


@pytest.mark.parametrize("pairs", [640, 641, 767, 768, 769, 1024, 1025, 2049])
def test_hard_crowd_has_the_intended_rows(pairs):
    sc = cr.hard_crowd(pairs)
    r = _probe("hard", sc)
    assert r["nrows"] == pairs and r["status"] == 0
    l = sc[0].reshape(len(sc[0]), 15, 3)
    d = np.sqrt(((l[1:] - l[:1]) ** 2 * [1, 1, 0.25]).sum(2))
    assert d.min() >= KW["rmin"]                           # feasible: the probe's prediction satisfies every hard row
    assert (d < 1).sum() == pairs and (d[:, :9] < 1).sum() == 0


@pytest.mark.parametrize("fourth", [False, True], ids=["three", "four"])
def test_corner_probe_has_three_hard_rows_and_three_walls(fourth):
    """crowds.corner_hard_rows, from the oracle's answer and the solver-independent working set of tests/exactqp.py: the probe's minimiser
    has exactly three collision rows active (|C a - d| <= 1e-9) with their slack at zero -- the row AND its slack's bound eps <= 0 are in
    the working set, so eps = 0 exactly at x* --, all on step kc = 6, and three walls at the last step.  The oracle's active-set count
    is 9 (four neighbours: 10): the three rows, the three walls and the bound eps <= 0 of EVERY slack, which the dense QP carries as
    a row of its own (multiplier 5e4 minus the row's share) -- the six constraints that act on the accelerations are counted apart.
    With the fourth neighbour its row (index 2) is one of the three and the first neighbour's row (index 0) is inactive."""
    import certificates as cert
    import exactqp as ex
    kw, sc = cr.corner_hard_rows(fourth)
    l, xp, xv, xa, pf = sc
    prm = orc.make_params("bound", **kw)
    ref = orc.solve_one(prm, l, 0, xp[0], xv[0], xa[0], pf[0])
    nrows = 4 if fourth else 3
    assert ref["status"] == 1 and ref["info"][orc.I_VIOLK] == cr.CORNER_KC and ref["info"][orc.I_NROWS] == nrows and ref["info"][orc.I_TRIES] == 1
    qp = orc.assemble_one(prm, l, 0, xp[0], xv[0], xa[0], pf[0])
    nc = qp["ncoll"]
    assert nc == nrows
    x = cert.complete_slack(qp, ref["a"])
    r = qp["C"] @ x - qp["d"]
    active = [i for i in range(nc) if abs(r[i]) <= 1e-9]
    assert active == ([1, 2, 3] if fourth else [0, 1, 2]) and np.abs(x[45:]).max() <= 1e-15
    W = ex.working_set(qp, ref["a"]).tolist()
    eps_ub = nc + 4 * 45                                     # the rows eps_i <= 0 (certificates.complete_slack)
    assert all(i in W and eps_ub + i in W for i in active)   # hard: the row holds with its slack pinned at zero
    on_a = [w for w in W if np.abs(qp["C"][w, :45]).max() > 0]
    p = ref["p"].reshape(15, 3)
    walls = np.abs(p - np.array(kw["pmax"])) < 1e-9
    assert walls.sum() == 3 and walls[14].all()
    assert len(on_a) == 6 and ref["info"][orc.I_NACTIVE] == 6 + nc
    e = ex.exact_minimiser(qp, ref["a"])
    assert e["resolved"] and np.abs(e["x"] - ref["a"]).max() <= 1e-10 and 100 < e["lam_max"] <= 5e4


def test_row_capacity_restated():
    """the capacity the GPU tests assume (row_capacity in dmpc_launch.hip): per-variant want/cap, at least 8, rounded up to even"""
    row_capacity = cr.row_capacity
    assert [row_capacity("bound", n) for n in (2, 6, 9, 10, 129, 130, 5000)] == [8, 8, 8, 10, 128, 128, 128]
    assert [row_capacity("all3", n) for n in (3, 4, 128, 129, 130)] == [8, 10, 382, 384, 384]
    assert [row_capacity("hard", n) for n in (2, 4, 43, 44)] == [16, 46, 630, 640]
    assert [row_capacity("softall", n) for n in (6, 4097, 4098)] == [8, 4096, 4096]
    assert row_capacity("scp", 274) == 4096 and 15 * 273 <= 4096 < 15 * 274


@pytest.mark.parametrize("c", [2.0, 1.5])
@pytest.mark.parametrize("axis", ["x", "z"])
def test_ties_are_strict_in_the_oracle(axis, c):
    """a neighbour exactly on a threshold is not inside it; one ulp below it is (`<` everywhere in the reference)"""
    kw = cr.solver_kw(c=c)
    rmin = kw["rmin"]
    for kind, variant, expect in (("rmin", "bound", lambda r: r["viol_k"] == 5), ("3rmin", "bound", lambda r: r["nrows"] == 2),
                                  ("hard1", "hard", lambda r: r["nrows"] == 11), ("cut", "bound", lambda r: r["status"] == 4),
                                  ("cpp", "cpp", lambda r: r["nrows"] == 2)):
        t = cr.threshold(kind, rmin)
        for d, inside in ((np.nextafter(t, 0.0), True), (t, False), (np.nextafter(t, 9.0), False)):
            r = _probe(variant, cr.tie_scene(kind, d, axis, c=c), kw)
            if axis == "x" or c == 2.0:
                assert expect(r) == inside, (kind, d, r["nrows"], r["viol_k"], r["status"])
            else:   # (z at c = 1.5: the offset d * c rounds, and (d * c) * (1/c) lands within an ulp of d -- on either side of t)
                dz = (d * c) * (1.0 / c)
                assert expect(r) == (dz < t), (kind, d, dz, r["nrows"], r["viol_k"], r["status"])
