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


def test_row_capacity_restated():
    """the capacity the GPU tests assume (dmpc_api.hip row_capacity): per-variant want/cap, at least 8, rounded up to even"""
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
