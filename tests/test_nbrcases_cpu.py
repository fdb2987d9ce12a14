"""CPU: the adversarial neighbour-filter scenes of tests/nbrcases.py are what they claim to be (fp64 numpy), and the oracle alone solves them.

Every fact a GPU test of tests/test_gpu_nbr_adversarial.py relies on is asserted here, so that test cannot pass on an input that misses its point."""
import functools

import numpy as np
import pytest

import nbrcases as nc
from oracle import oracle as orc


@functools.lru_cache(maxsize=None)
def _case(name, hard=False):
    return nc.CASES[name](hard)


@functools.lru_cache(maxsize=None)
def _oracle(name, variant="bound"):
    kw, l, xp, xv, xa, pf, _ = _case(name, variant == "hard")
    prm = orc.make_params(variant, **kw)
    return [orc.step(prm, l[s], xp[s], xv[s], xa[s], pf[s], nthreads=8) for s in range(l.shape[0])]


@pytest.mark.parametrize("name", list(nc.CASES))
def test_states_are_inside_and_separated_and_the_oracle_solves_the_case(name):
    kw, l, xp, xv, xa, pf, facts = _case(name)
    assert l.shape[0] <= 3 and l.shape[0] * l.shape[1] <= 600
    assert facts["inside"] and facts["separation"] > kw["rmin"], facts["separation"]
    assert np.isfinite(l).all()
    for s, o in enumerate(_oracle(name)):
        solved = (o["status"] & orc.ST_SOLVED) != 0
        print(name, s, "solved", solved.mean(), "with rows", int((o["info"][:, orc.I_NROWS] > 0).sum()), "coll", int(((o["status"] & orc.ST_COLL) != 0).sum()))
        assert solved.mean() >= 0.25, (name, s)
        assert (o["info"][:, orc.I_NROWS] > 0).any(), (name, s)
        # the cases with pairs deep inside rmin at step 0 trip the collision outcome of solveSoftDMPCbound, the others never
        d0 = nc.distances(l[s], kw["c"])[0]
        deep = d0.min(axis=1) < kw["rmin"] - 0.05
        assert deep.any() == (name in nc.COLLIDING), name
        assert np.array_equal((o["status"] & orc.ST_COLL) != 0, deep), name


@pytest.mark.parametrize("N", nc.ROUND_SIZES)
def test_rounds_every_query_is_one_run_of_all_entries(N):
    kw, l, *_, facts = _case(f"rounds-{N}")
    assert l.shape[1] == N
    assert tuple(facts["n"][1:]) == (1, 1) and facts["n"][0] > 1
    for tot, rows in zip(facts["tot"], facts["rows"]):
        assert (tot == N).all() and (rows == 1).all()


def test_many_runs_reach_more_than_64_cell_rows_with_the_oversize_agent_and_a_few_without():
    for name, big in (("many_runs-oversize", True), ("many_runs-plain", False)):
        kw, l, *_, facts = _case(name)
        assert facts["n"][1] >= 13 and facts["n"][2] >= 13
        for s, rows in enumerate(facts["rows"]):
            print(name, s, "cell rows in reach", rows.min(), rows.max())
            assert (rows > 64).all() if big else (rows.max() <= 25 and rows.min() >= 4)
        _planted_triples(name, kw, l, facts["planted"])


def _planted_triples(name, kw, l, trip):
    """most planted triples are the first violation of their agent a: b inside rmin and n inside 3 rmin at that step"""
    for s in range(l.shape[0]):
        d = nc.distances(l[s], kw["c"])
        fv = nc.first_violation(d, kw["rmin"])
        good = 0
        for a, b, n in trip:
            k = fv[a]
            good += int(k < nc.K and d[k, a, b] < kw["rmin"] and kw["rmin"] < d[k, a, n] < 3 * kw["rmin"])
        print(name, s, "clean planted triples", good, "of", len(trip))
        assert good >= len(trip) // 2


def test_curved_pairs_meet_far_from_their_chords():
    kw, l, xp, *_, facts = _case("curved")
    rmin, rs = kw["rmin"], nc.rsel_of(kw)
    for s, pairs in enumerate(facts["pairs"]):
        assert len(pairs) == facts["nplan"]
        d = nc.distances(l[s], kw["c"])
        p = nc.steps_of(l[s]).copy(); p[..., 2] /= kw["c"]
        for a, b, kind, ks in pairs:
            dab = d[:, a, b]
            others = np.setdiff1d(np.arange(nc.K), ks)
            assert (dab[list(ks)] <= 0.5 * rmin + 1e-12).all() and (dab[others] >= 2 * rs).all(), (s, a, b, kind, dab)
            if kind == "a":   # chords (segment end points) at least 3 m apart at every time, the meeting 1.5 m or more off both
                for sg in range(nc.NSEG):
                    e0, e1 = nc.SEG * sg, nc.SEG * sg + nc.SEG - 1
                    for t in np.linspace(0, 1, 9):
                        ca, cb = p[a, e0] + t * (p[a, e1] - p[a, e0]), p[b, e0] + t * (p[b, e1] - p[b, e0])
                        assert np.linalg.norm(ca - cb) >= 3.0
        # the zig-zags and walks do leave their chords: most agents by more than half a metre
        dev = np.zeros(l.shape[1])
        for sg in range(nc.NSEG):
            q = p[:, nc.SEG * sg:nc.SEG * sg + nc.SEG]
            t = (np.arange(nc.SEG) / (nc.SEG - 1))[None, :, None]
            dev = np.maximum(dev, np.linalg.norm(q - (q[:, :1] + t * (q[:, -1:] - q[:, :1])), axis=2).max(axis=1))
        assert np.median(dev) > 0.5 and dev.max() <= 4.0
    # step 0 pairs: a collision for solveSoftDMPCbound
    for s, o in enumerate(_oracle("curved")):
        for a, b, kind, ks in facts["pairs"][s]:
            if ks == (0,):
                assert o["status"][a] & orc.ST_COLL and o["status"][b] & orc.ST_COLL


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("place", nc.PLACEMENTS)
def test_threshold_pairs_sit_on_their_side_of_the_radius(place, hard):
    kw, l, xp, *_, facts = _case(f"threshold-{place}", hard)
    rs = facts["rsel"]
    assert rs == (1.0 if hard else 3 * kw["rmin"])
    q = facts["site"].copy(); q[:, 2] /= kw["c"]
    dd = np.sqrt(((q[:, None] - q[None]) ** 2).sum(-1)); np.fill_diagonal(dd, np.inf)
    assert dd.min() > 2 * rs
    if place == "far":
        assert min(kw["pmin"][:2]) >= 200.0
    for s in (0, 1):
        d = nc.distances(l[s], kw["c"])
        count = {}
        for A, B, k, dl, sg, radius in facts["planted"][s]:
            dist = d[k, A, B]
            assert (dist < radius) == (sg < 0), (s, A, B, dist, radius)
            assert abs(dist / radius - 1.0 - sg * dl) <= 0.05 * dl + 1e-12, (s, A, B, dl, dist / radius - 1.0)   # 1e-12: the fp64 rounding of a 200 m coordinate, 1e-5 of the smallest delta
            assert d[:, A, B].argmin() == k and (np.delete(d[:, A, B], k) > 2 * rs).all()
            count[(dl, sg)] = count.get((dl, sg), 0) + 1
            if s == 0:    # the agent at the site has its violation at that step
                assert nc.first_violation(d, kw["rmin"])[A] == k
        assert len(count) == 2 * len(nc.DELTAS) and all(v == 10 for v in count.values()), count
    if place == "corner":   # the planted agents are the ones nearest the far corner
        off = np.abs(facts["site"] - np.array(kw["pmax"])).max(axis=1)
        assert off[0] < 6.0 and off[:150].mean() < off[150:].mean()   # (the top lattice layer is 5.7 m below the ceiling)


def test_still_tables_do_not_move():
    kw, l, *_, facts = _case("still")
    lv = nc.steps_of(l)
    assert (lv[0] == lv[0][:, :1]).all()
    moving = (lv[1] != lv[1][:, :1]).any(axis=(1, 2))
    assert not moving[0::2].any() and moving[1::2].sum() >= 120
    for s in range(2):
        d = nc.distances(l[s], kw["c"])
        for t, (a, b, n) in enumerate(facts["trip"]):
            assert np.allclose(d[:, a, b], (0.9 if t < 10 else 0.5) * kw["rmin"], rtol=1e-9) and np.allclose(d[:, a, n], 2.5 * kw["rmin"], rtol=1e-9)
    clean = [0, 0]
    for s, o in enumerate(_oracle("still")):
        for t, (a, b, n) in enumerate(facts["trip"]):
            if t >= 10:
                assert o["status"][a] & orc.ST_COLL, (s, t)
            elif not o["status"][a] & orc.ST_COLL:   # (another triple's table may rest next to a: then a collides as well)
                clean[s] += 1
                assert o["info"][a, orc.I_VIOLK] == 1 and o["info"][a, orc.I_NROWS] >= 2
    assert min(clean) >= 6, clean


def test_outside_tables_leave_the_workspace():
    kw, l, xp, *_, facts = _case("outside")
    pmin, pmax = np.array(kw["pmin"]), np.array(kw["pmax"])
    lv = nc.steps_of(l)
    for s in range(l.shape[0]):
        d = nc.distances(l[s], kw["c"])
        axes = set()
        for i, ax in facts["leavers"]:
            exc = max((lv[s, i, :, ax] - pmax[ax]).max(), (pmin[ax] - lv[s, i, :, ax]).max())
            assert 0.9 <= exc <= 10.5, (i, exc)
            axes.add((ax, bool((lv[s, i, :, ax] > pmax[ax]).any())))
        assert len(facts["leavers"]) == 40 and len(axes) == 6
        for a, b in facts["met"]:
            out = ((lv[s, a, 10:] > pmax) | (lv[s, a, 10:] < pmin)).any(axis=1)
            assert out.all() and (d[10:, a, b] < kw["rmin"]).all()
        assert len(facts["met"]) == 10
        for a, b, k, ax in facts["straddle"]:
            ina = ((lv[s, a, k] >= pmin) & (lv[s, a, k] <= pmax)).all(); inb = ((lv[s, b, k] >= pmin) & (lv[s, b, k] <= pmax)).all()
            assert ina and not inb and d[k, a, b] < kw["rmin"]


@pytest.mark.parametrize("which", range(len(nc.METRICS)))
def test_metric_grids_hit_the_cap_and_the_single_cell(which):
    kw, l, *_, facts = _case(f"metric-{which}")
    n = facts["n"]
    print(which, "cells", n)
    if which == 0:
        assert n[0] == 32 and n[2] > 1
    else:
        assert n[2] == 1 and n[0] > 1
    if which < 2:
        _planted_triples(f"metric-{which}", kw, l, facts["planted"])
    else:   # rmin = 0.9: most agents violate on their own, and every one is solved on the first level of the retry ladder (the oracle leg's 1e-9 is the first level's tolerance)
        for variant in ("bound", "ondemand", "cpp"):
            for o in _oracle("metric-2", variant):
                assert (o["info"][:, orc.I_NROWS] > 0).sum() >= 200 and o["info"][:, orc.I_TRIES].max() <= 1, variant


def test_close_edge_counts_are_at_the_capacity():
    kw, l, *_, facts = _case("close_edge")
    X, Y = facts["hubs"]
    W, Wn, Wk = facts["single"]
    rmin = kw["rmin"]
    assert X == 7 and Y == 40
    for s, cnt in enumerate(nc.CLOSE_COUNTS):
        d = nc.distances(l[s], kw["c"])
        inside = d < rmin
        per_seg = lambda hub: [int(inside[nc.SEG * g:nc.SEG * g + nc.SEG, hub, :].sum()) for g in range(nc.NSEG)]
        assert inside[:, X, :].sum() == cnt and sum(per_seg(X)) == cnt
        assert per_seg(X)[2] == 20 and min(per_seg(X)[:2]) > 20           # the fifth neighbour's steps lie in two segments
        assert per_seg(Y) == [21, 21, 22]
        assert inside[:, W, :].sum() == 1 and inside[Wk, W, Wn]
        hubs = d[:, [X, Y, W], :]
        assert (np.abs(hubs[np.isfinite(hubs)] / rmin - 1.0) >= 0.3).all()       # every distance of a hub 0.3 rmin or more off the radius ...
        assert (np.abs(d[np.isfinite(d)] / rmin - 1.0) >= 0.05).all()            # ... and nothing in the scene near it
    for o in _oracle("close_edge"):
        assert o["status"][X] & orc.ST_COLL and o["status"][Y] & orc.ST_COLL
        assert o["status"][W] == orc.ST_SOLVED and o["info"][W, orc.I_VIOLK] == Wk + 1 and o["info"][W, orc.I_NROWS] >= 1
