"""CPU: the scenes of tests/querycases.py are what they are named for, and satisfy what tests/test_gpu_query_runs.py rests on.

* run structure (tests/querycases.py::run_lengths on gridcases.ranges, the fp64 restatement of the query's cell ranges): the run count, the
  empty runs, the candidate total and the positions at which runs start, per case;
* no pair of a scene lies within a relative 1e-4 of the selection radius or of rmin at any horizon step, and none in the band between the
  selection radius and the query's own, 1e-3 wider, radius: the lists of the device are then exactly the fp64 sets;
* no agent has more neighbours than a list holds;
* current states inside the workspace and more than rmin apart, planted violations present (rows will be built)."""
import numpy as np
import pytest

import gridcases as gc
import nbrcases as nc
import querycases as qc


def _runs(name, s=0):
    kw, l, *_ = qc.case(name)
    return qc.run_lengths(kw, l[s], nc.rsel_of(kw))


@pytest.mark.parametrize("name", list(qc.CASES))
def test_inputs_keep_clear_of_the_radii_and_fit_the_lists(name):
    kw, l, xp, xv, xa, pf, facts = qc.case(name)
    rsel = nc.rsel_of(kw)
    assert facts["inside"] and facts["separation"] > kw["rmin"]
    for s in range(l.shape[0]):
        (m_sel, m_min), band = qc.margins(l[s], kw["c"], rsel, kw["rmin"])
        print(f"{name} scene {s}: nearest a radius: {m_sel:.2e} (selection), {m_min:.2e} (rmin)")
        assert m_sel > 1e-4 and m_min > 1e-4 and not band, (name, s, m_sel, m_min, band)
        nb = qc.near(l[s], kw["c"], rsel)
        assert nb.sum(axis=1).max() <= qc.list_cap(l.shape[1])
        assert qc.near(l[s], kw["c"], kw["rmin"]).any()                # a violation: rows will be built
        if l.shape[1] <= 300:                                           # the step-by-step relation is the one of nbrcases.distances
            assert np.array_equal(nb, (nc.distances(l[s], kw["c"]) < rsel).any(axis=0))


@pytest.mark.parametrize("T", (63, 64, 65, 128, 129))
def test_one_run_of_T_candidates(T):
    kw, l, *_, facts = qc.case(f"one_run-{T}")
    assert 64 <= l.shape[1] <= 300
    runs = _runs(f"one_run-{T}")
    for i in facts["cluster"]:
        for sg in range(nc.NSEG):
            assert runs[i][sg].tolist() == [T], (i, sg, runs[i][sg])
    assert all(len(r) == 1 for per in runs for r in per)               # one run, whoever asks


def test_one_run_holding_the_agent_alone():
    kw, l, *_, facts = qc.case("one_run-1")
    runs = _runs("one_run-1")
    assert l.shape[1] >= 64
    for i in facts["alone"]:
        for sg in range(nc.NSEG):
            assert runs[i][sg].tolist() == [1]


@pytest.mark.parametrize("name", ["runs-64", "runs-65", "empties-a", "empties-b", "starts-63-64-65", "over_window"])
def test_pattern_scenes_show_every_query_their_counts(name):
    kw, l, *_, facts = qc.case(name)
    counts = facts["counts"]
    runs = _runs(name)
    for i in range(l.shape[1]):
        for sg in range(nc.NSEG):
            assert np.array_equal(runs[i][sg], counts), (name, i, sg)
    tot, nruns, n = gc.candidates(kw, l[0], nc.rsel_of(kw), gc.DEFAULT)
    assert (tot == counts.sum()).all() and (nruns == len(counts)).all() and (n[1], n[2]) == (facts["ny"], facts["nz"])
    if name != "over_window":
        assert 64 <= l.shape[1] <= 300


def test_batch_boundary_and_empty_runs_are_where_the_names_say():
    assert len(qc.case("runs-64")[-1]["counts"]) == 64 and (qc.case("runs-64")[-1]["counts"] > 0).all()
    assert len(qc.case("runs-65")[-1]["counts"]) == 65 and (qc.case("runs-65")[-1]["counts"] > 0).all()
    a = qc.case("empties-a")[-1]["counts"]
    b0, b1 = a[:64], a[64:]
    assert b0[0] == 0 and b0[63] == 0 and b0[1] > 0                     # the first and the last run of a batch
    assert b0[2] > 0 and (b0[3:7] == 0).all() and b0[7] > 0             # several in a row between two non-empty ones
    assert (b1[:63] == 0).all() and b1[63] > 0                          # every run of a batch but its last
    b = qc.case("empties-b")[-1]["counts"]
    assert (b[:64] == 0).all() and b[64] > 0 and b[127] > 0             # tot = 0, then a non-empty batch
    c = qc.case("starts-63-64-65")[-1]["counts"]
    starts = (np.cumsum(c) - c)[c > 0]
    assert {63, 64, 65} <= set(starts.tolist()) and c[1] == 1 and c[2] == 1
    assert c.sum() == 129                                               # two ranks: chunks of 65 and 64


def test_hundreds_of_runs_nearly_all_empty():
    kw, l, *_ = qc.case("runs-361")
    for s in range(l.shape[0]):
        runs = qc.run_lengths(kw, l[s], nc.rsel_of(kw))
        for i in range(0, l.shape[1], 7):
            for sg in range(nc.NSEG):
                r = runs[i][sg]
                assert len(r) == 361 and r.sum() == l.shape[1] and (r == 0).sum() > 150, (s, i, sg, (r == 0).sum())
                assert any((r[b:b + 64] == 0).all() or (r[b:b + 64] == 0).sum() > 20 for b in range(0, 361, 64))


def test_one_cell_holds_the_scene_and_the_window_case_is_longer_than_the_window():
    kw, l, *_ = qc.case("one_cell-3x300")
    assert l.shape[:2] == (3, 300)
    for s in range(3):
        runs = qc.run_lengths(kw, l[s], nc.rsel_of(kw))
        assert all(r.tolist() == [300] for per in runs for r in per)
        n, cc, _, _ = gc.ranges(kw, l[s], nc.rsel_of(kw), gc.DEFAULT)
        assert tuple(n) == (64, 1, 1) and len(np.unique(cc[..., 0])) == 1
    assert 300 < qc.WINDOW                                              # a run of five rounds inside one window: hence the case below
    c = qc.case("over_window")[-1]["counts"]
    ends = np.cumsum(c)
    assert ends[-1] > qc.WINDOW and ((ends[:-1] > qc.WINDOW) & (ends[:-1] < ends[-1])).any()     # a run ends inside the second window
    assert (ends[:-1] < qc.WINDOW).sum() >= 2                           # and the second window starts some runs in
