"""GPU: the neighbour filters of large scenes on inputs built to break them (tests/nbrcases.py; the facts of every scene are asserted on the
CPU in tests/test_nbrcases_cpu.py).

Whether a collision row is built at all is decided by filters that run before the scan: the segment-box test (nbr_kernel), the cell grid
with its chord pre-test (csrc/dmpc_lists.hip: grid_prep / grid_bin / grid_fill* / grid_query_kernel and the device functions both builds share --
box_cell, chord_record, nbrmajor_word; the grid itself is checked in tests/test_gpu_grid_build.py) and the close pairs the query hands to the scan.  Each must
return a superset of what the whole-table walk selects, so every output word of every leg must equal the walk's (option no_cull).  The fp64
walk itself is tied to the CPU oracle -- an independent fp64 statement of the selection: identical branch records, trajectories to 1e-9 --
because equality with the walk alone cannot see a mistake the walk shares.

Mixed precision is compared with its own mixed walk only: there the scan decides on the fp32 table, and at a pair within 1e-7 of a radius
(threshold-*) it may by design decide differently from fp64.

One MPC step per leg from the case's table; scenes of 64 - 300 agents take the list paths through cull_min = grid_min = 64.

The filter legs are asserted before the oracle leg, so a miss there does not hide them."""
import functools

import numpy as np
import pytest

import nbrcases as nc
import test_gpu_paths as paths
from helpers import compare_to_oracle
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KEYS = ("status", "info", "p", "v", "a")
VARIANTS = [("bound", "f64"), ("bound", "mixed"), ("ondemand", "f64"), ("cpp", "f64"), ("hard", "f64")]
GRID = dict(cull_min=64, grid_min=64)


@functools.lru_cache(maxsize=None)
def _case(name, hard):
    return nc.CASES[name](hard)


def _step(case, variant, precision, scenes, **opts):
    kw, l, xp, xv, xa, pf, _ = case
    return paths._steps(variant, kw, np.ascontiguousarray(xp[scenes]), np.ascontiguousarray(pf[scenes]), 1, precision,
                        table=np.ascontiguousarray(l[scenes]), **opts)[0]


def _same(name, variant, precision, leg, case, got, want, scenes):
    """every word equal; the message names the first agent that differs and its fp64 neighbourhood"""
    for k in KEYS:
        if np.array_equal(got[k], want[k]):
            continue
        g, w = got[k].reshape(got["status"].shape + (-1,)), want[k].reshape(want["status"].shape + (-1,))
        s, n = np.argwhere((g != w).any(-1))[0]
        scene = range(case[1].shape[0])[scenes][s]
        near = nc.describe(case[0], case[1][scene], n, variant == "hard")
        raise AssertionError(f"{name} {variant}/{precision} leg '{leg}': {k} of scene {scene} agent {n} differs from the walk: status {got['status'][s, n]} vs "
                             f"{want['status'][s, n]}, rows {got['info'][s, n, 1]} vs {want['info'][s, n, 1]}, info {got['info'][s, n].tolist()} vs {want['info'][s, n].tolist()}; "
                             f"(neighbour, step, fp64 distance, * = within 2e-3 of Rsel or rmin) within 1.01 Rsel, nearest a radius first: {near}")


@pytest.mark.parametrize("variant,precision", VARIANTS)
@pytest.mark.parametrize("name", list(nc.CASES))
def test_filters_select_a_superset_of_the_walk(name, variant, precision):
    hard = variant == "hard"
    case = _case(name, hard)
    kw, l, xp, xv, xa, pf, _ = case
    S = l.shape[0]
    every = slice(0, S)
    walk = _step(case, variant, precision, every, no_cull=1)
    legs = [("boxes", every, dict(cull_min=64, nbr_grid=0)), ("grid, batch", every, GRID)]
    for s in range(S):
        legs += [(f"grid, scene {s} alone", slice(s, s + 1), GRID), (f"grid, scene {s} alone, prep_fuse=0", slice(s, s + 1), dict(GRID, prep_fuse=0))]
    if not hard:
        legs += [("no close pairs", every, dict(GRID, close_pairs=0)),
                 ("close cap", every, dict(GRID, close_cap=64 if name == "close_edge" else 1))]
        if name == "close_edge":   # (and one record: agent 80's only pair sits in the last slot of its list)
            legs.append(("close cap 1", every, dict(GRID, close_cap=1)))
    for leg, scenes, opts in legs:
        got = _step(case, variant, precision, scenes, **opts)
        _same(name, variant, precision, leg, case, got, {k: walk[k][scenes] for k in KEYS}, scenes)
    assert (walk["info"][..., 1] > 0).any(), name      # rows were built
    if precision == "f64":
        prm = orc.make_params(variant, **kw)
        for s in range(S):
            ref = orc.step(prm, l[s], xp[s], xv[s], xa[s], pf[s], nthreads=16)
            compare_to_oracle({k: walk[k][s] for k in KEYS}, ref, what=f"{name} {variant} scene {s} (walk against the oracle)")
