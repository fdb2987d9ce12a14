"""CPU: the scenes of tests/test_gpu_grid_build.py are what that test says they are -- the cell counts of the default geometry, which of the
two builds a single scene takes, one cell along z where stated, tables beyond every face in `outside` -- and the cell check leaves out at
most 1 % of a scene's agents (centres within 1e-4 cell widths of an interior cell boundary, where the fp32 cell may differ from the fp64 one)."""
import numpy as np
import pytest

import gridbuild as gb
import gridcases as gc
import nbrcases as nc


@pytest.mark.parametrize("name", list(gb.SCENES))
def test_scene_has_the_stated_grid_and_few_agents_near_a_cell_boundary(name):
    build, precision, ncell = gb.SCENES[name]
    kw, l, xp, xv, xa, pf, facts = build()
    assert facts["inside"] and facts["separation"] > kw["rmin"]
    assert l.shape[1] in (260, 300) and l.shape[1] % 64 and l.shape[1] > 256      # two blocks of grid_prep_kernel, the second a tail
    shares = []
    for s in range(l.shape[0]):
        n, cell, near = gb.cells(kw, gb.source(l[s], precision))
        assert int(np.prod(n)) == ncell, (name, n)
        assert cell.min() >= 0 and cell.max() < ncell
        shares.append(near.any(axis=1).mean())
    print(f"{name}: cells {n.tolist()}, share of agents left out of the cell check per scene {shares}")
    assert max(shares) <= gb.NEAR_SHARE_MAX
    assert gc.fused(n) == (ncell <= 10920)
    if name in ("metric-1", "metric-2"):
        assert n[2] == 1
    if name == "metric-1":
        assert ncell < 256
    if name == "outside":
        lo, hi = gb.extents(l[0])
        pmin, pmax = np.array(kw["pmin"]), np.array(kw["pmax"])
        assert ((0.5 * (lo + hi) < pmin).any(axis=(0, 1)) & (0.5 * (lo + hi) > pmax).any(axis=(0, 1))).all()   # centres beyond all six faces


def test_close_edge_is_not_a_scene_of_the_cell_check():
    """close_edge's lattice sits on the cell boundaries of geometry 0 (a sixth of its agents within 1e-4 cell widths of one): why it is not in the list"""
    kw, l = nc.close_edge()[:2]
    n, cc, _, _ = gc.ranges(kw, l[0], nc.rsel_of(kw), 0)
    lo, hi = gb.extents(l[0])
    pmin = np.array(kw["pmin"])
    t = (0.5 * (lo + hi) - pmin) * (n / (np.array(kw["pmax"]) - pmin))
    k = np.rint(t)
    near = ((np.abs(t - k) < gb.NEAR) & (k >= 1) & (k <= n - 1)).any(axis=-1)
    assert near.any(axis=1).mean() > 0.1
    assert gb.cells(kw, l[0])[2].any(axis=1).mean() == 0.0      # (none in the default geometry)


def test_rounding_helpers_round_outwards():
    x = np.array([0.1, -0.1, 1.0, 40.0 + 1e-9, -40.0 - 1e-9, 0.0])
    lo, hi = gb.round_down(x), gb.round_up(x)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert (lo.astype(np.float64) <= x).all() and (hi.astype(np.float64) >= x).all()
    assert (np.nextafter(lo, np.float32(np.inf)).astype(np.float64) > x).all() and (np.nextafter(hi, np.float32(-np.inf)).astype(np.float64) < x).all()
    assert lo[2] == hi[2] == np.float32(1.0)
