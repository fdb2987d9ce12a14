"""The neighbour grid itself (what dmpc_debug_read_grid reads after a step): the scenes of tests/test_gpu_grid_build.py and
tests/test_grid_build_cpu.py, and an fp64 numpy model of what the build must have left -- segment boxes, half extents, cells, chord records.

Not a conftest: a plain helper like tests/gridcases.py, whose builders it reuses (imported, not edited).  Every model function takes ONE scene's
table l [N, 45] as the values the list builders read: the fp64 table, or (mixed precision) the fp32 copy of it, see `source`.
"""
import numpy as np

import gridcases as gc
import nbrcases as nc

# name -> (builder, precision, cells of the default geometry)
SCENES = {
    "metric-2": (lambda: nc.metric(2), "f64", 32),                   # one z cell
    "metric-1": (lambda: nc.metric(1), "f64", 242),                  # one z cell, fewer than 256 cells: one-cell chunks in grid_fill2_kernel
    "outside": (lambda: nc.outside(), "f64", 216),                   # clamped cells beyond every face
    "limit-under": (lambda: gc.limit_scene(False), "f64", 10920),    # the two-launch build's last size
    "limit-over": (lambda: gc.limit_scene(True), "f64", 11180),      # five kernels, a prefix over more than 1 024 cells
    "metric-0": (lambda: nc.metric(0), "f64", 19968),                # five kernels
    "c4-2x300": (lambda: gc.c4_scene(2, 300, 1), "mixed", 216),      # the fp32 table type
}
NEAR = 1e-4            # (agent, segment) centres within this many cell widths of an interior cell boundary are left out of the cell check
NEAR_SHARE_MAX = 0.01  # ... and at most this share of a scene's agents may be


def source(l, precision):
    """the table the list builders read, as fp64 values: mixed precision reads the fp32 copy"""
    return l.astype(np.float32).astype(np.float64) if precision == "mixed" else l


def round_down(x):
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)


def round_up(x):
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)


def extents(l):
    """fp64 minimum and maximum of every segment's five steps: lo, hi [N, NSEG, 3]"""
    p = nc.steps_of(l).reshape(l.shape[0], nc.NSEG, nc.SEG, 3)
    return p.min(axis=2), p.max(axis=2)


def bbox(l):
    """[18, N] fp32: per segment xmin, xmax, ymin, ymax, zmin, zmax, the fp64 extremes rounded outwards"""
    lo, hi = extents(l)
    out = np.empty((6 * nc.NSEG, l.shape[0]), dtype=np.float32)
    for sg in range(nc.NSEG):
        for a in range(3):
            out[6 * sg + 2 * a], out[6 * sg + 2 * a + 1] = round_down(lo[:, sg, a]), round_up(hi[:, sg, a])
    return out


def half_extents(l):
    """[NSEG, 3] fp64: the scene's largest half extent per segment and axis"""
    lo, hi = extents(l)
    return (0.5 * (hi - lo)).max(axis=0)


def cells(kw, l, rsel=None):
    """cells per axis n, the fp64 cell index of every (agent, segment) [N, NSEG], and which of them sit within NEAR cell widths of an interior
    cell boundary on some axis [N, NSEG]"""
    rsel = nc.rsel_of(kw) if rsel is None else rsel
    n, cc, _, _ = gc.ranges(kw, l, rsel, gc.DEFAULT)
    lo, hi = extents(l)
    pmin = np.array(kw["pmin"])
    t = (0.5 * (lo + hi) - pmin) * (n / (np.array(kw["pmax"]) - pmin))
    k = np.rint(t)
    near = ((np.abs(t - k) < NEAR) & (k >= 1) & (k <= n - 1)).any(axis=-1)
    return n, (cc[..., 2] * n[1] + cc[..., 1]) * n[0] + cc[..., 0], near


def chords(l, c):
    """the chord records' exact words in np.float32 arithmetic: first step a0 [N, NSEG, 3] (z times np.float32(1 / c)) and last minus first (z:
    the last step's product and the subtraction as ONE fma, as hipcc contracts them -- the fp64 product of two fp32 words is exact)"""
    t = nc.steps_of(l).astype(np.float32)
    e = np.float32(1.0 / c)
    w = t.copy()
    w[..., 2] = t[..., 2] * e
    a0, a1 = w[:, 0::nc.SEG], w[:, nc.SEG - 1::nc.SEG]
    da = a1 - a0
    da[..., 2] = (t[:, nc.SEG - 1::nc.SEG, 2].astype(np.float64) * np.float64(e) - a0[..., 2].astype(np.float64)).astype(np.float32)
    return a0, da


def deviations(l, c):
    """[N, NSEG] fp64: the largest distance of a segment's three interior steps from its chord at their own time, z in the metric's scale"""
    p = nc.steps_of(l).reshape(l.shape[0], nc.NSEG, nc.SEG, 3) / np.array([1.0, 1.0, c])
    a0, a1 = p[:, :, 0], p[:, :, nc.SEG - 1]
    dev = np.zeros(p.shape[:2])
    for u in range(1, nc.SEG - 1):
        t = u / (nc.SEG - 1.0)
        dev = np.maximum(dev, np.sqrt(((p[:, :, u] - (a0 + t * (a1 - a0))) ** 2).sum(-1)))
    return dev


def record_cells(start, nent):
    """the cell of entries 0 .. nent-1 read off an exclusive prefix start[0 .. ncell]"""
    return np.searchsorted(start, np.arange(nent), side="right") - 1


def canonical(g):
    """the entry records of a grid read by Dmpc.debug_read_grid, as int32 words [2, S, NSEG, G C, 4], sorted by code inside each cell (the
    order inside a cell is whatever the atomics gave); entries behind the last record are zeroed"""
    ent = g["ent"].view(np.int32).copy()
    nent = ent.shape[3]
    for s in range(ent.shape[1]):
        for sg in range(ent.shape[2]):
            st = g["start"][s, sg]
            cell = record_cells(st, nent)
            order = np.lexsort((ent[0, s, sg, :, 0], cell))
            ent[:, s, sg] = ent[:, s, sg][:, order]
            ent[:, s, sg, st[-1]:] = 0
    return ent
