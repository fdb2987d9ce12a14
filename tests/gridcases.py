"""Cell geometries of the neighbour grid (option grid_cells): a numpy model of the query's cell ranges, and the scenes of
tests/test_grid_geometry_cpu.py and tests/test_gpu_grid_geometry.py.

Not a conftest: a plain helper like tests/nbrcases.py, whose builders it reuses (imported, not edited).  `GEOMS`, `cells` and `ranges` restate
plan_lists (multiagent_planning_amd/csrc/dmpc_launch.hip) and the reach of grid_query_kernel in fp64; they GUARD inputs and carry the superset
argument, they are no reference for any output.  Every case is (kw, l, xp, xv, xa, pf, facts) as in nbrcases.py.
"""
import functools

import numpy as np

import nbrcases as nc
from multiagent_planning_amd import workload as wl

# rows of plan_lists: cell sizes in units of (R, R, R c), cells per axis at most
GEOMS = ((1.0, 1.5, 1.5, 32), (0.5, 1.5, 1.5, 64), (0.5, 1.0, 1.0, 64), (0.5, 1.0, 0.5, 64))
DEFAULT = 2
OFFERED = tuple(range(len(GEOMS)))
FILL2_LDS_MAX = 128 * 1024      # one scene: the grid in two launches while NSEG * (ncell + 1) * 4 bytes fit
LIST_CAP = 64                   # option list_cap of the capacity scenes


def cells(kw, rsel, which):
    """(R, cells per axis) of geometry `which`; a finer grid with more than 32^3 cells falls back to geometry 0"""
    R = rsel * 1.0001 + 1e-4
    span = np.array(kw["pmax"]) - np.array(kw["pmin"])

    def n_of(g):
        fx, fy, fz, cap = GEOMS[g]
        cell = np.array([fx * R, fy * R, fz * R * kw["c"]])
        return np.clip((span / cell).astype(int), 1, cap)
    n = n_of(which)
    if n.prod() > 32 ** 3:
        n = n_of(0)
    return R, n


def fused(n):
    return 3 * (int(np.prod(n)) + 1) * 4 <= FILL2_LDS_MAX


def ranges(kw, l, rsel, which):
    """one scene: cells per axis n, the cell of every segment-box centre cc [N, NSEG, 3] and the query's cell range c_lo, c_hi [N, NSEG, 3]
    (own segment box +- (R + the scene's largest half extent of that segment), clamped)"""
    R, n = cells(kw, rsel, which)
    pmin = np.array(kw["pmin"])
    span = np.array(kw["pmax"]) - pmin
    p = nc.steps_of(l).reshape(l.shape[0], nc.NSEG, nc.SEG, 3)
    lo, hi = p.min(axis=2), p.max(axis=2)
    coord = lambda x: np.clip(np.floor((x - pmin) * (n / span)).astype(int), 0, n - 1)
    cc = coord(0.5 * (lo + hi))
    rch = np.array([R, R, R * kw["c"]]) + (0.5 * (hi - lo)).max(axis=0)      # [NSEG, 3]
    return n, cc, coord(lo - rch), coord(hi + rch)


def candidates(kw, l, rsel, which):
    """one scene: per agent and segment the candidates (entries of the cells in range, the own one included) and the runs ((y, z) cell rows)"""
    n, cc, c_lo, c_hi = ranges(kw, l, rsel, which)
    inside = ((cc[None] >= c_lo[:, None]) & (cc[None] <= c_hi[:, None])).all(-1)   # [agent, entry, NSEG]
    runs = (c_hi[..., 1] - c_lo[..., 1] + 1) * (c_hi[..., 2] - c_lo[..., 2] + 1)
    return inside.sum(axis=1), runs, n


def missed_pairs(kw, l, rsel, which, d=None):
    """one scene: the (agent, neighbour, step) with a scaled distance below rsel whose neighbour's cell is outside the agent's range in
    the step's segment (fp64) -- the superset claim says there are none.  d: nbrcases.distances(l, c), when the caller has it"""
    n, cc, c_lo, c_hi = ranges(kw, l, rsel, which)
    d = nc.distances(l, kw["c"]) if d is None else d
    k, i, j = np.nonzero(d < rsel)
    sg = k // nc.SEG
    ok = ((cc[j, sg] >= c_lo[i, sg]) & (cc[j, sg] <= c_hi[i, sg])).all(-1)
    return [(int(a), int(b), int(c_)) for a, b, c_ in zip(i[~ok], j[~ok], k[~ok])]


# ------------------------------------------------------------------------------------------------------------------------------------
C4 = wl.CONFIGS["C4"]


@functools.lru_cache(maxsize=None)
def c4_scene(S, N, seed):
    """S scenes of N agents at the headline's density, initDMPC tables"""
    kw = wl.solver_kwargs(C4, N)
    po, pf = wl.make_scenes(C4, S, N, wl.SEED0 + seed)
    return nc._pack(kw, nc.lines(po, pf), po, pf, {})


def limit_scene(over, hard=False, N=300):
    """A workspace whose default grid has 42 x 26 x 10 = 10 920 cells (the two-launch build's last size: 10 921) or 43 x 26 x 10 = 11 180 (the
    five kernels), whatever the variant's radius; 300 agents at the headline's density in its middle, planted triples in the first table."""
    rsel = 1.0 if hard else 3.0 * C4["rmin"]
    R = rsel * 1.0001 + 1e-4
    fx, fy, fz, _ = GEOMS[DEFAULT]
    want = np.array([43 if over else 42, 26, 10])
    span = (want + 0.4) * np.array([fx * R, fy * R, fz * R * C4["c"]])
    pmin = np.array([-0.5 * span[0], -0.5 * span[1], 0.2])
    kw = nc.solver_kw(pmin, pmin + span, rmin=C4["rmin"], c=C4["c"])
    rng = np.random.default_rng(8000 + int(over))
    s = float(N) ** (1.0 / 3.0)
    mid = pmin + 0.5 * span
    blo, bhi = mid - 0.5 * np.array([s, s, s]), mid + 0.5 * np.array([s, s, s])
    po, pf = wl.random_test(N, blo, bhi, C4["rmin_init"], C4["c"], rng)
    l = nc.lines(po[None], pf[None])
    trip = np.arange(60).reshape(20, 3)
    nc._triples(nc.steps_of(l)[0], trip, kw, steps=list(range(1, nc.K)))
    return nc._pack(kw, l, po[None], pf[None], dict(want=want, planted=trip))


def capacity(extra, hard=False, N=200):
    """Lists at option list_cap = 64: a sparse lattice (sites 2.3 m apart), constant tables, and at step 7 the tables of agents 1 .. 64 + extra
    sit within 2.7 rmin of agent 0's site -- agent 1 at 0.5 rmin (agent 0's violation), the others on a lattice of 1.03 rmin (no two tables within 1.5 % of either radius).  Agent 0 then
    has exactly 64 + extra neighbours inside the selection radius, each 5 % or more inside it (the hard rows' radius of 1 included), everybody else far outside."""
    kw = nc.solver_kw((-11.0, -11.0, 0.2), (11.0, 11.0, 22.2))
    rmin, c = kw["rmin"], kw["c"]
    g = np.arange(9)
    ii, jj, kk = np.meshgrid(g, g, np.arange(4), indexing="ij")
    site = np.array(kw["pmin"]) + np.array([1.2, 1.2, 1.7]) + np.stack([ii.ravel() * 2.3, jj.ravel() * 2.3, kk.ravel() * 4.7], 1)
    ctr = 0.5 * (np.array(kw["pmin"]) + np.array(kw["pmax"]))
    site = site[np.argsort(np.abs((site - ctr) / np.array([1, 1, c])).max(axis=1), kind="stable")][:N]
    xp = site[None].copy()
    pf = np.clip(xp + np.array([0.4, -0.3, 0.2]), np.array(kw["pmin"]) + 0.05, np.array(kw["pmax"]) - 0.05)
    l = nc.constant(xp)
    lv = nc.steps_of(l)[0]
    m = np.arange(-3, 4)
    a, b, cz = np.meshgrid(m, m, m, indexing="ij")
    off = 1.03 * rmin * np.stack([a.ravel(), b.ravel(), cz.ravel()], 1).astype(float)
    r = np.linalg.norm(off, axis=1)
    off = off[(r > 0) & (r <= 2.7 * rmin)]
    off = off[np.argsort(np.linalg.norm(off, axis=1), kind="stable")]
    count = LIST_CAP + extra
    assert len(off) >= count - 1
    nc._place(lv, 1, 7, site[0], np.array([0.0, 0.5 * rmin, 0.0]), c)
    for t in range(count - 1):
        nc._place(lv, 2 + t, 7, site[0], off[t], c)
    return nc._pack(kw, l, xp, pf, dict(hub=0, count=count))


CASES = {}
for _n in (64, 65, 128, 129):       # the default geometry: 64 x 1 x 1 cells (x at the cap, one cell along y and z), every query ONE run of all N entries
    CASES[f"rounds-{_n}"] = (lambda hard=False, _n=_n: nc.rounds(_n))
CASES["many_runs-oversize"] = lambda hard=False: nc.many_runs(True)      # the default geometry: 19 x 19 cell rows, every one in reach of every query
CASES["metric-1"] = lambda hard=False: nc.metric(1)                      # one cell along z
CASES["limit-under"] = lambda hard=False: limit_scene(False, hard)
CASES["limit-over"] = lambda hard=False: limit_scene(True, hard)
CASES["capacity-0"] = lambda hard=False: capacity(0, hard)
CASES["capacity-1"] = lambda hard=False: capacity(1, hard)
