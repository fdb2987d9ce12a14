"""Run structures for the fetch of grid_query_kernel: scenes whose queries have a chosen sequence of run lengths.

Not a conftest: a plain helper of tests/test_query_runs_cpu.py and tests/test_gpu_query_runs.py; it imports tests/nbrcases.py and
tests/gridcases.py and edits neither.  Every builder returns (kw, l, xp, xv, xa, pf, facts) as theirs do.

The query of one agent and horizon segment walks the (y, z) cell rows in its reach, z-major: every row is one RUN of entries (the cells of a
row along x are contiguous), the runs of a batch of 64 rows are one sequence of candidates, and a round takes the next 64 positions of it.
The fetch maps a position to its run.  What can go wrong there depends on the run lengths alone -- empty runs, runs that start at a round's
boundary, more than 64 runs, a sequence longer than the fetch's bit window (2 048 positions) -- so the scenes here fix them:

  pattern   a grid of ny x nz cell rows (default geometry), `counts[qz * ny + qy]` agents with constant tables in row (qy, qz), and agent 0's
            table alternating between two points far outside the workspace on either side of a chosen cell centre: its half extents are the
            scene's largest, so EVERY query reaches every row and sees the same runs, `counts`, in the same order;
  line      one cell along y and along z: every query has one run.  Agent 0's table is stretched along x only, so a query reaches a cluster
            of T agents around it (tot = T) and not a second cluster far away;
  isolated  one run again, constant tables, and agents so far from everybody that their query holds themselves alone (tot = 1);
  one_cell  300 agents in ONE cell of a 64 x 1 x 1 grid: a single run of five rounds.

`run_lengths` restates the kernel's run order on top of gridcases.ranges (fp64); it GUARDS the inputs, it is no reference for any result.
`near` is the brute-force neighbour relation of the GPU test, step by step with the arithmetic of nbrcases.distances (which holds all
steps of all pairs at once: 600 MB for the 2 230 agents of the case longer than the window)."""
import functools

import numpy as np

import gridcases as gc
import nbrcases as nc

RMIN, CZ = 0.35, 2.0
RSEL = 3.0 * RMIN
R = RSEL * 1.0001 + 1e-4
FX, FY, FZ, CAP = gc.GEOMS[gc.DEFAULT]
WINDOW = 2048                       # positions of the fetch's bit window (GQ_WIN, csrc/dmpc_lists.hip)
SX = 0.60                           # stations along x; four lanes per station inside a cell row
LANES = ((-0.28, -0.5), (0.28, -0.5), (-0.28, 0.5), (0.28, 0.5))      # (y, z) offsets: 0.56 apart, 1.0 / c = 0.5 apart
JIT = 0.005                         # (with these numbers no two lattice sites, planted tables included, are within 4 % of either radius)
# the query's own radius is the selection radius widened by 1e-3 (thr2 = Rsel^2 x 1.002, on the fp32 table): a list equals the fp64 set
# {some step closer than Rsel} only if no pair sits in that band
BAND = 2e-3


def list_cap(N):
    """plan_lists: the capacity of a list (no option list_cap)"""
    return min(4096, (N + 63) & ~63)


def near(l, c, radius):
    """one scene: [N, N] bool, some horizon step's scaled distance below radius (fp64, the diagonal False)"""
    p = nc.steps_of(l).copy()
    p[..., 2] /= c
    out = np.zeros((l.shape[0], l.shape[0]), dtype=bool)
    for k in range(nc.K):
        q = p[:, k]
        d = np.sqrt(((q[:, None, :] - q[None, :, :]) ** 2).sum(-1))
        out |= d < radius
    np.fill_diagonal(out, False)
    return out


def margins(l, c, rsel, rmin):
    """one scene: the smallest |d / rsel - 1| and |d / rmin - 1| over all pairs and steps, and whether any distance lies in [rsel, rsel (1 + BAND)]"""
    marks = (rsel, rmin)
    p = nc.steps_of(l).copy()
    p[..., 2] /= c
    i = np.arange(l.shape[0])
    best = [np.inf] * len(marks)
    band = False
    for k in range(nc.K):
        q = p[:, k]
        d = np.sqrt(((q[:, None, :] - q[None, :, :]) ** 2).sum(-1))
        d[i, i] = np.inf
        for m, mark in enumerate(marks):
            best[m] = min(best[m], float(np.abs(d / mark - 1.0).min()))
        band = band or bool(((d >= rsel) & (d <= rsel * (1.0 + BAND))).any())
    return best, band


def run_lengths(kw, l, rsel, which=gc.DEFAULT):
    """one scene: out[agent][segment] = the lengths of the query's runs in the kernel's order (run = qz * ny + qy over the (y, z) cell rows of
    the range; its entries: the agents whose segment-box centre lies in the row's cells c_lo.x .. c_hi.x)"""
    n, cc, c_lo, c_hi = gc.ranges(kw, l, rsel, which)
    N = l.shape[0]
    out = [[None] * nc.NSEG for _ in range(N)]
    for sg in range(nc.NSEG):
        e = cc[:, sg]
        for i in range(N):
            lo, hi = c_lo[i, sg], c_hi[i, sg]
            ny, nz = hi[1] - lo[1] + 1, hi[2] - lo[2] + 1
            m = ((e >= lo) & (e <= hi)).all(-1)
            out[i][sg] = np.bincount((e[m, 2] - lo[2]) * ny + (e[m, 1] - lo[1]), minlength=ny * nz)
    return out


def _workspace(xspan, ny, nz, slack=0.4):
    """a workspace whose default geometry has ny x nz cell rows (x: int(xspan / (FX R)) cells, at most CAP)"""
    span = np.array([xspan, (ny + slack) * FY * R, (nz + slack) * FZ * R * CZ])
    pmin = np.array([-0.5 * xspan, 0.0, 0.2])
    return nc.solver_kw(pmin, pmin + span, rmin=RMIN, c=CZ), pmin, span


def _row_sites(count, x0, ycen, zcen):
    t = np.arange(count)
    lane = np.array(LANES)[t % 4]
    return np.stack([x0 + SX * (t // 4), ycen + lane[:, 0], zcen + lane[:, 1]], 1)


def _plant(lv, pairs):
    """b's table sits 0.2 m beside a's site (along x) at one step: a violation, so rows are built"""
    for t, (a, b) in enumerate(pairs):
        k = 1 + t % (nc.K - 1)
        lv[b, k] = lv[a, 0] + np.array([0.2, 0.0, 0.0])


def pattern(counts, ny, nz, seed, xspan=(CAP + 0.4) * FX * R, plant=6, slack=0.4):
    counts = np.asarray(counts, dtype=int)
    assert counts.shape == (ny * nz,) and counts.sum() >= 64
    kw, pmin, span = _workspace(xspan, ny, nz, slack)
    rng = np.random.default_rng(seed)
    N = int(counts.sum())
    cy, cz = span[1] / ny, span[2] / nz
    target = int(np.argmax(counts > 0))                  # agent 0's row: the first one that holds anybody
    others = 1 + rng.permutation(N - 1)                  # agent numbers in no order of the cells
    xp = np.empty((N, 3))
    pairs, at = [], 0
    for r, cnt in enumerate(counts):
        qz, qy = divmod(r, ny)
        site = _row_sites(cnt, pmin[0] + 1.2, pmin[1] + (qy + 0.5) * cy, pmin[2] + (qz + 0.5) * cz)
        who = others[at:at + cnt - (r == target)]
        at += len(who)
        if r == target:
            who = np.concatenate([[0], who])
        xp[who] = site + rng.uniform(-JIT, JIT, (cnt, 3))
        if cnt - (r == target) >= 2 and len(pairs) < plant:
            pairs.append((int(who[-2]), int(who[-1])))
    pf = np.clip(xp + rng.uniform(-0.4, 0.4, (N, 3)), pmin + 0.05, pmin + span - 0.05)
    l = nc.constant(xp[None])
    lv = nc.steps_of(l)[0]
    _plant(lv, pairs)
    # agent 0: between two points far outside on either side of the centre of an x cell of its row (not a cell boundary: fp32 and fp64 bin alike)
    nx = min(CAP, int(span[0] / (FX * R)))
    qz, qy = divmod(target, ny)
    ctr = pmin + np.array([(nx // 2 + 0.5) * span[0] / nx, (qy + 0.5) * cy, (qz + 0.5) * cz])
    lv[0, 0::2], lv[0, 1::2] = ctr - (span + 5.0), ctr + (span + 5.0)
    return nc._pack(kw, l, xp[None], pf[None], dict(counts=counts, ny=ny, nz=nz, planted=pairs))


def line(T, seed, far=70):
    """one run per query; the T agents of the first cluster (agent 0 among them) have tot = T in every segment"""
    kw, pmin, span = _workspace(120.0, 1, 1)
    rng = np.random.default_rng(seed)
    N = T + far
    ycen, zcen = pmin[1] + 0.5 * span[1], pmin[2] + 0.5 * span[2]
    xp = np.empty((N, 3))
    first = _row_sites(T, pmin[0] + 5.0, ycen, zcen)
    mid = int(np.argmin(np.abs(first[:, 0] - first[:, 0].mean())))
    first[[0, mid]] = first[[mid, 0]]                       # agent 0 in the middle of its cluster
    xp[:T] = first
    xp[T:] = _row_sites(far, pmin[0] + 60.0, ycen, zcen)
    xp += rng.uniform(-JIT, JIT, (N, 3))
    pf = np.clip(xp + rng.uniform(-0.4, 0.4, (N, 3)), pmin + 0.05, pmin + span - 0.05)
    l = nc.constant(xp[None])
    lv = nc.steps_of(l)[0]
    pairs = [(1, 2), (T, T + 1), (T + 10, T + 11)] + ([(5, 6)] if T > 6 else [])
    _plant(lv, pairs)
    h = np.array([22.0, 0.0, 0.0])                          # the cluster is at most 20 m long: within reach of every agent in it
    lv[0, 0::2], lv[0, 1::2] = xp[0] - h, xp[0] + h
    return nc._pack(kw, l, xp[None], pf[None], dict(T=T, cluster=np.arange(1, T), planted=pairs))


def isolated(seed=41, packed=60, alone=6):
    """one run per query, every table constant: the last `alone` agents are 6 m from each other and from everybody: tot = 1"""
    kw, pmin, span = _workspace(120.0, 1, 1)
    rng = np.random.default_rng(seed)
    N = packed + alone
    ycen, zcen = pmin[1] + 0.5 * span[1], pmin[2] + 0.5 * span[2]
    xp = np.empty((N, 3))
    xp[:packed] = _row_sites(packed, pmin[0] + 5.0, ycen, zcen)
    xp[packed:] = np.stack([pmin[0] + 60.0 + 6.0 * np.arange(alone), np.full(alone, ycen), np.full(alone, zcen)], 1)
    xp += rng.uniform(-JIT, JIT, (N, 3))
    pf = np.clip(xp + rng.uniform(-0.4, 0.4, (N, 3)), pmin + 0.05, pmin + span - 0.05)
    l = nc.constant(xp[None])
    pairs = [(1, 2), (9, 10), (20, 21)]
    _plant(nc.steps_of(l)[0], pairs)
    return nc._pack(kw, l, xp[None], pf[None], dict(alone=np.arange(packed, N), planted=pairs))


def one_cell(S=3, N=300, seed=51):
    """64 x 1 x 1 cells of 42 m and every agent in the 33rd: every query is one run of N entries (five rounds); S scenes of one batch"""
    kw, pmin, span = _workspace(2700.0, 1, 1)
    rng = np.random.default_rng(seed)
    ycen, zcen = pmin[1] + 0.5 * span[1], pmin[2] + 0.5 * span[2]
    # six lanes: the four of a pattern's rows and two on the cell's centre line
    t = np.arange(N)
    lane = np.array(LANES + ((0.0, -1.25), (0.0, 1.25)))[t % 6]
    sites = np.stack([2.0 + SX * (t // 6), ycen + lane[:, 0], zcen + lane[:, 1]], 1)
    xp = np.stack([sites[rng.permutation(N)] + rng.uniform(-JIT, JIT, (N, 3)) for _ in range(S)])
    pf = np.clip(xp + rng.uniform(-0.4, 0.4, (S, N, 3)), pmin + 0.05, pmin + span - 0.05)
    l = nc.constant(xp)
    pairs = []
    for s in range(S):
        order = np.argsort(xp[s, :, 0], kind="stable")
        mine = [(int(order[6 * j]), int(order[6 * j + 6])) for j in range(3, 9)]      # x neighbours six places on: the next station, the same lane or the one beside it
        _plant(nc.steps_of(l)[s], mine)
        pairs.append(mine)
    return nc._pack(kw, l, xp, pf, dict(planted=pairs))


def _fill(n, **at):
    """n zeros with counts at given positions: _fill(64, **{'3': 5})"""
    c = np.zeros(n, dtype=int)
    for k, v in at.items():
        c[int(k)] = v
    return c


def _counts_empties_a():
    """two batches of 64 runs.  Batch 0: the first run empty, four empty runs in a row between two non-empty ones, the last run empty.
    Batch 1: every run empty but the last."""
    b0 = np.zeros(64, dtype=int)
    b0[[1, 2, 7, 8, 20, 40, 62]] = [30, 9, 17, 1, 40, 25, 11]        # runs 3 .. 6 empty between 2 and 7; 0 and 63 empty
    b1 = _fill(64, **{"63": 37})
    return np.concatenate([b0, b1])


def _counts_empties_b():
    """batch 0 entirely empty (tot = 0), batch 1 begins and ends with non-empty runs"""
    b1 = np.zeros(64, dtype=int)
    b1[[0, 1, 31, 32, 33, 63]] = [50, 1, 20, 64, 3, 32]
    return np.concatenate([np.zeros(64, dtype=int), b1])


def _counts_starts():
    """runs start at positions 63, 64 and 65 of the concatenation (two one-entry runs side by side); 129 agents: two ranks of 65 and 64"""
    c = np.zeros(64, dtype=int)
    c[[0, 1, 2, 3, 30]] = [63, 1, 1, 40, 24]
    return c


def _counts_sparse():
    """361 runs (six batches), 40 of them non-empty, as nbrcases.many_runs(True) has them -- whose random sites put a pair inside the band
    between the selection radius and the query's"""
    rng = np.random.default_rng(77)
    c = np.zeros(361, dtype=int)
    c[rng.choice(361, 40, replace=False)] = rng.integers(1, 10, 40)
    return c


CASES = {}
for _t in (63, 64, 65, 128, 129):
    CASES[f"one_run-{_t}"] = (lambda _t=_t: line(_t, 100 + _t))
CASES["one_run-1"] = isolated
CASES["runs-64"] = lambda: pattern(np.full(64, 3), 8, 8, 201)
CASES["runs-65"] = lambda: pattern(np.full(65, 3), 13, 5, 202)
CASES["runs-361"] = lambda: pattern(_counts_sparse(), 19, 19, 207)
CASES["empties-a"] = lambda: pattern(_counts_empties_a(), 16, 8, 203)
CASES["empties-b"] = lambda: pattern(_counts_empties_b(), 16, 8, 204)
CASES["starts-63-64-65"] = lambda: pattern(_counts_starts(), 8, 8, 205)
CASES["one_cell-3x300"] = one_cell
CASES["over_window"] = lambda: pattern([260] * 8 + [150], 3, 3, 206, xspan=44.0, slack=0.8)
RANKS = "starts-63-64-65"          # the 129-agent scene whose two emulated ranks (chunks of 65 and 64) are queried in turn


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()
