"""Test helper: route planning round static vehicles (dmpc_plan_routes) -- the pinned rule of include/dmpc_hip.h restated literally in numpy and
plain Python, the scenes the tests use, and a raw ctypes call of the entry.

There is no reference counterpart (DMPC has no global planner).  The rule, per scene and commanded agent i (every fp64 operation rounded on its
own, everything after the blocked predicate integer arithmetic):
  grid      n_a = max(1, ceil((pmax_a - pmin_a) / cell)); cell of p = clamp(floor((p_a - pmin_a) / cell), 0, n_a - 1); centre = pmin_a + (i_a + 0.5) cell
  blocked   some obstacle m with (dx*dx + dy*dy) + dz*dz < R*R, dx, dy = centre - obst_m, dz = (centre - obst_m)_z * (1.0 / c), R = rmin + margin
  free_i    !blocked(q) or q == s_i (cell of po_i) or q == g_i (cell of goal_i)
  field     D(g_i) = 0, level L+1 = the unlabelled free_i cells with a 6-neighbour at level L, until s_i is labelled or a level adds nothing
  descent   from c_t the first neighbour in the order -x, +x, -y, +y, -z, +z with D = D(c_t) - 1
  clear     L = max_axis |b - a|; for j = 0 .. 2L the cell (2L a + j (b - a) + L) // (2L) per axis must be free_i
  pruning   t0 = 0; until t0 == H: t1 = the largest t > t0 that is t0 + 1 or has clear(c_t0, c_t); emit t1; t0 = t1
  output    a waypoint is the centre of c_t, an emitted t == H the goal itself; more than W emissions: the first W - 1, then the goal, TRUNCATED
"""
import ctypes as C
import functools
import math

import numpy as np

import route as rt
from obstacles import KW, _dp, _ip, _f   # noqa: F401

OK, TRUNCATED, UNREACHABLE = 0, 1, 2
MAX_CELLS = 32768
NBR = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------
def grid_shape(pmin, pmax, cell):
    return tuple(max(1, int(math.ceil((float(pmax[a]) - float(pmin[a])) / cell))) for a in range(3))


def cell_of(p, pmin, cell, n):
    """cells [..,3] (x, y, z) of points [..,3]"""
    p = np.asarray(p, dtype=np.float64)
    f = np.floor((p - np.asarray(pmin, dtype=np.float64)) / cell)
    return np.clip(f, 0, np.asarray(n) - 1).astype(np.int64)


def centres(pmin, cell, n):
    """three arrays [n_a]: pmin_a + (i + 0.5) * cell"""
    return [float(pmin[a]) + (np.arange(n[a], dtype=np.float64) + 0.5) * cell for a in range(3)]


def blocked_grid(obst, pmin, pmax, cell, margin, rmin, c):
    """bool [nx, ny, nz]"""
    n = grid_shape(pmin, pmax, cell)
    cx, cy, cz = centres(pmin, cell, n)
    cinv = 1.0 / c
    R = rmin + margin
    RR = R * R
    out = np.zeros(n, dtype=bool)
    for m in np.asarray(obst, dtype=np.float64).reshape(-1, 3):
        dx, dy, dz = cx - m[0], cy - m[1], (cz - m[2]) * cinv
        d2 = (dx * dx)[:, None, None] + (dy * dy)[None, :, None]
        out |= (d2 + (dz * dz)[None, None, :]) < RR
    return out


def field(free, s, g):
    """level-synchronous sweep from g over the free cells until s is labelled or a level adds nothing; int32 [nx,ny,nz], -1: unlabelled"""
    D = np.full(free.shape, -1, dtype=np.int32)
    D[g] = 0
    L = 0
    while D[s] < 0:
        at = D == L
        near = np.zeros_like(at)
        near[1:] |= at[:-1]; near[:-1] |= at[1:]
        near[:, 1:] |= at[:, :-1]; near[:, :-1] |= at[:, 1:]
        near[:, :, 1:] |= at[:, :, :-1]; near[:, :, :-1] |= at[:, :, 1:]
        new = near & free & (D < 0)
        if not new.any():
            break
        D[new] = L + 1
        L += 1
    return D


def descend(D, s):
    path = [s]
    n = D.shape
    while D[path[-1]] > 0:
        cur = path[-1]
        for d in NBR:
            q = (cur[0] + d[0], cur[1] + d[1], cur[2] + d[2])
            if all(0 <= q[a] < n[a] for a in range(3)) and D[q] == D[cur] - 1:
                path.append(q)
                break
        else:
            raise AssertionError("the field has no way down")
    return path


def clear(free, a, b):
    L = max(abs(b[k] - a[k]) for k in range(3))
    for j in range(2 * L + 1):
        q = tuple((2 * L * a[k] + j * (b[k] - a[k]) + L) // (2 * L) for k in range(3))
        if not free[q]:
            return False
    return True


def prune(free, path):
    """the emitted path indices"""
    H = len(path) - 1
    out, t0 = [], 0
    while t0 != H:
        t1 = t0 + 1
        for t in range(H, t0 + 1, -1):
            if clear(free, path[t0], path[t]):
                t1 = t
                break
        out.append(t1)
        t0 = t1
    return out


def plan_agent(blocked, po, goal, pmin, cell, W):
    """one agent on a scene's blocked grid: (waypoints [W,3], n_wp, status, hops, dict(path, emitted, free))"""
    n = blocked.shape
    s, g = tuple(int(v) for v in cell_of(po, pmin, cell, n)), tuple(int(v) for v in cell_of(goal, pmin, cell, n))
    free = ~blocked
    free[s] = True
    free[g] = True
    wp = np.tile(np.asarray(goal, dtype=np.float64), (W, 1))
    D = field(free, s, g)
    if D[s] < 0:
        return wp, 1, UNREACHABLE, -1, dict(path=None, emitted=[], free=free)
    path = descend(D, s)
    H = len(path) - 1
    assert H == D[s]
    if H == 0:
        return wp, 1, OK, 0, dict(path=path, emitted=[], free=free)
    em = prune(free, path)
    cx, cy, cz = centres(pmin, cell, n)
    status, keep = OK, em
    if len(em) > W:
        status, keep = TRUNCATED, em[:W - 1] + [H]
    for k, t in enumerate(keep):
        if t != H:
            q = path[t]
            wp[k] = (cx[q[0]], cy[q[1]], cz[q[2]])
    return wp, len(keep), status, H, dict(path=path, emitted=em, free=free)


def plan(po_cmd, goals, obst, cell, margin, W, kw=KW, detail=False):
    """dmpc_plan_routes restated.  po_cmd, goals [S,N_cmd,3], obst [S,M,3] (M may be 0) or None -> dict(waypoints [S,N_cmd,W,3], n_wp, plan_status,
    hops [S,N_cmd] int32) and, with detail, info [S][N_cmd]"""
    po_cmd, goals = np.asarray(po_cmd, dtype=np.float64), np.asarray(goals, dtype=np.float64)
    S, nc = po_cmd.shape[:2]
    wp = np.zeros((S, nc, W, 3))
    n_wp, st, hops = (np.zeros((S, nc), dtype=np.int32) for _ in range(3))
    info = []
    for s in range(S):
        ob = np.zeros((0, 3)) if obst is None else np.asarray(obst[s], dtype=np.float64)
        blocked = blocked_grid(ob, kw["pmin"], kw["pmax"], cell, margin, kw["rmin"], kw["c"])
        assert blocked.size <= MAX_CELLS
        row = []
        for i in range(nc):
            wp[s, i], n_wp[s, i], st[s, i], hops[s, i], d = plan_agent(blocked, po_cmd[s, i], goals[s, i], kw["pmin"], cell, W)
            row.append(d)
        info.append(row)
    out = dict(waypoints=wp, n_wp=n_wp, plan_status=st, hops=hops)
    if detail:
        out["info"] = info
    return out


KEYS = ("waypoints", "n_wp", "plan_status", "hops")


def same(out, ref, what=""):
    """the device's dict against the restatement's, byte for byte"""
    for k in KEYS:
        a, b = np.asarray(out[k]), np.asarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)[:4].tolist()
            raise AssertionError(f"{what}: {k} differs at {bad}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}")


def bfs_hops(free, s, g):
    """an independent queue BFS over the free cells: the number of 6-steps from s to g, -1 if there is no way"""
    from collections import deque
    n = free.shape
    seen = {s: 0}
    q = deque([s])
    while q:
        cur = q.popleft()
        if cur == g:
            return seen[cur]
        for d in NBR:
            nx = (cur[0] + d[0], cur[1] + d[1], cur[2] + d[2])
            if all(0 <= nx[a] < n[a] for a in range(3)) and free[nx] and nx not in seen:
                seen[nx] = seen[cur] + 1
                q.append(nx)
    return -1


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
WALL_GRIDS = ((0.25, 0.2), (0.2, 0.15), (0.3, 0.2))     # (cell, margin)


def wall():
    """route.wall() without its hand-made waypoints: dict(po [24,3], goals [3,3], kw)"""
    s = rt.wall()
    return dict(po=s["po"], goals=rt.WALL_START * np.array([-1.0, 1.0, 1.0]), kw=KW, capture=s["capture"], K_T_max=s["K_T_max"],
                error_tol=s["error_tol"])


def small_cases():
    """the table of small cases in ONE shape (2 agents, 26 obstacle points -- unused points rest far outside the box --, cell 0.5, margin 0, W 4,
    KW's box and rmin): [(name, po [2,3], goals [2,3], obst [26,3])]"""
    far = np.array([50.0, 50.0, 50.0])
    pad = lambda pts: np.vstack([np.asarray(pts, dtype=np.float64).reshape(-1, 3), np.tile(far, (26 - len(pts), 1))])
    g0 = np.array([1.25, 0.25, 1.45])                                       # the centre of cell (7, 5, 2)
    shell = [g0 + 0.5 * np.array(d) for d in NBR]                           # the six neighbours' centres: R = 0.35 blocks each of them and nothing else
    cases = [
        ("same-cell", [(-1.1, -1.1, 1.3), (0.3, 0.3, 0.8)], [(-1.4, -1.3, 1.4), (0.45, 0.05, 0.75)], pad([(0.0, 0.0, 1.2)])),
        ("start-blocked", [(-1.2, 0.3, 1.2), (-1.3, -0.2, 1.2)], [(1.2, 0.2, 1.2), (1.3, -0.3, 1.2)], pad([(-1.25, 0.25, 1.2), (-1.25, -0.25, 1.2), (0.0, 0.0, 1.2)])),
        ("goal-blocked", [(-1.2, 0.3, 1.2), (-1.3, -0.2, 1.2)], [(1.2, 0.2, 1.2), (1.3, -0.3, 1.2)], pad([(1.25, 0.25, 1.2), (1.25, -0.25, 1.2), (0.0, 0.0, 1.2)])),
        ("enclosed", [(-1.2, 0.3, 1.2), (2.0, 2.0, 0.5)], [tuple(g0), tuple(g0)], pad(shell)),
        ("outside", [(-4.0, 0.1, 1.2), (0.2, -3.7, 5.0)], [(6.0, 0.3, -1.0), (0.1, 9.0, 1.0)], pad([(0.0, 0.0, 1.2), (0.0, 0.4, 1.2), (0.0, -0.4, 1.2)])),
    ]
    return [(name, np.array(po, dtype=np.float64), np.array(g, dtype=np.float64), ob) for name, po, g, ob in cases]


SMALL = dict(cell=0.5, margin=0.0, W=4)

FLAT_KW = dict(KW, pmin=(-2.5, -2.5, 1.0), pmax=(2.5, 2.5, 1.1))            # thinner than one cell in z: n_z = 1


def flat():
    """two agents round a short wall in a box of one layer (cell 0.25: 20 x 20 x 1)"""
    obst = np.array([(0.0, y, 1.05) for y in np.arange(-0.75, 0.76, 0.25)])
    po = np.array([(-1.0, 0.1, 1.05), (1.1, -0.2, 1.02)])
    return dict(po=po, goals=po * np.array([-1.0, 1.0, 1.0]), obst=obst, kw=FLAT_KW, cell=0.25, margin=0.0)


MAZE_KW = dict(KW, rmin=0.1, pmin=(-2.5, -2.5, 1.0), pmax=(2.5, 2.5, 1.1))


def maze():
    """nine walls of obstacle points at x = -2 : 0.5 : 2 (on cell faces: R = 0.1 blocks the cell columns on both sides), one point per cell row,
    three rows open at alternating ends; one agent from (-2.2, -2.2) to (2.2, 2.2) on a grid of 40 x 40 x 1: hops = 350, 18 waypoints"""
    ys = np.arange(-2.4375, 2.5, 0.125)                                     # the cell centres in y
    pts = []
    for k, x in enumerate(np.arange(-2.0, 2.01, 0.5)):
        gap = ys > ys[-4] + 1e-9 if k % 2 == 0 else ys < ys[3] - 1e-9
        pts += [(x, y, 1.05) for y in ys[~gap]]
    return dict(po=np.array([(-2.2, -2.2, 1.05)]), goals=np.array([(2.2, 2.2, 1.05)]), obst=np.array(pts), kw=MAZE_KW, cell=0.125, margin=0.0)


CAP_KW = dict(KW, rmin=1.0, pmin=(0.0, 0.0, 0.0), pmax=(8.0, 8.0, 8.0))


def cap():
    """32 x 32 x 32 = 32768 cells, one obstacle with R = 1.5 in the middle, two agents across it"""
    return dict(po=np.array([(0.4, 4.1, 4.1), (7.7, 7.6, 0.3)]), goals=np.array([(7.6, 3.9, 3.9), (0.2, 0.3, 7.8)]), obst=np.array([(4.0, 4.0, 4.0)]),
                kw=CAP_KW, cell=0.25, margin=0.5)


def batch5(nc=70, M=12):
    """five scenes of nc agents with different obstacle sets in KW's box: dict(po, goals [5,nc,3], obst [5,M,3])"""
    rng = np.random.default_rng(4242)
    lo, hi = np.array(KW["pmin"]), np.array(KW["pmax"])
    po, goals = rng.uniform(lo, hi, (5, nc, 3)), rng.uniform(lo, hi, (5, nc, 3))
    obst = rng.uniform(lo + 0.5, hi - 0.5, (5, M, 3))
    obst[1, :, 0] = 0.0                                                     # a scene with a partial wall
    obst[3] = obst[3, 0]                                                    # a scene with one obstacle, repeated
    return dict(po=po, goals=goals, obst=obst, cell=0.25, margin=0.1)


@functools.lru_cache(maxsize=None)
def result(name, *args):
    """the restatement on a named scene, computed once per session (shared by the tests: do not modify)"""
    if name == "wall":
        s, (cell, margin) = wall(), args
        return plan(s["po"][None, :3], s["goals"][None], s["po"][None, 3:], cell, margin, 4, KW, detail=True)
    if name == "flat":
        s = flat()
        return plan(s["po"][None], s["goals"][None], s["obst"][None], s["cell"], s["margin"], 4, s["kw"], detail=True)
    if name == "maze":
        s, (W,) = maze(), args
        return plan(s["po"][None], s["goals"][None], s["obst"][None], s["cell"], s["margin"], W, s["kw"], detail=True)
    if name == "cap":
        s = cap()
        return plan(s["po"][None], s["goals"][None], s["obst"][None], s["cell"], s["margin"], 4, s["kw"], detail=True)
    if name == "small":
        cs = small_cases()
        return plan(np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs]), np.stack([c[3] for c in cs]), SMALL["cell"], SMALL["margin"], SMALL["W"],
                    KW, detail=True)
    if name == "batch5":
        b = batch5()
        return plan(b["po"], b["goals"], b["obst"], b["cell"], b["margin"], 4, KW)
    raise KeyError(name)


# ---- raw call of the entry ----------------------------------------------------------------------------------------------------------------------
def raw_plan(d, S, nc, M, W, po, goals, obst, cell, margin, outputs=(1, 1, 1, 1), ctx="own"):
    """dmpc_plan_routes with the shapes as given (po, goals, obst: arrays or None for a NULL pointer).  Returns (rc, message, dict)."""
    po, goals, obst = (None if a is None else _f(a) for a in (po, goals, obst))
    s, n, w = max(S, 1), max(nc, 1), max(W, 1)
    out = dict(waypoints=np.zeros((s, n, w, 3)), n_wp=np.zeros((s, n), dtype=np.int32), plan_status=np.zeros((s, n), dtype=np.int32),
               hops=np.zeros((s, n), dtype=np.int32))
    ptr = [(_dp if k == "waypoints" else _ip)(out[k] if on else None) for k, on in zip(KEYS, outputs)]
    h = d._ctx if ctx == "own" else ctx
    rc = d._L.dmpc_plan_routes(h, int(S), int(nc), int(M), int(W), _dp(po), _dp(goals), _dp(obst), C.c_double(cell), C.c_double(margin), *ptr)
    return rc, d._L.dmpc_last_error(h).decode(), out
