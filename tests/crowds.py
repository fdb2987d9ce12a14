"""Synthetic crowd scenes: a probe agent (index 0) with an exact, chosen number of collision rows at a chosen horizon step.

Not a conftest: a plain helper of tests/test_crowds_cpu.py and tests/test_gpu_capacity.py.  Every scene is closed-form (no random
numbers).  The prediction table `l` is written directly -- it is an input of the MPC step and needs no previous solve.

Geometry, in the scaled metric of the scan (x, y, z / c): the probe sits still at P0.  Its neighbours are points of a face-centred
cubic lattice about P0 (spacing `s`), taken in increasing distance; at the horizon steps where a neighbour is not "present" it is
parked on a plane 2.5 m away (beyond every neighbour radius: 3 rmin for the soft variants, 1 for the hard rows).  One extra
neighbour, the violator, sits at 1.2 rmin from the probe before the violating step `kc` and inside rmin from `kc` on, so that
the probe's first violation is exactly at `kc` and nothing is within rmin - 0.05 of it at step 1.  The workspace is large
enough that no wall is near.  Neighbours may collide with each other: they are solved and compared like the probe.
"""
import numpy as np

K = 15
RMIN = 0.35
P0 = np.zeros(3)   # (the origin: offsets along one axis are then exact table entries)
BOX = dict(pmin=(-40.0, -40.0, -40.0), pmax=(40.0, 40.0, 40.0))
VDIR = np.array([0.31, 0.53, 0.79]) / np.linalg.norm([0.31, 0.53, 0.79])   # the violator's direction (scaled metric): on no lattice axis


def solver_kw(rmin=RMIN, c=2.0, **over):
    kw = dict(rmin=rmin, c=c, alim=1.0, Q1=1000.0, S1=100.0, term=-5e4, h=0.2, **BOX)
    kw.update(over)
    return kw


def fcc(spacing, radius):
    """FCC points (scaled metric) with 0 < |u| < radius, sorted by distance, then lexicographically: shells fill in a fixed order"""
    a = spacing / np.sqrt(2.0)
    n = int(np.ceil(radius / a)) + 1
    g = np.arange(-n, n + 1)
    i, j, k = np.meshgrid(g, g, g, indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), k.ravel()], 1)
    pts = pts[(pts.sum(1) % 2) == 0]
    r2 = (pts ** 2).sum(1)
    keep = (r2 > 0) & (r2 * a * a < radius * radius)
    pts, r2 = pts[keep], r2[keep]
    order = np.lexsort((pts[:, 2], pts[:, 1], pts[:, 0], r2))
    return pts[order] * a


def cpp_radius(rmin, k):
    """DMPC::solveQPv2's neighbour radius at 1-based horizon step k: _rmin*(1+(float)(k-1)/_k_hor), every operand a float"""
    f = np.float32
    return float(f(rmin) * (f(1.0) + f(k - 1) / f(K)))


def _park(i):
    """parking place of neighbour i: a plane x = 2.5 m off the probe, 0.4 m apart along y and 0.8 m (0.4 scaled at c = 2) along z"""
    return P0 + np.array([2.5, 0.4 * (i % 24 - 11.5), 0.8 * (i // 24 - 7.5)])


def scene(offsets, present, c=2.0, violator=None, goal=(1.0, 0.0, 0.0)):
    """offsets [M,3]: neighbours' positions relative to P0 in the scaled metric; present [M,K] bool: steps at which neighbour m is
    at its offset (parked otherwise).  violator: (kc, near_offset, far_offset) -- an extra neighbour at far_offset before step kc
    (1-based) and at near_offset from kc on.  Returns l [N,45], x_p, x_v, x_a, pf (probe = 0)."""
    offsets = np.asarray(offsets, dtype=np.float64).reshape(-1, 3)
    present = np.asarray(present, dtype=bool).reshape(len(offsets), K)
    M = len(offsets) + (violator is not None)
    N = M + 1
    l = np.zeros((N, K, 3))
    l[0] = P0
    scale = np.array([1.0, 1.0, c])
    for m in range(len(offsets)):
        l[m + 1] = np.where(present[m][:, None], P0 + offsets[m] * scale, _park(m))
    if violator is not None:
        kc, near, far = violator
        steps = np.arange(1, K + 1)[:, None]
        l[M] = np.where(steps >= kc, P0 + np.asarray(near) * scale, P0 + np.asarray(far) * scale)
    x_p = l[:, 0].copy()
    z = np.zeros_like(x_p)
    pf = x_p.copy()
    pf[0] = P0 + np.asarray(goal)
    return l.reshape(N, 3 * K), x_p, z, z.copy(), pf


def soft_crowd(variant, rows, kc=10, rmin=RMIN, c=2.0, spacing=None, depth=0.8):
    """probe with exactly `rows` collision rows in a soft variant (bound, bound2, cpp, cpp2: one row per selected neighbour;
    all3: three rows per selected neighbour, kc in 3..K-1).  `kc`: the probe's first violating step (1-based; >= 2).  The rows
    constrain step kc (bound2 / cpp2: kc - 1); late steps by default, so that every row can become active within the reach of
    |a| <= alim and none is pruned.  depth: the violator's distance at kc, in rmin."""
    assert kc >= 2
    per = 3 if variant == "all3" else 1
    assert rows % per == 0 and rows >= per
    M = rows // per
    cpp = variant in ("cpp", "cpp2")
    R = cpp_radius(rmin, kc) if cpp else 3.0 * rmin
    s = spacing or (0.6 * rmin if cpp else 1.02 * rmin)     # (cpp: a radius of 1.07-1.93 rmin holds few points 1.02 rmin apart)
    lat = fcc(s, R * 0.985)
    lat = lat[np.linalg.norm(lat, axis=1) >= 1.02 * rmin]   # (nothing else inside rmin of the probe)
    assert len(lat) >= M - 1, f"{variant}: {len(lat)} lattice points inside the neighbour radius, {M - 1} wanted"
    off = lat[:M - 1]
    present = np.zeros((M - 1, K), dtype=bool)
    present[:, (kc - 2 if variant == "all3" else kc - 1):] = True   # (all3: rows on steps kc-1, kc, kc+1)
    return scene(off, present, c=c, violator=(kc, depth * rmin * VDIR, 1.2 * rmin * VDIR))


def hard_crowd(pairs, first=10, rmin=RMIN, c=2.0, spacing=None):
    """probe with exactly `pairs` (step, neighbour) pairs at scaled distance < 1 (solveHardDMPC's rows, CollConstrHardDMPC.m:19),
    all on steps first..K (late enough that the reach of |a| <= alim covers distance 1: no row is pruned).  No neighbour within
    rmin of the probe.  q neighbours are present on all K - first + 1 steps, one more on the remaining pairs' steps."""
    ns = K - first + 1
    q, r = divmod(pairs, ns)
    M = q + (r > 0)
    def outside(s):
        lat = fcc(s, 0.985)
        return lat[np.linalg.norm(lat, axis=1) >= 1.02 * rmin]
    s = spacing
    if s is None:
        s = 1.02 * rmin
        while len(outside(s)) < M:
            s *= 0.97
    lat = outside(s)
    assert len(lat) >= M, f"hard: {len(lat)} lattice points, {M} wanted"
    present = np.zeros((M, K), dtype=bool)
    present[:q, first - 1:] = True
    if r:
        present[q, first - 1:first - 1 + r] = True
    return scene(lat[:M], present, c=c)


def ladder_crowd(variant, rows, kc=10, rmin=RMIN, c=2.0):
    """soft_crowd whose violator is nearly on top of the probe (0.03 rmin): the lattice neighbour opposite to it, at 1.02 rmin,
    pins the probe, the level-0 slack bounds cannot separate them and the retry ladder climbs"""
    return soft_crowd(variant, rows, kc=kc, rmin=rmin, c=c, depth=0.03)


CORNER_BOX = dict(pmin=(-2.0, -2.0, -2.0), pmax=(1.0, 1.0, 1.0))
CORNER_KC = 6


def corner_hard_rows(fourth=False, rmin=RMIN, c=2.0):
    """the three-wall corner of the wall-limit test (a probe at rest 1 m from the corner (1, 1, 1) of its box, the goal 0.2 m beyond it: its
    last step ends on three walls) with three neighbours in general position just ahead of it, in the cone about the diagonal: two at
    rmin + 0.005 and rmin + 0.0075 at every step, the violator at rmin - 0.0025 from step 6 on.  Their planes meet in a vertex a few
    millimetres from the probe's start, the pull toward the goal presses the probe into it with multipliers of 80 ... 700 -- far below the
    slack penalty of 5e4, so all three slacks stay pinned at zero: three HARD rows on step kc = 6, and three walls on step 15.
    fourth: one more neighbour inside the cone at 1.01 rmin, whose plane cuts the vertex off: its row becomes active (hard), the first
    neighbour's row gives way -- the entering row meets three hard rows that already span w_kc.  Returns (solver kw, scene)."""
    dirs = [(1.0, 0.2, 0.1), (0.2, 1.0, 0.3)] + ([(0.6, 0.5, 0.55)] if fourth else [])
    dist = [rmin + 0.005, rmin + 0.0075] + ([1.01 * rmin] if fourth else [])
    off = [np.asarray(d) / np.linalg.norm(d) * r for d, r in zip(dirs, dist)]
    vd = np.array([0.3, 0.1, 1.0]) / np.linalg.norm([0.3, 0.1, 1.0])
    sc = scene(off, np.ones((len(off), K), dtype=bool), c=c, violator=(CORNER_KC, (rmin - 0.0025) * vd, 1.2 * rmin * vd), goal=(1.2, 1.2, 1.2))
    return solver_kw(rmin=rmin, c=c, **CORNER_BOX), sc


def row_capacity(variant, N):
    """rows per agent the scan builds (row_capacity in dmpc_launch.hip): want = rows of the worst case, capped per variant, at least 8,
    rounded up to an even number; one row more sets DMPC_ST_CAPACITY"""
    nb = N - 1 if N > 1 else 1
    if variant in ("hard", "scp"):
        want, cap = K * nb, (640 if variant == "hard" else 4096)
    elif variant == "all3":
        want, cap = 3 * nb, 384
    elif variant in ("bound", "bound2", "ondemand", "cpp", "cpp2"):
        want, cap = nb, 128
    else:                                               # ellip, softall, repair (and the other all-neighbour variants)
        want, cap = nb, 4096
    r = max(min(want, cap), 8)
    return (r + 1) & ~1


TIE_KINDS = ("rmin", "3rmin", "hard1", "cut", "cpp", "cppcut")


def threshold(kind, rmin, kc=5):
    """the distance thresholds of the scan, with the reference's own arithmetic"""
    f = np.float32
    return {"rmin": rmin, "3rmin": rmin * 3, "hard1": 1.0, "cut": rmin - 0.05, "cpp": cpp_radius(rmin, kc),
            "cppcut": float(f(rmin) - f(0.05))}[kind]


def tie_scene(kind, d, axis, c=2.0, kc=5):
    """the probe and one neighbour at scaled distance d along one axis ('x' or 'z'), placed for threshold `kind`:
    rmin / hard1: from step kc on (2 before); 3rmin / cpp: the same, with the violator of soft_crowd making step kc violating;
    cut / cppcut: at every step (the first step decides ST_COLL).  The z offset is written d * c: the scan's dz / c (or dz * (1/c))
    returns d exactly when c is a power of two.  With one non-zero component, sqrt(x*x) == |x| makes the distance exact."""
    u = np.zeros(3)
    u[{"x": 0, "z": 2}[axis]] = 1.0
    scale = np.array([1.0, 1.0, c])
    first = 1 if kind in ("cut", "cppcut") else kc
    vio = kind in ("3rmin", "cpp")
    N = 3 if vio else 2
    rmin = RMIN
    l = np.zeros((N, K, 3))
    l[0] = P0
    steps = np.arange(1, K + 1)[:, None]
    l[1] = np.where(steps >= first, P0 + u * d * scale, P0 + u * 2.0 * scale)
    if vio:
        l[2] = np.where(steps >= kc, P0 - 0.8 * rmin * VDIR * scale, P0 - 1.2 * rmin * VDIR * scale)
    x_p = l[:, 0].copy()
    z = np.zeros_like(x_p)
    pf = x_p.copy()
    pf[0] = P0 + np.array([1.0, 0.0, 0.0])
    return l.reshape(N, 3 * K), x_p, z, z.copy(), pf
