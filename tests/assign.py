"""Test helper: goal assignment (dmpc_assign_goals) -- a literal numpy restatement of the forward auction with eps-scaling in synchronous
(Jacobi) rounds that include/dmpc_hip.h pins, the scenes the tests use, and a raw ctypes call of the entry.

There is no reference counterpart (the reference plans a labelled problem).  The device must agree with auction() bit for bit in perm, price,
rounds and cost; what auction() itself is worth is checked against scipy.optimize.linear_sum_assignment (tests/test_assign_cpu.py).

  cost     cinv = 1 / c; dx, dy = po_i - g_j; dz = (po_i - g_j)_z * cinv; c(i,j) = (dx*dx + dy*dy) + dz*dz, every operation rounded on its own
  schedule cmax = max c(i,j); price = 0; e = cmax / 4; while e > eps: phase(e); e = e / 4; then phase(eps)
  phase    every agent unassigned, prices kept; rounds until nobody is unassigned
  round    every unassigned i: m_j = c(i,j) + price_j; j1 = the smallest m (ties: the smallest j); m2 = the smallest m over j != j1;
           bid = (price_j1 + (m2 - m1)) + e (N == 1: price_0 + e).  Then every goal with bids goes to its highest bidder (ties: the smallest i),
           its price becomes that bid, its previous owner becomes unassigned.
  cap      a scene that would need more than max_rounds rounds reports rounds = -1, perm = -1, cost = NaN, pf = 0
"""
import ctypes as C
import functools

import numpy as np

DEFAULT_ROUNDS = 1 << 20


def cost_matrix(po, goals, c):
    """c(i,j) [N,N], rounded as the kernel rounds it"""
    po, goals = np.asarray(po, dtype=np.float64), np.asarray(goals, dtype=np.float64)
    cinv = np.float64(1.0) / np.float64(c)
    dx = po[:, None, 0] - goals[None, :, 0]
    dy = po[:, None, 1] - goals[None, :, 1]
    dz = (po[:, None, 2] - goals[None, :, 2]) * cinv
    return (dx * dx + dy * dy) + dz * dz


def auction(po, goals, c, eps, max_rounds=0):
    """One scene: po, goals [N,3].  Returns dict(perm [N] int32, pf [N,3], price [N], cost, rounds, phases, cmax)."""
    po, goals = np.asarray(po, dtype=np.float64), np.asarray(goals, dtype=np.float64)
    N = po.shape[0]
    cap = DEFAULT_ROUNDS if max_rounds <= 0 else int(max_rounds)
    eps = np.float64(eps)
    Cm = cost_matrix(po, goals, c)
    cmax = Cm.max()
    price = np.zeros(N)
    owner = np.full(N, -1, dtype=np.int64)      # per goal
    assigned = np.full(N, -1, dtype=np.int64)   # per agent
    rounds = phases = 0
    cols = np.arange(N)

    def phase(e):
        nonlocal rounds
        owner[:] = -1
        assigned[:] = -1
        while True:
            U = np.flatnonzero(assigned < 0)
            if U.size == 0:
                return True
            if rounds + 1 > cap:
                return False
            rounds += 1
            if N == 1:
                j1 = np.zeros(1, dtype=np.int64)
                bid = price[j1] + e
            else:
                M = Cm[U] + price[None, :]
                j1 = np.argmin(M, axis=1)                     # the first smallest: ties go to the smallest j
                r = np.arange(U.size)
                m1 = M[r, j1]
                M[r, j1] = np.inf
                m2 = M.min(axis=1)
                bid = (price[j1] + (m2 - m1)) + e
            # the highest bid per goal, ties to the smallest agent: U is increasing, a stable sort by (goal, -bid) keeps it so
            order = np.lexsort((U, -bid, j1))
            first = np.ones(order.size, dtype=bool)
            first[1:] = j1[order][1:] != j1[order][:-1]
            win = order[first]
            g, a = j1[win], U[win]
            prev = owner[g]
            assigned[prev[prev >= 0]] = -1
            owner[g] = a
            assigned[a] = g
            price[g] = bid[win]

    ok = True
    e = cmax / np.float64(4.0)
    while ok and e > eps:
        phases += 1
        ok = phase(e)
        e = e / np.float64(4.0)
    if ok:
        phases += 1
        ok = phase(eps)
    if not ok:
        return dict(perm=np.full(N, -1, dtype=np.int32), pf=np.zeros((N, 3)), price=price, cost=np.float64(np.nan), rounds=-1, phases=phases,
                    cmax=cmax)
    perm = assigned.astype(np.int32)
    cost = np.float64(0.0)
    for i in range(N):
        cost = cost + Cm[i, perm[i]]
    return dict(perm=perm, pf=goals[perm].copy(), price=price, cost=cost, rounds=rounds, phases=phases, cmax=cmax)


def auction_batch(po, goals, c, eps, max_rounds=0):
    """po, goals [S,N,3] -> the arrays Dmpc.assign returns"""
    r = [auction(p, g, c, eps, max_rounds) for p, g in zip(po, goals)]
    return dict(perm=np.stack([x["perm"] for x in r]), pf=np.stack([x["pf"] for x in r]), price=np.stack([x["price"] for x in r]),
                cost=np.array([x["cost"] for x in r]), rounds=np.array([x["rounds"] for x in r], dtype=np.int32))


def slack(po, goals, c, perm, price):
    """per agent: max_j v_j - v_perm[i], v_j = -(c(i,j) + price_j); and cmax"""
    Cm = cost_matrix(po, goals, c)
    M = Cm + np.asarray(price)[None, :]
    return M[np.arange(len(perm)), perm] - M.min(axis=1), Cm.max()


def optimum(po, goals, c):
    """(cost, column indices) of scipy.optimize.linear_sum_assignment on the same cost matrix; the cost added in increasing i"""
    from scipy.optimize import linear_sum_assignment
    Cm = cost_matrix(po, goals, c)
    r, col = linear_sum_assignment(Cm)
    tot = np.float64(0.0)
    for i in range(len(r)):
        tot = tot + Cm[i, col[i]]
    return tot, col


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
C_LATTICE = 2.0     # with c = 2 and points on a 0.25 m lattice every c(i,j) is a multiple of 1/64: all sums are exact


@functools.lru_cache(maxsize=None)
def _lattice(N, seed):
    rng = np.random.default_rng(7000 + 31 * seed + N)
    side = max(4, int(np.ceil((4.0 * N) ** (1.0 / 3.0))) + 1)      # at least four times as many lattice points as agents

    def pts():
        idx = rng.choice(side ** 3, size=N, replace=False)
        return np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1).astype(np.float64) * 0.25
    return pts(), pts()


def lattice(N, seed=0):
    """(po, goals) [N,3]: two sets of N distinct points each on a 0.25 m lattice (shared by the tests: copies)"""
    po, g = _lattice(N, seed)
    return po.copy(), g.copy()


def lattice_eps(N):
    return 1.0 / (128.0 * N)


def uniform(N, seed=0):
    rng = np.random.default_rng(9000 + 17 * seed + N)
    return rng.uniform(-2.5, 2.5, (N, 3)), rng.uniform(-2.5, 2.5, (N, 3))


def exchange(N, seed=0):
    """goals = the starts, permuted"""
    rng = np.random.default_rng(9500 + 13 * seed + N)
    po = rng.uniform(-2.5, 2.5, (N, 3))
    return po, po[rng.permutation(N)].copy()


@functools.lru_cache(maxsize=None)
def lattice_result(N, seed=0):
    """auction() on lattice(N, seed) at lattice_eps(N), computed once per session (shared by the tests: do not modify)"""
    po, g = lattice(N, seed)
    return auction(po, g, C_LATTICE, lattice_eps(N))


def same(out, ref, s=None):
    """the device's dict (scene s of it) equals the restatement's bit for bit; returns the name of the first array that differs, or None"""
    for k in ("perm", "price", "rounds", "cost", "pf"):
        a = np.asarray(out[k] if s is None else out[k][s])
        b = np.asarray(ref[k])
        if a.shape != b.shape or a.tobytes() != b.astype(a.dtype).tobytes():
            return k
    return None


# ---- raw call of the entry ------------------------------------------------------------------------------------------------------------
def raw_assign(d, S, N, po, goals, eps, max_rounds=0):
    """dmpc_assign_goals with the arguments as given (po / goals: arrays or None for a NULL pointer).  Returns (rc, message)."""
    dp = C.POINTER(C.c_double)
    keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (po, goals)]
    ptr = [a.ctypes.data_as(dp) if a is not None else dp() for a in keep]
    n = max(S, 1) * max(N, 1)
    perm, pf, price = np.zeros(n, dtype=np.int32), np.zeros(3 * n), np.zeros(n)
    cost, rounds = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    rc = d._L.dmpc_assign_goals(d._ctx, int(S), int(N), ptr[0], ptr[1], C.c_double(eps), int(max_rounds),
                                perm.ctypes.data_as(C.POINTER(C.c_int32)), pf.ctypes.data_as(dp), price.ctypes.data_as(dp),
                                cost.ctypes.data_as(dp), rounds.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, d._L.dmpc_last_error(d._ctx).decode()
