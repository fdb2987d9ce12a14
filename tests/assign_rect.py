"""Test helper: rectangular goal assignment (dmpc_assign_rect) -- a literal numpy restatement of the forward/reverse auction with eps-scaling
in synchronous (Jacobi) rounds that include/dmpc_hip.h pins, the scenes the tests use, and a raw ctypes call of the entry.

N agents, M goals, n = min(N, M), m = max(N, M).  The smaller side are the persons, the larger side the objects (agents are persons when
N <= M); c(p,o) is always the cost of the agent-goal pair, computed as tests/assign.py computes it.

  schedule cmax = max c; price = 0 per object; e = cmax / 4; while e > eps: forward(e); reverse(e); e = e / 4; then forward(eps); reverse(eps)
  forward  the phase of tests/assign.py with objects in the place of goals (m == 1: the bid is price_0 + e)
  reverse  nothing when n == m.  u_p = c(p, o_p) + price[o_p]; lam = the smallest price over the owned objects, fixed for the call; rounds until
           no object is unowned with price > lam.  In a round every such object o, from the state at the round's start, takes
           g_p = u_p - c(p,o) over all persons; p1 = the largest g (ties: the smallest p), beta = g_p1, omega = the largest over p != p1
           (n == 1: -inf).  lam >= beta - e: price[o] = lam, the object is done.  Else it offers delta = min(beta - lam, (beta - omega) + e)
           to p1.  Then every person with offers takes the largest delta (ties: the smallest o): price[o] = beta_o - delta, u_p = u_p - delta,
           the person's previous object becomes unowned with its price as it is, the person owns o.
  cap      rounds counts forward and reverse rounds alike; a scene that would need more than max_rounds reports rounds = -1, perm = -1,
           owner = -1, cost = NaN, pf = 0 and price as the rounds left it
  outputs  perm [N] (the goal of agent i or -1), owner [M] (the agent of goal j or -1), pf [N,3] = goals[perm[i]] or po_i where perm[i] = -1,
           price [m] per object, cost = the sum of c(i, perm[i]) over the assigned agents in increasing i
"""
import ctypes as C
import functools

import numpy as np

from assign import C_LATTICE, DEFAULT_ROUNDS, cost_matrix

KEYS = ("perm", "owner", "price", "rounds", "cost", "pf")


def auction_rect(po, goals, c, eps, max_rounds=0):
    """One scene: po [N,3], goals [M,3].  Returns dict(perm [N] int32, owner [M] int32, pf [N,3], price [max(N,M)], cost, rounds, and -- for the
    tests -- fwd, rev (the rounds of either kind), kinds (one 'f' or 'r' per round, in order), cmax)."""
    po, goals = np.asarray(po, dtype=np.float64), np.asarray(goals, dtype=np.float64)
    N, M = po.shape[0], goals.shape[0]
    n, m = min(N, M), max(N, M)
    cap = DEFAULT_ROUNDS if max_rounds <= 0 else int(max_rounds)
    eps = np.float64(eps)
    Cm = cost_matrix(po, goals, c)                       # [agent, goal]
    Cpo = Cm if N <= M else Cm.T                         # [person, object]
    cmax = Cm.max()
    price = np.zeros(m)
    owner = np.full(m, -1, dtype=np.int64)               # per object: its person
    assigned = np.full(n, -1, dtype=np.int64)            # per person: its object
    kinds = []

    def forward(e):
        owner[:] = -1
        assigned[:] = -1
        while True:
            U = np.flatnonzero(assigned < 0)
            if U.size == 0:
                return True
            if len(kinds) + 1 > cap:
                return False
            kinds.append("f")
            if m == 1:
                o1 = np.zeros(1, dtype=np.int64)
                bid = price[o1] + e
            else:
                V = Cpo[U] + price[None, :]
                o1 = np.argmin(V, axis=1)                 # the first smallest: ties go to the smallest o
                r = np.arange(U.size)
                v1 = V[r, o1]
                V[r, o1] = np.inf
                v2 = V.min(axis=1)
                bid = (price[o1] + (v2 - v1)) + e
            order = np.lexsort((U, -bid, o1))             # per object the highest bid, ties to the smallest person
            first = np.ones(order.size, dtype=bool)
            first[1:] = o1[order][1:] != o1[order][:-1]
            win = order[first]
            o, p = o1[win], U[win]
            prev = owner[o]
            assigned[prev[prev >= 0]] = -1
            owner[o] = p
            assigned[p] = o
            price[o] = bid[win]

    def reverse(e):
        if n == m:
            return True
        u = Cpo[np.arange(n), assigned] + price[assigned]
        lam = price[owner >= 0].min()
        while True:
            A = np.flatnonzero((owner < 0) & (price > lam))
            if A.size == 0:
                return True
            if len(kinds) + 1 > cap:
                return False
            kinds.append("r")
            G = u[:, None] - Cpo[:, A]                    # [person, offering object], from the state at the round's start
            r = np.arange(A.size)
            p1 = np.argmax(G, axis=0)                     # the first largest: ties go to the smallest p
            beta = G[p1, r]
            G[p1, r] = -np.inf
            omega = G.max(axis=0)                         # (n == 1: -inf)
            done = lam >= beta - e
            price[A[done]] = lam
            off = ~done
            o, p, b = A[off], p1[off], beta[off]
            delta = np.minimum(b - lam, (b - omega[off]) + e)
            order = np.lexsort((o, -delta, p))            # per person the largest offer, ties to the smallest object
            first = np.ones(order.size, dtype=bool)
            first[1:] = p[order][1:] != p[order][:-1]
            win = order[first]
            ow, pw, dw = o[win], p[win], delta[win]
            owner[assigned[pw]] = -1
            price[ow] = b[win] - dw
            u[pw] = u[pw] - dw
            owner[ow] = pw
            assigned[pw] = ow

    ok = True
    e = cmax / np.float64(4.0)
    while ok and e > eps:
        ok = forward(e) and reverse(e)
        e = e / np.float64(4.0)
    ok = ok and forward(eps) and reverse(eps)
    extra = dict(fwd=kinds.count("f"), rev=kinds.count("r"), kinds="".join(kinds), cmax=cmax)
    if not ok:
        return dict(perm=np.full(N, -1, dtype=np.int32), owner=np.full(M, -1, dtype=np.int32), pf=np.zeros((N, 3)), price=price,
                    cost=np.float64(np.nan), rounds=-1, **extra)
    perm, own = (assigned, owner) if N <= M else (owner, assigned)
    perm, own = perm.astype(np.int32), own.astype(np.int32)
    pf = po.copy()
    cost = np.float64(0.0)
    for i in range(N):
        if perm[i] >= 0:
            pf[i] = goals[perm[i]]
            cost = cost + Cm[i, perm[i]]
    return dict(perm=perm, owner=own, pf=pf, price=price, cost=cost, rounds=len(kinds), **extra)


def auction_rect_batch(po, goals, c, eps, max_rounds=0):
    """po [S,N,3], goals [S,M,3] -> the arrays Dmpc.assign_rect returns"""
    r = [auction_rect(p, g, c, eps, max_rounds) for p, g in zip(po, goals)]
    out = {k: np.stack([x[k] for x in r]) for k in ("perm", "owner", "pf", "price")}
    out.update(cost=np.array([x["cost"] for x in r]), rounds=np.array([x["rounds"] for x in r], dtype=np.int32))
    return out


def optimum_rect(po, goals, c):
    """the cost of scipy.optimize.linear_sum_assignment on the rectangular cost matrix, added in increasing agent index"""
    from scipy.optimize import linear_sum_assignment
    Cm = cost_matrix(po, goals, c)
    r, col = linear_sum_assignment(Cm)
    tot = np.float64(0.0)
    for i, j in zip(r, col):
        tot = tot + Cm[i, j]
    return tot


def certificate(po, goals, c, res):
    """(the largest per-person slack v_own - min_o v_o with v = c + price, the largest unowned price - the smallest owned price (-inf when every
    object is owned), cmax)"""
    Cm = cost_matrix(po, goals, c)
    N, M = Cm.shape
    Cpo, obj, own = (Cm, res["perm"], res["owner"]) if N <= M else (Cm.T, res["owner"], res["perm"])
    V = Cpo + np.asarray(res["price"])[None, :]
    sl = (V[np.arange(len(obj)), obj] - V.min(axis=1)).max()
    free = res["price"][own < 0]
    over = free.max() - res["price"][own >= 0].min() if free.size else -np.inf
    return sl, over, Cm.max()


def consistent(po, res, N, M):
    """perm and owner are each other's inverse on exactly min(N, M) pairs, and an agent without a goal stays at its start"""
    perm, owner = np.asarray(res["perm"]), np.asarray(res["owner"])
    if perm.shape != (N,) or owner.shape != (M,):
        return False
    a = np.flatnonzero(perm >= 0)
    g = np.flatnonzero(owner >= 0)
    return (a.size == g.size == min(N, M) and np.array_equal(owner[perm[a]], a) and np.array_equal(perm[owner[g]], g)
            and np.asarray(res["pf"])[perm < 0].tobytes() == np.asarray(po, dtype=np.float64)[perm < 0].tobytes())


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice(N, M, seed):
    rng = np.random.default_rng(7100 + 31 * seed + 1009 * N + M)
    side = max(4, int(np.ceil((4.0 * max(N, M)) ** (1.0 / 3.0))) + 1)      # at least four times as many lattice points as max(N, M)

    def pts(k):
        idx = rng.choice(side ** 3, size=k, replace=False)
        return np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1).astype(np.float64) * 0.25
    return pts(N), pts(M)


def lattice(N, M, seed=0):
    """(po [N,3], goals [M,3]): two sets of distinct points each on a 0.25 m lattice (shared by the tests: copies)"""
    po, g = _lattice(N, M, seed)
    return po.copy(), g.copy()


def lattice_eps(N, M):
    return 1.0 / (128.0 * max(N, M))


def lattice_batch(N, M, seeds):
    sc = [lattice(N, M, s) for s in seeds]
    return np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc])


@functools.lru_cache(maxsize=None)
def lattice_result(N, M, seed=0):
    """auction_rect() on lattice(N, M, seed) at lattice_eps(N, M), computed once per session (shared by the tests: do not modify)"""
    po, g = lattice(N, M, seed)
    return auction_rect(po, g, C_LATTICE, lattice_eps(N, M))


def uniform(N, M, seed=0):
    rng = np.random.default_rng(9100 + 17 * seed + 1009 * N + M)
    return rng.uniform(-2.5, 2.5, (N, 3)), rng.uniform(-2.5, 2.5, (M, 3))


def tie_scene(name):
    """scenes full of ties, (po, goals); a trailing T is the transpose (agents and goals exchanged)"""
    if name.endswith("T"):
        po, g = tie_scene(name[:-1])
        return g, po
    if name == "equal":        # every point the same: every cost 0
        return np.tile([0.25, 0.5, 1.0], (64, 1)), np.tile([0.25, 0.5, 1.0], (200, 1))
    if name == "zero":         # the same on a size that keeps a device run short
        return np.tile([0.25, 0.5, 1.0], (5, 1)), np.tile([0.25, 0.5, 1.0], (12, 1))
    if name == "duplicates":   # every goal twice
        po, g = lattice(10, 8, 3)
        return po, np.concatenate([g, g])
    if name == "subset":       # the agents stand on some of the goals
        _, g = lattice(1, 24, 4)
        return g[::3].copy(), g
    if name == "grid":         # a 6 x 6 grid of goals, 20 agents shifted half a cell: four nearest goals each
        ax = np.arange(6) * 0.5
        g = np.stack([np.repeat(ax, 6), np.tile(ax, 6), np.ones(36)], axis=1)
        return g[:20] + np.array([0.25, 0.25, 0.0]), g
    raise KeyError(name)


def same(out, ref, s=None):
    """the device's dict (scene s of it) equals the restatement's bit for bit; returns the name of the first array that differs, or None"""
    for k in KEYS:
        a = np.asarray(out[k] if s is None else out[k][s])
        b = np.asarray(ref[k])
        if a.shape != b.shape or a.tobytes() != b.astype(a.dtype).tobytes():
            return k
    return None


# ---- raw call of the entry ------------------------------------------------------------------------------------------------------------
def raw_assign_rect(d, S, N, M, po, goals, eps, max_rounds=0):
    """dmpc_assign_rect with the arguments as given (po / goals: arrays or None for a NULL pointer).  Returns (rc, message, outputs)."""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (po, goals)]
    ptr = [a.ctypes.data_as(dp) if a is not None else dp() for a in keep]
    s, n, m = max(S, 1), max(N, 1), max(M, 1)
    perm, owner, pf, price = np.zeros((s, n), dtype=np.int32), np.zeros((s, m), dtype=np.int32), np.zeros((s, n, 3)), np.zeros((s, max(n, m)))
    cost, rounds = np.zeros(s), np.zeros(s, dtype=np.int32)
    rc = d._L.dmpc_assign_rect(d._ctx, int(S), int(N), int(M), ptr[0], ptr[1], C.c_double(eps), int(max_rounds), perm.ctypes.data_as(ip),
                               owner.ctypes.data_as(ip), pf.ctypes.data_as(dp), price.ctypes.data_as(dp), cost.ctypes.data_as(dp),
                               rounds.ctypes.data_as(ip))
    return rc, d._L.dmpc_last_error(d._ctx).decode(), dict(perm=perm, owner=owner, pf=pf, price=price, cost=cost, rounds=rounds)
