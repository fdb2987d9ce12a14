"""Test helper: scenes and the numpy reference of the clearance report (dmpc_postcheck_clearance): per commanded agent the nearest commanded
partner (slot 0) and the nearest uncommanded vehicle (slot 1) over the 100 Hz samples, and when.

The reference is a numpy all-pairs search over interpolated positions p [N_cmd,ns,3] / q [M,ns,3]: on the GPU the library's own `p` /
`p_scripted` from postcheck(interp=True), which the existing tests hold to the oracle; on the CPU the oracle's (oracle/postcheck.py).
The device forms d2 with two FMAs, numpy with three roundings: distances agree to ULPS = 8 ulp of the CPU value (np.spacing).  The identity
of (partner, sample) is NOT compared with numpy's argmin (ties, and near-ties inside those ulps, may legitimately differ): the distance
recomputed at the reported (i, partner, sample) must equal the reported one, and no other candidate of that kind may be smaller.
"""
import numpy as np

KW = dict(h=0.2, rmin=0.35, c=2.0, alim=1.0, Q1=1000.0, S1=100.0, term=-5e4, pmin=(-2.5, -2.5, 0.2), pmax=(2.5, 2.5, 2.2))
ULPS = 8
REACH3 = 3 * KW["rmin"]


def integrate(p0, v0, a, h=0.2):
    """histories pk, vk, ak [N,KT,3] of the recurrence the post-check's rescale re-integrates, from p0, v0 [N,3] and a [N,KT,3]"""
    p, v = np.zeros_like(a), np.zeros_like(a)
    p[:, 0], v[:, 0] = p0, v0
    for k in range(1, a.shape[1]):
        v[:, k] = v[:, k - 1] + h * a[:, k - 1]
        p[:, k] = p[:, k - 1] + h * v[:, k - 1] + h * h / 2 * a[:, k - 1]
    return p, v, a


# ---- case 3: a dense box at the boundary between the searches ------------------------------------------------------------------------------
BOX_KT, BOX_M, BOX_STEP = 8, 3, 1.6


def box_kw():
    """7 x 7 x 7 places BOX_STEP apart: in the metric of the check (z / c) the neighbour above is 0.8 m away, the one beside 1.6 m"""
    s = 7 * BOX_STEP
    return dict(KW, pmin=(-s / 2, -s / 2, 0.2), pmax=(s / 2, s / 2, s + 0.2))


def box_scene(n_cmd):
    """(pk, vk, ak [n_cmd,BOX_KT,3], po_static [BOX_M,3]): n_cmd of the 343 places taken, jittered, smooth random motion; the static
    vehicles stand half a metre beside the starts of agents 0, 100 and 200.  tests/test_clearance_cpu.py holds, with the oracle's
    post-check, that at n_cmd = 256, 257 and 300 some slots of either kind lie inside 3 rmin and some do not."""
    rng = np.random.default_rng(4000 + n_cmd)
    g = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(343)[:n_cmd]]
    p0 = (g + 0.5 + rng.uniform(-0.2, 0.2, (n_cmd, 3))) * BOX_STEP + (-3.5 * BOX_STEP, -3.5 * BOX_STEP, 0.2)
    a = rng.uniform(-1, 1, (n_cmd, BOX_KT, 3))
    pk, vk, ak = integrate(p0, np.zeros((n_cmd, 3)), a)
    return pk, vk, ak, p0[[0, 100, 200]] + (0.5, 0.0, 0.0)


# ---- case 4: exact ties ----------------------------------------------------------------------------------------------------------------------
def line_kw(n):
    return dict(KW, pmin=(-1.0, -2.5, -1.0), pmax=(n + 1.0, 2.5, 1.0))


def line_scene(n, KT=6):
    """agents at x = 0, 1, .., n-1 (exact in fp64), z = 0, ONE y-history with a non-zero velocity for all: x has neither velocity nor
    acceleration, so rescale and spline leave it alone and d2 between neighbours is exactly 1 at every sample"""
    a = np.zeros((n, KT, 3)); a[:, :, 1] = np.array([0.3, -0.2, 0.25, 0.1, -0.3, 0.2])[:KT]
    p0 = np.zeros((n, 3)); p0[:, 0] = np.arange(n)
    v0 = np.zeros((n, 3)); v0[:, 1] = 0.5
    return integrate(p0, v0, a)


def line_partner(n):
    """ties go to the smallest partner: the lower neighbour, and the only one for agent 0"""
    return np.array([1] + list(range(n - 1)), dtype=np.int32)


# ---- the numpy reference ----------------------------------------------------------------------------------------------------------------------
def distances(pi, others, c):
    """|E1 (p_i(t) - o_j(t))| of one agent pi [ns,3] against others [n,ns,3] -> [n,ns]"""
    e1 = np.array([1.0, 1.0, 1.0 / c])
    return np.sqrt((((pi[None] - others) * e1) ** 2).sum(-1))


def nearest(p, q, c):
    """(d0 [N_cmd], d1 [N_cmd]): every agent's smallest distance to another commanded agent / to an uncommanded vehicle (inf: none)"""
    n = p.shape[0]
    d0, d1 = np.full(n, np.inf), np.full(n, np.inf)
    for i in range(n):
        if n > 1:
            d = distances(p[i], p, c); d[i] = np.inf
            d0[i] = d.min()
        if q is not None and len(q):
            d1[i] = distances(p[i], q, c).min()
    return d0, d1


def check_scene(dist, partner, sample, p, q, c, reach=np.inf):
    """one scene of a report (dist, partner, sample [N_cmd,2]) against p [N_cmd,ns,3] and q [M,ns,3] (or None); no agent is exempted.
    Slots whose numpy distance is not < reach must be empty.  Returns the number of (filled, empty) slots."""
    n, ns = p.shape[0], p.shape[1]
    filled = empty = 0
    for i in range(n):
        for slot, others in ((0, p), (1, q)):
            got = (dist[i, slot], partner[i, slot], sample[i, slot])
            d = None
            if others is not None and len(others) > (1 if slot == 0 else 0):
                d = distances(p[i], others, c)
                if slot == 0:
                    d[i] = np.inf
            if d is None or not d.min() < reach:
                assert np.isposinf(got[0]) and got[1] == -1 and got[2] == -1, (i, slot, got)
                empty += 1
                continue
            filled += 1
            m = d.min()
            assert abs(got[0] - m) <= ULPS * np.spacing(m), (i, slot, got, m)
            j = got[1] - (n if slot else 0)
            assert 0 <= j < len(others) and 0 <= got[2] < ns and (slot == 1 or j != i), (i, slot, got)
            here = d[j, got[2]]
            assert abs(here - got[0]) <= ULPS * np.spacing(here), (i, slot, got, here)       # the report names a pair that IS that close ...
            assert m >= got[0] - ULPS * np.spacing(m), (i, slot, got, m)                      # ... and no other candidate of the kind is closer
    return filled, empty
