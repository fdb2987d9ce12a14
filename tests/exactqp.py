"""An extended-precision minimiser of a per-agent QP that involves NO active-set code: the reference the accuracy of the reduced solver
(csrc/dmpc_rsolve.hip) is measured against (tests/test_exactqp_cpu.py, tests/test_gpu_exact.py).

The QP  min 1/2 x'Hx + f'x  s.t.  Cx <= d,  x = [a; eps]  (oracle.assemble_one: the dense assembly of the .m files) is strictly convex, so
its minimiser is determined by its active set.  Given a candidate answer `a` (the GPU's, the oracle's):

  1. the slack is completed in closed form (certificates.complete_slack);
  2. the rows with residual >= -1e-7 x scale are the candidates, the support of their Lawson-Hanson NNLS multipliers is the working
     set W (as certificates.kkt_certificate recovers its multipliers);
  3. [H C_W'; C_W 0] [x; lam] = [-f; d_W] is solved in double (LU) and refined four times with residuals in np.longdouble; a system
     whose pivots look dependent only because its variables differ in scale by many decades (softall_c's slack weights) is solved
     again with the variables scaled to a unit diagonal of H.

If every refined multiplier is >= 0 and C x* - d <= 1e-11 on every row, x* satisfies the KKT conditions and is THE minimiser, to about
1e-15: the candidate only had to be near enough to name the right working set.  Anything else is `unresolved` -- counted by the
callers, never passed silently.  Plain numpy / scipy, like certificates.py.
"""
import numpy as np
from scipy.linalg import lu_factor, lu_solve
from scipy.optimize import nnls

from certificates import N3, complete_slack

LAM_FLOOR = 1e-9      # a refined multiplier below -LAM_FLOOR x max(1, |lam|max): wrong working set
ROW_TOL = 1e-11       # a row of C x* - d above it: wrong working set
REFINE = 4


def working_set(qp, a, tol_act=1e-7):
    """the rows in the support of the NNLS multipliers of the candidate answer `a` (steps 1-2)"""
    H, f, C, d = qp["H"], qp["f"], qp["C"], qp["d"]
    x = complete_slack(qp, np.asarray(a, float))
    r = C @ x - d
    act = np.where(r >= -tol_act * np.maximum(1.0, np.abs(C).max(axis=1)))[0]
    if not len(act):
        return act
    cn = np.linalg.norm(C[act], axis=1)
    lam_s, _ = nnls((C[act] / cn[:, None]).T, -(H @ x + f), maxiter=20 * max(len(act), C.shape[1]))
    return act[lam_s > 0.0]


def kkt_point(qp, W, equilibrate=False):
    """the stationary point of the QP with the rows W as equalities, refined in extended precision: (x, lam, singular).
    equilibrate: the variables are scaled to a unit diagonal of H first (see exact_minimiser)"""
    H, f, C, d = qp["H"], qp["f"], qp["C"], qp["d"]
    n, m = H.shape[0], len(W)
    Kd = np.zeros((n + m, n + m))
    Kd[:n, :n] = H
    Kd[:n, n:] = C[W].T
    Kd[n:, :n] = C[W]
    rhs = np.concatenate([-f, d[W]])
    # rows and columns of the constraints scaled to unit norm: the pivots of the LU then tell dependence from mere scale
    s = np.ones(n + m)
    if equilibrate:
        s[:n] = 1.0 / np.sqrt(np.diag(H))
    s[n:] = 1.0 / np.maximum(1e-300, np.linalg.norm(C[W] * s[None, :n], axis=1))
    Ks = Kd * s[:, None] * s[None, :]
    if not np.isfinite(Ks).all():
        return None, None, True
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lu, piv = lu_factor(Ks, check_finite=False)
    dg = np.abs(np.diag(lu))
    if dg.min() <= 1e-13 * dg.max():
        return None, None, True
    Kl, rl = Ks.astype(np.longdouble), (rhs * s).astype(np.longdouble)
    y = lu_solve((lu, piv), rhs * s, check_finite=False).astype(np.longdouble)
    for _ in range(REFINE):
        res = rl - Kl @ y
        y = y + lu_solve((lu, piv), res.astype(np.float64), check_finite=False)
    res = rl - Kl @ y
    if not np.isfinite(np.asarray(y, np.float64)).all() or float(np.abs(res).max()) > 1e-12 * max(1.0, float(np.abs(rl).max())):
        return None, None, True      # the refinement did not converge: numerically singular
    y = np.asarray(y, np.float64) * s
    return y[:n], y[n:], False


def exact_minimiser(qp, a):
    """dict(x = x*[:45], lam_max, resolved, why, n_active) for the candidate answer `a` of the dense QP `qp`.  Unresolved (x, lam_max
    are then None / nan): a singular KKT matrix, a refined multiplier below -1e-9 max(1, |lam|max), a row of C x* - d above 1e-11."""
    W = working_set(qp, a)
    x, lam, singular = kkt_point(qp, W)
    if singular:
        # The pivot test of kkt_point compares pivots of the KKT matrix with only its constraint rows scaled.  A QP whose variables differ
        # in scale by many decades fails it without being dependent: softall_c weighs a slack with 1e6 (K/k)^2 against about 1e3 on an
        # acceleration, the pivot of a slack's bound row is 1 / H_ii of that slack, and 1 / H_ii^2 lies below the test's 1e-13.  Such a
        # system is solved again with the variables scaled to a unit diagonal of H, where a small pivot again means dependence.  The
        # unscaled attempt stays first: every x* it resolves (all figures of DESIGN.md section 2) is unchanged to the bit.
        x, lam, singular = kkt_point(qp, W, equilibrate=True)
    bad = dict(x=None, lam_max=float("nan"), resolved=False, n_active=int(len(W)))
    if singular:
        return dict(bad, why="singular")
    lmax = float(np.abs(lam).max()) if len(lam) else 0.0
    if len(lam) and lam.min() < -LAM_FLOOR * max(1.0, lmax):
        return dict(bad, why=f"multiplier {lam.min():.2e}")
    viol = float((qp["C"] @ x - qp["d"]).max())
    if viol > ROW_TOL:
        return dict(bad, why=f"row violated by {viol:.2e}")
    return dict(x=x[:N3].copy(), lam_max=float(lam.max()) if len(lam) else 0.0, resolved=True, why="", n_active=int(len(W)))


_JOBS = None      # (orc, problems) of the running exact_many: the forked workers inherit it, only agent indices travel


def _run(task):
    j, agents = task
    orc, problems = _JOBS
    prm, l, xp, xv, xa, pf, a, status, tries = problems[j]
    out = []
    for n in agents:
        qp = orc.assemble_one(prm, l, n, xp[n], xv[n], xa[n], pf[n], level=max(int(tries[n]) - 1, 0))
        out.append(exact_minimiser(qp, a[n]))
    return out


def exact_many(orc, problems, nproc=8, chunk=48):
    """exact_minimiser of every solved agent (status & 1) of every problem (prm, l, xp, xv, xa, pf, a [N,45], status, tries), the
    candidate answers being a.  The work (about 2 ms per agent, mostly NNLS and the dense assembly, which do not overlap in threads) is
    spread over a pool of forked workers that touch nothing but the host; without fork it runs in this process.  Returns one
    (x [N,45], lam_max [N], resolved [N] bool, compared [N] bool) per problem: rows of agents not compared are nan / False."""
    global _JOBS
    import multiprocessing as mpx
    tasks = []
    for j, pb in enumerate(problems):
        todo = [int(n) for n in np.nonzero(np.asarray(pb[7]) & 1)[0]]
        tasks += [(j, todo[i:i + chunk]) for i in range(0, len(todo), chunk)]
    _JOBS = (orc, problems)
    try:
        if nproc > 1 and len(tasks) > 1:
            try:
                with mpx.get_context("fork").Pool(min(nproc, len(tasks))) as pool:
                    res = pool.map(_run, tasks)
            except (OSError, ValueError):      # no fork / no pool on this host
                res = [_run(t) for t in tasks]
        else:
            res = [_run(t) for t in tasks]
    finally:
        _JOBS = None
    outs = []
    for pb in problems:
        N = pb[1].shape[0]
        outs.append((np.full((N, N3), np.nan), np.full(N, np.nan), np.zeros(N, bool), np.zeros(N, bool)))
    for (j, agents), rs in zip(tasks, res):
        X, lam, ok, cmp_ = outs[j]
        for n, r in zip(agents, rs):
            cmp_[n] = True
            if r["resolved"]:
                X[n], lam[n], ok[n] = r["x"], r["lam_max"], True
    return outs


def exact_batch(orc, prm, l, xp, xv, xa, pf, a, status, tries, nproc=8):
    """exact_many of one MPC step"""
    return exact_many(orc, [(prm, l, xp, xv, xa, pf, a, status, tries)], nproc)[0]
