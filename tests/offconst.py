"""One MPC step away from the reference's constants (shared by tests/test_offconst_cpu.py and tests/test_gpu_offconst.py; no GPU here).

Every other context of the suite is built with h = 0.2, Q1 = 1000, S1 = 100, a handful of rmin / c / alim and a box at the origin, while the
ABI takes all of these as free parameters and the host tables, the reduced solver's per-axis solve, the selection radii, the grid cells
and the retry ladder depend on them.  Here: a table of parameter sets, a small dense scene per set, a teacher-forced closed loop whose
teacher is always the ORACLE (the next step's table and state come from the oracle's outputs), and the comparison of a cell -- one
(variant, set, offset) -- with the extended-precision minimiser x* of tests/exactqp.py.
"""
import numpy as np

from multiagent_planning_amd import workload as wl
from oracle import oracle as orc
import exactqp as ex

BASE = dict(h=0.2, rmin=0.35, c=2.0, alim=1.0, Q1=1000.0, S1=100.0, term=-5e4, Qfar=0.0, Qnear=0.0, Sfree=0.0)      # (0: the reference's own weights)
SETS = {
    "base": {},
    "h=0.1": dict(h=0.1), "h=0.05": dict(h=0.05), "h=0.25": dict(h=0.25), "h=0.3": dict(h=0.3),
    "Q1=1e5": dict(Q1=1e5), "Q1=10": dict(Q1=10.0), "S1=1": dict(S1=1.0), "S1=1e4": dict(S1=1e4),
    "alim=0.3": dict(alim=0.3), "alim=4": dict(alim=4.0),
    "term=-1e3": dict(term=-1e3), "term=-1e7": dict(term=-1e7),
    "rmin=0.2,c=1": dict(rmin=0.2, c=1.0), "rmin=0.6,c=3": dict(rmin=0.6, c=3.0),
    "Qfar=10,Qnear=1e5,Sfree=1": dict(Qfar=10.0, Qnear=1e5, Sfree=1.0),
}
ORIGIN, MOVED = (0.0, 0.0, 0.0), (40.0, -25.0, 12.0)
MOVED_SETS = ("base", "h=0.3", "S1=1", "rmin=0.6,c=3")       # the sets that also run at the offset MOVED
BOX = ((-1.6, -1.6, 0.2), (1.6, 1.6, 2.2))
N, STEPS = 32, 5
N_FILTER = 96           # the filter legs: enough agents for the box, grid and close-pair paths (cull_min = grid_min = 64), in a box of twice the
BOX_FILTER = ((-3.2, -3.2, 0.2), (3.2, 3.2, 4.2))      # side, which the separated draw of every set (rmin=0.6,c=3 too) still fills
SEED = 20261020
# Two sets draw a sparse scene at SEED: fewer than MIN_ROW_STEPS agent-steps with collision rows in some variant (rmin=0.2,c=1: 24 - 35, the
# small ellipsoid; h=0.05: 35 for scp, the 0.75 s horizon).  They take the first later seed at which all 13 variants reach it (56 and 55).
SEEDS = {"rmin=0.2,c=1": SEED + 2, "h=0.05": SEED + 41}
CAP_UNRESOLVED = 2      # agent-steps per cell (of N x STEPS = 160) exact_minimiser may leave unresolved
MIN_ROW_STEPS = 50      # agent-steps per cell that must carry collision rows
REDUCED = ("bound", "bound2", "cpp", "cpp2")


def solver_kw(name, offset=ORIGIN, box=BOX, **more):
    """the keyword block of a parameter set, its box moved by `offset`"""
    off = np.asarray(offset, float)
    kw = dict(BASE, **SETS[name])
    kw["pmin"], kw["pmax"] = tuple(np.asarray(box[0]) + off), tuple(np.asarray(box[1]) + off)
    kw.update(more)
    return kw


def scene(name, n=N, offset=ORIGIN, seed=None, box=BOX):
    """(kw, po, pf): starts and goals, each a separated draw in the metric diag(1, 1, 1/c) at 1.05 rmin inside the box; the draw depends on
    the set's rmin and c alone, and box and points are moved by `offset` afterwards (so the moved scene is the same scene)"""
    kw = solver_kw(name, offset, box)
    rng = np.random.default_rng(SEEDS.get(name, SEED) if seed is None else seed)
    po, pf = wl.random_test(n, box[0], box[1], 1.05 * kw["rmin"], kw["c"], rng)
    off = np.asarray(offset, float)
    return kw, po + off, pf + off


def init(po, pf, h):
    """initDMPC's table and the state at rest: (l, x_p, x_v, x_a, pf)"""
    l = np.stack([orc.init_one(po[n], pf[n], h, 15)[0] for n in range(len(po))])
    return (l, po.copy(), np.zeros_like(po), np.zeros_like(po), pf)


def teacher(sc, ref):
    """the next step's inputs from the oracle's outputs (an unsolved agent keeps its row and state)"""
    l, xp, xv, xa, pf = sc
    ok = ((ref["status"] & 1) == 1)[:, None]
    return (np.where(ok, ref["p"], l), np.where(ok, ref["p"][:, :3], xp), np.where(ok, ref["v"][:, :3], xv), np.where(ok, ref["a"][:, :3], xa), pf)


def closed_loop(variant, kw, po, pf, steps=STEPS, nthreads=8):
    """[(prm, inputs, oracle's result)] of `steps` teacher-forced closed-loop steps from init()"""
    prm = orc.make_params(variant, **kw)
    sc, out = init(po, pf, kw["h"]), []
    for _ in range(steps):
        ref = orc.step(prm, *sc, nthreads=nthreads)
        out.append((prm, sc, ref))
        sc = teacher(sc, ref)
    return out


def compare_cell(loop, answers=None, nproc=8):
    """The comparison of a cell with x*.  loop: closed_loop()'s list; answers: per step the dict (a, status, info) under test -- None: the
    oracle's own.  Every agent-step solved by the oracle AND by the answer is given to exact_minimiser, seeded with the answer under test.
    Returns arrays over those agent-steps: step, agent, level, rows, lam_max, resolved, e (the answer's |a - x*|_inf) and e_orc (the
    oracle's, against the same x*: the minimiser is unique, whoever named its working set); nan where unresolved."""
    if answers is None:
        answers = [ref for _, _, ref in loop]
    both = [((ref["status"] & 1) == 1) & ((np.asarray(o["status"]) & 1) == 1) for (_, _, ref), o in zip(loop, answers)]
    outs = ex.exact_many(orc, [(prm, *sc, np.asarray(o["a"]), np.where(b, 1, 0), ref["info"][:, orc.I_TRIES])
                               for (prm, sc, ref), o, b in zip(loop, answers, both)], nproc)
    cols = {k: [] for k in ("step", "agent", "level", "rows", "lam_max", "resolved", "e", "e_orc")}
    for k, ((prm, sc, ref), o, b, (X, lam, res, cmp_)) in enumerate(zip(loop, answers, both, outs)):
        idx = np.nonzero(b)[0]
        assert np.array_equal(cmp_, b)
        with np.errstate(invalid="ignore"):
            e = np.abs(np.asarray(o["a"])[idx] - X[idx]).max(axis=1) if len(idx) else np.zeros(0)
            e_orc = np.abs(ref["a"][idx] - X[idx]).max(axis=1) if len(idx) else np.zeros(0)
        for key, v in zip(cols, (np.full(len(idx), k), idx, ref["info"][idx, orc.I_TRIES], ref["info"][idx, orc.I_NROWS], lam[idx], res[idx], e, e_orc)):
            cols[key].append(np.asarray(v))
    return {k: np.concatenate(v) for k, v in cols.items()}


def cell_facts(loop):
    """what a cell's oracle run is: agent-steps with collision rows, the count of every status word, the highest ladder level"""
    st = np.concatenate([ref["status"] for _, _, ref in loop])
    rows = np.concatenate([ref["info"][:, orc.I_NROWS] for _, _, ref in loop])
    lev = np.concatenate([ref["info"][:, orc.I_TRIES] for _, _, ref in loop])
    return dict(row_steps=int((rows > 0).sum()), statuses={int(s): int((st == s).sum()) for s in np.unique(st)}, level=int(lev.max()))
