"""GPU: one MPC step off the reference's constants -- every variant on the 16 parameter sets of tests/offconst.py (h from 0.05 to 0.3, Q1 and
S1 over four decades, alim, term, rmin / c, the weights of the collision-free cost cases), and four of the sets again with box and points
moved to (40, -25, 12).  The facts the cells rest on are those of the oracle alone, pinned in tests/test_offconst_cpu.py.

A cell is (variant, set, offset): 32 agents, five closed-loop steps whose teacher is the oracle; every agent-step of Dmpc.step_batch is
checked on the oracle's inputs.
  (a) records: status word, viol_k, row count, cost case and retry-ladder level equal the oracle's (helpers.compare_to_oracle), outputs of
      unsolved agents are zero.  No agent is skipped.
  (b) accuracy against x*, the extended-precision minimiser of tests/exactqp.py seeded with the GPU's answer (as test_gpu_exact.vouch):
      |a_gpu - x*| <= bar for every agent solved on both sides, bar = 4 x e_orc, e_orc the ORACLE's worst |a - x*| of the same cell in the
      same run (the factor 4 is the margin of test_gpu_exact.BARS: a binade for launch order, one for the choice of scenes); never below the
      entry of test_gpu_exact.BARS for the agent's decade of lam_max; for the reduced-solver variants never above DESIGN.md section 2's
      5e-8 on the first ladder level and 5e-7 above.  A fixed bar between two active-set codes would say nothing: the oracle itself lies
      up to 5e-8 (cpp1) from x* on these cells.  GPU worst, oracle worst and lam_max are printed per cell.
  (c) agents unresolved from the GPU's answer: at most 2 per cell, as on the CPU; they are held to the KKT certificate (NNLS).
  (d) every infeasible verdict of the GPU is confirmed by the phase-1 LP.
  (e) bound, bound2, cpp, cpp2 run on the reduced solver (last_solve_kernel asserted) and again with reduced_solver = 0: both against x*.
  (f) filter paths (test_filter_paths_...): bound and hard, 96 agents, cull_min = grid_min = 64 -- the boxes, the cell grid and the close
      pairs, whose cell size and reach follow rmin and c -- one step, every output word equal to the whole-table walk (no_cull = 1).
  (g) translation: (a) - (f) at the offset for offconst.MOVED_SETS.  Translation leaves x* unchanged in exact arithmetic: same bars.

MEASURED holds the cells whose bar is a measurement (4 x the GPU's worst of that cell on an MI355X, after the attribution of test_gpu_exact
-- general solver next to reduced, lam_max -- showed conditioning, not error); each is also a row of DESIGN.md section 2's table.  Every other
cell of the 260 meets the bar of (b) as it stands there.
"""
import functools

import numpy as np
import pytest

import multiagent_planning_amd as mp
from oracle import oracle as orc
from helpers import ALL_VARIANTS, compare_to_oracle
from test_certificates_cpu import check_batch
import offconst as oc
import test_gpu_exact as tge

pytestmark = pytest.mark.gpu

KEYS = ("status", "info", "p", "v", "a")
CELLS = [(v, s, oc.ORIGIN) for v in ALL_VARIANTS for s in oc.SETS] + [(v, s, oc.MOVED) for v in ALL_VARIANTS for s in oc.MOVED_SETS]
FILTER_CELLS = [(v, s, off) for v in ("bound", "hard") for s, off in [(s, oc.ORIGIN) for s in oc.SETS] + [(s, oc.MOVED) for s in oc.MOVED_SETS]]

# (variant, set, origin / moved, solver) -> (the GPU's measured worst |a - x*| of the cell on one MI355X, what drives it).  The cell's bar is
# 4 x the measurement.  Three causes, each decided by the attribution the test prints (both solvers next to the oracle, lam_max, rows; two
# runs on different machines gave the same figures):
#  Q1: the REDUCED solver at Q1 = 1e5.  About half of the agents of the cell, all on the first ladder level with lam_max 5e4, sit at
#      0.6 - 5e-11 from x*, where the general solver is within 7.3e-13 on the same agents and the oracle within 2.1e-12.  The linear term
#      is 100 x that of Q1 = 1e3 and cancels to accelerations of order 1; cond(H1) is 2.5e5 (2.5e3 at Q1 = 1e3), eps x cond = 3e-11: the
#      rounding of a small system that is formed explicitly and solved without refinement, three decades inside
#      its stated 5e-8.
#  LAM: one agent on ladder level 2 at term = -1e7 with lam_max 2.5e8: reduced solver 4.81e-10, general solver 2.16e-11, oracle 1.0e-11
#      (the error follows the multipliers; the decade's entry of test_gpu_exact.BARS was measured at term = -5e4).
#  MOVED: at the offset (40, -25, 12) the data carry ulp(40) = 7e-15.  Agents WITHOUT any row (lam_max 0) are the worst, by the same
#      figure on both solvers and in every variant: the linear term 2 Q1 l_K (A0 x0 - pf) is formed from positions near 40.  On the CPU
#      the exact minimisers of the scene at the origin and of the moved scene differ THEMSELVES by 6.2e-12 (h=0.3, agent 16 of step 2,
#      the agent that is worst on the GPU at 6.15e-12) and by 1.3e-12 (hard, S1=1): x* of the moved cell is known no better than that,
#      and the oracle is closer to it only because x* is computed from the oracle's own rounding of the data.
MEASURED = {
    ("bound", "Q1=1e5", "origin", "reduced"): (4.83e-11, "Q1"),
    ("bound2", "Q1=1e5", "origin", "reduced"): (1.48e-11, "Q1"),
    ("cpp", "Q1=1e5", "origin", "reduced"): (4.37e-11, "Q1"),
    ("cpp2", "Q1=1e5", "origin", "reduced"): (1.59e-11, "Q1"),
    ("cpp", "term=-1e7", "origin", "reduced"): (4.81e-10, "LAM"),
    ("bound", "h=0.3", "moved", "reduced"): (6.15e-12, "MOVED"),
    ("bound", "h=0.3", "moved", "general"): (6.15e-12, "MOVED"),
    ("bound2", "h=0.3", "moved", "reduced"): (7.71e-12, "MOVED"),
    ("bound2", "h=0.3", "moved", "general"): (7.71e-12, "MOVED"),
    ("cpp", "h=0.3", "moved", "reduced"): (6.15e-12, "MOVED"),
    ("cpp", "h=0.3", "moved", "general"): (6.15e-12, "MOVED"),
    ("cpp2", "h=0.3", "moved", "reduced"): (7.71e-12, "MOVED"),
    ("cpp2", "h=0.3", "moved", "general"): (7.71e-12, "MOVED"),
    ("ondemand", "h=0.3", "moved", "general"): (6.15e-12, "MOVED"),
    ("ellip", "h=0.3", "moved", "general"): (6.15e-12, "MOVED"),
    ("softall_c", "h=0.3", "moved", "general"): (6.15e-12, "MOVED"),
    ("hard", "S1=1", "moved", "general"): (1.48e-12, "MOVED"),
}


def _id(cell):
    v, s, off = cell
    return f"{v}-{s}-{'moved' if off == oc.MOVED else 'origin'}"


@functools.lru_cache(maxsize=None)
def _scene(name, offset, n=oc.N, box=oc.BOX):
    kw, po, pf = oc.scene(name, n=n, offset=offset, box=box)
    po.setflags(write=False); pf.setflags(write=False)
    return kw, po, pf


def floor_bar(lam_max):
    """the entry of test_gpu_exact.BARS for the decade of lam_max (above the last measured decade: the last one's)"""
    keys = sorted(tge.BARS)
    return np.array([tge.BARS[int(d)] for d in np.clip(tge.decade(lam_max), keys[0], keys[-1])])


def _measure(what, loop, outs):
    """(a), (c), (d) of one solver on a cell, asserted; returns compare_cell's arrays of the resolved agent-steps and prints the cell's line"""
    # (a) records
    for k, ((prm, sc, ref), o) in enumerate(zip(loop, outs)):
        compare_to_oracle(o, ref, tol=np.inf, what=f"{what} step {k + 2}")
    # (d) infeasible verdicts
    n_inf = 0
    for k, ((prm, sc, ref), o) in enumerate(zip(loop, outs)):
        agents = np.nonzero(o["status"] & mp.ST_INFEAS)[0]
        ns, ni, _ = check_batch(prm, *sc, o["a"], o["status"], o["info"][:, 2], f"{what} step {k + 2}", agents=agents)
        assert ns == 0 and ni == len(agents)
        n_inf += ni
    # (c) against x*: the unresolved fall back to the KKT certificate and count against the cap
    A = oc.compare_cell(loop, outs)
    assert len(A["agent"]) == sum(int((o["status"] & 1).sum()) for o in outs) > 0
    res = A["resolved"].astype(bool)
    for k in np.unique(A["step"][~res]):
        prm, sc, ref = loop[int(k)]
        o = outs[int(k)]
        check_batch(prm, *sc, o["a"], o["status"], o["info"][:, 2], f"{what} step {k + 2} (unresolved: KKT certificate)", agents=[int(n) for n in A["agent"][~res & (A["step"] == k)]])
    assert int((~res).sum()) <= oc.CAP_UNRESOLVED, f"{what}: {int((~res).sum())} agent-steps unresolved from the GPU's answer"
    assert res.any()
    worst = int(np.argmax(np.where(res, A["e"], -1.0)))
    print(f"[{what}] {len(res)} agent-steps solved, {int((~res).sum())} unresolved, {n_inf} infeasible (LP confirmed), ladder level up to "
          f"{int(A['level'].max())}; worst |a - x*|: GPU {A['e'][worst]:.2e} (level {int(A['level'][worst])}, lam_max {A['lam_max'][worst]:.2e}), "
          f"oracle {A['e_orc'][res].max():.2e}; lam_max up to {A['lam_max'][res].max():.2e}")
    return A


def _bars(cell, solver, A):
    """(b): the bar of every agent-step of the cell (nan where unresolved)"""
    variant, name, offset = cell
    key = (variant, name, "moved" if offset == oc.MOVED else "origin", solver)
    if key in MEASURED:
        return np.full(len(A["e"]), 4.0 * MEASURED[key][0])
    res = A["resolved"].astype(bool)
    bar = np.maximum(4.0 * A["e_orc"][res].max(), floor_bar(np.where(res, A["lam_max"], 0.0)))
    if variant in oc.REDUCED:
        bar = np.minimum(bar, np.where(A["level"] <= 1, tge.FIRST, tge.LADDER))
    return np.where(res, bar, np.nan)


@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_step_off_the_constants_against_the_oracle_and_the_exact_minimiser(cell):
    variant, name, offset = cell
    kw, po, pf = _scene(name, offset)
    loop = oc.closed_loop(variant, kw, po, pf)
    runs = {}
    if variant in oc.REDUCED:      # (e) the reduced solver, and the same cell on the general solver
        d = mp.Dmpc(variant, **kw)
        outs = [d.step_batch(*sc) for _, sc, _ in loop]
        assert d.last_solve_kernel == "dmpc_rsolve_persist_kernel"
        runs["reduced"] = _measure(f"{_id(cell)} reduced solver", loop, outs)
    g = mp.Dmpc(variant, **kw)
    if variant in oc.REDUCED:
        g.debug_option("reduced_solver", 0)
    outs = [g.step_batch(*sc) for _, sc, _ in loop]
    assert g.last_solve_kernel != "dmpc_rsolve_persist_kernel"
    runs["general"] = _measure(f"{_id(cell)} general solver", loop, outs)
    # (b), after both solvers have been measured: an agent-step above its bar is printed with every solver's figure next to the oracle's
    # (the attribution of test_gpu_exact), then asserted
    over = {s: np.nan_to_num(A["e"], nan=0.0) > np.nan_to_num(_bars(cell, s, A), nan=np.inf) for s, A in runs.items()}
    for s, A in runs.items():
        bar = _bars(cell, s, A)
        for i in np.nonzero(over[s])[0][:8]:
            print(f"  above its bar ({s} solver): step {int(A['step'][i]) + 2} agent {int(A['agent'][i])} level {int(A['level'][i])} rows {int(A['rows'][i])} "
                  f"lam_max {A['lam_max'][i]:.3e}: " + ", ".join(f"{t} {B['e'][i]:.2e}" for t, B in runs.items()) + f", oracle {A['e_orc'][i]:.2e}, bar {bar[i]:.1e}")
    for s, A in runs.items():
        assert not over[s].any(), (f"{_id(cell)} {s} solver: {int(over[s].sum())} agent-steps above their bar, worst {A['e'][over[s]].max():.2e} "
                                   f"(lam_max {A['lam_max'][over[s]][np.argmax(A['e'][over[s]])]:.2e}); the oracle's worst of the cell {np.nanmax(A['e_orc']):.2e}")


@pytest.mark.parametrize("cell", FILTER_CELLS, ids=_id)
def test_filter_paths_select_what_the_walk_selects_off_the_constants(cell):
    """(f): one step of 96 agents from initDMPC's table, on the boxes, on the grid with close pairs, and on the whole-table walk"""
    variant, name, offset = cell
    kw, po, pf = _scene(name, offset, oc.N_FILTER, oc.BOX_FILTER)
    sc = oc.init(np.array(po), np.array(pf), kw["h"])

    def step(**opts):
        d = mp.Dmpc(variant, **kw)
        for k, v in opts.items():
            d.debug_option(k, v)
        return d.step_batch(*sc), d

    walk, _ = step(no_cull=1)
    boxes, _ = step(cull_min=64, nbr_grid=0)
    grid, dg = step(cull_min=64, grid_min=64)
    assert dg.debug_read_grid()["build"] in (1, 2), "the cell grid must have been built"
    for leg, got in (("boxes", boxes), ("grid", grid)):
        for k in KEYS:
            assert np.array_equal(got[k], walk[k]), f"{_id(cell)} leg '{leg}': {k} differs from the walk at agents {np.nonzero((got[k] != walk[k]).reshape(oc.N_FILTER, -1).any(-1))[0][:10]}"
    assert (walk["info"][:, 1] > 0).any(), "rows were built"
    # equality with the walk cannot see a mistake the walk shares: its records (rows selected, cost case, level) are the oracle's
    compare_to_oracle(walk, orc.step(orc.make_params(variant, **kw), *sc, nthreads=8), tol=np.inf, what=f"{_id(cell)} (walk against the oracle)")


def test_transition_at_a_second_h_matches_the_host_loop_and_reaches_its_goals():
    """the plain transition off the constants: one 8-agent scene at h = 0.25, Q1 = 10; the device loop equals the host loop over step_batch
    bit for bit (the pattern of test_gpu_api.test_transition_c1_reaches_goal_and_matches_python_loop) and reaches its goals"""
    n, KT, tol = 8, 100, 0.01
    kw, po, pf = oc.scene("base", n=n, seed=oc.SEED + 3)
    kw.update(h=0.25, Q1=10.0)
    d = mp.Dmpc("bound", **kw)
    res = d.transition(po[None], pf[None], KT, tol)
    used = int(res["K_T_used"][0])
    assert res["scene_status"][0] == (mp.ST_SOLVED | mp.ST_REACHED) and 20 < used < KT
    pk, vk, ak = res["pk"][0], res["vk"][0], res["ak"][0]
    assert np.linalg.norm(pk[:, used - 1] - pf, axis=1).max() < tol
    l = d.init_batch(po, pf)[0]
    xp, xv, xa = po.copy(), np.zeros((n, 3)), np.zeros((n, 3))
    rows = 0
    for k in range(1, used):
        out = d.step_batch(l, xp, xv, xa, pf)
        assert np.all(out["status"] == 1)
        rows += int((out["info"][:, 1] > 0).sum())
        l, xp, xv, xa = out["p"], out["p"][:, :3], out["v"][:, :3], out["a"][:, :3]
        assert np.array_equal(xp, pk[:, k]) and np.array_equal(xv, vk[:, k]) and np.array_equal(xa, ak[:, k]), f"column {k}"
    assert rows > 0, "the agents met on the way"
