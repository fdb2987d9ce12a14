"""GPU: three kernels can finish an agent of an MPC step -- the scan's unconstrained exit, the reduced solver (csrc/dmpc_rsolve.hip) and the
general solver (csrc/dmpc_solve.hip) -- and all of them end in ONE output stage (agent_outputs / agent_record, csrc/dmpc_kernels.hip).  The
same agents, with the same inputs, finished by each kernel in turn:

  * scan exit against the solver behind it (development option no_fast_exit; with and without reduced_solver = 0): p, v, a, status and
    info[:4] identical bit for bit, as tests/test_gpu_paths.py holds them;
  * the solve kernel's fused post-step against post_step_kernel (no_fuse) on a two-step transition: identical histories and verdicts;
  * reduced against general solver (reduced_solver = 0): same status and info[:4], p, v, a within the bars the suite holds the reduced
    solver to against the exact minimiser (FIRST / LADDER of tests/test_gpu_exact.py, which tests/test_gpu_reduced.py draws on: 5e-8 on
    the first ladder level, 5e-7 above).

Inputs: the recorded scene comp_kctr_3_bound2 (100 agents, MPC step 14) and a random 64-agent scene of workload (three teacher-forced steps),
with bound and with cpp2, the reduced solver's variant without an in-bounds test.

The in-bounds test itself: two agents of the random scene start 40 mm inside the workspace's x walls and move outward, one slowly enough
that the horizon can keep it inside (it ends ON the wall: the in-bounds test of is_inbounds.m runs and passes), one too fast for that.  The
oracle (checked here, on the CPU) reports SOLVED for the first and INFEAS for the second and never ST_OUTBOUND: the walls are hard
constraints of the QP, so a solved agent's first position is at most a rounding error beyond pmax and is_inbounds.m's 50 mm margin cannot
be exceeded.  Every leg must report exactly the oracle's status for the two."""
import functools

import numpy as np
import pytest

import multiagent_planning_amd as mp
from multiagent_planning_amd import workload as wl
from oracle import oracle as orc
from helpers import init_table, load_golden, step14_inputs
from test_gpu_exact import FIRST, LADDER

pytestmark = pytest.mark.gpu

WALL_HI, WALL_LO = 0, 1   # (after the reordering below) the agents at the +x and the -x wall
LEGS = {"default": {}, "no_fast_exit": dict(no_fast_exit=1), "general": dict(reduced_solver=0), "general_no_fast_exit": dict(reduced_solver=0, no_fast_exit=1)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """kw, the first step's inputs (l, xp, xv, xa, pf), closed-loop steps, the transition's (po, pf)"""
    if name == "golden":
        g, kw = load_golden("comp_kctr_3_bound2")
        return kw, step14_inputs(g), 1, (g["po"], g["pf"])
    cfg = wl.CONFIGS["C4"]
    N = 64
    kw = wl.solver_kwargs(cfg, N)
    po, pf = wl.make_scenes(cfg, 1, N, wl.SEED0 + 701)
    po, pf = po[0], pf[0]
    # the agents nearest the two x walls go to the front and 40 mm inside their wall (moving an extreme agent outward along x only takes it
    # away from every other agent), with an outward velocity: 0.3 m/s can still be braked (0.04 = 0.2 * 0.3 - 0.2^2 / 2 * alim), 1 m/s cannot
    hi, lo = int(po[:, 0].argmax()), int(po[:, 0].argmin())
    order = [hi, lo] + [n for n in range(N) if n not in (hi, lo)]
    po, pf = po[order].copy(), pf[order].copy()
    po[WALL_HI, 0], po[WALL_LO, 0] = kw["pmax"][0] - 0.04, kw["pmin"][0] + 0.04
    xv = np.zeros_like(po)
    xv[WALL_HI, 0], xv[WALL_LO, 0] = 0.3, -1.0
    return kw, (init_table(po, pf), po.copy(), xv, np.zeros_like(po), pf), 3, (po, pf)


@functools.lru_cache(maxsize=None)
def _oracle_first_step(variant):
    kw, inputs, _, _ = _scene("random")
    return orc.step(orc.make_params(variant, **kw), *inputs)


def _advance(inputs, o):
    l, xp, xv, xa, pf = inputs
    ok = (o["status"] == 1)[:, None]
    return (np.where(ok, o["p"], l), np.where(ok, o["p"][:, :3], xp), np.where(ok, o["v"][:, :3], xv), np.where(ok, o["a"][:, :3], xa), pf)


@pytest.mark.parametrize("variant", ["bound", "cpp2"])
@pytest.mark.parametrize("scene", ["golden", "random"])
def test_every_finisher_writes_the_same_words(scene, variant):
    kw, inputs, nsteps, _ = _scene(scene)
    ctx = {}
    for leg, opts in LEGS.items():
        ctx[leg] = mp.Dmpc(variant, **kw)
        for k_, v_ in opts.items():
            ctx[leg].debug_option(k_, v_)
    by_scan = by_solver = 0
    for step in range(nsteps):
        out = {leg: d.step_batch(*inputs) for leg, d in ctx.items()}   # every leg gets the default leg's states: the same agents in each
        ref = out["default"]
        if step == 0:
            assert ctx["default"].last_solve_kernel == "dmpc_rsolve_persist_kernel" and ctx["general"].last_solve_kernel.startswith("dmpc_solve_")
        # scan exit against the solver that would have finished the agent: the reduced one, the general one
        for a, b in (("default", "no_fast_exit"), ("general", "general_no_fast_exit")):
            for k in ("p", "v", "a", "status"):
                assert np.array_equal(out[a][k], out[b][k]), (scene, variant, step, a, b, k)
            assert np.array_equal(out[a]["info"][:, :4], out[b]["info"][:, :4]), (scene, variant, step, a, b, "info")
        # reduced against general solver
        gen = out["general"]
        assert np.array_equal(ref["status"], gen["status"]) and np.array_equal(ref["info"][:, :4], gen["info"][:, :4]), (scene, variant, step)
        ok = (ref["status"] & mp.ST_SOLVED) != 0
        e = np.zeros(len(ok))
        for k in ("p", "v", "a"):
            e = np.maximum(e, np.abs(ref[k] - gen[k]).max(axis=1))
        first = ref["info"][:, 2] == 1
        print(f"{scene} {variant} step {step}: reduced vs general l_inf first level {e[ok & first].max(initial=0.0):.2e}, ladder {e[ok & ~first].max(initial=0.0):.2e} "
              f"({int((ok & ~first).sum())} agents)")
        assert (e[ok & first] <= FIRST).all() and (e[ok & ~first] <= LADDER).all(), (scene, variant, step, float(e[ok].max()))
        assert (e[~ok] == 0.0).all()     # (outputs of unsolved agents are zero in every leg)
        if scene == "random" and step == 0:   # the agents at the walls: what the oracle says, in every leg
            want = _oracle_first_step(variant)["status"][[WALL_HI, WALL_LO]]
            assert list(want) == [mp.ST_SOLVED, mp.ST_INFEAS]
            for leg in LEGS:
                assert np.array_equal(out[leg]["status"][[WALL_HI, WALL_LO]], want), (variant, leg)
            # on the wall, to rounding: the in-bounds test (bound) looked at a position 50 mm inside its margin
            assert abs(ref["p"][WALL_HI, 0] - kw["pmax"][0]) <= 1e-9
        trivial = ok & (ref["info"][:, 4] == 0)      # no iteration: the unconstrained minimiser is feasible (the default leg's scan finished these)
        by_scan += int(trivial.sum()); by_solver += int((ok & ~trivial).sum())
        inputs = _advance(inputs, ref)
    print(f"{scene} {variant}: {by_scan} agent-steps finished by the scan's exit, {by_solver} by a solver")
    assert by_scan > 0 and by_solver > 0


@pytest.mark.parametrize("variant", ["bound", "cpp2"])
@pytest.mark.parametrize("scene", ["golden", "random"])
def test_fused_post_step_equals_the_post_step_kernel(scene, variant):
    """two MPC steps of a transition (three history columns): the solve kernels' own post-step -- agent_outputs for the agents they solve,
    agent_skip for the ones the scan finished -- against post_step_kernel"""
    kw, _, _, (po, pf) = _scene(scene)
    cfg = wl.CONFIGS["C4"]
    a = mp.Dmpc(variant, **kw).transition(po, pf, 3, cfg["error_tol"])
    b = mp.Dmpc(variant, **kw).debug_option("no_fuse", 1).transition(po, pf, 3, cfg["error_tol"])
    for k in ("pk", "vk", "ak", "K_T_used", "scene_status"):
        assert np.array_equal(a[k], b[k]), (scene, variant, k)
    assert np.abs(a["pk"][:, 2] - a["pk"][:, 0]).max() > 0     # the agents did move
