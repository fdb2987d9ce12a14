"""GPU: the launch rule, pinned.  Which solve kernel one MPC step launches for the bulk of its agents (dmpc_last_solve_kernel) for a table of
(variant, precision, scenes, agents per scene, development options), every branch of the rule once at the smallest launch that takes it.

The thresholds of the rule scale with the CU count, so the shapes are given relative to ncu = multi_processor_count.  The expected names are
those of the rule as it stood BEFORE it moved into plan_step, worked out by hand from it (below; LDS sizes for 256 CUs and 160 KB per CU), not
produced by the code under test.  `python tests/test_gpu_launch_plan.py` prints the table of the library it runs against and says whether it
equals this one; tools/with_lib.py selects another build (the one before the move, to record from it):

* tiny (< 8 ncu agents): one tier with the full capacity (64 slots, slack-free 48), one agent per workgroup;
* from 8 ncu on: first tier 48 slots (56: scenes of >= 1 024 agents, solveSoftDMPCall), one agent per workgroup while shallow
  (< 128 ncu; heavy agents < 28 ncu; large soft scenes < 8 ncu), persistent waves once deep (>= 16 pw ncu; heavy 28 ncu; large soft scenes at once);
  pw = 12 waves per workgroup for solveHardDMPC with the split factor (HARD_TS = 16 own columns), 9 without (no_split_t);
* solveSoftDMPCbound / bound2 / solveQPv2: the reduced solver in every launch form, unless reduced_solver = 0 or the fp32 factor;
* the fp32 factor: one tier with the full capacity; solveDMPC: its own kernel.

Names only, and that every status is a valid one: parity is the other suites' job."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multiagent_planning_amd as mp  # noqa: E402
from multiagent_planning_amd import workload as wl  # noqa: E402

pytestmark = pytest.mark.gpu

RSOLVE = "dmpc_rsolve_persist_kernel"
PW_HARD, PW_HARD_NOSPLIT = 12, 9   # persistent waves per workgroup of the slack-free kernels at N = 100 (see above)
GENERAL = dict(reduced_solver=0)


def _up(agents, n):
    """scenes of n agents that make at least `agents` agents"""
    return -(-agents // n)


# (id, variant, precision, shape(ncu) -> (S, N), options, expected name)
CASES = [
    # tiny / first tier: just below and at 8 ncu agents (16 scenes of ncu / 2)
    ("bound_below_8ncu", "bound", "f64", lambda c: (15, (c + 1) // 2), {}, RSOLVE),
    ("bound_at_8ncu", "bound", "f64", lambda c: (16, (c + 1) // 2), {}, RSOLVE),
    ("bound_general_below_8ncu", "bound", "f64", lambda c: (15, (c + 1) // 2), GENERAL, "dmpc_solve_kernel<true, 64, double>"),
    ("bound_general_at_8ncu", "bound", "f64", lambda c: (16, (c + 1) // 2), GENERAL, "dmpc_solve_kernel<true, 48, double>"),
    ("hard_below_8ncu", "hard", "f64", lambda c: (15, (c + 1) // 2), {}, "dmpc_solve_kernel<false, 48, double>"),
    ("hard_at_8ncu", "hard", "f64", lambda c: (16, (c + 1) // 2), {}, "dmpc_solve_kernel<false, 48, double>"),
    # slack-free, deep: one agent per workgroup up to 16 pw ncu, then persistent waves with HARD_TS own columns (all 48 with no_split_t)
    ("hard_at_128ncu", "hard", "f64", lambda c: (_up(128 * c, 100), 100), {}, "dmpc_solve_kernel<false, 48, double>"),
    ("hard_at_16pw_ncu", "hard", "f64", lambda c: (_up(16 * PW_HARD * c, 100), 100), {}, "dmpc_solve_persist_kernel<false, 48, 16, double>"),
    ("hard_nosplit_at_16pw_ncu", "hard", "f64", lambda c: (_up(16 * PW_HARD_NOSPLIT * c, 100), 100), dict(no_split_t=1), "dmpc_solve_persist_kernel<false, 48, 48, double>"),
    # large soft scenes: one scene of 1 024 agents (tiny on a GPU of more than 128 CUs), and 8 ncu agents in such scenes (the 56-slot split persistent tier)
    ("bound_1024_general", "bound", "f64", lambda c: (1, 1024), GENERAL, "dmpc_solve_kernel<true, 64, double>" ),
    ("bound_1024", "bound", "f64", lambda c: (1, 1024), {}, RSOLVE),
    ("bound_8ncu_of_1024_general", "bound", "f64", lambda c: (_up(8 * c, 1024), 1024), GENERAL, "dmpc_solve_persist_kernel<true, 56, 48, double>"),
    # heavy agents: all-neighbour variants in scenes of >= 200 agents go persistent from 28 ncu on
    ("softall_200_at_28ncu", "softall", "f64", lambda c: (_up(28 * c, 200), 200), {}, "dmpc_solve_persist_kernel<true, 48, 48, double>"),
    # solveSoftDMPCall: 56 slots first at any scene size -- once the launch has tiers at all
    ("all3_small", "all3", "f64", lambda c: (2, 20), {}, "dmpc_solve_kernel<true, 64, double>"),
    ("all3_at_8ncu", "all3", "f64", lambda c: (16, (c + 1) // 2), {}, "dmpc_solve_kernel<true, 56, double>"),
    # the options of the tests, 8 scenes of 60 agents: as they stand (the reduced solver takes solveSoftDMPCbound whatever they say) and on the general solver
    ("bound_tier32", "bound", "f64", lambda c: (8, 60), dict(tier1_qcap=32), RSOLVE),
    ("bound_force_persist", "bound", "f64", lambda c: (8, 60), dict(force_persist=1), RSOLVE),
    ("bound_no_persist", "bound", "f64", lambda c: (8, 60), dict(no_persist=1), RSOLVE),
    ("bound_general_tier32", "bound", "f64", lambda c: (8, 60), dict(GENERAL, tier1_qcap=32), "dmpc_solve_kernel<true, 32, double>"),
    ("bound_general_force_persist", "bound", "f64", lambda c: (8, 60), dict(GENERAL, force_persist=1), "dmpc_solve_persist_kernel<true, 48, 48, double>"),
    ("bound_general_force_no_persist", "bound", "f64", lambda c: (8, 60), dict(GENERAL, force_persist=1, no_persist=1), "dmpc_solve_kernel<true, 48, double>"),
    # fp32 inverse factor: one tier, full capacity, no reduced solver
    ("bound_f32factor", "bound", "f32factor", lambda c: (8, 60), {}, "dmpc_solve_kernel<true, 64, float>"),
    ("hard_f32factor", "hard", "f32factor", lambda c: (8, 60), {}, "dmpc_solve_kernel<false, 48, float>"),
    ("bound_f32factor_persist", "bound", "f32factor", lambda c: (8, 60), dict(force_persist=1), "dmpc_solve_persist_kernel<true, 64, 64, float>"),
    ("hard_f32factor_persist", "hard", "f32factor", lambda c: (8, 60), dict(force_persist=1), "dmpc_solve_persist_kernel<false, 48, 48, float>"),
    # solveDMPC
    ("scp", "scp", "f64", lambda c: (2, 8), {}, "dmpc_scp_kernel"),
]

_CFG = dict(hard="C2", softall="C3", scp="C2")   # the workload whose constants and generator a variant's scenes take (default: C4)
VALID = 1 | 2 | 4 | 8 | 16 | 32                  # DMPC_ST_* of an agent (64 is internal to the tiers and must not leave the library)


def ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(variant, precision, S, N, opts):
    """one MPC step (the first of a transition) of S random feasible scenes of N agents: (kernel name, statuses)"""
    cfg = wl.CONFIGS[_CFG.get(variant, "C4")]
    kw = wl.solver_kwargs(cfg, N)
    if variant == "scp":
        kw["tol"] = 0.05
    d = mp.Dmpc(variant, precision=precision, **kw)
    try:
        for k, v in opts.items():
            d.debug_option(k, v)
        if S * N > 4096:   # (the generators' rejection sampling on the GPU: the host's takes seconds at this size)
            po, pf = wl.make_scenes_device(d, cfg, S, N, wl.SEED0 + 77)
        else:
            po, pf = wl.make_scenes(cfg, S, N, wl.SEED0 + 77)
        l, _, _ = d.init_batch(po, pf)
        z = np.zeros_like(po)
        out = d.step_batch(l, po, z, z, pf)
        return d.last_solve_kernel, out["status"]
    finally:
        d.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_solve_kernel_of_one_step(case):
    _, variant, precision, shape, opts, expected = case
    S, N = shape(ncu())
    name, status = run_case(variant, precision, S, N, opts)
    print(f"{case[0]}: S={S} N={N} -> {name}")
    assert name == expected, (case[0], S, N)
    assert status.shape == (S, N)
    assert ((status & ~VALID) == 0).all() and (status != 0).all(), np.unique(status)


if __name__ == "__main__":   # the recording loop: the table of the library this process loads
    c = ncu()
    bad = 0
    for cid, variant, precision, shape, opts, expected in CASES:
        S, N = shape(c)
        name, status = run_case(variant, precision, S, N, opts)
        bad += name != expected
        print(f"{cid:34s} ncu={c} S={S:4d} N={N:5d} {name}{'' if name == expected else '   != table: ' + expected}"
              f"   statuses {sorted(int(x) for x in np.unique(status))}", flush=True)
    print("recorded names differ from the table" if bad else "recorded names equal the table")
