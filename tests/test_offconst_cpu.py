"""CPU: the oracle alone on the cells of tests/offconst.py -- 13 variants x 16 parameter sets off the reference's constants, 32 agents, five
teacher-forced closed-loop steps, the box at the origin.  It pins what tests/test_gpu_offconst.py relies on, so that its conditions are known
to be met by the reference before a GPU is involved.  Per cell:

  * at least 50 of the 160 agent-steps carry collision rows (the scene is not an unconstrained one);
  * exact_minimiser resolves the oracle's answers: at most 2 agent-steps per cell stay unresolved.  On the host these figures come from NO
    cell has any (another host's BLAS may move that; the cap is what is asserted, and the count of every cell is printed);
  * every infeasible verdict of the oracle is confirmed by the phase-1 LP of tests/certificates.py (no active-set code).

softall_c used to leave most agents of every cell unresolved (3 076 of 5 120 agent-steps): its slack weights 1e6 (K/k)^2 next to 1e3 on an
acceleration put the pivots of a sound KKT matrix below kkt_point's dependence test.  exactqp.exact_minimiser now solves such a system again
with the variables scaled to a unit diagonal of H, and softall_c is held to x* like every other variant.  (The same retry resolves the one
agent-step of all3 at Q1=1e5 that was `singular` before.)

Printed per cell: agent-steps with rows, statuses, highest ladder level, unresolved count, the oracle's worst |a - x*| and the largest
multiplier.  Measured on one host: worst per variant 1.6e-10 (bound), 1.4e-10 (bound2), 1.0e-11 (cpp), 3.6e-12 (cpp2, ondemand, ellip,
softall_c), 2.6e-12 (hard), 3.8e-12 (scp), 1.1e-9 (repair), 3.0e-9 (all3), 1.2e-9 (softall), 5.2e-8 (cpp1, at h=0.05); bound, bound2, cpp,
repair and all3 have theirs at term=-1e7.  The ladder reaches level 4 (bound2, cpp, cpp2) and 6 (all3); hard, ondemand, ellip and scp give
infeasible verdicts, 79 of 160 for hard at rmin=0.6,c=3.  These are facts about the reference, not bars for anything.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from helpers import ALL_VARIANTS
from test_certificates_cpu import check_batch
import offconst as oc


@functools.lru_cache(maxsize=None)
def _scene(name):
    kw, po, pf = oc.scene(name)
    po.setflags(write=False); pf.setflags(write=False)
    return kw, po, pf


@pytest.mark.parametrize("name", list(oc.SETS))
@pytest.mark.parametrize("variant", ALL_VARIANTS)
def test_oracle_cell_has_rows_resolves_and_its_infeasible_verdicts_hold(variant, name):
    kw, po, pf = _scene(name)
    loop = oc.closed_loop(variant, kw, po, pf)
    facts = oc.cell_facts(loop)
    A = oc.compare_cell(loop)
    res = A["resolved"].astype(bool)
    unresolved = int((~res).sum())
    n_inf = 0
    for k, (prm, sc, ref) in enumerate(loop):
        agents = np.nonzero(ref["status"] & orc.ST_INFEAS)[0]
        ns, ni, _ = check_batch(prm, *sc, ref["a"], ref["status"], ref["info"][:, orc.I_TRIES], f"oracle {variant} [{name}] step {k + 2}", agents=agents)
        assert ns == 0 and ni == len(agents)
        n_inf += ni
    print(f"[{variant} | {name}] rows on {facts['row_steps']} of {oc.N * oc.STEPS} agent-steps, statuses {facts['statuses']}, ladder level up to "
          f"{facts['level']}, {len(res)} solved, {unresolved} unresolved, {n_inf} infeasible (LP confirmed), oracle worst |a - x*| "
          f"{A['e'][res].max() if res.any() else 0.0:.2e}, lam_max up to {A['lam_max'][res].max() if res.any() else 0.0:.2e}")
    assert facts["row_steps"] >= oc.MIN_ROW_STEPS
    assert len(res) == sum(int(((ref["status"] & 1) == 1).sum()) for _, _, ref in loop) and len(res) > 0
    assert unresolved <= oc.CAP_UNRESOLVED, f"{unresolved} agent-steps unresolved: steps {A['step'][~res]}, agents {A['agent'][~res]}"


def test_the_moved_scene_is_the_same_scene():
    """translating box and points leaves the QP of every agent unchanged in exact arithmetic: the oracle's records at the offset equal those at
    the origin on the sets the GPU test runs at both (a decision within rounding of a threshold would show here first)"""
    for name in oc.MOVED_SETS:
        kw0, po0, pf0 = _scene(name)
        kw1, po1, pf1 = oc.scene(name, offset=oc.MOVED)
        assert np.abs(po1 - np.asarray(oc.MOVED) - po0).max() < 1e-13
        for variant in ("bound", "hard"):
            a, b = oc.closed_loop(variant, kw0, po0, pf0), oc.closed_loop(variant, kw1, po1, pf1)
            for (_, _, r0), (_, _, r1) in zip(a, b):
                assert np.array_equal(r0["status"], r1["status"]) and np.array_equal(r0["info"][:, :4], r1["info"][:, :4]), (name, variant)
