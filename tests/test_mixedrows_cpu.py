"""The conditions of tests/test_gpu_mixed_rows.py, proven without a GPU (tests/mixedrows.py): the helper's restatement of the scan equals the oracle,
its bounds admit honest fp32 -- two numpy emulations of the row builder's expressions, float32 left to right and with every a * b + c fused --, the
random cells stay under the ambiguity cap and hold the populations the GPU tests rest on, and the constructed sweeps straddle their thresholds."""
import numpy as np
import pytest

from oracle import oracle as orc
import mixedrows as mr


def _outcome(o):
    return (o["nrows"], o["viol_k"], o["status"])


@pytest.mark.parametrize("variant", mr.ORDER2)
def test_helper_restates_the_oracle(variant):
    """on the UNROUNDED inputs of every random cell: the helper's structured reference rows, expanded, equal the oracle's dense G to 1e-12, and its
    scan record decided on dist alone -- first violating step, row count, ST_COLL -- equals the oracle's on every agent that is not ambiguous
    (and on the rounded inputs too, which is where the GPU tests use it)"""
    rows = agents = 0
    for name in mr.CELLS:
        kw, raw = mr.cell_raw(variant, name)
        for sc in list(raw) + list(mr.cell(variant, name)[1]):
            for n in range(len(sc[0])):
                r = mr.reference(variant, kw, sc, n)
                if r["ambiguous"]:
                    continue
                o, rec = r["oracle"], r["rec"]
                assert (len(rec["rows"]), rec["viol_k"], 4 if rec["coll"] else 0) == _outcome(o), (name, n)
                if o["nrows"]:
                    assert np.abs(mr.expand(r["xi"], r["kc"], kw["h"]) - o["G"]).max() <= 1e-12, (name, n)
                    assert np.abs(r["d"] - o["dist"]).max() <= 1e-12
                rows += o["nrows"]; agents += 1
    assert rows > 0 and agents > 0


@pytest.mark.parametrize("variant", mr.ORDER2)
def test_bounds_admit_honest_fp32_and_cells_hold_their_populations(variant):
    """every row of every random cell: both emulations inside every bound (the worst err / bound is printed per quantity); every cell under the
    ambiguity cap; every cell of `bound` and `hard`, and the cells of every other variant together, with rows that the exact pruning must drop
    (b - |xi|_1 hw >= MARG + tau).  Certificate and ladder cases are counted:
    the random cells hold almost none, which is what the box-slack sweeps are for."""
    total = 0
    for name in mr.CELLS:
        kw, cols = mr.cell_refs(variant, name)
        worst = {False: {}, True: {}}
        amb = steps = nrows = prunable = cert = ladder = 0
        for sc, refs in cols:
            for r in refs:
                steps += 1
                if r["ambiguous"]:
                    amb += 1
                    continue
                if not len(r["kc"]):
                    continue
                nrows += len(r["kc"])
                prunable += int((r["b"] - r["x1"] * r["hw"] >= mr.MARG + r["tau"]).sum())
                cert += int(variant in mr.SLACK_FREE and (r["b"] + r["x1"] * r["hw"] < -mr.MARG - r["tau"]).any())
                ladder += int(variant in mr.LADDER and mr.ladder_level(r, mr.MARG + r["tau"]) > 0)
                for fused in (False, True):
                    q = mr.ratios(variant, kw, r, mr.emulate(variant, kw, sc, r, fused))
                    for key, v in q.items():
                        worst[fused][key] = max(worst[fused].get(key, 0.0), v)
        fmt = lambda w: " ".join(f"{k}={v:.3f}" for k, v in w.items())
        print(f"mixedrows [{variant} {name}]: {steps} agent-steps, {amb} ambiguous, {nrows} rows, {prunable} prunable, {cert} certificate agents, "
              f"{ladder} ladder agents; err/bound float32: {fmt(worst[False])}; fused: {fmt(worst[True])}")
        assert amb <= mr.AMBIGUOUS_CAP * steps, (name, amb, steps)
        assert nrows > 0 and (prunable > 0 or variant not in ("bound", "hard")), (name, nrows, prunable)
        total += prunable
        for fused in (False, True):
            assert all(v <= 1.0 for v in worst[fused].values()), (name, fused, worst[fused])
    # (cpp, cpp2: the radius rmin (1 + k / K) selects only neighbours the agent can still reach -- none of their 300-500 rows per cell is prunable)
    assert total > 0 or variant in ("cpp", "cpp2")


@pytest.mark.parametrize("c", [2.0, 3.0])
@pytest.mark.parametrize("axis", ["x", "z"])
@pytest.mark.parametrize("kind", mr.cr.TIE_KINDS)
def test_threshold_sweeps_straddle(kind, axis, c):
    """the outcome of the oracle's step for the probe (status, first violating step, row count) on the rounded inputs differs between m = -64 and m = +64, is constant on either side from |m| = 16 out,
    and the probe is ambiguous exactly inside the band"""
    variant, kw, scenes = mr.tie_sweep(kind, axis, c)
    prm = orc.make_params(variant, **kw)
    out = {m: mr.step_outcome(orc.step(prm, *sc), 0) for m, sc in scenes}
    assert out[-64] != out[64]
    assert out[-16] == out[-64] and out[16] == out[64]
    for m, sc in scenes:
        if abs(m) >= 16:
            assert not mr.reference(variant, kw, sc, 0)["ambiguous"], m


@pytest.mark.parametrize("variant", ["hard", "bound"])
def test_box_slack_sweeps_straddle(variant):
    """the constructed row sits where it should: b + |xi|_1 hw = d (hw - (rmin - d)) to fp64 round-off; at -4 tau the reference is certainly
    infeasible (hard) / its ladder certainly starts at level 1 (bound), at +4 tau certainly not, whatever side of MARG the fp32 error falls on"""
    kw, d0, tau, scenes = mr.box_sweep(variant)
    hw = kw["alim"] * (mr.BOX_KC * kw["h"]) ** 2 / 2.0
    side = {}
    for s, sc in scenes:
        r = mr.reference(variant, kw, sc, 0)
        assert not r["ambiguous"] and r["kc"][0] == mr.BOX_KC and r["rec"]["viol_k"] == (0 if variant == "hard" else mr.BOX_KC)
        d = sc[0][1, 3 * (mr.BOX_KC - 1)]
        assert abs((r["b"][0] + r["x1"][0] * r["hw"][0]) - d * (hw - (kw["rmin"] - d))) <= 1e-15
        assert abs(r["tau"][0] / tau - 1.0) < 1e-3
        if variant == "hard":
            lo, hi = (r["b"] + r["x1"] * r["hw"] < -mr.MARG - r["tau"]).any(), (r["b"] + r["x1"] * r["hw"] < -mr.MARG + r["tau"]).any()
        else:
            lo, hi = mr.ladder_level(r, mr.MARG + r["tau"]), mr.ladder_level(r, mr.MARG - r["tau"])
        side[s] = (int(lo), int(hi))
    assert side[-4.0] == (1, 1) and side[4.0] == (0, 0), side
    assert side[-0.25] == (0, 1) and side[0.25] == (0, 1), side
    if variant == "hard":      # (the sweep crosses -MARG, not zero: the row is infeasible in the reference on both sides, and the oracle's step says so)
        prm = orc.make_params(variant, **kw)
        assert all(int(orc.step(prm, *sc)["status"][0]) & orc.ST_INFEAS for _, sc in scenes)
