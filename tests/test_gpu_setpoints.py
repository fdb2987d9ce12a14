"""GPU: flight setpoints and limits report (dmpc_postcheck_setpoints, Dmpc.setpoints) -- p, v, a of every commanded agent at the 100 Hz samples
of the post-check and, per agent, the largest |v| and |a| over the whole transition with its sample.

The reference is tests/setpoints.py: scipy's not-a-knot spline through each of the three rescaled histories (tests/test_setpoints_cpu.py
shows what that tells apart).  Bars: p against MATLAB's record 1e-11 (test_postcheck_matches_matlab_record's), v and a against the
restatement 1e-10 (_check's bar for p against the same spline), peaks against numpy norms of the library's own setpoints 8 ulp (two FMAs
against three roundings, the clearance tests' bar); everything that must not depend on the call's shape is compared as bytes."""
import os

import numpy as np
import pytest

import multiagent_planning_amd as mp
from multiagent_planning_amd import resultio, workload as wl
import mission as ms
import setpoints as sp
from helpers import GOLD, lib_source, unrescale

pytestmark = pytest.mark.gpu

SETPOINTS = ("p", "v", "a")
REPORT = ("v_peak", "v_peak_sample", "a_peak", "a_peak_sample")
SCALARS = ("r_factor", "h_scaled", "n_samples")


def _same(a, b, what, keys=REPORT + SCALARS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _err(d):
    return d._L.dmpc_last_error(d._ctx).decode()


def _vs_restatement(out, s, ref, what):
    n = ref["n_samples"]
    assert out["n_samples"][s] == n and abs(out["h_scaled"][s] - ref["h_scaled"]) <= 1e-13 and abs(out["r_factor"][s] - ref["r_factor"]) <= 1e-13 * ref["r_factor"]
    for k in SETPOINTS:
        e = np.abs(out[k][s][:, :n] - ref[k]).max()
        print(f"{what}: |{k} - restatement| max {e:.3e}")
        assert e <= sp.TOL, (what, k, e)
        assert not out[k][s][:, n:].any(), (what, k)
    for k in "va":
        assert np.abs(out[k + "_peak"][s] - ref[k + "_peak"]).max() <= sp.TOL, (what, k)


def _peaks_vs_own_setpoints(out, s, what):
    """the report against numpy norms of the returned v / a of scene s (a full-window call)"""
    n = int(out["n_samples"][s])
    for k in "va":
        nrm = sp.norms(out[k][s][:, :n])
        peak, smp = out[k + "_peak"][s], out[k + "_peak_sample"][s]
        tol = sp.ULPS * np.spacing(nrm.max(axis=1))
        assert (np.abs(peak - nrm.max(axis=1)) <= tol).all(), (what, k)
        assert ((smp >= 0) & (smp < n)).all(), (what, k)
        at = nrm[np.arange(len(smp)), smp]
        assert (np.abs(at - peak) <= tol).all(), (what, k)
        for i in range(len(smp)):
            assert not (nrm[i, :smp[i]] > peak[i] + tol[i]).any(), (what, k, i)


# ---- 1. the recorded MATLAB block -------------------------------------------------------------------------------------------------------------
def test_recorded_block_p_is_matlabs_v_a_the_restatement_and_one_agent_exceeds_amax():
    g = np.load(os.path.join(GOLD, "postcheck_comp_kctr_2.npz"))
    p, v, a = unrescale(g)
    lim = dict(vmax=float(g["vmax"]), amax=float(g["amax"]), Ts=float(g["Ts"]))
    d = mp.Dmpc("bound2", **dict(sp.KW, h=float(g["h"]), rmin=float(g["rmin"]), c=float(g["c"])))
    out = d.setpoints([p.shape[1]], pk=p, vk=v, ak=a, **lim)
    assert out["p"].shape == (1, 20, int(g["n_samples"]), 3)
    assert np.abs(out["p"][0][:, g["p_idx"]] - g["p"]).max() < 1e-11          # MATLAB's own spline(tk, pk, t)
    _vs_restatement(out, 0, sp.restate(p, v, a, float(g["h"]), lim["vmax"], lim["amax"], lim["Ts"]), "recorded block")
    over = np.where(out["a_peak"][0] > lim["amax"])[0]
    print("a_peak", out["a_peak"][0, 2], "at sample", out["a_peak_sample"][0, 2], "v_peak max", out["v_peak"][0].max())
    assert list(over) == [2] and out["a_peak_sample"][0, 2] == 143 and abs(out["a_peak"][0, 2] - 1.0044) < 5e-5
    assert not (out["v_peak"][0] > lim["vmax"]).any()
    _peaks_vs_own_setpoints(out, 0, "recorded block")


# ---- 2, 3. the ragged batch ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    used, P, V, A = sp.ragged_batch()
    d = mp.Dmpc("bound", **sp.KW)
    keep = [x.copy() for x in (P, V, A)]
    full = d.setpoints(used, pk=P, vk=V, ak=A)
    for x, y in zip((P, V, A), keep):
        assert np.array_equal(x, y)                                            # inputs untouched
    return dict(d=d, used=used, hist=(P, V, A), full=full)


def test_ragged_batch_vs_restatement(ragged):
    d, used, (P, V, A), full = ragged["d"], ragged["used"], ragged["hist"], ragged["full"]
    assert full["p"].shape == (7, 7, int(full["n_samples"].max()), 3)
    for s in range(len(used)):
        n = int(used[s])
        _vs_restatement(full, s, sp.restate(P[s][:, :n], V[s][:, :n], A[s][:, :n]), f"scene {s} ({n} knots)")
        _peaks_vs_own_setpoints(full, s, f"scene {s}")
    again = d.setpoints(used, pk=P, vk=V, ak=A)
    _same(again, full, "repeated call", SETPOINTS + REPORT + SCALARS)


def test_p_is_postchecks_p_interp_byte_for_byte(ragged):
    d, used, (P, V, A), full = ragged["d"], ragged["used"], ragged["hist"], ragged["full"]
    pf = P[np.arange(len(used)), :, used - 1]
    pc = d.postcheck(used, pf, P, V, A, interp=True)
    assert pc["p"].shape == full["p"].shape and np.array_equal(pc["p"], full["p"])
    _same(pc, full, "postcheck / setpoints", SCALARS)


# ---- 4. windows --------------------------------------------------------------------------------------------------------------------------------
def test_windows_are_slices_of_the_full_call(ragged):
    d, used, hist, full = ragged["d"], ragged["used"], ragged["hist"], ragged["full"]
    ns = full["n_samples"]
    top = int(ns.max())
    inside = int(ns[ns > 0].min()) // 2
    for first, count in ((3, inside - 3), (inside, top), (top - 5, 40), (top + 7, 9), (257, 1), (0, 1)):
        w = d.setpoints(used, pk=hist[0], vk=hist[1], ak=hist[2], first=first, count=count)
        _same(w, full, f"window {first}+{count}")
        for k in SETPOINTS:
            want = np.zeros_like(w[k])
            hi = min(first + count, top)
            if hi > first:
                want[:, :, :hi - first] = full[k][:, :, first:hi]
            assert w[k].shape == (7, 7, count, 3) and w[k].tobytes() == want.tobytes(), (first, count, k)
    # only some of the arrays: the others are not written, the one asked for is the same bytes
    L, S, N = d._L, 7, 7
    v_only = np.zeros((S, N, top, 3))
    assert L.dmpc_postcheck_setpoints(d._ctx, S, N, 40, mp._lib._ip(used), None, *(mp._lib._dp(h) for h in hist), 2.0, 1.0, 0.01, 0, top, None, mp._lib._dp(v_only),
                                      None, None, None, None, None, None, None, None) == 0, _err(d)
    assert v_only.tobytes() == full["v"].tobytes()


# ---- 5. ties -----------------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_smallest_sample():
    p, v, a = sp.tie_scene()
    ref = sp.restate(p, v, a)
    for batch in (0, 100):
        d = mp.Dmpc("bound", **sp.KW).debug_option("setpoint_batch", batch)
        for first in (0, 300):
            out = d.setpoints([sp.TIE_KT], pk=p, vk=v, ak=a, first=first)
            for i in (0, 2):
                assert out["v_peak"][0, i] == ref["v_peak"][i] and out["v_peak_sample"][0, i] == 0, (batch, first, i)
                assert out["a_peak"][0, i] == 0.0 and out["a_peak_sample"][0, i] == 0, (batch, first, i)
                n = ref["n_samples"]
                assert (sp.norms(out["v"][0, i, :n - first]) == ref["v_peak"][i]).all()
            assert out["v_peak_sample"][0, 1] == ref["v_peak_sample"][1] and out["a_peak_sample"][0, 1] == ref["a_peak_sample"][1]
    _peaks_vs_own_setpoints(d.setpoints([sp.TIE_KT], pk=p, vk=v, ak=a), 0, "tie scene")


# ---- 6. independence ---------------------------------------------------------------------------------------------------------------------------
def test_report_and_setpoints_do_not_depend_on_the_shape_of_the_call(ragged):
    d, used, (P, V, A), full = ragged["d"], ragged["used"], ragged["hist"], ragged["full"]
    rep = d.setpoints(used, pk=P, vk=V, ak=A, report_only=True)
    assert not any(k in rep for k in SETPOINTS)
    _same(rep, full, "report only / full call")
    top = full["p"].shape[2]
    for s in range(len(used)):
        one = d.setpoints(used[s:s + 1], pk=P[s:s + 1], vk=V[s:s + 1], ak=A[s:s + 1], count=top)
        for k in SETPOINTS + REPORT + SCALARS:
            assert one[k][0].tobytes() == full[k][s].tobytes(), (s, k)
    for batch in (1, 7):
        e = mp.Dmpc("bound", **sp.KW).debug_option("setpoint_batch", batch)
        cut = 24 if batch == 1 else top                                        # (one sample per pass: a short window, and the report over all samples)
        out = e.setpoints(used, pk=P, vk=V, ak=A, count=cut)
        _same(out, full, f"setpoint_batch = {batch}")
        for k in SETPOINTS:
            assert out[k].tobytes() == np.ascontiguousarray(full[k][:, :, :cut]).tobytes(), (batch, k)


def test_agent_tiles_300_agents_equal_two_calls_of_150():
    p, v, a = sp.wide_scene()
    d = mp.Dmpc("bound", **sp.KW)
    whole = d.setpoints([sp.WIDE_KT], pk=p, vk=v, ak=a)
    for lo in (0, 150):
        half = d.setpoints([sp.WIDE_KT], pk=p[lo:lo + 150], vk=v[lo:lo + 150], ak=a[lo:lo + 150])
        _same(half, whole, "half / whole", SCALARS)
        for k in SETPOINTS + REPORT:
            assert half[k][0].tobytes() == np.ascontiguousarray(whole[k][0, lo:lo + 150]).tobytes(), (lo, k)
    _peaks_vs_own_setpoints(whole, 0, "300 agents")
    assert (whole["v_peak"] > 0).all() and (whole["a_peak"] > 0).all()


# ---- 7. resident histories ---------------------------------------------------------------------------------------------------------------------
def test_resident_histories_after_a_transition_equal_host_arrays():
    cfg, N, KTm = wl.CONFIGS["C4"], 12, 151
    po, pf = wl.make_scenes(cfg, 3, N=N)
    d = mp.Dmpc(cfg["variant"], **wl.solver_kwargs(cfg, N))
    tr = d.transition(po, pf, KTm)
    assert (tr["scene_status"] == (mp.ST_SOLVED | mp.ST_REACHED)).all()
    mask = np.array([1, 0, 1], dtype=np.int32)
    res = d.setpoints(tr["K_T_used"], N=N, KT_alloc=KTm, mask=mask)
    host = d.setpoints(tr["K_T_used"], pk=tr["pk"], vk=tr["vk"], ak=tr["ak"], mask=mask)
    _same(res, host, "resident / host", SETPOINTS + REPORT + SCALARS)
    # the masked scene: NaN / -1 / zeros
    assert np.isnan(res["v_peak"][1]).all() and np.isnan(res["a_peak"][1]).all() and (res["v_peak_sample"][1] == -1).all() and (res["a_peak_sample"][1] == -1).all()
    assert np.isnan(res["r_factor"][1]) and res["n_samples"][1] == 0 and not any(res[k][1].any() for k in SETPOINTS)
    for s in (0, 2):
        n = int(tr["K_T_used"][s])
        _vs_restatement(res, s, sp.restate(tr["pk"][s][:, :n], tr["vk"][s][:, :n], tr["ak"][s][:, :n], wl.solver_kwargs(cfg, N)["h"]), f"C4 scene {s}")
        _peaks_vs_own_setpoints(res, s, f"C4 scene {s}")


def test_resident_histories_of_a_split_batch_and_of_a_mission():
    b = ms.batch(["reached"] * 40, list(range(40)))
    d = mp.Dmpc("bound", **ms.KW)
    src = lib_source()
    assert "(S >= 128 ? 4 : (S >= 32 ? 2 : 1))" in src                        # (40 scenes: two parts on contexts of their own)
    tr = d.transition(b["po"], b["goals"][:, 0], 30, ms.ERROR_TOL)
    res = d.setpoints(tr["K_T_used"], N=4, KT_alloc=30)
    host = d.setpoints(tr["K_T_used"], pk=tr["pk"], vk=tr["vk"], ak=tr["ak"])
    _same(res, host, "split batch: resident / host", SETPOINTS + REPORT + SCALARS)
    assert (res["v_peak"] > 0).all() and res["p"][39].any()
    s = ms.scene("reached")
    mi = d.mission(s["po"][None], s["goals"][None], ms.KT, ms.ERROR_TOL)
    assert int(mi["scene_status"][0]) == ms.REACHED
    res = d.setpoints(mi["K_T_used"], N=4, KT_alloc=ms.KT)
    host = d.setpoints(mi["K_T_used"], pk=mi["pk"], vk=mi["vk"], ak=mi["ak"])
    _same(res, host, "mission: resident / host", SETPOINTS + REPORT + SCALARS)
    assert np.isfinite(res["a_peak"]).all() and (res["v_peak_sample"] > 0).all()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------
def _raw(d, hist, S=1, N=2, KTa=5, used=(5,), smp0=0, ns_alloc=4, arrays=(1, 1, 1), vmax=2.0, amax=1.0, Ts=0.01):
    f = lambda a: None if a is None else mp._lib._dp(np.ascontiguousarray(a, dtype=np.float64))
    out = [np.zeros((max(S, 1), max(N, 1), max(ns_alloc, 1), 3)) if on else None for on in arrays]
    pkv = [np.zeros((max(S, 1), max(N, 1))) for _ in range(2)]
    smp = [np.zeros((max(S, 1), max(N, 1)), dtype=np.int32) for _ in range(2)]
    return d._L.dmpc_postcheck_setpoints(d._ctx, S, N, KTa, mp._lib._ip(np.array(used, dtype=np.int32)) if used is not None else None, None, *(f(h) for h in hist),
                                         vmax, amax, Ts, smp0, ns_alloc, *(f(o) for o in out), f(pkv[0]), mp._lib._ip(smp[0]), f(pkv[1]), mp._lib._ip(smp[1]),
                                         None, None, None)


def test_bad_arguments_are_refused_by_name_and_launch_nothing():
    d = mp.Dmpc("bound", **sp.KW)
    n0 = d.solve_count
    rng = np.random.default_rng(2)
    h = tuple(x[None] for x in sp.random_hist(rng, 2, 5, 5))
    cases = ((dict(smp0=-1), "smp0"), (dict(ns_alloc=-1, arrays=(0, 0, 0)), "ns_alloc"), (dict(ns_alloc=0), "ns_alloc > 0"),
             (dict(ns_alloc=0, arrays=(0, 1, 0)), "ns_alloc > 0"), (dict(ns_alloc=4, arrays=(0, 0, 0)), "needs p_sp"),
             (dict(hist=(h[0], None, h[2])), "pk, vk, ak"), (dict(hist=(None, None, h[2])), "pk, vk, ak"), (dict(hist=(None, h[1], None)), "pk, vk, ak"),
             # what pc_prepare refuses
             (dict(S=0), "bad arguments"), (dict(N=0), "bad arguments"), (dict(KTa=1), "bad arguments"), (dict(used=None), "bad arguments"),
             (dict(vmax=0.0), "bad arguments"), (dict(amax=-1.0), "bad arguments"), (dict(Ts=0.0), "bad arguments"), (dict(Ts=np.nan), "bad arguments"),
             (dict(used=(1,)), "K_T_used out of range"), (dict(used=(6,)), "K_T_used out of range"),
             (dict(hist=tuple(np.zeros_like(x) for x in h)), "degenerate r_factor"))
    for args, word in cases:
        a = dict(hist=h); a.update(args)
        rc = _raw(d, a.pop("hist"), **a)
        assert rc == -1 and _err(d).startswith("dmpc_postcheck_setpoints: ") and word in _err(d), (args, _err(d))
    assert d.solve_count == n0
    with pytest.raises(mp.DmpcError, match="dmpc_postcheck_setpoints: no resident histories"):
        d.setpoints([5], N=2, KT_alloc=5)
    assert mp._lib.load().dmpc_postcheck_setpoints(None, *([0] * 3), None, None, None, None, None, 2.0, 1.0, 0.01, 0, 0, *([None] * 10)) == -1
    assert mp._lib.load().dmpc_last_error(None).decode().startswith("dmpc_postcheck_setpoints: ")
    # a good call after the refused ones
    assert _raw(d, h) == 0, _err(d)
    out = d.setpoints([5], pk=h[0], vk=h[1], ak=h[2])
    _vs_restatement(out, 0, sp.restate(h[0][0], h[1][0], h[2][0]), "after the refusals")


# ---- 9. to the file the vehicles fly -------------------------------------------------------------------------------------------------------------
def test_round_trip_through_trajectories2file(ragged, tmp_path):
    used, (P, V, A), full = ragged["used"], ragged["hist"], ragged["full"]
    s = 1
    n = int(full["n_samples"][s])
    p, v, a = (np.ascontiguousarray(full[k][s][:, :n]) for k in SETPOINTS)
    po, pf = P[s][:, 0], P[s][:, used[s] - 1]
    f = tmp_path / "trajectories.txt"
    resultio.write_trajectories(f, po, pf, p, v, a, float(full["h_scaled"][s]), sp.KW["pmin"], sp.KW["pmax"])
    back = resultio.read_trajectories(f)
    assert back["N"] == back["N_cmd"] == 7 and back["pk"].shape == p.shape
    for got, want in ((back["pk"], p), (back["vk"], v), (back["ak"], a)):
        assert np.allclose(got, want, rtol=1e-5, atol=0.0)                   # the file's 6 significant digits
