"""CPU: the inputs of tests/test_gpu_setpoints.py can tell a right implementation of dmpc_postcheck_setpoints from the wrong ones that
suggest themselves -- on the restatement (tests/setpoints.py), without the library."""
import os

import numpy as np

import setpoints as sp
from helpers import GOLD, unrescale


def _golden():
    g = np.load(os.path.join(GOLD, "postcheck_comp_kctr_2.npz"))
    p, v, a = unrescale(g)
    return g, sp.restate(p, v, a, float(g["h"]), float(g["vmax"]), float(g["amax"]), float(g["Ts"]))


def test_recorded_transition_exceeds_amax_between_the_knots():
    """the recorded MATLAB block (20 agents, 67 knots, 1 584 samples, amax = 1): the rescale holds the limits at the knots, the spline of the
    accelerations does not -- one agent, index 2, at sample 143 with 1.0044; nobody exceeds vmax"""
    g, r = _golden()
    amax, vmax = float(g["amax"]), float(g["vmax"])
    assert r["p"].shape == (20, 1584, 3) and r["pk"].shape == (20, 67, 3) and r["n_samples"] == int(g["n_samples"])
    assert np.abs(r["p"][:, g["p_idx"]] - g["p"]).max() < 1e-11                       # (the restatement's p is MATLAB's)
    assert sp.norms(r["ak"]).max() <= amax * (1 + 4e-16) and sp.norms(r["vk"]).max() <= vmax
    over = np.where(r["a_peak"] > amax)[0]
    print("a_peak", r["a_peak"].max(), "agent", over, "sample", r["a_peak_sample"][over], "v_peak", r["v_peak"].max(), "knots", sp.norms(r["vk"]).max())
    assert list(over) == [2] and int(r["a_peak_sample"][2]) == 143 and abs(r["a_peak"][2] - 1.0044) < 5e-5
    assert not (r["v_peak"] > vmax).any() and abs(r["v_peak"].max() - 0.68944) < 5e-6 and abs(sp.norms(r["vk"]).max() - 0.68871) < 5e-6


def test_velocity_spline_is_not_the_derivative_of_the_position_spline():
    """the reference interpolates three series independently: an implementation that differentiates the position spline (and that one again
    for a) is off by far more than the GPU tolerance, on the recorded block and on every random scene of the ragged batch with a real spline"""
    g, r = _golden()
    d = np.abs(sp.spline(r["tk"], r["pk"], r["t"], 1) - r["v"]).max()
    print("golden: |d/dt spline(pk) - spline(vk)| max", d)
    assert 5.2e-2 < d < 5.4e-2
    used, P, V, A = sp.ragged_batch()
    for s in range(len(used)):
        n = int(used[s])
        r = sp.restate(P[s][:, :n], V[s][:, :n], A[s][:, :n])
        if n < 4:
            continue
        dv = np.abs(sp.spline(r["tk"], r["pk"], r["t"], 1) - r["v"]).max()
        da = np.abs(sp.spline(r["tk"], r["pk"], r["t"], 2) - r["a"]).max()
        print(f"scene {s} ({n} knots): dv {dv:.3e}, da {da:.3e}")
        assert dv > 1e-3 and da > 1e-3


def test_tie_scene_has_samples_that_share_the_peak_to_the_bit():
    p, v, a = sp.tie_scene()
    r = sp.restate(p, v, a)
    assert r["n_samples"] > 2 * 256                                                   # (several chunks of the device kernel)
    for i, vel in ((0, 0.5), (2, np.sqrt(0.25 ** 2 + 0.5 ** 2 + 0.125 ** 2))):
        assert (r["v_norm"][i] == r["v_norm"][i][0]).all() and r["v_norm"][i][0] == vel and r["v_peak_sample"][i] == 0
        assert (r["a_norm"][i] == 0.0).all() and r["a_peak_sample"][i] == 0
        assert (r["vk"][i] == v[i]).all()                                             # exact knots: the device's spline is flat too
    assert r["v_peak_sample"][1] > 0 and r["a_peak_sample"][1] > 0 and r["r_factor"] != 1.0


def test_last_acceleration_column_is_visible():
    """failure_rate.m:156-162 multiplies a_1 .. a_{K-1} by r_factor and leaves a_K alone; an implementation that repairs this differs near the
    end of the trajectory by far more than the GPU tolerance"""
    used, P, V, A = sp.ragged_batch()
    for s in range(len(used)):
        n = int(used[s])
        r = sp.restate(P[s][:, :n], V[s][:, :n], A[s][:, :n])
        q = sp.restate(P[s][:, :n], V[s][:, :n], A[s][:, :n], scale_last=True)
        tail = r["t"] > r["tk"][-2]
        d = np.abs(r["a"] - q["a"])
        print(f"scene {s}: r_factor {r['r_factor']:.4f}, |a - a_repaired| max {d.max():.3e} (tail {d[:, tail].max():.3e})")
        assert d[:, tail].max() > 1e3 * sp.TOL and np.array_equal(r["p"], q["p"]) and np.array_equal(r["v"], q["v"])


def test_wide_scene_halves_share_r_factor():
    p, v, a = sp.wide_scene()
    whole = sp.restate(p, v, a)
    for lo in (0, 150):
        half = sp.restate(p[lo:lo + 150], v[lo:lo + 150], a[lo:lo + 150])
        assert half["r_factor"] == whole["r_factor"] and half["n_samples"] == whole["n_samples"]
    assert whole["n_samples"] > 256
