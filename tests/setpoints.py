"""Test helper: the CPU restatement of the flight setpoints and the limits report (dmpc_postcheck_setpoints), and the scenes its tests use.

The reference splines the three rescaled histories of a finished transition independently (dmpc_soft_bound.m:165-169):
    p = spline(tk, pk, t);  v = spline(tk, vk, t);  a = spline(tk, ak, t)
restate() takes the rescaled pk, vk, ak, h_scaled and the sample times from oracle.postcheck.postcheck (failure_rate.m:136-162, the last
acceleration column left un-multiplied as the reference's loop leaves it) and applies scipy's not-a-knot CubicSpline -- the interpolant
tests/test_oracle_golden.py pins to MATLAB's recorded p -- to each of the three; then norms, peaks and the first sample of each peak.
"""
import numpy as np
from scipy.interpolate import CubicSpline

from oracle import postcheck as PC

KW = dict(h=0.2, rmin=0.35, c=2.0, alim=1.0, Q1=1000.0, S1=100.0, term=-5e4, pmin=(-2.5, -2.5, 0.2), pmax=(2.5, 2.5, 2.2))
ULPS = 8          # device norm sqrt(fma(z, z, fma(y, y, x * x))) against numpy's three roundings (the bar of tests/clearance.py)
TOL = 1e-10       # v, a against the restatement: the bar tests/test_gpu_postcheck.py::_check sets for p against the same scipy spline


def spline(tk, y, t, nu=0):
    """MATLAB spline(tk, y, t) per agent, y [N,KT,3] -> [N,ns,3] (nu: derivative order); two or three knots: the line / parabola"""
    return np.stack([CubicSpline(tk, y[i], axis=0, bc_type="not-a-knot")(t, nu) for i in range(y.shape[0])])


def norms(x):
    return np.sqrt((x ** 2).sum(-1))


def restate(pk, vk, ak, h=KW["h"], vmax=2.0, amax=1.0, Ts=0.01, scale_last=False):
    """one scene, un-rescaled pk, vk, ak [N,KT,3] -> dict(p, v, a [N,ns,3], v_norm, a_norm [N,ns], v_peak, v_peak_sample, a_peak, a_peak_sample
    [N], r_factor, h_scaled, n_samples, tk, t, pk, vk, ak (rescaled)).  scale_last: ALSO multiply the last acceleration column by r_factor --
    what the reference does not do (tests/test_setpoints_cpu.py shows that the difference is visible)."""
    pk, vk, ak = (np.asarray(x, dtype=float) for x in (pk, vk, ak))
    ref = PC.postcheck(pk, vk, ak, pk[:, -1], h, KW["rmin"], KW["c"], vmax, amax, Ts, pairs="tree")
    tk, t = PC.sample_times(pk.shape[1], ref["h_scaled"], Ts)
    assert len(t) == ref["n_samples"]
    ak2 = ref["ak"].copy()
    if scale_last:
        ak2[:, -1] *= ref["r_factor"]
    out = dict(p=spline(tk, ref["pk"], t), v=spline(tk, ref["vk"], t), a=spline(tk, ak2, t), tk=tk, t=t, pk=ref["pk"], vk=ref["vk"], ak=ak2,
               r_factor=ref["r_factor"], h_scaled=ref["h_scaled"], n_samples=ref["n_samples"])
    out["v_norm"], out["a_norm"] = norms(out["v"]), norms(out["a"])
    for k in "va":
        out[k + "_peak"] = out[k + "_norm"].max(axis=1)
        out[k + "_peak_sample"] = out[k + "_norm"].argmax(axis=1)      # (numpy: the first of equal maxima)
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
def random_hist(rng, N, KT, KTa):
    """N agents, KT recorded columns of KTa: random accelerations integrated with the MPC model (the histories of
    tests/test_gpu_postcheck.py::test_postcheck_ragged_scenes_vs_oracle)"""
    a = np.zeros((N, KTa, 3)); v = np.zeros_like(a); p = np.zeros_like(a)
    a[:, :KT] = rng.uniform(-1, 1, (N, KT, 3)) * rng.uniform(0.2, 1.0)
    a[:, 0] = 0
    p[:, 0] = rng.uniform(-2, 2, (N, 3))
    for k in range(1, KT):
        v[:, k] = v[:, k - 1] + 0.2 * a[:, k]
        p[:, k] = p[:, k - 1] + 0.2 * v[:, k - 1] + 0.02 * a[:, k]
    return p, v, a


RAGGED_USED = np.array([40, 23, 4, 31, 12, 2, 3], dtype=np.int32)
RAGGED_N, RAGGED_KTA = 7, 40


def ragged_batch():
    """S = 7 scenes of 7 agents in KT_alloc = 40: the five column counts of test_postcheck_ragged_scenes_vs_oracle and the two degenerate
    splines, K_T_used = 2 (line) and 3 (parabola).  Returns (K_T_used, pk, vk, ak [7,7,40,3])."""
    rng = np.random.default_rng(5)
    S = len(RAGGED_USED)
    P, V, A = (np.zeros((S, RAGGED_N, RAGGED_KTA, 3)) for _ in range(3))
    for s in range(S):
        P[s], V[s], A[s] = random_hist(rng, RAGGED_N, int(RAGGED_USED[s]), RAGGED_KTA)
        if RAGGED_USED[s] == 2:
            A[s][:, 0] = 0.3          # (failure_rate.m rescales a_1 only: keep it away from zero)
    return RAGGED_USED.copy(), P, V, A


TIE_KT = 48


def tie_scene():
    """3 agents, 48 columns.  Agents 0 and 2 coast: zero acceleration and a velocity that is exact in fp64, so rescale and spline leave every
    velocity knot alone, |v| is the same double at EVERY sample and so is |a| = 0: all samples tie, sample 0 must win -- inside a wave, between
    the waves of a workgroup, between chunks and between launches.  Agent 1 moves at random and sets r_factor.  Returns (pk, vk, ak [3,48,3])."""
    rng = np.random.default_rng(12)
    p, v, a = random_hist(rng, 3, TIE_KT, TIE_KT)
    for i, vel in ((0, (0.5, 0.0, 0.0)), (2, (0.25, -0.5, 0.125))):
        a[i] = 0.0
        v[i] = vel
        for k in range(1, TIE_KT):
            p[i, k] = p[i, k - 1] + 0.2 * v[i, k - 1]
    return p, v, a


WIDE_N, WIDE_KT = 300, 12


def wide_scene():
    """300 agents (more than four 64-agent tiles), 12 columns.  Agents 0 and 150 share the one history with the largest acceleration and velocity,
    so the scene and its halves [0,150), [150,300) have the same r_factor and every agent the same setpoints in either.  (pk, vk, ak [300,12,3])"""
    rng = np.random.default_rng(300)
    p, v, a = random_hist(rng, WIDE_N, WIDE_KT, WIDE_KT)
    big = np.zeros((WIDE_KT, 3)); big[1:] = rng.uniform(-1, 1, (WIDE_KT - 1, 3)) * 1.5; big[1] = (1.8, -1.7, 1.75)
    for i in (0, 150):
        a[i] = big
        for k in range(1, WIDE_KT):
            v[i, k] = v[i, k - 1] + 0.2 * a[i, k]
            p[i, k] = p[i, k - 1] + 0.2 * v[i, k - 1] + 0.02 * a[i, k]
    return p, v, a
