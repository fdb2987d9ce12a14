"""CPU: the disturbance rule on the host -- dmpc_disturbance_sample (no context, no GPU) against the numpy restatement of tests/disturb.py, byte
for byte, and the descriptor's refusals.  The GPU side (tests/test_gpu_disturb.py) compares the device with the same restatement."""
import ctypes as C

import numpy as np
import pytest

import disturb as di
from multiagent_planning_amd import _lib

H = 0.2
WIND1 = np.array([0.3, -0.2, 0.05])


def _pushes(S, n):
    """two pushes on one (scene, agent, column), given out of order relative to other agents; one on a column that is never sampled"""
    s1, a1 = S - 1, n - 1
    return np.array([
        di.push(s1, a1, 2, dp=(0.01, 0.02, -0.03), dv=(0.1, 0.0, -0.1)),
        di.push(0, 0, 1, dp=(0.1, 0.0, 0.0)),
        di.push(0, 0, 39, dv=(0.0, 0.2, 0.0)),
        di.push(s1, a1, 2, dp=(1e-17, 0.3, 0.03), dv=(-0.1, 1e-3, 0.1)),
        di.push(0, n // 2, 2, dp=(0.0, -0.05, 0.0), dv=(0.01, 0.01, 0.01)),
        di.push(0, 0, 17, dp=(9.0, 9.0, 9.0)),
        di.push(s1, 0, 1, dp=(0.0, 0.0, 0.07)),
    ])


def _cases(S, n):
    wS = np.arange(3 * S, dtype=np.float64).reshape(S, 3) * 0.1 - 0.25
    return {
        "wind, every scene": dict(wind=WIND1),
        "wind per scene": dict(wind=wS),
        "noise": dict(noise_p=2e-3, noise_v=1e-2, seed=7),
        "pushes": dict(pushes=_pushes(S, n)),
        "all": dict(wind=wS, noise_p=3e-3, noise_v=2e-2, seed=(1 << 63) + 12345, pushes=_pushes(S, n)),
    }


@pytest.mark.parametrize("S,n", [(1, 1), (2, 3), (2, 65)])
def test_sample_equals_the_restatement_byte_for_byte(S, n):
    for name, kw in _cases(S, n).items():
        for k in (1, 2, 39):
            dp, dv = _lib.disturbance_sample(H, S, n, k, **kw)
            rp, rv = di.sample(H, S, n, k, **kw)
            assert dp.tobytes() == rp.tobytes() and dv.tobytes() == rv.tobytes(), (name, k)
        dp, dv = _lib.disturbance_sample(H, S, n, 0, **kw)
        assert not dp.any() and not dv.any(), name   # column 0 is never disturbed
    # what the cases are meant to exercise does show: the two pushes on one key add up in list order, noise differs between agents and columns
    dp, _ = _lib.disturbance_sample(H, S, n, 2, pushes=_pushes(S, n))
    assert dp[S - 1, n - 1, 1] == (0.0 + 0.02) + 0.3 or (S, n) == (1, 1)
    a, _ = _lib.disturbance_sample(H, S, n, 1, noise_p=1.0, seed=3)
    b, _ = _lib.disturbance_sample(H, S, n, 2, noise_p=1.0, seed=3)
    assert (np.abs(a) < 1.0).all() and not np.array_equal(a, b) and len(np.unique(a)) == a.size


def test_position_noise_off_leaves_exactly_the_wind_term():
    dp, dv = _lib.disturbance_sample(H, 2, 5, 3, wind=WIND1, noise_p=0.0, noise_v=0.5, seed=1)
    want = np.array([((0.5 * H) * H) * w for w in WIND1])
    assert np.array_equal(dp, np.broadcast_to(want, dp.shape))
    assert not np.array_equal(dv, np.broadcast_to(H * WIND1, dv.shape))
    # a seed alone draws nothing
    dp, dv = _lib.disturbance_sample(H, 2, 5, 3, seed=9)
    assert not dp.any() and not dv.any()


def _raw(d, S=2, n=3, k=1, h=H):
    L = _lib.load()
    dp, dv = np.zeros((S, n, 3)), np.zeros((S, n, 3))
    rc = L.dmpc_disturbance_sample(C.byref(d), h, S, n, k, _lib._dp(dp), _lib._dp(dv))
    return rc, L.dmpc_last_error(None).decode()


def test_descriptor_refusals():
    bad = [dict(noise_p=-1e-3), dict(noise_v=-1.0), dict(noise_p=float("nan")), dict(noise_v=float("inf")),
           dict(wind=[0.0, float("nan"), 0.0]), dict(wind=[[0.0, 0.0, 0.0], [float("inf"), 0.0, 0.0]]),
           dict(pushes=[di.push(0, 0, 1, dp=(float("nan"), 0, 0))]), dict(pushes=[di.push(0, 0, 1, dv=(0, 0, float("-inf")))]),
           dict(pushes=[di.push(-1, 0, 1)]), dict(pushes=[di.push(0, -1, 1)]), dict(pushes=[di.push(0, 0, 0)]),
           # the shape of the call
           dict(wind=np.zeros((3, 3))), dict(pushes=[di.push(2, 0, 1)]), dict(pushes=[di.push(0, 3, 1)])]
    for kw in bad:
        with pytest.raises(_lib.DmpcError, match="^dmpc_disturbance_sample: "):
            _lib.disturbance_sample(H, 2, 3, 1, **kw)
    # counts and NULL arrays, which the Python layer cannot express
    for field, val in (("n_push", -1), ("wind_scenes", -1), ("n_push", 1), ("wind_scenes", 1)):
        d, _ = _lib._disturbance()
        setattr(d, field, val)
        rc, msg = _raw(d)
        assert rc == -1 and msg.startswith("dmpc_disturbance_sample: "), (field, val, msg)
    d, _ = _lib._disturbance(noise_p=1e-3)
    assert _raw(d, k=-1)[0] == -1 and _raw(d, S=0)[0] == -1 and _raw(d, n=0)[0] == -1 and _raw(d)[0] == 0
    # a push on a far column is legal
    _lib.disturbance_sample(H, 2, 3, 1, pushes=[di.push(1, 2, 10 ** 6)])
    # the Python layer's own shape checks
    for kw in (dict(wind=[1.0, 2.0]), dict(pushes=np.zeros((2, 8))), dict(pushes=[di.push(0.5, 0, 1)])):
        with pytest.raises(_lib.DmpcError, match="^disturbance: "):
            _lib.disturbance_sample(H, 2, 3, 1, **kw)
