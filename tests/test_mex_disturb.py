"""The MEX gateway's 'transition_disturbed' command (multiagent_planning_amd/matlab/dmpc_mex.cpp) against the ctypes binding of the same calls --
dmpc_set_disturbance, dmpc_transition_cmd, clear -- through the mock MEX runtime of tests/mexharness.py."""
import numpy as np
import pytest

import disturb as di
import mexharness as mh
import obstacles as ob

KT = 14
WIND = np.array([0.1, -0.05, 0.02])
# MATLAB's view of a push: agent (1-based), column (0-based), dp, dv -- one per column of an 8 x n matrix
PUSHES_M = np.array([[8, 4, 0.0, 0.1, 0.0, 0.0, 0.0, 0.1], [1, 2, 0.05, 0.0, 0.0, 0.1, 0.0, 0.0]]).T


def _args(po, pf, *more):
    return [po.T, pf.T, KT, ob.ERROR_TOL] + list(more)


@pytest.mark.gpu
def test_gateway_transition_disturbed_matches_the_c_abi():
    import multiagent_planning_amd as mp
    po, pf = ob.wall_scene(8, 0)
    prm = mh.params("bound", ob.KW)
    pk, vk, ak, used, sst = mh.call("transition_disturbed", prm, _args(po, pf, 2e-3, 1e-2, 5.0, WIND, PUSHES_M), nlhs=5)
    pushes = [di.push(0, int(q[0]) - 1, int(q[1]), dp=q[2:5], dv=q[5:8]) for q in PUSHES_M.T]
    d = mp.Dmpc("bound", **ob.KW)
    ref = d.transition(po[None], pf[None], KT, ob.ERROR_TOL, disturb=dict(noise_p=2e-3, noise_v=1e-2, seed=5, wind=WIND, pushes=pushes))
    assert int(used.ravel()[0]) == int(ref["K_T_used"][0]) and int(sst.ravel()[0]) == int(ref["scene_status"][0])
    for got, want in ((pk, "pk"), (vk, "vk"), (ak, "ak")):
        assert got.shape == (3, KT, 8) and got.transpose(2, 1, 0).tobytes() == ref[want][0].tobytes(), want
    assert not np.array_equal(ref["pk"], d.transition(po[None], pf[None], KT, ob.ERROR_TOL)["pk"])
    # nothing to add: 'transition'
    plain = mh.call("transition", prm, _args(po, pf), nlhs=5)
    zero = mh.call("transition_disturbed", prm, _args(po, pf, 0.0, 0.0, 0.0, np.zeros((0, 0)), np.zeros((0, 0))), nlhs=5)
    for a, b in zip(plain, zero):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_gateway_transition_disturbed_refuses_bad_arguments_like_matlab():
    po, pf = ob.wall_scene(8, 0)
    prm = mh.params("bound", ob.KW)
    none = np.zeros((0, 0))
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("transition_disturbed", prm, _args(po, pf, 0.0, 0.0, 0.0, np.array([1.0, 2.0]), none), nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("transition_disturbed", prm, _args(po, pf, 0.0, 0.0, 0.0, none, np.zeros((9, 2))), nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("transition_disturbed", prm, _args(po, pf, 0.0, 0.0, 0.0, none), nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:transition_disturbed.*dmpc_set_disturbance: "):
        mh.call("transition_disturbed", prm, _args(po, pf, -1.0, 0.0, 0.0, none, none), nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:transition_disturbed.*dmpc_transition_cmd: .*push"):
        mh.call("transition_disturbed", prm, _args(po, pf, 0.0, 0.0, 0.0, none, np.array([[9, 4, 0, 0, 0, 0, 0, 0.0]]).T), nlhs=5)
