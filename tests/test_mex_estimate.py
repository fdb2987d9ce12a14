"""The MEX gateway's 'transition_estimated' command (multiagent_planning_amd/matlab/dmpc_mex.cpp) against the ctypes binding of the same calls --
dmpc_set_feedback, dmpc_set_measurement, dmpc_set_disturbance, dmpc_transition_cmd, dmpc_feedback_log, dmpc_estimate_log, clear all three --
through the mock MEX runtime of tests/mexharness.py."""
import numpy as np
import pytest

import disturb as di
import mexharness as mh
import obstacles as ob

KT = 14
WIND = np.array([0.1, -0.05, 0.02])
# MATLAB's view of a push: agent (1-based), column (0-based), dp, dv -- one per column of an 8 x n matrix
PUSHES_M = np.array([[8, 4, 0.0, 0.1, 0.0, 0.0, 0.0, 0.1], [1, 2, 0.05, 0.0, 0.0, 0.1, 0.0, 0.0]]).T
LOG_ORDER = ("event_count", "event_first", "event_last", "dev_p_max", "dev_p_col", "dev_v_max", "dev_v_col", "xh_p", "xh_v", "e_p", "e_v")
EST_ORDER = ("err_p_max", "err_p_col", "err_v_max", "err_v_col", "dev_p_max", "dev_p_col", "dev_v_max", "dev_v_col", "eh_p", "eh_v")
DIST = (2e-3, 1e-2, 5.0, WIND, PUSHES_M)
MEAS = (0.02, 0.05, 0.5, 1.0, 9.0)   # meas_p, meas_v, gain_p, gain_v, meas_seed


def _args(po, pf, *more):
    return [po.T, pf.T, KT, ob.ERROR_TOL] + list(more)


def test_the_wrapper_names_the_command_and_its_outputs():
    import os
    src = open(os.path.join(mh.ROOT, "multiagent_planning_amd", "matlab", "estimatedTransition.m")).read()
    assert "dmpc_mex('transition_estimated', prm, po, pf, K_T_max, error_tol, trigger_p, trigger_v, reanchor, ..." in src
    assert "noise_p, noise_v, seed, wind, pushes, meas_p, meas_v, gain_p, gain_v, meas_seed);" in src
    order = [src.index("log." + name) for name in LOG_ORDER] + [src.index("est." + name) for name in EST_ORDER]
    assert order == sorted(order)
    gate = open(os.path.join(mh.ROOT, "multiagent_planning_amd", "matlab", "dmpc_mex.cpp")).read()
    assert '"transition_estimated"' in gate and "nrhs == 19" in gate


@pytest.mark.gpu
def test_gateway_transition_estimated_matches_the_c_abi():
    import multiagent_planning_amd as mp
    po, pf = ob.wall_scene(8, 0)
    prm = mh.params("bound", ob.KW)
    out = mh.call("transition_estimated", prm, _args(po, pf, 0.04, 0.2, 1, *DIST, *MEAS), nlhs=26)
    pushes = [di.push(0, int(q[0]) - 1, int(q[1]), dp=q[2:5], dv=q[5:8]) for q in PUSHES_M.T]
    d = mp.Dmpc("bound", **ob.KW).set_feedback(0.04, 0.2).set_measurement(noise_p=0.02, noise_v=0.05, gain_p=0.5, gain_v=1.0, seed=9)
    ref = d.transition(po[None], pf[None], KT, ob.ERROR_TOL, disturb=dict(noise_p=2e-3, noise_v=1e-2, seed=5, wind=WIND, pushes=pushes))
    log, est = d.feedback_log(1, 8), d.estimate_log(1, 8)
    assert int(out[3].ravel()[0]) == int(ref["K_T_used"][0]) and int(out[4].ravel()[0]) == int(ref["scene_status"][0])
    for got, want in zip(out[:3], ("pk", "vk", "ak")):
        assert got.shape == (3, KT, 8) and got.transpose(2, 1, 0).tobytes() == ref[want][0].tobytes(), want
    for outs, rep, names in ((out[5:16], log, LOG_ORDER), (out[16:], est, EST_ORDER)):
        for got, name in zip(outs, names):
            want = rep[name][0]
            assert got.shape == ((3, 8) if want.ndim == 2 else (1, 8)) and np.array_equal(got.T.reshape(want.shape), want.astype(np.float64)), name
    assert log["event_count"].any() and (est["err_p_max"] > 0).all()
    # the command cleared what it set: in one session, the plain 'transition' before and after it, 'transition_feedback' behind it (no measurement
    # left), and no noise with gain 1 is 'transition_feedback'
    fbk = (0.04, 0.2, 1)
    plain, again, feedback, quiet, after = mh.session([("transition", prm, _args(po, pf), 5), ("transition_estimated", prm, _args(po, pf, *fbk, *DIST, *MEAS), 26),
                                                       ("transition_feedback", prm, _args(po, pf, *fbk, *DIST), 16),
                                                       ("transition_estimated", prm, _args(po, pf, *fbk, *DIST, 0.0, 0.0, 1.0, 1.0, 0.0), 16),
                                                       ("transition", prm, _args(po, pf), 5)])
    for a, b in zip(again, out):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(quiet, feedback):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(after, plain):
        assert a.tobytes() == b.tobytes()
    assert feedback[0].tobytes() != again[0].tobytes() and plain[0].tobytes() != feedback[0].tobytes()


@pytest.mark.gpu
def test_gateway_transition_estimated_refuses_bad_arguments_like_matlab():
    po, pf = ob.wall_scene(8, 0)
    prm = mh.params("bound", ob.KW)
    none = np.zeros((0, 0))
    quiet = (0.0, 0.0, 0.0, none, none)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("transition_estimated", prm, _args(po, pf, 0.05, 0.25, 1, 0.0, 0.0, 0.0, np.array([1.0, 2.0]), none, *MEAS), nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("transition_estimated", prm, _args(po, pf, 0.05, 0.25, 1, *quiet), nlhs=5)   # 'transition_feedback's arguments alone
    with pytest.raises(RuntimeError, match="dmpc:transition_estimated.*dmpc_set_feedback: "):
        mh.call("transition_estimated", prm, _args(po, pf, -0.05, 0.25, 1, *quiet, *MEAS), nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:transition_estimated.*dmpc_set_measurement: .*gain_p"):
        mh.call("transition_estimated", prm, _args(po, pf, 0.05, 0.25, 1, *quiet, 0.02, 0.05, 0.0, 1.0, 9.0), nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:transition_estimated.*dmpc_set_measurement: .*amp_v"):
        mh.call("transition_estimated", prm, _args(po, pf, 0.05, 0.25, 1, *quiet, 0.02, -0.05, 1.0, 1.0, 9.0), nlhs=5)
    # a refused disturbance leaves neither a policy nor a measurement behind: the next 'transition' of the session is the plain one
    bad, after = mh.session([("transition_estimated", prm, _args(po, pf, 0.05, 0.25, 1, -1.0, 0.0, 0.0, none, none, *MEAS), 5), ("transition", prm, _args(po, pf), 5)])
    assert isinstance(bad, RuntimeError) and "dmpc_set_disturbance: " in str(bad)
    for a, b in zip(after, mh.call("transition", prm, _args(po, pf), nlhs=5)):
        assert a.tobytes() == b.tobytes()
