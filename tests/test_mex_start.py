"""The MEX gateway's 'flight_end' and 'transition_from' commands (multiagent_planning_amd/matlab/dmpc_mex.cpp) against the ctypes binding of the
same calls -- dmpc_flight_end; dmpc_set_start, dmpc_transition_cmd -- through the mock MEX runtime of tests/mexharness.py, one session: the
gateway's context lives across the calls, as in MATLAB."""
import numpy as np
import pytest

import mexharness as mh
import obstacles as ob

KT, CUT = 14, 6
NONE = np.zeros((0, 0))


def _m(a):
    """[n,3] or [n,45] rows -> MATLAB's 3 x n / 3 x K x n"""
    return a.T if a.shape[-1] == 3 else a.reshape(a.shape[0], 15, 3).transpose(2, 1, 0)


@pytest.mark.gpu
def test_gateway_flight_end_and_transition_from_match_the_c_abi():
    import multiagent_planning_amd as mp
    po, pf = ob.wall_scene(8, 0)
    prm = mh.params("bound", ob.KW)
    fly = [po.T, pf.T, KT - CUT, ob.ERROR_TOL]
    calls = [("transition", prm, [po.T, pf.T, CUT + 1, ob.ERROR_TOL], 5), ("flight_end", prm, [8], 7),
             ("transition_from", prm, fly + [NONE] * 5 + [0, 1], 5),                                  # carried on the device
             ("transition", prm, [po.T, pf.T, KT, ob.ERROR_TOL], 5)]
    first, end, rest, whole = mh.session(calls)
    d = mp.Dmpc("bound", **ob.KW)
    ref_first = d.transition(po[None], pf[None], CUT + 1, ob.ERROR_TOL)
    ref_end = d.flight_end(1, 8)
    for got, k in zip(end[:6], ("x_p", "x_v", "x_a", "plan_p", "plan_v", "plan_a")):
        assert got.shape == _m(ref_end[k][0]).shape and np.asfortranarray(got).tobytes(order="F") == np.asfortranarray(_m(ref_end[k][0])).tobytes(order="F"), k
    assert int(end[6].ravel()[0]) == CUT == int(ref_end["col"][0])
    d.set_start(from_end=True, S=1, N_cmd=8)
    ref_rest = d.transition(po[None], pf[None], KT - CUT, ob.ERROR_TOL)
    for out, ref, kt in ((first, ref_first, CUT + 1), (rest, ref_rest, KT - CUT)):
        assert int(out[3].ravel()[0]) == int(ref["K_T_used"][0]) and int(out[4].ravel()[0]) == int(ref["scene_status"][0])
        for got, k in zip(out[:3], ("pk", "vk", "ak")):
            assert got.shape == (3, kt, 8) and got.transpose(2, 1, 0).tobytes() == ref[k][0].tobytes(), k
    # the two parts are the whole flight
    assert np.array_equal(rest[0][:, :KT - CUT], whole[0][:, CUT:KT]) and np.array_equal(first[0], whole[0][:, :CUT + 1])
    # the same through the host: what 'flight_end' returned goes into 'transition_from'; and the braking plan where no plan is given
    xp = np.vstack([end[0].T, po[8:]])
    host, brake = mh.session([("transition_from", prm, [xp.T, pf.T, KT - CUT, ob.ERROR_TOL, end[1], end[2], end[3], end[4], end[5], CUT], 5),
                              ("transition_from", prm, [xp.T, pf.T, KT - CUT, ob.ERROR_TOL, end[1], end[2], NONE, NONE, NONE, CUT], 5)])
    for a, b in zip(host, rest):
        assert a.tobytes() == b.tobytes()
    d.set_start(vo=ref_end["x_v"], ao=ref_end["x_a"], col0=CUT)
    ref_brake = d.transition(xp[None], pf[None], KT - CUT, ob.ERROR_TOL)
    assert brake[0].transpose(2, 1, 0).tobytes() == ref_brake["pk"][0].tobytes() and brake[0].tobytes() != rest[0].tobytes()


@pytest.mark.gpu
def test_gateway_start_commands_refuse_bad_arguments_like_matlab():
    po, pf = ob.wall_scene(8, 0)
    prm = mh.params("bound", ob.KW)
    fly = [po.T, pf.T, KT, ob.ERROR_TOL]
    v, p = np.zeros((3, 8)), np.zeros((3, 15, 8))
    for args in (fly + [NONE] * 5, fly + [np.zeros((3, 7)), NONE, NONE, NONE, NONE, 0], fly + [v, v, np.zeros((3, 14, 8)), NONE, NONE, 0],
                 [po.T, pf.T[:, :0], KT, ob.ERROR_TOL] + [NONE] * 5 + [0]):
        with pytest.raises(RuntimeError, match="dmpc:shape"):
            mh.call("transition_from", prm, args, nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("flight_end", prm, [], nlhs=7)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("flight_end", prm, [0], nlhs=7)
    with pytest.raises(RuntimeError, match="dmpc:flight_end.*dmpc_flight_end: the context holds no valid flight end"):
        mh.call("flight_end", prm, [8], nlhs=7)
    with pytest.raises(RuntimeError, match="dmpc:transition_from.*dmpc_set_start: plan_v and plan_a"):
        mh.call("transition_from", prm, fly + [v, v, p, p, NONE, 0], nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:transition_from.*dmpc_set_start: col0"):
        mh.call("transition_from", prm, fly + [v, v, NONE, NONE, NONE, -1], nlhs=5)
    with pytest.raises(RuntimeError, match="dmpc:transition_from.*dmpc_set_start: from_end"):
        mh.call("transition_from", prm, fly + [NONE] * 5 + [0, 1], nlhs=5)
    # a refused start arms nothing: the next 'transition' of the session flies from rest
    r = mh.session([("transition", prm, fly, 5), ("transition_from", prm, fly + [np.full((3, 8), np.inf), NONE, NONE, NONE, NONE, 0], 5),
                    ("transition", prm, fly, 5)])
    assert isinstance(r[1], RuntimeError) and "not finite" in str(r[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(r[0], r[2]))
