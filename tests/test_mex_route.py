"""The MEX gateway's 'route' command (multiagent_planning_amd/matlab/dmpc_mex.cpp) against the ctypes binding of the same entry,
dmpc_transition_route, through the mock MEX runtime of tests/mexharness.py."""
import numpy as np
import pytest

import mexharness as mh
import route as rt


def _args(s, *more):
    """MATLAB's view of a scene: po 3 x N, waypoints 3 x W x N_cmd"""
    return [s["po"].T, s["wp"].transpose(2, 1, 0), s["K_T_max"], s["error_tol"], s["capture"]] + list(more)


@pytest.mark.gpu
def test_gateway_route_matches_the_c_abi():
    import multiagent_planning_amd as mp
    s = rt.wall()
    pk, vk, ak, used, sst, col = mh.call("route", mh.params("bound", rt.KW), _args(s, s["n_wp"].astype(float)), nlhs=6)
    ref = mp.Dmpc("bound", **rt.KW).route(s["po"][None], s["wp"][None], s["K_T_max"], s["capture"], n_wp=s["n_wp"][None], error_tol=s["error_tol"])
    assert int(used.ravel()[0]) == int(ref["K_T_used"][0]) and int(sst.ravel()[0]) == int(ref["scene_status"][0]) == (mp.ST_SOLVED | mp.ST_REACHED)
    assert col.shape == (3, 3) and np.array_equal(col.T.astype(np.int32), ref["wp_col"][0]) and (col.T[:, 0] > 0).all() and col.T[2, 1] == -1
    for got, want in ((pk, "pk"), (vk, "vk"), (ak, "ak")):
        assert np.array_equal(got.transpose(2, 1, 0), ref[want][0]), want
    # a timeout in front of the capture radius: every agent leaves its first waypoint on column 5
    col5 = mh.call("route", mh.params("bound", rt.KW), _args(s, s["n_wp"].astype(float), 5.0), nlhs=6)[5]
    assert (col5.T[:, 0] == 5).all()


@pytest.mark.gpu
def test_gateway_route_refuses_bad_arguments_like_matlab():
    s = rt.wall()
    prm = mh.params("bound", rt.KW)
    with pytest.raises(RuntimeError, match="dmpc:route.*dmpc_transition_route: .*n_wp"):
        mh.call("route", prm, _args(s, np.array([3.0, 4.0, 2.0])), nlhs=6)
    with pytest.raises(RuntimeError, match="dmpc:route.*dmpc_transition_route: .*capture"):
        mh.call("route", prm, _args(s)[:4] + [0.0], nlhs=6)
    with pytest.raises(RuntimeError, match="dmpc:route.*dmpc_transition_route: .*timeout"):
        mh.call("route", prm, _args(s, s["n_wp"].astype(float), -1.0), nlhs=6)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("route", prm, _args(s, np.array([3.0, 3.0])), nlhs=6)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("route", prm, _args(s)[:4], nlhs=6)
