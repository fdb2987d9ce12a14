"""The MEX gateway's 'mission' command (multiagent_planning_amd/matlab/dmpc_mex.cpp) against the ctypes binding of the same entry,
dmpc_transition_mission, through the mock MEX runtime of tests/mexharness.py."""
import numpy as np
import pytest

import mexharness as mh
import mission as ms


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deadline", "static"])
def test_gateway_mission_matches_the_c_abi(name):
    import multiagent_planning_amd as mp
    s = ms.scene(name)
    prm = mh.params("bound", ms.KW)
    args = [s["po"].T, s["goals"].transpose(2, 1, 0), ms.KT, ms.ERROR_TOL] + ([s["deadline"].astype(float)] if s["deadline"] is not None else [])
    pk, vk, ak, used, sst, col = mh.call("mission", prm, args, nlhs=6)
    ref = mp.Dmpc("bound", **ms.KW).mission(s["po"][None], s["goals"][None], ms.KT, ms.ERROR_TOL,
                                            deadline=None if s["deadline"] is None else s["deadline"][None])
    assert int(used.ravel()[0]) == int(ref["K_T_used"][0]) and int(sst.ravel()[0]) == int(ref["scene_status"][0]) == (mp.ST_SOLVED | mp.ST_REACHED)
    assert np.array_equal(col.ravel().astype(np.int32), ref["stage_col"][0]) and (col.ravel() > 0).all()
    for got, want in ((pk, "pk"), (vk, "vk"), (ak, "ak")):
        assert np.array_equal(got.transpose(2, 1, 0), ref[want][0]), want


@pytest.mark.gpu
def test_gateway_mission_refuses_bad_deadlines_like_matlab():
    s = ms.scene("deadline")
    with pytest.raises(RuntimeError, match="dmpc:mission.*dmpc_transition_mission: "):
        mh.call("mission", mh.params("bound", ms.KW), [s["po"].T, s["goals"].transpose(2, 1, 0), ms.KT, ms.ERROR_TOL, np.array([8.0, 0.0, 3.0])], nlhs=6)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("mission", mh.params("bound", ms.KW), [s["po"].T, s["goals"].transpose(2, 1, 0), ms.KT, ms.ERROR_TOL, np.array([8.0, 0.0])], nlhs=6)
