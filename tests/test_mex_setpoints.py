"""The MEX gateway's 'setpoints' command (multiagent_planning_amd/matlab/dmpc_mex.cpp) against the ctypes binding of the same entry,
dmpc_postcheck_setpoints, through the mock MEX runtime of tests/mexharness.py."""
import numpy as np
import pytest

import mexharness as mh
import setpoints as sp


def _trial():
    used, P, V, A = sp.ragged_batch()
    n = int(used[4])                                                          # 12 knots, 7 agents
    return P[4][:, :n], V[4][:, :n], A[4][:, :n]


@pytest.mark.gpu
def test_gateway_setpoints_match_the_binding_and_count_samples_from_one():
    import multiagent_planning_amd as mp
    pk, vk, ak = _trial()
    m = lambda x: x.transpose(2, 1, 0)                                        # MATLAB pk(3,KT,N)
    prm = mh.params("bound", sp.KW)
    d = mp.Dmpc("bound", **sp.KW)
    full = d.setpoints([pk.shape[1]], pk=pk, vk=vk, ak=ak)
    ns = int(full["n_samples"][0])
    for margs, first, count in (([], 0, ns), ([41], 40, ns - 40), ([41, 25], 40, 25), ([ns - 2, 10], ns - 3, 10)):
        ref = full if not margs else d.setpoints([pk.shape[1]], pk=pk, vk=vk, ak=ak, first=first, count=count)
        p, v, a, peaks = mh.call("setpoints", prm, [m(pk), m(vk), m(ak), 2.0, 1.0, 0.01] + margs, nlhs=4)
        for got, k in ((p, "p"), (v, "v"), (a, "a")):
            assert got.shape == (3, count, 7) and got.transpose(2, 1, 0).tobytes() == ref[k][0].tobytes(), (margs, k)
        assert peaks.shape == (4, 7)
        assert peaks[0].tobytes() == full["v_peak"][0].tobytes() and peaks[2].tobytes() == full["a_peak"][0].tobytes()
        assert np.array_equal(peaks[1], full["v_peak_sample"][0] + 1.0) and np.array_equal(peaks[3], full["a_peak_sample"][0] + 1.0)   # 1-based
        assert (peaks[1] >= 1).all() and (peaks[1] <= ns).all()


@pytest.mark.gpu
def test_gateway_setpoints_refuses_wrong_arguments_like_matlab():
    pk, vk, ak = _trial()
    m = lambda x: x.transpose(2, 1, 0)
    prm = mh.params("bound", sp.KW)
    for args in ([m(pk), m(vk), m(ak), 2.0, 1.0], [m(pk), m(vk), m(ak), 2.0, 1.0, 0.01, 1, 5, 7]):                # too few, too many
        with pytest.raises(RuntimeError, match="dmpc:shape.*setpoints: "):
            mh.call("setpoints", prm, args, nlhs=4)
    with pytest.raises(RuntimeError, match="dmpc:shape.*vk, ak must match pk"):
        mh.call("setpoints", prm, [m(pk), m(vk)[:, :5], m(ak), 2.0, 1.0, 0.01], nlhs=4)
    with pytest.raises(RuntimeError, match="dmpc:shape.*first"):
        mh.call("setpoints", prm, [m(pk), m(vk), m(ak), 2.0, 1.0, 0.01, 0], nlhs=4)                                 # samples count from one
    with pytest.raises(RuntimeError, match="dmpc:shape.*count"):
        mh.call("setpoints", prm, [m(pk), m(vk), m(ak), 2.0, 1.0, 0.01, 1, 0], nlhs=4)
    with pytest.raises(RuntimeError, match="dmpc:setpoints.*dmpc_postcheck_setpoints: "):
        mh.call("setpoints", prm, [m(pk), m(vk), m(ak), 2.0, -1.0, 0.01], nlhs=4)
