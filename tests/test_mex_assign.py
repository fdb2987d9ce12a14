"""The MEX gateway's 'assign' command (multiagent_planning_amd/matlab/dmpc_mex.cpp) against the ctypes binding of the same entry,
dmpc_assign_goals, through the mock MEX runtime of tests/mexharness.py."""
import numpy as np
import pytest

import assign as asg
import mexharness as mh
from obstacles import KW


@pytest.mark.gpu
def test_gateway_assign_matches_the_c_abi():
    import multiagent_planning_amd as mp
    N = 65
    po, g = asg.lattice(N)
    eps = asg.lattice_eps(N)
    assert KW["c"] == asg.C_LATTICE
    perm, pf, cost, rounds = mh.call("assign", mh.params("bound", KW), [po.T, g.T, eps], nlhs=4)
    ref = mp.Dmpc("bound", **KW).assign(po, g, eps=eps)
    assert np.array_equal(perm.ravel().astype(np.int32), ref["perm"] + 1) and ref["perm"].min() == 0
    assert np.array_equal(pf.T, ref["pf"]) and float(cost.ravel()[0]) == float(ref["cost"]) and int(rounds.ravel()[0]) == int(ref["rounds"]) > 0
    # the default eps of the gateway is the binding's
    perm2, = mh.call("assign", mh.params("bound", KW), [po.T, g.T], nlhs=1)
    assert np.array_equal(perm2.ravel().astype(np.int32), mp.Dmpc("bound", **KW).assign(po, g)["perm"] + 1)


@pytest.mark.gpu
def test_gateway_assign_refuses_goals_of_another_shape():
    po, g = asg.lattice(8)
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("assign", mh.params("bound", KW), [po.T, g[:7].T], nlhs=4)
    with pytest.raises(RuntimeError, match="dmpc:assign.*dmpc_assign_goals: "):
        mh.call("assign", mh.params("bound", KW), [po.T, g.T, 0.0], nlhs=4)
