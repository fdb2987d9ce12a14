"""The MEX gateway's 'plan' command (multiagent_planning_amd/matlab/dmpc_mex.cpp) against the ctypes binding of the same entry,
dmpc_plan_routes, through the mock MEX runtime of tests/mexharness.py."""
import numpy as np
import pytest

import mexharness as mh
import plan as pl
from obstacles import KW


@pytest.mark.gpu
def test_gateway_plan_matches_the_c_abi():
    import multiagent_planning_amd as mp
    s = pl.wall()
    d = mp.Dmpc("bound", **KW)
    ref = d.plan(s["po"], s["goals"], 0.25, 0.2, W=4)
    wp, n_wp, st, hops = mh.call("plan", mh.params("bound", KW), [s["po"].T, s["goals"].T, 0.25, 0.2, 4], nlhs=4)
    assert wp.shape == (3, 4, 3) and np.array_equal(wp.transpose(2, 1, 0), ref["waypoints"])      # 3 x W x N_cmd, MATLAB's column-major
    for got, key in ((n_wp, "n_wp"), (st, "plan_status"), (hops, "hops")):
        assert got.shape == (1, 3) and np.array_equal(got.ravel().astype(np.int32), ref[key]), key
    assert ref["n_wp"].tolist() == [3, 3, 3]
    # the gateway's defaults are the binding's (margin 0, W 4); further obstacle points go behind po's
    extra = np.array([(0.0, 1.6, 1.2), (0.0, -1.6, 1.2)])
    wp2, n2 = mh.call("plan", mh.params("bound", KW), [s["po"].T, s["goals"].T, 0.25, [], [], extra.T], nlhs=2)
    ref2 = d.plan(s["po"], s["goals"], 0.25, obstacles=extra)
    assert np.array_equal(wp2.transpose(2, 1, 0), ref2["waypoints"]) and np.array_equal(n2.ravel().astype(np.int32), ref2["n_wp"])
    assert not np.array_equal(ref2["waypoints"], d.plan(s["po"], s["goals"], 0.25)["waypoints"])
    # ... and what comes back is what 'route' takes
    out = mh.call("route", mh.params("bound", KW), [s["po"].T, wp, s["K_T_max"], s["error_tol"], s["capture"], n_wp], nlhs=5)
    assert int(out[4].ravel()[0]) == (mp.ST_SOLVED | mp.ST_REACHED)


@pytest.mark.gpu
def test_gateway_plan_refuses_bad_shapes_and_passes_the_library_s_refusals_on():
    s = pl.wall()
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("plan", mh.params("bound", KW), [s["po"][:2].T, s["goals"].T, 0.25], nlhs=4)          # more goals than vehicles
    with pytest.raises(RuntimeError, match="dmpc:shape"):
        mh.call("plan", mh.params("bound", KW), [s["po"].T, s["goals"].T, 0.25, 0.0, 0], nlhs=4)
    with pytest.raises(RuntimeError, match="dmpc:plan.*dmpc_plan_routes: .*cell"):
        mh.call("plan", mh.params("bound", KW), [s["po"].T, s["goals"].T, 0.0], nlhs=4)
    with pytest.raises(RuntimeError, match="dmpc:plan.*dmpc_plan_routes: .*cells"):
        mh.call("plan", mh.params("bound", KW), [s["po"].T, s["goals"].T, 0.05], nlhs=4)
