"""CPU: the entries for uncommanded vehicles (N_cmd < N; ABI revision 8) without a device -- they are declared and exported, refuse a NULL
context by name, and the binding's shape rule (N_cmd = the agents of pf, the reference's _pf.cols()) refuses more goals than vehicles.
The argument checks proper need a context, hence a device: tests/test_gpu_obstacles.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from multiagent_planning_amd import _lib
from helpers import ROOT

CMD_ENTRIES = ["dmpc_step_batch_cmd", "dmpc_step_device_cmd", "dmpc_transition_cmd", "dmpc_postcheck_cmd"]


def test_cmd_entries_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmpc_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name in CMD_ENTRIES:
        assert re.search(r"DMPC_API int " + name + r"\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert re.search(r"#define DMPC_ABI_VERSION 8\b", hdr) and _lib.ABI_VERSION == 8 and L.dmpc_abi_version() == 8
    # no sharded / RCCL form in this revision, and the header says so
    assert not re.findall(r"dmpc_[a-z_]*sharded[a-z_]*_cmd", hdr)
    assert "NO *_cmd form" in open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()


def test_null_context_is_refused_by_name():
    L = _lib.load()
    nd, ni = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
    calls = {
        "dmpc_step_batch_cmd": lambda: L.dmpc_step_batch_cmd(None, 1, 4, 2, nd, nd, nd, nd, nd, nd, nd, nd, ni, ni),
        "dmpc_step_device_cmd": lambda: L.dmpc_step_device_cmd(None, 1, 4, 2, *([None] * 12)),
        "dmpc_transition_cmd": lambda: L.dmpc_transition_cmd(None, 1, 4, 2, nd, nd, 10, 0.01, nd, nd, nd, ni, ni),
        "dmpc_postcheck_cmd": lambda: L.dmpc_postcheck_cmd(None, 1, 4, 2, 10, ni, ni, nd, nd, nd, nd, nd, 2.0, 1.0, 0.01, nd, nd, ni, nd, ni, nd, nd, nd, 0, nd, ni),
    }
    assert sorted(calls) == sorted(CMD_ENTRIES)
    for name, fn in calls.items():
        assert fn() == -1
        assert name + ":" in L.dmpc_last_error(None).decode(), (name, L.dmpc_last_error(None))


def test_shape_rule_of_the_binding():
    """N = agents of the table / po, N_cmd = agents of pf; as many goals as vehicles: every vehicle commanded (the existing entries)"""
    pf = lambda *shape: np.zeros(shape + (3,))
    assert _lib._n_cmd((18,), pf(8), "t") == (1, 18, 8, (8,))
    assert _lib._n_cmd((4, 18), pf(4, 8), "t") == (4, 18, 8, (4, 8))
    assert _lib._n_cmd((4, 18), pf(4, 18), "t") == (4, 18, 18, (4, 18))
    assert _lib._n_cmd((18,), pf(1, 18), "t") == (1, 18, 18, (18,))            # (same size, another shape: taken as before this revision)
    with pytest.raises(_lib.DmpcError, match="pf has 19 agents, the table 18"):
        _lib._n_cmd((18,), pf(19), "t")
    with pytest.raises(_lib.DmpcError, match="pf has 20 agents"):
        _lib._n_cmd((4, 18), pf(4, 20), "t")
    with pytest.raises(_lib.DmpcError, match="does not batch"):
        _lib._n_cmd((4, 18), pf(3, 8), "t")
    with pytest.raises(_lib.DmpcError, match="does not batch"):
        _lib._n_cmd((4, 18), pf(8), "t")


def test_wall_scene_lies_inside_the_reference_workspace():
    import obstacles as ob
    po, pf = ob.wall_scene(8, 0)
    lo, hi = np.array(ob.KW["pmin"]), np.array(ob.KW["pmax"])
    assert po.shape == (18, 3) and pf.shape == (8, 3)
    assert (po >= lo).all() and (po <= hi).all() and (pf >= lo).all() and (pf <= hi).all()
    e1 = np.array([1, 1, 1 / ob.KW["c"]])
    for pts in (po, np.vstack([pf, po[8:]])):          # starts and resting places further apart than rmin (ellipsoidal norm)
        d = np.sqrt((((pts[:, None] - pts[None]) * e1) ** 2).sum(-1)) + 10 * np.eye(len(pts))
        assert d.min() > ob.KW["rmin"]
