"""CPU: the entries for scripted vehicles (uncommanded vehicles that follow a path) without a device -- declared, exported and bound, the
ABI revision still 8, a NULL context refused by name, the binding's argument rules -- and the conditions the test scenes of tests/scripted.py
must meet for the GPU tests (tests/test_gpu_scripted.py) to see a wrong window, checked with the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from multiagent_planning_amd import _lib
from helpers import ROOT
import scripted as sc

ENTRIES = ["dmpc_transition_scripted", "dmpc_scripted_cols_device", "dmpc_postcheck_scripted"]
LOOP_VARIANTS = ["bound", "bound2", "hard", "cpp"]      # tests/test_gpu_obstacles.py


def test_scripted_entries_are_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load()
    for name in ENTRIES:
        assert re.search(r"DMPC_API int " + name + r"\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    # additive: the revision stays 8, and there is still no sharded form
    assert re.search(r"#define DMPC_ABI_VERSION 8\b", hdr) and _lib.ABI_VERSION == 8 and L.dmpc_abi_version() == 8
    assert not re.findall(r"dmpc_[a-z_]*sharded[a-z_]*_(cmd|scripted)", hdr)
    # the header says that the reference has no such thing, and states the window and the clamp
    assert "NO REFERENCE COUNTERPART" in raw and "sample(j, k-1+kk)" in raw and "path[j][min(t, P-1)]" in raw


def test_null_context_is_refused_by_name():
    L = _lib.load()
    nd, ni = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
    calls = {
        "dmpc_transition_scripted": lambda: L.dmpc_transition_scripted(None, 1, 2, 1, 3, nd, nd, nd, 10, 0.01, nd, nd, nd, ni, ni),
        "dmpc_scripted_cols_device": lambda: L.dmpc_scripted_cols_device(None, 1, 3, 2, 3, None, 1, None, None, None),
        "dmpc_postcheck_scripted": lambda: L.dmpc_postcheck_scripted(None, 1, 3, 2, 10, ni, ni, nd, nd, nd, nd, nd, 3, 2.0, 1.0, 0.01, nd, nd, ni, nd, ni, nd, nd,
                                                                     nd, 0, nd, ni, nd),
    }
    assert sorted(calls) == sorted(ENTRIES)
    for name, fn in calls.items():
        assert fn() == -1
        assert name + ":" in L.dmpc_last_error(None).decode(), (name, L.dmpc_last_error(None))


def test_argument_rules_of_the_binding():
    """checked before anything reaches the library (no context needed: the methods are called unbound)"""
    po, pf, path = sc.batch("A")
    with pytest.raises(_lib.DmpcError, match="exclude each other"):
        _lib.Dmpc.postcheck(None, [5], pf, KT_alloc=10, po_static=path[:, :, 0], path=path)
    with pytest.raises(_lib.DmpcError, match="same commanded agents"):
        _lib.Dmpc.transition(None, np.concatenate([po, path[:, :, 0]], axis=1), pf, 10, path=path)      # po of all vehicles: the *_cmd rule, not this one
    with pytest.raises(_lib.DmpcError, match="same commanded agents"):
        _lib.Dmpc.transition(None, po, pf[:, :5], 10, path=path)
    with pytest.raises(_lib.DmpcError, match="does not batch"):
        _lib.Dmpc.transition(None, po, pf, 10, path=path[0])                                             # batched agents, unbatched path
    with pytest.raises(_lib.DmpcError, match="does not batch"):
        _lib.Dmpc.transition(None, po, pf, 10, path=path[:1])
    with pytest.raises(_lib.DmpcError, match="at least one vehicle and one sample"):
        _lib.Dmpc.transition(None, po, pf, 10, path=path[:, :, :0])
    assert _lib._path(path, (2, 8), "t")[1:] == (10, sc.P_A) and _lib._path(path[0], (8,), "t")[1:] == (10, sc.P_A)


def test_scenes_lie_inside_the_workspace_and_move_as_described():
    lo, hi = np.array(sc.KW["pmin"]), np.array(sc.KW["pmax"])
    for variant, P, nc, M in (("A", sc.P_A, 8, 10), ("B", sc.P_B, 8, 10), ("C", sc.P_C, 1, 1)):
        for seed in sc.SEEDS[variant]:
            po, pf, path = sc.scene(variant, seed)
            assert po.shape == pf.shape == (nc, 3) and path.shape == (M, P, 3)
            for pts in (po, pf, path.reshape(-1, 3)):
                assert (pts >= lo).all() and (pts <= hi).all()
            step = np.linalg.norm(np.diff(path, axis=1), axis=-1)
            assert np.allclose(step[:, :11], sc.STEP)                          # 0.1 m per step = 0.5 m/s at h = 0.2
    for v in "AB":                                                             # the wall differs by scene: no two scenes of a batch share a path
        paths = sc.batch(v)[2]
        assert not np.array_equal(paths[0], paths[1])
    mixed = sc.mixed_batch(36)[2]
    assert all(not np.array_equal(mixed[i], mixed[j]) for i in range(36) for j in range(i))
    assert (mixed >= lo).all() and (mixed <= hi).all()
    po, pf, path = sc.scene("A", 0)
    dy = path[:, 1, 1] - path[:, 0, 1]
    assert (dy[:5] > 0).all() and (dy[5:] < 0).all()                           # the two rows in opposite directions
    assert sc.P_A == sc.KT + 13 and sc.P_B == 12                               # A: no window ever reaches the end of the path (k-1+14 <= KT+12)
    assert np.array_equal(sc.window(path, 1)[:, :3], path[:, 0]) and np.array_equal(sc.window(path, 5)[:, 42:], path[:, 18])
    pb = sc.scene("B", 0)[2]
    assert np.array_equal(sc.window(pb, 40), np.tile(pb[:, 11], (1, 15)))      # B: clamped
    assert np.array_equal(sc.pad_path(pb, 20)[:, 12:], np.repeat(pb[:, 11:12], 8, axis=1))


def test_scene_conditions_hold_for_the_oracle():
    """1. with every solver variant of the closed-loop test, at least one scene of each variant ends SOLVED | REACHED;
    2. the motion matters: some agent-step builds another number of rows than with the vehicles frozen at their starts;
    3. the window's start matters: the loop with the window one column late (shift = +1) differs by more than 1e-4 in pk on some scene."""
    cases = [(v, s) for v in "ABC" for s in sc.SEEDS[v]]
    for solver in LOOP_VARIANTS:
        for v in "ABC":
            assert any(sc.oracle_result(solver, v, s)["scene_status"] == 257 for s in sc.SEEDS[v]), (solver, v)
    moved, late = 0, 0.0
    for v, s in cases:
        r, f, w = sc.oracle_result("bound", v, s), sc.oracle_result("bound", v, s, frozen=True), sc.oracle_result("bound", v, s, shift=1)
        moved += int(r["nrows"].shape != f["nrows"].shape or (r["nrows"] != f["nrows"]).any())
        u = min(r["K_T_used"], w["K_T_used"])
        late = max(late, float(np.abs(r["pk"][:, :u] - w["pk"][:, :u]).max()))
    assert moved > 0
    assert late > 1e-4


def test_post_check_scenes_as_the_oracle_sees_them():
    """the two well-ended scenes of the GPU post-check test, by the oracle's loop and oracle/postcheck.py alone: B/3 keeps rmin - 0.05 from
    every vehicle at 100 Hz; A/1 keeps it at the 5 Hz columns the MPC constrains and loses it between two of them"""
    bar = sc.KW["rmin"] - 0.05
    a, b = sc.oracle_min_dist_scripted("bound", "A", 1), sc.oracle_min_dist_scripted("bound", "B", 3)
    assert b is not None and b >= bar + 0.01
    assert a is not None and a < bar - 0.01
    r = sc.oracle_result("bound", "A", 1)
    u, path = r["K_T_used"], sc.scene("A", 1)[2]
    knots = np.stack([sc.sample(path, i) for i in range(u)], axis=1)
    e1 = np.array([1.0, 1.0, 1.0 / sc.KW["c"]])
    assert np.sqrt((((r["pk"][:, None, :u] - knots[None]) * e1) ** 2).sum(-1)).min() >= bar
