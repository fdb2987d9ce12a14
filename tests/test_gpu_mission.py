"""GPU: missions -- a transition through a sequence of goal sets -- through dmpc_transition_mission.  There is no reference counterpart; the
truth is the reference's own MPC step in the loop a caller could write on the host (mission.mission_loop), over the oracle's step and over
dmpc_step_batch / dmpc_step_batch_cmd.

Bars are the ones the existing files use for the same comparisons: bit identity against the one-leg entries, against the host loop and
between batch shapes; the closed loop against the oracle's at 1e-7 (tests/test_gpu_scripted.py, tests/test_gpu_obstacles.py)."""
import os

import numpy as np
import pytest

import multiagent_planning_amd as mp
from multiagent_planning_amd import workload as wl
from helpers import ROOT, lib_source
import obstacles as ob
import mission as ms

pytestmark = pytest.mark.gpu

KT, TOL = ms.KT, ms.ERROR_TOL
REACHED = mp.ST_SOLVED | mp.ST_REACHED
HIST = ("pk", "vk", "ak")


def _err(d):
    return d._L.dmpc_last_error(d._ctx).decode()


def _one_leg_equal(mis, leg, what):
    for k in HIST + ("K_T_used", "scene_status"):
        assert mis[k].dtype == leg[k].dtype and mis[k].shape == leg[k].shape and mis[k].tobytes() == leg[k].tobytes(), f"{what}: {k} differs"
    want = np.where(leg["scene_status"] == REACHED, leg["K_T_used"] - 1, -1)
    assert mis["stage_col"].shape == (len(want), 1) and np.array_equal(mis["stage_col"][:, 0], want), what


# ---- 1. Q == 1, no deadline: the one-leg entries byte for byte -------------------------------------------------------------------------------
def _tiny(n, seeds=None):
    seeds = range(n) if seeds is None else seeds
    r, s, p = (ms.batch([name] * n, list(seeds)) for name in ("reached", "static", "path"))
    return r, s, p


@pytest.mark.parametrize("shape", ["tiny", "split40", "mixed"])
def test_one_stage_equals_the_one_leg_entries_byte_for_byte(shape):
    """one tiny scene (the fused post step), 40 tiny scenes (two parts on contexts of their own) and mixed precision, against dmpc_transition,
    dmpc_transition_cmd and dmpc_transition_scripted; stage_col is the last column of a scene that reached and -1 otherwise.  K_T_max = 30
    columns in the batch of 40 with one scene's goals out of reach, so that both kinds are there."""
    n = 40 if shape == "split40" else (2 if shape == "mixed" else 1)
    kt = 30
    r, s, p = _tiny(n)
    if n == 40:
        src = lib_source()
        assert "(S >= 128 ? 4 : (S >= 32 ? 2 : 1))" in src
        for b in (r, s, p):
            b["goals"][7, 0, :, 0] += 2.0                                             # too far for 30 columns
    d = mp.Dmpc("bound", precision="mixed" if shape == "mixed" else "f64", **ms.KW)
    mis = d.mission(r["po"], r["goals"][:, :1], kt, TOL)
    _one_leg_equal(mis, d.transition(r["po"], r["goals"][:, 0], kt, TOL), shape + " / dmpc_transition")
    assert (mis["scene_status"] == REACHED).any() and (n != 40 or mis["scene_status"][7] == mp.ST_SOLVED)
    rc, cmd = ob.raw_transition_cmd(d, s["po"], s["goals"][:, 0], 4, kt, TOL)
    assert rc == 0, _err(d)
    _one_leg_equal(d.mission(s["po"], s["goals"][:, :1], kt, TOL), cmd, shape + " / dmpc_transition_cmd")
    _one_leg_equal(d.mission(p["po"], p["goals"][:, :1], kt, TOL, path=p["path"]), d.transition(p["po"], p["goals"][:, 0], kt, TOL, path=p["path"]),
                   shape + " / dmpc_transition_scripted")


def test_one_stage_equals_dmpc_transition_with_post_step_kernel_and_neighbour_lists():
    """scenes of 300 agents (cull_min = 256: neighbour lists), as many as it takes to leave the tiny launches that fuse the post step into the solve
    kernel: plan_step calls a launch tiny below 8 agents per CU"""
    import torch
    src = open(os.path.join(ROOT, "multiagent_planning_amd", "csrc", "dmpc_launch.hip")).read()
    assert "pl.tiny = (long)S * c_count < 8L * ncu" in src and "pl.fuse_post = pl.tiny &&" in src
    N = 300
    assert ob.launch_thresholds()["cull_min"] <= N
    S = -(-8 * torch.cuda.get_device_properties(0).multi_processor_count // N)
    assert S < 32                                                                     # (one part)
    cfg = wl.CONFIGS["C4"]
    kw = wl.solver_kwargs(cfg, N)
    po, pf = wl.make_scenes(cfg, S, N, wl.SEED0 + 77)
    d = mp.Dmpc("bound", **kw)
    leg = d.transition(po, pf, 40, 0.5)
    mis = d.mission(po, pf[:, None], 40, 0.5)
    _one_leg_equal(mis, leg, "post_step_kernel")
    assert leg["pk"][:, :, 1:].any()


# ---- 2. Q == 3 against the host loop (bit for bit) and the oracle's loop (1e-7) ---------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("name", ["reached", "static", "path", "deadline"])
def test_mission_vs_host_loop_and_oracle_loop(name, precision):
    s = ms.scene(name)
    d = mp.Dmpc("bound", precision=precision, **ms.KW)
    dl = None if s["deadline"] is None else s["deadline"][None]
    res = d.mission(s["po"][None], s["goals"][None], KT, TOL, deadline=dl, path=None if s["path"] is None else s["path"][None])
    host = ms.mission_loop(ms.device_step(d), s["po"], s["goals"], s["deadline"], s["path"])
    u = host["K_T_used"]
    print(f"{name} {precision}: K_T_used {res['K_T_used'][0]} / host {u}, status {res['scene_status'][0]}, stage_col {res['stage_col'][0]} / {host['stage_col']}")
    assert int(res["K_T_used"][0]) == u and int(res["scene_status"][0]) == host["scene_status"] == REACHED
    assert np.array_equal(res["stage_col"][0], host["stage_col"])
    for k in HIST:
        assert np.array_equal(res[k][0], host[k]), k
    if precision == "f64":
        o = ms.oracle_result("bound", name)
        assert u == o["K_T_used"] and np.array_equal(host["stage_col"], o["stage_col"])
        for k in HIST:
            err = np.abs(res[k][0] - o[k]).max()
            print(f"  l_inf({k}) vs the oracle's loop {err:.2e}")
            assert err < 1e-7, k


# ---- 3. batch independence -------------------------------------------------------------------------------------------------------------------
def _alone_equals_batch(d, b, res, s):
    one = mp.Dmpc("bound", **ms.KW).mission(b["po"][s:s + 1], b["goals"][s:s + 1], KT, TOL, deadline=b["deadline"][s:s + 1],
                                             path=None if b["path"] is None else b["path"][s:s + 1])
    for k in HIST + ("K_T_used", "scene_status", "stage_col"):
        assert one[k][0].tobytes() == res[k][s].tobytes(), (s, k)


def test_scenes_of_a_batch_switch_on_their_own():
    """five scenes of four agents that switch on different columns, and three wall crossings of which one fails early: every scene as when it runs alone"""
    d = mp.Dmpc("bound", **ms.KW)
    b = ms.batch(["reached", "deadline", "column0", "coincident", "reached"], [0, 0, 0, 0, 3])
    res = d.mission(b["po"], b["goals"], KT, TOL, deadline=b["deadline"])
    assert len({tuple(c) for c in res["stage_col"]}) >= 4
    for s in range(5):
        _alone_equals_batch(d, b, res, s)
    w = ms.batch(["failure"] * 3, [0, 1, 5])
    res = d.mission(w["po"], w["goals"], KT, TOL, deadline=w["deadline"], path=w["path"])
    assert res["scene_status"][0] & ~mp.ST_SOLVED and (res["K_T_used"][1:] > res["K_T_used"][0] + 8).all() and (res["stage_col"][1:, 1] > res["K_T_used"][0]).all()
    assert not res["pk"][0][:, res["K_T_used"][0]:].any()
    for s in range(3):
        _alone_equals_batch(d, w, res, s)


# ---- 4. the special scenes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["column0", "coincident", "failure"])
def test_special_scenes_report_what_the_cpu_loop_reports(name):
    s, o = ms.scene(name), ms.oracle_result("bound", name)
    d = mp.Dmpc("bound", **ms.KW)
    res = d.mission(s["po"][None], s["goals"][None], KT, TOL, deadline=None if s["deadline"] is None else s["deadline"][None],
                    path=None if s["path"] is None else s["path"][None])
    print(name, res["K_T_used"], res["scene_status"], res["stage_col"], "oracle", o["K_T_used"], o["scene_status"], o["stage_col"])
    assert int(res["K_T_used"][0]) == o["K_T_used"] and int(res["scene_status"][0]) == o["scene_status"]
    assert np.array_equal(res["stage_col"][0], o["stage_col"])
    u = o["K_T_used"]
    assert np.abs(res["pk"][0][:, :u] - o["pk"][:, :u]).max() < 1e-7 and not res["pk"][0][:, u:].any()


def test_an_intermediate_stage_reached_never_reports_reached():
    """the mission cut short after its first stage ended: the status stays DMPC_ST_SOLVED, the trial runs to K_T_max"""
    s, o = ms.scene("reached"), ms.oracle_result("bound", "reached")
    kt = int(o["stage_col"][0]) + 6
    res = mp.Dmpc("bound", **ms.KW).mission(s["po"][None], s["goals"][None], kt, TOL)
    assert int(res["scene_status"][0]) == mp.ST_SOLVED and int(res["K_T_used"][0]) == kt
    assert list(res["stage_col"][0]) == [int(o["stage_col"][0]), -1, -1]
    assert np.abs(res["pk"][0] - o["pk"][:, :kt]).max() < 1e-7                       # ... and it flew on towards the second goal set


# ---- 5. resident histories ---------------------------------------------------------------------------------------------------------------------
def test_postcheck_and_clearance_on_the_resident_histories():
    b = ms.batch(["static", "static"], [0, 2])
    d = mp.Dmpc("bound", **ms.KW)
    res = d.mission(b["po"], b["goals"], KT, TOL)
    assert (res["scene_status"] == REACHED).all()
    pf, pos = b["goals"][:, -1], b["po"][:, 4:]
    down = d.postcheck(res["K_T_used"], pf, res["pk"], res["vk"], res["ak"], po_static=pos)
    here = d.postcheck(res["K_T_used"], pf, KT_alloc=KT, po_static=pos)
    assert sorted(down) == sorted(here) and all(np.array_equal(down[k], here[k]) for k in down)
    cd = d.clearance(res["K_T_used"], pf, res["pk"], res["vk"], res["ak"], po_static=pos)
    d.mission(b["po"], b["goals"], KT, TOL, histories=False)
    ch = d.clearance(res["K_T_used"], pf, KT_alloc=KT, po_static=pos)
    assert all(np.array_equal(cd[k], ch[k], equal_nan=True) for k in cd) and np.isfinite(cd["dist"]).all()
    # the whole mission is ONE flight: it is longer than its last leg
    assert (down["totdist"] > 1.5 * np.linalg.norm(pf - b["goals"][:, 1], axis=-1).sum(-1)).all()


# ---- 6. argument checks --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name_and_launch_nothing():
    s = ms.scene("path")
    po, goals, path = s["po"][None], s["goals"][None], s["path"][None]
    d = mp.Dmpc("bound", **ms.KW)
    n0 = d.solve_count
    ok = np.array([[3, 0, 0]], dtype=np.int32)
    cases = [(dict(Q=0), "Q must"), (dict(Q=-1), "Q must"), (dict(goals=None, Q=3, n_cmd=4), "goals is NULL"),
             (dict(deadline=np.array([[3, -1, 0]])), "negative"), (dict(deadline=np.array([[0, 0, 2]])), "last stage"),
             (dict(n_cmd=0), "N_cmd must"), (dict(n_cmd=7), "N_cmd must"), (dict(P=0), "P must"), (dict(K_T_max=1), "bad arguments"),
             (dict(histories=(1, 0, 1)), "pk, vk, ak")]
    for kw, word in cases:
        args = dict(po=po, goals=goals, deadline=ok, path=path); args.update(kw)
        rc, _ = ms.raw_mission(d, **args)
        assert rc == -1 and _err(d).startswith("dmpc_transition_mission: ") and word in _err(d), (kw, _err(d))
    assert d.solve_count == n0
    leg = d.transition(po, goals[:, 0], 30, TOL, path=path)                           # the context still runs a normal transition
    assert int(leg["scene_status"][0]) == REACHED and d.solve_count > n0
    rc, res = ms.raw_mission(d, po, goals, ok, path, stage_col=False)                 # ... and a mission, without stage_col
    assert rc == 0 and int(res["scene_status"][0]) == REACHED
