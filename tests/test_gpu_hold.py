"""GPU: the hold policy -- an agent whose solve failed flies its previous plan while the scene goes on -- through dmpc_transition_hold.  There is
no reference counterpart; the truth is the reference's own MPC step in the loop a caller could write on the host (hold.hold_loop), over
dmpc_step_batch / dmpc_step_batch_cmd (bit for bit) and over the oracle's step (the hold log identical, the histories at 1e-7: the bar of
tests/test_gpu_mission.py, test_gpu_scripted.py and test_gpu_obstacles.py for the same comparison).

Scenes: 8 commanded agents that cross a wall of 10 vehicles (scripted.scene, obstacles.wall_scene), K_T_max = 100, unless noted."""
import os

import numpy as np
import pytest

import multiagent_planning_amd as mp
from multiagent_planning_amd import workload as wl
from helpers import ROOT, lib_source
import hold as ho
import mission as ms
import obstacles as ob

pytestmark = pytest.mark.gpu

KT, TOL = ho.KT, ho.ERROR_TOL
HELD, REACHED = mp.ST_HELD, mp.ST_SOLVED | mp.ST_REACHED
COMMON = ("pk", "vk", "ak", "K_T_used", "scene_status", "stage_col")
NEW = ("hold_count", "hold_first", "agent_status")


def _err(d):
    return d._L.dmpc_last_error(d._ctx).decode()


def _same(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k} differs"


def _no_hold(r, what):
    assert not r["hold_count"].any() and (r["hold_first"] == -1).all() and not (r["agent_status"] & HELD).any() and not (r["scene_status"] & HELD).any(), what


def _scene_of(r, i):
    return {k: r[k][i] for k in COMMON + NEW}


def _log(ast):
    """[(column, agent, raw status)] of the holds in agent_status [nc,KT], by column, then agent: hold_loop's order"""
    i, k = np.nonzero(ast & HELD)
    return sorted((int(kk), int(ii), int(ast[ii, kk] & ~HELD)) for ii, kk in zip(i, k))


def _equals_host(res, host, what):
    """scene 0 of a device result against hold_loop's dict, bit for bit"""
    for k in ("pk", "vk", "ak", "hold_count", "hold_first", "agent_status", "stage_col"):
        assert res[k][0].tobytes() == np.ascontiguousarray(host[k]).tobytes(), f"{what}: {k} differs"
    assert res["K_T_used"][0] == host["K_T_used"] and res["scene_status"][0] == host["scene_status"], what
    assert _log(res["agent_status"][0]) == host["log"], what


def _run(d, s, **kw):
    rc, r = ho.raw_hold(d, s["po"][None], s["goals"][None], None if s["deadline"] is None else s["deadline"][None],
                        None if s["path"] is None else s["path"][None], **kw)
    assert rc == 0, _err(d)
    return r


# ---- 1. no failure: nothing changes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["B", "wall"])
@pytest.mark.parametrize("shape", ["tiny", "split40", "mixed"])
def test_without_a_failure_hold_equals_stop_byte_for_byte(shape, kind):
    """bound on scripted B seeds 0-2 and wall_scene seeds 0-2 (the oracle's loop flies them without a failure, tests/test_hold_cpu.py): one tiny
    scene (stop fuses the post step into the solve launch, hold never does), 40 scenes (two parts on contexts of their own) and mixed precision"""
    n = 40 if shape == "split40" else (3 if shape == "mixed" else 1)
    if n == 40:
        src = lib_source()
        assert "(S >= 128 ? 4 : (S >= 32 ? 2 : 1))" in src
    b = ho.batch([(kind, i % 3) for i in range(n)])
    d = mp.Dmpc("bound", precision="mixed" if shape == "mixed" else "f64", **ho.KW)
    stop = d.mission(b["po"], b["goals"], KT, TOL, path=b["path"], on_fail="stop")
    hold = d.mission(b["po"], b["goals"], KT, TOL, path=b["path"], on_fail="hold")
    assert not (stop["scene_status"] & ~REACHED).any() and (stop["scene_status"] == REACHED).all()
    _same(hold, stop, COMMON, f"{shape} {kind}")
    _no_hold(hold, f"{shape} {kind}")
    assert hold["agent_status"].shape == (n, 8, KT) and hold["hold_count"].shape == (n, 8)
    for s in range(n):
        u = hold["K_T_used"][s]
        assert (hold["agent_status"][s, :, :u] == 1).all() and not hold["agent_status"][s, :, u:].any()
    if shape == "tiny":   # Dmpc.transition: the same call without stage_col
        pf = b["goals"][:, 0]
        tr = d.transition(b["po"], pf, KT, TOL, path=b["path"], on_fail="hold")
        assert "stage_col" not in tr
        _same(tr, hold, COMMON[:-1] + NEW, "Dmpc.transition")
        _same(tr, d.transition(b["po"], pf, KT, TOL, path=b["path"]), COMMON[:-1], "Dmpc.transition, stop")


def test_without_a_failure_hold_equals_stop_with_neighbour_lists_and_post_step_kernel():
    """the 300-agent scenes of test_gpu_mission.py::test_one_stage_equals_dmpc_transition_with_post_step_kernel_and_neighbour_lists (cull_min = 256:
    neighbour lists; as many scenes as it takes to leave the tiny launches).  Those scenes are NOT free of failures over their 40 columns: in the
    oracle's loop every one of them has agents that report COLL, the first on columns 14 .. 20.  So: over K_T_max = 14 columns (no failure) hold
    equals stop byte for byte and nothing is held; over 40 columns hold with max_hold = 0 equals stop byte for byte, and hold with the default
    budget equals stop on every column before the one that stops the scene."""
    import torch
    N = 300
    assert ob.launch_thresholds()["cull_min"] <= N
    S = -(-8 * torch.cuda.get_device_properties(0).multi_processor_count // N)
    assert S < 32                                                                     # (one part)
    cfg = wl.CONFIGS["C4"]
    kw = wl.solver_kwargs(cfg, N)
    po, pf = wl.make_scenes(cfg, S, N, wl.SEED0 + 77)
    d = mp.Dmpc("bound", **kw)
    stop = d.mission(po, pf[:, None], 14, 0.5)
    hold = d.mission(po, pf[:, None], 14, 0.5, on_fail="hold")
    assert (stop["scene_status"] == mp.ST_SOLVED).all() and stop["pk"][:, :, 1:].any()
    _same(hold, stop, COMMON, "14 columns")
    _no_hold(hold, "14 columns")
    stop = d.mission(po, pf[:, None], 40, 0.5)
    _same(d.mission(po, pf[:, None], 40, 0.5, on_fail="hold", max_hold=0), stop, COMMON, "40 columns, max_hold = 0")
    hold = d.mission(po, pf[:, None], 40, 0.5, on_fail="hold")
    print("stop: K_T_used", stop["K_T_used"], "status", stop["scene_status"], "| hold: K_T_used", hold["K_T_used"], "status", hold["scene_status"],
          "holds", hold["hold_count"].sum(axis=1))
    for s in range(S):
        if stop["scene_status"][s] & ~REACHED:
            u = stop["K_T_used"][s] - 1                                               # the column that stops the scene
            hf = hold["hold_first"][s]
            assert hold["K_T_used"][s] > u and hf[hf >= 0].min() == u and (hold["agent_status"][s, :, u] & HELD).any()
            for k in ("pk", "vk", "ak"):
                assert np.array_equal(hold[k][s, :, :u], stop[k][s, :, :u])
        else:
            _same(_scene_of(hold, s), {k: stop[k][s] for k in COMMON}, COMMON, f"scene {s}")
            assert not hold["hold_count"][s].any()


# ---- 2. max_hold = 0 ------------------------------------------------------------------------------------------------------------------------------
def test_max_hold_zero_is_dmpc_transition_mission_byte_for_byte():
    """hard on scripted A 0: both stop on column 3 with an infeasible agent"""
    s = ho.scene("A", 0)
    d = mp.Dmpc("hard", **ho.KW)
    rc, mis = ms.raw_mission(d, s["po"][None], s["goals"][None], None, s["path"][None], K_T_max=KT, error_tol=TOL)
    assert rc == 0, _err(d)
    r = _run(d, s, max_hold=0)
    _same(r, mis, COMMON, "max_hold = 0")
    assert r["K_T_used"][0] == 4 and r["scene_status"][0] == 9
    _no_hold(r, "max_hold = 0")
    assert r["agent_status"][0, 5, 3] == 8 and (r["agent_status"][0, :, :3] == 1).all() and not r["agent_status"][0, :, 4:].any()


# ---- 3. against the host loop (bit for bit) and the oracle's loop (log identical, histories 1e-7) ------------------------------------------------
@pytest.mark.parametrize("case,precision", [(c, "f64") for c in ho.FAILING] + [(("bound", "A", 0), "mixed")],
                         ids=lambda c: c if isinstance(c, str) else "-".join(map(str, c)))
def test_hold_vs_host_loop_and_oracle_loop(case, precision):
    """the four wall crossings that stop today (tests/test_hold_cpu.py has their hold logs).  Measured on an MI355X, l_inf of pk / vk / ak against the
    oracle's loop over the columns flown: hard 1.0e-10 / 7.4e-11 / 2.0e-10, ondemand 8.2e-13 / 5.6e-13 / 1.5e-12, bound 6.3e-10 / 2.8e-10 / 7.1e-10, bound2 2.9e-12 / 1.6e-12 / 2.3e-12;
    every hold log and K_T_used identical"""
    solver, kind, seed = case
    s = ho.scene(kind, seed)
    d = mp.Dmpc(solver, precision=precision, **ho.KW)
    res = _run(d, s)
    host = ho.hold_loop(ms.device_step(d), s["po"], s["goals"], None, s["path"])
    print(f"{case} {precision}: K_T_used {res['K_T_used'][0]} / host {host['K_T_used']}, status {res['scene_status'][0]}, holds {_log(res['agent_status'][0])}")
    _equals_host(res, host, f"{case} {precision}")
    assert res["scene_status"][0] & HELD and res["hold_count"].sum() > 0
    if precision != "f64":
        return
    orc = ho.oracle_result(solver, kind, seed)
    print(f"  oracle: K_T_used {orc['K_T_used']}, status {orc['scene_status']}, holds {orc['log']}")
    assert _log(res["agent_status"][0]) == orc["log"] and res["K_T_used"][0] == orc["K_T_used"] and res["scene_status"][0] == orc["scene_status"]
    assert np.array_equal(res["hold_count"][0], orc["hold_count"]) and np.array_equal(res["hold_first"][0], orc["hold_first"])
    assert np.array_equal(res["agent_status"][0], orc["agent_status"])
    u = orc["K_T_used"]
    for k in ("pk", "vk", "ak"):
        err = float(np.abs(res[k][0][:, :u] - orc[k][:, :u]).max())
        print(f"  {k}: l_inf vs oracle loop = {err:.2e}")
        assert err <= 1e-7, (case, k, err)


# ---- 4. the budget --------------------------------------------------------------------------------------------------------------------------------
def test_budget_ends_the_scene_with_raw_bits():
    """ondemand / wall_scene(8,1), max_hold = 3: agent 2 is held on columns 6, 7, 8 and fails a fourth time on column 9 (tests/test_hold_cpu.py)"""
    s = ho.scene("wall", 1)
    d = mp.Dmpc("ondemand", **ho.KW)
    res = _run(d, s, max_hold=3)
    host = ho.hold_loop(ms.device_step(d), s["po"], s["goals"], None, s["path"], max_hold=3)
    _equals_host(res, host, "max_hold = 3")
    orc = ho.oracle_result("ondemand", "wall", 1, max_hold=3)
    u = int(res["K_T_used"][0])
    assert u == orc["K_T_used"] == 10 and res["scene_status"][0] == orc["scene_status"] == (1 | 8 | HELD) and res["stage_col"][0, 0] == -1
    ast = res["agent_status"][0]
    assert ast[2, u - 1] == 8 and not (ast[:, u - 1] & HELD).any() and (ast[2, 6:9] == (8 | HELD)).all()
    assert not ast[:, u:].any() and ast[:, :u].all()
    for k in ("pk", "vk", "ak"):
        assert not res[k][0][:, u:].any()


# ---- 5. neighbour lists, many holds ----------------------------------------------------------------------------------------------------------------
def test_hold_with_neighbour_lists_vs_host_loop():
    """one scene of 300 agents (cull_min = 256: neighbour lists), ondemand, 25 columns.  workload.make_scenes(C4, 1, 300, SEED0 + 903): in the
    oracle's loop 77 different agents are held within those columns (137 holds, the first on column 1, up to 12 of one agent), the fewest of the ten
    seeds SEED0 + 900 .. 909 (137 .. 235 holds each)"""
    N = 300
    assert ob.launch_thresholds()["cull_min"] <= N
    cfg = wl.CONFIGS["C4"]
    kw = wl.solver_kwargs(cfg, N)
    po, pf = wl.make_scenes(cfg, 1, N, wl.SEED0 + 903)
    d = mp.Dmpc("ondemand", **kw)
    rc, res = ho.raw_hold(d, po, pf[:, None], K_T_max=25, error_tol=0.5)
    assert rc == 0, _err(d)
    host = ho.hold_loop(ms.device_step(d), po[0], pf[0][None], K_T_max=25, error_tol=0.5, h=kw["h"], alim=kw["alim"])
    print("holds", int(res["hold_count"].sum()), "agents", int((res["hold_count"] > 0).sum()), "longest", int(res["hold_count"].max()))
    _equals_host(res, host, "300 agents")
    assert (res["hold_count"][0] > 0).sum() >= 3


# ---- 6. batch independence -------------------------------------------------------------------------------------------------------------------------
BATCH = (("A", 0), ("A", 1), ("A", 2), ("A", 5), ("B", 0), ("B", 3), ("B", 4))


@pytest.fixture(scope="module")
def alone():
    """bound2, max_hold = 2: every scene of BATCH run alone (in the oracle's loop A 0, A 2 and B 4 end over budget, A 5 and B 0 arrive with holds,
    A 1 and B 3 without)"""
    d = mp.Dmpc("bound2", **ho.KW)
    out = []
    for sc_ in BATCH:
        b = ho.batch([sc_])
        rc, r = ho.raw_hold(d, b["po"], b["goals"], None, b["path"], max_hold=2)
        assert rc == 0, _err(d)
        out.append(_scene_of(r, 0))
    return out


@pytest.mark.parametrize("S", [7, 40])
def test_every_scene_of_a_batch_equals_its_run_alone(alone, S):
    st = np.array([a["scene_status"] for a in alone])
    print("alone: status", st, "K_T_used", [int(a["K_T_used"]) for a in alone])
    assert (st == (REACHED | HELD)).any() and (st == REACHED).any() and ((st & HELD != 0) & (st & ~(REACHED | HELD) != 0)).any()   # held, unheld, over budget
    b = ho.batch([BATCH[i % 7] for i in range(S)])
    d = mp.Dmpc("bound2", **ho.KW)
    rc, r = ho.raw_hold(d, b["po"], b["goals"], None, b["path"], max_hold=2)
    assert rc == 0, _err(d)
    for i in range(S):
        _same(_scene_of(r, i), alone[i % 7], COMMON + NEW, f"scene {i} of {S}")


# ---- 7. missions ----------------------------------------------------------------------------------------------------------------------------------
def test_mission_passes_the_stage_in_which_it_fails_today():
    """mission.scene("failure"), Q = 3: today an agent collides on column 25, in stage 1; held there, the mission goes on (the oracle's loop: stage 1
    ends on column 58)"""
    s = ms.scene("failure")
    d = mp.Dmpc("bound", **ms.KW)
    rc, today = ms.raw_mission(d, s["po"][None], s["goals"][None], s["deadline"][None], s["path"][None])
    assert rc == 0 and today["scene_status"][0] & ~REACHED and today["stage_col"][0, 1] == -1
    res = _run(d, s, K_T_max=ms.KT, error_tol=ms.ERROR_TOL)
    host = ho.hold_loop(ms.device_step(d), s["po"], s["goals"], s["deadline"], s["path"], K_T_max=ms.KT, error_tol=ms.ERROR_TOL)
    print("today", today["K_T_used"][0], today["scene_status"][0], today["stage_col"][0], "| hold", res["K_T_used"][0], res["scene_status"][0], res["stage_col"][0])
    _equals_host(res, host, "mission")
    assert res["stage_col"][0, 0] == today["stage_col"][0, 0] and res["stage_col"][0, 1] > today["K_T_used"][0] - 1
    assert res["scene_status"][0] & HELD and res["hold_first"][0].max() >= today["K_T_used"][0] - 1
    api = d.mission(s["po"], s["goals"], ms.KT, ms.ERROR_TOL, deadline=s["deadline"], path=s["path"], on_fail="hold")
    for k in COMMON + NEW:
        assert np.asarray(api[k]).tobytes() == res[k].tobytes(), k


# ---- 8. the resident histories --------------------------------------------------------------------------------------------------------------------
def test_postcheck_and_clearance_on_the_resident_histories_of_a_held_transition():
    s = ho.scene("A", 0)
    d = mp.Dmpc("bound", **ho.KW)
    r = d.transition(s["po"], s["goals"][0], KT, TOL, path=s["path"], on_fail="hold")
    assert r["scene_status"][0] == (REACHED | HELD)
    pf = s["goals"][0]
    for call in (d.postcheck, d.clearance):
        res = call(r["K_T_used"], pf, KT_alloc=KT, path=s["path"])
        dl = call(r["K_T_used"], pf, r["pk"], r["vk"], r["ak"], path=s["path"])
        assert set(res) == set(dl)
        for k in res:
            assert np.asarray(res[k]).tobytes() == np.asarray(dl[k]).tobytes(), (call.__name__, k)
    assert np.isfinite(d.postcheck(r["K_T_used"], pf, KT_alloc=KT, path=s["path"])["min_dist"]).all()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_and_leave_the_context_usable():
    s = ho.scene("A", 0)
    d = mp.Dmpc("bound", **ho.KW)
    po, g, path = s["po"][None], s["goals"][None], s["path"][None]
    rc, ok = ho.raw_hold(d, po, g, None, path)
    assert rc == 0, _err(d)
    before = d.solve_count
    bad = [dict(max_hold=-1), dict(max_hold=-2147483648), dict(Q=0), dict(n_cmd=0), dict(n_cmd=19), dict(P=0), dict(K_T_max=1),
           dict(histories=(1, 0, 1)), dict(deadline=np.array([[-1]], dtype=np.int32)), dict(deadline=np.array([[3]], dtype=np.int32))]
    for kw in bad:
        rc, _ = ho.raw_hold(d, po, g, kw.pop("deadline", None), path, **kw)
        assert rc == -1 and _err(d).startswith("dmpc_transition_hold"), (kw, _err(d))
    rc, _ = ho.raw_hold(d, po, None, None, path, Q=1, n_cmd=8)
    assert rc == -1 and _err(d).startswith("dmpc_transition_hold: goals is NULL")
    rc, _ = ho.raw_hold(d, po, g, None, path, max_hold=-1)
    assert rc == -1 and "max_hold" in _err(d)
    assert d.solve_count == before                                                  # nothing launched
    with pytest.raises(mp.DmpcError):
        d.transition(s["po"], s["goals"][0], KT, TOL, path=s["path"], on_fail="hover")
    rc, again = ho.raw_hold(d, po, g, None, path, outputs=(0, 0, 0))                  # (and every new output may be NULL)
    assert rc == 0, _err(d)
    _same(again, ok, COMMON, "after the refusals")


# ---- 10. a batch in parts --------------------------------------------------------------------------------------------------------------------------
def _in_parts_and_whole(b):
    """bound, max_hold = 2, deadlines and all nine outputs, on a context that runs the batch in three parts and on one that never splits"""
    out = []
    for option in ("split_parts", 3), ("no_split", 1):
        d = mp.Dmpc("bound", **ms.KW).debug_option(*option)
        rc, r = ho.raw_hold(d, b["po"], b["goals"], b["deadline"], b["path"], K_T_max=ms.KT, error_tol=ms.ERROR_TOL, max_hold=2)
        assert rc == 0, _err(d)
        out.append((d, r))
    return out


def test_a_batch_in_three_parts_equals_the_whole_batch():
    """every per-scene array of a call reaches the part that runs its scenes: Q = 3 with deadlines, stage_col and the three hold outputs.  (a) the five
    four-agent scenes of test_gpu_mission.py::test_scenes_of_a_batch_switch_on_their_own in parts of 1, 2, 2; (b) the three wall crossings with their
    paths in parts of 1, 1, 1, the one that is held (seed 0) last; then dmpc_postcheck on the histories the parts left resident"""
    a = ms.batch(["reached", "deadline", "column0", "coincident", "reached"], [0, 0, 0, 0, 3])
    (_, parts), (_, whole) = _in_parts_and_whole(a)
    print("(a) stage_col", whole["stage_col"].tolist(), "K_T_used", whole["K_T_used"], "status", whole["scene_status"])
    assert len({tuple(c) for c in whole["stage_col"]}) >= 3
    _same(parts, whole, ho.OUTPUTS, "(a) five scenes in parts of 1, 2, 2")
    b = ms.batch(["failure"] * 3, [1, 5, 0])
    (dp, parts), (dw, whole) = _in_parts_and_whole(b)
    print("(b) holds per scene", whole["hold_count"].sum(axis=1), "K_T_used", whole["K_T_used"], "status", whole["scene_status"], "stage_col", whole["stage_col"].tolist())
    assert whole["hold_count"][2].sum() > 0
    _same(parts, whole, ho.OUTPUTS, "(b) three wall crossings in parts of 1, 1, 1")
    pf = b["goals"][:, -1]
    pc = [d.postcheck(whole["K_T_used"], pf, KT_alloc=ms.KT, path=b["path"]) for d in (dp, dw)]
    assert set(pc[0]) == set(pc[1]) and np.isfinite(pc[1]["min_dist"]).all()
    _same(pc[0], pc[1], sorted(pc[0]), "postcheck on the resident histories of the parts")
