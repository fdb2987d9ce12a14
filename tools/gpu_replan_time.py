"""development: what re-planning during a flight costs, on one MI355X.
  columns   wall time per history column of ONE 100-agent scene (configs[3] shape, bound) with four static vehicles far outside the workspace -- no
            cell is blocked, so the plan is every agent's goal alone and nobody is ever flagged --, closed loop on the device, histories not
            downloaded: dmpc_transition_route on that plan ("route"), dmpc_transition_replan with every = 0 ("replan0": route's launches per column;
            the call also plans before column 0) and with every = 5 ("replan5": a memset, the check and the list form of the planner on every
            fifth column, every workgroup of which returns at once).  --other LIB: dmpc_transition_route of another build of the library (the
            parent commit's, say) as a fourth mode "other", loaded next to this one in the same process.  The modes are alternated within every
            repetition; each timing is a host clock around `calls` whole transitions (a call ends in a stream synchronise).
  step      one re-plan step (dmpc_replan_routes_device: the blocked mask, the check, the planner for the flagged agents) on the large shape of
            tools/gpu_plan_time.py -- one scene of 10 000 agents, 1 000 obstacle points, cell 0.7 (31^3 = 29 791 cells) --, every agent on a
            straight line to its goal, with 0 %, 1 % and 100 % of the agents flagged: the (start, goal) pairs whose straight line is blocked, and
            those whose line is clear, are found with one call and tiled to the share.  HIP events on the stream around ONE call; the state is
            restored between calls (a re-planned agent's legs are clear); next to it a full plan (dmpc_plan_routes_device) of the same agents.
Prints median, minimum and maximum over the repetitions as text and as one JSON line.
--step-only: the second part alone (a short run to put under a kernel trace, which splits a step into its three kernels).
usage: python tools/gpu_replan_time.py [--step-only] [--other LIB.so] [repetitions [calls]]"""
import sys, os, time, json
import ctypes as C
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multiagent_planning_amd as mp
from multiagent_planning_amd import _lib, workload as wl

args = sys.argv[1:]
step_only = bool(args) and args[0] == "--step-only"
if step_only:
    args = args[1:]
other = None
if args and args[0] == "--other":
    other, args = os.path.abspath(args[1]), args[2:]
reps = int(args[0]) if len(args) > 0 else 15
calls = int(args[1]) if len(args) > 1 else 20
out = {"repetitions": reps, "calls_per_timing": calls}


def stats(a, digits=2):
    a = np.asarray(a)
    return {"median": round(float(np.median(a)), digits), "min": round(float(a.min()), digits), "max": round(float(a.max()), digits)}


# ---- per column of a 100-agent scene ----------------------------------------------------------------------------------------------------------
cfg = wl.CONFIGS["C4"]
W = 4
if not step_only:
    N = 100
    kw = wl.solver_kwargs(cfg, N)
    po, pf = wl.make_scenes(cfg, 1, N, wl.SEED0 + 100)
    KT, tol = cfg["K_T"], cfg["error_tol"]
    far = np.array(kw["pmax"]) + 50.0 + np.arange(4)[:, None] * np.array([3.0, 0.0, 0.0])   # four static vehicles nobody ever sees
    po_all = np.concatenate([po, far[None]], axis=1)
    cell = float(max(np.array(kw["pmax"]) - np.array(kw["pmin"]))) / 20.0
    d = mp.Dmpc("bound", **kw)
    plan = d.plan(po_all, pf, cell, 0.0, W=W)
    assert (plan["n_wp"] == 1).all() and plan["waypoints"].tobytes() == np.repeat(pf[:, :, None, :], W, axis=2).tobytes()
    modes = {"route": lambda: d.route(po_all, plan["waypoints"], KT, 0.5, n_wp=plan["n_wp"], error_tol=tol, histories=False),
             "replan0": lambda: d.replan(po_all, pf, KT, cell, 0.5, W=W, every=0, error_tol=tol, histories=False),
             "replan5": lambda: d.replan(po_all, pf, KT, cell, 0.5, W=W, every=5, error_tol=tol, histories=False)}
    if other:
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L2 = C.CDLL(other)
        L2.dmpc_create.restype = C.c_void_p
        L2.dmpc_create.argtypes = [C.POINTER(_lib.DmpcParams), C.c_int, C.c_int]
        L2.dmpc_transition_route.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, ip, C.c_double, C.c_int, dp, C.c_int, C.c_int, C.c_double,
                                             C.c_int, dp, dp, dp, ip, ip, ip, ip, ip, ip, ip]
        ctx2 = L2.dmpc_create(C.byref(d.prm), 0, 0)
        assert ctx2
        po_c, wp_c, n_c = np.ascontiguousarray(po_all), np.ascontiguousarray(plan["waypoints"]), np.ascontiguousarray(plan["n_wp"])

        def run_other():
            used, sst = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
            assert L2.dmpc_transition_route(ctx2, 1, N + 4, N, W, po_c.ctypes.data_as(dp), wp_c.ctypes.data_as(dp), n_c.ctypes.data_as(ip), 0.5, 0, dp(), 0, int(KT),
                                            float(tol), 0, dp(), dp(), dp(), used.ctypes.data_as(ip), sst.ctypes.data_as(ip), ip(), ip(), ip(), ip(), ip()) == 0
            return dict(K_T_used=used, scene_status=sst)
        modes["other"] = run_other
    cols = {}
    for name, f in modes.items():   # warm-up of every shape; and the scene must fly without a failure, the same columns in every mode
        for _ in range(3):
            r = f()
        st = int(r["scene_status"][0])
        assert st in (1, 1 | 256), f"{name}: scene_status {st}: the scene has a failure"
        cols[name] = int(r["K_T_used"][0]) - 1
        if name.startswith("replan"):
            assert not r["replan_count"].any()
    assert len(set(cols.values())) == 1, cols
    t = {name: [] for name in modes}
    for rep in range(reps):
        for name, f in modes.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            t[name].append((time.perf_counter() - t0) / calls)
    out["columns"] = {"agents": N, "columns": cols["route"], "replan_columns": len([k for k in range(1, cols["route"] + 1) if k % 5 == 0])}
    for name in modes:
        us = np.array(t[name]) / cols[name] * 1e6
        out["columns"][name] = {"us_per_column": stats(us)}
        print(f"{name:8s} {np.median(us):7.2f} us per column (min {us.min():.2f}, max {us.max():.2f}; {cols[name]} columns, {reps} x {calls} transitions)")
    d.close()

# ---- one re-plan step on the large shape ------------------------------------------------------------------------------------------------------------
dev = torch.device("cuda")
Nl, M, cell = 10000, 1000, 0.7
kw = wl.solver_kwargs(cfg, Nl)
po, pf = wl.random_test(Nl + M, kw["pmin"], kw["pmax"], cfg["rmin_init"], cfg["c"], np.random.default_rng(wl.SEED0 + 31))
xp, goals, obst = po[:Nl], pf[:Nl], po[Nl:]
d = mp.Dmpc("bound", **kw)
stream = torch.cuda.current_stream()
up = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
tob = up(obst[None])


def state(xp, goals):
    """every agent on a straight line to its goal: the tensors of one step and the values to restore them from"""
    t = dict(x_p=up(xp[None]), goals=up(goals[None]), wp=up(np.repeat(goals[None, :, None, :], W, axis=2)), n_wp=torch.ones((1, Nl), dtype=torch.int32, device=dev),
             cur=torch.zeros((1, Nl), dtype=torch.int32, device=dev), cnt=torch.zeros((1, Nl), dtype=torch.int32, device=dev))
    t["keep"] = {k: t[k].clone() for k in ("wp", "n_wp", "cur", "cnt")}
    return t


def step(t):
    d.replan_routes_device(1, Nl, M, W, t["x_p"].data_ptr(), t["goals"].data_ptr(), tob.data_ptr(), cell, 0.0, 7, t["wp"].data_ptr(), t["n_wp"].data_ptr(),
                           t["cur"].data_ptr(), replan_count=t["cnt"].data_ptr(), stream=stream.cuda_stream)


def restore(t):
    for k, v in t["keep"].items():
        t[k].copy_(v)


t0 = state(xp, goals)
step(t0)
torch.cuda.synchronize()
hit = t0["cnt"].cpu().numpy().ravel() > 0
print(f"large shape: {int(hit.sum())} of {Nl} straight lines are blocked")
assert hit.sum() >= 100 and (~hit).sum() >= 100
tile = lambda idx, n: np.resize(idx, n)
shares = {}
for name, flagged in (("0%", 0), ("1%", Nl // 100), ("100%", Nl)):
    idx = np.concatenate([tile(np.nonzero(hit)[0], flagged), tile(np.nonzero(~hit)[0], Nl - flagged)]).astype(int)
    ts = state(xp[idx], goals[idx])
    ms = []
    for r in range(reps + 3):
        restore(ts)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        step(ts)
        e1.record(stream)
        e1.synchronize()
        if r >= 3:
            ms.append(e0.elapsed_time(e1))
    got = int((ts["cnt"].cpu().numpy() > 0).sum())
    assert got == flagged, (name, got, flagged)
    shares[name] = {"flagged": got, "ms": stats(ms, 4)}
    print(f"re-plan step, {name:4s} flagged ({got} agents): {np.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}; {reps} calls)")
wp = torch.zeros((1, Nl, W, 3), dtype=torch.float64, device=dev)
n_wp = torch.zeros((1, Nl), dtype=torch.int32, device=dev)
ms = []
for r in range(reps + 3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    d.plan_routes_device(1, Nl, M, W, t0["x_p"].data_ptr(), t0["goals"].data_ptr(), tob.data_ptr(), cell, 0.0, wp.data_ptr(), n_wp.data_ptr(), stream=stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    if r >= 3:
        ms.append(e0.elapsed_time(e1))
print(f"full plan of the {Nl} agents: {np.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})")
out["step"] = {"agents": Nl, "obstacles": M, "cells": 31 ** 3, "blocked_lines": int(hit.sum()), "shares": shares, "full_plan_ms": stats(ms, 4)}
d.close()
print(json.dumps(out))
