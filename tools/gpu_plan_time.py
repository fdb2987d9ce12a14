"""development: what the route planner costs -- dmpc_plan_routes_device timed with HIP events (torch.cuda.Event on the stream the call is enqueued
on; both kernels of a call, device arrays, no copies) on two shapes:
  wall    tests/plan.py's wall: 3 agents, 21 static vehicles, cell 0.25 / margin 0.2 (20 x 20 x 8 = 3200 cells)
  crowd   one scene of 10 000 agents and 1 000 obstacle points (workload.random_test, 11 000 points) in the C4 density box, cell 0.7 (31^3 = 29 791 cells)
Every timing brackets `calls` calls back to back; prints median, minimum and maximum per call over the repetitions, and the distribution of hops
and n_wp, as text and as one JSON line.
usage: python tools/gpu_plan_time.py [repetitions [calls]]"""
import sys, os, json
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiagent_planning_amd as mp
from multiagent_planning_amd import workload as wl
import plan as pl

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = torch.device("cuda")


def shapes():
    w = pl.wall()
    yield "wall", pl.KW, w["po"][None, :3], w["goals"][None], w["po"][None, 3:], 0.25, 0.2
    cfg, N, M = wl.CONFIGS["C4"], 10000, 1000
    kw = wl.solver_kwargs(cfg, N)
    po, pf = wl.random_test(N + M, kw["pmin"], kw["pmax"], cfg["rmin_init"], cfg["c"], np.random.default_rng(wl.SEED0 + 31))
    yield "crowd", kw, po[None, :N], pf[None, :N], po[None, N:], 0.7, 0.0


out = {"repetitions": reps, "calls_per_timing": calls}
for name, kw, po, goals, obst, cell, margin in shapes():
    d = mp.Dmpc("bound", **kw)
    S, nc, M, W = po.shape[0], po.shape[1], obst.shape[1], 4
    tpo, tg, tob = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (po, goals, obst))
    wp = torch.zeros((S, nc, W, 3), dtype=torch.float64, device=dev)
    n_wp, st, hops = (torch.zeros((S, nc), dtype=torch.int32, device=dev) for _ in range(3))
    stream = torch.cuda.current_stream()
    run = lambda: d.plan_routes_device(S, nc, M, W, tpo.data_ptr(), tg.data_ptr(), tob.data_ptr(), cell, margin, wp.data_ptr(), n_wp.data_ptr(),
                                       st.data_ptr(), hops.data_ptr(), stream=stream.cuda_stream)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            run()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    ms = np.array(ms)
    h, n, s = hops.cpu().numpy().ravel(), n_wp.cpu().numpy().ravel(), st.cpu().numpy().ravel()
    grid = pl.grid_shape(kw["pmin"], kw["pmax"], cell)
    out[name] = {"agents": nc, "obstacles": M, "grid": list(grid), "cells": int(np.prod(grid)), "median_ms": round(float(np.median(ms)), 4),
                 "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4), "hops_mean": round(float(h[h >= 0].mean()), 1),
                 "hops_max": int(h.max()), "n_wp_counts": np.bincount(n, minlength=W + 1).tolist(), "status_counts": np.bincount(s, minlength=3).tolist()}
    print(f"{name:6s} {nc} agents, {M} obstacles, {grid} = {int(np.prod(grid))} cells: {np.median(ms):.4f} ms per call (min {ms.min():.4f}, max {ms.max():.4f}; "
          f"{reps} x {calls} calls), hops mean {h[h >= 0].mean():.1f} max {h.max()}, n_wp counts {np.bincount(n, minlength=W + 1).tolist()}, "
          f"status counts {np.bincount(s, minlength=3).tolist()}")
    d.close()
print(json.dumps(out))
