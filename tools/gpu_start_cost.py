"""development: what a start in motion costs on ONE 100-agent scene (configs[3] shape, bound): the wall time of
  rest        dmpc_transition with K_T_max = 2 from rest: the initDMPC column, one step, the call's uploads and its last synchronisation
  from_end    dmpc_set_start(from_end) -- the gather of the last flight's end -- and the same flight from it
  set_start   dmpc_set_start(from_end) alone (cleared again)
  flight_end  dmpc_flight_end: the gather and the copies to the host
The modes are alternated within every repetition; each timing is a host clock around `calls` calls.  Prints median, minimum and maximum per mode.
usage: python tools/gpu_start_cost.py [repetitions [calls]]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multiagent_planning_amd as mp
from multiagent_planning_amd import workload as wl

args = sys.argv[1:]
reps = int(args[0]) if len(args) > 0 else 15
calls = int(args[1]) if len(args) > 1 else 50
cfg = wl.CONFIGS["C4"]
N = 100
po, pf = wl.make_scenes(cfg, 1, N, wl.SEED0 + 100)
tol = 0.0   # no scene ever reports ReachedGoal: the continued flights go on solving when the fleet has arrived
d = mp.Dmpc("bound", **wl.solver_kwargs(cfg, N))


def from_end():
    d.set_start(from_end=True, S=1, N_cmd=N)
    return d.transition(po, pf, 2, tol, histories=False)


def set_start():
    d.set_start(from_end=True, S=1, N_cmd=N)
    d.clear_start()


modes = {"rest": lambda: d.transition(po, pf, 2, tol, histories=False), "from_end": from_end, "set_start": set_start, "flight_end": lambda: d.flight_end(1, N)}
d.transition(po, pf, 10, tol, histories=False)   # a flight in motion to continue: every mode below leaves a valid end behind
for f in modes.values():
    for _ in range(3):
        f()
t = {name: [] for name in modes}
for rep in range(reps):
    for name, f in modes.items():
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        t[name].append((time.perf_counter() - t0) / calls)
out = {"agents": N, "repetitions": reps, "calls_per_timing": calls}
for name in modes:
    us = np.array(t[name]) * 1e6
    out[name] = {"median_us": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}
    print(f"{name:12s} {np.median(us):8.2f} us per call (min {us.min():.2f}, max {us.max():.2f}; {reps} x {calls} calls)")
print(json.dumps(out))
