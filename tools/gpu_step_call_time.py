"""development: call time of dmpc_step_batch on ONE scene of 100 agents (host arrays in and out: uploads, the step, downloads, synchronise) -- the host
side of the step entries.  The state is MPC step 12 of a C4 transition (bench.capture_state); warm calls, REPS repeats, median / min / max in us.
Run per build in a process of its own (tools/with_lib.py), alternated:   python tools/gpu_step_call_time.py [label]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multiagent_planning_amd as mp   # noqa: E402
from multiagent_planning_amd import workload as wl   # noqa: E402
import bench   # noqa: E402

REPS, N = 400, 100
cfg = wl.CONFIGS["C4"]
d = mp.Dmpc("bound", **wl.solver_kwargs(cfg, N))
l, xp, xv, xa, pf, _ = bench.capture_state(d, cfg, 1, N, 12, wl.SEED0 + 2)
for _ in range(50):
    d.step_batch(l, xp, xv, xa, pf)
t = np.empty(REPS)
for i in range(REPS):
    t0 = time.perf_counter()
    d.step_batch(l, xp, xv, xa, pf)
    t[i] = time.perf_counter() - t0
print(" ".join(sys.argv[1:]), f"dmpc_step_batch S=1 N={N}: median {np.median(t) * 1e6:.1f} us (min {t.min() * 1e6:.1f}, max {t.max() * 1e6:.1f}; {REPS} calls)")
