"""development: what the post-checks cost on the resident histories of a split batch -- 512 transitions of 100 agents (bench.py's "512 whole
transitions": four parts on four contexts), then dmpc_postcheck, dmpc_postcheck_clearance and dmpc_postcheck_setpoints (report only) on the
histories the parts hold.  Host clock around each call, one warm call, 15 repeats; one JSON line: median, min, max in ms per entry.

  python tools/gpu_postcheck_time.py                                    (this build)
  python tools/with_lib.py OTHER.so tools/gpu_postcheck_time.py         (another build, in a process of its own; alternate the two)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multiagent_planning_amd as mp   # noqa: E402
from multiagent_planning_amd import _lib, workload as wl   # noqa: E402

cfg = dict(wl.CONFIGS["C4"])
d = mp.Dmpc("bound", **wl.solver_kwargs(cfg, 100))
po, pf = wl.make_scenes(cfg, 512, 100, wl.SEED0 + 100)
tr = d.transition(po, pf, cfg["K_T"], cfg["error_tol"], histories=False)
used, mask, KT = tr["K_T_used"], ((tr["scene_status"] & 256) != 0).astype(np.int32), cfg["K_T"]
calls = dict(postcheck=lambda: d.postcheck(used, pf, KT_alloc=KT, mask=mask), clearance=lambda: d.clearance(used, pf, KT_alloc=KT, mask=mask),
             setpoints=lambda: d.setpoints(used, N=100, KT_alloc=KT, mask=mask, report_only=True))
out = dict(lib=os.path.basename(_lib.LIB_PATH), completed=int(mask.sum()))
for name, f in calls.items():
    f()
    t = []
    for _ in range(15):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    out[name] = dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))
print(json.dumps(out), flush=True)
