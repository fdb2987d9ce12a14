"""development: what the waypoint rule costs a scene that never switches -- wall time per history column of ONE 100-agent scene (configs[3] shape,
bound), closed loop on the device: dmpc_transition ("stop"), dmpc_transition_hold ("hold": the post step out of the solve launch, one more launch
per column) and dmpc_transition_route with W = 1 and the stop rule ("route": hold's launches with max_hold = 0 and route_kernel behind the
verdict of every column).  The modes are alternated within every repetition; each timing is a host clock around `calls` whole transitions (a
call ends in a stream synchronise).  Prints median, minimum and maximum per mode.
--other LIB: dmpc_transition of another build of the library (the parent commit's, say) as a fourth mode "other", loaded next to this one in the
same process and alternated with the rest.
usage: python tools/gpu_route_cost.py [--other LIB.so] [repetitions [calls]]"""
import sys, os, time, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multiagent_planning_amd as mp
from multiagent_planning_amd import _lib, workload as wl
import ctypes as C
args = sys.argv[1:]
other = None
if args and args[0] == "--other":
    other, args = os.path.abspath(args[1]), args[2:]
reps = int(args[0]) if len(args) > 0 else 15
calls = int(args[1]) if len(args) > 1 else 20
cfg = wl.CONFIGS["C4"]
N = 100
kw = wl.solver_kwargs(cfg, N)
po, pf = wl.make_scenes(cfg, 1, N, wl.SEED0 + 100)
KT, tol = cfg["K_T"], cfg["error_tol"]
d = mp.Dmpc("bound", **kw)
wp = np.ascontiguousarray(pf[:, :, None, :])
modes = {"stop": lambda: d.transition(po, pf, KT, tol, histories=False),
         "hold": lambda: d.transition(po, pf, KT, tol, histories=False, on_fail="hold"),
         "route": lambda: d.route(po, wp, KT, 0.5, error_tol=tol, histories=False)}
if other:
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L2 = C.CDLL(other)
    L2.dmpc_create.restype = C.c_void_p
    L2.dmpc_create.argtypes = [C.POINTER(_lib.DmpcParams), C.c_int, C.c_int]
    L2.dmpc_transition.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, C.c_int, C.c_double, dp, dp, dp, ip, ip]
    ctx2 = L2.dmpc_create(C.byref(d.prm), 0, 0)
    assert ctx2
    po_c, pf_c = np.ascontiguousarray(po, dtype=np.float64), np.ascontiguousarray(pf, dtype=np.float64)

    def run_other():
        used, sst = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        assert L2.dmpc_transition(ctx2, 1, N, po_c.ctypes.data_as(dp), pf_c.ctypes.data_as(dp), int(KT), float(tol), dp(), dp(), dp(), used.ctypes.data_as(ip),
                                  sst.ctypes.data_as(ip)) == 0
        return dict(K_T_used=used, scene_status=sst)
    modes["other"] = run_other
cols = {}
for name, f in modes.items():   # warm-up of every shape; and the scene must fly without a failure
    for _ in range(3):
        r = f()
    st = int(r["scene_status"][0])
    assert st in (1, 1 | 256), f"{name}: scene_status {st}: the scene has a failure"
    cols[name] = int(r["K_T_used"][0]) - 1
    if name == "hold":
        assert not r["hold_count"].any()
assert len(set(cols.values())) == 1, cols
t = {name: [] for name in modes}
for rep in range(reps):
    for name, f in modes.items():
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        t[name].append((time.perf_counter() - t0) / calls)
out = {"agents": N, "columns": cols["stop"], "repetitions": reps, "calls_per_timing": calls}
for name in modes:
    us = np.array(t[name]) / cols[name] * 1e6
    out[name] = {"median_us_per_column": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}
    print(f"{name:12s} {np.median(us):7.2f} us per column (min {us.min():.2f}, max {us.max():.2f}; {cols[name]} columns, {reps} x {calls} transitions)")
print(json.dumps(out))
