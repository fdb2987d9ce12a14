"""development: what a measurement model costs a flight under a feedback policy -- wall time per history column of ONE scene (configs[3] shape,
bound), closed loop on the device, on the model of tools/gpu_feedback_cost.py: dmpc_transition with a policy and a disturbance ("feedback": the
trigger (0.05 m, 0.25 m/s) against noise of 1e-6, so post_step_feedback_kernel runs and no agent is re-anchored), the same with a measurement of
no noise and gain 1 ("quiet": post_step_estimate_kernel in its place, the same bytes -- the new kernel's overhead alone), and sensor noise (0.02 m,
0.05 m/s) with trigger 0 and no disturbance ("every": every agent's planner re-initialised to its estimate and its plan re-anchored on every
column).  The modes are alternated within every repetition; each timing is a host clock around `calls` whole transitions (a call ends in a
stream synchronise).  Prints median, minimum and maximum per mode.
--other LIB: the "feedback" flight of another build of the library (the parent commit's, say) as a mode "other", loaded next to this one in the
same process and alternated with the rest.
--hold 1: every flight with on_fail="hold" (a dense scene of thousands of agents does not fly ten columns without a failed agent; held, it goes on).
usage: python tools/gpu_estimate_cost.py [--other LIB.so] [--agents N] [--columns K_T_max] [--hold 1] [repetitions [calls]]"""
import sys, os, time, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multiagent_planning_amd as mp
from multiagent_planning_amd import _lib, workload as wl
import ctypes as C
args = sys.argv[1:]
other, N, KT, on_fail = None, 100, None, "stop"
while args and args[0].startswith("--"):
    if args[0] == "--other":
        other = os.path.abspath(args[1])
    elif args[0] == "--agents":
        N = int(args[1])
    elif args[0] == "--columns":
        KT = int(args[1])
    elif args[0] == "--hold":
        on_fail = "hold" if int(args[1]) else "stop"
    else:
        sys.exit(__doc__)
    args = args[2:]
reps = int(args[0]) if len(args) > 0 else 15
calls = int(args[1]) if len(args) > 1 else 20
cfg = wl.CONFIGS["C4"]
kw = wl.solver_kwargs(cfg, N)
po, pf = wl.make_scenes(cfg, 1, N, wl.SEED0 + 100)
KT, tol = cfg["K_T"] if KT is None else KT, cfg["error_tol"]
NOISE = dict(noise_p=1e-6, noise_v=1e-6, seed=1)
TRIGGER = (0.05, 0.25)
ctx = {name: mp.Dmpc("bound", **kw) for name in ("feedback", "quiet", "every")}
ctx["feedback"].set_disturbance(**NOISE).set_feedback(*TRIGGER, reanchor=True)
ctx["quiet"].set_disturbance(**NOISE).set_feedback(*TRIGGER, reanchor=True).set_measurement()
ctx["every"].set_feedback(0.0, 0.0, reanchor=True).set_measurement(noise_p=0.02, noise_v=0.05, seed=1)
modes = {name: (lambda d=d: d.transition(po, pf, KT, tol, histories=False, on_fail=on_fail)) for name, d in ctx.items()}
if other:
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L2 = C.CDLL(other)
    L2.dmpc_create.restype = C.c_void_p
    L2.dmpc_create.argtypes = [C.POINTER(_lib.DmpcParams), C.c_int, C.c_int]
    L2.dmpc_set_disturbance.argtypes = [C.c_void_p, C.POINTER(_lib.DmpcDisturbance)]
    L2.dmpc_set_feedback.argtypes = [C.c_void_p, C.POINTER(_lib.DmpcFeedback)]
    L2.dmpc_transition.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, C.c_int, C.c_double, dp, dp, dp, ip, ip]
    L2.dmpc_transition_hold.argtypes = _lib.load().dmpc_transition_hold.argtypes
    ctx2 = L2.dmpc_create(C.byref(ctx["feedback"].prm), 0, 0)
    assert ctx2
    desc, keep = _lib._disturbance(**NOISE)
    fbk = _lib.DmpcFeedback(TRIGGER[0], TRIGGER[1], 1)
    assert L2.dmpc_set_disturbance(ctx2, C.byref(desc)) == 0 and L2.dmpc_set_feedback(ctx2, C.byref(fbk)) == 0
    po_c, pf_c = np.ascontiguousarray(po, dtype=np.float64), np.ascontiguousarray(pf, dtype=np.float64)

    def run_other():
        used, sst = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        if on_fail == "hold":   # (one stage, no deadline, no path: Dmpc.transition(on_fail="hold")'s call)
            rc = L2.dmpc_transition_hold(ctx2, 1, N, N, 1, po_c.ctypes.data_as(dp), pf_c.ctypes.data_as(dp), ip(), dp(), 0, int(KT), float(tol), 14, dp(), dp(), dp(),
                                         used.ctypes.data_as(ip), sst.ctypes.data_as(ip), ip(), ip(), ip(), ip())
        else:
            rc = L2.dmpc_transition(ctx2, 1, N, po_c.ctypes.data_as(dp), pf_c.ctypes.data_as(dp), int(KT), float(tol), dp(), dp(), dp(), used.ctypes.data_as(ip),
                                    sst.ctypes.data_as(ip))
        assert rc == 0
        return dict(K_T_used=used, scene_status=sst)
    modes["other"] = run_other
cols, status = {}, {}
for name, f in modes.items():   # warm-up of every shape
    for _ in range(2):
        r = f()
    cols[name], status[name] = int(r["K_T_used"][0]) - 1, int(r["scene_status"][0])
events = {name: int(ctx[name].feedback_log(1, N)["event_count"].sum()) for name in ctx}
assert events["feedback"] == 0 and events["quiet"] == 0 and events["every"] == N * cols["every"], (events, cols)
assert cols["quiet"] == cols["feedback"] and status["quiet"] == status["feedback"]
t = {name: [] for name in modes}
for rep in range(reps):
    for name, f in modes.items():
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        t[name].append((time.perf_counter() - t0) / calls)
out = {"agents": N, "on_fail": on_fail, "columns": cols, "scene_status": status, "events": events, "repetitions": reps, "calls_per_timing": calls}
for name in modes:
    us = np.array(t[name]) / cols[name] * 1e6
    out[name] = {"median_us_per_column": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}
    print(f"{name:12s} {np.median(us):9.2f} us per column (min {us.min():.2f}, max {us.max():.2f}; {cols[name]} columns, status {status[name]}, {reps} x {calls} transitions)")
print(json.dumps(out))
