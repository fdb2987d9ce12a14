"""development: what a disturbance costs a batch -- wall time of one transition of 512 scenes of 100 agents (configs[3] shape, bound), closed loop
on the device: dmpc_transition with nothing set ("plain") and with a noise-only disturbance set ("noise", "noise_small": the post step is a launch
of its own and draws six uniforms per agent and column).  The modes are alternated within every repetition; each timing is a host clock around one whole
transition (a call ends in a stream synchronise).  Prints median, minimum and maximum per mode, and the columns the batch flew.
--other LIB: dmpc_transition of another build of the library (the parent commit's, say) as a third mode "other", loaded next to this one in the
same process and alternated with the rest.
usage: python tools/gpu_disturb_time.py [--other LIB.so] [repetitions [scenes]]"""
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
reps = int(args[0]) if len(args) > 0 else 9
S = int(args[1]) if len(args) > 1 else 512
cfg = wl.CONFIGS["C4"]
N = 100
kw = wl.solver_kwargs(cfg, N)
po, pf = wl.make_scenes(cfg, S, N, wl.SEED0 + 100)
KT, tol = cfg["K_T"], cfg["error_tol"]
d = mp.Dmpc("bound", **kw)
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
po_c, pf_c = np.ascontiguousarray(po, dtype=np.float64), np.ascontiguousarray(pf, dtype=np.float64)


def raw(L, ctx):   # dmpc_transition without histories, the same call for both builds
    def run():
        used, sst = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
        assert L.dmpc_transition(ctx, S, N, po_c.ctypes.data_as(dp), pf_c.ctypes.data_as(dp), int(KT), float(tol), dp(), dp(), dp(), used.ctypes.data_as(ip),
                                 sst.ctypes.data_as(ip)) == 0
        return dict(K_T_used=used, scene_status=sst)
    return run


def noisy(amp_p, amp_v):
    def run():
        d.set_disturbance(noise_p=amp_p, noise_v=amp_v, seed=1)
        try:
            return raw(d._L, d._ctx)()
        finally:
            d.clear_disturbance()
    return run


# "noise": 2 mm and 1 cm/s, more than error_tol lets a scene settle within, so every scene flies all K_T_max columns; "noise_small": 0.02 mm and
# 0.1 mm/s, the scenes end as the undisturbed ones do, so that the two columns counts are alike
modes = {"plain": raw(d._L, d._ctx), "noise": noisy(2e-3, 1e-2), "noise_small": noisy(2e-5, 1e-4)}
if other:
    L2 = C.CDLL(other)
    L2.dmpc_create.restype = C.c_void_p
    L2.dmpc_create.argtypes = [C.POINTER(_lib.DmpcParams), C.c_int, C.c_int]
    L2.dmpc_transition.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, C.c_int, C.c_double, dp, dp, dp, ip, ip]
    ctx2 = L2.dmpc_create(C.byref(d.prm), 0, 0)
    assert ctx2
    modes["other"] = raw(L2, ctx2)
cols = {}
for name, f in modes.items():   # warm-up of every shape
    for _ in range(2):
        r = f()
    cols[name] = dict(columns_max=int(r["K_T_used"].max()), columns_sum=int(r["K_T_used"].sum()), reached=int((r["scene_status"] == (1 | 256)).sum()))
if other:
    assert cols["other"] == cols["plain"], cols
t = {name: [] for name in modes}
for rep in range(reps):
    for name, f in modes.items():
        t0 = time.perf_counter()
        f()
        t[name].append((time.perf_counter() - t0) * 1e3)
out = {name: dict(ms_median=float(np.median(v)), ms_min=float(min(v)), ms_max=float(max(v)), **cols[name]) for name, v in t.items()}
print(json.dumps(dict(scenes=S, agents=N, K_T_max=int(KT), repetitions=reps, modes=out)))
