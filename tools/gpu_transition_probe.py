"""development: one small call per closed-loop entry and split path, every output array dumped, for a comparison of two builds of the library.

  python tools/gpu_transition_probe.py A.npz                                       (this build)
  python tools/with_lib.py OTHER.so tools/gpu_transition_probe.py B.npz            (another build, in a process of its own)
  python tools/npz_equal.py A.npz B.npz

Rows: dmpc_transition_sharded_gather as two ranks run in turn (dmpc_debug_set_rank; K_T_max = 2: the one step reads the first table, which every
rank builds whole -- without a transport the other rank's slots of the next table are never written); the five entries -- dmpc_transition, _cmd, _scripted, _mission,
_hold -- on one context; dmpc_transition and _mission in mixed precision; the five with split_parts = 3 (parts of 1, 2, 2 and 1, 1, 1 scenes) and
dmpc_postcheck on the histories the last of them left resident in its parts; a DMPC_DEVICE_ALL context over two emulated devices as one group and,
split_parts = 2, as two.  The scenes are those of tests/mission.py: four agents in a square, alone / beside two static / two scripted vehicles
(Q = 3, deadlines), and the wall crossing of eight agents and ten scripted vehicles in which an agent is held (max_hold = 2).
tools/gpu_launch_trace.py --closed-loop runs the rows of single_context() under a kernel trace."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiagent_planning_amd as mp   # noqa: E402
from multiagent_planning_amd import _lib   # noqa: E402
import mission as ms   # noqa: E402

KT, TOL = ms.KT, ms.ERROR_TOL
FIVE = ("reached", "deadline", "column0", "coincident", "reached"), (0, 0, 0, 0, 3)


def scenes():
    return dict(a=ms.batch(*FIVE), static=ms.batch(["static"] * 3, [0, 1, 2]), path=ms.batch(["path"] * 3, [0, 1, 2]),
                wall=ms.batch(["failure"] * 3, [1, 5, 0]))


def five_entries(d, sc, only=None):
    """(entry, result) of one call per entry on context d"""
    a, st, pa, w = sc["a"], sc["static"], sc["path"], sc["wall"]
    calls = dict(transition=lambda: d.transition(a["po"], a["goals"][:, 0], KT, TOL),
                 cmd=lambda: d.transition(st["po"], st["goals"][:, 0], KT, TOL),
                 scripted=lambda: d.transition(pa["po"], pa["goals"][:, 0], KT, TOL, path=pa["path"]),
                 mission=lambda: d.mission(a["po"], a["goals"], KT, TOL, deadline=a["deadline"]),
                 hold=lambda: d.mission(w["po"], w["goals"], KT, TOL, deadline=w["deadline"], path=w["path"], on_fail="hold", max_hold=2))
    for name in only or calls:
        yield name, calls[name]()


def single_context(sc):
    """the rows that enqueue on one stream: the five entries in fp64, dmpc_transition and _mission in mixed precision"""
    for name, r in five_entries(mp.Dmpc("bound", **ms.KW), sc):
        yield name, r
    for name, r in five_entries(mp.Dmpc("bound", precision="mixed", **ms.KW), sc, ("transition", "mission")):
        yield "mixed_" + name, r


def rows():
    sc = scenes()
    a = sc["a"]
    L = _lib.load()
    L.dmpc_debug_set_rank.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for r in range(2):
        d = mp.Dmpc("bound", **ms.KW)
        assert L.dmpc_debug_set_rank(d._ctx, 2, r) == 0
        d.nranks, d.rank = 2, r
        yield f"sharded_gather_rank{r}", d.transition_sharded(a["po"], a["goals"][:, 0], 2, TOL, gather=True)
    yield from single_context(sc)
    d = mp.Dmpc("bound", **ms.KW).debug_option("split_parts", 3)
    for name, r in five_entries(d, sc):
        yield "split3_" + name, r
    w = sc["wall"]
    yield "split3_postcheck", d.postcheck(r["K_T_used"], w["goals"][:, -1], KT_alloc=KT, path=w["path"])
    mp.Dmpc.emulate_devices(2)
    try:
        for parts in (1, 2):
            d = mp.Dmpc("bound", device=mp.Dmpc.DEVICE_ALL, **ms.KW)
            assert d.n_devices == 2
            if parts > 1:
                d.debug_option("split_parts", parts)
            yield f"device_all_{parts}", d.transition(a["po"], a["goals"][:, 0], KT, TOL)
    finally:
        mp.Dmpc.emulate_devices(0)


if __name__ == "__main__":
    out = {}
    for name, res in rows():
        arrays = {k: np.asarray(v) for k, v in res.items() if v is not None}
        out.update({f"{name}.{k}": v for k, v in arrays.items()})
        print(f"{name}: {len(arrays)} arrays, K_T_used {arrays['K_T_used'].tolist() if 'K_T_used' in arrays else '-'}", flush=True)
    np.savez(sys.argv[1], **out)
    print(f"{len(out)} arrays, {sum(v.size * v.itemsize // 4 for v in out.values())} 32-bit words -> {sys.argv[1]}")
