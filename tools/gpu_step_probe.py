"""development: one small call of every single-step entry, every output array dumped, for a comparison of two builds of the library.

  python tools/gpu_step_probe.py A.npz                                       (this build)
  python tools/with_lib.py OTHER.so tools/gpu_step_probe.py B.npz            (another build, in a process of its own)
  python tools/npz_equal.py A.npz B.npz

Rows: dmpc_init_batch, dmpc_step_batch, dmpc_step_batch_cmd and dmpc_solve_one on scenes of S = 2, N = 7, N_cmd = 5, variants bound (the reduced
solver) and hard, fp64 and mixed; dmpc_rows_one for bound, all3, hard (both sort branches), softall with order = 4, and scp; dmpc_step_device and
dmpc_step_device_cmd on torch tensors, both precisions, info given and null; dmpc_step_sharded_device as two ranks run in turn
(dmpc_debug_set_rank; N = 7: clusters of 4 and 3 agents, short_from = 1); dmpc_step_batch on a DMPC_DEVICE_ALL context over two emulated devices
with N = 7 and with N = 1 (fewer agents than GPUs: the first GPU alone).  The scenes are workload.make_scenes with a fixed seed in a box of
2 x 2 x 2 m, after init_batch: the straight lines cross, so agents carry rows.  The info arrays are keyed "<row>.info" like the others, so
npz_equal.py compares all eight words of every agent.  tools/gpu_launch_trace.py --step-entries runs the rows of single_context() under a kernel trace."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multiagent_planning_amd as mp   # noqa: E402
from multiagent_planning_amd import _lib, workload as wl   # noqa: E402

S, N, N_CMD, SEED = 2, 7, 5, 20261
CFG = dict(wl.CONFIGS["C2"], box=None, pmin=(-1.0, -1.0, 0.2), pmax=(1.0, 1.0, 2.2))
KW = wl.solver_kwargs(CFG, N)
PRECISIONS = ("f64", "mixed")


def scene(n=N):
    """po, pf [S,n,3], zeros of that shape, and the initDMPC rows l [S,n,45] of a context of its own"""
    po, pf = wl.make_scenes(CFG, S, n, seed=SEED)
    l, _, _ = mp.Dmpc("bound", **KW).init_batch(po, pf)
    return po, pf, np.zeros_like(po), l


def host_entries(variant, precision):
    po, pf, z, l = scene()
    d = mp.Dmpc(variant, precision=precision, **KW)
    l2, v2, a2 = d.init_batch(po, pf)
    yield "init_batch", dict(l=l2, v=v2, a=a2)
    yield "step_batch", d.step_batch(l, po, z, z, pf)
    c = slice(0, N_CMD)
    yield "step_batch_cmd", d.step_batch(l, po[:, c], z[:, c], z[:, c], pf[:, c])
    for n in (0, N - 1):
        r = d.solve_one(l[1], n, po[1, n], z[1, n], z[1, n], pf[1, n])
        yield f"solve_one_{n}", dict(r, status=np.int32(r["status"]))


def rows_one():
    po, pf, z, l = scene()
    for variant, kw in (("bound", {}), ("all3", {}), ("hard", {}), ("softall", dict(order=4)), ("scp", {})):
        d = mp.Dmpc(variant, **dict(KW, **kw))
        for n in range(N):
            r = d.rows_one(l[0], n, po[0, n], z[0, n])
            yield f"rows_one_{variant}_{n}", {k: np.asarray(v) for k, v in r.items()}


def device_entries(precision):
    import torch
    dev = torch.device("cuda", 0)
    po, pf, z, l = scene()
    lT = torch.from_numpy(np.ascontiguousarray(l.transpose(0, 2, 1))).to(dev)   # [S,45,N]
    for entry, n_cmd in (("step_device", N), ("step_device_cmd", N_CMD)):
        for with_info in (True, False):
            d = mp.Dmpc("bound", precision=precision, **KW)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, :n_cmd])).to(dev)
            xp, xv, xa, gf = t(po), t(z), t(z), t(pf)
            p = torch.zeros((S, n_cmd, 45), dtype=torch.float64, device=dev)
            v, a, nxt = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(lT)
            st = torch.zeros((S, n_cmd), dtype=torch.int32, device=dev)
            inf = torch.zeros((S, n_cmd, 8), dtype=torch.int32, device=dev)
            ptrs = (lT.data_ptr(), xp.data_ptr(), xv.data_ptr(), xa.data_ptr(), gf.data_ptr(), p.data_ptr(), v.data_ptr(), a.data_ptr(),
                    nxt.data_ptr(), st.data_ptr(), inf.data_ptr() if with_info else 0, torch.cuda.current_stream().cuda_stream)
            if entry == "step_device":
                d.step_device(S, 1, N, 0, *ptrs)
            else:
                d.step_device_cmd(S, N, n_cmd, *ptrs)
            torch.cuda.synchronize()
            out = dict(p=p, v=v, a=a, lT_next=nxt, status=st)
            if with_info:
                out["info"] = inf
            yield f"{entry}_{'info' if with_info else 'noinfo'}", {k: x.cpu().numpy() for k, x in out.items()}


def single_context():
    """the rows that enqueue on one stream of one context each"""
    for precision in PRECISIONS:
        for variant in ("bound", "hard"):
            for name, r in host_entries(variant, precision):
                yield f"{variant}_{precision}_{name}", r
        for name, r in device_entries(precision):
            yield f"{precision}_{name}", r
    yield from rows_one()


def sharded(precision):
    import torch
    dev = torch.device("cuda", 0)
    G = 2
    po, pf, z, l = scene()
    parts = [_lib.partition(N, G, r) for r in range(G)]
    cmax = parts[0][2]
    lT = np.zeros((G, S, 45, cmax))
    for r, (lo, cnt, _) in enumerate(parts):
        lT[r, :, :, :cnt] = l[:, lo:lo + cnt].transpose(0, 2, 1)
    lT_d = torch.from_numpy(lT).to(dev)
    L = _lib.load()
    L.dmpc_debug_set_rank.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for r, (lo, cnt, _) in enumerate(parts):
        d = mp.Dmpc("bound", precision=precision, **KW)
        assert L.dmpc_debug_set_rank(d._ctx, G, r) == 0
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, lo:lo + cnt])).to(dev)
        xp, xv, xa, gf = t(po), t(z), t(z), t(pf)
        p = torch.zeros((S, cnt, 45), dtype=torch.float64, device=dev)
        v, a, nxt = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(lT_d)
        st = torch.zeros((S, cnt), dtype=torch.int32, device=dev)
        inf = torch.zeros((S, cnt, 8), dtype=torch.int32, device=dev)
        d.step_sharded_device(S, N, lT_d.data_ptr(), xp.data_ptr(), xv.data_ptr(), xa.data_ptr(), gf.data_ptr(), p.data_ptr(), v.data_ptr(),
                              a.data_ptr(), nxt.data_ptr(), st.data_ptr(), inf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        yield f"{precision}_sharded_rank{r}", {k: x.cpu().numpy() for k, x in dict(p=p, v=v, a=a, lT_next=nxt, status=st, info=inf).items()}


def device_all(precision):
    mp.Dmpc.emulate_devices(2)
    try:
        for n in (N, 1):
            po, pf, z, l = scene(n)
            d = mp.Dmpc("bound", device=mp.Dmpc.DEVICE_ALL, precision=precision, **KW)
            assert d.n_devices == 2
            yield f"{precision}_device_all_N{n}", d.step_batch(l, po, z, z, pf)
    finally:
        mp.Dmpc.emulate_devices(0)


def rows():
    yield from single_context()
    for precision in PRECISIONS:
        yield from sharded(precision)
        yield from device_all(precision)


if __name__ == "__main__":
    out = {}
    for name, res in rows():
        arrays = {k: np.asarray(v) for k, v in res.items() if v is not None}
        out.update({f"{name}.{k}": v for k, v in arrays.items()})
        st = arrays.get("status")
        print(f"{name}: {len(arrays)} arrays" + (f", status {st.ravel().tolist()}" if st is not None else "") +
              (f", rows {int(arrays['nrows'])}" if "nrows" in arrays else ""), flush=True)
    np.savez(sys.argv[1], **out)
    print(f"{len(out)} arrays, {sum(v.size * v.itemsize // 4 for v in out.values())} 32-bit words -> {sys.argv[1]}")
