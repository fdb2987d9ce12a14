"""development: one MPC step per leg on the list paths of large scenes, the step's outputs and everything dmpc_debug_read_grid reads dumped,
for a comparison of two builds of the library.

  python tools/gpu_lists_probe.py A.npz                                       (this build)
  python tools/with_lib.py OTHER.so tools/gpu_lists_probe.py B.npz            (another build, in a process of its own)
  python tools/npz_equal.py A.npz B.npz

Legs (solveSoftDMPCbound, cull_min = grid_min = grid_min_part = 64):
  scenes   every scene of tests/gridbuild.py: the batch of its scenes, and its first scene alone with prep_fuse = 1 and prep_fuse = 0;
  options  metric-1 with nbr_grid = 0 (nbr_kernel: no cell grid, lists in sixteen pieces), outside with close_pairs = 0;
  ranks    the two emulated ranks of rounds-129 (chunks of 65 and 64 agents: the second one's last column is padding) in turn.
What the device leaves unordered or unwritten is put in a canonical form first: entry records sorted by code inside each cell, close pairs sorted
per agent, and zeros behind the last record of a cell grid, behind a list's count, in the count slots a one-piece list does not use and in the
padding column of a short chunk's next table."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiagent_planning_amd as mp   # noqa: E402
from multiagent_planning_amd import _lib   # noqa: E402
import gridbuild as gb   # noqa: E402
import nbrcases as nc   # noqa: E402
import test_gpu_paths as paths   # noqa: E402

SMALL = dict(cull_min=64, grid_min=64, grid_min_part=64)


def grid_arrays(d):
    """the canonical form of what the context's last list build left"""
    g = d.debug_read_grid()
    out = {k: np.array(g[k]) for k in ("S", "G", "C", "n", "ncell", "build", "cap", "close_cap", "agents", "parts")}
    out.update(bbox=g["bbox"], maxhalf=g["maxhalf"], start=g["start"], ent=gb.canonical(g))
    cnt, lst = g["nbr_cnt"].copy(), g["nbr_list"].copy()
    pieces = 1 if g["build"] else g["parts"]
    cnt[:, pieces:] = 0
    pcap = g["cap"] // pieces
    for q in range(pieces):
        n = np.where(cnt[:, q] < 0, pcap, cnt[:, q])
        lst[:, q * pcap:(q + 1) * pcap][np.arange(pcap)[None, :] >= n[:, None]] = 0
    out.update(nbr_cnt=cnt, nbr_list=lst)
    if g["close_cap"]:
        cl = g["close_list"].copy()
        n = np.maximum(g["close_cnt"], 0)
        big = np.iinfo(np.int32).max
        cl[np.arange(g["close_cap"])[None, :] >= n[:, None]] = big      # (unwritten records behind every written one, then zeroed)
        order = np.lexsort((cl[..., 1], cl[..., 0]), axis=-1)
        cl = np.take_along_axis(cl, order[..., None], axis=1)
        cl[cl == big] = 0
        out.update(close_cnt=g["close_cnt"], close_list=cl)
    return out


def step_leg(case, precision, sl, **opts):
    kw, l, xp, xv, xa, pf, _ = case
    keep = []
    o = paths._steps("bound", kw, xp[sl], pf[sl], 1, precision, table=l[sl], keep=keep, **dict(SMALL, **opts))[0]
    return dict(o, **grid_arrays(keep[0]))


def rank_legs():
    import torch
    kw, l, xp, xv, xa, pf, _ = nc.rounds(129)
    S, N, G = l.shape[0], l.shape[1], 2
    dev = torch.device("cuda", 0)
    parts = [_lib.partition(N, G, r) for r in range(G)]
    cmax = parts[0][2]
    lT = np.zeros((G, S, 45, cmax))
    for r, (lo, cnt, _) in enumerate(parts):
        lT[r, :, :, :cnt] = l[:, lo:lo + cnt].transpose(0, 2, 1)
    lT_d = torch.from_numpy(lT).to(dev)
    L = _lib.load()
    L.dmpc_debug_set_rank.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for r, (lo, cnt, _) in enumerate(parts):
        d = mp.Dmpc("bound", **kw).debug_watch_grid()
        for k, v in SMALL.items():
            d.debug_option(k, v)
        assert L.dmpc_debug_set_rank(d._ctx, G, r) == 0
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, lo:lo + cnt])).to(dev)
        x, v, a, gf = t(xp), t(xv), t(xa), t(pf)
        p = torch.zeros((S, cnt, 45), dtype=torch.float64, device=dev); vo, ao = torch.zeros_like(p), torch.zeros_like(p)
        st = torch.zeros((S, cnt), dtype=torch.int32, device=dev); inf = torch.zeros((S, cnt, 8), dtype=torch.int32, device=dev)
        nxt = torch.zeros_like(lT_d)
        d.step_sharded_device(S, N, lT_d.data_ptr(), x.data_ptr(), v.data_ptr(), a.data_ptr(), gf.data_ptr(), p.data_ptr(), vo.data_ptr(), ao.data_ptr(),
                              nxt.data_ptr(), st.data_ptr(), inf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        nxt[r, :, :, cnt:] = 0      # (the padding column of a short chunk's next table is undefined: it differs between two runs of one build)
        yield f"rounds-129.rank{r}", dict(status=st.cpu().numpy(), info=inf.cpu().numpy(), p=p.cpu().numpy(), v=vo.cpu().numpy(), a=ao.cpu().numpy(),
                                           nxt=nxt[r].cpu().numpy(), **grid_arrays(d))


def rows():
    for name, (build, precision, _) in gb.SCENES.items():
        case = build()
        S = case[1].shape[0]
        yield f"{name}.batch", step_leg(case, precision, slice(0, S))
        yield f"{name}.alone_fused", step_leg(case, precision, slice(0, 1), prep_fuse=1)
        yield f"{name}.alone_five", step_leg(case, precision, slice(0, 1), prep_fuse=0)
    yield "metric-1.nbr_grid0", step_leg(nc.metric(1), "f64", slice(0, 2), nbr_grid=0)
    yield "outside.close_pairs0", step_leg(nc.outside(), "f64", slice(0, 2), close_pairs=0)
    yield from rank_legs()


if __name__ == "__main__":
    out = {}
    for name, res in rows():
        out.update({f"{name}.{k}": np.asarray(v) for k, v in res.items()})
        print(f"{name}: build {int(res['build'])}, {int(res['ncell'])} cells, lists of up to {int(np.abs(res['nbr_cnt']).max())} entries, rows built by {int((res['info'][..., 1] > 0).sum())} agents", flush=True)
    np.savez(sys.argv[1], **out)
    print(f"{len(out)} arrays, {sum(v.size * v.itemsize // 4 for v in out.values())} 32-bit words -> {sys.argv[1]}")
