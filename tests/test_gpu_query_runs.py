"""GPU: the fetch of grid_query_kernel -- from a lane's position in a batch's candidate sequence to its run -- on the run structures of
tests/querycases.py (their facts are asserted on the CPU in tests/test_query_runs_cpu.py): one run of 1, 63, 64, 65, 128, 129 and 300
candidates, exactly 64 and 65 runs, hundreds of runs nearly all empty, empty runs first, last, in a row, everywhere but last, a whole batch
empty, runs that start at positions 63, 64 and 65, a sequence longer than the fetch's bit window, a batch of scenes, two ranks.

Per case, one MPC step of solveSoftDMPCbound from the case's table, the list paths taken through cull_min = grid_min = 64:

* lists against brute force: every agent's list (Dmpc.debug_read_grid: nbr_cnt, nbr_list) is, in increasing order, exactly the set
  {j != i : some horizon step's scaled distance < selection radius}, computed in fp64 -- exact, because no pair of these scenes is near the
  radius (nor between it and the query's own, 1e-3 wider one);
* outputs against the walk: status, info, p, v, a of every grid leg equal the whole-table walk's (option no_cull) word for word; the legs
  are those of tests/test_gpu_nbr_adversarial.py.  The fp64 walk itself is tied to the oracle there."""
import ctypes as C
import functools

import numpy as np
import pytest

import multiagent_planning_amd as mp
from multiagent_planning_amd import _lib
import nbrcases as nc
import querycases as qc
import test_gpu_paths as paths

pytestmark = pytest.mark.gpu

KEYS = ("status", "info", "p", "v", "a")
GRID = dict(cull_min=64, grid_min=64)


@functools.lru_cache(maxsize=None)
def _sets(name):
    """per scene the fp64 neighbour relation [N, N]"""
    kw, l, *_ = qc.case(name)
    return [qc.near(l[s], kw["c"], nc.rsel_of(kw)) for s in range(l.shape[0])]


def _step(case, scenes, keep=None, **opts):
    kw, l, xp, xv, xa, pf, _ = case
    return paths._steps("bound", kw, np.ascontiguousarray(xp[scenes]), np.ascontiguousarray(pf[scenes]), 1, "f64",
                        table=np.ascontiguousarray(l[scenes]), keep=keep, **opts)[0]


def _lists_are_the_sets(name, leg, g, sets, index_of=lambda code: code):
    """g: debug_read_grid of a query over len(sets) scenes; sets[s]: [agents of the scene queried, N] bool"""
    assert g["build"] in (1, 2), (name, leg, g["build"])          # the cell grid, not the all-pairs test
    per = g["agents"] // len(sets)
    for s, want in enumerate(sets):
        assert want.shape[0] == per
        for i in range(per):
            cnt = int(g["nbr_cnt"][s * per + i, 0])
            exp = np.nonzero(want[i])[0]
            got = index_of(g["nbr_list"][s * per + i, :max(cnt, 0)])
            assert cnt == len(exp) and np.array_equal(got, exp), \
                f"{name} leg '{leg}' scene {s} agent {i}: list of {cnt}, expected {len(exp)}; missing {sorted(set(exp) - set(got))[:8]}, extra {sorted(set(got) - set(exp))[:8]}"


def _same(name, leg, got, want):
    for k in KEYS:
        if not np.array_equal(got[k], want[k]):
            g, w = got[k].reshape(got["status"].shape + (-1,)), want[k].reshape(want["status"].shape + (-1,))
            raise AssertionError(f"{name} leg '{leg}': {k} differs from the walk, first (scene, agent) {np.argwhere((g != w).any(-1))[:3].tolist()}")


@pytest.mark.parametrize("name", list(qc.CASES))
def test_lists_are_the_brute_force_sets_and_outputs_the_walks(name):
    case = qc.case(name)
    S = case[1].shape[0]
    every = slice(0, S)
    sets = _sets(name)
    walk = _step(case, every, no_cull=1)
    legs = [("grid, batch", every, GRID)]
    for s in range(S):
        legs += [(f"grid, scene {s} alone", slice(s, s + 1), GRID), (f"grid, scene {s} alone, prep_fuse=0", slice(s, s + 1), dict(GRID, prep_fuse=0))]
    legs += [("no close pairs", every, dict(GRID, close_pairs=0)), ("close cap", every, dict(GRID, close_cap=1))]
    for leg, scenes, opts in legs:
        keep = []
        got = _step(case, scenes, keep=keep, **opts)
        _lists_are_the_sets(name, leg, keep[0].debug_read_grid(), sets[scenes])
        _same(name, leg, got, {k: walk[k][scenes] for k in KEYS})
    assert (walk["info"][..., 1] > 0).any(), name      # rows were built


def test_two_ranks_of_a_129_agent_scene_in_turn():
    """chunks of 65 and 64 agents (the second one's last column is padding), each rank's query against the rank-major table"""
    import torch
    name = qc.RANKS
    kw, l, xp, xv, xa, pf, _ = qc.case(name)
    S, N, G = l.shape[0], l.shape[1], 2
    assert N == 129
    near = _sets(name)
    dev = torch.device("cuda", 0)
    parts = [_lib.partition(N, G, r) for r in range(G)]
    assert [p[1] for p in parts] == [65, 64]
    cmax = parts[0][2]
    lT = np.zeros((G, S, 45, cmax))
    for r, (lo, cnt, _) in enumerate(parts):
        lT[r, :, :, :cnt] = l[:, lo:lo + cnt].transpose(0, 2, 1)
    lT_d = torch.from_numpy(lT).to(dev)
    L = _lib.load()
    L.dmpc_debug_set_rank.argtypes = [C.c_void_p, C.c_int, C.c_int]
    first = np.array([p[0] for p in parts])
    rows = 0
    for r, (lo, cnt, _) in enumerate(parts):
        res = []
        for opts in (dict(GRID, grid_min_part=64), dict(no_cull=1)):
            d = mp.Dmpc("bound", **kw).debug_watch_grid()
            for k_, v_ in opts.items():
                d.debug_option(k_, v_)
            assert L.dmpc_debug_set_rank(d._ctx, G, r) == 0
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, lo:lo + cnt])).to(dev)
            x, v, a, gf = t(xp), t(xv), t(xa), t(pf)
            p = torch.zeros((S, cnt, 45), dtype=torch.float64, device=dev); vo, ao = torch.zeros_like(p), torch.zeros_like(p)
            st = torch.zeros((S, cnt), dtype=torch.int32, device=dev); inf = torch.zeros((S, cnt, 8), dtype=torch.int32, device=dev)
            nxt = torch.zeros_like(lT_d)
            d.step_sharded_device(S, N, lT_d.data_ptr(), x.data_ptr(), v.data_ptr(), a.data_ptr(), gf.data_ptr(), p.data_ptr(), vo.data_ptr(), ao.data_ptr(),
                                  nxt.data_ptr(), st.data_ptr(), inf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res.append(dict(status=st.cpu().numpy(), info=inf.cpu().numpy(), p=p.cpu().numpy(), v=vo.cpu().numpy(), a=ao.cpu().numpy()))
            if "no_cull" not in opts:
                _lists_are_the_sets(name, f"rank {r}", d.debug_read_grid(), [near[s][lo:lo + cnt] for s in range(S)],
                                    index_of=lambda code: first[code >> 20] + (code & 0xfffff))
        _same(name, f"rank {r}", res[0], res[1])
        rows += int((res[0]["info"][..., 1] > 0).sum())
    assert rows > 0
