"""GPU: the cell geometry of the neighbour grid (option grid_cells) and the one-piece neighbour lists change which candidates the query looks
at and how the scan reads a list's length -- never which neighbours are listed, nor any arithmetic on them.  So every output word (p, v, a,
status, info, the next table) of every leg equals the whole-table walk's (option no_cull), over three closed-loop MPC steps on the device:

  legs     the default geometry; grid_cells = 0 (the cells of rounds 4-6) and every other offered row; nbr_grid = 0 (nbr_kernel: lists in
           sixteen pieces, the scan closes the gaps); close_pairs = 0 (the scan walks its one-piece list for the pairs inside rmin);
  scenes   one scene of 1 024 agents (the grid in two launches), two scenes of 800 (the five kernels), a grid just under and just over the
           two-launch build's limit, and the adversarial tables of tests/gridcases.py (their facts are asserted in
           tests/test_grid_geometry_cpu.py): candidate totals of 64, 65, 128, 129, queries of 361 runs, an axis at the cap of 64, one cell
           along z, a list of exactly the capacity and of one more (count -1: the scan walks the table);
  variants bound, hard, all3 in fp64 and in mixed precision (compared with their own walk)."""
import functools

import numpy as np
import pytest

import gridcases as gc
import multiagent_planning_amd as mp

pytestmark = pytest.mark.gpu

KEYS = ("status", "info", "p", "v", "a", "next")
VARIANTS = [(v, p) for v in ("bound", "hard", "all3") for p in ("f64", "mixed")]
SMALL = dict(cull_min=64, grid_min=64)      # scenes of 64 - 300 agents take the list paths
SCENES = {"c4-1x1024": (lambda hard: gc.c4_scene(1, 1024, 72), {}), "c4-2x800": (lambda hard: gc.c4_scene(2, 800, 73), {})}
for _name, _build in gc.CASES.items():
    SCENES[_name] = (_build, dict(SMALL, list_cap=gc.LIST_CAP) if _name.startswith("capacity") else SMALL)


@functools.lru_cache(maxsize=None)
def _scene(name, hard):
    return SCENES[name][0](hard)


def _loop(variant, precision, case, nsteps, **opts):
    """closed-loop steps on the device from the case's table: dmpc_step_device + dmpc_advance_device + the table swap; every output of every step"""
    import torch
    kw, l, xp, xv, xa, pf, _ = case
    S, N = l.shape[0], l.shape[1]
    d = mp.Dmpc(variant, precision=precision, **kw)
    for k_, v_ in opts.items():
        d.debug_option(k_, v_)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.float64)
    rows = t(l)
    tab = [torch.empty((1, S, 45, N), dtype=torch.float64, device=dev) for _ in range(2)]
    d.table_from_rows_device(S, 1, N, rows.data_ptr(), tab[0].data_ptr(), st)
    x = [t(xp), t(xv), t(xa)]
    goal = t(pf)
    o = [torch.empty((S, N, 45), dtype=torch.float64, device=dev) for _ in range(3)]
    status = torch.zeros((S, N), dtype=torch.int32, device=dev)
    info = torch.zeros((S, N, 8), dtype=torch.int32, device=dev)
    outs, cur = [], 0
    for _ in range(nsteps):
        tab[cur ^ 1].zero_()
        d.step_device(S, 1, N, 0, tab[cur].data_ptr(), x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), goal.data_ptr(), o[0].data_ptr(), o[1].data_ptr(),
                      o[2].data_ptr(), tab[cur ^ 1].data_ptr(), status.data_ptr(), info.data_ptr(), st)
        d.advance_device(S * N, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), status.data_ptr(), x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), st)
        torch.cuda.synchronize()
        outs.append(dict(status=status.cpu().numpy(), info=info.cpu().numpy(), p=o[0].cpu().numpy(), v=o[1].cpu().numpy(), a=o[2].cpu().numpy(),
                         next=tab[cur ^ 1].cpu().numpy()))
        cur ^= 1
    return outs


@pytest.mark.parametrize("variant,precision", VARIANTS)
@pytest.mark.parametrize("name", list(SCENES))
def test_every_geometry_and_list_form_gives_the_walks_outputs(name, variant, precision):
    case = _scene(name, variant == "hard")
    base = SCENES[name][1]
    walk = _loop(variant, precision, case, 3, no_cull=1)
    legs = [("default geometry", base)]
    legs += [(f"grid_cells={g}", dict(base, grid_cells=g)) for g in gc.OFFERED if g != gc.DEFAULT]
    legs += [("nbr_grid=0", dict(base, nbr_grid=0)), ("close_pairs=0", dict(base, close_pairs=0))]
    for leg, opts in legs:
        got = _loop(variant, precision, case, 3, **opts)
        for step, (g, w) in enumerate(zip(got, walk)):
            for k in KEYS:
                if not np.array_equal(g[k], w[k]):
                    bad = np.argwhere((g["status"] != w["status"]) | (g["info"] != w["info"]).any(-1) | (g["p"] != w["p"]).any(-1))
                    raise AssertionError(f"{name} {variant}/{precision} leg '{leg}', step {step}: {k} differs from the walk; first (scene, agent) {bad[:3].tolist()}")
    assert any((w["info"][..., 1] > 0).any() for w in walk), name      # rows were built
    assert all((w["next"] != 0).any() for w in walk), name             # the next table was written
