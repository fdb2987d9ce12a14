"""GPU: the neighbour grid itself.  The list tests compare a step's outputs with the whole-table walk, and a build that makes boxes, half
extents or deviations too LARGE still yields supersets and passes them all; these tests read what the build left on the device
(Dmpc.debug_read_grid) after ONE MPC step of solveSoftDMPCbound and compare it with fp64 numpy (tests/gridbuild.py).

Scenes (tests/gridbuild.py: SCENES; their facts are asserted in tests/test_grid_build_cpu.py): 32, 216, 242, 10 920, 11 180 and 19 968 cells,
one cell along z, clamped cells beyond every face, the two-launch build's last size and the first of the five kernels, the fp32 table of
mixed precision; 300 and 260 agents, so grid_prep_kernel runs two blocks, the second a tail.  Legs per scene, cull_min = grid_min = 64: every
scene alone with prep_fuse = 1 and with prep_fuse = 0, and the batch of its scenes (five kernels).

The two-launch build's counters -- cell counts AND largest half extents -- are set back to zero by the step's own scan kernel for the next
step's grid_prep_kernel (StepParams::gzero).  A context on which dmpc_debug_read_grid has been called keeps a copy of the half extents, made right
after grid_prep_kernel / grid_bin_kernel (Dmpc.debug_watch_grid before the step; test_gpu_paths._steps arms the contexts it hands out), so
both builds' half extents are read as the build left them; a context that was not armed shows the zeros (the refusal test at the end).

Tolerances.  Boxes: none -- each bound is the fp64 extreme rounded outwards to fp32.  Half extents: the stored m is
0.5f * (hi - lo) * 1.0001f + 1e-5f of the rounded-out fp32 bounds, so m >= h (the margin of 1e-4 h + 1e-5 is far above the three fp32 roundings
of the expression, 2e-7 relative) and m <= 1.0001 h' + 1e-5 with h' <= h + one fp32 ulp of each bound (at most 8e-6 in all at 40 m):
h <= m <= 1.0002 h + 2e-5.  Chord records: code, first step and last minus first are fp32 operations on the table's words -- exact (x, y: one
subtraction; z: hipcc contracts the product z * (1 / c) of the last step and the subtraction into ONE fma, -ffp-contract=fast, so the expected word is
fl(z_last * e - fl(z_first * e)), which differs from two roundings only when 1 / c is no power of two: metric-1); the deviation d = sqrtf(dev2) * 1.0001f + 1e-5f, where dev2 comes from fp32 words (relative 6e-8 of coordinates up to 40 m: 2.4e-6 per
coordinate, a few times that after the interpolation and the norm, below the 1e-5 + 1e-4 delta margin): delta <= d <= 1.0002 delta + 2e-5.
Cells: fp32 (x - org) * inv is good to 1e-5 cell widths in these workspaces; centres within 1e-4 of an interior boundary are left out."""
import functools

import numpy as np
import pytest

import gridbuild as gb
import gridcases as gc
import nbrcases as nc
import test_gpu_paths as paths

pytestmark = pytest.mark.gpu

NAMES = list(gb.SCENES)
EXACT = ("bbox", "maxhalf", "start")


@functools.lru_cache(maxsize=None)
def _legs(name):
    """(case, precision, [(fused, five) per scene alone], batch or None): one step per leg, the grid read after it"""
    build, precision, _ = gb.SCENES[name]
    case = build()
    kw, l, xp, xv, xa, pf, _ = case

    def leg(sl, fuse):
        keep = []
        paths._steps("bound", kw, xp[sl], pf[sl], 1, precision, table=l[sl], keep=keep, cull_min=64, grid_min=64, prep_fuse=fuse)
        g = keep[0].debug_read_grid()
        g["canon"] = gb.canonical(g)
        return g
    S = l.shape[0]
    alone = [(leg(slice(s, s + 1), 1), leg(slice(s, s + 1), 0)) for s in range(S)]
    return case, precision, alone, (leg(slice(0, S), 0) if S > 1 else None)


def _scenes(name):
    """(kw, the scene's table as the builders read it, the scene-alone grid of the first build, of the five kernels) per scene"""
    (kw, l, *_), precision, alone, _ = _legs(name)
    return [(kw, gb.source(l[s], precision), alone[s][0], alone[s][1]) for s in range(l.shape[0])]


@pytest.mark.parametrize("name", NAMES)
def test_fused_build_equals_the_five_kernels(name):
    (kw, l, *_), _, alone, _ = _legs(name)
    for s, (f, u) in enumerate(alone):
        n = np.array(f["n"])
        assert f["ncell"] == gb.SCENES[name][2] == int(n.prod()) and (f["S"], f["G"], f["C"]) == (1, 1, l.shape[1])
        assert f["build"] == (2 if gc.fused(n) else 1) and u["build"] == 1, (name, f["build"], u["build"])
        for k in EXACT:
            assert f[k].tobytes() == u[k].tobytes(), (name, s, k)
        assert np.array_equal(f["canon"], u["canon"]), (name, s)


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("limit")])
def test_batch_equals_its_scenes_alone(name):
    _, _, alone, batch = _legs(name)
    assert batch["build"] == 1 and batch["S"] == len(alone) == 2
    for s, (_, u) in enumerate(alone):
        assert batch["bbox"][:, s].tobytes() == u["bbox"][:, 0].tobytes(), (name, s)
        assert batch["maxhalf"][s].tobytes() == u["maxhalf"][0].tobytes(), (name, s)
        assert batch["start"][s].tobytes() == u["start"][0].tobytes(), (name, s)
        assert np.array_equal(batch["canon"][:, s], u["canon"][:, 0]), (name, s)


@pytest.mark.parametrize("name", NAMES)
def test_boxes_are_the_fp64_extremes_rounded_outwards(name):
    for s, (kw, l, g, u) in enumerate(_scenes(name)):
        assert g["bbox"][0, 0].tobytes() == gb.bbox(l).tobytes() and u["bbox"][0, 0].tobytes() == gb.bbox(l).tobytes(), (name, s)


@pytest.mark.parametrize("name", NAMES)
def test_half_extents_cover_and_do_not_grow(name):
    for s, (kw, l, f, u) in enumerate(_scenes(name)):
        h = gb.half_extents(l)
        for leg, g in (("first build", f), ("five kernels", u)):
            m = g["maxhalf"][0].astype(np.float64)
            print(f"{name} scene {s} {leg} (build {g['build']}): largest m - h {float((m - h).max()):.3e}, smallest {float((m - h).min()):.3e}, largest m - (1.0002 h + 2e-5) {float((m - 1.0002 * h - 2e-5).max()):.3e}")
            assert (h <= m).all() and (m <= 1.0002 * h + 2e-5).all(), (name, s, leg, h, m)


@pytest.mark.parametrize("name", NAMES)
def test_every_column_once_per_segment_in_its_fp64_cell(name):
    for s, (kw, l, g, _) in enumerate(_scenes(name)):
        N = l.shape[0]
        n, cell, near = gb.cells(kw, l)
        assert tuple(n) == g["n"]
        assert near.any(axis=1).mean() <= gb.NEAR_SHARE_MAX
        for sg in range(nc.NSEG):
            st = g["start"][0, sg]
            code = g["ent"][0, 0, sg, :, 0].view(np.int32)
            assert np.array_equal(np.sort(code), np.arange(N)), (name, s, sg)          # every column once (one chunk: code = column)
            got = np.empty(N, dtype=np.int64)
            got[code] = gb.record_cells(st, N)
            ok = near[:, sg] | (got == cell[:, sg])
            assert ok.all(), (name, s, sg, np.nonzero(~ok)[0][:5], got[~ok][:5], cell[~ok, sg][:5])
            # the prefix: start must be the exclusive prefix of the counts of the FP64 cells (an independent count: `got` was read off start itself
            # and enters only for the few centres left out of the cell check, whose fp32 cell may be the neighbouring one)
            counts = np.bincount(np.where(near[:, sg], got, cell[:, sg]), minlength=g["ncell"])
            assert st[0] == 0 and st[-1] == N and np.array_equal(st[1:], np.cumsum(counts)), (name, s, sg)


@pytest.mark.parametrize("name", NAMES)
def test_chord_records(name):
    for s, (kw, l, g, _) in enumerate(_scenes(name)):
        a0, da = gb.chords(l, kw["c"])
        delta = gb.deviations(l, kw["c"])
        for sg in range(nc.NSEG):
            r0, r1 = g["ent"][0, 0, sg], g["ent"][1, 0, sg]
            col = r0[:, 0].view(np.int32)
            assert r0[:, 1:].tobytes() == a0[col, sg].tobytes(), (name, s, sg, "first step")
            assert r1[:, :3].tobytes() == da[col, sg].tobytes(), (name, s, sg, "last minus first")
            d, dl = r1[:, 3].astype(np.float64), delta[col, sg]
            print(f"{name} scene {s} segment {sg}: smallest d - delta {float((d - dl).min()):.3e}, largest d - (1.0002 delta + 2e-5) {float((d - 1.0002 * dl - 2e-5).max()):.3e}")
            assert (dl <= d).all() and (d <= 1.0002 * dl + 2e-5).all(), (name, s, sg)


def test_read_grid_is_refused_before_a_list_build_and_with_a_small_buffer():
    import ctypes as C
    import multiagent_planning_amd as mp
    kw, l, xp, xv, xa, pf, _ = nc.metric(2)
    d = mp.Dmpc("bound", **kw)
    with pytest.raises(mp.DmpcError, match="no step of this context has built neighbour lists"):
        d.debug_read_grid()
    d = mp.Dmpc("bound", **kw)      # (a context nobody has called the entry on: not armed)
    d.debug_option("cull_min", 64).debug_option("grid_min", 64)
    d.step_batch(l[:1], xp[:1], xv[:1], xa[:1], pf[:1])
    g = d.debug_read_grid()
    assert g["build"] == 2 and not g["maxhalf"].any() and g["start"][0, 0, -1] == l.shape[1]      # the scan kernel has set the half extents back
    d.step_batch(l[:1], xp[:1], xv[:1], xa[:1], pf[:1])      # armed by that read: the copy is kept from now on
    assert d.debug_read_grid()["maxhalf"].all()
    d.step_batch(l, xp, xv, xa, pf)
    shape = np.zeros(12, dtype=np.int32)
    buf = np.zeros(16, dtype=np.int32)
    assert d._L.dmpc_debug_read_grid(d._ctx, shape.ctypes.data_as(C.POINTER(C.c_int32)), buf.ctypes.data_as(C.c_void_p), buf.nbytes) == -1
    assert b"too small" in d._L.dmpc_last_error(d._ctx)
    assert d.debug_read_grid()["build"] == 1
