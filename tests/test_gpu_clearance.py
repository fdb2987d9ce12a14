"""GPU: the clearance report (dmpc_postcheck_clearance, Dmpc.clearance) -- per commanded agent the nearest commanded partner (slot 0) and the
nearest uncommanded vehicle (slot 1) over the 100 Hz samples of the post-check, and when.

The reference is numpy's all-pairs search over the library's own interpolated positions (postcheck(interp=True): `p`, `p_scripted`), which
tests/test_gpu_postcheck.py and tests/test_gpu_scripted.py hold to the oracle.  Bars (tests/clearance.py): distances within 8 ulp of the
CPU value (two FMAs against three roundings); the reported (partner, sample) must be a pair that IS that close while no other is closer;
the per-scene minima must equal min_dist / min_dist_static / min_dist_scripted of the existing post-checks as bytes."""
import numpy as np
import pytest

import multiagent_planning_amd as mp
from multiagent_planning_amd import workload as wl
import clearance as cl
import mission as ms
import scripted as sc

pytestmark = pytest.mark.gpu

KEYS = ("dist", "partner", "sample")


def _same(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _err(d):
    return d._L.dmpc_last_error(d._ctx).decode()


def _bytes_equal(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _anchors(rep, pc, s, extra=None):
    """min over the agents of a scene == what the existing post-checks report for the scene, as bytes"""
    assert _bytes_equal(rep["dist"][s, :, 0].min(), pc["min_dist"][s]), (s, rep["dist"][s, :, 0].min(), pc["min_dist"][s])
    if extra:
        assert _bytes_equal(rep["dist"][s, :, 1].min(), pc[extra][s]), (s, extra, rep["dist"][s, :, 1].min(), pc[extra][s])
    else:
        assert np.isposinf(rep["dist"][s, :, 1]).all() and (rep["partner"][s, :, 1] == -1).all() and (rep["sample"][s, :, 1] == -1).all()


# ---- 1, 2, 5: a small batch with every kind of vehicle ----------------------------------------------------------------------------------------
USED = np.array([6, 9, 12], dtype=np.int32)
MASK = np.array([1, 0, 1], dtype=np.int32)
KT_SMALL = 12


@pytest.fixture(scope="module")
def small():
    """S = 3 scenes of 5 commanded agents: a transition cut off at 12 columns leaves its histories resident; the post-checks read 6, 9 and 12
    columns of them.  3 static vehicles / 2 scripted ones with P = 4 stand next to the agents' ways (the planner never saw them: only the
    check is under test)."""
    cfg, N = wl.CONFIGS["C4"], 5
    kw = wl.solver_kwargs(cfg, N)
    po, pf = wl.make_scenes(cfg, 3, N=N)
    d = mp.Dmpc(cfg["variant"], **kw)
    tr = d.transition(po, pf, KT_SMALL)
    assert (tr["K_T_used"] == KT_SMALL).all()
    rng = np.random.default_rng(8)
    mid = 0.5 * (po + pf)
    pos = mid[:, :3] + rng.uniform(-0.3, 0.3, (3, 3, 3))
    path = mid[:, 3:5, None, :] + np.cumsum(rng.uniform(-0.15, 0.15, (3, 2, 4, 3)), axis=2)
    return dict(d=d, kw=kw, pf=pf, hist=(tr["pk"], tr["vk"], tr["ak"]), pos=pos, path=path)


@pytest.mark.parametrize("kind", ["alone", "static", "scripted"])
def test_small_scene_all_kinds(small, kind):
    """cases 1 and 2: against numpy on every agent and slot; resident histories == host histories; the masked scene reports NaN / -1 / -1;
    the per-scene minima are the existing post-checks' as bytes; a finite reach empties exactly the slots beyond it"""
    d, pf, hist = small["d"], small["pf"], small["hist"]
    extra = dict(alone={}, static=dict(po_static=small["pos"]), scripted=dict(path=small["path"]))[kind]
    host = d.clearance(USED, pf, *hist, mask=MASK, **extra)
    res = d.clearance(USED, pf, KT_alloc=KT_SMALL, mask=MASK, **extra)
    _same(res, host, "resident / host histories")
    assert host["dist"].shape == (3, 5, 2) and host["partner"].dtype == np.int32 and host["sample"].dtype == np.int32
    assert np.isnan(host["dist"][1]).all() and (host["partner"][1] == -1).all() and (host["sample"][1] == -1).all() and np.isnan(host["time"][1]).all()
    pc = d.postcheck(USED, pf, *hist, interp=True, mask=MASK, **extra)
    key = dict(alone=None, static="min_dist_static", scripted="min_dist_scripted")[kind]
    c = small["kw"]["c"]
    near = cl.REACH3 if kind == "alone" else 0.9
    cut = d.clearance(USED, pf, *hist, mask=MASK, reach=near, **extra)
    for s in (0, 2):
        n = int(pc["n_samples"][s])
        p = pc["p"][s][:, :n]
        q = None if kind == "alone" else (pc["p_scripted"][s][:, :n] if kind == "scripted" else np.repeat(small["pos"][s][:, None], n, axis=1))
        filled, empty = cl.check_scene(host["dist"][s], host["partner"][s], host["sample"][s], p, q, c)
        assert filled == (10 if q is not None else 5) and empty == 10 - filled
        assert np.array_equal(host["time"][s][host["sample"][s] >= 0], host["sample"][s][host["sample"][s] >= 0] * 0.01)
        _anchors(host, pc, s, key)
        inside = host["dist"][s] < near
        print(f"{kind} scene {s}: {n} samples, min {host['dist'][s].min(axis=0)}, {int(inside.sum())} of 10 slots inside reach {near}")
        for k in KEYS:
            assert np.array_equal(cut[k][s][inside], host[k][s][inside]), (s, k)
        assert np.isposinf(cut["dist"][s][~inside]).all() and (cut["partner"][s][~inside] == -1).all() and (cut["sample"][s][~inside] == -1).all()


def test_batch_and_chunk_geometry_do_not_matter(small):
    """case 5: scene s of the batch of three == the same scene run alone, byte for byte; so are other numbers of samples per workgroup
    (development option clear_chunk), in the tiled search and in the cell grid"""
    d, pf, hist = small["d"], small["pf"], small["hist"]
    batch = d.clearance(USED, pf, *hist, path=small["path"])
    for s in range(3):
        one = d.clearance(USED[s:s + 1], pf[s:s + 1], *(h[s:s + 1] for h in hist), path=small["path"][s:s + 1])
        _same({k: one[k][0] for k in KEYS}, {k: batch[k][s] for k in KEYS}, f"scene {s} alone / in the batch")
    for chunk in (1, 5, 64):
        e = mp.Dmpc("bound", **small["kw"]).debug_option("clear_chunk", chunk)
        _same(e.clearance(USED, pf, *hist, path=small["path"]), batch, f"clear_chunk = {chunk}")
    kw = cl.box_kw()
    pk, vk, ak, pos = cl.box_scene(257)
    a, b = mp.Dmpc("bound", **kw), mp.Dmpc("bound", **kw).debug_option("clear_chunk", 3)
    for reach in (np.inf, cl.REACH3):
        _same(b.clearance([cl.BOX_KT], pk[:, -1], pk, vk, ak, po_static=pos, reach=reach),
              a.clearance([cl.BOX_KT], pk[:, -1], pk, vk, ak, po_static=pos, reach=reach), f"box, clear_chunk = 3, reach {reach}")


# ---- 3: the boundary between the searches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cmd", [256, 257, 300])
def test_regime_boundary_tiled_search_and_cell_grid(n_cmd):
    """N_cmd = 256, 257, 300 plus 3 static vehicles in a dense box (tests/test_clearance_cpu.py: slots inside and outside 3 rmin of either
    kind).  reach = inf: the tiled all-pairs search, against numpy and the anchors; reach = 3 rmin: the cell grid -- every slot whose numpy
    distance is < reach equals the reach = inf result byte for byte, every other slot is +inf / -1 / -1."""
    kw = cl.box_kw()
    pk, vk, ak, pos = cl.box_scene(n_cmd)
    pf = pk[:, -1]
    d = mp.Dmpc("bound", **kw)
    pc = d.postcheck([cl.BOX_KT], pf, pk, vk, ak, interp=True, po_static=pos)
    n = int(pc["n_samples"][0])
    p, q = pc["p"][0][:, :n], np.repeat(pos[:, None], n, axis=1)
    full = d.clearance([cl.BOX_KT], pf, pk, vk, ak, po_static=pos)
    filled, empty = cl.check_scene(full["dist"][0], full["partner"][0], full["sample"][0], p, q, kw["c"])
    assert filled == 2 * n_cmd and empty == 0
    _anchors(full, pc, 0, "min_dist_static")
    grid = d.clearance([cl.BOX_KT], pf, pk, vk, ak, po_static=pos, reach=cl.REACH3)
    filled, empty = cl.check_scene(grid["dist"][0], grid["partner"][0], grid["sample"][0], p, q, kw["c"], reach=cl.REACH3)
    d0, d1 = cl.nearest(p, q, kw["c"])
    inside = np.stack([d0, d1], axis=1) < cl.REACH3
    print(f"N_cmd {n_cmd}: {n} samples, {int(inside[:, 0].sum())} / {int(inside[:, 1].sum())} slots of kind 0 / 1 inside 3 rmin")
    assert inside[:, 0].any() and inside[:, 1].any() and not inside[:, 0].all() and not inside[:, 1].all()
    assert filled == int(inside.sum()) and empty == 2 * n_cmd - filled
    for k in KEYS:
        assert grid[k][0][inside].tobytes() == full[k][0][inside].tobytes(), k
    assert np.isposinf(grid["dist"][0][~inside]).all() and (grid["partner"][0][~inside] == -1).all() and (grid["sample"][0][~inside] == -1).all()
    _anchors(grid, pc, 0, "min_dist_static")


# ---- 4: exact ties -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,reach", [(4, np.inf), (257, np.inf), (257, 1.5)])
def test_exact_ties_go_to_the_first_sample_and_the_lower_neighbour(n, reach):
    """agents 1 m apart on a line with one common y-history: d2 is exactly 1 between neighbours at every sample, so every agent ties between
    all samples and, inside the line, between two partners.  Sample 0 and the lower neighbour win, in the tiled search (n = 4, and n = 257
    where agent 256's neighbour sits in the other tile) and in the cell grid (reach = 1.5)."""
    pk, vk, ak = cl.line_scene(n)
    out = mp.Dmpc("bound", **cl.line_kw(n)).clearance([pk.shape[1]], pk[:, -1], pk, vk, ak, reach=reach)
    assert (out["dist"][0, :, 0] == 1.0).all() and (out["sample"][0, :, 0] == 0).all() and (out["time"][0, :, 0] == 0.0).all()
    assert np.array_equal(out["partner"][0, :, 0], cl.line_partner(n))
    assert np.isposinf(out["dist"][0, :, 1]).all() and (out["partner"][0, :, 1] == -1).all() and (out["sample"][0, :, 1] == -1).all()


# ---- 6: the documented near miss -----------------------------------------------------------------------------------------------------------------
def test_near_miss_between_two_columns_is_named():
    """scene A/1 of tests/scripted.py ends SOLVED | REACHED with every 5 Hz column clear, and between two columns agent 1 passes vehicle 3 at
    0.214 m (tests/test_gpu_scripted.py::test_postcheck_scripted): violation_scripted says that it happened, the report says who, with whom
    and when"""
    po, pf, path = sc.scene("A", 1)
    d = mp.Dmpc("bound", **sc.KW)
    tr = d.transition(po[None], pf[None], sc.KT, sc.ERROR_TOL, path=path[None], histories=False)
    assert int(tr["scene_status"][0]) == (mp.ST_SOLVED | mp.ST_REACHED)
    pc = d.postcheck(tr["K_T_used"], pf[None], KT_alloc=sc.KT, path=path[None])
    rep = d.clearance(tr["K_T_used"], pf[None], KT_alloc=sc.KT, path=path[None])
    assert pc["violation_scripted"][0] == 1
    _anchors(rep, pc, 0, "min_dist_scripted")
    i = int(np.argmin(rep["dist"][0, :, 1]))
    dist, partner, t = rep["dist"][0, i, 1], int(rep["partner"][0, i, 1]), rep["time"][0, i, 1]
    hs = pc["h_scaled"][0]
    print(f"agent {i} passes vehicle {partner - po.shape[0]} at {dist:.4f} m, t = {t:.2f} s = column {t / hs:.3f}")
    assert i == 1 and partner == po.shape[0] + 3 and dist < sc.KW["rmin"] - 0.05
    k = int(np.floor(t / hs))
    assert k * hs < t < (k + 1) * hs and 0 < k < int(tr["K_T_used"][0]) - 1


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------------------
def _raw(d, pk, vk, ak, N, n_cmd, pos=None, path=None, P=0, reach=np.inf, used=(5,)):
    f = lambda a: None if a is None else sc._dp(np.ascontiguousarray(a, dtype=np.float64))
    S = len(used)
    dist, partner, sample = np.zeros((S, max(n_cmd, 1), 2)), np.zeros((S, max(n_cmd, 1), 2), dtype=np.int32), np.zeros((S, max(n_cmd, 1), 2), dtype=np.int32)
    return d._L.dmpc_postcheck_clearance(d._ctx, S, N, n_cmd, 5, sc._ip(np.array(used, dtype=np.int32)), None, f(pk), f(vk), f(ak), f(pos), f(path), P,
                                         2.0, 1.0, 0.01, float(reach), sc._dp(dist), sc._ip(partner), sc._ip(sample))


def test_bad_arguments_are_refused_by_name_and_launch_nothing():
    d = mp.Dmpc("bound", **cl.KW)
    n0 = d.solve_count
    pk, vk, ak = cl.line_scene(2, KT=5)
    h = tuple(x[None] for x in (pk, vk, ak))
    pos, path = np.zeros((1, 1, 3)), np.zeros((1, 1, 2, 3))
    for args, word in ((dict(N=3, pos=pos, path=path, P=2), "exclude each other"), (dict(N=3), "needs po_static or path"), (dict(reach=0.0), "reach must"),
                       (dict(reach=-1.0), "reach must"), (dict(reach=np.nan), "reach must"), (dict(hist=(h[0], None, h[2])), "pk, vk, ak"),
                       (dict(hist=(None, None, h[2])), "pk, vk, ak"), (dict(N=3, path=path, P=0), "P must"), (dict(n_cmd=0), "N_cmd must"),
                       (dict(n_cmd=3), "N_cmd must")):
        a = dict(N=2, n_cmd=2, hist=h); a.update(args)
        hist = a.pop("hist")
        rc = _raw(d, *hist, **a)
        assert rc == -1 and _err(d).startswith("dmpc_postcheck_clearance: ") and word in _err(d), (args, _err(d))
    assert d.solve_count == n0
    with pytest.raises(mp.DmpcError, match="exclude each other"):
        d.clearance([5], pk[:, -1], pk, vk, ak, po_static=pos[0], path=path[0])
    with pytest.raises(mp.DmpcError, match="dmpc_postcheck_clearance: no resident histories"):
        d.clearance([5], pk[:, -1], KT_alloc=5)
    # a good call after the refused ones: two agents 1 m apart, one vehicle
    assert _raw(d, *h, N=2, n_cmd=2) == 0, _err(d)
    out = d.clearance([5], pk[:, -1], pk, vk, ak, po_static=[[0.0, 0.0, 4.0]])
    assert (out["dist"][0, :, 0] == 1.0).all() and np.array_equal(out["partner"][0], [[1, 2], [0, 2]])
    # an only agent has no partner: +inf, as min_dist of dmpc_postcheck; masked, NaN
    lone = d.clearance([5], pk[:1, -1], pk[:1], vk[:1], ak[:1])
    assert np.isposinf(lone["dist"]).all() and (lone["partner"] == -1).all()
    assert np.isnan(d.clearance([5], pk[:1, -1], pk[:1], vk[:1], ak[:1], mask=[0])["dist"]).all()


# ---- 8: the resident histories of a split batch -----------------------------------------------------------------------------------------------
SPLIT_USED = np.array([12, 7, 9, 12, 5], dtype=np.int32)
SPLIT_MASK = np.array([1, 1, 0, 1, 1], dtype=np.int32)
SPLIT_SEEDS = [0, 1, 2, 3, 5]           # (scene("path", 4) stops on column 2 with a failed agent)


@pytest.mark.parametrize("kind", ["static", "scripted"])
def test_resident_histories_of_a_split_batch(kind):
    """S = 5 scenes of tests/mission.py -- four commanded agents, two static / two scripted vehicles -- through a transition with
    split_parts = 3: parts of 1, 2 and 2 scenes (cut at 1 and 3), whose histories stay on three contexts.  The clearance arrays of the resident
    call (each part searched where it lives, every array offset per part) == those of the same call on host histories on a context that
    never splits, byte for byte; so are the post-check's outputs, with po_static (dmpc_postcheck_cmd) and, scripted, with the path."""
    b = ms.batch(["static" if kind == "static" else "path"] * 5, SPLIT_SEEDS)
    pf = b["goals"][:, 0]
    d = mp.Dmpc("bound", **ms.KW).debug_option("split_parts", 3)
    tr = d.transition(b["po"], pf, KT_SMALL, ms.ERROR_TOL, path=b["path"])
    assert (tr["K_T_used"] == KT_SMALL).all() and tr["pk"].shape == (5, 4, KT_SMALL, 3)
    hist = (tr["pk"], tr["vk"], tr["ak"])
    e = mp.Dmpc("bound", **ms.KW).debug_option("no_split", 1)
    pos = b["po"][:, 4:] if kind == "static" else np.repeat(ms.STATIC[None], 5, axis=0)
    extra = dict(po_static=pos) if kind == "static" else dict(path=b["path"])
    res = d.clearance(SPLIT_USED, pf, KT_alloc=KT_SMALL, mask=SPLIT_MASK, **extra)
    host = e.clearance(SPLIT_USED, pf, *hist, mask=SPLIT_MASK, **extra)
    _same(res, host, f"{kind}: split resident / host histories")
    assert np.isnan(host["dist"][2]).all() and (host["partner"][2] == -1).all()
    on = SPLIT_MASK == 1
    assert np.isfinite(host["dist"][on]).all() and (host["partner"][on][..., 1] >= 4).all() and len(set(host["dist"][on, 0, 1])) == 4
    print(f"{kind}: nearest vehicle per scene {host['dist'][:, :, 1].min(axis=1)}")
    for ex in (dict(po_static=pos), extra)[:1 if kind == "static" else 2]:
        a = d.postcheck(SPLIT_USED, pf, KT_alloc=KT_SMALL, mask=SPLIT_MASK, interp=True, **ex)
        h = e.postcheck(SPLIT_USED, pf, *hist, mask=SPLIT_MASK, interp=True, **ex)
        assert set(a) == set(h) and ("min_dist_static" in h or "p_scripted" in h)
        for k in h:
            assert a[k].dtype == h[k].dtype and a[k].shape == h[k].shape and a[k].tobytes() == h[k].tobytes(), (kind, sorted(ex), k)
        assert (h["n_samples"][on] > 0).all() and h["n_samples"][2] == 0 and len(set(h["n_samples"][on])) > 1


# ---- the MEX gateway ---------------------------------------------------------------------------------------------------------------------------
def test_gateway_clearance_matches_the_binding(small):
    """dmpc_mex('clearance', ...) on one trial: dist / partner (1-based, 0 = none) / time, 2 x N, against Dmpc.clearance"""
    import mexharness as mh
    d, pf, pos = small["d"], small["pf"][0], small["pos"][0]
    pk, vk, ak = (h[0][:, :9] for h in small["hist"])
    m = lambda a: a.transpose(2, 1, 0)                                        # MATLAB pk(3,KT,N)
    prm = mh.params("bound", small["kw"])
    for extra, margs in ((dict(po_static=pos), [pos.T]), (dict(po_static=pos, reach=0.9), [pos.T, 0.9]), (dict(reach=cl.REACH3), [np.zeros((0, 0)), cl.REACH3]), ({}, [])):
        ref = d.clearance([9], pf, pk, vk, ak, **extra)
        dist, partner, time = mh.call("clearance", prm, [m(pk), m(vk), m(ak), pf.T, 2.0, 1.0, 0.01] + margs, nlhs=3)
        assert dist.shape == (2, 5) and dist.T.tobytes() == ref["dist"][0].tobytes()
        assert np.array_equal(partner.T, ref["partner"][0] + 1.0) and np.array_equal(time.T, ref["time"][0], equal_nan=True)
