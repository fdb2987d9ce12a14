"""development: one small call per post-check entry and path, every output array and every refusal's message dumped, for a comparison of two
builds of the library.

  python tools/gpu_postcheck_probe.py A.npz                                       (this build)
  python tools/with_lib.py OTHER.so tools/gpu_postcheck_probe.py B.npz            (another build, in a process of its own)
  python tools/npz_equal.py A.npz B.npz

Rows (rows(); tools/gpu_launch_trace.py --postcheck runs those of single_context() under a kernel trace):
  small   S = 5 scenes of tests/mission.py -- four commanded agents alone / beside two static / two scripted vehicles -- after a transition of
          12 columns; K_T_used = 12, 7, 9, 12, 5 with scene 2 masked.  The entry of the kind (dmpc_postcheck / _cmd / _scripted) with
          ns_alloc = 0, below and above the largest sample count (p_interp, p_scripted), dmpc_postcheck_clearance with reach = inf and
          0.9 m, dmpc_postcheck_setpoints over the whole window, over samples 5 .. 34 in one pass and (setpoint_batch = 12) in three,
          and report-only (ns_alloc = 0); clearance again with clear_chunk = 3.  Each on host histories, on the resident ones of one
          context, and on those of a split_parts = 3 batch (parts of 1, 2 and 2 scenes on three contexts).
  big     S = 3 scenes of N = 300 agents (> PC_BRUTE_MAX: the cell grid), ragged, scene 2 sparse -- no pair within the grid's cell edge, so
          it takes the brute-force pass (what ctx->pc_fallback_scenes counts; the ABI does not export it, the launch trace shows the pass)
          -- alone, with two static and two scripted vehicles, interpolated; clearance with reach = 3 rmin (grid) and inf (tiles).
  refused the bad calls of tests/test_gpu_postcheck.py, test_gpu_clearance.py, test_gpu_setpoints.py and test_gpu_scripted.py, and a NULL
          K_T_used / a NULL pf on a context whose last batch was split: the return code and the message of each, as bytes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiagent_planning_amd as mp   # noqa: E402
import clearance as cl   # noqa: E402
import mission as ms   # noqa: E402
from mission import _dp, _ip, _f   # noqa: E402  (None -> a NULL pointer)

KT = 12
USED = np.array([12, 7, 9, 12, 5], dtype=np.int32)
MASK = np.array([1, 1, 0, 1, 1], dtype=np.int32)
SEEDS = [0, 1, 2, 3, 5]   # (scene("path", 4) stops on column 2)
KINDS = dict(alone="reached", static="static", scripted="path")


def err(d):
    return d._L.dmpc_last_error(d._ctx).decode()


def report(d, used, pf, hist=None, KTa=None, mask=None, pos=None, path=None, ns_alloc=0, M=None, P=None):
    """dmpc_postcheck (pos, path None), _cmd (pos [S,M,3]) or _scripted (path [S,M,P,3]) with ns_alloc as given; used / pf None: NULL;
    hist None: the resident histories of shape KTa.  Returns (rc, dict of the outputs)"""
    S, nc = (pf.shape[0], pf.shape[1]) if pf is not None else (len(mask), 4)
    used = None if used is None else np.ascontiguousarray(used, dtype=np.int32)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
    hist = (None, None, None) if hist is None else tuple(None if h is None else _f(h) for h in hist)
    KTa = hist[0].shape[2] if KTa is None else KTa
    o = dict(r_factor=np.zeros(S), h_scaled=np.zeros(S), n_samples=np.zeros(S, dtype=np.int32), min_dist=np.zeros(S),
             violation=np.zeros(S, dtype=np.int32), totdist=np.zeros(S), traj_time=np.zeros(S))
    if ns_alloc:
        o["p"] = np.zeros((S, nc, ns_alloc, 3))
    other = path if path is not None else pos
    shape = (S, nc) if other is None else (S, nc + (other.shape[1] if M is None else M), nc)
    mid = (KTa, _ip(used), _ip(mask), _dp(hist[0]), _dp(hist[1]), _dp(hist[2]), _dp(None if pf is None else _f(pf)))
    tail = (2.0, 1.0, 0.01, _dp(o["r_factor"]), _dp(o["h_scaled"]), _ip(o["n_samples"]), _dp(o["min_dist"]), _ip(o["violation"]), _dp(o["totdist"]),
            _dp(o["traj_time"]), _dp(o.get("p")), int(ns_alloc))
    if path is not None:
        o.update(min_dist_scripted=np.zeros(S), violation_scripted=np.zeros(S, dtype=np.int32))
        if ns_alloc:
            o["p_scripted"] = np.zeros((S, path.shape[1], ns_alloc, 3))
        rc = d._L.dmpc_postcheck_scripted(d._ctx, *shape, *mid, _dp(_f(path)), path.shape[2] if P is None else P, *tail, _dp(o["min_dist_scripted"]),
                                          _ip(o["violation_scripted"]), _dp(o.get("p_scripted")))
    elif pos is not None:
        o.update(min_dist_static=np.zeros(S), violation_static=np.zeros(S, dtype=np.int32))
        rc = d._L.dmpc_postcheck_cmd(d._ctx, *shape, *mid, _dp(_f(pos)), *tail, _dp(o["min_dist_static"]), _ip(o["violation_static"]))
    else:
        rc = d._L.dmpc_postcheck(d._ctx, *shape, *mid, *tail)
    return rc, o


def calls(d, pf, hist, extra):
    """(name, outputs) of every call of one kind of scene on context d; hist None: the resident histories"""
    h = dict(KT_alloc=KT) if hist is None else dict(pk=hist[0], vk=hist[1], ak=hist[2])
    raw = dict(KTa=KT) if hist is None else dict(hist=hist)
    rep = dict(pos=extra.get("po_static"), path=extra.get("path"))
    rc, base = report(d, USED, pf, mask=MASK, **raw, **rep)
    assert rc == 0, err(d)
    yield "report", base
    ns = int(base["n_samples"].max())
    for name, n in (("report_short", ns // 3), ("report_long", ns + 7)):
        rc, o = report(d, USED, pf, mask=MASK, ns_alloc=n, **raw, **rep)
        assert rc == 0, err(d)
        yield name, o
    for name, reach in (("clearance", np.inf), ("clearance_reach", 0.9)):
        yield name, d.clearance(USED, pf, *(hist or ()), KT_alloc=KT, mask=MASK, reach=reach, **extra)
    yield "setpoints", d.setpoints(USED, N=4, mask=MASK, **h)
    yield "setpoints_window", d.setpoints(USED, N=4, mask=MASK, first=5, count=30, **h)
    yield "setpoints_report", d.setpoints(USED, N=4, mask=MASK, report_only=True, **h)
    d.debug_option("setpoint_batch", 12).debug_option("clear_chunk", 3)
    yield "setpoints_window_3_passes", d.setpoints(USED, N=4, mask=MASK, first=5, count=30, **h)
    yield "clearance_chunk3", d.clearance(USED, pf, *(hist or ()), KT_alloc=KT, mask=MASK, **extra)
    d.debug_option("setpoint_batch", 0).debug_option("clear_chunk", 0)


def small(kind, parts=0):
    """(name, outputs): the transition of 12 columns and the calls on its host histories (parts = 0), or on the resident ones of a context
    (parts = 1) / of a split batch (parts = 3)"""
    b = ms.batch([KINDS[kind]] * 5, SEEDS)
    pf = b["goals"][:, 0]
    d = mp.Dmpc("bound", **ms.KW)
    d.debug_option(*(("split_parts", parts) if parts > 1 else ("no_split", 1)))
    tr = d.transition(b["po"], pf, KT, ms.ERROR_TOL, path=b["path"])
    assert (tr["K_T_used"] == KT).all()
    extra = dict(alone={}, static=dict(po_static=b["po"][:, 4:]), scripted=dict(path=b["path"]))[kind]
    tag = f"{kind}.{('host', 'resident', 'split2', 'split3')[parts]}"
    if not parts:
        yield f"{tag}.transition", tr
        d = mp.Dmpc("bound", **ms.KW).debug_option("no_split", 1)   # (nothing resident)
    for name, o in calls(d, pf, None if parts else (tr["pk"], tr["vk"], tr["ak"]), extra):
        yield f"{tag}.{name}", o


def big():
    from test_gpu_postcheck import KW, _swarm_hist
    S, N, KTa = 3, 300, 8
    used, rng = np.array([8, 5, 6], dtype=np.int32), np.random.default_rng(3000)
    kw = dict(KW, pmin=(-10, -10, 0.2), pmax=(10, 10, 20.0))
    pk, vk, ak = (np.zeros((S, N, KTa, 3)) for _ in range(3))
    for s in range(S):   # scenes 0, 1: the density of the large-scene tests; scene 2: 18 m wide, every neighbour metres away
        pk[s, :, :used[s]], vk[s, :, :used[s]], ak[s, :, :used[s]] = _swarm_hist(rng, N, used[s], 18.0 if s == 2 else N ** (1.0 / 3.0), speed=0.5 if s == 2 else 2.5)
    pf = pk[np.arange(S), :, used - 1]
    pos = pk[:, [0, 100], 0] + (0.5, 0.0, 0.0)
    path = pk[:, [50, 200], :1] + (0.0, 0.5, 0.0) + np.cumsum(rng.uniform(-0.1, 0.1, (S, 2, 5, 3)), axis=2)
    d = mp.Dmpc("bound", **kw)
    for name, extra in (("alone", {}), ("static", dict(po_static=pos)), ("scripted", dict(path=path))):
        o = d.postcheck(used, pf, pk, vk, ak, interp=True, **extra)
        assert (o["min_dist"][:2] < 2 * kw["rmin"]).all() and o["min_dist"][2] > 2 * kw["rmin"], o["min_dist"]   # (scene 2: the fallback)
        yield f"big.{name}.report", o
        for tag, reach in (("grid", cl.REACH3), ("tiles", np.inf)):
            yield f"big.{name}.clearance_{tag}", d.clearance(used, pf, pk, vk, ak, reach=reach, **extra)
    yield "big.setpoints_report", d.setpoints(used, pk=pk, vk=vk, ak=ak, report_only=True)


def refused():
    """(name, (rc, message)) of every refused call"""
    import scripted as sc
    import setpoints as sp
    import test_gpu_clearance as tc
    import test_gpu_setpoints as ts
    d = mp.Dmpc("bound", **cl.KW)
    z = np.zeros((1, 2, 5, 3))
    for name, (used, hist, KTa) in dict(used_1=([1], (z, z, z), None), all_zero=([5], (z, z, z), None), none_resident=([5], None, 5)).items():
        yield f"postcheck.{name}", (report(d, used, np.zeros((1, 2, 3)), hist, KTa)[0], err(d))
    pk, vk, ak = cl.line_scene(2, KT=5)
    h = tuple(x[None] for x in (pk, vk, ak))
    pos, path = np.zeros((1, 1, 3)), np.zeros((1, 1, 2, 3))
    for i, args in enumerate((dict(N=3, pos=pos, path=path, P=2), dict(N=3), dict(reach=0.0), dict(reach=-1.0), dict(reach=np.nan), dict(hist=(h[0], None, h[2])),
                              dict(hist=(None, None, h[2])), dict(N=3, path=path, P=0), dict(n_cmd=0), dict(n_cmd=3), dict(hist=(None, None, None)))):
        a = dict(N=2, n_cmd=2, hist=h); a.update(args)
        yield f"clearance.{i}", (tc._raw(d, *a.pop("hist"), **a), err(d))
    g = tuple(x[None] for x in sp.random_hist(np.random.default_rng(2), 2, 5, 5))
    cases = (dict(smp0=-1), dict(ns_alloc=-1, arrays=(0, 0, 0)), dict(ns_alloc=0), dict(ns_alloc=0, arrays=(0, 1, 0)), dict(ns_alloc=4, arrays=(0, 0, 0)),
             dict(hist=(g[0], None, g[2])), dict(hist=(None, None, g[2])), dict(hist=(None, g[1], None)), dict(S=0), dict(N=0), dict(KTa=1), dict(used=None),
             dict(vmax=0.0), dict(amax=-1.0), dict(Ts=0.0), dict(Ts=np.nan), dict(used=(1,)), dict(used=(6,)), dict(hist=tuple(np.zeros_like(x) for x in g)),
             dict(hist=(None, None, None)), dict(smp0=0x7fff0000))
    for i, args in enumerate(cases):
        a = dict(hist=g); a.update(args)
        yield f"setpoints.{i}", (ts._raw(d, a.pop("hist"), **a), err(d))
    L = mp._lib.load()
    rc = L.dmpc_postcheck_setpoints(None, *([0] * 3), None, None, None, None, None, 2.0, 1.0, 0.01, 0, 0, *([None] * 10))
    yield "setpoints.null_ctx", (rc, L.dmpc_last_error(None).decode())
    po, pf, spath = sc.batch("C")
    ones = np.ones((1, 1, 5, 3))
    for name, kw in dict(M0=dict(M=0), P0=dict(P=0), no_path=dict(path=None)).items():
        a = dict(path=spath); a.update(kw)
        yield f"scripted.{name}", (sc.raw_postcheck_scripted(d, [5], ones, ones, ones, pf, a.pop("path"), **a)[0], err(d))
    yield "scripted.p_scripted_ns0", (d._L.dmpc_postcheck_scripted(d._ctx, 1, 2, 1, 5, _ip(np.array([5], dtype=np.int32)), None, *([None] * 3), _dp(_f(pf)), _dp(_f(spath)), 3,
                                                                   2.0, 1.0, 0.01, *([None] * 8), 0, None, None, _dp(ones)), err(d))
    yield "cmd.no_po_static", (d._L.dmpc_postcheck_cmd(d._ctx, 1, 3, 2, 5, None, None, *([None] * 4), None, 2.0, 1.0, 0.01, *([None] * 8), 0, None, None), err(d))
    # a context whose last batch was split: NULL K_T_used, NULL pf, vk without pk
    b = ms.batch(["static"] * 5, SEEDS)
    pf5, pos5 = b["goals"][:, 0], b["po"][:, 4:]
    d = mp.Dmpc("bound", **ms.KW).debug_option("split_parts", 3)
    d.transition(b["po"], pf5, KT, ms.ERROR_TOL, histories=False)
    yield "split.report_null_used", (report(d, None, pf5, KTa=KT, mask=MASK, pos=pos5)[0], err(d))
    yield "split.report_null_pf", (report(d, USED, None, KTa=KT, mask=MASK, pos=pos5, M=2)[0], err(d))
    yield "split.report_null_pf_plain", (report(d, USED, None, KTa=KT, mask=MASK)[0], err(d))
    yield "split.report_used_out_of_range", (report(d, USED + 8, pf5, KTa=KT, pos=pos5)[0], err(d))
    f = lambda a: None if a is None else _dp(_f(a))
    o3 = [np.zeros((5, 4, 2)), np.zeros((5, 4, 2), dtype=np.int32), np.zeros((5, 4, 2), dtype=np.int32)]
    yield "split.clearance_null_used", (d._L.dmpc_postcheck_clearance(d._ctx, 5, 6, 4, KT, None, None, None, None, None, f(pos5), None, 0, 2.0, 1.0, 0.01, np.inf,
                                                                      _dp(o3[0]), _ip(o3[1]), _ip(o3[2])), err(d))
    yield "split.setpoints_null_used", (ts._raw(d, (None, None, None), S=5, N=4, KTa=KT, used=None, ns_alloc=0, arrays=(0, 0, 0)), err(d))
    yield "split.setpoints_out_of_range", (ts._raw(d, (None, None, None), S=5, N=4, KTa=KT, used=tuple(USED + 8), ns_alloc=0, arrays=(0, 0, 0)), err(d))
    assert d.clearance(USED, pf5, KT_alloc=KT, mask=MASK, po_static=pos5)["dist"].shape == (5, 4, 2)   # (a good call after the refused ones)


def single_context():
    """the rows that enqueue on one stream: host and resident histories of every kind, and the big scenes"""
    for kind in KINDS:
        for parts in (0, 1):
            yield from small(kind, parts)
    yield from big()


def rows():
    yield from single_context()
    for kind in KINDS:
        yield from small(kind, 3)


if __name__ == "__main__":
    out = {}
    for name, res in rows():
        arrays = {k: np.asarray(v) for k, v in res.items() if v is not None}
        out.update({f"{name}.{k}": v for k, v in arrays.items()})
        print(f"{name}: {len(arrays)} arrays", flush=True)
    n_arr = len(out)
    for name, (rc, msg) in refused():
        assert rc == -1 and msg, (name, rc, msg)
        out[f"refused.{name}"] = np.frombuffer(msg.encode(), dtype=np.uint8)
        print(f"refused.{name}: {msg}", flush=True)
    np.savez(sys.argv[1], **out)
    print(f"{n_arr} arrays, {sum(v.size * v.itemsize // 4 for k, v in out.items() if not k.startswith('refused'))} 32-bit words, {len(out) - n_arr} messages -> {sys.argv[1]}")
