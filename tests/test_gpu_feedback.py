"""GPU: event-triggered feedback (dmpc_set_feedback) -- dmpc_feedback_device and the closed loop against the numpy restatement of
tests/feedback.py byte for byte, the policies that must reproduce an existing flight (trigger 0 without re-anchoring: the disturbed loop; no
disturbance: the plain call; trigger inf: the plain accelerations), the oracle's loop, hold, every flight flavour by a property of one event,
cut-and-continue, the split batch and the refusals.  The rule itself and the scene conditions are checked on the host in
tests/test_feedback_cpu.py."""
import functools

import numpy as np
import pytest

import multiagent_planning_amd as mp
from multiagent_planning_amd import workload as wl
import disturb as di
import feedback as fb
import hold as ho
import obstacles as ob
import start as stt
from test_gpu_disturb import _flavours

pytestmark = pytest.mark.gpu

HIST = ("pk", "vk", "ak")
OUT = HIST + ("K_T_used", "scene_status")
INF = float("inf")
COL = ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "event", "lT_next", "v_rows")


def _same(a, b, keys=OUT, what=""):
    for key in keys:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)


def _same_log(d, S, n, want, what=""):
    got = d.feedback_log(S, n)
    for key in fb.LOG:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), (what, key, got[key], want[key])
    return got


# ---- 1. the device form ---------------------------------------------------------------------------------------------------------------------
def _device_column(d, k, c, done):
    """dmpc_feedback_device on copies of the arrays of c (feedback.random_column); returns the dict feedback.column returns (without g, n)"""
    import torch
    dev = torch.device("cuda", 0)
    S, n = c["status"].shape
    t = {key: torch.from_numpy(np.ascontiguousarray(c[key])).to(dev) for key in ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next")}
    t["event"] = torch.full((S, n), -7, dtype=torch.int32, device=dev)
    t_done = torch.from_numpy(done).to(dev) if done is not None else None
    d.feedback_device(S, c["lT_next"].shape[2], n, k, *[t[key].data_ptr() for key in ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next", "event")],
                      t_done.data_ptr() if done is not None else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {key: t[key].cpu().numpy() for key in ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "event", "lT_next")}
    out["v_rows"] = t["v"].cpu().numpy()
    return out


@pytest.mark.parametrize("S,n,N", [(1, 1, 1), (2, 64, 64), (2, 65, 65), (3, 300, 300), (2, 65, 70)])
def test_feedback_device_equals_the_restatement(S, n, N):
    h = ob.KW["h"]
    dist = dict(noise_p=2e-3, noise_v=1e-2, seed=11, wind=np.random.default_rng(n).uniform(-0.5, 0.5, (S, 3)),
                pushes=[di.push(S - 1, n - 1, 2, dp=(0.1, 0.0, -0.1)), di.push(0, 0, 2, dv=(0.0, 0.3, 0.0)), di.push(0, n // 2, 3, dp=(9.0, 9.0, 9.0))])
    c = fb.random_column(S, n, N, 1000 * S + n)
    done = np.zeros(S, dtype=np.int32)
    done[S - 1] = S > 1   # one finished scene
    d = mp.Dmpc("bound", **ob.KW)
    # nothing set: nothing written (the event array keeps its mark)
    got = _device_column(d, 2, c, done)
    assert (got["event"] == -7).all() and all(got[key].tobytes() == np.asarray(c["v" if key == "v_rows" else key]).tobytes() for key in COL if key != "event")
    for pol, with_d in (((0.05, 0.25, 1), True), ((0.0, 0.0, 0), True), ((INF, INF, 1), True), ((0.03, 0.1, 1), False)):
        d.set_feedback(*pol)
        d.set_disturbance(**dist) if with_d else d.clear_disturbance()
        cur, hit = dict(c), False
        for k in (2, 3):   # two consecutive columns: the second starts from what the first left (and reuses its upload)
            dp, dv = di.sample(h, S, n, k, **dist) if with_d else (None, None)
            args = [cur[key] for key in ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next")]
            want = fb.column(*pol, h, *args, dp, dv, done)
            got = _device_column(d, k, cur, done)
            if S > 1:
                got["event"][S - 1] = 0   # (a finished scene's flags are not written: the mark stays)
            _same(got, want, COL, (pol, with_d, k))
            cur = dict(cur, v=want["v_rows"], **{key: want[key] for key in ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next")})
            hit = hit or bool(want["event"].any())
        assert hit == (pol[0] != INF) or n == 1
    got = _device_column(d, 2, c, None)   # no scene_done: every scene
    _same(got, fb.column(0.03, 0.1, 1, h, *[c[key] for key in ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "lT_next")]), COL, "all scenes")
    for bad in (dict(k=0), dict(n=N + 1)):
        with pytest.raises(mp.DmpcError, match="^dmpc_feedback_device: "):
            d.feedback_device(S, N, bad.get("n", n), bad.get("k", 1), *[8] * 13)


# ---- 2. policies that must reproduce a flight that exists already ---------------------------------------------------------------------------------
def _c4(S=3, N=16, seed=99):
    cfg = dict(wl.CONFIGS["C4"])
    po, pf = wl.make_scenes(cfg, S, N, wl.SEED0 + seed)
    return cfg, wl.solver_kwargs(cfg, N), po, pf


def _dist_4f(S):
    """the disturbance of tests/test_gpu_disturb.py::test_disturbed_transition_equals_the_host_loop"""
    wind = np.zeros((S, 3))
    wind[1] = (0.15, -0.1, 0.05)
    return dict(noise_p=2e-3, noise_v=1e-2, seed=5, wind=wind, pushes=[di.push(0, 3, 5, dp=(0.0, 0.1, 0.0))])


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_trigger_zero_without_reanchor_is_the_disturbed_loop(precision):
    cfg, kw, po, pf = _c4()
    d = mp.Dmpc("bound", precision=precision, **kw)
    base = d.transition(po, pf, 40, cfg["error_tol"], disturb=_dist_4f(3))
    d.set_feedback(0.0, 0.0, reanchor=False)
    res = d.transition(po, pf, 40, cfg["error_tol"], disturb=_dist_4f(3))
    _same(res, base)
    log = d.feedback_log(3, 16)
    cols = np.asarray(res["K_T_used"]) - 1
    assert (log["event_count"] == cols[:, None]).all() and (log["event_first"] == 1).all() and (log["event_last"] == cols[:, None]).all()
    assert not log["e_p"].any() and not log["e_v"].any() and log["dev_p_max"].max() > 0.09
    for s in range(3):
        assert np.array_equal(log["xh_p"][s], res["pk"][s][:, cols[s]]) and np.array_equal(log["xh_v"][s], res["vk"][s][:, cols[s]])


@pytest.mark.parametrize("flavour", ["plain", "n_cmd", "path", "hold", "mission", "route", "replan"])
def test_a_policy_without_a_disturbance_is_inert(flavour):
    kw, fly = _flavours()[flavour]
    d = mp.Dmpc("bound", **kw)
    plain = fly(d)
    d.set_feedback(0.01, 0.05)
    res = fly(d)
    for key in plain:
        assert np.asarray(res[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    S, n = plain["pk"].shape[:2]
    log = d.feedback_log(S, n)
    cols = np.asarray(res["K_T_used"]) - 1
    assert not log["event_count"].any() and (log["event_first"] == -1).all() and (log["event_last"] == -1).all() and not log["dev_p_max"].any()
    assert not log["e_p"].any() and not log["e_v"].any()
    for s in range(S):
        assert np.array_equal(log["xh_p"][s], res["pk"][s][:, cols[s]]) and np.array_equal(log["xh_v"][s], res["vk"][s][:, cols[s]])


def test_trigger_inf_is_the_open_loop():
    """one push of dp alone, never fed back: the planner flies the plain flight (ak byte for byte), the vehicle flies beside it by e"""
    cfg, kw, po, pf = _c4(S=2)
    d = mp.Dmpc("bound", **kw)
    KT = 20
    plain = d.transition(po, pf, KT, cfg["error_tol"])
    dist = dict(pushes=[di.push(1, 3, 5, dp=(0.0, 0.1, 0.0))])
    d.set_feedback(INF, INF, reanchor=True).set_disturbance(**dist)
    res = d.transition(po, pf, KT, cfg["error_tol"])
    assert (res["K_T_used"] > 8).all() and (plain["K_T_used"] > 8).all()
    both = [int(min(a, b)) for a, b in zip(res["K_T_used"], plain["K_T_used"])]   # (ReachedGoal judges the true state: the pushed scene may fly longer)
    for s in range(2):
        assert res["ak"][s][:, :both[s]].tobytes() == plain["ak"][s][:, :both[s]].tobytes(), s
    want = fb.loop(fb.device_batch_step(d), po, pf, KT, cfg["error_tol"], kw["h"], (INF, INF, 1), dist, l0=d.init_batch(po, pf)[0])
    _same(res, want)
    log = _same_log(d, 2, 16, want["log"])
    assert not log["event_count"].any() and log["dev_p_col"][1, 3] == 5 and abs(log["dev_p_max"][1, 3] - 0.1) < 1e-15
    off = res["pk"] - plain["pk"]
    assert np.abs(off[1, 3, 5:both[1]] - (0.0, 0.1, 0.0)).max() < 1e-12 and not off[0, :, :both[0]].any() and not off[1, :3, :both[1]].any()


# ---- 3. the loop ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_transition_with_a_policy_equals_the_host_loop(precision):
    cfg, kw, po, pf = _c4()
    KT, pol = 40, (0.05, 0.25, 1)
    dist = _dist_4f(3)
    d = mp.Dmpc("bound", precision=precision, **kw)
    d.set_feedback(*pol)
    res = d.transition(po, pf, KT, cfg["error_tol"], disturb=dist)
    log = d.feedback_log(3, 16)
    want = fb.loop(fb.device_batch_step(d), po, pf, KT, cfg["error_tol"], kw["h"], pol, dist, l0=d.init_batch(po, pf)[0])
    print("events", want["events"], "K_T_used", want["K_T_used"], "largest deviation", want["log"]["dev_p_max"].max(), want["log"]["dev_v_max"].max())
    _same(res, want)
    for key in fb.LOG:
        assert log[key].tobytes() == np.ascontiguousarray(want["log"][key]).tobytes(), key
    # what the case is meant to exercise: the push is an event, most agent-columns are not, some error is in flight at the end
    assert (5, 0, 3) in want["events"] and 0 < len(want["events"]) < (np.asarray(res["K_T_used"]) - 1).sum() * 16 / 4
    assert log["e_p"].any() and (res["K_T_used"] > 6).all()


@functools.lru_cache(maxsize=None)
def _head_on_oracle():
    """the oracle's loop on the head-on scene with the push of tests/test_feedback_cpu.py (shared: do not modify)"""
    from oracle import oracle as orc
    po, pf = stt.head_on()
    return fb.loop(fb.oracle_batch_step(orc, orc.make_params("bound", **ob.KW)), po[None], pf[None], 60, 0.1, ob.KW["h"], (0.05, 0.25, 1),
                   dict(pushes=[di.push(0, 0, 5, dp=(0.0, 0.15, 0.0))]))


def test_head_on_push_against_the_oracle_loop():
    po, pf = stt.head_on()
    want = _head_on_oracle()
    d = mp.Dmpc("bound", **ob.KW).set_feedback(0.05, 0.25).set_disturbance(pushes=[di.push(0, 0, 5, dp=(0.0, 0.15, 0.0))])
    res = d.transition(po[None], pf[None], 60, 0.1)
    log = d.feedback_log(1, 2)
    assert log["event_count"].tolist() == want["log"]["event_count"].tolist() == [[1, 0]] and log["event_first"].tolist() == [[5, -1]]
    assert int(res["K_T_used"][0]) == int(want["K_T_used"][0]) and int(res["scene_status"][0]) == int(want["scene_status"][0])
    err = max(float(np.abs(res[key] - want[key]).max()) for key in HIST)
    print(f"head-on with a push and one event: histories, device vs oracle loop: {err:.3e}")
    assert err < 1e-7


# ---- 4. hold --------------------------------------------------------------------------------------------------------------------------------
def test_a_held_plan_continues_the_reanchored_one():
    """bound on scripted.scene("A", 0) holds agent 3 on column 19 (tests/test_hold_cpu.py).  A small push on the column before the first hold of
    the flight, trigger 0 and re-anchoring: the event moves the plan the hold rule then shifts"""
    s = ho.scene("A", 0)
    po, pf, path = s["po"][None], s["goals"][0][None], s["path"][None]
    d = mp.Dmpc("bound", **ho.KW)
    fly = lambda: d.transition(po, pf, ho.KT, ho.ERROR_TOL, path=path, on_fail="hold")
    plain = fly()
    i = int(np.argmin(np.where(plain["hold_first"][0] < 0, 10 ** 6, plain["hold_first"][0])))   # the agent that is held first
    kh = int(plain["hold_first"][0, i])
    assert kh > 2
    dv = (1e-4, -2e-4, 1e-4)
    dist = dict(pushes=[di.push(0, i, kh - 1, dv=dv)])
    d.set_feedback(0.0, 0.0, reanchor=True).set_disturbance(**dist)
    res = fly()
    want = fb.loop(fb.device_batch_step(d), po, pf, ho.KT, ho.ERROR_TOL, ho.KW["h"], (0.0, 0.0, 1), dist, l0=d.init_batch(po, pf)[0], path=path,
                   max_hold=ho.MAX_HOLD, alim=ho.KW["alim"])
    print("holds", want["holds"], "events", want["events"])
    _same(res, want)
    assert np.array_equal(res["hold_count"], want["hold_count"])
    _same_log(d, 1, 8, want["log"])
    assert want["events"] == [(kh - 1, 0, i)] and (kh, 0, i) in want["holds"]
    # the held plan's velocities carry g_v: column kh's velocity is entry 1 of the plan solved on column kh - 1, moved by the push
    d.clear_feedback()
    unanchored = fly()
    assert np.array_equal(res["vk"][0, i, kh - 1], unanchored["vk"][0, i, kh - 1])
    moved = res["vk"][0, i, kh] - unanchored["vk"][0, i, kh]
    assert np.abs(moved - dv).max() < 1e-12 and np.abs(unanchored["vk"][0, i, kh] - plain["vk"][0, i, kh]).max() < 1e-12


# ---- 5. every flavour, by a property of one event -------------------------------------------------------------------------------------------
K0, DP = 4, (0.03, -0.05, 0.02)


@pytest.mark.parametrize("flavour", ["plain", "n_cmd", "path", "hold", "mission", "route", "replan"])
def test_one_event_in_every_flavour(flavour):
    kw, fly = _flavours()[flavour]
    d = mp.Dmpc("bound", **kw)
    plain = fly(d)
    S, n = plain["pk"].shape[:2]
    s, i = S - 1, n - 1
    d.set_feedback(0.01, 0.05)
    dist = dict(pushes=[di.push(s, i, K0, dp=DP)])
    res = fly(d, disturb=dist)
    assert (res["K_T_used"] > K0 + 2).all()
    for key in HIST:
        assert np.array_equal(res[key][:, :, :K0], plain[key][:, :, :K0]), key
    assert np.array_equal(res["pk"][s, i, K0], plain["pk"][s, i, K0] + np.array(DP))
    log = d.feedback_log(S, n)
    others = np.ones((S, n), bool)
    others[s, i] = False
    assert log["event_first"][s, i] == K0 and log["event_count"][s, i] == 1 and not log["event_count"][others].any()
    assert log["dev_p_col"][s, i] == K0 and not log["e_p"].any()
    # the setting outlives the call until it is cleared
    _same(fly(d, disturb=dist), res)
    d.clear_feedback()
    for key in plain:
        assert np.asarray(fly(d)[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    with pytest.raises(mp.DmpcError, match="^dmpc_feedback_log: "):
        d.feedback_log(S, n)   # (the last flight had no policy)


# ---- 6. cut and continue --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [6, 7])
def test_cut_a_flight_that_feeds_back_on_every_column(cut):
    """trigger (0, 0): every column ends with e = 0, so the end of a flight holds everything the rest needs -- the re-anchored plan included"""
    po, pf = (x[None] for x in stt.head_on())
    d = mp.Dmpc("bound", **ob.KW)
    d.set_feedback(0.0, 0.0, reanchor=True)
    d.set_disturbance(noise_p=2e-3, noise_v=1e-2, seed=7, pushes=[di.push(0, 0, 5, dp=(0.0, 0.15, 0.0)), di.push(0, 1, 9, dp=(0.01, 0.0, 0.0), dv=(0.0, 0.05, 0.0))])
    whole = d.transition(po, pf, stt.KT, 0.1)
    used = int(whole["K_T_used"][0])
    assert used > cut + 3
    first = d.transition(po, pf, cut + 1, 0.1)
    assert int(first["K_T_used"][0]) == cut + 1
    d.set_start(from_end=True, S=1, N_cmd=2)
    rest = d.transition(po, pf, stt.KT - cut, 0.1)
    assert int(rest["K_T_used"][0]) == used - cut and rest["scene_status"][0] == whole["scene_status"][0]
    for key in HIST:
        assert first[key][0][:, :cut + 1].tobytes() == whole[key][0][:, :cut + 1].tobytes(), key
        assert rest[key][0][:, :used - cut].tobytes() == whole[key][0][:, cut:used].tobytes(), key
    d.clear_feedback()   # re-anchoring is what the flight is about: without it the columns differ
    assert d.transition(po, pf, stt.KT, 0.1)["pk"].tobytes() != whole["pk"].tobytes()


# ---- 7. split batch, refusals ---------------------------------------------------------------------------------------------------------------
def test_split_batch_equals_the_unsplit_call():
    cfg, kw, po, pf = _c4(S=5, seed=7)
    KT = 16
    dist = dict(noise_p=2e-3, noise_v=1e-2, seed=3, wind=np.arange(15.0).reshape(5, 3) * 0.02 - 0.1,
                pushes=[di.push(4, 15, 4, dp=(0.1, 0.0, 0.0)), di.push(0, 0, 2, dv=(0.0, 0.3, 0.0)), di.push(2, 0, 3, dp=(0.0, 0.0, 0.06)), di.push(3, 7, 3, dp=(0.0, -0.07, 0.0))])
    one, three = mp.Dmpc("bound", **kw).debug_option("no_split", 1), mp.Dmpc("bound", **kw).debug_option("split_parts", 3)
    res = []
    for d in (one, three):
        d.set_feedback(0.05, 0.25)
        res.append((d.transition(po, pf, KT, cfg["error_tol"], disturb=dist), d.feedback_log(5, 16)))
    _same(res[1][0], res[0][0])
    for key in fb.LOG:
        assert res[1][1][key].tobytes() == res[0][1][key].tobytes(), key
    assert 1 <= res[0][1]["event_first"][4, 15] <= 4 and 1 <= res[0][1]["event_first"][0, 0] <= 2 and (res[0][0]["K_T_used"] > 5).all()   # (the pushes at the latest)
    with pytest.raises(mp.DmpcError, match="^dmpc_feedback_log: "):
        three.feedback_log(4, 16)


def test_refusals():
    cfg, kw, po, pf = _c4(S=2)
    d = mp.Dmpc("bound", **kw)
    with pytest.raises(mp.DmpcError, match="^dmpc_feedback_log: "):
        d.feedback_log(2, 16)   # before any flight
    plain = d.transition(po, pf, 12, cfg["error_tol"])
    with pytest.raises(mp.DmpcError, match="^dmpc_feedback_log: "):
        d.feedback_log(2, 16)   # a flight without a policy
    for bad in ((float("nan"), 0.0, 0), (0.0, float("nan"), 1), (-1e-9, 0.0, 0), (0.0, -INF, 0), (0.05, 0.25, 2), (0.05, 0.25, -1)):
        rc, msg = fb.raw_set_feedback(d, *bad)
        assert rc == -1 and msg.startswith("dmpc_set_feedback: "), (bad, msg)
    _same(d.transition(po, pf, 12, cfg["error_tol"]), plain)   # a refused policy is no policy
    d.set_feedback(0.05, INF)
    for gather in (False, True):
        with pytest.raises(mp.DmpcError, match="^dmpc_transition_sharded" + ("_gather" if gather else "") + ": a feedback policy is set"):
            d.transition_sharded(po, pf, 12, cfg["error_tol"], gather=gather)
    d.transition(po, pf, 12, cfg["error_tol"])
    for S, n in ((3, 16), (2, 15), (0, 16)):
        with pytest.raises(mp.DmpcError, match="feedback_log: "):
            d.feedback_log(S, n)
    assert fb.raw_set_feedback(d, 0.0, 0.0, 0, null=True)[0] == 0   # NULL clears
    _same(d.transition(po, pf, 12, cfg["error_tol"], disturb=dict(noise_p=1e-3, seed=1)), mp.Dmpc("bound", **kw).transition(po, pf, 12, cfg["error_tol"], disturb=dict(noise_p=1e-3, seed=1)))
