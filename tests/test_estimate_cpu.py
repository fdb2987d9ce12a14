"""CPU: the measured state (dmpc_set_measurement) on the host -- the entries and their refusals, dmpc_measurement_sample and
dmpc_estimate_apply_host (no context, no GPU) against the numpy restatement of tests/estimate.py byte for byte, and the conditions of the head-on
scene that the GPU tests (tests/test_gpu_estimate.py) rely on, by the oracle's MPC step in the restated loop."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import disturb as di
import estimate as es
import feedback as fb
import mission as mi
import obstacles as ob
import start as stt
from helpers import ROOT
from multiagent_planning_amd import _lib

H = ob.KW["h"]
INF = float("inf")
NAN = float("nan")
NAMES = ("dmpc_set_measurement", "dmpc_measurement_sample", "dmpc_estimate_device", "dmpc_estimate_apply_host", "dmpc_estimate_log")
OUT = ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "eh_p", "eh_v", "event", "lT_next", "v_rows")
COLUMN = ("p", "v", "a", "status", "x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v")
GAINS = ((1.0, 1.0), (0.5, 0.5), (1.0, 0.25))


def _args(c, eh):
    return [c[k] for k in COLUMN] + [eh[0], eh[1], c["lT_next"]]


def _meas(amp=(0.02, 0.05), gain=(1.0, 1.0), seed=1):
    return dict(noise_p=amp[0], noise_v=amp[1], gain_p=gain[0], gain_v=gain[1], seed=seed)


# ---- 1. the entries -------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()
    for name, nargs in zip(NAMES, (2, 6, 22, 24, 13)):
        assert re.search(r"DMPC_API int " + name + r"\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == nargs, name
    for method in ("set_measurement", "clear_measurement", "estimate_log", "estimate_device"):
        assert callable(getattr(_lib.Dmpc, method)), method
    assert callable(_lib.estimate_apply) and callable(_lib.measurement_sample)


def test_struct_layout_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()
    body = re.search(r"typedef struct dmpc_measurement \{(.*?)\} dmpc_measurement;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("seed", "uint64_t"), ("amp_p", "double"), ("amp_v", "double"), ("gain_p", "double"), ("gain_v", "double")]
    ct = {"double": C.c_double, "uint64_t": C.c_uint64}
    M = _lib.DmpcMeasurement
    assert [(n, t) for n, t in M._fields_] == [(n, ct[t]) for n, t in fields]
    assert [getattr(M, n).offset for n, _ in fields] == [0, 8, 16, 24, 32]
    assert C.sizeof(M) == 40


def test_a_null_context_is_refused_by_name():
    L = _lib.load()
    m = es.descriptor()
    z = C.c_void_p(0)
    nd, ni = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
    calls = {"dmpc_set_measurement": lambda: L.dmpc_set_measurement(None, C.byref(m)),
             "dmpc_estimate_device": lambda: L.dmpc_estimate_device(None, 1, 1, 1, 1, *[z] * 17),
             "dmpc_estimate_log": lambda: L.dmpc_estimate_log(None, 1, 1, nd, ni, nd, ni, nd, ni, nd, ni, nd, nd)}
    for name, call in calls.items():
        assert call() == -1 and L.dmpc_last_error(None).decode() == f"{name}: ctx is NULL", name


# (field named in the message, descriptor)
BAD = [("amp_p", dict(noise_p=-1e-9)), ("amp_p", dict(noise_p=INF)), ("amp_p", dict(noise_p=NAN)), ("amp_v", dict(noise_v=-0.5)), ("amp_v", dict(noise_v=INF)),
       ("amp_v", dict(noise_v=NAN)), ("gain_p", dict(gain_p=0.0)), ("gain_p", dict(gain_p=-0.5)), ("gain_p", dict(gain_p=np.nextafter(1.0, 2.0))),
       ("gain_p", dict(gain_p=NAN)), ("gain_v", dict(gain_v=0.0)), ("gain_v", dict(gain_v=1.5)), ("gain_v", dict(gain_v=NAN)), ("gain_v", dict(gain_v=INF))]
GOOD = [dict(), dict(noise_p=0.02, noise_v=0.05, gain_p=0.5, gain_v=1.0, seed=3), dict(gain_p=5e-324, gain_v=np.nextafter(1.0, 0.0))]


def test_set_measurement_refuses_bad_descriptors_by_name():
    """dmpc_set_measurement checks the descriptor before it looks at the context, as dmpc_set_feedback does, so its refusals show without a GPU; a
    good descriptor then meets the NULL context"""
    for field, bad in BAD:
        rc, msg = es.raw_set_measurement(None, ctx=None, **bad)
        assert rc == -1 and msg.startswith("dmpc_set_measurement: ") and field in msg and "ctx" not in msg, (bad, msg)
    for good in GOOD:
        rc, msg = es.raw_set_measurement(None, ctx=None, **good)
        assert rc == -1 and msg == "dmpc_set_measurement: ctx is NULL", (good, msg)


def test_sample_and_apply_host_refuse_bad_descriptors_and_shapes():
    c = fb.random_column(2, 3, 3, 1)
    eh = es.random_belief(2, 3, 1)
    args = _args(c, eh)
    src = dict(c, v_rows=c["v"], eh_p=eh[0], eh_v=eh[1])
    for field, bad in BAD:
        rc, msg, mp, mv = es.raw_sample(2, 3, 1, **bad)
        assert rc == -1 and msg.startswith("dmpc_measurement_sample: ") and field in msg and (mp == 7.0).all() and (mv == 7.0).all(), (bad, msg)
        rc, msg, o = es.raw_apply((0.05, 0.25, 1), bad, H, 1, *args)
        assert rc == -1 and msg.startswith("dmpc_estimate_apply_host: ") and field in msg, (bad, msg)
        assert all(o[k].tobytes() == np.asarray(src[k]).tobytes() for k in OUT if k != "event"), bad   # nothing written
    for good in GOOD:
        assert es.raw_sample(2, 3, 1, **good)[0] == 0 and es.raw_apply((0.05, 0.25, 1), good, H, 1, *args)[0] == 0, good
    for bad in ((NAN, 0.0, 0), (-1e-9, 0.0, 0), (0.05, 0.25, 2)):   # the policy's refusals, as dmpc_feedback_apply_host
        rc, msg, _ = es.raw_apply(bad, _meas(), H, 1, *args)
        assert rc == -1 and msg.startswith("dmpc_estimate_apply_host: "), (bad, msg)
    for kw in (dict(k=0), dict(S=0), dict(n=0), dict(n=4), dict(dist=dict(pushes=[di.push(2, 0, 1)])), dict(dist=dict(noise_p=-1.0))):
        k = kw.pop("k", 1)
        rc, msg, _ = es.raw_apply((0.05, 0.25, 1), _meas(), H, k, *args, **kw)
        assert rc == -1 and msg.startswith("dmpc_estimate_apply_host: "), (kw, msg)
    for S, n, k in ((0, 3, 1), (2, 0, 1), (2, 3, -1)):
        rc, msg, _, _ = es.raw_sample(S, n, k)
        assert rc == -1 and msg.startswith("dmpc_measurement_sample: "), (S, n, k, msg)
    L = _lib.load()
    f = _lib.DmpcFeedback(0.05, 0.25, 1)
    assert L.dmpc_estimate_apply_host(None, None, None, H, 1, 1, 1, 1, *[None] * 16) == -1 and L.dmpc_last_error(None).decode() == "dmpc_estimate_apply_host: fb is NULL"
    assert L.dmpc_estimate_apply_host(C.byref(f), None, None, H, 1, 1, 1, 1, *[None] * 16) == -1 and L.dmpc_last_error(None).decode() == "dmpc_estimate_apply_host: m is NULL"
    assert L.dmpc_measurement_sample(None, 1, 1, 1, None, None) == -1 and L.dmpc_last_error(None).decode().startswith("dmpc_measurement_sample: ")
    # the Python layer's own shape checks, and its pass-through of the library's message
    with pytest.raises(_lib.DmpcError, match="^estimate_apply: "):
        _lib.estimate_apply(0.05, 0.25, 1, H, 1, c["p"][:, :, :44], *args[1:])
    with pytest.raises(_lib.DmpcError, match="^estimate_apply: "):
        _lib.estimate_apply(0.05, 0.25, 1, H, 1, *args[:11], eh[0][:, :2], *args[12:])
    with pytest.raises(_lib.DmpcError, match="^dmpc_estimate_apply_host: "):
        _lib.estimate_apply(0.05, 0.25, 1, H, 1, *args, measure=dict(gain_p=2.0))
    with pytest.raises(_lib.DmpcError, match="^dmpc_measurement_sample: "):
        _lib.measurement_sample(1, 1, 1, noise_p=-1.0)


# ---- 2. the noise ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n", [(1, 1), (2, 65)])
def test_measurement_sample_equals_the_restatement_byte_for_byte(S, n):
    for seed, amp in ((1, (0.02, 0.05)), (2 ** 63 + 5, (0.04, 0.0)), (0, (0.0, 0.0))):
        for k in (1, 2, 40):
            rc, msg, mp, mv = es.raw_sample(S, n, k, noise_p=amp[0], noise_v=amp[1], seed=seed)
            want = es.sample(S, n, k, amp[0], amp[1], seed)
            assert rc == 0 and mp.tobytes() == want[0].tobytes() and mv.tobytes() == want[1].tobytes(), (seed, amp, k, msg)
            if amp[0] > 0:
                assert (np.abs(mp) <= amp[0]).all() and np.abs(mp).max() > 0.5 * amp[0] or n == 1
    got = _lib.measurement_sample(S, n, 2, noise_p=0.02, noise_v=0.05, seed=9)
    want = es.sample(S, n, 2, 0.02, 0.05, 9)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_measurement_sample_column_0_is_zero_and_the_stream_is_not_the_disturbances():
    rc, _, mp, mv = es.raw_sample(2, 5, 0, noise_p=0.02, noise_v=0.05, seed=4)
    assert rc == 0 and not mp.any() and not mv.any() and not np.signbit(mp).any()
    # equal seeds, equal amplitudes, no wind and no push: the disturbance is amp * u of ITS stream
    for k in (1, 7):
        dp, dv = _lib.disturbance_sample(H, 2, 5, k, noise_p=0.02, noise_v=0.05, seed=4)
        _, _, mp, mv = es.raw_sample(2, 5, k, noise_p=0.02, noise_v=0.05, seed=4)
        assert (dp != mp).all() and (dv != mv).all(), k
    # columns differ among themselves, scenes and agents too
    _, _, a, _ = es.raw_sample(2, 5, 1, noise_p=0.02, seed=4)
    _, _, b, _ = es.raw_sample(2, 5, 2, noise_p=0.02, seed=4)
    assert (a != b).all() and (a[0] != a[1]).all() and (a[:, 0] != a[:, 1]).all()


# ---- 3. the rule ----------------------------------------------------------------------------------------------------------------------------
def _dists(S, n):
    return {"none": None,
            "wind, noise, push": dict(noise_p=2e-3, noise_v=1e-2, seed=7, wind=np.arange(3.0 * S).reshape(S, 3) * 0.1 - 0.2,
                                      pushes=[di.push(S - 1, n - 1, 2, dp=(0.1, 0.0, -0.1), dv=(0.0, 0.3, 0.0)), di.push(0, 0, 3, dp=(0.0, 0.2, 0.0))])}


POLICIES = ((0.0, 0.0, 0), (0.0, 0.0, 1), (0.05, 0.25, 1), (0.05, 0.25, 0), (INF, INF, 1), (INF, 0.25, 1), (0.05, INF, 0))


def _same(got, want, what, keys=OUT):
    for key in keys:
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), (what, key)


def _want(pol, meas, k, S, n, args, dist, sd):
    dp, dv = di.sample(H, S, n, k, **dist) if dist else (None, None)
    mp, mv = es.sample(S, n, k, meas["noise_p"], meas["noise_v"], meas["seed"])
    return es.column(*pol, H, *args, (meas["noise_p"], meas["noise_v"], meas["gain_p"], meas["gain_v"]), mp, mv, dp, dv, sd)


@pytest.mark.parametrize("S,n", [(1, 1), (2, 64), (2, 65)])
def test_apply_host_equals_the_restatement_byte_for_byte(S, n):
    N = n + (5 if n == 65 else 0)   # (a table wider than the commanded agents: the stride is N)
    c = fb.random_column(S, n, N, 100 * S + n)
    eh = es.random_belief(S, n, 100 * S + n)
    assert (c["status"] & 1).any() or n == 1
    args = _args(c, eh)
    src = dict(c, v_rows=c["v"], eh_p=eh[0], eh_v=eh[1])
    done = np.zeros(S, dtype=np.int32)
    done[S - 1] = S > 1   # a finished scene
    seen = set()
    for dname, dist in _dists(S, n).items():
        for gain in GAINS:
            for amp in ((0.02, 0.05), (0.0, 0.05), (0.0, 0.0)):
                meas = _meas(amp, gain, seed=11)
                for pol in POLICIES:
                    for k, sd in ((2, None), (3, done)):
                        want = _want(pol, meas, k, S, n, args, dist, sd)
                        rc, msg, got = es.raw_apply(pol, meas, H, k, *args, dist=dist, scene_done=sd)
                        assert rc == 0, msg
                        _same(got, want, (dname, gain, amp, pol, k))
                        seen.add((int(want["event"].sum()) > 0, int((want["event"] == 0).sum()) > 0))
                        if sd is not None and S > 1:   # the finished scene: nothing of it moved
                            assert all(np.array_equal(got[key][S - 1], np.asarray(src[key])[S - 1]) for key in OUT if key != "event")
        # the Python form returns the same
        meas = _meas((0.02, 0.05), (1.0, 0.25), seed=11)
        got = _lib.estimate_apply(0.05, 0.25, 1, H, 2, *args, scene_done=done, disturb=dist, measure=meas)
        _same(got, _want((0.05, 0.25, 1), meas, 2, S, n, args, dist, done), dname)
    assert (True, True) in seen or n == 1   # columns with events and columns with agents that had none


@pytest.mark.parametrize("S,n", [(1, 1), (2, 65)])
def test_without_noise_and_with_gain_1_it_is_the_feedback_rule_byte_for_byte(S, n):
    c = fb.random_column(S, n, n, 31 * S + n)
    eh = es.random_belief(S, n, 5)
    args = _args(c, eh)
    fargs = [c[k] for k in COLUMN] + [c["lT_next"]]
    for dname, dist in _dists(S, n).items():
        for pol in POLICIES:
            rc, msg, got = es.raw_apply(pol, es.NO_NOISE, H, 2, *args, dist=dist)
            rc2, _, want = fb.raw_apply(pol, H, 2, *fargs, dist=dist)
            assert rc == 0 and rc2 == 0, msg
            _same(got, want, (dname, pol), [k for k in OUT if k not in ("eh_p", "eh_v")])
            # the belief: 0 after an event, the deviation g otherwise -- which is what the rule left in e
            ev = got["event"][..., None] != 0
            assert got["eh_p"].tobytes() == np.where(ev, 0.0, got["e_p"]).tobytes() and got["eh_v"].tobytes() == np.where(ev, 0.0, got["e_v"]).tobytes()
            g = fb.column(*pol, H, *fargs, *(di.sample(H, S, n, 2, **dist) if dist else (None, None)))
            assert np.array_equal(got["eh_p"], np.where(ev, 0.0, g["g_p"])) and np.array_equal(got["eh_v"], np.where(ev, 0.0, g["g_v"]))


def test_the_measurement_never_moves_the_vehicle_and_an_event_keeps_what_the_estimate_missed():
    S, n = 2, 9
    c = fb.random_column(S, n, n, 77)
    eh = es.random_belief(S, n, 77)
    args = _args(c, eh)
    fargs = [c[k] for k in COLUMN] + [c["lT_next"]]
    dist = _dists(S, n)["wind, noise, push"]
    _, _, plain = fb.raw_apply((0.0, 0.0, 1), H, 2, *fargs, dist=dist)
    for gain in GAINS:
        meas = _meas((0.02, 0.05), gain, seed=3)
        rc, _, got = es.raw_apply((0.0, 0.0, 1), meas, H, 2, *args, dist=dist)
        assert rc == 0 and got["event"].all()
        for key in ("x_p", "x_v", "x_a"):
            assert got[key].tobytes() == plain[key].tobytes(), (gain, key)
        w = _want((0.0, 0.0, 1), meas, 2, S, n, args, dist, None)
        g = np.concatenate([w["g_p"], w["g_v"]], axis=-1)
        assert np.array_equal(np.concatenate([got["e_p"], got["e_v"]], axis=-1), g - w["gh"]) and got["e_p"].any()
        assert not got["eh_p"].any() and not got["eh_v"].any()
        # the planner is set to q + gh: off the vehicle by exactly what stays in e (up to the rounding of the two sums)
        assert np.abs((got["x_p"] - got["xh_p"]) - got["e_p"]).max() < 1e-14


# ---- 4. the head-on scene with the oracle's step --------------------------------------------------------------------------------------------
KT, TOL = 60, 0.1
TRIG = (0.05, 0.25, 1)
PUSH = dict(pushes=[di.push(0, 0, 5, dp=(0.0, 0.15, 0.0))])
COLL = 2   # DMPC_ST_COLL


@functools.lru_cache(maxsize=None)
def _plain():
    """the head-on flight with no policy, no disturbance and no measurement (shared: do not modify)"""
    from oracle import oracle as orc
    po, pf = stt.head_on()
    return stt.rest_loop(mi.oracle_step(orc, orc.make_params("bound", **ob.KW)), po, pf, KT, TOL)


@functools.lru_cache(maxsize=None)
def _oracle_loop(amp, gain, seed, push=False):
    """the restated loop over oracle.step on start.head_on() (shared: do not modify)"""
    from oracle import oracle as orc
    po, pf = stt.head_on()
    return es.loop(fb.oracle_batch_step(orc, orc.make_params("bound", **ob.KW)), po[None], pf[None], KT, TOL, H, TRIG, _meas(amp, (gain, gain), seed),
                   PUSH if push else None)


def min_distance(pk, used):
    """the smallest collision-metric distance |E1 (p_i - p_j)| over the columns flown; pk [n,K_T,3]"""
    e1 = np.array([1.0, 1.0, 1.0 / ob.KW["c"]])
    n = pk.shape[0]
    return min(float(np.sqrt((((pk[i, k] - pk[j, k]) * e1) ** 2).sum())) for k in range(used) for i in range(n) for j in range(i))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_inside_the_trigger_is_the_plain_flight(seed):
    """(a): sqrt(3) * 0.02 < 0.05 and sqrt(3) * 0.05 < 0.25 -- with e = 0 the estimate is the noise alone, which never passes the trigger"""
    plain, res = _plain(), _oracle_loop((0.02, 0.05), 1.0, seed)
    used = int(plain["K_T_used"])
    print(f"seed {seed}: {len(res['events'])} events, {int(res['K_T_used'][0])} columns (plain {used}), smallest distance {min_distance(res['pk'][0], used):.4f} m, "
          f"largest estimation error {res['est']['err_p_max'].max():.4f} m, {res['est']['err_v_max'].max():.4f} m/s")
    assert res["events"] == [] and int(res["K_T_used"][0]) == used and int(res["scene_status"][0]) == int(plain["scene_status"])
    for key in ("pk", "vk", "ak"):
        assert np.array_equal(res[key][0], plain[key]), key
    assert 0 < res["est"]["err_p_max"].max() <= np.sqrt(3) * 0.02 * (1 + 1e-12) and not res["est"]["dev_p_max"].any()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_beyond_the_trigger_makes_false_events_and_a_gain_below_1_makes_fewer(seed):
    """(b)"""
    hi, lo = _oracle_loop((0.04, 0.05), 1.0, seed), _oracle_loop((0.04, 0.05), 0.5, seed)
    for gain, r in ((1.0, hi), (0.5, lo)):
        print(f"seed {seed}, gain {gain}: {len(r['events'])} events, {int(r['K_T_used'][0])} columns, status {int(r['scene_status'][0])}"
              f"{' (DMPC_ST_COLL)' if int(r['scene_status'][0]) & COLL else ''}, smallest distance {min_distance(r['pk'][0], int(r['K_T_used'][0])):.4f} m")
    assert len(hi["events"]) >= 1
    assert len(lo["events"]) < len(hi["events"])
    assert not hi["est"]["dev_p_max"].max() == 0.0   # an event leaves e = g - gh behind: the true deviation is no longer 0


def test_the_push_is_seen_on_its_column_at_both_gains():
    """(c)"""
    cut = ob.KW["rmin"] - 0.05
    for gain in (1.0, 0.5):
        r = _oracle_loop((0.02, 0.05), gain, 1, True)
        used = int(r["K_T_used"][0])
        print(f"gain {gain}: events {r['events']}, {used} columns, status {int(r['scene_status'][0])}, smallest distance {min_distance(r['pk'][0], used):.4f} m "
              f"(rmin - 0.05 = {cut:.2f} m)")
        assert (5, 0, 0) in r["events"] and all(i == 0 for _, _, i in r["events"])
        assert r["log"]["event_first"].tolist() == [[5, -1]] and r["est"]["dev_p_col"][0, 0] >= 5
