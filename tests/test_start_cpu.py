"""CPU: start in motion -- the four entries are declared, exported and bound; the braking plan on the host (dmpc_start_plan: no context, no GPU)
against the numpy restatement of tests/start.py, byte for byte; and the scene conditions the GPU tests rely on, checked with the oracle's MPC step
in start.start_loop.  The GPU side (tests/test_gpu_start.py) compares dmpc_set_start / dmpc_flight_end with the same loops."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mission as mi
import obstacles as ob
import start as st
from helpers import ROOT
from multiagent_planning_amd import _lib

ENTRIES = ("dmpc_set_start", "dmpc_flight_end", "dmpc_start_plan", "dmpc_start_plan_device")
H, ALIM = ob.KW["h"], ob.KW["alim"]


def _host_only():
    """a Dmpc without a context: what the methods refuse before they touch one, and the host-only start_plan"""
    d = object.__new__(_lib.Dmpc)
    d._L, d._ctx, d.prm = _lib.load(), None, _lib.make_params("bound", **ob.KW)
    return d


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "dmpc_hip.h")).read()
    L = _lib.load()
    assert L.dmpc_abi_version() == 8 == _lib.ABI_VERSION and re.search(r"#define DMPC_ABI_VERSION 8\b", header)
    for name in ENTRIES:
        assert re.search(r"DMPC_API int " + name + r"\(", header), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for words in ("THE START IS CONSUMED BY ONE FLIGHT", "COLUMN 0 IS THE CALLER'S COLUMN col0"):
        assert words in header
    for method in ("set_start", "clear_start", "flight_end", "start_plan", "starting"):
        assert callable(getattr(_lib.Dmpc, method))
    # the struct the binding passes is the header's: field order and size
    fields = re.search(r"typedef struct dmpc_start \{(.*?)\} dmpc_start;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in decl.split(None, 2 if "const" in decl else 1)[-1].split(",")]
    assert names == [f[0] for f in _lib.DmpcStart._fields_]
    assert C.sizeof(_lib.DmpcStart) == 72


def test_null_context_is_refused_by_name():
    L = _lib.load()
    z = np.zeros((1, 1, 45))
    s = _lib.DmpcStart(1, 1, 0)
    calls = dict(dmpc_set_start=lambda: L.dmpc_set_start(None, C.byref(s)),
                 dmpc_flight_end=lambda: L.dmpc_flight_end(None, 1, 1, *[_lib._dpn(None)] * 6, _lib._ipn(None)),
                 dmpc_start_plan_device=lambda: L.dmpc_start_plan_device(None, 1, *[z.ctypes.data] * 6, None))
    for name, call in calls.items():
        assert call() == -1 and L.dmpc_last_error(None).decode() == name + ": ctx is NULL"
    # dmpc_start_plan takes no context: its refusals
    prm = _lib.make_params("bound", **ob.KW)
    x = np.zeros((2, 3))
    for bad in (dict(n=0), dict(n=-1), dict(prm=None), dict(x_p=None)):
        args = dict(prm=C.byref(prm), n=2, x_p=x)
        args.update(bad)
        assert L.dmpc_start_plan(args["prm"], args["n"], _lib._dpn(args["x_p"]), _lib._dp(x), _lib._dp(x), *[_lib._dp(np.zeros((2, 45)))] * 3) == -1
        assert L.dmpc_last_error(None).decode().startswith("dmpc_start_plan: "), bad


def test_binding_refusals():
    d = _host_only()
    v, p = np.zeros((2, 3, 3)), np.zeros((2, 3, 45))
    bad = [dict(vo=np.zeros((2, 3, 4))), dict(vo=np.zeros(3)), dict(vo=v, ao=np.zeros((2, 4, 3))), dict(vo=v, plan=np.zeros((2, 3, 44))),
           dict(vo=v, plan=(p, p)), dict(vo=v, from_end=True), dict(plan=p, from_end=True), dict(vo=v, src_scene=[0, 1]), dict(), dict(col0=3),
           dict(from_end=True), dict(vo=v, S=3), dict(vo=v, N_cmd=2), dict(vo=np.zeros((3, 3)), plan=p)]
    for kw in bad:
        with pytest.raises(_lib.DmpcError, match="^set_start: "):
            d.set_start(**kw)
    with pytest.raises(_lib.DmpcError, match="^flight_end: "):
        d.flight_end(0, 2)
    for shapes in (((2, 3), (2, 3), (3, 3)), ((2, 4),) * 3, ((0, 3),) * 3):
        with pytest.raises(_lib.DmpcError, match="^start_plan: "):
            d.start_plan(*[np.zeros(s) for s in shapes])


@pytest.mark.parametrize("n", [1, 7, 300])
def test_host_braking_plan_equals_the_restatement_byte_for_byte(n):
    d = _host_only()
    rng = np.random.default_rng(70 + n)
    x_p, x_a = rng.uniform(-2, 2, (n, 3)), rng.uniform(-1, 1, (n, 3))
    cases = {"random": rng.uniform(-0.5, 0.5, (n, 3)), "rest": np.zeros((n, 3)), "negative zero": -np.zeros((n, 3)),
             "clamped": rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(ALIM * H, 14 * ALIM * H, (n, 3)),
             "exactly the clamp": np.full((n, 3), ALIM * H), "beyond the horizon": np.full((n, 3), 20 * ALIM * H)}
    for name, x_v in cases.items():
        got, want = d.start_plan(x_p, x_v, x_a), st.brake_plan(x_p, x_v, x_a)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), name
        rc, raw = st.raw_start_plan(d, x_p, x_v, x_a)
        assert rc == 0 and all(r.tobytes() == w.tobytes() for r, w in zip(raw, want)), name
        p, v, a = want
        assert np.array_equal(p[:, :3], x_p) and np.array_equal(v[:, :3], x_v) and np.array_equal(a[:, :3], x_a)
        if name == "clamped":      # the clamp fires, and |v| <= 14 alim h still stops inside the plan: the last velocity is zero exactly
            assert (np.abs(a[:, 3:6]) == ALIM).all() and (v[:, 42:] == 0.0).all()
        if name in ("random", "rest", "negative zero", "exactly the clamp"):
            assert (v[:, 42:] == 0.0).all(), name
        if name == "rest":         # a fleet at rest gets the hover plan
            assert np.array_equal(p, np.tile(x_p, (1, 15))) and not v.any() and not a[:, 3:].any()
        if name == "beyond the horizon":
            assert (v[:, 42:] > 0.0).all() and (np.abs(a[:, 3:]) == ALIM).all()
    # the shapes of the method follow the states'
    one = d.start_plan(x_p[0], cases["random"][0], x_a[0])
    assert one[0].shape == (45,) and one[0].tobytes() == st.brake_plan(x_p[:1], cases["random"][:1], x_a[:1])[0].tobytes()


# ---- the scene conditions, by the oracle's loop -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step():
    from oracle import oracle as orc
    return mi.oracle_step(orc, orc.make_params("bound", **ob.KW))


@pytest.fixture(scope="module")
def whole(step):
    """the head-on flight from rest (shared: do not modify)"""
    po, pf = st.head_on()
    return st.rest_loop(step, po, pf, st.KT)


def test_head_on_reaches_its_goals_in_35_columns(whole):
    """the oracle's loop (solveSoftDMPCbound, obstacles.KW, error_tol 0.1): SOLVED | REACHED, K_T_used = 35"""
    print("head-on:", whole["K_T_used"], whole["scene_status"])
    assert whole["scene_status"] == st.REACHED
    assert whole["K_T_used"] == 35


@pytest.mark.parametrize("cut", [6, 8])
def test_a_cut_flight_continued_with_its_plan_is_the_whole_flight(step, whole, cut):
    """cut at columns 6 and 8 the fleet moves (measured 0.234 and 0.344 m/s)"""
    po, pf = st.head_on()
    u = whole["K_T_used"]
    first = st.rest_loop(step, po, pf, cut + 1)
    assert first["K_T_used"] == cut + 1 and first["scene_status"] == 1
    speed = np.linalg.norm(first["x_v"], axis=1).max()
    print("cut", cut, "speed", speed)
    assert abs(speed - {6: 0.23, 8: 0.34}[cut]) < 0.01
    rest = st.continue_loop(step, first, pf, st.KT - cut)
    assert rest["K_T_used"] == u - cut and rest["scene_status"] == st.REACHED
    for k in ("pk", "vk", "ak"):
        assert first[k][:, :cut + 1].tobytes() == whole[k][:, :cut + 1].tobytes()
        assert rest[k][:, :u - cut].tobytes() == whole[k][:, cut:u].tobytes()
        assert not rest[k][:, u - cut:].any()


@pytest.mark.parametrize("cut", [6, 8])
def test_the_braking_plan_flies_another_flight_than_the_carried_plan(step, whole, cut):
    """Started from the braking plan the flight still reaches, and differs from the whole flight by more than 1e-3 m (measured 1.5e-2 and 7.1e-3 m):
    the two kinds of plan can be told apart.  (Cut at column 7 the difference is 0.0 -- neither agent's solve builds a collision row from the
    other's braking plan there -- which is why the cuts are 6 and 8.)"""
    po, pf = st.head_on()
    u = whole["K_T_used"]
    first = st.rest_loop(step, po, pf, cut + 1)
    plan = st.brake_plan(first["x_p"], first["x_v"], first["x_a"])
    b = st.start_loop(step, first["x_p"], first["x_v"], first["x_a"], plan[0], pf, st.KT - cut)
    assert b["scene_status"] == st.REACHED
    n = min(b["K_T_used"], u - cut)
    diff = np.abs(b["pk"][:, :n] - whole["pk"][:, cut:cut + n]).max()
    print("cut", cut, "braking plan: K_T_used", b["K_T_used"], "difference", diff)
    assert diff > 1e-3


def test_deadline_mission_is_three_continued_transitions(step):
    s = mi.scene("deadline")
    m = mi.oracle_result("bound", "deadline")
    col = m["stage_col"]
    assert list(col[:2]) == [8, 18] and m["scene_status"] == mi.REACHED
    legs, end, k0 = [], None, 0
    for q in range(3):
        kt = (col[q] - k0 + 1) if q < 2 else mi.KT - k0
        leg = st.rest_loop(step, s["po"], s["goals"][q], kt, mi.ERROR_TOL) if end is None else st.continue_loop(step, end, s["goals"][q], kt, mi.ERROR_TOL)
        assert leg["K_T_used"] == (kt if q < 2 else m["K_T_used"] - k0) and leg["scene_status"] == (1 if q < 2 else mi.REACHED)
        legs.append(leg)
        end, k0 = leg, col[q]
    u = m["K_T_used"]
    for k in ("pk", "vk", "ak"):
        flown = np.concatenate([legs[0][k][:, :9], legs[1][k][:, 1:11], legs[2][k][:, 1:u - 18]], axis=1)
        assert flown.tobytes() == m[k][:, :u].tobytes(), k
    # pretending the fleet stands still on column 8 is another flight
    speed = np.linalg.norm(m["vk"][:, 8], axis=1).max()
    still = st.rest_loop(step, m["pk"][:, 8], s["goals"][1], 21, mi.ERROR_TOL)
    diff = np.linalg.norm(still["pk"][:, :21] - m["pk"][:, 8:29], axis=2).max()
    print("deadline: speed on column 8", speed, "difference within 20 columns", diff)
    assert speed > mi.SPEED_FLOOR and diff > 0.1
