"""ctypes binding of libdmpc_hip.so (the C ABI in include/dmpc_hip.h).

The shared library is built in-tree (multiagent_planning_amd/libdmpc_hip.so) by
`__graft_entry__.build()` / `make -C multiagent_planning_amd/csrc`.  There is no fallback of any
kind: if the library is missing, or no HIP device is present, the calls raise.
"""
import contextlib
import ctypes as C
import functools
import inspect
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdmpc_hip.so")

VARIANTS = dict(bound=0, bound2=1, all3=2, hard=3, ondemand=4, ellip=5, softall=6, repair=7, cpp=8, cpp2=9, cpp1=10, softall_c=11, scp=12)
ST_SOLVED, ST_OUTBOUND, ST_COLL, ST_INFEAS, ST_CAPACITY, ST_ITERCAP = 1, 2, 4, 8, 16, 32
PRECISIONS = dict(f64=0, mixed=1, f32factor=2, low=3)
ST_REACHED = 256   # scene_status of transition(): every agent reached its goal
PLAN_OK, PLAN_TRUNCATED, PLAN_UNREACHABLE = 0, 1, 2   # plan_status of plan()
ST_HELD = 64       # transition(on_fail="hold") / mission(on_fail="hold") / route(on_fail="hold"): the agent flew its previous plan on this column
INFO_LEN = 8
I_VIOLK, I_NROWS, I_TRIES, I_CASE, I_ITERS, I_NSLACK, I_NACTIVE, I_MAXQ = range(8)
K_HOR = 15
ABI_VERSION = 8    # DMPC_ABI_VERSION of include/dmpc_hip.h

# every symbol include/dmpc_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "dmpc_create", "dmpc_destroy", "dmpc_last_error", "dmpc_set_params", "dmpc_model_matrices",
    "dmpc_posvel_matrix", "dmpc_init_batch", "dmpc_step_batch", "dmpc_solve_one", "dmpc_step_device",
    "dmpc_table_from_rows_device", "dmpc_advance_device", "dmpc_transition", "dmpc_solve_count",
    "dmpc_profile", "dmpc_profile_read", "dmpc_profile_read2", "dmpc_rows_one", "dmpc_postcheck",
    "dmpc_coll_rows", "dmpc_coll_rows_device", "dmpc_add_coll_constr", "dmpc_add_coll_constr_device",
    "dmpc_trajectories2file", "dmpc_test2file", "dmpc_random_test", "dmpc_random_exchange", "dmpc_random_sets_device",
    "dmpc_prop_state", "dmpc_is_inbounds", "dmpc_reached_goal", "dmpc_rows_dense",
    "dmpc_partition", "dmpc_comm_unique_id", "dmpc_comm_init", "dmpc_comm_destroy", "dmpc_step_sharded_device",
    "dmpc_transition_sharded", "dmpc_transition_sharded_gather", "dmpc_group_size", "dmpc_comm_size", "dmpc_abi_version", "dmpc_last_solve_kernel",
    "dmpc_max_deviation",
    "dmpc_step_batch_cmd", "dmpc_step_device_cmd", "dmpc_transition_cmd", "dmpc_postcheck_cmd",
    "dmpc_transition_scripted", "dmpc_scripted_cols_device", "dmpc_postcheck_scripted",
    "dmpc_postcheck_clearance",
    "dmpc_transition_mission",
    "dmpc_postcheck_setpoints",
    "dmpc_transition_hold",
    "dmpc_assign_goals", "dmpc_assign_goals_device",
    "dmpc_assign_rect", "dmpc_assign_rect_device",
    "dmpc_transition_route",
    "dmpc_plan_routes", "dmpc_plan_routes_device",
    "dmpc_transition_replan", "dmpc_replan_routes_device",
    "dmpc_set_disturbance", "dmpc_disturbance_sample", "dmpc_disturb_device",
    "dmpc_set_start", "dmpc_flight_end", "dmpc_start_plan", "dmpc_start_plan_device",
    "dmpc_set_feedback", "dmpc_feedback_device", "dmpc_feedback_apply_host", "dmpc_feedback_log",
    "dmpc_set_measurement", "dmpc_measurement_sample", "dmpc_estimate_device", "dmpc_estimate_apply_host", "dmpc_estimate_log",
]


class DmpcParams(C.Structure):
    _fields_ = [
        ("K", C.c_int32), ("variant", C.c_int32), ("order", C.c_int32), ("max_tries", C.c_int32),
        ("h", C.c_double), ("rmin", C.c_double), ("c", C.c_double), ("alim", C.c_double),
        ("Q1", C.c_double), ("S1", C.c_double), ("term", C.c_double),
        ("pmin", C.c_double * 3), ("pmax", C.c_double * 3),
        ("Qfar", C.c_double), ("Qnear", C.c_double), ("Sfree", C.c_double),
        ("tol", C.c_double),
    ]


class DmpcPush(C.Structure):
    _fields_ = [("scene", C.c_int32), ("agent", C.c_int32), ("column", C.c_int32), ("dp", C.c_double * 3), ("dv", C.c_double * 3)]


class DmpcDisturbance(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("amp_p", C.c_double), ("amp_v", C.c_double), ("wind", C.POINTER(C.c_double)), ("wind_scenes", C.c_int),
                ("push", C.POINTER(DmpcPush)), ("n_push", C.c_int)]


class DmpcStart(C.Structure):
    _fields_ = [("S", C.c_int32), ("N_cmd", C.c_int32), ("from_end", C.c_int32), ("src_scene", C.POINTER(C.c_int32)),
                ("vo", C.POINTER(C.c_double)), ("ao", C.POINTER(C.c_double)), ("plan_p", C.POINTER(C.c_double)), ("plan_v", C.POINTER(C.c_double)),
                ("plan_a", C.POINTER(C.c_double)), ("col0", C.c_int32)]


class DmpcFeedback(C.Structure):
    _fields_ = [("trigger_p", C.c_double), ("trigger_v", C.c_double), ("reanchor", C.c_int32)]


class DmpcMeasurement(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("amp_p", C.c_double), ("amp_v", C.c_double), ("gain_p", C.c_double), ("gain_v", C.c_double)]


class DmpcError(RuntimeError):
    pass


_lib = None


def load():
    """Load libdmpc_hip.so; raises DmpcError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own libamdhip64; two HIP runtimes in one process only work if torch's is
    # loaded first (then this library binds to the same runtime by soname).  Import torch, when present,
    # before loading -- it is the device-memory / stream / RCCL plumbing of the callers anyway.
    try:
        import torch  # noqa: F401
    except Exception:   # torch is optional for the pure C-ABI use
        pass
    if not os.path.exists(LIB_PATH):
        raise DmpcError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C multiagent_planning_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    # the header revision these bindings were written against (DMPC_ABI_VERSION: the special device values DEVICE_ALL / DEVICE_CURRENT below
    # changed once between revisions): refuse another library instead of passing it values that mean something else there
    # (DMPC_SKIP_ABI_CHECK=1: development A/B runs against an older build of the library, tools/with_lib.py)
    if not os.environ.get("DMPC_SKIP_ABI_CHECK") and (not hasattr(L, "dmpc_abi_version") or L.dmpc_abi_version() != ABI_VERSION):
        raise DmpcError(f"{LIB_PATH}: ABI revision {L.dmpc_abi_version() if hasattr(L, 'dmpc_abi_version') else '< 5'}, these bindings need {ABI_VERSION}: rebuild the library")
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    pp = C.POINTER(DmpcParams)
    L.dmpc_create.restype = vp
    L.dmpc_create.argtypes = [pp, C.c_int, C.c_int]
    L.dmpc_destroy.restype = None
    L.dmpc_destroy.argtypes = [vp]
    L.dmpc_last_error.restype = C.c_char_p
    L.dmpc_last_error.argtypes = [vp]
    L.dmpc_set_params.argtypes = [vp, pp]
    L.dmpc_model_matrices.argtypes = [pp, dp, dp, dp, dp]
    L.dmpc_posvel_matrix.argtypes = [C.c_double, C.c_int, dp]
    L.dmpc_init_batch.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp]
    L.dmpc_step_batch.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip]
    L.dmpc_solve_one.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip]
    L.dmpc_rows_one.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, C.c_int, dp, dp, dp, ip, ip, ip, ip]
    L.dmpc_step_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 12
    L.dmpc_table_from_rows_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.dmpc_advance_device.argtypes = [vp, C.c_int] + [vp] * 8
    L.dmpc_transition.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_int, C.c_double, dp, dp, dp, ip, ip]
    i64 = C.c_int64
    L.dmpc_coll_rows.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, dp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, dp,
                                 C.c_int, C.c_int, i64, i64, dp, i64, i64, dp, dp]
    L.dmpc_coll_rows_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, vp, i64, i64,
                                        C.c_int, vp, i64, i64, vp, vp, vp]
    L.dmpc_add_coll_constr.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, dp, C.c_int, i64, i64, dp, i64, i64, dp]
    L.dmpc_add_coll_constr_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_double, C.c_double, vp, i64, i64, C.c_int, vp, i64,
                                              i64, vp, vp]
    L.dmpc_trajectories2file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double, dp, dp, dp, dp, dp, dp, dp]
    L.dmpc_test2file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, dp, dp, dp]
    L.dmpc_random_test.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, C.c_uint64, dp, dp]
    L.dmpc_random_exchange.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_uint64, dp, dp]
    L.dmpc_random_sets_device.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, C.c_uint64, C.c_int, vp, vp]
    L.dmpc_rows_dense.argtypes = [vp, C.c_int, dp, ip, dp, C.c_int, C.c_int, i64, i64, dp, i64, i64]
    L.dmpc_prop_state.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp]
    L.dmpc_is_inbounds.argtypes = [vp, C.c_int, dp, dp, dp, ip]
    L.dmpc_reached_goal.argtypes = [vp, C.c_int, dp, dp, C.c_double, ip]
    L.dmpc_max_deviation.argtypes = [vp, C.c_int, dp, dp, dp]
    L.dmpc_postcheck.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, ip, dp, dp, dp, dp, C.c_double, C.c_double, C.c_double,
                                 dp, dp, ip, dp, ip, dp, dp, dp, C.c_int]
    # uncommanded vehicles (ABI revision 8)
    L.dmpc_step_batch_cmd.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip]
    L.dmpc_step_device_cmd.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [vp] * 12
    L.dmpc_transition_cmd.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_double, dp, dp, dp, ip, ip]
    L.dmpc_postcheck_cmd.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, dp, dp, dp, dp, dp, C.c_double, C.c_double, C.c_double,
                                     dp, dp, ip, dp, ip, dp, dp, dp, C.c_int, dp, ip]
    # scripted vehicles: uncommanded vehicles that follow a path (additive, still revision 8)
    L.dmpc_transition_scripted.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, dp, C.c_int, C.c_double, dp, dp, dp, ip, ip]
    L.dmpc_scripted_cols_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
    L.dmpc_postcheck_scripted.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, dp, dp, dp, dp, dp, C.c_int, C.c_double, C.c_double,
                                          C.c_double, dp, dp, ip, dp, ip, dp, dp, dp, C.c_int, dp, ip, dp]
    # clearance report: nearest vehicle, and when, per agent (additive, still revision 8)
    L.dmpc_postcheck_clearance.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, dp, dp, dp, dp, dp, C.c_int, C.c_double, C.c_double,
                                           C.c_double, C.c_double, dp, ip, ip]
    # missions: a transition through a sequence of goal sets (additive, still revision 8)
    L.dmpc_transition_mission.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, ip, dp, C.c_int, C.c_int, C.c_double, dp, dp, dp, ip, ip, ip]
    L.dmpc_transition_hold.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, ip, dp, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, dp, ip, ip, ip,
                                       ip, ip, ip]
    # flight setpoints p, v, a at 100 Hz and the limits report (additive, still revision 8)
    L.dmpc_postcheck_setpoints.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, ip, dp, dp, dp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                           dp, dp, dp, dp, ip, dp, ip, dp, dp, ip]
    # goal assignment ahead of a transition (additive, still revision 8)
    L.dmpc_assign_goals.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_int, ip, dp, dp, dp, ip]
    L.dmpc_assign_goals_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_double, C.c_int, vp, vp, vp, vp, vp, vp]
    # rectangular goal assignment: N agents, M goals (additive, still revision 8)
    L.dmpc_assign_rect.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, C.c_int, ip, ip, dp, dp, dp, ip]
    L.dmpc_assign_rect_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_double, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    # routes: every agent through waypoints of its own (additive, still revision 8)
    L.dmpc_transition_route.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, ip, C.c_double, C.c_int, dp, C.c_int, C.c_int, C.c_double, C.c_int,
                                        dp, dp, dp, ip, ip, ip, ip, ip, ip, ip]
    # route planning round static vehicles, ahead of route() (additive, still revision 8)
    L.dmpc_plan_routes.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, dp, C.c_double, C.c_double, dp, ip, ip, ip]
    L.dmpc_plan_routes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp, vp, vp]
    # re-planned routes: plan_routes, transition_route and re-plans during the flight (additive, still revision 8)
    L.dmpc_transition_replan.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, dp,
                                         C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, dp, ip, ip, dp, ip, ip, ip, ip, ip, ip, ip, ip, ip]
    L.dmpc_replan_routes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp, vp, vp, vp, vp,
                                            vp, vp, vp, vp, vp]
    # disturbed transitions: wind, noise and pushes on the state, in the loop (additive, still revision 8)
    if hasattr(L, "dmpc_set_disturbance"):   # (absent from the older builds tools/with_lib.py may load)
        L.dmpc_set_disturbance.argtypes = [vp, C.POINTER(DmpcDisturbance)]
        L.dmpc_disturbance_sample.argtypes = [C.POINTER(DmpcDisturbance), C.c_double, C.c_int, C.c_int, C.c_int, dp, dp]
        L.dmpc_disturb_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    # start in motion: a flight from a given or carried state and plan (additive, still revision 8)
    if hasattr(L, "dmpc_set_start"):   # (absent from the older builds tools/with_lib.py may load)
        L.dmpc_set_start.argtypes = [vp, C.POINTER(DmpcStart)]
        L.dmpc_flight_end.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, ip]
        L.dmpc_start_plan.argtypes = [pp, C.c_int, dp, dp, dp, dp, dp, dp]
        L.dmpc_start_plan_device.argtypes = [vp, C.c_int] + [vp] * 7
    # event-triggered feedback: the planning state apart from the true state (additive, still revision 8)
    if hasattr(L, "dmpc_set_feedback"):   # (absent from the older builds tools/with_lib.py may load)
        L.dmpc_set_feedback.argtypes = [vp, C.POINTER(DmpcFeedback)]
        L.dmpc_feedback_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 15
        L.dmpc_feedback_apply_host.argtypes = [C.POINTER(DmpcFeedback), C.POINTER(DmpcDisturbance), C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                               dp, dp, dp, ip, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip]
        L.dmpc_feedback_log.argtypes = [vp, C.c_int, C.c_int, ip, ip, ip, dp, ip, dp, ip, dp, dp, dp, dp]
    # measured state: sensor noise and a fixed-gain estimate in the loop (additive, still revision 8)
    if hasattr(L, "dmpc_set_measurement"):   # (absent from the older builds tools/with_lib.py may load)
        L.dmpc_set_measurement.argtypes = [vp, C.POINTER(DmpcMeasurement)]
        L.dmpc_measurement_sample.argtypes = [C.POINTER(DmpcMeasurement), C.c_int, C.c_int, C.c_int, dp, dp]
        L.dmpc_estimate_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 17
        L.dmpc_estimate_apply_host.argtypes = [C.POINTER(DmpcFeedback), C.POINTER(DmpcMeasurement), C.POINTER(DmpcDisturbance), C.c_double, C.c_int, C.c_int,
                                               C.c_int, C.c_int, dp, dp, dp, ip, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip]
        L.dmpc_estimate_log.argtypes = [vp, C.c_int, C.c_int, dp, ip, dp, ip, dp, ip, dp, ip, dp, dp]
    L.dmpc_partition.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip]
    L.dmpc_comm_unique_id.argtypes = [C.c_char_p]
    L.dmpc_comm_init.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    L.dmpc_comm_destroy.argtypes = [vp]
    L.dmpc_comm_size.argtypes = [vp]
    L.dmpc_step_sharded_device.argtypes = [vp, C.c_int, C.c_int] + [vp] * 12
    L.dmpc_transition_sharded.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_int, C.c_double, dp, dp, dp, ip, ip]
    L.dmpc_transition_sharded_gather.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_int, C.c_double, dp, dp, dp, ip, ip]
    L.dmpc_group_size.argtypes = [vp]
    L.dmpc_debug_emulate_devices.argtypes = [C.c_int]
    L.dmpc_debug_option.argtypes = [vp, C.c_char_p, C.c_int]
    if hasattr(L, "dmpc_debug_read_grid"):   # (absent from the older builds tools/with_lib.py may load)
        L.dmpc_debug_read_grid.argtypes = [vp, ip, vp, C.c_size_t]
    L.dmpc_solve_count.restype = C.c_int64
    L.dmpc_solve_count.argtypes = [vp]
    L.dmpc_profile.argtypes = [vp, C.c_int]
    L.dmpc_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.dmpc_profile_read2.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.dmpc_last_solve_kernel.argtypes = [vp]
    L.dmpc_last_solve_kernel.restype = C.c_char_p
    _lib = L
    return L


def make_params(variant="bound", K=K_HOR, h=0.2, rmin=0.35, c=2.0, alim=1.0, Q1=1000.0, S1=100.0, term=-5e4,
                pmin=(-2.5, -2.5, 0.2), pmax=(2.5, 2.5, 2.2), order=2, max_tries=0, Qfar=0.0, Qnear=0.0, Sfree=0.0, tol=2.0):
    p = DmpcParams()
    p.K, p.order, p.max_tries = int(K), int(order), int(max_tries)
    p.variant = VARIANTS[variant] if isinstance(variant, str) else int(variant)
    p.h, p.rmin, p.c, p.alim, p.Q1, p.S1, p.term = float(h), float(rmin), float(c), float(alim), float(Q1), float(S1), float(term)
    for i in range(3):
        p.pmin[i] = float(pmin[i])
        p.pmax[i] = float(pmax[i])
    p.Qfar, p.Qnear, p.Sfree = float(Qfar), float(Qnear), float(Sfree)
    p.tol = float(tol)
    return p


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _strided_base(A):
    """(pointer, row stride, column stride) in elements of a 2-D float64 array with positive strides (C or Fortran order,
    or a view): the ABI's A[i*rs + j*cs] addressing covers MATLAB's column-major arrays without a copy."""
    return A.ctypes.data_as(C.POINTER(C.c_double)), A.strides[0] // 8, A.strides[1] // 8


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dpn(a):
    """_dp, or the null pointer for None"""
    return _dp(a) if a is not None else C.POINTER(C.c_double)()


def _ipn(a):
    return _ip(a) if a is not None else C.POINTER(C.c_int32)()


def _n_cmd(lead_table, cmd, what):
    """The reference's rule (DMPC::solveParallelDMPCv2, dmpc/cpp/dmpc.cpp:1572-1573): N = _po.cols(), N_cmd = _pf.cols().
    lead_table: leading shape ([N] or [S,N]) of the table-sized array (l, po); cmd: a commanded-sized array (pf [..,3]).
    Returns (S, N, N_cmd, leading shape of the commanded-sized outputs).  As many goals as vehicles: every vehicle is commanded, whatever
    the goals' shape.  More commanded agents than vehicles, or another batch shape, is refused."""
    S, N = (1, lead_table[0]) if len(lead_table) == 1 else lead_table
    if cmd.size == S * N * 3:
        return int(S), int(N), int(N), tuple(lead_table)
    lead_cmd = cmd.shape[:-1]
    if len(lead_table) != len(lead_cmd) or tuple(lead_table[:-1]) != tuple(lead_cmd[:-1]) or cmd.shape[-1] != 3:
        raise DmpcError(f"{what}: pf {tuple(cmd.shape)} does not batch like the table {tuple(lead_table)}")
    n_cmd = lead_cmd[-1]
    if n_cmd < 1 or n_cmd > N:
        raise DmpcError(f"{what}: pf has {n_cmd} agents, the table {N}: the commanded agents are the FIRST N_cmd <= N vehicles")
    return int(S), int(N), int(n_cmd), tuple(lead_cmd)


def _path(path, lead_cmd, what):
    """path [S,M,P,3] (or [M,P,3] next to unbatched po / pf) of the scripted vehicles -> (contiguous array, M, P); lead_cmd: leading shape
    ([N_cmd] or [S,N_cmd]) of the commanded-sized arrays"""
    path = _f(path)
    if path.ndim != len(lead_cmd) + 2 or path.shape[-1] != 3 or tuple(path.shape[:-3]) != tuple(lead_cmd[:-1]):
        raise DmpcError(f"{what}: path {tuple(path.shape)} does not batch like the commanded agents {tuple(lead_cmd)}: [S,M,P,3] (or [M,P,3])")
    M, P = path.shape[-3], path.shape[-2]
    if M < 1 or P < 1:
        raise DmpcError(f"{what}: path {tuple(path.shape)} needs at least one vehicle and one sample")
    return path, int(M), int(P)


# ---- the flight methods (transition, mission, route, replan, transition_sharded) and the check methods (postcheck, clearance, setpoints) of
# Dmpc share the functions from here to _other_vehicles.  They are functions of the module, not methods: every refusal fires before anything
# touches the context (tests/bindingcalls.py records what the methods pass down)
def _disturbable(method):
    """disturb= of a flight method: the method runs inside _disturbed(disturb) and is itself called without it"""
    sig = inspect.signature(method)

    @functools.wraps(method)
    def wrapped(*args, **kw):
        call = sig.bind(*args, **kw)
        disturb = call.arguments.pop("disturb", None)
        if disturb is None:
            return method(*call.args, **call.kwargs)
        with call.arguments["self"]._disturbed(disturb):
            return method(*call.args, **call.kwargs)
    return wrapped


def _on_fail(what, on_fail):
    """on_fail= of a flight method -> whether failed agents hold"""
    if on_fail not in ("stop", "hold"):
        raise DmpcError(f"{what}: on_fail is 'stop' or 'hold', not {on_fail!r}")
    return on_fail == "hold"


def _assign_mode(what, assign):
    """assign= of transition() / mission() -> (whether to assign, whether by assign_rect())"""
    if isinstance(assign, str) or assign not in (True, False):
        if assign != "rect":
            raise DmpcError(f"{what}: assign is False, True or 'rect', not {assign!r}")
        return True, True
    return bool(assign), False


def _cmd_shape(what, po, cmd, axes, noun, last=True):
    """The shape rule of mission(), route() and replan(), first half: po is [N,3] or [S,N,3] and cmd -- the goals or waypoints, `noun` in the
    messages -- has the axes `axes` ("Q,N_cmd,3", "N_cmd,W,3" or "N_cmd,3") behind po's batch axis, the last of them before the 3 not empty
    (last=False: not asked here).  Returns N_cmd."""
    names = axes.split(",")
    if (po.ndim not in (2, 3) or cmd.ndim != po.ndim + len(names) - 2 or po.shape[-1] != 3 or cmd.shape[-1] != 3
            or cmd.shape[:-len(names)] != po.shape[:-2] or (last and cmd.shape[-2] < 1)):
        raise DmpcError(f"{what}: {noun} {tuple(cmd.shape)} must be [{axes}] next to po [N,3], or [S,{axes}] next to po [S,N,3]: po is {tuple(po.shape)}")
    return cmd.shape[names.index("N_cmd") - len(names)]


def _commanded(what, po, cmd, axes, noun, path, last=True):
    """The shape rule of mission(), route() and replan(): _cmd_shape, then N_cmd <= N = po's vehicles means static vehicles behind the commanded
    ones, and a path means M scripted ones behind N == N_cmd commanded ones.  Returns (S, N, N_cmd, lead: the leading shape of the per-agent
    outputs, path, M, P), M = P = 0 without a path."""
    n_cmd = _cmd_shape(what, po, cmd, axes, noun, last)
    S, N = (1 if po.ndim == 2 else po.shape[0]), po.shape[-2]
    lead = po.shape[:-2] + (n_cmd,)
    M = P = 0
    if path is not None:
        if N != n_cmd:
            raise DmpcError(f"{what}: with path, po {tuple(po.shape)} and {noun} {tuple(cmd.shape)} must cover the same commanded agents")
        path, M, P = _path(path, lead, what)
    elif n_cmd < 1 or n_cmd > N:
        raise DmpcError(f"{what}: {noun} have {n_cmd} agents, po {N}: the commanded agents are the FIRST N_cmd <= N vehicles")
    return S, N, n_cmd, lead, path, M, P


def _flight_outputs(S, lead, K_T_max, histories, hold=None):
    """The outputs every flight has, as (out, common, held, trio).  out: K_T_used, scene_status [S] and the histories pk, vk, ak
    [lead, K_T_max, 3] (histories=False: None, they stay on the device); common: the pointers to them in every entry's order, pk vk ak K_T_used
    scene_status.  hold=None: the entry has no hold record (held and trio are empty); otherwise it has one: held holds hold_count, hold_first
    [lead] and agent_status [lead, K_T_max] and trio points to them when hold is true, held is empty and trio null when it is false."""
    out = dict(pk=None, vk=None, ak=None, K_T_used=np.zeros(S, dtype=np.int32), scene_status=np.zeros(S, dtype=np.int32))
    if histories:
        out.update((k, np.zeros(lead + (K_T_max, 3))) for k in ("pk", "vk", "ak"))
    common = [_dpn(out[k]) for k in ("pk", "vk", "ak")] + [_ip(out["K_T_used"]), _ip(out["scene_status"])]
    held = {}
    if hold:
        held = dict(hold_count=np.zeros(lead, dtype=np.int32), hold_first=np.zeros(lead, dtype=np.int32),
                    agent_status=np.zeros(lead + (K_T_max,), dtype=np.int32))
    trio = [] if hold is None else [_ip(a) for a in held.values()] if hold else [_ipn(None)] * 3
    return out, common, held, trio


def _stage_head(shape, Q, po, goals, deadline, K_T_max, error_tol):
    """what dmpc_transition_mission and dmpc_transition_hold take between the context and the histories (the latter: and max_hold); shape: what
    _commanded returns"""
    S, N, n_cmd, _, path, M, P = shape
    return [S, N + M, n_cmd, Q, _dp(po), _dp(goals), _ipn(deadline), _dpn(path), P, int(K_T_max), float(error_tol)]


def _check_inputs(K_T_used, hist, KT_alloc, mask):
    """What postcheck(), clearance() and setpoints() check.  hist = (pk, vk, ak): given histories, or pk None for the ones the last transition
    left on the device, whose K_T_max KT_alloc then says.  Returns (K_T_used as int32, the histories as contiguous arrays, KT_alloc, run), run:
    the arguments every post-check entry has in a row -- KT_alloc, K_T_used, mask, pk, vk, ak."""
    used = np.ascontiguousarray(np.atleast_1d(K_T_used), dtype=np.int32)
    if hist[0] is not None:
        hist = [None if x is None else _f(x) for x in hist]
        KT_alloc = hist[0].shape[-2]
    else:
        hist = [None] * 3
    assert KT_alloc is not None
    msk = None if mask is None else np.ascontiguousarray(np.atleast_1d(mask), dtype=np.int32)
    return used, hist, KT_alloc, [int(KT_alloc), _ip(used), _ipn(msk)] + [_dpn(x) for x in hist]


def _other_vehicles(what, pf_shape, po_static, path):
    """The vehicles postcheck() and clearance() check the commanded agents of pf against: po_static [S,M,3] (or [M,3]), resting, or path
    [S,M,P,3], scripted, never both.  Returns (po_static, None where M = 0; path; M; P)."""
    if path is not None and po_static is not None:
        raise DmpcError(f"{what}: path and po_static exclude each other (scripted vehicles move, static ones rest)")
    lead = tuple(pf_shape[:-1])
    if path is not None:
        return (None,) + _path(path, lead, what)
    if po_static is None:
        return None, None, 0, 0
    pos = _f(po_static)
    if pos.shape[:-2] != lead[:-1] or pos.shape[-1] != 3:
        raise DmpcError(f"{what}: po_static {pos.shape} does not batch like pf {tuple(pf_shape)}")
    return (pos if pos.shape[-2] else None), None, pos.shape[-2], 0


def _disturbance(noise_p=0.0, noise_v=0.0, wind=None, pushes=None, seed=0):
    """The dmpc_disturbance descriptor of set_disturbance()'s arguments -> (descriptor, the arrays it points into).  wind [3] or [S,3]; pushes
    [n,9], rows of scene, agent, column, dp (3), dv (3).  Shapes are checked here, values by the library."""
    d, keep = DmpcDisturbance(), []
    d.seed, d.amp_p, d.amp_v = int(seed), float(noise_p), float(noise_v)
    if wind is not None:
        wind = _f(wind)
        if wind.ndim not in (1, 2) or wind.shape[-1] != 3:
            raise DmpcError(f"disturbance: wind {tuple(wind.shape)} must be [3] or [S,3]")
        d.wind, d.wind_scenes = _dp(wind), wind.size // 3
        keep.append(wind)
    if pushes is not None and np.size(pushes):
        pushes = _f(pushes)
        if pushes.ndim != 2 or pushes.shape[1] != 9:
            raise DmpcError(f"disturbance: pushes {tuple(pushes.shape)} must be [n,9]: scene, agent, column, dp (3), dv (3)")
        if not np.array_equal(pushes[:, :3], np.trunc(pushes[:, :3])) or np.abs(pushes[:, :3]).max() > 0x7fffffff:
            raise DmpcError("disturbance: scene, agent and column of a push must be integers")
        arr = (DmpcPush * len(pushes))()
        for q, row in zip(arr, pushes):
            q.scene, q.agent, q.column = int(row[0]), int(row[1]), int(row[2])
            q.dp[:], q.dv[:] = row[3:6], row[6:9]
        d.push, d.n_push = arr, len(pushes)
        keep.append(arr)
    return d, keep


def disturbance_sample(h, S, n_cmd, k, **kw):
    """dmpc_disturbance_sample (host, no context, no GPU): (dp, dv), [S,n_cmd,3] each, of column k by the rule include/dmpc_hip.h pins, for
    Dmpc.set_disturbance()'s arguments and the step h"""
    L = load()
    d, keep = _disturbance(**kw)
    dp, dv = np.zeros((int(S), int(n_cmd), 3)), np.zeros((int(S), int(n_cmd), 3))
    if L.dmpc_disturbance_sample(C.byref(d), float(h), int(S), int(n_cmd), int(k), _dp(dp), _dp(dv)):
        raise DmpcError(L.dmpc_last_error(None).decode())
    del keep
    return dp, dv


def _feedback(trigger_p, trigger_v, reanchor):
    """the dmpc_feedback descriptor of set_feedback()'s arguments; values are checked by the library"""
    return DmpcFeedback(float(trigger_p), float(trigger_v), int(reanchor))


def feedback_apply(trigger_p, trigger_v, reanchor, h, k, p_rows, v_rows, a_rows, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, lT_next, scene_done=None,
                   disturb=None):
    """dmpc_feedback_apply_host (host, no context, no GPU): one column of the feedback rule include/dmpc_hip.h pins.  p_rows, v_rows, a_rows
    [S,n_cmd,45] and status [S,n_cmd] of the step; x_p .. e_v [S,n_cmd,3]; lT_next [S,45,N]; scene_done [S] or None; disturb: a dict of
    Dmpc.set_disturbance()'s arguments or None.  Nothing is changed in place: returns dict(x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, v_rows, lT_next,
    event [S,n_cmd])."""
    L = load()
    p_rows, a_rows = _f(p_rows), _f(a_rows)
    o = {key: _f(a).copy() for key, a in dict(x_p=x_p, x_v=x_v, x_a=x_a, xh_p=xh_p, xh_v=xh_v, e_p=e_p, e_v=e_v, v_rows=v_rows, lT_next=lT_next).items()}
    status = np.ascontiguousarray(status, dtype=np.int32)
    if p_rows.ndim != 3 or p_rows.shape[2] != 3 * K_HOR or o["lT_next"].ndim != 3 or o["lT_next"].shape[:2] != (p_rows.shape[0], 3 * K_HOR):
        raise DmpcError(f"feedback_apply: p_rows {tuple(p_rows.shape)} must be [S,n_cmd,{3 * K_HOR}] and lT_next {tuple(o['lT_next'].shape)} [S,{3 * K_HOR},N]")
    S, n_cmd = p_rows.shape[:2]
    for key, a in dict(a_rows=a_rows, v_rows=o["v_rows"]).items():
        if a.shape != p_rows.shape:
            raise DmpcError(f"feedback_apply: {key} {tuple(a.shape)} is not shaped like p_rows {tuple(p_rows.shape)}")
    for key in ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v"):
        if o[key].shape != (S, n_cmd, 3):
            raise DmpcError(f"feedback_apply: {key} {tuple(o[key].shape)} must be [{S},{n_cmd},3]")
    if status.shape != (S, n_cmd):
        raise DmpcError(f"feedback_apply: status {tuple(status.shape)} must be [{S},{n_cmd}]")
    if scene_done is not None:
        scene_done = np.ascontiguousarray(scene_done, dtype=np.int32)
        if scene_done.shape != (S,):
            raise DmpcError(f"feedback_apply: scene_done {tuple(scene_done.shape)} must be [{S}]")
    fb = _feedback(trigger_p, trigger_v, reanchor)
    d, keep = _disturbance(**disturb) if disturb is not None else (None, None)
    o["event"] = np.zeros((S, n_cmd), dtype=np.int32)
    if L.dmpc_feedback_apply_host(C.byref(fb), C.byref(d) if d is not None else None, float(h), S, o["lT_next"].shape[2], n_cmd, int(k), _dp(p_rows),
                                  _dp(o["v_rows"]), _dp(a_rows), _ip(status), _dp(o["x_p"]), _dp(o["x_v"]), _dp(o["x_a"]), _dp(o["xh_p"]), _dp(o["xh_v"]),
                                  _dp(o["e_p"]), _dp(o["e_v"]), _dp(o["lT_next"]), _ip(o["event"]), _ipn(scene_done)):
        raise DmpcError(L.dmpc_last_error(None).decode())
    del keep
    return o


def _measurement(noise_p=0.0, noise_v=0.0, gain_p=1.0, gain_v=1.0, seed=0):
    """the dmpc_measurement descriptor of set_measurement()'s arguments; values are checked by the library"""
    return DmpcMeasurement(int(seed), float(noise_p), float(noise_v), float(gain_p), float(gain_v))


def measurement_sample(S, n_cmd, k, **kw):
    """dmpc_measurement_sample (host, no context, no GPU): (m_p, m_v), [S,n_cmd,3] each, the sensor noise of column k by the rule
    include/dmpc_hip.h pins, for Dmpc.set_measurement()'s arguments"""
    L = load()
    m = _measurement(**kw)
    mp, mv = np.zeros((int(S), int(n_cmd), 3)), np.zeros((int(S), int(n_cmd), 3))
    if L.dmpc_measurement_sample(C.byref(m), int(S), int(n_cmd), int(k), _dp(mp), _dp(mv)):
        raise DmpcError(L.dmpc_last_error(None).decode())
    return mp, mv


def estimate_apply(trigger_p, trigger_v, reanchor, h, k, p_rows, v_rows, a_rows, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v, lT_next,
                   scene_done=None, disturb=None, measure=None):
    """dmpc_estimate_apply_host (host, no context, no GPU): one column of the feedback rule behind a measurement, as include/dmpc_hip.h pins it.
    feedback_apply()'s arguments with the belief eh_p, eh_v [S,n_cmd,3] behind e_v; measure: a dict of Dmpc.set_measurement()'s arguments (None:
    no noise, gain 1).  Nothing is changed in place: returns dict(x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v, v_rows, lT_next, event
    [S,n_cmd])."""
    L = load()
    p_rows, a_rows = _f(p_rows), _f(a_rows)
    o = {key: _f(a).copy() for key, a in dict(x_p=x_p, x_v=x_v, x_a=x_a, xh_p=xh_p, xh_v=xh_v, e_p=e_p, e_v=e_v, eh_p=eh_p, eh_v=eh_v, v_rows=v_rows,
                                              lT_next=lT_next).items()}
    status = np.ascontiguousarray(status, dtype=np.int32)
    if p_rows.ndim != 3 or p_rows.shape[2] != 3 * K_HOR or o["lT_next"].ndim != 3 or o["lT_next"].shape[:2] != (p_rows.shape[0], 3 * K_HOR):
        raise DmpcError(f"estimate_apply: p_rows {tuple(p_rows.shape)} must be [S,n_cmd,{3 * K_HOR}] and lT_next {tuple(o['lT_next'].shape)} [S,{3 * K_HOR},N]")
    S, n_cmd = p_rows.shape[:2]
    for key, a in dict(a_rows=a_rows, v_rows=o["v_rows"]).items():
        if a.shape != p_rows.shape:
            raise DmpcError(f"estimate_apply: {key} {tuple(a.shape)} is not shaped like p_rows {tuple(p_rows.shape)}")
    for key in ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "eh_p", "eh_v"):
        if o[key].shape != (S, n_cmd, 3):
            raise DmpcError(f"estimate_apply: {key} {tuple(o[key].shape)} must be [{S},{n_cmd},3]")
    if status.shape != (S, n_cmd):
        raise DmpcError(f"estimate_apply: status {tuple(status.shape)} must be [{S},{n_cmd}]")
    if scene_done is not None:
        scene_done = np.ascontiguousarray(scene_done, dtype=np.int32)
        if scene_done.shape != (S,):
            raise DmpcError(f"estimate_apply: scene_done {tuple(scene_done.shape)} must be [{S}]")
    fb = _feedback(trigger_p, trigger_v, reanchor)
    m = _measurement(**(measure or {}))
    d, keep = _disturbance(**disturb) if disturb is not None else (None, None)
    o["event"] = np.zeros((S, n_cmd), dtype=np.int32)
    if L.dmpc_estimate_apply_host(C.byref(fb), C.byref(m), C.byref(d) if d is not None else None, float(h), S, o["lT_next"].shape[2], n_cmd, int(k),
                                  _dp(p_rows), _dp(o["v_rows"]), _dp(a_rows), _ip(status), _dp(o["x_p"]), _dp(o["x_v"]), _dp(o["x_a"]), _dp(o["xh_p"]),
                                  _dp(o["xh_v"]), _dp(o["e_p"]), _dp(o["e_v"]), _dp(o["eh_p"]), _dp(o["eh_v"]), _dp(o["lT_next"]), _ip(o["event"]),
                                  _ipn(scene_done)):
        raise DmpcError(L.dmpc_last_error(None).decode())
    del keep
    return o


def model_matrices(h, K=K_HOR):
    """(Lambda, A_v, A_initp, Delta) -- getPosMat.m / dmpc_soft_bound.m:92-108 / getDeltaMat.m (host, no GPU needed)."""
    L = load()
    prm = make_params(K=K, h=h)
    n = 3 * K
    Lam, Av, A0, Dl = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, 6)), np.zeros((n, n))
    if L.dmpc_model_matrices(C.byref(prm), _dp(Lam), _dp(Av), _dp(A0), _dp(Dl)) != 0:
        raise DmpcError(L.dmpc_last_error(None).decode())
    return Lam, Av, A0, Dl


def posvel_matrix(h, K):
    L = load()
    A = np.zeros((12, 3 * K))
    if L.dmpc_posvel_matrix(float(h), int(K), _dp(A)) != 0:
        raise DmpcError(L.dmpc_last_error(None).decode())
    return A


def partition(N, G, rank):
    """(lo, count, cmax) of rank's contiguous cluster (dmpc/cpp/dmpc.cpp:1600-1625; dmpc_partition of the C ABI: host arithmetic)"""
    lo, cnt, cmax = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if load().dmpc_partition(int(N), int(G), int(rank), C.byref(lo), C.byref(cnt), C.byref(cmax)):
        raise DmpcError(load().dmpc_last_error(None).decode())
    return lo.value, cnt.value, cmax.value


class Dmpc:
    """One solver context on one HIP device (wraps dmpc_create/dmpc_destroy)."""

    def __init__(self, variant="bound", device=0, precision="f64", **kw):
        """precision: "f64" (DMPC_PREC_F64), "mixed" (DMPC_PREC_MIXED: fp32 table / scan / rows, fp64 QP), "f32factor" (DMPC_PREC_F32FACTOR: the solver's
        inverse factor stored in fp32, refined against fp64 residuals) or "low" (both);
        device: a HIP device index, DEVICE_ALL (-100: every visible GPU from this process, agents sharded over them) or
        DEVICE_CURRENT (-1: the calling thread's current device)"""
        self._L = load()
        self.prm = make_params(variant, **kw)
        self.precision = precision
        self._ctx = self._L.dmpc_create(C.byref(self.prm), int(device), PRECISIONS[precision])
        if not self._ctx:
            raise DmpcError(self._L.dmpc_last_error(None).decode())
        self.device = device

    DEVICE_ALL, DEVICE_CURRENT = -100, -1

    @property
    def n_devices(self):
        """GPUs this context drives (1 unless created with DEVICE_ALL on a multi-GPU node)"""
        return int(self._L.dmpc_group_size(self._ctx))

    @staticmethod
    def emulate_devices(n):
        """tests: DEVICE_ALL contexts created from now on run n ranks that all sit on the current GPU (0: off)"""
        if load().dmpc_debug_emulate_devices(int(n)):
            raise DmpcError("emulate_devices: bad count")

    def debug_option(self, name, value):
        """development / tests: launch forms and tiers of this context (dmpc_debug_option: no_cull, no_persist, force_persist, tier1_qcap,
        crash_min, no_fast_exit, iter_cap, split_parts ...); never arithmetic"""
        self._chk(self._L.dmpc_debug_option(self._ctx, name.encode(), int(value)))
        return self

    def debug_watch_grid(self):
        """development / tests: list builds of this context keep a copy of their largest half extents from now on (the two-launch build's are set
        back to zero by the step's own scan kernel); any call of dmpc_debug_read_grid arms this, here one made before a build"""
        self._L.dmpc_debug_read_grid(self._ctx, _ip(np.zeros(12, dtype=np.int32)), None, 0)
        return self

    def debug_read_grid(self):
        """development / tests: what the last list build of a step left on the device (dmpc_debug_read_grid): the shape -- S, G, C, n (cells
        per axis), ncell, build (0: all-pairs box test, 1: five kernels, 2: two launches), cap, close_cap, agents, parts -- and bbox [G,S,18,C]
        fp32, maxhalf [S,3,3] fp32, start [S,3,ncell+1], ent [2,S,3,G*C,4] fp32 (word 0 of the first half: the code's bits), nbr_cnt
        [agents,parts], nbr_list [agents,cap], close_cnt [agents], close_list [agents,close_cap,2]; the grid's arrays are empty with build = 0;
        maxhalf after the two-launch build needs debug_watch_grid before the step (zeros otherwise)"""
        sh = np.zeros(12, dtype=np.int32)
        self._chk(self._L.dmpc_debug_read_grid(self._ctx, _ip(sh), None, 0))
        S, G, Cc, nx, ny, nz, ncell, build, cap, ccap, agents, parts = (int(x) for x in sh)
        g = 1 if build else 0
        shapes = dict(bbox=(G, S, 18, Cc), maxhalf=(g * S, 3, 3), start=(g * S, 3, ncell + 1), ent=(2, g * S, 3, G * Cc, 4), nbr_cnt=(agents, parts),
                      nbr_list=(agents, cap), close_cnt=(agents if ccap else 0,), close_list=(agents, ccap, 2))
        words = np.zeros(sum(int(np.prod(v)) for v in shapes.values()), dtype=np.int32)
        self._chk(self._L.dmpc_debug_read_grid(self._ctx, _ip(sh), words.ctypes.data_as(C.c_void_p), words.nbytes))
        out = dict(S=S, G=G, C=Cc, n=(nx, ny, nz), ncell=ncell, build=build, cap=cap, close_cap=ccap, agents=agents, parts=parts)
        at = 0
        for k, shp in shapes.items():
            n = int(np.prod(shp))
            a = words[at:at + n].reshape(shp)
            out[k] = a.view(np.float32) if k in ("bbox", "maxhalf", "ent") else a
            at += n
        return out

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.dmpc_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def _chk(self, rc):
        if rc != 0:
            raise DmpcError(self._L.dmpc_last_error(self._ctx).decode())

    def set_params(self, variant=None, **kw):
        """dmpc_set_params: re-tune this context.  Every parameter not named keeps its value (K, order, Qfar, Qnear, Sfree and tol included);
        a refused block leaves the context, and self.prm, as they were."""
        base = {f: getattr(self.prm, f) for f in ("K", "h", "rmin", "c", "alim", "Q1", "S1", "term", "max_tries", "order", "Qfar", "Qnear", "Sfree", "tol")}
        base["pmin"], base["pmax"] = tuple(self.prm.pmin), tuple(self.prm.pmax)
        base.update(kw)
        prm = make_params(self.prm.variant if variant is None else variant, **base)
        self._chk(self._L.dmpc_set_params(self._ctx, C.byref(prm)))
        self.prm = prm

    # ---- disturbed transitions -----------------------------------------------------------------
    def set_disturbance(self, noise_p=0.0, noise_v=0.0, wind=None, pushes=None, seed=0):
        """dmpc_set_disturbance: from now on transition(), mission(), route() and replan() add wind, noise and pushes to the state of every
        commanded agent between the state advance and the history record of every column k >= 1 (the rule include/dmpc_hip.h pins).  noise_p
        (metres), noise_v (m/s): half-widths of the uniform noise drawn from stream `seed`; wind [3] (every scene) or [S,3]: a constant
        acceleration (m/s^2); pushes [n,9]: rows of scene, agent, column, dp (3), dv (3).  Everything zero / None clears."""
        d, keep = _disturbance(noise_p, noise_v, wind, pushes, seed)
        self._chk(self._L.dmpc_set_disturbance(self._ctx, C.byref(d)))
        del keep   # (the library has copied everything)
        return self

    def clear_disturbance(self):
        self._chk(self._L.dmpc_set_disturbance(self._ctx, None))
        return self

    def disturbance_sample(self, S, n_cmd, k, **kw):
        """disturbance_sample() of this module with the context's h"""
        return disturbance_sample(float(self.prm.h), S, n_cmd, k, **kw)

    @contextlib.contextmanager
    def _disturbed(self, disturb):
        """disturb= of the transition methods: set before the call, cleared after it, also on an error"""
        if not isinstance(disturb, dict):
            raise DmpcError(f"disturb is None or a dict of set_disturbance()'s arguments, not {disturb!r}")
        self.set_disturbance(**disturb)
        try:
            yield
        finally:
            self.clear_disturbance()

    # ---- event-triggered feedback --------------------------------------------------------------
    def set_feedback(self, trigger_p, trigger_v, reanchor=True):
        """dmpc_set_feedback: from now on transition(), mission(), route() and replan() keep a planning state apart from the true state of every
        commanded agent (the rule include/dmpc_hip.h pins): the solver starts from its own prediction, and from the true state again only on
        an EVENT -- the tracking error |g_p| > trigger_p (metres) or |g_v| > trigger_v (m/s).  (0, 0): feed back on every column (the disturbed
        loop as it was); inf: never.  reanchor: on an event, shift the agent's announced plan onto the true state.  The setting is persistent,
        like set_disturbance(); without a disturbance it is inert."""
        fb = _feedback(trigger_p, trigger_v, reanchor)
        self._chk(self._L.dmpc_set_feedback(self._ctx, C.byref(fb)))
        return self

    def clear_feedback(self):
        self._chk(self._L.dmpc_set_feedback(self._ctx, None))
        return self

    def feedback_log(self, S, n_cmd):
        """dmpc_feedback_log: the report on this context's last flight with a policy -- dict(event_count, event_first, event_last [S,n_cmd]
        (local columns, -1: none), dev_p_max, dev_v_max [S,n_cmd] (the largest tracking error seen, events included), dev_p_col, dev_v_col,
        xh_p, xh_v, e_p, e_v [S,n_cmd,3]: the planning state and the error at the scene's last column)"""
        S, n_cmd = int(S), int(n_cmd)
        if S < 1 or n_cmd < 1:
            raise DmpcError("feedback_log: S and n_cmd must be >= 1")
        o = {k: np.zeros((S, n_cmd), dtype=np.int32) for k in ("event_count", "event_first", "event_last", "dev_p_col", "dev_v_col")}
        o.update({k: np.zeros((S, n_cmd)) for k in ("dev_p_max", "dev_v_max")})
        o.update({k: np.zeros((S, n_cmd, 3)) for k in ("xh_p", "xh_v", "e_p", "e_v")})
        self._chk(self._L.dmpc_feedback_log(self._ctx, S, n_cmd, _ip(o["event_count"]), _ip(o["event_first"]), _ip(o["event_last"]), _dp(o["dev_p_max"]),
                                            _ip(o["dev_p_col"]), _dp(o["dev_v_max"]), _ip(o["dev_v_col"]), _dp(o["xh_p"]), _dp(o["xh_v"]), _dp(o["e_p"]),
                                            _dp(o["e_v"])))
        return o

    # ---- measured state --------------------------------------------------------------------------
    def set_measurement(self, noise_p=0.0, noise_v=0.0, gain_p=1.0, gain_v=1.0, seed=0):
        """dmpc_set_measurement: from now on the feedback rule of a flight decides on an ESTIMATE of the tracking error -- the true deviation plus
        uniform sensor noise of half-widths noise_p (m), noise_v (m/s), blended into the planner's belief with the fixed gains gain_p, gain_v in
        (0, 1] (1: the estimate is the measurement) -- and re-initialises the planner to it (the rule include/dmpc_hip.h pins).  It never moves the
        vehicle.  Persistent, like set_disturbance() and set_feedback(); a flight with a measurement and no feedback policy is refused."""
        m = _measurement(noise_p, noise_v, gain_p, gain_v, seed)
        self._chk(self._L.dmpc_set_measurement(self._ctx, C.byref(m)))
        return self

    def clear_measurement(self):
        self._chk(self._L.dmpc_set_measurement(self._ctx, None))
        return self

    def estimate_log(self, S, n_cmd):
        """dmpc_estimate_log: the report on this context's last flight with a measurement -- dict(err_p_max, err_v_max [S,n_cmd]: the largest
        estimation error |g - gh|; dev_p_max, dev_v_max: the largest TRUE tracking error |g|; err_p_col, err_v_col, dev_p_col, dev_v_col their
        local columns; eh_p, eh_v [S,n_cmd,3]: the belief at the scene's last column)"""
        S, n_cmd = int(S), int(n_cmd)
        if S < 1 or n_cmd < 1:
            raise DmpcError("estimate_log: S and n_cmd must be >= 1")
        o = {k: np.zeros((S, n_cmd), dtype=np.int32) for k in ("err_p_col", "err_v_col", "dev_p_col", "dev_v_col")}
        o.update({k: np.zeros((S, n_cmd)) for k in ("err_p_max", "err_v_max", "dev_p_max", "dev_v_max")})
        o.update({k: np.zeros((S, n_cmd, 3)) for k in ("eh_p", "eh_v")})
        self._chk(self._L.dmpc_estimate_log(self._ctx, S, n_cmd, _dp(o["err_p_max"]), _ip(o["err_p_col"]), _dp(o["err_v_max"]), _ip(o["err_v_col"]),
                                            _dp(o["dev_p_max"]), _ip(o["dev_p_col"]), _dp(o["dev_v_max"]), _ip(o["dev_v_col"]), _dp(o["eh_p"]), _dp(o["eh_v"])))
        return o

    # ---- start in motion ------------------------------------------------------------------------
    def set_start(self, vo=None, ao=None, plan=None, col0=0, from_end=False, src_scene=None, S=None, N_cmd=None):
        """dmpc_set_start: THE START IS CONSUMED BY ONE FLIGHT -- the next transition(), mission(), route() or replan() that passes its own
        checks starts from it instead of from rest, and clears it.  Host form: vo, ao [S,N_cmd,3] (or [N_cmd,3]; None: zeros) next to the
        flight's po; plan: None (the braking plan, made on the device), plan_p [S,N_cmd,45], or (plan_p, plan_v, plan_a).  from_end=True: the
        end of this context's last flight, gathered on the device now; src_scene [S]: scene s starts where scene src_scene[s] ended (None:
        identity).  COLUMN 0 IS THE CALLER'S COLUMN col0 (scripted windows, the disturbance's counter and pushes; from_end: added to the end's
        col).  S, N_cmd: the flight's shape; taken from the arrays (from_end: from src_scene / the last flight_end) where they are not given."""
        what = "set_start"
        arrs = dict(vo=vo, ao=ao)
        if plan is not None and not isinstance(plan, (tuple, list)):
            plan = (plan,)
        if plan is not None:
            if len(plan) not in (1, 3):
                raise DmpcError(f"{what}: plan is plan_p or (plan_p, plan_v, plan_a)")
            arrs.update(zip(("plan_p", "plan_v", "plan_a"), plan))
        arrs = {k: _f(a) for k, a in arrs.items() if a is not None}
        if from_end and arrs:
            raise DmpcError(f"{what}: from_end takes no host arrays ({', '.join(arrs)})")
        if src_scene is not None:
            if not from_end:
                raise DmpcError(f"{what}: src_scene needs from_end=True")
            src_scene = np.ascontiguousarray(src_scene, dtype=np.int32).reshape(-1)
            S = src_scene.size if S is None else S
        for k, a in arrs.items():
            w = 3 if k in ("vo", "ao") else 3 * K_HOR
            if a.ndim not in (2, 3) or a.shape[-1] != w:
                raise DmpcError(f"{what}: {k} {tuple(a.shape)} must be [S,N_cmd,{w}] or [N_cmd,{w}]")
            s_, n_ = (1, a.shape[0]) if a.ndim == 2 else a.shape[:2]
            S, N_cmd = (s_ if S is None else S), (n_ if N_cmd is None else N_cmd)
            if (s_, n_) != (S, N_cmd):
                raise DmpcError(f"{what}: {k} {tuple(a.shape)} is not for S = {S}, N_cmd = {N_cmd}")
        if S is None or N_cmd is None:
            raise DmpcError(f"{what}: S and N_cmd are needed (no array gives them)")
        d = DmpcStart(int(S), int(N_cmd), int(bool(from_end)), _ipn(src_scene), _dpn(arrs.get("vo")), _dpn(arrs.get("ao")), _dpn(arrs.get("plan_p")),
                      _dpn(arrs.get("plan_v")), _dpn(arrs.get("plan_a")), int(col0))
        self._chk(self._L.dmpc_set_start(self._ctx, C.byref(d)))
        del arrs   # (the library has copied everything)
        return self

    def clear_start(self):
        self._chk(self._L.dmpc_set_start(self._ctx, None))
        return self

    @contextlib.contextmanager
    def starting(self, **kw):
        """set_start(**kw) on entry; cleared on exit if no flight consumed it (also on an error)"""
        self.set_start(**kw)
        try:
            yield self
        finally:
            self.clear_start()

    def flight_end(self, S, N_cmd):
        """dmpc_flight_end: where the S scenes of this context's last flight ended -- dict(x_p, x_v, x_a [S,N_cmd,3], plan_p, plan_v, plan_a
        [S,N_cmd,45]: every agent's plan of the step that produced its scene's last column, col [S]: that column in the caller's count).
        Valid until the next step or flight on the context; refused if a scene did not end SOLVED."""
        S, N_cmd = int(S), int(N_cmd)
        if S < 1 or N_cmd < 1:
            raise DmpcError("flight_end: S and N_cmd must be >= 1")
        o = {k: np.zeros((S, N_cmd, 3)) for k in ("x_p", "x_v", "x_a")}
        o.update({k: np.zeros((S, N_cmd, 3 * K_HOR)) for k in ("plan_p", "plan_v", "plan_a")})
        o["col"] = np.zeros(S, dtype=np.int32)
        self._chk(self._L.dmpc_flight_end(self._ctx, S, N_cmd, _dp(o["x_p"]), _dp(o["x_v"]), _dp(o["x_a"]), _dp(o["plan_p"]), _dp(o["plan_v"]),
                                          _dp(o["plan_a"]), _ip(o["col"])))
        return o

    def start_plan(self, x_p, x_v, x_a):
        """dmpc_start_plan: the braking plan of states [..,3] on the host (no GPU) -> (plan_p, plan_v, plan_a) [..,45]"""
        x_p, x_v, x_a = _f(x_p), _f(x_v), _f(x_a)
        if x_p.shape != x_v.shape or x_p.shape != x_a.shape or x_p.ndim < 1 or x_p.shape[-1] != 3 or x_p.size < 3:
            raise DmpcError(f"start_plan: x_p, x_v, x_a must share a shape [..,3]: {tuple(x_p.shape)}, {tuple(x_v.shape)}, {tuple(x_a.shape)}")
        out = [np.zeros(x_p.shape[:-1] + (3 * K_HOR,)) for _ in range(3)]
        if self._L.dmpc_start_plan(C.byref(self.prm), x_p.size // 3, _dp(x_p), _dp(x_v), _dp(x_a), _dp(out[0]), _dp(out[1]), _dp(out[2])):
            raise DmpcError(self._L.dmpc_last_error(None).decode())
        return tuple(out)

    # ---- host-array entry points -------------------------------------------------------------
    def init_batch(self, po, pf):
        po, pf = _f(po), _f(pf)
        shp = po.shape[:-1]
        S, N = (1, shp[0]) if len(shp) == 1 else shp
        l = np.zeros(shp + (45,))
        v = np.zeros_like(l)
        a = np.zeros_like(l)
        self._chk(self._L.dmpc_init_batch(self._ctx, S, N, _dp(po), _dp(pf), _dp(l), _dp(v), _dp(a)))
        return l, v, a

    def step_batch(self, l, x_p, x_v, x_a, pf):
        """l: [N,45] or [S,N,45]; states/goals [..,3]. Returns dict(p,v,a,status,info).
        States and goals with FEWER agents than the table (N_cmd < N, dmpc_step_batch_cmd): the first N_cmd vehicles are commanded, the
        rows behind them are uncommanded vehicles the caller keeps constant; the outputs cover the commanded agents."""
        l, x_p, x_v, x_a, pf = _f(l), _f(x_p), _f(x_v), _f(x_a), _f(pf)
        lead = l.shape[:-1]
        S, N, n_cmd, lead_c = _n_cmd(lead, pf, "step_batch")
        if n_cmd < N and not (x_p.shape == x_v.shape == x_a.shape == pf.shape):
            raise DmpcError("step_batch: x_p, x_v, x_a and pf must cover the same commanded agents")
        p, v, a = np.zeros(lead_c + (45,)), np.zeros(lead_c + (45,)), np.zeros(lead_c + (45,))
        status = np.zeros(lead_c, dtype=np.int32)
        info = np.zeros(lead_c + (INFO_LEN,), dtype=np.int32)
        if n_cmd == N:
            self._chk(self._L.dmpc_step_batch(self._ctx, S, N, _dp(l), _dp(x_p), _dp(x_v), _dp(x_a), _dp(pf), _dp(p), _dp(v),
                                              _dp(a), _ip(status), _ip(info)))
        else:
            self._chk(self._L.dmpc_step_batch_cmd(self._ctx, S, N, n_cmd, _dp(l), _dp(x_p), _dp(x_v), _dp(x_a), _dp(pf), _dp(p), _dp(v),
                                                  _dp(a), _ip(status), _ip(info)))
        return dict(p=p, v=v, a=a, status=status, info=info)

    def solve_one(self, l, n, po, vo, ao, pf):
        l, po, vo, ao, pf = _f(l), _f(po), _f(vo), _f(ao), _f(pf)
        p, v, a = np.zeros(45), np.zeros(45), np.zeros(45)
        status = np.zeros(1, dtype=np.int32)
        info = np.zeros(INFO_LEN, dtype=np.int32)
        self._chk(self._L.dmpc_solve_one(self._ctx, l.shape[0], int(n), _dp(l), _dp(po), _dp(vo), _dp(ao), _dp(pf), _dp(p),
                                         _dp(v), _dp(a), _ip(status), _ip(info)))
        return dict(p=p, v=v, a=a, status=int(status[0]), info=info)

    def rows_one(self, l, n, po, vo, max_rows=4096):
        """a5/a6 standalone: structured collision rows of agent n (reference order, unpruned)."""
        l, po, vo = _f(l), _f(po), _f(vo)
        xi, rhs, sc = np.zeros((max_rows, 3)), np.zeros(max_rows), np.zeros(max_rows)
        kc = np.zeros(max_rows, dtype=np.int32)
        nr, vk, st = (np.zeros(1, dtype=np.int32) for _ in range(3))
        self._chk(self._L.dmpc_rows_one(self._ctx, l.shape[0], int(n), _dp(l), _dp(po), _dp(vo), max_rows, _dp(xi), _dp(rhs),
                                        _dp(sc), _ip(kc), _ip(nr), _ip(vk), _ip(st)))
        k = min(int(nr[0]), max_rows)
        return dict(xi=xi[:k], rhs=rhs[:k], slack_coef=sc[:k], kc=kc[:k], nrows=int(nr[0]), viol_k=int(vk[0]), status=int(st[0]))

    def assign(self, po, goals, eps=None, max_rounds=0):
        """dmpc_assign_goals: which agent takes which goal.  po, goals [S,N,3] (or [N,3]); the permutation that minimises the sum of
        |E1 (po_i - goals_perm[i])|^2, E1 = diag(1,1,1/c) of the context's parameters, by the forward auction include/dmpc_hip.h pins, to within
        N eps of the optimum.  eps=None means 1e-4 / N, so that the total is within 1e-4 m^2 of optimal: an interface choice, not a measurement.
        max_rounds <= 0: 1 << 20.  Returns dict(perm [S,N] int32 (the goal of agent i), pf [S,N,3] = goals[perm], price [S,N] (per goal),
        cost [S], rounds [S]); a scene that met the round cap has rounds = -1, perm = -1, cost = NaN and pf zero."""
        po, goals = _f(po), _f(goals)
        if po.ndim not in (2, 3) or po.shape != goals.shape or po.shape[-1] != 3:
            raise DmpcError(f"assign: po {tuple(po.shape)} and goals {tuple(goals.shape)} must both be [S,N,3] (or [N,3])")
        lead = po.shape[:-1]
        S, N = (1, lead[0]) if len(lead) == 1 else lead
        eps = 1e-4 / max(N, 1) if eps is None else float(eps)
        perm, pf, price = np.zeros(lead, dtype=np.int32), np.zeros(lead + (3,)), np.zeros(lead)
        cost, rounds = np.zeros(lead[:-1]), np.zeros(lead[:-1], dtype=np.int32)
        self._chk(self._L.dmpc_assign_goals(self._ctx, int(S), int(N), _dp(po), _dp(goals), eps, int(max_rounds), _ip(perm), _dp(pf), _dp(price),
                                            _dp(cost), _ip(rounds)))
        return dict(perm=perm, pf=pf, price=price, cost=cost, rounds=rounds)

    def assign_rect(self, po, goals, eps=None, max_rounds=0):
        """dmpc_assign_rect: which agent takes which goal when the counts differ.  po [S,N,3] (or [N,3]), goals [S,M,3] (or [M,3]); of all ways
        to match min(N, M) agent-goal pairs the one that minimises the sum of |E1 (po_i - goals_perm[i])|^2 over the pairs, by the forward/reverse
        auction include/dmpc_hip.h pins, to within min(N, M) eps of the optimum.  eps=None means 1e-4 / max(N, M): an interface choice, as
        assign()'s.  max_rounds <= 0: 1 << 20.  max(N, M) <= 1024.  Returns dict(perm [S,N] int32 (the goal of agent i or -1), owner [S,M] int32
        (the agent of goal j or -1), pf [S,N,3] = goals[perm], or po where perm = -1, price [S,max(N,M)] (per goal when N <= M, per agent
        otherwise), cost [S], rounds [S]); a scene that met the round cap has rounds = -1, perm = -1, owner = -1, cost = NaN and pf zero."""
        po, goals = _f(po), _f(goals)
        if po.ndim not in (2, 3) or goals.ndim != po.ndim or po.shape[-1] != 3 or goals.shape[-1] != 3 or po.shape[:-2] != goals.shape[:-2]:
            raise DmpcError(f"assign_rect: po {tuple(po.shape)} must be [S,N,3] and goals {tuple(goals.shape)} [S,M,3] (or [N,3] and [M,3])")
        lead = po.shape[:-2]
        S, N, M = (lead[0] if lead else 1), po.shape[-2], goals.shape[-2]
        eps = 1e-4 / max(N, M, 1) if eps is None else float(eps)
        perm, owner = np.zeros(lead + (N,), dtype=np.int32), np.zeros(lead + (M,), dtype=np.int32)
        pf, price = np.zeros(lead + (N, 3)), np.zeros(lead + (max(N, M),))
        cost, rounds = np.zeros(lead), np.zeros(lead, dtype=np.int32)
        self._chk(self._L.dmpc_assign_rect(self._ctx, int(S), int(N), int(M), _dp(po), _dp(goals), eps, int(max_rounds), _ip(perm), _ip(owner),
                                           _dp(pf), _dp(price), _dp(cost), _ip(rounds)))
        return dict(perm=perm, owner=owner, pf=pf, price=price, cost=cost, rounds=rounds)

    def _assigned(self, what, start, stages, rect):
        """The assignment pre-pass of transition() / mission(): assign() -- rect: assign_rect() -- of the agents at start [..,n,3] to each goal set
        of `stages` in turn, the assigned goals of one stage being the starts of the next.  Returns (the goals to fly per stage, {perm: per stage,
        and owner: per stage when rect}); a scene that met the round cap has no labelling to fly."""
        flown, labels = [], {k: [] for k in (("perm", "owner") if rect else ("perm",))}
        for goals in stages:
            a = self.assign_rect(start, goals) if rect else self.assign(start, goals)
            if (np.asarray(a["rounds"]) < 0).any():
                raise DmpcError(f"{what}: the goal assignment met its round cap")
            start = a["pf"]
            flown.append(start)
            for k in labels:
                labels[k].append(a[k])
        return flown, labels

    def _fly(self, entry, head, outputs, tail=(), extra=()):
        """The one flight call: entry(context, *head, pk, vk, ak, K_T_used, scene_status, *tail, and the hold record where the entry has one), on
        outputs = _flight_outputs(...); head and tail: the entry's own arguments before and behind those.  Returns the result dict: the common
        outputs, then extra (the method's own keys), then the hold record."""
        out, common, held, trio = outputs
        self._chk(entry(self._ctx, *head, *common, *tail, *trio))
        return {**out, **dict(extra), **held}

    @_disturbable
    def transition(self, po, pf, K_T_max, error_tol=0.01, histories=True, path=None, on_fail="stop", max_hold=14, assign=False, disturb=None):
        """disturb: a dict of set_disturbance()'s arguments, in force for this call alone (with assign too); None: the context's standing setting.
        histories=False: pk/vk/ak are not downloaded (they stay on the device for postcheck()).
        assign=True: the goals are a formation, not a labelling: the commanded agents are assigned to them first (assign(), default eps), agent i
        flies to pf[perm[i]], and the dict also has perm.
        assign="rect": ALL N agents of po are commanded and pf holds any M >= 1 points [S,M,3]: assign_rect() (default eps) chooses who flies
        where, an agent without a goal gets pf = po (it stays, and still dodges); the result is transition(po, pf_assigned, ...) plus perm and owner.
        on_fail="hold" (dmpc_transition_hold; "stop": the entries below, unchanged): an agent whose solve failed flies its previous plan, shifted
        by one entry and with a braking tail, for up to max_hold consecutive columns while the scene goes on; the dict then also has hold_count,
        hold_first (per agent) and agent_status (per agent and column: the raw status, ST_HELD where held), and scene_status carries ST_HELD.
        pf with FEWER agents than po (N_cmd = pf's agents < N = po's, the reference's _pf.cols() / _po.cols(); dmpc_transition_cmd): the vehicles
        behind the first N_cmd are not commanded and stay at po as static obstacles; histories, K_T_used and scene_status cover the commanded ones.
        path [S,M,P,3] (or [M,P,3]; dmpc_transition_scripted): M scripted vehicles behind the commanded agents of po / pf (same agent count in
        both), sample t of a path = the vehicle's position at history column t, held at its last sample once the path has ended."""
        po, pf = _f(po), _f(pf)
        assign, rect = _assign_mode("transition", assign)
        if assign:
            if rect:
                if pf.ndim != po.ndim or pf.ndim not in (2, 3) or pf.shape[-1] != 3 or po.shape[-1] != 3 or pf.shape[:-2] != po.shape[:-2]:
                    raise DmpcError(f"transition: with assign='rect', po {tuple(po.shape)} must be [S,N,3] and the goals {tuple(pf.shape)} [S,M,3]")
                start = po
            else:
                if pf.size == po.size:
                    pf = pf.reshape(po.shape)
                if pf.ndim != po.ndim or pf.ndim not in (2, 3) or pf.shape[-1] != 3 or pf.shape[-2] > po.shape[-2]:
                    raise DmpcError(f"transition: with assign, pf {tuple(pf.shape)} must cover the first agents of po {tuple(po.shape)}")
                start = po[..., :pf.shape[-2], :]
            flown, labels = self._assigned("transition", start, [pf], rect)
            out = self.transition(po, flown[0], K_T_max, error_tol, histories, path, on_fail, max_hold)
            out.update((k, v[0]) for k, v in labels.items())
            return out
        hold = _on_fail("transition", on_fail)
        if path is not None:
            if po.shape != pf.shape or po.ndim not in (2, 3) or po.shape[-1] != 3:
                raise DmpcError(f"transition: with path, po {tuple(po.shape)} and pf {tuple(pf.shape)} must cover the same commanded agents")
            lead = po.shape[:-1]
            path, M, P = _path(path, lead, "transition")
            S, n_cmd = (1, lead[0]) if len(lead) == 1 else lead
            N = n_cmd
        else:
            S, N, n_cmd, lead = _n_cmd(po.shape[:-1], pf, "transition")
            M = P = 0
        outputs = _flight_outputs(S, lead, K_T_max, histories, True if hold else None)
        if hold:   # (pf [S][N_cmd][3] is goals [S][1][N_cmd][3]; stage_col is mission()'s to return)
            head = _stage_head((S, N, n_cmd, lead, path, M, P), 1, po, pf, None, K_T_max, error_tol)
            return self._fly(self._L.dmpc_transition_hold, head + [int(max_hold)], outputs, [_ip(np.zeros((S, 1), dtype=np.int32))])
        if path is not None:
            entry, head = self._L.dmpc_transition_scripted, [S, n_cmd, M, P, _dp(po), _dp(pf), _dp(path)]
        elif n_cmd < N:
            entry, head = self._L.dmpc_transition_cmd, [S, N, n_cmd, _dp(po), _dp(pf)]
        else:
            entry, head = self._L.dmpc_transition, [S, N, _dp(po), _dp(pf)]
        return self._fly(entry, head + [int(K_T_max), float(error_tol)], outputs)

    @_disturbable
    def mission(self, po, goals, K_T_max, error_tol=0.01, histories=True, deadline=None, path=None, on_fail="stop", max_hold=14, assign=False,
                disturb=None):
        """disturb: as transition().
        dmpc_transition_mission: one transition through the Q goal sets goals [Q,N_cmd,3] (next to an unbatched po) or [S,Q,N_cmd,3].  A stage
        ends at the first column where its goals are reached or -- deadline [Q] / [S,Q], 0 = none, the last 0 -- its deadline has passed; the
        next step is solved with the next goal set, the last stage ends the trial.  po with MORE vehicles than the goals: static vehicles, as
        transition(); path [S,M,P,3]: scripted vehicles, po then covers the commanded agents.  Returns what transition() returns, and stage_col
        [S,Q]: the column each stage ended on (-1: it never did).  on_fail, max_hold: as transition() (a held plan counts as a solved one in the
        stage rule).  assign=True: every goal set is a formation: the commanded agents are assigned to goals[0] from po, then stage by stage -- the
        assigned goals of stage q are the starts of stage q+1 -- and the dict also has perm [S,Q,N_cmd].  assign="rect": goals [S,Q,M,3] with any
        M >= 1, all N agents of po commanded; assign_rect() stage by stage from the previous stage's assigned targets (po for stage 0), an agent
        without a goal in a stage keeps its previous target; the dict also has perm [S,Q,N] and owner [S,Q,M]."""
        po, goals = _f(po), _f(goals)
        hold = _on_fail("mission", on_fail)
        _cmd_shape("mission", po, goals, "Q,N_cmd,3", "goals", last=False)   # (last: a mission without agents is refused by their count, below)
        assign, rect = _assign_mode("mission", assign)
        if assign:
            if rect and goals.shape[-2] < 1:
                raise DmpcError(f"mission: with assign='rect', goals {tuple(goals.shape)} must hold at least one point per stage")
            if not rect and not 1 <= goals.shape[-2] <= po.shape[-2]:
                raise DmpcError(f"mission: goals have {goals.shape[-2]} agents, po {po.shape[-2]}: the commanded agents are the FIRST N_cmd <= N vehicles")
            start = po if rect else po[..., :goals.shape[-2], :]
            flown, labels = self._assigned("mission", start, [goals[..., q, :, :] for q in range(goals.shape[-3])], rect)
            out = self.mission(po, np.stack(flown, axis=-3), K_T_max, error_tol, histories, deadline, path, on_fail, max_hold)
            out.update((k, np.stack(v, axis=-2)) for k, v in labels.items())
            return out
        shape = S, _, _, lead, _, _, _ = _commanded("mission", po, goals, "Q,N_cmd,3", "goals", path, last=False)
        Q = goals.shape[-3]
        if deadline is not None:
            deadline = np.ascontiguousarray(np.broadcast_to(np.asarray(deadline, dtype=np.int32), (S, Q)))
        stage_col = np.zeros((S, Q), dtype=np.int32)
        head = _stage_head(shape, Q, po, goals, deadline, K_T_max, error_tol)
        entry = self._L.dmpc_transition_hold if hold else self._L.dmpc_transition_mission
        return self._fly(entry, head + [int(max_hold)] * hold, _flight_outputs(S, lead, K_T_max, histories, hold or None), [_ip(stage_col)],
                         dict(stage_col=stage_col))

    @_disturbable
    def route(self, po, waypoints, K_T_max, capture, n_wp=None, timeout=0, error_tol=0.01, histories=True, path=None, on_fail="stop", max_hold=14,
              disturb=None):
        """disturb: as transition().
        dmpc_transition_route: one transition in which every commanded agent flies through waypoints of its own, waypoints [N_cmd,W,3] (next
        to an unbatched po) or [S,N_cmd,W,3]; n_wp [N_cmd] / [S,N_cmd] (1 .. W; None: every agent has W) counts an agent's waypoints, the last
        of them is its goal.  An agent leaves a waypoint that is not its last at the first column where it is closer to it than capture (metres)
        or -- timeout > 0, in columns -- has flown towards it for timeout columns; the next step is solved with its next waypoint.  The trial ends
        when every agent is on its last waypoint and they are all reached.  po with MORE vehicles than the waypoints: static vehicles, as
        transition(); path [S,M,P,3]: scripted vehicles, po then covers the commanded agents.  Returns what transition() returns, and wp_col
        [S,N_cmd,W]: the column on which the agent left each waypoint (-1: it never did), wp_index [S,N_cmd]: the waypoint it was flying to when
        the scene ended.  on_fail, max_hold: as transition() (a held plan counts as a solved one in the waypoint rule)."""
        po, waypoints = _f(po), _f(waypoints)
        hold = _on_fail("route", on_fail)
        S, N, n_cmd, lead, path, M, P = _commanded("route", po, waypoints, "N_cmd,W,3", "waypoints", path)
        W = waypoints.shape[-2]
        if n_wp is not None:
            n_wp = np.asarray(n_wp)
            if n_wp.shape != lead or not np.issubdtype(n_wp.dtype, np.integer) or n_wp.min() < 1 or n_wp.max() > W:
                raise DmpcError(f"route: n_wp must be integers in 1 .. W = {W} of shape {lead}")
            n_wp = np.ascontiguousarray(n_wp, dtype=np.int32)
        if not float(capture) > 0.0:
            raise DmpcError(f"route: capture must be > 0 (metres), not {capture!r}")
        if int(timeout) < 0:
            raise DmpcError(f"route: timeout must be >= 0 (columns; 0: none), not {timeout!r}")
        extra = dict(wp_col=np.zeros(lead + (W,), dtype=np.int32), wp_index=np.zeros(lead, dtype=np.int32))
        head = [S, N + M, n_cmd, W, _dp(po), _dp(waypoints), _ipn(n_wp), float(capture), int(timeout), _dpn(path), P, int(K_T_max), float(error_tol),
                int(max_hold) if hold else 0]
        return self._fly(self._L.dmpc_transition_route, head, _flight_outputs(S, lead, K_T_max, histories, hold), map(_ip, extra.values()), extra)

    def plan(self, po, goals, cell, margin=0.0, W=4, obstacles=None):
        """dmpc_plan_routes: which way round the static vehicles every commanded agent goes.  goals [S,N_cmd,3] (or [N_cmd,3]); po [S,N,3] with
        N >= N_cmd rows as in transition(): the rows behind the goals are the obstacles; obstacles [S,M,3] (or [M,3]): further obstacle points
        (a snapshot of scripted vehicles, say), behind po's.  A wavefront over a grid of `cell` metres on the context's workspace, a cell blocked
        when its centre is within rmin + margin of an obstacle in the collision metric, the cell path pruned by line of sight to at most W
        waypoints -- the rule include/dmpc_hip.h pins.  Returns dict(waypoints [S,N_cmd,W,3], n_wp [S,N_cmd], plan_status [S,N_cmd] (PLAN_OK,
        PLAN_TRUNCATED: more corners than W, the goal took the last slot, PLAN_UNREACHABLE: no way, the goal alone), hops [S,N_cmd] (cells of
        the path, -1: no way)); waypoints and n_wp go into route() as they are."""
        po, goals = _f(po), _f(goals)
        if (po.ndim not in (2, 3) or goals.ndim != po.ndim or po.shape[-1] != 3 or goals.shape[-1] != 3 or goals.shape[:-2] != po.shape[:-2]
                or not 1 <= goals.shape[-2] <= po.shape[-2]):
            raise DmpcError(f"plan: goals {tuple(goals.shape)} must be [S,N_cmd,3] next to po [S,N,3] (or [N_cmd,3] next to [N,3]) with N_cmd <= N: po is {tuple(po.shape)}")
        n_cmd = goals.shape[-2]
        lead = goals.shape[:-1]
        S = 1 if po.ndim == 2 else po.shape[0]
        obst = po[..., n_cmd:, :]
        if obstacles is not None:
            obstacles = _f(obstacles)
            if obstacles.ndim != po.ndim or obstacles.shape[-1] != 3 or obstacles.shape[:-2] != po.shape[:-2]:
                raise DmpcError(f"plan: obstacles {tuple(obstacles.shape)} must be [S,M,3] next to po [S,N,3] (or [M,3] next to [N,3])")
            obst = np.concatenate([obst, obstacles], axis=-2)
        obst = _f(obst)
        M, W = obst.shape[-2], int(W)
        wp = np.zeros(lead + (max(W, 1), 3))
        n_wp, st, hops = (np.zeros(lead, dtype=np.int32) for _ in range(3))
        self._chk(self._L.dmpc_plan_routes(self._ctx, int(S), int(n_cmd), int(M), W, _dp(np.ascontiguousarray(po[..., :n_cmd, :])), _dp(goals),
                                           _dp(obst) if M else C.POINTER(C.c_double)(), float(cell), float(margin), _dp(wp), _ip(n_wp), _ip(st),
                                           _ip(hops)))
        return dict(waypoints=wp, n_wp=n_wp, plan_status=st, hops=hops)

    @_disturbable
    def replan(self, po, goals, K_T_max, cell, capture, margin=0.0, W=4, every=5, ahead=0, timeout=0, error_tol=0.01, histories=True, path=None,
               on_fail="stop", max_hold=14, disturb=None):
        """disturb: as transition().
        dmpc_transition_replan: plan() before column 0, route() from there, and every `every` columns (0: never) the agents whose remaining
        legs are no longer clear are planned again on the device, from where they are, round the vehicles where they are on that column and on
        the `ahead` columns behind it.  goals [N_cmd,3] next to an unbatched po, or [S,N_cmd,3]; po with MORE vehicles than goals: static
        vehicles; path [S,M,P,3]: scripted ones, po then covers the commanded agents.  cell, margin, W: plan()'s; capture, timeout, on_fail,
        max_hold: route()'s.  Returns what route() returns, and waypoints [S,N_cmd,W,3], n_wp, plan_status [S,N_cmd]: the plan in force when the
        scene ended (wp_col and wp_index refer to it), replan_count [S,N_cmd], replan_col [S,N_cmd]: the last re-plan's column (-1: none)."""
        po, goals, W = _f(po), _f(goals), int(W)
        hold = _on_fail("replan", on_fail)
        S, N, n_cmd, lead, path, M, P = _commanded("replan", po, goals, "N_cmd,3", "goals", path)
        if W < 1:
            raise DmpcError(f"replan: W must be >= 1, not {W!r}")
        if not float(capture) > 0.0:
            raise DmpcError(f"replan: capture must be > 0 (metres), not {capture!r}")
        if int(timeout) < 0 or int(every) < 0 or int(ahead) < 0:
            raise DmpcError(f"replan: timeout, every and ahead must be >= 0 (columns), not {timeout!r}, {every!r}, {ahead!r}")
        wp, wp_col = np.zeros(lead + (W, 3)), np.zeros(lead + (W,), dtype=np.int32)
        n_wp, pst, wp_index, rcnt, rcol = (np.zeros(lead, dtype=np.int32) for _ in range(5))
        head = [S, N + M, n_cmd, W, _dp(po), _dp(goals), float(cell), float(margin), int(every), int(ahead), float(capture), int(timeout), _dpn(path), P,
                int(K_T_max), float(error_tol), int(max_hold) if hold else 0]
        tail = [_dp(wp), _ip(n_wp), _ip(pst), _ip(wp_col), _ip(wp_index), _ip(rcnt), _ip(rcol)]
        extra = dict(wp_col=wp_col, wp_index=wp_index, waypoints=wp, n_wp=n_wp, plan_status=pst, replan_count=rcnt, replan_col=rcol)
        return self._fly(self._L.dmpc_transition_replan, head, _flight_outputs(S, lead, K_T_max, histories, hold), tail, extra)

    # ---- multi-GPU (one process per GPU): dmpc_multigpu.hip ----
    @staticmethod
    def comm_unique_id():
        """rank 0: the 128-byte RCCL id every rank passes to comm_init (hand it over by any out-of-band means)"""
        buf = C.create_string_buffer(128)
        if load().dmpc_comm_unique_id(buf):
            raise DmpcError(load().dmpc_last_error(None).decode())
        return buf.raw

    def comm_init(self, id128, nranks, rank):
        self._chk(self._L.dmpc_comm_init(self._ctx, bytes(id128), int(nranks), int(rank)))
        self.nranks, self.rank = int(nranks), int(rank)

    def comm_size(self):
        """ranks of this context's communicator as RCCL counts them (ncclCommCount)"""
        return int(self._L.dmpc_comm_size(self._ctx))

    def comm_destroy(self):
        self._L.dmpc_comm_destroy(self._ctx)
        self.nranks, self.rank = 1, 0

    def step_sharded_device(self, S, N, lT, x_p, x_v, x_a, pf, p_out, v_out, a_out, lT_next, status, info, stream=0):
        self._chk(self._L.dmpc_step_sharded_device(self._ctx, S, N, lT, x_p, x_v, x_a, pf, p_out, v_out, a_out, lT_next, status, info, stream))

    def transition_sharded(self, po, pf, K_T_max, error_tol=0.01, histories=True, gather=False):
        """dmpc_transition_sharded: po, pf [S,N,3] (the same on every rank); returns this rank's histories [S,count,K_T_max,3].
        gather=True (dmpc_transition_sharded_gather): the scene-wide histories are assembled on every rank's device afterwards, so that
        postcheck(K_T_used, pf, KT_alloc=K_T_max) checks the whole transition."""
        po, pf = _f(po), _f(pf)
        S, N = po.shape[0], po.shape[1]
        lo, cnt, cmax = partition(N, getattr(self, "nranks", 1), getattr(self, "rank", 0))
        entry = self._L.dmpc_transition_sharded_gather if gather else self._L.dmpc_transition_sharded
        return self._fly(entry, [S, N, _dp(po), _dp(pf), int(K_T_max), float(error_tol)], _flight_outputs(S, (S, cnt), K_T_max, histories),
                         extra=dict(lo=lo, count=cnt))

    def postcheck(self, K_T_used, pf, pk=None, vk=None, ak=None, KT_alloc=None, vmax=2.0, amax=1.0, Ts=0.01, interp=False,
                  mask=None, po_static=None, path=None):
        """failure_rate.m:136-195 for S scenes.  pk/vk/ak [S,N,KT_alloc,3] (or [N,KT,3]); None: use the histories the
        last transition() left on the device (then KT_alloc = its K_T_max).
        po_static [S,M,3] (or [M,3]): positions of M uncommanded vehicles (dmpc_postcheck_cmd; pf and the histories are the commanded
        agents'): the result gains min_dist_static / violation_static, the commanded-against-static check; everything else is unchanged.
        path [S,M,P,3] (or [M,P,3]; dmpc_postcheck_scripted, not together with po_static): M scripted vehicles, splined on the commanded agents'
        knots; the result gains min_dist_scripted / violation_scripted and, with interp, p_scripted [S,M,ns,3]."""
        pf = _f(pf)
        pos, path, M, P = _other_vehicles("postcheck", pf.shape, po_static, path)
        used, hist, KT_alloc, run = _check_inputs(K_T_used, (pk, vk, ak), KT_alloc, mask)
        S, N = (1, pf.shape[0]) if pf.ndim == 2 else pf.shape[:-1]
        out = dict(r_factor=np.zeros(S), h_scaled=np.zeros(S), n_samples=np.zeros(S, dtype=np.int32), min_dist=np.zeros(S),
                   violation=np.zeros(S, dtype=np.int32), totdist=np.zeros(S), traj_time=np.zeros(S))
        ns_alloc, p_i, p_s = 0, None, None
        if interp:   # upper bound of the sample count: r_factor is not known yet, so run once without and size from it
            pre = self.postcheck(used, pf, *hist, KT_alloc, vmax, amax, Ts, False, mask)   # (sizes only: no static pass)
            ns_alloc = max(int(pre["n_samples"].max()), 1)
            p_i = np.zeros((S, N, ns_alloc, 3))
        if path is not None:
            out["min_dist_scripted"], out["violation_scripted"] = np.zeros(S), np.zeros(S, dtype=np.int32)
            p_s = np.zeros((S, M, ns_alloc, 3)) if interp else None
            entry, dims, others = self._L.dmpc_postcheck_scripted, [S, N + M, N], [_dp(path), P]
            tail = [_dp(out["min_dist_scripted"]), _ip(out["violation_scripted"]), _dpn(p_s)]
        elif po_static is not None:
            out["min_dist_static"], out["violation_static"] = np.zeros(S), np.zeros(S, dtype=np.int32)
            entry, dims, others = self._L.dmpc_postcheck_cmd, [S, N + M, N], [_dpn(pos)]
            tail = [_dp(out["min_dist_static"]), _ip(out["violation_static"])]
        else:
            entry, dims, others, tail = self._L.dmpc_postcheck, [S, N], [], []
        self._chk(entry(self._ctx, *dims, *run, _dp(pf), *others, float(vmax), float(amax), float(Ts), _dp(out["r_factor"]), _dp(out["h_scaled"]),
                        _ip(out["n_samples"]), _dp(out["min_dist"]), _ip(out["violation"]), _dp(out["totdist"]), _dp(out["traj_time"]), _dpn(p_i),
                        ns_alloc, *tail))
        if interp:
            out["p"] = p_i
            if path is not None:
                out["p_scripted"] = p_s
        return out

    def clearance(self, K_T_used, pf, pk=None, vk=None, ak=None, KT_alloc=None, vmax=2.0, amax=1.0, Ts=0.01, mask=None, po_static=None,
                  path=None, reach=np.inf):
        """dmpc_postcheck_clearance: per commanded agent the nearest commanded partner (slot 0) and the nearest uncommanded vehicle (slot 1) over
        the 100 Hz samples of postcheck(), and when.  The leading arguments are postcheck()'s (pf gives the shape only).  Returns
        dict(dist [S,N_cmd,2], partner (0-based in the table: commanded agents first), sample, time = sample * Ts, NaN where there is no sample).
        reach: slots with a distance < reach are exact, the others report inf / -1 / -1 (inf: all exact); masked scenes NaN / -1 / -1."""
        shp = np.shape(pf)
        pos, path, M, P = _other_vehicles("clearance", shp, po_static, path)
        used, hist, KT_alloc, run = _check_inputs(K_T_used, (pk, vk, ak), KT_alloc, mask)
        S, N = (1, shp[0]) if len(shp) == 2 else shp[:-1]
        dist = np.zeros((S, N, 2))
        partner, sample = np.zeros((S, N, 2), dtype=np.int32), np.zeros((S, N, 2), dtype=np.int32)
        self._chk(self._L.dmpc_postcheck_clearance(self._ctx, S, N + M, N, *run, _dpn(pos), _dpn(path), P, float(vmax), float(amax), float(Ts),
                                                   float(reach), _dp(dist), _ip(partner), _ip(sample)))
        return dict(dist=dist, partner=partner, sample=sample, time=np.where(sample >= 0, sample * float(Ts), np.nan))

    def setpoints(self, K_T_used, N=None, pk=None, vk=None, ak=None, KT_alloc=None, vmax=2.0, amax=1.0, Ts=0.01, mask=None, first=0, count=None,
                  report_only=False):
        """dmpc_postcheck_setpoints: the 100 Hz setpoints p, v, a [S,N,count,3] of the commanded agents (samples first .. first+count-1, zero
        from n_samples on) and the limits report v_peak, v_peak_sample, a_peak, a_peak_sample [S,N] over ALL samples, next to r_factor,
        h_scaled, n_samples [S] of postcheck().  pk/vk/ak [S,N,KT_alloc,3] (or [N,KT,3]); None: the resident histories of the last transition
        (then N and KT_alloc say their shape).  count=None: the window runs from `first` to the largest n_samples (sized by a report-only
        call, as postcheck(interp=True) sizes p).  report_only: no p, v, a."""
        used, hist, KT_alloc, run = _check_inputs(K_T_used, (pk, vk, ak), KT_alloc, mask)
        S = used.size
        if hist[0] is not None:
            N = hist[0].shape[-3]
        assert N is not None
        if report_only:
            count = 0
        elif count is None:
            pre = self.setpoints(used, N, *hist, KT_alloc, vmax, amax, Ts, mask, report_only=True)
            count = max(int(pre["n_samples"].max()) - int(first), 1)
        count = int(count)
        out = dict(v_peak=np.zeros((S, N)), v_peak_sample=np.zeros((S, N), dtype=np.int32), a_peak=np.zeros((S, N)),
                   a_peak_sample=np.zeros((S, N), dtype=np.int32), r_factor=np.zeros(S), h_scaled=np.zeros(S), n_samples=np.zeros(S, dtype=np.int32))
        sp = [None] * 3 if report_only else [np.zeros((S, N, count, 3)) for _ in range(3)]
        self._chk(self._L.dmpc_postcheck_setpoints(self._ctx, S, int(N), *run, float(vmax), float(amax), float(Ts), int(first), count, *map(_dpn, sp),
                                                   _dp(out["v_peak"]), _ip(out["v_peak_sample"]), _dp(out["a_peak"]), _ip(out["a_peak_sample"]),
                                                   _dp(out["r_factor"]), _dp(out["h_scaled"]), _ip(out["n_samples"])))
        if not report_only:
            out["p"], out["v"], out["a"] = sp
        return out

    # ---- standalone small helpers (propStatedmpc.m, propState.m, is_inbounds.m, ReachedGoal.m) -----------
    def prop_state(self, A_p, A_v, a, A_initp=None, po=None, vo=None, off_p=None, off_v=None):
        A_p, A_v, a = _f(A_p), _f(A_v), _f(np.ravel(a))
        n_rows, n_cols = A_p.shape
        assert A_v.shape == A_p.shape and a.size == n_cols
        nul = C.POINTER(C.c_double)()
        opt = lambda x: _dp(_f(np.ravel(x))) if x is not None else nul
        A0 = _f(A_initp) if A_initp is not None else None
        p, v = np.zeros(n_rows), np.zeros(n_rows)
        self._chk(self._L.dmpc_prop_state(self._ctx, n_rows, n_cols, _dp(A_p), _dp(A_v), _dp(A0) if A0 is not None else nul, opt(po), opt(vo),
                                          opt(off_p), opt(off_v), _dp(a), _dp(p), _dp(v)))
        return p, v

    def is_inbounds(self, p, pmin, pmax):
        p = _f(np.asarray(p, float).reshape(-1, 3))
        out = np.zeros(1, dtype=np.int32)
        self._chk(self._L.dmpc_is_inbounds(self._ctx, p.shape[0], _dp(p), _dp(_f(np.ravel(pmin))), _dp(_f(np.ravel(pmax))), _ip(out)))
        return bool(out[0])

    def reached_goal(self, p, pf, error_tol):
        p, pf = _f(np.asarray(p, float).reshape(-1, 3)), _f(np.asarray(pf, float).reshape(-1, 3))
        out = np.zeros(1, dtype=np.int32)
        self._chk(self._L.dmpc_reached_goal(self._ctx, p.shape[0], _dp(p), _dp(pf), float(error_tol), _ip(out)))
        return bool(out[0])

    # ---- start / goal generators (randomTest.m, randomExchange.m) on the device ---------------
    def max_deviation(self, p, prev_p):
        """maxDeviation.m: p, prev_p [K,3] (the transposes of the MATLAB 3 x K matrices)."""
        p, prev_p = _f(p), _f(prev_p)
        out = np.zeros(1)
        self._chk(self._L.dmpc_max_deviation(self._ctx, p.shape[0], _dp(p), _dp(prev_p), _dp(out)))
        return float(out[0])

    def random_test(self, S, N, pmin, pmax, rmin, c, seed):
        """S scenes of randomTest(N,pmin,pmax,rmin,E1,order=2): (po, pf) each [S,N,3]."""
        po, pf = np.zeros((S, N, 3)), np.zeros((S, N, 3))
        self._chk(self._L.dmpc_random_test(self._ctx, S, N, _dp(_f(pmin)), _dp(_f(pmax)), float(rmin), float(c), int(seed), _dp(po), _dp(pf)))
        return po, pf

    def random_exchange(self, S, N, pmin, pmax, rmin, seed):
        """S scenes of randomExchange(N,pmin,pmax,rmin): (po, pf) each [S,N,3]."""
        po, pf = np.zeros((S, N, 3)), np.zeros((S, N, 3))
        self._chk(self._L.dmpc_random_exchange(self._ctx, S, N, _dp(_f(pmin)), _dp(_f(pmax)), float(rmin), int(seed), _dp(po), _dp(pf)))
        return po, pf

    # ---- dense collision rows (CollConstr* / AddCollConstr helpers) --------------------------
    def coll_rows(self, l, sel, k_cmp, k_blk, p, a0, rmin, c, A):
        """rows for the obstacles `sel` (0-based) of l [N_obs,K,3] at horizon column k_cmp against block k_blk of A
        [a_rows, ncols] (any strides).  Returns (Ain [n_sel, ncols], bin [n_sel], dist [n_sel])."""
        l = _f(l); A = np.asarray(A, dtype=np.float64)
        N_obs, K = l.shape[0], l.shape[1]
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        n_sel, (a_rows, ncols) = len(sel), A.shape
        if A.strides[0] % 8 or A.strides[1] % 8 or min(A.strides) <= 0:
            A = np.ascontiguousarray(A)
        base, rs, cs = _strided_base(A)
        Ain = np.zeros((n_sel, ncols)); b = np.zeros(n_sel); d = np.zeros(n_sel)
        self._chk(self._L.dmpc_coll_rows(self._ctx, K, N_obs, n_sel, _ip(sel), _dp(l), int(k_cmp), int(k_blk), _dp(_f(p)), _dp(_f(a0)),
                                         float(rmin), float(c), base, a_rows, ncols, rs, cs, _dp(Ain), ncols, 1, _dp(b), _dp(d)))
        return Ain, b, d

    def rows_dense(self, xi, kc, A):
        """structured rows (xi [nr,3], kc [nr] 1-based) -> dense Ain [nr, ncols] = -(xi . A(3kc-2:3kc, :))."""
        xi, A = _f(np.asarray(xi, float).reshape(-1, 3)), np.ascontiguousarray(A, dtype=np.float64)
        kc = np.ascontiguousarray(kc, dtype=np.int32)
        nr, (a_rows, ncols) = xi.shape[0], A.shape
        Ain = np.zeros((nr, ncols))
        self._chk(self._L.dmpc_rows_dense(self._ctx, nr, _dp(xi), _ip(kc), _dp(A), a_rows, ncols, ncols, 1, _dp(Ain), ncols, 1))
        return Ain

    def add_coll_constr(self, p, po, rmin, c, A, out_order="C"):
        """cup-SCP pairwise rows: p [N,K,3], po [N,3], A [3KN, ncols] -> (Ain [K N(N-1)/2, ncols], bin).
        out_order: "C" row-major, "F" column-major (MATLAB), "S" generic strides (a padded row-major buffer)."""
        p, po = _f(p), _f(po); A = np.asarray(A, dtype=np.float64)
        N, K = p.shape[0], p.shape[1]
        assert A.shape[0] == 3 * K * N
        if A.strides[0] % 8 or A.strides[1] % 8 or min(A.strides) <= 0:
            A = np.ascontiguousarray(A)
        base, rs, cs = _strided_base(A)
        nrows, ncols = K * N * (N - 1) // 2, A.shape[1]
        if out_order == "S":
            buf = np.zeros((nrows, 2 * ncols + 3)); Ain = buf[:, 1:2 * ncols + 1:2]
        else:
            Ain = np.zeros((nrows, ncols), order=out_order)
        b = np.zeros(nrows)
        self._chk(self._L.dmpc_add_coll_constr(self._ctx, K, N, _dp(p), _dp(po), float(rmin), float(c), base, ncols, rs, cs,
                                               Ain.ctypes.data_as(C.POINTER(C.c_double)), Ain.strides[0] // 8, Ain.strides[1] // 8, _dp(b)))
        return Ain, b

    # ---- device-pointer entry points (torch tensors: pass t.data_ptr()) ------------------------
    def step_device_cmd(self, S, N, n_cmd, lT, x_p, x_v, x_a, pf, p_out, v_out, a_out, lT_next, status, info, stream=0):
        """dmpc_step_device_cmd: the first n_cmd agents of a one-chunk table lT [S,45,N]; only columns < n_cmd of lT_next are written"""
        self._chk(self._L.dmpc_step_device_cmd(self._ctx, S, N, n_cmd, lT, x_p, x_v, x_a, pf, p_out, v_out, a_out,
                                               lT_next or None, status, info or None, stream or None))

    def scripted_cols_device(self, S, N, n_cmd, P, path, k, lT, lTf=0, stream=0):
        """dmpc_scripted_cols_device: columns n_cmd .. N-1 of lT [S,45,N] (and of the fp32 table lTf, if given) for MPC step k >= 1 from the
        device-resident path [S,N-n_cmd,P,3]: horizon entry kk of a vehicle = its sample min(k-1+kk, P-1)"""
        self._chk(self._L.dmpc_scripted_cols_device(self._ctx, S, N, n_cmd, P, path, int(k), lT, lTf or None, stream or None))

    def disturb_device(self, S, n_cmd, k, x_p, x_v, scene_done=0, stream=0):
        """dmpc_disturb_device: the disturbance in force, of column k, on device arrays x_p, x_v [S,n_cmd,3] (behind advance_device)"""
        self._chk(self._L.dmpc_disturb_device(self._ctx, S, n_cmd, k, x_p, x_v, scene_done, stream))

    def feedback_device(self, S, N, n_cmd, k, p_rows, v_rows, a_rows, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, lT_next, event, scene_done=0, stream=0):
        """dmpc_feedback_device: one column of the feedback rule (the disturbance in force inside it) on device arrays, behind step_device_cmd and
        INSTEAD of advance_device / disturb_device; v_rows and lT_next are in/out, event [S,n_cmd] is written"""
        self._chk(self._L.dmpc_feedback_device(self._ctx, S, N, n_cmd, k, p_rows, v_rows, a_rows, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, lT_next, event,
                                               scene_done, stream))

    def estimate_device(self, S, N, n_cmd, k, p_rows, v_rows, a_rows, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v, lT_next, event, scene_done=0,
                        stream=0):
        """dmpc_estimate_device: feedback_device with the measurement in force between the true deviation and the rule's decision; eh_p, eh_v
        [S,n_cmd,3] is the belief (in/out).  With no policy or no measurement set it launches nothing."""
        self._chk(self._L.dmpc_estimate_device(self._ctx, S, N, n_cmd, k, p_rows, v_rows, a_rows, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v,
                                               lT_next, event, scene_done, stream))

    def step_device(self, S, G, Cn, g_local, lT, x_p, x_v, x_a, pf, p_out, v_out, a_out, lT_next, status, info, stream=0):
        self._chk(self._L.dmpc_step_device(self._ctx, S, G, Cn, g_local, lT, x_p, x_v, x_a, pf, p_out, v_out, a_out,
                                           lT_next or None, status, info or None, stream or None))

    def table_from_rows_device(self, S, G, Cn, rows, lT, stream=0):
        self._chk(self._L.dmpc_table_from_rows_device(self._ctx, S, G, Cn, rows, lT, stream or None))

    def advance_device(self, count, p_out, v_out, a_out, status, x_p, x_v, x_a, stream=0):
        self._chk(self._L.dmpc_advance_device(self._ctx, count, p_out, v_out, a_out, status, x_p, x_v, x_a, stream or None))

    def assign_goals_device(self, S, N, po, goals, eps, max_rounds=0, perm=0, pf=0, price=0, cost=0, rounds=0, stream=0):
        """dmpc_assign_goals_device: po, goals [S,N,3] fp64 and the outputs (0: not wanted; perm, rounds int32) on the device"""
        self._chk(self._L.dmpc_assign_goals_device(self._ctx, S, N, po, goals, float(eps), int(max_rounds), perm or None, pf or None, price or None,
                                                   cost or None, rounds or None, stream or None))

    def assign_rect_device(self, S, N, M, po, goals, eps, max_rounds=0, perm=0, owner=0, pf=0, price=0, cost=0, rounds=0, stream=0):
        """dmpc_assign_rect_device: po [S,N,3], goals [S,M,3] fp64 and the outputs (0: not wanted; perm, owner, rounds int32) on the device"""
        self._chk(self._L.dmpc_assign_rect_device(self._ctx, S, N, M, po, goals, float(eps), int(max_rounds), perm or None, owner or None, pf or None,
                                                  price or None, cost or None, rounds or None, stream or None))

    def plan_routes_device(self, S, n_cmd, M, W, po_cmd, goals, obst, cell, margin, waypoints=0, n_wp=0, plan_status=0, hops=0, stream=0):
        """dmpc_plan_routes_device: po_cmd, goals [S,n_cmd,3], obst [S,M,3] fp64 and the outputs (0: not wanted; all but waypoints int32) on the device"""
        self._chk(self._L.dmpc_plan_routes_device(self._ctx, S, n_cmd, M, W, po_cmd, goals, obst or None, float(cell), float(margin), waypoints or None,
                                                  n_wp or None, plan_status or None, hops or None, stream or None))

    def replan_routes_device(self, S, n_cmd, M, W, x_p, goals, obst, cell, margin, k, waypoints, n_wp, cur, since=0, wp_col=0, pf=0, plan_status=0,
                             replan_count=0, replan_col=0, scene_done=0, stream=0):
        """dmpc_replan_routes_device: one re-plan step on column k.  x_p, goals [S,n_cmd,3], obst [S,M,3] fp64; waypoints [S,n_cmd,W,3] fp64, n_wp,
        cur [S,n_cmd] int32 are read and, for the agents with a leg that is not clear, rewritten; the others (0: not wanted) int32 but pf
        [S,n_cmd,3] fp64; scene_done [S] int32: scenes to skip.  All on the device."""
        self._chk(self._L.dmpc_replan_routes_device(self._ctx, S, n_cmd, M, W, x_p, goals, obst or None, float(cell), float(margin), int(k), waypoints, n_wp,
                                                    cur, since or None, wp_col or None, pf or None, plan_status or None, replan_count or None,
                                                    replan_col or None, scene_done or None, stream or None))

    def profile(self, enable=True):
        self._chk(self._L.dmpc_profile(self._ctx, 1 if enable else 0))

    def profile_read(self):
        ms, n = C.c_double(0.0), C.c_int64(0)
        self._chk(self._L.dmpc_profile_read(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_read2(self):
        """(solve-kernel avg ms, scan+order avg ms, steps) since the previous read."""
        a, b, n = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        self._chk(self._L.dmpc_profile_read2(self._ctx, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    @property
    def last_solve_kernel(self):
        """profiler name of the solve kernel the last MPC step launched for the bulk of its agents (dmpc_last_solve_kernel)"""
        return self._L.dmpc_last_solve_kernel(self._ctx).decode()

    @property
    def solve_count(self):
        return int(self._L.dmpc_solve_count(self._ctx))
