"""What the Python binding passes down: a stand-in for libdmpc_hip.so that records every call, the cases that drive the flight methods
(transition, mission, route, replan, transition_sharded) and the check methods (postcheck, clearance, setpoints) of multiagent_planning_amd/_lib.py
through it, and record(), which runs them all.  tests/binding_calls.json is record() of the binding BEFORE a change to it; tests/
test_binding_calls_cpu.py requires the binding as it stands to give the same.  No library and no GPU are needed.

    python tests/bindingcalls.py --record [--binding PATH/_lib.py]     # writes tests/binding_calls.json (DESIGN.md says when)

Per call the record holds [entry, [argument, ...]]: an int as it is, a float by repr, None for a null pointer, "out:<key>" for a pointer to
the array the method returns under <key>, "in:<first element>" for any other pointer (the cases give every input a leading value of its own:
po 100, goals / pf / waypoints 200, path 300, pk 400, vk 500, ak 600, po_static 700), and a structure passed by reference by its scalar fields
and the null-ness of its pointers.  Per case: the calls in order, the returned dict's keys in order with shape and dtype, and the values of what
is returned without being bound to an argument.  Per error case: the exception's type and message."""
import ast
import ctypes as C
import importlib.util
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
JSON_PATH = os.path.join(HERE, "binding_calls.json")
S, N, NC, M, P, Q, W, KT = 2, 5, 4, 2, 3, 2, 2, 6      # the smallest shapes that tell the branches apart (NC: commanded agents)
METHODS = ("transition", "mission", "route", "replan", "transition_sharded", "postcheck", "clearance", "setpoints")
LAST_ERROR = b"stand-in: refused"


# ---- the stand-in library -----------------------------------------------------------------------------------------------------------------
def _seen(a):
    """an argument as the stand-in sees it at call time: a plain value, or ("ptr", address, first element)"""
    if a is None:
        return None
    if isinstance(a, (bool, int, np.integer)):
        return int(a)
    if isinstance(a, float):
        return repr(a)
    if isinstance(a, bytes):
        return "bytes:" + a.decode()
    if isinstance(a, C._Pointer):
        if not a:
            return None
        arr = getattr(a, "_arr", None)      # (numpy's data_as keeps the array here)
        first = "empty" if arr is not None and arr.size == 0 else a[0]
        return ("ptr", C.cast(a, C.c_void_p).value, first)
    if type(a).__name__ == "CArgObject":    # C.byref(structure)
        st = a._obj
        fields = {}
        for name, _ in st._fields_:
            v = getattr(st, name)
            fields[name] = _seen(v) if isinstance(v, (int, float)) else ("set" if v else None)
        return {type(st).__name__: fields}
    raise TypeError(f"stand-in library: an argument of type {type(a).__name__}")


class StandIn:
    """every attribute is a function that records its arguments and returns 0.  fail: the entry that returns -1 instead; poke: {entry:
    (argument index, value)} written to the first element behind that pointer (what a case needs the library to have answered), next to
    ANSWERS: the assigned goals lead with 250, so that the flight behind an assignment shows whose goals it flies"""
    ANSWERS = {"dmpc_assign_goals": (8, 250.0), "dmpc_assign_rect": (10, 250.0)}

    def __init__(self, fail=None, poke=None):
        self.calls, self.keep, self.fail, self.poke = [], [], fail, poke or {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def entry(*args):
            self.keep.append(args)          # (no array is freed, so no address comes twice)
            self.calls.append((name, [_seen(a) for a in args]))
            if name == "dmpc_last_error":
                return LAST_ERROR
            for answers in (self.ANSWERS, self.poke):
                if name in answers:
                    i, v = answers[name]
                    args[i][0] = v
            return -1 if name == self.fail else 0
        return entry


def standin_dmpc(b, lib):
    d = object.__new__(b.Dmpc)
    d._ctx, d.prm, d._L = 7, b.make_params(), lib
    return d


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def arr(start, *shape):
    return start + 0.001 * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


def iarr(start, *shape):
    return (start + np.zeros(shape, dtype=np.int64)).astype(np.int32)


def _b(batched):
    return (S,) if batched else ()


def hist(batched=True, n=NC):
    return dict(pk=arr(400, *_b(batched), n, KT, 3), vk=arr(500, *_b(batched), n, KT, 3), ak=arr(600, *_b(batched), n, KT, 3))


DISTURB = dict(noise_p=0.01, noise_v=0.02, wind=[0.1, 0.0, 0.0], pushes=[[0, 1, 2, 0.1, 0, 0, 0, 0.2, 0]], seed=9)
USED = np.array([6, 5], dtype=np.int32)


def _forms(extra_axes):
    """the shape forms shared by mission (goals [.., Q, N_cmd, 3]), route (waypoints [.., N_cmd, W, 3]) and replan (goals [.., N_cmd, 3]):
    name -> (po, commanded array, path)"""
    def cmd(bt, n):
        shape = {"Q": _b(bt) + (Q, n, 3), "W": _b(bt) + (n, W, 3), "": _b(bt) + (n, 3)}[extra_axes]
        return arr(200, *shape)
    return {
        "static": (arr(100, S, N, 3), cmd(True, NC), None),
        "all": (arr(100, S, NC, 3), cmd(True, NC), None),
        "path": (arr(100, S, NC, 3), cmd(True, NC), arr(300, S, M, P, 3)),
        "unbatched": (arr(100, N, 3), cmd(False, NC), None),
        "unbatched-path": (arr(100, NC, 3), cmd(False, NC), arr(300, M, P, 3)),
    }


def cases():
    """[(name, method, args, kwargs, options)]; options: nranks / rank (attributes of the context), fail, poke (StandIn's)"""
    out = []

    def add(name, method, *args, _opt=None, **kw):
        out.append((name, method, args, kw, _opt or {}))

    # transition
    tforms = {
        "plain": (arr(100, S, N, 3), arr(200, S, N, 3), None),
        "unbatched": (arr(100, N, 3), arr(200, N, 3), None),
        "flat": (arr(100, S, N, 3), arr(200, S * N * 3), None),
        "cmd": (arr(100, S, N, 3), arr(200, S, NC, 3), None),
        "unbatched-cmd": (arr(100, N, 3), arr(200, NC, 3), None),
        "path": (arr(100, S, NC, 3), arr(200, S, NC, 3), arr(300, S, M, P, 3)),
        "unbatched-path": (arr(100, NC, 3), arr(200, NC, 3), arr(300, M, P, 3)),
    }
    for f, (po, pf, path) in tforms.items():
        for on_fail in ("stop", "hold"):
            for h in (True, False):
                add(f"transition-{f}-{on_fail}-{'hist' if h else 'nohist'}", "transition", po, pf, KT, histories=h, path=path, on_fail=on_fail)
    add("transition-positional", "transition", tforms["cmd"][0], tforms["cmd"][1], KT, 0.02, False, None, "hold", 3)
    add("transition-assign-cmd", "transition", arr(100, S, N, 3), arr(200, S, NC, 3), KT, assign=True)
    add("transition-assign-flat-hold", "transition", arr(100, S, N, 3), arr(200, S * N * 3), KT, assign=True, on_fail="hold", max_hold=2)
    add("transition-assign-unbatched-path", "transition", arr(100, NC, 3), arr(200, NC, 3), KT, assign=True, path=arr(300, M, P, 3), histories=False)
    add("transition-rect", "transition", arr(100, S, N, 3), arr(200, S, 3, 3), KT, assign="rect")
    add("transition-rect-unbatched-hold", "transition", arr(100, N, 3), arr(200, 7, 3), KT, 0.02, assign="rect", on_fail="hold")
    add("transition-rect-path", "transition", arr(100, S, NC, 3), arr(200, S, 3, 3), KT, assign="rect", path=arr(300, S, M, P, 3))
    add("transition-disturb", "transition", arr(100, S, N, 3), arr(200, S, N, 3), KT, disturb=DISTURB)
    add("transition-disturb-noise-only-hold", "transition", arr(100, S, N, 3), arr(200, S, NC, 3), KT, on_fail="hold", disturb=dict(noise_p=0.01))
    add("transition-disturb-assign", "transition", arr(100, S, N, 3), arr(200, S, NC, 3), KT, assign=True, disturb=DISTURB)
    add("transition-disturb-rect", "transition", arr(100, S, N, 3), arr(200, S, 3, 3), KT, assign="rect", disturb=dict(wind=np.ones((S, 3))))
    add("transition-disturb-cleared-after-a-refusal-of-the-library", "transition", arr(100, S, N, 3), arr(200, S, N, 3), KT, disturb=DISTURB,
        _opt=dict(fail="dmpc_transition"))

    # mission
    for f, (po, goals, path) in _forms("Q").items():
        for on_fail in ("stop", "hold"):
            for h in (True, False):
                add(f"mission-{f}-{on_fail}-{'hist' if h else 'nohist'}", "mission", po, goals, KT, histories=h, path=path, on_fail=on_fail)
    po, goals, path = _forms("Q")["static"]
    for on_fail in ("stop", "hold"):
        add(f"mission-deadline-row-{on_fail}", "mission", po, goals, KT, deadline=[5, 0], on_fail=on_fail)
        add(f"mission-deadline-full-{on_fail}", "mission", po, goals, KT, 0.02, deadline=iarr(5, S, Q), on_fail=on_fail, max_hold=3)
    add("mission-deadline-unbatched", "mission", arr(100, N, 3), arr(200, Q, NC, 3), KT, deadline=[5, 0])
    add("mission-positional", "mission", po, goals, KT, 0.02, False, [5, 0], None, "hold", 3)
    add("mission-assign", "mission", po, goals, KT, assign=True, deadline=[5, 0])
    add("mission-assign-unbatched-path-hold", "mission", arr(100, NC, 3), arr(200, Q, NC, 3), KT, assign=True, path=arr(300, M, P, 3), on_fail="hold")
    add("mission-rect", "mission", po, arr(200, S, Q, 3, 3), KT, assign="rect")
    add("mission-rect-unbatched-hold", "mission", arr(100, N, 3), arr(200, Q, 7, 3), KT, assign="rect", on_fail="hold", histories=False)
    add("mission-disturb", "mission", po, goals, KT, disturb=DISTURB)
    add("mission-disturb-assign-hold", "mission", po, goals, KT, assign=True, on_fail="hold", disturb=dict(noise_v=0.5, seed=3))

    # route
    n_wp = np.array([[2, 1, 2, 1], [1, 2, 2, 2]])
    for f, (po, wp, path) in _forms("W").items():
        for on_fail in ("stop", "hold"):
            for h in (True, False):
                add(f"route-{f}-{on_fail}-{'hist' if h else 'nohist'}", "route", po, wp, KT, 0.3, histories=h, path=path, on_fail=on_fail)
    po, wp, path = _forms("W")["static"]
    for on_fail in ("stop", "hold"):
        add(f"route-n_wp-timeout-{on_fail}", "route", po, wp, KT, 0.3, n_wp, 4, on_fail=on_fail, max_hold=3)
    add("route-n_wp-unbatched-path", "route", arr(100, NC, 3), arr(200, NC, W, 3), KT, 0.3, n_wp=n_wp[0], path=arr(300, M, P, 3))
    add("route-positional", "route", po, wp, KT, 0.3, n_wp.astype(np.int32), 4, 0.02, False, None, "hold", 3)
    add("route-disturb", "route", po, wp, KT, 0.3, timeout=4, disturb=DISTURB)
    add("route-disturb-hold", "route", po, wp, KT, 0.3, on_fail="hold", disturb=dict(noise_p=0.01))

    # replan
    for f, (po, goals, path) in _forms("").items():
        for on_fail in ("stop", "hold"):
            for h in (True, False):
                add(f"replan-{f}-{on_fail}-{'hist' if h else 'nohist'}", "replan", po, goals, KT, 0.25, 0.3, histories=h, path=path, on_fail=on_fail)
    po, goals, path = _forms("")["static"]
    for on_fail in ("stop", "hold"):
        add(f"replan-every0-timeout-{on_fail}", "replan", po, goals, KT, 0.25, 0.3, every=0, timeout=4, ahead=2, margin=0.1, W=3, on_fail=on_fail)
    add("replan-positional", "replan", po, goals, KT, 0.25, 0.3, 0.1, 3, 2, 1, 4, 0.02, False, None, "hold", 3)
    add("replan-disturb", "replan", po, goals, KT, 0.25, 0.3, disturb=DISTURB)
    add("replan-disturb-path-hold", "replan", arr(100, S, NC, 3), goals, KT, 0.25, 0.3, path=arr(300, S, M, P, 3), on_fail="hold",
        disturb=dict(noise_p=0.01))

    # transition_sharded
    for gather in (False, True):
        for h in (True, False):
            add(f"sharded-{'gather' if gather else 'own'}-{'hist' if h else 'nohist'}", "transition_sharded", arr(100, S, N, 3), arr(200, S, N, 3), KT,
                histories=h, gather=gather)
    add("sharded-second-rank-of-two", "transition_sharded", arr(100, S, N, 3), arr(200, S, N, 3), KT, 0.02, _opt=dict(nranks=2, rank=1))

    # postcheck
    pf, pfu = arr(200, S, NC, 3), arr(200, NC, 3)
    modes = {"plain": {}, "static": dict(po_static=arr(700, S, M, 3)), "path": dict(path=arr(300, S, M, P, 3))}
    for m, kw in modes.items():
        for interp in (False, True):
            tag = f"postcheck-{m}{'-interp' if interp else ''}"
            add(tag + "-resident", "postcheck", USED, pf, KT_alloc=KT, interp=interp, **kw)
            add(tag + "-given", "postcheck", USED, pf, **hist(), interp=interp, **kw)
    add("postcheck-mask", "postcheck", USED, pf, KT_alloc=KT, mask=[1, 0])
    add("postcheck-mask-interp-path-limits", "postcheck", USED, pf, **hist(), vmax=3.0, amax=1.5, Ts=0.02, interp=True, mask=[1, 0], path=arr(300, S, M, P, 3))
    add("postcheck-mask-interp-static", "postcheck", USED, pf, KT_alloc=KT, interp=True, mask=np.array([1, 0]), po_static=arr(700, S, M, 3))
    add("postcheck-static-none", "postcheck", USED, pf, KT_alloc=KT, po_static=np.zeros((S, 0, 3)))
    add("postcheck-unbatched", "postcheck", 6, pfu, **hist(False))
    add("postcheck-unbatched-static-interp", "postcheck", 6, pfu, **hist(False), interp=True, po_static=arr(700, M, 3))
    add("postcheck-unbatched-path", "postcheck", 6, pfu, KT_alloc=KT, path=arr(300, M, P, 3))
    add("postcheck-positional", "postcheck", USED, pf, *hist().values(), None, 3.0, 1.5, 0.02, True, [1, 0])

    # clearance
    for m, kw in modes.items():
        for reach in (np.inf, 0.8):
            add(f"clearance-{m}-reach-{reach}-resident", "clearance", USED, pf, KT_alloc=KT, reach=reach, **kw)
            add(f"clearance-{m}-reach-{reach}-given", "clearance", USED, pf, **hist(), reach=reach, **kw)
    add("clearance-mask-limits", "clearance", USED, pf, KT_alloc=KT, vmax=3.0, amax=1.5, Ts=0.02, mask=[1, 0])
    add("clearance-static-none", "clearance", USED, pf, KT_alloc=KT, po_static=np.zeros((S, 0, 3)))
    add("clearance-unbatched-static", "clearance", 6, pfu, **hist(False), po_static=arr(700, M, 3))
    add("clearance-unbatched-path", "clearance", 6, pfu.tolist(), KT_alloc=KT, path=arr(300, M, P, 3))

    # setpoints
    add("setpoints-report-only", "setpoints", USED, **hist(), report_only=True)
    add("setpoints-report-only-resident", "setpoints", USED, N=NC, KT_alloc=KT, report_only=True, mask=[1, 0])
    add("setpoints-sized", "setpoints", USED, **hist())
    add("setpoints-sized-resident-first-limits", "setpoints", USED, NC, KT_alloc=KT, vmax=3.0, amax=1.5, Ts=0.02, mask=[1, 0], first=2)
    add("setpoints-window", "setpoints", USED, **hist(), first=3, count=4)
    add("setpoints-window-resident", "setpoints", USED, N=NC, KT_alloc=KT, first=3, count=4)
    add("setpoints-unbatched", "setpoints", 6, **hist(False), count=2)
    return out


def error_cases():
    """[(name, method, bound, args, kwargs, options)]: every refusal of the flight and check methods.  bound False: called with self = None,
    which is how the *_cpu.py tests reach the argument rules -- they fire before anything touches the context"""
    out = []

    def add(name, method, *args, _bound=False, _opt=None, **kw):
        out.append((name, method, _bound, args, kw, _opt or {}))

    po, poc, pf, pfc = arr(100, S, N, 3), arr(100, S, NC, 3), arr(200, S, N, 3), arr(200, S, NC, 3)
    path = arr(300, S, M, P, 3)
    # transition
    add("transition-assign-value", "transition", po, pf, KT, assign="square")
    add("transition-assign-value-2", "transition", po, pf, KT, assign=2)
    add("transition-rect-shape", "transition", po, arr(200, 3, 3), KT, assign="rect")
    add("transition-assign-shape", "transition", poc, pf, KT, assign=True)
    add("transition-assign-round-cap", "transition", po, pfc, KT, assign=True, _bound=True, _opt=dict(poke={"dmpc_assign_goals": (11, -1)}))
    add("transition-rect-round-cap", "transition", po, arr(200, S, 3, 3), KT, assign="rect", _bound=True, _opt=dict(poke={"dmpc_assign_rect": (13, -1)}))
    add("transition-on_fail", "transition", po, pf, KT, on_fail="go on")
    add("transition-path-agents", "transition", po, pfc, KT, path=path)
    add("transition-path-batch", "transition", poc, pfc, KT, path=path[0])
    add("transition-path-empty", "transition", poc, pfc, KT, path=np.zeros((S, M, 0, 3)))
    add("transition-pf-batch", "transition", po, pfc[0], KT)
    add("transition-pf-more-agents", "transition", poc, pf, KT)
    add("transition-disturb-value", "transition", po, pf, KT, disturb=[0.1], _bound=True)
    add("transition-library-refuses", "transition", po, pfc, KT, _bound=True, _opt=dict(fail="dmpc_transition_cmd"))
    # mission
    g = arr(200, S, Q, NC, 3)
    add("mission-on_fail", "mission", po, g, KT, on_fail="go on")
    add("mission-goals-shape", "mission", po, g[0], KT)
    add("mission-assign-value", "mission", po, g, KT, assign="square")
    add("mission-rect-no-points", "mission", po, np.zeros((S, Q, 0, 3)), KT, assign="rect")
    add("mission-assign-agents", "mission", poc, arr(200, S, Q, N, 3), KT, assign=True)
    add("mission-assign-round-cap", "mission", po, g, KT, assign=True, _bound=True, _opt=dict(poke={"dmpc_assign_goals": (11, -1)}))
    add("mission-path-agents", "mission", po, g, KT, path=path)
    add("mission-path-batch", "mission", poc, g, KT, path=path[0])
    add("mission-more-agents", "mission", poc, arr(200, S, Q, N, 3), KT)
    add("mission-no-agents", "mission", po, np.zeros((S, Q, 0, 3)), KT)
    add("mission-disturb-value", "mission", po, g, KT, disturb="wind", _bound=True)
    # route
    wp = arr(200, S, NC, W, 3)
    add("route-on_fail", "route", po, wp, KT, 0.3, on_fail="go on")
    add("route-waypoints-shape", "route", po, wp[0], KT, 0.3)
    add("route-no-waypoints", "route", po, np.zeros((S, NC, 0, 3)), KT, 0.3)
    add("route-path-agents", "route", po, wp, KT, 0.3, path=path)
    add("route-path-batch", "route", poc, wp, KT, 0.3, path=path[0])
    add("route-more-agents", "route", poc, arr(200, S, N, W, 3), KT, 0.3)
    add("route-n_wp-shape", "route", po, wp, KT, 0.3, n_wp=np.ones(NC, dtype=int))
    add("route-n_wp-range", "route", po, wp, KT, 0.3, n_wp=np.full((S, NC), W + 1))
    add("route-n_wp-dtype", "route", po, wp, KT, 0.3, n_wp=np.ones((S, NC)))
    add("route-capture", "route", po, wp, KT, float("nan"))
    add("route-timeout", "route", po, wp, KT, 0.3, timeout=-1)
    add("route-disturb-value", "route", po, wp, KT, 0.3, disturb=0.1, _bound=True)
    # replan
    add("replan-on_fail", "replan", po, pfc, KT, 0.25, 0.3, on_fail="go on")
    add("replan-goals-shape", "replan", po, pfc[0], KT, 0.25, 0.3)
    add("replan-path-agents", "replan", po, pfc, KT, 0.25, 0.3, path=path)
    add("replan-path-batch", "replan", poc, pfc, KT, 0.25, 0.3, path=path[0])
    add("replan-more-agents", "replan", poc, pf, KT, 0.25, 0.3)
    add("replan-W", "replan", po, pfc, KT, 0.25, 0.3, W=0)
    add("replan-capture", "replan", po, pfc, KT, 0.25, 0.0)
    add("replan-columns", "replan", po, pfc, KT, 0.25, 0.3, every=-1)
    add("replan-disturb-value", "replan", po, pfc, KT, 0.25, 0.3, disturb=(), _bound=True)
    # postcheck, clearance
    for m in ("postcheck", "clearance"):
        add(m + "-path-and-static", m, USED, pfc, KT_alloc=KT, path=path, po_static=arr(700, S, M, 3))
        add(m + "-static-batch", m, USED, pfc, KT_alloc=KT, po_static=arr(700, M, 3))
        add(m + "-static-xyz", m, USED, pfc, KT_alloc=KT, po_static=arr(700, S, M, 2))
        add(m + "-path-batch", m, USED, pfc, KT_alloc=KT, path=path[0])
        add(m + "-path-no-vehicle", m, USED, pfc, KT_alloc=KT, path=np.zeros((S, 0, P, 3)))
    return out


# ---- running them ---------------------------------------------------------------------------------------------------------------------------
def _plain(x):
    """numpy values as JSON-ready ones, floats by repr"""
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return repr(float(x))
    if isinstance(x, (int, np.integer)):
        return int(x)
    return x


def _context(b, opt):
    lib = StandIn(opt.get("fail"), opt.get("poke"))
    d = standin_dmpc(b, lib)
    for k in ("nranks", "rank"):
        if k in opt:
            setattr(d, k, opt[k])
    return d, lib


def _calls(lib, out):
    key_of = {}
    if isinstance(out, dict):
        key_of = {v.ctypes.data: k for k, v in out.items() if isinstance(v, np.ndarray) and v.size}
    bound, calls = set(), []
    for name, args in lib.calls:
        row = []
        for a in args:
            if isinstance(a, tuple):
                _, addr, first = a
                if addr in key_of:
                    bound.add(key_of[addr])
                    a = "out:" + key_of[addr]
                else:
                    a = f"in:{first}"
            row.append(a)
        calls.append([name, row])
    return calls, bound


def run_case(b, method, args, kw, opt):
    d, lib = _context(b, opt)
    partition = b.partition
    b.partition = lambda n, g, rank: (lib.partition(int(n), int(g), int(rank)), (1, 3, 3))[1]     # (partition() would load the library)
    try:
        out = getattr(d, method)(*args, **kw)
    except b.DmpcError as e:
        calls, _ = _calls(lib, None)
        return dict(calls=calls, raised=[type(e).__name__, str(e)])
    finally:
        b.partition = partition
    calls, bound = _calls(lib, out)
    returns, values = [], {}
    for k, v in out.items():
        if isinstance(v, np.ndarray):
            returns.append([k, list(v.shape), str(v.dtype)])
            if k not in bound:
                values[k] = _plain(v.tolist())
        else:
            returns.append([k, None if v is None else _plain(v)])
    return dict(calls=calls, returns=returns, values=values)


def run_error(b, method, bound, args, kw, opt):
    """the DmpcError an error case ends in (an error case that ends in none is itself an error)"""
    d, lib = _context(b, opt) if bound else (None, None)
    try:
        getattr(b.Dmpc, method)(d, *args, **kw)
    except b.DmpcError as e:
        return e
    raise AssertionError(f"{method}: no DmpcError")


def record(b):
    """{"cases": {name: ...}, "errors": {name: [type, message]}} of binding module b"""
    rec = dict(cases={}, errors={})
    for name, method, args, kw, opt in cases():
        assert name not in rec["cases"], name
        rec["cases"][name] = run_case(b, method, args, kw, opt)
    for name, method, bound, args, kw, opt in error_cases():
        assert name not in rec["errors"], name
        e = run_error(b, method, bound, args, kw, opt)
        rec["errors"][name] = [type(e).__name__, str(e)]
    return json.loads(json.dumps(rec))


# ---- which refusals the error cases reach ---------------------------------------------------------------------------------------------------
def refusals(b):
    """[(function, first line, last line)] of every `raise DmpcError` in METHODS and in the private functions and methods of the module they
    use, directly or through one another (found by name in the source; line numbers are those of the module's file)"""
    tree = ast.parse(inspect.getsource(b))
    defs = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            defs[node.name] = node
        elif isinstance(node, ast.ClassDef) and node.name == "Dmpc":
            defs.update({f.name: f for f in node.body if isinstance(f, ast.FunctionDef)})
    todo, seen = list(METHODS), set()
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        for n in ast.walk(defs[name]):
            ref = n.id if isinstance(n, ast.Name) else n.attr if isinstance(n, ast.Attribute) else None
            if ref in defs and ref.startswith("_") and not ref.startswith("__"):
                todo.append(ref)
    out = []
    for name in sorted(seen):
        for n in ast.walk(defs[name]):
            if isinstance(n, ast.Raise) and isinstance(n.exc, ast.Call) and getattr(n.exc.func, "id", None) == "DmpcError":
                out.append((name, n.lineno, n.end_lineno))
    return out


def raised_at(b):
    """{line of the module's file} on which the error cases' exceptions were raised"""
    lines = set()
    for name, method, bound, args, kw, opt in error_cases():
        tb = run_error(b, method, bound, args, kw, opt).__traceback__
        while tb.tb_next is not None:
            tb = tb.tb_next
        assert tb.tb_frame.f_code.co_filename == b.__file__, name
        lines.add(tb.tb_lineno)
    return lines


# ---- the file -------------------------------------------------------------------------------------------------------------------------------
def dumps(rec):
    """one line per call and per returned key, so that a change shows as the lines it changes"""
    j = lambda x: json.dumps(x, separators=(", ", ": "))
    lines = ["{", ' "cases": {']
    for i, (name, c) in enumerate(rec["cases"].items()):
        lines.append(f"  {j(name)}: {{")
        lines.append('   "calls": [')
        lines += [f"    {j(call)}{',' if k + 1 < len(c['calls']) else ''}" for k, call in enumerate(c["calls"])]
        rest = [k for k in c if k != "calls"]
        lines.append("   ]," if rest else "   ]")
        for k in rest:
            if k == "returns":
                lines.append('   "returns": [')
                lines += [f"    {j(r)}{',' if n + 1 < len(c[k]) else ''}" for n, r in enumerate(c[k])]
                lines.append("   ]" + ("," if k != rest[-1] else ""))
            else:
                lines.append(f"   {j(k)}: {j(c[k])}" + ("," if k != rest[-1] else ""))
        lines.append("  }" + ("," if i + 1 < len(rec["cases"]) else ""))
    lines += [" },", ' "errors": {']
    lines += [f"  {j(name)}: {j(e)}{',' if i + 1 < len(rec['errors']) else ''}" for i, (name, e) in enumerate(rec["errors"].items())]
    lines += [" }", "}", ""]
    return "\n".join(lines)


def load_binding(path=None):
    if path is None:
        sys.path.insert(0, os.path.dirname(HERE))
        from multiagent_planning_amd import _lib
        return _lib
    spec = importlib.util.spec_from_file_location("bindingcalls_binding", path)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="write tests/binding_calls.json")
    ap.add_argument("--binding", metavar="PATH", default=None, help="a _lib.py file to record in place of the package's")
    ap.add_argument("--out", metavar="FILE", default=JSON_PATH, help="with --record: another file")
    a = ap.parse_args()
    text = dumps(record(load_binding(a.binding)))
    assert json.loads(text) == record(load_binding(a.binding))
    if a.record:
        open(a.out, "w").write(text)
        print("wrote", a.out)
    else:
        print("differs from" if text != open(JSON_PATH).read() else "equals", JSON_PATH)
