"""Test helper: the measured state (dmpc_set_measurement) -- the rule of include/dmpc_hip.h restated in numpy, every operation an fp64 operation
rounded on its own (numpy fuses nothing), one column (column), the sensor noise over the counter-based stream of oracle/generators.py (sample),
the closed loop a caller could write on the host over an MPC step (loop), and raw ctypes calls of the entries.  The device,
dmpc_estimate_apply_host, dmpc_measurement_sample and this file must agree bit for bit.

There is no reference counterpart.  Per commanded agent, beside tests/feedback.py's true state x, planning state xh and tracking error e: the
belief eh, the planner's estimate of e.  Column 0: eh = 0.  Column k >= 1: see column()."""
import ctypes as C

import numpy as np

import disturb as di
import feedback as fb
import mission as mi
from multiagent_planning_amd import _lib
from obstacles import _dp, _ip, _f   # noqa: F401
from oracle.generators import Stream

K = 15
EST_INT = ("err_p_col", "err_v_col", "dev_p_col", "dev_v_col")
EST_MAX = ("err_p_max", "err_v_max", "dev_p_max", "dev_v_max")
EST_LOG = EST_INT + EST_MAX + ("eh_p", "eh_v")
NO_NOISE = dict(noise_p=0.0, noise_v=0.0, gain_p=1.0, gain_v=1.0, seed=0)


def sample(S, n, k, amp_p, amp_v, seed, col0=0):
    """(m_p, m_v), [S,n,3] each: the sensor noise of local column k of a flight whose column 0 is the caller's col0; k == 0 gives zeros"""
    mp, mv = np.zeros((S, n, 3)), np.zeros((S, n, 3))
    if k == 0:
        return mp, mv
    amp_p, amp_v = float(amp_p), float(amp_v)
    for s in range(S):
        for i in range(n):
            st = Stream(int(seed), (1 << 63) | (int(s) << 32) | int(i))
            st.ctr = 6 * (int(col0) + int(k))
            u = [2.0 * st.draw() - 1.0 for _ in range(6)]
            for c in range(3):
                mp[s, i, c] = amp_p * u[c]
                mv[s, i, c] = amp_v * u[3 + c]
    return mp, mv


def _estimate(b, g, m, amp, gain):
    """gh of one of (p, v): y = amp > 0 ? g + m : g;  gh = gain == 1 ? y : b + gain * (y - b)"""
    y = g + m if amp > 0 else g
    if gain == 1.0:
        return y
    d = y - b
    d = gain * d
    return b + d


def column(trigger_p, trigger_v, reanchor, h, p, v, a, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v, lT_next, meas, mp=None, mv=None, dp=None,
           dv=None, scene_done=None):
    """One column of the rule.  tests/feedback.py::column's arguments with the belief eh_p, eh_v [S,n,3] behind e_v; meas = (amp_p, amp_v, gain_p,
    gain_v); mp, mv [S,n,3] the sensor noise of the column (None: zeros).  Nothing is changed in place; returns what feedback.column returns (n_p,
    n_v are the norms of gh, the ones the events are decided on) plus eh_p, eh_v, gh [S,n,6], err_p, err_v [S,n] (the norms of g - gh) and
    true_p, true_v [S,n] (the norms of g) -- for a finished scene the inputs, event 0, everything else 0."""
    amp_p, amp_v, gain_p, gain_v = (float(t) for t in meas)
    p, v, a = (np.asarray(t, float) for t in (p, v, a))
    x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v = (np.asarray(t, float) for t in (x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v))
    S, n = p.shape[:2]
    zero = np.zeros((S, n, 3))
    dp, dv, mp, mv = (zero if t is None else t for t in (dp, dv, mp, mv))
    live = np.ones(S, bool) if scene_done is None else np.asarray(scene_done) == 0
    live3 = np.broadcast_to(live[:, None, None], (S, n, 3))
    adv = np.broadcast_to(((np.asarray(status) & 1) == 1)[..., None], (S, n, 3))
    he = h * e_v
    ga = e_p + he
    ga = ga + dp
    gn = e_p + dp
    g_p = np.where(adv, ga, gn)
    g_v = e_v + dv
    q_p, q_v = np.where(adv, p[..., :3], xh_p), np.where(adv, v[..., :3], xh_v)
    nx_p, nx_v = q_p + g_p, q_v + g_v
    nx_a = np.where(adv, a[..., :3], x_a)
    hb = h * eh_v
    ba = eh_p + hb
    b_p, b_v = np.where(adv, ba, eh_p), eh_v
    gh_p, gh_v = _estimate(b_p, g_p, mp, amp_p, gain_p), _estimate(b_v, g_v, mv, amp_v, gain_v)
    n_p, n_v = fb.norm3(gh_p), fb.norm3(gh_v)
    event = ((n_p > trigger_p) | (n_v > trigger_v)) & live[:, None]
    ev3 = np.broadcast_to(event[..., None], (S, n, 3))
    d_p, d_v = g_p - gh_p, g_v - gh_v
    hx_p, hx_v = q_p + gh_p, q_v + gh_v
    l2 = live[:, None]
    o = dict(x_p=np.where(live3, nx_p, x_p), x_v=np.where(live3, nx_v, x_v), x_a=np.where(live3, nx_a, x_a),
             xh_p=np.where(live3, np.where(ev3, hx_p, q_p), xh_p), xh_v=np.where(live3, np.where(ev3, hx_v, q_v), xh_v),
             e_p=np.where(live3, np.where(ev3, d_p, g_p), e_p), e_v=np.where(live3, np.where(ev3, d_v, g_v), e_v),
             eh_p=np.where(live3, np.where(ev3, 0.0, gh_p), eh_p), eh_v=np.where(live3, np.where(ev3, 0.0, gh_v), eh_v),
             event=event.astype(np.int32), g_p=np.where(live3, g_p, 0.0), g_v=np.where(live3, g_v, 0.0),
             gh=np.where(np.broadcast_to(live[:, None, None], (S, n, 6)), np.concatenate([gh_p, gh_v], axis=-1), 0.0),
             n_p=np.where(l2, n_p, 0.0), n_v=np.where(l2, n_v, 0.0), err_p=np.where(l2, fb.norm3(d_p), 0.0), err_v=np.where(l2, fb.norm3(d_v), 0.0),
             true_p=np.where(l2, fb.norm3(g_p), 0.0), true_v=np.where(l2, fb.norm3(g_v), 0.0))
    v_rows, lT = v.copy(), np.array(lT_next, float)
    if reanchor:
        for kk in range(K):
            t = float(kk) * h
            sh = t * gh_v
            sh = gh_p + sh
            sl = slice(3 * kk, 3 * kk + 3)
            new_l = lT[:, sl, :n] + sh.transpose(0, 2, 1)
            lT[:, sl, :n] = np.where(ev3.transpose(0, 2, 1), new_l, lT[:, sl, :n])
            v_rows[..., sl] = np.where(ev3, v_rows[..., sl] + gh_v, v_rows[..., sl])
    o["v_rows"], o["lT_next"] = v_rows, lT
    return o


def new_log(S, n):
    log = {k: np.zeros((S, n), dtype=np.int32) for k in EST_INT}
    log.update({k: np.zeros((S, n)) for k in EST_MAX})
    return log


def log_column(log, k, c, live):
    """column k's result c of column() into dmpc_estimate_log's log (scenes `live` [S] only): ties stay with the smallest column"""
    for key, col, nn in (("err_p_max", "err_p_col", c["err_p"]), ("err_v_max", "err_v_col", c["err_v"]), ("dev_p_max", "dev_p_col", c["true_p"]),
                         ("dev_v_max", "dev_v_col", c["true_v"])):
        up = (nn > log[key]) & live[:, None]
        log[key][up], log[col][up] = nn[up], k


def loop(step, po, pf, K_T_max, error_tol, h, policy, meas, dist=None, l0=None, path=None, max_hold=None, alim=1.0, col0=0):
    """tests/feedback.py::loop with the measurement meas = dict(noise_p, noise_v, gain_p, gain_v, seed) between the true deviation and the
    rule's decision.  Returns what that returns (log: dmpc_feedback_log's dict, its dev_* the norms of gh), plus est: dmpc_estimate_log's dict."""
    import hold as ho
    import scripted as sc
    po, pf = np.asarray(po, float), np.asarray(pf, float)
    S, N = po.shape[:2]
    M = 0 if path is None else path.shape[1]
    mt = (meas["noise_p"], meas["noise_v"], meas["gain_p"], meas["gain_v"])
    l = np.stack([fb.init_rows(po[s], pf[s], h) for s in range(S)]) if l0 is None else np.array(l0, float)
    V, A = np.zeros((S, N, 45)), np.zeros((S, N, 45))
    xp, xv, xa = po.copy(), np.zeros_like(po), np.zeros_like(po)
    xh_p, xh_v, e_p, e_v = xp.copy(), xv.copy(), np.zeros_like(po), np.zeros_like(po)
    eh_p, eh_v = np.zeros_like(po), np.zeros_like(po)
    pk, vk, ak = (np.zeros((S, N, K_T_max, 3)) for _ in range(3))
    pk[:, :, 0] = po
    used, sst, done = np.full(S, K_T_max, dtype=np.int32), np.ones(S, dtype=np.int32), np.zeros(S, bool)
    log, est, events, columns, holds = fb.new_log(S, N), new_log(S, N), [], [], []
    fails, cnt = np.zeros((S, N), dtype=int), np.zeros((S, N), dtype=np.int32)
    for s in range(S):
        if mi.reached_goal(xp[s], pf[s], error_tol):
            done[s], used[s], sst[s] = True, 1, mi.REACHED
    for k in range(1, K_T_max):
        if done.all():
            break
        running = ~done
        table = l if not M else np.concatenate([l, np.stack([sc.window(path[s], k) for s in range(S)])], axis=1)
        out = step(table, xh_p, xh_v, xa, pf)
        p, v, a, st = out["p"].copy(), out["v"].copy(), out["a"].copy(), np.asarray(out["status"]).astype(np.int32)
        if max_hold is not None:
            fail = (st != 1) & running[:, None]
            fails = np.where(fail, fails + 1, np.where(running[:, None], 0, fails))
            held = fail & (fails <= max_hold)
            if held.any():
                p[held], v[held], a[held] = ho.shift_plan(l[held], V[held], A[held], h, alim)
                cnt[held] += 1
                holds += [(k, int(s), int(i)) for s, i in zip(*np.nonzero(held))]
            st = np.where(held, 1, st)
        ok = ((st & 1) == 1)[..., None]
        dp, dv = di.sample(h, S, N, col0 + k, **dist) if dist else (None, None)
        mp, mv = sample(S, N, k, meas["noise_p"], meas["noise_v"], meas["seed"], col0)
        lT = np.where(ok, p, l).transpose(0, 2, 1)
        c = column(policy[0], policy[1], policy[2], h, p, v, a, st, xp, xv, xa, xh_p, xh_v, e_p, e_v, eh_p, eh_v, lT, mt, mp, mv, dp, dv,
                   scene_done=done.astype(np.int32))
        r3 = running[:, None, None]
        l = np.where(r3, c["lT_next"].transpose(0, 2, 1), l)
        V = np.where(r3 & ok, c["v_rows"], V)
        A = np.where(r3 & ok, a, A)
        xp, xv, xa, xh_p, xh_v, e_p, e_v, eh_p, eh_v = (c[key] for key in ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v", "eh_p", "eh_v"))
        fb.log_column(log, k, c, running)
        log_column(est, k, c, running)
        columns.append((k, c["n_p"], c["n_v"], c["event"]))
        events += [(k, int(s), int(i)) for s, i in zip(*np.nonzero(c["event"]))]
        for s in np.nonzero(running)[0]:
            pk[s, :, k], vk[s, :, k], ak[s, :, k] = xp[s], xv[s], xa[s]
            bits = int(np.bitwise_or.reduce(st[s]))
            if bits & ~1:
                done[s], used[s], sst[s] = True, k + 1, bits
            elif mi.reached_goal(xp[s], pf[s], error_tol):
                done[s], used[s], sst[s] = True, k + 1, mi.REACHED
    sst = np.where(cnt.any(axis=1), sst | ho.HELD, sst).astype(np.int32)
    log.update(xh_p=xh_p, xh_v=xh_v, e_p=e_p, e_v=e_v)
    est.update(eh_p=eh_p, eh_v=eh_v)
    return dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, log=log, est=est, events=events, columns=columns, holds=holds, hold_count=cnt,
                plan_p=l, plan_v=V)


# ---- raw calls of the entries ---------------------------------------------------------------------------------------------------------------
def descriptor(noise_p=0.0, noise_v=0.0, gain_p=1.0, gain_v=1.0, seed=0):
    return _lib.DmpcMeasurement(int(seed), float(noise_p), float(noise_v), float(gain_p), float(gain_v))


def raw_set_measurement(d, ctx="own", null=False, **kw):
    """dmpc_set_measurement with exactly these fields (d None: no context object, ctx is passed as it is); returns (rc, message)"""
    L = _lib.load() if d is None else d._L
    m = descriptor(**kw)
    c = d._ctx if ctx == "own" else ctx
    rc = L.dmpc_set_measurement(c, None if null else C.byref(m))
    return rc, L.dmpc_last_error(c if d is not None else None).decode()


def raw_sample(S, n, k, **kw):
    """dmpc_measurement_sample; returns (rc, message, m_p, m_v)"""
    L = _lib.load()
    m = descriptor(**kw)
    mp, mv = np.full((max(S, 1), max(n, 1), 3), 7.0), np.full((max(S, 1), max(n, 1), 3), 7.0)
    rc = L.dmpc_measurement_sample(C.byref(m), int(S), int(n), int(k), _dp(mp), _dp(mv))
    return rc, L.dmpc_last_error(None).decode(), mp, mv


def raw_apply(policy, meas, h, k, p, v, a, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, eh_p, eh_v, lT_next, dist=None, scene_done=None, S=None, N=None,
              n=None):
    """dmpc_estimate_apply_host with policy = (trigger_p, trigger_v, reanchor) and meas = dict of descriptor()'s arguments, on copies of the
    arrays; S, N, n override the shapes.  Returns (rc, message, dict as column() returns it, without g, gh and the norms)."""
    L = _lib.load()
    p, a = _f(p), _f(a)
    o = {key: _f(t).copy() for key, t in dict(x_p=x_p, x_v=x_v, x_a=x_a, xh_p=xh_p, xh_v=xh_v, e_p=e_p, e_v=e_v, eh_p=eh_p, eh_v=eh_v, v_rows=v,
                                              lT_next=lT_next).items()}
    status = np.ascontiguousarray(status, dtype=np.int32)
    done = np.ascontiguousarray(scene_done, dtype=np.int32) if scene_done is not None else None
    o["event"] = np.zeros(status.shape, dtype=np.int32)
    desc = _lib.DmpcFeedback(float(policy[0]), float(policy[1]), int(policy[2]))
    m = descriptor(**meas)
    dd, keep = _lib._disturbance(**dist) if dist else (None, None)
    rc = L.dmpc_estimate_apply_host(C.byref(desc), C.byref(m), C.byref(dd) if dd is not None else None, float(h), p.shape[0] if S is None else S,
                                    o["lT_next"].shape[2] if N is None else N, p.shape[1] if n is None else n, int(k), _dp(p), _dp(o["v_rows"]), _dp(a),
                                    _ip(status), _dp(o["x_p"]), _dp(o["x_v"]), _dp(o["x_a"]), _dp(o["xh_p"]), _dp(o["xh_v"]), _dp(o["e_p"]), _dp(o["e_v"]),
                                    _dp(o["eh_p"]), _dp(o["eh_v"]), _dp(o["lT_next"]), _ip(o["event"]), _ip(done))
    del keep
    return rc, L.dmpc_last_error(None).decode(), o


def raw_log(d, S, n_cmd, ctx="own"):
    """dmpc_estimate_log with every output; returns (rc, message, dict)"""
    s, m = max(S, 1), max(n_cmd, 1)
    o = {k: np.zeros((s, m), dtype=np.int32) for k in EST_INT}
    o.update({k: np.zeros((s, m)) for k in EST_MAX})
    o.update({k: np.zeros((s, m, 3)) for k in ("eh_p", "eh_v")})
    c = d._ctx if ctx == "own" else ctx
    rc = d._L.dmpc_estimate_log(c, int(S), int(n_cmd), _dp(o["err_p_max"]), _ip(o["err_p_col"]), _dp(o["err_v_max"]), _ip(o["err_v_col"]),
                                _dp(o["dev_p_max"]), _ip(o["dev_p_col"]), _dp(o["dev_v_max"]), _ip(o["dev_v_col"]), _dp(o["eh_p"]), _dp(o["eh_v"]))
    return rc, d._L.dmpc_last_error(c).decode(), o


def random_belief(S, n, seed):
    """a random belief (eh_p, eh_v) [S,n,3]; some components are -0.0"""
    rng = np.random.default_rng(seed + 77)
    eh_p, eh_v = rng.uniform(-0.05, 0.05, (S, n, 3)), rng.uniform(-0.2, 0.2, (S, n, 3))
    for t in (eh_p, eh_v):
        flat = t.reshape(-1)
        flat[rng.integers(0, flat.size, max(1, flat.size // 7))] = -0.0
    return eh_p, eh_v
