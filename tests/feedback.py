"""Test helper: event-triggered feedback (dmpc_set_feedback) -- the rule of include/dmpc_hip.h restated in numpy, every operation an fp64
operation rounded on its own (numpy fuses nothing), one column (column) and the closed loop a caller could write on the host over an MPC step
(loop), and raw ctypes calls of the entries.  The device, dmpc_feedback_apply_host and this file must agree bit for bit.

There is no reference counterpart.  Per commanded agent: the true state x, the planning state xh the solver starts from, the tracking error e.
Column 0: xh = x, e = 0.  Column k >= 1: see column()."""
import ctypes as C

import numpy as np

import disturb as di
import mission as mi
from multiagent_planning_amd import _lib
from obstacles import _dp, _ip, _f   # noqa: F401

K = 15
INF = float("inf")
LOG_INT = ("event_count", "event_first", "event_last", "dev_p_col", "dev_v_col")
LOG = LOG_INT + ("dev_p_max", "dev_v_max", "xh_p", "xh_v", "e_p", "e_v")


def norm3(g):
    """sqrt((gx*gx + gy*gy) + gz*gz) over the last axis"""
    xx, yy, zz = g[..., 0] * g[..., 0], g[..., 1] * g[..., 1], g[..., 2] * g[..., 2]
    s = xx + yy
    return np.sqrt(s + zz)


def column(trigger_p, trigger_v, reanchor, h, p, v, a, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, lT_next, dp=None, dv=None, scene_done=None):
    """One column of the rule.  p, v, a [S,n,45], status [S,n], x_p .. e_v [S,n,3], lT_next [S,45,N] (N >= n), dp, dv [S,n,3] or None (no
    disturbance), scene_done [S] or None.  Nothing is changed in place; returns dict(x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, v_rows, lT_next, event
    [S,n] int32, g_p, g_v [S,n,3], n_p, n_v [S,n]) -- for a finished scene the inputs, event 0, g = n = 0."""
    p, v, a = (np.asarray(t, float) for t in (p, v, a))
    x_p, x_v, x_a, xh_p, xh_v, e_p, e_v = (np.asarray(t, float) for t in (x_p, x_v, x_a, xh_p, xh_v, e_p, e_v))
    S, n = p.shape[:2]
    dp = np.zeros((S, n, 3)) if dp is None else dp
    dv = np.zeros((S, n, 3)) if dv is None else dv
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
    n_p, n_v = norm3(g_p), norm3(g_v)
    event = ((n_p > trigger_p) | (n_v > trigger_v)) & live[:, None]
    ev3 = np.broadcast_to(event[..., None], (S, n, 3))
    o = dict(x_p=np.where(live3, nx_p, x_p), x_v=np.where(live3, nx_v, x_v), x_a=np.where(live3, nx_a, x_a),
             xh_p=np.where(live3, np.where(ev3, nx_p, q_p), xh_p), xh_v=np.where(live3, np.where(ev3, nx_v, q_v), xh_v),
             e_p=np.where(live3, np.where(ev3, 0.0, g_p), e_p), e_v=np.where(live3, np.where(ev3, 0.0, g_v), e_v),
             event=event.astype(np.int32), g_p=np.where(live3, g_p, 0.0), g_v=np.where(live3, g_v, 0.0),
             n_p=np.where(live[:, None], n_p, 0.0), n_v=np.where(live[:, None], n_v, 0.0))
    v_rows, lT = v.copy(), np.array(lT_next, float)
    if reanchor:
        for kk in range(K):
            t = float(kk) * h
            sh = t * g_v
            sh = g_p + sh
            sl = slice(3 * kk, 3 * kk + 3)
            new_l = lT[:, sl, :n] + sh.transpose(0, 2, 1)
            lT[:, sl, :n] = np.where(ev3.transpose(0, 2, 1), new_l, lT[:, sl, :n])
            v_rows[..., sl] = np.where(ev3, v_rows[..., sl] + g_v, v_rows[..., sl])
    o["v_rows"], o["lT_next"] = v_rows, lT
    return o


def new_log(S, n):
    log = {k: np.zeros((S, n), dtype=np.int32) for k in LOG_INT}
    log["event_first"][:] = -1
    log["event_last"][:] = -1
    log["dev_p_max"], log["dev_v_max"] = np.zeros((S, n)), np.zeros((S, n))
    return log


def log_column(log, k, c, live):
    """column k's result c of column() into the log (scenes `live` [S] only)"""
    hit = (c["event"] != 0) & live[:, None]
    log["event_count"][hit] += 1
    log["event_first"][hit & (log["event_first"] < 0)] = k
    log["event_last"][hit] = k
    for key, col, nn in (("dev_p_max", "dev_p_col", c["n_p"]), ("dev_v_max", "dev_v_col", c["n_v"])):
        up = (nn > log[key]) & live[:, None]
        log[key][up], log[col][up] = nn[up], k


def loop(step, po, pf, K_T_max, error_tol, h, fb, dist=None, l0=None, path=None, max_hold=None, alim=1.0):
    """dmpc_transition's loop with a policy fb = (trigger_p, trigger_v, reanchor) and the disturbance `dist` (a dict of tests/disturb.py::sample's
    arguments, or None), as a host loop over a batch.  po, pf [S,nc,3]; path [S,M,P,3] or None: scripted vehicles behind the commanded agents;
    l0: the commanded rows of the first table (None: init_rows).  step(l [S,nc+M,45], xp, xv, xa, pf [S,nc,3]) -> dict(p, v, a [S,nc,45], status
    [S,nc]) is one MPC step FROM THE PLANNING STATE.  max_hold (None: no hold): the hold rule of tests/hold.py between the solve and the rule --
    the previous plan is the table's column and the v rows AS RE-ANCHORED.  Returns dict(pk, vk, ak [S,nc,K_T_max,3], K_T_used, scene_status [S],
    log: the dict of dmpc_feedback_log, events: [(k, s, i)], columns: [(k, n_p, n_v, event [S,nc])] of every column that ran, holds: [(k, s, i)],
    hold_count [S,nc], plan_p, plan_v [S,nc,45]: the (re-anchored) plan of the last step of every scene)."""
    import hold as ho
    import scripted as sc
    po, pf = np.asarray(po, float), np.asarray(pf, float)
    S, N = po.shape[:2]
    M = 0 if path is None else path.shape[1]
    l = np.stack([init_rows(po[s], pf[s], h) for s in range(S)]) if l0 is None else np.array(l0, float)
    V, A = np.zeros((S, N, 45)), np.zeros((S, N, 45))
    xp, xv, xa = po.copy(), np.zeros_like(po), np.zeros_like(po)
    xh_p, xh_v, e_p, e_v = xp.copy(), xv.copy(), np.zeros_like(po), np.zeros_like(po)
    pk, vk, ak = (np.zeros((S, N, K_T_max, 3)) for _ in range(3))
    pk[:, :, 0] = po
    used, sst, done = np.full(S, K_T_max, dtype=np.int32), np.ones(S, dtype=np.int32), np.zeros(S, bool)
    log, events, columns, holds = new_log(S, N), [], [], []
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
        dp, dv = di.sample(h, S, N, k, **dist) if dist else (None, None)
        lT = np.where(ok, p, l).transpose(0, 2, 1)
        c = column(fb[0], fb[1], fb[2], h, p, v, a, st, xp, xv, xa, xh_p, xh_v, e_p, e_v, lT, dp, dv, scene_done=done.astype(np.int32))
        r3 = running[:, None, None]
        l = np.where(r3, c["lT_next"].transpose(0, 2, 1), l)
        V = np.where(r3 & ok, c["v_rows"], V)
        A = np.where(r3 & ok, a, A)
        xp, xv, xa, xh_p, xh_v, e_p, e_v = (c[key] for key in ("x_p", "x_v", "x_a", "xh_p", "xh_v", "e_p", "e_v"))
        log_column(log, k, c, running)
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
    return dict(pk=pk, vk=vk, ak=ak, K_T_used=used, scene_status=sst, log=log, events=events, columns=columns, holds=holds, hold_count=cnt, plan_p=l,
                plan_v=V)


def init_rows(po, pf, h):
    """initDMPC's table rows [N,45] as init_rows_kernel writes them: po + 1 * t * (pf - po) / 10, t = kk * h"""
    diff = pf - po
    out = np.empty((po.shape[0], 45))
    for kk in range(K):
        t = float(kk) * h
        out[:, 3 * kk:3 * kk + 3] = po + 1 * t * diff / 10
    return out


def oracle_batch_step(orc, prm):
    """loop's step over oracle.step, scene by scene"""
    def step(l, xp, xv, xa, pf):
        outs = [orc.step(prm, l[s], xp[s], xv[s], xa[s], pf[s]) for s in range(l.shape[0])]
        return {key: np.stack([o[key] for o in outs]) for key in ("p", "v", "a", "status")}
    return step


def device_batch_step(d):
    """loop's step over dmpc_step_batch (every vehicle commanded) / dmpc_step_batch_cmd (the table has more rows than there are states)"""
    import obstacles as ob

    def step(l, xp, xv, xa, pf):
        if l.shape[1] == xp.shape[1]:
            o = d.step_batch(np.ascontiguousarray(l), np.ascontiguousarray(xp), np.ascontiguousarray(xv), np.ascontiguousarray(xa), pf)
        else:
            rc, o = ob.raw_step_batch_cmd(d, l, xp, xv, xa, pf, xp.shape[1])
            assert rc == 0
        return {key: o[key] for key in ("p", "v", "a", "status")}
    return step


# ---- raw calls of the entries ---------------------------------------------------------------------------------------------------------------
def raw_set_feedback(d, trigger_p, trigger_v, reanchor, ctx="own", null=False):
    """dmpc_set_feedback with exactly these fields; returns (rc, message)"""
    L = _lib.load() if d is None else d._L
    fb = _lib.DmpcFeedback(float(trigger_p), float(trigger_v), int(reanchor))
    rc = L.dmpc_set_feedback(d._ctx if ctx == "own" else ctx, None if null else C.byref(fb))
    return rc, L.dmpc_last_error(d._ctx if (ctx == "own" and d is not None) else None).decode()


def raw_apply(fb, h, k, p, v, a, status, x_p, x_v, x_a, xh_p, xh_v, e_p, e_v, lT_next, dist=None, scene_done=None, S=None, N=None, n=None):
    """dmpc_feedback_apply_host with fb = (trigger_p, trigger_v, reanchor) on copies of the arrays; S, N, n override the shapes.  Returns (rc,
    message, dict as column() returns it, without g and n)."""
    L = _lib.load()
    p, a = _f(p), _f(a)
    o = {key: _f(t).copy() for key, t in dict(x_p=x_p, x_v=x_v, x_a=x_a, xh_p=xh_p, xh_v=xh_v, e_p=e_p, e_v=e_v, v_rows=v, lT_next=lT_next).items()}
    status = np.ascontiguousarray(status, dtype=np.int32)
    done = np.ascontiguousarray(scene_done, dtype=np.int32) if scene_done is not None else None
    o["event"] = np.zeros(status.shape, dtype=np.int32)
    desc = _lib.DmpcFeedback(float(fb[0]), float(fb[1]), int(fb[2]))
    dd, keep = _lib._disturbance(**dist) if dist else (None, None)
    rc = L.dmpc_feedback_apply_host(C.byref(desc), C.byref(dd) if dd is not None else None, float(h), p.shape[0] if S is None else S,
                                    o["lT_next"].shape[2] if N is None else N, p.shape[1] if n is None else n, int(k), _dp(p), _dp(o["v_rows"]), _dp(a),
                                    _ip(status), _dp(o["x_p"]), _dp(o["x_v"]), _dp(o["x_a"]), _dp(o["xh_p"]), _dp(o["xh_v"]), _dp(o["e_p"]), _dp(o["e_v"]),
                                    _dp(o["lT_next"]), _ip(o["event"]), _ip(done))
    del keep
    return rc, L.dmpc_last_error(None).decode(), o


def raw_log(d, S, n_cmd, ctx="own"):
    """dmpc_feedback_log with every output; returns (rc, message, dict)"""
    s, m = max(S, 1), max(n_cmd, 1)
    o = {k: np.zeros((s, m), dtype=np.int32) for k in LOG_INT}
    o.update(dev_p_max=np.zeros((s, m)), dev_v_max=np.zeros((s, m)))
    o.update({k: np.zeros((s, m, 3)) for k in ("xh_p", "xh_v", "e_p", "e_v")})
    c = d._ctx if ctx == "own" else ctx
    rc = d._L.dmpc_feedback_log(c, int(S), int(n_cmd), _ip(o["event_count"]), _ip(o["event_first"]), _ip(o["event_last"]), _dp(o["dev_p_max"]),
                                _ip(o["dev_p_col"]), _dp(o["dev_v_max"]), _ip(o["dev_v_col"]), _dp(o["xh_p"]), _dp(o["xh_v"]), _dp(o["e_p"]), _dp(o["e_v"]))
    return rc, d._L.dmpc_last_error(c).decode(), o


def random_column(S, n, N, seed, e_zero=False):
    """a random column's inputs: dict(p, v, a [S,n,45], status [S,n] (solved, failed and held-like words mixed), x_p .. e_v [S,n,3], lT_next
    [S,45,N]); some components are -0.0"""
    rng = np.random.default_rng(seed)
    c = dict(p=rng.uniform(-2, 2, (S, n, 45)), v=rng.uniform(-1, 1, (S, n, 45)), a=rng.uniform(-1, 1, (S, n, 45)),
             status=rng.choice(np.array([1, 1, 1, 2, 4, 1 | 64], dtype=np.int32), (S, n)),
             x_p=rng.uniform(-2, 2, (S, n, 3)), x_v=rng.uniform(-1, 1, (S, n, 3)), x_a=rng.uniform(-1, 1, (S, n, 3)),
             xh_p=rng.uniform(-2, 2, (S, n, 3)), xh_v=rng.uniform(-1, 1, (S, n, 3)),
             e_p=rng.uniform(-0.05, 0.05, (S, n, 3)), e_v=rng.uniform(-0.2, 0.2, (S, n, 3)), lT_next=rng.uniform(-2, 2, (S, 45, N)))
    if e_zero:
        c["e_p"][:], c["e_v"][:] = 0.0, 0.0
    for key in ("e_p", "e_v", "xh_p", "p"):
        flat = c[key].reshape(-1)
        flat[rng.integers(0, flat.size, max(1, flat.size // 7))] = -0.0
    return c
