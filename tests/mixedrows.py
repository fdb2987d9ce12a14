"""The fp32 scan and row builder of the mixed-precision mode (DMPC_PREC_MIXED: scan_body<.., TT = float, ..> in dmpc_kernels.hip) held to fp64
bounds: the reference, the bounds and the scenes.  Shared by tests/test_mixedrows_cpu.py and tests/test_gpu_mixed_rows.py; a plain helper, no GPU
here.

The rule.  The float scan reads the table through table_to_f32_kernel and the agent's position and velocity by a cast, so its INPUTS are l, x_p and
x_v rounded to float32.  The reference is the fp64 oracle on those rounded inputs (widened back to double).  What the float instantiation computes
may differ from that reference only by the roundings of its own expressions, counted below in units of u = 2^-24, and a DECISION (d < threshold)
may differ only where d lies inside the rounding band of the distance around its threshold: such an agent is `ambiguous`, skipped and counted
against a cap.  An FMA contraction replaces two roundings by one, so it only removes roundings from every count.

Counts (first order in u; every factor (1 + u)^n - 1 <= 1.0000004 n u for the n <= 24 used here, which the small constants below absorb):

  distance  dist = sqrt(dx dx + dy dy + ez ez), ez = dz e1z.  dx, dy, dz: one rounding each (differences of floats): u.  e1z = (float)(1/c): u,
            the product: u, so ez carries 3u.  A square doubles and rounds: 7u on ez ez, 3u on dx dx and dy dy; two additions of positive terms add
            one rounding each: <= 9u on d2.  The root halves and rounds once: 4.5u + u <= 8u.            |dist32 - dist| <= 8u dist
  row       xi = (dx, dy, dz e2z), e2z = (float)(1/c^2): u, 3u on the z component.                      |xi32 - xi| <= 4u |xi| per component
            Dense row G = -xi . Lambda[3 (kc - 1) : 3 kc, :] (expanded in fp64 on both sides):           |G32 - G| <= 4u sum_d |xi_d| |Lambda_d,col|
  rhs       b = -(pd (rmin - dist + (xi.p) / pd) - xi.a0), pd = dist, a0 = po + sh vo, sh = (float)(kc h).  With
            M = sum_d |xi_d| (|p_d| + |a0|_d) + pd (rmin + dist), where |a0|_d is taken as |po_d| + sh |vo_d| (equal to |a0_d| unless position and
            velocity term have opposite signs, never smaller: the roundings of a0 scale with its operands, not with their sum):
              xi.p   : products 4u + u, two additions 2u: 7u; the division by pd and the multiplication by pd cancel pd's own error and round
                       once each: 2u; the addition to (rmin - dist): u; the final subtraction: u.                       11u sum |xi_d p_d|
              pd(..) : rmin cast u, dist 8u, the subtraction u: <= 9u (rmin + dist); the addition u; pd's error 8u and the product u; the final
                       subtraction u.                                                                                  20u pd (rmin + dist)
              xi.a0  : sh = (float)(kc + 1) * (float)h: 2u; vo cast u, product u: 4u on sh vo; po cast u; the addition u: <= 6u |a0|; xi 4u, product
                       u, two additions 2u, the final subtraction u.                                                   14u sum |xi_d| |a0|_d
            C_B = 20 (the largest of the three).                                                        |b32 - b| <= C_B u M
  slack     coefficient pd = dist: 8u relative (1 and 1 / sqrt(EPS) of the all-neighbour variants: one cast, u).  repair's cost term (float)(term / pd):
            8u + u <= 10u relative.  Cost terms that are parameters or literals, and every lower bound (-0.05, -0.01, -(double)0.01f, -inf): exact.
  box slack order 2: xi.d = dist^2, so the row builder's lin_min - pd rmin = b - |xi|_1 hw(kc) and lin_max - pd rmin = b + |xi|_1 hw(kc) with
            hw = alim (kc h)^2 / 2, kc 1-based.  Their fp32 error: tau = C_B u M + 4u |xi|_1 hw.  The pruning keeps a margin MARG around zero.
"""
import functools

import numpy as np

from oracle import oracle as orc
import crowds as cr
import offconst as oc

U = 2.0 ** -24
K = 15
MARG = 2e-5                # dmpc_kernels.hip:520, `constexpr real MARG = std::is_same<TT, float>::value ? (real)2e-5 : (real)1e-9`
C_DIST, C_XI, C_B, C_COEF, C_RTERM = 8.0, 4.0, 20.0, 8.0, 10.0
AMBIGUOUS_CAP = 0.02       # of the agent-steps of a random cell
ORDER2 = ("bound", "bound2", "all3", "hard", "ondemand", "ellip", "softall", "repair", "cpp", "cpp2", "cpp1", "softall_c")
LADDER = ("bound", "bound2", "all3", "cpp", "cpp2")      # slack bounded below: a retry ladder with a certified start level
SLACK_FREE = ("hard", "ondemand", "ellip")               # the infeasibility certificate
f32 = np.float32


def round32(a):
    """what the float scan reads of a double array"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def rounded(sc):
    """a scene (l, x_p, x_v, x_a, pf) with the scan's inputs rounded (the scan reads no acceleration and no goal)"""
    l, xp, xv, xa, pf = sc
    return (round32(l), round32(xp), round32(xv), np.asarray(xa, float), np.asarray(pf, float))


# ------------------------------------------------------------------------------------------------------------------------------
# the scan, restated on dist[j, k]
# ------------------------------------------------------------------------------------------------------------------------------

def distances(l, n, c):
    """dist[j, k]: ellipsoidal distance of agent n to vehicle j at horizon step k (0-based), fp64; inf on j == n"""
    P = np.asarray(l, float).reshape(len(l), K, 3)
    d = P[n][None] - P
    dist = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2 + (d[..., 2] / c) ** 2)
    dist[n] = np.inf
    return dist


def cut_f(rmin):
    """dmpc.cpp:419: `_rmin - _collision_tol` in floats"""
    return float(f32(rmin) - f32(0.05))


def thresholds(variant, rmin, k_sel=None):
    """[(threshold, horizon steps it is tested at (0-based) or None: every step)] of a variant's scan.  The neighbour radius (3 rmin, the cpp radius of
    step k) is tested at ONE step only, the violating step k_sel the rows are built for (None: no rows)"""
    if variant == "hard":
        return [(1.0, None)]
    out = [(rmin, None)]
    if variant in ("bound", "bound2", "all3", "repair"):
        out.append((rmin - 0.05, [0]))
    if variant in ("cpp", "cpp2"):
        out.append((cut_f(rmin), [0]))
    if k_sel is not None and variant in ("bound", "bound2", "all3", "ondemand"):
        out.append((3.0 * rmin, [k_sel]))
    if k_sel is not None and variant in ("cpp", "cpp2"):
        out.append((cr.cpp_radius(rmin, k_sel + 1), [k_sel]))
    return out


def ambiguous(variant, rmin, dist):
    """some distance of the agent lies inside the rounding band of a threshold its variant uses: first the thresholds that decide the violating step,
    then -- the step being certain -- the neighbour radius at that step"""
    def near(ths):
        return any((np.abs((dist if steps is None else dist[:, steps]) - t) <= C_DIST * U * t).any() for t, steps in ths)
    if near(thresholds(variant, rmin)):
        return True
    rec = scan_record(variant, rmin, dist)
    return bool(rec["rows"]) and variant != "hard" and near(thresholds(variant, rmin, rec["viol_k"] - 1)[-1:])


def scan_record(variant, rmin, dist):
    """CheckCollSoftDMPC.m and the loops of solve*DMPC*.m around it, decided on dist[j, k] alone: dict(viol_k, coll, coll_flag, rows_exist,
    violation, rows [(j, ke, kc)]: neighbour, step the positions are evaluated at, step the row constrains, both 1-based, in the reference's order)"""
    N = dist.shape[0]
    rec = dict(viol_k=0, coll=False, coll_flag=False, rows_exist=False, violation=False, rows=[])
    if variant == "hard":
        rec["rows"] = [(j, k + 1, k + 1) for k in range(K) for j in range(N) if dist[j, k] < 1.0]
        rec["rows_exist"] = N > 1
        return rec
    cpp = variant in ("cpp", "cpp2")
    near = variant in ("bound", "bound2", "all3", "ondemand") or cpp
    coll_check = variant in ("bound", "bound2", "all3", "repair")
    skip_k1 = variant in ("bound2", "all3", "repair", "cpp2")
    for k in range(K):
        if not (dist[:, k] < rmin).any():
            continue
        if variant == "all3":
            rec["violation"] = True
        mind = dist[:, k].min()
        if cpp and k == 0 and mind < cut_f(rmin):
            rec["coll_flag"] = True
        if (coll_check and k == 0 and mind < rmin - 0.05) or (variant == "cpp1" and k == 0):
            rec["coll"], rec["viol_k"] = True, 1
            return rec
        if skip_k1 and k == 0:
            continue
        near_r = cr.cpp_radius(rmin, k + 1) if cpp else 3.0 * rmin
        sel = [j for j in range(N) if np.isfinite(dist[j, k]) and (dist[j, k] < near_r or not near)]
        rec.update(viol_k=k + 1, violation=True, rows_exist=True)
        if variant == "all3":
            ks = [k + 1, k + 2] if k == 1 else ([k, k + 1] if k == K - 1 else [k, k + 1, k + 2])
            rec["rows"] = [(j, kk, kk) for kk in ks for j in sel]
        else:
            kc = k if variant in ("bound2", "cpp2", "cpp1") else k + 1
            rec["rows"] = [(j, k + 1, kc) for j in sel]
        break
    return rec


# ------------------------------------------------------------------------------------------------------------------------------
# the reference rows of one agent, and their bounds
# ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lam(h):
    return orc.model_matrices(h, K)[0]


def expand(xi, kc, h):
    """dense rows of structured ones: G[r] = -xi_r . Lambda[3 (kc_r - 1) : 3 kc_r, :]  (kc 1-based), numpy fp64"""
    L = lam(h)
    xi, kc = np.asarray(xi, float).reshape(-1, 3), np.asarray(kc, int).reshape(-1)
    blocks = L.reshape(K, 3, 3 * K)[kc - 1] if len(kc) else np.zeros((0, 3, 3 * K))
    return -np.einsum("rd,rdc->rc", xi, blocks)


def slack_of(variant, term, dist, kc):
    """(coefficient, cost term, lower bound) per row in fp64, as the solver takes them (slack_cfg of the oracle; zeros for the slack-free variants)"""
    one, z = np.ones_like(dist), np.zeros_like(dist)
    if variant in ("bound",):
        return dist, term * one, -0.05 * one
    if variant in ("bound2", "all3"):
        return dist, term * one, -0.01 * one
    if variant in ("cpp", "cpp2"):
        return dist, term * one, -float(f32(0.01)) * one
    if variant == "repair":
        return dist, term / dist, -np.inf * one
    if variant == "softall":
        return one, -1e5 * one, -np.inf * one
    if variant == "cpp1":
        return one, -1e6 * one, -np.inf * one
    if variant == "softall_c":     # unit slack weight: eps = eps' / sqrt(EPS), EPS = 1e6 (K / k)^2, f_eps = -1e4 (K / k)^2
        rk = K / np.asarray(kc, float)
        isq = 1.0 / np.sqrt(1e6 * rk * rk)
        return isq, -1e4 * rk * rk * isq, -np.inf * one
    return z, z, z


def reference(variant, kw, sc, n):
    """The reference of agent n on the scene sc AS GIVEN (callers pass rounded(...) scenes): the oracle's rows_one, the scan record restated on
    dist, and per reference row the structured quantities and the bounds of the module's header."""
    l, xp, xv = (np.asarray(a, float) for a in sc[:3])
    rmin, c, h, alim = kw["rmin"], kw["c"], kw["h"], kw["alim"]
    prm = orc.make_params(variant, **kw)
    o = orc.rows_one(prm, l, n, xp[n], xv[n], max_rows=max(8, K * len(l)))
    dist = distances(l, n, c)
    rec = scan_record(variant, rmin, dist)
    rows = rec["rows"]
    R = len(rows)
    j = np.array([r[0] for r in rows], int)
    ke = np.array([r[1] for r in rows], int)
    kc = np.array([r[2] for r in rows], int)
    P = l.reshape(len(l), K, 3)
    p = P[n, ke - 1].reshape(R, 3)
    pj = P[j, ke - 1].reshape(R, 3)
    d = p - pj
    xi = d * np.array([1.0, 1.0, 1.0 / (c * c)])
    dr = dist[j, ke - 1] if R else np.zeros(0)
    sh = kc * h
    a0abs = np.abs(xp[n])[None] + sh[:, None] * np.abs(xv[n])[None]
    M = (np.abs(xi) * (np.abs(p) + a0abs)).sum(1) + dr * (rmin + dr)
    hw = alim * sh * sh / 2.0
    x1 = np.abs(xi).sum(1)
    coef, term, slb = slack_of(variant, kw["term"], dr, kc)
    return dict(oracle=o, dist=dist, rec=rec, ambiguous=ambiguous(variant, rmin, dist), n=n, j=j, ke=ke, kc=kc, p=p, pj=pj, xi=xi, d=dr, M=M, hw=hw,
                x1=x1, tau=C_B * U * M + C_XI * U * x1 * hw, coef=coef, term=term, slb=slb,
                b=o["b"] if o["nrows"] == R else np.full(R, np.nan), G=o["G"])


def ratios(variant, kw, ref, got):
    """err / bound of a set of rows `got` (dict(xi [R,3], b, coef, term, slb; dist where it can be seen)) against the reference of the same rows:
    dict(quantity -> worst ratio); asserts what must be exact.  A bound of zero admits an error of zero only."""
    def worst(err, bound):
        err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
        assert (err[bound == 0] == 0).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, err / bound, 0.0)
        return float(r.max(initial=0.0))
    out = {}
    if "dist" in got:
        out["dist"] = worst(got["dist"] - ref["d"], C_DIST * U * ref["d"])
    out["xi"] = worst(got["xi"] - ref["xi"], C_XI * U * np.abs(ref["xi"]))
    blocks = np.abs(lam(kw["h"]).reshape(K, 3, 3 * K)[ref["kc"] - 1])
    out["G"] = worst(expand(got["xi"], ref["kc"], kw["h"]) - ref["G"], C_XI * U * np.einsum("rd,rdc->rc", np.abs(ref["xi"]), blocks) + 1e-15)
    out["b"] = worst(got["b"] - ref["b"], C_B * U * ref["M"])
    if variant not in SLACK_FREE + ("hard",):
        unit = variant in ("softall", "cpp1")
        out["coef"] = worst(got["coef"] - ref["coef"], (0.0 if unit else (U if variant == "softall_c" else C_COEF * U)) * np.abs(ref["coef"]))
        rel = {"repair": C_RTERM * U, "softall_c": U}.get(variant, 0.0)
        out["term"] = worst(got["term"] - ref["term"], rel * np.abs(ref["term"]))
        assert np.array_equal(got["slb"], ref["slb"]), (variant, got["slb"][:4], ref["slb"][:4])
    return out


def emulate(variant, kw, sc, ref, fused):
    """The row builder's expressions (emit_row / build_rows in dmpc_kernels.hip) for the reference's rows in numpy float32: left to right, or
    `fused` -- every a * b + c formed in float64 (the product of two floats is exact there) and rounded once.  sc: the rounded scene."""
    def fma(a, b, cc):
        if fused:
            return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(cc, np.float64)).astype(f32)
        return (a * b).astype(f32) + cc
    l, xp, xv = sc[:3]
    n, kc = ref["n"], ref["kc"]
    rmin, e1z, e2z, h_ = f32(kw["rmin"]), f32(1.0 / kw["c"]), f32(1.0 / (kw["c"] * kw["c"])), f32(kw["h"])
    p, pj = ref["p"].astype(f32), ref["pj"].astype(f32)
    po, vo = xp[n].astype(f32), xv[n].astype(f32)
    dx, dy, dz = (p[:, i] - pj[:, i] for i in range(3))
    ez = dz * e1z
    dist = np.sqrt(fma(ez, ez, fma(dy, dy, dx * dx)))
    x = [dx, dy, dz * e2z]
    sh = kc.astype(f32) * h_
    a0 = [fma(sh, np.broadcast_to(vo[i], sh.shape), po[i]) for i in range(3)]
    s = fma(x[2], p[:, 2], fma(x[1], p[:, 1], x[0] * p[:, 0]))
    t = fma(x[2], a0[2], fma(x[1], a0[1], x[0] * a0[0]))
    inner = (rmin - dist) + s / dist
    rr = fma(dist, inner, -t) if fused else dist * inner - t
    _, term, slb = slack_of(variant, kw["term"], dist.astype(np.float64), kc)
    coef = ref["coef"] if variant in ("softall", "cpp1") else (ref["coef"].astype(f32) if variant == "softall_c" else dist)
    if variant == "repair":
        term = (kw["term"] / dist.astype(np.float64)).astype(f32)
    elif variant == "softall_c":
        term = ref["term"].astype(f32)
    return dict(dist=dist.astype(np.float64), xi=np.stack(x, 1).astype(np.float64), b=-rr.astype(np.float64), coef=np.asarray(coef, np.float64),
                term=np.asarray(term, np.float64), slb=slb)


def ladder_level(ref, delta):
    """L(delta) = max over the rows of min{t : b + |xi|_1 hw + delta >= dist slb 2^t} (0 without rows)"""
    lev = 0
    for b, x1, hw, d, slb, dl in zip(ref["b"], ref["x1"], ref["hw"], ref["d"], ref["slb"], np.broadcast_to(delta, ref["b"].shape)):
        t = 0
        while t < 40 and not (b + x1 * hw + dl >= d * slb * 2.0 ** t):
            t += 1
        lev = max(lev, t)
    return lev


# ------------------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------------------

CELLS = {"base@origin": ("base", oc.ORIGIN, oc.N, oc.BOX), "rmin=0.6,c=3@moved": ("rmin=0.6,c=3", oc.MOVED, oc.N, oc.BOX),
         "base,n=70": ("base", oc.ORIGIN, 70, oc.BOX_FILTER)}
CELL_SEEDS = {}            # (variant, cell) -> another seed, for a cell that broke the ambiguity cap at the set's own (none did)
COLUMNS = (1, 2, 3, 4)     # steps of the oracle-taught closed loop (step 0 starts from initDMPC's straight lines at rest)


@functools.lru_cache(maxsize=None)
def cell_raw(variant, name):
    """(kw, [scene of every column]) of a random cell: the set's scene, an oracle-taught closed loop of the variant"""
    setname, offset, n, box = CELLS[name]
    kw, po, pf = oc.scene(setname, n=n, offset=offset, box=box, seed=CELL_SEEDS.get((variant, name)))
    loop = oc.closed_loop(variant, kw, po, pf, steps=max(COLUMNS) + 1)
    return kw, [loop[k][1] for k in COLUMNS]


def cell(variant, name):
    """the same with the scan's inputs rounded"""
    kw, cols = cell_raw(variant, name)
    return kw, [rounded(sc) for sc in cols]


@functools.lru_cache(maxsize=None)
def cell_refs(variant, name):
    """(kw, [(rounded scene, [reference of every agent])] per column)"""
    kw, cols = cell(variant, name)
    return kw, [(sc, [reference(variant, kw, sc, n) for n in range(len(sc[0]))]) for sc in cols]


TIE_VARIANT = dict(rmin="bound", hard1="hard", cut="bound", cpp="cpp", cppcut="cpp")
TIE_VARIANT["3rmin"] = "bound"
TIE_M = (-64, -16, -2, -1, 0, 1, 2, 16, 64)


def tie_threshold32(kind, rmin, kc=5):
    """the threshold as the float scan forms it: rmin cast; `3.0 * rmin` a double product rounded to the float argument; the literal 1; the cut of
    the MATLAB variants `rmin - 0.05`, a float minus a double literal, compared in double; the cpp radius and cut in float arithmetic"""
    r = float(f32(rmin))
    return {"rmin": r, "3rmin": float(f32(3.0 * r)), "hard1": 1.0, "cut": r - 0.05, "cpp": cr.cpp_radius(rmin, kc), "cppcut": cut_f(rmin)}[kind]


def step_outcome(out, n):
    """what a step decides for agent n: (status, first violating step, reference row count) -- of the oracle's step or of Dmpc.step_batch"""
    return (int(out["status"][n]), int(out["info"][n][orc.I_VIOLK]), int(out["info"][n][orc.I_NROWS if "obj" in out else 1]))


def tie_sweep(kind, axis, c):
    """(variant, kw, [(m, rounded scene)]) of a threshold sweep: crowds.tie_scene at d = t (1 + m u)"""
    kw = cr.solver_kw(c=c)
    t = tie_threshold32(kind, kw["rmin"])
    return TIE_VARIANT[kind], kw, [(m, rounded(cr.tie_scene(kind, t * (1.0 + m * U), axis, c=c))) for m in TIE_M]


BOX_KC = 2
BOX_STEPS = (-4.0, -0.25, 0.25, 4.0)       # in tau about the threshold


def box_scene(d, kc=BOX_KC):
    """two agents in the style of crowds.tie_scene: the probe at rest with its plan at P0, the neighbour at scaled distance d along x from step kc
    (1-based) on and 2 m away before.  The probe's row on step kc has xi = (-d, 0, 0), p = a0 = 0: b + |xi|_1 hw = d (hw - (rmin - d)) exactly."""
    l = np.zeros((2, K, 3))
    l[0] = cr.P0
    steps = np.arange(1, K + 1)[:, None]
    l[1] = np.where(steps >= kc, cr.P0 + np.array([d, 0.0, 0.0]), cr.P0 + np.array([2.0, 0.0, 0.0]))
    x_p = l[:, 0].copy()
    z = np.zeros_like(x_p)
    pf = x_p.copy()
    pf[0] = cr.P0 + np.array([1.0, 0.0, 0.0])
    return l.reshape(2, 3 * K), x_p, z, z.copy(), pf


def box_sweep(variant):
    """(kw, d*, tau, [(s, rounded scene)]): `hard` -- the certificate's threshold b + |xi|_1 hw = -MARG, i.e. d = rmin - hw - MARG / d; `bound` -- the
    ladder's, b + |xi|_1 hw + MARG = dist slb at level 0, i.e. rmin - d - hw = 0.05 + MARG / d.  The scenes sit at b + |xi|_1 hw + MARG - d slb =
    s tau for s in BOX_STEPS (tau taken at the threshold: it changes by a part in 10^5 over the sweep)."""
    kw = cr.solver_kw()
    rmin, hw = kw["rmin"], kw["alim"] * (BOX_KC * kw["h"]) ** 2 / 2.0
    q = rmin - hw - (0.05 if variant == "bound" else 0.0)      # d^2 - q d + MARG - s tau = 0
    root = lambda rhs: (q + np.sqrt(q * q - 4.0 * (MARG - rhs))) / 2.0
    d0 = root(0.0)
    tau = C_B * U * d0 * (rmin + d0) + C_XI * U * d0 * hw
    return kw, d0, tau, [(s, rounded(box_scene(root(s * tau)))) for s in BOX_STEPS]
