// dmpc_kernels.hip -- gfx950 (MI355X, CDNA4) device code of the DMPC per-agent horizon-QP hot path.
//
// One 64-lane wavefront (= one workgroup) owns one agent for one MPC step:
//   scan   (a5)  CheckCollSoftDMPC.m:7-15 / CheckCollEllipDMPC.m:4-11 : coalesced reads of the
//                transposed prediction table lT[G][S][3K][C], lane = neighbour
//   rows   (a6)  CollConstrSoftDMPC.m:16-28 (+2/Hard/OnDemand/Ellip variants): compacted into LDS in
//                structured form (xi, kc, rhs, slack descriptor) -- 5..9 numbers per row, never dense
//   solve  (a7)  the QP of solveSoftDMPCbound.m:43-103 (and variants) by a dual active-set
//                (Goldfarb-Idnani) method in Schur-complement form: the Hessian is input-independent
//                and per-axis (H = H1 (x) I3), so H1^-1, H1^-1 L', L H1^-1 L' (15x15 each) are
//                precomputed per cost case and staged in LDS; the only per-agent matrix is the
//                upper-triangular inverse Cholesky factor T of the active-set Schur matrix
//                (T T' = (N' H^-1 N)^-1), kept in LDS and updated by column append / Givens deletes.
//                Slack variables (solveSoftDMPCbound.m:60-88) are explicit but their eps<=0 pins are
//                instantiated lazily, so the working set only holds what is really active.
//                (dmpc_solve.hip, included below)
//   prop   (a9)  propStatedmpc.m:3-4, is_inbounds.m:2-5 (a10), outputs + next table chunk.
//
// All arithmetic is fp64 (the reference is MATLAB double).  The data path has no atomics: every reduction is a
// fixed butterfly, so results are bit-reproducible and independent of how agents are sharded.  (Atomics only
// serve scheduling: the queue head of the persistent waves, the tier-2 list, the histograms of order_kernel.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "dmpc_device.h"

namespace dmpc {

// --------------------------------------------------------------------------------------------
// wave64 helpers
// --------------------------------------------------------------------------------------------
// The workgroup is ONE wavefront and the LDS executes a wave's DS instructions in issue order, so lanes
// exchanging data through LDS need no hardware barrier or counter wait -- only the compiler must not
// reorder the accesses.  (A __syncthreads() here would also drain outstanding global loads.)
#define LSYNC() asm volatile("" ::: "memory")

__device__ __forceinline__ double readlane_d(double v, int l /*uniform*/)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int readlane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
// wave-uniform by construction, not by what the compiler can see (a value read from LDS or global memory at a uniform address, the result
// of an out-of-line function): say so -- everything derived from it is then scalar, branches on it are scalar branches
#define UNI(x_) __builtin_amdgcn_readfirstlane(x_)
__device__ __forceinline__ bool uni_b(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }

// Wave-wide reductions on the VALU with DPP row shifts / row broadcasts (gfx9 scan idiom): six
// steps, no LDS crossbar traffic (a ds_bpermute butterfly costs ~10x more here).  Lane 63 ends up
// with the total, which is then broadcast through an SGPR.  Fixed order => bit-reproducible.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_d(double ident, double v)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(ident), __double2loint(v), CTRL, ROWMASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(ident), __double2hiint(v), CTRL, ROWMASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
#define DMPC_WAVE_REDUCE(NAME, IDENT, OP)                                     \
    __device__ __forceinline__ double NAME(double v)                          \
    {                                                                         \
        const double id = IDENT;                                              \
        v = OP(v, dpp_d<0x111, 0xf>(id, v)); /* row_shr:1 */                  \
        v = OP(v, dpp_d<0x112, 0xf>(id, v)); /* row_shr:2 */                  \
        v = OP(v, dpp_d<0x114, 0xf>(id, v)); /* row_shr:4 */                  \
        v = OP(v, dpp_d<0x118, 0xf>(id, v)); /* row_shr:8 */                  \
        v = OP(v, dpp_d<0x142, 0xa>(id, v)); /* row_bcast:15 -> rows 1,3 */   \
        v = OP(v, dpp_d<0x143, 0xc>(id, v)); /* row_bcast:31 -> rows 2,3 */   \
        return readlane_d(v, 63);                                             \
    }
__device__ __forceinline__ double op_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double op_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double op_add(double a, double b) { return a + b; }
DMPC_WAVE_REDUCE(wave_max, -INFINITY, op_max)
DMPC_WAVE_REDUCE(wave_min, INFINITY, op_min)

// value of lane + N of the same 16-lane row (row_shl DPP); lanes whose source falls off the row keep their own value
template <int N>
__device__ __forceinline__ double dpp_row_shl(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x100 + N, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x100 + N, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int N>
__device__ __forceinline__ float dpp_row_shl(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x100 + N, 0xf, 0xf, false));
}
DMPC_WAVE_REDUCE(wave_sum, 0.0, op_add)
__device__ __forceinline__ unsigned wave_or(unsigned v)
{
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane)
{
    return __popcll(mask & ((1ull << lane) - 1ull));
}

// Division of a per-lane index (< 2^31) by a wave-uniform divisor d: product with the double reciprocal (off by at most
// one), one correction step in either direction makes it exact.  Branch-free.
struct UDiv {
    int d;
    double inv;
    __device__ __forceinline__ explicit UDiv(unsigned d_) : d(d_ ? (int)d_ : 1), inv(1.0 / (double)(d_ ? d_ : 1u)) {}
    __device__ __forceinline__ void divmod(unsigned e, int &q, int &rem) const
    {
        int qq = (int)((double)e * inv);
        int rr = (int)e - qq * d;
        const int up = rr >= d ? 1 : 0, dn = rr < 0 ? 1 : 0;
        q = qq + up - dn;
        rem = rr - (up - dn) * d;
    }
};

__device__ __forceinline__ double sel3(const double *v, int ax) { return ax == 0 ? v[0] : (ax == 1 ? v[1] : v[2]); }

// constraint types
#ifndef SCAN_WAVES_PER_SIMD
#define SCAN_WAVES_PER_SIMD 4
#endif
#ifndef SCAN_WAVES_PER_WG
#define SCAN_WAVES_PER_WG 4
#endif
#ifndef QUEUE_CHUNK
#define QUEUE_CHUNK 2   // measured on the headline workload (M solves/s), tickets claimed at the end of a solve (round 3): 1: 48.9, 2: 52.0, 3: 51.4, 4: 50.5
#endif
#ifndef QUEUE_T1
#define QUEUE_T1 1
#endif
#ifndef QUEUE_T3
#define QUEUE_T3 2   // single-position tickets for the last 2 x #waves positions (1: 52.0, 2: 52.3, 4: 50.9, 8: 49.3 M solves/s)
#endif
#ifndef SOLVE_WAVES_PER_SIMD
#define SOLVE_WAVES_PER_SIMD 2
#endif
enum { TY_BOXHI = 0, TY_BOXLO = 1, TY_POSHI = 2, TY_POSLO = 3, TY_COLL = 4, TY_SLKU = 5, TY_SLKL = 6 };
// row flags
enum { RF_COLL = 1, RF_SLKU = 2, RF_SLKL = 4, RF_LIVE = 8 };

// what the scan phase addresses: its LDS vectors and the per-agent slice of the global row scratch
struct Lds {
    double *w_s, *own_s;
    double *r_xi;   // nrmax x 3
    double *r_b;
    double *r_sd, *r_st, *r_slb;  // soft variants only
    int *r_kc;
};

struct Agent {   // wave-uniform agent data
    double po[3], vo[3], ao[3], pf[3];
};

// ---- arithmetic shared by the scan's unconstrained exit and the solver (explicit contractions: both kernels must produce the
// ---- same bits for an agent whichever of them finishes it)
// cost case of solveSoftDMPCbound.m:43-58 (0 far, 1 near, 2 collision rows)
__device__ __forceinline__ int cost_case(int var, double d0, double d1, double d2 /* po - pf */, bool rows_exist)
{
    if (var == VAR_SCP) return rows_exist ? 2 : 0;   // solveDMPC.m:38-48: `isempty(Ain_total)` alone decides (Q = 1000, S = 10, or Q1, S1)
    const double dn = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0)));
    const bool far = (var == VAR_ELLIP) ? (dn > 1.0) : (dn >= 1.0);
    if (!rows_exist && far) return 0;
    if (!rows_exist && dn < 1.0) return 1;
    return 2;
}
// g = pf - (po + K h vo): what is left to the goal after coasting through the horizon (per axis)
__device__ __forceinline__ double goal_gap(double pf, double po, double vo, double h) { return pf - fma((double)K * h, vo, po); }
// a_unc(k) or w_unc(k) = 2 q g T1 + 2 s ao T2 with the two table entries of the component
__device__ __forceinline__ double unc_entry(double qw, double sw, double gax, double ao, double t1, double t2)
{
    return fma(2.0 * qw * gax, t1, (2.0 * sw * ao) * t2);
}
// A_initp(k,:) [po;vo] of component (k, axis)
__device__ __forceinline__ double init_pos(int k, double h, double vo, double po) { return fma((double)(k + 1) * h, vo, po); }
// v(k) = h sum_{kk<=k} a(kk) + vo   (propStatedmpc.m:4); a_s: the stacked accelerations in LDS
__device__ __forceinline__ double vel_out(const double *a_s, int k_l, int ax_l, double h, double vo)
{
    double sv = 0.0;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) { const double ak = a_s[3 * kk + ax_l]; sv += (kk <= k_l) ? ak : 0.0; }
    return fma(h, sv, vo);
}

// The kernel's StepParams argument as it lies in the kernel-argument segment (first and only argument of every solve kernel), through a
// pointer in the CONSTANT address space: fields read through it are scalar loads (s_load, the scalar cache) issued where they are used.
// The empty asm keeps the compiler from recognising the pointer and hoisting the loads -- values kept in SGPRs across the solver loop
// were spilled to VGPR lanes.  (A generic pointer here made every field a flat VECTOR load with the pointer in VGPRs: two dependent
// memory round trips per output array in the output stage of every agent.)
typedef const StepParams __attribute__((address_space(4))) *KargPtr;
__device__ __forceinline__ KargPtr kernarg_params()
{
    KargPtr p = (KargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
typedef const double __attribute__((address_space(4))) *ConstD;

// ---- the agent prologue, output stage and record of the three kernels that can finish an agent: the scan's unconstrained exit, the general
// ---- solver (dmpc_solve.hip) and the reduced solver (dmpc_rsolve.hip).  One definition each: the outputs are the same words whichever finishes it.
// which agent a wave works for: index vb of the launch -> scene, column ci of the launch, column cl of chunk g_local, index gid into the launch's arrays
struct AgentId { int scene, ci, cl, gid; };
__device__ __forceinline__ AgentId agent_id(const StepParams &P, const int vb)
{
    AgentId I;
    I.scene = vb / P.c_count; I.ci = vb - I.scene * P.c_count;
    I.cl = P.c_first + I.ci;
    I.gid = I.scene * P.c_count + I.ci;
    return I;
}
// ... and what the scan handed over about it: the eight-int header, and the branch record unpacked from it.  (Wave-uniform integers only: the
// agent's state vectors stay plain local arrays of the callers -- a struct the compiler sends to scratch must not make them addressable.)
struct Handoff : AgentId {
    int hdr[8];
    int nr, status, nrows_built, viol_k;
    bool violation, rows_exist, coll0;   // coll0 (cpp): collision noticed at the first step, solution still returned
};
// (readfirstlane: the header is read with vector loads -- the scan wrote it in this launch's lifetime, no scalar load -- and everything
// derived from it, the row count, the status word, the ladder start, would be compiled as lane-dependent: masked loops, vector compares)
__device__ __forceinline__ Handoff agent_handoff(const StepParams &P, const int vb)
{
    Handoff I;
    static_cast<AgentId &>(I) = agent_id(P, vb);
    const int *hdr = P.hdr + (size_t)I.gid * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) I.hdr[i] = UNI(hdr[i]);
    I.nr = I.hdr[0]; I.nrows_built = I.hdr[1]; I.viol_k = I.hdr[2]; I.status = I.hdr[3];
    I.violation = (I.hdr[4] & 1) != 0; I.coll0 = (I.hdr[4] & 4) != 0; I.rows_exist = I.hdr[5] != 0;
    return I;
}

// Closed loops, tiny launches: the work of post_step_kernel for one agent (dmpc_soft_bound.m:132-134, the history column,
// ReachedGoal.m:3-11), done by the wave that produced the agent's step; p_out, v_out, a_out: lanes 0..2 hold the first horizon column.
// The scene's maximum / OR / count are order-independent, so which wave finishes last changes nothing.
__device__ __forceinline__ void post_step_part(const KargPtr Qp, const int lane, const int gid, const int scene, const bool solved,
                                               const int status, const double p_out, const double v_out, const double a_out)
{
    double xn = 0.0, vn = 0.0, an = 0.0, e2 = 0.0;
    if (lane < 3) {
        const size_t b = (size_t)gid * 3 + lane;
        xn = solved ? p_out : Qp->post_xp[b]; vn = solved ? v_out : Qp->post_xv[b]; an = solved ? a_out : Qp->post_xa[b];
        if (solved) { Qp->post_xp[b] = xn; Qp->post_xv[b] = vn; Qp->post_xa[b] = an; }
        const size_t ho = ((size_t)gid * Qp->post_KT + Qp->post_k) * 3 + lane;
        Qp->post_pk[ho] = xn; Qp->post_vk[ho] = vn; Qp->post_ak[ho] = an;
        const double dd = xn - Qp->pf[b];
        e2 = dd * dd;
    }
    const double dx2 = readlane_d(e2, 0), dy2 = readlane_d(e2, 1), dz2 = readlane_d(e2, 2);
    if (lane == 0) {
        const double dist = sqrt(dx2 + dy2 + dz2);
        atomicMax(Qp->post_max + scene, (unsigned long long)__double_as_longlong(dist));
        atomicOr(Qp->post_or + scene, status);
        __threadfence();
        if (atomicAdd(Qp->post_cnt + scene, 1) == Qp->c_count - 1) {   // the scene's last agent of this step
            const unsigned long long mb = atomicExch(Qp->post_max + scene, 0ull);
            const int orv = atomicExch(Qp->post_or + scene, 0);
            Qp->post_cnt[scene] = 0;
            const int reached = __longlong_as_double((long long)mb) < Qp->post_tol ? 1 : 0;
            Qp->post_flags[(size_t)scene * 2] = reached; Qp->post_flags[(size_t)scene * 2 + 1] = orv;
            if (Qp->post_done && (reached || (orv & ~ST_SOLVED))) Qp->post_done[scene] = 1;
        }
    }
}

// Nothing to do for this agent in a solve launch: its scene already stopped, or the scan finished it (unconstrained exit) -- a fused
// post-step still takes its outputs then.  Returns whether the caller returns.
__device__ __forceinline__ bool agent_skip(const StepParams &P, const int lane, const Handoff &I)
{
    if (I.hdr[4] & 8) return true;
    if (I.hdr[4] & 16) {
        if (P.post_on) {
            const KargPtr Qp = kernarg_params();
            const int st_done = Qp->status[I.gid];
            double p1 = 0.0, v1 = 0.0, a1 = 0.0;
            if (lane < 3) { p1 = Qp->p_out[(size_t)I.gid * N3 + lane]; v1 = Qp->v_out[(size_t)I.gid * N3 + lane]; a1 = Qp->a_out[(size_t)I.gid * N3 + lane]; }
            post_step_part(Qp, lane, I.gid, I.scene, (st_done & ST_SOLVED) != 0, st_done, p1, v1, a1);
        }
        return true;
    }
    return false;
}

// solveQPv2 / solveQP / solveSoftDMPC[_c] / solveDMPC have no in-bounds test behind the solve
// (the reduced solver only ever sees bound, bound2, cpp and cpp2: there this is !cppv)
__device__ __forceinline__ bool has_inbounds_test(const int var)
{
    return !(var == VAR_ELLIP || var == VAR_SOFTALL || var == VAR_SOFTALL_C || var == VAR_SCP || var == VAR_CPP1 || var == VAR_CPP || var == VAR_CPP2);
}

// The agent's position and velocity on axis `ax`, read AGAIN behind the solver loop -- six SCALAR loads through constant-address-space
// pointers (the values are wave-uniform) -- instead of living in registers across it
__device__ __forceinline__ void state_again(const KargPtr Qp, const int gid, const int ax, double &po_l, double &vo_l)
{
    const ConstD sp = (ConstD)(unsigned long long)(Qp->x_p + 3 * (size_t)gid), sv_ = (ConstD)(unsigned long long)(Qp->x_v + 3 * (size_t)gid);
    const double po0 = sp[0], po1 = sp[1], po2 = sp[2], vo0 = sv_[0], vo1 = sv_[1], vo2 = sv_[2];
    vo_l = ax == 0 ? vo0 : (ax == 1 ? vo1 : vo2);
    po_l = ax == 0 ? po0 : (ax == 1 ? po1 : po2);
}

// a9/a10, the output stage: propagate, in-bounds test, outputs + next table chunk, fused post-step.  `oc`: this lane holds output component
// (k, ax) = lane 3 k + ax of the stacked vectors, `w` and `a` its position offset and acceleration, `a_s` the stacked accelerations in LDS;
// `post`: a fused post-step is this kernel's to do (the solvers; the scan leaves it to the solve launch: agent_skip); `status` comes in
// with everything but ST_OUTBOUND and goes out complete.
__device__ __forceinline__ int agent_outputs(const KargPtr Qp, const int lane, const AgentId &I, const bool oc, const int k, const int ax,
                                             const bool solved, const double w, const double a, const double *a_s,
                                             const bool inbounds_test, const bool post, int status)
{
    const int gid = I.gid;
    double p_out = 0.0, v_out = 0.0, a_out = 0.0;
    if (solved && oc) {   // p = A_p a + A_initp [po;vo] ; v = A_v a + vo   (propStatedmpc.m:3-4)
        double po_l, vo_l;
        state_again(Qp, gid, ax, po_l, vo_l);
        p_out = w + init_pos(k, Qp->h, vo_l, po_l);
        v_out = vel_out(a_s, k, ax, Qp->h, vo_l);
        a_out = a;
    }
    if (solved && inbounds_test) {   // is_inbounds.m:2-5 on p(:,1)
        const double tolb = 50e-3;
        bool bad = false;
        const double hi3 = lane == 0 ? Qp->pmax[0] : (lane == 1 ? Qp->pmax[1] : Qp->pmax[2]), lo3 = lane == 0 ? Qp->pmin[0] : (lane == 1 ? Qp->pmin[1] : Qp->pmin[2]);
        if (lane < 3) bad = !(p_out < hi3 + tolb) || !(p_out > lo3 - tolb);
        if (__any(bad)) status |= ST_OUTBOUND;
    }
    if (oc) {
        Qp->p_out[(size_t)gid * N3 + lane] = p_out;
        Qp->v_out[(size_t)gid * N3 + lane] = v_out;
        Qp->a_out[(size_t)gid * N3 + lane] = a_out;
        if (Qp->lT_next) {
            // next table chunk [S][3K][C]: uniform 64-bit base, 32-bit per-lane offset; unsolved agents keep their old prediction
            const int Cq = Qp->C;
            // (mixed precision: Qp->lT is the fp32 table of the scan; the fp64 predictions of this chunk are in Qp->own_prev)
            const double *own = Qp->own_prev ? Qp->own_prev + (size_t)I.scene * N3 * Cq + I.cl : Qp->lT + ((size_t)(Qp->g_local * Qp->S + I.scene) * N3) * Cq + I.cl;
            Qp->lT_next[(size_t)I.scene * N3 * Cq + I.cl + (size_t)(unsigned)(lane * Cq)] = solved ? p_out : own[(size_t)(unsigned)(lane * Cq)];
        }
    }
    if (post && Qp->post_on) post_step_part(Qp, lane, gid, I.scene, solved, status, p_out, v_out, a_out);
    return status;
}

// lane 0 of a solver: the agent's status word, work estimate and branch record
__device__ __forceinline__ void agent_record(const KargPtr Qp, const Handoff &I, const int status, const int cost, const bool solved, const int tries,
                                             const int ccase, const int iters, const int nslack, const int q, const int maxq)
{
    Qp->status[I.gid] = status;
    if (Qp->cost_out) Qp->cost_out[I.gid] = cost;
    if (Qp->info) {
        int *inf = Qp->info + (size_t)I.gid * 8;
        inf[0] = I.viol_k; inf[1] = I.nrows_built; inf[2] = tries; inf[3] = (!solved && (status & ST_COLL)) ? 0 : ccase;   // (`coll` return: no QP, no cost case)
        inf[4] = iters; inf[5] = nslack; inf[6] = solved ? q : 0; inf[7] = maxq;
    }
}

// Persistent forms: the wave's NEXT queue ticket is claimed (lane 0, result left in flight in `ticket`) when the agent is as good as done
// -- the first violation scan that finds nothing, or the start of the output stage -- so that the atomic's latency hides behind the
// output stage and nothing is claimed ahead of a solve: a position claimed before a 300-500 us infeasibility proof waited behind
// it, and such parked agents were the last to end the launch (round 3: the waves ended 779-878 us, busy fraction 0.90).
template <bool PERSIST>
__device__ __forceinline__ void claim_next(const int lane, const bool want_ticket, int &ticket, bool &claimed)
{
    if (PERSIST && want_ticket && !claimed) { claimed = true; if (lane == 0) ticket = atomicAdd(kernarg_params()->counter, 1); }
}

// Retry-ladder certificate (bounded-slack variants).  The rows of one horizon step k constrain only w_k = (Lambda a)_k,
// and with |a| <= alim the reachable set of w_k is EXACTLY the box |w_k| <= alim ((k+1) h)^2 / 2 per axis (cut by the
// workspace bounds of that step).  With every slack at its lower bound slb*f the rows are the half-spaces
// -xi.w <= b - sd slb f; if their intersection with the box is empty the QP is infeasible at that ladder level.  A
// bounded non-empty polytope has an edge on the intersection line of two of its planes, so it is empty iff on every
// such line the interval cut out by the other planes is empty: one lane per plane pair (<= 26 rows + 6 faces), one
// pass over the planes each.  Conservative (row subset, 1e-7 relative margin): a level it does not reject is still
// decided by the active-set iteration.  For solveSoftDMPCbound/bound2 all rows sit on ONE step, so the test is
// nearly exact and the ladder jumps straight to the first level that can work instead of proving 2-3 levels
// infeasible with 100+ iterations each.  Only the first 128 rows are used.  Out of line: it runs for a handful
// of agents per launch and must not cost the solver's hot loop any registers.
// `pl_planes`: planes (4 doubles each) the scratch `pl` holds -- the rows of a step beyond pl_planes - 6 are left out.  Until round 5 that was
// 26 rows everywhere (the two 64-double staging vectors), and the heaviest agents of the 10^4-agent scene are exactly those with 27-40 rows on
// their step: the certificate passed levels that the rows it did not look at make infeasible, and the dual method then proved each of them
// with 40-50 iterations at 4-5 us (tools/gpu_c4_iter_trace.py: 81 + 73 of an agent's 207 iterations).  The callers now hand over what is dead
// at the time: the three staging vectors inside a solve (44 planes), the inverse factor's block between two solves (128 rows).
__device__ __attribute__((noinline)) bool ladder_level_infeasible(const double *__restrict__ r_xi, const double *__restrict__ r_b,
                                                                  const double *__restrict__ r_sd, const double *__restrict__ r_slb,
                                                                  const int *__restrict__ r_kc, int nr, double *pl, double h,
                                                                  double alim, double f, double whi_l, double wlo_l, int lane, const int pl_planes = 32)
{
    const int mcap = pl_planes - 6;
    const int kc0 = lane < nr ? r_kc[lane] : -1, kc1 = lane + 64 < nr ? r_kc[lane + 64] : -1;
    bool empty_any = false;
    for (int k = 0; k < K && !empty_any; ++k) {
        const bool t0 = (lane < nr) && kc0 == k, t1 = (lane + 64 < nr) && kc1 == k;
        if (!__any(t0 || t1)) continue;
        const double sh = (double)(k + 1) * h, R = 0.5 * alim * sh * sh;
        // Round 5: rows that the WHOLE reachable box satisfies at this level -- max over |w| <= R of -xi.w = |xi|_1 R <= rhs -- cannot cut the
        // polytope and are left out (exact: the box faces are planes of the set).  The search is cubic in the planes -- every pair's line against
        // every plane, all of them when the level IS infeasible -- and most rows of a step belong to neighbours that only come near: at N = 10^4 a
        // ladder climber spent more time here than iterating.  A row that the whole box violates settles the level at once.
        double rx0[2], rx1[2], rx2[2], rrhs[2];
        bool keep[2], dead = false;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const bool sel = c ? t1 : t0;
            const int i = sel ? lane + 64 * c : 0;
            rx0[c] = r_xi[3 * i]; rx1[c] = r_xi[3 * i + 1]; rx2[c] = r_xi[3 * i + 2];
            rrhs[c] = r_b[i] - r_sd[i] * r_slb[i] * f;
            const double n1 = (fabs(rx0[c]) + fabs(rx1[c]) + fabs(rx2[c])) * R;
            keep[c] = sel && !(n1 * (1.0 + 1e-9) + 1e-12 * fabs(rrhs[c]) <= rrhs[c]);
            dead = dead || (sel && -n1 > rrhs[c] + 1e-7 * (n1 + fabs(rrhs[c])));
        }
        if (__any(dead)) { empty_any = true; break; }
        const bool s0 = keep[0], s1 = keep[1];
        const unsigned long long m0 = __ballot(s0), m1 = __ballot(s1);
        const int c0 = __popcll(m0), m = c0 + __popcll(m1);
        if (m == 0) continue;
        const int M = m < mcap ? m : mcap;
        LSYNC();
        {
            const int p0 = lanes_below(m0, lane), p1 = c0 + lanes_below(m1, lane);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const bool sel = c ? s1 : s0;
                const int pp = c ? p1 : p0;
                if (sel && pp < mcap) {
                    const double x0 = rx0[c], x1 = rx1[c], x2 = rx2[c];
                    const double rhs = rrhs[c];
                    const double sn = 1.0 / ((fabs(x0) + fabs(x1) + fabs(x2)) * R + fabs(rhs) + 1e-300);
                    pl[4 * pp] = -x0 * sn; pl[4 * pp + 1] = -x1 * sn; pl[4 * pp + 2] = -x2 * sn; pl[4 * pp + 3] = rhs * sn;
                }
            }
            // box faces of step k: w <= min(R, whi), -w <= min(R, -wlo); the bounds of component (k, ax) live in lane 3k + ax
            if (lane >= 3 * k && lane < 3 * k + 3) {
                const int ax = lane - 3 * k;
                const double hi = fmin(R, whi_l), lo = fmax(-R, wlo_l), sn = 0.5 / R;
                double *fc = pl + 4 * (M + 2 * ax);
                fc[0] = ax == 0 ? sn : 0.0; fc[1] = ax == 1 ? sn : 0.0; fc[2] = ax == 2 ? sn : 0.0; fc[3] = hi * sn;
                fc[4] = -fc[0]; fc[5] = -fc[1]; fc[6] = -fc[2]; fc[7] = -lo * sn;
            }
        }
        LSYNC();
        const int Mt = M + 6, npair = Mt * (Mt - 1) / 2;
        double best = INFINITY;     // smallest emptiness gap over the lines seen by this lane
        bool found = false;
        for (int base = 0; base < npair && !found; base += 64) {
            const int pr = base + lane;
            const bool valid = pr < npair;
            const int n = Mt, prc = valid ? pr : 0;
            int ii = (int)((2.0f * n - 1.0f - sqrtf((2.0f * n - 1.0f) * (2.0f * n - 1.0f) - 8.0f * (float)prc)) * 0.5f);
            ii = ii < 0 ? 0 : (ii > n - 2 ? n - 2 : ii);
            while (ii > 0 && ii * (2 * n - ii - 1) / 2 > prc) --ii;
            while (ii < n - 2 && (ii + 1) * (2 * n - ii - 2) / 2 <= prc) ++ii;
            int jj = prc - ii * (2 * n - ii - 1) / 2 + ii + 1;
            jj = jj > n - 1 ? n - 1 : jj;
            const double a0 = pl[4 * ii], a1 = pl[4 * ii + 1], a2 = pl[4 * ii + 2], ab = pl[4 * ii + 3];
            const double b0 = pl[4 * jj], b1 = pl[4 * jj + 1], b2 = pl[4 * jj + 2], bb = pl[4 * jj + 3];
            // line: direction d = a x b (normalised), point w0 = (ab (b x d) + bb (d x a)) / |a x b|^2
            double d0 = a1 * b2 - a2 * b1, d1 = a2 * b0 - a0 * b2, d2 = a0 * b1 - a1 * b0;
            const double dd = d0 * d0 + d1 * d1 + d2 * d2;
            const double na2 = a0 * a0 + a1 * a1 + a2 * a2, nb2 = b0 * b0 + b1 * b1 + b2 * b2;
            const bool ok = valid && dd > 1e-16 * na2 * nb2;      // not (nearly) parallel planes
            const double idd = ok ? 1.0 / dd : 0.0;
            const double w0 = (ab * (b1 * d2 - b2 * d1) + bb * (d1 * a2 - d2 * a1)) * idd,
                         w1 = (ab * (b2 * d0 - b0 * d2) + bb * (d2 * a0 - d0 * a2)) * idd,
                         w2 = (ab * (b0 * d1 - b1 * d0) + bb * (d0 * a1 - d1 * a0)) * idd;
            const double idn = ok ? rsqrt(dd) : 0.0;
            d0 *= idn; d1 *= idn; d2 *= idn;
            // the interval [lo, hi] the other planes leave on the line, its ends kept as fractions with positive denominators
            // (lo = ln / ld, hi = hn / hd; -inf and +inf are -1/0 and 1/0): candidates are compared by cross-multiplication, two
            // divisions per line instead of one per plane (the certificate was 10-20 % of a long ladder solve)
            double ln = -1.0, ld = 0.0, hn = 1.0, hd = 0.0, par = -INFINITY;   // par: worst violation among planes parallel to the line
            const double2 *pl2 = (const double2 *)__builtin_assume_aligned(pl, 16);
            for (int c = 0; c < Mt; ++c) {
                const double2 pa = pl2[2 * c], pb = pl2[2 * c + 1];
                const double c0_ = pa.x, c1 = pa.y, c2 = pb.x;
                const double g = c0_ * d0 + c1 * d1 + c2 * d2;                        // slope along the line
                const double r = pb.y - (c0_ * w0 + c1 * w1 + c2 * w2);               // slack at w0 (relative units)
                if (g > 1e-12) { if (r * hd < hn * g) { hn = r; hd = g; } }           // hi = min(hi, r / g)
                else if (g < -1e-12) { if (-r * ld > ln * -g) { ln = -r; ld = -g; } } // lo = max(lo, r / g)
                else par = fmax(par, -r);
            }
            const double gap = fmax((ln / ld - hn / hd) / R, par);   // positive = the line misses the polytope
            if (ok) best = fmin(best, gap);
            found = __any(ok && gap <= 1e-9);
        }
        if (!found && wave_min(best) > 1e-7) empty_any = true;
    }
LSYNC();
return empty_any;
}

// --------------------------------------------------------------------------------------------
// the MPC step: a scan launch (a5/a6) and a solve launch (a7-a10, dmpc_solve.hip)
// --------------------------------------------------------------------------------------------
// scan + collision rows (a5/a6) -> global row scratch + 8-int header per agent.  Splitting the step keeps the solver's
// register and LDS footprint free of the scan's needs (more resident agents per CU) and lets the solver be re-launched
// for the few agents that overflow the tier-1 working-set capacity.
// `vb`: the agent's index in the launch (already renumbered XCD-aware by the kernel); `smem`: this wave's LDS.
// SCP (solveDMPC.m, dmpc_scp_kernel): `scp_prev` = prev_p of the pass (the previous pass's prediction of this agent, 45 doubles; null in the
// first pass: the table's own column, solveDMPC.m:10), `scp_mask` = addConstr as a bit per horizon step (in / out).
template <bool SOFT, typename TT, bool FAST, bool ORD4 = false, bool SCP = false>
__device__ __forceinline__ void scan_body(const StepParams &P, const int lane, const int vb, unsigned char *smem,
                                          const double *scp_prev = nullptr, unsigned *scp_mask = nullptr)
{
    const int S = P.S, G = P.G, C = P.C, nrmax = P.nrmax;
    const AgentId I = agent_id(P, vb);
    const int scene = I.scene, cl = I.cl, gid = I.gid;
    const int var = P.variant;
    constexpr bool soft = SOFT;   // slack-carrying variants (bound, bound2, all3, softall, repair) vs hard rows (hard, ondemand, ellip)

    // `real`: the arithmetic (and table) type of the scan and the row builder -- double, or float in the mixed-precision mode
    // (fp32 table, distance tests and rows; the QP itself stays fp64: rows are stored as doubles)
    using real = TT;
    const TT *const tab = (const TT *)P.lT;
    const real rmin = (real)P.rmin, h_ = (real)P.h, e1z = (real)P.e1z, e2z = (real)P.e2z, alim_ = (real)P.alim;
    // safety margin of the exact pruning / certificates: far below any geometric quantity in fp64, a few float roundings of a
    // workspace-sized coordinate in the mixed mode
    constexpr real MARG = std::is_same<TT, float>::value ? (real)2e-5 : (real)1e-9;
    Lds L;
    real *own_s, *w_s;
    int *scan_cand = nullptr;
    const int *scan_nbr = nullptr;
    {
        double *p = (double *)smem;
        own_s = (real *)p; p += 48;
        w_s = (real *)p; p += 48;   // unconstrained minimiser in position space (launch-order key of the slack-free variants)
        scan_cand = (int *)p;   // SCAN_CAND_CAP ints
        // Collision rows live in a per-agent slice of a GLOBAL scratch buffer (L2-resident; lane = row, so
        // every access is a coalesced wave load): keeping them out of LDS is what lets several times more
        // agents be resident per CU.  Only the per-row working-set flags and the slack values stay in LDS.
        const size_t per = (size_t)nrmax * (soft ? 7 : 4);
        double *g = P.rowbuf + (size_t)gid * per;
        L.r_xi = g; g += 3 * nrmax;
        L.r_b = g; g += nrmax;
        if (soft) { L.r_sd = g; g += nrmax; L.r_st = g; g += nrmax; L.r_slb = g; g += nrmax; }
        else { L.r_sd = L.r_st = L.r_slb = nullptr; }
        L.r_kc = P.rowkc + (size_t)gid * nrmax;
    }
    int *hdr = P.hdr + (size_t)gid * 8;
    if (P.scene_done && __builtin_amdgcn_readfirstlane(P.scene_done[scene])) {
        // the scene's transition is over (dmpc_transition): nothing to solve, the state stays frozen (status 0 = no update)
        if (lane == 0) { hdr[0] = 0; hdr[1] = 0; hdr[2] = 0; hdr[3] = 0; hdr[4] = 8; hdr[5] = 0; hdr[6] = 0; hdr[7] = 0; P.status[gid] = 0; }
        return;
    }

    // ---------------------------------------------------------------- agent state (uniform)
    Agent A;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        A.po[d] = P.x_p[3 * gid + d]; A.vo[d] = P.x_v[3 * gid + d];
        A.ao[d] = P.x_a[3 * gid + d]; A.pf[d] = P.pf[3 * gid + d];
    }
    // own previous prediction: prev_p = l(:,:,n)  (solveSoftDMPCbound.m:6)
    const TT *lT_own = tab + ((size_t)(P.g_local * S + scene) * N3) * C + cl;
    if (lane < N3) own_s[lane] = (SCP && scp_prev) ? (real)scp_prev[lane] : lT_own[(size_t)lane * C];
    LSYNC();
    real po_[3], vo_[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { po_[d] = (real)A.po[d]; vo_[d] = (real)A.vo[d]; }

    // ---------------------------------------------------------------- a5/a6: scan + rows
    int nr = 0, nrows_ref = 0, viol_k = 0, status = 0;
    bool cert_infeasible = false;
    int ladder_start = 0;   // first retry-ladder level that is not certainly infeasible (soft ladder variants)
    bool rows_exist = false, violation = false;
    const bool cppv = (var == VAR_CPP || var == VAR_CPP2);   // dmpc/cpp solveQPv2 flavour (dmpc.cpp:803-1287)
    // Super-ellipsoid of ORDER 4 (round 4; CheckCollEllipDMPC.m:7, CollConstrEllipDMPC.m:13-19 with order = 4, E1 = E^-1, E2 = E^-4 as
    // test/comp_test_ellipconstr.m:158-187 sets them for solveSoftDMPC): dist = |E1 d|_4, xi = E2 d.^3, prev_dist = dist^3,
    // r = dist^3 (rmin - dist) + xi.p - xi.A0 x0.  Only the variants whose scan is "any neighbour inside rmin, rows for every neighbour"
    // (softall, ellip, repair, cpp1: the generic walk below + build_rows) take it; the API refuses the others.
    constexpr bool ord4 = ORD4;   // (a template parameter: the order-2 kernels carry none of it)
    const bool near_sel = (var == VAR_BOUND || var == VAR_BOUND2 || var == VAR_ALL3 || var == VAR_ONDEMAND || cppv);
    const bool coll_check = (var == VAR_BOUND || var == VAR_BOUND2 || var == VAR_ALL3 || var == VAR_REPAIR);
    const bool skip_k1 = (var == VAR_BOUND2 || var == VAR_ALL3 || var == VAR_REPAIR || var == VAR_CPP2);
    bool coll_flag = false;
    // Neighbour list (large scenes, nbr_kernel): a neighbour can come within ellipsoidal distance R of the agent at some
    // horizon step only if the bounding boxes of the two predicted horizons are within R per axis.  The survivors of
    // that test (3 % of the scene at N = 10^4) come, in increasing index order, from the pre-pass; the distance tests /
    // row builders below walk the list instead of all N neighbours.  Conservative: results are unchanged.
    // nnbr < 0: no list (small scenes, variants that take every neighbour, or more survivors than the list holds).
    int nnbr = -1;
    if (P.nbr_cnt && P.nbr_parts == 1) {
        // the grid query leaves the list in ONE piece: one count, nothing to close (sixteen counts read one after the other were fifteen
        // serialised round trips for a zero at the head of every scan wave)
        const int n = __builtin_amdgcn_readfirstlane(P.nbr_cnt[(size_t)gid * NBR_PARTS]);
        if (n >= 0) { nnbr = n; scan_nbr = P.nbr_list + (size_t)gid * P.nbr_cap; }
    } else if (P.nbr_cnt) {
        // nbr_kernel leaves the list in NBR_PARTS pieces (one per part of the scene, each in increasing neighbour order): close the gaps
        int *lst = P.nbr_list + (size_t)gid * P.nbr_cap;
        const int pcap = P.nbr_cap / NBR_PARTS;
        int tot = 0;
        bool fits = true;
        for (int q = 0; q < NBR_PARTS; ++q) {
            const int n = __builtin_amdgcn_readfirstlane(P.nbr_cnt[(size_t)gid * NBR_PARTS + q]);   // (a vector load of a wave-uniform value: the list length steers every loop of the walk)
            if (n < 0) { fits = false; break; }
            if (q > 0 && tot < q * pcap)
                for (int i = lane; i < n; i += 64) lst[tot + i] = lst[q * pcap + i];   // moves down: a round's reads are at or above its writes
            tot += n;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (fits) { nnbr = tot; scan_nbr = lst; }
    }
    // the neighbours are walked 64 at a time: entry e0 + lane of the list, or neighbour (r, j0 + lane) of the table
    const int cpad = (C + 63) & ~63;
    const int n_entries = nnbr >= 0 ? nnbr : G * cpad;
    auto entry = [&](int e0, int &r, int &jc) -> bool {
        if (nnbr >= 0) {
            const bool have = e0 + lane < nnbr;
            const int code = have ? scan_nbr[e0 + lane] : 0;
            r = code >> 20; jc = code & 0xfffff;
            return have;
        }
        r = e0 / cpad;
        const int jj = e0 - r * cpad + lane;
        jc = jj < C ? jj : C - 1;   // clamped: loads are unconditional, results masked
        // unequal clusters (dmpc.cpp:1600-1625: the first N mod G clusters hold one agent more): the chunks from
        // P.short_from on use C-1 columns, their last column is padding
        return jj < C - ((P.short_from && r >= P.short_from) ? 1 : 0) && !(r == P.g_local && jj == cl);
    };

    // Launch-order key of the slack-free variants (see order_kernel): which horizon steps have a row that is violated
    // at the unconstrained minimiser, and how tight the tightest row is against the reachable box.
    unsigned key_steps = 0, key_tight = 0;
    float key_soft = 0.f;    // slack variants: the launch-order key before the terms of the unconstrained-exit block
    float key_share = 1.f;   // slack ladder variants: the smallest share of the reachable box a row leaves feasible at ladder level 0
    if (!soft) {
        // w_unc = Lambda a_unc of the collision cost case (rows exist): 2 q g P1[k][K-1] + 2 s ao M1[0][k]  (Gram table
        // of case 2: G[W k][W K-1] and G[W k][A 0])
        if (lane < N3) {
            const int k = lane / 3, ax = lane - 3 * k;
            const double *tb = P.tables + 2 * TAB_CASE_DOUBLES;
            const double gax = sel3(A.pf, ax) - (sel3(A.po, ax) + (double)K * h_ * sel3(A.vo, ax));
            w_s[lane] = (real)(2.0 * P.Q1 * gax * tb[(15 + k) * 30 + 15 + (K - 1)] + 2.0 * P.S1 * sel3(A.ao, ax) * tb[(15 + k) * 30]);
        }
        LSYNC();
    }
    {
        // appends the rows of horizon step ke (evaluated positions) constraining step kc for every
        // neighbour with dist < sel_r (or all), in increasing neighbour index (CollConstrSoftDMPC.m:11-31)
        // one collision row, CollConstrSoftDMPC.m:16-28: neighbour offset (dx,dy,dz) and ellipsoidal distance at
        // the evaluation step (own position px,py,pz), constraining horizon step kc; compacted by ballot
        auto emit_row = [&](bool sel, int kc, real dx, real dy, real dz, real dist, real px, real py, real pz) {
            const real sh = (real)(kc + 1) * h_;
            const real a0x = po_[0] + sh * vo_[0], a0y = po_[1] + sh * vo_[1], a0z = po_[2] + sh * vo_[2];
            // diff = E2*(p - pj).^(order-1); pd = prev_dist = dist^(order-1) (P.e2z = c^-order)
            // (order 4, DMPC::solveQP: dmpc.cpp:47,478 scale before the power, (E2 d).^3 -- z component (c^-4 dz)^3; the MATLAB helpers E2 * d.^3)
            const real dzs = dz * e2z;
            const real x0 = ord4 ? dx * dx * dx : dx, x1 = ord4 ? dy * dy * dy : dy, x2 = ord4 ? (var == VAR_CPP1 ? dzs * dzs * dzs : dz * dz * dz * e2z) : dzs;
            const real pd = ord4 ? dist * dist * dist : dist;
            {
                const unsigned long long m0 = __ballot(sel);
                if (m0 == 0ull) return;                         // no neighbour of this chunk is close at this step
                nrows_ref += __popcll(m0);                      // the reference's row count (branch record)
            }
            // Exact pruning: with |a| <= alim the position at step kc stays in the box
            // A0_kc x0 +- alim (kc h)^2/2, so a row whose linearised distance cannot drop below rmin anywhere in
            // that box can never become active; dropping it (and its slack, which stays 0) leaves the minimiser
            // unchanged.  Margin 1e-9 keeps borderline rows.
            {
                const real hw = 0.5 * alim_ * sh * sh;
                if (!soft && sel) {
                    // the row reads  xi.w_kc >= rr  for the position offset w = Lambda a;  |w_kc| <= hw per axis
                    // (the right-hand side of the row without the reference's division: dist (xi.p / dist) = xi.p)
                    const real rr = pd * (rmin - dist) + (x0 * px + x1 * py + x2 * pz) - (x0 * a0x + x1 * a0y + x2 * a0z);
                    const real rng = (fabs(x0) + fabs(x1) + fabs(x2)) * hw;
                    if (rr - (x0 * w_s[3 * kc] + x1 * w_s[3 * kc + 1] + x2 * w_s[3 * kc + 2]) > (real)0.1 * MARG) key_steps |= 1u << kc;
                    key_tight |= (rr > 0.8 * rng) ? 8u : ((rr > 0.5 * rng) ? 4u : ((rr > 0.0) ? 2u : 1u));
                }
                const real lin_min = x0 * (a0x - (px - dx)) + x1 * (a0y - (py - dy)) + x2 * (a0z - (pz - dz)) - (fabs(x0) + fabs(x1) + fabs(x2)) * hw;
                if (lin_min >= pd * rmin + MARG && !P.no_prune) sel = false;
                // Exact infeasibility certificate for rows without slack: if even the BEST point of the
                // reachable box violates the row (max of the linearised distance < dist*rmin), no acceleration
                // within |a| <= alim satisfies it -> the QP is infeasible; the long active-set proof is skipped.
                if (sel) {
                    const real lin_max = lin_min + 2.0 * (fabs(x0) + fabs(x1) + fabs(x2)) * hw;
                    if (!soft) {
                        if (lin_max < pd * rmin - MARG) cert_infeasible = true;
                    } else if (var == VAR_BOUND || var == VAR_BOUND2 || var == VAR_ALL3 || cppv) {
                        // Soft rows with a bounded slack (coefficient dist): the row needs
                        //   lin >= dist*(rmin + eps),  eps >= slb * 2^t at ladder level t (solveSoftDMPCbound.m:147-153),
                        // so every level with lin_max < dist*(rmin + slb 2^t) is certainly infeasible and the
                        // retry ladder can start at the first level that passes this necessary test.
                        real slb_t = (var == VAR_BOUND) ? -0.05 : (cppv ? -(real)0.01f : -0.01);
                        {   // launch-order key: the feasible share of the reachable box at ladder level 0 (as the slack-free variants' tightness class)
                            const real share = (lin_max - dist * (rmin + slb_t)) / (lin_max - lin_min + (real)1e-30);
                            key_share = fminf(key_share, (float)share);
                        }
                        int t = 0;
                        while (t < 40 && lin_max < dist * (rmin + slb_t) - MARG) { slb_t *= 2.0; ++t; }
                        if (t > ladder_start) ladder_start = t;
                    }
                }
            }
            const unsigned long long m = __ballot(sel);
            const int pos = nr + lanes_below(m, lane);
            if (sel && pos < nrmax) {
                // r = dist*(rmin - dist + diff*p/dist) - diff*A_initp(kc)*[po;vo]   (:21)
                const real rr = pd * (rmin - dist + (x0 * px + x1 * py + x2 * pz) / pd) - (x0 * a0x + x1 * a0y + x2 * a0z);
                L.r_xi[3 * pos] = x0; L.r_xi[3 * pos + 1] = x1; L.r_xi[3 * pos + 2] = x2;
                L.r_b[pos] = -rr;
                L.r_kc[pos] = kc;
                    if (soft) {
                    // (cost term and lower bound are constants of the fp64 QP, not results of the row arithmetic: they stay doubles in the float
                    // instantiation too -- -0.05 and -0.01 are no floats, and a term that is none would lose its low bits;
                    // tests/test_gpu_mixed_rows.py holds them to the reference's bits)
                    real sd = pd;
                    double st = P.term, slb = -0.05;
                    if (var == VAR_BOUND2 || var == VAR_ALL3) slb = -0.01;           // bound2:77, all:92
                    else if (cppv) slb = -(double)0.01f;                            // dmpc.cpp:907-914,1079: -eps <= lim, float lim = 0.01
                    else if (var == VAR_SOFTALL) { sd = 1.0; st = -1e5; slb = -INFINITY; }  // solveSoftDMPC.m:21,65
                    else if (var == VAR_SOFTALL_C) {
                        // solveSoftDMPC_c.m:18-20,60-63: rows [Ainr I], cost EPS eps^2 + f_eps eps with EPS = 1e6 (K/k)^2, f_eps = -1e4 (K/k)^2, k the
                        // violating step (1-based).  The solver's slack variables carry the unit weight of every other variant (H_eps = 2): substitute
                        // eps = eps' / sqrt(EPS) -- the row's slack coefficient becomes 1 / sqrt(EPS), the linear cost f_eps / sqrt(EPS), the pin
                        // eps <= 0 is eps' <= 0; the minimiser in a is the same.
                        const double rk = (double)K / (double)(kc + 1), quad = 1.0 * 1e6 * (rk * rk), lin = -1.0 * 1e4 * (rk * rk);
                        const double isq = 1.0 / sqrt(quad);
                        sd = (real)isq; st = (real)(lin * isq); slb = -INFINITY;
                    }
                    else if (var == VAR_CPP1) { sd = 1.0; st = -1e6; slb = -INFINITY; }     // dmpc.cpp:629-633,715: [A I] x <= b, eps <= 0, f_w = -10^6
                    else if (var == VAR_REPAIR) { st = (real)(P.term / pd); slb = -INFINITY; }   // repair:77,81 (term ./ prev_dist)
                    L.r_sd[pos] = sd; L.r_st[pos] = st; L.r_slb[pos] = slb;
                }
            }
            nr += __popcll(m);
        };

        // rows of horizon step ke (positions evaluated there) constraining step kc for every neighbour whose
        // distance AT STEP ksel is < sel_r (viol_constr of CheckCollSoftDMPC.m:12) or for all neighbours,
        // in increasing neighbour index (CollConstrSoftDMPC.m:11-31)
        auto build_rows = [&](int ksel, int ke, int kc, real sel_r, bool sel_all) {
            const real qx = own_s[3 * ksel], qy = own_s[3 * ksel + 1], qz = own_s[3 * ksel + 2];
            const real px = own_s[3 * ke], py = own_s[3 * ke + 1], pz = own_s[3 * ke + 2];
            for (int e0 = 0; e0 < n_entries; e0 += 64) {
                int r, jc;
                const bool valid = entry(e0, r, jc);
                const real *nbp = tab + ((size_t)(r * S + scene) * N3) * C + jc;
                const real *base = nbp + (size_t)(3 * ke) * C, *bsel = nbp + (size_t)(3 * ksel) * C;
                const real dx = px - base[0], dy = py - base[(size_t)C], dz = pz - base[2 * (size_t)C];
                const real ez = dz * e1z;
                const real dist = ord4 ? sqrt(sqrt(dx * dx * dx * dx + dy * dy * dy * dy + ez * ez * ez * ez)) : sqrt(dx * dx + dy * dy + ez * ez);
                real dsel = dist;
                if (ksel != ke && !sel_all) {
                    const real sx = qx - bsel[0], sy = qy - bsel[(size_t)C];
                    const real sz = (qz - bsel[2 * (size_t)C]) * e1z;
                    dsel = sqrt(sx * sx + sy * sy + sz * sz);
                }
                emit_row(valid && (sel_all || dsel < sel_r), kc, dx, dy, dz, dist, px, py, pz);
            }
        };

        // Scan (CheckCollSoftDMPC.m:7-15): all K distances of a neighbour are computed from loads issued
        // together (5 horizon steps = 15 coalesced wave loads per batch) instead of one dependent round per
        // step; per-step "any neighbour inside rmin" bits are OR-reduced across the wave afterwards.
        int ncand = 0;
        // second pass of the hard-row scan: one lane per buffered candidate
        auto flush_candidates = [&]() {
            LSYNC();
            for (int b0 = 0; b0 < ncand; b0 += 64) {
                const bool have = b0 + lane < ncand;
                const int code = have ? scan_cand[b0 + lane] : 0;
                const int kk = (code >> 28) & 15, rr = (code >> 20) & 255, jj = code & 0xfffff;
                const real *nb = tab + ((size_t)(rr * S + scene) * N3 + 3 * kk) * C + jj;
                const real px = own_s[3 * kk], py = own_s[3 * kk + 1], pz = own_s[3 * kk + 2];
                const real dx = px - nb[0], dy = py - nb[(size_t)C], dz = pz - nb[2 * (size_t)C];
                const real ez = dz * e1z;
                const real dist = sqrt(dx * dx + dy * dy + ez * ez);
                emit_row(have && dist < 1.0, kk, dx, dy, dz, dist, px, py, pz);
            }
            ncand = 0;
            LSYNC();
        };
        unsigned anyb = 0;
        real mind0 = INFINITY;
        const real rmin2_hi = (ord4 ? rmin * rmin * rmin * rmin : rmin * rmin) * ((real)1.0 + (real)4.0 * MARG);
        if (var == VAR_HARD) {
            // solveHardDMPC.m:18-22 + CollConstrHardDMPC.m:19: every k, neighbours with dist < 1.  Two passes.  The first
            // only tests the 15 N distances and compacts the (step, neighbour) candidates -- about one in ten -- into an
            // LDS list; flush_candidates() then builds the rows of 64 candidates at a time, so the row arithmetic runs on
            // full waves.  The first pass walks the FLAT index e = k * ne + entry (step-major, the reference's row order),
            // 64 pairs per round: every round is a full wave whatever N is (lanes = neighbours wastes 22 % of the issue
            // slots at N = 100, and the scan is instruction-issue bound), a lane's three loads share one address
            // computation, and runs of lanes with the same k still read contiguous table rows.
            const unsigned ne = (unsigned)(nnbr >= 0 ? nnbr : G * C);
            const unsigned total = ne * (unsigned)K;
            // (k, entry) of a lane advance by 64 pairs per round: running counters with one wrap test, no division in the
            // loop (64 = step_q * ne + step_r; lanes past the end have k >= K)
            const UDiv div_ne(ne), div_c((unsigned)C);
            const int step_q = (int)(64u / (ne ? ne : 1u)), step_r = (int)(64u - (unsigned)step_q * ne);
            const size_t slab = (size_t)N3 * C;
            auto pass = [&](auto single_tag) {
                constexpr bool single = decltype(single_tag)::value;   // one chunk, no neighbour list: entry == neighbour index
                constexpr int UR = 4;   // rounds in flight: the loads of four rounds are issued before the first is used
                int k_run, idx_run;
                div_ne.divmod((unsigned)lane, k_run, idx_run);
                for (unsigned e0 = 0; e0 < total; e0 += 64 * UR) {
                    // room for a whole group of rounds is made BEFORE its loads are issued, so that the row builder never
                    // runs with the group's registers live
                    if (ncand + 64 * UR > SCAN_CAND_CAP) flush_candidates();
                    real nx[UR], ny[UR], nz[UR];
                    int kk[UR], code[UR];
                    bool ok[UR];
#pragma unroll
                    for (int u = 0; u < UR; ++u) {
                        bool valid = k_run < K;
                        const int k = valid ? k_run : 0, idx = valid ? idx_run : 0;
                        idx_run += step_r; k_run += step_q;
                        if (idx_run >= (int)ne) { idx_run -= (int)ne; k_run += 1; }
                        int r = 0, jc = idx;
                        if (!single) {
                            if (nnbr >= 0) {
                                const int c = scan_nbr[idx];
                                r = c >> 20; jc = c & 0xfffff;
                            } else {
                                div_c.divmod((unsigned)idx, r, jc);
                                valid = valid && !(r == P.g_local && jc == cl) && jc < C - ((P.short_from && r >= P.short_from) ? 1 : 0);
                            }
                        } else valid = valid && jc != cl;
                        const real *nb = tab + ((size_t)(single ? P.g_local : r) * S + scene) * slab + (unsigned)(3 * k * C + jc);
                        nx[u] = nb[0]; ny[u] = nb[(size_t)C]; nz[u] = nb[2 * (size_t)C];
                        kk[u] = k; code[u] = (k << 28) | (r << 20) | jc; ok[u] = valid;
                    }
#pragma unroll
                    for (int u = 0; u < UR; ++u) {
                        if (e0 + 64u * u >= total) break;
                        const int k = kk[u];
                        const real px = own_s[3 * k], py = own_s[3 * k + 1], pz = own_s[3 * k + 2];
                        const real dx = px - nx[u], dy = py - ny[u], dz = pz - nz[u];
                        const real ez = dz * e1z;
                        const real d2 = dx * dx + dy * dy + ez * ez;
                        // squared distance against a slightly inflated threshold (a superset); the exact `norm(...) < 1`
                        // decision is made on the IEEE square root in the second pass
                        const bool cand = ok[u] && d2 < (real)1.0 + (real)4.0 * MARG;
                        const unsigned long long cm = __ballot(cand);
                        if (cm) {
                            if (cand) scan_cand[ncand + lanes_below(cm, lane)] = code[u];
                            ncand += __popcll(cm);
                        }
                    }
                }
            };
            if (G == 1 && nnbr < 0) pass(std::true_type{});
            else pass(std::false_type{});
        } else if (nnbr >= 0 && P.lrow) {
            // Neighbour list: the walk is TRANSPOSED -- lanes = horizon components, one listed neighbour per step of the loop.
            // With lanes = neighbours every table load of a round is a gather of 64 cache lines (45 of them per round: at
            // N = 10^4 the list walk took 1-2 ms of gathers); here a neighbour's whole horizon is ONE coalesced 256-byte load
            // from the neighbour-major fp32 copy of the table (table_nbrmajor_kernel: [chunk][scene][column][15 x (x, y, z, 0) + 4];
            // 2.5 MB at N = 10^4: L2 resident), and the three squares of a step are summed with two row-shift DPP moves (groups
            // of 4 lanes never straddle a row).  The fp32 distance only SELECTS (threshold widened by 1e-3, a hundred times the
            // rounding of a workspace-sized coordinate); the decision dist < rmin is made on the table itself, with the
            // arithmetic of the other walk, for the few (step, neighbour) pairs that pass.
            // Close pairs (grid_query_kernel): the query's distance test has just formed these fp32 distances from the same rows and left the
            // (neighbour, step) pairs below the same threshold, rmin^2 * 1.001: lanes = pairs, one round of exact tests, no walk.  The bits
            // cannot change: the fp32 test only SELECTS, and with the threshold widened by 1e-3 -- a hundred times the fp32 rounding of a
            // workspace-sized coordinate -- the query's selection and the walk's are both supersets of the pairs with exact dist < rmin (they
            // may differ from each other at the threshold's edge: another summation order).  anyb is an OR over the exact decisions, made
            // here with the walk's expression and operand order; mind0 is read only when some neighbour is inside rmin at k = 0, and the
            // minimising pair is then in every superset.  Count -1 (more pairs than the list holds) or no close list: the walk below.
            const int ncl = (!SCP && P.close_cnt) ? __builtin_amdgcn_readfirstlane(P.close_cnt[gid]) : -1;
            if (ncl >= 0) {
                typedef int i2_t __attribute__((ext_vector_type(2)));
                const i2_t *cl = (const i2_t *)P.close_list + (size_t)gid * P.close_cap;
                for (int e0 = 0; e0 < ncl; e0 += 64) {
                    const bool have = e0 + lane < ncl;
                    const i2_t rec = cl[have ? e0 + lane : e0];
                    const int code = rec.x, kq = rec.y, k3 = 3 * kq;
                    const real *nb = tab + ((size_t)((code >> 20) * S + scene) * N3 + k3) * C + (code & 0xfffff);
                    if (have) {
                        const real dx = own_s[k3] - nb[0], dy = own_s[k3 + 1] - nb[(size_t)C], dz = own_s[k3 + 2] - nb[2 * (size_t)C];
                        const real ez = dz * e1z;
                        const real d2 = dx * dx + dy * dy + ez * ez;
                        const real dist = sqrt(d2);
                        if (dist < rmin) anyb |= (1u << kq);       // CheckCollSoftDMPC.m:11
                        if (kq == 0) mind0 = fmin(mind0, d2);       // (only ever used when some neighbour is inside rmin at k = 0)
                    }
                }
            } else {
            const float *rt = (const float *)P.lrow;
            const float *rt1 = rt + (size_t)scene * C * 64;
            constexpr int TW = 8;
            const int k4 = lane >> 2, a4 = lane & 3;
            const bool act = a4 < 3 && k4 < K;
            const bool head = a4 == 0 && k4 < K;
            const float ownc = act ? (float)own_s[3 * k4 + a4] : 0.f;
            const float sc = act ? (a4 == 2 ? (float)e1z : 1.f) : 0.f;
            const float thr = (float)(rmin * rmin) * 1.001f;
            const int k3 = head ? 3 * k4 : 0;
            // (two copies of the loop: one chunk -- a scene on one GPU, the code IS the column -- and the general form, which costs eight more
            // scalar instructions per listed neighbour; a test per neighbour cost branches instead.  The walk of the 100-700 neighbours of an
            // agent of a 10^4-agent scene is scalar-bound.)
            auto walk = [&](auto one_tag) {
            constexpr bool one = decltype(one_tag)::value;
            for (int e0 = 0; e0 < nnbr; e0 += 64) {
                const int codes = (e0 + lane < nnbr) ? scan_nbr[e0 + lane] : 0;
                const int m = (nnbr - e0) < 64 ? (nnbr - e0) : 64;
                for (int u0 = 0; u0 < m; u0 += TW) {
                    float nv[TW];   // loads in flight
                    int cu[TW];
#pragma unroll
                    for (int u = 0; u < TW; ++u) {
                        const int uu = (u0 + u < m) ? u0 + u : m - 1;   // (a repeated neighbour changes nothing: OR and min)
                        cu[u] = readlane_i(codes, uu);
                        nv[u] = one ? rt1[(size_t)(unsigned)cu[u] * 64 + lane]
                                    : rt[((size_t)((cu[u] >> 20) * S + scene) * C + (cu[u] & 0xfffff)) * 64 + lane];
                    }
#pragma unroll
                    for (int u = 0; u < TW; ++u) {
                        const float d = (ownc - nv[u]) * sc;
                        const float q2 = d * d;
                        const float d2f = (q2 + dpp_row_shl<1>(q2)) + dpp_row_shl<2>(q2);   // lanes 4k: squared distance at step k
                        const bool flag = head && d2f < thr;
                        if (__any(flag)) {
                            const real *nb = tab + ((size_t)((cu[u] >> 20) * S + scene) * N3 + k3) * C + (cu[u] & 0xfffff);
                            if (flag) {
                                const real dx = own_s[k3] - nb[0], dy = own_s[k3 + 1] - nb[(size_t)C], dz = own_s[k3 + 2] - nb[2 * (size_t)C];
                                const real ez = dz * e1z;
                                const real d2 = dx * dx + dy * dy + ez * ez;
                                const real dist = sqrt(d2);
                                if (dist < rmin) anyb |= (1u << k4);       // CheckCollSoftDMPC.m:11
                                if (k4 == 0) mind0 = fmin(mind0, d2);       // (only ever used when some neighbour is inside rmin at k = 0)
                            }
                        }
                    }
                }
            }
            };
            if (G == 1) walk(std::true_type{}); else walk(std::false_type{});
            }
        } else {
            for (int e0 = 0; e0 < n_entries; e0 += 64) {
                int r, jc;
                const bool valid = entry(e0, r, jc);
                const real *base = tab + ((size_t)(r * S + scene) * N3) * C + jc;
                // the 45 component rows of a neighbour are C doubles apart: a running (uniform) offset, advanced by one
                // 64-bit scalar add per load (written as (3k+c)*C the compiler spends five scalar instructions per load)
                size_t roff = 0;
    #pragma unroll 1
                for (int kg = 0; kg < 3; ++kg) {   // not unrolled: keeps the scan's register footprint small
                    real nx[5], ny[5], nz[5];
    #pragma unroll
                    for (int u = 0; u < 5; ++u) {
                        nx[u] = base[roff]; roff += (size_t)C; if (!SCP) asm volatile("" : "+s"(roff));   // (not in the SCP instantiation: inside dmpc_scp_kernel's pass loop the compiler keeps the offset in a vector register and refuses the constraint)
                        ny[u] = base[roff]; roff += (size_t)C; if (!SCP) asm volatile("" : "+s"(roff));
                        nz[u] = base[roff]; roff += (size_t)C; if (!SCP) asm volatile("" : "+s"(roff));
                    }
    #pragma unroll
                    for (int u = 0; u < 5; ++u) {
                        const int k = 5 * kg + u;
                        const real px = own_s[3 * k], py = own_s[3 * k + 1], pz = own_s[3 * k + 2];
                        const real dx = px - nx[u], dy = py - ny[u], dz = pz - nz[u];
                        const real ez = dz * e1z;
                        // (order 4: the sum of fourth powers against rmin^4; the root of the root decides)
                        const real d2 = ord4 ? dx * dx * dx * dx + dy * dy * dy * dy + ez * ez * ez * ez : dx * dx + dy * dy + ez * ez;
                        // The IEEE square root (a dozen instructions in fp64) is taken only when some lane of the
                        // wave can pass the distance test: d2 is first compared against a slightly inflated squared
                        // threshold (a superset), the exact `norm(...) < r` decision is then made on sqrt(d2) itself.
                        if (__any(valid && d2 < rmin2_hi)) {
                            // (the empty asm keeps this a BRANCH: the compiler turned the wave-uniform test into selects and ran the 25
                            // instructions of the IEEE root for every step of every neighbour -- 800 of the 3 000 instructions of an agent's scan)
                            asm volatile("");
                            const real dist = ord4 ? sqrt(sqrt(d2)) : sqrt(d2);
                            if (valid && dist < rmin) anyb |= (1u << k);       // CheckCollSoftDMPC.m:11
                        }
                        if (k == 0 && valid) mind0 = fmin(mind0, d2);           // squared; the root is taken once below
                    }
                }
            }
        }
        if (SCP) {
            // solveDMPC.m:21-35: CheckCollDMPC at every step of prev_p (anyb: the walk above with E1 = I); rows for ALL other agents at every step
            // of addConstr, and at the FIRST violating step that is not in it yet (at most one new step per pass); ascending k = the reference's order
            anyb = wave_or(anyb);
            unsigned m = *scp_mask;
            bool newc = false;
            for (int k = 0; k < K; ++k) {
                bool add = (m >> k) & 1u;
                if (!add && !newc && ((anyb >> k) & 1u)) { add = true; newc = true; m |= 1u << k; }
                if (add) build_rows(k, k, k, (real)0, true);
            }
            *scp_mask = m;
            rows_exist = nrows_ref > 0;               // `isempty(Ain_total)` (:38)
            violation = m != 0u;
            viol_k = m ? __ffs((int)m) : 0;           // smallest member of addConstr, 1-based
        } else if (var == VAR_HARD) {
            flush_candidates();
            rows_exist = (G * C - (P.short_from ? G - P.short_from : 0) > 1);   // preallocated zero rows make Ain_coll non-empty (CollConstrHardDMPC.m:3-4)
        } else {
            anyb = wave_or(anyb);
            for (int k = 0; k < K; ++k) {
                if (!((anyb >> k) & 1u)) continue;
                if (var == VAR_ALL3) violation = true;   // solveSoftDMPCall.m:22 (some_violation)
                if ((coll_check || cppv) && k == 0) {
                    mind0 = sqrt((real)wave_min((double)mind0));   // min of the roots == root of the min (sqrt is monotone)
                    if (ord4) mind0 = sqrt(mind0);                // (order 4: the walk accumulated sums of fourth powers)
                    if (coll_check && mind0 < rmin - 0.05) { status = ST_COLL; viol_k = 1; break; }   // :25-31
                    // cpp: `dist < _rmin - _collision_tol` (floats) raises execution_ended, the build goes on (dmpc.cpp:419-424)
                    if (cppv && mind0 < (real)((float)rmin - 0.05f)) coll_flag = true;
                }
                // DMPC::solveQP (dmpc.cpp:626-637): rows on step k-1 (`3*(k-1)`, :480-485); k = 0 indexes row -3 there (undefined): `coll`, no QP
                if (var == VAR_CPP1 && k == 0) { status = ST_COLL; viol_k = 1; break; }
                if (skip_k1 && k == 0) continue;          // solveSoftDMPCbound2.m:29-31
                viol_k = k + 1; violation = true; rows_exist = true;
                if (var == VAR_ALL3) {                     // solveSoftDMPCall.m:34-48: steps k-1,k,k+1
                    const int k0 = (k == 1) ? k : k - 1, k1 = (k == K - 1) ? k : k + 1;
                    for (int kk = k0; kk <= k1; ++kk) build_rows(k, kk, kk, 3.0 * rmin, false);
                } else {
                    const int kc = (var == VAR_BOUND2 || var == VAR_CPP2 || var == VAR_CPP1) ? k - 1 : k;   // CollConstrSoftDMPC2.m:8; dmpc.cpp:516; :480-485
                    // neighbour radius: 3 rmin (CheckCollSoftDMPC.m:12); cpp: _rmin*(1+(float)k/_k_hor) in float arithmetic
                    // (dmpc.cpp:418) -- __f*_rn keep the three float operations unfused
                    const real near_r = cppv ? (real)__fmul_rn((float)rmin, __fadd_rn(1.0f, __fdiv_rn((float)k, (float)K))) : 3.0 * rmin;
                    build_rows(k, k, kc, near_r, !near_sel);
                }
                break;
            }
        }
        // header for the solve phase
        if (nr > nrmax) { status |= ST_CAPACITY; nr = nrmax; }
        if (__any(cert_infeasible)) status |= ST_INFEAS;
        if (lane == 0) {
            hdr[0] = nr; hdr[1] = nrows_ref; hdr[2] = viol_k; hdr[3] = status;
            hdr[4] = (violation ? 1 : 0) | (coll_flag ? 4 : 0); hdr[5] = rows_exist ? 1 : 0; hdr[6] = 0;
        }
        const int ls_key = (int)wave_max((double)ladder_start);
        if (lane == 0) hdr[6] = ls_key;
        {
            // launch-order key (order_kernel, heaviest first).  Slack-carrying variants: the row count.  Slack-free
            // variants: 4 x (horizon steps with a row violated at the unconstrained minimiser) + tightness class of the
            // tightest row (its feasible share of the reachable box: > 1/2, > 1/4, > 1/10, less).  Forcing launch orders on
            // the hardware (tools/gpu_order_probe.py, 51 200 C2 agents): natural 1240 us, by row count 1137, by the true
            // iteration counts 1096, by this key 1064.
            int key = nr >> 2;
            if (soft) {
                // Slack variants (round 4): rows / 4 said little about the work -- at N = 10^4 the solve launch took 1.6 times its work per wave
                // slot and ended with agents of 100-450 us from the END of the queue.  Ingredients fitted on that scene's closed loop
                // (tools/gpu_key_features.py + tools/key_fit.py: list scheduling of the agents' measured work in the order a candidate key gives):
                // the smallest feasible share of the reachable box a row leaves at ladder level 0, the ladder levels the scan certified
                // infeasible, and -- added in the unconstrained-exit block below, where the unconstrained minimiser is known -- the acceleration
                // bounds and the rows it violates.  (An agent's own previous solve predicts the bulk, rank correlation 0.8, but not the heavy
                // agents: a retry ladder is a one-step event.  The perfect order would be worth 0.97 -> 0.72 ms; this key 0.97 -> 0.8x.)
                const float smin = -(float)wave_max((double)-key_share);
                key_soft = 0.7f * (float)nr + 56.f * (1.f - fminf(fmaxf(smin, 0.f), 1.f)) + 52.f * (float)ls_key;
                key = (int)key_soft;
            }
            if (!soft) {
                const unsigned ks = wave_or(key_steps), kt = wave_or(key_tight);
                key = 4 * __popc(ks) + (kt ? 31 - __clz((int)kt) : 0);
            }
            if (lane == 0) hdr[7] = key > 255 ? 255 : key;
        }
        // ---- unconstrained exit.  Most agent-steps of a transition are trivial: no bound, workspace wall or collision row is violated
        // at the unconstrained minimiser a_unc (closed form from the tables), so the active-set loop would stop before its first
        // iteration.  Such an agent is finished HERE -- same arithmetic as the solver's set-up and output stage (the shared helpers
        // above), its header flagged (hdr[4] & 16) -- and never enters the solve queue: the scan runs at twice the solver's
        // occupancy and the agent's state is already in registers.  (43 % of the agents of the solveSoftDMPCbound replay of
        // bench.py, nearly all of them once the swarm has spread out.)
        if (FAST && status == 0 && !__any(cert_infeasible) && nr <= 128) {   // (FAST: a template parameter -- launches without the exit do not carry its registers)
            const int ls = (int)wave_max((double)ladder_start);
            // The launch parameters and the agent's state are read AGAIN here -- scalar loads through constant-address-space pointers --
            // instead of staying live in SGPRs across the neighbour walk and the row builder: the slack variants' scan spilled 190
            // scalar registers to VGPR lanes (a fifth of its instructions were v_readlane / v_writelane and the s_nop around them).
            const KargPtr Qp = kernarg_params();
            Agent B_;
            {
                const ConstD sp = (ConstD)(unsigned long long)(Qp->x_p + 3 * (size_t)gid), sv = (ConstD)(unsigned long long)(Qp->x_v + 3 * (size_t)gid);
                const ConstD sa = (ConstD)(unsigned long long)(Qp->x_a + 3 * (size_t)gid), sf = (ConstD)(unsigned long long)(Qp->pf + 3 * (size_t)gid);
#pragma unroll
                for (int d = 0; d < 3; ++d) { B_.po[d] = sp[d]; B_.vo[d] = sv[d]; B_.ao[d] = sa[d]; B_.pf[d] = sf[d]; }
            }
            const int ccase = cost_case(var, B_.po[0] - B_.pf[0], B_.po[1] - B_.pf[1], B_.po[2] - B_.pf[2], rows_exist);
            const double qw = ccase == 0 ? Qp->Qfar : (ccase == 1 ? Qp->Qnear : Qp->Q1);
            const double sw = ccase == 2 ? ((var == VAR_ALL3) ? 10.0 : Qp->S1) : Qp->Sfree;
            const bool comp = lane < N3;
            const int k_l = comp ? lane / 3 : 0, ax_l = comp ? lane - 3 * k_l : 0;
            const double *tb = Qp->tables + (size_t)ccase * TAB_CASE_DOUBLES;
            double a_unc = 0.0, w_unc = 0.0;
            bool viol = false;
            const double tol = 1e-10;
            if (comp) {
                const double po_l = sel3(B_.po, ax_l), vo_l = sel3(B_.vo, ax_l);   // (picked once: with a sel3 per use the compiler kept B_.po addressable, 32 bytes of scratch)
                const double gax = goal_gap(sel3(B_.pf, ax_l), po_l, vo_l, Qp->h);
                const double ao_l = sel3(B_.ao, ax_l);
                a_unc = unc_entry(qw, sw, gax, ao_l, tb[k_l * 30 + 15 + (K - 1)], tb[k_l * 30]);
                w_unc = unc_entry(qw, sw, gax, ao_l, tb[(15 + k_l) * 30 + 15 + (K - 1)], tb[(15 + k_l) * 30]);
                const double sh = (double)(k_l + 1) * Qp->h * vo_l;
                const double whi = (ax_l == 0 ? Qp->pmax[0] : (ax_l == 1 ? Qp->pmax[1] : Qp->pmax[2])) - po_l - sh, wlo = (ax_l == 0 ? Qp->pmin[0] : (ax_l == 1 ? Qp->pmin[1] : Qp->pmin[2])) - po_l - sh;
                viol = (fabs(a_unc) - Qp->alim > tol) || (fmax(w_unc - whi, wlo - w_unc) > tol);
            }
            bool trivial = ls == 0 && !__any(viol);
            double *a_s = (double *)smem, *wu_s = a_s + 48;   // (own prediction and key vector are dead by now)
            if (soft) {   // launch-order key, second part: acceleration bounds and rows violated at the unconstrained minimiser
                const int nsat = __popcll(__ballot(comp && fabs(a_unc) - Qp->alim > tol));
                LSYNC();
                if (comp) { a_s[lane] = a_unc; wu_s[lane] = w_unc; }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the rows this wave wrote are read back
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                LSYNC();
                int nrv = 0;   // (wave-uniform: whole rounds)
                for (int i0 = 0; i0 < nr; i0 += 64) {
                    const bool in = i0 + lane < nr;
                    const int i = in ? i0 + lane : 0;
                    const int kc = L.r_kc[i];
                    const double v = -(L.r_xi[3 * i] * wu_s[3 * kc] + L.r_xi[3 * i + 1] * wu_s[3 * kc + 1] + L.r_xi[3 * i + 2] * wu_s[3 * kc + 2]) - L.r_b[i];
                    nrv += __popcll(__ballot(in && v > tol));
                }
                trivial = trivial && nrv == 0;
                const int key2 = (int)(key_soft + 1.5f * (float)nsat + 5.6f * (float)nrv);
#ifdef DMPC_DEV_TRACE   // development: the raw ingredients in the upper bits of the word (tools/gpu_key_features.py; order_kernel reads bits 0-8 only)
                const float smin = -(float)wave_max((double)-key_share);
                const int qs = smin >= 1.f ? 31 : (smin <= 0.f ? 0 : (int)(smin * 31.f));
                if (lane == 0) hdr[7] = (key2 > 255 ? 255 : key2) | (qs << 9) | ((nsat > 63 ? 63 : nsat) << 14) | ((nrv > 63 ? 63 : nrv) << 20) | ((ls > 7 ? 7 : ls) << 26);
#else
                if (lane == 0) hdr[7] = key2 > 255 ? 255 : key2;
#endif
            }
            if (trivial && !soft) {
                LSYNC();
                if (comp) { a_s[lane] = a_unc; wu_s[lane] = w_unc; }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the rows this wave wrote are read back
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                LSYNC();
                bool rv = false;
                for (int i = lane; i < nr; i += 64) {
                    const int kc = L.r_kc[i];
                    const double v = -(L.r_xi[3 * i] * wu_s[3 * kc] + L.r_xi[3 * i + 1] * wu_s[3 * kc + 1] + L.r_xi[3 * i + 2] * wu_s[3 * kc + 2]) - L.r_b[i];
                    rv = rv || v > tol;
                }
                trivial = !__any(rv);
            }
            if (trivial) {
                // (the solvers' output stage; a fused post-step of this agent is left to the solve launch: agent_skip)
                const int st = agent_outputs(Qp, lane, I, comp, k_l, ax_l, true, w_unc, a_unc, a_s, has_inbounds_test(var), false, ST_SOLVED | (coll_flag ? ST_COLL : 0));
                if (lane == 0) {
                    Qp->status[gid] = st;
                    hdr[4] = (violation ? 1 : 0) | (coll_flag ? 4 : 0) | 16;
                    hdr[7] = 256;   // (the order kernel reads this word only)
                    if (Qp->info) {   // (the solvers' agent_record with its constants: one try, no iteration, no work estimate)
                        int *inf = Qp->info + (size_t)gid * 8;
                        inf[0] = viol_k; inf[1] = nrows_ref; inf[2] = 1; inf[3] = ccase;
                        inf[4] = 0; inf[5] = 0; inf[6] = 0; inf[7] = 0;
                    }
                }
            }
        }
    }
}

extern __shared__ __attribute__((aligned(16))) unsigned char dmpc_smem[];

#include "dmpc_solve.hip"
#include "dmpc_rsolve.hip"

// Scan phase: blockDim.x / 64 independent waves per workgroup, one agent each (P.lds_per_wave bytes of LDS per wave).
// Single-wave workgroups leave the launch bound by the workgroup dispatch rate (51 200 workgroups in ~180 us whatever the
// waves do); the waves never synchronise.
// XCD-aware mapping: workgroups are dealt round-robin to the 8 XCDs (block b -> XCD b % 8, private L2 each), so they are
// renumbered such that every XCD works on whole scenes: a scene's prediction table is then fetched into ONE L2 instead of
// eight.  Pure performance remap (a bijection on [0, gridDim)).
template <bool SOFT, typename TT, bool FAST, bool ORD4 = false>
__global__ __launch_bounds__(64 * SCAN_WAVES_PER_WG, SCAN_WAVES_PER_SIMD) void dmpc_scan_kernel(StepParams P)
{
    const int W = (int)(blockDim.x >> 6);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const int nb = (int)gridDim.x, x = (int)blockIdx.x & 7, y = (int)blockIdx.x >> 3;
    int off = 0;
    for (int xx = 0; xx < x; ++xx) off += (nb - xx + 7) >> 3;
    const int agent = (off + y) * W + wave, total = P.S * P.c_count;
    if (P.zero4 && blockIdx.x == 0 && threadIdx.x < 4) P.zero4[threadIdx.x] = 0;   // (nothing reads them before the order / solve kernels of this step)
    if (P.gzero) for (int z = (int)(blockIdx.x * blockDim.x + threadIdx.x); z < P.gzero_n; z += (int)(gridDim.x * blockDim.x)) P.gzero[z] = 0;   // (the cell grid's counters: their last reader, the list query, ran before this launch)
    if (agent >= total) return;
    scan_body<SOFT, TT, FAST, ORD4>(P, lane, agent, dmpc_smem + (size_t)wave * P.lds_per_wave);
}
// Solve phase, one agent per 64-thread workgroup (shallow launches: bound by their slowest agent)
template <bool SOFT, int QCAP, typename TF = double>
__global__ __launch_bounds__(64, SOLVE_WAVES_PER_SIMD) void dmpc_solve_kernel(StepParams P)
{
    int tk_unused = 0; bool cl_unused = false;
    solve_body<SOFT, QCAP, false, QCAP, TF>(P, threadIdx.x, blockIdx.x, gridDim.x, dmpc_smem, nullptr, false, tk_unused, cl_unused);
}

// solveDMPC.m:17-72, the SCP loop of ONE agent inside one launch: every pass is the scan (CheckCollDMPC + CollConstrDMPC about the previous
// pass's prediction, scan_body<.., SCP>) followed by the slack-free QP (solve_body) of the same wave; between the two and between passes the
// agent's rows, header and outputs travel through its slices of the global scratch / output arrays (same wave, same CU: workgroup-scope fences
// order them).  The loop ends when the pass's largest position change is <= tol (maxDeviation.m), after k_hor passes, or with the first
// infeasible pass (`success = 0`, :58-63).  Scan and solver use the same LDS one after the other.
__global__ __launch_bounds__(64, SOLVE_WAVES_PER_SIMD) void dmpc_scp_kernel(StepParams P)
{
    const int lane = (int)threadIdx.x;
    const int nb = (int)gridDim.x, x = (int)blockIdx.x & 7, y = (int)blockIdx.x >> 3;
    int off = 0;
    for (int xx = 0; xx < x; ++xx) off += (nb - xx + 7) >> 3;
    const int vb = off + y;   // (solve_body renumbers blockIdx the same way)
    const int scene = vb / P.c_count, ci = vb - scene * P.c_count, gid = scene * P.c_count + ci;
    if (P.zero4 && blockIdx.x == 0 && threadIdx.x < 4) P.zero4[threadIdx.x] = 0;
    unsigned mask = 0u;
    double prev_l = 0.0;
    if (lane < N3) prev_l = P.lT[((size_t)(P.g_local * P.S + scene) * N3 + lane) * P.C + P.c_first + ci];   // prev_p = l(:,:,n) (:10)
    int passes = 0, iters_sum = 0, st = 0;
    const double *own_out = P.p_out + (size_t)gid * N3;
    for (int i = 1; i <= K; ++i) {   // `while (i <= k_hor && val > tol)` (:17); val = tol + 2 before the first pass
        scan_body<false, double, false, false, true>(P, lane, vb, dmpc_smem, i > 1 ? own_out : nullptr, &mask);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        LSYNC();
        if (UNI(P.hdr[(size_t)gid * 8 + 4]) & 8) return;   // scene of a transition that already stopped
        int tk_unused = 0; bool cl_unused = false;
        solve_body<false, 48, false>(P, lane, (int)blockIdx.x, nb, dmpc_smem, nullptr, false, tk_unused, cl_unused);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        LSYNC();
        ++passes;
        st = UNI(P.status[gid]);
        if (P.info) iters_sum += UNI(P.info[(size_t)gid * 8 + 4]);
        if (!(st & ST_SOLVED)) break;
        // val = maxDeviation(p, prev_p) (:69): maxDeviation.m:3 takes K = length(p)/3 of the 3 x k_hor matrix -- the first max(3, k_hor)/3 = 5 steps
        const double new_l = lane < N3 ? own_out[lane] : 0.0;
        const double dl = new_l - prev_l, d2 = dl * dl;
        // (lanes 3k: the squared distance of step k; the maximum over the first five steps through the fixed-order wave reduction)
        const double s3 = (d2 + dpp_row_shl<1>(d2)) + dpp_row_shl<2>(d2);
        const bool head = lane < 3 * ((K > 3 ? K : 3) / 3) && (lane % 3) == 0 && (lane & 15) <= 13;
        double val = wave_max(head ? sqrt(s3) : 0.0);
        {   // steps whose three lanes straddle a 16-lane row (step 5 = lanes 15..17 is beyond the five steps looked at: none here)
            static_assert(((K > 3 ? K : 3) / 3) * 3 <= 16, "maxDeviation: the steps looked at lie in the first DPP row");
        }
        prev_l = new_l;   // (:70)
        if (!(val > P.scp_tol)) break;
    }
    if (lane == 0 && P.info) { P.info[(size_t)gid * 8 + 2] = passes; P.info[(size_t)gid * 8 + 4] = iters_sum; }
}

// Persistent form of the REDUCED solver (dmpc_rsolve.hip): workgroups of RSOLVE_WAVES independent waves, as many per CU as the registers
// allow (no tables, 768 bytes of LDS per wave); the queue is the one of dmpc_solve_persist_kernel.
#ifndef RSOLVE_WAVES
#define RSOLVE_WAVES 8
#endif
constexpr int RSOLVE_LDS_PER_WAVE = 4 * 70 * 8;   // the output stage's 96 doubles; the ladder certificate's planes (4 doubles each: 64 rows + 6 box faces)
__global__ __launch_bounds__(RSOLVE_WAVES * 64) void dmpc_rsolve_persist_kernel(StepParams P)
{
    int total = P.S * P.c_count;
    if (P.live_bound) { const int lb = *P.live_bound; total = lb < total ? lb : total; }
    if (total == 0) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned char *mine = (unsigned char *)__builtin_assume_aligned(dmpc_smem + (size_t)wave * RSOLVE_LDS_PER_WAVE, 16);
    const int nw = (int)(gridDim.x * (blockDim.x >> 6));
    const int rest = total > nw ? total - nw : 0;
    const int T1 = rest < QUEUE_T1 * nw ? rest : QUEUE_T1 * nw;
    const int T3 = (rest - T1) < QUEUE_T3 * nw ? (rest - T1) : QUEUE_T3 * nw;
    const int CHUNK = P.queue_chunk > 0 ? P.queue_chunk : QUEUE_CHUNK;
    const int mid = rest - T1 - T3, T2 = (mid + CHUNK - 1) / CHUNK;
    const bool dyn = P.counter != nullptr;
    auto resolve = [&](int ps) -> int { return (ps < total && P.order) ? P.order[ps] : ps; };
    auto decode = [&](int t, int &left) -> int {
        left = 0;
        if (t < T1) return nw + t;
        if (t < T1 + T2) {
            const int ps = nw + T1 + CHUNK * (t - T1), end = nw + T1 + mid;
            left = (end - ps < CHUNK ? end - ps : CHUNK) - 1;
            return ps;
        }
        return nw + T1 + mid + (t - T1 - T2);
    };
    int pos = wave * (int)gridDim.x + (int)blockIdx.x, left = 0;
    for (;;) {
        if (pos >= total) break;
        int tkv = 0;
        bool claimed = false;
        const bool want = dyn && left == 0;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int agent = resolve(pos);
#ifdef RSOLVE_TRACE
        const long long t_a = wall_clock64();
#endif
        rsolve_body(P, ln, agent, mine, want, tkv, claimed);
        if (want && !claimed && lane == 0) tkv = atomicAdd(P.counter, 1);
        LSYNC();
#ifdef RSOLVE_TRACE
        // development: start time and duration of every agent (dmpc_debug_trace with agent = -5), 100 MHz ticks
        if (P.dbg && P.dbg_agent == -5 && lane == 0) { P.dbg[(size_t)agent * 2] = (double)t_a; P.dbg[(size_t)agent * 2 + 1] = (double)(wall_clock64() - t_a); }
#endif
        if (!dyn) { pos += nw; continue; }
        if (left > 0) { pos++; left--; continue; }
        pos = decode(__builtin_amdgcn_readfirstlane(tkv), left);
    }
}

// Persistent form of the solve phase: one workgroup of up to 8 independent waves per CU (two per SIMD).  The Gram tables of the three
// cost cases and the Lambda table (23 KB) are staged in LDS ONCE per workgroup and shared by its waves; every wave then
// claims agents from a global queue (heaviest first when order_kernel ran) until it is empty, so a wave that finishes a
// light agent immediately starts the next one and the launch ends when the LAST agent ends, not when the slowest
// workgroup slot drains.  No workgroup barrier after the table load: the waves never synchronise.
// (slack-free variants: 9 waves per workgroup -- with the row flags as bits a ninth wave fits next to the tables in the CU's 160 KB,
// and 168 registers per lane hold the kernel without spills; the slack variants need 17 KB of LDS and 230 registers per wave: 8)
// (round 4, slack-free variants: TWELVE waves per workgroup -- three per SIMD, what 168 registers per lane allow -- with the split T of
// dmpc_solve.hip: TS columns of the factor per wave and a pool of P.n_ext extensions behind the waves' blocks)
template <bool SOFT, int QCAP, int TS = QCAP, typename TF = double>
__global__ __launch_bounds__(SOFT ? 512 : DMPC_HARD_PW * 64, 1) void dmpc_solve_persist_kernel(StepParams P)
{
    // tier 2 works through the list of agents tier 1 flagged (P.order points at it); usually it is empty
    int total = P.only_flagged ? *P.flag_count : P.S * P.c_count;
    if (!P.only_flagged && P.live_bound) { const int lb = *P.live_bound; total = lb < total ? lb : total; }   // the rest of the order: agents the scan finished
    if (total == 0) return;
    double *shtab = (double *)dmpc_smem;
    for (int i = threadIdx.x; i < TAB_DOUBLES; i += blockDim.x) shtab[i] = P.tables[i];
    if (TS < QCAP) {   // the pool of T extensions: all free, all zero
        double *ex = (double *)(dmpc_smem + PERSIST_TABLE_BYTES + (size_t)(blockDim.x >> 6) * P.lds_per_wave);
        for (int i = threadIdx.x; i < P.n_ext * ext_doubles(QCAP, TS) + (int)(EXT_PAD_BYTES / 8); i += blockDim.x) ex[i] = 0.0;
        if (threadIdx.x == 0) *(unsigned *)(dmpc_smem + PERSIST_TABLE_BYTES - 16) = (1u << P.n_ext) - 1u;
    }
    __syncthreads();
    // readfirstlane: tells the compiler the wave index (and with it every LDS base address and every value read
    // through one) is wave-uniform -- otherwise the solver's uniform branches are compiled as divergent ones
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned char *mine = (unsigned char *)__builtin_assume_aligned(dmpc_smem + PERSIST_TABLE_BYTES + (size_t)wave * P.lds_per_wave, 16);
    // The queue.  First round: position wave * #workgroups + workgroup, i.e. the heaviest #waves agents each get a wave (and
    // the heaviest #workgroups a CU) of their own.  Later positions are claimed with TICKETS from one global counter.  An
    // atomic on one address costs ~12 ns of serialised service on this part (51 200 single claims = 0.6 ms, measured: the
    // launch could not end sooner whatever the solver did), and its result takes microseconds to arrive; so
    //   * a ticket stands for one position where the agents are heavy (the #waves positions after the first round) and
    //     where the launch ends (the last #waves positions: a fine-grained tail), and for QUEUE_CHUNK adjacent positions in
    //     between (the light bulk): fewer atomics, at most one light chunk of imbalance -- and a pre-claimed chunk waits behind
    //     its wave's current agent, which is why the chunk is short;
    //   * the next ticket is claimed when the current agent is as good as solved (claim_next) and read after its output
    //     stage: most of the latency hides there, and no position waits behind a solve that turns out long.
    const int nw = (int)(gridDim.x * (blockDim.x >> 6));
    const int rest = total > nw ? total - nw : 0;
    const int T1 = rest < QUEUE_T1 * nw ? rest : QUEUE_T1 * nw;
    const int T3 = (rest - T1) < QUEUE_T3 * nw ? (rest - T1) : QUEUE_T3 * nw;
    // (round 5: per launch -- two positions per ticket pay where the queue is deep and its agents light, the 512-scene replays: fewer atomics;
    // in a shallow queue of heavy agents, the 10^4-agent scene at 5.6 agents per wave, the second position waits behind a solve that may turn
    // out long and such positions ended the launch: 0.75 -> 0.71 ms with single positions)
    const int CHUNK = P.queue_chunk > 0 ? P.queue_chunk : QUEUE_CHUNK;
    const int mid = rest - T1 - T3, T2 = (mid + CHUNK - 1) / CHUNK;
    // (Rounds 2-3 claimed the next ticket right BEFORE the current agent was solved -- the atomic's latency hides completely -- and the
    // positions parked behind long solves ended the launch late: waves ending 779-878 us.  Claiming two positions ahead -- the agent behind the next ticket resolved through the order during the solve, so that
    // only one memory round trip per agent is exposed -- was built and measured in round 3: 0.935 against 0.891 ms on the headline
    // launch.  A claimed position waits behind its wave's current agent, and when that one is a 300-500 us infeasibility proof the
    // light agents parked behind it end the launch late.)
    const bool dyn = P.counter != nullptr;
    auto resolve = [&](int ps) -> int { return (ps < total && P.order) ? P.order[ps] : ps; };   // queue position -> agent
    auto decode = [&](int t, int &left) -> int {   // ticket -> first position it stands for (+ `left` further ones)
        left = 0;
        if (t < T1) return nw + t;
        if (t < T1 + T2) {
            const int ps = nw + T1 + CHUNK * (t - T1), end = nw + T1 + mid;
            left = (end - ps < CHUNK ? end - ps : CHUNK) - 1;
            return ps;
        }
        return nw + T1 + mid + (t - T1 - T2);
    };
    int pos = wave * (int)gridDim.x + (int)blockIdx.x, left = 0;
#ifdef DMPC_DEV_TRACE
    // development: start / end time and agent count of every wave (dmpc_debug_trace with agent = -2)
    const long long t_begin = wall_clock64();
    int n_done = 0;
#endif
    for (;;) {
        if (pos >= total) break;
#ifdef DMPC_DEV_TRACE
        n_done++;
        const long long t_a = wall_clock64();
#endif
        int tkv = 0;
        bool claimed = false;
        const bool want = dyn && left == 0;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int agent = resolve(pos);
        solve_body<SOFT, QCAP, true, TS, TF>(P, ln, agent, total, mine, shtab, want, tkv, claimed,
                                         (int)(((blockDim.x >> 6) - wave) * (P.lds_per_wave >> 3)));
        if (want && !claimed && lane == 0) tkv = atomicAdd(P.counter, 1);   // (the quick ways out of the solver: stopped scene, agent finished by the scan)
        LSYNC();
#ifdef DMPC_DEV_TRACE
        // development: start time and duration of every queue position (dmpc_debug_trace with agent = -3) / of every agent (-5)
        if (P.dbg && P.dbg_agent == -3 && lane == 0) { P.dbg[(size_t)pos * 2] = (double)t_a; P.dbg[(size_t)pos * 2 + 1] = (double)(wall_clock64() - t_a); }
        if (P.dbg && P.dbg_agent == -5 && lane == 0) { P.dbg[(size_t)agent * 2] = (double)t_a; P.dbg[(size_t)agent * 2 + 1] = (double)(wall_clock64() - t_a); }
#endif
        if (!dyn) { pos += nw; continue; }
        if (left > 0) { pos++; left--; continue; }
        pos = decode(__builtin_amdgcn_readfirstlane(tkv), left);
    }
#ifdef DMPC_DEV_TRACE
    if (P.dbg && P.dbg_agent == -2 && lane == 0) {
        double *d = P.dbg + ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * 3;
        d[0] = (double)t_begin; d[1] = (double)wall_clock64(); d[2] = (double)n_done;
    }
#endif
}

// --------------------------------------------------------------------------------------------
// small layout / bookkeeping kernels
// --------------------------------------------------------------------------------------------

#include "dmpc_lists.hip"   // the neighbour lists of large scenes: segment boxes, the cell grid (two builds), the grid query, the all-pairs box test

// calibration of the HBM-side counters (profiles/: FETCH_SIZE is documented for 16-byte-per-lane streams only): a streaming read of a known
// number of bytes at 8 or 16 bytes per lane, coalesced, as this library's kernels read their tables and rows
template <typename T>
__global__ void read_probe_kernel(size_t n, const T *__restrict__ src, double *__restrict__ sink)
{
    double acc = 0.0;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
        const T v = src[t];
        acc += ((const double *)&v)[0];
    }
    if (acc == 1.2345e300) sink[0] = acc;   // (keeps the loads alive; never true for a zeroed buffer)
}

// Longest-processing-time-first launch order for the solve phase: agents are bucketed by the key the scan left in
// hdr[7] (row count for the slack-carrying variants, violated steps + tightness for the slack-free ones) and the solve
// kernel takes them heaviest first, so the long solves do not end up alone at the tail of the launch.  Pure scheduling:
// results do not depend on the order.  gridDim.x workgroups: workgroup b sorts the agents i = b (mod gridDim.x)
// (statistically identical slices) and writes its r-th heaviest agent to position r * gridDim.x + b, so the
// interleaved sequence is heaviest-first overall up to the differences between the slices.
// Order hint (round 4): when the context solved the same batch shape in its previous step, `prev_cost` holds every agent's work estimate of
// THAT solve (quarter microseconds, written by the solve kernel; 0: finished by the scan) -- in a closed loop the best predictor there is of
// this step's solve (an agent in a conflict stays in it for several steps), where the scan's key (row count) says little about the retry
// ladder or the size of the final working set: at N = 10^4 the launch took 1.6 times its work per wave slot and ended with agents of
// 100-450 us that the row count had put at the END of the queue.  key = max(previous cost / 4 us, scan key); the entry is reset to 0 for
// agents the scan finishes this step.
__global__ void order_kernel(int count, const int *__restrict__ hdr, int *__restrict__ order, int *__restrict__ live_bound, int *__restrict__ prev_cost, int use_hint)
{
    // (agents the scan already finished -- hdr[7] & 256, as hdr[4] & 16 -- sort behind everything else: bucket 256.  Slice b puts its live agents at
    // positions b, b + nb, ...: every position from nb * max_b(live agents of slice b) on holds a finished agent, and that bound
    // is what the solve queue runs to.)
    __shared__ int hist[257];
    __shared__ int offs[257];
    short *keys = (short *)dmpc_smem;   // dynamic LDS: the slice's keys, first pass -> second pass (ceil(count / gridDim.x) entries)
    const int nb = gridDim.x, b = blockIdx.x;
    for (int i = threadIdx.x; i < 257; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int i = b + nb * (int)threadIdx.x; i < count; i += nb * (int)blockDim.x) {
        const int h7 = hdr[(size_t)i * 8 + 7];
        int heavy = h7 & 255;
        if (prev_cost) {
            const int pc = prev_cost[i] >> 4;
            if (use_hint == 2 ? pc > 0 : (use_hint && pc > heavy)) heavy = pc > 255 ? 255 : pc;   // (2: the previous work alone -- in a replay of ONE step the perfect order: tools/gpu_order_oracle.py)
            if (h7 & 256) prev_cost[i] = 0;
        }
        const int key = (h7 & 256) ? 256 : 255 - heavy;   // bucket: heaviest first
        keys[(i - b) / nb] = (short)key;
        atomicAdd(&hist[key], 1);
    }
    __syncthreads();
    {   // exclusive prefix of the 257 buckets: a scan inside each of the first four waves, their totals through LDS (one thread walking the buckets was 3 us of a 7 us kernel)
        __shared__ int wsum[4];
        const int t = (int)threadIdx.x, ln = t & 63, wv = t >> 6;
        int v = 0, inc = 0;
        if (t < 256) {
            v = hist[t]; inc = v;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(inc, off); if (ln >= off) inc += o; }
            if (ln == 63) wsum[wv] = inc;
        }
        __syncthreads();
        if (t < 256) {
            int base = 0;
            for (int w = 0; w < wv; ++w) base += wsum[w];
            offs[t] = base + inc - v;
        }
        if (t == 0) {
            const int live = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            offs[256] = live;
            if (live_bound) atomicMax(live_bound, nb * live);
        }
    }
    __syncthreads();
    for (int i = b + nb * (int)threadIdx.x; i < count; i += nb * (int)blockDim.x) {
        const int key = keys[(i - b) / nb];
        order[(size_t)atomicAdd(&offs[key], 1) * nb + b] = i;
    }
}

// rows[S][N][3K] -> lT[G][S][3K][C], N = G*C
__global__ void table_from_rows_kernel(int S, int G, int C, const double *__restrict__ rows, double *__restrict__ lT)
{
    const size_t total = (size_t)S * G * C * N3;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        // t enumerates the destination (coalesced writes): [g][s][j][c]
        const int c = (int)(t % C);
        size_t u = t / C;
        const int j = (int)(u % N3); u /= N3;
        const int s = (int)(u % S);
        const int g = (int)(u / S);
        lT[t] = rows[((size_t)s * (G * C) + (size_t)g * C + c) * N3 + j];
    }
}

// Uncommanded vehicles (columns N_cmd .. N-1 of a one-chunk table lT[S][3K][N]): po replicated over the horizon (dmpc.cpp:1633-1649),
// written into BOTH tables of the transition's ping-pong pair once -- the solve kernels only ever write the columns of the agents they solved.
// po: [S][N][3]
__global__ void static_cols_kernel(int S, int N, int N_cmd, const double *__restrict__ po, double *__restrict__ lTa, double *__restrict__ lTb)
{
    const int M = N - N_cmd;
    const size_t total = (size_t)S * N3 * M;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = N_cmd + (int)(t % M);   // t enumerates the destination: [s][j][c - N_cmd]
        const size_t u = t / M;
        const int j = (int)(u % N3), s = (int)(u / N3);
        const double v = po[((size_t)s * N + c) * 3 + j % 3];
        const size_t o = ((size_t)s * N3 + j) * N + c;
        lTa[o] = v;
        lTb[o] = v;
    }
}

// Scripted vehicles (columns N_cmd .. N-1 of a one-chunk table lT[S][3K][N]) for the MPC step that produces history column k (k >= 1):
// horizon entry kk of vehicle j is sample(j, k-1+kk) = path[j][min(k-1+kk, P-1)] -- the window STARTS at column k-1, like a commanded
// neighbour's row (the output of step k-1, whose first column is history column k-1); a path that has ended stays at its last sample.
// Written into the CURRENT table before every step (the solve kernels only ever write the columns of the agents they solved); lTf
// non-null: the same columns of the table's fp32 copy.  path: [S][M][P][3], M = N - N_cmd
__global__ void scripted_cols_kernel(int S, int N, int N_cmd, int P, int k, const double *__restrict__ path, double *__restrict__ lT,
                                     float *__restrict__ lTf)
{
    const int M = N - N_cmd;
    const size_t total = (size_t)S * N3 * M;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(t % M);   // t enumerates the destination: [s][j][c - N_cmd]
        const size_t u = t / M;
        const int j = (int)(u % N3), s = (int)(u / N3);
        const long col = (long)k - 1 + j / 3;
        const size_t smp = (size_t)(col < (long)P - 1 ? col : (long)P - 1);
        const double v = path[(((size_t)s * M + m) * P + smp) * 3 + j % 3];
        const size_t o = ((size_t)s * N3 + j) * N + N_cmd + m;
        lT[o] = v;
        if (lTf) lTf[o] = (float)v;
    }
}

// rows[S][N_cmd][3K] of the commanded agents -> columns 0 .. N_cmd-1 of the one-chunk table lT[S][3K][N]
__global__ void cmd_cols_from_rows_kernel(int S, int N, int N_cmd, const double *__restrict__ rows, double *__restrict__ lT)
{
    const size_t total = (size_t)S * N3 * N_cmd;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % N_cmd);
        const size_t u = t / N_cmd;
        const int j = (int)(u % N3), s = (int)(u / N3);
        lT[((size_t)s * N3 + j) * N + c] = rows[((size_t)s * N_cmd + c) * N3 + j];
    }
}

// mixed precision: the fp32 copy of a table the scan of the next step reads
__global__ void table_to_f32_kernel(size_t n, const double *__restrict__ src, float *__restrict__ dst)
{
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) dst[t] = (float)src[t];
}

// x <- first horizon column for solved agents (dmpc_soft_bound.m:132-134)
__global__ void advance_kernel(int count, const double *__restrict__ p, const double *__restrict__ v,
                               const double *__restrict__ a, const int *__restrict__ status, double *x_p, double *x_v, double *x_a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * 3) return;
    const int ag = i / 3, d = i - 3 * ag;
    if (status[ag] & ST_SOLVED) {
        x_p[i] = p[(size_t)ag * N3 + d];
        x_v[i] = v[(size_t)ag * N3 + d];
        x_a[i] = a[(size_t)ag * N3 + d];
    }
}

// initDMPC.m:6-12: p(:,i) = po + t_i (pf - po)/10, v = a = 0 ; writes rows [count][3K]
__global__ void init_rows_kernel(int count, double h, const double *__restrict__ po, const double *__restrict__ pf,
                                 double *__restrict__ l_rows)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * N3) return;
    const int ag = i / N3, j = i - ag * N3;
    const int k = j / 3, d = j - 3 * k;
    const double t = (double)k * h;
    const double diff = pf[3 * ag + d] - po[3 * ag + d];
    l_rows[i] = po[3 * ag + d] + 1 * t * diff / 10;
}

// pk/vk/ak(:,k,n) = state after MPC step k   (dmpc_soft_bound.m:132-134); hist: [S][N][KT][3]
__global__ void record_kernel(int S, int N, int KT, int k, const double *__restrict__ x_p, const double *__restrict__ x_v,
                              const double *__restrict__ x_a, double *pk, double *vk, double *ak)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * N * 3) return;
    const int ag = i / 3, d = i - 3 * ag;
    const size_t o = ((size_t)ag * KT + k) * 3 + d;
    pk[o] = x_p[i]; vk[o] = x_v[i]; ak[o] = x_a[i];
}

// The three small kernels that follow a solve in a transition, in one launch (one block per scene; a 100-agent step is
// latency bound, and three launches cost more than their work): x <- first horizon column of the solved agents
// (dmpc_soft_bound.m:132-134), the history column k (pk/vk/ak(:,k,n)), then the scene verdict as scene_reduce_kernel.
// `disturb` is the hook between the state advance and the history record: NoDisturb here, dmpc_disturb.hip's rule in post_step_disturbed_kernel.
struct NoDisturb {
    static constexpr bool on = false;
    __device__ void operator()(int, int, int, int, double *, double *) const {}
};
template <class Disturb>
__device__ __forceinline__ void post_step_body(int N, int KT, int k, double tol, const double *__restrict__ p, const double *__restrict__ v,
                                               const double *__restrict__ a, const int *__restrict__ status, double *x_p, double *x_v, double *x_a,
                                               const double *__restrict__ pf, double *pk, double *vk, double *ak, int *flags, int *scene_done,
                                               const int *__restrict__ stopped, const Disturb &disturb)
{
    __shared__ double smax[256];
    __shared__ int sor[256];
    const int s = blockIdx.x;
    // a scene whose trial ended at an earlier step is left alone: its history columns stay zero, as the preallocated pk/vk/ak of
    // the reference do after its `break` (failure_rate.m:112-125)
    if (stopped && stopped[s]) return;
    double m = 0.0; int o = 0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const size_t ag = (size_t)s * N + i, b = ag * 3;
        const int st = status[ag];
        const bool advance = (st & ST_SOLVED) != 0;
        double xp[3], xv[3], xa[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (advance) { xp[d] = p[ag * N3 + d]; xv[d] = v[ag * N3 + d]; xa[d] = a[ag * N3 + d]; }
            else { xp[d] = x_p[b + d]; xv[d] = x_v[b + d]; xa[d] = x_a[b + d]; }
        }
        disturb(s, i, N, k, xp, xv);   // (every agent of a running scene, whether it advanced or not)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (advance || Disturb::on) { x_p[b + d] = xp[d]; x_v[b + d] = xv[d]; x_a[b + d] = xa[d]; }
            const size_t ho = (ag * KT + k) * 3 + d;
            pk[ho] = xp[d]; vk[ho] = xv[d]; ak[ho] = xa[d];
        }
        const double dx = xp[0] - pf[b], dy = xp[1] - pf[b + 1], dz = xp[2] - pf[b + 2];
        m = fmax(m, sqrt(dx * dx + dy * dy + dz * dz));
        o |= st;
    }
    smax[threadIdx.x] = m; sor[threadIdx.x] = o;
    __syncthreads();
    for (int w = blockDim.x / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) { smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + w]); sor[threadIdx.x] |= sor[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int reached = smax[0] < tol ? 1 : 0;
        flags[(size_t)s * 2] = reached; flags[(size_t)s * 2 + 1] = sor[0];
        if (scene_done && (reached || (sor[0] & ~ST_SOLVED))) scene_done[s] = 1;
    }
}
__global__ void post_step_kernel(int N, int KT, int k, double tol, const double *__restrict__ p, const double *__restrict__ v,
                                 const double *__restrict__ a, const int *__restrict__ status, double *x_p, double *x_v, double *x_a,
                                 const double *__restrict__ pf, double *pk, double *vk, double *ak, int *flags, int *scene_done,
                                 const int *__restrict__ stopped)
{
    post_step_body(N, KT, k, tol, p, v, a, status, x_p, x_v, x_a, pf, pk, vk, ak, flags, scene_done, stopped, NoDisturb{});
}

// one block per scene: flags[0] = ReachedGoal.m:3-11 (max_i ||p_i - pf_i|| < tol), flags[1] = OR of status bits
__global__ void scene_reduce_kernel(int N, double tol, const double *__restrict__ x_p, const double *__restrict__ pf,
                                    const int *__restrict__ status, int *flags, int *scene_done)
{
    __shared__ double smax[256];
    __shared__ int sor[256];
    const int s = blockIdx.x;
    double m = 0.0; int o = 0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const size_t b = ((size_t)s * N + i) * 3;
        const double dx = x_p[b] - pf[b], dy = x_p[b + 1] - pf[b + 1], dz = x_p[b + 2] - pf[b + 2];
        m = fmax(m, sqrt(dx * dx + dy * dy + dz * dz));
        o |= status[(size_t)s * N + i];
    }
    smax[threadIdx.x] = m; sor[threadIdx.x] = o;
    __syncthreads();
    for (int w = blockDim.x / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) { smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + w]); sor[threadIdx.x] |= sor[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int reached = smax[0] < tol ? 1 : 0;
        flags[(size_t)s * 2] = reached; flags[(size_t)s * 2 + 1] = sor[0];
        // the trial of this scene is over (failure_rate.m:112-125): later steps skip it on the device as well
        if (scene_done && (reached || (sor[0] & ~ST_SOLVED))) scene_done[s] = 1;
    }
}

// Missions (dmpc_transition_mission): the stage rule of one scene after the post step of history column k, one block per scene.  Launched in
// stream order behind whatever wrote flags[s] = (reached, OR of status bits) and scene_done[s] for column k: scene_reduce_kernel (k = 0),
// post_step_kernel, or the fused post step of a tiny launch.  The fused post step's per-scene accumulators (post_max / post_or / post_cnt) need
// nothing from here: the wave that counts a scene's last agent of a step exchanges the maximum and the OR for zero and stores zero to the
// count before it writes the verdict, and a scene that is skipped never touches them, so they are zero for every scene when that solve launch
// has ended -- before this kernel starts, whether the scene goes on or not.
//   goals [S][Q][N][3], deadline [S][Q] or null, flags: column k's [S][2], stage / k_start / stage_col: [S], [S], [S][Q]
// stage[s] == Q: the mission of the scene is over (last stage reached, or an agent failed).  Every value the branches test is the same for all
// threads of a block, and the barrier stands in front of them.
__global__ void mission_stage_kernel(int N, int Q, int k, const double *__restrict__ goals, const int *__restrict__ deadline, int *flags,
                                     int *scene_done, int *stage, int *k_start, int *stage_col, double *pf)
{
    const int s = blockIdx.x;
    const int q = stage[s];
    const int reached = flags[(size_t)s * 2], bits = flags[(size_t)s * 2 + 1];
    const int k0 = k_start[s];
    const int dl = (deadline && q < Q) ? deadline[(size_t)s * Q + q] : 0;
    __syncthreads();   // every thread has read the scene's words before thread 0 rewrites them
    if (q >= Q || bits == 0) return;   // over, or column k was never written (the scene had stopped before)
    if (bits & ~ST_SOLVED) {           // a failed agent stops the scene as in dmpc_transition: scene_done stays set, no stage ends
        if (threadIdx.x == 0) stage[s] = Q;
        return;
    }
    if (q == Q - 1) {                  // the last stage ends the trial when it is reached (the verdict stands as the post step wrote it)
        if (reached && threadIdx.x == 0) { stage_col[(size_t)s * Q + q] = k; stage[s] = Q; }
        return;
    }
    if (!(reached || (dl > 0 && k - k0 >= dl))) return;
    // stage q ends on column k: the step that produces column k + 1 is solved with the next goal set; the table is left as it is
    const double *src = goals + ((size_t)s * Q + q + 1) * (size_t)N * 3;
    double *dst = pf + (size_t)s * N * 3;
    for (int i = threadIdx.x; i < N * 3; i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x == 0) {
        stage_col[(size_t)s * Q + q] = k;
        stage[s] = q + 1;
        k_start[s] = k;
        flags[(size_t)s * 2] = 0;      // the host must not read "reached" for an intermediate stage
        scene_done[s] = 0;             // (the status word is clean here: a failed scene returned above and stays done)
    }
}

// Routes (dmpc_transition_route): the waypoint rule of one scene after the post step of history column k, one block per scene, a stride loop over
// its N commanded agents.  Launched where mission_stage_kernel is, in stream order behind whatever wrote flags[s] and scene_done[s] for column k;
// what the comment there says of the fused post step's accumulators holds here as well.
//   wp [S][N][W][3], n_wp [S][N] (1 .. W), x_p [S][N][3]: the states column k recorded, flags: column k's [S][2], cur / since [S][N], wp_col [S][N][W]
// An agent belongs to one thread (i = threadIdx.x + j blockDim.x) in both loops, so its cur / since / wp_col need no barrier of their own; the
// scene's two flag words are read by every thread in front of the barrier and rewritten by thread 0 behind it.  Every value the branches test
// is the same for all threads of a block.  A scene that failed or arrived keeps scene_done set, so none of its later columns is written
// (bits == 0) and its waypoints stay as they were.
__global__ void route_kernel(int N, int W, int k, double cap2, int timeout, const double *__restrict__ wp, const int *__restrict__ n_wp,
                             const double *__restrict__ x_p, int *flags, int *scene_done, int *cur, int *since, int *wp_col, double *pf)
{
#pragma clang fp contract(off)   // the capture test as the host loop computes it: no fused multiply-add
    const int s = blockIdx.x;
    const int bits = flags[(size_t)s * 2 + 1];
    const size_t a0 = (size_t)s * N;
    int last = 1;   // all_last over this thread's agents, BEFORE any switch of this column
    for (int i = threadIdx.x; i < N; i += blockDim.x) last &= cur[a0 + i] == n_wp[a0 + i] - 1;
    __syncthreads();   // every thread has read the scene's words before thread 0 rewrites them
    const int all_last = __syncthreads_and(last);
    if (bits == 0) return;             // column k was never written (the scene had stopped before)
    if (bits & ~ST_SOLVED) return;     // a failed agent stops the scene as in dmpc_transition: scene_done stays set, no waypoint switches
    if (all_last) return;              // every agent flies to its goal: the verdict stands as the post step wrote it (reached ends the trial)
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const size_t ag = a0 + i;
        const int c = cur[ag];
        if (c >= n_wp[ag] - 1) continue;
        const double *w = wp + (ag * W + c) * 3;
        const double dx = x_p[ag * 3] - w[0], dy = x_p[ag * 3 + 1] - w[1], dz = x_p[ag * 3 + 2] - w[2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 < cap2 || (timeout > 0 && k - since[ag] >= timeout))) continue;
        // the agent leaves waypoint c on column k: the step that produces column k + 1 is solved with the next one; the table is left as it is
        wp_col[ag * W + c] = k;
        cur[ag] = c + 1;
        since[ag] = k;
        for (int d = 0; d < 3; ++d) pf[ag * 3 + d] = w[3 + d];
    }
    if (threadIdx.x == 0) {
        flags[(size_t)s * 2] = 0;      // the host must not read "reached" while some agent is not on its last waypoint
        scene_done[s] = 0;             // (the status word is clean here: a failed scene returned above and stays done)
    }
}

// Hold policy (dmpc_transition_hold): between the solve of the step that produces history column k and its post step, over the S * N_cmd
// commanded agents, one wave per 64 of them.  An agent whose status is not exactly ST_SOLVED has failed; while its run of consecutive failures
// is <= max_hold it is HELD: its plan of this step is its previous plan shifted by one entry, with a braking tail appended
//   a_t = clamp(-v[K-1] / h, -alim, alim),  v' = v[K-1] + h a_t,  p' = (p[K-1] + h v[K-1]) + (0.5 h h) a_t        (per axis)
// -- every operation rounded on its own (contraction is switched off in the kernel: the rounded-multiply intrinsics are plain products that
// the compiler would fuse), so that a host loop reproduces the bits.  The previous positions are the agent's
// column of the table the step read (lT [S][3K][N]), the previous v / a rows stand in the OTHER set of the alternating output buffers
// (pv, pa [S][N_cmd][3K]).  The shifted plan goes into the current output rows (the next step's "previous") and into the agent's column of
// lT_next; the working status becomes ST_SOLVED, so that post_step_kernel and mission_stage_kernel take the held plan as a solved one.  An
// agent past its budget keeps its raw status and ends the scene there as in dmpc_transition.
//   run, hold_count, hold_first: [S][N_cmd]; log: [S][N_cmd][KT], column k = the raw status, ST_HELD OR-ed in where the agent was held
// Phase 1 is per lane (one status load; an agent that did not fail stores run = 0 and its log entry); phase 2 visits the wave's held agents
// one after the other (they are rare), lane j < 3K moving entry j of p, v and a: the 45 stores at stride N into lT_next are one store
// instruction of 45 lanes per held agent, as the solvers' output stage writes a column.
enum { ST_HELD = 64 /* = DMPC_ST_HELD; the internal ST_QOVER of the same value never survives a step */ };
__global__ __launch_bounds__(64) void hold_kernel(int total, int N_cmd, int N, int KT, int k, int max_hold, double h, double alim,
                                                  const double *__restrict__ lT, double *__restrict__ lT_next, const double *__restrict__ pv,
                                                  const double *__restrict__ pa, double *__restrict__ p_out, double *__restrict__ v_out,
                                                  double *__restrict__ a_out, int *status, const int *__restrict__ scene_done, int *run, int *log,
                                                  int *hold_count, int *hold_first)
{
#pragma clang fp contract(off)   // the tail as the host loop computes it: no fused multiply-add
    const int lane = (int)threadIdx.x;
    const int first = (int)blockIdx.x * 64;
    const int ag = first + lane;
    bool held = false;
    if (ag < total && (k == 0 || !scene_done[ag / N_cmd])) {   // (k = 0, behind the verdict of the initDMPC column: every status is ST_SOLVED -- run = 0 and the log's first column)
        const int st = status[ag];
        int r = 0, rec = st;
        if (st != ST_SOLVED) {
            r = run[ag] + 1;
            held = r <= max_hold;
            if (held) {
                rec |= ST_HELD;
                hold_count[ag] += 1;
                if (hold_first[ag] < 0) hold_first[ag] = k;
            }
        }
        run[ag] = r;
        log[(size_t)ag * KT + k] = rec;
    }
    unsigned long long m = __ballot(held);
    const double half_hh = (0.5 * h) * h;
    while (m) {   // (wave-uniform)
        const int a = first + (__ffsll((long long)m) - 1);
        m &= m - 1;
        const int s = a / N_cmd, i = a - s * N_cmd;
        if (lane < N3) {
            const size_t col = (size_t)s * N3 * N + i, row = (size_t)a * N3 + lane;
            double pn, vn, an;
            if (lane < N3 - 3) {
                pn = lT[col + (size_t)(lane + 3) * N]; vn = pv[row + 3]; an = pa[row + 3];
            } else {
                const double pl = lT[col + (size_t)lane * N], vl = pv[row];
                an = fmin(fmax(-vl / h, -alim), alim);
                vn = vl + h * an;
                pn = (pl + h * vl) + half_hh * an;
            }
            p_out[row] = pn; v_out[row] = vn; a_out[row] = an;
            lT_next[col + (size_t)lane * N] = pn;
        }
        if (lane == 0) status[a] = ST_SOLVED;
    }
}

}  // namespace dmpc
