// dmpc_launch.hip -- one MPC step on the caller's stream (host code only; part of the single translation unit of dmpc_api.hip).
//
// launch_step is a sequence: plan_step decides (a pure function of the context and the launch's shape: no HIP call, no allocation, no
// write to the context), then five stages allocate and launch what the plan says -- fill_params, build_neighbour_lists, launch_scan,
// launch_order, launch_solve.  Which instantiation of a kernel family a launch uses comes from ONE table per family (solve_kernels_*,
// scan_kernel): the launch, the LDS limits and dmpc_last_solve_kernel read the same entry.

static bool variant_soft(int v)
{
    return v == DMPC_VAR_BOUND || v == DMPC_VAR_BOUND2 || v == DMPC_VAR_ALL3 || v == DMPC_VAR_SOFTALL || v == DMPC_VAR_REPAIR ||
           v == DMPC_VAR_CPP || v == DMPC_VAR_CPP2 || v == DMPC_VAR_CPP1 || v == DMPC_VAR_SOFTALL_C;
}

// row capacity per agent.  Rows live in global scratch (40-64 B each); LDS only holds 4-12 B per row
// (working-set flags, slack value), so the exact worst case is affordable up to a few thousand rows.
// The kernel flags DMPC_ST_CAPACITY if a cap is ever exceeded (never silently truncated).
static int row_capacity(int variant, int N)
{
    const long nb = N > 1 ? N - 1 : 1;
    long want, cap;
    switch (variant) {
    case DMPC_VAR_HARD: want = (long)K * nb; cap = 640; break;
    case DMPC_VAR_SCP: want = (long)K * nb; cap = 4096; break;     // every neighbour at every step of addConstr (up to all k_hor of them), after exact pruning     // every k, neighbours with d < 1 (CollConstrHardDMPC.m:19), after exact pruning
    case DMPC_VAR_ALL3: want = 3 * nb; cap = 384; break;           // three steps x neighbours with d < 3 rmin
    case DMPC_VAR_BOUND: case DMPC_VAR_BOUND2: case DMPC_VAR_ONDEMAND: case DMPC_VAR_CPP: case DMPC_VAR_CPP2: want = nb; cap = 128; break;   // d < 3 rmin only
    default: want = nb; cap = 4096; break;                         // ellip / softall / repair: all N-1 neighbours
    }
    long r = want < cap ? want : cap;
    if (r < 8) r = 8;
    return (int)((r + 1) & ~1L);
}

// Working-set capacity of the first solve launch.  The capacity is a template parameter of the solve kernels: 32 / 48 / 64
// (slack-carrying variants), 48 (slack-free: 45 variables => at most 45 independent active rows, one tier).
// Slack variants, deep launches: 48 slots first -- 17 KB of LDS per wave, still 8 resident agents per CU -- and a second launch
// with 64 for the agents that outgrow them (none at N = 100; 4 in 10^4 at N = 10^4).  Round 1 used 32 slots first: the agents
// that outgrow 32 are exactly the long ones (several retry-ladder levels, many active rows) and re-solving them in a second,
// serialized launch cost more than anything else in the step.  Measured (bench secondaries, 51 200 agents of
// solveSoftDMPCbound): 32/64 tiers 1.38 ms per step, one 64-slot tier (5 agents per CU) 1.07 ms, 48/64 tiers 1.02 ms;
// 512 whole transitions 110 / 107 / 100 ms.  development option tier1_qcap = 32 | 64 selects the other forms (tests cover the 32/64 hand-off).
static int tier1_qcap(const dmpc_ctx *ctx, int variant, int scene_agents)
{
    if (!variant_soft(variant)) return 48;
    const int t1 = ctx->opt.tier1_env;
    if (t1 == 32 || t1 == 48 || t1 == 56 || t1 == 64) return t1;
    // Large scenes: 56 slots first.  Far from its goal an agent saturates most of its 45 acceleration bounds (the crash start appends up
    // to 44 of them), and with a handful of rows and their pins the working set peaks at 48-50 slots: at N = 10^4 (C4) 50-75 agents per
    // step outgrew a 48-slot tier, none needs more than 50 -- and the few that overflow are re-solved from scratch in a second,
    // serialized launch that lasts as long as its slowest agent (0.56 ms of a 2.7 ms step).  56 slots cost 3.6 KB of LDS per agent
    // (5 instead of 6 one-agent workgroups per CU) and take them all: solve 1.81 -> 1.44 ms per step.
    // (round 5: solveSoftDMPCall too, at any scene size -- its agents carry three rows per neighbour, 2-3 % of them outgrow 48 slots, and the second
    // launch that re-solves those from scratch lasted 1.6 ms of a 4.5 ms step of 512 scenes: 3.16 -> 2.17 ms of solve launches per step)
    return (scene_agents >= 1024 || variant == DMPC_VAR_ALL3) ? 56 : 48;
}
// hard: 45 variables => at most 45 independent active rows; 48 leaves room for a numerically near-dependent addition
static int full_qcap(int variant) { return variant_soft(variant) ? QMAX : 48; }

// what follows a solve in a closed loop (post_step_kernel); the step folds it into the solve kernel when the launch is tiny and
// single-tier (StepPlan::fuse_post), and reports that in ctx->post_fused
struct PostStep {
    int KT, k;
    double tol;
    double *xp, *xv, *xa, *pk, *vk, *ak;
    int *flags, *done;
};

// the agents of a launch: columns [c_first, c_first + c_count) of chunk g_local of a table of S scenes x G chunks x C columns
struct StepShape { int S, G, C, g_local, c_first, c_count; };

// what a step reads and writes (device pointers)
struct StepIO {
    const double *lT = nullptr;                                           // [G][S][3K][C] predictions of the previous step
    const double *x_p = nullptr, *x_v = nullptr, *x_a = nullptr, *pf = nullptr;   // [S][c_count][3] states and goals
    double *p_out = nullptr, *v_out = nullptr, *a_out = nullptr;          // [S][c_count][3K]
    double *lT_next = nullptr;                                            // [S][3K][C] or null
    int32_t *status = nullptr, *info = nullptr;
    const int *scene_done = nullptr;   // [S] or null: scenes of a transition that already stopped
    int short_from = 0;                // unequal clusters: chunks from here on hold C-1 agents (dmpc_multigpu.hip)
    const float *lTf = nullptr;        // mixed precision: the fp32 copy of lT the scan reads
    const PostStep *post = nullptr;    // closed loops: the step after the solve, for the launches that can fuse it
    const double *own_prev = nullptr;  // mixed: fp64 predictions of chunk g_local [S][3K][C] when lT is not the full fp64 table
};

// ---------------------------------------------------------------------------------------------
// kernel instantiations: one table per family
// ---------------------------------------------------------------------------------------------

// every kernel of a step but the list builders takes the parameter block alone
static void launch_params_kernel(const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t st, StepParams &P)
{
    void *args[] = {&P};
    (void)hipLaunchKernel(fn, grid, block, args, lds, st);   // (an error surfaces in the step's hipGetLastError)
}

// The solve kernels: the working-set capacity, the own columns of a split inverse factor (ts == qcap: unsplit) and the factor's type are
// template parameters.  These rows are every instantiation the library has: the launch, the LDS limits and dmpc_last_solve_kernel read them, and
// a launch whose key is not here fails.
// (The compiler emits device code in the order this file first names an instantiation.  The sections stand in the order that keeps the code object
// what it was -- one-agent solve kernels, list builders, scan kernels, persistent solve kernels -- which is why the table has two segments.)
struct SolveKernel {
    bool soft; int qcap, ts; bool f32;
    const void *fn;
};
static const SolveKernel solve_kernels_plain[] = {   // one agent per workgroup
    {true, 32, 32, false, (const void *)dmpc_solve_kernel<true, 32>}, {true, 48, 48, false, (const void *)dmpc_solve_kernel<true, 48>},
    {true, 56, 56, false, (const void *)dmpc_solve_kernel<true, 56>}, {true, 64, 64, false, (const void *)dmpc_solve_kernel<true, 64>},
    {false, 48, 48, false, (const void *)dmpc_solve_kernel<false, 48>},
    {true, 64, 64, true, (const void *)dmpc_solve_kernel<true, 64, float>}, {false, 48, 48, true, (const void *)dmpc_solve_kernel<false, 48, float>}};

// the neighbour lists of large scenes
constexpr int GRID_CELLS_DEFAULT = 2;                 // row of plan_lists' cell geometries taken when option grid_cells names none
constexpr size_t GRID_FILL2_LDS_MAX = 128 * 1024;     // dynamic LDS of a grid_fill2_kernel block up to which one scene's grid is built in two launches
struct ListPlan {
    bool build = false;      // lists at all
    bool use_grid = false;   // from the cell grid + distance filter (grid_query_kernel); else the all-pairs box test (nbr_kernel)
    bool fused = false;      // ONE scene: the grid in two launches (grid_prep_kernel, grid_fill2_kernel) instead of five
    bool nbr_major = false;  // the neighbour-major fp32 copy of the table is made
    long cap = 0;            // entries per agent
    double R = 0, Rsel = 0;  // radius of the boxes' test / of the scan's selection
    size_t gq_lds = 0;
    bool close = false;      // the query also leaves the (neighbour, step) pairs inside rmin: the scan tests those instead of walking its list
    GridGeom gg{};
    int ncell = 1, close_cap = 0;   // cells of the grid; close records per agent (the context's default is DevOptions::close_cap)
};
// the cell grid's buffer (carve_grid)
struct GridBuffers {
    int *cnt = nullptr, *maxhalf = nullptr, *start = nullptr, *cell = nullptr, *pos = nullptr;
    f4_t *ent = nullptr;
    size_t n_zero = 0;   // ints zeroed together at the buffer's front: counts and largest half extents
};

// The list builders' kernels that read the prediction table, by the table's type: its fp64 original, or the fp32 copy of mixed precision.
template <typename TT>
static void launch_list_inputs(dmpc_ctx *ctx, const StepShape &sh, const ListPlan &L, const GridBuffers &g, const TT *lT, int short_from, hipStream_t st)
{
    const int total = sh.G * sh.S * sh.C, C = sh.C;
    const size_t tot = (size_t)total * 64;
    const dim3 gA((unsigned)((total + 255) / 256)), gC((unsigned)((tot + 255) / 256)), b(256);
    float *bbox = ctx->bbox.as<float>(), *bbox_nm = ctx->bbox_nm.as<float>(), *lrow = ctx->lrow.as<float>();
    if (L.fused) {   // (grid_prep_kernel makes the boxes and the copy)
        hipLaunchKernelGGL(grid_prep_kernel<TT>, dim3(gA.x + gC.x), b, 0, st, total, C, short_from, L.gg, (int)gA.x, lT, bbox, bbox_nm, lrow, g.cell, g.pos, g.cnt, g.maxhalf);
        return;
    }
    hipLaunchKernelGGL(bbox_kernel<TT>, gA, b, 0, st, total, C, lT, bbox, bbox_nm);
    if (L.nbr_major) hipLaunchKernelGGL(table_nbrmajor_kernel<TT>, gC, b, 0, st, tot, C, lT, lrow, g.cnt, g.n_zero);
}
// Instantiated explicitly, and HERE: the compiler emits the device code of bbox_kernel, table_nbrmajor_kernel and grid_prep_kernel where the host first
// names an instantiation, and the code object keeps its order -- one-agent solve kernels, list builders, scan kernels, persistent solve kernels (see
// solve_kernels_plain) -- only while these two lines stand between the two solve tables.  (That is also why ListPlan stands up here and not with the plan.)
template void launch_list_inputs<float>(dmpc_ctx *, const StepShape &, const ListPlan &, const GridBuffers &, const float *, int, hipStream_t);
template void launch_list_inputs<double>(dmpc_ctx *, const StepShape &, const ListPlan &, const GridBuffers &, const double *, int, hipStream_t);

// The scan kernel by row type, table type and exit: the super-ellipsoid of order 4 (all-neighbour variants) has its own scan kernels,
// without the unconstrained exit.
static const void *scan_kernel(bool soft, bool f32_table, bool fast_exit, bool order4)
{
    static const void *const ord4[2][2] = {   // [fp32 table, then fp64][slack rows, then slack-free]
        {(const void *)dmpc_scan_kernel<true, float, false, true>, (const void *)dmpc_scan_kernel<false, float, false, true>},
        {(const void *)dmpc_scan_kernel<true, double, false, true>, (const void *)dmpc_scan_kernel<false, double, false, true>}};
    static const void *const ord2[2][2][2] = {   // the same, then [with the unconstrained exit, without]
        {{(const void *)dmpc_scan_kernel<true, float, true>, (const void *)dmpc_scan_kernel<true, float, false>}, {(const void *)dmpc_scan_kernel<false, float, true>, (const void *)dmpc_scan_kernel<false, float, false>}},
        {{(const void *)dmpc_scan_kernel<true, double, true>, (const void *)dmpc_scan_kernel<true, double, false>}, {(const void *)dmpc_scan_kernel<false, double, true>, (const void *)dmpc_scan_kernel<false, double, false>}}};
    return order4 ? ord4[!f32_table][!soft] : ord2[!f32_table][!soft][!fast_exit];
}

static const SolveKernel solve_kernels_persist[] = {   // persistent waves
    {true, 64, 64, true, (const void *)dmpc_solve_persist_kernel<true, 64, 64, float>}, {false, 48, 48, true, (const void *)dmpc_solve_persist_kernel<false, 48, 48, float>},
    {true, 32, 32, false, (const void *)dmpc_solve_persist_kernel<true, 32>}, {true, 48, 48, false, (const void *)dmpc_solve_persist_kernel<true, 48>},
    {true, 56, SOFT_TS, false, (const void *)dmpc_solve_persist_kernel<true, 56, SOFT_TS>}, {true, 56, 56, false, (const void *)dmpc_solve_persist_kernel<true, 56>},
    {true, 64, 64, false, (const void *)dmpc_solve_persist_kernel<true, 64>},
    {false, 48, HARD_TS, false, (const void *)dmpc_solve_persist_kernel<false, 48, HARD_TS>}, {false, 48, 48, false, (const void *)dmpc_solve_persist_kernel<false, 48>}};

static const SolveKernel *find_solve_kernel(bool persistent, bool soft, int qcap, int ts, bool f32)
{
    const SolveKernel *tab = persistent ? solve_kernels_persist : solve_kernels_plain;
    const size_t n = persistent ? sizeof(solve_kernels_persist) / sizeof(SolveKernel) : sizeof(solve_kernels_plain) / sizeof(SolveKernel);
    for (size_t i = 0; i < n; ++i)
        if (tab[i].soft == soft && tab[i].qcap == qcap && tab[i].ts == ts && tab[i].f32 == f32) return &tab[i];
    return nullptr;
}
// as the profiler prints it (bench.py looks it up; dmpc_last_solve_kernel)
static std::string solve_kernel_name(bool persistent, const SolveKernel &k)
{
    return std::string(persistent ? "dmpc_solve_persist_kernel<" : "dmpc_solve_kernel<") + (k.soft ? "true, " : "false, ") + std::to_string(k.qcap) +
           (persistent ? ", " + std::to_string(k.ts) : std::string()) + (k.f32 ? ", float>" : ", double>");
}
// the dynamic-LDS limit of every one-agent / every persistent solve kernel
static int raise_solve_lds(dmpc_ctx *ctx, bool persistent, int bytes)
{
    const SolveKernel *tab = persistent ? solve_kernels_persist : solve_kernels_plain;
    const size_t n = persistent ? sizeof(solve_kernels_persist) / sizeof(SolveKernel) : sizeof(solve_kernels_plain) / sizeof(SolveKernel);
    for (size_t i = 0; i < n; ++i) HIPCHK(ctx, hipFuncSetAttribute(tab[i].fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------

// one solve launch of the general solver
struct TierPlan {
    int qcap = 0;              // working-set capacity (template parameter of the kernel)
    int tsplit = 0;            // persistent form: own columns of the inverse factor per wave (0: all qcap of them)
    int n_ext = 0;             // persistent form with a split factor: extensions in the workgroup's pool
    int pw = 0;                // persistent form: waves per workgroup
    size_t per_wave_lds = 0;   // persistent form: bytes per wave behind the shared tables
    size_t lds_plain = 0;      // one agent per workgroup: bytes of the workgroup
    size_t lds_persist = 0;    // persistent form: bytes of the workgroup
    bool persistent = false;
    int wgs = 0;               // persistent form: workgroups
    int queue_chunk = 0;       // persistent form: positions per ticket of the queue's light bulk
};

struct StepPlan {
    StepShape sh{};
    int total = 0;            // agents of the launch
    int nrmax = 0;            // row capacity per agent
    bool soft = false, f32t = false, tiny = false, heavy_agents = false, big_soft = false, shallow = false, deep = false;
    bool two_tier = false, reduced = false, run_order = false, scp = false, finite_radius = false;
    int fast_exit = 0, crash_min = 0;
    bool fuse_post = false;   // a closed loop's post step goes into the solve kernel (when the caller hands one in)
    bool zero_counters = false;
    ListPlan lists;
    size_t scan_lds = 0;      // per scan wave
    int scan_waves = 1;       // scan waves per workgroup
    int order_slices = 0;     // workgroups of the order kernel
    bool t2_list = false;     // tier 1 leaves the list of the agents that outgrew it for a persistent tier 2
    TierPlan tier[2];
};

// persistent waves (one workgroup per CU, shared tables, agents claimed from a queue): how many fit next to the shared tables
static TierPlan plan_tier(const dmpc_ctx *ctx, const StepPlan &pl, int qcap)
{
    const size_t LDS_CU = 160 * 1024;
    const DevOptions &o = ctx->opt;
    TierPlan t;
    t.qcap = qcap;
    t.lds_plain = solve_lds_bytes(pl.nrmax, pl.soft, qcap, false, 0, pl.f32t) + (size_t)o.lds_pad_kb * 1024;
    // Slack-free variants (round 4): split T -- HARD_TS columns of the inverse factor in every wave's block, the rest of the 48 in
    // extensions that the waves of a workgroup take from a pool when an agent's working set outgrows them (dmpc_solve.hip) -- so that
    // twelve waves (three per SIMD: what 168 registers per lane allow) share a CU's LDS instead of nine.
    // Slack variants, 56-slot tier of large scenes (round 5): the same split with 48 own columns -- the eight columns beyond them (3.6 KB) come from
    // the pool for the 2 % of the agents whose working set outgrows 48 slots -- so that SEVEN waves share a CU where five one-agent workgroups
    // (30 KB each, their own copy of the tables) or six unsplit persistent waves did: the 10^4-agent scene is bound by its work per wave slot
    // (four / five resident agents per CU: 1.03 / 0.88 ms, option lds_pad_kb).
    const bool split = !o.no_split_t && !pl.f32t;
    t.tsplit = pl.soft ? ((qcap == 56 && split) ? SOFT_TS : 0) : (split ? HARD_TS : 0);
    t.per_wave_lds = solve_lds_bytes(pl.nrmax, pl.soft, qcap, true, t.tsplit, pl.f32t);
    int pw = (int)((LDS_CU - PERSIST_TABLE_BYTES) / t.per_wave_lds);
#ifdef DMPC_DEV_PW   // development builds: fewer persistent waves per CU (how much does a long agent lose to the wave it shares a SIMD with?)
    if (pw > DMPC_DEV_PW) pw = DMPC_DEV_PW;
#endif
    const int cap = pl.soft ? 8 : ((t.tsplit || pl.f32t) ? HARD_PW : 9);   // waves per workgroup the kernels are compiled for (launch bounds)
    pw = pw > cap ? cap : pw;
    if (t.tsplit) {   // the extensions need room too: at least a third as many as waves (3 % of the headline launch's agents need one, for 15 % of its iterations)
        const size_t eb = (size_t)ext_doubles(qcap, t.tsplit) * 8;
        for (;; --pw) {
            t.n_ext = (int)((LDS_CU - PERSIST_TABLE_BYTES - EXT_PAD_BYTES - (size_t)pw * t.per_wave_lds) / eb);
            if (t.n_ext > 31) t.n_ext = 31;
            if (pw < 2 || 3 * t.n_ext >= pw) break;
        }
        if (o.ext_cap > 0 && t.n_ext > o.ext_cap) t.n_ext = o.ext_cap;
    }
    t.pw = pw;
    if (pw >= 2 && ctx->num_cu >= 1) {   // (the only shape the persistent form is launched in)
        t.lds_persist = PERSIST_TABLE_BYTES + (size_t)pw * t.per_wave_lds + (t.tsplit ? (size_t)t.n_ext * ext_doubles(qcap, t.tsplit) * 8 + EXT_PAD_BYTES : 0);
        t.wgs = (pl.total + pw - 1) / pw;
        if (t.wgs > ctx->num_cu) t.wgs = ctx->num_cu;
        // tickets of the queue's light bulk: single positions where a wave solves few, heavy agents (fewer than 12 per wave, or solveSoftDMPCall)
        t.queue_chunk = o.queue_chunk > 0 ? o.queue_chunk : ((pl.total < 12 * t.wgs * pw || ctx->prm.variant == DMPC_VAR_ALL3) ? 1 : 2);
    }
    return t;
}

static ListPlan plan_lists(const dmpc_ctx *ctx, const StepPlan &pl)
{
    const dmpc_params &p = ctx->prm;
    const DevOptions &o = ctx->opt;
    const StepShape &sh = pl.sh;
    ListPlan L;
    // neighbour culling boxes (worth it once a scene has more than a few chunks of neighbours)
    // only for the variants whose scan and rows have a finite neighbour radius (d < 1 for the hard rows, d < 3 rmin for the
    // near-neighbour selections); solveEllipDMPC / solveSoftDMPC / solveSoftDMPCrepair take every neighbour
    L.build = sh.G * sh.C >= o.cull_min && !o.no_cull && pl.finite_radius;
    if (!L.build) return L;
    // neighbour lists from the boxes (nbr_kernel): up to 4096 entries per agent, within 1 GB of scratch
    const size_t agents = (size_t)pl.total;
    L.cap = ((long)sh.G * sh.C + 63) & ~63L;
    if (L.cap > 4096) L.cap = 4096;
    while (L.cap > 256 && agents * (size_t)L.cap * 4 > ((size_t)1 << 30)) L.cap >>= 1;
    if (o.list_cap > 0 && (((long)o.list_cap + 63) & ~63L) < L.cap) L.cap = ((long)o.list_cap + 63) & ~63L;
    L.Rsel = (p.variant == DMPC_VAR_HARD) ? 1.0 : 3.0 * p.rmin;
    L.R = L.Rsel * 1.0001 + 1e-4;   // a little more than the scan's radius: conservative in fp32 too
    // round 4: lists from a cell grid, filtered by the fp32 distance test (grid_query_kernel); the all-pairs box test of round 3 stays
    // behind option nbr_grid = 0 (A/B runs, tests) and for scenes whose bitmap would not fit a wave's LDS
    // (with the close pairs' staging list, when the variant's scan walks its list for them and the option is on)
    const bool close_want = p.variant != DMPC_VAR_HARD && o.close_pairs && o.close_cap > 0;
    L.close_cap = close_want ? (o.close_cap > 4096 ? 4096 : o.close_cap) : 0;
    L.gq_lds = grid_query_lds(sh.G * sh.C, L.close_cap);
    // (from grid_min agents per scene on: in a scene of a few hundred agents the reach of a query covers most of the workspace and the
    // all-pairs test with the neighbours' boxes as scalar operands is the cheaper pass -- tools/gpu_grid_min_ab.py, 102 400 agents, scan
    // side all-pairs / grid: hard rows 400 agents per scene 0.81 / 0.81 ms, 800: 1.07 / 0.91, 1 600: 1.42 / 1.06, 3 200: 1.92 / 1.24;
    // solveSoftDMPCbound 400: 0.62 / 0.66, 800: 0.71 / 0.69, 1 600: 0.84 / 0.73, 3 200: 1.04 / 0.81.  A rank that queries ONE chunk of
    // 8 x 100 agents per scene still bins all 800: 0.87 against 0.64 ms, `bench.py --emulate-gpus 8 --debug-option grid_min=512`)
    // (one chunk of which at least half is queried -- the commanded agents of a scene with uncommanded vehicles -- counts as the whole scene: binning
    // all C columns is then at most twice the query's own share; grid_min_part was fitted on a rank's chunk, an eighth of the scene.  Not measured.)
    const int grid_from = (sh.c_count == sh.G * sh.C || (sh.G == 1 && 2L * sh.c_count >= (long)sh.C)) ? o.grid_min : o.grid_min_part;
    L.use_grid = o.nbr_grid && sh.G * sh.C >= grid_from && L.gq_lds <= 64 * 1024;
    L.nbr_major = p.variant != DMPC_VAR_HARD || L.use_grid;
    L.close = L.use_grid && close_want;
    if (!L.close) L.close_cap = 0;
    if (!L.use_grid) return L;
    // Cells, in units of (R, R, R c) -- c: the metric's z scale -- and the most cells an axis gets: decided here alone, the kernels take
    // whatever GridGeom says.  The cells of a run along x are contiguous in the entry array, so fine x cells cost the query nothing; every
    // (y, z) cell row in reach is one run of its candidate sequence, and since round 5 the runs of a query are one sequence (64 run bounds
    // per batch, one fetch), so finer y and z cells cost a few more run bounds and save the candidates of the cells' rounding: per agent and
    // MPC step 2 / 6 / 10 of the 10^4-agent scene 1 115 / 1 855 / 2 621 candidates in geometry 0, 810 / 1 432 / 2 074 in geometry 2
    // (DESIGN.md section 7 has the measured table).  Option grid_cells selects the row; the default is the one that measured best.
    // A finer grid is taken only while it has no more cells than geometry 0 can have (32^3): no buffer, no prefix pass over the cells
    // grows beyond what it could be before.
    static const struct { double f[3]; int cap; } geoms[] = {
        {{1.0, 1.5, 1.5}, 32},    // 0: rounds 4-6
        {{0.5, 1.5, 1.5}, 64},    // 1: finer along x only
        {{0.5, 1.0, 1.0}, 64},    // 2
        {{0.5, 1.0, 0.5}, 64}};   // 3: finer in z (above the fused build's limit at N = 10^4)
    constexpr int n_geoms = (int)(sizeof(geoms) / sizeof(geoms[0]));
    auto cells = [&](int which) {
        L.ncell = 1;
        for (int a = 0; a < 3; ++a) {
            const double span = p.pmax[a] - p.pmin[a];
            const double cell = geoms[which].f[a] * L.R * (a == 2 ? p.c : 1.0);
            int n = (int)(span / cell);
            n = n < 1 ? 1 : (n > geoms[which].cap ? geoms[which].cap : n);
            L.gg.n[a] = n; L.gg.org[a] = (float)p.pmin[a]; L.gg.inv[a] = (float)(n / (span > 0 ? span : 1.0));
            L.ncell *= n;
        }
    };
    cells((o.grid_cells >= 0 && o.grid_cells < n_geoms) ? o.grid_cells : GRID_CELLS_DEFAULT);
    if (L.ncell > 32 * 32 * 32) cells(0);
    // (every block of grid_fill2_kernel keeps the prefix of all NSEG x (ncell + 1) counts in its LDS: up to GRID_FILL2_LDS_MAX = 128 KB of a
    // CU's 160 -- 10 921 cells; the 8 200 of geometry 2 at N = 10^4 take 96 KB, one block per CU, 40 blocks -- above it the five kernels)
    L.fused = sh.S == 1 && o.prep_fuse && (size_t)NSEG * (L.ncell + 1) * 4 <= GRID_FILL2_LDS_MAX;
    return L;
}

// Everything a step decides, from the context (parameters, precision, development options, CU count) and the launch's shape alone.
static StepPlan plan_step(const dmpc_ctx *ctx, const StepShape &sh)
{
    const dmpc_params &p = ctx->prm;
    const DevOptions &o = ctx->opt;
    const int S = sh.S, G = sh.G, C = sh.C, c_count = sh.c_count;
    StepPlan pl;
    pl.sh = sh;
    pl.total = S * c_count;
    pl.soft = variant_soft(p.variant);
    pl.scp = p.variant == DMPC_VAR_SCP;
    pl.nrmax = row_capacity(p.variant, G * C);
    // (not for solveHardDMPC: rows at every horizon step, 3 % of the agents would qualify and every scan would pay for the test)
    pl.fast_exit = (o.no_fast_exit || p.variant == DMPC_VAR_HARD || p.variant == DMPC_VAR_SCP || p.order == 4) ? 0 : 1;
    // measured: the crash start pays for the slack-carrying variants (C4, N = 10^4: solve launch -16 %) and costs on solveHardDMPC
    // (C2: -16 % throughput: with rows at every horizon step the bounds violated at the unconstrained minimiser are a poor guess)
    pl.crash_min = (pl.soft || o.crash_any) ? o.crash_min : 0;
    // tiny launches (a scene or a few, every agent resident at once: bound by the latency of their slowest agent, LDS is no
    // constraint) solve with the full working-set capacity in one launch; larger ones use the first tier and re-solve the few
    // agents that outgrow it (the smaller footprint also puts 6 instead of 4 one-agent workgroups on a CU: 512 transitions
    // in two halves of 25 600 agents 75 -> 63 ms); from `shallow` up the first tier runs as persistent waves
    const long ncu = ctx->num_cu > 0 ? ctx->num_cu : 256;
    pl.tiny = (long)S * c_count < 8L * ncu && !o.force_persist && !o.tier1_env;
    // (round 4, with the fitted launch-order key: launches whose agents are HEAVY -- the all-neighbour variants in scenes of >= 200 agents, every
    // violating agent carries a row per neighbour: C3 16 x 1 000 agents 37 iterations each, C5 64 x 200 agents 29 -- are throughput-bound from a
    // quarter of that depth on: persistent waves 1.50 / 0.89 ms against 1.77 / 1.05.  Light launches of the same depth -- 128 scenes x 100 agents
    // of solveSoftDMPC at MPC step 12, one iteration per agent -- stay with one agent per workgroup: 0.21 against 0.25 ms.)
    pl.heavy_agents = (p.variant == DMPC_VAR_SOFTALL || p.variant == DMPC_VAR_SOFTALL_C || p.variant == DMPC_VAR_REPAIR || p.variant == DMPC_VAR_ELLIP || p.variant == DMPC_VAR_CPP1) && G * C >= 200;
    // (crossover, agents per launch: C3 4 000: 0.72 / 0.71 ms, 8 000: 1.06 / 0.96; C5 3 200: 0.37 / 0.47, 6 400: 0.59 / 0.61 -- one agent per workgroup / persistent)
    // (round 5: the slack variants in LARGE scenes -- the 56-slot tier, agents of ~100 us each -- are bound by their work per wave slot: persistent
    // waves with the split factor, seven per CU, from two launches' worth of one-agent workgroups on)
    pl.f32t = (ctx->precision & DMPC_PREC_F32FACTOR) != 0 && p.variant != DMPC_VAR_ALL3;   // (solveSoftDMPCall keeps the fp64 factor under every precision)
    pl.big_soft = pl.soft && G * C >= 1024 && !o.no_split_t && !pl.f32t && !ctx->single_tier && !o.tier1_env;
    pl.shallow = (long)S * c_count < (pl.big_soft ? 8L : (pl.heavy_agents ? 28L : 128L)) * ncu && !o.force_persist && !o.tier1_env;
    // fp32 inverse factor: one tier with the full capacity, no split T.  Not for solveSoftDMPCall: its three nearly parallel rows per neighbour
    // need the fp64 factor (sweep of round 4: 1 % of its agent-steps ended on another ladder level) -- that variant keeps it whatever the context says.
    const int q1 = (ctx->single_tier || pl.tiny || pl.f32t) ? full_qcap(p.variant) : tier1_qcap(ctx, p.variant, G * C), q2 = full_qcap(p.variant);
    pl.two_tier = q1 < q2;
    pl.fuse_post = pl.tiny && !pl.two_tier && sh.g_local == 0 && G == 1 && !o.no_fuse && !pl.scp;
    pl.finite_radius = p.variant == DMPC_VAR_HARD || p.variant == DMPC_VAR_BOUND || p.variant == DMPC_VAR_BOUND2 ||
                       p.variant == DMPC_VAR_ALL3 || p.variant == DMPC_VAR_ONDEMAND || p.variant == DMPC_VAR_CPP ||
                       p.variant == DMPC_VAR_CPP2;
    pl.lists = plan_lists(ctx, pl);
    // the scan: several independent waves per workgroup (fewer workgroups to dispatch), as many as fit the default 64 KB of
    // dynamic LDS (the neighbour list of large scenes can take 37 KB per wave)
    pl.scan_lds = scan_lds_bytes();
    pl.scan_waves = SCAN_WAVES_PER_WG;
    while (pl.scan_waves > 1 && pl.scan_lds * pl.scan_waves > 64 * 1024) pl.scan_waves >>= 1;
    // heaviest-first launch order for the solve phase (key left by the scan in hdr[7]).  Tiny launches do not need it.
    pl.run_order = !pl.scp && ctx->forced_n != pl.total && pl.total >= 512 && !o.no_lpt;
    // (slices: the kernel is a chain of dependent memory round trips per thread -- 8 workgroups of 1024 threads took 20 us for 51 200
    // agents, six agents per thread one after the other; with one agent per thread 7 us: headline 52.3 -> 53.2 M solves/s)
    pl.order_slices = o.order_slices > 0 ? o.order_slices : (pl.total >= 65536 ? 64 : (pl.total >= 1024 ? pl.total / 1024 : 1));
    if ((pl.total + pl.order_slices - 1) / pl.order_slices > 24576) pl.order_slices = (pl.total + 24575) / 24576;   // (a slice's keys live in LDS, 2 bytes each next to the histograms: at most 48 KB of them)
    // the reduced solver (dmpc_rsolve.hip) takes solveSoftDMPCbound / bound2 and DMPC::solveQPv2 in every launch form: which kernel solves an agent must not depend on how deep the launch is
    pl.reduced = o.reduced_solver && (p.variant == DMPC_VAR_BOUND || p.variant == DMPC_VAR_BOUND2 || p.variant == DMPC_VAR_CPP || p.variant == DMPC_VAR_CPP2) && !pl.f32t && ctx->num_cu >= 1;   // the variants with slack rows on ONE horizon step
    // queue heads of the persistent solve launches, tier-2 count, live bound: zeroed by the scan kernel (a memset is a launch of its own, 5 us)
    pl.zero_counters = !pl.scp && (!pl.tiny || pl.run_order || pl.reduced);
    pl.tier[0] = plan_tier(ctx, pl, q1);
    pl.tier[1] = plan_tier(ctx, pl, q2);
    const int pw1 = pl.tier[0].pw, pw2 = pl.tier[1].pw;
    // Measured on C2 (hard, 100 agents/scene): persistent waves win once the launch is deep enough to be
    // throughput-bound (+6 % at 102 400 agents: 8 instead of 7 resident agents per CU), while short launches are
    // bound by their single slowest agent, which runs ~4 % faster in the leaner one-agent-per-workgroup kernel.
    pl.deep = !pl.shallow && (pl.big_soft || (long)S * c_count >= (pl.heavy_agents ? 28L : 16L * (pw1 > 0 ? pw1 : 1)) * ctx->num_cu);
    const bool can_persist[2] = {!o.no_persist && pw1 >= 2 && ctx->num_cu >= 1, !o.no_persist && pw2 >= 2 && ctx->num_cu >= 1};
    // tier 2 as persistent waves over the flagged list (nearly always empty: the launch then costs a few microseconds
    // instead of one workgroup per agent just to find out that there is nothing to do)
    pl.t2_list = !pl.reduced && pl.two_tier && !pl.tiny && can_persist[1];
    // phase 1: persistent waves when the launch is deep and at least two waves fit next to the shared tables; otherwise one agent per workgroup.
    // Behind the reduced solver the general one runs once, with its full capacity (tier[1]), over the list of the agents handed over.
    pl.tier[0].persistent = !pl.reduced && (pl.deep || o.force_persist) && can_persist[0];
    pl.tier[1].persistent = pl.reduced ? can_persist[1] : pl.t2_list;
    return pl;
}

// ---------------------------------------------------------------------------------------------
// the stages
// ---------------------------------------------------------------------------------------------

// the parameter block zeroed, and the part of it that a context's parameters, tables and hsum decide alone (every launch of the scan family starts
// from it: a step's, and dmpc_rows_one's single wave)
static void fill_constants(const dmpc_ctx *ctx, StepParams &P)
{
    const dmpc_params &p = ctx->prm;
    memset(&P, 0, sizeof(P));
    P.variant = p.variant;
    P.max_tries = p.max_tries;
    P.ell_order = p.order;
    P.h = p.h; P.rmin = p.rmin; P.e1z = 1.0 / p.c; P.e2z = p.order == 4 ? 1.0 / (p.c * p.c * p.c * p.c) : 1.0 / (p.c * p.c);   // E1 = E^-1, E2 = E^-order
    if (p.variant == DMPC_VAR_SCP) { P.e1z = 1.0; P.e2z = 1.0; }   // solveDMPC: plain Euclidean norm (CheckCollDMPC.m:6, CollConstrDMPC.m:12-13)
    P.alim = p.alim; P.Q1 = p.Q1; P.S1 = p.S1; P.term = p.term;
    P.Qfar = p.Qfar > 0 ? p.Qfar : 1000.0; P.Qnear = p.Qnear > 0 ? p.Qnear : 10000.0; P.Sfree = p.Sfree > 0 ? p.Sfree : 10.0;
    for (int d = 0; d < 3; ++d) { P.pmin[d] = p.pmin[d]; P.pmax[d] = p.pmax[d]; }
    P.tables = ctx->d_tables.as<double>();
    for (int i = 0; i < 3; ++i) P.hsum[i] = ctx->hsum[i];
    P.scp_tol = p.tol;
}

// the parameter block of a step: the constant part, the launch's shape and arrays, the row scratch, and a closed loop's post step when the launch fuses it
static int fill_params(dmpc_ctx *ctx, const StepPlan &pl, const StepIO &io, StepParams &P, hipStream_t st)
{
    const DevOptions &o = ctx->opt;
    const StepShape &sh = pl.sh;
    fill_constants(ctx, P);
    P.S = sh.S; P.G = sh.G; P.C = sh.C; P.g_local = sh.g_local;
    P.c_first = sh.c_first; P.c_count = sh.c_count;
    P.nrmax = pl.nrmax;
    if (ctx->prm.variant == DMPC_VAR_HARD && (sh.G > 256 || sh.C >= (1 << 20)))   // packing of the scan's candidate list
        FAIL(ctx, "solveHardDMPC scan: at most 256 chunks of fewer than 2^20 agents");
    // mixed precision: the scan reads the fp32 copy lTf of the table; lT (fp64, chunk g_local) is the solve's fallback
    P.lT = io.lTf ? (const double *)io.lTf : io.lT;
    P.own_prev = io.lTf ? (io.own_prev ? io.own_prev : io.lT + (size_t)sh.g_local * sh.S * N3 * sh.C) : nullptr;
    P.x_p = io.x_p; P.x_v = io.x_v; P.x_a = io.x_a; P.pf = io.pf;
    P.p_out = io.p_out; P.v_out = io.v_out; P.a_out = io.a_out; P.lT_next = io.lT_next;
    P.status = io.status; P.info = io.info;
    {
        const size_t agents = (size_t)pl.total;
        if (ctx->rowbuf.ensure(agents * P.nrmax * (pl.soft ? 7 : 4) * 8) || ctx->rowkc.ensure(agents * P.nrmax * 4) ||
            ctx->hdr.ensure(agents * 8 * 4) || ctx->order.ensure(agents * 4) || ctx->counter.ensure(16) || ctx->flag_list.ensure(agents * 4))
            FAIL(ctx, "device allocation failed (row scratch)");
        P.rowbuf = ctx->rowbuf.as<double>(); P.rowkc = ctx->rowkc.as<int>(); P.hdr = ctx->hdr.as<int>();
    }
    P.dbg = ctx->dbg.as<double>(); P.dbg_agent = ctx->dbg_agent; P.dbg_cap = ctx->dbg_cap;
    P.iter_cap = o.iter_cap;
    P.rsolve_cap = o.rsolve_cap;
    P.dep_tol_f32 = std::pow(10.0, -(double)o.f32_dep_exp);
    P.no_level_check = o.no_level_check;
    P.no_level_skip = o.no_level_skip;
    P.fast_exit = pl.fast_exit;
    P.crash_min = pl.crash_min;
    P.pivot_explore = o.pivot_explore;
    ctx->post_fused = 0;
    if (io.post && pl.fuse_post) {
        const PostStep *post = io.post;
        const int S = sh.S;
        if (ctx->post_acc.ensure((size_t)S * 16 + 64)) FAIL(ctx, "device allocation failed (post-step accumulators)");
        if (ctx->post_acc_S != S) {   // zero once per batch shape; the last wave of a scene leaves them zeroed again
            HIPCHK(ctx, hipMemsetAsync(ctx->post_acc.p, 0, (size_t)S * 16 + 64, st));
            ctx->post_acc_S = S;
        }
        P.post_on = 1; P.post_KT = post->KT; P.post_k = post->k; P.post_tol = post->tol;
        P.post_xp = post->xp; P.post_xv = post->xv; P.post_xa = post->xa; P.post_pk = post->pk; P.post_vk = post->vk; P.post_ak = post->ak;
        P.post_flags = post->flags; P.post_done = post->done;
        P.post_max = ctx->post_acc.as<unsigned long long>();
        P.post_or = (int *)(ctx->post_acc.as<unsigned long long>() + S); P.post_cnt = P.post_or + S;
        ctx->post_fused = 1;
    }
    P.scene_done = io.scene_done;
    P.short_from = io.short_from;   // unequal clusters: chunks from here on hold C-1 agents (dmpc_multigpu.hip)
    P.zero4 = pl.zero_counters ? ctx->counter.as<int>() : nullptr;
    // the one-agent-per-workgroup solve kernels' LDS limit covers both tiers
    const size_t ldsmax = std::max(pl.tier[0].lds_plain, pl.tier[1].lds_plain);
    if (o.lds_pad_kb < 0 || ldsmax > 160 * 1024) FAIL(ctx, "development option lds_pad_kb: the solve workgroup's LDS block would exceed the CU's 160 KB");
    if ((int)ldsmax > ctx->max_lds_set) {
        if (raise_solve_lds(ctx, false, (int)ldsmax)) return -1;
        ctx->max_lds_set = (int)ldsmax;
    }
    return 0;
}

// ctx->grid carved for a plan's cell grid; true: the allocation failed.  One grid per third of the horizon (keyed by the centre of that segment's box:
// a third of the extent of the whole horizon's).  Ints, in this order: [S][3][ncell] counts, [S][3][3] largest half extents (zeroed together),
// [S][3][ncell + 1] starts, [3][G S C] cells, [3][G S C] positions within the cell (the two-launch build); behind them, 32-byte aligned, the entry
// records: two arrays [S][3][G C] of 16-byte halves.
static bool carve_grid(dmpc_ctx *ctx, const StepShape &sh, const ListPlan &L, GridBuffers &g)
{
    const size_t total = (size_t)sh.G * sh.S * sh.C, grids = (size_t)sh.S * NSEG;
    const size_t n_cnt = grids * L.ncell, n_mh = grids * 3, n_st = grids * ((size_t)L.ncell + 1);
    const size_t n_hd = (n_cnt + n_mh + n_st + 2 * NSEG * total + 7) & ~(size_t)7;
    if (ctx->grid.ensure((n_hd + 8 * NSEG * total) * 4)) return true;
    g.cnt = ctx->grid.as<int>(); g.maxhalf = g.cnt + n_cnt; g.start = g.maxhalf + n_mh; g.cell = g.start + n_st; g.pos = g.cell + NSEG * total;
    g.ent = (f4_t *)(g.cnt + n_hd);
    g.n_zero = n_cnt + n_mh;
    return false;
}

// neighbour lists of large scenes: segment boxes, the neighbour-major copy of the table, the cell grid (five kernels, or two for one
// scene), and the lists themselves from the grid query or the all-pairs box test
static int build_neighbour_lists(dmpc_ctx *ctx, const StepPlan &pl, const StepIO &io, StepParams &P, hipStream_t st)
{
    const ListPlan &L = pl.lists;
    if (!L.build) return 0;
    ctx->lists_built.S = 0; ctx->lists_built.kept = false;   // (nothing to read until this build is through)
    const dmpc_params &p = ctx->prm;
    const int S = pl.sh.S, G = pl.sh.G, C = pl.sh.C, g_local = pl.sh.g_local, c_first = pl.sh.c_first, c_count = pl.sh.c_count;
    const int total = G * S * C, short_from = io.short_from;
    if (ctx->bbox.ensure((size_t)total * 6 * NSEG * 4) || ctx->bbox_nm.ensure((size_t)total * NBOX_NM * 4)) FAIL(ctx, "device allocation failed (bbox)");
    if (C >= (1 << 20) || G > 2047)   // a list entry packs (chunk << 20) | column into an int
        FAIL(ctx, "neighbour lists: at most 2047 chunks of fewer than 2^20 agents");
    const size_t agents = (size_t)pl.total;
    if (ctx->nbr_list.ensure(agents * (size_t)L.cap * 4) || ctx->nbr_cnt.ensure(agents * 4 * NBR_PARTS)) FAIL(ctx, "device allocation failed (neighbour lists)");
    // (grid geometry and buffer first: the counters are zeroed by the neighbour-major copy kernel, which runs anyway -- a memset of an odd
    // size is two fill launches, 9 us)
    GridBuffers g;
    if (L.use_grid && carve_grid(ctx, pl.sh, L, g)) FAIL(ctx, "device allocation failed (neighbour grid)");
    if (L.nbr_major) {   // neighbour-major fp32 copy of the table: the list walk of the per-step distance scan, the distance test of the grid query
        if (ctx->lrow.ensure((size_t)total * 64 * 4)) FAIL(ctx, "device allocation failed (neighbour-major table)");
        if (p.variant != DMPC_VAR_HARD) P.lrow = ctx->lrow.p;
    }
    if (L.fused) {
        // the counters are zero when the last scan launch left them so (for this buffer and size); a memset otherwise (first step, another batch shape in between)
        // (n_zero follows the cell count: up to 3 x 32^3 + 9, seventeen bits -- multiplied through the word, not shifted out of it)
        const unsigned long long key = (unsigned long long)(size_t)g.cnt ^ ((unsigned long long)g.n_zero * 0x9E3779B97F4A7C15ull) ^ ((unsigned long long)total << 20);
        if (!ctx->grid_clean || ctx->grid_clean_key != key) HIPCHK(ctx, hipMemsetAsync(g.cnt, 0, g.n_zero * 4, st));
        ctx->grid_clean = false; ctx->grid_clean_key = key;
        P.gzero = g.cnt; P.gzero_n = (int)g.n_zero;
    } else if (L.use_grid)
        ctx->grid_clean = false;
    if (io.lTf) launch_list_inputs(ctx, pl.sh, L, g, io.lTf, short_from, st);
    else launch_list_inputs(ctx, pl.sh, L, g, io.lT, short_from, st);
    if (L.fused) {
        const size_t lds_fill = (size_t)NSEG * (L.ncell + 1) * 4;
        if ((int)lds_fill > ctx->max_lds_fill2) {   // (the limit of a kernel's dynamic LDS is 64 KB until it is raised)
            HIPCHK(ctx, hipFuncSetAttribute((const void *)grid_fill2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fill));
            ctx->max_lds_fill2 = (int)lds_fill;
        }
        hipLaunchKernelGGL(grid_fill2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), lds_fill, st, total, C, L.ncell, (float)(1.0 / p.c), (const int *)g.cell, (const int *)g.pos, (const int *)g.cnt, g.start, (const float *)ctx->lrow.as<float>(), g.ent);
    } else if (L.use_grid) {
        hipLaunchKernelGGL(grid_bin_kernel, dim3((unsigned)((total + 255) / 256), NSEG), dim3(256), 0, st, total, S, C, short_from, L.gg, (const float *)ctx->bbox_nm.as<float>(), g.cell, g.cnt, g.maxhalf);
        hipLaunchKernelGGL(grid_scan_kernel, dim3((unsigned)(S * NSEG)), dim3(1024), 0, st, L.ncell, g.cnt, g.start);
        hipLaunchKernelGGL(grid_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, S, C, L.ncell, (float)(1.0 / p.c), (const int *)g.cell, g.cnt, (const int *)g.start, (const float *)ctx->lrow.as<float>(), g.ent);
    }
    if (L.use_grid && ctx->lists_built.armed) {   // (dmpc_debug_read_grid: the half extents as the build left them)
        if (ctx->maxhalf_kept.ensure((size_t)S * NSEG * 3 * 4)) FAIL(ctx, "device allocation failed (neighbour grid)");
        HIPCHK(ctx, hipMemcpyAsync(ctx->maxhalf_kept.p, g.maxhalf, (size_t)S * NSEG * 3 * 4, hipMemcpyDeviceToDevice, st));
        ctx->lists_built.kept = true;
    }
    if (L.close && (ctx->close_list.ensure(agents * (size_t)L.close_cap * 8) || ctx->close_cnt.ensure(agents * 4))) FAIL(ctx, "device allocation failed (close pairs)");
    if (L.use_grid) {
        hipLaunchKernelGGL(grid_query_kernel, dim3((unsigned)pl.total), dim3(64 * GQ_WAVES), L.gq_lds, st, S, G, C, g_local, c_first, c_count, L.gg,
                           (float)L.R, (float)(L.R * p.c), (float)(1.0 / p.c), (float)(L.Rsel * L.Rsel * 1.002), (const float *)ctx->bbox_nm.as<float>(), (const float *)ctx->lrow.as<float>(),
                           (const int *)g.start, (const f4_t *)g.ent, (const int *)g.maxhalf, (int)L.cap, (G == 1 && c_first == 0 && c_count == C && !short_from) ? 1 : 0,
                           ctx->nbr_list.as<int>(), ctx->nbr_cnt.as<int>(),
                           L.close ? (float)(p.rmin * p.rmin) * 1.001f : -1.f, L.close_cap, L.close ? ctx->close_list.as<int>() : nullptr, L.close ? ctx->close_cnt.as<int>() : nullptr);
        if (L.close) { P.close_list = ctx->close_list.as<int>(); P.close_cnt = ctx->close_cnt.as<int>(); P.close_cap = L.close_cap; }
    } else {
        const int nblk = (c_count + 63) / 64;
        hipLaunchKernelGGL(nbr_kernel, dim3((unsigned)(S * nblk * NBR_PARTS)), dim3(64), 0, st, S, G, C, g_local, c_first, c_count, short_from, (float)L.R, (float)(L.R * p.c),
                           (const float *)ctx->bbox.as<float>(), (const float *)ctx->bbox_nm.as<float>(), (int)L.cap, ctx->nbr_list.as<int>(), ctx->nbr_cnt.as<int>());
    }
    P.nbr_cap = (int)L.cap; P.nbr_list = ctx->nbr_list.as<int>(); P.nbr_cnt = ctx->nbr_cnt.as<int>();
    P.nbr_parts = L.use_grid ? 1 : NBR_PARTS;   // (the query writes a list as one run; nbr_cnt keeps NBR_PARTS slots per agent either way)
    dmpc_ctx::ListsBuilt &b = ctx->lists_built;   // (dmpc_debug_read_grid)
    b.S = S; b.G = G; b.C = C; b.ncell = L.use_grid ? L.ncell : 0; b.build = L.fused ? 2 : (L.use_grid ? 1 : 0);
    for (int a = 0; a < 3; ++a) b.n[a] = L.use_grid ? L.gg.n[a] : 0;
    b.cap = (int)L.cap; b.close_cap = L.close_cap; b.agents = pl.total; b.parts = NBR_PARTS;
    b.maxhalf = g.maxhalf; b.start = g.start; b.ent = g.ent;
    return 0;
}

// What differs between the launches of a step that take the parameter block: written into it right before each launch, every field every time.
struct LaunchArgs {
    int qcap = 0, only_flagged = 0, qover_bit = 0;
    const int *order = nullptr;        // launch order / tier-2 list
    int *flag_list = nullptr, *flag_count = nullptr;
    const int *live_bound = nullptr;
    int *counter = nullptr;            // persistent forms: queue head (null: positions round-robin)
    int lds_per_wave = 0, n_ext = 0, queue_chunk = 0;
    void apply(StepParams &P) const
    {
        P.qcap = qcap; P.only_flagged = only_flagged; P.qover_bit = qover_bit;
        P.order = order; P.flag_list = flag_list; P.flag_count = flag_count; P.live_bound = live_bound;
        P.counter = counter; P.lds_per_wave = lds_per_wave; P.n_ext = n_ext; P.queue_chunk = queue_chunk;
    }
};

// phase 0: scan + rows (solveDMPC scans inside its one kernel: no scan launch, no order)
static int launch_scan(dmpc_ctx *ctx, const StepPlan &pl, const StepIO &io, StepParams &P, hipStream_t st)
{
    if (pl.scp) {
        if (io.lTf) FAIL(ctx, "solveDMPC (DMPC_VAR_SCP) runs in fp64 only: create the context with DMPC_PREC_F64");
        return 0;
    }
    LaunchArgs a;
    a.qcap = pl.tier[0].qcap; a.qover_bit = pl.two_tier ? ST_QOVER : ST_CAPACITY; a.lds_per_wave = (int)pl.scan_lds;
    a.apply(P);
    const int W = pl.scan_waves;
    launch_params_kernel(scan_kernel(pl.soft, io.lTf != nullptr, P.fast_exit != 0, ctx->prm.order == 4), dim3((unsigned)((pl.total + W - 1) / W)), dim3(64u * W), pl.scan_lds * W, st, P);
    if (P.gzero) ctx->grid_clean = true;   // (this scan launch leaves the cell grid's counters zero for the next step's grid_prep_kernel)
    return 0;
}

// heaviest-first launch order for the solve phase: leaves the order, the live bound and the cost hint of the solve launches in P
static int launch_order(dmpc_ctx *ctx, const StepPlan &pl, StepParams &P, hipStream_t st)
{
    const int total = pl.total;
    if (pl.scp) return 0;
    if (ctx->forced_n == total) { P.order = ctx->forced_order.as<int>(); return 0; }   // development aid: externally supplied launch order
    if (!pl.run_order) return 0;
    const int nb = pl.order_slices;
    int *hint = nullptr;
    if (ctx->opt.order_hint) {   // the previous step's work estimates: valid while the batch keeps its shape
        if (ctx->prev_cost.ensure((size_t)total * 4)) FAIL(ctx, "device allocation failed (order hint)");
        // (the agents of the launch: which columns of how large a table -- a sub-range of another start or of another table is another set of agents)
        const long shape = ((((long)pl.sh.S * 1000003L + (long)pl.sh.G * pl.sh.C) * 1000003L + pl.sh.c_first) * 1000003L + pl.sh.c_count) * 16L + (long)ctx->prm.variant;
        if (shape != ctx->prev_cost_shape) { HIPCHK(ctx, hipMemsetAsync(ctx->prev_cost.p, 0, (size_t)total * 4, st)); ctx->prev_cost_shape = shape; }
        hint = ctx->prev_cost.as<int>();
        P.cost_out = hint;
    }
    hipLaunchKernelGGL(order_kernel, dim3((unsigned)nb), dim3(1024), (size_t)((total + nb - 1) / nb) * 2, st, total, (const int *)P.hdr, ctx->order.as<int>(), ctx->counter.as<int>() + 3,
                       hint, ctx->opt.order_hint);
    P.order = ctx->order.as<int>();
    P.live_bound = ctx->counter.as<int>() + 3;
    return 0;
}

// one launch of the general solver; `tier` is its queue head among the step's counters
static int launch_tier(dmpc_ctx *ctx, const StepPlan &pl, const TierPlan &t, int tier, LaunchArgs a, StepParams &P, hipStream_t st)
{
    const SolveKernel *k = find_solve_kernel(t.persistent, pl.soft, t.qcap, (t.persistent && t.tsplit) ? t.tsplit : t.qcap, pl.f32t);
    if (!k) FAIL(ctx, "no solve kernel for a working set of " + std::to_string(t.qcap) + " slots");
    a.qcap = t.qcap;
    if (t.persistent) {
        if ((int)t.lds_persist > ctx->max_lds_persist) {
            if (raise_solve_lds(ctx, true, (int)t.lds_persist)) return -1;
            ctx->max_lds_persist = (int)t.lds_persist;
        }
        a.counter = ctx->opt.static_queue ? nullptr : ctx->counter.as<int>() + tier;
        a.lds_per_wave = (int)t.per_wave_lds; a.n_ext = t.n_ext; a.queue_chunk = t.queue_chunk;
    }
    a.apply(P);
    if (!a.only_flagged) ctx->last_kernel = solve_kernel_name(t.persistent, *k);
    if (t.persistent) launch_params_kernel(k->fn, dim3((unsigned)t.wgs), dim3((unsigned)(64 * t.pw)), t.lds_persist, st, P);
    else launch_params_kernel(k->fn, dim3((unsigned)pl.total), dim3(64), t.lds_plain, st, P);
    return 0;
}

// solveDMPC.m: the whole SCP loop of an agent -- up to k_hor passes of {scan about the previous pass's prediction, slack-free QP} -- in ONE
// launch, one agent per 64-thread workgroup (dmpc_scp_kernel); no neighbour lists (rows for every other agent), no launch order
static int launch_scp(dmpc_ctx *ctx, const StepPlan &pl, StepParams &P, hipStream_t st)
{
    LaunchArgs a;
    a.qcap = 48; a.qover_bit = ST_CAPACITY; a.lds_per_wave = (int)pl.scan_lds;
    a.apply(P);
    const size_t lds_scp = std::max(solve_lds_bytes(P.nrmax, false, 48, false), pl.scan_lds);
    if ((int)lds_scp > ctx->max_lds_scp) {
        HIPCHK(ctx, hipFuncSetAttribute((const void *)dmpc_scp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_scp));
        ctx->max_lds_scp = (int)lds_scp;
    }
    launch_params_kernel((const void *)dmpc_scp_kernel, dim3((unsigned)pl.total), dim3(64), lds_scp, st, P);
    ctx->last_kernel = "dmpc_scp_kernel";
    return 0;
}

// tier 0: the reduced solver over every agent of the launch (persistent waves, as many workgroups per CU as its registers allow); the agents it
// does not take -- more than 64 rows, a third active wall, more than five hard constraints -- go to the general solver with its full capacity
static int launch_reduced(dmpc_ctx *ctx, const StepPlan &pl, StepParams &P, hipStream_t st)
{
    if (ctx->rsolve_blocks == 0) {   // (the one query of the launch path: once per context)
        int nb = 0;
        HIPCHK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)dmpc_rsolve_persist_kernel, RSOLVE_WAVES * 64, (size_t)RSOLVE_WAVES * RSOLVE_LDS_PER_WAVE));
        ctx->rsolve_blocks = nb > 0 ? nb : 1;
    }
    const int total = pl.total;
    int wgs = (total + RSOLVE_WAVES - 1) / RSOLVE_WAVES;
    if (wgs > ctx->rsolve_blocks * ctx->num_cu) wgs = ctx->rsolve_blocks * ctx->num_cu;
    int *const counters = ctx->counter.as<int>(), *const flagged = ctx->flag_list.as<int>();
    LaunchArgs a;
    a.qcap = 0; a.qover_bit = ST_QOVER;
    a.order = P.order;
    a.live_bound = P.post_on ? nullptr : P.live_bound;   // fused post-step: the agents the scan finished are visited too (their part of the state advance and of the scene's verdict)
    a.flag_count = counters + 2; a.flag_list = flagged;
    a.counter = ctx->opt.static_queue ? nullptr : counters;
    a.lds_per_wave = RSOLVE_LDS_PER_WAVE;
    a.queue_chunk = ctx->opt.queue_chunk > 0 ? ctx->opt.queue_chunk : (total < 12 * wgs * RSOLVE_WAVES ? 1 : 2);
    a.apply(P);
    ctx->last_kernel = "dmpc_rsolve_persist_kernel";
    launch_params_kernel((const void *)dmpc_rsolve_persist_kernel, dim3((unsigned)wgs), dim3(RSOLVE_WAVES * 64), (size_t)RSOLVE_WAVES * RSOLVE_LDS_PER_WAVE, st, P);
    // persistent waves over the flagged list (nearly always empty); else one workgroup per agent, each looking at its agent's flag
    LaunchArgs b;
    b.only_flagged = 1; b.qover_bit = ST_CAPACITY;
    b.order = pl.tier[1].persistent ? flagged : nullptr;
    b.flag_count = counters + 2;
    return launch_tier(ctx, pl, pl.tier[1], 1, b, P, st);
}

// the solve phase: the SCP kernel, the reduced solver and the general one behind it, or tier 1 and (two tiers) tier 2
static int launch_solve(dmpc_ctx *ctx, const StepPlan &pl, StepParams &P, hipStream_t st)
{
    if (pl.scp) return launch_scp(ctx, pl, P, st);
    if (pl.reduced) return launch_reduced(ctx, pl, P, st);
    int *const counters = ctx->counter.as<int>(), *const flagged = ctx->flag_list.as<int>();
    LaunchArgs a;
    a.qover_bit = pl.two_tier ? ST_QOVER : ST_CAPACITY;
    a.order = P.order; a.live_bound = P.live_bound;
    if (pl.t2_list) { a.flag_count = counters + 2; a.flag_list = flagged; }
    if (launch_tier(ctx, pl, pl.tier[0], 0, a, P, st)) return -1;
    if (!pl.two_tier) return 0;
    // tier 2: only agents flagged ST_QOVER do any work
    LaunchArgs b = a;
    b.only_flagged = 1; b.qover_bit = ST_CAPACITY; b.flag_list = nullptr;
    if (pl.t2_list) b.order = flagged;
    return launch_tier(ctx, pl, pl.tier[1], 1, b, P, st);
}

static int launch_step(dmpc_ctx *ctx, const StepShape &sh, const StepIO &io, hipStream_t st)
{
    const StepPlan pl = plan_step(ctx, sh);
    StepParams P;
    if (fill_params(ctx, pl, io, P, st)) return -1;
    Ev ev{nullptr, nullptr, nullptr};
    if (ctx->profile) {   // event triples are recycled (dmpc_profile_read2 returns them to the pool): no event is created inside a timed loop
        if (!ctx->ev_pool.empty()) { ev = ctx->ev_pool.back(); ctx->ev_pool.pop_back(); }
        else {
            HIPCHK(ctx, hipEventCreate(&ev.t0));
            HIPCHK(ctx, hipEventCreate(&ev.t1));
            HIPCHK(ctx, hipEventCreate(&ev.t2));
        }
        HIPCHK(ctx, hipEventRecord(ev.t0, st));
    }
    if (build_neighbour_lists(ctx, pl, io, P, st)) return -1;
    if (launch_scan(ctx, pl, io, P, st)) return -1;
    if (launch_order(ctx, pl, P, st)) return -1;
    if (ctx->profile) HIPCHK(ctx, hipEventRecord(ev.t1, st));
    if (launch_solve(ctx, pl, P, st)) return -1;
    HIPCHK(ctx, hipGetLastError());
    if (ctx->profile) {
        HIPCHK(ctx, hipEventRecord(ev.t2, st));
        ctx->events.push_back(ev);
    }
    ctx->solves += (int64_t)sh.S * sh.c_count;
    return 0;
}
