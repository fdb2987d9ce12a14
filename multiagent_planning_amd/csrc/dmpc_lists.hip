// dmpc_lists.hip -- the neighbour lists of large scenes on the device (part of dmpc_kernels.hip, inside namespace dmpc).  The cell grid is built in five
// launches (bbox, table_nbrmajor, grid_bin, grid_scan, grid_fill: any batch) or in two (grid_prep, grid_fill2: one scene) and the query reads what either
// left: what both state is ONE device function here -- nbrmajor_word, box_cell, chord_record.  (The segment boxes stay written out in bbox_kernel and grid_prep_kernel, see bbox_kernel.)

// Axis-aligned bounding boxes of every agent's predicted horizon, one per third of the horizon (steps 0-4, 5-9, 10-14):
// bbox[G][S][18][C] (fp32, rounded outwards) = per segment xmin,xmax,ymin,ymax,zmin,zmax.  A neighbour can come within R of the agent at step k only
// if the boxes of the segment that holds k are within R per axis.  (One box for the whole horizon lets 20 % of a 10^4-agent
// scene through once the agents move -- 4.3 m of horizon each; the three segments 4-5 times fewer.)
constexpr int NSEG = 3, SEG_STEPS = K / NSEG;
static_assert(NSEG * SEG_STEPS == K, "horizon segments");
template <typename TT>
__global__ void bbox_kernel(int total, int C, const TT *__restrict__ lT, float *__restrict__ bbox, float *__restrict__ bbox_nm /* [total][NBOX_NM]: the same boxes, one neighbour's 18 numbers contiguous (scalar loads of nbr_kernel) */)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // enumerates (g*S + s)*C + c
    if (i >= total) return;
    const int c = i % C;
    const size_t gs = (size_t)(i / C);
    const TT *src = lT + gs * N3 * C + c;
    float *dst = bbox + gs * (6 * NSEG) * C + c;
    // (the boxes stand here and in grid_prep_kernel: through a shared helper this kernel took 5.0 us against the parent's 4.6 - 4.8, DESIGN.md section 7;
    // tests/test_gpu_grid_build.py holds both builds' boxes to the fp64 extremes word for word)
    for (int sg = 0; sg < NSEG; ++sg) {
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int k = sg * SEG_STEPS; k < (sg + 1) * SEG_STEPS; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double v = (double)src[(size_t)(3 * k + a) * C];
                lo[a] = fmin(lo[a], v); hi[a] = fmax(hi[a], v);
            }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float flo = __double2float_rd(lo[a]), fhi = __double2float_ru(hi[a]);
            dst[(size_t)(6 * sg + 2 * a) * C] = flo; dst[(size_t)(6 * sg + 2 * a + 1) * C] = fhi;
            bbox_nm[(size_t)i * NBOX_NM + 6 * sg + 2 * a] = flo; bbox_nm[(size_t)i * NBOX_NM + 6 * sg + 2 * a + 1] = fhi;
        }
    }
}

// Neighbour-major fp32 copy of the prediction table for the list walk of the scan: out[chunk][scene][column][64] with element
// 4k + axis = component (k, axis) of that neighbour's horizon, 0 in the fourth slot of every step and in the last four.
template <typename TT>
__device__ __forceinline__ float nbrmajor_word(const TT *lT, int C, size_t t)
{
    const int l = (int)(t & 63), k4 = l >> 2, a4 = l & 3;
    const size_t gc = t >> 6, gs = gc / (size_t)C, c = gc - gs * (size_t)C;
    return (a4 < 3 && k4 < K) ? (float)lT[(gs * N3 + 3 * k4 + a4) * C + c] : 0.f;
}
template <typename TT>
__global__ void table_nbrmajor_kernel(size_t total, int C, const TT *__restrict__ lT, float *__restrict__ out, int *__restrict__ zbuf /* or null: the cell-grid counters, zeroed here */, size_t nz)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t z = t; z < nz; z += (size_t)gridDim.x * blockDim.x) zbuf[z] = 0;
    if (t >= total) return;
    out[t] = nbrmajor_word(lT, C, t);
}

// Neighbour lists of large scenes: the all-pairs test of the segment boxes.  LANES = 64 AGENTS of a scene (their inflated boxes in
// registers), the neighbours are walked one by one with the neighbour's 18 box numbers in SGPRs (five 16-byte scalar loads from the
// neighbour-major copy of the boxes): 18 compares per neighbour test 64 agent-neighbour pairs, nothing goes through LDS.  A neighbour
// whose box overlaps an agent's in any segment is appended to that agent's list -- per-lane counters, so every list is in increasing
// neighbour order.  (Round 2 had the roles the other way round -- a tile of 64 neighbours in the lanes, 8 agents' boxes broadcast from
// LDS, 144 LDS reads per tile and wave: at N = 10^4 that is 2.8e7 LDS instructions through ONE LDS pipe per CU, 0.2-0.37 ms whatever
// the VALU did.)
// code = (chunk << 20) | column, as the scan decodes it.  The neighbours of a scene are split over NBR_PARTS waves per agent block
// (N / 64 waves alone do not fill the chip); part q writes its survivors to the q-th piece of every agent's list (cap / NBR_PARTS
// entries) and their number to cnt_out[agent][q] (-1: did not fit: the scan walks the whole table); the scan kernel closes the gaps.
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef const f4_t __attribute__((address_space(4))) *ConstF4;
__global__ __launch_bounds__(64) void nbr_kernel(int S, int G, int C, int g_local, int c_first, int c_count, int short_from, float R, float Rz,
                                                 const float *__restrict__ bbox, const float *__restrict__ bbox_nm, int cap, int *__restrict__ list,
                                                 int *__restrict__ cnt_out)
{
    constexpr int NB = 6 * NSEG;
    const int nblk = (c_count + 63) >> 6;
    const int part = blockIdx.x % NBR_PARTS, sb = blockIdx.x / NBR_PARTS;
    const int scene = sb / nblk, b = sb - scene * nblk;
    const int lane = threadIdx.x;
    const int ci = b * 64 + lane;
    const bool mine = ci < c_count;
    const int cl = c_first + (mine ? ci : 0);
    // own boxes, inflated: even entries lower bound - R, odd entries upper bound + R (R carries a 1e-4 margin: far above the fp32
    // rounding of these sums); z by Rz (the metric's z scale)
    float ob[NB];
#pragma unroll
    for (int x = 0; x < NB; ++x) {
        const float v = bbox[((size_t)(g_local * S + scene) * NB + x) * C + cl];
        const float infl = (x % 6 < 4) ? R : Rz;
        ob[x] = (x & 1) ? v + infl : v - infl;
    }
    const int pcap = cap / NBR_PARTS;
    const size_t gid = (size_t)scene * c_count + (mine ? ci : 0);
    int *mylist = list + gid * (size_t)cap + (size_t)part * pcap;
    const long E = (long)G * C;
    const int e_lo = (int)(E * part / NBR_PARTS), e_hi = (int)(E * (part + 1) / NBR_PARTS);
    int cnt = 0;
    // the overlap test in arithmetic form: two boxes overlap on an axis iff max(n_lo - o_hi, o_lo - n_hi) <= 0; a segment overlaps iff the
    // maximum over its six differences is <= 0, a neighbour is listed iff the minimum over the three segments is.  6 subtractions + 3
    // three-operand maxima per segment with the neighbour's numbers as scalar operands: no mask logic on the scalar unit.  (A difference
    // that rounds or flushes to zero reads as "touching": the list only ever grows by that, it is a superset by design.)
    for (int e = e_lo; e < e_hi;) {
        const int r = e / C, j_lo = e - r * C;
        const int j_hi = (e_hi - e) < (C - j_lo) ? j_lo + (e_hi - e) : C;                      // this part's columns of chunk r
        const int j_end = j_hi < C - ((short_from && r >= short_from) ? 1 : 0) ? j_hi : C - ((short_from && r >= short_from) ? 1 : 0);   // (padding column of a short chunk)
        const float *base = bbox_nm + ((size_t)(r * S + scene) * C) * NBOX_NM;
        const int self = (r == g_local) ? cl : -1;
        for (int jc = j_lo; jc < j_end; ++jc) {
            const ConstF4 nb = (ConstF4)(unsigned long long)(base + (size_t)jc * NBOX_NM);
            const f4_t n0 = nb[0], n1 = nb[1], n2 = nb[2], n3 = nb[3], n4 = nb[4];
            const float nv[20] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, n3.x, n3.y, n3.z, n3.w, n4.x, n4.y, n4.z, n4.w};
            float sgm[NSEG];
#pragma unroll
            for (int sg = 0; sg < NSEG; ++sg) {
                const float a0 = nv[6 * sg] - ob[6 * sg + 1], a1 = ob[6 * sg] - nv[6 * sg + 1], a2 = nv[6 * sg + 2] - ob[6 * sg + 3];
                const float a3 = ob[6 * sg + 2] - nv[6 * sg + 3], a4 = nv[6 * sg + 4] - ob[6 * sg + 5], a5 = ob[6 * sg + 4] - nv[6 * sg + 5];
                sgm[sg] = fmaxf(__builtin_fmaxf(__builtin_fmaxf(a0, a1), a2), __builtin_fmaxf(__builtin_fmaxf(a3, a4), a5));
            }
            const float worst = __builtin_fminf(__builtin_fminf(sgm[0], sgm[1]), sgm[2]);
            if (worst <= 0.f && mine && jc != self) {
                if (cnt < pcap) mylist[cnt] = (r << 20) | jc;
                cnt++;
            }
        }
        e += j_hi - j_lo;
    }
    if (mine) cnt_out[gid * NBR_PARTS + part] = cnt > pcap ? -1 : cnt;
}

// --------------------------------------------------------------------------------------------
// Neighbour lists of large scenes, round 4: a cell grid instead of the all-pairs box test, and the fp32 DISTANCE test of the scan's list
// walk moved in here.  (C4, 10^4 agents, round 3: nbr_kernel is an O(N^2) box test -- 222 us -- whose lists hold the 100-700 neighbours
// whose horizon boxes come close; every lane appended to its own list at a 16 KB stride, 137 MB of written cache lines for 12 MB of
// entries; the scan then walked those lists once per agent with a whole horizon of distances per entry, 327 us.)
//   grid_bin / grid_scan / grid_fill: the agents of a scene binned by the CENTRE of their whole-horizon box (counting sort: count,
//     exclusive scan per scene, scatter; the order inside a cell is whatever the atomics give -- nothing below depends on it);
//   grid_query: one workgroup per agent, one wave per horizon segment.  Candidates = the entries of the cells within own half extent + R +
//     the scene's LARGEST half extent of the own box centre (a running maximum from grid_bin), streamed as two coalesced 16-byte halves
//     per candidate, lanes = candidates; pre-test = closest approach of the two segment CHORDS at equal time against R + both deviations
//     from the chord (grid_fill_kernel; the segment-box test of nbr_kernel passed 609 candidates per agent at N = 10^4, this one 157);
//     survivors compacted into an LDS staging list; full waves of survivors then take the distance test itself -- the candidate's segment
//     from the fp32 neighbour-major table (5 x 16 bytes per lane) against the own one (LDS broadcasts), pass = some horizon step closer
//     than the selection radius (3 rmin; 1 for the hard rows), widened by 1e-3 as in the scan -- and set their bit in the workgroup's
//     BITMAP over the scene's agents; the list is the bitmap read in order: increasing neighbour index whatever order the candidates came
//     in (the scan builds rows in list order = the reference's row order), duplicates impossible, written as one contiguous run.  Lists of
//     10-40 entries (100 at N = 10^4) instead of 100-700: a superset of every pair the scan can select at any step, so results are
//     unchanged bit for bit (tests/test_gpu_paths.py against option no_cull).
//     N = 10^4, one scene: 171 us with the box pre-test and 32-byte records -> 106 (chord pre-test) -> 94 (records as two arrays: a wave's
//     load is whole cache lines) -> 91 (agents taken in cell order) -> 88 us (a wave per segment).  What is left is the candidate stream,
//     2 046 records per agent = 655 MB per step out of the L2s, at ~80 instructions per round of 64: without any survivor the kernel took
//     90 of 106 us, without the stream 18 (both compiled out); its loads were NOT in flight during the previous round's test until the
//     instruction stream was read (see the loop), and putting them in flight changed nothing -- throughput, not latency.
//     After round 6: 96 -> 86 us with finer cells (810 - 2 074 candidates per agent); 86 -> 74 us with a lane's run taken from a bit count
//     instead of a binary search over the runs' prefix sums (58 -> 13 instructions per round for the fetch, see the loop).
// --------------------------------------------------------------------------------------------
struct GridGeom {
    float org[3], inv[3];   // cell index along axis a = clamp(floor((x - org[a]) * inv[a]), 0, n[a] - 1)
    int n[3];
};
__device__ __forceinline__ int grid_coord(const GridGeom &g, int a, float x)
{
    const float t = (x - g.org[a]) * g.inv[a];
    const int c = (int)floorf(t);
    return c < 0 ? 0 : (c >= g.n[a] ? g.n[a] - 1 : c);   // clamping is monotone: points within d of each other stay within ceil(d / cell) cells
}
// The cell of a segment box's centre, and the box's half extents ROUNDED UP: the query's reach must cover them.
__device__ __forceinline__ int box_cell(const GridGeom &gg, const float (&lo)[3], const float (&hi)[3], float (&half)[3])
{
    int cc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        half[a] = 0.5f * (hi[a] - lo[a]) * 1.0001f + 1e-5f;
        cc[a] = grid_coord(gg, a, 0.5f * (lo[a] + hi[a]));
    }
    return (cc[2] * gg.n[1] + cc[1]) * gg.n[0] + cc[0];
}
// thread per table column (chunk, scene, column): per horizon segment the cell of the segment box's centre, cell counts, the scene's
// largest half extents (one atomic per wave and quantity when the wave's columns belong to one scene -- 10^4 same-address atomics are
// 0.1 ms of serialised service each)
__global__ void grid_bin_kernel(int total, int S, int C, int short_from, GridGeom gg, const float *__restrict__ bbox_nm, int *__restrict__ cellof,
                                int *__restrict__ cnt, int *__restrict__ maxhalf)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // (r * S + scene) * C + c
    const bool in = i < total;
    const int ii = in ? i : total - 1;
    const int c = ii % C, rs = ii / C, scene = rs % S, r = rs / S;
    const bool valid = in && !(short_from && r >= short_from && c == C - 1);   // (padding column of a short chunk)
    const float *b = bbox_nm + (size_t)ii * NBOX_NM;
    const int ncell = gg.n[0] * gg.n[1] * gg.n[2];
    const int sc0 = __builtin_amdgcn_readfirstlane(scene);
    const bool uni = __all(scene == sc0);
    // (blockIdx.y = segment: a thread's work is a chain of dependent round trips -- loads, wave maxima, atomics -- and 10^4 threads do not fill
    // the chip: three times as many, a third as long)
    {
        const int sg = (int)blockIdx.y;
        float lo[3], hi[3], half[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = b[6 * sg + 2 * a]; hi[a] = b[6 * sg + 2 * a + 1]; }
        const int cell = box_cell(gg, lo, hi, half);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int hb = valid ? __float_as_int(half[a]) : 0;   // non-negative floats order like integers
            int *dst = maxhalf + ((size_t)scene * NSEG + sg) * 3 + a;
            if (uni) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(hb, off); hb = o > hb ? o : hb; }
                if ((threadIdx.x & 63) == 0 && hb > *(volatile int *)dst) atomicMax(dst, hb);
            } else if (valid && hb > *(volatile int *)dst) atomicMax(dst, hb);
        }
        if (in) cellof[(size_t)sg * total + i] = valid ? cell : -1;
        if (valid) atomicAdd(cnt + ((size_t)scene * NSEG + sg) * ncell + cell, 1);
    }
}
// block of 1024 threads per grid (scene and segment here; scene and sample of the post-check, dmpc_postcheck_host.hip): start[0 .. ncell] = exclusive
// prefix of the cell counts, number of entries in cells < c; the counts go back to zero (grid_fill / the post-check's scatter count them up again)
__global__ void grid_scan_kernel(int ncell, int *__restrict__ cnt, int *__restrict__ start)
{
    __shared__ int part[1024];
    int *f = cnt + (size_t)blockIdx.x * ncell, *st = start + (size_t)blockIdx.x * (ncell + 1);
    const int per = (ncell + 1023) / 1024, lo = threadIdx.x * per, hi = lo + per < ncell ? lo + per : ncell;
    int a = 0;
    for (int c = lo; c < hi; ++c) a += f[c];
    part[threadIdx.x] = a;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive scan of the partial sums
        const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - a;
    for (int c = lo; c < hi; ++c) { st[c] = run; run += f[c]; f[c] = 0; }
    if (threadIdx.x == 1023) st[ncell] = part[1023];
}
// entry = 32-byte record: the query streams its candidates COALESCED (a gather of the candidates' data -- 64 cache lines per wave load --
// kept the address units busy for the whole kernel).  What a record holds is the segment's CHORD: {code, first step x, y, z/c, last - first step
// x, y, z/c, largest distance of the segment's steps from the chord at their own time} -- the query's pre-test is the closest approach of
// two chords AT EQUAL TIME (two agents whose segment boxes overlap are usually at the overlap at different times: the box test let 609
// candidates per agent through to the distance test at N = 10^4, the chord test 157; 100 are listed)
__device__ __forceinline__ void chord_record(const f4_t *row /* the segment's first step in the neighbour-major table */, float e1z, int code, f4_t &r0, f4_t &r1)
{
    f4_t v[SEG_STEPS];
#pragma unroll
    for (int u = 0; u < SEG_STEPS; ++u) { v[u] = row[u]; v[u].z *= e1z; }
    const f4_t a0 = v[0], a1 = v[SEG_STEPS - 1];
    float dev2 = 0.f;
#pragma unroll
    for (int u = 1; u < SEG_STEPS - 1; ++u) {
        const float t = (float)u / (float)(SEG_STEPS - 1);
        const float dx = v[u].x - (a0.x + t * (a1.x - a0.x)), dy = v[u].y - (a0.y + t * (a1.y - a0.y)), dz = v[u].z - (a0.z + t * (a1.z - a0.z));
        dev2 = fmaxf(dev2, dx * dx + dy * dy + dz * dz);
    }
    r0.x = __int_as_float(code); r0.y = a0.x; r0.z = a0.y; r0.w = a0.z;
    r1.x = a1.x - a0.x; r1.y = a1.y - a0.y; r1.z = a1.z - a0.z; r1.w = sqrtf(dev2) * 1.0001f + 1e-5f;   // (rounded up)
}
__global__ void grid_fill_kernel(int total, int S, int C, int ncell, float e1z, const int *__restrict__ cellof, int *__restrict__ cnt, const int *__restrict__ start,
                                 const float *__restrict__ lrow, f4_t *__restrict__ ent)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = i % C, rs = i / C, scene = rs % S, r = rs / S;
    const size_t nag = (size_t)total / S;
#pragma unroll
    for (int sg = 0; sg < NSEG; ++sg) {
        const int cell = cellof[(size_t)sg * total + i];
        if (cell < 0) return;
        const size_t ss = (size_t)scene * NSEG + sg;
        const int pos = atomicAdd(cnt + ss * ncell + cell, 1);
        f4_t r0, r1;
        chord_record((const f4_t *)lrow + (size_t)i * 16 + SEG_STEPS * sg, e1z, (r << 20) | c, r0, r1);
        const size_t ei = ss * nag + start[ss * (ncell + 1) + cell] + pos;
        ent[ei] = r0; ent[(size_t)S * NSEG * nag + ei] = r1;   // two arrays of 16-byte halves: a wave's load of either is whole cache lines
    }
}
// ---- the cell grid of ONE scene in two launches (round 6; the five kernels above -- boxes, neighbour-major copy, bin, scan, fill: 42 us of
// a 0.7 ms MPC step at N = 10^4, every one of them a chain of dependent round trips at the launch floor -- stay for batches of scenes).
// grid_prep_kernel: blocks [0, nbA): thread per table column -- segment boxes (bbox_kernel), cell of each segment's centre, its position within the
// cell (the value the count's atomicAdd returns: the fill needs no second round of atomics), the scene's largest half extents through a
// block-wide maximum in LDS (nine global atomics per block); blocks [nbA, ..): the neighbour-major fp32 copy (table_nbrmajor_kernel).  The
// counters must be ZERO at entry: the scan kernel of the previous step leaves them so (StepParams::gzero), a memset the first time.
template <typename TT>
__global__ __launch_bounds__(256) void grid_prep_kernel(int total, int C, int short_from, GridGeom gg, int nbA, const TT *__restrict__ lT, float *__restrict__ bbox,
                                                        float *__restrict__ bbox_nm, float *__restrict__ lrow, int *__restrict__ cellof, int *__restrict__ posof,
                                                        int *__restrict__ cnt, int *__restrict__ maxhalf)
{
    if ((int)blockIdx.x >= nbA) {
        const size_t t = (size_t)((int)blockIdx.x - nbA) * 256 + threadIdx.x;
        if (t >= (size_t)total * 64) return;
        lrow[t] = nbrmajor_word(lT, C, t);
        return;
    }
    __shared__ int mh[NSEG * 3];
    if (threadIdx.x < NSEG * 3) mh[threadIdx.x] = 0;
    __syncthreads();
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;   // r * C + c (one scene)
    if (i < total) {
        const int c = i % C, r = i / C;
        const bool valid = !(short_from && r >= short_from && c == C - 1);   // (padding column of a short chunk)
        const TT *src = lT + (size_t)r * N3 * C + c;
        float *dst = bbox + (size_t)r * (6 * NSEG) * C + c;
        const int ncell = gg.n[0] * gg.n[1] * gg.n[2];
#pragma unroll
        for (int sg = 0; sg < NSEG; ++sg) {
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
#pragma unroll
            for (int k = sg * SEG_STEPS; k < (sg + 1) * SEG_STEPS; ++k)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double v = (double)src[(size_t)(3 * k + a) * C];
                    lo[a] = fmin(lo[a], v); hi[a] = fmax(hi[a], v);
                }
            float flo[3], fhi[3], half[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {   // (as bbox_kernel)
                flo[a] = __double2float_rd(lo[a]); fhi[a] = __double2float_ru(hi[a]);
                dst[(size_t)(6 * sg + 2 * a) * C] = flo[a]; dst[(size_t)(6 * sg + 2 * a + 1) * C] = fhi[a];
                bbox_nm[(size_t)i * NBOX_NM + 6 * sg + 2 * a] = flo[a]; bbox_nm[(size_t)i * NBOX_NM + 6 * sg + 2 * a + 1] = fhi[a];
            }
            const int cell = box_cell(gg, flo, fhi, half);
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (valid) atomicMax(&mh[3 * sg + a], __float_as_int(half[a]));   // non-negative floats order like integers
            cellof[(size_t)sg * total + i] = valid ? cell : -1;
            posof[(size_t)sg * total + i] = valid ? atomicAdd(cnt + (size_t)sg * ncell + cell, 1) : 0;
        }
    }
    __syncthreads();
    if (threadIdx.x < NSEG * 3) { const int v = mh[threadIdx.x]; if (v > *(volatile int *)(maxhalf + threadIdx.x)) atomicMax(maxhalf + threadIdx.x, v); }
}
// grid_fill2_kernel: every block forms the exclusive prefix of the three segments' cell counts in its LDS (8 200 cells each at N = 10^4: cheaper
// than a launch of its own and a trip through memory) and writes its slice of it out for the query; then the entry records as grid_fill_kernel,
// at start[cell] + the position grid_prep_kernel drew.  Dynamic LDS: NSEG * (ncell + 1) ints (plan_lists: up to 128 KB, the limit raised by the launcher).
__global__ __launch_bounds__(256) void grid_fill2_kernel(int total, int C, int ncell, float e1z, const int *__restrict__ cellof, const int *__restrict__ posof,
                                                         const int *__restrict__ cnt, int *__restrict__ start, const float *__restrict__ lrow, f4_t *__restrict__ ent)
{
    int *st = (int *)dmpc_smem;   // [NSEG][ncell + 1]
    __shared__ int wtot[NSEG][4];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    // the counts come into LDS coalesced and become their prefix in place (a thread that read its chunk from memory did so at a stride of
    // the chunk, twice: 33 cells at the 8 200 cells of a fine grid); an ODD chunk keeps the threads of a wave on different banks
    const int chunk = ((ncell + 255) / 256) | 1;
    const int lo = t * chunk, hi = lo + chunk < ncell ? lo + chunk : ncell;
    // (the three segments side by side in every loop: three independent chains of loads / LDS round trips instead of one after the other)
#pragma unroll 4
    for (int j = t; j < ncell; j += 256)
#pragma unroll
        for (int sg = 0; sg < NSEG; ++sg) st[sg * (ncell + 1) + j] = cnt[(size_t)sg * ncell + j];
    __syncthreads();
    // the three segments' prefixes together: a thread sums its chunk of each, one scan inside the wave (shuffles), the four waves' totals through LDS
    int sum[NSEG], inc[NSEG];
#pragma unroll
    for (int sg = 0; sg < NSEG; ++sg) sum[sg] = 0;
    for (int j = lo; j < hi; ++j)
#pragma unroll
        for (int sg = 0; sg < NSEG; ++sg) sum[sg] += st[sg * (ncell + 1) + j];
#pragma unroll
    for (int sg = 0; sg < NSEG; ++sg) inc[sg] = sum[sg];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
#pragma unroll
        for (int sg = 0; sg < NSEG; ++sg) { const int o = __shfl_up(inc[sg], off); if (lane >= off) inc[sg] += o; }
    if (lane == 63)
#pragma unroll
        for (int sg = 0; sg < NSEG; ++sg) wtot[sg][wave] = inc[sg];
    __syncthreads();
    int run[NSEG];
#pragma unroll
    for (int sg = 0; sg < NSEG; ++sg) {
        run[sg] = inc[sg] - sum[sg];   // exclusive inside the wave
        for (int w = 0; w < wave; ++w) run[sg] += wtot[sg][w];
        if (t == 255) st[sg * (ncell + 1) + ncell] = wtot[sg][0] + wtot[sg][1] + wtot[sg][2] + wtot[sg][3];
    }
    for (int j = lo; j < hi; ++j)   // (a thread's own chunk: nobody else reads or writes it)
#pragma unroll
        for (int sg = 0; sg < NSEG; ++sg) { int *c = st + sg * (ncell + 1) + j; const int n = *c; *c = run[sg]; run[sg] += n; }
    __syncthreads();
    {   // the prefix for the query: every block holds all of it and writes its own slice (block 0 alone wrote 96 rounds at 8 200 cells)
        const int all = NSEG * (ncell + 1), slice = (all + (int)gridDim.x - 1) / (int)gridDim.x;
        const int j0 = (int)blockIdx.x * slice, j1 = j0 + slice < all ? j0 + slice : all;
        for (int j = j0 + t; j < j1; j += 256) start[j] = st[j];
    }
    const int i = (int)blockIdx.x * 256 + t;
    if (i >= total) return;
    const int code = ((i / C) << 20) | (i % C);   // (chunk << 20) | column
#pragma unroll
    for (int sg = 0; sg < NSEG; ++sg) {
        const int cell = cellof[(size_t)sg * total + i];
        if (cell < 0) return;
        const int pos = posof[(size_t)sg * total + i];
        f4_t r0, r1;
        chord_record((const f4_t *)lrow + (size_t)i * 16 + SEG_STEPS * sg, e1z, code, r0, r1);
        const size_t ei = (size_t)sg * total + st[sg * (ncell + 1) + cell] + pos;
        ent[ei] = r0; ent[(size_t)NSEG * total + ei] = r1;
    }
}
// A workgroup = ONE agent, a wave per horizon segment (the segments are independent up to the bitmap, which the three waves share): three
// times as many, shorter waves -- the launch is a little more than one round of resident waves deep (39 agents per CU at N = 10^4 against
// 28 wave slots), and ends with the last agents' whole chains otherwise.
constexpr int GQ_WAVES = NSEG;
constexpr int GQ_STAGE = 128;      // staging list of box-test survivors per wave (a full wave is taken off it as soon as there is one)
// Close pairs (close_cap > 0): the distance test has every per-step squared distance of a candidate in a register; the (neighbour, step) pairs
// below thr_close = rmin^2 * 1.001 -- the pairs the scan's list walk selected for its exact test by loading every listed neighbour's row
// AGAIN and forming the same distances -- are appended to a per-agent list behind a counter in LDS (the three waves share it) and written out
// coalesced: close_list[agent][close_cap] records {code, step}, close_cnt[agent] (-1: more than close_cap, the scan walks the list as before).
// A neighbour is an entry of ONE cell per segment and a step belongs to one segment: no pair is recorded twice.
// Lane -> run of the fetch: per wave the entry bases of a batch's non-empty runs by ordinal (GQ_RUNS ints) and a bit window over
// GQ_WIN positions of the batch's concatenation (one 32-bit word per lane).  Fixed sizes: nothing here grows with the agent count.
constexpr int GQ_RUNS = 64;
constexpr int GQ_WIN = 2048;
constexpr int GQ_WAVE_INTS = GQ_STAGE + GQ_RUNS + GQ_WIN / 32;   // stage, run bases, window
static_assert(GQ_WIN / 32 == 64, "the window is one word per lane");
inline size_t grid_query_lds(int nagents, int close_cap = 0)
{
    return (((size_t)((nagents + 31) / 32) * 4 + GQ_WAVES * GQ_WAVE_INTS * 4 + 15) & ~(size_t)15) + 16 * 16 + (close_cap > 0 ? 16 + (size_t)close_cap * 8 : 0);
}
typedef float f2_t __attribute__((ext_vector_type(2)));
// inclusive prefix sum of an int over the lanes (the gfx9 DPP scan of wave_scan_sum: row_shr 1/2/4/8, the two row broadcasts; a lane
// without a source adds 0).  A wave collective: never inside a lane-dependent branch.
__device__ __forceinline__ int wave_scan_add(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}
__global__ __launch_bounds__(64 * GQ_WAVES) void grid_query_kernel(int S, int G, int C, int g_local, int c_first, int c_count, GridGeom gg, float R, float Rz, float e1z, float thr2,
                                                                   const float *__restrict__ bbox_nm, const float *__restrict__ lrow, const int *__restrict__ start,
                                                                   const f4_t *__restrict__ ent, const int *__restrict__ maxhalf, int cap, int cell_order,
                                                                   int *__restrict__ list, int *__restrict__ cnt_out,
                                                                   float thr_close, int close_cap, int *__restrict__ close_list, int *__restrict__ close_cnt)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const int gid = (int)blockIdx.x;
    const int nag = G * C, nwords = (nag + 31) >> 5, ncell = gg.n[0] * gg.n[1] * gg.n[2];
    const int scene = gid / c_count;
    int ci = gid - scene * c_count;
    // cell_order (a query over whole scenes): wave number -> agent through the first segment's entry array, which IS the scene's agents sorted
    // by cell -- the waves of a workgroup, and of a CU, then stream the same cells' candidates (one trip to the L2 for the lot; in agent
    // order every wave fetched its 65 KB of candidates on its own: 655 MB per step at N = 10^4, 11 TB/s out of the L2s)
    if (cell_order) ci = __builtin_amdgcn_readfirstlane(__float_as_int(ent[(size_t)scene * NSEG * nag + ci].x) & 0xfffff);
    const int cl = c_first + ci;
    const int oid = scene * c_count + ci;   // where this agent's list goes
    unsigned *bits = (unsigned *)dmpc_smem;
    int *stage = (int *)(dmpc_smem + (size_t)nwords * 4) + wave * GQ_WAVE_INTS;
    int *runbase = stage + GQ_STAGE;                       // entry base of the batch's non-empty run of ordinal o
    unsigned *win = (unsigned *)(runbase + GQ_RUNS);       // the bit window, as it is built (the rounds read it from a register)
    f4_t *ownrow = (f4_t *)(dmpc_smem + (((size_t)nwords * 4 + GQ_WAVES * GQ_WAVE_INTS * 4 + 15) & ~(size_t)15));
    int *ccnt = (int *)(ownrow + 16), *crec = ccnt + 4;   // close pairs: counter (16 bytes), close_cap records of two ints (only there when close_cap > 0)
    for (int i = (int)threadIdx.x; i < nwords; i += 64 * GQ_WAVES) bits[i] = 0u;
    if (close_cap > 0 && threadIdx.x == 0) *ccnt = 0;
    const size_t self_i = (size_t)(g_local * S + scene) * C + cl;
    if (threadIdx.x < 16) ownrow[lane] = ((const f4_t *)lrow)[self_i * 16 + lane];   // the own horizon: 15 x (x, y, z, 0) + 4 zeros
    // own boxes (wave-uniform: scalar loads)
    const ConstF4 ob4 = (ConstF4)(unsigned long long)(bbox_nm + self_i * NBOX_NM);
    const f4_t o0 = ob4[0], o1 = ob4[1], o2 = ob4[2], o3 = ob4[3], o4 = ob4[4];
    const float obx[18] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w, o2.x, o2.y, o2.z, o2.w, o3.x, o3.y, o3.z, o3.w, o4.x, o4.y};
    __syncthreads();
    const int self_code = (g_local << 20) | cl;
    {
        const int sg = wave;
        // this segment's own box, inflated by the selection radius; the cells its neighbours' centres can lie in.  Why the range is a superset
        // whatever the cell size and however many cells an axis has (plan_lists: up to 64): a neighbour that comes within R of this agent at a
        // step of the segment has, per axis, a point of its segment box within R of the own box, and its box centre lies within its half
        // extent <= maxhalf of that point: centre in [lo - reach, hi + reach].  grid_coord is monotone (floor, then the clamp to [0, n - 1]), so
        // the centre's cell lies between the cells of the two ends -- for any org, inv and n; binning and query use the same function and
        // the same GridGeom.
        int c_lo[3], c_hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = sg == 0 ? obx[2 * a] : (sg == 1 ? obx[6 + 2 * a] : obx[12 + 2 * a]);
            const float hi = sg == 0 ? obx[2 * a + 1] : (sg == 1 ? obx[6 + 2 * a + 1] : obx[12 + 2 * a + 1]);
            const float infl = a < 2 ? R : Rz;
            const float reach = infl + __int_as_float(maxhalf[((size_t)scene * NSEG + sg) * 3 + a]);   // a neighbour's centre is at most its half extent from its box
            c_lo[a] = grid_coord(gg, a, lo - reach); c_hi[a] = grid_coord(gg, a, hi + reach);
        }
        // The candidates: per (y, z) cell row in reach one RUN of entries (the cells of a run along x are contiguous), ~50 entries each at
        // N = 10^4; the bounds of up to 64 runs are fetched at once (lanes = runs).  The first batch's bounds are requested HERE, as soon as the
        // cell range exists: the own chord's deviation below needs LDS alone and runs under the trip instead of in front of it.
        const size_t ss = (size_t)scene * NSEG + sg;
        const int *st = start + ss * (ncell + 1);
        const int ny = c_hi[1] - c_lo[1] + 1, nruns_all = ny * (c_hi[2] - c_lo[2] + 1);
        const UDiv div_ny((unsigned)ny);
        auto run_bounds = [&](int run0, int &rb, int &re) {
            const int nruns = nruns_all - run0 < 64 ? nruns_all - run0 : 64;
            rb = 0; re = 0;
            if (lane < nruns) {
                int qz, qy;
                div_ny.divmod((unsigned)(run0 + lane), qz, qy);
                const int row0 = ((c_lo[2] + qz) * gg.n[1] + c_lo[1] + qy) * gg.n[0];
                rb = st[row0 + c_lo[0]]; re = st[row0 + c_hi[0] + 1];
            }
        };
        int rb_first, re_first;
        run_bounds(0, rb_first, re_first);
        // the own chord of this segment (z in the metric's scale) and the steps' largest distance from it, as grid_fill computes them
        f4_t oa0 = ownrow[SEG_STEPS * sg], oa1 = ownrow[SEG_STEPS * sg + SEG_STEPS - 1];
        oa0.z *= e1z; oa1.z *= e1z;
        const float odx = oa1.x - oa0.x, ody = oa1.y - oa0.y, odz = oa1.z - oa0.z;
        float odev2 = 0.f;
#pragma unroll
        for (int u = 1; u < SEG_STEPS - 1; ++u) {
            const f4_t o = ownrow[SEG_STEPS * sg + u];
            const float t = (float)u / (float)(SEG_STEPS - 1);
            const float dx = o.x - (oa0.x + t * odx), dy = o.y - (oa0.y + t * ody), dz = o.z * e1z - (oa0.z + t * odz);
            odev2 = fmaxf(odev2, dx * dx + dy * dy + dz * dz);
        }
        const float lim0 = sqrtf(thr2) + sqrtf(odev2) * 1.0001f + 2e-4f;   // selection radius + own deviation (+ slack for the fp32 arithmetic of the test)
        const f4_t *en = ent + ss * nag, *en2 = ent + (size_t)S * NSEG * nag + ss * nag;
        int nst = 0;
        // the distance test over this segment's horizon steps on a full wave (or the rest) of staged survivors
        auto traj_test = [&](int n) {
            const bool have = lane < n;
            const int code = stage[have ? lane : 0];
            const int r = code >> 20, jc = code & 0xfffff;
            const f4_t *row = (const f4_t *)lrow + ((size_t)(r * S + scene) * C + jc) * 16 + SEG_STEPS * sg;
            bool pass = false;
            int cmask = 0;   // steps of the segment closer than thr_close (close pairs; thr_close < thr2: a subset of the passes; never with close_cap = 0, thr_close < 0)
            // (A loop that is NOT unrolled: with one test per step the compiler made the unrolled form a chain of early exits, a row quarter loaded
            // per step, 56 registers; a second test per step on the unrolled form keeps all five quarters in registers -- 85, five waves per SIMD
            // instead of eight; unrolled with three-component loads 80, and 78 with the loads held two ahead by scheduling barriers.  One step
            // per pass of the loop was a chain of five round trips at 60 registers.  This form takes two steps per pass from two register sets
            // of three floats in turn -- the next step's load goes out before the current step is waited for (s_waitcnt vmcnt(1)), and a set is
            // loaded again where it was last used: no copy at the loop's end.  Three trips' worth instead of five, 61 registers, eight waves.
            // Same loads, same comparisons in the same order over u.)
            typedef float f3_t __attribute__((ext_vector_type(3)));
            auto step = [&](int u, const f3_t w) {
                const f4_t o = ownrow[SEG_STEPS * sg + u];
                const float dx = o.x - w.x, dy = o.y - w.y, dz = (o.z - w.z) * e1z;
                const float d2 = dx * dx + dy * dy + dz * dz;
                pass = pass || (d2 < thr2);
                cmask |= (d2 < thr_close) ? (1 << u) : 0;
            };
            static_assert(SEG_STEPS % 2 == 1, "two steps per pass of the loop, the last one behind it");
            f3_t wa = *(const f3_t *)(row + 0);
#pragma unroll 1
            for (int u = 0; u < SEG_STEPS - 1; u += 2) {
                const f3_t wb = *(const f3_t *)(row + u + 1);
                step(u, wa);
                wa = *(const f3_t *)(row + u + 2);
                step(u + 1, wb);
            }
            step(SEG_STEPS - 1, wa);
            if (have && pass) {
                const int idx = r * C + jc;
                atomicOr(bits + (idx >> 5), 1u << (idx & 31));
                if (cmask != 0) {   // rare; a lane claims its records with one LDS atomic of its own: no wave collective in this lane-dependent branch
                    int pos = atomicAdd(ccnt, __popc(cmask));
                    while (cmask) {
                        const int u = __ffs(cmask) - 1;
                        cmask &= cmask - 1;
                        if (pos < close_cap) { crec[2 * pos] = code; crec[2 * pos + 1] = SEG_STEPS * sg + u; }
                        ++pos;
                    }
                }
            }
        };
        // (the runs' bounds: above; the records of the next round are in flight during a round's test)
        for (int run0 = 0; run0 < nruns_all; run0 += 64) {
            int rb = rb_first, re = re_first;
            if (run0 > 0) run_bounds(run0, rb, re);
            // The runs of this batch as ONE sequence of entries (a run holds ~50 entries at N = 10^4: a round of 64 lanes per run left a third of
            // the lanes idle and, worse, made every run a memory round trip of its own): lanes = the next 64 entries of the concatenation.
            // Lane -> run without a search (it was a binary search over the prefix sums, six dependent ds_bpermute round trips per round and
            // 60 % of a round's instructions): the NON-EMPTY runs are numbered in order (an empty run holds no position; the search passed
            // over it because its prefix equals its predecessor's), run o leaves its entry base in runbase[o] and -- all but the last one --
            // a bit at its LAST position in a window over the positions.  The run of position v is then the number of bits below v: the
            // bits of the rounds before (a prefix of the words' popcounts, once per window) + v_mbcnt over the round's own 64 bits.  The
            // window is 64 words, a word per lane, and stays in a register: a round reads its two words and the prefix with v_readlane.
            // Without the last run's bit the lanes past tot, which take position tot - 1, count the last run as well.
            const int len = re - rb;
            const int pre = wave_scan_add(len);   // inclusive prefix of the run lengths
            const int tot = __builtin_amdgcn_readlane(pre, 63);
            const unsigned long long ne = __ballot(len > 0);
            LSYNC();
            if (len > 0) runbase[lanes_below(ne, lane)] = rb - (pre - len);   // entry index of sequence position v in run o: runbase[o] + v
            const int endpos = (len > 0 && pre < tot) ? pre - 1 : -1;
            int ord0 = 0;   // ordinal of the run at the window's first position
            struct Rec { f4_t a, b; bool hv; };
            auto test = [&](const Rec &rc) {
                // closest approach of the two chords at equal time: r(t) = q + t e on [0, 1], against radius + both deviations.  (Any t gives
                // an upper bound of the minimum; the rounded t* is off by parts in 10^6 and |r(t)|^2 is flat there to second order.)
                const float qx = rc.a.y - oa0.x, qy = rc.a.z - oa0.y, qz = rc.a.w - oa0.z;
                const float ex = rc.b.x - odx, ey = rc.b.y - ody, ez = rc.b.z - odz;
                const float ee = ex * ex + ey * ey + ez * ez, qe = qx * ex + qy * ey + qz * ez, qq = qx * qx + qy * qy + qz * qz;
                const float tt = __builtin_fminf(__builtin_fmaxf(-qe * __builtin_amdgcn_rcpf(__builtin_fmaxf(ee, 1e-20f)), 0.f), 1.f);
                const float d2 = qq + tt * (qe + qe + tt * ee);   // |q + t e|^2 (rounding: parts in 10^7 of qq <= 60: the slack in lim0 covers it)
                const float lim = lim0 + rc.b.w;
                const int c0 = __float_as_int(rc.a.x);
                const bool surv = rc.hv && c0 != self_code && d2 <= lim * lim;
                const unsigned long long m = __ballot(surv);
                if (m) {
                    if (surv) stage[nst + lanes_below(m, lane)] = c0;
                    nst += __popcll(m);
                    LSYNC();
                    if (nst >= 64) {
                        traj_test(64);
                        LSYNC();
                        const int keep = lane < nst - 64 ? stage[64 + lane] : 0;
                        LSYNC();
                        if (lane < nst - 64) stage[lane] = keep;
                        nst -= 64;
                        LSYNC();
                    }
                }
            };
            for (int w0 = 0; w0 < tot; w0 += GQ_WIN) {   // (one window unless a batch holds more than GQ_WIN candidates)
                win[lane] = 0u;
                LSYNC();
                if ((unsigned)(endpos - w0) < (unsigned)GQ_WIN) atomicOr(win + ((endpos - w0) >> 5), 1u << ((endpos - w0) & 31));   // (per lane, no collective)
                LSYNC();
                const unsigned myw = win[lane];
                const int cumi = wave_scan_add(__popc(myw));
                const int cumw = ord0 + cumi - __popc(myw);   // runs that end before this lane's word
                ord0 += __builtin_amdgcn_readlane(cumi, 63);
                const int nround = ((tot - w0 < GQ_WIN ? tot - w0 : GQ_WIN) + 63) >> 6;
                // (the loads of a round are issued UNCONDITIONALLY, into registers of their own -- two record sets, the loop unrolled by two: a
                // fetch behind a branch, or a copy of the loaded registers at the loop's end, makes the compiler wait for the loads it has just
                // issued (s_waitcnt vmcnt(0)) and the prefetch is gone: that was the state of this loop until the instruction stream was read)
                auto fetch = [&](int k, Rec &rc) {
                    const int vi = w0 + 64 * k + lane;
                    rc.hv = vi < tot;
                    const int vq = rc.hv ? vi : tot - 1;
                    const unsigned mlo = (unsigned)__builtin_amdgcn_readlane((int)myw, 2 * k), mhi = (unsigned)__builtin_amdgcn_readlane((int)myw, 2 * k + 1);
                    const int o = (int)__builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, (unsigned)__builtin_amdgcn_readlane(cumw, 2 * k)));
                    const unsigned eb = (unsigned)(runbase[o] + vq) << 4;   // (a byte offset of 32 bits from a uniform base: no 64-bit address arithmetic per lane; a scene's entries are below 2^28)
                    rc.a = *(const f4_t *)((const char *)en + eb); rc.b = *(const f4_t *)((const char *)en2 + eb);
                };
                if (nround > 0) {
                    Rec ra, rb2;
                    fetch(0, ra);
                    for (int k = 0; k < nround; k += 2) {
                        fetch(k + 1 < nround ? k + 1 : nround - 1, rb2);   // (past the end: the last round once more, never tested)
                        test(ra);
                        if (k + 1 >= nround) break;
                        fetch(k + 2 < nround ? k + 2 : nround - 1, ra);
                        test(rb2);
                    }
                }
            }
        }
        if (nst > 0) traj_test(nst);
    }
    __syncthreads();
    if (wave == 1 && close_cap > 0) {   // the close pairs, next to wave 0's list: whole records, coalesced (the count went past close_cap: none, the scan walks the list)
        const int n = *ccnt;
        int *dst = close_list + (size_t)oid * 2 * close_cap;
        if (n <= close_cap) for (int i = lane; i < 2 * n; i += 64) dst[i] = crec[i];
        if (lane == 0) close_cnt[oid] = n > close_cap ? -1 : n;
    }
    if (wave != 0) return;
    // the list = the bitmap in order (increasing neighbour index), one contiguous run per agent
    int *out = list + (size_t)oid * cap;
    int total = 0;
    const UDiv div_c((unsigned)C);
    for (int w0 = 0; w0 < nwords; w0 += 64) {
        unsigned word = w0 + lane < nwords ? bits[w0 + lane] : 0u;
        if (__ballot(word != 0u) == 0ull) continue;   // (most chunks of a large scene: the neighbours are a hundred of 10^4)
        const int mycnt = __popc(word);
        const int pre = wave_scan_add(mycnt);   // inclusive prefix of the lanes' counts
        const int wave_total = __builtin_amdgcn_readlane(pre, 63);
        int pos = total + pre - mycnt;
        while (word) {
            const int b = __ffs((int)word) - 1;
            word &= word - 1u;
            const int idx = ((w0 + lane) << 5) + b;
            int r = 0, jc = idx;
            if (G > 1) div_c.divmod((unsigned)idx, r, jc);
            if (pos < cap) out[pos] = (r << 20) | jc;
            ++pos;
        }
        total += wave_total;
    }
    if (lane == 0) cnt_out[(size_t)oid * NBR_PARTS] = total > cap ? -1 : total;   // one piece, one count (StepParams::nbr_parts = 1: the scan reads slot 0 alone)
}
