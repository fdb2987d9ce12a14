// dmpc_debug.hip -- development aids (host code only; included by dmpc_api.hip behind dmpc_step.hip): the trace of one agent's iterations, the
// streaming read a counter is calibrated on, the readers of the last step's hand-off headers and list build, the forced launch order.  None of
// them is part of the public header (include/dmpc_hip_dev.h declares them).

// trace the active-set iterations of one agent.  host_out on an armed context: read the trace back.  Otherwise (re-)arm: the old buffer goes, and
// `cap` > 0 records of 8 doubles for one of the agent codes below get a zeroed one; anything else leaves the trace off (a read then writes nothing)
extern "C" int dmpc_debug_trace(dmpc_ctx *ctx, int agent, int cap, double *host_out)
{
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (host_out && ctx->dbg.p) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(host_out, ctx->dbg.p, sizeof(double) * 8 * ctx->dbg_cap, hipMemcpyDeviceToHost));
        return 0;
    }
    ctx->dbg.release();
    ctx->dbg_agent = agent; ctx->dbg_cap = cap;
    if ((agent >= 0 || agent == -2 || agent == -3 || agent == -5 || agent == -7) && cap > 0) {
        if (ctx->dbg.ensure(sizeof(double) * 8 * cap)) FAIL(ctx, "dmpc_debug_trace: out of device memory");
        HIPCHK(ctx, hipMemset(ctx->dbg.p, 0, sizeof(double) * 8 * cap));
    }
    return 0;
}

// a coalesced streaming read of `bytes` bytes at lane_bytes (8 | 16) per lane, `reps` launches -- the known byte count the FETCH_SIZE counter is
// calibrated on (tools/gpu_fetch_calib.py under rocprofv3 --pmc FETCH_SIZE)
extern "C" int dmpc_debug_read_probe(dmpc_ctx *ctx, size_t bytes, int lane_bytes, int reps)
{
    if (!ctx || (lane_bytes != 8 && lane_bytes != 16) || bytes < 4096) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf buf, sink;   // (every exit frees them)
    if (buf.ensure(bytes) || sink.ensure(64)) FAIL(ctx, "dmpc_debug_read_probe: out of device memory");
    HIPCHK(ctx, hipMemsetAsync(buf.p, 0, bytes, ctx->stream));
    for (int r = 0; r < reps; ++r) {
        if (lane_bytes == 8) hipLaunchKernelGGL(read_probe_kernel<double>, dim3(256 * 16), dim3(256), 0, ctx->stream, bytes / 8, (const double *)buf.p, sink.as<double>());
        else hipLaunchKernelGGL(read_probe_kernel<double2>, dim3(256 * 16), dim3(256), 0, ctx->stream, bytes / 16, (const double2 *)buf.p, sink.as<double>());
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// the scan's hand-off headers of the last step (8 ints per agent: rows, reference row count, violating step, status, flags, rows exist, ladder
// start, launch-order key)
extern "C" int dmpc_debug_read_hdr(dmpc_ctx *ctx, int *host_out, int n_agents)
{
    if (!ctx || !host_out) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if ((size_t)n_agents * 32 > ctx->hdr.cap) { ctx->err = "dmpc_debug_read_hdr: more agents than the last step had"; return -1; }
    HIPCHK(ctx, hipMemcpy(host_out, ctx->hdr.p, (size_t)n_agents * 32, hipMemcpyDeviceToHost));
    return 0;
}

// what the last list build of a step left on the device (include/dmpc_hip_dev.h has the layout)
extern "C" int dmpc_debug_read_grid(dmpc_ctx *ctx, int *shape, void *out, size_t out_bytes)
{
    if (!ctx || !shape) return -1;
    dmpc_ctx::ListsBuilt &b = ctx->lists_built;
    b.armed = true;
    if (b.S == 0) { ctx->err = "dmpc_debug_read_grid: no step of this context has built neighbour lists"; return -1; }
    const int sh[12] = {b.S, b.G, b.C, b.n[0], b.n[1], b.n[2], b.ncell, b.build, b.cap, b.close_cap, b.agents, b.parts};
    memcpy(shape, sh, sizeof(sh));
    if (!out) return 0;
    const size_t nag = (size_t)b.G * b.C, grid = b.build ? 1 : 0, agents = (size_t)b.agents;
    const struct { const void *src; size_t words; } part[] = {
        {ctx->bbox.p, nag * b.S * 6 * NSEG}, {b.kept ? ctx->maxhalf_kept.p : b.maxhalf, grid * b.S * NSEG * 3}, {b.start, grid * b.S * NSEG * ((size_t)b.ncell + 1)},
        {b.ent, grid * 2 * b.S * NSEG * nag * 4}, {ctx->nbr_cnt.p, agents * b.parts}, {ctx->nbr_list.p, agents * b.cap},
        {ctx->close_cnt.p, b.close_cap ? agents : 0}, {ctx->close_list.p, agents * b.close_cap * 2}};
    size_t words = 0;
    for (const auto &q : part) words += q.words;
    if (out_bytes < words * 4) { ctx->err = "dmpc_debug_read_grid: the buffer is too small (" + std::to_string(words * 4) + " bytes)"; return -1; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    char *dst = (char *)out;
    for (const auto &q : part) {
        if (q.words) HIPCHK(ctx, hipMemcpy(dst, q.src, q.words * 4, hipMemcpyDeviceToHost));
        dst += q.words * 4;
    }
    return 0;
}

// force the solve launch order (a permutation of the S*c_count agents of the next launches; n = 0 returns to the built-in policy).  Used to
// measure what an ideal order would give.
extern "C" int dmpc_debug_set_order(dmpc_ctx *ctx, const int *host_order, int n)
{
    if (!ctx) return -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->forced_n = 0;
    if (n > 0 && host_order) {
        if (ctx->forced_order.ensure(sizeof(int) * (size_t)n)) { ctx->err = "dmpc_debug_set_order: out of device memory"; return -1; }
        HIPCHK(ctx, hipMemcpy(ctx->forced_order.p, host_order, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
        ctx->forced_n = n;
    }
    return 0;
}
