/* dmpc_hip_dev.h -- DEVELOPMENT interface of libdmpc_hip.so: what the test suite and the probes under tools/ use to select launch forms,
 * emulate ranks and read internal records.  NOT part of the drop-in boundary (include/dmpc_hip.h): nothing here replaces a reference
 * interface, none of it changes a result beyond solver round-off (most not a bit: tests/test_gpu_paths.py), and it may change between
 * rounds.  Exported so that the checks run against the PRODUCT binary instead of a special build. */
#ifndef DMPC_HIP_DEV_H
#define DMPC_HIP_DEV_H
#include "dmpc_hip.h"
/* dmpc_assign_goals: scenes of up to this many agents run their whole auction in one launch, one workgroup per scene with prices and
 * ownership in LDS; larger scenes take two launches per round.  The result is the same bits on either side (tests/test_gpu_assign.py runs both).
 * dmpc_assign_rect: the largest max(N, M) it accepts (it has the one-launch path only). */
#define DMPC_ASSIGN_ONE_LAUNCH_MAX 1024
#ifdef __cplusplus
extern "C" {
#endif
/* launch forms / tiers / pre-passes of a context by name (the list: INTEGRATION.md section 6); also through ONE environment variable read at
 * context creation, DMPC_DEBUG_OPTIONS="name=value,..." */
DMPC_API int dmpc_debug_option(dmpc_ctx *ctx, const char *name, int value);
/* DMPC_DEVICE_ALL contexts created from now on run n ranks that all sit on the calling thread's current device (0: off) -- the
 * single-process multi-GPU protocol on a one-GPU box */
DMPC_API int dmpc_debug_emulate_devices(int n);
/* a context without a communicator acts as rank `rank` of `nranks` (the ranks of a job run one after the other on one GPU) */
DMPC_API int dmpc_debug_set_rank(dmpc_ctx *ctx, int nranks, int rank);
/* DEV_TRACE builds: per-iteration trace of one agent / per-wave and per-agent clocks (agent = -2, -3, -5) / crash statistics (-4) */
DMPC_API int dmpc_debug_trace(dmpc_ctx *ctx, int agent, int cap, double *host_out);
/* the scan's hand-off headers of the last step (8 ints per agent) */
DMPC_API int dmpc_debug_read_hdr(dmpc_ctx *ctx, int *host_out, int n_agents);
/* the neighbour-list build of the last step that built lists.  shape[12] = S, G, C, cells along x, y, z, ncell, build (0: all-pairs box test,
 * no cell grid; 1: the five kernels; 2: the two launches of one scene), list capacity, close capacity, agents of the launch (S * c_count),
 * pieces per list count.  out = NULL: the shape alone.  Otherwise these arrays as 4-byte words, one behind the other (the cell grid's are
 * empty with build = 0, the close pairs' with a close capacity of 0): bbox [G][S][18][C], largest half extents [S][3][3] (as the build left them if
 * this entry had been called on the context before the step -- a refused call will do: such a context keeps a copy, one device-to-device copy per
 * build; otherwise zeros after build 2, whose counters the step's scan kernel sets back for the next step), start
 * [S][3][ncell + 1], entry records [2][S][3][G C][4] (the two 16-byte halves), nbr_cnt [agents][pieces], nbr_list [agents][capacity],
 * close_cnt [agents], close_list [agents][close capacity][2].  Refused before any list build and when out_bytes is too small. */
DMPC_API int dmpc_debug_read_grid(dmpc_ctx *ctx, int *shape, void *out, size_t out_bytes);
/* the scan's own records of ONE agent (column n of the table; host pointers, one wave, as dmpc_rows_one) as a step of this context forms them:
 * a DMPC_PREC_MIXED context on the fp32 copy of the table, with the float instantiation of the scan and the row builder.  prune = 0: every row
 * the reference builds; 1: the step's exact pruning.  hdr[8]: rows kept, the reference's row count, viol_k, status (DMPC_ST_INFEAS from the
 * slack-free variants' certificate), flags (1: violation, 4: the cpp flavour's collision flag), rows_exist, first retry-ladder level that is not
 * certainly infeasible, launch-order key.  The first min(hdr[0], max_rows) kept rows in the reference's order: xi[3], rhs, kc (1-based), slack
 * coefficient, slack cost term, slack lower bound (zeros for the slack-free variants).  Order 2 only, not DMPC_VAR_SCP
 * (tests/test_gpu_mixed_rows.py). */
DMPC_API int dmpc_debug_scan_rows(dmpc_ctx *ctx, int N, int n, const double *l, const double *po, const double *vo, int prune, int max_rows,
                                  int32_t *hdr, double *xi, double *rhs, int32_t *kc, double *slack_coef, double *slack_term, double *slack_lb);
/* force the solve launch order of the next launches (n = 0: the built-in policy) */
DMPC_API int dmpc_debug_set_order(dmpc_ctx *ctx, const int *host_order, int n);
/* a coalesced streaming read of `bytes` bytes at 8 or 16 bytes per lane, `reps` launches: the known byte count rocprofv3's FETCH_SIZE is
 * calibrated on (tools/gpu_fetch_calib.py) */
DMPC_API int dmpc_debug_read_probe(dmpc_ctx *ctx, size_t bytes, int lane_bytes, int reps);
#ifdef __cplusplus
}
#endif
#endif
