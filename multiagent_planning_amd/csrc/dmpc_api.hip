// dmpc_api.hip -- the root of libdmpc_hip.so's single translation unit (the C ABI declared in include/dmpc_hip.h and include/dmpc_hip_dev.h): a table
// of contents.  The build and the tools compile this file by name; it defines nothing itself.  The parts, in the order they need one another:
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dmpc_hip.h"
#include "../../include/dmpc_hip_dev.h"
#include "dmpc_device.h"

#include "dmpc_kernels.hip"          // the step's kernels: scan, order, solve (dmpc_solve.hip, dmpc_rsolve.hip), post-step, lists (dmpc_lists.hip)
#include "dmpc_postcheck.hip"        // the post-checks' kernels
#include "dmpc_rowbuild.hip"         // the dense row builders' kernels
#include "dmpc_generators.hip"       // the start / goal generators' kernel
#include "dmpc_context.hip"          // a context and its life: owner types, dmpc_ctx, FAIL / HIPCHK, create, destroy, set_params, profile, error and count readers
#include "dmpc_tables.hip"           // the model matrices and the device tables (pure host arithmetic, no HIP)
#include "dmpc_launch.hip"           // plan_step, the five stages, launch_step
#include "dmpc_step.hip"             // the single step: scratch, StepIO and mixed-precision helpers, the record of a host-pointer call, the step entries
#include "dmpc_debug.hip"            // development aids: trace, read probe, header and grid readers, forced order
#include "dmpc_plan.hip"             // route planning round static vehicles, before and during a flight: the wavefront planner's kernels, the three entries
#include "dmpc_disturb.hip"          // disturbed transitions: the rule on the host and the device, the descriptor's check and upload, the three entries
#include "dmpc_feedback.hip"         // event-triggered feedback: the rule on the host and the device, the post step with it, the re-anchoring, the four entries; the measurement model (dmpc_set_measurement) and its five
#include "dmpc_start.hip"            // a flight from a given or carried state and plan: the braking plan, the gather of a flight's end, the four entries
#include "dmpc_transition.hip"       // the closed loop: batch_parts, the record of a call, transition_one, transition_any, the seven entries
#include "dmpc_postcheck_host.hip"   // the post-checks on the host: the record of a call, PcPrep, the three checks, pc_run, the five entries
#include "dmpc_fileio.hip"           // the reference's text files
#include "dmpc_multigpu.hip"         // several GPUs: the RCCL transport and the one-process group
#include "dmpc_assign.hip"           // goal assignment: the auction's kernels and the four entries
#include "dmpc_hostforms.hip"        // host-pointer forms of small things: dense row builders, generators, the path's helpers and their kernels
