"""development: the launch sequence of one MPC step per case of tests/test_gpu_launch_plan.py, for a comparison of two builds of the library.

  rocprofv3 --kernel-trace --output-format csv -d DIR_A -- python tools/gpu_launch_trace.py                                   (this build)
  rocprofv3 --kernel-trace --output-format csv -d DIR_B -- python tools/with_lib.py OTHER.so tools/gpu_launch_trace.py        (another build)
  python tools/gpu_launch_trace.py --compare DIR_A DIR_B

The comparison is of the ordered lists of (kernel name, grid size, workgroup size, LDS bytes) per dispatch; it prints the first difference or
"identical" and exits 0 / 1.  Every case is a host-pointer step of one context (dmpc_step_batch): no child context, no second group.
--closed-loop (in place of the step cases): one small call of every closed-loop entry -- dmpc_transition, _cmd, _scripted, _mission, _hold, and
dmpc_transition / _mission in mixed precision -- each on one context and one stream (tools/gpu_transition_probe.py: single_context).
--postcheck (likewise): the calls of tools/gpu_postcheck_probe.py that enqueue on one stream -- every post-check entry on host and on resident
histories, the scenes of 300 agents on the cell grid with their brute-force pass (single_context there).
--step-entries (likewise): one small call of every single-step entry on one context each -- dmpc_init_batch, dmpc_step_batch, _cmd, dmpc_solve_one,
dmpc_step_device, _cmd in fp64 and mixed precision, dmpc_rows_one per variant (tools/gpu_step_probe.py: single_context)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dispatches(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        sys.exit(f"{directory}: expected one *kernel_trace.csv, found {files}")
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ") if "Grid_Size_X" in r else int(r["Grid_Size"]),
             tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ") if "Workgroup_Size_X" in r else int(r["Workgroup_Size"]),
             int(r["LDS_Block_Size"])) for r in rows]


def compare(dir_a, dir_b):
    a, b = dispatches(dir_a), dispatches(dir_b)
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            print(f"dispatch {i} differs:\n  {dir_a}: {x}\n  {dir_b}: {y}")
            return 1
    if len(a) != len(b):
        print(f"{len(a)} against {len(b)} dispatches; the first {min(len(a), len(b))} are equal")
        return 1
    print(f"identical: {len(a)} dispatches, {len(set(d[0] for d in a))} kernels")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if sys.argv[1:] == ["--closed-loop"]:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gpu_transition_probe as probe
        for name, r in probe.single_context(probe.scenes()):
            print(f"{name}: K_T_used {r['K_T_used'].tolist()} status {r['scene_status'].tolist()}", flush=True)
        sys.exit(0)
    if sys.argv[1:] == ["--postcheck"]:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gpu_postcheck_probe as probe
        for name, r in probe.single_context():
            print(f"{name}: {sum(v is not None for v in r.values())} arrays", flush=True)
        sys.exit(0)
    if sys.argv[1:] == ["--step-entries"]:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gpu_step_probe as probe
        for name, r in probe.single_context():
            print(f"{name}: {sum(v is not None for v in r.values())} arrays", flush=True)
        sys.exit(0)
    import test_gpu_launch_plan as plan
    c = plan.ncu()
    for cid, variant, precision, shape, opts, _ in plan.CASES:
        S, N = shape(c)
        name, _ = plan.run_case(variant, precision, S, N, opts)
        print(f"{cid}: S={S} N={N} {name}", flush=True)
