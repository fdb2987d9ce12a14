"""development: what the rectangular goal assignment costs -- dmpc_assign_rect_device timed with HIP events (torch.cuda.Event on the stream the
call is enqueued on; one launch per call, device arrays, no copies) at the default eps = 1e-4 / max(N, M) on random_test scenes in the C2
density box of max(N, M) points (the first N starts, the first M goals):
  (S, N, M) = (512, 80, 100), (512, 100, 80), (1, 300, 1000), (1, 1000, 300), (1, 900, 1024)
  and the square (512, 100, 100) through dmpc_assign_rect_device AND dmpc_assign_goals_device, interleaved on the same scenes: their ratio per
  repetition
Every timing brackets `calls` calls back to back; prints median, minimum and maximum per call over the repetitions, the round counts -- the
device's total, and the forward / reverse split from the numpy restatement (tests/assign_rect.py) on the first `split` scenes, whose total must
equal the device's --, microseconds per round of the slowest scene, and scipy.optimize.linear_sum_assignment on one CPU core on the same scenes
(cost matrix included) as a stated baseline.  Text, and one JSON line.
usage: python tools/gpu_assign_rect_time.py [repetitions [calls [split]]]"""
import sys, os, json, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiagent_planning_amd as mp
from multiagent_planning_amd import workload as wl
import assign_rect as ar
from scipy.optimize import linear_sum_assignment  # noqa: F401  (loaded before it is timed)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
split = int(sys.argv[3]) if len(sys.argv) > 3 else 512
dev = torch.device("cuda")
cfg = wl.CONFIGS["C2"]
SHAPES = [(512, 80, 100), (512, 100, 80), (1, 300, 1000), (1, 1000, 300), (1, 900, 1024), (512, 100, 100)]


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return [int(a.min()), round(float(a.mean()), 1), int(a.max())]


def timed(runs, stream):
    """per repetition and per run of `runs`: milliseconds per call, the runs interleaved"""
    ms = np.zeros((reps, len(runs)))
    for r in range(reps):
        for k, run in enumerate(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                run()
            e1.record(stream)
            e1.synchronize()
            ms[r, k] = e0.elapsed_time(e1) / calls
    return ms


out = {"repetitions": reps, "calls_per_timing": calls, "shapes": []}
for S, N, M in SHAPES:
    X = max(N, M)
    kw = wl.solver_kwargs(cfg, X)
    d = mp.Dmpc("bound", **kw)
    po, g = wl.make_scenes_device(d, cfg, S, X, seed=wl.SEED0 + 7 * N + M)
    po, g = np.ascontiguousarray(po[:, :N]), np.ascontiguousarray(g[:, :M])
    eps = 1e-4 / X
    tpo, tg = torch.from_numpy(po).to(dev), torch.from_numpy(g).to(dev)
    rounds, rounds_sq = (torch.zeros((S,), dtype=torch.int32, device=dev) for _ in range(2))
    cost = torch.zeros((S,), dtype=torch.float64, device=dev)
    perm, owner = torch.zeros((S, N), dtype=torch.int32, device=dev), torch.zeros((S, M), dtype=torch.int32, device=dev)
    pf, price = torch.zeros((S, N, 3), dtype=torch.float64, device=dev), torch.zeros((S, X), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream()
    rect = lambda: d.assign_rect_device(S, N, M, tpo.data_ptr(), tg.data_ptr(), eps, 0, perm.data_ptr(), owner.data_ptr(), pf.data_ptr(),
                                        price.data_ptr(), cost.data_ptr(), rounds.data_ptr(), stream=stream.cuda_stream)
    square = lambda: d.assign_goals_device(S, N, tpo.data_ptr(), tg.data_ptr(), eps, 0, perm.data_ptr(), pf.data_ptr(), price.data_ptr(),
                                           cost.data_ptr(), rounds_sq.data_ptr(), stream=stream.cuda_stream)
    runs = [rect, square] if N == M else [rect]
    for _ in range(3):
        for run in runs:
            run()
    torch.cuda.synchronize()
    ms = timed(runs, stream)
    r = rounds.cpu().numpy()
    assert (r > 0).all()
    k = min(S, split)
    ref = [ar.auction_rect(po[s], g[s], cfg["c"], eps) for s in range(k)]
    assert [x["rounds"] for x in ref] == r[:k].tolist(), "the device's round counts are not the restatement's"
    t0 = time.perf_counter()
    opt = np.array([ar.optimum_rect(po[s], g[s], cfg["c"]) for s in range(S)])
    lsa = time.perf_counter() - t0
    gap = float((cost.cpu().numpy() - opt).max())
    med = float(np.median(ms[:, 0]))
    rec = {"S": S, "N": N, "M": M, "median_ms": round(med, 4), "min_ms": round(float(ms[:, 0].min()), 4), "max_ms": round(float(ms[:, 0].max()), 4),
           "rounds": stats(r), "forward": stats([x["fwd"] for x in ref]), "reverse": stats([x["rev"] for x in ref]), "split_scenes": k,
           "us_per_round_slowest": round(1e3 * med / float(r.max()), 3), "lsa_one_core_s": round(lsa, 4), "cost_minus_optimum_worst": gap}
    line = (f"({S}, {N}, {M}): {med:.4f} ms per call (min {ms[:, 0].min():.4f}, max {ms[:, 0].max():.4f}; {reps} x {calls} calls), rounds min/mean/max "
            f"{rec['rounds']}, forward {rec['forward']} reverse {rec['reverse']} (first {k} scenes), {rec['us_per_round_slowest']} us per round of the "
            f"slowest scene, linear_sum_assignment {lsa:.4f} s, cost - optimum (worst) {gap:.2e}")
    if N == M:
        assert np.array_equal(r, rounds_sq.cpu().numpy())
        ratio = ms[:, 0] / ms[:, 1]
        rec.update(goals_median_ms=round(float(np.median(ms[:, 1])), 4), goals_min_ms=round(float(ms[:, 1].min()), 4),
                   goals_max_ms=round(float(ms[:, 1].max()), 4), ratio_median=round(float(np.median(ratio)), 4),
                   ratio_min=round(float(ratio.min()), 4), ratio_max=round(float(ratio.max()), 4))
        line += (f"; dmpc_assign_goals_device {np.median(ms[:, 1]):.4f} ms (min {ms[:, 1].min():.4f}, max {ms[:, 1].max():.4f}), rect / goals "
                 f"{np.median(ratio):.4f} (min {ratio.min():.4f}, max {ratio.max():.4f})")
    print(line, flush=True)
    out["shapes"].append(rec)
    d.close()
print(json.dumps(out))
