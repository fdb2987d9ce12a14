"""development: what goal assignment costs -- dmpc_assign_rect_device and dmpc_assign_goals_device timed with HIP events (torch.cuda.Event on
the stream the call is enqueued on; device arrays, no copies) at the default eps = 1e-4 / max(N, M) on random_test scenes in the C2 density box
of max(N, M) points (the first N starts, the first M goals):
  dmpc_assign_rect_device   (S, N, M) = (512, 80, 100), (512, 100, 80), (1, 300, 1000), (1, 1000, 300), (1, 900, 1024)
  dmpc_assign_goals_device  (S, N) = (512, 100), (512, 256), (64, 512), (1, 1024) -- one launch per call -- and (1, 1100), the round launches
Every timing brackets `calls` calls back to back; prints median, minimum and maximum per call over the repetitions, the round counts -- the
device's total, and the forward / reverse split from the numpy restatement (tests/assign_rect.py) on the first `split` scenes, whose total must
equal the device's --, microseconds per round of the slowest scene, and scipy.optimize.linear_sum_assignment on one CPU core on the same scenes
(cost matrix included) as a stated baseline.  Text, and one JSON line.  Run on two commits in turn, it is their before / after table.
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
# (S, N, M); M = None: N goals through dmpc_assign_goals_device
SHAPES = [(512, 80, 100), (512, 100, 80), (1, 300, 1000), (1, 1000, 300), (1, 900, 1024),
          (512, 100, None), (512, 256, None), (64, 512, None), (1, 1024, None), (1, 1100, None)]


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return [int(a.min()), round(float(a.mean()), 1), int(a.max())]


def timed(run, stream):
    """per repetition: milliseconds per call"""
    ms = np.zeros(reps)
    for r in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            run()
        e1.record(stream)
        e1.synchronize()
        ms[r] = e0.elapsed_time(e1) / calls
    return ms


out = {"repetitions": reps, "calls_per_timing": calls, "shapes": []}
for S, N, M in SHAPES:
    entry = "dmpc_assign_goals_device" if M is None else "dmpc_assign_rect_device"
    square, M = M is None, N if M is None else M
    X = max(N, M)
    kw = wl.solver_kwargs(cfg, X)
    d = mp.Dmpc("bound", **kw)
    po, g = wl.make_scenes_device(d, cfg, S, X, seed=wl.SEED0 + 7 * N + M)
    po, g = np.ascontiguousarray(po[:, :N]), np.ascontiguousarray(g[:, :M])
    eps = 1e-4 / X
    tpo, tg = torch.from_numpy(po).to(dev), torch.from_numpy(g).to(dev)
    rounds = torch.zeros((S,), dtype=torch.int32, device=dev)
    cost = torch.zeros((S,), dtype=torch.float64, device=dev)
    perm, owner = torch.zeros((S, N), dtype=torch.int32, device=dev), torch.zeros((S, M), dtype=torch.int32, device=dev)
    pf, price = torch.zeros((S, N, 3), dtype=torch.float64, device=dev), torch.zeros((S, X), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream()
    if square:
        run = lambda: d.assign_goals_device(S, N, tpo.data_ptr(), tg.data_ptr(), eps, 0, perm.data_ptr(), pf.data_ptr(), price.data_ptr(),
                                            cost.data_ptr(), rounds.data_ptr(), stream=stream.cuda_stream)
    else:
        run = lambda: d.assign_rect_device(S, N, M, tpo.data_ptr(), tg.data_ptr(), eps, 0, perm.data_ptr(), owner.data_ptr(), pf.data_ptr(),
                                           price.data_ptr(), cost.data_ptr(), rounds.data_ptr(), stream=stream.cuda_stream)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = timed(run, stream)
    r = rounds.cpu().numpy()
    assert (r > 0).all()
    k = min(S, split)
    ref = [ar.auction_rect(po[s], g[s], cfg["c"], eps) for s in range(k)]
    assert [x["rounds"] for x in ref] == r[:k].tolist(), "the device's round counts are not the restatement's"
    t0 = time.perf_counter()
    opt = np.array([ar.optimum_rect(po[s], g[s], cfg["c"]) for s in range(S)])
    lsa = time.perf_counter() - t0
    gap = float((cost.cpu().numpy() - opt).max())
    med = float(np.median(ms))
    rec = {"entry": entry, "S": S, "N": N, "M": M, "median_ms": round(med, 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
           "rounds": stats(r), "forward": stats([x["fwd"] for x in ref]), "reverse": stats([x["rev"] for x in ref]), "split_scenes": k,
           "us_per_round_slowest": round(1e3 * med / float(r.max()), 3), "lsa_one_core_s": round(lsa, 4), "cost_minus_optimum_worst": gap}
    print(f"{entry} ({S}, {N}{'' if square else f', {M}'}): {med:.4f} ms per call (min {ms.min():.4f}, max {ms.max():.4f}; {reps} x {calls} calls), "
          f"rounds min/mean/max {rec['rounds']}, forward {rec['forward']} reverse {rec['reverse']} (first {k} scenes), {rec['us_per_round_slowest']} us "
          f"per round of the slowest scene, linear_sum_assignment {lsa:.4f} s, cost - optimum (worst) {gap:.2e}", flush=True)
    out["shapes"].append(rec)
    d.close()
print(json.dumps(out))
