"""The heatmap -> tour merge of ``solve_tsp_batch`` with ``merge_method="loop"`` (one library call per instance, the host
walk) against ``"batched"`` (``difusco_tsp_merge_batch``: one launch sequence per chunk, the walk on the GPU).

    python scripts/bench_merge_batch.py [--out-dir profiles/batched_merge] [--only tsp50_dense_p1 ...] [--repeats 5]

Synthetic weights (H 256, 12 layers, categorical), 50 steps, uniform points; the answers are not looked at
(tests/test_gpu_merge_batch.py pins the two methods to each other).  Per workload both methods run in one process: one untimed
pass of each, then ``--repeats`` timed passes with the methods interleaved; the clock covers the whole call and ends in a device
synchronise.  Reported per method: median (min, max) of the ``merge`` stage in ms, of the whole call in ms and of instances/s.

  tsp50_dense_p1 / _p4   64 dense TSP-50 instances, P = 1 / 4 (array form)
  tsp500_k50             16 TSP-500 instances, K = 50, P = 1 (array form)
  dense_20_100           64 dense instances, n uniform in 20..100 (list form; the set of bench_mixed_solve.py)
  sparse_300_700         16 sparse instances, K = 50, n in 300..700 (list form)
  tsp10000_single        the merge alone on one TSP-10000 / K = 100 sample with a synthetic heatmap: ``decode.merge_tours``
                         against ``decode.merge_tours_batch`` with the path state in LDS (state "auto" at this size) and in
                         the workspace (state "global")"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difusco_amd import TSPModel  # noqa: E402
from difusco_amd.decode import MERGE_METHODS, merge_tours, merge_tours_batch  # noqa: E402
from difusco_amd.engine import DenoiseEngine  # noqa: E402
from difusco_amd.pipeline import solve_tsp_batch  # noqa: E402
from difusco_amd.synthetic import random_state_dict, tsp_instance  # noqa: E402

SOLVE = {      # name: (sparse_factor, instances, n_lo, n_hi, P)
    "tsp50_dense_p1": (-1, 64, 50, 50, 1),
    "tsp50_dense_p4": (-1, 64, 50, 50, 4),
    "tsp500_k50": (50, 16, 500, 500, 1),
    "dense_20_100": (-1, 64, 20, 100, 1),
    "sparse_300_700": (50, 16, 300, 700, 1),
}


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def run_solve(name, args, dev, engine):
    k, B, lo, hi, P = SOLVE[name]
    rng = np.random.default_rng(0)
    if lo == hi:
        sizes, data = [lo] * B, rng.random((B, lo, 2))
    else:
        sizes = [int(n) for n in rng.integers(lo, hi + 1, size=B)]
        data = [rng.random((n, 2)) for n in sizes]
    margs = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, n_layers=12, hidden_dim=256,
                 inference_trick="ddim", inference_diffusion_steps=args.steps, inference_schedule="cosine", sparse_factor=k)
    m = TSPModel(margs, engine=engine, seed=1)

    def solve(method, t):
        solve_tsp_batch(m, data, k, parallel_sampling=P, two_opt_iterations=args.two_opt, seeds=list(range(B)),
                        generators=[torch.Generator().manual_seed(b) for b in range(B)], timings=t, step_offset=0,
                        merge_method=method)

    for method in MERGE_METHODS:                                 # one untimed pass of each
        solve(method, None)
    torch.cuda.synchronize(dev)
    walls, merges = {mm: [] for mm in MERGE_METHODS}, {mm: [] for mm in MERGE_METHODS}
    for _ in range(args.repeats):
        for method in MERGE_METHODS:                             # interleaved
            t = {}
            t0 = time.perf_counter()
            solve(method, t)
            torch.cuda.synchronize(dev)
            walls[method].append(time.perf_counter() - t0)
            merges[method].append(t["merge"])
    rec = {"workload": name, "instances": B, "sparse_factor": k, "n": sizes if lo != hi else lo, "parallel_sampling": P,
           "inference_steps": args.steps, "two_opt_iterations": args.two_opt, "repeats": args.repeats}
    for method in MERGE_METHODS:
        rec[method] = {"merge_ms": spread([1e3 * v for v in merges[method]]), "wall_ms": spread([1e3 * w for w in walls[method]]),
                       "instances_per_s": spread([B / w for w in walls[method]])}
    rec["merge_loop_over_batched"] = round(rec["loop"]["merge_ms"]["median"] / rec["batched"]["merge_ms"]["median"], 3)
    rec["wall_loop_over_batched"] = round(rec["loop"]["wall_ms"]["median"] / rec["batched"]["wall_ms"]["median"], 3)
    return rec


def run_single(args, dev):
    n, k = 10000, 100
    pts, ei = tsp_instance(n, k, seed=3)
    rng = np.random.default_rng(0)
    d = np.linalg.norm(pts[ei[0]] - pts[ei[1]], axis=1)
    heat = (np.exp(-d / (0.5 * d.mean())) * rng.random(ei.shape[1])).astype(np.float32) + np.float32(1e-6)
    heat_d, pts_d, ei_d = torch.from_numpy(heat).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(ei).to(dev)

    def loop():
        return merge_tours(heat_d, pts_d, ei_d, sparse_graph=True, device=dev, return_completed=True)

    def batched(state="auto"):
        return merge_tours_batch([heat_d], [pts_d], [ei_d], sparse_graph=True, device=dev, return_completed=True, state=state)[0]

    fns = {"loop": loop, "batched": batched, "batched_global": lambda: batched("global")}
    res = {mm: fn() for mm, fn in fns.items()}                   # one untimed pass of each
    ms = {mm: [] for mm in fns}
    for _ in range(args.repeats):
        for mm, fn in fns.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            ms[mm].append(1e3 * (time.perf_counter() - t0))
    rec = {"workload": "tsp10000_single", "n": n, "sparse_factor": k, "parallel_sampling": 1, "repeats": args.repeats,
           "same_result": res["loop"] == res["batched"] == res["batched_global"], "completed": res["loop"][2],
           **{mm: {"merge_ms": spread(ms[mm])} for mm in fns}}
    rec["merge_loop_over_batched"] = round(rec["loop"]["merge_ms"]["median"] / rec["batched"]["merge_ms"]["median"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", dest="out_dir", default=None)
    ap.add_argument("--only", nargs="*", default=list(SOLVE) + ["tsp10000_single"])
    ap.add_argument("--steps", type=int, default=50, help="inference diffusion steps")
    ap.add_argument("--two-opt", dest="two_opt", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_merge_batch measures on the GPU: no device found")
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3")
    dev = torch.device("cuda:0")
    engine = None
    for name in args.only:
        if name == "tsp10000_single":
            rec = run_single(args, dev)
        else:
            engine = engine or DenoiseEngine(random_state_dict(256, 12, 2, seed=0), device=dev)
            rec = run_solve(name, args, dev, engine)
        rec["device"] = torch.cuda.get_device_name(dev)
        print(json.dumps(rec), flush=True)
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, name + ".json"), "w") as f:
                json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
