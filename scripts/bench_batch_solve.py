"""Instances per second of a test set solved one instance per call (``pipeline.solve_tsp`` / ``solve_mis`` in a loop, the
reference's batch size 1) against many instances per pass (``solve_tsp_batch`` / ``solve_mis_batch``), split by stage.

    python scripts/bench_batch_solve.py [--out profiles/r07/batch_solve.json] [--only tsp500] [--mode batch] [--P 1 4]
                                        [--merge_method batched]

Synthetic weights (H 256, 12 layers, categorical) and synthetic instances (uniform points; ER graphs); the numbers are
throughput, the answers are not looked at (the GPU tests pin them to the solo calls).  Every workload runs a small warm-up
of both modes first; the clock then covers the whole call with the device synchronised at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difusco_amd import MISModel, TSPModel  # noqa: E402
from difusco_amd.engine import DenoiseEngine  # noqa: E402
from difusco_amd.pipeline import solve_mis, solve_mis_batch, solve_tsp, solve_tsp_batch  # noqa: E402
from difusco_amd.synthetic import er_mis_edge_index, random_state_dict  # noqa: E402

WORKLOADS = {      # name: (task, n, sparse_factor, instances)
    "tsp50_dense": ("tsp", 50, -1, 64),
    "tsp500": ("tsp", 500, 50, 16),
    "tsp1000": ("tsp", 1000, 100, 8),
    "mis_er700_800": ("mis", None, None, 16),
}


def make_model(task, sparse_factor, steps, dev, engine):
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, n_layers=12, hidden_dim=256,
                inference_trick="ddim", inference_diffusion_steps=steps, inference_schedule="cosine",
                sparse_factor=sparse_factor if task == "tsp" else -1)
    return (TSPModel if task == "tsp" else MISModel)(args, engine=engine, seed=1)


def run(name, P, args, dev, engine):
    task, n, k, B = WORKLOADS[name]
    rng = np.random.default_rng(0)
    if task == "tsp":
        data = rng.random((B, n, 2))
    else:
        sizes = rng.integers(700, 801, size=B)
        data = [(int(s), er_mis_edge_index(int(s), 0.15, seed=i)) for i, s in enumerate(sizes)]
    m = make_model(task, k, args.steps, dev, engine)
    seeds = list(range(B))

    def solo(idx, timings):
        for b in idx:
            g = torch.Generator().manual_seed(int(b))
            if task == "tsp":
                solve_tsp(m, data[b], k, parallel_sampling=P, two_opt_iterations=args.two_opt, generator=g, timings=timings)
            else:
                solve_mis(m, data[b][0], data[b][1], parallel_sampling=P, generator=g, timings=timings)

    def batch(idx, timings):
        gens = [torch.Generator().manual_seed(int(b)) for b in idx]
        if task == "tsp":
            solve_tsp_batch(m, data[idx], k, parallel_sampling=P, two_opt_iterations=args.two_opt, seeds=[seeds[int(b)] for b in idx],
                            generators=gens, timings=timings, instances_per_call=args.per_call, merge_method=args.merge_method)
        else:
            solve_mis_batch(m, [data[b] for b in idx], parallel_sampling=P, seeds=[seeds[int(b)] for b in idx], generators=gens,
                            timings=timings, instances_per_call=args.per_call)

    rec = {"workload": name, "instances": B, "parallel_sampling": P, "inference_steps": args.steps,
           "merge_method": args.merge_method}
    for mode, fn in (("solo_loop", solo), ("batch", batch)):
        if args.mode not in ("both", mode):
            continue
        fn(list(range(min(2, B))), None)      # warm-up: workspaces, prepared state, library load
        torch.cuda.synchronize(dev)
        timings = {}
        t0 = time.perf_counter()
        fn(list(range(B)) if mode == "solo_loop" else np.arange(B), timings)
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
        rec[mode] = {"wall_s": round(wall, 4), "instances_per_s": round(B / wall, 3),
                     "stages_s": {k_: round(v, 4) for k_, v in sorted(timings.items())}}
    if "solo_loop" in rec and "batch" in rec:
        rec["speedup"] = round(rec["solo_loop"]["wall_s"] / rec["batch"]["wall_s"], 3)
        rec["stage_speedup"] = {s: round(rec["solo_loop"]["stages_s"][s] / max(rec["batch"]["stages_s"].get(s, 0), 1e-9), 3)
                                for s in rec["solo_loop"]["stages_s"]}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--P", nargs="*", type=int, default=[1, 4])
    ap.add_argument("--mode", choices=("both", "solo_loop", "batch"), default="both")
    ap.add_argument("--steps", type=int, default=50, help="inference diffusion steps")
    ap.add_argument("--two-opt", dest="two_opt", type=int, default=1000)
    ap.add_argument("--per-call", dest="per_call", type=int, default=None, help="instances_per_call (default: all)")
    ap.add_argument("--merge_method", choices=("loop", "batched"), default="loop", help="heatmap -> tour merge of the batch mode")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    engine = DenoiseEngine(random_state_dict(256, 12, 2, seed=0), device=dev)
    recs = [run(name, P, args, dev, engine) for name in args.only for P in args.P]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "records": recs}, f, indent=1)


if __name__ == "__main__":
    main()
