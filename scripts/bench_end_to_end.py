#!/usr/bin/env python
"""Whole inference flow of the reference's test_step on the GPU path (difusco_amd.pipeline.solve_tsp): k-NN graph ->
50-step sampling of `parallel_sampling` noise samples -> merge -> 2-opt, per-stage wall time.  Random-init weights
(no checkpoints offline): the tours are only as good as 2-opt makes them; the point is the time split.  One JSON line.
``--two_opt_methods exact screened`` runs every case once per 2-opt method (same model, same seed: same tours);
``--tsp10000_cap`` sets the 2-opt cap of the TSP-10000 case (the reference's command uses 5000)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difusco_amd.models import TSPModel  # noqa: E402
from difusco_amd.pipeline import solve_tsp  # noqa: E402
from difusco_amd.synthetic import random_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--two_opt_methods", nargs="+", default=["exact"], choices=["exact", "screened"])
ap.add_argument("--tsp10000_cap", type=int, default=1000)
ap.add_argument("--sizes", nargs="+", type=int, default=[1000, 10000], choices=[1000, 10000])
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
opts = ap.parse_args()

dev = torch.device("cuda:0")
out = {"data": "synthetic, random-init weights", "cases": []}
for n, k, par, cap in ((1000, 100, 8, 1000), (10000, 100, 1, opts.tsp10000_cap)):
    if n not in opts.sizes:
        continue
    params = random_state_dict(256, 12, 2, seed=1)
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=k, n_layers=12,
                hidden_dim=256, inference_trick="ddim", inference_diffusion_steps=50, inference_schedule="cosine")
    pts = np.random.default_rng(n).random((n, 2))
    tours = {}
    for method in opts.two_opt_methods:
        m = TSPModel(args, params, device=dev, seed=7)            # a fresh engine per method: the same draws in both calls
        solve_tsp(m, pts, k, parallel_sampling=par, two_opt_iterations=2, two_opt_method=method,
                  generator=torch.Generator().manual_seed(0))                                 # warm-up
        t = {}
        tour, cost, costs, info = solve_tsp(m, pts, k, parallel_sampling=par, two_opt_iterations=cap, timings=t,
                                            two_opt_method=method, generator=torch.Generator().manual_seed(0))
        tours[method] = (tour, info["two_opt_iterations"])
        out["cases"].append({"workload": f"TSP-{n} K={k}, parallel_sampling={par}, 50 steps, 2-opt cap {cap}",
                             "two_opt_method": method,
                             "seconds": {a: round(b, 4) for a, b in t.items()}, "total_s": round(sum(t.values()), 4),
                             "two_opt_moves": info["two_opt_iterations"], "merge_iterations": info["merge_iterations"],
                             "best_cost": cost, "merged_cost_mean": float(np.mean(info["merged_costs"]))})
    if len(tours) == 2:
        out["cases"][-1]["same_tour_and_moves_as_exact"] = bool(tours["exact"] == tours["screened"])
print(json.dumps(out))
if opts.out:
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
