#!/usr/bin/env python
"""Tour refinement timing on the GPU box: the exact 2-opt (``batched_two_opt_torch``) beside the 2-opt + Or-opt local search
(``batched_local_search_torch``) from the decoded start tour of ``scripts/bench_decode.py`` (TSP-N, K = 100, synthetic heat),
N = 10^3 and 10^4, cap 200 and 5000 moves per phase.  Prints one JSON line (``--out PATH`` also writes it).

Three runs per repeat, interleaved in this one process after a warm-up of each:
  two_opt        the exact 2-opt from the start tour: ms per applied move (the code of the parent commit, unchanged);
  local_search   the local search from the same start tour: its time, counters and tour length;
  or_opt_phase   one round of the local search from the 2-opt-CONVERGED tour: one 2-opt sweep that applies nothing, then the
                 Or-opt phase alone.  ms per Or-opt move = (time - one 2-opt move's time) / Or-opt sweeps, a sweep per counted
                 iteration plus the one that finds nothing when the phase ends below the cap.
An Or-opt sweep evaluates n^2 (i, j) pairs of 30 float64 operations (two distances of 2 sub, 2 mul, 1 add, 1 sqrt; 3 + 5 x 3
additions), none of them fused: ``fp64_vector_fraction`` holds that rate against the 78.6 TFLOP/s FP64 vector peak of the MI355X,
which counts a fused multiply-add as two."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difusco_amd.decode import batched_local_search_torch, batched_two_opt_torch, merge_tours  # noqa: E402
from difusco_amd.synthetic import tsp_instance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sizes", nargs="+", type=int, default=[1000, 10000], choices=[1000, 10000])
ap.add_argument("--max_rounds", type=int, default=16)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
opts = ap.parse_args()

FP64_VECTOR_PEAK = 78.6e12
OPS_PER_PAIR = 30
dev = torch.device("cuda:0")
out = {"metric": "ms per applied move", "unit": "ms", "data": "synthetic", "repeats": opts.repeats, "cases": []}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def spread(ms):
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "all": ms}


for n in opts.sizes:
    k = 100
    pts, ei = tsp_instance(n, k, seed=11)
    rng = np.random.default_rng(n)
    d = np.linalg.norm(pts[ei[0]] - pts[ei[1]], axis=1)
    heat = (np.exp(-d / (0.5 * d.mean())) * rng.random(ei.shape[1])).astype(np.float32) + np.float32(1e-6)
    tours, _ = merge_tours(torch.from_numpy(heat).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(ei).to(dev),
                           sparse_graph=True, device=dev)
    tour0 = np.asarray(tours, dtype=np.int64)
    pts64 = pts.astype(np.float64)
    length = lambda t: float(np.linalg.norm(pts64[t[:-1]] - pts64[t[1:]], axis=1).sum())
    cap = 200 if n <= 1000 else 5000
    converged, conv_moves = batched_two_opt_torch(pts64, tour0, max_iterations=10 ** 6, device=dev)
    batched_two_opt_torch(pts64, tour0, max_iterations=10, device=dev)                        # warm-up
    batched_local_search_torch(pts64, tour0, max_iterations=10, device=dev, max_rounds=2)
    two, ls, phase = [], [], []
    for _ in range(opts.repeats):                                                             # interleaved: same clocks for all
        t, (refined, moves) = timed(lambda: batched_two_opt_torch(pts64, tour0, max_iterations=cap, device=dev))
        two.append(t / max(moves, 1))
        s_ls = {}
        t, (searched, a) = timed(lambda: batched_local_search_torch(pts64, tour0, max_iterations=cap, device=dev,
                                                                    max_rounds=opts.max_rounds, stats=s_ls))
        ls.append(t)
        s_ph = {}
        t, (polished, a_ph) = timed(lambda: batched_local_search_torch(pts64, converged, max_iterations=cap, device=dev,
                                                                       max_rounds=1, stats=s_ph))
        b = s_ph["or_opt_iterations"]
        sweeps = b + (1 if b < cap else 0)
        phase.append((t - two[-1]) / sweeps)
    or_ms = float(np.median(phase))
    case = {"workload": f"TSP-{n} K={k}, decoded start tour", "cap": cap, "max_rounds": opts.max_rounds,
            "tour_length_start": length(tour0[0]),
            "two_opt": {"moves": int(moves), "ms_per_move": spread(two), "tour_length_after": length(refined[0]),
                        "pairs_per_sweep": n * (n - 3) // 2, "converged_after_moves": int(conv_moves),
                        "tour_length_converged": length(converged[0])},
            "local_search": {"two_opt_iterations": int(a), "or_opt_iterations": s_ls["or_opt_iterations"], "rounds": s_ls["rounds"],
                             "ms": spread(ls), "tour_length_after": length(searched[0]),
                             "length_over_two_opt": length(searched[0]) / length(refined[0])},
            "or_opt_phase": {"start": "the 2-opt-converged tour", "two_opt_moves": int(a_ph), "or_opt_iterations": b,
                             "sweeps": sweeps, "ms_per_move": spread(phase), "pairs_per_sweep": n * n,
                             "tour_length_after": length(polished[0]),
                             "over_two_opt_ms_per_move": or_ms / float(np.median(two)),
                             "fp64_ops_per_s": n * n * OPS_PER_PAIR / (1e-3 * or_ms),
                             "fp64_vector_fraction": n * n * OPS_PER_PAIR / (1e-3 * or_ms) / FP64_VECTOR_PEAK}}
    out["cases"].append(case)
print(json.dumps(out))
if opts.out:
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
