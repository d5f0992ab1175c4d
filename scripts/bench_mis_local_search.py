#!/usr/bin/env python
"""MIS refinement timing on the GPU box: the greedy decode (``mis_decode_np``) alone beside decode + swap local search
(``mis_local_search_np``) on the union the MIS workload of BASELINE.json hands one GPU: 16 Erdos-Renyi graphs G(n, 0.15),
n ~ U{700..800} (the graphs of ``bench.py``), as P = 1 and P = 4 copies.  Prints one JSON line (``--out PATH`` also writes it).

The scores are SYNTHETIC (uniform random per node and copy, not a trained checkpoint's heatmap): the sizes say what the rule does
on such scores, not what it gains on a trained model.

Per repeat, interleaved in this one process after a warm-up of each:
  decode        ``mis_decode_np`` on the union's CSR and device scores (the code of the parent commit, unchanged);
  local_search  ``mis_local_search_np`` from the decoded set on the same CSR and scores: its time, counters and sizes.
Both include the copy of the 0/1 array to the host, as ``solve_mis_batch`` pays it.  ``sampling_50_steps_ms``: one 50-step
``MISModel.sample`` of the same batch (12 layers, hidden 256, random weights), the stage the decode follows in the pipeline."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difusco_amd.decode import mis_decode_np, mis_local_search_np  # noqa: E402
from difusco_amd.graph import build_csr  # noqa: E402
from difusco_amd.synthetic import er_mis_edge_index, random_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--graphs", type=int, default=16)
ap.add_argument("--parallel", nargs="+", type=int, default=[1, 4])
ap.add_argument("--max_rounds", type=int, default=1000)
ap.add_argument("--no_sampling", action="store_true", help="skip the 50-step sampling time")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
opts = ap.parse_args()

dev = torch.device("cuda:0")
out = {"metric": "ms per call on the union", "unit": "ms", "box": "one MI355X (gfx950)", "data": "synthetic",
       "scores": "uniform random per node and copy (synthetic: not a trained checkpoint's heatmap; no gain on a trained model "
                 "is claimed)", "repeats": opts.repeats,
       "decode": "difusco_mis_decode, the code of the parent commit unchanged", "cases": []}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), res


def spread(ms):
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "all": ms}


sizes = [int(np.random.default_rng(5000 + g).integers(700, 801)) for g in range(opts.graphs)]      # bench.py's graphs
graphs = [torch.from_numpy(er_mis_edge_index(n, 0.15, seed=1000 + g)) for g, n in enumerate(sizes)]
model = None
if not opts.no_sampling:
    from difusco_amd.models import MISModel
    margs = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, inference_diffusion_steps=50,
                 inference_schedule="cosine", sparse_factor=-1, n_layers=12, hidden_dim=256, inference_trick="ddim")
    model = MISModel(margs, random_state_dict(256, 12, 2, seed=20240926), device=dev, seed=1234)

for P in opts.parallel:
    ns = [n for n in sizes for _ in range(P)]                  # the copies of a graph are components of their own
    off = np.concatenate([[0], np.cumsum(ns)])
    ei = torch.cat([graphs[c // P] + int(off[c]) for c in range(len(ns))], dim=1).to(dev)
    N = int(off[-1])
    graph = build_csr(ei, N, dev)
    scores = torch.from_numpy(np.random.default_rng(P).random(N).astype(np.float32)).to(dev)
    decoded = mis_decode_np(scores, graph=graph, device=dev)   # warm-up of both
    mis_local_search_np(scores, decoded, graph=graph, device=dev, max_rounds=opts.max_rounds)
    dec, ls = [], []
    stats = {}
    for _ in range(opts.repeats):                              # interleaved: same clocks for both
        t, decoded = timed(lambda: mis_decode_np(scores, graph=graph, device=dev))
        dec.append(t)
        t, searched = timed(lambda: mis_local_search_np(scores, decoded, graph=graph, device=dev, max_rounds=opts.max_rounds,
                                                        stats=stats))
        ls.append(t)
    per = lambda sol: [int(sol[off[c]:off[c + 1]].sum()) for c in range(len(ns))]
    before, after = per(decoded), per(searched)
    case = {"workload": f"{opts.graphs} x G(700..800, 0.15), P = {P}: one union", "parallel_sampling": P, "nodes": N,
            "csr_entries": int(graph.col.shape[0]), "max_rounds": opts.max_rounds,
            "decode_ms": spread(dec), "local_search_ms": spread(ls),
            "local_search_over_decode": float(np.median(ls)) / float(np.median(dec)),
            "rounds": stats["rounds"], "swaps": stats["swaps"], "inserts": stats["inserts"],
            "size_decoded": {"mean": float(np.mean(before)), "min": min(before), "max": max(before)},
            "size_after": {"mean": float(np.mean(after)), "min": min(after), "max": max(after)},
            "size_gain_pct_mean": float(np.mean([100.0 * (a - b) / b for a, b in zip(after, before)])),
            "best_of_P_decoded_mean": float(np.mean([max(before[g * P:(g + 1) * P]) for g in range(opts.graphs)])),
            "best_of_P_after_mean": float(np.mean([max(after[g * P:(g + 1) * P]) for g in range(opts.graphs)]))}
    if model is not None:
        model.sample(N, ei)                                    # warm-up (graph preparation, first-launch costs)
        t, _ = timed(lambda: model.sample(N, ei))
        case["sampling_50_steps_ms"] = t
        case["local_search_over_sampling"] = float(np.median(ls)) / t
    out["cases"].append(case)
print(json.dumps(out))
if opts.out:
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
