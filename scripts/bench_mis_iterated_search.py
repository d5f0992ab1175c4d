#!/usr/bin/env python
"""Iterated MIS swap search timing on the GPU box: ``mis_iterated_search_np`` at kicks in {0, 10, 30, 100, 300} beside the swap
descent alone (``mis_local_search_np``, the code of the parent commit unchanged) on the union the MIS workload of BASELINE.json
hands one GPU: 16 Erdos-Renyi graphs G(n, 0.15), n ~ U{700..800} (the graphs of ``bench.py``), as P = 1 and P = 4 copies, every
copy its own row of the instance table (key 1000 + graph, offset ``2^62 + p 2^32``, the tables of ``solve_mis_batch``).  Prints
one JSON line (``--out PATH`` also writes it).

The scores are SYNTHETIC (uniform random per node and copy, not a trained checkpoint's heatmap): the sizes say what the rule does
on such scores, not what it gains on a trained model.

One process; after a warm-up of every variant, ``--repeats`` rounds in each of which every variant runs once, in turn (same
clocks for all); median [min, max].  All start from the decoded set and include the copy of the 0/1 array to the host, as
``solve_mis_batch`` pays it.  ``kicks = 0`` and ``local_search`` run the same descent and should agree within the spread.
``sampling_50_steps_ms``: one 50-step ``MISModel.sample`` of the same batch (12 layers, hidden 256, random weights), the stage the
search follows in the pipeline."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difusco_amd import _lib  # noqa: E402
from difusco_amd.decode import MIS_KICK_OFFSET, mis_decode_np, mis_iterated_search_np, mis_local_search_np  # noqa: E402
from difusco_amd.graph import build_csr  # noqa: E402
from difusco_amd.synthetic import er_mis_edge_index, random_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--graphs", type=int, default=16)
ap.add_argument("--parallel", nargs="+", type=int, default=[1, 4])
ap.add_argument("--kicks", nargs="+", type=int, default=[0, 10, 30, 100, 300])
ap.add_argument("--kick_size", type=int, default=4)
ap.add_argument("--max_rounds", type=int, default=1000)
ap.add_argument("--no_sampling", action="store_true", help="skip the 50-step sampling time")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
opts = ap.parse_args()

dev = torch.device("cuda:0")
out = {"metric": "ms per call on the union", "unit": "ms", "box": "one MI355X (gfx950)", "data": "synthetic",
       "scores": "uniform random per node and copy (synthetic: not a trained checkpoint's heatmap; no gain on a trained model "
                 "is claimed)", "repeats": opts.repeats, "kick_size": opts.kick_size,
       "local_search": "difusco_mis_local_search, the code of the parent commit unchanged", "cases": []}


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
    ns = [n for n in sizes for _ in range(P)]                  # the copies of a graph are instances of their own
    off = np.concatenate([[0], np.cumsum(ns)])
    ei = torch.cat([graphs[c // P] + int(off[c]) for c in range(len(ns))], dim=1).to(dev)
    N = int(off[-1])
    graph = build_csr(ei, N, dev)
    scores = torch.from_numpy(np.random.default_rng(P).random(N).astype(np.float32)).to(dev)
    decoded = mis_decode_np(scores, graph=graph, device=dev)
    table = dict(instance_rows=off.tolist(), seeds=[1000 + c // P for c in range(len(ns))],
                 offsets=[MIS_KICK_OFFSET + ((c % P) << 32) for c in range(len(ns))])
    stats = {k: {} for k in opts.kicks}
    local_stats = {}

    def local():
        sol = mis_local_search_np(scores, decoded, graph=graph, device=dev, max_rounds=opts.max_rounds, stats=local_stats)
        local_stats["host_syncs"] = int(_lib.lib().difusco_mis_search_host_syncs())
        return sol

    def iterated(k):
        return lambda: mis_iterated_search_np(scores, decoded, graph=graph, device=dev, max_rounds=opts.max_rounds, kicks=k,
                                              kick_size=opts.kick_size, stats=stats[k], **table)

    variants = [("local_search", local)] + [(k, iterated(k)) for k in opts.kicks]
    ms, sols = {name: [] for name, _ in variants}, {}
    for _, fn in variants:                                     # warm-up of every variant
        fn()
    for _ in range(opts.repeats):                              # interleaved: same clocks for all
        for name, fn in variants:
            t, sols[name] = timed(fn)
            ms[name].append(t)
    per = lambda sol: [int(sol[off[c]:off[c + 1]].sum()) for c in range(len(ns))]
    best = lambda v: float(np.mean([max(v[g * P:(g + 1) * P]) for g in range(opts.graphs)]))
    before, swap = per(decoded), per(sols["local_search"])
    case = {"workload": f"{opts.graphs} x G(700..800, 0.15), P = {P}: one union", "parallel_sampling": P, "nodes": N,
            "instances": len(ns), "csr_entries": int(graph.col.shape[0]), "max_rounds": opts.max_rounds,
            "size_decoded_mean": float(np.mean(before)), "best_of_P_decoded_mean": best(before),
            "local_search": {"ms": spread(ms["local_search"]), "host_syncs": local_stats["host_syncs"],
                             "size_mean": float(np.mean(swap)), "best_of_P_mean": best(swap)},
            "kicks_0_equals_local_search": bool(np.array_equal(sols["local_search"], sols[0])) if 0 in sols else None,
            "iterated": []}
    if model is not None:
        model.sample(N, ei)                                    # warm-up (graph preparation, first-launch costs)
        case["sampling_50_steps_ms"], _ = timed(lambda: model.sample(N, ei))
    for k in opts.kicks:
        after, med = per(sols[k]), float(np.median(ms[k]))
        row = {"kicks": k, "ms": spread(ms[k]), "host_syncs": stats[k]["host_syncs"],
               "ms_per_kick": (med - float(np.median(ms[0]))) / k if k and 0 in ms else None,
               "rounds": stats[k]["rounds"], "swaps": stats[k]["swaps"], "inserts": stats[k]["inserts"],
               "kicks_entered_mean": float(np.mean(stats[k]["entered"])), "kicks_accepted_mean": float(np.mean(stats[k]["accepted"])),
               "size_mean": float(np.mean(after)), "size_min": min(after), "size_max": max(after), "best_of_P_mean": best(after),
               "never_below_the_descent": all(a >= s for a, s in zip(after, swap))}
        if model is not None:
            row["over_sampling"] = med / case["sampling_50_steps_ms"]
        case["iterated"].append(row)
    out["cases"].append(case)
print(json.dumps(out))
if opts.out:
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
