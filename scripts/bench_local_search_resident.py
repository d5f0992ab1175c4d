#!/usr/bin/env python
"""Resident against launched 2-opt + Or-opt search on the GPU box: ``batched_local_search_ragged`` with ``mode="resident"``
(``difusco_tsp_local_search_resident``: one block per instance, tours in LDS through both phases and all rounds, no launch or
host read per step) beside ``mode="launches"`` (``difusco_tsp_local_search_ragged``, the code of the parent commit unchanged), on
G instances of n cities with P tours each: n in {20, 50, 100, 200, 500}, P in {1, 4}, G in {1, 64, 512}, wherever ``P (n + 1)``
is within ``difusco_tsp_local_search_resident_max_cells()``; ``max_iterations`` 1000, ``max_rounds`` 16.  Prints one JSON line
(``--out PATH`` also writes it).

The start tours are the same for both variants: decoded (``merge_tours_batch``) from a SYNTHETIC heatmap over the 10-NN graph of
uniform points, as ``scripts/bench_two_opt_resident.py`` makes one - short edges hot, times uniform noise per sample - not a
trained checkpoint's.  Instance g has the points of seed g % 64 and its own noise.  The two variants return the same tours and
counters by construction and the script asserts it for every shape; a group in which they differ is settled by the CPU
emulation (``tests/or_opt_emulation.py``), which the resident variant must equal.

One process; per shape a warm-up of both variants, then ``--repeats`` rounds in each of which every variant runs once, in turn
(same clocks for both); median [min, max].  A call includes the upload of points and tours and the copy of the tours back, the
same for both.  ``verdict``: ``resident`` if the resident maximum is below the launched minimum, ``launched`` if the launched
maximum is below the resident minimum, else ``overlap``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from difusco_amd.decode import (TSP_LOCAL_SEARCH_MODES, batched_local_search_ragged, local_search_resident_max_cells,  # noqa: E402
                                merge_tours_batch)
from difusco_amd.synthetic import tsp_instance  # noqa: E402
import or_opt_emulation as emulation  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sizes", nargs="+", type=int, default=[20, 50, 100, 200, 500])
ap.add_argument("--parallel", nargs="+", type=int, default=[1, 4])
ap.add_argument("--groups", nargs="+", type=int, default=[1, 64, 512])
ap.add_argument("--max_iterations", type=int, default=1000)
ap.add_argument("--max_rounds", type=int, default=16)
ap.add_argument("--steps_per_launch", type=int, default=0, help="of the resident mode (0: the library's default)")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
opts = ap.parse_args()

dev = torch.device("cuda:0")
limit = local_search_resident_max_cells()
out = {"metric": "ms per call", "unit": "ms", "box": "one MI355X (gfx950)", "data": "synthetic",
       "start_tours": "merge_tours_batch on a synthetic heatmap over the 10-NN graph (short edges hot, times uniform noise per "
                      "sample): not a trained checkpoint's heatmap; the variants return equal tours by construction",
       "repeats": opts.repeats, "max_iterations": opts.max_iterations, "max_rounds": opts.max_rounds,
       "steps_per_launch": opts.steps_per_launch, "resident_max_cells": limit,
       "launches": "difusco_tsp_local_search_ragged, the code of the parent commit unchanged",
       "verdict": "resident: resident max < launched min; launched: launched max < resident min; else overlap",
       "verified": True, "cases": [], "skipped": []}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), res


def spread(ms):
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "all": list(ms)}


def start_tours(n, P, G):
    """(float64 points, decoded closed tours [P, n + 1]) of G instances."""
    k = min(10, n - 1)
    base = [tsp_instance(n, k, seed=4000 + s) for s in range(min(G, 64))]
    pts, eis, heats = [], [], []
    for g in range(G):
        p, ei = base[g % 64]
        d = np.linalg.norm(p[ei[0]] - p[ei[1]], axis=1)
        noise = np.random.default_rng(100000 * n + 1000 * P + g).random((P, ei.shape[1]))
        heats.append(((np.exp(-d / (0.5 * d.mean())) * noise).astype(np.float32) + np.float32(1e-6)).reshape(-1))
        pts.append(p)
        eis.append(ei)
    merged = merge_tours_batch(heats, pts, eis, sparse_graph=True, parallel_sampling=P, device=dev)
    return [p.astype(np.float64) for p in pts], [np.asarray(t, dtype=np.int64) for t, _ in merged]


for n in opts.sizes:
    for P in opts.parallel:
        if P * (n + 1) > limit:
            out["skipped"].append({"n": n, "parallel_sampling": P, "cells": P * (n + 1), "why": "above resident_max_cells"})
            continue
        for G in opts.groups:
            pts, tours = start_tours(n, P, G)
            stats = {mode: {} for mode in TSP_LOCAL_SEARCH_MODES}

            def run(mode):
                more = dict(mode="resident", steps_per_launch=opts.steps_per_launch) if mode == "resident" else {}
                return lambda: batched_local_search_ragged(pts, tours, max_iterations=opts.max_iterations, device=dev,
                                                           max_rounds=opts.max_rounds, stats=stats[mode], **more)

            variants = [(mode, run(mode)) for mode in TSP_LOCAL_SEARCH_MODES]
            ms, res = {name: [] for name, _ in variants}, {}
            for _, fn in variants:                             # warm-up of every variant
                fn()
            for _ in range(opts.repeats):                      # interleaved: same clocks for both
                for name, fn in variants:
                    t, res[name] = timed(fn)
                    ms[name].append(t)
            counters = lambda mode: (res[mode][1], stats[mode]["or_opt_iterations"], stats[mode]["rounds"])
            departed = {g for g in range(G) if not np.array_equal(res["launches"][0][g], res["resident"][0][g])
                        or any(int(a[g]) != int(b[g]) for a, b in zip(counters("launches"), counters("resident")))}
            for g in sorted(departed):                         # the emulation decides, and the resident form must equal it
                want = emulation.local_search(pts[g], tours[g], opts.max_iterations, opts.max_rounds)
                got = (res["resident"][0][g],) + tuple(int(c[g]) for c in counters("resident"))
                assert np.array_equal(got[0], want[0]) and got[1:] == tuple(want[1:]), (n, P, G, g)
            two, orr, rounds = (np.asarray(c) for c in counters("resident"))
            steps = two + orr
            case = {"n": n, "parallel_sampling": P, "groups": G, "cells_per_group": P * (n + 1),
                    "steps_slowest_group": int(steps.max()), "steps_total": int(steps.sum()), "two_opt_iterations_total": int(two.sum()),
                    "or_opt_iterations_total": int(orr.sum()), "rounds_most": int(rounds.max()),
                    "groups_where_launched_departs_from_emulation": sorted(departed), "variants": {}}
            for mode, t in ms.items():
                case["variants"][mode] = {"ms": spread(t), **({"host_syncs": stats[mode]["host_syncs"]} if mode == "resident" else {})}
            a, b = case["variants"]["launches"]["ms"], case["variants"]["resident"]["ms"]
            case["launches_over_resident"] = a["median"] / b["median"]
            case["verdict"] = "resident" if b["max"] < a["min"] else "launched" if a["max"] < b["min"] else "overlap"
            out["cases"].append(case)
            print(f"n={n} P={P} G={G}: steps {int(steps.max())}; launches {a['median']:.3f} ms; resident {b['median']:.3f} ms; "
                  f"{case['verdict']}", file=sys.stderr, flush=True)
print(json.dumps(out))
if opts.out:
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
