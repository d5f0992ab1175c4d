#!/usr/bin/env python
"""Resident against launched single-move 2-opt on the GPU box: ``batched_two_opt_ragged`` with ``mode="resident"``
(``difusco_tsp_two_opt_resident``: one block per instance, tours in LDS, no launch or host read per move) beside
``mode="launches"`` (``difusco_tsp_two_opt_ragged``, the code of the parent commit unchanged), each with ``method="exact"`` and
``"screened"``, on G instances of n cities with P tours each: n in {20, 50, 100, 200, 500, 1000}, P in {1, 4}, G in {1, 64, 512},
wherever ``P (n + 1)`` is within ``difusco_tsp_two_opt_resident_max_cells()``.  Prints one JSON line (``--out PATH`` also writes it).

The start tours are the same for every variant: decoded (``merge_tours_batch``) from a SYNTHETIC heatmap over the 10-NN graph of
uniform points, as ``scripts/bench_decode.py`` makes one - short edges hot, times uniform noise per sample - not a trained
checkpoint's.  Instance g has the points of seed g % 64 and its own noise.  The four variants return the same tours and
iteration counts by construction and the script asserts it for every shape; where a launched variant hands a tour back
reversed (see the comment at the assertion) the CPU oracle decides, and the resident variants must equal it.

One process; per shape a warm-up of every variant, then ``--repeats`` rounds in each of which every variant runs once, in turn
(same clocks for all); median [min, max].  A call includes the upload of points and tours and the copy of the tours back, the
same for all variants.  ``ms_per_move``: the call over the moves of its slowest instance, the length of the launched chain.
``resident_below_launched``: the resident maximum is below the launched minimum of the same method, i.e. the resident form is
faster by more than the launched form's own spread."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difusco_amd.decode import (TWO_OPT_METHODS, TWO_OPT_MODES, batched_two_opt_ragged, merge_tours_batch,  # noqa: E402
                                two_opt_resident_max_cells)
from difusco_amd.synthetic import tsp_instance  # noqa: E402
from oracle import tsp_decode_oracle as oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sizes", nargs="+", type=int, default=[20, 50, 100, 200, 500, 1000])
ap.add_argument("--parallel", nargs="+", type=int, default=[1, 4])
ap.add_argument("--groups", nargs="+", type=int, default=[1, 64, 512])
ap.add_argument("--max_iterations", type=int, default=1000)
ap.add_argument("--moves_per_launch", type=int, default=0, help="of the resident mode (0: the library's default)")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
opts = ap.parse_args()

dev = torch.device("cuda:0")
limit = two_opt_resident_max_cells()
out = {"metric": "ms per call", "unit": "ms", "box": "one MI355X (gfx950)", "data": "synthetic",
       "start_tours": "merge_tours_batch on a synthetic heatmap over the 10-NN graph (short edges hot, times uniform noise per "
                      "sample): not a trained checkpoint's heatmap; the variants return equal tours by construction",
       "repeats": opts.repeats, "max_iterations": opts.max_iterations, "moves_per_launch": opts.moves_per_launch,
       "resident_max_cells": limit, "launches": "difusco_tsp_two_opt_ragged, the code of the parent commit unchanged",
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
            stats = {(mode, method): {} for mode in TWO_OPT_MODES for method in TWO_OPT_METHODS}

            def run(mode, method):
                more = dict(mode="resident", moves_per_launch=opts.moves_per_launch) if mode == "resident" else {}
                return lambda: batched_two_opt_ragged(pts, tours, max_iterations=opts.max_iterations, device=dev, method=method,
                                                      stats=stats[mode, method], **more)

            variants = [((mode, method), run(mode, method)) for method in TWO_OPT_METHODS for mode in TWO_OPT_MODES]
            ms, res = {name: [] for name, _ in variants}, {}
            for _, fn in variants:                             # warm-up of every variant
                fn()
            for _ in range(opts.repeats):                      # interleaved: same clocks for all
                for name, fn in variants:
                    t, res[name] = timed(fn)
                    ms[name].append(t)
            ref_tours, ref_its = res["launches", "exact"]
            departed = set()
            for name, (t, its) in res.items():                 # equal tours and iterations across the variants
                assert np.array_equal(its, ref_its), (n, P, G, name)
                departed |= {g for g in range(G) if not np.array_equal(t[g], ref_tours[g])}
            # A group in which the variants differ is settled by the CPU oracle: the resident variants must equal it (they add
            # the two products of a distance without a fused multiply-add, as the reference does; the launched kernels are
            # compiled with contraction and can give a finished tour's whole reversal, pair (0, n - 1), a change of -1 ulp
            # instead of 0 and hand the tour back reversed - DESIGN 5.2n).
            reversed_only = True
            for g in sorted(departed):
                want, want_it = oracle.batched_two_opt(pts[g], tours[g], max_iterations=opts.max_iterations)
                assert want_it == int(ref_its[g]), (n, P, G, g)
                for method in TWO_OPT_METHODS:
                    assert np.array_equal(res["resident", method][0][g], want), (n, P, G, g, method)
                    reversed_only &= all(np.array_equal(a, b) or np.array_equal(a[::-1], b)
                                         for a, b in zip(res["launches", method][0][g], want))
            chain = max(int(ref_its.max()), 1)
            case = {"n": n, "parallel_sampling": P, "groups": G, "cells_per_group": P * (n + 1),
                    "moves_slowest_group": int(ref_its.max()), "moves_total": int(ref_its.sum()),
                    "groups_where_launched_departs_from_oracle": sorted(departed),
                    "launched_departures_are_reversed_tours": reversed_only, "variants": {}}
            for (mode, method), t in ms.items():
                case["variants"][f"{mode}_{method}"] = {
                    "ms": spread(t), "ms_per_move": spread([v / chain for v in t]), "exact_pairs": stats[mode, method]["exact_pairs"],
                    **({"host_syncs": stats[mode, method]["host_syncs"]} if mode == "resident" else {})}
            for method in TWO_OPT_METHODS:
                a, b = case["variants"][f"launches_{method}"]["ms"], case["variants"][f"resident_{method}"]["ms"]
                case[f"{method}_launches_over_resident"] = a["median"] / b["median"]
                case[f"{method}_resident_below_launched"] = b["max"] < a["min"]
                case[f"{method}_launched_below_resident"] = a["max"] < b["min"]
            out["cases"].append(case)
            print(f"n={n} P={P} G={G}: moves {chain}; " + "; ".join(
                f"{k} {v['ms']['median']:.3f} ms" for k, v in case["variants"].items()), file=sys.stderr, flush=True)
print(json.dumps(out))
if opts.out:
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
