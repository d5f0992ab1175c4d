#!/usr/bin/env python
"""Focused against full descents of the iterated multi-move local search, timed on the GPU box:
``batched_iterated_search_torch`` with ``descent="full"`` (``difusco_tsp_iterated_search_ragged``, the parent commit's code, which
the focused search does not touch) and ``descent="focused"`` (``difusco_tsp_focused_search_ragged``), kicks in {0, 10, 30, 100}
(``--kicks``), from the decoded start tour of ``scripts/bench_decode.py`` (TSP-N, K = 100, synthetic heat - no trained checkpoint,
so the lengths say nothing about solution quality on real heatmaps), N = 10^3 at cap 200 and N = 10^4 at cap 5000 per descent.
Writes ``profiles/tsp_focused_search/bench.json`` (``--out``).

Timed run (the default): one tour, seed 0, offset 0, one process, a warm-up of each entry, ``--repeats`` interleaved repeats (one
pass over all settings of both descents per repeat, so drifting clocks hit every setting alike), median [min, max] of the time
to stop; ms per kick = (time at k kicks - time at 0 kicks) / k from the medians, and its worst case for either side from the
extremes; the end length over the first descent's, the kicks kept, ``closing_sweeps`` and the host synchronisations.  The focused
figure counts as a gain only where its maximum lies below the parent's minimum (``focused_max_below_parent_min``).
``--save_tours PATH`` keeps the start tours and the results (npz).

  --verify NPZ          no GPU: replays N = 10^3 at 0, 10 and 30 kicks with tests/tsp_focused_search_emulation.py from the saved
                        start tours and adds to ``--out`` whether tours, counters and per-tour arrays equal the GPU's.
  --trace N KICKS       one warm-up and ONE focused call at that size: the program of a separate
                        ``rocprofv3 --kernel-trace --stats -- python scripts/bench_tsp_focused_search.py --trace N KICKS`` pass, with
                        nothing else traced.
  --trace_stats CSV     no GPU: reads that pass's kernel statistics and adds the per-kernel split to ``--out``.

No time or length printed here is a test."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sizes", nargs="+", type=int, default=[1000, 10000], choices=[1000, 10000])
ap.add_argument("--kicks", nargs="+", type=int, default=[0, 10, 30, 100])
ap.add_argument("--select_rounds", type=int, default=4)
ap.add_argument("--max_rounds", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_focused_search", "bench.json"))
ap.add_argument("--save_tours", default=None)
ap.add_argument("--verify", default=None)
ap.add_argument("--trace", nargs=2, type=int, default=None, metavar=("N", "KICKS"))
ap.add_argument("--trace_stats", default=None)
opts = ap.parse_args()
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")
PER = ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length", "closing_sweeps")
DESCENTS = ("full", "focused")


def update_out(key, value):
    doc = {}
    if os.path.exists(opts.out):
        with open(opts.out) as f:
            doc = json.load(f)
    doc[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps({key: value}))


if opts.verify:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tsp_focused_search_emulation as F
    saved = np.load(opts.verify)
    res = []
    for kicks in (0, 10, 30):
        n = 1000
        t0 = time.perf_counter()
        tour, c, per = F.search_tour(saved[f"pts_{n}"], saved[f"start_{n}"][0], 0, 0, kicks=kicks, kick_size=int(saved["kick_size"]),
                                     span=int(saved["span"]), max_iterations=int(saved[f"cap_{n}"]), max_rounds=opts.max_rounds,
                                     select_rounds=opts.select_rounds)
        tag = f"focused_{n}_{kicks}"
        gpu = {k: int(saved[f"{k}_{tag}"]) for k in KEYS}
        gpu_per = {k: saved[f"{k}_{tag}"].tolist()[0] for k in PER}
        res.append({"n": n, "kicks": kicks, "emulation": c, "gpu": gpu, "emulation_per_tour": per, "gpu_per_tour": gpu_per,
                    "tours_equal": bool(np.array_equal(tour, saved[f"tours_{tag}"][0])), "emulation_s": time.perf_counter() - t0})
        assert c == gpu and res[-1]["tours_equal"] and {k: per[k] for k in PER} == gpu_per
    update_out("emulation", res)
    sys.exit(0)

if opts.trace_stats:
    # the launch sequences of the traced call: five launches each, from mls_prep_kernel to mls_keep_kick_focused_kernel; a
    # sequence in which mls_focused_row_best_kernel took longer than mls_row_best_kernel is a focused sweep of the one tour
    names = ("mls_prep_kernel", "mls_row_best_kernel", "mls_focused_row_best_kernel", "mls_select_focused_kernel",
             "mls_keep_kick_focused_kernel")
    launches = []
    with open(opts.trace_stats) as f:
        for r in csv.DictReader(f):
            hit = [k for k in names if k in r["Kernel_Name"]]      # no name is part of another
            if hit:
                launches.append((int(r["Start_Timestamp"]), hit[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    launches.sort()
    seqs = [launches[i:i + 5] for i in range(0, len(launches) - 4, 5)]
    assert all([k for _, k, _ in s] == list(names) for s in seqs), "the trace is not a run of whole launch sequences"
    kinds = {"focused": [s for s in seqs if s[2][2] > s[1][2]], "full": [s for s in seqs if s[2][2] <= s[1][2]]}
    update_out("kernel_trace", {
        "source": "rocprofv3 --kernel-trace --stats of --trace, its own run, the warm-up call included",
        **{kind: {"sequences": len(v), "mean_us": {k: float(np.mean([s[q][2] for s in v])) for q, k in enumerate(names)} if v else None,
                  "mean_us_start_to_start": float(np.mean([b[0][0] - a[0][0] for a, b in zip(seqs, seqs[1:]) if a in v]) / 1e3) if v else None}
           for kind, v in kinds.items()}})
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd.decode import TSP_KICK_SIZE, TSP_KICK_SPAN, batched_iterated_search_torch, merge_tours  # noqa: E402
from difusco_amd.synthetic import tsp_instance  # noqa: E402

dev = torch.device("cuda:0")
kick_size, span = TSP_KICK_SIZE, TSP_KICK_SPAN
out = {"metric": "time to stop", "unit": "ms", "data": "synthetic heat, no trained checkpoint", "repeats": opts.repeats,
       "select_rounds": opts.select_rounds, "max_rounds": opts.max_rounds, "kick_size": kick_size, "span": span,
       "parent": "descent='full': difusco_tsp_iterated_search_ragged", "cases": []}
keep = {"kick_size": kick_size, "span": span}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


def start_of(n):
    k = 100
    pts, ei = tsp_instance(n, k, seed=11)
    rng = np.random.default_rng(n)
    d = np.linalg.norm(pts[ei[0]] - pts[ei[1]], axis=1)
    heat = (np.exp(-d / (0.5 * d.mean())) * rng.random(ei.shape[1])).astype(np.float32) + np.float32(1e-6)
    tours, _ = merge_tours(torch.from_numpy(heat).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(ei).to(dev),
                           sparse_graph=True, device=dev)
    return pts.astype(np.float64), np.asarray(tours, dtype=np.int64), 200 if n <= 1000 else 5000


def search(pts64, tour0, cap, descent, kicks, per):
    return batched_iterated_search_torch(pts64, tour0, max_iterations=cap, device=dev, max_rounds=opts.max_rounds,
                                         select_rounds=opts.select_rounds, kicks=kicks, kick_size=kick_size, span=span,
                                         seeds=[0], offsets=[0], stats=per, descent=descent)


if opts.trace:
    pts64, tour0, cap = start_of(opts.trace[0])
    search(pts64, tour0, 3, "focused", 2, {})                                                  # warm-up
    per = {}
    t, _ = timed(lambda: search(pts64, tour0, cap, "focused", opts.trace[1], per))
    print(json.dumps({"trace": opts.trace, "ms": t, "closing_sweeps": per["closing_sweeps"].tolist()}))
    sys.exit(0)

for n in opts.sizes:
    pts64, tour0, cap = start_of(n)
    for d in DESCENTS:
        search(pts64, tour0, 3, d, 2, {})                                                      # warm-up
    ms = {(d, kicks): [] for d in DESCENTS for kicks in opts.kicks}
    last = {}
    for _ in range(opts.repeats):                                                              # interleaved: same clocks for all
        for kicks in opts.kicks:
            for d in DESCENTS:
                per = {}
                t, (got, stats) = timed(lambda: search(pts64, tour0, cap, d, kicks, per))
                ms[d, kicks].append(t)
                last[d, kicks] = (got, stats, per)
    case = {"workload": f"TSP-{n} K=100, decoded start tour, one tour", "cap_per_descent": cap, "full": {}, "focused": {}}
    for d in DESCENTS:
        for kicks in opts.kicks:
            got, stats, per = last[d, kicks]
            row = dict(stats, ms=spread(ms[d, kicks]), host_syncs=per["host_syncs"],
                       **{key: per[key].tolist()[0] for key in PER if key in per},
                       length_over_first=float(per["final_length"][0] / per["first_length"][0]))
            if kicks > 0 and 0 in opts.kicks:
                t0 = ms[d, 0]
                row["ms_per_kick"] = {"median": float((np.median(ms[d, kicks]) - np.median(t0)) / kicks),
                                      "min": float((min(ms[d, kicks]) - max(t0)) / kicks),
                                      "max": float((max(ms[d, kicks]) - min(t0)) / kicks)}
            case[d][str(kicks)] = row
            keep.update({f"tours_{d}_{n}_{kicks}": got, **{f"{k2}_{d}_{n}_{kicks}": stats[k2] for k2 in KEYS},
                         **{f"{k2}_{d}_{n}_{kicks}": per[k2] for k2 in PER if k2 in per}})
    case["focused_max_below_parent_min"] = {str(kicks): bool(max(ms["focused", kicks]) < min(ms["full", kicks]))
                                            for kicks in opts.kicks if kicks > 0}
    if 0 in opts.kicks:
        case["kicks_0_equal"] = bool(np.array_equal(last["full", 0][0], last["focused", 0][0]) and last["full", 0][1] == last["focused", 0][1])
    out["cases"].append(case)
    keep.update({f"pts_{n}": pts64, f"start_{n}": tour0, f"cap_{n}": cap})
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
with open(opts.out, "w") as f:
    f.write(json.dumps(out) + "\n")
if opts.save_tours:
    os.makedirs(os.path.dirname(os.path.abspath(opts.save_tours)), exist_ok=True)
    np.savez(opts.save_tours, **keep)
