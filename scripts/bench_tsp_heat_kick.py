#!/usr/bin/env python
"""Heat-biased against uniform kicks of the iterated multi-move local search, timed on the GPU box:
``batched_iterated_search_torch`` with ``kick_bias="uniform"`` (``difusco_tsp_iterated_search_ragged`` /
``difusco_tsp_focused_search_ragged``, the parent commit's entries, which the heat bias does not touch) and ``kick_bias="heat"``
(``difusco_tsp_guided_search_ragged``), both descents, kicks in {0, 10, 30, 100} (``--kicks``), in the set-up of
``scripts/bench_tsp_focused_search.py``: the decoded start tour of TSP-N, K = 100, and the synthetic heat it was decoded from (no
trained checkpoint, so the lengths say nothing about solution quality on real heatmaps), N = 10^3 at cap 200 and N = 10^4 at cap
5000 per descent.  Writes ``profiles/tsp_heat_kick/bench.json`` (``--out``).

Timed run (the default): one tour, seed 0, offset 0, one process, a warm-up of each entry, ``--repeats`` interleaved repeats (one
pass over all settings of both biases per repeat), median [min, max] of the time to stop; ms per kick = (time at k kicks - time at
0 kicks) / k from the medians, and its worst case for either side from the extremes.  ``heat_minus_uniform_ms_per_kick`` is the
cost of the weight and scan pass plus whatever the other trajectory costs: the two biases draw different kicks, so their descents
differ; the kernel trace isolates the pass.  ``--save_tours PATH`` keeps the start tours, the heat and the results (npz).

  --verify NPZ          no GPU: replays the heat rows of N = 10^3 at 0, 10 and 30 kicks, both descents, with
                        tests/tsp_heat_kick_emulation.py from the saved start tours and heat and adds to ``--out`` whether tours,
                        counters and per-tour arrays equal the GPU's.
  --trace N KICKS       one warm-up and ONE focused heat call at that size: the program of a separate
                        ``rocprofv3 --kernel-trace --stats -- python scripts/bench_tsp_heat_kick.py --trace N KICKS`` pass, with
                        nothing else traced.
  --trace_stats CSV     no GPU: reads that pass's kernel trace and adds the keep / kick launches' times to ``--out``.

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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_heat_kick", "bench.json"))
ap.add_argument("--save_tours", default=None)
ap.add_argument("--verify", default=None)
ap.add_argument("--trace", nargs=2, type=int, default=None, metavar=("N", "KICKS"))
ap.add_argument("--trace_stats", default=None)
opts = ap.parse_args()
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")
PER = ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length", "closing_sweeps")
DESCENTS = ("full", "focused")
BIASES = ("uniform", "heat")
PARENT_KEEP_KICK_US = 6.755      # profiles/tsp_focused_search/bench.json: the focused keep / kick launch, all launches, N = 10^4


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
    import tsp_heat_kick_emulation as H
    saved = np.load(opts.verify)
    res = []
    n = 1000
    ei, heat = saved[f"ei_{n}"], saved[f"heat_{n}"]
    order = np.argsort(ei[0], kind="stable")                     # the layer's stable sort by row
    rp = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))]).astype(np.int32)
    for d in DESCENTS:
        for kicks in (0, 10, 30):
            t0 = time.perf_counter()
            tour, c, per = H.search_tour(saved[f"pts_{n}"], saved[f"start_{n}"][0], rp, ei[1][order], heat[order], 0, 0, kicks=kicks,
                                         kick_size=int(saved["kick_size"]), span=int(saved["span"]),
                                         max_iterations=int(saved[f"cap_{n}"]), max_rounds=opts.max_rounds,
                                         select_rounds=opts.select_rounds, descent=d)
            tag = f"heat_{d}_{n}_{kicks}"
            gpu = {k: int(saved[f"{k}_{tag}"]) for k in KEYS}
            gpu_per = {k: saved[f"{k}_{tag}"].tolist()[0] for k in PER if f"{k}_{tag}" in saved}
            res.append({"n": n, "kicks": kicks, "descent": d, "emulation": c, "gpu": gpu, "emulation_per_tour": per,
                        "gpu_per_tour": gpu_per, "tours_equal": bool(np.array_equal(tour, saved[f"tours_{tag}"][0])),
                        "emulation_s": time.perf_counter() - t0})
            assert c == gpu and res[-1]["tours_equal"] and per == gpu_per
    update_out("emulation", res)
    sys.exit(0)

if opts.trace_stats:
    # every launch of the heat instantiation of the focused keep / kick kernel; the launches that draw a kick run the weight and
    # scan pass, the others return at their first test or only keep
    us = []
    with open(opts.trace_stats) as f:
        for r in csv.DictReader(f):
            if "mls_keep_kick_focused_kernel" in r["Kernel_Name"]:
                us.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    us = np.array(us)
    update_out("kernel_trace", {
        "source": "rocprofv3 --kernel-trace --stats of --trace, its own run, the warm-up call included",
        "kernel": "mls_keep_kick_focused_kernel<true>", "launches": int(len(us)), "mean_us": float(us.mean()),
        "median_us": float(np.median(us)), "max_us": float(us.max()), "sum_us": float(us.sum()),
        "parent_mean_us": PARENT_KEEP_KICK_US, "launches_above_twice_the_median": int((us > 2 * np.median(us)).sum()),
        "mean_us_of_those": float(us[us > 2 * np.median(us)].mean()) if (us > 2 * np.median(us)).any() else None})
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd.decode import TSP_KICK_SIZE, TSP_KICK_SPAN, batched_iterated_search_torch, merge_tours  # noqa: E402
from difusco_amd.synthetic import tsp_instance  # noqa: E402

dev = torch.device("cuda:0")
kick_size, span = TSP_KICK_SIZE, TSP_KICK_SPAN
out = {"metric": "time to stop", "unit": "ms", "data": "synthetic heat, no trained checkpoint", "repeats": opts.repeats,
       "select_rounds": opts.select_rounds, "max_rounds": opts.max_rounds, "kick_size": kick_size, "span": span,
       "parent": "kick_bias='uniform': difusco_tsp_iterated_search_ragged / difusco_tsp_focused_search_ragged", "cases": []}
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
    d_heat, d_ei = torch.from_numpy(heat).to(dev), torch.from_numpy(ei).to(dev)
    tours, _ = merge_tours(d_heat, torch.from_numpy(pts).to(dev), d_ei, sparse_graph=True, device=dev)
    return pts.astype(np.float64), np.asarray(tours, dtype=np.int64), 200 if n <= 1000 else 5000, (heat, ei, d_heat, d_ei)


def search(pts64, tour0, cap, descent, bias, kicks, per, graph):
    extra = dict(kick_bias="heat", heat=graph[2].reshape(1, -1), edge_index=graph[3]) if bias == "heat" else {}
    return batched_iterated_search_torch(pts64, tour0, max_iterations=cap, device=dev, max_rounds=opts.max_rounds,
                                         select_rounds=opts.select_rounds, kicks=kicks, kick_size=kick_size, span=span,
                                         seeds=[0], offsets=[0], stats=per, descent=descent, **extra)


if opts.trace:
    pts64, tour0, cap, graph = start_of(opts.trace[0])
    search(pts64, tour0, 3, "focused", "heat", 2, {}, graph)                                   # warm-up
    per = {}
    t, _ = timed(lambda: search(pts64, tour0, cap, "focused", "heat", opts.trace[1], per, graph))
    print(json.dumps({"trace": opts.trace, "ms": t, "closing_sweeps": per["closing_sweeps"].tolist()}))
    sys.exit(0)

for n in opts.sizes:
    pts64, tour0, cap, graph = start_of(n)
    settings = [(d, b) for d in DESCENTS for b in BIASES]
    for d, b in settings:
        search(pts64, tour0, 3, d, b, 2, {}, graph)                                            # warm-up
    ms = {(d, b, kicks): [] for d, b in settings for kicks in opts.kicks}
    last = {}
    for _ in range(opts.repeats):                                                              # interleaved: same clocks for all
        for kicks in opts.kicks:
            for d, b in settings:
                per = {}
                t, (got, stats) = timed(lambda: search(pts64, tour0, cap, d, b, kicks, per, graph))
                ms[d, b, kicks].append(t)
                last[d, b, kicks] = (got, stats, per)
    case = {"workload": f"TSP-{n} K=100, decoded start tour and its heat, one tour", "cap_per_descent": cap}
    for d, b in settings:
        rows = {}
        for kicks in opts.kicks:
            got, stats, per = last[d, b, kicks]
            row = dict(stats, ms=spread(ms[d, b, kicks]), host_syncs=per["host_syncs"],
                       **{key: per[key].tolist()[0] for key in PER if key in per},
                       length_over_first=float(per["final_length"][0] / per["first_length"][0]))
            if kicks > 0 and 0 in opts.kicks:
                t0 = ms[d, b, 0]
                row["ms_per_kick"] = {"median": float((np.median(ms[d, b, kicks]) - np.median(t0)) / kicks),
                                      "min": float((min(ms[d, b, kicks]) - max(t0)) / kicks),
                                      "max": float((max(ms[d, b, kicks]) - min(t0)) / kicks)}
            rows[str(kicks)] = row
            keep.update({f"tours_{b}_{d}_{n}_{kicks}": got, **{f"{k2}_{b}_{d}_{n}_{kicks}": stats[k2] for k2 in KEYS},
                         **{f"{k2}_{b}_{d}_{n}_{kicks}": per[k2] for k2 in PER if k2 in per}})
        case[f"{d}_{b}"] = rows
    if 0 in opts.kicks:
        case["heat_minus_uniform_ms_per_kick"] = {
            d: {str(k): case[f"{d}_heat"][str(k)]["ms_per_kick"]["median"] - case[f"{d}_uniform"][str(k)]["ms_per_kick"]["median"]
                for k in opts.kicks if k > 0} for d in DESCENTS}
        case["kicks_0_equal"] = bool(all(np.array_equal(last["full", "uniform", 0][0], last[d, b, 0][0]) for d, b in settings))
    out["cases"].append(case)
    keep.update({f"pts_{n}": pts64, f"start_{n}": tour0, f"cap_{n}": cap})
    if n == 1000:                                                                              # what --verify replays
        keep.update({f"heat_{n}": graph[0], f"ei_{n}": graph[1]})
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
with open(opts.out, "w") as f:
    f.write(json.dumps(out) + "\n")
if opts.save_tours:
    os.makedirs(os.path.dirname(os.path.abspath(opts.save_tours)), exist_ok=True)
    np.savez(opts.save_tours, **keep)
