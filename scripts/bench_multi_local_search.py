#!/usr/bin/env python
"""Multi-move local search timing on the GPU box: the exact 2-opt + Or-opt search (``batched_local_search_torch``), the multi-move
2-opt (``batched_multi_two_opt_torch``) - both the code of the parent commit, unchanged - and the multi-move local search
(``batched_multi_local_search_torch``) from the decoded start tour of ``scripts/bench_decode.py`` (TSP-N, K = 100, synthetic
heat - no trained checkpoint, so the lengths say nothing about solution quality on real heatmaps), N = 10^3 at cap 200 and
N = 10^4 at cap 5000.  Writes ``profiles/multi_local_search/bench.json`` (``--out``).

Timed run (the default): one tour, one process, a warm-up of each method, ``--repeats`` interleaved repeats, median [min, max] of
the time to stop; sweeps by kind, moves and end length of every method.  ``--save_tours PATH`` keeps the start tours and the
results of the new search (npz).

Three more modes, all separate from the timed run:
  --profile_pass        one multi-move local search per size after a warm-up and nothing else: the program to put behind
                        ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME --``;
  --kernel_stats CSV    no GPU: reads that run's ``*_kernel_stats.csv`` and adds the per-launch averages of the three kernels
                        to ``--out`` under ``kernel_stats_n<sizes>`` (pass the run's ``--sizes``; the profiled run holds the
                        warm-up's launches too; the averages are over all of them, both phases together);
  --kernel_trace CSV    no GPU: reads that run's ``*_kernel_trace.csv`` and adds the per-launch split by phase: a launch
                        sequence is prep, row-best, select + apply in stream order; after the ``--skip_sequences`` of the warm-up
                        the sequences of the search proper are labelled from ``--phase_sweeps`` = "a,b,a,b,..", the launch
                        sequences of the 2-opt and Or-opt phase of every round, each with the sweep that ends it (one size per
                        profiled run);
  --verify NPZ          no GPU: runs tests/multi_local_search_emulation.py from the saved start tours and adds to ``--out``
                        whether the five counters and the tours equal the GPU's."""
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
ap.add_argument("--select_rounds", type=int, default=4)
ap.add_argument("--max_rounds", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_local_search", "bench.json"))
ap.add_argument("--save_tours", default=None)
ap.add_argument("--profile_pass", action="store_true")
ap.add_argument("--kernel_stats", default=None)
ap.add_argument("--kernel_trace", default=None)
ap.add_argument("--phase_sweeps", default=None)
ap.add_argument("--skip_sequences", type=int, default=4)     # the warm-up (cap 3): three sweeps and the poll's fourth sequence
ap.add_argument("--verify", default=None)
opts = ap.parse_args()
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")
KERNELS = ("mls_prep_kernel", "mls_row_best_kernel", "mls_select_kernel")


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


if opts.kernel_stats:
    rows = {}
    with open(opts.kernel_stats) as f:
        for r in csv.DictReader(f):
            for name in KERNELS:
                if name in r["Name"]:
                    rows[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                                  "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                  "max_us": float(r["MaxNs"]) / 1e3}
    update_out("kernel_stats_n" + "_".join(str(n) for n in opts.sizes),
               {"source": "rocprofv3 --kernel-trace --stats of --profile_pass, its own run", "sizes": opts.sizes, "kernels": rows})
    sys.exit(0)

if opts.kernel_trace:
    launches = []
    with open(opts.kernel_trace) as f:
        for r in csv.DictReader(f):
            for name in KERNELS:
                if name in r["Kernel_Name"]:
                    launches.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    launches.sort()
    counts = [int(x) for x in opts.phase_sweeps.split(",")]     # launch sequences per phase: 2-opt, Or-opt, 2-opt, ..
    total = sum(counts)
    tail = launches[3 * opts.skip_sequences:3 * (opts.skip_sequences + total)]
    idle = launches[3 * (opts.skip_sequences + total):]          # enqueued before the poll that saw the tour done
    assert len(tail) == 3 * total and [k for _, k, _ in tail[:3]] == list(KERNELS)
    split = {ph: {k: [] for k in KERNELS} for ph in ("two_opt", "or_opt")}
    at = 0
    for p, c in enumerate(counts):
        for _ in range(c):
            for q, k in enumerate(KERNELS):
                assert tail[at + q][1] == k
                split["two_opt" if p % 2 == 0 else "or_opt"][k].append(tail[at + q][2])
            at += 3
    summary = {ph: {k: {"launches": len(v), "avg_us": float(np.mean(v)) if v else None, "total_ms": float(np.sum(v)) / 1e3}
                    for k, v in d.items()} for ph, d in split.items()}
    update_out("kernel_trace_n" + "_".join(str(n) for n in opts.sizes),
               {"source": "rocprofv3 --kernel-trace of --profile_pass, its own run; the launch sequences of the search proper",
                "sizes": opts.sizes, "warm_up_sequences_skipped": opts.skip_sequences, "launch_sequences_by_phase": counts,
                "by_phase": summary, "launches_after_the_tour_was_done": len(idle),
                "after_done_total_ms": float(sum(x[2] for x in idle)) / 1e3})
    sys.exit(0)

if opts.verify:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_local_search_emulation as E
    saved = np.load(opts.verify)
    res = []
    for n in opts.sizes:
        t0 = time.perf_counter()
        phases = []
        tour, c = E.search_tour(saved[f"pts_{n}"], saved[f"start_{n}"][0], int(saved[f"cap_{n}"]), opts.max_rounds,
                                opts.select_rounds, phases=phases)
        gpu = {k: int(saved[f"{k}_{n}"]) for k in KEYS}
        res.append({"n": n, "emulation": c, "gpu": gpu, "phases": phases, "tours_equal": bool(np.array_equal(tour, saved[f"tours_{n}"][0])),
                    "emulation_s": time.perf_counter() - t0})
        assert c == gpu and res[-1]["tours_equal"]
    update_out("emulation", res)
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd.decode import (batched_local_search_torch, batched_multi_local_search_torch, batched_multi_two_opt_torch,  # noqa: E402
                                merge_tours)
from difusco_amd.synthetic import tsp_instance  # noqa: E402

dev = torch.device("cuda:0")
out = {"metric": "time to stop", "unit": "ms", "data": "synthetic heat, no trained checkpoint", "repeats": opts.repeats,
       "select_rounds": opts.select_rounds, "max_rounds": opts.max_rounds, "cases": []}
keep = {}


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
    new = lambda c=cap: batched_multi_local_search_torch(pts64, tour0, max_iterations=c, device=dev, max_rounds=opts.max_rounds,
                                                         select_rounds=opts.select_rounds)
    new(3)                                                                                     # warm-up
    if opts.profile_pass:
        _, stats = new()
        print(json.dumps({"n": n, **stats}))
        continue
    batched_local_search_torch(pts64, tour0, max_iterations=10, device=dev, max_rounds=opts.max_rounds)
    batched_multi_two_opt_torch(pts64, tour0, max_iterations=3, device=dev, select_rounds=opts.select_rounds)
    ms = {"2opt+oropt": [], "multi2opt": [], "multi2opt+oropt": []}
    for _ in range(opts.repeats):                                                              # interleaved: same clocks for all
        ls_stats = {}
        t, (exact, exact_two) = timed(lambda: batched_local_search_torch(pts64, tour0, max_iterations=cap, device=dev,
                                                                         max_rounds=opts.max_rounds, stats=ls_stats))
        ms["2opt+oropt"].append(t)
        m_stats = {}
        t, (multi, multi_sweeps) = timed(lambda: batched_multi_two_opt_torch(pts64, tour0, max_iterations=cap, device=dev,
                                                                             select_rounds=opts.select_rounds, stats=m_stats))
        ms["multi2opt"].append(t)
        t, (got, stats) = timed(lambda: new(cap))
        ms["multi2opt+oropt"].append(t)
    med = {m: float(np.median(v)) for m, v in ms.items()}
    sweeps = stats["two_opt_sweeps"] + stats["or_opt_sweeps"]
    gap = min(ms["2opt+oropt"]) - max(ms["multi2opt+oropt"])
    case = {"workload": f"TSP-{n} K={k}, decoded start tour, one tour", "cap": cap, "tour_length_start": length(tour0[0]),
            "2opt+oropt": {"two_opt_sweeps": int(exact_two), "or_opt_sweeps": int(ls_stats["or_opt_iterations"]),
                           "moves": int(exact_two) + int(ls_stats["or_opt_iterations"]), "rounds": int(ls_stats["rounds"]),
                           "cap_is_per_phase": True, "ms": spread(ms["2opt+oropt"]), "tour_length_after": length(exact[0])},
            "multi2opt": {"two_opt_sweeps": int(multi_sweeps), "moves": int(m_stats["moves"]), "stopped_by_cap": bool(multi_sweeps >= cap),
                          "ms": spread(ms["multi2opt"]), "tour_length_after": length(multi[0])},
            "multi2opt+oropt": dict(stats, stopped_by_cap=bool(sweeps >= cap), ms=spread(ms["multi2opt+oropt"]),
                                    tour_length_after=length(got[0]), length_over_2opt_oropt=length(got[0]) / length(exact[0]),
                                    length_over_multi2opt=length(got[0]) / length(multi[0])),
            "2opt+oropt_over_new": med["2opt+oropt"] / med["multi2opt+oropt"], "new_over_multi2opt": med["multi2opt+oropt"] / med["multi2opt"],
            "new_below_2opt+oropt_by_more_than_both_spreads": bool(gap > 0)}
    out["cases"].append(case)
    keep.update({f"pts_{n}": pts64, f"start_{n}": tour0, f"cap_{n}": cap, f"tours_{n}": got, **{f"{k2}_{n}": stats[k2] for k2 in KEYS}})
if not opts.profile_pass:
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    if opts.save_tours:
        os.makedirs(os.path.dirname(os.path.abspath(opts.save_tours)), exist_ok=True)
        np.savez(opts.save_tours, **keep)
