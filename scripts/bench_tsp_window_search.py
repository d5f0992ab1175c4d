#!/usr/bin/env python
"""The windowed iterated search against the two iterated entries it does not touch, timed on the GPU box in one process:
``batched_window_search_torch`` (``difusco_tsp_window_search_ragged``) at ``--window`` / ``--kick_size`` / ``--span`` (default: the
recommended ``decode.TSP_WINDOW`` / ``TSP_WINDOW_KICK_SIZE`` / ``TSP_WINDOW_KICK_SPAN``), ``--window_kicks`` per window and pass and
passes in ``--passes``, against ``batched_iterated_search_torch`` with ``descent="full"`` (``difusco_tsp_iterated_search_ragged``)
and ``descent="focused"`` (``difusco_tsp_focused_search_ragged``) at kicks in {0, 100} - the parent commit's code.  The set-up is
that of scripts/bench_tsp_focused_search.py: the decoded start tour of ``scripts/bench_decode.py`` (TSP-N, K = 100, synthetic heat -
no trained checkpoint, so the lengths say nothing about solution quality on real heatmaps), N = 10^3 at cap 200 and N = 10^4 at
cap 5000 per descent, one tour, seed 0, offset 0, a warm-up of each entry, ``--repeats`` interleaved repeats, median [min, max].
Writes ``profiles/tsp_window_search/bench.json`` (``--out``).

Per mode: the time to stop, the time per kick draw - iterated entries: (time at 100 kicks - time at 0 kicks) / 100; window mode:
(time at K kicks - time at 0 kicks, same passes) / (windows searched x K) -, the end length over the first descent's and the host
synchronisations (the window mode's are those of its two descents: it has none of its own between them).  ``equal_time``: the
focused search at 100 kicks against the window mode at the largest number of passes whose median time is not above the
focused median.  A figure counts as a gain only where the window mode's worst repeat beats the parent's best.

  --trace N PASSES      one warm-up and ONE window call at that size: the program of a separate
                        ``rocprofv3 --kernel-trace --stats -- python scripts/bench_tsp_window_search.py --trace N PASSES`` pass.
  --trace_stats CSV     no GPU: reads that pass's kernel trace and adds the two new kernels' figures to ``--out``.

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
ap.add_argument("--window", type=int, default=None)
ap.add_argument("--window_kicks", type=int, default=4)
ap.add_argument("--kick_size", type=int, default=None)
ap.add_argument("--span", type=int, default=None)
ap.add_argument("--passes", nargs="+", type=int, default=[1, 2, 4, 8, 16, 32])
ap.add_argument("--select_rounds", type=int, default=4)
ap.add_argument("--max_rounds", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_window_search", "bench.json"))
ap.add_argument("--trace", nargs=2, type=int, default=None, metavar=("N", "PASSES"))
ap.add_argument("--trace_stats", default=None)
opts = ap.parse_args()


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


if opts.trace_stats:
    us = {"win_search_kernel": [], "win_keep_kernel": []}
    with open(opts.trace_stats) as f:
        for r in csv.DictReader(f):
            for k in us:
                if k in r["Kernel_Name"]:
                    us[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    update_out("kernel_trace", {"source": "rocprofv3 --kernel-trace --stats of --trace, its own run, the warm-up call included",
                                **{k: {"launches": len(v), "mean_us": float(np.mean(v)), "min_us": float(min(v)), "max_us": float(max(v)),
                                       "all_us": [float(x) for x in v]} for k, v in us.items() if v}})
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd.decode import (TSP_WINDOW, TSP_WINDOW_KICK_SIZE, TSP_WINDOW_KICK_SPAN, batched_iterated_search_torch,  # noqa: E402
                                batched_window_search_torch, merge_tours)
from difusco_amd.synthetic import tsp_instance  # noqa: E402

dev = torch.device("cuda:0")
if opts.window is None:                                      # the recommended window mode
    opts.window = TSP_WINDOW
win_size = TSP_WINDOW_KICK_SIZE if opts.kick_size is None else opts.kick_size
win_span = TSP_WINDOW_KICK_SPAN if opts.span is None else opts.span
KICKS = 100


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


def iterated(pts64, tour0, cap, descent, kicks, per):
    from difusco_amd.decode import TSP_KICK_SIZE, TSP_KICK_SPAN
    return batched_iterated_search_torch(pts64, tour0, max_iterations=cap, device=dev, max_rounds=opts.max_rounds,
                                         select_rounds=opts.select_rounds, kicks=kicks, kick_size=TSP_KICK_SIZE, span=TSP_KICK_SPAN,
                                         seeds=[0], offsets=[0], stats=per, descent=descent)


def window(pts64, tour0, cap, passes, kicks, per):
    return batched_window_search_torch(pts64, tour0, max_iterations=cap, device=dev, max_rounds=opts.max_rounds,
                                       select_rounds=opts.select_rounds, kicks=kicks, kick_size=win_size, span=win_span, seeds=[0],
                                       offsets=[0], stats=per, window=opts.window, passes=passes)


if opts.trace:
    pts64, tour0, cap = start_of(opts.trace[0])
    window(pts64, tour0, 3, 1, 1, {})                                                          # warm-up
    per = {}
    t, _ = timed(lambda: window(pts64, tour0, cap, opts.trace[1], opts.window_kicks, per))
    print(json.dumps({"trace": opts.trace, "ms": t, "windows_searched": per["windows_searched"].tolist()}))
    sys.exit(0)

out = {"metric": "time to stop", "unit": "ms", "data": "synthetic heat, no trained checkpoint", "repeats": opts.repeats,
       "select_rounds": opts.select_rounds, "max_rounds": opts.max_rounds, "window": opts.window, "window_kicks": opts.window_kicks,
       "window_kick_size": win_size, "window_span": win_span,
       "parents": "descent='full': difusco_tsp_iterated_search_ragged, descent='focused': difusco_tsp_focused_search_ragged, "
                  "at their default kick_size 16 and span 30", "cases": []}
for n in opts.sizes:
    pts64, tour0, cap = start_of(n)
    for d in ("full", "focused"):
        iterated(pts64, tour0, 3, d, 2, {})                                                    # warm-up
    window(pts64, tour0, 3, 2, 1, {})
    settings = [("full", 0), ("full", KICKS), ("focused", 0), ("focused", KICKS)]
    settings += [("window", (r, k)) for r in opts.passes for k in (0, opts.window_kicks)]
    ms = {s: [] for s in settings}
    last = {}
    for _ in range(opts.repeats):                                                              # interleaved: same clocks for all
        for s in settings:
            per = {}
            if s[0] == "window":
                t, (got, stats) = timed(lambda: window(pts64, tour0, cap, s[1][0], s[1][1], per))
            else:
                t, (got, stats) = timed(lambda: iterated(pts64, tour0, cap, s[0], s[1], per))
            ms[s].append(t)
            last[s] = per
    case = {"workload": f"TSP-{n} K=100, decoded start tour, one tour", "cap_per_descent": cap}
    for d in ("full", "focused"):
        per = last[d, KICKS]
        a, b = ms[d, KICKS], ms[d, 0]
        case[d] = {"kicks": KICKS, "ms": spread(a), "ms_at_0_kicks": spread(b), "host_syncs": int(per["host_syncs"]),
                   "host_syncs_at_0_kicks": int(last[d, 0]["host_syncs"]),
                   "ms_per_kick": {"median": float((np.median(a) - np.median(b)) / KICKS), "min": float((min(a) - max(b)) / KICKS),
                                   "max": float((max(a) - min(b)) / KICKS)},
                   "kicks_improved": int(per["kicks_improved"][0]),
                   "length_over_first": float(per["final_length"][0] / per["first_length"][0])}
    case["window"] = {}
    for r in opts.passes:
        per = last["window", (r, opts.window_kicks)]
        a, b = ms["window", (r, opts.window_kicks)], ms["window", (r, 0)]
        draws = int(per["windows_searched"][0]) * opts.window_kicks
        case["window"][str(r)] = {
            "passes": r, "kicks_per_window_and_pass": opts.window_kicks, "kick_draws": draws, "ms": spread(a), "ms_at_0_kicks": spread(b),
            "host_syncs_between_the_descents": 0,
            "ms_per_kick_draw": {"median": float((np.median(a) - np.median(b)) / draws), "min": float((min(a) - max(b)) / draws),
                                 "max": float((max(a) - min(b)) / draws)},
            "passes_kept": int(per["passes_kept"][0]), "kicks_improved": int(per["kicks_improved"][0]),
            "closing_sweeps": int(per["closing_sweeps"][0]), "window_sweeps": int(per["window_sweeps"][0]),
            "length_over_first": float(per["final_length"][0] / per["first_length"][0])}
    foc = case["focused"]
    fit = [r for r in opts.passes if case["window"][str(r)]["ms"]["median"] <= foc["ms"]["median"]]
    if fit:
        w = case["window"][str(max(fit))]
        case["equal_time"] = {"focused_ms": foc["ms"]["median"], "focused_length_over_first": foc["length_over_first"],
                              "window_passes": max(fit), "window_ms": w["ms"]["median"], "window_kick_draws": w["kick_draws"],
                              "window_length_over_first": w["length_over_first"]}
    else:
        case["equal_time"] = None                                # one pass already takes longer than the focused search
    case["window_per_draw_max_below_parent_per_kick_min"] = {
        str(r): {d: bool(case["window"][str(r)]["ms_per_kick_draw"]["max"] < case[d]["ms_per_kick"]["min"]) for d in ("full", "focused")}
        for r in opts.passes}
    out["cases"].append(case)
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
with open(opts.out, "w") as f:
    f.write(json.dumps(out) + "\n")
