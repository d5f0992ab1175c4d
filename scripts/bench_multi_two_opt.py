#!/usr/bin/env python
"""Multi-move 2-opt timing on the GPU box: the exact 2-opt, the screened 2-opt (``batched_two_opt_torch``, both the code of the
parent commit, unchanged) and the multi-move 2-opt (``batched_multi_two_opt_torch``) from the decoded start tour of
``scripts/bench_decode.py`` (TSP-N, K = 100, synthetic heat - no trained checkpoint, so the lengths say nothing about solution
quality on real heatmaps), N = 10^3 at cap 200 and N = 10^4 at cap 5000.  Writes ``profiles/multi_two_opt/bench.json`` (``--out``).

Timed run (the default): one process, a warm-up of each method, ``--repeats`` interleaved repeats, median [min, max] of the time
to stop; sweeps, moves and end length of every method.  A multi-move sweep is three launches; an exact sweep applies one move.
``--save_tours PATH`` keeps the start tours and the multi-move results (npz).

Three more modes, all separate from the timed run:
  --profile_pass        one multi-move search per size after a warm-up and nothing else: the program to put behind
                        ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME --``;
  --kernel_stats CSV    no GPU: reads that run's ``*_kernel_stats.csv`` and adds the per-launch averages of the three kernels
                        to ``--out`` under ``kernel_stats_n<sizes>`` (pass the run's ``--sizes``; the profiled run holds the
                        warm-up's launches too; the averages are over all of them);
  --verify NPZ          no GPU: runs tests/multi_two_opt_emulation.py from the saved start tours and adds to ``--out`` whether
                        sweeps, moves and tours equal the GPU's."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_two_opt", "bench.json"))
ap.add_argument("--save_tours", default=None)
ap.add_argument("--profile_pass", action="store_true")
ap.add_argument("--kernel_stats", default=None)
ap.add_argument("--verify", default=None)
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


if opts.kernel_stats:
    rows = {}
    with open(opts.kernel_stats) as f:
        for r in csv.DictReader(f):
            for name in ("mt_prep_kernel", "mt_row_full_kernel", "mt_select_kernel"):
                if name in r["Name"]:
                    rows[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                                  "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                  "max_us": float(r["MaxNs"]) / 1e3}
    update_out("kernel_stats_n" + "_".join(str(n) for n in opts.sizes),
               {"source": "rocprofv3 --kernel-trace --stats of --profile_pass, its own run", "sizes": opts.sizes, "kernels": rows})
    sys.exit(0)

if opts.verify:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_two_opt_emulation as E
    saved = np.load(opts.verify)
    res = []
    for n in opts.sizes:
        t0 = time.perf_counter()
        tours, sweeps, moves = E.multi_two_opt(saved[f"pts_{n}"], saved[f"start_{n}"], int(saved[f"cap_{n}"]), opts.select_rounds)
        res.append({"n": n, "emulation_sweeps": int(sweeps), "emulation_moves": int(moves), "gpu_sweeps": int(saved[f"sweeps_{n}"]),
                    "gpu_moves": int(saved[f"moves_{n}"]), "tours_equal": bool(np.array_equal(tours, saved[f"tours_{n}"])),
                    "emulation_s": time.perf_counter() - t0})
        assert res[-1]["emulation_sweeps"] == res[-1]["gpu_sweeps"] and res[-1]["emulation_moves"] == res[-1]["gpu_moves"]
        assert res[-1]["tours_equal"]
    update_out("emulation", res)
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd.decode import batched_multi_two_opt_torch, batched_two_opt_torch, merge_tours  # noqa: E402
from difusco_amd.synthetic import tsp_instance  # noqa: E402

dev = torch.device("cuda:0")
out = {"metric": "time to stop", "unit": "ms", "data": "synthetic heat, no trained checkpoint", "repeats": opts.repeats,
       "select_rounds": opts.select_rounds, "cases": []}
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
    multi = lambda c=cap, s=None: batched_multi_two_opt_torch(pts64, tour0, max_iterations=c, device=dev,
                                                              select_rounds=opts.select_rounds, stats=s)
    multi(3)                                                                                   # warm-up
    if opts.profile_pass:
        multi()
        continue
    batched_two_opt_torch(pts64, tour0, max_iterations=10, device=dev)
    batched_two_opt_torch(pts64, tour0, max_iterations=10, device=dev, method="screened")
    ms = {"exact": [], "screened": [], "multi2opt": []}
    for _ in range(opts.repeats):                                                              # interleaved: same clocks for all
        t, (exact, exact_moves) = timed(lambda: batched_two_opt_torch(pts64, tour0, max_iterations=cap, device=dev))
        ms["exact"].append(t)
        t, (screened, screened_moves) = timed(lambda: batched_two_opt_torch(pts64, tour0, max_iterations=cap, device=dev,
                                                                            method="screened"))
        ms["screened"].append(t)
        stats = {}
        t, (multi_tours, sweeps) = timed(lambda: multi(cap, stats))
        ms["multi2opt"].append(t)
    assert np.array_equal(exact, screened) and exact_moves == screened_moves
    launches = sweeps + (1 if sweeps < cap else 0)                # the sweep that finds no proposal ends a search below the cap
    med = {m: float(np.median(v)) for m, v in ms.items()}
    gap = min(ms["screened"]) - max(ms["multi2opt"])
    case = {"workload": f"TSP-{n} K={k}, decoded start tour", "cap": cap, "tour_length_start": length(tour0[0]),
            "exact": {"sweeps": int(exact_moves), "moves": int(exact_moves), "stopped_by_cap": bool(exact_moves >= cap),
                      "ms": spread(ms["exact"]), "ms_per_sweep": med["exact"] / max(exact_moves, 1), "tour_length_after": length(exact[0])},
            "screened": {"sweeps": int(screened_moves), "moves": int(screened_moves), "stopped_by_cap": bool(screened_moves >= cap),
                         "ms": spread(ms["screened"]), "ms_per_sweep": med["screened"] / max(screened_moves, 1),
                         "tour_length_after": length(screened[0])},
            "multi2opt": {"sweeps": int(sweeps), "moves": int(stats["moves"]), "stopped_by_cap": bool(sweeps >= cap),
                          "launch_sequences": int(launches), "ms": spread(ms["multi2opt"]),
                          "ms_per_sweep": med["multi2opt"] / max(launches, 1), "tour_length_after": length(multi_tours[0]),
                          "length_over_exact": length(multi_tours[0]) / length(exact[0])},
            "exact_over_multi2opt": med["exact"] / med["multi2opt"], "screened_over_multi2opt": med["screened"] / med["multi2opt"],
            "multi2opt_below_screened_by_more_than_both_spreads": bool(gap > 0)}
    out["cases"].append(case)
    keep.update({f"pts_{n}": pts64, f"start_{n}": tour0, f"cap_{n}": cap, f"tours_{n}": multi_tours, f"sweeps_{n}": sweeps,
                 f"moves_{n}": stats["moves"]})
if not opts.profile_pass:
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    if opts.save_tours:
        os.makedirs(os.path.dirname(os.path.abspath(opts.save_tours)), exist_ok=True)
        np.savez(opts.save_tours, **keep)
