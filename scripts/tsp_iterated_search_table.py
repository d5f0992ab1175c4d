#!/usr/bin/env python
"""The CPU table of DESIGN 5.2g: the end length of the iterated multi-move local search
(tests/tsp_iterated_search_emulation.py) after 30, 100 and 300 kicks, for kick_size in {1, 2, 4, 8, 16} and span in
{3, 10, 30, 100}.  Uniform points from ``np.random.default_rng(n)``, n in {200, 500, 1000}, nearest-neighbour start, seed 0,
offset 0.  No GPU.  One JSON line per (n, kick_size, span), then one line with the mean relative end length (end / first
descent) of every pair at 100 kicks and the pair with the lowest one: the defaults of ``kick_size`` and ``span``.

    python scripts/tsp_iterated_search_table.py [--sizes 200,500,1000] [--jobs J]

A run of 300 kicks is read at 30 and 100 as well (a kick depends on the kicks before it only)."""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multi_two_opt_emulation as M  # noqa: E402
import tsp_iterated_search_emulation as T  # noqa: E402

KICKS = (30, 100, 300)
KICK_SIZES = (1, 2, 4, 8, 16)
SPANS = (3, 10, 30, 100)


def run(job):
    n, kick_size, span = job
    pts = np.random.default_rng(n).random((n, 2))
    start = M.nearest_neighbour_tour(pts)
    trace = []
    _, c, per = T.search_tour(pts, start, 0, 0, kicks=max(KICKS), kick_size=kick_size, span=span, max_iterations=10 ** 6,
                              trace=trace)
    row = {"n": n, "kick_size": kick_size, "span": span, "first_length": per["first_length"],
           "sweeps": c["two_opt_sweeps"] + c["or_opt_sweeps"], "segments_swapped": per["segments_swapped"]}
    length, improved = per["first_length"], 0
    for t, (_, _, lc, take) in enumerate(trace):
        if take:
            improved += lc < length
            length = lc
        if t + 1 in KICKS:
            row[f"length_{t + 1}"], row[f"improved_{t + 1}"] = length, improved
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,500,1000")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(",")]
    jobs = [(n, k, s) for n in sorted(sizes, reverse=True) for k in KICK_SIZES for s in SPANS]
    rel = {}
    with ProcessPoolExecutor(max_workers=args.jobs) as pool:
        for row in pool.map(run, jobs):
            print(json.dumps(row), flush=True)
            rel.setdefault((row["kick_size"], row["span"]), []).append(row["length_100"] / row["first_length"])
    mean = {k: float(np.mean(v)) for k, v in rel.items()}
    best = min(mean, key=lambda k: (mean[k], k))
    print(json.dumps({"mean_relative_length_100": {f"{k[0]},{k[1]}": v for k, v in sorted(mean.items())},
                      "best_kick_size": best[0], "best_span": best[1]}), flush=True)
