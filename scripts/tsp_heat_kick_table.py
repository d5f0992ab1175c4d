#!/usr/bin/env python
"""The CPU table of DESIGN 5.2i: the iterated multi-move local search with uniform kicks (tests/tsp_iterated_search_emulation.py,
tests/tsp_focused_search_emulation.py) against the one with heat-biased kicks (tests/tsp_heat_kick_emulation.py), on uniform
points from ``np.random.default_rng(n)``, n in {200, 500, 1000}, nearest-neighbour start, kick_size 16, span 30, offset 0, at 30
and 100 kicks, full and focused descents, for the Philox seeds 0 .. ``--seeds`` - 1.  No GPU, no trained checkpoint.

THE HEAT IS SYNTHETIC, so the table ranks nothing for a trained model.  The graph is the k-NN graph with K = 10; a GUIDE tour
(150 uniform kicks of the full search from a random start, Philox seed 12345) labels its edges:

    guide    heat 1.0 on an edge of the guide tour (either direction), 0.0 elsewhere
    flip10   the same with 10 % of the labels flipped        flip30   with 30 % flipped
    noise    uniform random heat: no information

Writes one JSON line per (n, kicks, seed, descent, heat) to ``profiles/tsp_heat_kick/table.jsonl`` (``--out``), then one line per
n with the guide's length over the first descent's, then one summary line per (n, kicks, descent): mean [min, max] over the seeds
of end length / first length and of the kicks kept, for ``uniform`` and every heat.

    python scripts/tsp_heat_kick_table.py [--sizes 200,500,1000] [--kicks 30,100] [--seeds 5] [--jobs J]"""
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
import tsp_focused_search_emulation as F  # noqa: E402
import tsp_heat_kick_emulation as H  # noqa: E402
import tsp_iterated_search_emulation as T  # noqa: E402

KICK_SIZE, SPAN, K, GUIDE_KICKS, GUIDE_SEED = 16, 30, 10, 150, 12345
HEATS = ("guide", "flip10", "flip30", "noise")


def points_of(n):
    return np.random.default_rng(n).random((n, 2))


def guide_of(n):
    pts = points_of(n)
    rng = np.random.default_rng(10 ** 6 + n)
    start = np.concatenate([[0], rng.permutation(n - 1) + 1, [0]])
    tour, _, per = T.search_tour(pts, start, GUIDE_SEED, 0, kicks=GUIDE_KICKS, kick_size=KICK_SIZE, span=SPAN, max_iterations=10 ** 6)
    return n, tour, per["final_length"]


def heat_of(kind, n, rp, col, guide):
    on = set()
    for u, v in zip(guide[:-1].tolist(), guide[1:].tolist()):
        on.add((u, v))
        on.add((v, u))
    rows = np.repeat(np.arange(n), np.diff(rp))
    label = np.array([(int(u), int(v)) in on for u, v in zip(rows, col)])
    rng = np.random.default_rng(77 + n)
    if kind == "noise":
        return rng.random(len(col)).astype(np.float32)
    if kind != "guide":
        label = label ^ (rng.random(len(col)) < int(kind[4:]) / 100)
    return label.astype(np.float32)


def run(job):
    n, kicks, seed, descent, kind, guide = job
    pts = points_of(n)
    start = M.nearest_neighbour_tour(pts)
    kw = dict(kicks=kicks, kick_size=KICK_SIZE, span=SPAN, max_iterations=10 ** 6)
    if kind == "uniform":
        _, c, per = (T if descent == "full" else F).search_tour(pts, start, seed, 0, **kw)
    else:
        rp, col = H.knn_csr(pts, K)
        _, c, per = H.search_tour(pts, start, rp, col, heat_of(kind, n, rp, col, guide), seed, 0, descent=descent, **kw)
    return {"n": n, "kicks": kicks, "seed": seed, "descent": descent, "heat": kind, "first_length": per["first_length"],
            "final_length": per["final_length"], "length_over_first": per["final_length"] / per["first_length"],
            "kicks_kept": per["kicks_kept"], "sweeps": c["two_opt_sweeps"] + c["or_opt_sweeps"]}


def spread(v):
    return {"mean": float(np.mean(v)), "min": float(min(v)), "max": float(max(v))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,500,1000")
    ap.add_argument("--kicks", default="30,100")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_heat_kick", "table.jsonl"))
    args = ap.parse_args()
    sizes = sorted((int(v) for v in args.sizes.split(",")), reverse=True)
    kicks = sorted((int(v) for v in args.kicks.split(",")), reverse=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows = []
    with open(args.out, "w") as f, ProcessPoolExecutor(max_workers=args.jobs) as pool:
        guides = {n: (tour, length) for n, tour, length in pool.map(guide_of, sizes)}
        jobs = [(n, k, s, d, h, guides[n][0]) for n in sizes for k in kicks for s in range(args.seeds) for d in ("full", "focused")
                for h in ("uniform",) + HEATS]
        for row in pool.map(run, jobs):
            rows.append(row)
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(json.dumps(row), flush=True)
        for n in sizes:
            first = next(r["first_length"] for r in rows if r["n"] == n)
            line = {"n": n, "guide_kicks": GUIDE_KICKS, "guide_length_over_first": guides[n][1] / first, "heat": "synthetic"}
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
        for n in sizes:
            for k in kicks:
                for d in ("full", "focused"):
                    line = {"n": n, "kicks": k, "descent": d, "seeds": args.seeds, "heat": "synthetic: ranks nothing for a trained model"}
                    for h in ("uniform",) + HEATS:
                        sel = [r for r in rows if (r["n"], r["kicks"], r["descent"], r["heat"]) == (n, k, d, h)]
                        line[h] = {"length_over_first": spread([r["length_over_first"] for r in sel]),
                                   "kicks_kept": spread([r["kicks_kept"] for r in sel])}
                    f.write(json.dumps(line) + "\n")
                    print(json.dumps(line), flush=True)
