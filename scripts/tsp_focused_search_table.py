#!/usr/bin/env python
"""The CPU table of DESIGN 5.2h: the iterated multi-move local search with full descents
(tests/tsp_iterated_search_emulation.py) against the one with focused descents (tests/tsp_focused_search_emulation.py), on
uniform points from ``np.random.default_rng(n)``, n in {200, 500, 1000}, nearest-neighbour start, kick_size 16, span 30, offset
0, at 30 and 100 kicks, for the Philox seeds 0 .. ``--seeds`` - 1 (one trajectory ranks nothing).  No GPU, no trained checkpoint.
Writes one JSON line per (n, kicks, seed, descent) to ``profiles/tsp_focused_search/table.jsonl`` (``--out``) and then one
summary line per (n, kicks): the mean [min, max] over the seeds of both descents.

    python scripts/tsp_focused_search_table.py [--sizes 200,500,1000] [--kicks 30,100] [--seeds 5] [--jobs J]

Columns: end length / first length, kicks kept, the share of pairs evaluated (pairs of all focused sweeps / (sweeps n^2 / 2)),
mean and max proposals per focused sweep, ``closing_sweeps``."""
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
import tsp_iterated_search_emulation as T  # noqa: E402

KICK_SIZE, SPAN = 16, 30


def run(job):
    n, kicks, seed, descent = job
    pts = np.random.default_rng(n).random((n, 2))
    start = M.nearest_neighbour_tour(pts)
    kw = dict(kicks=kicks, kick_size=KICK_SIZE, span=SPAN, max_iterations=10 ** 6)
    row = {"n": n, "kicks": kicks, "seed": seed, "descent": descent}
    if descent == "full":
        _, c, per = T.search_tour(pts, start, seed, 0, **kw)
    else:
        log, count = [], [0]
        _, c, per = F.search_tour(pts, start, seed, 0, log=log, count=count, **kw)
        props = [m for _, m, _ in log]
        row.update(focused_sweeps=len(log), pair_share=count[0] / (len(log) * n * n / 2), proposals_mean=float(np.mean(props)),
                   proposals_max=int(max(props)), closing_sweeps=per["closing_sweeps"])
    row.update(first_length=per["first_length"], final_length=per["final_length"],
               length_over_first=per["final_length"] / per["first_length"], kicks_kept=per["kicks_kept"],
               sweeps=c["two_opt_sweeps"] + c["or_opt_sweeps"])
    return row


def spread(v):
    return {"mean": float(np.mean(v)), "min": float(min(v)), "max": float(max(v))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,500,1000")
    ap.add_argument("--kicks", default="30,100")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_focused_search", "table.jsonl"))
    args = ap.parse_args()
    sizes = sorted((int(v) for v in args.sizes.split(",")), reverse=True)
    kicks = sorted((int(v) for v in args.kicks.split(",")), reverse=True)
    jobs = [(n, k, s, d) for n in sizes for k in kicks for s in range(args.seeds) for d in ("full", "focused")]
    rows = []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f, ProcessPoolExecutor(max_workers=args.jobs) as pool:
        for row in pool.map(run, jobs):
            rows.append(row)
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(json.dumps(row), flush=True)
        for n in sizes:
            for k in kicks:
                line = {"n": n, "kicks": k, "seeds": args.seeds}
                for d in ("full", "focused"):
                    sel = [r for r in rows if (r["n"], r["kicks"], r["descent"]) == (n, k, d)]
                    line[d] = {"length_over_first": spread([r["length_over_first"] for r in sel]),
                               "kicks_kept": spread([r["kicks_kept"] for r in sel])}
                    if d == "focused":
                        line[d].update(pair_share=spread([r["pair_share"] for r in sel]),
                                       proposals_mean=spread([r["proposals_mean"] for r in sel]),
                                       proposals_max=max(r["proposals_max"] for r in sel),
                                       closing_sweeps=spread([r["closing_sweeps"] for r in sel]))
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)
