#!/usr/bin/env python
"""Which window, kick size and span for the windowed iterated search?  CPU only: the numpy restatement of the rule
(tests/tsp_window_search_emulation.py) on uniform instances - points from ``default_rng(n)``, n in {1000, 2000} (``--sizes``),
the nearest-neighbour tour descended once as the start, Philox seeds 0 .. 4 (``--seeds``) - over window in {128, 256, 512} x
kick_size in {1, 2, 4, 8} x span in {10, 30} at equal passes x kicks (``--passes`` 2, ``--kicks`` 2).  Baseline: the full iterated
search (tests/tsp_iterated_search_emulation.py) with the row's kick size and span at the same total number of kick draws per
city, passes x kicks x (windows of a pass) kicks; one run per (n, seed, kick_size, span) at the count of the smallest window,
read off at the lower counts of the larger windows (the kicks of a run are a prefix of any longer run).  Writes one JSON line per
run and per table row to ``profiles/tsp_window_search/table.jsonl`` (``--out``): mean [min, max] over the seeds of end length /
first length, the lowest row of every size and the lowest row over the sizes.  Three to five synthetic instances choose a default and rank nothing."""
import argparse
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", nargs="+", type=int, default=[1000, 2000])
ap.add_argument("--seeds", nargs="+", type=int, default=[0, 1, 2, 3, 4])
ap.add_argument("--windows", nargs="+", type=int, default=[128, 256, 512])
ap.add_argument("--kick_sizes", nargs="+", type=int, default=[1, 2, 4, 8])
ap.add_argument("--spans", nargs="+", type=int, default=[10, 30])
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--kicks", type=int, default=2)
ap.add_argument("--workers", type=int, default=4)
ap.add_argument("--summarise", default=None, help="a file of runs written earlier: rewrite its table rows, run nothing")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_window_search", "table.jsonl"))
opts = ap.parse_args()
STARTS = {}


def start_of(n):
    import multi_local_search_emulation as E
    import multi_two_opt_emulation as M
    if n not in STARTS:
        pts = np.random.default_rng(n).random((n, 2))
        STARTS[n] = (pts, E.search_tour(pts, M.nearest_neighbour_tour(pts))[0])
    return STARTS[n]


def windows_of(n, window):
    return -(-n // window)                                       # of an even pass


def run(task):
    import tsp_iterated_search_emulation as T
    import tsp_window_search_emulation as W
    kind, n, seed, kick_size, span, window = task
    pts, start = start_of(n)
    if kind == "window":
        _, _, _, per = W.search_tour(pts, start, seed, 0, window=window, passes=opts.passes, kicks=opts.kicks, kick_size=kick_size,
                                     span=span)
        return dict(kind=kind, n=n, seed=seed, kick_size=kick_size, span=span, window=window, passes=opts.passes, kicks=opts.kicks,
                    ratio=per["final_length"] / per["first_length"], kicks_improved=per["kicks_improved"],
                    passes_kept=per["passes_kept"], closing_sweeps=per["closing_sweeps"])
    counts = {w: opts.passes * opts.kicks * windows_of(n, w) for w in opts.windows}
    trace = []
    _, _, per = T.search_tour(pts, start, seed, 0, kicks=max(counts.values()), kick_size=kick_size, span=span, trace=trace)
    lengths = [per["first_length"]]
    for _, _, lc, take in trace:
        lengths.append(lc if take else lengths[-1])
    return dict(kind=kind, n=n, seed=seed, kick_size=kick_size, span=span,
                ratio_at={str(w): lengths[c] / lengths[0] for w, c in counts.items()}, kicks_at={str(w): c for w, c in counts.items()})


def spread(v):
    return {"mean": float(np.mean(v)), "min": float(min(v)), "max": float(max(v))}


def summarise(runs):
    """The table rows of the runs, the lowest row of every size and the lowest row over the sizes (the mean of their means)."""
    rows = []
    for n in opts.sizes:
        for w in opts.windows:
            for ks in opts.kick_sizes:
                for sp in opts.spans:
                    pick = lambda kind: sorted((r for r in runs if (r["kind"], r["n"], r["kick_size"], r["span"]) == (kind, n, ks, sp)
                                                and r.get("window", w) == w), key=lambda r: r["seed"])
                    win, full = pick("window"), pick("full")
                    rows.append(dict(kind="row", n=n, window=w, kick_size=ks, span=sp, passes=opts.passes, kicks=opts.kicks,
                                     seeds=[r["seed"] for r in win], window_ratio=spread([r["ratio"] for r in win]),
                                     full_kicks=full[0]["kicks_at"][str(w)],
                                     full_ratio=spread([r["ratio_at"][str(w)] for r in full])))
    out = list(rows)
    keys = ("window", "kick_size", "span")
    for n in opts.sizes:
        best = min((r for r in rows if r["n"] == n), key=lambda r: r["window_ratio"]["mean"])
        out.append(dict(kind="lowest", n=n, **{k: best[k] for k in keys + ("window_ratio", "full_ratio")}))
    over = {}
    for r in rows:
        over.setdefault(tuple(r[k] for k in keys), []).append(r)
    best = min(over.values(), key=lambda v: np.mean([r["window_ratio"]["mean"] for r in v]))
    out.append(dict(kind="lowest_over_sizes", **{k: best[0][k] for k in keys}, sizes=[r["n"] for r in best],
                    window_ratio_mean=float(np.mean([r["window_ratio"]["mean"] for r in best])),
                    full_ratio_mean=float(np.mean([r["full_ratio"]["mean"] for r in best]))))
    return out


if __name__ == "__main__":
    if opts.summarise:                                           # no search: the rows of the runs of an earlier file
        runs = [r for r in map(json.loads, open(opts.summarise)) if r["kind"] in ("window", "full")]
        with open(opts.out, "w") as f:
            for r in runs + summarise(runs):
                f.write(json.dumps(r) + "\n")
        print("".join(l for l in open(opts.out) if '"kind": "lowest' in l))
        sys.exit(0)
    for n in opts.sizes:
        start_of(n)                                              # before the fork: the workers share the starts
    tasks = [(kind, n, seed, ks, sp, w) for n in opts.sizes for kind in ("window", "full") for ks in opts.kick_sizes
             for sp in opts.spans for seed in opts.seeds for w in (opts.windows if kind == "window" else [0])]
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    runs = []
    with open(opts.out, "w") as f, Pool(opts.workers) as pool:
        for r in pool.imap_unordered(run, tasks):
            runs.append(r)
            f.write(json.dumps(r) + "\n")
            f.flush()
        for r in summarise(runs):
            f.write(json.dumps(r) + "\n")
    print("".join(l for l in open(opts.out) if '"kind": "lowest' in l))
