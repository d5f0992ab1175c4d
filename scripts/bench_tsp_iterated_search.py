#!/usr/bin/env python
"""Iterated multi-move local search timing on the GPU box: ``batched_iterated_search_torch`` with kicks in {0, 10, 30, 100, 300}
(``--kicks``) from the decoded start tour of ``scripts/bench_decode.py`` (TSP-N, K = 100, synthetic heat - no trained checkpoint,
so the lengths say nothing about solution quality on real heatmaps), N = 10^3 at cap 200 and N = 10^4 at cap 5000 per descent,
and beside ``kicks = 0`` the multi-move local search of the parent commit, unchanged (``batched_multi_local_search_torch``).
Writes ``profiles/tsp_iterated_search/bench.json`` (``--out``).

Timed run (the default): one tour, seed 0, offset 0, one process, a warm-up of each entry, ``--repeats`` interleaved repeats (one
pass over all settings per repeat, so drifting clocks hit every setting alike), median [min, max] of the time to stop; the end
length (the library's fixed-order sum), the kicks kept and improved, the sweeps and the host synchronisations of every setting.
``--save_tours PATH`` keeps the start tours and the results (npz).

  --verify NPZ          no GPU: runs tests/tsp_iterated_search_emulation.py from the saved start tours for ``--sizes`` and
                        ``--kicks`` (the emulation takes about a second per kick at N = 10^3, far longer at 10^4) and adds to
                        ``--out`` whether tours, counters and lengths equal the GPU's.

No time or length printed here is a test."""
import argparse
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
ap.add_argument("--kicks", nargs="+", type=int, default=[0, 10, 30, 100, 300])
ap.add_argument("--kick_size", type=int, default=None)
ap.add_argument("--span", type=int, default=None)
ap.add_argument("--select_rounds", type=int, default=4)
ap.add_argument("--max_rounds", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_iterated_search", "bench.json"))
ap.add_argument("--save_tours", default=None)
ap.add_argument("--verify", default=None)
opts = ap.parse_args()
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")
PER = ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length")


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
    import tsp_iterated_search_emulation as T
    saved = np.load(opts.verify)
    res = []
    for n in opts.sizes:
        for kicks in opts.kicks:
            t0 = time.perf_counter()
            tour, c, per = T.search_tour(saved[f"pts_{n}"], saved[f"start_{n}"][0], 0, 0, kicks=kicks, kick_size=int(saved["kick_size"]),
                                         span=int(saved["span"]), max_iterations=int(saved[f"cap_{n}"]), max_rounds=opts.max_rounds,
                                         select_rounds=opts.select_rounds)
            tag = f"{n}_{kicks}"
            gpu = {k: int(saved[f"{k}_{tag}"]) for k in KEYS}
            gpu_per = {k: saved[f"{k}_{tag}"].tolist()[0] for k in PER}
            res.append({"n": n, "kicks": kicks, "emulation": c, "gpu": gpu, "emulation_per_tour": per, "gpu_per_tour": gpu_per,
                        "tours_equal": bool(np.array_equal(tour, saved[f"tours_{tag}"][0])), "emulation_s": time.perf_counter() - t0})
            assert c == gpu and res[-1]["tours_equal"] and {k: per[k] for k in PER} == gpu_per
    update_out("emulation", res)
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd.decode import (TSP_KICK_SIZE, TSP_KICK_SPAN, batched_iterated_search_torch,  # noqa: E402
                                batched_multi_local_search_torch, merge_tours)
from difusco_amd.synthetic import tsp_instance  # noqa: E402

dev = torch.device("cuda:0")
kick_size = TSP_KICK_SIZE if opts.kick_size is None else opts.kick_size
span = TSP_KICK_SPAN if opts.span is None else opts.span
out = {"metric": "time to stop", "unit": "ms", "data": "synthetic heat, no trained checkpoint", "repeats": opts.repeats,
       "select_rounds": opts.select_rounds, "max_rounds": opts.max_rounds, "kick_size": kick_size, "span": span, "cases": []}
keep = {"kick_size": kick_size, "span": span}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


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
    cap = 200 if n <= 1000 else 5000
    parent = lambda c=cap: batched_multi_local_search_torch(pts64, tour0, max_iterations=c, device=dev, max_rounds=opts.max_rounds,
                                                            select_rounds=opts.select_rounds)

    def new(kicks, per, c=cap):
        return batched_iterated_search_torch(pts64, tour0, max_iterations=c, device=dev, max_rounds=opts.max_rounds,
                                             select_rounds=opts.select_rounds, kicks=kicks, kick_size=kick_size, span=span,
                                             seeds=[0], offsets=[0], stats=per)
    parent(3)                                                                                  # warm-up
    new(2, {}, 3)
    ms = {"parent": [], **{kicks: [] for kicks in opts.kicks}}
    last = {}
    for _ in range(opts.repeats):                                                              # interleaved: same clocks for all
        t, (base, base_stats) = timed(parent)
        ms["parent"].append(t)
        for kicks in opts.kicks:
            per = {}
            t, (got, stats) = timed(lambda: new(kicks, per))
            ms[kicks].append(t)
            last[kicks] = (got, stats, per)
    case = {"workload": f"TSP-{n} K={k}, decoded start tour, one tour", "cap_per_descent": cap,
            "parent_multi2opt+oropt": dict(base_stats, ms=spread(ms["parent"])), "kicks": {}}
    for kicks in opts.kicks:
        got, stats, per = last[kicks]
        case["kicks"][str(kicks)] = dict(stats, ms=spread(ms[kicks]), host_syncs=per["host_syncs"],
                                         **{key: per[key].tolist()[0] for key in PER},
                                         length_over_first=float(per["final_length"][0] / per["first_length"][0]),
                                         ms_over_parent=float(np.median(ms[kicks]) / np.median(ms["parent"])))
        keep.update({f"tours_{n}_{kicks}": got, **{f"{k2}_{n}_{kicks}": stats[k2] for k2 in KEYS},
                     **{f"{k2}_{n}_{kicks}": per[k2] for k2 in PER}})
    if 0 in opts.kicks:
        case["kicks_0_equals_parent"] = bool(np.array_equal(last[0][0], base) and last[0][1] == base_stats)
    out["cases"].append(case)
    keep.update({f"pts_{n}": pts64, f"start_{n}": tour0, f"cap_{n}": cap})
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
with open(opts.out, "w") as f:
    f.write(json.dumps(out) + "\n")
if opts.save_tours:
    os.makedirs(os.path.dirname(os.path.abspath(opts.save_tours)), exist_ok=True)
    np.savez(opts.save_tours, **keep)
