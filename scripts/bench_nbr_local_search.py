#!/usr/bin/env python
"""Neighbour-list multi-move 2-opt + Or-opt search timing on the GPU box: ``batched_multi_local_search_ragged`` (the code of the
parent commit, unchanged) against ``batched_nbr_local_search_ragged`` with ``candidates`` in {5, 8, 16}, closing on and off, from
the decoded start tours of ``scripts/bench_decode.py`` (synthetic heat - no trained checkpoint, so the lengths say nothing about
solution quality on real heatmaps).  Shapes (``--shapes``), those of ``scripts/bench_nbr_two_opt.py``: ``n1000`` one tour of
TSP-1000, ``n10000`` one tour of TSP-10000, ``b64x1000x4`` 64 instances of TSP-1000 with 4 tours each, ``b10x500x4``,
``b512x100x1``.  Writes ``profiles/nbr_local_search/bench.json`` (``--out``).

Timed run (the default): one process, a warm-up of each method, ``--repeats`` interleaved repeats, median [min, max] of the time
to stop of the whole call (upload, search, download); the seven counters and the summed end length of every method, the length
against ``multi2opt+oropt``'s.  The lists are the first K of the 16 nearest other cities of one ``knn_edge_index_gpu`` call per
shape, made before the clock starts (the solvers take them from the instance's graph); its time is reported as ``knn16_ms``.
``--save_tours PATH`` keeps the start tours, the lists and every method's result (npz).

Three more modes, all separate from the timed run:
  --profile_pass        per shape one search with ``candidates`` = 8, closing on, after a warm-up, and nothing else: the program
                        to put behind ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME --``;
  --kernel_stats CSV    no GPU: reads that run's ``*_kernel_stats.csv`` and adds the per-launch averages of the six kernels to
                        ``--out`` under ``kernel_stats_<shapes>`` (the profiled run holds the warm-up's launches too);
  --verify NPZ          no GPU: runs tests/nbr_local_search_emulation.py from the saved start tours and lists - every method of
                        every shape of ``--shapes`` (``--methods``: only these), the first ``--verify_groups`` instances of a
                        batch (an instance of a call is a search of its own) - and adds to ``--out`` whether the seven counters
                        and the tours equal the GPU's."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"n1000": (1, 1000, 1, 200), "n10000": (1, 10000, 1, 5000), "b64x1000x4": (64, 1000, 4, 1000),
          "b10x500x4": (10, 500, 4, 1000), "b512x100x1": (512, 100, 1, 1000)}      # instances, N, tours each, cap
KS = [5, 8, 16]
METHODS = ["multi2opt+oropt"] + [f"k{K}_{c}" for K in KS for c in ("closing", "open")]

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
ap.add_argument("--select_rounds", type=int, default=4)
ap.add_argument("--max_rounds", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbr_local_search", "bench.json"))
ap.add_argument("--save_tours", default=None)
ap.add_argument("--profile_pass", action="store_true")
ap.add_argument("--kernel_stats", default=None)
ap.add_argument("--verify", default=None)
ap.add_argument("--verify_groups", type=int, default=2)
ap.add_argument("--methods", nargs="+", default=METHODS, choices=METHODS, help="--verify: the methods to check (default: all)")
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


def method_args(m):
    K, c = m[1:].split("_")
    return int(K), c == "closing"


if opts.kernel_stats:
    rows = {}
    with open(opts.kernel_stats) as f:
        for r in csv.DictReader(f):
            for name in ("nls_prep_kernel", "nls_row_value_kernel", "nls_row_col_kernel", "nls_full_two_kernel", "nls_full_or_kernel",
                         "mls_select_listed_kernel"):
                if name in r["Name"]:
                    rows[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                                  "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                  "max_us": float(r["MaxNs"]) / 1e3}
    update_out("kernel_stats_" + "_".join(opts.shapes),
               {"source": "rocprofv3 --kernel-trace --stats of --profile_pass (candidates 8, closing on), its own run",
                "shapes": opts.shapes, "kernels": rows})
    sys.exit(0)

if opts.verify:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multi_local_search_emulation as M
    import nbr_local_search_emulation as NL
    saved = np.load(opts.verify)
    res = []
    for shape in opts.shapes:
        G, n, P, cap = SHAPES[shape]
        groups = min(G, opts.verify_groups)
        pts, start, lists = saved[f"pts_{shape}"], saved[f"start_{shape}"], saved[f"lists_{shape}"]
        for m in opts.methods:
            t0 = time.perf_counter()
            ok = True
            for g in range(groups):
                s = start[g * P:(g + 1) * P]
                if m == "multi2opt+oropt":
                    tours, want = M.multi_local_search(pts[g], s, cap, opts.max_rounds, opts.select_rounds)
                    want.update(full_sweeps=0, full_rounds=0)
                else:
                    K, closing = method_args(m)
                    tours, want = NL.nbr_local_search(pts[g], s, lists[g][:, :K], closing, cap, opts.max_rounds, opts.select_rounds)
                got = {k: int(saved[f"{k}_{shape}_{m}"][g]) for k in NL.COUNTERS}
                ok = ok and np.array_equal(tours, saved[f"tours_{shape}_{m}"][g * P:(g + 1) * P]) and got == want
            res.append({"shape": shape, "method": m, "groups_checked": groups, "equal": bool(ok),
                        "emulation_s": time.perf_counter() - t0})
            print(json.dumps(res[-1]), flush=True)
            assert ok, res[-1]
    update_out("emulation_" + "_".join(opts.shapes) + ("" if opts.methods == METHODS else "_" + "_".join(opts.methods)), res)
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd.decode import (batched_multi_local_search_ragged, batched_nbr_local_search_ragged, merge_tours_batch,  # noqa: E402
                                tsp_candidate_lists)
from difusco_amd.graph import knn_edge_index_gpu  # noqa: E402
from difusco_amd.synthetic import tsp_instance  # noqa: E402

dev = torch.device("cuda:0")
out = {"metric": "time to stop of one call", "unit": "ms", "data": "synthetic heat, no trained checkpoint", "repeats": opts.repeats,
       "select_rounds": opts.select_rounds, "max_rounds": opts.max_rounds, "cases": []}
keep = {}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def spread(ms):
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "all": ms}


for shape in opts.shapes:
    G, n, P, cap = SHAPES[shape]
    k = min(100, n // 2)
    pts_l, ei_l, heat_l = [], [], []
    for g in range(G):
        pts, ei = tsp_instance(n, k, seed=11 + g)
        rng = np.random.default_rng(n + g)
        d = np.linalg.norm(pts[ei[0]] - pts[ei[1]], axis=1)
        heat = np.stack([(np.exp(-d / (0.5 * d.mean())) * rng.random(ei.shape[1])).astype(np.float32) + np.float32(1e-6)
                         for _ in range(P)])
        pts_l.append(pts)
        ei_l.append(ei)
        heat_l.append(heat.reshape(-1))
    merged = merge_tours_batch(heat_l, pts_l, ei_l, sparse_graph=True, parallel_sampling=P, device=dev)
    tours0 = [np.asarray(t, dtype=np.int64) for t, _ in merged]
    pts64 = [p.astype(np.float64) for p in pts_l]
    length = lambda tours: float(sum(np.linalg.norm(p[t[:, :-1]] - p[t[:, 1:]], axis=2).sum() for p, t in zip(pts64, tours)))
    t_knn, ei16 = timed(lambda: (knn_edge_index_gpu(np.concatenate(pts64), 17, device=dev, sizes=[n] * G), torch.cuda.synchronize())[0])
    lists = {K: tsp_candidate_lists(ei16, [n] * G, K) for K in KS}

    def run(m, c=cap):
        kw = dict(max_iterations=c, device=dev, max_rounds=opts.max_rounds, select_rounds=opts.select_rounds)
        if m == "multi2opt+oropt":
            return batched_multi_local_search_ragged(pts64, tours0, **kw)
        K, closing = method_args(m)
        return batched_nbr_local_search_ragged(pts64, tours0, neighbors=lists[K], closing=closing, **kw)
    if opts.profile_pass:
        run("k8_closing", 3)
        run("k8_closing")
        continue
    for m in METHODS:
        run(m, 3)                                                                              # warm-up
    ms = {m: [] for m in METHODS}
    last = {}
    for _ in range(opts.repeats):                                                              # interleaved: same clocks for all
        for m in METHODS:
            t, (tours, stats) = timed(lambda: run(m))
            ms[m].append(t)
            stats = dict(stats)
            stats.setdefault("full_sweeps", np.zeros(G, dtype=np.int64))
            stats.setdefault("full_rounds", np.zeros(G, dtype=np.int32))
            last[m] = (tours, stats)
    base = "multi2opt+oropt"
    base_len = length(last[base][0])
    case = {"shape": shape, "workload": f"{G} x TSP-{n} x {P} tours, decoded start tours", "cap": cap, "knn16_ms": t_knn,
            "tour_length_start": length(tours0), "methods": {}}
    for m in METHODS:
        tours, st = last[m]
        sweeps = st["two_opt_sweeps"] + st["or_opt_sweeps"]          # an upper bound of a tour's own sum: the maxima of two kinds
        case["methods"][m] = {"ms": spread(ms[m]), "two_opt_sweeps_mean": float(st["two_opt_sweeps"].mean()),
                              "or_opt_sweeps_mean": float(st["or_opt_sweeps"].mean()), "two_opt_sweeps_max": int(st["two_opt_sweeps"].max()),
                              "or_opt_sweeps_max": int(st["or_opt_sweeps"].max()), "rounds_mean": float(st["rounds"].mean()),
                              "rounds_max": int(st["rounds"].max()), "full_sweeps_mean": float(st["full_sweeps"].mean()),
                              "full_sweeps_max": int(st["full_sweeps"].max()), "full_rounds_max": int(st["full_rounds"].max()),
                              "moves": int(st["two_opt_moves"].sum() + st["or_opt_moves"].sum()),
                              "stopped_by_cap": bool((sweeps >= cap).any()), "tour_length_after": length(tours),
                              "length_over_multi2opt_oropt": length(tours) / base_len,
                              "multi2opt_oropt_over_this": float(np.median(ms[base]) / np.median(ms[m])),
                              "faster_beyond_the_spread": bool(max(ms[m]) < min(ms[base])),
                              "slower_beyond_the_spread": bool(min(ms[m]) > max(ms[base]))}
        keep.update({f"tours_{shape}_{m}": np.concatenate(tours)})
        keep.update({f"{k}_{shape}_{m}": st[k] for k in st})
    out["cases"].append(case)
    print(json.dumps(case), flush=True)
    keep.update({f"pts_{shape}": np.stack(pts64), f"start_{shape}": np.concatenate(tours0),
                 f"lists_{shape}": np.stack([t.cpu().numpy() for t in lists[16]])})
if not opts.profile_pass:
    doc = {}
    if os.path.exists(opts.out):
        with open(opts.out) as f:
            doc = json.load(f)
    doc.update(out)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(doc) + "\n")
    if opts.save_tours:
        os.makedirs(os.path.dirname(os.path.abspath(opts.save_tours)), exist_ok=True)
        np.savez(opts.save_tours, **keep)
