#!/usr/bin/env python
"""Neighbour lists drawn from the heatmaps (``tsp_heat_candidate_lists``, ``difusco_tsp_heat_candidates_ragged``) on the GPU box,
in one process: what building them costs against the parent's lists, and what the neighbour-list searches - the parent's code,
untouched - do on them.  Shapes (``--shapes``), those of ``scripts/bench_kopt_search.py``:

    100x512     512 x TSP-100, one tour each          1000x64x4   64 x TSP-1000, four tours each
    500x10x4    10 x TSP-500, four tours each         1000x1      one TSP-1000 tour          10000x1    one TSP-10000 tour

Uniform points from ``np.random.default_rng``.  THE HEAT IS SYNTHETIC, the two kinds of ``bench_kopt_search.label_heat``
(``--heats``) on the k-NN graph with k = 10, self included: ``flip10`` labels the edges of a guide tour per instance (150 uniform
kicks of the iterated search on the GPU, Philox seed 12345) 1.0, every other entry 0.0, and flips 10 % of the labels, other flips
for every sample; ``noise`` is uniform random heat: it shows the cost of heat lists without their benefit.  No trained checkpoint
is available, so the lengths say nothing about heatmaps of a trained model.

1. List building (``build``), per shape and k in {10, 50, 100} (``noise`` heat, P samples; k capped at n), K = 8: the whole
   ``tsp_heat_candidate_lists`` call on device tensors (``heat_lists_ms``; it includes ``_heat_graph``, which checks and lays out
   every instance's graph with host synchronisations), the library call alone on the laid-out arrays (``heat_library_ms``), the
   parent's ``tsp_candidate_lists`` on the same ``edge_index`` (``knn_lists_ms``) and the k-NN call of ``_nbr_lists``,
   ``knn_edge_index_gpu`` with K + 1 neighbours, plus ``tsp_candidate_lists`` (``knn_own_call_ms``).
2. Search (``search``), per shape and heat kind: the start tours are the greedy merge of the heat (``merge_tours_batch``), as in
   the solvers.  ``nbr2opt+oropt`` (``batched_nbr_local_search_ragged``) and ``multi2opt`` with K > 0
   (``batched_nbr_two_opt_ragged``) on heat lists at K in {3, 4, 5, 8} and on distance lists at K in {8, 16}, closing ``full`` and
   ``none``; ``multi2opt+oropt`` (``batched_multi_local_search_ragged``) is the yardstick of the lengths.  The lists are built
   before the clock starts.  Reported: time to stop (median [min, max] of ``--repeats`` interleaved repeats after a warm-up of
   every method), sweeps, full sweeps, and the summed end length over ``multi2opt+oropt``'s.

``--no_gpu`` builds the inputs of every shape and stops: a rehearsal of the host side.  Writes
``profiles/heat_candidates/bench.json`` (``--out``).  No time or length printed here is a test."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"100x512": (100, 512, 1), "500x10x4": (500, 10, 4), "1000x64x4": (1000, 64, 4), "1000x1": (1000, 1, 1),
          "10000x1": (10000, 1, 1)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
ap.add_argument("--heats", nargs="+", default=["flip10", "noise"], choices=("flip10", "noise"))
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--cap", type=int, default=5000)
ap.add_argument("--skip_build", action="store_true", help="no list-building timings")
ap.add_argument("--skip_search", action="store_true", help="no search timings")
ap.add_argument("--no_gpu", action="store_true", help="build the inputs of every shape and stop: a rehearsal of the host side")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heat_candidates", "bench.json"))
opts = ap.parse_args()
K_GRAPH, BUILD_KS, BUILD_K, GUIDE_KICKS, GUIDE_SEED, KICK_SIZE, SPAN = 10, (10, 50, 100), 8, 150, 12345, 16, 30
HEAT_KS, KNN_KS = (3, 4, 5, 8), (8, 16)
LISTS = [f"heat{K}" for K in HEAT_KS] + [f"knn{K}" for K in KNN_KS]
METHODS = ["multi2opt+oropt"] + [f"{s}:{l}:{c}" for s in ("nbr2opt+oropt", "multi2opt") for l in LISTS for c in ("full", "none")]


def knn_edges(pts, k):
    """[2, n k] of the k nearest cities of every city, self included, rows in city order (numpy, in chunks of rows)."""
    n = len(pts)
    cols = np.empty((n, k), dtype=np.int64)
    for lo in range(0, n, 512):
        d = ((pts[lo:lo + 512, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
        part = np.argpartition(d, k - 1, axis=1)[:, :k] if k < n else np.broadcast_to(np.arange(n), d.shape).copy()
        order = np.argsort(np.take_along_axis(d, part, axis=1), axis=1, kind="stable")
        cols[lo:lo + 512] = np.take_along_axis(part, order, axis=1)
    return np.stack([np.repeat(np.arange(n), k), cols.reshape(-1)])


def strip_tour(pts, strips):
    """A closed tour through vertical strips, up one and down the next."""
    s = np.minimum((pts[:, 0] * strips).astype(np.int64), strips - 1)
    key = np.where(s % 2 == 0, pts[:, 1], -pts[:, 1])
    order = np.lexsort((key, s))
    return np.concatenate([order, order[:1]])


def label_heat(ei, guide, rng, kind):
    if kind == "noise":
        return rng.random(ei.shape[1]).astype(np.float32)
    n = len(guide) - 1
    nxt, prv = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    nxt[guide[:-1]], prv[guide[1:]] = guide[1:], guide[:-1]
    label = (nxt[ei[0]] == ei[1]) | (prv[ei[0]] == ei[1])
    return (label ^ (rng.random(ei.shape[1]) < 0.10)).astype(np.float32)


def inputs_of(name):
    n, G, P = SHAPES[name]
    rng = np.random.default_rng(n * 1000 + G)
    pts = [rng.random((n, 2)) for _ in range(G)]
    eis = [knn_edges(p, K_GRAPH) for p in pts]
    base = max(2, int(round(np.sqrt(n / 2))))
    starts = [strip_tour(p, base)[None] for p in pts]
    return n, G, P, pts, eis, starts, rng


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


if opts.no_gpu:
    for name in opts.shapes:
        n, G, P, pts, eis, starts, rng = inputs_of(name)
        heat = {kind: label_heat(eis[0], starts[0][0], rng, kind) for kind in opts.heats}
        wide = knn_edges(pts[0], min(n, BUILD_KS[-1]))
        assert sorted(starts[0][0][:-1].tolist()) == list(range(n)) and all(h.shape == (n * K_GRAPH,) for h in heat.values())
        assert wide.shape == (2, n * min(n, BUILD_KS[-1])) and np.all(wide[1].reshape(n, -1)[:, 0] == np.arange(n))
        print(json.dumps({"shape": name, "instances": G, "tours": G * P, "edges": int(eis[0].shape[1]), "methods": len(METHODS),
                          "heat_mean": {k: float(h.mean()) for k, h in heat.items()}}))
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd import _lib, decode  # noqa: E402
from difusco_amd.decode import (batched_iterated_search_ragged, batched_multi_local_search_ragged,  # noqa: E402
                                batched_nbr_local_search_ragged, batched_nbr_two_opt_ragged, merge_tours_batch, tsp_candidate_lists,
                                tsp_heat_candidate_lists)
from difusco_amd.graph import knn_edge_index_gpu  # noqa: E402

dev = torch.device("cuda:0")
out = {"metric": "time to stop / time to build", "unit": "ms", "data": "synthetic heat, no trained checkpoint", "repeats": opts.repeats,
       "cap": opts.cap, "graph_k": K_GRAPH, "build": [], "search": []}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), res


def library_call(pts, d_heat, d_ei, P, K):
    """The arrays ``tsp_heat_candidate_lists`` hands to the library, laid out once -> a function that makes the call alone."""
    G = len(pts)
    graph = decode._heat_graph("bench", pts, [decode._Samples(P)] * G, d_heat, d_ei, dev)
    group_edges, row_ptr, col, heat = graph
    group_n, group_tours = np.array([len(p) for p in pts], dtype=np.int32), np.full(G, P, dtype=np.int32)
    d_pts = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pts])).to(dev)
    lists = torch.empty(int(group_n.sum()) * K, dtype=torch.int32, device=dev)
    L = _lib.lib()
    sizes = (G, group_n.ctypes.data, group_tours.ctypes.data, group_edges.ctypes.data)
    nbytes = ctypes.c_size_t()
    _lib.check(L.difusco_tsp_heat_candidates_ragged_workspace_bytes(*sizes, K, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    listed, pads = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(keep=(group_n, group_tours, listed, pads)):         # the host arrays behind the pointers stay alive with the closure
        _lib.check(L.difusco_tsp_heat_candidates_ragged(*sizes, vp(d_pts), vp(row_ptr), vp(col), vp(heat), K, vp(lists), vp(ws),
                                                        nbytes.value, listed.ctypes.data, pads.ctypes.data, None))
        return graph, d_pts, lists
    return call, nbytes.value


for name in opts.shapes:
    n, G, P, pts, eis, starts, rng = inputs_of(name)
    sizes = [n] * G
    if not opts.skip_build:
        for k in BUILD_KS:
            k = min(k, n)
            wide = [knn_edges(p, k) for p in pts]
            d_ei = [torch.from_numpy(e).to(dev) for e in wide]
            d_heat = [torch.from_numpy(rng.random((P, e.shape[1])).astype(np.float32)).to(dev) for e in wide]
            call, ws_bytes = library_call(pts, d_heat, d_ei, P, BUILD_K)
            all_pts = np.concatenate(pts)
            ways = {"heat_lists_ms": lambda: tsp_heat_candidate_lists(pts, d_heat, d_ei, BUILD_K, device=dev),
                    "heat_library_ms": call,
                    "knn_lists_ms": lambda: tsp_candidate_lists(d_ei, sizes, BUILD_K),
                    "knn_own_call_ms": lambda: tsp_candidate_lists(knn_edge_index_gpu(all_pts, BUILD_K + 1, device=dev, sizes=sizes),
                                                                   sizes, BUILD_K)}
            for fn in ways.values():
                fn()                                                                           # warm-up
            ms = {w: [] for w in ways}
            for _ in range(opts.repeats):                                                      # interleaved: same clocks for all
                for w, fn in ways.items():
                    ms[w].append(timed(fn)[0])
            case = {"shape": name, "workload": f"{G} x TSP-{n}, {P} sample(s) each", "k": k, "K": BUILD_K,
                    "entries": int(sum(e.shape[1] for e in wide)), "workspace_bytes": ws_bytes, **{w: spread(v) for w, v in ms.items()}}
            print(json.dumps(case), flush=True)
            out["build"].append(case)
    if opts.skip_search:
        continue
    d_ei = [torch.from_numpy(e).to(dev) for e in eis]
    guides, _ = batched_iterated_search_ragged(pts, starts, opts.cap, device=dev, kicks=GUIDE_KICKS, kick_size=KICK_SIZE, span=SPAN,
                                               seeds=[GUIDE_SEED] * G, offsets=[0] * G)
    ei17 = knn_edge_index_gpu(np.concatenate(pts), max(KNN_KS) + 1, device=dev, sizes=sizes)
    length = lambda tours: float(sum(np.linalg.norm(p[t[:, :-1]] - p[t[:, 1:]], axis=2).sum() for p, t in zip(pts, tours)))
    for kind in opts.heats:
        heat = [np.stack([label_heat(eis[g], guides[g][0], rng, kind) for _ in range(P)]) for g in range(G)]
        d_heat = [torch.from_numpy(h).to(dev) for h in heat]
        merged = merge_tours_batch([h.reshape(-1) for h in d_heat], [p.astype(np.float32) for p in pts], d_ei, sparse_graph=True,
                                   parallel_sampling=P, device=dev)
        tours0 = [np.asarray(t, dtype=np.int64) for t, _ in merged]
        lists, share = {}, {}
        for K in HEAT_KS:
            st = {}
            lists[f"heat{K}"] = tsp_heat_candidate_lists(pts, d_heat, d_ei, K, device=dev, stats=st)
            share[f"heat{K}"] = {"listed": float(st["listed"].sum() / (G * n * K)), "pads": float(st["pads"].sum() / (G * n * K))}
        for K in KNN_KS:
            lists[f"knn{K}"] = tsp_candidate_lists(ei17, sizes, K)

        def run(m, cap=opts.cap):
            if m == "multi2opt+oropt":
                return batched_multi_local_search_ragged(pts, tours0, cap, device=dev)
            search, which, closing = m.split(":")
            if search == "nbr2opt+oropt":
                return batched_nbr_local_search_ragged(pts, tours0, cap, device=dev, neighbors=lists[which], closing=closing == "full")
            st = {}
            tours, _ = batched_nbr_two_opt_ragged(pts, tours0, cap, device=dev, neighbors=lists[which], closing=closing == "full", stats=st)
            return tours, st
        for m in METHODS:
            run(m, 3)                                                                          # warm-up
        ms, last = {m: [] for m in METHODS}, {}
        for _ in range(opts.repeats):                                                          # interleaved: same clocks for all
            for m in METHODS:
                t, last[m] = timed(lambda: run(m))
                ms[m].append(t)
        base_len = length(last["multi2opt+oropt"][0])
        case = {"shape": name, "heat": kind, "workload": f"{G} x TSP-{n}, {P} tour(s) each, merged start tours, graph k = {K_GRAPH}",
                "tour_length_start": length(tours0), "tour_length_multi2opt_oropt": base_len, "heat_lists": share, "methods": {}}
        for m in METHODS:
            tours, st = last[m]
            sweeps = st["two_opt_sweeps"] + st["or_opt_sweeps"] if "two_opt_sweeps" in st else st["sweeps"]
            case["methods"][m] = {"ms": spread(ms[m]), "sweeps_mean": float(np.mean(sweeps)), "sweeps_max": int(np.max(sweeps)),
                                  "full_sweeps_mean": float(np.mean(st["full_sweeps"])) if "full_sweeps" in st else 0.0,
                                  "length_over_multi2opt_oropt": length(tours) / base_len}
        for s in ("nbr2opt+oropt", "multi2opt"):                 # heat lists against the best distance setting of the same run
            for c in ("full", "none"):
                knn_best = min((f"{s}:knn{K}:{c}" for K in KNN_KS), key=lambda m: np.median(ms[m]))
                for K in HEAT_KS:
                    m = f"{s}:heat{K}:{c}"
                    case["methods"][m].update(
                        best_knn=knn_best, best_knn_over_this=float(np.median(ms[knn_best]) / np.median(ms[m])),
                        faster_beyond_the_spread=bool(max(ms[m]) < min(ms[knn_best])),
                        slower_beyond_the_spread=bool(min(ms[m]) > max(ms[knn_best])),
                        length_over_best_knn=case["methods"][m]["length_over_multi2opt_oropt"] /
                        case["methods"][knn_best]["length_over_multi2opt_oropt"])
        print(json.dumps(case), flush=True)
        out["search"].append(case)
doc = {}
if os.path.exists(opts.out):
    with open(opts.out) as f:
        doc = json.load(f)
for key in ("build", "search"):                                  # a run of some shapes keeps the cases of the others
    mine = {(c["shape"], c.get("k"), c.get("heat")) for c in out[key]}
    out[key] = [c for c in doc.get(key, []) if (c["shape"], c.get("k"), c.get("heat")) not in mine] + out[key]
os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
with open(opts.out, "w") as f:
    f.write(json.dumps(out) + "\n")
