#!/usr/bin/env python
"""The heatmap-guided sampled k-opt search (``batched_kopt_search_ragged``, ``difusco_tsp_kopt_search_ragged``) timed on the GPU
box against what the parent's best search, ``multi2opt+oropt`` iterated with uniform kicks (``batched_iterated_search_ragged``,
which this feature does not touch), gains in the same wall time, in one process.  Shapes (``--shapes``):

    100x512     512 x TSP-100, one tour each          1000x64x4   64 x TSP-1000, four tours each
    500x10x4    10 x TSP-500, four tours each         1000x1      one TSP-1000 tour          10000x1    one TSP-10000 tour

Uniform points from ``np.random.default_rng``; the candidate graph is the k-NN graph with K = 10, self included.  THE HEAT IS
SYNTHETIC, that of ``scripts/tsp_heat_kick_table.py``: a guide tour per instance (here 150 uniform kicks of the iterated search on
the GPU, Philox seed 12345) labels its edges 1.0, every other entry 0.0, and 10 % of the labels are flipped (``flip10``), with
other flips for every tour; ``--heat noise`` takes uniform random heat instead.  No trained checkpoint is available, so the
lengths say nothing about heatmaps of a trained model.  Every tour starts from its own ``multi2opt+oropt`` result (from a strip
tour, another strip count per tour of an instance).

Per shape: a warm-up of both searches, then ``--repeats`` interleaved repeats of (the k-opt search at ``--rounds`` rounds, the
k-opt search at 0 rounds, the kicked search at the probe kick count, the kicked search at 0 kicks) - host clock around calls that
end in a device synchronisation.  ms per round = (median time at R rounds - median at 0 rounds) / rounds enqueued (the rounds of
the slowest tour, rounded up to the poll interval 8, at most R).  From the probe, ms per kick; the kicked search is then run at
the kick count that fits the k-opt search's median time and its gain at that time is reported next to the k-opt search's, both
as the mean over the tours of (first length - final length) / first length.  Writes ``profiles/kopt_search/bench.json`` (``--out``).

No time or length printed here is a test."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"100x512": (100, 512, 1), "1000x64x4": (1000, 64, 4), "500x10x4": (500, 10, 4), "1000x1": (1000, 1, 1),
          "10000x1": (10000, 1, 1)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rounds", type=int, default=64)
ap.add_argument("--samples", type=int, default=1024)
ap.add_argument("--depth", type=int, default=10)
ap.add_argument("--probe_kicks", type=int, default=8)
ap.add_argument("--heat", default="flip10", choices=("flip10", "noise"))
ap.add_argument("--cap", type=int, default=5000)
ap.add_argument("--no_gpu", action="store_true", help="build the inputs of every shape and stop: a rehearsal of the host side")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kopt_search", "bench.json"))
opts = ap.parse_args()
K, GUIDE_KICKS, GUIDE_SEED, KICK_SIZE, SPAN = 10, 150, 12345, 16, 30


def knn_edges(pts, k):
    """[2, n k] of the k nearest cities of every city, self included, rows in city order (numpy, in chunks of rows)."""
    n = len(pts)
    cols = np.empty((n, k), dtype=np.int64)
    for lo in range(0, n, 512):
        d = ((pts[lo:lo + 512, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
        part = np.argpartition(d, k - 1, axis=1)[:, :k]
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
    eis = [knn_edges(p, K) for p in pts]
    base = max(2, int(round(np.sqrt(n / 2))))
    starts = [np.stack([strip_tour(p, base + q) for q in range(P)]) for p in pts]
    return n, G, P, pts, eis, starts, rng


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


if opts.no_gpu:
    for name in opts.shapes:
        n, G, P, pts, eis, starts, rng = inputs_of(name)
        heat = label_heat(eis[0], starts[0][0], rng, opts.heat)
        assert all(sorted(t[:-1].tolist()) == list(range(n)) for t in starts[0]) and heat.shape == (n * K,)
        print(json.dumps({"shape": name, "instances": G, "tours": G * P, "edges": int(eis[0].shape[1]), "heat_mean": float(heat.mean())}))
    sys.exit(0)

import torch  # noqa: E402

from difusco_amd.decode import (batched_iterated_search_ragged, batched_kopt_search_ragged,  # noqa: E402
                                batched_multi_local_search_ragged)

dev = torch.device("cuda:0")
out = {"metric": "time to stop", "unit": "ms", "data": f"synthetic heat ({opts.heat}), no trained checkpoint", "repeats": opts.repeats,
       "rounds": opts.rounds, "samples": opts.samples, "depth": opts.depth, "patience": 10, "alpha": 1.0, "beta": 10.0,
       "parent": "batched_iterated_search_ragged, uniform kicks, full descent, kick_size 16, span 30", "cases": []}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), res


def gain(per):
    return float(np.mean((per["first_length"] - per["final_length"]) / per["first_length"]))


for name in opts.shapes:
    n, G, P, pts, eis, starts, rng = inputs_of(name)
    T = G * P
    keys = dict(seeds=list(range(T)), offsets=[0] * T)
    guides, _ = batched_iterated_search_ragged(pts, [s[:1] for s in starts], opts.cap, device=dev, kicks=GUIDE_KICKS, kick_size=KICK_SIZE,
                                               span=SPAN, seeds=[GUIDE_SEED] * G, offsets=[0] * G)
    heat = [np.stack([label_heat(eis[g], guides[g][0], rng, opts.heat) for _ in range(P)]) for g in range(G)]
    d_heat, d_ei = [torch.from_numpy(h).to(dev) for h in heat], [torch.from_numpy(e).to(dev) for e in eis]
    descended, _ = batched_multi_local_search_ragged(pts, starts, opts.cap, device=dev)

    def kopt(rounds, per):
        return batched_kopt_search_ragged(pts, descended, heat=d_heat, edge_index=d_ei, samples=opts.samples, depth=opts.depth,
                                          rounds=rounds, stats=per, device=dev, **keys)

    def kicked(kicks, per):
        return batched_iterated_search_ragged(pts, descended, opts.cap, device=dev, kicks=kicks, kick_size=KICK_SIZE, span=SPAN,
                                              stats=per, **keys)

    kopt(2, {}), kicked(2, {})                                                                 # warm-up
    ms = {k: [] for k in ("kopt", "kopt0", "probe", "kick0")}
    per_kopt, per_probe = {}, {}
    for _ in range(opts.repeats):                                                              # interleaved: same clocks for all
        per_kopt, per_probe = {}, {}
        ms["kopt"].append(timed(lambda: kopt(opts.rounds, per_kopt))[0])
        ms["kopt0"].append(timed(lambda: kopt(0, {}))[0])
        ms["probe"].append(timed(lambda: kicked(opts.probe_kicks, per_probe))[0])
        ms["kick0"].append(timed(lambda: kicked(0, {}))[0])
    slowest = int(per_kopt["rounds"].max())
    enqueued = min(opts.rounds, -(-slowest // 8) * 8)
    ms_per_round = (np.median(ms["kopt"]) - np.median(ms["kopt0"])) / max(enqueued, 1)
    ms_per_kick = max((np.median(ms["probe"]) - np.median(ms["kick0"])) / opts.probe_kicks, 1e-3)
    fit = int(max(0, (np.median(ms["kopt"]) - np.median(ms["kick0"])) / ms_per_kick))
    per_fit, ms_fit = {}, []
    for _ in range(opts.repeats):
        per_fit = {}
        ms_fit.append(timed(lambda: kicked(fit, per_fit))[0])
    case = {"workload": f"{G} x TSP-{n}, {P} tour(s) each, K = {K}", "tours": T,
            "start": "multi2opt+oropt of strip tours", "mean_start_length": float(per_kopt["first_length"].mean()),
            "kopt": {"ms": spread(ms["kopt"]), "ms_at_0_rounds": spread(ms["kopt0"]), "rounds_enqueued": enqueued,
                     "ms_per_round": float(ms_per_round), "rounds_to_stop": {"max": slowest, "mean": float(per_kopt["rounds"].mean()),
                                                                              "min": int(per_kopt["rounds"].min())},
                     "tours_stopped_by_stall": int((per_kopt["rounds"] < opts.rounds).sum()),
                     "actions": {"sum": int(per_kopt["actions"].sum()), "mean": float(per_kopt["actions"].mean())},
                     "mean_depth": float(per_kopt["depth_sum"].sum() / max(1, per_kopt["actions"].sum())),
                     "reverted": int(per_kopt["reverted"].sum()), "gain": gain(per_kopt), "host_syncs": per_kopt["host_syncs"]},
            "kicked": {"ms_at_0_kicks": spread(ms["kick0"]), "probe_kicks": opts.probe_kicks, "ms_at_probe": spread(ms["probe"]),
                       "ms_per_kick": float(ms_per_kick), "gain_at_probe": gain(per_probe), "kicks_that_fit": fit,
                       "ms_at_fit": spread(ms_fit), "gain_at_fit": gain(per_fit)}}
    case["kopt_gain_minus_kicked_gain"] = case["kopt"]["gain"] - case["kicked"]["gain_at_fit"]
    print(json.dumps(case), flush=True)
    out["cases"].append(case)
os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
with open(opts.out, "w") as f:
    f.write(json.dumps(out) + "\n")
