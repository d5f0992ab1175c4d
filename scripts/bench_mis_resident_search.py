#!/usr/bin/env python
"""Resident against launched iterated MIS swap search on the GPU box: ``mis_iterated_search_np`` with ``mode="resident"``
(``difusco_mis_resident_search``: one block per instance, one host synchronisation per call) beside ``mode="launches"``
(``difusco_mis_iterated_search``, the code of the parent commit unchanged) at kicks in {0, 10, 100, 1000}, on the union of
``bench_mis_iterated_search.py``: 16 Erdos-Renyi graphs G(n, 0.15), n ~ U{700..800} (the graphs of ``bench.py``), as P = 1 and
P = 4 copies, every copy its own row of the instance table (key 1000 + graph, offset ``2^62 + p 2^32``).  Prints one JSON line
(``--out PATH`` also writes it).

The scores are SYNTHETIC (uniform random per node and copy, not a trained checkpoint's heatmap).  The two modes return the same
sets by construction, so the sizes say nothing about either mode; ``--verify`` asserts that the sets, the call counters and the
per-instance counters of the two modes are equal for every variant.

One process; after a warm-up of every variant, ``--repeats`` rounds in each of which every variant runs once, in turn (same
clocks for all); median [min, max].  All start from the decoded set and include the copy of the 0/1 array to the host.
``ms_per_kick``: (t(kicks) - t(0)) / kicks of the same mode within one round, then median [min, max] over the rounds.
``resident_below_launched``: the resident maximum of ``ms_per_kick`` is below the launched minimum."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difusco_amd import _lib  # noqa: E402
from difusco_amd.decode import MIS_KICK_OFFSET, MIS_SEARCH_MODES, mis_decode_np, mis_iterated_search_np  # noqa: E402
from difusco_amd.graph import build_csr  # noqa: E402
from difusco_amd.synthetic import er_mis_edge_index  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--graphs", type=int, default=16)
ap.add_argument("--parallel", nargs="+", type=int, default=[1, 4])
ap.add_argument("--kicks", nargs="+", type=int, default=[0, 10, 100, 1000])
ap.add_argument("--kick_size", type=int, default=4)
ap.add_argument("--max_rounds", type=int, default=1000)
ap.add_argument("--kicks_per_launch", type=int, default=0, help="of the resident mode (0: the library's default)")
ap.add_argument("--verify", action="store_true", help="assert that the two modes returned equal sets and counters")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
opts = ap.parse_args()
assert 0 in opts.kicks, "the time per kick is measured against kicks = 0"

dev = torch.device("cuda:0")
out = {"metric": "ms per call on the union", "unit": "ms", "box": "one MI355X (gfx950)", "data": "synthetic",
       "scores": "uniform random per node and copy (synthetic: not a trained checkpoint's heatmap); the two modes return equal "
                 "sets by construction", "repeats": opts.repeats, "kick_size": opts.kick_size,
       "resident_max_nodes": int(_lib.lib().difusco_mis_resident_max_nodes()), "kicks_per_launch": opts.kicks_per_launch,
       "launches": "difusco_mis_iterated_search, the code of the parent commit unchanged", "verified": bool(opts.verify),
       "cases": []}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), res


def spread(ms):
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "all": list(ms)}


sizes = [int(np.random.default_rng(5000 + g).integers(700, 801)) for g in range(opts.graphs)]      # bench.py's graphs
graphs = [torch.from_numpy(er_mis_edge_index(n, 0.15, seed=1000 + g)) for g, n in enumerate(sizes)]
COUNTERS = ("rounds", "swaps", "inserts", "entered", "accepted", "size_before", "size_after")

for P in opts.parallel:
    ns = [n for n in sizes for _ in range(P)]                  # the copies of a graph are instances of their own
    off = np.concatenate([[0], np.cumsum(ns)])
    ei = torch.cat([graphs[c // P] + int(off[c]) for c in range(len(ns))], dim=1).to(dev)
    N = int(off[-1])
    graph = build_csr(ei, N, dev)
    scores = torch.from_numpy(np.random.default_rng(P).random(N).astype(np.float32)).to(dev)
    decoded = mis_decode_np(scores, graph=graph, device=dev)
    table = dict(instance_rows=off.tolist(), seeds=[1000 + c // P for c in range(len(ns))],
                 offsets=[MIS_KICK_OFFSET + ((c % P) << 32) for c in range(len(ns))])
    stats = {(mode, k): {} for mode in MIS_SEARCH_MODES for k in opts.kicks}

    def search(mode, k):
        more = dict(kicks_per_launch=opts.kicks_per_launch) if mode == "resident" else {}
        return lambda: mis_iterated_search_np(scores, decoded, graph=graph, device=dev, max_rounds=opts.max_rounds, kicks=k,
                                              kick_size=opts.kick_size, stats=stats[mode, k], mode=mode, **more, **table)

    variants = [((mode, k), search(mode, k)) for k in opts.kicks for mode in MIS_SEARCH_MODES]
    ms, sols = {name: [] for name, _ in variants}, {}
    for _, fn in variants:                                     # warm-up of every variant
        fn()
    for _ in range(opts.repeats):                              # interleaved: same clocks for all
        for name, fn in variants:
            t, sols[name] = timed(fn)
            ms[name].append(t)
    per = lambda sol: [int(sol[off[c]:off[c + 1]].sum()) for c in range(len(ns))]
    case = {"workload": f"{opts.graphs} x G(700..800, 0.15), P = {P}: one union", "parallel_sampling": P, "nodes": N,
            "instances": len(ns), "csr_entries": int(graph.col.shape[0]), "max_rounds": opts.max_rounds,
            "size_decoded_mean": float(np.mean(per(decoded))), "kicks": []}
    for k in opts.kicks:
        if opts.verify:
            assert np.array_equal(sols["launches", k], sols["resident", k]), (P, k)
            for key in COUNTERS:
                assert stats["launches", k][key] == stats["resident", k][key], (P, k, key)
        row = {"kicks": k, "size_mean": float(np.mean(per(sols["resident", k]))),
               "rounds": stats["resident", k]["rounds"], "swaps": stats["resident", k]["swaps"],
               "inserts": stats["resident", k]["inserts"],
               "equal_sets": bool(np.array_equal(sols["launches", k], sols["resident", k]))}
        for mode in MIS_SEARCH_MODES:
            row[mode] = {"ms": spread(ms[mode, k]), "host_syncs": stats[mode, k]["host_syncs"],
                         "size_mean": float(np.mean(per(sols[mode, k])))}
            if k:
                row[mode]["ms_per_kick"] = spread([(a - b) / k for a, b in zip(ms[mode, k], ms[mode, 0])])
        row["launches_over_resident"] = row["launches"]["ms"]["median"] / row["resident"]["ms"]["median"]
        if k:
            row["per_kick_launches_over_resident"] = (row["launches"]["ms_per_kick"]["median"] /
                                                      row["resident"]["ms_per_kick"]["median"])
            row["resident_below_launched"] = row["resident"]["ms_per_kick"]["max"] < row["launches"]["ms_per_kick"]["min"]
        case["kicks"].append(row)
    out["cases"].append(case)
print(json.dumps(out))
if opts.out:
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(json.dumps(out) + "\n")
