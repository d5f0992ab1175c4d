"""Graph preparation (``edge_index`` -> ``CsrGraph``) with ``method="host"`` (C helper + numpy, the default) against
``method="device"`` (``difusco_graph_build``), and the ``sampling`` stage of whole solves under ``graph_build="host"`` /
``"device"``.

    python scripts/bench_graph_build.py [--out-dir profiles/graph_build] [--only build_tsp10000_p1 ...] [--repeats 7]

Per workload both methods run in one process: one untimed pass of each, then ``--repeats`` timed passes with the methods
interleaved; every timed call starts after a device synchronise and ends in one.  Reported per method: median (min, max) in ms.
The answers are compared once per workload (``same_graph``; tests/test_gpu_graph_build.py pins the two methods to each other).

  build_*   the build alone, from an ``edge_index`` (and points) already on the device to the complete ``CsrGraph``:
            build_tsp10000_p1 / _p4   one TSP-10000, K = 100, 1 / 4 parallel samples (``build_csr``)
            build_tsp1000_x8          8 TSP-1000, K = 100 (``build_union_csr``)
            build_tsp500_x16          16 TSP-500, K = 50 (``build_union_csr``)
            build_er_x16              16 Erdos-Renyi graphs, n in 700..800, p = 0.15, MIS layout and node rows
  solve_*   ``solve_tsp_batch`` / ``solve_mis_batch`` with ``timings=`` on the same sets, synthetic weights (H 256, 12 layers,
            categorical), ``--steps`` inference steps: the ``sampling`` stage (where the build sits) and the whole call"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difusco_amd import MISModel, TSPModel  # noqa: E402
from difusco_amd.engine import DenoiseEngine  # noqa: E402
from difusco_amd.graph import GRAPH_BUILDS, build_csr, build_union_csr, knn_edge_index_gpu  # noqa: E402
from difusco_amd.pipeline import solve_mis_batch, solve_tsp_batch  # noqa: E402
from difusco_amd.synthetic import random_state_dict  # noqa: E402

TSP_SETS = {      # name: (instances, n, K, P)
    "tsp10000_p1": (1, 10000, 100, 1),
    "tsp10000_p4": (1, 10000, 100, 4),
    "tsp1000_x8": (8, 1000, 100, 1),
    "tsp500_x16": (16, 500, 50, 1),
}
ER_SET = ("er_x16", 16, 700, 800, 0.15)
FIELDS = ("rowptr", "col", "row", "perm", "node_order", "seg_ptr")


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def same_graph(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
            return False
    return a.n_segments == b.n_segments


def er_edge_index(n, p, rng):
    """The MIS dataset's layout: undirected edges, their reversed copies, one self loop per node."""
    iu = np.triu_indices(n, k=1)
    keep = rng.random(iu[0].shape[0]) < p
    e = np.stack([iu[0][keep], iu[1][keep]]).astype(np.int64)
    loops = np.arange(n, dtype=np.int64)
    return np.concatenate([e, e[::-1], np.stack([loops, loops])], axis=1)


def er_instances(rng):
    _, B, lo, hi, p = ER_SET
    ns = [int(n) for n in rng.integers(lo, hi + 1, size=B)]
    return [(n, er_edge_index(n, p, rng)) for n in ns]


def interleaved(fns, repeats, dev):
    """fns: {method: callable}.  -> ({method: first result}, {method: [ms, ...]})"""
    first = {m: fn() for m, fn in fns.items()}                   # one untimed pass of each
    ms = {m: [] for m in fns}
    for _ in range(repeats):
        for m, fn in fns.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ms[m].append(1e3 * (time.perf_counter() - t0))
    return first, ms


def run_build(name, args, dev):
    rng = np.random.default_rng(0)
    if name == ER_SET[0]:
        inst = er_instances(rng)
        eis = [torch.from_numpy(e).to(dev) for _, e in inst]
        ns = [n for n, _ in inst]
        fns = {m: (lambda m=m: build_union_csr(eis, ns, dev, task_rows="nodes", method=m)[0]) for m in GRAPH_BUILDS}
        shape = dict(instances=len(ns), n_nodes=sum(ns), n_edges=sum(int(e.shape[1]) for e in eis))
    else:
        B, n, k, P = TSP_SETS[name]
        pts = rng.random((B * n, 2))
        ei = knn_edge_index_gpu(pts, k, device=dev, graphs=B)
        pts32 = torch.from_numpy(pts.astype(np.float32)).to(dev)
        if B == 1:
            shift = torch.arange(P, device=dev).view(1, -1, 1) * n                     # duplicate_edge_index
            ei_rep = (ei.reshape(2, 1, -1) + shift).reshape(2, -1).contiguous()
            pts_rep = pts32.repeat(P, 1)
            fns = {m: (lambda m=m: build_csr(ei_rep, n * P, dev, points=pts_rep, method=m)) for m in GRAPH_BUILDS}
            shape = dict(instances=1, parallel_sampling=P, n_nodes=n * P, n_edges=int(ei_rep.shape[1]))
        else:
            eis = [(ei[:, b * n * k:(b + 1) * n * k] - b * n).contiguous() for b in range(B)]
            fns = {m: (lambda m=m: build_union_csr(eis, [n] * B, dev, points=pts32, method=m)[0]) for m in GRAPH_BUILDS}
            shape = dict(instances=B, n_nodes=B * n, n_edges=int(ei.shape[1]))
    first, ms = interleaved(fns, args.repeats, dev)
    rec = {"workload": "build_" + name, **shape, "repeats": args.repeats, "same_graph": same_graph(first["host"], first["device"]),
           "renumbered": first["host"].node_order is not None, "perm_identity": first["host"].perm is None,
           **{m: {"build_ms": spread(ms[m])} for m in GRAPH_BUILDS}}
    rec["host_over_device"] = round(rec["host"]["build_ms"]["median"] / rec["device"]["build_ms"]["median"], 3)
    return rec


def run_solve(name, args, dev, engine):
    margs = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, n_layers=12, hidden_dim=256,
                 inference_trick="ddim", inference_diffusion_steps=args.steps, inference_schedule="cosine")
    rng = np.random.default_rng(0)
    if name == ER_SET[0]:
        inst = er_instances(rng)
        B, P = len(inst), 1
        models = {m: MISModel(dict(margs, sparse_factor=-1), engine=engine, seed=1, graph_build=m) for m in GRAPH_BUILDS}

        def solve(m, t):
            return solve_mis_batch(models[m], inst, seeds=list(range(B)), generators=[torch.Generator().manual_seed(b) for b in range(B)],
                                   timings=t, step_offset=0)
        same = lambda a, b: all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))      # noqa: E731
    else:
        B, n, k, P = TSP_SETS[name]
        data = rng.random((B, n, 2))
        models = {m: TSPModel(dict(margs, sparse_factor=k), engine=engine, seed=1, graph_build=m) for m in GRAPH_BUILDS}

        def solve(m, t):
            return solve_tsp_batch(models[m], data, k, parallel_sampling=P, two_opt_iterations=args.two_opt, seeds=list(range(B)),
                                   generators=[torch.Generator().manual_seed(b) for b in range(B)], timings=t, step_offset=0)
        same = lambda a, b: all(x[0] == y[0] for x, y in zip(a, b))      # noqa: E731
    first = {m: solve(m, None) for m in GRAPH_BUILDS}            # one untimed pass of each
    torch.cuda.synchronize(dev)
    walls, stage = {m: [] for m in GRAPH_BUILDS}, {m: [] for m in GRAPH_BUILDS}
    for _ in range(args.repeats):
        for m in GRAPH_BUILDS:                                   # interleaved
            t = {}
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            solve(m, t)
            torch.cuda.synchronize(dev)
            walls[m].append(1e3 * (time.perf_counter() - t0))
            stage[m].append(1e3 * t["sampling"])
    rec = {"workload": "solve_" + name, "instances": B, "parallel_sampling": P, "inference_steps": args.steps,
           "two_opt_iterations": args.two_opt, "repeats": args.repeats, "same_result": same(first["host"], first["device"]),
           **{m: {"sampling_ms": spread(stage[m]), "wall_ms": spread(walls[m])} for m in GRAPH_BUILDS}}
    rec["sampling_host_minus_device_ms"] = round(rec["host"]["sampling_ms"]["median"] - rec["device"]["sampling_ms"]["median"], 3)
    return rec


def main():
    names = list(TSP_SETS) + [ER_SET[0]]
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", dest="out_dir", default=None)
    ap.add_argument("--only", nargs="*", default=["build_" + n for n in names] + ["solve_" + n for n in names])
    ap.add_argument("--steps", type=int, default=50, help="inference diffusion steps of the solve_* workloads")
    ap.add_argument("--two-opt", dest="two_opt", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph_build measures on the GPU: no device found")
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3")
    dev = torch.device("cuda:0")
    engine = None
    for full in args.only:
        kind, name = full.split("_", 1)
        if kind not in ("build", "solve") or name not in names:
            raise SystemExit(f"unknown workload {full}")
        if kind == "build":
            rec = run_build(name, args, dev)
        else:
            engine = engine or DenoiseEngine(random_state_dict(256, 12, 2, seed=0), device=dev)
            rec = run_solve(name, args, dev, engine)
        rec["device_name"] = torch.cuda.get_device_name(dev)
        print(json.dumps(rec), flush=True)
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, full + ".json"), "w") as f:
                json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
