"""Per-instance sampling latency of one instance per call: the eager loop of ``sample()`` against ``sample(..., graphed=True)``
(the whole loop replayed as one captured HIP graph).

    python scripts/bench_latency.py [--out profiles/r07/latency_graphed.json] [--only tsp50_dense_p1 ...] [--instances 20]
                                    [--mode both|eager|graphed]

Synthetic weights (H 256, 12 layers, categorical, 50 cosine steps) and synthetic instances.  Twin models (same weights and seed,
separate engines) take the same instances in the same order, eager and graphed alternating in one process, so their call
counters stay equal and their outputs must be bitwise equal; the JSON records that comparison for every instance.  The clock
is the host clock around one call with the device synchronised before and after; the graphed model's first call of a shape
(warm-up run + capture) is reported as ``capture_ms`` and kept out of the percentiles, as is one eager warm-up call.
``--mode eager`` / ``graphed`` runs one side only (for a kernel trace of it)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difusco_amd import MISModel, TSPModel  # noqa: E402
from difusco_amd.graph import knn_edge_index_gpu  # noqa: E402
from difusco_amd.synthetic import er_mis_edge_index, random_state_dict  # noqa: E402

WORKLOADS = {      # name: (task, n, sparse_factor, parallel_sampling, sequential_sampling)
    "tsp50_dense_p1": ("tsp", 50, -1, 1, 1),
    "tsp50_dense_p4": ("tsp", 50, -1, 4, 1),
    "tsp100_dense_p1": ("tsp", 100, -1, 1, 1),
    "tsp500_k50": ("tsp", 500, 50, 1, 1),
    "tsp1000_k100": ("tsp", 1000, 100, 1, 1),
    "mis_er700_800_seq4": ("mis", None, None, 1, 4),      # sequential_sampling = 4 on one ER graph per instance
}


def make_model(task, sparse_factor, sd, dev):
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, n_layers=12, hidden_dim=256,
                inference_trick="ddim", inference_diffusion_steps=50, inference_schedule="cosine",
                sparse_factor=sparse_factor if task == "tsp" else -1)
    return (TSPModel if task == "tsp" else MISModel)(args, sd, device=dev, seed=1)


def instance(task, n, k, P, i, dev):
    if task == "mis":      # ER-[700,800]: each size is a new shape, so its first sample captures and the other three replay
        size = int(np.random.default_rng(100 + i).integers(700, 801))
        return (size, torch.from_numpy(er_mis_edge_index(size, 0.15, seed=i)).to(dev))
    pts = np.random.default_rng(100 + i).random((n, 2))
    p32 = torch.from_numpy(pts.astype(np.float32)).to(dev)
    if k > 0:
        return (p32, knn_edge_index_gpu(pts, k, device=dev))
    return (p32.reshape(1, n, 2).repeat(P, 1, 1), None)


def timed_call(m, task, inst, seq, seed, graphed, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    outs = []
    for s in range(seq):
        gen = torch.Generator(device=dev).manual_seed(seed * 16 + s)
        outs.append(m.sample(inst[0], inst[1], generator=gen, graphed=graphed))
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, outs


def pct(v, q):
    return float(np.percentile(np.asarray(v), q)) if v else None


def run(name, args, sd, dev):
    task, n, k, P, seq = WORKLOADS[name]
    eager_m = make_model(task, k, sd, dev) if args.mode in ("both", "eager") else None
    graph_m = make_model(task, k, sd, dev) if args.mode in ("both", "graphed") else None
    eager_ms, graph_ms, capture_ms, equal = [], [], [], []
    for i in range(args.instances + 1):          # instance 0: warm-up of both sides
        inst = instance(task, n, k, P, i, dev)
        captures = graph_m.graph_captures if graph_m is not None else 0
        te = tg = oe = og = None
        if eager_m is not None:
            te, oe = timed_call(eager_m, task, inst, seq, i, False, dev)
        if graph_m is not None:
            tg, og = timed_call(graph_m, task, inst, seq, i, True, dev)
        if oe is not None and og is not None:
            equal.append(all(torch.equal(a, b) for a, b in zip(oe, og)))
        if i == 0:
            if tg is not None:
                capture_ms.append(tg)
            continue
        if te is not None:
            eager_ms.append(te)
        if tg is not None:
            if graph_m.graph_captures != captures:        # this instance's shape was new: its first call captured
                capture_ms.append(tg)
            graph_ms.append(tg)
    rec = dict(workload=name, task=task, n=n, sparse_factor=k, parallel_sampling=P, sequential_sampling=seq,
               instances=args.instances, steps=50, hidden=256, n_layers=12,
               eager_ms_median=pct(eager_ms, 50), eager_ms_p90=pct(eager_ms, 90),
               graphed_ms_median=pct(graph_ms, 50), graphed_ms_p90=pct(graph_ms, 90),
               capture_ms=capture_ms, graph_captures=graph_m.graph_captures if graph_m is not None else None,
               graph_replays=graph_m.graph_replays if graph_m is not None else None,
               bitwise_equal=(all(equal) if equal else None), eager_ms=eager_ms, graphed_ms=graph_ms)
    if rec["eager_ms_median"] and rec["graphed_ms_median"]:
        rec["speedup_median"] = rec["eager_ms_median"] / rec["graphed_ms_median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--instances", type=int, default=20)
    ap.add_argument("--mode", choices=("both", "eager", "graphed"), default="both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latency.py needs a GPU")
    dev = torch.device("cuda:0")
    sd = random_state_dict(256, 12, 2, seed=0)
    recs = []
    for name in (args.only or list(WORKLOADS)):
        rec = run(name, args, sd, dev)
        recs.append(rec)
        print(json.dumps({k: v for k, v in rec.items() if k not in ("eager_ms", "graphed_ms")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), mode=args.mode, results=recs), f, indent=1)


if __name__ == "__main__":
    main()
