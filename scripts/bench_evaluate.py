"""Throughput of the evaluation runner (``python -m difusco_amd.evaluate``) against ``solve_tsp_batch`` / ``solve_mis_batch``
called directly on the same instances, chunks, seeds and offsets.  Synthetic splits written in the reference's formats (TSP
text lines, MIS ``.gpickle`` files), synthetic H 256 / 12-layer categorical weights in a Lightning-shaped checkpoint, 50
cosine steps, P = S = 1.

    python scripts/bench_evaluate.py [--out-dir profiles/r07] [--only tsp50_dense mis_er700_800] [--reps 2]

Writes ``<out-dir>/evaluate_<workload>.json``.  ``overhead_beyond_parse_pct`` = 100 ((runner wall - runner parse) / direct wall
- 1), medians of ``--reps`` alternating runs after one warm-up run of each.  The runner's wall covers reading the split,
solving, building the records and the metrics; the direct wall covers the solve calls only.  Tour quality is not looked at
(random weights)."""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difusco_amd import MISModel, TSPModel  # noqa: E402
from difusco_amd import evaluate as E  # noqa: E402
from difusco_amd.pipeline import solve_mis_batch, solve_tsp_batch  # noqa: E402
from difusco_amd.synthetic import er_mis_edge_index, random_state_dict  # noqa: E402

WORKLOADS = {      # name: (task, n, sparse_factor, instances)
    "tsp50_dense": ("tsp", 50, -1, 1280),
    "tsp500_k50": ("tsp", 500, 50, 128),
    "tsp1000_k100": ("tsp", 1000, 100, 32),
    "mis_er700_800": ("mis", None, -1, 64),
}


def write_split(folder, name, task, n, B):
    """The split in the reference's format; returns its path relative to ``folder`` (the runner's --storage_path)."""
    rng = np.random.default_rng(0)
    if task == "tsp":
        with open(os.path.join(folder, f"{name}.txt"), "w") as f:
            for _ in range(B):
                pts, perm = rng.random((n, 2)), rng.permutation(n)
                tour = np.concatenate([perm, perm[:1]]) + 1
                f.write(" ".join(str(float(v)) for v in pts.reshape(-1)) + " output " + " ".join(map(str, tour.tolist())) + "\n")
        return f"{name}.txt"
    import networkx as nx
    os.makedirs(os.path.join(folder, name))
    for i, s in enumerate(rng.integers(700, 801, size=B)):
        s = int(s)
        ei = er_mis_edge_index(s, 0.15, seed=i)
        g = nx.Graph()
        g.add_nodes_from(range(s))
        g.add_edges_from(ei[:, :(ei.shape[1] - s) // 2].T.tolist())
        with open(os.path.join(folder, name, f"er_{i:03d}.gpickle"), "wb") as f:
            pickle.dump(g, f)
    return os.path.join(name, "*gpickle")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--only", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = random_state_dict(256, 12, 2, seed=0)
    tmp = tempfile.mkdtemp(prefix="bench_evaluate_")
    ckpt = os.path.join(tmp, "last.ckpt")
    torch.save({"epoch": 0, "global_step": 0, "state_dict": {"model." + k: v for k, v in sd.items()}}, ckpt)
    for name in args.only:
        task, n, k, B = WORKLOADS[name]
        rel = write_split(tmp, name, task, n, B)
        argv = ["--task", task, "--diffusion_type", "categorical", "--do_test", "--do_valid_only", "--storage_path", tmp,
                "--validation_split", rel, "--validation_examples", str(B), "--inference_schedule", "cosine",
                "--inference_diffusion_steps", str(args.steps), "--sparse_factor", str(k), "--ckpt_path", ckpt]
        margs = dict(diffusion_type="categorical", inference_schedule="cosine", inference_diffusion_steps=args.steps,
                     sparse_factor=k)
        model = (TSPModel if task == "tsp" else MISModel)(margs, sd, device=dev)
        examples = E.read_split(task, os.path.join(tmp, rel), B)
        chunks = E.split_chunks(task, examples, k, 1)

        def direct():
            timings, res = {}, []
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for lo, hi in chunks:
                seeds = [E.instance_seed(0, "val", i) for i in range(lo, hi)]
                gens = [E.instance_generator(s) for s in seeds]
                if task == "tsp":
                    res += solve_tsp_batch(model, np.stack([examples[i].points for i in range(lo, hi)]), k, seeds=seeds,
                                           generators=gens, timings=timings, step_offset=0)
                else:
                    res += solve_mis_batch(model, [(examples[i].n_nodes, examples[i].edge_index) for i in range(lo, hi)],
                                           seeds=seeds, generators=gens, timings=timings, step_offset=0)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0, timings, res

        runs = {"runner": [], "direct": []}
        for rep in range(args.reps + 1):                 # rep 0: warm-up of both
            lines, recs = E.run(argv)
            wall_d, timings_d, res = direct()
            if rep:
                runs["runner"].append(lines[0])
                runs["direct"].append((wall_d, timings_d))
        r_wall = statistics.median(l["wall_s"] for l in runs["runner"])
        r_parse = statistics.median(l["stages_s"]["parse"] for l in runs["runner"])
        d_wall = statistics.median(w for w, _ in runs["direct"])
        rec = {"workload": name, "task": task, "n": n, "sparse_factor": k, "instances": B, "parallel_sampling": 1,
               "inference_steps": args.steps, "chunks": len(chunks), "chunk_lengths": sorted({hi - lo for lo, hi in chunks}),
               "runner": {"wall_s": [l["wall_s"] for l in runs["runner"]], "median_wall_s": r_wall, "median_parse_s": round(r_parse, 4),
                          "instances_per_s": round(B / r_wall, 3), "stages_s": runs["runner"][-1]["stages_s"]},
               "direct": {"wall_s": [round(w, 4) for w, _ in runs["direct"]], "median_wall_s": round(d_wall, 4),
                          "instances_per_s": round(B / d_wall, 3),
                          "stages_s": {s: round(v, 4) for s, v in sorted(runs["direct"][-1][1].items())}},
               "overhead_beyond_parse_pct": round(100.0 * ((r_wall - r_parse) / d_wall - 1.0), 2),
               "records_equal_direct": all(r["solved_cost"] == float(x[1]) for r, x in zip(recs, res)) and len(recs) == len(res)}
        print(json.dumps(rec), flush=True)
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, f"evaluate_{name}.json"), "w") as f:
                json.dump(dict(rec, device=torch.cuda.get_device_name(dev)), f, indent=1)


if __name__ == "__main__":
    main()
