"""TSP instances of different sizes in one batched call (the list form of ``pipeline.solve_tsp_batch``) against the two things
it can be compared with, and the ragged 2-opt entry against the grouped one at equal sizes.

    python scripts/bench_mixed_solve.py [--out-dir profiles/mixed_sizes] [--only dense_20_100 sparse_300_700 two_opt_equal]
                                        [--merge_method batched]

Synthetic weights (H 256, 12 layers, categorical), 50 steps, P = 1, uniform points; the numbers are throughput, the answers are
not looked at (tests/test_gpu_mixed_sizes.py pins them to the solo calls).

(a) dense_20_100: 64 dense instances, n uniform in 20..100.   (b) sparse_300_700: 16 sparse instances, K = 50, n in 300..700.
    Three modes, each warmed up by one full untimed pass, then ``--repeats`` timed passes with the modes interleaved; the clock
    covers the whole call and ends in a device synchronise.  Reported: median (min, max) of wall seconds, instances/s, and the
    median per-stage seconds.
      mixed_batch       one ``solve_tsp_batch`` call over the list;
      solo_loop         ``solve_tsp`` per instance - what such a set costs without the list form;
      equal_size_batch  the same number of instances, all of the mean n, in one array call - the ceiling.
(c) two_opt_equal: the 2-opt stage alone, G = 16 groups of P = 4 random tours over n = 500, both methods:
    ``difusco_tsp_two_opt_ragged`` against ``difusco_tsp_two_opt_grouped[_screened]`` on device-resident inputs, interleaved
    repeats, ms per move = call time / moves of the call.  ``within_grouped_spread`` says whether the ragged median lies inside
    the grouped entry's min-max.  ``--two-opt-entries ragged`` (or ``grouped``) runs one entry alone, for a kernel trace."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difusco_amd import TSPModel, _lib  # noqa: E402
from difusco_amd.engine import DenoiseEngine  # noqa: E402
from difusco_amd.pipeline import solve_tsp, solve_tsp_batch  # noqa: E402
from difusco_amd.synthetic import random_state_dict  # noqa: E402

SOLVE = {      # name: (sparse_factor, instances, n_lo, n_hi)
    "dense_20_100": (-1, 64, 20, 100),
    "sparse_300_700": (50, 16, 300, 700),
}


def spread(values):
    return {"median": round(statistics.median(values), 5), "min": round(min(values), 5), "max": round(max(values), 5)}


def make_model(sparse_factor, steps, engine):
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, n_layers=12, hidden_dim=256,
                inference_trick="ddim", inference_diffusion_steps=steps, inference_schedule="cosine", sparse_factor=sparse_factor)
    return TSPModel(args, engine=engine, seed=1)


def run_solve(name, args, dev, engine):
    k, B, lo, hi = SOLVE[name]
    rng = np.random.default_rng(0)
    sizes = [int(n) for n in rng.integers(lo, hi + 1, size=B)]
    mixed = [rng.random((n, 2)) for n in sizes]
    mean_n = int(round(float(np.mean(sizes))))
    equal = rng.random((B, mean_n, 2))
    m = make_model(k, args.steps, engine)
    kw = dict(parallel_sampling=1, two_opt_iterations=args.two_opt)

    def gens():
        return [torch.Generator().manual_seed(b) for b in range(B)]

    def mixed_batch(t):
        solve_tsp_batch(m, mixed, k, seeds=list(range(B)), generators=gens(), timings=t, merge_method=args.merge_method, **kw)

    def solo_loop(t):
        for b, g in enumerate(gens()):
            solve_tsp(m, mixed[b], k, generator=g, timings=t, **kw)

    def equal_size_batch(t):
        solve_tsp_batch(m, equal, k, seeds=list(range(B)), generators=gens(), timings=t, merge_method=args.merge_method, **kw)

    modes = (("mixed_batch", mixed_batch), ("solo_loop", solo_loop), ("equal_size_batch", equal_size_batch))
    for _, fn in modes:                                          # warm-up: every shape of the timed passes
        fn(None)
    torch.cuda.synchronize(dev)
    walls = {mode: [] for mode, _ in modes}
    stages = {mode: [] for mode, _ in modes}
    for _ in range(args.repeats):
        for mode, fn in modes:                                   # interleaved
            t = {}
            t0 = time.perf_counter()
            fn(t)
            torch.cuda.synchronize(dev)
            walls[mode].append(time.perf_counter() - t0)
            stages[mode].append(t)
    rec = {"workload": name, "instances": B, "sparse_factor": k, "sizes": sizes, "mean_n": mean_n, "parallel_sampling": 1,
           "inference_steps": args.steps, "two_opt_iterations": args.two_opt, "repeats": args.repeats,
           "merge_method": args.merge_method}
    for mode, _ in modes:
        rec[mode] = {"wall_s": spread(walls[mode]),
                     "instances_per_s": spread([B / w for w in walls[mode]]),
                     "stages_s_median": {s: round(statistics.median(t[s] for t in stages[mode]), 5) for s in sorted(stages[mode][0])}}
    med = {mode: rec[mode]["wall_s"]["median"] for mode, _ in modes}
    rec["mixed_vs_solo_loop"] = round(med["solo_loop"] / med["mixed_batch"], 3)
    rec["mixed_vs_equal_size_batch"] = round(med["equal_size_batch"] / med["mixed_batch"], 3)
    rec["stage_speedup_vs_solo_loop"] = {s: round(v / max(rec["mixed_batch"]["stages_s_median"].get(s, 0.0), 1e-9), 3)
                                         for s, v in rec["solo_loop"]["stages_s_median"].items()}
    return rec


def run_two_opt(args, dev):
    """(c): both entries on the same device-resident inputs; every repeat starts from the same tours."""
    G, P, n, cap = 16, 4, 500, args.two_opt_moves
    L = _lib.lib()
    rng = np.random.default_rng(1)
    pts = torch.from_numpy(rng.random((G, n, 2))).to(dev)
    start = torch.from_numpy(np.stack([np.concatenate([[0], 1 + rng.permutation(n - 1), [0]]) for _ in range(G * P)])
                             .astype(np.int32)).to(dev)
    tours = torch.empty_like(start)
    group_n, group_tours = np.full(G, n, dtype=np.int32), np.full(G, P, dtype=np.int32)
    its = np.zeros(G, dtype=np.int64)
    pairs = ctypes.c_int64()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = ctypes.c_void_p
    rec = {"workload": "two_opt_equal", "groups": G, "tours_per_group": P, "n": n, "max_iterations": cap, "repeats": args.repeats_two_opt}
    for code, method in enumerate(("exact", "screened")):
        nb = ctypes.c_size_t()
        _lib.check((L.difusco_tsp_two_opt_grouped_screened_workspace_bytes if code else L.difusco_tsp_two_opt_grouped_workspace_bytes)(
            n, G, P, ctypes.byref(nb)))
        ws_g = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        _lib.check(L.difusco_tsp_two_opt_ragged_workspace_bytes(G, group_n.ctypes.data, group_tours.ctypes.data, code, ctypes.byref(nb)))
        ws_r = torch.empty(nb.value, dtype=torch.uint8, device=dev)

        def grouped():
            head = (n, G, P, vp(pts.data_ptr()), vp(tours.data_ptr()), cap, vp(ws_g.data_ptr()), ws_g.numel(), its.ctypes.data)
            if code:
                _lib.check(L.difusco_tsp_two_opt_grouped_screened(*head, ctypes.byref(pairs), stream))
            else:
                _lib.check(L.difusco_tsp_two_opt_grouped(*head, stream))

        def ragged():
            _lib.check(L.difusco_tsp_two_opt_ragged(G, group_n.ctypes.data, group_tours.ctypes.data, vp(pts.data_ptr()),
                                                    vp(tours.data_ptr()), cap, code, vp(ws_r.data_ptr()), ws_r.numel(),
                                                    its.ctypes.data, ctypes.byref(pairs), stream))

        entries = tuple(e for e in (("grouped", grouped), ("ragged", ragged)) if e[0] in args.two_opt_entries)
        ms, moves, result = {e: [] for e, _ in entries}, {}, {}
        for r in range(args.repeats_two_opt + 1):                # repeat 0 is the warm-up
            for e, fn in entries:                                # interleaved
                tours.copy_(start)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()                                             # blocks until every group is done
                dt = time.perf_counter() - t0
                moves[e] = int(its.max())
                result[e] = (tours.clone(), its.copy())
                if r:
                    ms[e].append(1e3 * dt / moves[e])
        rec[method] = {"moves": moves, **{e + "_ms_per_move": spread(ms[e]) for e, _ in entries}}
        if len(entries) == 2:
            g, rg = rec[method]["grouped_ms_per_move"], rec[method]["ragged_ms_per_move"]
            rec[method].update(
                same_tours_and_iterations=bool(torch.equal(result["grouped"][0], result["ragged"][0]))
                and result["grouped"][1].tolist() == result["ragged"][1].tolist(),
                ragged_over_grouped_median=round(rg["median"] / g["median"], 4),
                within_grouped_spread=bool(g["min"] <= rg["median"] <= g["max"]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", dest="out_dir", default=None)
    ap.add_argument("--only", nargs="*", default=list(SOLVE) + ["two_opt_equal"])
    ap.add_argument("--steps", type=int, default=50, help="inference diffusion steps")
    ap.add_argument("--two-opt", dest="two_opt", type=int, default=1000, help="2-opt cap of (a) and (b)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--two-opt-moves", dest="two_opt_moves", type=int, default=400, help="2-opt cap of (c)")
    ap.add_argument("--two-opt-entries", dest="two_opt_entries", nargs="*", default=["grouped", "ragged"],
                    choices=("grouped", "ragged"), help="(c): one entry alone, for a kernel trace of it")
    ap.add_argument("--repeats-two-opt", dest="repeats_two_opt", type=int, default=9)
    ap.add_argument("--merge_method", choices=("loop", "batched"), default="loop", help="heatmap -> tour merge of the batched modes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixed_solve measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    engine = None
    for name in args.only:
        if name == "two_opt_equal":
            rec = run_two_opt(args, dev)
        else:
            engine = engine or DenoiseEngine(random_state_dict(256, 12, 2, seed=0), device=dev)
            rec = run_solve(name, args, dev, engine)
        rec["device"] = torch.cuda.get_device_name(dev)
        print(json.dumps(rec), flush=True)
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, name + ".json"), "w") as f:
                json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
