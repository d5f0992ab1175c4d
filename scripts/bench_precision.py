"""fp16x3 (the default) against fp16x1 (one fp16 product per edge-GEMM term, the reference's --fp16) on one GPU, in one process.

    python scripts/bench_precision.py [--workload tsp1000 tsp10000] [--steps 20] [--warmup 5] [--reps 3] [--out FILE]

Workloads as bench.py: tsp1000 = TSP-1000, K = 100, 8 graphs, categorical (the headline configuration); tsp10000 = TSP-10000,
K = 100, 1 graph, Gaussian.  H = 256, 12 layers, synthetic weights.  Each precision has its own engine on the same weights; after
the warm-up, timed loops of `steps` steps alternate between the two precisions `reps` times (so both see the same thermal and
power history), each loop between two device fences, with the firmware's limiter residency (scripts/smu_metrics.py) sampled
around it.  Printed per precision: graph-steps/s (the median loop), power.throttle; then the ratio and the L_inf between the two
heatmaps (categorical: the posterior probability of one step from the same x_t; Gaussian: the eps prediction)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from difusco_amd import TSPModel  # noqa: E402
from difusco_amd.engine import DenoiseEngine  # noqa: E402
from difusco_amd.schedules import InferenceSchedule  # noqa: E402
from difusco_amd.synthetic import random_state_dict, tsp_batch_gpu  # noqa: E402

WORKLOADS = {"tsp1000": dict(diffusion="categorical", nodes=1000, knn=100, graphs=8),
             "tsp10000": dict(diffusion="gaussian", nodes=10000, knn=100, graphs=1)}
PRECISIONS = ("fp16x3", "fp16x1")


def sampler(dev):
    try:
        from smu_metrics import SmuMetrics, SmuSampler
        pr = torch.cuda.get_device_properties(dev)
        m = SmuMetrics(pci_bdf=f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0",
                       index=dev.index or 0)
        return lambda: SmuSampler(m, period=0.02) if m.available else None
    except Exception:      # noqa: BLE001
        return lambda: None


def run(name, args, dev, new_sampler):
    wl = WORKLOADS[name]
    gaussian = wl["diffusion"] == "gaussian"
    params = random_state_dict(256, 12, 1 if gaussian else 2, seed=20240926)
    margs = dict(diffusion_type=wl["diffusion"], diffusion_schedule="linear", diffusion_steps=1000, inference_diffusion_steps=50,
                 inference_schedule="cosine", sparse_factor=wl["knn"], n_layers=12, hidden_dim=256, inference_trick="ddim")
    models = {}
    for prec in PRECISIONS:
        eng = DenoiseEngine(params, device=dev, precision=prec)
        models[prec] = TSPModel(margs, engine=eng, seed=1234)
    points, edge_index = tsp_batch_gpu(wl["nodes"], wl["knn"], range(wl["graphs"]), dev)
    gen = torch.Generator().manual_seed(0)
    xt0 = torch.randn(edge_index.shape[1], generator=gen)
    xt0 = (xt0 if gaussian else (xt0 > 0).float()).to(dev)
    sched = InferenceSchedule("cosine", T=1000, inference_T=50)

    def one_step(m, i, xt, aux=False):
        t1, t2 = sched(i % 49)
        t1, t2 = np.array([t1]), np.array([t2])
        if gaussian:
            return m.gaussian_denoise_step(points, xt, t1, dev, edge_index, target_t=t2, return_aux=aux)
        return m.categorical_denoise_step(points, xt, t1, dev, edge_index, target_t=t2, return_aux=aux)

    xts = {}
    for prec, m in models.items():
        m.model.prepare_times([int(sched(i)[0]) for i in range(49)])
        xt = xt0
        for i in range(args.warmup):
            xt = one_step(m, i, xt)
        xts[prec] = xt
    torch.cuda.synchronize(dev)
    # heatmaps of one step from the same x_t
    heat = {}
    for prec, m in models.items():
        r = one_step(m, 0, xt0, aux=True)
        heat[prec] = r[-1].float().reshape(-1)
    torch.cuda.synchronize(dev)
    linf = (heat["fp16x1"] - heat["fp16x3"]).abs().max().item()
    loops = {p: [] for p in PRECISIONS}
    smu = {p: new_sampler() for p in PRECISIONS}
    for rep in range(args.reps):
        for prec in (PRECISIONS if rep % 2 == 0 else PRECISIONS[::-1]):
            m, xt = models[prec], xts[prec]
            torch.cuda.synchronize(dev)
            if smu[prec] is not None:
                smu[prec].start()
            t0 = time.perf_counter()
            for i in range(args.steps):
                xt = one_step(m, args.warmup + i, xt)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            if smu[prec] is not None:
                smu[prec].stop()
            xts[prec] = xt
            loops[prec].append(wl["graphs"] * args.steps / dt)
    out = {"workload": name, "what": f"TSP-{wl['nodes']} K={wl['knn']} x{wl['graphs']} {wl['diffusion']}, H 256, L 12",
           "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "heatmap_linf_fp16x1_vs_fp16x3": linf,
           "heatmap": "posterior probability" if not gaussian else "eps prediction"}
    for prec in PRECISIONS:
        s = smu[prec].summary() if smu[prec] is not None else {"available": False}
        out[prec] = {"graph_steps_per_s": float(np.median(loops[prec])), "loops": loops[prec], "power": s}
    out["ratio_fp16x1_over_fp16x3"] = out["fp16x1"]["graph_steps_per_s"] / out["fp16x3"]["graph_steps_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["tsp1000", "tsp10000"], choices=sorted(WORKLOADS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    new_sampler = sampler(dev)
    res = []
    for name in args.workload:
        r = run(name, args, dev, new_sampler)
        res.append(r)
        print(f"{r['what']}: fp16x3 {r['fp16x3']['graph_steps_per_s']:.1f} graph-steps/s, "
              f"fp16x1 {r['fp16x1']['graph_steps_per_s']:.1f} graph-steps/s, ratio {r['ratio_fp16x1_over_fp16x3']:.3f}, "
              f"heatmap L_inf {r['heatmap_linf_fp16x1_vs_fp16x3']:.2e}", flush=True)
        for prec in PRECISIONS:
            print(f"  {prec} power.throttle: {json.dumps(r[prec]['power'].get('residency', r[prec]['power']))[:400]}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
