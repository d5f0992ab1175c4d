"""Which launches a step configuration produces (``-m gpu``): the standing guard of the step driver's launch plan
(``csrc/api.hip``: ``make_plan`` and the stage functions).

One step per configuration runs with the in-library profiler on all categories (``difusco_profile_enable(1, ..)``), and the
launches per category - (E-row linears / fused edge layers, node linears, gate / node update, head, embedding) - are compared
with literal tuples.  A later edit of the plan can therefore not silently add, drop or recategorise a launch: ``bench.py``
times the dominant kernel through category 0, and the graphed sampler captures exactly this sequence.

The shapes are the smallest that take every path: H = 256, L = 3 on a k-NN graph of N = 72, K = 7 (E = 504: no multiple of
256 or 32, so the partial-tile and pad paths run), a second graph with E = 512 (the pad reset has zero bytes), an
Erdos-Renyi MIS graph of 60 nodes, and H = 64 for the widths without a fused kernel."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NCAT = 5      # PROF_LINEAR_EDGE, PROF_LINEAR_NODE, PROF_GATE, PROF_HEAD, PROF_EMBED (csrc/api.hip)
T_STEP = 500.0
POST_CATEGORICAL = np.array([0.9, 0.2, 0.1, 0.8, 1.0, 0, 0, 0], dtype=np.float32)      # draws (Philox)
POST_GAUSSIAN = np.array([1.02, 0.3, 0.05, 0.1, 0.0, 0, 0, 0], dtype=np.float32)       # DDIM branch: no draw

# name -> configuration.  graph: ("knn", N, K) or "er"; flags: _lib.FLAG_* names; everything else as DenoiseEngine / step take it.
CASES = {
    "tsp_fused":         dict(),
    "tsp_prepared":      dict(prepared=True),
    "tsp_caller_tbias":  dict(tbias=True, graph=("knn", 64, 8)),
    "tsp_no_l0_fold":    dict(flags=("FLAG_NO_L0_FOLD",)),
    "tsp_no_tail_fold":  dict(flags=("FLAG_NO_TAIL_FOLD",)),
    "tsp_unfused":       dict(fused=False),
    "tsp_fp16x1":        dict(precision="fp16x1"),
    "tsp_gauss_table":   dict(diffusion="gaussian"),
    "tsp_gauss_notable": dict(diffusion="gaussian", use_gen_table=False),
    "mis_fused":         dict(task="mis", graph="er"),
    "mis_unfused":       dict(task="mis", graph="er", fused=False),
    "tsp_gn_phases":     dict(gn_phases=True),
    "tsp_fp32_h64":      dict(precision="fp32", hidden=64, layers=2),
}

# Launches per category of one step, RECORDED FROM THE LIBRARY OF THE COMMIT BEFORE THE LAUNCH PLAN EXISTED (the monolithic
# difusco_denoise_step_shifted), not derived by hand and not taken from the code under test.  "tsp_gn_phases" holds the
# phase-1 call followed by the phase-2 call.
EXPECTED = {
    "tsp_fused":         [(3, 5, 2, 1, 6)],
    "tsp_prepared":      [(3, 2, 2, 1, 2)],
    "tsp_caller_tbias":  [(3, 5, 2, 1, 5)],
    "tsp_no_l0_fold":    [(3, 5, 2, 1, 7)],
    "tsp_no_tail_fold":  [(3, 5, 3, 1, 6)],
    "tsp_unfused":       [(6, 7, 3, 1, 5)],
    "tsp_fp16x1":        [(3, 5, 2, 1, 6)],
    "tsp_gauss_table":   [(3, 5, 2, 1, 4)],
    "tsp_gauss_notable": [(3, 5, 2, 1, 4)],
    "mis_fused":         [(3, 5, 3, 1, 4)],
    "mis_unfused":       [(6, 7, 3, 1, 3)],
    "tsp_gn_phases":     [(3, 5, 2, 1, 6), (0, 0, 0, 1, 0)],
    "tsp_fp32_h64":      [(4, 3, 2, 1, 5)],
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _collect():
    from difusco_amd import _lib
    ms, cnt = (ctypes.c_double * NCAT)(), (ctypes.c_int64 * NCAT)()
    _lib.check(_lib.lib().difusco_profile_collect(ms, cnt, NCAT))
    return tuple(int(v) for v in cnt)


def run_case(dev, name):
    """One step of configuration ``name`` -> (launch tuples: one per C call of the step, outputs as numpy arrays)."""
    from difusco_amd import _lib
    from difusco_amd.engine import DenoiseEngine
    from difusco_amd.graph import build_csr
    from difusco_amd.synthetic import er_mis_edge_index, random_state_dict, tsp_instance
    cfg = CASES[name]
    hidden, layers = cfg.get("hidden", 256), cfg.get("layers", 3)
    gaussian = cfg.get("diffusion") == "gaussian"
    mis = cfg.get("task") == "mis"
    flags = 0
    for f in cfg.get("flags", ()):
        flags |= getattr(_lib, f)
    eng = DenoiseEngine(random_state_dict(hidden, layers, 1 if gaussian else 2, seed=3), device=dev,
                        precision=cfg.get("precision", "fp16x3"), fused=cfg.get("fused", True), backend="ctypes", flags=flags,
                        use_gen_table=cfg.get("use_gen_table", True))
    gen = torch.Generator().manual_seed(11)
    pts = None
    if mis:
        g = build_csr(torch.from_numpy(er_mis_edge_index(60, 0.15, seed=3)), 60, dev)
        rows = g.n_nodes
    else:
        _, n, k = cfg.get("graph", ("knn", 72, 7))
        p, ei = tsp_instance(n, k, seed=5)
        pts = torch.from_numpy(p).to(dev)
        g = build_csr(torch.from_numpy(ei), n, dev, points=pts)
        rows = g.n_edges
    x = torch.randn(rows, generator=gen)
    xt = (x if gaussian else (x > 0).float()).to(dev)
    prepared = eng.prepare(g, pts) if cfg.get("prepared") else None
    if cfg.get("tbias"):
        eng.prepare_times([T_STEP])
    if gaussian:
        eng.gen_table()      # (built outside the profiled step)
    counts = []
    gn_reduce = (lambda sums: counts.append(_collect())) if cfg.get("gn_phases") else None      # (runs between the two phases)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().difusco_profile_enable(1, 256))
    try:
        out = eng.step(g, _lib.TASK_MIS if mis else _lib.TASK_TSP, _lib.GAUSSIAN if gaussian else _lib.CATEGORICAL, xt, T_STEP,
                       POST_GAUSSIAN if gaussian else POST_CATEGORICAL, points=pts, xt_is_binary=not gaussian and not mis,
                       seed=7, offset=3, want_pred=True, want_prob=True, gn_reduce=gn_reduce, prepared=prepared)
        torch.cuda.synchronize()
        counts.append(_collect())
    finally:
        _lib.lib().difusco_profile_enable(0, 0)
    return counts, [None if o is None else o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", list(CASES))
def test_launches_per_category(dev, name):
    counts, out = run_case(dev, name)
    print(name, counts)
    assert np.isfinite(out[0]).all()
    assert counts == EXPECTED[name]
