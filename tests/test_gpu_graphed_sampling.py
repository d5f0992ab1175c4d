"""Graphed sampling on the GPU: ``sample(..., graphed=True)`` replays the whole loop as one captured HIP graph and returns the
bits of the eager loop at the same engine call counter.  Every comparison runs twin models built from the same weights and seed
(separate engines, equal call counters): one graphed, one eager."""
import numpy as np
import pytest
import torch

from difusco_amd import _lib
from difusco_amd.synthetic import er_mis_edge_index, random_state_dict, tsp_instance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _args(diffusion, sparse_factor, L, steps, trick="ddim"):
    return dict(diffusion_type=diffusion, diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=L, hidden_dim=256, inference_trick=trick, inference_diffusion_steps=steps,
                inference_schedule="cosine")


def _twins(cls_name, diffusion, dev, L=3, steps=8, trick="ddim", sparse_factor=20, args_over=None, **kw):
    from difusco_amd import models
    cls = getattr(models, cls_name)
    sd = random_state_dict(256, L, 2 if diffusion == "categorical" else 1, seed=3)
    args = dict(_args(diffusion, sparse_factor, L, steps, trick), **(args_over or {}))
    return [cls(args, sd, device=dev, seed=11, **kw) for _ in range(2)]


def _tsp(dev, n, k, seed):
    p, ei = tsp_instance(n, k, seed=seed)
    return torch.from_numpy(p).to(dev), torch.from_numpy(ei).to(dev)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} values differ"


# ---- the kernel-side shift -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["torch", "ctypes"])
@pytest.mark.parametrize("diffusion,trick", [("categorical", "ddim"), ("gaussian", None)])
def test_offset_shift_adds_to_the_philox_offset(dev, backend, diffusion, trick):
    """A step at offset o with a device shift s draws what the plain step at offset o + s draws (Bernoulli / DDPM normal)."""
    m, _ = _twins("TSPModel", diffusion, dev, backend=backend, trick=trick)
    pts, ei = _tsp(dev, 120, 12, seed=4)
    g = m.prepare_graph(ei, 120, points=pts)
    x = torch.randn(ei.shape[1], generator=_gen(dev, 1), device=dev)
    if diffusion == "categorical":
        x = (x > 0).float()
    post = m._post_constants(500, 450)
    assert post[4] != 0                    # the step draws
    C = _lib.CATEGORICAL if diffusion == "categorical" else _lib.GAUSSIAN
    step = lambda off, sh: m.model.step(g, _lib.TASK_TSP, C, x, 500.0, post, points=pts, xt_is_binary=C == _lib.CATEGORICAL,
                                        seed=m.seed, offset=off, offset_shift=sh)[0]
    shift = torch.tensor([37], dtype=torch.int64, device=dev)
    ref = step(42, None)
    _same(step(5, shift), ref)
    _same(step(42, torch.zeros(1, dtype=torch.int64, device=dev)), ref)
    assert not torch.equal(step(5, None), ref)          # (the offset does change the draws)
    with pytest.raises((ValueError, RuntimeError)):
        step(5, shift.cpu())


def test_step_op_refuses_a_host_shift(dev):
    m, _ = _twins("TSPModel", "categorical", dev, backend="torch")
    pts, ei = _tsp(dev, 64, 8, seed=2)
    g = m.prepare_graph(ei, 64, points=pts)
    x = torch.zeros(ei.shape[1], device=dev)
    call = lambda sh: m.model._step_torch_op(g, _lib.TASK_TSP, _lib.CATEGORICAL, x, 500.0, m._post_constants(500, 450), pts,
                                             True, None, m.seed, 0, False, False, None, m.model._workspace(g), offset_shift=sh)
    for bad in (torch.zeros(1, dtype=torch.int64),                      # host tensor
                torch.zeros(1, dtype=torch.int32, device=dev),          # wrong dtype
                torch.zeros(2, dtype=torch.int64, device=dev)):         # two elements
        with pytest.raises(RuntimeError, match="offset_shift"):
            call(bad)
    call(torch.zeros(1, dtype=torch.int64, device=dev))                 # (the op itself runs)


# ---- 1. the offset shift across replays ------------------------------------------------------------------------------------
def test_replays_draw_fresh_numbers_like_eager_calls(dev):
    """TSP-500 k-NN (K = 50), categorical, H = 256, L = 12, fused fp16x3, 50 steps.  The same x_T three times: the calls differ
    only by their Philox offsets, so without the device shift replay 2 would repeat replay 1."""
    g_m, e_m = _twins("TSPModel", "categorical", dev, L=12, steps=50, sparse_factor=50, precision="fp16x3", fused=True)
    pts, ei = _tsp(dev, 500, 50, seed=9)
    x0 = torch.randn(ei.shape[1], generator=_gen(dev, 3), device=dev)
    outs = []
    for _ in range(3):
        a = g_m.sample(pts, ei, xt0=x0, graphed=True)
        b = e_m.sample(pts, ei, xt0=x0)
        _same(a, b)
        assert g_m.model.calls == e_m.model.calls
        outs.append(a)
    assert g_m.graph_captures == 1 and g_m.graph_replays == 2
    assert not torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[1])


# ---- 2. one capture serves every instance of a shape -----------------------------------------------------------------------
def test_instances_of_one_shape_share_one_capture(dev):
    g_m, e_m = _twins("TSPModel", "categorical", dev)
    for i in range(3):
        pts, ei = _tsp(dev, 200, 20, seed=20 + i)
        _same(g_m.sample(pts, ei, generator=_gen(dev, i), graphed=True), e_m.sample(pts, ei, generator=_gen(dev, i)))
    assert g_m.graph_captures == 1 and g_m.graph_replays == 2


# ---- 3. the configurations -------------------------------------------------------------------------------------------------
CASES = {      # name: (diffusion, inference_trick, model keywords, args overrides)
    "dense_p1": ("categorical", "ddim", {}, {}), "dense_p4": ("categorical", "ddim", {}, {}),
    "gauss_ddim": ("gaussian", "ddim", {}, {}), "gauss_ddpm": ("gaussian", None, {}, {}),
    "gauss_ddpm_dense_p4": ("gaussian", None, {}, {}),
    "fp16x1": ("categorical", "ddim", dict(precision="fp16x1"), {}), "ctypes": ("categorical", "ddim", dict(backend="ctypes"), {}),
    "gauss_ctypes": ("gaussian", None, dict(backend="ctypes"), {}),
    "unfused_fp32": ("categorical", "ddim", dict(precision="fp32", fused=False), {}),
    "bf16x3": ("gaussian", "ddim", dict(precision="bf16x3"), {}), "no_prepare": ("categorical", "ddim", dict(prepare=False), {}),
    "mean_agg": ("categorical", "ddim", {}, dict(aggregation="mean")), "max_agg": ("gaussian", None, {}, dict(aggregation="max")),
    "no_l0_fold": ("categorical", "ddim", dict(flags=_lib.FLAG_NO_L0_FOLD), {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_tsp_configurations(dev, case):
    diffusion, trick, kw, over = CASES[case]
    g_m, e_m = _twins("TSPModel", diffusion, dev, trick=trick, sparse_factor=-1 if "dense" in case else 20, args_over=over, **kw)
    for i in range(2):
        if "dense" in case:
            P = 4 if case.endswith("p4") else 1
            p, _ = tsp_instance(50, 1, seed=40 + i)
            pts, ei = torch.from_numpy(p).to(dev).reshape(1, 50, 2).repeat(P, 1, 1), None
        else:
            pts, ei = _tsp(dev, 150, 20, seed=40 + i)
        a = g_m.sample(pts, ei, generator=_gen(dev, 7 + i), graphed=True)
        b = e_m.sample(pts, ei, generator=_gen(dev, 7 + i))
        _same(a, b)
    assert g_m.graph_captures == 1 and g_m.graph_replays == 1
    assert g_m.model.calls == e_m.model.calls


def test_sequential_reuse_of_one_graph(dev):
    g_m, e_m = _twins("TSPModel", "categorical", dev)
    pts, ei = _tsp(dev, 300, 20, seed=5)
    for i in range(3):
        _same(g_m.sample(pts, ei, generator=_gen(dev, i), graphed=True), e_m.sample(pts, ei, generator=_gen(dev, i)))
    assert g_m.graph_captures == 1 and g_m.graph_replays == 2


@pytest.mark.parametrize("diffusion,trick", [("categorical", "ddim"), ("gaussian", None)])
def test_mis_sequential_reuse(dev, diffusion, trick):
    g_m, e_m = _twins("MISModel", diffusion, dev, trick=trick)
    n = 300
    ei = torch.from_numpy(er_mis_edge_index(n, 0.03, seed=5)).to(dev)
    for i in range(3):
        _same(g_m.sample(n, ei, generator=_gen(dev, i), graphed=True), e_m.sample(n, ei, generator=_gen(dev, i)))
    assert g_m.graph_captures == 1 and g_m.graph_replays == 2


# ---- 4. eager and graphed calls interleave -----------------------------------------------------------------------------------
def test_interleaved_eager_and_graphed_calls(dev):
    g_m, e_m = _twins("TSPModel", "categorical", dev)
    pts, ei = _tsp(dev, 150, 20, seed=50)
    for i, graphed in enumerate([False, True, False, True, False]):
        _same(g_m.sample(pts, ei, generator=_gen(dev, i), graphed=graphed), e_m.sample(pts, ei, generator=_gen(dev, i)))
    assert g_m.graph_captures == 1 and g_m.graph_replays == 1


# ---- 5. lifetime ------------------------------------------------------------------------------------------------------------
def test_replay_survives_cache_eviction_and_clear_graphs_frees(dev):
    g_m, e_m = _twins("TSPModel", "categorical", dev)
    pts, ei = _tsp(dev, 200, 20, seed=60)
    _same(g_m.sample(pts, ei, generator=_gen(dev, 0)), e_m.sample(pts, ei, generator=_gen(dev, 0)))     # caches built
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    _same(g_m.sample(pts, ei, generator=_gen(dev, 1), graphed=True), e_m.sample(pts, ei, generator=_gen(dev, 1)))
    g_m._prep_cache.clear()
    g_m.model._tbias.clear()
    torch.cuda.empty_cache()
    _same(g_m.sample(pts, ei, generator=_gen(dev, 2), graphed=True), e_m.sample(pts, ei, generator=_gen(dev, 2)))
    assert g_m.graph_captures == 1 and g_m.graph_replays == 1
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(dev)
    g_m.clear_graphs()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated(dev)
    # the graph's static buffers, pool and capture-stream workspace are gone; the evicted caches were dropped as well
    assert after < held and after <= base + (1 << 20), (base, held, after)
    _same(g_m.sample(pts, ei, generator=_gen(dev, 3), graphed=True), e_m.sample(pts, ei, generator=_gen(dev, 3)))
    assert g_m.graph_captures == 2


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    pts, ei = _tsp(dev, 64, 8, seed=70)
    m, _ = _twins("TSPModel", "categorical", dev, gn_reduce=lambda t: None)
    with pytest.raises(ValueError, match="gn_reduce"):
        m.sample(pts, ei, graphed=True)
    m, _ = _twins("TSPModel", "categorical", dev, flags=_lib.FLAG_CHECK_FINITE)
    with pytest.raises(ValueError, match="FLAG_CHECK_FINITE"):
        m.sample(pts, ei, graphed=True)
    m, _ = _twins("TSPModel", "categorical", dev)
    m.prepare_graph(ei, 64, points=pts)
    scratch = torch.zeros(16, device=dev)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with pytest.raises(ValueError, match="capture"):
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            m.sample(pts, ei, graphed=True)
    assert m.graph_captures == 0 and m.model.calls == 0


# ---- 7. the pipeline -------------------------------------------------------------------------------------------------------
def test_solve_tsp_and_solve_mis_graphed_equal_eager(dev):
    from difusco_amd.pipeline import solve_mis, solve_tsp
    g_m, e_m = _twins("TSPModel", "categorical", dev)
    p, _ = tsp_instance(100, 1, seed=80)
    kw = dict(sparse_factor=20, parallel_sampling=2, sequential_sampling=2, two_opt_iterations=200)
    a = solve_tsp(g_m, p, generator=_gen(dev, 1), graphed=True, **kw)
    b = solve_tsp(e_m, p, generator=_gen(dev, 1), **kw)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
    assert g_m.graph_captures == 1 and g_m.graph_replays == 1

    # dense TSP-50 with P = 4
    g_m, e_m = _twins("TSPModel", "categorical", dev, sparse_factor=-1)
    p, _ = tsp_instance(50, 1, seed=82)
    kw = dict(sparse_factor=-1, parallel_sampling=4, sequential_sampling=2, two_opt_iterations=200)
    a = solve_tsp(g_m, p, generator=_gen(dev, 2), graphed=True, **kw)
    b = solve_tsp(e_m, p, generator=_gen(dev, 2), **kw)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]

    g_m, e_m = _twins("MISModel", "categorical", dev)
    n = 250
    ei = er_mis_edge_index(n, 0.03, seed=81)
    a = solve_mis(g_m, n, ei, generator=_gen(dev, 2), sequential_sampling=2, graphed=True)
    b = solve_mis(e_m, n, ei, generator=_gen(dev, 2), sequential_sampling=2)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    assert g_m.graph_captures == 1 and g_m.graph_replays == 1
