"""GPU parity where the MEAN of what a normalisation sees dwarfs its SPREAD (``-m gpu``).

The cases of tests/offset_statistics.py add a constant c in {16, 64, 256} to one bias vector: |mean| / sigma of a GroupNorm group of
the head reaches 40 .. 1200 (every other adversarial case of the suite leaves it at ~1), the rows of both LayerNorms get a mean of
3c.  A one-pass variance loses 2 log2(|mean| / sigma) bits.  Every statistics path runs: the sums the fused last layer leaves per
32-edge tile (default TSP engine; also what the two-phase shard sums are made of), gn_partial_tiled_kernel (no tail fold),
gn_partial_kernel at VEC 1, 2 and 4 (unfused, MIS), gn_partial_tiled_seg_kernel (dense mode, per-sample segments that are not tile
aligned), the LayerNorms of the fused kernel and wave_layer_norm.

The judge is the round-6 rule, unchanged (tests/graph_zoo.py ``calibrated``, tests/test_gpu_round6.py): with the fp32 oracle's own
distance from the float64 value as the yardstick.  tests/test_offset_statistics_host.py keeps that yardstick below 1e-4 for every
case here, and shows that one-pass fp32 tile sums fail this rule at c = 64 and c = 256.  Every case prints its three distances.
"""
import numpy as np
import pytest
import torch

from tests import offset_statistics as S
from tests.graph_zoo import calibrated

pytestmark = pytest.mark.gpu

T, TT = np.array([S.T_STEP]), np.array([S.T_TARGET])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _args(shape, diffusion):
    _, H, L, graph = S.SHAPES[shape]
    k = graph[2] if graph[0] == "knn" else -1
    return dict(diffusion_type=diffusion, diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=k, n_layers=L,
                hidden_dim=H, inference_trick="ddim")


def _engines():
    from difusco_amd import _lib
    return {"default": {}, "no_tail_fold": dict(flags=_lib.FLAG_NO_TAIL_FOLD),
            "no_folds": dict(flags=_lib.FLAG_NO_L0_FOLD | _lib.FLAG_NO_TAIL_FOLD), "unfused": dict(fused=False)}


def hip_step(dev, shape, diffusion, p, **kw):
    """One step of the shape's inputs on the GPU with parameters ``p`` -> (x, network output, prob or None), CPU tensors."""
    from difusco_amd import MISModel, TSPModel
    d = S.inputs(shape, diffusion)
    to = lambda t: None if t is None else t.to(dev)      # noqa: E731
    if S.SHAPES[shape][0] == "mis":
        m = MISModel(_args(shape, diffusion), p, device=dev, **kw)
        res = m.categorical_denoise_step(to(d["xt"]), T, dev, to(d["ei"]), target_t=TT, uniform=d["u"], return_aux=True)
    else:
        m = TSPModel(_args(shape, diffusion), p, device=dev, **kw)
        if diffusion == "categorical":
            res = m.categorical_denoise_step(to(d["points"]), to(d["xt"]), T, dev, to(d["ei"]), target_t=TT, uniform=d["u"],
                                             return_aux=True)
        else:
            res = m.gaussian_denoise_step(to(d["points"]), to(d["xt"]), T, dev, to(d["ei"]), target_t=TT, return_aux=True) + (None,)
    return tuple(None if r is None else r.cpu() for r in res)


def judge(label, res, ref, u):
    """The round-6 rule on one step: res = (x, out, prob) from the GPU, ref from offset_statistics.reference."""
    x, out, prob = res
    assert torch.isfinite(out).all() and torch.isfinite(x).all()
    e_hip_ref, e_ref_true, e_hip_true = S.distances(out, ref)
    print(f"{label}: HIP vs fp32 oracle {e_hip_ref:.2e}; fp32 oracle vs float64 {e_ref_true:.2e}; HIP vs float64 {e_hip_true:.2e}")
    bound = calibrated(S.CLASS_TOL, e_ref_true)
    assert e_hip_true < bound, (e_hip_true, e_ref_true)
    strict = e_ref_true < S.CLASS_TOL / 3      # the fp32 oracle is a usable arbiter at the class: direct comparison
    if strict:
        assert e_hip_ref < S.CLASS_TOL, e_hip_ref
    # tie band of the sampled bits = the bound that holds on |prob - ref_prob|.  strict: the class, asserted.  Otherwise
    # |out - ref_out| <= e_hip_true + e_ref_true < bound + e_ref_true, and the posterior probability moves by no more than the
    # logits do (the softmax of 2 classes has slope <= 1/4 in l1 - l0, the posterior is a convex combination of two probabilities)
    band = S.CLASS_TOL if strict else bound + e_ref_true
    if prob is not None:
        e_prob = (prob.reshape(-1) - ref["prob"].reshape(-1)).abs().max().item()
        assert e_prob < band, e_prob
        safe = (u.reshape(-1) - ref["prob"].reshape(-1)).abs() > band
        assert int(safe.sum()) > safe.numel() // 2
        assert torch.equal(x.reshape(-1)[safe], ref["x"].reshape(-1)[safe])
    elif strict:
        assert (x.reshape(-1) - ref["x"].reshape(-1)).abs().max().item() < S.CLASS_TOL
    return e_hip_ref, e_ref_true, e_hip_true


def _run(dev, case, engine="default", **kw):
    shape, diffusion, kind, c = case
    res = hip_step(dev, shape, diffusion, S.params(shape, kind, c, diffusion), **kw)
    return judge(f"{S.case_id(case)} [{engine}]", res, S.reference(shape, kind, c, diffusion), S.inputs(shape, diffusion)["u"])


@pytest.mark.parametrize("engine", ["default", "no_tail_fold", "no_folds", "unfused"])
@pytest.mark.parametrize("case", S.GRID_TSP60, ids=S.case_id)
def test_tsp_sparse(dev, case, engine):
    """600 edges = 19 tiles, the last one 24 of 32; H = 256, 2 layers; categorical and Gaussian; dead_group included (true
    variance 0, rstd = 1 / sqrt(eps): summation noise on the constant group must not be amplified)."""
    _run(dev, case, engine, **_engines()[engine])


@pytest.mark.parametrize("case", S.GRID_TSP150, ids=S.case_id)
def test_tsp_sparse_more_tiles(dev, case):
    """3,000 edges = 94 tiles: every block of the tile reduction adds several tiles."""
    _run(dev, case)


@pytest.mark.parametrize("case", S.GRID_NARROW, ids=S.case_id)
def test_narrow_widths_unfused(dev, case):
    """H = 64 and H = 128, 3 layers: gn_partial_kernel and wave_layer_norm at VEC 1 and 2."""
    _run(dev, case, "unfused", fused=False)


@pytest.mark.parametrize("case", S.GRID_DENSE, ids=S.case_id)
def test_dense_per_sample_statistics(dev, case):
    """B = 2, V = 14: statistic segments of 196 rows, not tile aligned (gn_partial_tiled_seg_kernel)."""
    _run(dev, case)


@pytest.mark.parametrize("engine", ["default", "unfused"])
@pytest.mark.parametrize("case", S.GRID_MIS, ids=S.case_id)
def test_mis(dev, case, engine):
    """er_mis_instance(120, 0.12): the head normalises node rows."""
    _run(dev, case, engine, **_engines()[engine])


@pytest.fixture(scope="module")
def other_precision_baseline(dev):
    """HIP vs float64 of the engines of another precision class WITHOUT an offset, once per precision."""
    cache = {}

    def get(precision):
        if precision not in cache:
            res = hip_step(dev, "tsp60", "categorical", S.params("tsp60", None, 0.0), precision=precision)
            cache[precision] = S.distances(res[1], S.reference("tsp60", None, 0.0))[2]
        return cache[precision]
    return get


@pytest.mark.parametrize("precision", ["bf16x3", "fp16x1"])
@pytest.mark.parametrize("c", S.OFFSETS)
def test_other_precisions_differential(dev, other_precision_baseline, precision, c):
    """bf16x3 / fp16x1: the GEMM error is not the subject.  last_out_bias touches only the last residual add and the head, so the
    offset may add no more than 4 x the fp32 oracle's own distance to what the engine shows without it."""
    e0 = other_precision_baseline(precision)
    res = hip_step(dev, "tsp60", "categorical", S.params("tsp60", "last_out_bias", c), precision=precision)
    assert torch.isfinite(res[1]).all()
    e_hip_ref, e_ref_true, e_hip_true = S.distances(res[1], S.reference("tsp60", "last_out_bias", c))
    print(f"tsp60 last_out_bias c = {c:g} [{precision}]: HIP vs fp32 oracle {e_hip_ref:.2e}; fp32 oracle vs float64 {e_ref_true:.2e}; "
          f"HIP vs float64 {e_hip_true:.2e} (without the offset {e0:.2e})")
    assert e_hip_true <= e0 + 4.0 * e_ref_true, (e_hip_true, e0, e_ref_true)


def test_shard_sums(dev):
    """Two-phase global statistics (gn_phase 1 / 2, the shard sums) on last_out_bias, c = 64: the batch of two graphs sharded over
    two "ranks" in this process (the all-reduce emulated by adding the partner's 65 doubles, as in
    test_gpu_parity.py::test_global_groupnorm_statistics_over_shards) against the oracle's single call over both graphs.  The
    sums that the fused last layer leaves per tile feed the shard sums too."""
    from difusco_amd import TSPModel
    from oracle import difusco_oracle as O
    shape, c, N, K = "tsp60", 64.0, 60, 10
    p = S.params(shape, "last_out_bias", c)
    insts = [O.tsp_instance(N, K, seed=70 + g) for g in range(2)]
    pts = torch.from_numpy(np.concatenate([i[0] for i in insts]))
    ei = torch.from_numpy(np.concatenate([i[1] + g * N for g, i in enumerate(insts)], axis=1))
    E1 = N * K
    gen = torch.Generator().manual_seed(5)
    xt = (torch.randn(2 * E1, generator=gen) > 0).float()
    u = torch.rand(2 * E1, generator=gen)
    ref = dict(zip(("x", "out", "prob"), O.tsp_categorical_denoise_step(p, O.CategoricalTables(), pts, xt, S.T_STEP, ei, S.T_TARGET,
                                                                       uniform=u, return_aux=True)))
    ref["truth"] = O.encoder_sparse_f64(p, pts, xt, torch.tensor([float(S.T_STEP)]), ei)
    shards = [(pts[r * N:(r + 1) * N].to(dev), (ei[:, r * E1:(r + 1) * E1] - r * N).to(dev), xt[r * E1:(r + 1) * E1].to(dev),
               u[r * E1:(r + 1) * E1]) for r in range(2)]
    sums = []
    for s_pts, s_ei, s_xt, s_u in shards:      # phase-1 pre-pass: this shard's sums
        grab = {}
        m = TSPModel(_args(shape, "categorical"), p, device=dev, gn_reduce=lambda s, grab=grab: grab.setdefault("s", s.clone()))
        m.categorical_denoise_step(s_pts, s_xt, T, dev, s_ei, target_t=TT, uniform=s_u)
        sums.append(grab["s"])
    assert sums[0][64].item() == E1
    xs, outs, probs = [], [], []
    for r, (s_pts, s_ei, s_xt, s_u) in enumerate(shards):
        other = sums[1 - r]
        m = TSPModel(_args(shape, "categorical"), p, device=dev, gn_reduce=lambda s, other=other: s.add_(other))
        x, out, prob = m.categorical_denoise_step(s_pts, s_xt, T, dev, s_ei, target_t=TT, uniform=s_u, return_aux=True)
        xs.append(x.cpu()), outs.append(out.cpu().reshape(E1, -1)), probs.append(prob.cpu().reshape(-1))
    judge("two shards of tsp60, last_out_bias c = 64 [default, global statistics]", (torch.cat(xs), torch.cat(outs), torch.cat(probs)),
          ref, u)
