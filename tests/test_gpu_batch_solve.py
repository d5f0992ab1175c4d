"""Batched instances on the GPU (ABI 13): per-instance random streams (DIFUSCO_RAND_PHILOX_INSTANCES), one head statistic
segment per instance, ``sample_batch``, the grouped 2-opt and ``solve_*_batch`` - every instance of a batch gets what its
solo call gets."""
import glob
import os

import numpy as np
import pytest
import torch

from difusco_amd import _lib
from difusco_amd.graph import build_csr, build_union_csr
from oracle import difusco_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIE = 1e-5        # the tie band of test_gpu_parity.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _args(diffusion, sparse_factor, hidden, steps=5, trick="ddim"):
    return dict(diffusion_type=diffusion, diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=2, hidden_dim=hidden, inference_trick=trick, inference_diffusion_steps=steps,
                inference_schedule="cosine")


def _model(cls, diffusion, hidden, dev, seed, backend=None, sparse_factor=8, trick="ddim", steps=5):
    from difusco_amd.engine import DenoiseEngine
    p = O.init_params(hidden, 2, 2 if diffusion == "categorical" else 1, seed=0)
    eng = DenoiseEngine(p, device=dev, backend=backend)
    return cls(_args(diffusion, sparse_factor, hidden, steps, trick), engine=eng, seed=seed)


def _tsp(sizes, k, seed0=20):
    out = []
    for i, n in enumerate(sizes):
        p, ei = O.tsp_instance(n, k, seed=seed0 + i)
        out.append((torch.from_numpy(p), torch.from_numpy(ei)))
    return out


def _mis(sizes, seed0=30):
    from difusco_amd.synthetic import er_mis_edge_index
    return [(n, torch.from_numpy(er_mis_edge_index(n, 0.08, seed=seed0 + i))) for i, n in enumerate(sizes)]


def _instances(dev, rows, seeds):
    return (torch.as_tensor(np.asarray(rows, dtype=np.int64)).to(dev), torch.tensor(seeds, dtype=torch.int64).to(dev))


def _assert_bits_off_ties(out_a, prob_a, out_b, prob_b):
    """Both sides draw the same uniform u per row (test_batched_draws_equal_solo_draws): a bit can differ only where u lies
    between the two probabilities - inside the tie band |u - p| <= |p_a - p_b| < 1e-5 - and then it is 1 on the side whose
    probability is larger."""
    diff = out_a != out_b
    pa, pb = prob_a.clamp(0, 1)[diff], prob_b.clamp(0, 1)[diff]
    assert bool(((pa - pb).abs() < TIE).all()) and bool(((out_a[diff] == 1) == (pa > pb)).all())
    assert int(diff.sum()) <= max(2, out_a.numel() // 1000)


def _one_step(m, g, task, pts, xt, instances=None):
    """One categorical / Gaussian step of model m at t = 500 -> 450 with return_aux, offset 0."""
    m.model.calls = 0
    if m.diffusion_type == "categorical":
        return m._categorical(g, task, pts, xt, 500, 450, None, True, instances=instances)
    return m._gaussian(g, task, pts, xt, 500, 450, None, True, instances=instances)


# ---- per-instance random streams -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["ctypes", "torch"])
@pytest.mark.parametrize("diffusion,trick", [("categorical", "ddim"), ("gaussian", None)])
@pytest.mark.parametrize("task,hidden", [("tsp", 256), ("tsp", 64), ("mis", 64)])
def test_one_instance_mode3_equals_mode2(dev, backend, diffusion, trick, task, hidden):
    """Mode 3 with one instance whose seed is the call's seed draws exactly what mode 2 draws: bit-identical step."""
    from difusco_amd import MISModel, TSPModel
    seed = 1234567
    if task == "tsp":
        m = _model(TSPModel, diffusion, hidden, dev, seed, backend, trick=trick)
        pts, ei = _tsp([96], 8)[0]
        g = build_csr(ei, 96, dev, points=pts)
        pts, tk, rows = pts.to(dev), _lib.TASK_TSP, ei.shape[1]
    else:
        m = _model(MISModel, diffusion, hidden, dev, seed, backend, trick=trick)
        n, ei = _mis([150])[0]
        g, pts, tk, rows = build_csr(ei, n, dev), None, _lib.TASK_MIS, n
    xt = torch.randn(rows, generator=torch.Generator().manual_seed(3)).to(dev)
    if diffusion == "categorical":
        xt = (xt > 0).float()
    a = _one_step(m, g, tk, pts, xt)
    b = _one_step(m, g, tk, pts, xt, _instances(dev, [0, rows], [seed]))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = _one_step(m, g, tk, pts, xt, _instances(dev, [0, rows], [seed + 1]))     # the instance seed is what keys the draw
    assert not torch.equal(a[0], c[0])


def _union_and_solo(dev, task, sizes, k=8):
    """(union graph, union points, instance rows, [(solo graph, solo points)]) of instances of different sizes."""
    if task == "tsp":
        inst = _tsp(sizes, k)
        g, _, rows = build_union_csr([e for _, e in inst], [p.shape[0] for p, _ in inst], dev,
                                     points=torch.cat([p for p, _ in inst]))
        solo = [(build_csr(e, p.shape[0], dev, points=p), p.to(dev)) for p, e in inst]
        return g, torch.cat([p for p, _ in inst]).to(dev), rows, solo
    inst = _mis(sizes)
    g, _, rows = build_union_csr([e for _, e in inst], [n for n, _ in inst], dev, task_rows="nodes")
    return g, None, rows, [(build_csr(e, n, dev), None) for n, e in inst]


@pytest.mark.parametrize("backend", ["ctypes", "torch"])
@pytest.mark.parametrize("task,hidden", [("tsp", 256), ("tsp", 64), ("mis", 64)])
def test_batched_draws_equal_solo_draws(dev, backend, task, hidden):
    """x_s = x_t + z (post = {1, 0, 0, 1, DDPM}) with x_t = 0 exposes the normals of a step: every instance of a batch draws
    bit for bit what its solo call with its own seed draws."""
    from difusco_amd.engine import DenoiseEngine
    eng = DenoiseEngine(O.init_params(hidden, 2, 1, seed=0), device=dev, backend=backend)
    sizes = [70, 130, 45, 100] if task == "tsp" else [120, 300, 80]
    g, pts, rows, solo = _union_and_solo(dev, task, sizes)
    tk = _lib.TASK_TSP if task == "tsp" else _lib.TASK_MIS
    seeds = [11, 2 ** 62 + 5, 7, 11][:len(sizes)]
    post = np.array([1, 0, 0, 1, 1, 0, 0, 0], np.float32)
    z, _, _ = eng.step(g, tk, _lib.GAUSSIAN, torch.zeros(int(rows[-1]), device=dev), 500.0, post, points=pts, seed=99,
                       offset=17, instances=_instances(dev, rows, seeds))
    for b, (gs, ps) in enumerate(solo):
        zs, _, _ = eng.step(gs, tk, _lib.GAUSSIAN, torch.zeros(int(rows[b + 1] - rows[b]), device=dev), 500.0, post,
                            points=ps, seed=seeds[b], offset=17)
        assert torch.equal(z[int(rows[b]):int(rows[b + 1])], zs), b
    if task == "tsp":      # the streams are per instance and local: instances 0 and 3 share seed 11, instance 2 has its own
        n0 = int(rows[3] - rows[2])
        assert torch.equal(z[:n0], z[int(rows[3]):int(rows[3]) + n0])
        assert not torch.equal(z[:n0], z[int(rows[2]):int(rows[3])])


@pytest.mark.parametrize("task,hidden", [("tsp", 256), ("tsp", 64), ("mis", 64)])
def test_batched_step_matches_solo_steps(dev, task, hidden):
    """A categorical step over 3-4 instances: per instance, logits and probabilities within the 1e-5 class of its solo step,
    sampled bits identical outside the tie band; with ONE statistic segment for the whole union the logits measurably differ."""
    from difusco_amd import MISModel, TSPModel
    sizes = [70, 130, 45, 100] if task == "tsp" else [120, 300, 80]
    g, pts, rows, solo = _union_and_solo(dev, task, sizes)
    tk = _lib.TASK_TSP if task == "tsp" else _lib.TASK_MIS
    seeds = [5, 6, 7, 8][:len(sizes)]
    xt = (torch.randn(int(rows[-1]), generator=torch.Generator().manual_seed(4)) > 0).float().to(dev)
    models = [_model(TSPModel if task == "tsp" else MISModel, "categorical", hidden, dev, s) for s in seeds]
    out, logits, prob = _one_step(models[0], g, tk, pts, xt, _instances(dev, rows, seeds))
    worst = 0.0
    for b, (gs, ps) in enumerate(solo):
        sl = slice(int(rows[b]), int(rows[b + 1]))
        o_s, l_s, p_s = _one_step(models[b], gs, tk, ps, xt[sl])
        e_l = (logits[sl] - l_s).abs().max().item()
        e_p = (prob[sl] - p_s).abs().max().item()
        assert e_l < 1e-5 and e_p < 1e-5, (b, e_l, e_p)
        worst = max(worst, e_l)
        _assert_bits_off_ties(out[sl], prob[sl], o_s, p_s)
    # one statistic segment over all instances (what a plain concatenation would do): measurably different logits
    seg_ptr, n_seg = g.seg_ptr, g.n_segments
    g.seg_ptr, g.n_segments = None, 1
    try:
        _, l1, _ = _one_step(models[0], g, tk, pts, xt, _instances(dev, rows, seeds))
    finally:
        g.seg_ptr, g.n_segments = seg_ptr, n_seg
    assert (l1 - logits).abs().max().item() > 100 * max(worst, 1e-7)


# ---- sample_batch ----------------------------------------------------------------------------------------------------------
def _heat_equal(a, b):
    """The last categorical step returns probabilities (no draw, target_t = 0): equal to the 1e-5 class of a step; a sampled bit
    of an earlier step flipped inside the tie band would show as an isolated larger difference."""
    assert a.shape == b.shape
    d = (a - b).abs()
    assert int((d > 1e-5).sum()) <= max(2, a.numel() // 1000), (int((d > 1e-5).sum()), d.max().item())


@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_tsp_sample_batch_matches_solo_sample(dev, mode):
    from difusco_amd import TSPModel
    seeds, P = [3, 4, 5], 2
    sizes = [60, 90, 75] if mode == "sparse" else [50, 50, 50]
    inst = _tsp(sizes, 8)
    k = 8 if mode == "sparse" else -1
    pts_rep, ei_rep = [], []
    for p, e in inst:
        n = p.shape[0]
        if mode == "sparse":
            pts_rep.append(p.repeat(P, 1).to(dev))
            ei_rep.append((e.reshape(2, 1, -1) + torch.arange(P).view(1, -1, 1) * n).reshape(2, -1).to(dev))
        else:
            pts_rep.append(p.reshape(1, n, 2).repeat(P, 1, 1).to(dev))
    gens = [torch.Generator().manual_seed(100 + b) for b in range(3)]
    mb = _model(TSPModel, "categorical", 256, dev, 0, sparse_factor=k)
    heats = mb.sample_batch(pts_rep, ei_rep if mode == "sparse" else None, seeds=seeds, generators=gens)
    for b in range(3):
        ms = _model(TSPModel, "categorical", 256, dev, seeds[b], sparse_factor=k)      # fresh engine: the same offsets
        hs = ms.sample(pts_rep[b], ei_rep[b] if mode == "sparse" else None, generator=torch.Generator().manual_seed(100 + b))
        _heat_equal(heats[b], hs)


def test_mis_sample_batch_matches_solo_sample(dev):
    from difusco_amd import MISModel
    inst = _mis([150, 260, 90])
    seeds = [9, 10, 11]
    mb = _model(MISModel, "categorical", 64, dev, 0)
    xt0 = [torch.randn(n, generator=torch.Generator().manual_seed(7 + b)) for b, (n, _) in enumerate(inst)]
    heats = mb.sample_batch([n for n, _ in inst], [e.to(dev) for _, e in inst], seeds=seeds, xt0=xt0)
    for b, (n, e) in enumerate(inst):
        ms = _model(MISModel, "categorical", 64, dev, seeds[b])
        _heat_equal(heats[b], ms.sample(n, e.to(dev), xt0=xt0[b]))


def test_sample_batch_refuses_global_statistics_with_several_instances(dev):
    from difusco_amd import MISModel
    inst = _mis([40, 50])
    m = _model(MISModel, "categorical", 64, dev, 0)
    m.gn_reduce = lambda t: None
    with pytest.raises(ValueError, match="gn_reduce"):
        m.sample_batch([n for n, _ in inst], [e.to(dev) for _, e in inst])


# ---- grouped 2-opt ---------------------------------------------------------------------------------------------------------
def _random_tours(rng, G, P, n):
    t = np.stack([np.concatenate([[0], 1 + rng.permutation(n - 1), [0]]) for _ in range(G * P)])
    return t.astype(np.int64)


@pytest.mark.parametrize("max_it", [1000, 7, 0])
def test_grouped_two_opt_equals_per_group_two_opt(dev, max_it):
    from difusco_amd.decode import batched_two_opt_grouped, batched_two_opt_torch
    rng = np.random.default_rng(5)
    G, P, n = 4, 3, 60
    pts = rng.random((G, n, 2))
    tours = _random_tours(rng, G, P, n)
    # group 1 starts from converged tours: it stops at once while the others go on
    tours[P:2 * P], _ = batched_two_opt_torch(pts[1], tours[P:2 * P], max_iterations=1000, device=dev)
    out, its = batched_two_opt_grouped(pts, tours, max_iterations=max_it, device=dev)
    for g in range(G):
        ref, ref_it = batched_two_opt_torch(pts[g], tours[g * P:(g + 1) * P], max_iterations=max_it, device=dev)
        assert np.array_equal(out[g * P:(g + 1) * P], ref), g
        assert its[g] == ref_it, (g, its[g], ref_it)
    if max_it == 1000:
        assert its[1] == 0 and len(set(its.tolist())) > 1
    if max_it == 7:
        assert its.max() == 7


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "tsp_twoopt_*.npz"))),
                         ids=lambda p: os.path.basename(p)[11:-4])
def test_grouped_two_opt_matches_reference_fixture(dev, path):
    from difusco_amd.decode import batched_two_opt_grouped
    z = np.load(path)
    P = z["tours_in"].shape[0]
    pts = np.stack([z["points"]] * 3)
    tours = np.concatenate([z["tours_in"]] * 3)
    out, its = batched_two_opt_grouped(pts, tours, max_iterations=int(z["max_iterations"]), device=dev)
    for g in range(3):
        assert np.array_equal(out[g * P:(g + 1) * P], z["tours_out"]) and its[g] == int(z["iterations"])


# ---- decode and pipelines --------------------------------------------------------------------------------------------------
def test_mis_union_decode_equals_per_instance_decode(dev):
    from difusco_amd.decode import mis_decode_np
    inst = _mis([100, 230, 60, 180])
    scores = [torch.rand(n, generator=torch.Generator().manual_seed(b)) for b, (n, _) in enumerate(inst)]
    g, _, rows = build_union_csr([e for _, e in inst], [n for n, _ in inst], dev, task_rows="nodes")
    sol = mis_decode_np(torch.cat(scores), graph=g, device=dev)
    for b, (n, e) in enumerate(inst):
        assert np.array_equal(sol[int(rows[b]):int(rows[b + 1])], mis_decode_np(scores[b], edge_index=e, device=dev)), b


@pytest.mark.parametrize("sparse_factor", [8, -1])
def test_solve_tsp_batch_matches_solo(dev, sparse_factor):
    from difusco_amd import TSPModel
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    B, n, P = 3, 50, 2
    pts = np.random.default_rng(12).random((B, n, 2))
    seeds = [21, 22, 23]
    mb = _model(TSPModel, "categorical", 256, dev, 0, sparse_factor=sparse_factor)
    timings = {}
    res = solve_tsp_batch(mb, pts, sparse_factor, parallel_sampling=P, sequential_sampling=2, two_opt_iterations=100,
                          seeds=seeds, generators=[torch.Generator().manual_seed(b) for b in range(B)], timings=timings)
    assert set(timings) >= {"sampling", "merge", "two_opt"}
    for b in range(B):
        ms = _model(TSPModel, "categorical", 256, dev, seeds[b], sparse_factor=sparse_factor)
        tour, cost, costs, info = solve_tsp(ms, pts[b], sparse_factor, parallel_sampling=P, sequential_sampling=2,
                                            two_opt_iterations=100, generator=torch.Generator().manual_seed(b))
        assert res[b][0] == tour and res[b][1] == cost and res[b][2] == costs, b
        assert res[b][3]["merged_costs"] == info["merged_costs"] and res[b][3]["two_opt_iterations"] == info["two_opt_iterations"]


def test_solve_mis_batch_matches_solo(dev):
    from difusco_amd import MISModel
    from difusco_amd.pipeline import solve_mis, solve_mis_batch
    inst = _mis([120, 200, 90])
    seeds = [31, 32, 33]
    mb = _model(MISModel, "categorical", 64, dev, 0)
    res = solve_mis_batch(mb, [(n, e.numpy()) for n, e in inst], parallel_sampling=2, sequential_sampling=2, seeds=seeds,
                          generators=[torch.Generator().manual_seed(b) for b in range(3)])
    for b, (n, e) in enumerate(inst):
        ms = _model(MISModel, "categorical", 64, dev, seeds[b])
        sol, size, sizes = solve_mis(ms, n, e.numpy(), parallel_sampling=2, sequential_sampling=2,
                                     generator=torch.Generator().manual_seed(b))
        assert np.array_equal(res[b][0], sol) and res[b][1] == size and res[b][2] == sizes, b

