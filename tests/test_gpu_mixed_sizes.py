"""TSP instances of different sizes in one batched call: the ragged 2-opt (``difusco_tsp_two_opt_ragged``), the ragged k-NN,
dense ``sample_batch`` with mixed n, the list form of ``solve_tsp_batch`` and ``evaluate --mixed_size_chunks``.  Every instance
must get what its solo call gets.  Models: 2 layers, 5 steps, hidden 64 / 256, as tests/test_gpu_batch_solve.py."""
import os

import numpy as np
import pytest
import torch

from difusco_amd import _lib
from difusco_amd import evaluate as E
from oracle import difusco_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ["exact", "screened"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _model(dev, hidden, seed, sparse_factor):
    from difusco_amd import TSPModel
    from difusco_amd.engine import DenoiseEngine
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=2, hidden_dim=hidden, inference_trick="ddim", inference_diffusion_steps=5, inference_schedule="cosine")
    return TSPModel(args, engine=DenoiseEngine(O.init_params(hidden, 2, 2, seed=0), device=dev), seed=seed)


def _heat_equal(a, b):
    """The rule of tests/test_gpu_batch_solve.py: the last categorical step returns probabilities, equal to the 1e-5 class of a
    step; a sampled bit of an earlier step flipped inside the tie band shows as an isolated larger difference, so at most
    max(2, numel // 1000) entries may differ by more than 1e-5."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape
    d = (a - b).abs()
    assert int((d > 1e-5).sum()) <= max(2, a.numel() // 1000), (int((d > 1e-5).sum()), d.max().item())


def _random_tours(rng, P, n):
    return np.stack([np.concatenate([[0], 1 + rng.permutation(n - 1), [0]]) for _ in range(P)]).astype(np.int64)


def _pairs(n):
    return (n - 1) * (n - 2) // 2


# ---- 1. reference fixtures, ragged ------------------------------------------------------------------------------------------
def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"tsp_twoopt_{name}.npz"))


@pytest.mark.parametrize("method", METHODS)
def test_ragged_two_opt_matches_reference_fixtures_in_one_call(dev, method):
    from difusco_amd.decode import batched_two_opt_ragged
    zs = [_fixture(n) for n in ("n120_merge_b3", "n300_merge", "n40_converged", "n50_random")]
    assert [z["tours_in"].shape[0] for z in zs] == [3, 1, 1, 1]
    out, its = batched_two_opt_ragged([z["points"] for z in zs], [z["tours_in"] for z in zs], max_iterations=1000, device=dev,
                                      method=method)
    assert its.tolist() == [29, 64, 0, 48] == [int(z["iterations"]) for z in zs]
    for g, z in enumerate(zs):
        assert out[g].dtype == np.int64 and np.array_equal(out[g], z["tours_out"]), g


@pytest.mark.parametrize("method", METHODS)
def test_ragged_two_opt_cap_5_over_all_fixtures(dev, method):
    from difusco_amd.decode import batched_two_opt_ragged, batched_two_opt_torch
    names = ("n120_merge_b3", "n200_cap5_b2", "n300_merge", "n40_converged", "n50_random")
    zs = [_fixture(n) for n in names]
    out, its = batched_two_opt_ragged([z["points"] for z in zs], [z["tours_in"] for z in zs], max_iterations=5, device=dev,
                                      method=method)
    assert int(zs[1]["max_iterations"]) == 5 and its[1] == 5 == int(zs[1]["iterations"])
    assert np.array_equal(out[1], zs[1]["tours_out"])
    for g, z in enumerate(zs):
        ref, ref_it = batched_two_opt_torch(z["points"], z["tours_in"], max_iterations=5, device=dev)
        assert np.array_equal(out[g], ref) and its[g] == ref_it, names[g]


# ---- 2. ragged equals solo at the sizes where indexing can break ------------------------------------------------------------
SIZES, TOURS, CONVERGED = [4, 5, 16, 17, 33, 60], [1, 3, 2, 1, 2, 3], 4


@pytest.fixture(scope="module")
def small_groups(dev):
    """Random points and random-permutation tours; group CONVERGED starts from converged tours.  Shared, never modified."""
    from difusco_amd.decode import batched_two_opt_torch
    rng = np.random.default_rng(11)
    pts = [rng.random((n, 2)) for n in SIZES]
    tours = [_random_tours(rng, P, n) for n, P in zip(SIZES, TOURS)]
    tours[CONVERGED], _ = batched_two_opt_torch(pts[CONVERGED], tours[CONVERGED], max_iterations=1000, device=dev)
    return pts, tours


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("max_it", [1000, 7, 0])
def test_ragged_two_opt_equals_per_group_two_opt(dev, small_groups, max_it, method):
    from difusco_amd.decode import batched_two_opt_ragged, batched_two_opt_torch
    pts, tours = small_groups
    out, its = batched_two_opt_ragged(pts, tours, max_iterations=max_it, device=dev, method=method)
    assert its.dtype == np.int64 and its.shape == (len(SIZES),)
    for g in range(len(SIZES)):
        ref, ref_it = batched_two_opt_torch(pts[g], tours[g], max_iterations=max_it, device=dev)
        assert out[g].shape == (TOURS[g], SIZES[g] + 1) and np.array_equal(out[g], ref), g
        assert its[g] == ref_it, (g, its.tolist(), ref_it)
    assert its[CONVERGED] == 0                                   # it stops at once while the others go on
    assert len(set(its.tolist())) > 1
    if max_it == 7:
        assert its.max() == 7


# ---- 3. chunk boundary of the screen ----------------------------------------------------------------------------------------
BIG_SIZES, BIG_TOURS, BIG_CAP = [1023, 5, 1025, 1027], [1, 2, 1, 2], 30


@pytest.fixture(scope="module")
def big_groups(dev):
    """Groups on both sides of the 1024-column chunk of the screen, with the exact per-group reference.  Shared, never modified."""
    from difusco_amd.decode import batched_two_opt_torch
    rng = np.random.default_rng(12)
    pts = [rng.random((n, 2)) for n in BIG_SIZES]
    tours = [_random_tours(rng, P, n) for n, P in zip(BIG_SIZES, BIG_TOURS)]
    ref = [batched_two_opt_torch(p, t, max_iterations=BIG_CAP, device=dev) for p, t in zip(pts, tours)]
    return pts, tours, ref


def test_ragged_screen_across_the_chunk_boundary(dev, big_groups):
    from difusco_amd.decode import batched_two_opt_ragged
    pts, tours, ref = big_groups
    stats = {}
    out, its = batched_two_opt_ragged(pts, tours, max_iterations=BIG_CAP, device=dev, method="screened", stats=stats)
    for g, (r, r_it) in enumerate(ref):
        assert np.array_equal(out[g], r) and its[g] == r_it, g
    # every applied move of a group is one sweep over P_g (n_g - 1)(n_g - 2) / 2 pairs; the exact path evaluates all of them
    swept = sum(int(its[g]) * BIG_TOURS[g] * _pairs(BIG_SIZES[g]) for g in range(len(BIG_SIZES)))
    print("exact_pairs", stats["exact_pairs"], "of", swept, "=", stats["exact_pairs"] / swept)
    assert its.max() == BIG_CAP and 0 < stats["exact_pairs"] < 0.01 * swept


def test_ragged_screen_without_a_bound_in_one_group_runs_the_exact_sweep(dev, big_groups):
    from difusco_amd.decode import batched_two_opt_ragged, batched_two_opt_torch, two_opt_screen_bound
    pts, tours, ref = big_groups
    rng = np.random.default_rng(13)
    far = (rng.integers(0, 2, (9, 2)) * 2.0 - 1.0) * 2.0 ** 70 * (1 + rng.random((9, 2)) / 4)
    far[0, 0] = 2.0 ** 70
    assert two_opt_screen_bound(np.abs(far).max()) is None
    far_tours = _random_tours(rng, 2, 9)
    far_ref, far_it = batched_two_opt_torch(far, far_tours, max_iterations=BIG_CAP, device=dev)
    stats = {}
    out, its = batched_two_opt_ragged(pts[:2] + [far] + pts[2:], tours[:2] + [far_tours] + tours[2:], max_iterations=BIG_CAP,
                                      device=dev, method="screened", stats=stats)
    refs = ref[:2] + [(far_ref, far_it)] + ref[2:]
    sizes, P = BIG_SIZES[:2] + [9] + BIG_SIZES[2:], BIG_TOURS[:2] + [2] + BIG_TOURS[2:]
    for g, (r, r_it) in enumerate(refs):
        assert np.array_equal(out[g], r) and its[g] == r_it, g
    sweeps = [int(i) + 1 if int(i) < BIG_CAP else int(i) for i in its]           # + the sweep that finds nothing to apply
    assert stats["exact_pairs"] == sum(s * p * _pairs(n) for s, p, n in zip(sweeps, P, sizes))


# ---- 4. ragged k-NN ---------------------------------------------------------------------------------------------------------
def test_ragged_knn_equals_solo_knn_plus_offset(dev):
    from difusco_amd.graph import knn_edge_index_gpu
    k = 10
    pts = [np.load(os.path.join(GOLDEN, "knn_n50_k10.npz"))["points"], np.random.default_rng(3).random((64, 2)),
           np.load(os.path.join(GOLDEN, "knn_n700_k40.npz"))["points"]]
    sizes = [p.shape[0] for p in pts]
    assert sizes == [50, 64, 700]
    ei = knn_edge_index_gpu(np.concatenate(pts), k, device=dev, sizes=sizes)
    assert ei.shape == (2, sum(sizes) * k) and ei.dtype == torch.int64
    node, col = 0, 0
    for p in pts:
        solo = knn_edge_index_gpu(p, k, device=dev)
        assert torch.equal(ei[:, col:col + p.shape[0] * k], solo + node)
        node, col = node + p.shape[0], col + p.shape[0] * k
    # `graphs=` keeps its meaning
    two = np.concatenate([pts[0], pts[0][::-1]])
    assert torch.equal(knn_edge_index_gpu(two, k, device=dev, graphs=2), knn_edge_index_gpu(two, k, device=dev, sizes=[50, 50]))
    with pytest.raises(ValueError, match="instance 1"):
        knn_edge_index_gpu(np.concatenate([pts[0], pts[1][:8]]), k, device=dev, sizes=[50, 8])


# ---- 5. dense mixed sampling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [256, 64])
def test_dense_sample_batch_of_mixed_sizes_matches_solo_sample(dev, hidden):
    sizes, P, seeds = [20, 50, 33], [2, 1, 2], [3, 4, 5]
    rng = np.random.default_rng(21)
    pts = [torch.from_numpy(rng.random((n, 2)).astype(np.float32)).reshape(1, n, 2).repeat(p, 1, 1).to(dev)
           for n, p in zip(sizes, P)]
    mb = _model(dev, hidden, 0, -1)
    heats = mb.sample_batch(pts, None, seeds=seeds, generators=[torch.Generator().manual_seed(100 + b) for b in range(3)])
    assert ("dense_union", (20, 20, 50, 33, 33)) in mb._graph_cache
    for b in range(3):
        assert heats[b].shape == (P[b], sizes[b], sizes[b])
        ms = _model(dev, hidden, seeds[b], -1)                   # fresh engine: the same offsets
        _heat_equal(heats[b], ms.sample(pts[b], None, generator=torch.Generator().manual_seed(100 + b)))


def test_dense_union_of_equal_sizes_is_todays_dense_batch(dev):
    from difusco_amd.graph import complete_graph_batch, complete_graph_union
    a, b = complete_graph_union([50, 50, 50], dev), complete_graph_batch(3, 50, dev)
    for k in ("rowptr", "col", "row", "seg_ptr"):
        assert getattr(a, k).dtype == getattr(b, k).dtype and torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.perm is None and b.perm is None and (a.n_nodes, a.n_edges, a.n_segments) == (b.n_nodes, b.n_edges, b.n_segments)
    m = _model(dev, 256, 7, -1)
    assert m._dense_union_graph([50, 50, 50]) is m._dense_graph(3, 50)      # equal n keeps today's key and graph
    pts = torch.rand((150, 2), generator=torch.Generator().manual_seed(1)).to(dev)
    xt = (torch.randn(3 * 50 * 50, generator=torch.Generator().manual_seed(2)) > 0).float().to(dev)
    steps = []
    for g in (a, b):                                             # one step at t = 500 -> 450, offset 0, on each graph
        m.model.calls = 0
        steps.append(m._categorical(g, _lib.TASK_TSP, pts, xt, 500, 450, None, True))
    for x, y in zip(*steps):
        assert torch.equal(x, y)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", [8, -1], ids=["sparse", "dense"])
def test_solve_tsp_batch_of_mixed_sizes(dev, K, method):
    from difusco_amd.decode import batched_two_opt_torch, merge_tours
    from difusco_amd.graph import knn_edge_index_gpu
    from difusco_amd.pipeline import solve_tsp_batch, tour_length
    sizes, P, S, cap, seeds = [30, 50, 41], 2, 2, 100, [21, 22, 23]
    rng = np.random.default_rng(31)
    pts = [rng.random((n, 2)) for n in sizes]
    heatmaps, timings = [], {}
    res = solve_tsp_batch(_model(dev, 256, 0, K), pts, K, parallel_sampling=P, sequential_sampling=S, two_opt_iterations=cap,
                          seeds=seeds, generators=[torch.Generator().manual_seed(b) for b in range(3)], timings=timings,
                          heatmaps=heatmaps, two_opt_method=method)
    assert len(res) == len(heatmaps) == 3 and set(timings) >= {"knn", "sampling", "merge", "two_opt"}
    for b, n in enumerate(sizes):
        pts32 = torch.from_numpy(pts[b].astype(np.float32)).to(dev)
        p64 = pts32.cpu().numpy().astype(np.float64)
        ei = knn_edge_index_gpu(pts[b], K, device=dev) if K > 0 else None
        # (i) the heatmaps are those of the solo sample chain
        ms, gen = _model(dev, 256, seeds[b], K), torch.Generator().manual_seed(b)
        pts_rep = pts32.repeat(P, 1) if K > 0 else pts32.reshape(1, n, 2).repeat(P, 1, 1)
        ei_rep = ms.duplicate_edge_index(ei, n, dev, copies=P) if K > 0 else None
        assert len(heatmaps[b]) == S
        for r in range(S):
            _heat_equal(heatmaps[b][r], ms.sample(pts_rep, ei_rep, generator=gen).cpu())
        # (ii) the decode of the batch's own heatmaps, solo: deterministic, so exactly the batch's answer
        solved, merged_costs = [], []
        for r in range(S):
            tours, merge_it = merge_tours(heatmaps[b][r], pts32, ei, sparse_graph=K > 0, parallel_sampling=P, device=dev)
            sol, ns = batched_two_opt_torch(p64, np.asarray(tours, dtype=np.int64), max_iterations=cap, device=dev)
            solved.append(sol)
            merged_costs += [tour_length(p64, t) for t in tours]
        solved = np.concatenate(solved)
        costs = [tour_length(p64, t) for t in solved]
        best = int(np.argmin(costs))
        tour, cost, all_costs, info = res[b]
        assert tour == solved[best].tolist() and cost == costs[best] and all_costs == costs, b
        assert info == {"merge_iterations": merge_it, "two_opt_iterations": ns, "merged_costs": merged_costs}, b


@pytest.mark.parametrize("K", [8, -1], ids=["sparse", "dense"])
def test_solve_tsp_batch_array_form_equals_list_form(dev, K):
    from difusco_amd.pipeline import solve_tsp_batch
    pts = np.random.default_rng(32).random((3, 40, 2))
    runs = []
    for form in (pts, [p for p in pts]):
        heat = []
        res = solve_tsp_batch(_model(dev, 64, 0, K), form, K, parallel_sampling=2, sequential_sampling=2, two_opt_iterations=100,
                              seeds=[5, 6, 7], generators=[torch.Generator().manual_seed(b) for b in range(3)], heatmaps=heat)
        runs.append((res, heat))
    assert runs[0][0] == runs[1][0]
    for ha, hb in zip(runs[0][1], runs[1][1]):
        assert all(np.array_equal(x, y) for x, y in zip(ha, hb))


# ---- 7. evaluation ----------------------------------------------------------------------------------------------------------
EVAL_SIZES = [20, 30] * 6


def _write_split(path, sizes, seed):
    rng = np.random.default_rng(seed)
    lines = []
    for n in sizes:
        pts, perm = rng.random((n, 2)), rng.permutation(n)
        tour = np.concatenate([perm, perm[:1]]) + 1
        lines.append(" ".join(str(float(v)) for v in pts.reshape(-1)) + " output " + " ".join(str(int(t)) for t in tour))
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _checkpoint(path):
    from difusco_amd.synthetic import random_state_dict
    sd = random_state_dict(64, 2, 2, seed=0)
    torch.save({"epoch": 0, "global_step": 0, "state_dict": {"model." + k: v for k, v in sd.items()}, "optimizer_states": [],
                "lr_schedulers": []}, path)
    return str(path), sd


def test_evaluate_mixed_size_chunks(dev, tmp_path):
    from difusco_amd import TSPModel
    from difusco_amd.datasets import read_tsp_split
    split = _write_split(tmp_path / "tsp.txt", EVAL_SIZES, seed=4)
    ckpt, sd = _checkpoint(tmp_path / "last.ckpt")
    argv = ["--task", "tsp", "--do_test", "--do_valid_only", "--diffusion_type", "categorical", "--storage_path", str(tmp_path),
            "--validation_split", split, "--test_split", split, "--validation_examples", "12", "--inference_schedule", "cosine",
            "--inference_diffusion_steps", "5", "--ckpt_path", ckpt, "--hidden_dim", "64", "--n_layers", "2", "--sparse_factor", "8",
            "--parallel_sampling", "2", "--two_opt_iterations", "100"]
    lines_off, recs_off = E.run(argv)
    lines_on, recs_on = E.run(argv + ["--mixed_size_chunks"])
    lines_one, recs_one = E.run(argv + ["--mixed_size_chunks", "--instances_per_call", "1"])
    (test_off,), (test_on,), (test_one,) = lines_off, lines_on, lines_one
    # N alternates: runs of equal N are single instances, a mixed run takes the whole split
    assert test_off["chunks"] == 12 and "mixed_size_chunks" not in test_off
    assert test_on["chunks"] == 1 < test_off["chunks"] and test_on["mixed_size_chunks"] is True and test_on["chunk_lengths"] == [12]
    assert test_one["chunks"] == 12 and test_one["mixed_size_chunks"] is True
    assert recs_one == recs_off                                  # one instance per call: the records of the run without the flag
    assert [(r["split"], r["index"], r["n_nodes"], r["seed"]) for r in recs_on] == \
        [(r["split"], r["index"], r["n_nodes"], r["seed"]) for r in recs_off]
    for r in recs_on:
        assert sorted(r["tour"][:-1]) == list(range(r["n_nodes"])) and r["tour"][0] == r["tour"][-1] == 0
    # world sizes 1 and 2 over the same chunk list (the host-side planner; ranks take whole chunks)
    examples = read_tsp_split(split)
    chunks = E.mixed_size_chunks([ex.points.shape[0] for ex in examples], 8, 2, instances_per_call=5)
    assert chunks == [(0, 5), (5, 10), (10, 12)]
    margs = dict(diffusion_type="categorical", inference_schedule="cosine", inference_diffusion_steps=5, sparse_factor=8,
                 hidden_dim=64, n_layers=2)
    kw = dict(seed=0, sparse_factor=8, parallel_sampling=2, two_opt_iterations=100)

    def solve(rank, world):
        return E.solve_split(TSPModel(margs, sd, device=dev, seed=9), "tsp", examples, "val", E.shard_chunks(chunks, rank, world),
                             **kw)
    one = solve(0, 1)
    two = sorted(solve(0, 2) + solve(1, 2), key=lambda r: r["index"])
    assert [r["index"] for r in one] == list(range(12)) and one == two
