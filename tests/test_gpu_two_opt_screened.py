"""Screened 2-opt on the GPU (``method="screened"``: difusco_tsp_two_opt_screened / _grouped_screened): the tours and iteration
counts of the exact method, bit for bit - against the reference's fixtures, the CPU oracle, the exact method on scaled and
degenerate inputs and at TSP-10000 - with float64 spent on a small share of the pairs, and through the solve flows."""
import os

import numpy as np
import pytest
import torch

from oracle import tsp_decode_oracle as D
from test_decode_oracle import TWO_OPT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _pairs(n):
    return n * (n - 3) // 2


def _random_tours(rng, n, batch):
    return np.stack([np.concatenate([[0], 1 + rng.permutation(n - 1), [0]]) for _ in range(batch)])


def _nn_tour(pts):
    n = len(pts)
    left = np.ones(n, dtype=bool)
    tour = [0]
    left[0] = False
    while len(tour) < n:
        d = ((pts - pts[tour[-1]]) ** 2).sum(-1)
        d[~left] = np.inf
        tour.append(int(d.argmin()))
        left[tour[-1]] = False
    return np.array(tour + [0])


def _strip_tour(pts):
    """The start tour of test_two_opt_full_size_properties."""
    order = np.argsort(pts[:, 0] // 0.05 * 10 + pts[:, 1] * (1 - 2 * ((pts[:, 0] // 0.05) % 2)))
    order = np.roll(order, -int(np.where(order == 0)[0][0]))
    return np.concatenate([order, [0]])[None, :]


# ---- the reference's fixtures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", TWO_OPT, ids=[os.path.basename(p)[11:-4] for p in TWO_OPT])
def test_screened_matches_reference_fixture(dev, path):
    from difusco_amd.decode import batched_two_opt_grouped, batched_two_opt_torch
    z = np.load(path)
    out, it = batched_two_opt_torch(z["points"], z["tours_in"], max_iterations=int(z["max_iterations"]), device=dev,
                                    method="screened")
    assert it == int(z["iterations"]) and np.array_equal(out, z["tours_out"])
    P = z["tours_in"].shape[0]
    out, its = batched_two_opt_grouped(np.stack([z["points"]] * 3), np.concatenate([z["tours_in"]] * 3),
                                       max_iterations=int(z["max_iterations"]), device=dev, method="screened")
    for g in range(3):
        assert np.array_equal(out[g * P:(g + 1) * P], z["tours_out"]) and its[g] == int(z["iterations"])


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,max_it", [(33, 2, 1000), (257, 1, 1000), (500, 4, 40), (1000, 1, 25)])
def test_screened_matches_oracle_on_random_tours(dev, n, batch, max_it):
    """The cases of test_two_opt_matches_oracle: random-permutation tours, where half of all pairs improve the tour."""
    from difusco_amd.decode import batched_two_opt_torch
    rng = np.random.default_rng(n + batch)
    pts = rng.random((n, 2))
    tours = _random_tours(rng, n, batch)
    ref, ref_it = D.batched_two_opt(pts, tours, max_iterations=max_it)
    stats = {}
    out, it = batched_two_opt_torch(pts, tours, max_iterations=max_it, device=dev, method="screened", stats=stats)
    sweeps = it + (1 if it < max_it else 0)
    print(f"n={n} batch={batch}: {it} moves, float64 share {stats['exact_pairs'] / (sweeps * batch * _pairs(n)):.3e} "
          f"({stats['exact_pairs']} pairs)")
    assert it == ref_it and np.array_equal(out, ref)


def test_screened_matches_oracle_on_decoded_like_tour(dev):
    from difusco_amd.decode import batched_two_opt_torch
    n = 1000
    pts = np.random.default_rng(21).random((n, 2))
    tours = _nn_tour(pts)[None, :]
    ref, ref_it = D.batched_two_opt(pts, tours, max_iterations=25)
    out, it = batched_two_opt_torch(pts, tours, max_iterations=25, device=dev, method="screened")
    assert it == ref_it and np.array_equal(out, ref)


# ---- scales and degeneracy: bit-equal to the exact method ------------------------------------------------------------------
def _degenerate_points(name, n, rng):
    pts = rng.random((n, 2))
    if name == "scaled_1e-3":
        return pts * 1e-3
    if name == "scaled_1e4":
        return pts * 1e4
    if name == "offset_1000":
        return pts + 1000.0
    if name == "duplicates":
        pts[n // 2:] = pts[:n // 2]
        return pts
    if name == "coarse_grid":
        return np.round(pts * 16) / 16              # 17 x 17 positions for n points: exact ties, the lowest flat index wins
    if name == "nan":                               # M is NaN: no bound, the whole call takes the exact sweep
        pts[n // 3, 1] = np.nan
        return pts
    raise KeyError(name)


@pytest.mark.parametrize("name", ["scaled_1e-3", "scaled_1e4", "offset_1000", "duplicates", "coarse_grid", "nan"])
def test_screened_equals_exact_on_scaled_and_degenerate_points(dev, name):
    from difusco_amd.decode import batched_two_opt_grouped, batched_two_opt_torch
    n, batch = 400, 2
    rng = np.random.default_rng(7)
    pts = _degenerate_points(name, n, rng)
    tours = np.concatenate([_random_tours(rng, n, batch - 1), _nn_tour(np.nan_to_num(pts))[None, :]])
    for max_it in (60, 1000) if name != "nan" else (20,):
        ref, ref_it = batched_two_opt_torch(pts, tours, max_iterations=max_it, device=dev)
        stats = {}
        out, it = batched_two_opt_torch(pts, tours, max_iterations=max_it, device=dev, method="screened", stats=stats)
        assert it == ref_it and np.array_equal(out, ref), (name, max_it)
        print(f"{name} cap {max_it}: {it} moves, {stats['exact_pairs']} pairs in float64")
    # grouped: this instance beside a plain one, every group as its own call
    other = rng.random((n, 2))
    gp = np.stack([pts, other])
    gt = np.concatenate([tours, _random_tours(rng, n, batch)])
    ref, ref_its = batched_two_opt_grouped(gp, gt, max_iterations=30, device=dev)
    out, its = batched_two_opt_grouped(gp, gt, max_iterations=30, device=dev, method="screened")
    assert np.array_equal(its, ref_its) and np.array_equal(out, ref)


def test_screened_equals_exact_with_several_tours_over_several_chunks(dev):
    """n > 1024 (more than one column chunk per row tile) with several tours per call, plain and grouped: the per-block minima
    are indexed by tour, row tile and chunk together."""
    from difusco_amd.decode import batched_two_opt_grouped, batched_two_opt_torch
    n, P = 2100, 3
    rng = np.random.default_rng(31)
    pts = rng.random((2, n, 2))
    tours = np.concatenate([_random_tours(rng, n, 2 * P - 1), _nn_tour(pts[1])[None, :]])
    ref, ref_it = batched_two_opt_torch(pts[0], tours[:P], max_iterations=12, device=dev)
    stats = {}
    out, it = batched_two_opt_torch(pts[0], tours[:P], max_iterations=12, device=dev, method="screened", stats=stats)
    assert it == ref_it == 12 and np.array_equal(out, ref)
    assert stats["exact_pairs"] < 0.01 * 12 * P * _pairs(n)
    ref, ref_its = batched_two_opt_grouped(pts, tours, max_iterations=12, device=dev)
    out, its = batched_two_opt_grouped(pts, tours, max_iterations=12, device=dev, method="screened")
    assert np.array_equal(its, ref_its) and np.array_equal(out, ref)


def test_screened_without_a_bound_runs_the_exact_sweep(dev):
    """Coordinates beyond the float32 range of the screen: same answer, every pair in float64."""
    from difusco_amd.decode import batched_two_opt_torch, two_opt_screen_bound
    n = 64
    rng = np.random.default_rng(2)
    pts = rng.random((n, 2)) * 1e25
    assert two_opt_screen_bound(np.abs(pts).max()) is None
    tours = _random_tours(rng, n, 1)
    ref, ref_it = batched_two_opt_torch(pts, tours, max_iterations=5, device=dev)
    stats = {}
    out, it = batched_two_opt_torch(pts, tours, max_iterations=5, device=dev, method="screened", stats=stats)
    assert it == ref_it == 5 and np.array_equal(out, ref)
    assert stats["exact_pairs"] == 5 * (n - 1) * (n - 2) // 2


# ---- full size -----------------------------------------------------------------------------------------------------------------
def test_screened_full_size_equals_exact_and_screens(dev):
    """TSP-10000 on the strip tour of test_two_opt_full_size_properties: bit-equal to the exact method at 30 moves,
    deterministic, a capped run is a prefix of a longer one, and the float64 path takes less than 1 % of the pairs."""
    from difusco_amd.decode import batched_two_opt_torch
    n = 10000
    pts = np.random.default_rng(5).random((n, 2))
    tour0 = _strip_tour(pts)
    ref, ref_it = batched_two_opt_torch(pts, tour0, max_iterations=30, device=dev)
    stats = {}
    a, it_a = batched_two_opt_torch(pts, tour0, max_iterations=30, device=dev, method="screened", stats=stats)
    b, it_b = batched_two_opt_torch(pts, tour0, max_iterations=30, device=dev, method="screened")
    assert it_a == it_b == ref_it == 30 and np.array_equal(a, ref) and np.array_equal(a, b)
    c, it_c = batched_two_opt_torch(pts, tour0, max_iterations=10, device=dev, method="screened")
    d, it_d = batched_two_opt_torch(pts, c, max_iterations=20, device=dev, method="screened")
    assert it_c == 10 and it_d == 20 and np.array_equal(d, a)
    share = stats["exact_pairs"] / (30 * _pairs(n))
    print(f"TSP-10000 strip tour, 30 moves: {stats['exact_pairs']} pairs in float64, share {share:.3e}")
    assert 0 < stats["exact_pairs"] and share < 0.01


# ---- flows ---------------------------------------------------------------------------------------------------------------------
def _tsp_model(dev, seed, sparse_factor):
    from difusco_amd import TSPModel
    from oracle import difusco_oracle as O
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=2, hidden_dim=64, inference_trick="ddim", inference_diffusion_steps=8, inference_schedule="cosine")
    return TSPModel(args, O.init_params(64, 2, 2, seed=0), device=dev, seed=seed)


def test_solve_tsp_screened_equals_default(dev):
    from difusco_amd.pipeline import solve_tsp
    pts = np.random.default_rng(4).random((80, 2))
    runs = []
    for kw in ({}, {"two_opt_method": "screened"}):
        runs.append(solve_tsp(_tsp_model(dev, 3, 10), pts, sparse_factor=10, parallel_sampling=3, two_opt_iterations=200,
                              sequential_sampling=2, generator=torch.Generator().manual_seed(1), **kw))
    (tour, cost, costs, info), (tour_s, cost_s, costs_s, info_s) = runs
    assert tour_s == tour and cost_s == cost and costs_s == costs and info_s == info
    assert info["two_opt_iterations"] > 0


def test_solve_tsp_batch_screened_equals_default(dev):
    from difusco_amd.pipeline import solve_tsp_batch
    B = 3
    pts = np.random.default_rng(12).random((B, 50, 2))
    runs = []
    for kw in ({}, {"two_opt_method": "screened"}):
        runs.append(solve_tsp_batch(_tsp_model(dev, 0, 8), pts, 8, parallel_sampling=2, sequential_sampling=2,
                                    two_opt_iterations=100, seeds=[21, 22, 23],
                                    generators=[torch.Generator().manual_seed(b) for b in range(B)], **kw))
    for b in range(B):
        for field in range(4):
            assert runs[1][b][field] == runs[0][b][field], (b, field)


def test_evaluate_screened_gives_the_same_records(dev, tmp_path):
    from difusco_amd import evaluate as E
    from difusco_amd.synthetic import random_state_dict
    rng = np.random.default_rng(1)
    lines = []
    for n in (60, 60, 48, 60):
        p = rng.random((n, 2))
        perm = rng.permutation(n)
        t = np.concatenate([perm, perm[:1]]) + 1
        lines.append(" ".join(str(float(v)) for v in p.reshape(-1)) + " output " + " ".join(str(int(v)) for v in t))
    (tmp_path / "tsp.txt").write_text("\n".join(lines) + "\n")
    sd = random_state_dict(64, 2, 2, seed=0)
    ckpt = str(tmp_path / "last.ckpt")
    torch.save({"epoch": 0, "global_step": 0, "state_dict": {"model." + k: v for k, v in sd.items()},
                "optimizer_states": [], "lr_schedulers": []}, ckpt)
    argv = ["--task", "tsp", "--do_test", "--diffusion_type", "categorical", "--storage_path", str(tmp_path),
            "--validation_split", "tsp.txt", "--test_split", "tsp.txt", "--validation_examples", "2", "--inference_schedule",
            "cosine", "--inference_diffusion_steps", "6", "--ckpt_path", ckpt, "--hidden_dim", "64", "--n_layers", "2",
            "--sparse_factor", "10", "--parallel_sampling", "2", "--two_opt_iterations", "100", "--instances_per_call", "3"]
    lines_a, recs_a = E.run(argv)
    lines_b, recs_b = E.run(argv + ["--two_opt_method", "screened"])
    assert recs_a == recs_b and len(recs_a) == 6 and any(r["2opt_iterations"] > 0 for r in recs_a)
    assert [l["two_opt_method"] for l in lines_a] == ["exact", "exact"]
    assert [l["two_opt_method"] for l in lines_b] == ["screened", "screened"] and lines_b[0]["ignored_args"] == []
    for la, lb in zip(lines_a, lines_b):
        assert all(la[k] == lb[k] for k in la if k.startswith(la["split"] + "/"))
