"""The multi-move 2-opt on the GPU (``difusco_tsp_multi_two_opt_ragged``): tours, sweeps and moves equal the numpy restatement of
the rule (tests/multi_two_opt_emulation.py) bit for bit - below, at and across a row tile (16), the powers of two of the level
table and a column chunk (1024) of the sweep, with one and several tours per group, one and several selection rounds, capped, in
ragged and grouped calls, next to a group that has nothing to do and on coordinates far from the unit square; then against the
existing 2-opt and through ``solve_tsp`` / ``solve_tsp_batch`` and the evaluation runner."""
import functools

import numpy as np
import pytest
import torch

import multi_two_opt_emulation as E
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def group(n, P, S=4, cap=1000):
    """Points, P different random-permutation start tours and the emulation's result for them, computed once per session."""
    rng = np.random.default_rng(9000 + n)
    pts = rng.random((n, 2))
    starts = np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)])
    return pts, starts, E.multi_two_opt(pts, starts, cap, S)


def _same(got, stats, g, want):
    tours, sweeps = got
    ref, s, m = want
    assert np.array_equal(tours, ref)
    assert (int(sweeps), int(np.asarray(stats["moves"]).reshape(-1)[g])) == (s, m)


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n", [4, 5, 8, 16, 17, 31, 32, 33, 63, 64, 65, 200])
def test_solo_call_equals_emulation(dev, n, P, S):
    from difusco_amd.decode import batched_multi_two_opt_torch
    pts, starts, want = group(n, P, S)
    stats = {}
    got = batched_multi_two_opt_torch(pts, starts, device=dev, select_rounds=S, stats=stats)
    assert got[0].dtype == np.int64 and got[0].shape == (P, n + 1)
    _same(got, stats, 0, want)


def test_across_a_column_chunk(dev):
    """n = 1030 > 1024: the second column chunk holds 6 columns.  Cities on a circle in angular order; the tour walks them in
    order but for two swapped neighbours at positions 1025, 1026 and two at 1028, 1029: the first sweep has two winners, both
    with row and column beyond 1024."""
    from difusco_amd.decode import batched_multi_two_opt_torch
    n = 1030
    ang = np.sort(np.random.default_rng(9000 + n).random(n)) * 2 * np.pi
    pts = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    start = np.array(list(range(1025)) + [1026, 1025, 1027, 1029, 1028, 0])[None]
    log = []
    want = E.multi_two_opt(pts, start, 1000, 4, log=log)
    first = log[0][2]
    assert len(first) == 2 and all(i >= 1024 and j >= 1024 for _, i, j in first)
    assert want[1:] == (1, 2) and np.array_equal(want[0][0], np.concatenate([np.arange(n), [0]]))
    stats = {}
    _same(batched_multi_two_opt_torch(pts, start, device=dev, stats=stats), stats, 0, want)


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_capped(dev, cap):
    from difusco_amd.decode import batched_multi_two_opt_torch
    pts, starts, full = group(64, 3)
    want = E.multi_two_opt(pts, starts, cap, 4)
    assert want[1] == cap < full[1]
    stats = {}
    _same(batched_multi_two_opt_torch(pts, starts, cap, device=dev, stats=stats), stats, 0, want)


def test_ragged_call_equals_solo_calls(dev):
    from difusco_amd.decode import batched_multi_two_opt_ragged
    groups = [group(5, 3), group(33, 1), group(200, 3)]
    stats = {}
    tours, sweeps = batched_multi_two_opt_ragged([g[0] for g in groups], [g[1] for g in groups], device=dev, stats=stats)
    assert sweeps.dtype == np.int64 and sweeps.shape == (3,)
    for g, (_, _, want) in enumerate(groups):
        _same((tours[g], sweeps[g]), stats, g, want)


def test_grouped_call_equals_solo_calls(dev):
    from difusco_amd.decode import batched_multi_two_opt_grouped
    a = group(64, 3)
    pts_b = np.random.default_rng(5).random((64, 2))             # the second group: the same starts over other points
    want_b = E.multi_two_opt(pts_b, a[1], 1000, 4)
    stats = {}
    tours, sweeps = batched_multi_two_opt_grouped(np.stack([a[0], pts_b]), np.concatenate([a[1], a[1]]), device=dev, stats=stats)
    _same((tours[:3], sweeps[0]), stats, 0, a[2])
    _same((tours[3:], sweeps[1]), stats, 1, want_b)


def test_a_finished_group_next_to_a_working_one(dev):
    from difusco_amd.decode import batched_multi_two_opt_ragged
    pts, starts, want = group(33, 1)
    optimum = want[0]                                              # 2-opt optimal: no proposal
    stats = {}
    tours, sweeps = batched_multi_two_opt_ragged([pts, pts, pts], [optimum, starts, optimum], device=dev, stats=stats)
    for g in (0, 2):
        _same((tours[g], sweeps[g]), stats, g, (optimum, 0, 0))
    _same((tours[1], sweeps[1]), stats, 1, want)


@pytest.mark.parametrize("scale,offset", [(1.0, 1e3), (1e-3, 0.0), (1e-3, 1e3)])
def test_scaled_and_offset_points(dev, scale, offset):
    from difusco_amd.decode import batched_multi_two_opt_torch
    pts, start = E.instance(64, 3)
    pts = pts * scale + offset
    want = E.multi_two_opt(pts, start[None])
    assert want[2] > want[1] > 0
    stats = {}
    _same(batched_multi_two_opt_torch(pts, start[None], device=dev, stats=stats), stats, 0, want)


def test_the_existing_two_opt_finds_nothing_to_do_on_a_converged_result(dev):
    from difusco_amd.decode import batched_multi_two_opt_torch, batched_two_opt_torch
    pts, starts, _ = group(200, 3)
    tours, _ = batched_multi_two_opt_torch(pts, starts, device=dev)
    again, its = batched_two_opt_torch(pts, tours, device=dev)
    assert its == 0 and np.array_equal(again, tours)


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
def test_solve_tsp_batch_matches_solo(dev):
    from difusco_amd import TSPModel
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    from difusco_amd.synthetic import random_state_dict
    sd = random_state_dict(64, 2, 2, seed=0)
    B, n, P = 3, 50, 2
    pts = np.random.default_rng(12).random((B, n, 2))
    seeds = [21, 22, 23]
    model = lambda seed: TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=seed)
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(B)]
    kw = dict(parallel_sampling=P, two_opt_iterations=100)
    res = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), local_search="multi2opt", **kw)
    lst = solve_tsp_batch(model(0), list(pts), -1, seeds=seeds, generators=gens(), local_search="multi2opt", **kw)
    base = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), **kw)
    for b in range(B):
        solo = solve_tsp(model(seeds[b]), pts[b], -1, generator=torch.Generator().manual_seed(b), local_search="multi2opt", **kw)
        assert res[b] == solo and lst[b] == solo, b
        assert set(solo[3]) == {"merge_iterations", "two_opt_iterations", "merged_costs", "two_opt_moves"}
        assert set(base[b][3]) == {"merge_iterations", "two_opt_iterations", "merged_costs"}
        assert solo[3]["merged_costs"] == base[b][3]["merged_costs"]              # the same decoded tours went in
        assert sorted(solo[0][:-1]) == list(range(n)) and solo[0][0] == solo[0][-1] == 0
        assert all(x <= y for x, y in zip(solo[2], solo[3]["merged_costs"])) and solo[1] < min(solo[3]["merged_costs"])
        # several moves per sweep: fewer sweeps than the moves they apply, and than the one-move sweeps of the default
        assert 0 < solo[3]["two_opt_iterations"] < solo[3]["two_opt_moves"]
        assert solo[3]["two_opt_iterations"] < base[b][3]["two_opt_iterations"]


def test_evaluate_with_the_flag(dev, tmp_path):
    from difusco_amd import TSPModel, evaluate as EV
    from difusco_amd.datasets import read_tsp_split
    from difusco_amd.pipeline import solve_tsp
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 4, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "4")
    lines, recs = EV.run(argv + ["--local_search", "multi2opt"])
    plain_lines, plain = EV.run(argv)
    assert len(recs) == len(plain) == 4 and lines[0]["local_search"] == "multi2opt"
    assert list(lines[0]) == list(plain_lines[0]) + ["local_search"]
    examples = read_tsp_split(split)
    for r, p in zip(recs, plain):
        assert list(r) == list(p) + ["two_opt_moves"]
        assert r["merged_costs"] == p["merged_costs"] and r["solved_cost"] < min(r["merged_costs"])
        assert 0 < r["2opt_iterations"] < r["two_opt_moves"]
    # one instance per call: the record of a solo call
    for r in EV.run(argv + ["--local_search", "multi2opt", "--instances_per_call", "1"])[1]:
        m = TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=r["seed"])
        solo = solve_tsp(m, examples[r["index"]].points, -1, two_opt_iterations=100, generator=torch.Generator().manual_seed(r["seed"]),
                         local_search="multi2opt")
        assert r == EV.tsp_record("val", r["index"], examples[r["index"]], r["seed"], solo)
        assert r == {x["index"]: x for x in recs}[r["index"]]     # and the same answer as in the batch
