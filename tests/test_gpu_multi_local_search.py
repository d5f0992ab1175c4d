"""The multi-move local search on the GPU (``difusco_tsp_multi_local_search_ragged``): tours and all five counters equal the numpy
restatement of the rule (tests/multi_local_search_emulation.py) bit for bit - at the sizes where the L = 3 variants have no, one
or a few rows, below, at and across a row tile (16), a wave and a column chunk (1024) of the sweeps, with one and several tours
per group, one and several selection rounds, on clustered points (a 2-opt phase after round 1 moves) and on a lattice (equal
deltas), capped, in ragged and grouped calls, next to a group that has nothing to do and on coordinates far from the unit square;
then against the existing searches and through ``solve_tsp`` / ``solve_tsp_batch`` and the evaluation runner."""
import functools

import numpy as np
import pytest
import torch

import multi_local_search_emulation as E
import multi_two_opt_emulation as M
import or_opt_emulation as O
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def group(n, P, S=4, cap=1000, rounds=16):
    """Points, P different random-permutation start tours and the emulation's result for them, computed once per session."""
    rng = np.random.default_rng(9000 + n)
    pts = rng.random((n, 2))
    starts = np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)])
    return pts, starts, E.multi_local_search(pts, starts, cap, rounds, S)


def _same(tours, stats, g, want):
    ref, c = want
    assert np.array_equal(tours, ref)
    assert set(stats) == set(KEYS)
    assert {k: int(np.asarray(stats[k]).reshape(-1)[g]) for k in KEYS} == c


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n", [4, 5, 6, 7, 8, 16, 17, 31, 32, 33, 63, 64, 65, 200])
def test_solo_call_equals_emulation(dev, n, P, S):
    from difusco_amd.decode import batched_multi_local_search_torch
    pts, starts, want = group(n, P, S)
    tours, stats = batched_multi_local_search_torch(pts, starts, device=dev, select_rounds=S)
    assert tours.dtype == np.int64 and tours.shape == (P, n + 1)
    _same(tours, stats, 0, want)


def test_across_a_column_chunk(dev):
    """n = 1100 > 1024 from a nearest-neighbour start, uncapped: both phases sweep two column chunks, and Or-opt moves are
    applied with rows and columns on either side of column 1024."""
    from difusco_amd.decode import batched_multi_local_search_torch
    n = 1100
    pts = M.instance(n, 1)[0]
    start = M.nearest_neighbour_tour(pts)
    log = []
    want = E.search_tour(pts, start, 10 ** 6, 16, 4, log=log)
    moved = [(i, j) for kind, _, winners, _ in log if kind == "oropt" for _, _, i, j in winners]
    assert any(i >= 1024 or j >= 1024 for i, j in moved) and any(i < 1024 and j < 1024 for i, j in moved)
    tours, stats = batched_multi_local_search_torch(pts, start[None], 10 ** 6, device=dev)
    _same(tours, stats, 0, (want[0][None], want[1]))


def test_a_two_opt_phase_after_round_one_moves(dev):
    from difusco_amd.decode import batched_multi_local_search_torch
    pts, start = E.clustered_instance(64, 10)
    phases = []
    want = E.search_tour(pts, start, phases=phases)
    assert phases == [(23, 5), (2, 1), (0, 0)]
    tours, stats = batched_multi_local_search_torch(pts, start[None], device=dev)
    _same(tours, stats, 0, (want[0][None], want[1]))


@pytest.mark.parametrize("k", [6, 8])
def test_ties_on_a_lattice(dev, k):
    from difusco_amd.decode import batched_multi_local_search_torch
    pts, start = E.lattice_instance(k, E.LATTICE_SEEDS[k])
    want = E.search_tour(pts, start)
    assert want[1]["or_opt_moves"] > 0
    tours, stats = batched_multi_local_search_torch(pts, start[None], device=dev)
    _same(tours, stats, 0, (want[0][None], want[1]))


@pytest.mark.parametrize("cap,rounds", [(0, 16), (1, 16), (3, 16), (1000, 1)])
def test_capped(dev, cap, rounds):
    from difusco_amd.decode import batched_multi_local_search_torch
    if rounds == 1:                                              # the clustered case has three rounds uncapped
        pts, start = E.clustered_instance(64, 10)
        starts = start[None]
    else:
        pts, starts, full = group(64, 3)
        assert cap < min(full[1]["two_opt_sweeps"], 8)
    want = E.multi_local_search(pts, starts, cap, rounds, 4)
    assert want[1]["rounds"] == 1
    tours, stats = batched_multi_local_search_torch(pts, starts, cap, device=dev, max_rounds=rounds)
    _same(tours, stats, 0, want)


def test_ragged_call_equals_solo_calls(dev):
    from difusco_amd.decode import batched_multi_local_search_ragged
    groups = [group(5, 3), group(33, 1), group(200, 3)]
    tours, stats = batched_multi_local_search_ragged([g[0] for g in groups], [g[1] for g in groups], device=dev)
    assert stats["two_opt_sweeps"].dtype == np.int64 and stats["rounds"].dtype == np.int32 and stats["rounds"].shape == (3,)
    for g, (_, _, want) in enumerate(groups):
        _same(tours[g], stats, g, want)


def test_grouped_call_equals_solo_calls(dev):
    from difusco_amd.decode import batched_multi_local_search_grouped
    a = group(64, 3)
    pts_b = np.random.default_rng(5).random((64, 2))             # the second group: the same starts over other points
    want_b = E.multi_local_search(pts_b, a[1], 1000, 16, 4)
    tours, stats = batched_multi_local_search_grouped(np.stack([a[0], pts_b]), np.concatenate([a[1], a[1]]), device=dev)
    _same(tours[:3], stats, 0, a[2])
    _same(tours[3:], stats, 1, want_b)


def test_a_finished_group_next_to_a_working_one(dev):
    """Group 0 and 2 start at a local optimum of both neighbourhoods: their first sweep ends the 2-opt phase, their second the
    Or-opt phase, while group 1 is still in its first 2-opt phase; the clustered group 3 is in an Or-opt phase while group 1 is
    in a 2-opt phase."""
    from difusco_amd.decode import batched_multi_local_search_ragged
    pts, starts, want = group(33, 1)
    optimum = want[0]
    rest = (optimum, {"two_opt_sweeps": 0, "or_opt_sweeps": 0, "rounds": 1, "two_opt_moves": 0, "or_opt_moves": 0})
    pts_c, start_c = E.clustered_instance(64, 10)
    want_c = E.multi_local_search(pts_c, start_c[None])
    tours, stats = batched_multi_local_search_ragged([pts, pts, pts, pts_c], [optimum, starts, optimum, start_c[None]], device=dev)
    for g in (0, 2):
        _same(tours[g], stats, g, rest)
    _same(tours[1], stats, 1, want)
    _same(tours[3], stats, 3, want_c)


@pytest.mark.parametrize("scale,offset", [(1.0, 1e3), (1e-3, 0.0), (1e-3, 1e3)])
def test_scaled_and_offset_points(dev, scale, offset):
    from difusco_amd.decode import batched_multi_local_search_torch
    pts, start = M.instance(64, 3)
    pts = pts * scale + offset
    want = E.multi_local_search(pts, start[None])
    assert want[1]["two_opt_moves"] > want[1]["two_opt_sweeps"] > 0
    tours, stats = batched_multi_local_search_torch(pts, start[None], device=dev)
    _same(tours, stats, 0, want)


def test_the_existing_searches_find_nothing_to_do_and_multi2opt_is_no_shorter(dev):
    from difusco_amd.decode import batched_local_search_torch, batched_multi_local_search_torch, batched_multi_two_opt_torch
    pts, starts, want = group(200, 3)
    assert want[1]["or_opt_moves"] > 0 and want[1]["rounds"] < 16
    tours, _ = batched_multi_local_search_torch(pts, starts, device=dev)
    ls_stats = {}
    again, its = batched_local_search_torch(pts, tours, device=dev, stats=ls_stats)      # the exact sweep, one move at a time
    assert its == 0 and ls_stats["or_opt_iterations"] == 0 and np.array_equal(again, tours)
    m_stats = {}
    again, sweeps = batched_multi_two_opt_torch(pts, tours, device=dev, stats=m_stats)
    assert sweeps == 0 and m_stats["moves"] == 0 and np.array_equal(again, tours)
    multi, _ = batched_multi_two_opt_torch(pts, starts, device=dev)
    for p in range(3):
        assert O.tour_length(pts, tours[p]) <= O.tour_length(pts, multi[p])
    assert any(O.tour_length(pts, tours[p]) < O.tour_length(pts, multi[p]) for p in range(3))


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
INFO = {"merge_iterations", "two_opt_iterations", "merged_costs", "two_opt_moves", "or_opt_iterations", "or_opt_moves",
        "local_search_rounds"}


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
    res = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), local_search="multi2opt+oropt", **kw)
    lst = solve_tsp_batch(model(0), list(pts), -1, seeds=seeds, generators=gens(), local_search="multi2opt+oropt", **kw)
    base = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), local_search="multi2opt", **kw)
    for b in range(B):
        solo = solve_tsp(model(seeds[b]), pts[b], -1, generator=torch.Generator().manual_seed(b), local_search="multi2opt+oropt", **kw)
        assert res[b] == solo and lst[b] == solo, b
        assert set(solo[3]) == INFO
        assert solo[3]["merged_costs"] == base[b][3]["merged_costs"]              # the same decoded tours went in
        assert sorted(solo[0][:-1]) == list(range(n)) and solo[0][0] == solo[0][-1] == 0
        assert all(x <= y for x, y in zip(solo[2], base[b][2]))                   # no tour longer than multi2opt leaves it
        assert 0 < solo[3]["two_opt_iterations"] < solo[3]["two_opt_moves"]
        assert solo[3]["or_opt_iterations"] <= solo[3]["or_opt_moves"] and solo[3]["local_search_rounds"] >= 1


def test_evaluate_with_the_flag(dev, tmp_path):
    from difusco_amd import TSPModel, evaluate as EV
    from difusco_amd.datasets import read_tsp_split
    from difusco_amd.pipeline import solve_tsp
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 4, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "4")
    lines, recs = EV.run(argv + ["--local_search", "multi2opt+oropt"])
    plain_lines, plain = EV.run(argv + ["--local_search", "multi2opt"])
    assert len(recs) == len(plain) == 4 and lines[0]["local_search"] == "multi2opt+oropt"
    examples = read_tsp_split(split)
    for r, p in zip(recs, plain):
        assert set(r) == set(p) | {"or_opt_iterations", "or_opt_moves", "local_search_rounds"}
        assert r["merged_costs"] == p["merged_costs"] and r["solved_cost"] <= p["solved_cost"]
        assert 0 < r["2opt_iterations"] < r["two_opt_moves"]
    # one instance per call: the record of a solo call
    for r in EV.run(argv + ["--local_search", "multi2opt+oropt", "--instances_per_call", "1"])[1]:
        m = TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=r["seed"])
        solo = solve_tsp(m, examples[r["index"]].points, -1, two_opt_iterations=100, generator=torch.Generator().manual_seed(r["seed"]),
                         local_search="multi2opt+oropt")
        assert r == EV.tsp_record("val", r["index"], examples[r["index"]], r["seed"], solo)
        assert r == {x["index"]: x for x in recs}[r["index"]]     # and the same answer as in the batch
