"""The neighbour-list multi-move 2-opt on the GPU (``difusco_tsp_nbr_two_opt_ragged``): tours, sweeps, full sweeps and moves
equal the numpy restatement of the rule (tests/nbr_two_opt_emulation.py) bit for bit.  Sizes sit at the edges of the kernels: 4 is
the smallest legal tour, 17, 33 and 65 are one past a row tile and a wave, 257 one past a block of the walk, 1025 one past a
column chunk of the full sweep.  Then the full lists against the multi-move 2-opt, the position-n wrap, list hygiene,
independence of the groups of a call, and the wrappers, solvers and the evaluation runner.

Every case of ``test_against_the_emulation`` is one size and one K; inside it runs closing on and off, the caps 0, 1, 3 and
1000, and groups of 1 and 3 tours with random-permutation and nearest-neighbour starts, each combination as one ragged call.
At n = 1025 the groups are three random-permutation tours (caps 0, 1 and 3 only: to convergence the emulation alone needs
minutes there) and the nearest-neighbour tour (every cap)."""
import functools
import json

import numpy as np
import pytest
import torch

import multi_two_opt_emulation as E
import nbr_two_opt_emulation as NB
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu

SIZES = [4, 5, 6, 7, 17, 33, 64, 65, 257, 1025]
CAPS = [0, 1, 3, 1000]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def points(n):
    return np.random.default_rng(7000 + n).random((n, 2))


@functools.lru_cache(maxsize=None)
def lists(n, K):
    """The K nearest other cities, padded with -1 where the instance has fewer."""
    nb = NB.knn_lists(points(n), K)
    return np.concatenate([nb, np.full((n, K - nb.shape[1]), -1, dtype=np.int32)], axis=1)


@functools.lru_cache(maxsize=None)
def starts(n, kind, P):
    """P start tours: random permutations; kind "nearest": the first is the nearest-neighbour tour."""
    rng = np.random.default_rng(7100 + n)
    t = [np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)]
    if kind == "nearest":
        t[0] = E.nearest_neighbour_tour(points(n))
    return np.stack(t)


@functools.lru_cache(maxsize=None)
def emulated(n, kind, P, K, closing, cap):
    return NB.nbr_two_opt(points(n), starts(n, kind, P), lists(n, K), closing, cap, 4)


def _same(tours, stats, g, want):
    ref, sweeps, full, moves = want
    got = tuple(int(np.asarray(stats[k]).reshape(-1)[g]) for k in ("sweeps", "full_sweeps", "moves"))
    assert got == (sweeps, full, moves), (g, got, (sweeps, full, moves))
    assert np.array_equal(tours, ref), g


def _ragged(dev, groups, nbr, closing, cap=1000, **kw):
    """One ragged call on [(points, start tours)], the lists of every group in ``nbr``: (tours, stats)."""
    from difusco_amd.decode import batched_nbr_two_opt_ragged
    stats = {}
    tours, sweeps = batched_nbr_two_opt_ragged([g[0] for g in groups], [g[1] for g in groups], cap, device=dev, neighbors=nbr,
                                               closing=closing, stats=stats, **kw)
    assert np.array_equal(sweeps, stats["sweeps"]) and sweeps.dtype == np.int64
    return tours, stats


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_against_the_emulation(dev, n, K):
    closed_some = False
    for closing in (True, False):
        for cap in CAPS:
            kinds = [(kind, P) for kind in ("random", "nearest") for P in (1, 3)]
            if n == 1025:
                kinds = [("nearest", 1)] if cap == 1000 else [("random", 3), ("nearest", 1)]
            tours, stats = _ragged(dev, [(points(n), starts(n, kind, P)) for kind, P in kinds], [lists(n, K)] * len(kinds), closing, cap)
            for g, (kind, P) in enumerate(kinds):
                want = emulated(n, kind, P, K, closing, cap)
                _same(tours[g], stats, g, want)
                closed_some |= want[2] > 0
    assert closed_some or K > 1                                   # the closing phase ran: lists of one city leave full moves behind


@pytest.mark.parametrize("n", [5, 33, 64])
def test_full_lists_equal_the_multi_move_two_opt(dev, n):
    from difusco_amd.decode import (batched_multi_two_opt_grouped, batched_multi_two_opt_ragged, batched_multi_two_opt_torch,
                                    batched_nbr_two_opt_grouped, batched_nbr_two_opt_ragged, batched_nbr_two_opt_torch)
    pts, t3, t1, every = points(n), starts(n, "random", 3), starts(n, "nearest", 1), NB.all_others(n)
    for closing in (True, False):
        for cap in (1000, 2):
            ms, ns = {}, {}
            want = batched_multi_two_opt_torch(pts, t3, cap, device=dev, stats=ms)
            got = batched_nbr_two_opt_torch(pts, t3, cap, device=dev, neighbors=every, closing=closing, stats=ns)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and ns["moves"] == ms["moves"] and ns["full_sweeps"] == 0
            want = batched_multi_two_opt_grouped(np.stack([pts, pts]), np.concatenate([t3, t3[::-1]]), cap, device=dev, stats=ms)
            got = batched_nbr_two_opt_grouped(np.stack([pts, pts]), np.concatenate([t3, t3[::-1]]), cap, device=dev,
                                              neighbors=np.stack([every, every]), closing=closing, stats=ns)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(ns["moves"], ms["moves"])
            want = batched_multi_two_opt_ragged([pts, pts], [t3, t1], cap, device=dev, stats=ms)
            got = batched_nbr_two_opt_ragged([pts, pts], [t3, t1], cap, device=dev, neighbors=[every, every], closing=closing, stats=ns)
            assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0])) and np.array_equal(got[1], want[1])
            assert np.array_equal(ns["moves"], ms["moves"]) and not ns["full_sweeps"].any()


@pytest.mark.parametrize("n,K", [(65, 1), (257, 3), (257, 8)])
def test_closed_results_are_two_opt_optima(dev, n, K):
    from difusco_amd.decode import batched_multi_two_opt_torch, batched_nbr_two_opt_torch
    pts, t = points(n), starts(n, "nearest", 3)
    stats = {}
    tours, sweeps = batched_nbr_two_opt_torch(pts, t, device=dev, neighbors=lists(n, K), stats=stats)
    assert 0 < sweeps < 1000 and stats["moves"] >= sweeps
    ms = {}
    again, more = batched_multi_two_opt_torch(pts, tours, device=dev, stats=ms)
    assert more == 0 and ms["moves"] == 0 and np.array_equal(again, tours)
    for a, b in zip(t, tours):
        assert E.tour_length(pts, b) < E.tour_length(pts, a)


def wrap_instance(n=12, i=4):
    """Cities on a circle in angular order; the tour walks 0 .. i, then n-1 down to i+1: the move (i, n-1) puts it in order.
    The only list entry: city tour[i+1] = n-1 lists tour[0] = 0 - the TAIL edge of the pair (i, n-1), through position n."""
    ang = np.sort(np.random.default_rng(7300 + n).random(n)) * 2 * np.pi
    pts = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    tour = np.array(list(range(i + 1)) + list(range(n - 1, i, -1)) + [0])
    nbr = np.full((n, 2), -1, dtype=np.int32)
    nbr[tour[i + 1], 1] = tour[0]
    return pts, tour, nbr, i


def test_the_wrap_of_position_n(dev):
    pts, tour, nbr, i = wrap_instance()
    n = len(pts)
    # the construction: (i, n-1) is the only improving pair of the tour, and the only candidate the list yields that improves
    c = E.row_changes(pts, tour, 0, n - 2)
    assert np.argwhere(c < -1e-6).tolist() == [[i, n - 1]]
    L = NB.listed(nbr, n)
    mask = NB.candidate_mask(L | L.T, tour)
    assert mask[i, n - 1] and mask.sum() <= 2
    for closing in (False, True):
        want = NB.nbr_two_opt(pts, tour[None], nbr, closing, 1000, 4)
        assert want[1:] == (1, 0, 1) and np.array_equal(want[0][0], np.concatenate([np.arange(n), [0]]))
        tours, stats = _ragged(dev, [(pts, tour[None])], [nbr], closing)
        _same(tours[0], stats, 0, want)


def hygiene_lists(n):
    base = lists(n, 4).copy()
    out = {}
    a = base.copy(); a[::2, 1] = -1; a[1::2, 2] = n; a[::3, 3] = 2 ** 31 - 1; a[::5, 0] = -(2 ** 31)
    out["pads"] = a
    a = base.copy(); a[:, 0] = np.arange(n); a[::2, 2] = np.arange(n)[::2]
    out["self"] = a
    a = base.copy(); a[:, 1] = a[:, 0]; a[::2, 3] = a[::2, 2]
    out["duplicates"] = a
    a = np.full((n, 4), -1, dtype=np.int32)
    for c in range(n):                                           # a lists c only where a < c: never both directions
        mine = [x for x in base[c] if x > c]
        a[c, :len(mine)] = mine
    out["asymmetric"] = a
    out["pads only"] = np.full((n, 4), -1, dtype=np.int32)
    return out


@pytest.mark.parametrize("n", [33, 65])
def test_list_hygiene(dev, n):
    pts = points(n)
    t = starts(n, "nearest", 3)
    for name, nbr in hygiene_lists(n).items():
        for closing in (True, False):
            want = NB.nbr_two_opt(pts, t, nbr, closing, 1000, 4)
            tours, stats = _ragged(dev, [(pts, t)], [nbr], closing)
            _same(tours[0], stats, 0, want)
            assert (want[3] > 0) == (closing or name != "pads only"), name


def test_coincident_cities_and_an_optimal_tour(dev):
    n = 40
    pts = points(n).copy()
    pts[5] = pts[6] = pts[7]                                      # three cities on one spot
    pts[20] = pts[30]
    nbr = NB.knn_lists(pts, 5)
    t = starts(n, "random", 3)
    for closing in (True, False):
        want = NB.nbr_two_opt(pts, t, nbr, closing, 1000, 4)
        assert want[3] > 0
        tours, stats = _ragged(dev, [(pts, t)], [nbr], closing)
        _same(tours[0], stats, 0, want)
    best = NB.nbr_two_opt(points(n), starts(n, "random", 1), lists(n, 5), True, 1000, 4)[0]       # a 2-opt optimum
    for closing in (True, False):
        tours, stats = _ragged(dev, [(points(n), best)], [lists(n, 5)], closing)
        _same(tours[0], stats, 0, (best, 0, 0, 0))


INDEPENDENT = [4, 5, 6, 7, 17, 33, 64, 65, 100, 130, 257]


def test_groups_do_not_depend_on_their_company(dev):
    K = 3
    groups = [(points(n), starts(n, "nearest", 1 + g % 3)) for g, n in enumerate(INDEPENDENT)]
    nbr = [lists(n, K) for n in INDEPENDENT]
    alone = []
    for g in range(len(groups)):
        tours, stats = _ragged(dev, [groups[g]], [nbr[g]], True)
        alone.append((tours[0], int(stats["sweeps"][0]), int(stats["full_sweeps"][0]), int(stats["moves"][0])))
    _same(alone[4][0], {"sweeps": [alone[4][1]], "full_sweeps": [alone[4][2]], "moves": [alone[4][3]]}, 0,
          emulated(17, "nearest", 2, K, True, 1000))
    for order in (list(range(11)), list(range(10, -1, -1)), [3, 8, 8, 0, 10, 8]):
        tours, stats = _ragged(dev, [groups[g] for g in order], [nbr[g] for g in order], True)
        for k, g in enumerate(order):
            _same(tours[k], stats, k, alone[g])


def test_three_hundred_small_groups(dev):
    sizes = [4 + g % 9 for g in range(300)]
    rng = np.random.default_rng(7400)
    groups, nbr = [], []
    for n in sizes:
        pts = rng.random((n, 2))
        groups.append((pts, np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(1 + n % 2)])))
        nbr.append(NB.knn_lists(pts, 2))
    tours, stats = _ragged(dev, groups, nbr, True)
    for g in range(300):
        _same(tours[g], stats, g, NB.nbr_two_opt(groups[g][0], groups[g][1], nbr[g], True, 1000, 4))
    assert stats["moves"].sum() > 300


# ---- wrappers, solvers and the runner -----------------------------------------------------------------------------------------
def test_lists_built_by_the_wrapper(dev):
    from difusco_amd.decode import batched_nbr_two_opt_ragged, batched_nbr_two_opt_torch, tsp_candidate_lists
    from difusco_amd.graph import knn_edge_index_gpu
    ns, K = [33, 65, 257], 5
    groups = [(points(n), starts(n, "nearest", 2)) for n in ns]
    ei = knn_edge_index_gpu(np.concatenate([g[0] for g in groups]), K + 1, device=dev, sizes=ns)
    explicit = tsp_candidate_lists(ei, ns, K)
    for nb, n in zip(explicit, ns):
        nb = nb.cpu().numpy()
        assert nb.shape == (n, K) and nb.dtype == np.int32 and (nb != np.arange(n)[:, None]).all() and nb.min() >= 0 and nb.max() < n
        assert np.array_equal(nb, NB.knn_lists(points(n), K))     # distinct distances: the order is the emulation's
    s0, s1 = {}, {}
    built = batched_nbr_two_opt_ragged([g[0] for g in groups], [g[1] for g in groups], device=dev, candidates=K, stats=s0)
    given = batched_nbr_two_opt_ragged([g[0] for g in groups], [g[1] for g in groups], device=dev, neighbors=explicit, stats=s1)
    assert all(np.array_equal(a, b) for a, b in zip(built[0], given[0])) and np.array_equal(built[1], given[1])
    assert all(np.array_equal(s0[k], s1[k]) for k in ("sweeps", "full_sweeps", "moves")) and s0["moves"].min() > 0
    solo = batched_nbr_two_opt_torch(*groups[1], device=dev, candidates=K)
    assert np.array_equal(solo[0], built[0][1]) and solo[1] == built[1][1]


def test_solve_tsp_takes_the_lists_of_the_instance_graph(dev):
    from difusco_amd import TSPModel
    from difusco_amd.decode import batched_nbr_two_opt_torch, tsp_candidate_lists
    from difusco_amd.graph import knn_edge_index_gpu
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    from difusco_amd.synthetic import random_state_dict
    sd = random_state_dict(64, 2, 2, seed=0)
    pts = np.random.default_rng(14).random((2, 50, 2)).astype(np.float32).astype(np.float64)
    model = lambda seed: TSPModel(_model_args(sparse_factor=8, hidden_dim=64, n_layers=2), sd, device=dev, seed=seed)
    kw = dict(parallel_sampling=2, local_search="multi2opt")
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(2)]
    for K, closing in ((5, True), (7, False), (12, True)):        # 12 > sparse_factor - 1: a k-NN call of the search's own
        nkw = dict(two_opt_iterations=100, local_search_candidates=K, local_search_closing=closing, **kw)
        res = solve_tsp_batch(model(0), pts, 8, seeds=[5, 6], generators=gens(), **nkw)
        lst = solve_tsp_batch(model(0), list(pts), 8, seeds=[5, 6], generators=gens(), **nkw)
        for b in range(2):
            solo = solve_tsp(model(5 + b), pts[b], 8, generator=torch.Generator().manual_seed(b), **nkw)
            assert res[b] == solo and lst[b] == solo
            merged = solve_tsp(model(5 + b), pts[b], 8, generator=torch.Generator().manual_seed(b), two_opt_iterations=0, **kw)
            assert merged[3]["two_opt_iterations"] == 0 and merged[2] == solo[3]["merged_costs"]
            info = solo[3]
            assert info["local_search_candidates"] == K and info["local_search_closing"] is closing
            assert 0 <= info["two_opt_full_sweeps"] <= info["two_opt_iterations"] and (closing or info["two_opt_full_sweeps"] == 0)
            assert sorted(solo[0][:-1]) == list(range(50)) and solo[1] < min(info["merged_costs"])
    # the decode call on the same lists and the same merged tours
    K = 5
    captured = {}
    import difusco_amd.decode as D
    real = D.batched_nbr_two_opt_torch

    def spy(points, tours, **kw):
        captured.update(points=np.array(points), tours=np.array(tours), neighbors=kw["neighbors"])
        return real(points, tours, **kw)
    D.batched_nbr_two_opt_torch = spy
    try:
        solo = solve_tsp(model(5), pts[0], 8, generator=torch.Generator().manual_seed(0), two_opt_iterations=100,
                         local_search_candidates=K, **kw)
    finally:
        D.batched_nbr_two_opt_torch = real
    want_lists = tsp_candidate_lists(knn_edge_index_gpu(pts[0], 8, device=dev), [50], K)[0]
    assert torch.equal(captured["neighbors"], want_lists) and np.array_equal(captured["points"], pts[0])
    stats = {}
    direct = batched_nbr_two_opt_torch(pts[0], captured["tours"], 100, device=dev, neighbors=want_lists.cpu().numpy(), stats=stats)
    from difusco_amd.pipeline import tour_length
    costs = [tour_length(pts[0], t) for t in direct[0]]
    assert solo[2] == costs and solo[0] == direct[0][int(np.argmin(costs))].tolist()
    assert solo[3]["two_opt_iterations"] == direct[1] and solo[3]["two_opt_moves"] == stats["moves"]


def test_evaluate_with_and_without_the_flag(dev, tmp_path):
    from difusco_amd import TSPModel, evaluate as EV
    from difusco_amd.datasets import read_tsp_split
    from difusco_amd.pipeline import solve_tsp
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 3, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "3",
                 "--local_search", "multi2opt")
    plain_lines, plain = EV.run(argv)
    # without the flag: the records of the multi-move 2-opt as they are, key for key and byte for byte
    zero_lines, zero = EV.run(argv + ["--tsp_local_search_candidates", "0"])
    assert json.dumps(zero) == json.dumps(plain)
    assert list(plain[0]) == ["split", "index", "source", "n_nodes", "gt_cost", "solved_cost", "all_costs", "merged_costs",
                              "2opt_iterations", "merge_iterations", "seed", "tour", "two_opt_moves"]
    assert not any(k.startswith("tsp_local_search_c") for k in plain_lines[0])
    volatile = ("wall_s", "instances_per_s", "stages_s")
    assert {k: v for k, v in zero_lines[0].items() if k not in volatile} == {k: v for k, v in plain_lines[0].items() if k not in volatile}
    examples = read_tsp_split(split)
    for K, closing in ((6, "full"), (3, "none")):
        flags = ["--tsp_local_search_candidates", str(K), "--tsp_local_search_closing", closing]
        lines, recs = EV.run(argv + flags)
        assert lines[0]["tsp_local_search_candidates"] == K and lines[0]["tsp_local_search_closing"] == closing
        for r, p in zip(recs, plain):
            assert list(r) == list(p) + ["two_opt_full_sweeps", "tsp_local_search_candidates", "tsp_local_search_closing"]
            assert (r["tsp_local_search_candidates"], r["tsp_local_search_closing"]) == (K, closing)
            assert r["merged_costs"] == p["merged_costs"] and r["solved_cost"] < min(r["merged_costs"])
            m = TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=r["seed"])
            one = solve_tsp(m, examples[r["index"]].points, -1, two_opt_iterations=100, generator=torch.Generator().manual_seed(r["seed"]),
                            local_search="multi2opt", local_search_candidates=K, local_search_closing=closing == "full")
            want = EV.tsp_record("val", r["index"], examples[r["index"]], r["seed"], one)
            assert {k: v for k, v in r.items() if not k.startswith("tsp_local_search")} == want
        assert recs == EV.run(argv + flags + ["--instances_per_call", "1"])[1]
