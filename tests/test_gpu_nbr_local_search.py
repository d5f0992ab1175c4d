"""The neighbour-list multi-move 2-opt + Or-opt search on the GPU (``difusco_tsp_nbr_local_search_ragged``): tours and all seven
counters equal the numpy restatement of the rule (tests/nbr_local_search_emulation.py) bit for bit.  Sizes sit at the edges of the
kernels: 4 .. 7 are where the L = 3 bounds and the wrap of position n bite, 9 is the size of the brute-force host test, 33, 64
and 65 are around a wave, 257 is one past a block of the walk, 1025 one past a column chunk of the full sweeps.  Then the full
lists against the multi-move local search, list hygiene, the wrap of position n, a segment that ends at position n - 1,
independence of the groups of a call, and the wrappers, solvers and the evaluation runner.

Every case of ``test_against_the_emulation`` is one size and one K; inside it runs closing on and off and the pairs
``CONFIGS`` of (max_iterations, max_rounds) - every cap of {0, 1, 3, 1000} and every max_rounds of {1, 2, 16} - on groups of 1
and 3 tours with random-permutation and nearest-neighbour starts, each combination as one ragged call.  At n = 1025 the
emulation alone needs seconds per search to convergence, so there only the nearest-neighbour tour runs uncapped, with closing,
and one tour of either start runs the capped pairs; at n = 257 one tour of either start runs uncapped.  At n <= 9 a fifth
group of 24 random tours joins every call; still few tours that small leave an Or-opt move behind their 2-opt phase, so
``EDGE_CASES`` pins, per small size, instances on which the neighbour-stage Or-opt sweep does move."""
import functools
import json

import numpy as np
import pytest
import torch

import multi_local_search_emulation as M
import multi_two_opt_emulation as E
import nbr_local_search_emulation as NL
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu

SIZES = [4, 5, 6, 7, 9, 33, 64, 65, 257, 1025]
CONFIGS = [(0, 16), (1, 16), (3, 16), (1000, 16), (1000, 1), (1000, 2), (3, 2), (1, 1)]      # (max_iterations, max_rounds)
KINDS = [("random", 1), ("random", 3), ("nearest", 1), ("nearest", 3)]
MANY = 24                                  # random start tours of the extra group at n <= 9, where few tours leave Or-opt moves


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def points(n):
    return np.random.default_rng(8000 + n).random((n, 2))


@functools.lru_cache(maxsize=None)
def lists(n, K):
    """The K nearest other cities, padded with -1 where the instance has fewer."""
    nb = NL.knn_lists(points(n), K)
    return np.concatenate([nb, np.full((n, K - nb.shape[1]), -1, dtype=np.int32)], axis=1)


@functools.lru_cache(maxsize=None)
def starts(n, kind, P):
    """P start tours: random permutations, the same ones for every P; kind "nearest": the first is the nearest-neighbour tour."""
    rng = np.random.default_rng(8100 + n)
    t = [np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(max(P, 3))][:P]
    if kind == "nearest":
        t[0] = E.nearest_neighbour_tour(points(n))
    return np.stack(t)


@functools.lru_cache(maxsize=None)
def emulated_tour(n, kind, p, K, closing, cap, max_rounds):
    """The emulated search of tour p of ``starts(n, kind, 3)``: computed once per tour, shared by the groups that hold it."""
    return NL.search_tour(points(n), starts(n, kind, max(3, p + 1))[p], lists(n, K), closing, cap, max_rounds, 4)


def emulated(n, kind, P, K, closing, cap, max_rounds):
    runs = [emulated_tour(n, kind if p == 0 else "random", p, K, closing, cap, max_rounds) for p in range(P)]
    return np.stack([r[0] for r in runs]), reduce_counters([r[1] for r in runs])


def reduce_counters(cs):
    return {k: (sum if k in ("two_opt_moves", "or_opt_moves") else max)(c[k] for c in cs) for k in NL.COUNTERS}


def _same(tours, stats, g, want):
    ref, counters = want
    got = {k: int(np.asarray(stats[k]).reshape(-1)[g]) for k in NL.COUNTERS}
    assert got == counters, (g, got, counters)
    assert np.array_equal(tours, ref), g


def _ragged(dev, groups, nbr, closing, cap=1000, max_rounds=16, **kw):
    """One ragged call on [(points, start tours)], the lists of every group in ``nbr``: (tours, stats)."""
    from difusco_amd.decode import batched_nbr_local_search_ragged
    tours, stats = batched_nbr_local_search_ragged([g[0] for g in groups], [g[1] for g in groups], cap, device=dev, neighbors=nbr,
                                                   closing=closing, max_rounds=max_rounds, **kw)
    assert set(stats) == set(NL.COUNTERS)
    assert all(stats[k].dtype == (np.int32 if k in ("rounds", "full_rounds") else np.int64) for k in stats)
    return tours, stats


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_against_the_emulation(dev, n, K):
    closed_some = moved_some = False
    for closing in (True, False):
        for cap, max_rounds in CONFIGS:
            kinds = KINDS + ([("random", MANY)] if n <= 9 else [])
            if n >= 257 and cap == 1000:                          # the emulation to convergence: fewer searches
                if max_rounds == 1 or (max_rounds == 2 and not closing) or (n == 1025 and (max_rounds, closing) != (16, True)):
                    continue
                kinds = [("nearest", 1)] if n == 1025 else [("nearest", 1), ("random", 1)]
            elif n == 1025:
                if (cap, max_rounds) in ((3, 2), (1, 1)):
                    continue
                kinds = [("nearest", 1), ("random", 1)]
            tours, stats = _ragged(dev, [(points(n), starts(n, kind, P)) for kind, P in kinds], [lists(n, K)] * len(kinds), closing,
                                   cap, max_rounds)
            for g, (kind, P) in enumerate(kinds):
                want = emulated(n, kind, P, K, closing, cap, max_rounds)
                _same(tours[g], stats, g, want)
                closed_some |= want[1]["full_sweeps"] > 0
                moved_some |= want[1]["or_opt_moves"] > 0
    assert moved_some or n <= 9                                   # Or-opt moves were applied (n <= 9: see EDGE_CASES below)
    assert closed_some or K > 1 or n <= 9                         # the full stage moved: lists of one city leave moves behind


def test_clustered_points_where_round_two_moves(dev):
    pts, tour = M.clustered_instance(64, 10)
    others = np.stack([tour, np.concatenate([[0], np.random.default_rng(5).permutation(63) + 1, [0]])])
    two_rounds = False
    for K in (3, 8):
        nbr = NL.knn_lists(pts, K)
        for closing in (True, False):
            for max_rounds in (1, 2, 16):
                want = NL.nbr_local_search(pts, others, nbr, closing, 1000, max_rounds, 4)
                tours, stats = _ragged(dev, [(pts, others)], [nbr], closing, 1000, max_rounds)
                _same(tours[0], stats, 0, want)
                two_rounds |= want[1]["rounds"] >= 2
    assert two_rounds


@pytest.mark.parametrize("n", [5, 33, 64])
def test_full_lists_equal_the_multi_move_local_search(dev, n):
    from difusco_amd.decode import (batched_multi_local_search_grouped, batched_multi_local_search_ragged,
                                    batched_multi_local_search_torch, batched_nbr_local_search_grouped,
                                    batched_nbr_local_search_ragged, batched_nbr_local_search_torch)
    pts, t3, t1, every = points(n), starts(n, "random", 3), starts(n, "nearest", 1), NL.all_others(n)
    shared = lambda st: {k: st[k] for k in ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")}
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in b)
    for closing in (True, False):
        for cap, max_rounds in ((1000, 16), (2, 16), (1000, 1)):
            kw = dict(device=dev, max_rounds=max_rounds)
            want = batched_multi_local_search_torch(pts, t3, cap, **kw)
            got = batched_nbr_local_search_torch(pts, t3, cap, neighbors=every, closing=closing, **kw)
            assert np.array_equal(got[0], want[0]) and shared(got[1]) == want[1] and got[1]["full_sweeps"] == 0
            assert got[1]["full_rounds"] <= int(closing)
            if closing and (cap, max_rounds) == (1000, 16):
                assert got[1]["full_rounds"] == 1                 # below both caps the closing phases ran, and found nothing
            want = batched_multi_local_search_grouped(np.stack([pts, pts]), np.concatenate([t3, t3[::-1]]), cap, **kw)
            got = batched_nbr_local_search_grouped(np.stack([pts, pts]), np.concatenate([t3, t3[::-1]]), cap,
                                                   neighbors=np.stack([every, every]), closing=closing, **kw)
            assert np.array_equal(got[0], want[0]) and same(shared(got[1]), want[1]) and not got[1]["full_sweeps"].any()
            want = batched_multi_local_search_ragged([pts, pts], [t3, t1], cap, **kw)
            got = batched_nbr_local_search_ragged([pts, pts], [t3, t1], cap, neighbors=[every, every], closing=closing, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0])) and same(shared(got[1]), want[1])
            assert not got[1]["full_sweeps"].any()


@pytest.mark.parametrize("n,K", [(65, 1), (257, 3), (257, 8)])
def test_closed_results_are_local_optima(dev, n, K):
    from difusco_amd.decode import batched_multi_local_search_torch, batched_nbr_local_search_torch
    pts, t = points(n), starts(n, "nearest", 3)
    tours, stats = batched_nbr_local_search_torch(pts, t, device=dev, neighbors=lists(n, K))
    assert 0 < stats["two_opt_sweeps"] + stats["or_opt_sweeps"] < 1000 and stats["rounds"] < 16 and stats["full_rounds"] >= 1
    again, more = batched_multi_local_search_torch(pts, tours, device=dev)
    assert more["two_opt_moves"] == 0 and more["or_opt_moves"] == 0 and np.array_equal(again, tours)
    for a, b in zip(t, tours):
        assert E.tour_length(pts, b) < E.tour_length(pts, a)


# (what the case is, n and seed of multi_two_opt_emulation.instance, K, the Or-opt winner (v, i, j) of a neighbour sweep): found by
# running the emulation over seeds; the test re-derives every property from the emulation's log before it trusts the case
EDGE_CASES = [
    ("j = n-1: the insertion edge (b, tour[0]) alone is listed", 10, 3, 2, (0, 0, 9)),
    ("j = n-1: (b, tour[0]) is listed only from the anchor's side, by tour[0]", 13, 148, 2, (0, 7, 12)),
    ("j = n-1 and a reversed segment of three from position 1, anchor's side only", 10, 369, 2, (4, 0, 9)),
    ("a city at position n-1 moves", 10, 58, 2, (0, 8, 7)),
    ("a segment of two ends at position n-1", 10, 197, 2, (1, 7, 0)),
    ("a reversed segment of two ends at position n-1", 10, 61, 2, (2, 7, 0)),
    ("a segment of three ends at position n-1", 10, 217, 3, (3, 6, 0)),
    ("a reversed segment of three ends at position n-1", 10, 346, 2, (4, 6, 0)),
    ("a segment of three starts at position 1 and goes to j = n-1", 10, 71, 3, (3, 0, 9)),
    # the smallest tours on which a neighbour-stage Or-opt sweep moves a segment of every length that fits and was found
    ("n = 4, one city", 4, 3, 1, (0, 1, 3)),
    ("n = 5, one city", 5, 1, 1, (0, 0, 2)),
    ("n = 5, two cities reversed", 5, 3, 1, (2, 1, 0)),
    ("n = 6, one city to j = n-1", 6, 1, 1, (0, 0, 5)),
    ("n = 6, two cities reversed", 6, 8, 1, (2, 0, 3)),
    ("n = 6, three cities reversed", 6, 21, 1, (4, 1, 0)),
    ("n = 7, two cities reversed to j = n-1", 7, 25, 1, (2, 0, 6)),
    ("n = 7, three cities to j = n-1", 7, 12, 2, (3, 0, 6)),
    ("n = 9, one city to j = 0", 9, 0, 1, (0, 7, 0)),
    ("n = 9, two cities reversed to j = n-1", 9, 2, 2, (2, 4, 8)),
    ("n = 9, three cities reversed", 9, 12, 1, (4, 2, 6)),
]


@pytest.mark.parametrize("what,n,seed,K,move", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_position_n_wrap_and_segments_at_the_ends(dev, what, n, seed, K, move):
    from or_opt_emulation import VARIANTS
    pts, tour = E.instance(n, seed)
    nbr = NL.knn_lists(pts, K)
    listed = NL.listed(nbr, n)
    S = listed | listed.T
    v, i, j = move
    L, rev = VARIANTS[v]
    for closing in (False, True):
        log = []
        want = NL.search_tour(pts, tour, nbr, closing, 1000, 16, 4, log=log)
        hits = [before for stage, kind, before, ws in log if (stage, kind) == ("nbr", "oropt") and move in [w[1:] for w in ws]]
        assert hits, what                                         # the move is a winner of a neighbour-stage Or-opt sweep
        t = hits[0]
        a, b = (t[i + L], t[i + 1]) if rev else (t[i + 1], t[i + L])
        if what.startswith("j = n-1"):                            # found through the edge that ends at tour[n] = tour[0] alone
            assert j == n - 1 and not S[t[j], a] and S[t[0], b], what
        if "anchor's side" in what:
            assert b in nbr[t[0]] and t[0] not in nbr[b], what
        if "position n-1" in what:
            assert i + L == n - 1, what
        tours, stats = _ragged(dev, [(pts, tour[None])], [nbr], closing)
        _same(tours[0], stats, 0, (want[0][None], want[1]))


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
            want = NL.nbr_local_search(pts, t, nbr, closing, 1000, 16, 4)
            tours, stats = _ragged(dev, [(pts, t)], [nbr], closing)
            _same(tours[0], stats, 0, want)
            moves = want[1]["two_opt_moves"] + want[1]["or_opt_moves"]
            assert (moves > 0) == (closing or name != "pads only"), name


def test_coincident_cities_and_an_optimal_tour(dev):
    n = 40
    pts = points(n).copy()
    pts[5] = pts[6] = pts[7]                                      # three cities on one spot
    pts[20] = pts[30]
    nbr = NL.knn_lists(pts, 5)
    t = starts(n, "random", 3)
    for closing in (True, False):
        want = NL.nbr_local_search(pts, t, nbr, closing, 1000, 16, 4)
        assert want[1]["or_opt_moves"] > 0
        tours, stats = _ragged(dev, [(pts, t)], [nbr], closing)
        _same(tours[0], stats, 0, want)
    best, c = NL.search_tour(points(n), starts(n, "random", 1)[0], lists(n, 5), True, 1000, 16, 4)      # a local optimum
    for closing in (True, False):
        tours, stats = _ragged(dev, [(points(n), best[None])], [lists(n, 5)], closing)
        zero = dict.fromkeys(NL.COUNTERS, 0)
        zero.update(rounds=1, full_rounds=int(closing))
        _same(tours[0], stats, 0, (best[None], zero))


INDEPENDENT = [4, 5, 6, 7, 9, 33, 64, 65, 100, 130, 257]


def test_groups_do_not_depend_on_their_company(dev):
    K = 3
    groups = [(points(n), starts(n, "nearest", 1 + g % 3)) for g, n in enumerate(INDEPENDENT)]
    nbr = [lists(n, K) for n in INDEPENDENT]
    alone = []
    for g in range(len(groups)):
        tours, stats = _ragged(dev, [groups[g]], [nbr[g]], True)
        alone.append((tours[0], {k: int(stats[k][0]) for k in NL.COUNTERS}))
    _same(alone[5][0], {k: [v] for k, v in alone[5][1].items()}, 0, emulated(33, "nearest", 3, K, True, 1000, 16))
    for order in (list(range(11)), list(range(10, -1, -1)), [3, 8, 8, 0, 10, 8]):
        tours, stats = _ragged(dev, [groups[g] for g in order], [nbr[g] for g in order], True)
        for k, g in enumerate(order):
            _same(tours[k], stats, k, alone[g])
    # every tour gets its solo answer: the tours of a group of three, one by one
    g = 5
    for p in range(3):
        tours, stats = _ragged(dev, [(groups[g][0], groups[g][1][p:p + 1])], [nbr[g]], True)
        assert np.array_equal(tours[0][0], alone[g][0][p])


# ---- wrappers, solvers and the runner -----------------------------------------------------------------------------------------
def test_lists_built_by_the_wrappers(dev):
    from difusco_amd.decode import (batched_nbr_local_search_grouped, batched_nbr_local_search_ragged,
                                    batched_nbr_local_search_torch, tsp_candidate_lists)
    from difusco_amd.graph import knn_edge_index_gpu
    ns, K = [33, 65, 257], 5
    groups = [(points(n), starts(n, "nearest", 2)) for n in ns]
    ei = knn_edge_index_gpu(np.concatenate([g[0] for g in groups]), K + 1, device=dev, sizes=ns)
    explicit = tsp_candidate_lists(ei, ns, K)
    built = batched_nbr_local_search_ragged([g[0] for g in groups], [g[1] for g in groups], device=dev, candidates=K)
    given = batched_nbr_local_search_ragged([g[0] for g in groups], [g[1] for g in groups], device=dev, neighbors=explicit)
    assert all(np.array_equal(a, b) for a, b in zip(built[0], given[0]))
    assert all(np.array_equal(built[1][k], given[1][k]) for k in NL.COUNTERS) and built[1]["or_opt_moves"].min() > 0
    for g, n in enumerate(ns):
        _same(built[0][g], built[1], g, NL.nbr_local_search(groups[g][0], groups[g][1], NL.knn_lists(points(n), K), True))
    solo, st = batched_nbr_local_search_torch(*groups[1], device=dev, candidates=K)
    assert np.array_equal(solo, built[0][1]) and st == {k: int(built[1][k][1]) for k in NL.COUNTERS}
    assert all(isinstance(v, int) for v in st.values())
    two, st2 = batched_nbr_local_search_grouped(np.stack([groups[1][0]] * 2), np.concatenate([groups[1][1]] * 2), device=dev,
                                                candidates=K, closing=False)
    open_, st1 = batched_nbr_local_search_torch(*groups[1], device=dev, candidates=K, closing=False)
    assert np.array_equal(two, np.concatenate([open_, open_])) and all(st2[k].tolist() == [st1[k]] * 2 for k in NL.COUNTERS)
    assert st1["full_rounds"] == 0 and st1["full_sweeps"] == 0


def test_solvers_run_the_search_on_the_lists_of_the_instance_graph(dev):
    from difusco_amd import TSPModel
    from difusco_amd.decode import batched_nbr_local_search_torch, tsp_candidate_lists
    from difusco_amd.graph import knn_edge_index_gpu
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch, tour_length
    from difusco_amd.synthetic import random_state_dict
    sd = random_state_dict(64, 2, 2, seed=0)
    pts = np.random.default_rng(14).random((2, 50, 2)).astype(np.float32).astype(np.float64)
    model = lambda seed: TSPModel(_model_args(sparse_factor=8, hidden_dim=64, n_layers=2), sd, device=dev, seed=seed)
    kw = dict(parallel_sampling=2, local_search="nbr2opt+oropt")
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(2)]
    for K, closing in ((5, True), (7, False), (12, True)):        # 12 > sparse_factor - 1: a k-NN call of the search's own
        nkw = dict(two_opt_iterations=100, local_search_candidates=K, local_search_closing=closing, **kw)
        res = solve_tsp_batch(model(0), pts, 8, seeds=[5, 6], generators=gens(), **nkw)
        lst = solve_tsp_batch(model(0), [pts[0], pts[1][:40]], 8, seeds=[5, 6], generators=gens(), **nkw)
        for b in range(2):
            solo = solve_tsp(model(5 + b), pts[b], 8, generator=torch.Generator().manual_seed(b), **nkw)
            assert res[b] == solo
            info = solo[3]
            assert info["local_search_candidates"] == K and info["local_search_closing"] is closing
            assert {"two_opt_iterations", "or_opt_iterations", "two_opt_moves", "or_opt_moves", "local_search_rounds",
                    "local_search_full_sweeps", "local_search_full_rounds"} <= set(info)
            assert 0 <= info["local_search_full_sweeps"] <= info["two_opt_iterations"] + info["or_opt_iterations"]
            assert info["local_search_full_rounds"] >= 1 if closing else info["local_search_full_rounds"] == 0
            assert sorted(solo[0][:-1]) == list(range(50)) and solo[1] < min(info["merged_costs"])
        assert lst[0] == res[0]                                   # a list of mixed sizes: every instance its solo answer
        short = solve_tsp(model(6), pts[1][:40], 8, generator=torch.Generator().manual_seed(1), **nkw)
        assert lst[1] == short
    # the decode call on the same lists and the same merged tours
    K = 5
    captured = {}
    import difusco_amd.decode as D
    real = D.batched_nbr_local_search_torch

    def spy(points, tours, **kw):
        captured.update(points=np.array(points), tours=np.array(tours), neighbors=kw["neighbors"])
        return real(points, tours, **kw)
    D.batched_nbr_local_search_torch = spy
    try:
        solo = solve_tsp(model(5), pts[0], 8, generator=torch.Generator().manual_seed(0), two_opt_iterations=100,
                         local_search_candidates=K, **kw)
    finally:
        D.batched_nbr_local_search_torch = real
    want_lists = tsp_candidate_lists(knn_edge_index_gpu(pts[0], 8, device=dev), [50], K)[0]
    assert torch.equal(captured["neighbors"], want_lists) and np.array_equal(captured["points"], pts[0])
    direct, stats = batched_nbr_local_search_torch(pts[0], captured["tours"], 100, device=dev, neighbors=want_lists.cpu().numpy())
    costs = [tour_length(pts[0], t) for t in direct]
    assert solo[2] == costs and solo[0] == direct[int(np.argmin(costs))].tolist()
    assert solo[3]["two_opt_iterations"] == stats["two_opt_sweeps"] and solo[3]["or_opt_moves"] == stats["or_opt_moves"]
    assert solo[3]["local_search_full_rounds"] == stats["full_rounds"]
    want = NL.nbr_local_search(pts[0], captured["tours"], want_lists.cpu().numpy(), True, 100, 16, 4)
    _same(direct, {k: [v] for k, v in stats.items()}, 0, want)


def test_evaluate_records(dev, tmp_path):
    from difusco_amd import TSPModel, evaluate as EV
    from difusco_amd.datasets import read_tsp_split
    from difusco_amd.pipeline import solve_tsp
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 3, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 64, 2)
    base = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "3")
    plain_lines, plain = EV.run(base + ["--local_search", "multi2opt+oropt"])
    examples = read_tsp_split(split)
    for K, closing in ((6, "full"), (3, "none")):
        flags = ["--local_search", "nbr2opt+oropt", "--tsp_local_search_candidates", str(K), "--tsp_local_search_closing", closing]
        lines, recs = EV.run(base + flags)
        assert lines[0]["local_search"] == "nbr2opt+oropt"
        assert lines[0]["tsp_local_search_candidates"] == K and lines[0]["tsp_local_search_closing"] == closing
        for r, p in zip(recs, plain):
            # the fields of the multi-move local search, then the new ones
            assert list(r) == list(p) + ["local_search_full_sweeps", "local_search_full_rounds", "tsp_local_search_candidates",
                                         "tsp_local_search_closing"]
            assert (r["tsp_local_search_candidates"], r["tsp_local_search_closing"]) == (K, closing)
            assert r["merged_costs"] == p["merged_costs"] and r["solved_cost"] < min(r["merged_costs"])
            assert (r["local_search_full_rounds"] >= 1) == (closing == "full")
            m = TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=r["seed"])
            one = solve_tsp(m, examples[r["index"]].points, -1, two_opt_iterations=100, generator=torch.Generator().manual_seed(r["seed"]),
                            local_search="nbr2opt+oropt", local_search_candidates=K, local_search_closing=closing == "full")
            want = EV.tsp_record("val", r["index"], examples[r["index"]], r["seed"], one)
            assert {k: v for k, v in r.items() if not k.startswith("tsp_local_search")} == want
        assert recs == EV.run(base + flags + ["--instances_per_call", "1"])[1]
    # the other searches' records carry none of the new fields
    assert not any(k.startswith("local_search_full") or k.startswith("tsp_local_search_c") for k in plain[0])
    assert json.dumps(plain) == json.dumps(EV.run(base + ["--local_search", "multi2opt+oropt"])[1])
