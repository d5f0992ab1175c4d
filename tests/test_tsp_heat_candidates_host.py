"""The heat-ranked candidate lists on the CPU: what the rule promises (include/difusco_hip.h), asserted on its numpy restatement
(tests/tsp_heat_candidates_emulation.py) over the groups of tests/tsp_heat_candidates_cases.py; the option checks, the runner's
parser and the wrapper's refusals, which all come before any library call; the defaults of the new keyword."""
import inspect
import types

import numpy as np
import pytest
import torch

import tsp_heat_candidates_cases as C
import tsp_heat_candidates_emulation as E


def candidate_sets(n, rp, col):
    rows = E.rows_of(rp)
    sets = [set() for _ in range(n)]
    for u, v in zip(rows.tolist(), np.asarray(col).tolist()):
        if u != v:
            sets[u].add(v)
            sets[v].add(u)
    return sets


@pytest.mark.parametrize("name,K", C.PAIRS)
def test_rows_are_distinct_candidates_padded_at_the_end(name, K):
    pts, rp, col, heat = C.case(name)
    lists, listed, pads = C.expected(name, K)
    sets = candidate_sets(len(pts), rp, col)
    S, _ = E.score_table(len(pts), rp, col, heat)
    assert lists.shape == (len(pts), K) and lists.dtype == np.int32
    total_pads = 0
    for a, row in enumerate(lists):
        kept = row[row >= 0]
        assert len(set(kept.tolist())) == len(kept) and a not in kept and set(kept.tolist()) <= sets[a]
        assert np.all(row[len(kept):] == -1)                                     # pads only at the end
        assert K - len(kept) == max(0, K - len(sets[a]))
        total_pads += K - len(kept)
        keys = [(-int(S[a, b]), E.d2_table(pts[[a, b]])[0, 1], int(b)) for b in kept]
        assert keys == sorted(keys)
        rest = sets[a] - set(kept.tolist())
        if rest:                                                                 # nothing left out lists before the last one kept
            assert min((-int(S[a, b]), E.d2_table(pts[[a, b]])[0, 1], b) for b in rest) > keys[-1]
    assert pads == total_pads
    assert listed == sum(int(S[a, b] > 0) for a, row in enumerate(lists) for b in row[row >= 0])


@pytest.mark.parametrize("name,K", [p for p in C.PAIRS if p[0] != "hub1100"])
def test_entry_and_tour_order_do_not_matter(name, K):
    pts, rp, col, heat = C.permuted(name)
    got = E.lists(pts, rp, col, heat, K)
    want = C.expected(name, K)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]


def test_the_cases_hold_what_they_are_there_for():
    deg = lambda name: np.bincount(C.case(name)[2], minlength=len(C.case(name)[0]))
    assert deg("hub200")[0] >= 200 > 128 and deg("hub1100")[0] >= 1100 > 1024      # every row names city 0
    assert np.all(np.diff(C.case("hub1100")[1]) == 3)
    assert (C.expected("n3", 5)[0] == -1).any(axis=1).all()                      # pads everywhere
    pts, rp, col, _ = C.case("empty-rows")
    assert rp[6] == rp[5] and rp[8] == rp[7] and 7 not in col and np.all(C.expected("empty-rows", 4)[0][7] == -1)
    pts, rp, col, heat = C.case("duplicates")
    pairs = list(zip(E.rows_of(rp).tolist(), col.tolist()))
    assert len(set(pairs)) < len(pairs) and any(u == v for u, v in pairs)
    q = E.quantise(C.case("corners")[3])
    assert np.isnan(C.case("corners")[3]).any() and q.min() == 0 and q.max() == 65535 and E.quantise(np.float32(1e-6)) == 0
    lists = C.expected("saturated", 9)[0]
    for a in range(10):
        row = lists[a].tolist()
        if a not in (3, 4):
            assert row.index(3) + 1 == row.index(4)                              # equal S and d2: the index decides
    assert lists[3][0] == 4 and lists[4][0] == 3                                 # d2 = 0
    assert (C.expected("hub200", 128)[0][0] >= 0).all() and (C.expected("dense14", 128)[0][:, 13:] == -1).all()


def test_tour_indicator_heat_puts_the_tour_neighbours_first():
    n, P = 14, 3
    rng = np.random.default_rng(14)
    pts = rng.random((n, 2))
    rp, col = np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n)
    tour = rng.permutation(n)
    nxt, prv = np.empty(n, dtype=int), np.empty(n, dtype=int)
    nxt[tour], prv[tour] = np.roll(tour, -1), np.roll(tour, 1)
    heat = np.zeros((P, n * n), dtype=np.float32)
    heat[:, np.arange(n) * n + nxt] = 1.0                                        # a -> next(a): one direction only
    lists, listed, pads = E.lists(pts, rp, col, heat, 4)
    assert all(set(lists[a, :2].tolist()) == {int(nxt[a]), int(prv[a])} for a in range(n))
    assert listed == 2 * n and pads == 0


def test_complete_graph_with_all_other_cities_listed():
    for name, K in (("complete5", 4), ("dense14", 13), ("saturated", 9)):
        lists = C.expected(name, K)[0]
        assert all(sorted(row.tolist()) == [b for b in range(K + 1) if b != a] for a, row in enumerate(lists))


@pytest.mark.parametrize("n,k,K", [(37, 8, 5), (64, 10, 8), (200, 17, 16), (12, 5, 4), (37, 8, 7), (64, 10, 9)])
def test_zero_heat_gives_the_knn_lists(n, k, K):
    from difusco_amd.decode import tsp_candidate_lists
    pts = np.random.default_rng(n * k).random((n, 2))
    rp, col, d2 = E.knn_graph(pts, k)
    for a in range(n):                                                           # the premise: a city's distances are distinct
        assert len(np.unique(d2[a])) == n
    ei = torch.from_numpy(C.edge_index_of(rp, col))
    want = tsp_candidate_lists(ei, [n], K)[0].numpy()
    for P in (1, 2):
        got, listed, pads = E.lists(pts, rp, col, np.zeros((P, len(col)), dtype=np.float32), K)
        assert np.array_equal(got, want) and listed == 0 and pads == 0


def test_check_tsp_candidate_source():
    from difusco_amd.decode import TSP_CANDIDATE_SOURCES, check_tsp_candidate_source, check_tsp_candidates
    assert TSP_CANDIDATE_SOURCES == ("knn", "heat")
    assert check_tsp_candidate_source("knn", 0) == "knn" and check_tsp_candidate_source("knn", 8) == "knn"
    assert check_tsp_candidate_source("heat", 1) == "heat" and check_tsp_candidate_source("heat", 128) == "heat"
    for source, K in (("heat", 0), ("heat", 129), ("heat", -1), ("warm", 8), (None, 8)):
        with pytest.raises(ValueError):
            check_tsp_candidate_source(source, K)
    # check_tsp_candidates is what it was
    assert list(inspect.signature(check_tsp_candidates).parameters) == ["local_search", "candidates", "kicks", "window", "two_opt_mode"]
    assert check_tsp_candidates("multi2opt", 8) == 8 and check_tsp_candidates("nbr2opt+oropt", 3) == 3
    for bad in (("multi2opt+oropt", 8), ("nbr2opt+oropt", 0), ("multi2opt", 8, 2), ("multi2opt", 8, 0, 64)):
        with pytest.raises(ValueError):
            check_tsp_candidates(*bad)


def test_solvers_refuse_heat_lists_without_candidates():
    """Before the model is touched: a heat source with no neighbour-list search to feed."""
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace()                                              # any use of it is an AttributeError
    pts = np.random.default_rng(0).random((12, 2))
    for kw in (dict(local_search="multi2opt"), dict(local_search="2opt"), dict(local_search="multi2opt+oropt"),
               dict(local_search="multi2opt", local_search_candidates=129),
               dict(local_search="multi2opt", local_search_candidates=4, local_search_candidate_source="warm")):
        kw.setdefault("local_search_candidate_source", "heat")
        with pytest.raises(ValueError):
            solve_tsp(model, pts, 5, **kw)
        with pytest.raises(ValueError):
            solve_tsp_batch(model, pts[None], 5, **kw)
        with pytest.raises(ValueError):
            solve_tsp_batch(model, [pts], 5, **kw)


def test_defaults_are_knn():
    from difusco_amd import evaluate as EV
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    assert inspect.signature(solve_tsp).parameters["local_search_candidate_source"].default == "knn"
    assert inspect.signature(solve_tsp_batch).parameters["local_search_candidate_source"].default == "knn"
    assert inspect.signature(EV.solve_split).parameters["tsp_local_search_candidate_source"].default == "knn"


def test_evaluate_flag():
    from difusco_amd import evaluate as EV
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    assert EV.parse_args(base)[0].tsp_local_search_candidate_source == "knn"
    heat = ["--tsp_local_search_candidate_source", "heat"]
    args = EV.parse_args(base + heat + ["--local_search", "nbr2opt+oropt", "--tsp_local_search_candidates", "5"])[0]
    assert (args.tsp_local_search_candidate_source, args.tsp_local_search_candidates) == ("heat", 5)
    args = EV.parse_args(base + heat + ["--local_search", "multi2opt", "--tsp_local_search_candidates", "128"])[0]
    assert args.tsp_local_search_candidate_source == "heat"
    for bad in (heat,                                                                             # needs K >= 1
                heat + ["--local_search", "multi2opt"],
                heat + ["--local_search", "multi2opt", "--tsp_local_search_candidates", "0"],
                heat + ["--local_search", "multi2opt", "--tsp_local_search_candidates", "129"],
                heat + ["--local_search", "multi2opt+oropt", "--tsp_local_search_candidates", "5"],
                ["--tsp_local_search_candidate_source", "warm", "--local_search", "multi2opt", "--tsp_local_search_candidates", "5"]):
        with pytest.raises(SystemExit):
            EV.parse_args(base + bad)
    with pytest.raises(SystemExit):
        EV.parse_args(["--task", "mis", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."] + heat)
    info = {"merge_iterations": 1.0, "two_opt_iterations": 7, "merged_costs": [4.0], "two_opt_moves": 31, "or_opt_iterations": 3,
            "or_opt_moves": 9, "local_search_rounds": 2, "local_search_candidates": 5, "local_search_closing": True,
            "local_search_full_sweeps": 1, "local_search_full_rounds": 1}
    ex = types.SimpleNamespace(source=["f", 0], points=np.zeros((4, 2)), tour=[0, 1, 2, 3, 0])
    plain = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    rec = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0],
                                          dict(info, local_search_candidate_source="heat", local_search_heat_listed=0.75)))
    assert "heat_listed" not in plain and rec == dict(plain, heat_listed=0.75)


def test_wrapper_refuses_before_any_library_call(monkeypatch):
    from difusco_amd import _lib, decode

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(decode, "_heat_graph", lambda *a, **k: no_library())
    n, P, E_ = 12, 2, 40
    pts = np.random.default_rng(1).random((n, 2))
    ei = np.stack([np.sort(np.random.default_rng(2).integers(0, n, E_)), np.random.default_rng(3).integers(0, n, E_)])
    heat = np.zeros((P, E_), dtype=np.float32)
    dense = np.zeros((P, n, n), dtype=np.float32)
    f = decode.tsp_heat_candidate_lists
    for K in (0, 129, -3, 2.0, 2.5, True, "4", None):
        with pytest.raises(ValueError, match="candidates"):
            f(pts, heat, ei, K)
    bad = [(pts[:, :1], heat, ei), (pts.reshape(-1), heat, ei), (np.zeros((0, 2)), heat, ei),      # points
           (pts, heat[:, :-1], ei), (pts, heat, ei[:, :-1]), (pts, heat.reshape(-1), ei), (pts, heat[:0], ei),   # heat against the edges
           (pts, heat, ei[0]), (pts, heat, ei.T), (pts, dense, ei),                                # edge_index
           (pts, heat, None), (pts, dense[:, :, :-1], None), (pts, dense[0], None), (pts, dense[:0], None)]     # dense
    for p, h, e in bad:
        with pytest.raises(ValueError):
            f(p, h, e, 4)
    for p, h, e in (([pts, pts], [heat], [ei, ei]), ([pts], [heat, heat], [ei]), ([pts, pts], [heat, heat], [ei]), ([], [], []),
                    ([pts, pts], [heat, dense], [ei, None])):
        with pytest.raises(ValueError):
            f(p, h, e, 4)
    with pytest.raises(_lib.DifuscoHipError, match="GPU only"):                  # everything in order: the device is asked for last
        f(pts, heat, ei, 4, device="cpu")
    with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
        f([pts, pts], [dense, dense], None, 4, device="cpu")
