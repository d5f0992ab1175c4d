"""The neighbour-list multi-move 2-opt without a GPU: the numpy restatement of the rule (tests/nbr_two_opt_emulation.py) against
the rule's consequences and the full-sweep emulation, the workspace function, and every refusal of the new entries with its text.

Instances: ``multi_two_opt_emulation.instance`` (uniform points, random-permutation start) or a nearest-neighbour start."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import multi_two_opt_emulation as E
import nbr_two_opt_emulation as NB
from difusco_amd import _lib
from difusco_amd.decode import (batched_nbr_two_opt_grouped, batched_nbr_two_opt_ragged, batched_nbr_two_opt_torch,
                                check_tsp_candidates, tsp_candidate_lists)


def start_tour(n, kind, s=1):
    pts, tour = E.instance(n, s)
    return pts, (tour if kind == "random" else E.nearest_neighbour_tour(pts))


@functools.lru_cache(maxsize=None)
def run(n, kind, K, closing):
    pts, start = start_tour(n, kind)
    log = []
    tours, sweeps, full, moves = NB.nbr_two_opt(pts, start[None], NB.knn_lists(pts, K), closing, 1000, 4, log=log)
    return pts, start, tours[0], sweeps, full, moves, log


# ---- the emulation against the rule's consequences ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "nearest"])
@pytest.mark.parametrize("n", [5, 8, 40])
def test_lists_of_all_other_cities_are_the_multi_move_two_opt(n, kind):
    pts, start = start_tour(n, kind)
    starts = np.stack([start, start_tour(n, "random", 2)[1]])
    for cap in (1000, 2):
        want = E.multi_two_opt(pts, starts, cap, 4)
        for closing in (True, False):
            got = NB.nbr_two_opt(pts, starts, NB.all_others(n), closing, cap, 4)
            assert np.array_equal(got[0], want[0]) and (got[1], got[3]) == want[1:] and got[2] == 0


@pytest.mark.parametrize("kind", ["random", "nearest"])
@pytest.mark.parametrize("n,K", [(8, 2), (40, 2), (40, 8), (120, 3)])
def test_consequences_of_the_rule(n, K, kind):
    pts, start, tour, sweeps, full, moves, log = run(n, kind, K, True)
    assert tour[0] == tour[n] == start[0] and sorted(tour[:-1]) == list(range(n))
    assert sweeps == len(log) < 1000 and moves == sum(len(w) for _, _, w in log)
    assert full == sum(ph for _, ph, _ in log) and [ph for _, ph, _ in log] == sorted(ph for _, ph, _ in log)
    assert all(ch < -1e-6 and 0 <= i and i + 2 <= j <= n - 1 for _, _, w in log for ch, i, j in w)
    assert E.tour_length(pts, start) - E.tour_length(pts, tour) > 1e-6 * moves - 1e-12 * n
    # closed below the cap: one more full sweep applies nothing
    again = E.multi_two_opt(pts, tour[None], 1000, 4)
    assert again[1:] == (0, 0) and np.array_equal(again[0][0], tour)
    # without closing: the neighbour sweeps of the same search, and never a longer tour than the start
    o_tour, o_sweeps, o_full, o_moves = run(n, kind, K, False)[2:6]
    assert o_full == 0 and o_sweeps == sweeps - full and E.tour_length(pts, o_tour) <= E.tour_length(pts, start)
    assert np.array_equal(o_tour, tour) == (full == 0)


def test_a_neighbour_sweep_sees_its_candidates_only():
    pts, start = start_tour(40, "random")
    lists = NB.knn_lists(pts, 3)
    L = NB.listed(lists, 40)
    change, i, j = NB.proposals(pts, start, L | L.T)
    all_c = E.row_changes(pts, start, 0, 38)
    t = start
    for c, a, b in zip(change, i, j):
        heads = L[t[a], t[b]] or L[t[b], t[a]]
        tails = L[t[a + 1], t[b + 1]] or L[t[b + 1], t[a + 1]]
        assert (heads or tails) and c == all_c[a, b] and c < -1e-6
    assert 0 < len(i) <= len(E.proposals(pts, start)[1])


def test_pads_only_propose_nothing():
    pts, start = start_tour(33, "random")
    for pad in (-1, 33, 10 ** 6):
        lists = np.full((33, 4), pad, dtype=np.int32)
        lists[:, 1] = np.arange(33)                               # the city itself is a pad too
        tours, sweeps, full, moves = NB.nbr_two_opt(pts, start[None], lists, False, 1000, 4)
        assert np.array_equal(tours[0], start) and (sweeps, full, moves) == (0, 0, 0)
        tours, sweeps, full, moves = NB.nbr_two_opt(pts, start[None], lists, True, 1000, 4)
        want = E.multi_two_opt(pts, start[None], 1000, 4)
        assert np.array_equal(tours, want[0]) and (sweeps, moves) == want[1:] and full == sweeps


def test_caps_count_both_phases():
    pts, start, tour, sweeps, full, moves, log = run(120, "nearest", 3, True)
    assert full >= 1 and sweeps - full >= 1
    for cap in (0, 1, sweeps - full, sweeps - 1):
        got = NB.nbr_two_opt(pts, start[None], NB.knn_lists(pts, 3), True, cap, 4)
        assert got[1] == cap and got[2] == max(0, cap - (sweeps - full)) and got[3] == sum(len(w) for _, _, w in log[:cap])


# ---- the workspace function ----------------------------------------------------------------------------------------------------
def ws_bytes(ns, ts, K, closing):
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    n, t = np.array(ns, dtype=np.int32), np.array(ts, dtype=np.int32)
    assert L.difusco_tsp_nbr_two_opt_ragged_workspace_bytes(len(ns), n.ctypes.data, t.ctypes.data, K, closing, ctypes.byref(nbytes)) == 0
    return nbytes.value


def test_exported_symbols_and_workspace():
    L = _lib.lib()
    assert hasattr(L, "difusco_tsp_nbr_two_opt_ragged") and hasattr(L, "difusco_tsp_nbr_two_opt_ragged_workspace_bytes")
    assert L.difusco_abi_version() == 13
    base = ws_bytes([33], [3], 8, 1)
    # at least the selection's tables and the rows of every tour: 6 levels of 34 keys (12 B), 33 rows of pos / key / value / column
    assert base > 3 * (6 * 34 * 12 + 33 * (4 + 8 + 8 + 4))
    assert ws_bytes([4], [1], 1, 0) > 0
    sizes = [ws_bytes([n], [3], 8, 1) for n in (4, 5, 33, 64, 65, 1025, 5000)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert [ws_bytes([33], [3], K, 1) for K in (1, 8, 32)] == sorted(ws_bytes([33], [3], K, 1) for K in (1, 8, 32))
    assert ws_bytes([33], [3], 8, 0) <= ws_bytes([33], [3], 8, 1)
    assert ws_bytes([33], [1], 8, 1) < ws_bytes([33], [2], 8, 1)
    # a group's share of a call is what it needs alone, up to the 256-byte rounding of each of the 19 arrays and the fixed tables
    alone = ws_bytes([33], [3], 8, 1) + ws_bytes([257], [2], 8, 1)
    assert abs(ws_bytes([33, 257], [3, 2], 8, 1) - alone) <= 19 * 256 * 2


def test_c_entries_reject_bad_arguments_without_gpu():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    n_ok, t_ok = np.array([5, 33], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    outs3 = tuple(np.zeros(2, np.int64) for _ in range(3))
    err = lambda: L.difusco_last_error().decode()
    size = lambda n=n_ok, t=t_ok, g=2, K=8, closing=1: L.difusco_tsp_nbr_two_opt_ragged_workspace_bytes(
        g, n.ctypes.data, t.ctypes.data, K, closing, ctypes.byref(nbytes))
    assert size(g=0) < 0 and "groups" in err()
    assert size(n=np.array([3, 33], dtype=np.int32)) < 0 and "n >= 4" in err()
    assert size(n=np.array([5, 65535 * 16 + 1], dtype=np.int32)) < 0 and "nodes" in err()
    assert size(t=np.array([1, 0], dtype=np.int32)) < 0 and "tours" in err()
    assert size(t=np.array([1, 65535], dtype=np.int32)) < 0
    assert size(K=0) < 0 and "K = 0" in err()
    assert size(K=-3) < 0 and "K = -3" in err()
    assert size(closing=2) < 0 and "closing = 2" in err()
    assert size(closing=-1) < 0 and "closing" in err()
    assert L.difusco_tsp_nbr_two_opt_ragged_workspace_bytes(2, None, t_ok.ctypes.data, 8, 1, ctypes.byref(nbytes)) < 0
    assert L.difusco_tsp_nbr_two_opt_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, 8, 1, None) < 0 and "bytes" in err()
    assert size() == 0

    def call(points=p, tours=p, nbr=p, K=8, closing=1, cap=10, select_rounds=4, ws=p, ws_bytes=None, outs=outs3):
        o = [None if x is None else x.ctypes.data for x in outs]
        return L.difusco_tsp_nbr_two_opt_ragged(2, n_ok.ctypes.data, t_ok.ctypes.data, points, tours, nbr, K, closing, cap,
                                                select_rounds, ws, nbytes.value if ws_bytes is None else ws_bytes, *o, None)
    # every refusal comes before any GPU work: the device pointers are not memory
    assert call(nbr=None) < 0 and "neighbors" in err()
    assert call(K=0) < 0 and "K = 0" in err()
    assert call(closing=3) < 0 and "closing = 3" in err()
    assert call(select_rounds=0) < 0 and "select_rounds" in err()
    assert call(cap=-1) < 0 and "max_iterations" in err()
    assert call(points=None) < 0 and call(tours=None) < 0 and call(ws=None) < 0
    for k in range(3):
        assert call(outs=tuple(None if i == k else x for i, x in enumerate(outs3))) < 0 and "_out" in err()
    assert call(ws_bytes=nbytes.value - 1) < 0 and "workspace" in err()


# ---- the Python checks ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pts = np.random.default_rng(0).random((20, 2))
    tour = np.concatenate([np.arange(20), [0]])[None]
    lists = NB.knn_lists(pts, 4)
    calls = [lambda nb=lists, **kw: batched_nbr_two_opt_torch(pts, tour, neighbors=nb, **kw),
             lambda nb=lists, **kw: batched_nbr_two_opt_grouped(pts[None], tour, neighbors=None if nb is None else nb[None], **kw),
             lambda nb=lists, **kw: batched_nbr_two_opt_ragged([pts], [tour], neighbors=None if nb is None else [nb], **kw)]
    for call in calls:
        with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
            call(device="cpu")
        with pytest.raises(ValueError, match="select_rounds"):
            call(select_rounds=0)
        with pytest.raises(ValueError, match="max_iterations"):
            call(max_iterations=-1)
        with pytest.raises(ValueError, match=r"must be \[20, K\]"):
            call(nb=lists[:19])
        with pytest.raises(ValueError, match=r"must be \[20, K\]"):
            call(nb=lists[:, :0])
        with pytest.raises(ValueError, match="must be integers"):
            call(nb=lists.astype(np.float32))
        with pytest.raises(ValueError, match="candidates = 20"):
            call(nb=None, candidates=20)
        with pytest.raises(ValueError, match="candidates = 0"):
            call(nb=None, candidates=0)
    with pytest.raises(ValueError, match=r"must be \[20, K\]"):
        batched_nbr_two_opt_torch(pts, tour, neighbors=lists.reshape(-1))
    with pytest.raises(ValueError, match="closed tours"):
        batched_nbr_two_opt_torch(pts, tour[:, :-1], neighbors=lists)
    with pytest.raises(ValueError, match="neighbour arrays"):
        batched_nbr_two_opt_ragged([pts, pts], [tour, tour], neighbors=[lists])
    with pytest.raises(ValueError, match="one K"):
        batched_nbr_two_opt_ragged([pts, pts], [tour, tour], neighbors=[lists, lists[:, :3]])


def test_check_tsp_candidates():
    assert check_tsp_candidates("2opt", 0) == 0 and check_tsp_candidates("multi2opt", 8) == 8
    for ls in ("2opt", "2opt+oropt", "multi2opt+oropt"):
        with pytest.raises(ValueError, match="needs local_search='multi2opt'"):
            check_tsp_candidates(ls, 5)
    with pytest.raises(ValueError, match="neither kicks nor windows"):
        check_tsp_candidates("multi2opt", 5, kicks=3)
    with pytest.raises(ValueError, match="neither kicks nor windows"):
        check_tsp_candidates("multi2opt", 5, window=64)
    with pytest.raises(ValueError, match="resident"):
        check_tsp_candidates("multi2opt", 5, two_opt_mode="resident")
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="local_search_candidates"):
            check_tsp_candidates("multi2opt", bad)
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    pts = np.random.default_rng(0).random((20, 2))
    for kw in (dict(local_search="2opt"), dict(local_search="multi2opt+oropt", local_search_kicks=2)):
        with pytest.raises(ValueError, match="local_search_candidates"):
            solve_tsp(model, pts, 5, local_search_candidates=4, **kw)
        with pytest.raises(ValueError, match="local_search_candidates"):
            solve_tsp_batch(model, pts[None], 5, local_search_candidates=4, **kw)
        with pytest.raises(ValueError, match="local_search_candidates"):
            solve_tsp_batch(model, [pts, pts[:10]], 5, local_search_candidates=4, **kw)


def test_candidate_lists_from_an_edge_index():
    """Self dropped wherever it stands, order kept, local ids - on the CPU (torch only)."""
    nb = torch.tensor([[0, 2, 1, 3], [2, 1, 0, 3], [3, 0, 1, 2],      # graph 0: nodes 0 .. 2 (+ a node 3), self first / second / last
                       [3, 0, 1, 2]])
    rows = torch.arange(4).repeat_interleave(4)
    ei = torch.stack([rows, nb.reshape(-1)])
    one = tsp_candidate_lists(ei, [4], 3)[0]
    assert one.dtype == torch.int32 and one.tolist() == [[2, 1, 3], [2, 0, 3], [3, 0, 1], [0, 1, 2]]
    assert tsp_candidate_lists(ei, [4], 2)[0].tolist() == [[2, 1], [2, 0], [3, 0], [0, 1]]
    two = tsp_candidate_lists(torch.cat([ei, ei + 4], dim=1), [4, 4], 3)
    assert [t.tolist() for t in two] == [one.tolist()] * 2
    assert [t.tolist() for t in tsp_candidate_lists([ei, ei], [4, 4], 3)] == [one.tolist()] * 2
    with pytest.raises(ValueError, match="candidates = 4"):
        tsp_candidate_lists(ei, [4], 4)


def test_evaluate_flags():
    from difusco_amd import evaluate as EV
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    args = EV.parse_args(base)[0]
    assert (args.tsp_local_search_candidates, args.tsp_local_search_closing) == (0, "full")
    args = EV.parse_args(base + ["--local_search", "multi2opt", "--tsp_local_search_candidates", "8"])[0]
    assert (args.tsp_local_search_candidates, args.tsp_local_search_closing) == (8, "full")
    args = EV.parse_args(base + ["--local_search", "multi2opt", "--tsp_local_search_candidates", "5",
                                 "--tsp_local_search_closing", "none"])[0]
    assert (args.tsp_local_search_candidates, args.tsp_local_search_closing) == (5, "none")
    for bad in (["--tsp_local_search_candidates", "8"],                                           # needs multi2opt
                ["--local_search", "multi2opt+oropt", "--tsp_local_search_candidates", "8"],
                ["--local_search", "multi2opt", "--tsp_local_search_candidates", "-1"],
                ["--local_search", "multi2opt", "--tsp_local_search_closing", "none"],            # needs K > 0
                ["--local_search", "multi2opt", "--tsp_local_search_candidates", "8", "--tsp_local_search_closing", "some"]):
        with pytest.raises(SystemExit):
            EV.parse_args(base + bad)
    with pytest.raises(SystemExit):
        EV.parse_args(["--task", "mis", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", ".",
                       "--local_search", "multi2opt", "--tsp_local_search_candidates", "8"])
    info = {"merge_iterations": 1.0, "two_opt_iterations": 7, "merged_costs": [4.0], "two_opt_moves": 31,
            "local_search_candidates": 8, "local_search_closing": True, "two_opt_full_sweeps": 2}
    ex = types.SimpleNamespace(source=["f", 0], points=np.zeros((4, 2)), tour=[0, 1, 2, 3, 0])
    rec = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    assert rec["2opt_iterations"] == 7 and rec["two_opt_moves"] == 31 and rec["two_opt_full_sweeps"] == 2
    del info["two_opt_full_sweeps"]
    assert "two_opt_full_sweeps" not in EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
