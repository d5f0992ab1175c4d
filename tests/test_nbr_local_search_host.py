"""The neighbour-list multi-move 2-opt + Or-opt search without a GPU: the numpy restatement of the rule
(tests/nbr_local_search_emulation.py) against the rule's consequences, the full search's emulation and a brute-force enumeration
of the candidate predicate; the workspace function; every refusal of the new entries with its text; the Python checks and the
runner's parser.

Instances: ``multi_two_opt_emulation.instance`` (uniform points, random-permutation start), a nearest-neighbour start, or
``multi_local_search_emulation.clustered_instance``."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import multi_local_search_emulation as M
import multi_two_opt_emulation as E
import nbr_local_search_emulation as NL
from difusco_amd import _lib
from difusco_amd.decode import (LOCAL_SEARCHES, batched_nbr_local_search_grouped, batched_nbr_local_search_ragged,
                                batched_nbr_local_search_torch, check_local_search, check_tsp_candidates)
from or_opt_emulation import VARIANTS

SHARED = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")


def start_tour(n, kind, s=1):
    pts, tour = E.instance(n, s)
    return pts, (tour if kind == "random" else E.nearest_neighbour_tour(pts))


@functools.lru_cache(maxsize=None)
def run(n, kind, K, closing):
    pts, start = (M.clustered_instance(n, 10) if kind == "clustered" else start_tour(n, kind))
    log = []
    tour, c = NL.search_tour(pts, start, NL.knn_lists(pts, K), closing, 1000, 16, 4, log=log)
    return pts, start, tour, c, log


# ---- the emulation against the full search ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "nearest"])
@pytest.mark.parametrize("n", [5, 8, 40])
def test_lists_of_all_other_cities_are_the_multi_move_local_search(n, kind):
    pts, start = start_tour(n, kind)
    starts = np.stack([start, start_tour(n, "random", 2)[1]])
    for cap, max_rounds in ((1000, 16), (3, 16), (1000, 1), (1000, 2)):
        want_t, want_c = M.multi_local_search(pts, starts, cap, max_rounds, 4)
        for closing in (True, False):
            got_t, got_c = NL.nbr_local_search(pts, starts, NL.all_others(n), closing, cap, max_rounds, 4)
            assert np.array_equal(got_t, want_t) and {k: got_c[k] for k in SHARED} == want_c
            assert got_c["full_sweeps"] == 0
            if not closing:
                assert got_c["full_rounds"] == 0
        # per tour: the closing phases ran, and found nothing, wherever the tour stopped below both caps
        for t in starts:
            _, c = NL.search_tour(pts, t, NL.all_others(n), True, cap, max_rounds, 4)
            if c["two_opt_sweeps"] + c["or_opt_sweeps"] < cap and c["rounds"] < max_rounds:
                assert c["full_rounds"] == 1
            assert c["full_rounds"] in (0, 1) and c["full_sweeps"] == 0


# ---- the Or-opt neighbour sweep against a brute-force enumeration of the predicate ------------------------------------------------
def brute_force_rows(pts, tour, lists):
    """Per row the lowest (delta, v, j) over the candidates that pass the predicate, from scalar loops over (v, i, j)."""
    t = [int(x) for x in tour]
    n = len(t) - 1
    N = [set(int(c) for c in row if 0 <= c < n and c != a) for a, row in enumerate(np.asarray(lists))]
    near = lambda x, y: y in N[x] or x in N[y]
    table = M.or_opt_row_deltas(pts, tour, 0, n - 1)
    best = {}
    for v, (L, rev) in enumerate(VARIANTS):
        for i in range(0, n - L):
            a, b = (t[i + L], t[i + 1]) if rev else (t[i + 1], t[i + L])
            for j in range(n):
                if i <= j <= i + L:
                    continue
                if near(t[j], a) or near(t[j + 1], b):
                    key = (table[i, v, j], v, j)
                    if i not in best or key < best[i]:
                        best[i] = key
    return {i: k for i, k in best.items() if k[0] < -1e-6}


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_or_opt_neighbour_sweep_is_the_predicate_on_nine_cities(s, K):
    pts, tour = E.instance(9, s)
    lists = NL.knn_lists(pts, K).copy()
    lists[2, 0] = -1                                              # a pad, a self entry and an asymmetric list
    lists[3, 0] = 3
    lists[4] = lists[4, 0]
    L = NL.listed(lists, 9)
    delta, i, v, j = NL.or_opt_proposals(pts, tour, L | L.T)
    want = brute_force_rows(pts, tour, lists)
    assert sorted(want) == list(i)
    for d, r, vv, jj in zip(delta, i, v, j):
        assert want[int(r)] == (d, int(vv), int(jj))
    full = M.or_opt_proposals(pts, tour)
    assert len(i) <= len(full[1])
    # with every other city listed the predicate holds everywhere
    La = NL.listed(NL.all_others(9), 9)
    for got, ref in zip(NL.or_opt_proposals(pts, tour, La | La.T), full):
        assert np.array_equal(got, ref)


# ---- consequences of the rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind,K", [(8, "random", 2), (40, "random", 3), (40, "nearest", 8), (64, "clustered", 3), (120, "nearest", 3)])
def test_consequences_of_the_rule(n, kind, K):
    pts, start, tour, c, log = run(n, kind, K, True)
    assert tour[0] == tour[n] == start[0] and sorted(tour[:-1]) == list(range(n))
    assert c["two_opt_sweeps"] + c["or_opt_sweeps"] == len(log) < 1000 and c["rounds"] < 16
    assert c["two_opt_moves"] == sum(len(w) for _, kind_, _, w in log if kind_ == "2opt")
    assert c["or_opt_moves"] == sum(len(w) for _, kind_, _, w in log if kind_ == "oropt")
    stages = [st for st, _, _, _ in log]
    assert stages == sorted(stages, key=("nbr", "full").index) and c["full_sweeps"] == stages.count("full")
    assert c["full_rounds"] >= 1
    # every move shortens its tour by more than 1e-6, so no tour is longer than its start
    assert all(w[0] < -1e-6 for _, _, _, ws in log for w in ws)
    moves = c["two_opt_moves"] + c["or_opt_moves"]
    assert E.tour_length(pts, start) - E.tour_length(pts, tour) > 1e-6 * moves - 1e-12 * n
    # closed below both caps: the full 2-opt sweep and the full Or-opt sweep propose nothing on the end tour
    assert len(E.proposals(pts, tour)[1]) == 0 and len(M.or_opt_proposals(pts, tour)[1]) == 0
    # without closing: the neighbour stage of the same search, never a longer tour than the start
    o_tour, o_c = run(n, kind, K, False)[2:4]
    assert o_c["full_sweeps"] == 0 and o_c["full_rounds"] == 0
    assert E.tour_length(pts, o_tour) <= E.tour_length(pts, start)
    assert np.array_equal(o_tour, tour) == (c["full_sweeps"] == 0)
    nbr_log = [e for e in log if e[0] == "nbr"]
    assert o_c["two_opt_sweeps"] + o_c["or_opt_sweeps"] == len(nbr_log)


def or_only_instance():
    """Ten cities on a circle in the order of their numbers, city 5 lifted out of its place to the end of the tour, and lists
    that name nobody near the place it belongs to: the neighbour stage stops, and a full Or-opt sweep still moves city 5 home."""
    angle = 2.0 * np.pi * np.arange(10) / 10.0
    pts = np.stack([np.cos(angle), np.sin(angle)], axis=1)
    tour = np.array([0, 1, 2, 3, 4, 6, 7, 8, 9, 5, 0], dtype=np.int64)
    lists = np.full((10, 1), -1, dtype=np.int32)
    lists[0, 0] = 1                                               # one listed pair, already adjacent in the tour
    return pts, tour, lists


def test_the_closing_stage_is_not_vacuous():
    pts, tour, lists = or_only_instance()
    open_t, open_c = NL.search_tour(pts, tour, lists, False)
    assert np.array_equal(open_t, tour) and open_c["full_rounds"] == 0 and open_c["or_opt_moves"] == 0
    assert len(M.or_opt_proposals(pts, open_t)[1]) > 0           # a full Or-opt sweep still improves it
    closed_t, closed_c = NL.search_tour(pts, tour, lists, True)
    assert closed_c["full_rounds"] >= 1 and closed_c["full_sweeps"] >= 1
    assert E.tour_length(pts, closed_t) < E.tour_length(pts, tour) - 1e-6
    want_t, want_c = M.search_tour(pts, tour)
    assert np.array_equal(closed_t, want_t)                      # nothing moved before the full stage: it is the full search


def test_caps_count_both_stages():
    pts, start, tour, c, log = run(120, "nearest", 3, True)
    total = len(log)
    nbr = sum(1 for e in log if e[0] == "nbr")
    assert 1 <= nbr < total
    lists = NL.knn_lists(pts, 3)
    for cap in (0, 1, nbr, total - 1):
        t, cc = NL.search_tour(pts, start, lists, True, cap, 16, 4)
        assert cc["two_opt_sweeps"] + cc["or_opt_sweeps"] == cap and cc["full_sweeps"] == max(0, cap - nbr)
        assert np.array_equal(t, log[cap][2]) if cap < total else True
    # max_rounds counts the rounds of both stages: a tour whose last allowed round moved an Or-opt segment does not go on
    for max_rounds in (1, 2):
        t, cc = NL.search_tour(pts, start, lists, True, 1000, max_rounds, 4)
        assert cc["rounds"] <= max_rounds
        want_t, want_c = NL.search_tour(pts, start, lists, False, 1000, max_rounds, 4)
        if cc["full_rounds"] == 0:
            assert np.array_equal(t, want_t)


# ---- the workspace function and the refusals ----------------------------------------------------------------------------------------
def ws_bytes(ns, ts, K, closing):
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    n, t = np.array(ns, dtype=np.int32), np.array(ts, dtype=np.int32)
    assert L.difusco_tsp_nbr_local_search_ragged_workspace_bytes(len(ns), n.ctypes.data, t.ctypes.data, K, closing,
                                                                 ctypes.byref(nbytes)) == 0
    return nbytes.value


def test_exported_symbols_and_workspace():
    L = _lib.lib()
    assert hasattr(L, "difusco_tsp_nbr_local_search_ragged") and hasattr(L, "difusco_tsp_nbr_local_search_ragged_workspace_bytes")
    assert L.difusco_abi_version() == 13
    # at least the selection's tables and the rows of every tour: 6 levels of 34 keys (12 B), 33 rows of pos / key / value / column
    assert ws_bytes([33], [3], 8, 1) > 3 * (6 * 34 * 12 + 33 * (4 + 8 + 8 + 4))
    assert ws_bytes([4], [1], 1, 0) > 0
    sizes = [ws_bytes([n], [3], 8, 1) for n in (4, 5, 33, 64, 65, 1025, 5000)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert ws_bytes([33], [1], 8, 1) < ws_bytes([33], [2], 8, 1)
    # a group's share of a call is what it needs alone, up to the 256-byte rounding of each of the 16 arrays and the fixed tables
    alone = ws_bytes([33], [3], 8, 1) + ws_bytes([257], [2], 8, 1)
    assert abs(ws_bytes([33, 257], [3, 2], 8, 1) - alone) <= 16 * 256 * 2


def test_c_entries_reject_bad_arguments_without_gpu():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    n_ok, t_ok = np.array([5, 33], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    outs7 = tuple(np.zeros(2, np.int32 if k in (2, 6) else np.int64) for k in range(7))
    err = lambda: L.difusco_last_error().decode()
    size = lambda n=n_ok, t=t_ok, g=2, K=8, closing=1: L.difusco_tsp_nbr_local_search_ragged_workspace_bytes(
        g, n.ctypes.data, t.ctypes.data, K, closing, ctypes.byref(nbytes))
    assert size(g=0) < 0 and "groups" in err()
    assert size(n=np.array([3, 33], dtype=np.int32)) < 0 and "n >= 4" in err()
    assert size(t=np.array([1, 0], dtype=np.int32)) < 0 and "tours" in err()
    assert size(K=0) < 0 and "K = 0" in err()
    assert size(K=-3) < 0 and "K = -3" in err()
    assert size(closing=2) < 0 and "closing = 2" in err()
    assert size(closing=-1) < 0 and "closing" in err()
    assert L.difusco_tsp_nbr_local_search_ragged_workspace_bytes(2, None, t_ok.ctypes.data, 8, 1, ctypes.byref(nbytes)) < 0
    assert L.difusco_tsp_nbr_local_search_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, 8, 1, None) < 0
    assert "bytes" in err()
    assert size() == 0

    def call(points=p, tours=p, nbr=p, K=8, closing=1, cap=10, max_rounds=16, select_rounds=4, ws=p, ws_bytes=None, outs=outs7):
        o = [None if x is None else x.ctypes.data for x in outs]
        return L.difusco_tsp_nbr_local_search_ragged(2, n_ok.ctypes.data, t_ok.ctypes.data, points, tours, nbr, K, closing, cap,
                                                     max_rounds, select_rounds, ws, nbytes.value if ws_bytes is None else ws_bytes,
                                                     *o, None)
    # every refusal comes before any GPU work: the device pointers are not memory
    assert call(nbr=None) < 0 and "neighbors is null" in err()
    assert call(K=0) < 0 and "K = 0, needs at least 1" in err()
    assert call(closing=3) < 0 and "closing = 3, needs 0 or 1" in err()
    assert call(max_rounds=0) < 0 and "max_rounds = 0, needs at least 1" in err()
    assert call(select_rounds=0) < 0 and "select_rounds = 0, needs at least 1" in err()
    assert call(cap=-1) < 0 and "max_iterations >= 0" in err()
    assert call(points=None) < 0 and call(tours=None) < 0 and call(ws=None) < 0
    for k in range(7):
        assert call(outs=tuple(None if i == k else x for i, x in enumerate(outs7))) < 0 and "seven host output arrays" in err()
    assert call(ws_bytes=nbytes.value - 1) < 0 and "workspace" in err() and "bytes" in err()
    # max_iterations = 0 returns before any GPU work as well: nothing is applied, every tour has started round 1
    assert call(cap=0) == 0
    assert [o.tolist() for o in outs7] == [[0, 0], [0, 0], [1, 1], [0, 0], [0, 0], [0, 0], [0, 0]]


# ---- the Python checks ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pts = np.random.default_rng(0).random((20, 2))
    tour = np.concatenate([np.arange(20), [0]])[None]
    lists = NL.knn_lists(pts, 4)
    calls = [lambda nb=lists, **kw: batched_nbr_local_search_torch(pts, tour, neighbors=nb, **kw),
             lambda nb=lists, **kw: batched_nbr_local_search_grouped(pts[None], tour, neighbors=None if nb is None else nb[None], **kw),
             lambda nb=lists, **kw: batched_nbr_local_search_ragged([pts], [tour], neighbors=None if nb is None else [nb], **kw)]
    for call in calls:
        with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
            call(device="cpu")
        with pytest.raises(ValueError, match="select_rounds"):
            call(select_rounds=0)
        with pytest.raises(ValueError, match="max_rounds"):
            call(max_rounds=0)
        with pytest.raises(ValueError, match="max_iterations"):
            call(max_iterations=-1)
        with pytest.raises(ValueError, match=r"must be \[20, K\]"):
            call(nb=lists[:19])
        with pytest.raises(ValueError, match="must be integers"):
            call(nb=lists.astype(np.float32))
        with pytest.raises(ValueError, match="candidates = 20"):
            call(nb=None, candidates=20)
        with pytest.raises(ValueError, match="candidates = 0"):
            call(nb=None, candidates=0)
    with pytest.raises(ValueError, match="closed tours"):
        batched_nbr_local_search_torch(pts, tour[:, :-1], neighbors=lists)
    with pytest.raises(ValueError, match="one K"):
        batched_nbr_local_search_ragged([pts, pts], [tour, tour], neighbors=[lists, lists[:, :3]])


def test_the_new_name_and_its_combinations():
    assert "nbr2opt+oropt" in LOCAL_SEARCHES and check_local_search("nbr2opt+oropt") == "nbr2opt+oropt"
    with pytest.raises(ValueError, match="not built"):
        check_local_search("nbr2opt+oropt", "screened")
    assert check_tsp_candidates("nbr2opt+oropt", 1) == 1 and check_tsp_candidates("nbr2opt+oropt", 8) == 8
    with pytest.raises(ValueError, match="needs local_search_candidates = K >= 1, not 0"):
        check_tsp_candidates("nbr2opt+oropt", 0)
    with pytest.raises(ValueError, match="neither kicks nor windows"):
        check_tsp_candidates("nbr2opt+oropt", 5, kicks=3)
    with pytest.raises(ValueError, match="neither kicks nor windows"):
        check_tsp_candidates("nbr2opt+oropt", 5, window=64)
    with pytest.raises(ValueError, match="resident"):
        check_tsp_candidates("nbr2opt+oropt", 5, two_opt_mode="resident")
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="local_search_candidates"):
            check_tsp_candidates("nbr2opt+oropt", bad)
    # the multi-move 2-opt + Or-opt search with candidates is still refused: the new search has a name of its own
    with pytest.raises(ValueError, match="needs local_search='multi2opt'"):
        check_tsp_candidates("multi2opt+oropt", 5)
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    pts = np.random.default_rng(0).random((20, 2))
    for kw, text in ((dict(), "K >= 1"), (dict(local_search_candidates=4, local_search_kicks=2), "local_search_kicks"),
                     (dict(local_search_candidates=4, local_search_window=64), "local_search_window"),
                     (dict(local_search_candidates=4, two_opt_mode="resident"), "resident")):
        with pytest.raises(ValueError, match=text):
            solve_tsp(model, pts, 5, local_search="nbr2opt+oropt", **kw)
        with pytest.raises(ValueError, match=text):
            solve_tsp_batch(model, pts[None], 5, local_search="nbr2opt+oropt", **kw)
        with pytest.raises(ValueError, match=text):
            solve_tsp_batch(model, [pts, pts[:10]], 5, local_search="nbr2opt+oropt", **kw)
    with pytest.raises(ValueError, match="local_search_candidates"):
        solve_tsp(model, pts, 5, local_search="multi2opt+oropt", local_search_candidates=4)


def test_evaluate_flags():
    from difusco_amd import evaluate as EV
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    args = EV.parse_args(base + ["--local_search", "nbr2opt+oropt", "--tsp_local_search_candidates", "8"])[0]
    assert (args.local_search, args.tsp_local_search_candidates, args.tsp_local_search_closing) == ("nbr2opt+oropt", 8, "full")
    args = EV.parse_args(base + ["--local_search", "nbr2opt+oropt", "--tsp_local_search_candidates", "1",
                                 "--tsp_local_search_closing", "none"])[0]
    assert (args.tsp_local_search_candidates, args.tsp_local_search_closing) == (1, "none")
    nbr = ["--local_search", "nbr2opt+oropt"]
    for bad in (nbr,                                                                              # needs K >= 1
                nbr + ["--tsp_local_search_candidates", "0"],
                nbr + ["--tsp_local_search_candidates", "-1"],
                nbr + ["--tsp_local_search_candidates", "8", "--tsp_local_search_kicks", "2"],
                nbr + ["--tsp_local_search_candidates", "8", "--tsp_local_search_window", "64"],
                nbr + ["--tsp_local_search_candidates", "8", "--two_opt_mode", "resident"],
                nbr + ["--tsp_local_search_candidates", "8", "--two_opt_method", "screened"],
                ["--local_search", "multi2opt+oropt", "--tsp_local_search_candidates", "8"]):     # still refused
        with pytest.raises(SystemExit):
            EV.parse_args(base + bad)
    with pytest.raises(SystemExit):
        EV.parse_args(["--task", "mis", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."] + nbr +
                      ["--tsp_local_search_candidates", "8"])
    info = {"merge_iterations": 1.0, "two_opt_iterations": 7, "merged_costs": [4.0], "two_opt_moves": 31, "or_opt_iterations": 3,
            "or_opt_moves": 9, "local_search_rounds": 2, "local_search_candidates": 8, "local_search_closing": True,
            "local_search_full_sweeps": 1, "local_search_full_rounds": 1}
    ex = types.SimpleNamespace(source=["f", 0], points=np.zeros((4, 2)), tour=[0, 1, 2, 3, 0])
    rec = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    assert list(rec)[-2:] == ["local_search_full_sweeps", "local_search_full_rounds"]             # appended after every other field
    assert (rec["local_search_full_sweeps"], rec["local_search_full_rounds"], rec["or_opt_moves"]) == (1, 1, 9)
    del info["local_search_full_sweeps"], info["local_search_full_rounds"]
    rec = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    assert "local_search_full_sweeps" not in rec and "local_search_full_rounds" not in rec
