"""The windowed iterated search on the host: the numpy restatement of the rule (tests/tsp_window_search_emulation.py) - its cut
lists, its equality with the iterated emulation where one window holds the tour, its invariants - and the argument checks of
the library (which come before any GPU work), of the Python layers and of the runner."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import multi_local_search_emulation as E
import multi_two_opt_emulation as M
import tsp_iterated_search_emulation as T
import tsp_window_search_emulation as W
from difusco_amd import _lib
from difusco_amd.decode import (batched_window_search_grouped, batched_window_search_ragged, batched_window_search_torch,
                                check_tsp_window)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "difusco_hip.h")


def is_closed_permutation(tour, n, first):
    t = np.asarray(tour)
    return len(t) == n + 1 and t[0] == t[-1] == first and sorted(t[:-1].tolist()) == list(range(n))


def test_symbols_are_declared_and_exported_and_the_abi_stays():
    text = open(HEADER).read()
    L = _lib.lib()
    for name in ("difusco_tsp_window_search_ragged", "difusco_tsp_window_search_ragged_workspace_bytes"):
        assert f"int {name}(" in text
        assert hasattr(L, name)
    assert _lib.ABI_VERSION == 13 and L.difusco_abi_version() == 13 and "#define DIFUSCO_ABI_VERSION 13" in text


def test_cut_lists():
    assert W.cuts(197, 64, 0) == W.cuts(197, 64, 2) == [0, 64, 128, 192, 197]     # windows of 64, 64, 64, 5: the last is skipped
    assert W.cuts(197, 64, 1) == W.cuts(197, 64, 3) == [0, 32, 96, 160, 197]      # 32, 64, 64, 37
    assert W.cuts(100, 128, 0) == [0, 100] and W.cuts(100, 128, 1) == [0, 64, 100]
    assert W.cuts(128, 64, 0) == [0, 64, 128] and W.cuts(64, 64, 0) == [0, 64]    # a cut on n is n itself
    pts, start = M.instance(197, 0)
    out, _, _, per = W.search_tour(pts, start, 1, 2, window=64, passes=2, kicks=0)
    assert per["windows_searched"] == 3 + 4


def test_one_window_over_the_tour_is_the_iterated_search():
    pts, start = M.instance(100, 3)
    kw = dict(kicks=5, kick_size=4, span=16)
    got, first, closing, per = W.search_tour(pts, start, 11, 1 << 62, window=128, passes=1, **kw)
    want, c, p = T.search_tour(pts, start, 11, 1 << 62, **kw)
    assert np.array_equal(got, want) and first == E.search_tour(pts, start)[1]
    assert all(per[k] == p[k] for k in p)
    assert per["passes_kept"] == 1 and per["windows_searched"] == 1 and per["closing_sweeps"] == 0
    assert closing["two_opt_moves"] == closing["or_opt_moves"] == 0


def test_the_iterated_emulation_takes_an_open_path():
    """Positions 0 and m of a path stay, whatever its last city, and the kicks draw with n := m."""
    pts, start = M.instance(40, 1)
    path = start[5:30]                                            # 25 positions, m = 24, first and last city differ
    trace = []
    out, c, per = T.search_tour(pts, path, 3, 9, kicks=6, kick_size=4, span=16, trace=trace)
    assert out[0] == path[0] and out[-1] == path[-1] and sorted(out.tolist()) == sorted(path.tolist())
    for K, C, lc, take in trace:
        assert K[0] == C[0] == path[0] and K[-1] == C[-1] == path[-1]
    assert per["final_length"] <= per["first_length"] == T.tour_length(pts, E.search_tour(pts, path)[0])
    assert all(1 <= a and a + l1 + l2 <= 24 for a, l1, l2 in T.kick_draws(3, 9, 0, 24, 8, 16))


@pytest.mark.parametrize("name", ["uniform", "clustered", "lattice"])
def test_closed_permutation_never_longer_than_the_first_descent(name):
    n = 197
    pts, start = {"uniform": lambda: M.instance(n, 2), "clustered": lambda: E.clustered_instance(n, 2),
                  "lattice": lambda: W.lattice_instance(n, 2)}[name]()
    trace = []
    out, first, closing, per = W.search_tour(pts, start, 7, 1 << 62, window=64, passes=3, kicks=3, kick_size=2, span=5, trace=trace)
    assert is_closed_permutation(out, n, start[0])
    assert per["first_length"] == T.tour_length(pts, E.search_tour(pts, start)[0])
    assert per["final_length"] == T.tour_length(pts, out) <= per["first_length"]
    assert len(trace) == 3 and per["passes_kept"] == sum(t[2] for t in trace)
    for cand, lc, take in trace:
        assert is_closed_permutation(cand, n, start[0]) and lc == T.tour_length(pts, cand)
    assert 0 <= per["kicks_improved"] <= per["kicks_kept"] <= 3 * per["windows_searched"]
    # another offset of the odd passes moves other cities: the cities on the cuts of a pass stay where they are in that pass
    prev = E.search_tour(pts, start)[0]
    for r, (cand, lc, take) in enumerate(trace):
        for c in W.cuts(n, 64, r):
            assert cand[c] == prev[c]
        prev = cand if take else prev


def test_a_group_is_its_tours():
    pts, a = M.instance(64, 0)
    b = M.instance(64, 1)[1]
    kw = dict(window=32, passes=2, kicks=2, kick_size=2, span=5)
    tours, c, per = W.window_search(pts, np.stack([a, b]), [5, 6], [0, 1 << 32], **kw)
    x, y = W.search_tour(pts, a, 5, 0, **kw), W.search_tour(pts, b, 6, 1 << 32, **kw)
    assert np.array_equal(tours[0], x[0]) and np.array_equal(tours[1], y[0])
    assert per["final_length"] == [x[3]["final_length"], y[3]["final_length"]]
    assert c["two_opt_moves"] == sum(t[k]["two_opt_moves"] for t in (x, y) for k in (1, 2))
    assert c["two_opt_sweeps"] == max(x[1]["two_opt_sweeps"], y[1]["two_opt_sweeps"]) + max(x[2]["two_opt_sweeps"], y[2]["two_opt_sweeps"])


def test_check_tsp_window():
    assert check_tsp_window("2opt", 0) == (0, 1)
    assert check_tsp_window("multi2opt+oropt", 64, 3, 0) == (64, 3)
    assert check_tsp_window("multi2opt+oropt", 1024, 1, 1024) == (1024, 1)
    for bad in (dict(window=15), dict(window=1025), dict(window=-1), dict(window=64.5), dict(window=64, passes=0),
                dict(window=0, passes=2), dict(window=64, kicks=1025), dict(window=64, descent="focused"),
                dict(window=64, kick_bias="heat")):
        with pytest.raises(ValueError, match="local_search_"):
            check_tsp_window("multi2opt+oropt", **bad)
    for ls in ("2opt", "2opt+oropt", "multi2opt"):
        with pytest.raises(ValueError, match=r"multi2opt\+oropt"):
            check_tsp_window(ls, 64)


def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pts = np.random.default_rng(0).random((20, 2))
    tour = np.concatenate([np.arange(20), [0]])[None]
    calls = [lambda **kw: batched_window_search_torch(pts, tour, **kw),
             lambda **kw: batched_window_search_grouped(pts[None], tour, **kw),
             lambda **kw: batched_window_search_ragged([pts], [tour], **kw)]
    for call in calls:
        with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
            call(device="cpu", window=16)
        with pytest.raises(TypeError):
            call(kicks=1)                                         # window has no default
        for bad, word in ((dict(window=15), "window"), (dict(window=1025), "window"), (dict(window=16, passes=0), "passes"),
                          (dict(window=16, kicks=-1), "kicks"), (dict(window=16, kicks=1025), "kicks"),
                          (dict(window=16, kicks=1, kick_size=0), "kick_size"), (dict(window=16, kicks=1, kick_size=65), "kick_size"),
                          (dict(window=16, kicks=1, span=0), "span"), (dict(window=16, select_rounds=0), "select_rounds"),
                          (dict(window=16, max_rounds=0), "max_rounds"), (dict(window=16, max_iterations=-1), "max_iterations"),
                          (dict(window=16, passes=2 ** 30, kicks=2), "Philox"), (dict(window=16, seeds=[1, 2]), "seeds")):
            with pytest.raises(ValueError, match=word):
                call(**bad)
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    ok = dict(local_search="multi2opt+oropt", local_search_window=64)
    for bad, word in ((dict(ok, local_search="multi2opt"), "local_search_window"), (dict(ok, local_search="2opt"), "local_search_window"),
                      (dict(ok, local_search_window=8), "local_search_window"), (dict(ok, local_search_passes=0), "local_search_passes"),
                      (dict(local_search="multi2opt+oropt", local_search_passes=2), "local_search_passes"),
                      (dict(ok, local_search_kicks=2, local_search_descent="focused"), "local_search_descent"),
                      (dict(ok, local_search_kicks=2, local_search_kick_bias="heat"), "local_search_kick_bias"),
                      (dict(ok, local_search_kicks=2000), "local_search_kicks")):
        with pytest.raises(ValueError, match=word):
            solve_tsp(model, pts, 5, **bad)
        with pytest.raises(ValueError, match=word):
            solve_tsp_batch(model, pts[None], 5, **bad)
        with pytest.raises(ValueError, match=word):
            solve_tsp_batch(model, [pts, pts[:10]], 5, **bad)


def test_evaluate_flags():
    from difusco_amd import evaluate as EV
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    args = EV.parse_args(base)[0]
    assert (args.tsp_local_search_window, args.tsp_local_search_passes) == (0, 1)
    multi = ["--local_search", "multi2opt+oropt"]
    args = EV.parse_args(base + multi + ["--tsp_local_search_window", "256", "--tsp_local_search_passes", "4"])[0]
    assert (args.tsp_local_search_window, args.tsp_local_search_passes, args.tsp_local_search_kicks) == (256, 4, 0)
    win = ["--tsp_local_search_window", "64"]
    for bad in (win, ["--local_search", "multi2opt"] + win, multi + ["--tsp_local_search_window", "15"],
                multi + ["--tsp_local_search_window", "1025"], multi + win + ["--tsp_local_search_passes", "0"],
                multi + ["--tsp_local_search_passes", "2"], multi + win + ["--tsp_local_search_kicks", "1025"],
                multi + win + ["--tsp_local_search_kicks", "2", "--tsp_local_search_descent", "focused"],
                multi + win + ["--tsp_local_search_kicks", "2", "--tsp_local_search_kick_bias", "heat"]):
        with pytest.raises(SystemExit):
            EV.parse_args(base + bad)
    with pytest.raises(SystemExit):
        EV.parse_args(["--task", "mis", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."] + multi + win)
    info = {"merge_iterations": 1.0, "two_opt_iterations": 7, "merged_costs": [4.0], "two_opt_moves": 31, "or_opt_iterations": 3,
            "or_opt_moves": 9, "local_search_rounds": 2, "local_search_kicks_improved": [2, 0], "local_search_window": 64,
            "local_search_passes": 2, "local_search_passes_kept": [2, 1], "local_search_closing_sweeps": [0, 3]}
    ex = types.SimpleNamespace(source=["f", 0], points=np.zeros((4, 2)), tour=[0, 1, 2, 3, 0])
    rec = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    assert rec["passes_kept"] == [2, 1] and rec["closing_sweeps"] == [0, 3] and rec["kicks_improved"] == [2, 0]


def test_library_argument_checks_come_before_any_gpu_work():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    n_ok, t_ok = np.array([5, 333], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    size = L.difusco_tsp_window_search_ragged_workspace_bytes
    assert size(2, n_ok.ctypes.data, t_ok.ctypes.data, 64, None) < 0
    assert size(0, n_ok.ctypes.data, t_ok.ctypes.data, 64, ctypes.byref(nbytes)) < 0 and b"groups" in L.difusco_last_error()
    assert size(2, None, t_ok.ctypes.data, 64, ctypes.byref(nbytes)) < 0
    small = np.array([5, 3], dtype=np.int32)
    assert size(2, small.ctypes.data, t_ok.ctypes.data, 64, ctypes.byref(nbytes)) < 0
    for w in (15, 1025, 0, -64):
        assert size(2, n_ok.ctypes.data, t_ok.ctypes.data, w, ctypes.byref(nbytes)) < 0 and b"window" in L.difusco_last_error()
    assert size(2, n_ok.ctypes.data, t_ok.ctypes.data, 64, ctypes.byref(nbytes)) == 0
    plain = ctypes.c_size_t()
    assert L.difusco_tsp_multi_local_search_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, ctypes.byref(plain)) == 0
    # a candidate per tour and a table entry per window of either parity (7 and 7 windows per tour of 333, 1 and 1 of 5)
    assert nbytes.value >= plain.value + 4 * (6 + 3 * 334) + 16 * 2 * (1 + 3 * 7)
    o = [np.zeros(4, np.int64) for _ in range(15)]
    #     G  group_n            group_tours        points tours cap rounds S kicks size span seeds offsets W  R  ws bytes
    ok = [2, n_ok.ctypes.data, t_ok.ctypes.data, p, p, 100, 16, 4, 3, 4, 16, p, p, 64, 2, p, 1 << 30] + [x.ctypes.data for x in o] + [None]
    entry = L.difusco_tsp_window_search_ragged
    for i in (1, 2, 3, 4, 11, 12, 15) + tuple(range(17, 32)):
        bad = list(ok)
        bad[i] = None
        assert entry(*bad) == -1, i
    for i, v, word in ((0, 0, b"groups"), (5, -1, b"max_iterations"), (6, 0, b"max_rounds"), (7, 0, b"select_rounds"),
                       (8, -1, b"kicks"), (8, 1025, b"kicks"), (9, 0, b"kick_size"), (9, 65, b"kick_size"), (10, 0, b"span"),
                       (13, 15, b"window"), (13, 1025, b"window"), (14, 0, b"passes"), (14, 2 ** 30, b"Philox"),
                       (16, nbytes.value - 1, b"workspace")):
        bad = list(ok)
        bad[i] = v
        assert entry(*bad) == -1 and word in L.difusco_last_error(), i
    assert b"tsp_window_search_ragged" in L.difusco_last_error()
