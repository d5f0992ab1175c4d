"""The iterated search with focused descents on the host: the invariants of the numpy restatement of the rule
(tests/tsp_focused_search_emulation.py), its one-against-all selection against ``select_ranges``, and the argument checks of the
library (which come before any GPU work), the Python layers and the runner, so that the GPU tests compare against a reference
that is itself held to the rule."""
import ctypes
import types

import numpy as np
import pytest
import torch

import multi_local_search_emulation as E
import tsp_focused_search_emulation as F
import tsp_iterated_search_emulation as T
from difusco_amd import _lib
from difusco_amd.decode import (batched_iterated_search_grouped, batched_iterated_search_ragged, batched_iterated_search_torch,
                                check_tsp_descent)


def instance(n, s):
    rng = np.random.default_rng(100 * n + s)
    return rng.random((n, 2)), np.concatenate([[0], rng.permutation(n - 1) + 1, [0]])


def is_closed_permutation(tour, n, first):
    t = np.asarray(tour)
    return len(t) == n + 1 and t[0] == t[-1] == first and sorted(t[:-1].tolist()) == list(range(n))


@pytest.mark.parametrize("n", [8, 33, 200])
def test_emulation_properties(n):
    pts, start = instance(n, 1)
    kw = dict(kicks=8, kick_size=4, span=16)
    log = []
    out, c, per = F.search_tour(pts, start, 7, 3, log=log, **kw)
    assert is_closed_permutation(out, n, start[0])
    assert per["final_length"] <= per["first_length"] == T.tour_length(pts, E.search_tour(pts, start)[0])
    assert per["final_length"] == T.tour_length(pts, out)
    again, moved = E.search_tour(pts, out)                       # no cap binds: no improving move is left
    assert np.array_equal(again, out) and moved["two_opt_sweeps"] == moved["or_opt_sweeps"] == 0
    assert 0 <= per["kicks_improved"] <= per["kicks_kept"] <= 8 and per["closing_sweeps"] >= 0
    assert len(log) >= 2 * 8 and all(w <= m for _, m, w in log) and all((w > 0) == (m > 0) for _, m, w in log)
    # kicks = 0 is the multi-move search, tours and counters
    want, wc = E.search_tour(pts, start)
    got, gc, gp = F.search_tour(pts, start, 7, 3, kicks=0)
    assert np.array_equal(got, want) and gc == wc and gp["closing_sweeps"] == gp["kicks_kept"] == 0
    # the same seed gives the same answer, another seed another kick
    b = F.search_tour(pts, start, 7, 3, **kw)
    assert np.array_equal(b[0], out) and b[1:] == (c, per)
    assert T.kick_draws(7, 3, 0, n, 4, 16) != T.kick_draws(8, 3, 0, n, 4, 16)
    # the counters sum all descents, the closing one included
    assert c["two_opt_sweeps"] + c["or_opt_sweeps"] >= sum(1 for _, m, _ in log if m > 0) + per["closing_sweeps"]


def test_focused_sweeps_evaluate_fewer_pairs_and_miss_nothing_here():
    n = 200
    pts, start = instance(n, 2)
    count, log = [0], []
    out, c, per = F.search_tour(pts, start, 1, 0, kicks=10, kick_size=16, span=30, log=log, count=count)
    assert count[0] < 0.6 * len(log) * n * n / 2                 # well below all pairs of every sweep
    assert per["closing_sweeps"] == 0 or per["final_length"] <= per["first_length"]


def test_marks_after_a_kick_and_active_positions():
    K = np.array([0, 1, 3, 4, 5, 2, 6, 7, 8, 9, 10, 11, 0])     # [2, 6) swapped with l1 = 1, l2 = 3
    Tm = F.kick_marks(K, [(2, 1, 3), (8, 1, 1)], [True, False])
    assert np.flatnonzero(Tm).tolist() == [1, 2, 3, 5, 6]        # positions 1, 2, 4, 5, 5, 6 of the kicked tour
    act = F.active_positions(K, Tm)
    assert np.flatnonzero(act).tolist() == [1, 4, 5]             # the three new edges 1-3, 5-2, 2-6
    assert np.flatnonzero(F.row_active(act)).tolist() == [0, 1, 2, 3, 4, 5]


def _random_proposals(rng, n, m, ties):
    row = np.sort(rng.choice(n - 1, size=m, replace=False))
    length = rng.integers(1, max(2, n // 3), size=m)
    a = np.minimum(row, rng.integers(0, n - 1, size=m))
    b = np.minimum(a + length, n)
    value = -rng.random(m) - 1e-3
    if ties:                                                     # equal values in different rows: the row decides
        value = np.round(value * 3) / 3 - 1e-3
    return value, row, a, b


@pytest.mark.parametrize("ties", [False, True])
def test_compact_selection_equals_select_ranges(ties):
    rng = np.random.default_rng(5 + ties)
    for n, m in ((12, 5), (40, 20), (200, 90), (300, 299)):
        for rounds in (1, 2, 4, 64):
            value, row, a, b = _random_proposals(rng, n, m, ties)
            assert F.select_compact(value, row, a, b, rounds) == E.select_ranges(value, row, a, b, rounds)
    # adjacent ranges do not meet, nested ranges do; equal values: the lower row wins
    value, row = np.array([-1.0, -1.0, -1.0, -2.0]), np.array([0, 4, 8, 9])
    a, b = np.array([0, 4, 2, 5]), np.array([4, 8, 3, 6])
    for rounds in (1, 4):
        got = F.select_compact(value, row, a, b, rounds)
        assert got == E.select_ranges(value, row, a, b, rounds)
    assert F.select_compact(value, row, a, b, 1) == [3, 0]       # row 9 beats row 4 (nested), row 0 beats row 8 (nested, tie)
    assert F.select_compact(value, row, a, b, 4) == [3, 0]       # rows 4 and 8 met a winner and were dropped


def test_library_surface_and_argument_checks_before_any_gpu_work():
    L = _lib.lib()
    assert L.difusco_abi_version() == 13
    assert hasattr(L, "difusco_tsp_focused_search_ragged") and hasattr(L, "difusco_tsp_focused_search_ragged_workspace_bytes")
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    n_ok, t_ok = np.array([5, 33], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    size = L.difusco_tsp_focused_search_ragged_workspace_bytes
    assert size(2, n_ok.ctypes.data, t_ok.ctypes.data, None) < 0
    assert size(0, n_ok.ctypes.data, t_ok.ctypes.data, ctypes.byref(nbytes)) < 0
    small = np.array([5, 3], dtype=np.int32)
    assert size(2, small.ctypes.data, t_ok.ctypes.data, ctypes.byref(nbytes)) < 0
    assert size(2, n_ok.ctypes.data, t_ok.ctypes.data, ctypes.byref(nbytes)) == 0
    iterated = ctypes.c_size_t()
    assert L.difusco_tsp_iterated_search_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, ctypes.byref(iterated)) == 0
    assert nbytes.value >= iterated.value + 4 * 4 * (5 + 3 * 33)  # S, T and the two lists on top of the iterated search's
    more_n, more_t = ctypes.c_size_t(), ctypes.c_size_t()        # the workspace grows with n and with T
    assert size(2, np.array([5, 34], dtype=np.int32).ctypes.data, t_ok.ctypes.data, ctypes.byref(more_n)) == 0
    assert size(2, n_ok.ctypes.data, np.array([1, 4], dtype=np.int32).ctypes.data, ctypes.byref(more_t)) == 0
    assert more_n.value > nbytes.value and more_t.value > nbytes.value
    o = [np.zeros(4, np.int64) for _ in range(11)]
    #     G  group_n            group_tours        points tours cap rounds S kicks size span seeds offsets cmax ws bytes
    ok = [2, n_ok.ctypes.data, t_ok.ctypes.data, p, p, 100, 16, 4, 3, 4, 16, p, p, 1024, p, 1 << 30] + [x.ctypes.data for x in o] + [None]
    for i in (1, 2, 3, 4, 11, 12, 14) + tuple(range(16, 27)):
        bad = list(ok)
        bad[i] = None
        assert L.difusco_tsp_focused_search_ragged(*bad) == -1, i
    for i, v, word in ((0, 0, b"groups"), (5, -1, b"max_iterations"), (6, 0, b"max_rounds"), (7, 0, b"select_rounds"),
                       (8, -1, b"kicks"), (9, 0, b"kick_size"), (9, 65, b"kick_size"), (10, 0, b"span"),
                       (13, -1, b"compact_select_max"), (13, 1025, b"compact_select_max"), (15, nbytes.value - 1, b"workspace")):
        bad = list(ok)
        bad[i] = v
        assert L.difusco_tsp_focused_search_ragged(*bad) == -1 and word in L.difusco_last_error(), i
    assert L.difusco_tsp_search_host_syncs() == 0                # the refused call is the thread's last one: no synchronisation


def test_check_tsp_descent():
    assert check_tsp_descent("full") == "full" and check_tsp_descent("focused") == "focused"
    assert check_tsp_descent("full", 0) == "full" and check_tsp_descent("focused", 3) == "focused"
    with pytest.raises(ValueError, match="local_search_descent"):
        check_tsp_descent("narrow")
    with pytest.raises(ValueError, match="local_search_kicks > 0"):
        check_tsp_descent("focused", 0)


def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pts = np.random.default_rng(0).random((20, 2))
    tour = np.concatenate([np.arange(20), [0]])[None]
    calls = [lambda **kw: batched_iterated_search_torch(pts, tour, **kw),
             lambda **kw: batched_iterated_search_grouped(pts[None], tour, **kw),
             lambda **kw: batched_iterated_search_ragged([pts], [tour], **kw)]
    for call in calls:
        with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
            call(device="cpu", kicks=1, descent="focused")
        for bad, word in ((dict(descent="narrow"), "descent"), (dict(descent=None), "descent"),
                          (dict(descent="focused", compact_select_max=-1), "compact_select_max"),
                          (dict(descent="focused", compact_select_max=1025), "compact_select_max"),
                          (dict(descent="focused", compact_select_max=1.5), "compact_select_max"),
                          (dict(descent="focused", kicks=-1), "kicks"), (dict(descent="focused", kicks=1, kick_size=65), "kick_size")):
            with pytest.raises(ValueError, match=word):
                call(**bad)
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    ls = dict(local_search="multi2opt+oropt", local_search_descent="focused")
    for kicks in (dict(), dict(local_search_kicks=0)):
        with pytest.raises(ValueError, match="local_search_kicks > 0"):
            solve_tsp(model, pts, 5, **ls, **kicks)
        with pytest.raises(ValueError, match="local_search_kicks > 0"):
            solve_tsp_batch(model, pts[None], 5, **ls, **kicks)
        with pytest.raises(ValueError, match="local_search_kicks > 0"):
            solve_tsp_batch(model, [pts, pts[:10]], 5, **ls, **kicks)
    with pytest.raises(ValueError, match="local_search_descent"):
        solve_tsp(model, pts, 5, local_search="multi2opt+oropt", local_search_kicks=2, local_search_descent="narrow")
    with pytest.raises(ValueError, match="local_search_kicks"):  # the kicks' own check still comes first
        solve_tsp(model, pts, 5, local_search="2opt", local_search_kicks=2, local_search_descent="focused")


def test_evaluate_flag(monkeypatch):
    from difusco_amd import evaluate as EV
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    assert EV.parse_args(base)[0].tsp_local_search_descent == "full"
    kicked = ["--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "5"]
    assert EV.parse_args(base + kicked + ["--tsp_local_search_descent", "focused"])[0].tsp_local_search_descent == "focused"
    assert EV.parse_args(base + kicked + ["--tsp_local_search_descent", "full"])[0].tsp_local_search_descent == "full"
    assert EV.parse_args(base + ["--tsp_local_search_descent", "full"])[0].tsp_local_search_kicks == 0
    import argparse
    said = []
    real = argparse.ArgumentParser.error

    def error(self, message):
        said.append(message)
        real(self, message)
    monkeypatch.setattr(argparse.ArgumentParser, "error", error)
    for bad in (["--tsp_local_search_descent", "focused"],
                ["--local_search", "multi2opt+oropt", "--tsp_local_search_descent", "focused"],
                ["--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "0", "--tsp_local_search_descent", "focused"]):
        with pytest.raises(SystemExit):
            EV.parse_args(base + bad)
        assert "--tsp_local_search_kicks N > 0" in said[-1]
    with pytest.raises(SystemExit):
        EV.parse_args(base + kicked + ["--tsp_local_search_descent", "narrow"])
    info = {"merge_iterations": 1.0, "two_opt_iterations": 7, "merged_costs": [4.0], "two_opt_moves": 31, "or_opt_iterations": 3,
            "or_opt_moves": 9, "local_search_rounds": 2, "local_search_kicks_improved": [2, 0], "local_search_closing_sweeps": [0, 1]}
    ex = types.SimpleNamespace(source=["f", 0], points=np.zeros((4, 2)), tour=[0, 1, 2, 3, 0])
    rec = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    assert rec["closing_sweeps"] == [0, 1] and rec["kicks_improved"] == [2, 0]
    del info["local_search_closing_sweeps"]
    assert "closing_sweeps" not in EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
