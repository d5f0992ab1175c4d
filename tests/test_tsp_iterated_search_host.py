"""The iterated multi-move local search on the host: the numpy restatement of the rule (tests/tsp_iterated_search_emulation.py) on
hand cases with injected draws, its own invariants, the fixed-order length against an independent restatement, and the argument
checks of the Python layers, the runner and the library (which come before any GPU work), so that the GPU tests compare against
a reference that is itself held to the rule."""
import ctypes
import types

import numpy as np
import pytest
import torch

import multi_local_search_emulation as E
import tsp_iterated_search_emulation as T
from difusco_amd import _lib
from difusco_amd.decode import (TSP_KICK_SIZE, TSP_KICK_SPAN, batched_iterated_search_grouped, batched_iterated_search_ragged,
                                batched_iterated_search_torch, check_tsp_kicks)


def instance(n, s):
    rng = np.random.default_rng(100 * n + s)
    return rng.random((n, 2)), np.concatenate([[0], rng.permutation(n - 1) + 1, [0]])


def length_restated(points, tour):
    """``tour_length`` once more, with python floats and explicit loops: partial sum r takes d_r, d_r+1024, .. in rising k, then
    the halving tree."""
    P = np.asarray(points, dtype=np.float64)[np.asarray(tour)]
    n = len(tour) - 1
    part = [0.0] * 1024
    for k in range(n):
        dx, dy = float(P[k, 0]) - float(P[k + 1, 0]), float(P[k, 1]) - float(P[k + 1, 1])
        part[k % 1024] = part[k % 1024] + float(np.sqrt(np.float64(dx * dx + dy * dy)))
    h = 512
    while h >= 1:
        for r in range(h):
            part[r] = part[r] + part[r + h]
        h //= 2
    return part[0]


def is_closed_permutation(tour, n, first):
    t = np.asarray(tour)
    return len(t) == n + 1 and t[0] == t[-1] == first and sorted(t[:-1].tolist()) == list(range(n))


def test_kicks_zero_is_search_tour():
    for n, cap, rounds in ((8, 1000, 16), (33, 2, 16), (64, 1000, 1), (17, 0, 16)):
        pts, start = instance(n, 0)
        want, wc = E.search_tour(pts, start, cap, rounds, 4)
        got, c, per = T.search_tour(pts, start, 5, 9, kicks=0, max_iterations=cap, max_rounds=rounds)
        assert np.array_equal(got, want) and c == wc
        assert per["kicks_kept"] == per["kicks_improved"] == per["segments_swapped"] == 0
        assert per["first_length"] == per["final_length"] == T.tour_length(pts, want)


def test_hand_cases_with_injected_draws():
    I = np.array(list(range(12)) + [0])
    # draws (a, l1, l2): [2, 6) is kept, [4, 7) overlaps it and is dropped although it comes with the longer range, [8, 11) is kept
    C, kept = T.apply_kick(I, [(2, 1, 3), (4, 2, 1), (8, 2, 1)])
    assert kept == [True, False, True]
    assert C.tolist() == [0, 1, 3, 4, 5, 2, 6, 7, 10, 8, 9, 11, 0]
    # the lower c wins whatever the order of the ranges in the tour
    C, kept = T.apply_kick(I, [(4, 2, 1), (2, 1, 3)])
    assert kept == [True, False] and C.tolist() == [0, 1, 2, 3, 6, 4, 5, 7, 8, 9, 10, 11, 0]
    # adjacent ranges [2, 5) and [5, 8): both kept
    C, kept = T.apply_kick(I, [(2, 1, 2), (5, 2, 1)])
    assert kept == [True, True] and C.tolist() == [0, 1, 3, 4, 2, 7, 5, 6, 8, 9, 10, 11, 0]
    # a = 1 and b = n at the boundaries: positions 0 and n stay
    C, kept = T.apply_kick(I, [(1, 2, 2), (9, 1, 2)])
    assert kept == [True, True] and C.tolist() == [0, 3, 4, 1, 2, 5, 6, 7, 8, 10, 11, 9, 0]
    # a draw dropped by a dropped draw's range only is kept: the filter looks at kept draws
    C, kept = T.apply_kick(I, [(2, 1, 1), (3, 1, 3), (5, 1, 1)])
    assert kept == [True, False, True]


def test_n_four_has_one_segment_length():
    # Lc = min(span, 3 // 2) = 1: l1 = l2 = 1, a = 1 + w0 % 2, so [1, 3) or [2, 4)
    seen = set()
    for t in range(16):
        for a, l1, l2 in T.kick_draws(3, 100, t, 4, 5, 30):
            assert (l1, l2) == (1, 1) and a in (1, 2)
            seen.add(a)
    assert seen == {1, 2}
    C, kept = T.apply_kick([0, 1, 2, 3, 0], [(2, 1, 1), (1, 1, 1)])
    assert kept == [True, False] and C.tolist() == [0, 1, 3, 2, 0]


def test_the_draws_follow_the_stated_arithmetic():
    from philox_reference import philox4x32_10
    n, span = 65, 16
    d = T.kick_draws(2 ** 63 + 5, 2 ** 64 - 2, 3, n, 6, span)    # the offset wraps: kick 3 draws at offset 1
    for c, (a, l1, l2) in enumerate(d):
        w = [int(x) for x in philox4x32_10(2 ** 63 + 5, 1, c)]
        assert (l1, l2) == (1 + w[1] % 16, 1 + w[2] % 16) and a == 1 + w[0] % (n - l1 - l2)
        assert 1 <= a and a + l1 + l2 <= n
    assert all(max(l1, l2) <= 3 for _, l1, l2 in T.kick_draws(1, 0, 0, 8, 64, 100))      # span >= n: Lc = (n - 1) // 2


@pytest.mark.parametrize("n", [4, 5, 8, 17, 64])
def test_permutation_and_closed_tour_after_every_kick(n):
    pts, start = instance(n, 1)
    trace = []
    out, c, per = T.search_tour(pts, start, 7, 3, kicks=12, kick_size=4, span=16, trace=trace)
    assert len(trace) == 12
    for K, C, lc, take in trace:
        assert is_closed_permutation(K, n, start[0]) and is_closed_permutation(C, n, start[0])
        assert lc == T.tour_length(pts, C)
    assert is_closed_permutation(out, n, start[0])
    assert per["final_length"] <= per["first_length"]
    assert per["final_length"] == length_restated(pts, out) == T.tour_length(pts, out)
    assert per["first_length"] == length_restated(pts, E.search_tour(pts, start)[0])
    assert 0 <= per["kicks_improved"] <= per["kicks_kept"] <= 12 and 0 <= per["segments_swapped"] <= 12 * 4
    assert per["kicks_improved"] == sum(1 for i, (_, _, lc, take) in enumerate(trace)
                                        if take and lc < min([per["first_length"]] + [x[2] for x in trace[:i] if x[3]]))


def test_fixed_order_length_of_a_long_tour():
    """More than one term per partial sum (n > 1024), and the sum is not numpy's."""
    rng = np.random.default_rng(3)
    pts = rng.random((2500, 2))
    tour = np.concatenate([[0], rng.permutation(2499) + 1, [0]])
    assert T.tour_length(pts, tour) == length_restated(pts, tour)
    assert abs(T.tour_length(pts, tour) - E.M.tour_length(pts, tour)) < 1e-9


@pytest.mark.parametrize("cap", [1, 3])
def test_a_capped_descent_never_returns_a_longer_tour(cap):
    for n in (17, 64):
        pts, start = instance(n, 2)
        base, _ = E.search_tour(pts, start, cap, 16, 4)
        out, c, per = T.search_tour(pts, start, 1, 0, kicks=10, kick_size=4, span=16, max_iterations=cap)
        assert per["first_length"] == T.tour_length(pts, base)
        assert T.tour_length(pts, out) <= T.tour_length(pts, base)
        assert c["two_opt_sweeps"] + c["or_opt_sweeps"] <= cap * 11


def test_same_seed_same_result_other_seed_other_kicks():
    pts, start = instance(64, 0)
    kw = dict(kicks=6, kick_size=4, span=16)
    a = T.search_tour(pts, start, 11, 1 << 62, **kw)
    b = T.search_tour(pts, start, 11, 1 << 62, **kw)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert T.kick_draws(11, 1 << 62, 0, 64, 4, 16) != T.kick_draws(12, 1 << 62, 0, 64, 4, 16)
    assert T.kick_draws(11, 1 << 62, 0, 64, 4, 16) != T.kick_draws(11, (1 << 62) + 1, 0, 64, 4, 16)
    assert T.kick_draws(11, 1 << 62, 1, 64, 4, 16) == T.kick_draws(11, (1 << 62) + 1, 0, 64, 4, 16)
    # a group is its tours, one by one
    tours, c, per = T.iterated_search(pts, np.stack([start, start]), [11, 12], [1 << 62, 1 << 62], **kw)
    other = T.search_tour(pts, start, 12, 1 << 62, **kw)
    assert np.array_equal(tours[0], a[0]) and np.array_equal(tours[1], other[0])
    assert per["final_length"] == [a[2]["final_length"], other[2]["final_length"]]
    assert c["two_opt_moves"] == a[1]["two_opt_moves"] + other[1]["two_opt_moves"]
    assert c["rounds"] == max(a[1]["rounds"], other[1]["rounds"])


@pytest.mark.parametrize("n", [64, 65])
def test_random_start_instances_end_strictly_shorter(n):
    pts, start = instance(n, 0)
    out, c, per = T.search_tour(pts, start, 0, 0, kicks=40, kick_size=4, span=16)
    assert per["kicks_improved"] >= 1 and per["final_length"] < per["first_length"]
    assert per["first_length"] == T.tour_length(pts, E.search_tour(pts, start)[0])


def test_check_tsp_kicks():
    assert check_tsp_kicks("2opt", 0) == (0, TSP_KICK_SIZE, TSP_KICK_SPAN)
    assert check_tsp_kicks("multi2opt+oropt", 3, 64, 1) == (3, 64, 1)
    for ls in ("2opt", "2opt+oropt", "multi2opt"):
        with pytest.raises(ValueError, match=r"multi2opt\+oropt"):
            check_tsp_kicks(ls, 1)
    for bad in (dict(kicks=-1), dict(kicks=1.5), dict(kicks=1, kick_size=0), dict(kicks=1, kick_size=65), dict(kicks=1, span=0)):
        with pytest.raises(ValueError, match="local_search_kick"):
            check_tsp_kicks("multi2opt+oropt", **bad)


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
            call(device="cpu", kicks=1)
        for bad, word in ((dict(kicks=-1), "kicks"), (dict(kicks=1, kick_size=0), "kick_size"), (dict(kicks=1, kick_size=65), "kick_size"),
                          (dict(kicks=1, span=0), "span"), (dict(select_rounds=0), "select_rounds"), (dict(max_rounds=0), "max_rounds"),
                          (dict(max_iterations=-1), "max_iterations")):
            with pytest.raises(ValueError, match=word):
                call(**bad)
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    for ls in ("2opt", "multi2opt"):
        with pytest.raises(ValueError, match="local_search_kicks"):
            solve_tsp(model, pts, 5, local_search=ls, local_search_kicks=2)
        with pytest.raises(ValueError, match="local_search_kicks"):
            solve_tsp_batch(model, pts[None], 5, local_search=ls, local_search_kicks=2)
        with pytest.raises(ValueError, match="local_search_kicks"):
            solve_tsp_batch(model, [pts, pts[:10]], 5, local_search=ls, local_search_kicks=2)
    with pytest.raises(ValueError, match="kick_size"):
        solve_tsp(model, pts, 5, local_search="multi2opt+oropt", local_search_kicks=2, local_search_kick_size=65)


def test_evaluate_flags():
    from difusco_amd import evaluate as EV
    assert (EV.TSP_KICK_SIZE, EV.TSP_KICK_SPAN) == (TSP_KICK_SIZE, TSP_KICK_SPAN)
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    args = EV.parse_args(base)[0]
    assert (args.tsp_local_search_kicks, args.tsp_local_search_kick_size, args.tsp_local_search_kick_span) == (0, TSP_KICK_SIZE, TSP_KICK_SPAN)
    args = EV.parse_args(base + ["--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "5", "--tsp_local_search_kick_size", "2",
                                 "--tsp_local_search_kick_span", "7"])[0]
    assert (args.tsp_local_search_kicks, args.tsp_local_search_kick_size, args.tsp_local_search_kick_span) == (5, 2, 7)
    for bad in (["--tsp_local_search_kicks", "5"], ["--local_search", "multi2opt", "--tsp_local_search_kicks", "5"],
                ["--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "-1"],
                ["--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "1", "--tsp_local_search_kick_size", "65"],
                ["--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "1", "--tsp_local_search_kick_span", "0"]):
        with pytest.raises(SystemExit):
            EV.parse_args(base + bad)
    with pytest.raises(SystemExit):
        EV.parse_args(["--task", "mis", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", ".", "--local_search", "multi2opt+oropt",
                       "--tsp_local_search_kicks", "1"])
    info = {"merge_iterations": 1.0, "two_opt_iterations": 7, "merged_costs": [4.0], "two_opt_moves": 31, "or_opt_iterations": 3,
            "or_opt_moves": 9, "local_search_rounds": 2, "local_search_kicks_improved": [2, 0]}
    ex = types.SimpleNamespace(source=["f", 0], points=np.zeros((4, 2)), tour=[0, 1, 2, 3, 0])
    assert EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))["kicks_improved"] == [2, 0]


def test_library_argument_checks_come_before_any_gpu_work():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    n_ok, t_ok = np.array([5, 33], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    assert L.difusco_tsp_iterated_search_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, None) < 0
    assert L.difusco_tsp_iterated_search_ragged_workspace_bytes(0, n_ok.ctypes.data, t_ok.ctypes.data, ctypes.byref(nbytes)) < 0
    small = np.array([5, 3], dtype=np.int32)
    assert L.difusco_tsp_iterated_search_ragged_workspace_bytes(2, small.ctypes.data, t_ok.ctypes.data, ctypes.byref(nbytes)) < 0
    assert L.difusco_tsp_iterated_search_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, ctypes.byref(nbytes)) == 0
    plain = ctypes.c_size_t()
    assert L.difusco_tsp_multi_local_search_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, ctypes.byref(plain)) == 0
    assert nbytes.value >= plain.value + 4 * (6 + 3 * 34)         # the incumbents on top of the descent's workspace
    o = [np.zeros(4, np.int64) for _ in range(10)]
    #     G  group_n            group_tours        points tours cap rounds S kicks size span seeds offsets ws bytes
    ok = [2, n_ok.ctypes.data, t_ok.ctypes.data, p, p, 100, 16, 4, 3, 4, 16, p, p, p, 1 << 30] + [x.ctypes.data for x in o] + [None]
    for i in (1, 2, 3, 4, 11, 12, 13) + tuple(range(15, 25)):
        bad = list(ok)
        bad[i] = None
        assert L.difusco_tsp_iterated_search_ragged(*bad) == -1, i
    for i, v, word in ((0, 0, b"groups"), (5, -1, b"max_iterations"), (6, 0, b"max_rounds"), (7, 0, b"select_rounds"),
                       (8, -1, b"kicks"), (9, 0, b"kick_size"), (9, 65, b"kick_size"), (10, 0, b"span"),
                       (14, nbytes.value - 1, b"workspace")):
        bad = list(ok)
        bad[i] = v
        assert L.difusco_tsp_iterated_search_ragged(*bad) == -1 and word in L.difusco_last_error(), i
    assert L.difusco_tsp_search_host_syncs() == 0
