"""The multi-move 2-opt without a GPU: the numpy restatement of the rule (tests/multi_two_opt_emulation.py) against the rule's
consequences, the reference's single move, an independent sequential greedy and one pinned result, and the argument checks of
every new entry.

Instances: uniform points from ``np.random.default_rng(1000 n + s)`` with a random-permutation start
(``multi_two_opt_emulation.instance``) or a nearest-neighbour start."""
import ctypes
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import multi_two_opt_emulation as E
from difusco_amd import _lib
from difusco_amd.decode import (LOCAL_SEARCHES, batched_multi_two_opt_grouped, batched_multi_two_opt_ragged,
                                batched_multi_two_opt_torch, check_local_search)
from oracle.tsp_decode_oracle import batched_two_opt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_two_opt_n64.json")
SIZES = [4, 5, 8, 33, 200]


def start_tour(n, kind):
    pts, tour = E.instance(n, 1)
    return pts, (tour if kind == "random" else E.nearest_neighbour_tour(pts))


@functools.lru_cache(maxsize=None)
def run(n, kind, S, cap=1000):
    """One search of the emulation, computed once per test session: (points, start, tour, sweeps, moves, log)."""
    pts, start = start_tour(n, kind)
    log = []
    tours, sweeps, moves = E.multi_two_opt(pts, start[None], cap, S, log=log)
    return pts, start, tours[0], sweeps, moves, log


def brute_changes(pts, tour):
    """Every change of one tour the way the oracle forms them: full distance matrices, +inf outside j >= i + 2."""
    n = len(tour) - 1
    p, p1 = pts[tour[:-1]], pts[tour[1:]]
    dmat = lambda a, b: np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    d = np.sqrt(((p - p1) ** 2).sum(-1))
    change = dmat(p, p) + dmat(p1, p1) - d[:, None] - d[None, :]
    return np.where(np.triu(np.ones((n, n), dtype=bool), k=2), change, np.inf)


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("kind", ["random", "nearest"])
@pytest.mark.parametrize("n", SIZES)
def test_consequences_of_the_rule(n, kind, S):
    pts, start, tour, sweeps, moves, log = run(n, kind, S)
    assert len(tour) == n + 1 and tour[0] == tour[n] == start[0] and sorted(tour[:-1]) == list(range(n))
    assert sweeps == len(log) < 1000 and moves == sum(len(w) for _, _, w, _ in log)
    for k, (_, before, winners, m) in enumerate(log):
        after = log[k + 1][1] if k + 1 < len(log) else tour
        assert 1 <= len(winners) <= m
        assert E.tour_length(pts, before) - E.tour_length(pts, after) > 1e-6 * len(winners)
        # the first winner is the exact 2-opt's pair: lowest change, lowest flat index
        c = brute_changes(pts, before)
        flat = int(c.reshape(-1).argmin())
        assert winners[0] == (c.reshape(-1)[flat], flat // n, flat % n)
        spans = sorted((i, j + 1) for _, i, j in winners)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))             # disjoint ranges
        assert all(ch < -1e-6 and 0 <= i and i + 2 <= j <= n - 1 for ch, i, j in winners)
    assert not (brute_changes(pts, tour) < -1e-6).any()           # stopped below the cap: no improving move is left
    assert moves > 0 or n <= 5


def test_a_sweep_with_one_proposal_is_one_step_of_the_reference_rule():
    seen = 0
    for n in (8, 33, 200):
        for kind in ("random", "nearest"):
            pts, _, tour, _, _, log = run(n, kind, 4)
            for k, (_, before, winners, m) in enumerate(log):
                if m == 1:
                    after = log[k + 1][1] if k + 1 < len(log) else tour
                    ref, its = batched_two_opt(pts, before[None], 1)
                    assert its == 1 and np.array_equal(ref[0], after)
                    seen += 1
    assert seen >= 3


def sequential_greedy(pts, tour):
    """A second implementation of a sweep with unbounded rounds: the proposals in key order, each taken unless it shares a
    position with one taken before.  Plain Python on the brute-force changes."""
    n = len(tour) - 1
    c = brute_changes(pts, tour)
    props = []
    for i in range(n - 2):
        j = min(range(i + 2, n), key=lambda jj: (c[i, jj], jj))
        if c[i, j] < -1e-6:
            props.append((c[i, j], i, j))
    taken = np.zeros(n, dtype=bool)
    t = tour.copy()
    count = 0
    for _, i, j in sorted(props):
        if not taken[i:j + 1].any():
            taken[i:j + 1] = True
            t[i + 1:j + 1] = t[i + 1:j + 1][::-1].copy()
            count += 1
    return t, count


@pytest.mark.parametrize("n,kind", [(8, "random"), (33, "random"), (200, "random"), (200, "nearest")])
def test_unbounded_rounds_are_the_sequential_greedy(n, kind):
    pts, start = start_tour(n, kind)
    want, sweeps, moves = E.multi_two_opt(pts, start[None], 1000, 10 ** 6)
    t, s, m = start.copy(), 0, 0
    while True:
        t, count = sequential_greedy(pts, t)
        if count == 0:
            break
        s, m = s + 1, m + count
    assert (s, m) == (sweeps, moves) and np.array_equal(t, want[0])


def test_more_rounds_select_more_per_sweep():
    one, four = run(200, "random", 1), run(200, "random", 4)
    # winners of the first sweep: on a random start the ranges are long and overlap, one round finds few that are disjoint
    assert len(four[5][0][2]) > len(one[5][0][2]) >= 1
    assert four[3] < one[3]                                       # and fewer sweeps to the end


def test_caps_and_groups():
    pts, start = E.instance(33, 1)
    other = E.instance(33, 2)[1]
    full = run(33, "random", 4)
    assert full[3] > 3
    zero = E.multi_two_opt(pts, start[None], 0, 4)
    assert np.array_equal(zero[0][0], start) and zero[1:] == (0, 0)
    log = []
    capped = E.multi_two_opt(pts, start[None], 3, 4, log=log)
    assert capped[1] == 3 and np.array_equal(capped[0][0], full[5][3][1])      # the tour before the fourth sweep
    # a tour's result does not depend on the tours next to it; the group counts the sweeps of its slowest tour
    solo = E.multi_two_opt(pts, other[None], 1000, 4)
    both = E.multi_two_opt(pts, np.stack([start, other]), 1000, 4)
    assert np.array_equal(both[0][0], full[2]) and np.array_equal(both[0][1], solo[0][0])
    assert both[1] == max(full[3], solo[1]) and both[2] == full[4] + solo[2]


def test_pinned_case():
    with open(GOLDEN) as f:
        pin = json.load(f)
    assert (pin["n"], pin["select_rounds"]) == (64, 4)
    pts, start = E.instance(64, pin["seed"])
    tours, sweeps, moves = E.multi_two_opt(pts, start[None], 1000, 4)
    assert (sweeps, moves) == (pin["sweeps"], pin["moves"]) and tours[0].tolist() == pin["tour"]


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pts = np.random.default_rng(0).random((20, 2))
    tour = np.concatenate([np.arange(20), [0]])[None]
    calls = [lambda **kw: batched_multi_two_opt_torch(pts, tour, **kw),
             lambda **kw: batched_multi_two_opt_grouped(pts[None], tour, **kw),
             lambda **kw: batched_multi_two_opt_ragged([pts], [tour], **kw)]
    for call in calls:
        with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
            call(device="cpu")
        with pytest.raises(ValueError, match="select_rounds"):
            call(select_rounds=0)
        with pytest.raises(ValueError, match="select_rounds"):
            call(select_rounds=1.5)
        with pytest.raises(ValueError, match="max_iterations"):
            call(max_iterations=-1)
    with pytest.raises(ValueError, match="closed tours"):
        batched_multi_two_opt_torch(pts, tour[:, :-1])
    with pytest.raises(ValueError, match="n >= 4"):
        batched_multi_two_opt_torch(pts[:3], tour[:, :4])
    with pytest.raises(ValueError, match=r"\[groups, N, 2\]"):
        batched_multi_two_opt_grouped(pts, tour)
    with pytest.raises(ValueError, match="tour arrays"):
        batched_multi_two_opt_ragged([pts, pts], [tour])
    assert "multi2opt" in LOCAL_SEARCHES and check_local_search("multi2opt") == "multi2opt"
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    for bad, kw in (("multi3opt", {}), ("multi2opt", dict(two_opt_method="screened"))):
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp(model, pts, 5, local_search=bad, **kw)
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp_batch(model, pts[None], 5, local_search=bad, **kw)
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp_batch(model, [pts, pts[:10]], 5, local_search=bad, **kw)


def test_evaluate_flag():
    from difusco_amd import evaluate as EV
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    assert EV.parse_args(base + ["--local_search", "multi2opt"])[0].local_search == "multi2opt"
    with pytest.raises(SystemExit):
        EV.parse_args(base + ["--local_search", "multi2opt", "--two_opt_method", "screened"])
    info = {"merge_iterations": 1.0, "two_opt_iterations": 7, "merged_costs": [4.0], "two_opt_moves": 31}
    ex = types.SimpleNamespace(source=["f", 0], points=np.zeros((4, 2)), tour=[0, 1, 2, 3, 0])
    rec = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    assert rec["2opt_iterations"] == 7 and rec["two_opt_moves"] == 31 and list(rec)[-1] == "two_opt_moves"


def test_c_entries_reject_bad_arguments_without_gpu():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    n_ok, t_ok = np.array([5, 33], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    sweeps, moves = np.zeros(2, np.int64), np.zeros(2, np.int64)
    size = lambda n, t, g=2: L.difusco_tsp_multi_two_opt_ragged_workspace_bytes(g, n.ctypes.data, t.ctypes.data, ctypes.byref(nbytes))
    # floor(log2(n + 1)) + 1 levels of n + 1 keys per tour: 3 levels of 6, 6 levels of 34 three times
    assert size(n_ok, t_ok) == 0 and nbytes.value > (3 * 6 + 3 * 6 * 34) * 12
    assert size(n_ok, t_ok, 0) < 0
    assert size(np.array([3, 33], dtype=np.int32), t_ok) < 0
    assert size(np.array([5, 65535 * 16 + 1], dtype=np.int32), t_ok) < 0
    assert size(n_ok, np.array([1, 0], dtype=np.int32)) < 0
    assert size(n_ok, np.array([1, 65535], dtype=np.int32)) < 0
    assert L.difusco_tsp_multi_two_opt_ragged_workspace_bytes(2, None, t_ok.ctypes.data, ctypes.byref(nbytes)) < 0
    assert L.difusco_tsp_multi_two_opt_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, None) < 0
    assert size(n_ok, t_ok) == 0

    def call(points=p, tours=p, cap=10, select_rounds=4, ws=p, ws_bytes=None, outs=(sweeps, moves)):
        o = [None if x is None else x.ctypes.data for x in outs]
        return L.difusco_tsp_multi_two_opt_ragged(2, n_ok.ctypes.data, t_ok.ctypes.data, points, tours, cap, select_rounds, ws,
                                                  nbytes.value if ws_bytes is None else ws_bytes, o[0], o[1], None)
    assert call(select_rounds=0) < 0 and "select_rounds" in L.difusco_last_error().decode()
    assert call(cap=-1) < 0
    assert call(points=None) < 0 and call(tours=None) < 0 and call(ws=None) < 0
    assert call(outs=(sweeps, None)) < 0 and call(outs=(None, moves)) < 0
    assert call(ws_bytes=nbytes.value - 1) < 0 and "workspace" in L.difusco_last_error().decode()
    assert L.difusco_abi_version() == 13
