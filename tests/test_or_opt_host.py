"""The 2-opt + Or-opt local search without a GPU: the numpy restatement of the rule (tests/or_opt_emulation.py) against its own
invariants and pinned results, and the argument checks of every new entry.

Instances: ``or_opt_emulation.instance(n, s)`` - uniform points and a random permutation start from
``np.random.default_rng(1000 n + s)``.  All pins use one tour per instance."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import or_opt_emulation as E
from difusco_amd import _lib
from difusco_amd.decode import batched_local_search_grouped, batched_local_search_ragged, batched_local_search_torch
from oracle.tsp_decode_oracle import batched_two_opt

# n, s, max_iterations, max_rounds -> two_opt_iterations, or_opt_iterations, rounds, final length
PINS = [
    (5, 0, 1000, 16, 1, 0, 1, 2.087564336819),
    (8, 1, 1000, 16, 4, 1, 2, 3.596360638823),
    (33, 2, 1000, 16, 24, 2, 2, 4.638877985998),
    (64, 3, 1000, 16, 55, 13, 2, 6.440686172330),
    (64, 3, 5, 16, 25, 25, 6, 6.425443614713),
    (64, 3, 1000, 1, 55, 13, 1, 6.440686172330),
    (200, 1, 1000, 16, 210, 24, 2, 10.968398414057),
]
TWO_OPT_ONLY = {(64, 3): 7.173680645214, (200, 1): 11.841275287303}


@functools.lru_cache(maxsize=None)
def run(n, s, cap=1000, max_rounds=16):
    """One local search of the emulation, computed once per test session: (points, start, tours, a, b, rounds, moves, phases)."""
    pts, start = E.instance(n, s)
    moves, phases = [], []
    tours, two, orr, rounds = E.local_search(pts, start[None], cap, max_rounds, moves=moves, phases=phases)
    return pts, start, tours, two, orr, rounds, moves, phases


@functools.lru_cache(maxsize=None)
def two_opt_only(n, s):
    pts, start = E.instance(n, s)
    return batched_two_opt(pts, start[None], 1000)


@pytest.mark.parametrize("n,s,cap,max_rounds,two,orr,rounds,length", PINS)
def test_pins(n, s, cap, max_rounds, two, orr, rounds, length):
    pts, _, tours, a, b, r, _, _ = run(n, s, cap, max_rounds)
    assert (a, b, r) == (two, orr, rounds)
    assert E.tour_length(pts, tours[0]) == pytest.approx(length, abs=5e-12)


@pytest.mark.parametrize("n,s", sorted(TWO_OPT_ONLY))
def test_first_phase_is_the_oracles_two_opt_and_the_result_is_never_longer(n, s):
    pts, start, tours, _, _, _, _, phases = run(n, s)
    ref, its = two_opt_only(n, s)
    assert phases[0][0] == its
    assert E.tour_length(pts, ref[0]) == pytest.approx(TWO_OPT_ONLY[(n, s)], abs=5e-12)
    assert E.tour_length(pts, tours[0]) <= E.tour_length(pts, ref[0])
    # with max_iterations = 0 the Or-opt phase has no iteration: the oracle's 2-opt (one move), tour for tour
    only, a, b, r = E.local_search(pts, start[None], 0, 1)
    one, it1 = batched_two_opt(pts, start[None], 0)
    assert np.array_equal(only, one) and (a, b, r) == (it1, 0, 1)


@pytest.mark.parametrize("n,s", [(5, 0), (8, 1), (33, 2), (64, 3), (200, 1)])
def test_every_move_keeps_a_closed_permutation_and_changes_the_length_by_its_delta(n, s):
    pts, start = E.instance(n, s)
    tour = batched_two_opt(pts, start[None], 1000)[0][0]
    applied = 0
    while True:
        best = E.best_or_opt_move(pts, tour)
        if best is None or not best[0] < E.THRESHOLD:
            break
        delta, v, i, j = best
        L = E.VARIANTS[v][0]
        assert 0 <= i <= n - 1 - L and 0 <= j <= n - 1 and not i <= j <= i + L
        new = E.apply_or_opt_move(tour, v, i, j)
        assert len(new) == n + 1 and new[0] == new[n] == tour[0] and sorted(new[:-1]) == list(range(n))
        assert E.tour_length(pts, new) - E.tour_length(pts, tour) == pytest.approx(delta, abs=1e-9)
        tour, applied = new, applied + 1
        assert applied <= 1000
    assert applied > 0 or n == 5


def test_moves_cover_every_variant_in_both_directions():
    seen = set()
    for s in (0, 1):
        for _, _, v, i, j in run(200, s)[6]:
            seen.add((v, j < i))
    assert seen == {(v, left) for v in range(5) for left in (False, True)}


def test_a_capped_run_applies_two_opt_moves_after_the_first_round():
    phases = run(64, 3, 5, 16)[7]
    assert len(phases) == 6 and any(a > 0 for a, _ in phases[1:])
    assert all(a <= 5 and b <= 5 for a, b in phases)


def test_ties_go_to_the_lowest_flat_index():
    # a 2 x 4 grid walked in order is symmetric enough for exact ties; argmin over the flattened [5, n, n] array is the rule
    pts = np.array([[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [2, 1], [1, 1], [0, 1]], dtype=np.float64)
    tour = np.array([0, 4, 1, 5, 2, 6, 3, 7, 0])
    d = E.or_opt_deltas(pts, tour)
    delta, v, i, j = E.best_or_opt_move(pts, tour)
    flat = (v * 8 + i) * 8 + j
    assert d.reshape(-1)[flat] == delta == d.min() and not (d.reshape(-1)[:flat] <= delta).any()
    assert (d == delta).sum() > 1                                  # there is a tie to break


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pts = np.random.default_rng(0).random((20, 2))
    tour = np.concatenate([np.arange(20), [0]])[None]
    calls = [lambda **kw: batched_local_search_torch(pts, tour, **kw),
             lambda **kw: batched_local_search_grouped(pts[None], tour, **kw),
             lambda **kw: batched_local_search_ragged([pts], [tour], **kw)]
    for call in calls:
        with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
            call(device="cpu")
        with pytest.raises(ValueError, match="max_rounds"):
            call(max_rounds=0)
        with pytest.raises(ValueError, match="max_iterations"):
            call(max_iterations=-1)
    with pytest.raises(ValueError, match="closed tours"):
        batched_local_search_torch(pts, tour[:, :-1])
    with pytest.raises(ValueError, match="n >= 4"):
        batched_local_search_torch(pts[:3], tour[:, :4])
    with pytest.raises(ValueError, match=r"\[groups, N, 2\]"):
        batched_local_search_grouped(pts, tour)
    with pytest.raises(ValueError, match="groups \\* P"):
        batched_local_search_grouped(np.stack([pts, pts]), tour)
    with pytest.raises(ValueError, match="tour arrays"):
        batched_local_search_ragged([pts, pts], [tour])
    with pytest.raises(ValueError, match="at least one"):
        batched_local_search_ragged([], [])
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    for bad, kw in (("3opt", {}), ("2opt+oropt", dict(two_opt_method="screened"))):
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp(model, pts, 5, local_search=bad, **kw)
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp_batch(model, pts[None], 5, local_search=bad, **kw)
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp_batch(model, [pts, pts[:10]], 5, local_search=bad, **kw)


def test_evaluate_flag():
    from difusco_amd import evaluate as EV
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    assert EV.parse_args(base)[0].local_search == "2opt"
    assert EV.parse_args(base + ["--local_search", "2opt+oropt"])[0].local_search == "2opt+oropt"
    for bad in (["--local_search", "oropt"], ["--local_search", "2opt+oropt", "--two_opt_method", "screened"]):
        with pytest.raises(SystemExit):
            EV.parse_args(base + bad)


def test_c_entries_reject_bad_arguments_without_gpu():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    n_ok, t_ok = np.array([5, 33], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    two, orr, rounds = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2, np.int32)
    size = lambda n, t, g=2: L.difusco_tsp_local_search_ragged_workspace_bytes(g, n.ctypes.data, t.ctypes.data, ctypes.byref(nbytes))
    assert size(n_ok, t_ok) == 0 and nbytes.value > (6 + 3 * 34) * (16 + 4)      # tp and the staging copy of every tour
    assert size(n_ok, t_ok, 0) < 0
    assert size(np.array([3, 33], dtype=np.int32), t_ok) < 0
    assert size(np.array([5, 65535 * 16 + 1], dtype=np.int32), t_ok) < 0
    assert size(n_ok, np.array([1, 0], dtype=np.int32)) < 0
    assert size(n_ok, np.array([1, 65535], dtype=np.int32)) < 0
    assert L.difusco_tsp_local_search_ragged_workspace_bytes(2, None, t_ok.ctypes.data, ctypes.byref(nbytes)) < 0
    assert L.difusco_tsp_local_search_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, None) < 0
    assert size(n_ok, t_ok) == 0

    def call(points=p, tours=p, cap=10, max_rounds=16, ws=p, ws_bytes=None, outs=(two, orr, rounds)):
        o = [None if x is None else x.ctypes.data for x in outs]
        return L.difusco_tsp_local_search_ragged(2, n_ok.ctypes.data, t_ok.ctypes.data, points, tours, cap, max_rounds, ws,
                                                 nbytes.value if ws_bytes is None else ws_bytes, o[0], o[1], o[2], None)
    assert call(max_rounds=0) < 0 and "max_rounds" in L.difusco_last_error().decode()
    assert call(cap=-1) < 0
    assert call(points=None) < 0 and call(tours=None) < 0 and call(ws=None) < 0
    assert call(outs=(two, None, rounds)) < 0 and call(outs=(two, orr, None)) < 0 and call(outs=(None, orr, rounds)) < 0
    assert call(ws_bytes=nbytes.value - 1) < 0 and "workspace" in L.difusco_last_error().decode()
    assert L.difusco_abi_version() == 13
