"""The multi-move local search without a GPU: the numpy restatement of the rule (tests/multi_local_search_emulation.py) against
the rule's consequences, the multi-move 2-opt, the single Or-opt move of ``or_opt_emulation``, an independent sequential greedy
and pinned cases, and the argument checks of every new entry.

Instances: uniform points with a random-permutation start (``multi_two_opt_emulation.instance``) or a nearest-neighbour start,
points in five tight clusters (``clustered_instance``) and the k x k integer grid (``lattice_instance``)."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import multi_local_search_emulation as E
import multi_two_opt_emulation as M
import or_opt_emulation as O
from difusco_amd import _lib
from difusco_amd.decode import (LOCAL_SEARCHES, batched_multi_local_search_grouped, batched_multi_local_search_ragged,
                                batched_multi_local_search_torch, check_local_search)
from oracle.tsp_decode_oracle import batched_two_opt

SIZES = [4, 5, 8, 16, 17, 33, 64]
CAP, ROUNDS = 1000, 16


@functools.lru_cache(maxsize=None)
def run(n, kind, S, cap=CAP, rounds=ROUNDS):
    """One search of the emulation, computed once per test session: (points, start, tour, counters, log, phases).  kind: a seed
    of ``instance``, "nearest", "clustered" (seed 10) or "lattice" (n = k k)."""
    if kind == "clustered":
        pts, start = E.clustered_instance(n, 10)
    elif kind == "lattice":
        k = int(round(n ** 0.5))
        pts, start = E.lattice_instance(k, E.LATTICE_SEEDS[k])
    else:
        pts, start = M.instance(n, 1 if kind == "nearest" else kind)
        if kind == "nearest":
            start = M.nearest_neighbour_tour(pts)
    log, phases = [], []
    tour, c = E.search_tour(pts, start, cap, rounds, S, log=log, phases=phases)
    return pts, start, tour, c, log, phases


def check_run(n, r):
    """The consequences of the rule on one run of the emulation."""
    pts, start, tour, c, log, phases = r
    assert len(tour) == n + 1 and tour[0] == tour[n] == start[0] and sorted(tour[:-1]) == list(range(n))
    kinds = [k for k, _, _, _ in log]
    assert (c["two_opt_sweeps"], c["or_opt_sweeps"]) == (kinds.count("2opt"), kinds.count("oropt"))
    assert c["two_opt_moves"] == sum(len(w) for k, _, w, _ in log if k == "2opt")
    assert c["or_opt_moves"] == sum(len(w) for k, _, w, _ in log if k == "oropt")
    assert c["rounds"] == len(phases) and [sum(p) for p in zip(*phases)] == [c["two_opt_sweeps"], c["or_opt_sweeps"]]
    for k, (kind, before, winners, m) in enumerate(log):
        after = log[k + 1][1] if k + 1 < len(log) else tour
        assert 1 <= len(winners) <= m
        deltas = [w[0] for w in winners]
        assert all(d < -1e-6 for d in deltas)
        # the sweep's drop is the sum of its winners' deltas, up to the rounding of two sums of n terms of size <= n sqrt(2)
        drop = O.tour_length(pts, before) - O.tour_length(pts, after)
        scale = max(1.0, float(np.abs(pts).max()))
        assert abs(drop + sum(deltas)) <= 8 * n * n * scale * np.finfo(np.float64).eps
        if kind == "oropt":
            for d, v, i, j in winners:
                L = O.VARIANTS[v][0]
                assert 0 <= i <= n - 1 - L and 0 <= j <= n - 1 and not i <= j <= i + L
            a, b = E.or_opt_range(*(np.array(x) for x in zip(*[(i, v, j) for _, v, i, j in winners])))
            spans = sorted(zip(a.tolist(), b.tolist()))
        else:
            spans = sorted((i, j + 1) for _, i, j in winners)
        assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))                 # disjoint ranges
        changed = np.flatnonzero(before != after)
        assert all(any(a <= p < b for a, b in spans) for p in changed)             # nothing moves outside them


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("kind", [1, "nearest"])
@pytest.mark.parametrize("n", SIZES)
def test_consequences_of_the_rule(n, kind, S):
    r = run(n, kind, S)
    check_run(n, r)
    pts, start, tour, c, log, phases = r
    # stopped below both caps: no improving Or-opt move and no improving 2-opt move is left
    assert c["two_opt_sweeps"] + c["or_opt_sweeps"] < CAP and c["rounds"] < ROUNDS
    best = O.best_or_opt_move(pts, tour)
    assert best is None or best[0] >= -1e-6
    again, its = batched_two_opt(pts, tour[None], 10)
    assert its == 0 and np.array_equal(again[0], tour)
    # and no longer than the multi-move 2-opt leaves the same start
    multi = M.multi_two_opt(pts, start[None], CAP, S)[0][0]
    assert O.tour_length(pts, tour) <= O.tour_length(pts, multi)


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("n,kind", [(16, 0), (33, 1), (64, 1), (64, "nearest")])
def test_the_first_phase_is_the_multi_move_two_opt(n, kind, S):
    pts, start, tour, c, log, phases = run(n, kind, S)
    multi, sweeps, moves = M.multi_two_opt(pts, start[None], CAP, S)
    first = phases[0][0]
    assert first == sweeps and sum(len(w) for k, _, w, _ in log[:first]) == moves
    assert all(k == "2opt" for k, _, _, _ in log[:first])
    assert np.array_equal(log[first][1] if len(log) > first else tour, multi[0])


def test_without_an_or_opt_proposal_the_search_is_the_multi_move_two_opt():
    pts, start, tour, c, log, phases = run(16, 0, 4)
    assert phases == [(8, 0)]                                     # the first Or-opt phase proposes nothing
    multi, sweeps, moves = M.multi_two_opt(pts, start[None], CAP, 4)
    assert np.array_equal(tour, multi[0])
    assert c == {"two_opt_sweeps": sweeps, "or_opt_sweeps": 0, "rounds": 1, "two_opt_moves": moves, "or_opt_moves": 0}


def test_row_deltas_are_the_deltas_of_the_exact_search():
    for n in (4, 5, 6, 7, 33):
        pts, tour = M.instance(n, 2)
        full = O.or_opt_deltas(pts, tour)                         # [5, n, n]
        assert np.array_equal(E.or_opt_row_deltas(pts, tour, 0, n - 1), full[:, :n - 1].transpose(1, 0, 2))
        assert np.isinf(full[:, n - 1]).all()                     # row n - 1 has no candidate
        lo, hi = 1, min(3, n - 1)
        assert np.array_equal(E.or_opt_row_deltas(pts, tour, lo, hi), full[:, lo:hi].transpose(1, 0, 2))


def test_an_or_opt_sweep_with_one_proposal_is_one_step_of_the_exact_rule():
    seen = 0
    for n, kind in [(8, 1), (17, 1), (33, 1), (64, 1), (64, "nearest"), (64, "clustered"), (36, "lattice")]:
        pts, _, tour, _, log, _ = run(n, kind, 4)
        for k, (name, before, winners, m) in enumerate(log):
            if name == "oropt" and m == 1:
                after = log[k + 1][1] if k + 1 < len(log) else tour
                best = O.best_or_opt_move(pts, before)
                assert winners == [best]
                assert np.array_equal(O.apply_or_opt_move(before, *best[1:]), after)
                seen += 1
    assert seen >= 3


def or_opt_sequential_greedy(pts, tour):
    """A second implementation of an Or-opt sweep with unbounded rounds: the row proposals in key order, each taken unless it
    shares a position of its range with one taken before.  Plain Python on ``or_opt_deltas``."""
    n = len(tour) - 1
    d = O.or_opt_deltas(pts, tour)
    props = []
    for i in range(n - 1):
        delta, v, j = min((d[v, i, j], v, j) for v in range(5) for j in range(n))
        if delta < -1e-6:
            L = O.VARIANTS[v][0]
            props.append((delta, i, v, j, min(i, j), (j if j > i + L else i + L) + 1))
    taken = np.zeros(n + 1, dtype=bool)
    t = tour.copy()
    count = 0
    for delta, i, v, j, a, b in sorted(props):
        if not taken[a:b].any():
            taken[a:b] = True
            new = O.apply_or_opt_move(tour, v, i, j)
            t[a:b] = new[a:b]
            count += 1
    return t, count


@pytest.mark.parametrize("n,kind", [(17, 1), (33, 1), (64, 1), (64, "nearest"), (64, "clustered"), (64, "lattice")])
def test_unbounded_rounds_are_the_sequential_greedy(n, kind):
    pts, start, tour, c, log, phases = run(n, kind, 10 ** 6)
    seen = 0
    for k, (name, before, winners, m) in enumerate(log):
        if name == "oropt":
            after = log[k + 1][1] if k + 1 < len(log) else tour
            t, count = or_opt_sequential_greedy(pts, before)
            assert count == len(winners) and np.array_equal(t, after)
            seen += 1
    assert seen >= 1
    check_run(n, (pts, start, tour, c, log, phases))


def test_caps():
    pts, start, full_tour, full, log, phases = run(64, 1, 4)
    assert phases == [(24, 2), (0, 0)]
    zero = E.search_tour(pts, start, 0, ROUNDS, 4)
    assert np.array_equal(zero[0], start)
    assert zero[1] == {"two_opt_sweeps": 0, "or_opt_sweeps": 0, "rounds": 1, "two_opt_moves": 0, "or_opt_moves": 0}
    for cap in (1, 3, 25):                                        # 25: the cap falls into the Or-opt phase
        t, c = E.search_tour(pts, start, cap, ROUNDS, 4)
        assert c["two_opt_sweeps"] + c["or_opt_sweeps"] == cap and c["rounds"] == 1
        assert np.array_equal(t, log[cap][1])                     # the tour before sweep cap + 1
    assert E.search_tour(pts, start, 25, ROUNDS, 4)[1]["or_opt_sweeps"] == 1
    # max_rounds = 1: the tour stops after its first Or-opt phase, where the full search starts round 2
    t, c = E.search_tour(pts, start, CAP, 1, 4)
    assert c == dict(full, rounds=1) and np.array_equal(t, full_tour)
    pts_c, start_c, tour_c, full_c, log_c, phases_c = run(64, "clustered", 4)
    t, c = E.search_tour(pts_c, start_c, CAP, 1, 4)
    assert (c["two_opt_sweeps"], c["or_opt_sweeps"], c["rounds"]) == (phases_c[0][0], phases_c[0][1], 1)
    assert np.array_equal(t, log_c[sum(phases_c[0])][1]) and not np.array_equal(t, tour_c)


@pytest.mark.parametrize("cap,rounds", [(CAP, ROUNDS), (3, ROUNDS), (CAP, 1)])
def test_a_tour_is_the_same_alone_and_in_a_group_of_three(cap, rounds):
    pts = M.instance(33, 1)[0]
    starts = np.stack([M.instance(33, s)[1] for s in (1, 2, 3)])
    solo = [E.search_tour(pts, s, cap, rounds, 4) for s in starts]
    tours, c = E.multi_local_search(pts, starts, cap, rounds, 4)
    for p in range(3):
        assert np.array_equal(tours[p], solo[p][0])
    for k in ("two_opt_sweeps", "or_opt_sweeps", "rounds"):
        assert c[k] == max(s[1][k] for s in solo)
    for k in ("two_opt_moves", "or_opt_moves"):
        assert c[k] == sum(s[1][k] for s in solo)


def test_a_two_opt_phase_after_round_one_applies_moves():
    """Clustered points: an Or-opt move between clusters opens 2-opt moves again.  Found by a scan of ``clustered_instance`` over
    n in (64, 100) and seeds 0 .. 29 with this emulation: (64, 10) and (100, 10) have the property."""
    pts, start, tour, c, log, phases = run(64, "clustered", 4)
    assert phases == [(23, 5), (2, 1), (0, 0)] and c["rounds"] == 3
    assert phases[1][0] > 0                                       # the property itself
    check_run(64, (pts, start, tour, c, log, phases))
    best = O.best_or_opt_move(pts, tour)
    assert best[0] >= -1e-6 and batched_two_opt(pts, tour[None], 10)[1] == 0
    assert run(100, "clustered", 4)[5] == [(33, 2), (4, 0)]


@pytest.mark.parametrize("n", [36, 64])
def test_ties_on_a_lattice(n):
    r = run(n, "lattice", 4)
    check_run(n, r)
    pts, start, tour, c, log, phases = r
    assert c["or_opt_moves"] > 0
    # equal deltas do occur: among the rows' lowest deltas, and among the candidates of one row
    tied_rows = tied_in_row = 0
    for name, before, winners, m in log:
        if name == "oropt":
            delta, i, v, j = E.or_opt_proposals(pts, before)
            tied_rows += len(delta) - len(set(delta.tolist()))
            d = E.or_opt_row_deltas(pts, before, 0, n - 1).reshape(n - 1, -1)
            tied_in_row += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1)[i] > 1).sum())
    assert tied_rows > 0 and tied_in_row > 0
    best = O.best_or_opt_move(pts, tour)
    assert best[0] >= -1e-6 and batched_two_opt(pts, tour[None], 10)[1] == 0


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pts = np.random.default_rng(0).random((20, 2))
    tour = np.concatenate([np.arange(20), [0]])[None]
    calls = [lambda **kw: batched_multi_local_search_torch(pts, tour, **kw),
             lambda **kw: batched_multi_local_search_grouped(pts[None], tour, **kw),
             lambda **kw: batched_multi_local_search_ragged([pts], [tour], **kw)]
    for call in calls:
        with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
            call(device="cpu")
        with pytest.raises(ValueError, match="select_rounds"):
            call(select_rounds=0)
        with pytest.raises(ValueError, match="select_rounds"):
            call(select_rounds=1.5)
        with pytest.raises(ValueError, match="max_rounds"):
            call(max_rounds=0)
        with pytest.raises(ValueError, match="max_iterations"):
            call(max_iterations=-1)
    with pytest.raises(ValueError, match="closed tours"):
        batched_multi_local_search_torch(pts, tour[:, :-1])
    with pytest.raises(ValueError, match="n >= 4"):
        batched_multi_local_search_torch(pts[:3], tour[:, :4])
    with pytest.raises(ValueError, match=r"\[groups, N, 2\]"):
        batched_multi_local_search_grouped(pts, tour)
    with pytest.raises(ValueError, match="tour arrays"):
        batched_multi_local_search_ragged([pts, pts], [tour])
    assert "multi2opt+oropt" in LOCAL_SEARCHES and check_local_search("multi2opt+oropt") == "multi2opt+oropt"
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    for bad, kw in (("multi2opt+3opt", {}), ("multi2opt+oropt", dict(two_opt_method="screened"))):
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp(model, pts, 5, local_search=bad, **kw)
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp_batch(model, pts[None], 5, local_search=bad, **kw)
        with pytest.raises(ValueError, match="local.search"):
            solve_tsp_batch(model, [pts, pts[:10]], 5, local_search=bad, **kw)


def test_evaluate_flag():
    from difusco_amd import evaluate as EV
    base = ["--task", "tsp", "--do_test", "--ckpt_path", "x.ckpt", "--storage_path", "."]
    assert EV.parse_args(base + ["--local_search", "multi2opt+oropt"])[0].local_search == "multi2opt+oropt"
    with pytest.raises(SystemExit):
        EV.parse_args(base + ["--local_search", "multi2opt+oropt", "--two_opt_method", "screened"])
    info = {"merge_iterations": 1.0, "two_opt_iterations": 7, "merged_costs": [4.0], "two_opt_moves": 31, "or_opt_iterations": 3,
            "or_opt_moves": 9, "local_search_rounds": 2}
    ex = types.SimpleNamespace(source=["f", 0], points=np.zeros((4, 2)), tour=[0, 1, 2, 3, 0])
    rec = EV.tsp_record("val", 0, ex, 5, ([0, 1, 2, 3, 0], 4.0, [4.0], info))
    assert (rec["2opt_iterations"], rec["two_opt_moves"], rec["or_opt_iterations"], rec["or_opt_moves"],
            rec["local_search_rounds"]) == (7, 31, 3, 9, 2)


def test_c_entries_reject_bad_arguments_without_gpu():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    n_ok, t_ok = np.array([5, 33], dtype=np.int32), np.array([1, 3], dtype=np.int32)
    o64 = [np.zeros(2, np.int64) for _ in range(4)]
    o32 = np.zeros(2, np.int32)
    good = (o64[0], o64[1], o32, o64[2], o64[3])
    size = lambda n, t, g=2: L.difusco_tsp_multi_local_search_ragged_workspace_bytes(g, n.ctypes.data, t.ctypes.data,
                                                                                     ctypes.byref(nbytes))
    # floor(log2(n + 1)) + 1 levels of n + 1 keys per tour: 3 levels of 6, 6 levels of 34 three times
    assert size(n_ok, t_ok) == 0 and nbytes.value > (3 * 6 + 3 * 6 * 34) * 12
    assert size(n_ok, t_ok, 0) < 0
    assert size(np.array([3, 33], dtype=np.int32), t_ok) < 0
    assert size(np.array([5, 65535 * 16 + 1], dtype=np.int32), t_ok) < 0
    assert size(n_ok, np.array([1, 0], dtype=np.int32)) < 0
    assert size(n_ok, np.array([1, 65535], dtype=np.int32)) < 0
    assert L.difusco_tsp_multi_local_search_ragged_workspace_bytes(2, None, t_ok.ctypes.data, ctypes.byref(nbytes)) < 0
    assert L.difusco_tsp_multi_local_search_ragged_workspace_bytes(2, n_ok.ctypes.data, t_ok.ctypes.data, None) < 0
    assert size(n_ok, t_ok) == 0

    def call(points=p, tours=p, cap=10, max_rounds=16, select_rounds=4, ws=p, ws_bytes=None, outs=good):
        o = [None if x is None else x.ctypes.data for x in outs]
        return L.difusco_tsp_multi_local_search_ragged(2, n_ok.ctypes.data, t_ok.ctypes.data, points, tours, cap, max_rounds,
                                                       select_rounds, ws, nbytes.value if ws_bytes is None else ws_bytes, *o, None)
    assert call(select_rounds=0) < 0 and "select_rounds" in L.difusco_last_error().decode()
    assert call(max_rounds=0) < 0 and "max_rounds" in L.difusco_last_error().decode()
    assert call(cap=-1) < 0
    assert call(points=None) < 0 and call(tours=None) < 0 and call(ws=None) < 0
    for k in range(5):
        assert call(outs=tuple(None if q == k else x for q, x in enumerate(good))) < 0
    assert call(ws_bytes=nbytes.value - 1) < 0 and "workspace" in L.difusco_last_error().decode()
    assert L.difusco_abi_version() == 13
