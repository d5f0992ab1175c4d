"""The iterated search with focused descents on the GPU (``difusco_tsp_focused_search_ragged``): tours, the five group counters,
the per-tour arrays - the float64 lengths and ``closing_sweeps`` included - equal the numpy restatement of the rule
(tests/tsp_focused_search_emulation.py) bit for bit, whichever selection path a sweep takes (``compact_select_max`` 0, 8 and
1024): over the size ladder of the iterated search's tests, across a column chunk, on clustered points and lattices, with more
than 1024 live proposals in a focused sweep, capped, with kicks whose draws are mostly dropped, in ragged and grouped calls
against solo calls; then through ``solve_tsp`` / ``solve_tsp_batch`` and the evaluation runner."""
import functools

import numpy as np
import pytest
import torch

import multi_local_search_emulation as E
import multi_two_opt_emulation as M
import tsp_focused_search_emulation as F
import tsp_iterated_search_emulation as T
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")
PER = ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length", "closing_sweeps")
SELECT_PATHS = (0, 8, 1024)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def keys_of(n, P):
    """Distinct seeds and offsets per tour; the last offset wraps 2^64 at kick 2."""
    seeds = [1000 * n + 17 * p + 1 for p in range(P)]
    offsets = [(1 << 62) + (p << 32) for p in range(P - 1)] + [2 ** 64 - 2]
    return seeds, offsets


@functools.lru_cache(maxsize=None)
def group(n, P, kicks, kick_size=4, span=16, cap=1000, rounds=16):
    """Points, P different random-permutation start tours, their keys and the emulation's result, computed once per session."""
    rng = np.random.default_rng(9000 + n)
    pts = rng.random((n, 2))
    starts = np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)])
    seeds, offsets = keys_of(n, P)
    want = F.focused_search(pts, starts, seeds, offsets, kicks=kicks, kick_size=kick_size, span=span, max_iterations=cap,
                            max_rounds=rounds)
    return pts, starts, seeds, offsets, want


def _same(tours, stats, per, g, first, want):
    """Group ``g`` of a call, whose tours start at ``first`` of the per-tour arrays, against the emulation's (tours, c, per)."""
    ref, c, p = want
    assert np.array_equal(tours, ref)
    assert set(stats) == set(KEYS)
    assert {k: int(np.asarray(stats[k]).reshape(-1)[g]) for k in KEYS} == c
    assert set(per) == set(PER) | {"host_syncs"}
    for k in PER:
        got = np.asarray(per[k])[first:first + len(ref)]
        assert got.dtype == (np.float64 if k.endswith("length") else np.int64 if k == "segments_swapped" else np.int32)
        assert got.tolist() == list(p[k]), k                      # the lengths: the same float64 bits


def _solo(dev, pts, starts, want, **kw):
    """One solo call per selection path against the emulation's result."""
    from difusco_amd.decode import batched_iterated_search_torch
    for cmax in SELECT_PATHS:
        per = {}
        tours, stats = batched_iterated_search_torch(pts, starts, device=dev, stats=per, descent="focused", compact_select_max=cmax,
                                                     **kw)
        assert tours.dtype == np.int64 and tours.shape == np.shape(starts)
        _same(tours, {k: [v] for k, v in stats.items()}, per, 0, 0, want)
    return per


def _one(want):
    ref, c, p = want
    return ref[None], c, {k: [v] for k, v in p.items()}


@pytest.mark.parametrize("kicks", [1, 7])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n", [4, 5, 6, 7, 8, 16, 17, 33, 64, 65, 200])
def test_solo_call_equals_emulation(dev, n, P, kicks):
    pts, starts, seeds, offsets, want = group(n, P, kicks)
    per = _solo(dev, pts, starts, want, kicks=kicks, kick_size=4, span=16, seeds=seeds, offsets=offsets)
    assert per["host_syncs"] >= 3


def test_across_a_column_chunk(dev):
    """n = 1025 > 1024 from a nearest-neighbour start: the full sweeps walk two column chunks, the length has a partial sum of
    two terms, and kicks - so the lists of the focused sweeps - land on either side of position 1024."""
    n = 1025
    pts = M.instance(n, 1)[0]
    start = M.nearest_neighbour_tour(pts)
    kw = dict(kicks=3, kick_size=16, span=100)
    draws = [d for t in range(3) for d in T.kick_draws(5, 7, t, n, 16, 100)]
    assert any(a + l1 + l2 > 1000 for a, l1, l2 in draws) and any(a < 500 for a, l1, l2 in draws)
    log = []
    want = F.search_tour(pts, start, 5, 7, max_iterations=10 ** 6, log=log, **kw)
    assert any(m > 0 for _, m, _ in log)
    _solo(dev, pts, start[None], _one(want), max_iterations=10 ** 6, seeds=[5], offsets=[7], **kw)


@pytest.mark.parametrize("name", ["clustered", "lattice6", "lattice8"])
def test_other_instances(dev, name):
    """Clustered points (round 2 moves) and integer lattices: rows with equal lowest values, candidates with equal deltas."""
    pts, start = E.clustered_instance(64, 10) if name == "clustered" else E.lattice_instance(int(name[-1]), E.LATTICE_SEEDS[int(name[-1])])
    log = []
    want = F.search_tour(pts, start, 3, 1, kicks=5, kick_size=4, span=16, log=log)
    assert any(m > 0 for _, m, _ in log)
    _solo(dev, pts, start[None], _one(want), kicks=5, kick_size=4, span=16, seeds=[3], offsets=[1])


@functools.lru_cache(maxsize=None)
def crowded():
    """A random-permutation start of 2000 cities, one moving sweep per descent and 64 draws per kick: the incumbent is far from
    an optimum, so nearly every row of the focused sweep finds an improving move among the active columns."""
    n = 2000
    pts, start = M.instance(n, 3)
    log = []
    want = F.search_tour(pts, start, 9, 4, kicks=1, kick_size=64, span=30, max_iterations=1, log=log)
    return pts, start, want, max(m for _, m, _ in log)


def test_more_than_1024_live_proposals(dev):
    pts, start, want, most = crowded()
    assert most > 1024                                           # the compact selection cannot hold them: select_disjoint runs
    _solo(dev, pts, start[None], _one(want), max_iterations=1, kicks=1, kick_size=64, span=30, seeds=[9], offsets=[4])


@pytest.mark.parametrize("cap,rounds", [(0, 16), (1, 16), (3, 16), (1000, 1)])
def test_capped(dev, cap, rounds):
    """The caps are per descent, the closing one included; with a cap of 0 the call is the keeps and kicks alone."""
    if rounds == 1:                                              # the clustered case has three rounds uncapped
        pts, start = E.clustered_instance(64, 10)
        starts, (seeds, offsets) = start[None], keys_of(64, 1)
        want = F.focused_search(pts, starts, seeds, offsets, kicks=4, kick_size=4, span=16, max_iterations=cap, max_rounds=1)
    else:
        pts, starts, seeds, offsets, want = group(64, 3, 4, cap=cap)
    assert want[1]["rounds"] == 1
    assert all(a <= b for a, b in zip(want[2]["final_length"], want[2]["first_length"]))
    _solo(dev, pts, starts, want, max_iterations=cap, max_rounds=rounds, kicks=4, kick_size=4, span=16, seeds=seeds,
          offsets=offsets)


@pytest.mark.parametrize("n,kick_size,span", [(16, 64, 1), (16, 64, 10 ** 6), (33, 8, 33)])
def test_kick_parameters(dev, n, kick_size, span):
    """64 draws of two cities each on 16 positions: most draws are dropped; a span above n is clipped to (n - 1) / 2."""
    pts, starts, seeds, offsets, want = group(n, 3, 5, kick_size, span)
    _solo(dev, pts, starts, want, kicks=5, kick_size=kick_size, span=span, seeds=seeds, offsets=offsets)


def test_ragged_call_equals_solo_calls(dev):
    """Sizes 5, 64 and 200 with the same kicks: the tours of n = 5 are through their kicks and their closing descent while those
    of n = 64 are in focused sweeps and those of n = 200 still in their first full descent; and twice the same call gives the
    same answer."""
    from difusco_amd.decode import batched_iterated_search_ragged
    groups = [group(5, 3, 7), group(64, 3, 7), group(200, 3, 7)]
    kw = dict(device=dev, kicks=7, kick_size=4, span=16, seeds=sum((g[2] for g in groups), []), offsets=sum((g[3] for g in groups), []),
              descent="focused")
    per = {}
    tours, stats = batched_iterated_search_ragged([g[0] for g in groups], [g[1] for g in groups], stats=per, **kw)
    assert stats["two_opt_sweeps"].dtype == np.int64 and stats["rounds"].dtype == np.int32 and stats["rounds"].shape == (3,)
    first = 0
    for g, grp in enumerate(groups):
        _same(tours[g], stats, per, g, first, grp[4])
        first += len(grp[1])
    per2 = {}
    tours2, stats2 = batched_iterated_search_ragged([g[0] for g in groups], [g[1] for g in groups], stats=per2, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(tours, tours2))
    assert all(np.array_equal(stats[k], stats2[k]) for k in KEYS) and all(np.array_equal(per[k], per2[k]) for k in PER)


def test_grouped_call_equals_solo_calls(dev):
    from difusco_amd.decode import batched_iterated_search_grouped
    pts, starts, seeds, offsets, want = group(64, 3, 7)
    pts_b = np.random.default_rng(5).random((64, 2))             # the second group: the same starts and keys over other points
    want_b = F.focused_search(pts_b, starts, seeds, offsets, kicks=7, kick_size=4, span=16)
    per = {}
    tours, stats = batched_iterated_search_grouped(np.stack([pts, pts_b]), np.concatenate([starts, starts]), device=dev, kicks=7,
                                                   kick_size=4, span=16, seeds=seeds * 2, offsets=offsets * 2, stats=per,
                                                   descent="focused")
    _same(tours[:3], stats, per, 0, 0, want)
    _same(tours[3:], stats, per, 1, 3, want_b)


def test_a_finished_group_next_to_a_working_one(dev):
    """Groups 0 and 2 hold four nodes: every descent of theirs ends after two launch sequences, so they are done while group 1
    (n = 200) is still in its first descent."""
    from difusco_amd.decode import batched_iterated_search_ragged
    small, big = group(4, 1, 7), group(200, 3, 7)
    per = {}
    tours, stats = batched_iterated_search_ragged([small[0], big[0], small[0]], [small[1], big[1], small[1]], device=dev, kicks=7,
                                                  kick_size=4, span=16, seeds=small[2] + big[2] + small[2],
                                                  offsets=small[3] + big[3] + small[3], stats=per, descent="focused")
    _same(tours[0], stats, per, 0, 0, small[4])
    _same(tours[1], stats, per, 1, 1, big[4])
    _same(tours[2], stats, per, 2, 4, small[4])


def test_kicks_zero_is_the_multi_move_search(dev):
    from difusco_amd.decode import batched_iterated_search_ragged, batched_multi_local_search_ragged
    gs = [group(5, 3, 7), group(65, 3, 7), group(200, 3, 7)]
    for cap in (0, 3, 1000):
        want_t, want_s = batched_multi_local_search_ragged([g[0] for g in gs], [g[1] for g in gs], cap, device=dev)
        per = {}
        tours, stats = batched_iterated_search_ragged([g[0] for g in gs], [g[1] for g in gs], cap, device=dev, kicks=0, stats=per,
                                                      descent="focused")
        assert all(np.array_equal(a, b) for a, b in zip(tours, want_t))
        assert set(stats) == set(want_s) and all(np.array_equal(stats[k], want_s[k]) and stats[k].dtype == want_s[k].dtype for k in KEYS)
        assert not per["kicks_kept"].any() and not per["segments_swapped"].any() and not per["closing_sweeps"].any()
        flat = [(g[0], t) for g, ts in zip(gs, tours) for t in ts]
        assert per["first_length"].tolist() == per["final_length"].tolist() == [T.tour_length(p, t) for p, t in flat]


def test_no_move_left_after_thirty_kicks(dev):
    from difusco_amd.decode import batched_iterated_search_torch, batched_multi_local_search_torch
    n = 200
    pts = np.random.default_rng(n).random((n, 2))
    start = M.nearest_neighbour_tour(pts)
    kw = dict(kicks=30, kick_size=4, span=50)
    want = F.search_tour(pts, start, 0, 0, **kw)
    per = _solo(dev, pts, start[None], _one(want), **kw)
    tours, _ = batched_iterated_search_torch(pts, start[None], device=dev, descent="focused", **kw)
    again, stats = batched_multi_local_search_torch(pts, tours, device=dev)
    assert stats["two_opt_sweeps"] == stats["or_opt_sweeps"] == 0 and np.array_equal(again, tours)
    assert per["final_length"][0] <= per["first_length"][0]


def test_descent_full_is_todays_call(dev):
    from difusco_amd.decode import batched_iterated_search_ragged
    gs = [group(33, 1, 7), group(200, 3, 7)]
    kw = dict(device=dev, kicks=7, kick_size=4, span=16, seeds=sum((g[2] for g in gs), []), offsets=sum((g[3] for g in gs), []))
    a, b = {}, {}
    ta, sa = batched_iterated_search_ragged([g[0] for g in gs], [g[1] for g in gs], stats=a, **kw)
    tb, sb = batched_iterated_search_ragged([g[0] for g in gs], [g[1] for g in gs], stats=b, descent="full", **kw)
    assert all(np.array_equal(x, y) for x, y in zip(ta, tb)) and all(np.array_equal(sa[k], sb[k]) for k in KEYS)
    assert set(a) == set(b) == set(PER[:-1]) | {"host_syncs"} and all(np.array_equal(a[k], b[k]) for k in a)
    first = 0
    for g, grp in enumerate(gs):                                 # and it is the iterated search of the full descents
        want = T.iterated_search(grp[0], grp[1], grp[2], grp[3], kicks=7, kick_size=4, span=16)
        assert np.array_equal(tb[g], want[0])
        assert np.asarray(b["final_length"])[first:first + len(grp[1])].tolist() == want[2]["final_length"]
        first += len(grp[1])


def test_refused_inputs_leave_the_tours_alone(dev):
    import ctypes
    from difusco_amd import _lib
    L = _lib.lib()
    n = 16
    pts, starts, seeds, offsets, _ = group(n, 3, 5, 64, 1)
    d_pts = torch.from_numpy(pts.reshape(-1)).to(dev)
    d_tours = torch.from_numpy(starts.astype(np.int32).reshape(-1)).to(dev)
    d_keys = torch.zeros(3, dtype=torch.int64, device=dev)
    group_n, group_tours = np.array([n], dtype=np.int32), np.array([3], dtype=np.int32)
    nbytes = ctypes.c_size_t()
    assert L.difusco_tsp_focused_search_ragged_workspace_bytes(1, group_n.ctypes.data, group_tours.ctypes.data, ctypes.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    o = [np.zeros(3, np.int64) for _ in range(11)]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    ok = [1, group_n.ctypes.data, group_tours.ctypes.data, vp(d_pts), vp(d_tours), 100, 16, 4, 3, 4, 16, vp(d_keys), vp(d_keys), 1024,
          vp(ws), nbytes.value] + [x.ctypes.data for x in o] + [None]
    for i, v in ((8, -1), (9, 0), (9, 65), (10, 0), (11, None), (12, None), (13, -1), (13, 1025), (15, nbytes.value - 1), (21, None),
                 (26, None), (6, 0), (7, 0)):
        bad = list(ok)
        bad[i] = v
        assert L.difusco_tsp_focused_search_ragged(*bad) == -1, i
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_tours.cpu().numpy().reshape(3, n + 1), starts)


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
INFO = {"merge_iterations", "two_opt_iterations", "merged_costs", "two_opt_moves", "or_opt_iterations", "or_opt_moves",
        "local_search_rounds", "local_search_kicks_improved", "local_search_closing_sweeps"}


def test_solve_tsp_batch_matches_solo(dev):
    from difusco_amd import TSPModel
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    from difusco_amd.synthetic import random_state_dict
    sd = random_state_dict(64, 2, 2, seed=0)
    B, n, P = 3, 50, 2
    pts = np.random.default_rng(12).random((B, n, 2))
    mixed = [pts[0], pts[1][:40], pts[2]]
    seeds = [21, 22, 23]
    model = lambda seed: TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=seed)
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(B)]
    kw = dict(parallel_sampling=P, sequential_sampling=2, two_opt_iterations=100, local_search="multi2opt+oropt")
    kicked = dict(kw, local_search_kicks=10, local_search_kick_size=4, local_search_kick_span=16, local_search_descent="focused")
    res = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), **kicked)
    mix = solve_tsp_batch(model(0), mixed, -1, seeds=seeds, generators=gens(), **kicked)
    base = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), **kw)
    for b in range(B):
        solo = solve_tsp(model(seeds[b]), pts[b], -1, generator=torch.Generator().manual_seed(b), **kicked)
        assert res[b] == solo, b
        if b != 1:
            assert mix[b] == solo, b
        assert set(solo[3]) == INFO and len(solo[3]["local_search_closing_sweeps"]) == P
        assert solo[3]["merged_costs"] == base[b][3]["merged_costs"]              # the same decoded tours went in
        assert sorted(solo[0][:-1]) == list(range(n)) and solo[0][0] == solo[0][-1] == 0
        assert len(solo[2]) == 2 * P and all(x <= y for x, y in zip(solo[2], base[b][2]))   # never above the kicks = 0 cost
    solo = solve_tsp(model(seeds[1]), mixed[1], -1, generator=torch.Generator().manual_seed(1), **kicked)
    assert mix[1] == solo


def test_evaluate_with_the_flag(dev, tmp_path):
    from difusco_amd import evaluate as EV
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 4, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "4",
                 "--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "10", "--tsp_local_search_kick_size", "4",
                 "--tsp_local_search_kick_span", "16")
    flag = ["--tsp_local_search_descent", "focused"]
    lines, recs = EV.run(argv + flag)
    full_lines, full = EV.run(argv)
    assert len(recs) == len(full) == 4
    assert lines[0]["tsp_local_search_descent"] == "focused" and "tsp_local_search_descent" not in full_lines[0]
    for r, p in zip(recs, full):
        assert set(r) == set(p) | {"closing_sweeps", "tsp_local_search_descent"} and r["tsp_local_search_descent"] == "focused"
        assert r["merged_costs"] == p["merged_costs"] and len(r["closing_sweeps"]) == 1
    one = EV.run(argv + flag + ["--instances_per_call", "1"])[1]              # another chunking: the same records
    two = EV.run(argv + flag + ["--instances_per_call", "3"])[1]
    by = lambda rs: {x["index"]: x for x in rs}
    assert by(one) == by(two) == by(recs)
