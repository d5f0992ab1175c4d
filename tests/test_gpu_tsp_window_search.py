"""The windowed iterated search on the GPU (difusco_tsp_window_search_ragged) against tests/tsp_window_search_emulation.py: tours,
lengths and every counter bit for bit - both pass parities, a skipped and a short last window, descents only, kicks only, the
largest window -, against the iterated entry where one window holds the tour, alone against ragged and grouped calls, and
through ``solve_tsp`` / ``solve_tsp_batch`` and the evaluation runner."""
import functools

import numpy as np
import pytest
import torch

import multi_local_search_emulation as E
import multi_two_opt_emulation as M
import tsp_iterated_search_emulation as T
import tsp_window_search_emulation as W
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")
PER = ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length", "passes_kept", "windows_searched",
       "window_sweeps", "window_moves", "closing_sweeps")
I64 = ("segments_swapped", "window_sweeps", "window_moves")
SEED, OFFSET = 12345, (1 << 62) + (3 << 32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def instance(name, n):
    """Points and one start tour: a random permutation, or the nearest-neighbour tour ("near": few sweeps to an optimum, which
    keeps the numpy reference of a large n quick).  The lattice has ties in every comparison."""
    if name == "near":
        pts = M.instance(n, 4)[0]
        return pts, M.nearest_neighbour_tour(pts)
    return {"uniform": lambda: M.instance(n, 4), "clustered": lambda: E.clustered_instance(n, 4),
            "lattice": lambda: W.lattice_instance(n, 4)}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, n, seed, offset, window, passes, kicks, kick_size, span, cap, select_rounds):
    """The emulation's result of one tour, computed once per session."""
    pts, start = instance(name, n)
    return W.search_tour(pts, start, seed, offset, window=window, passes=passes, kicks=kicks, kick_size=kick_size, span=span,
                         max_iterations=cap, select_rounds=select_rounds)


def check_invariants(pts, start, tour, per, b=0):
    n = len(start) - 1
    assert tour[0] == tour[-1] == start[0] and sorted(tour[:-1].tolist()) == list(range(n))
    assert per["final_length"][b] <= per["first_length"][b]
    assert per["final_length"][b] == T.tour_length(pts, tour)


def same_tour(tour, per, b, want):
    """Tour ``b`` of a call against the emulation's (tour, first, closing, per)."""
    ref, _, _, p = want
    assert np.array_equal(tour, ref)
    assert set(per) == set(PER)
    for k in PER:
        got = np.asarray(per[k])
        assert got.dtype == (np.float64 if k.endswith("length") else np.int64 if k in I64 else np.int32)
        assert got[b].item() == p[k], k                           # the lengths: the same float64 bits


def solo(dev, name, n, window, passes, kicks, kick_size=2, span=5, cap=200, select_rounds=4, seed=SEED, offset=OFFSET):
    """One solo call against the emulation: the tour, the per-tour arrays, the group counters and the invariants."""
    from difusco_amd.decode import batched_window_search_torch
    pts, start = instance(name, n)
    want = reference(name, n, seed, offset, window, passes, kicks, kick_size, span, cap, select_rounds)
    per = {}
    tours, stats = batched_window_search_torch(pts, start[None], cap, dev, select_rounds=select_rounds, kicks=kicks,
                                               kick_size=kick_size, span=span, seeds=[seed], offsets=[offset], stats=per,
                                               window=window, passes=passes)
    assert tours.dtype == np.int64 and tours.shape == (1, n + 1)
    check_invariants(pts, start, tours[0], per)
    same_tour(tours[0], per, 0, want)
    first, closing = want[1], want[2]
    assert stats == {k: max(first[k], closing[k]) if k == "rounds" else first[k] + closing[k] for k in KEYS}
    return tours[0], per


def test_one_window_over_the_tour_equals_the_iterated_entry(dev):
    """n = 100, W = 128, R = 1: the cuts are 0 and n, the path is the closed tour, the offset the tour's own."""
    from difusco_amd.decode import batched_iterated_search_torch
    tour, per = solo(dev, "uniform", 100, 128, 1, 5, kick_size=4, span=16, cap=1000)
    pts, start = instance("uniform", 100)
    it = {}
    want, _ = batched_iterated_search_torch(pts, start[None], 1000, dev, kicks=5, kick_size=4, span=16, seeds=[SEED], offsets=[OFFSET],
                                            stats=it)
    assert np.array_equal(tour, want[0])
    for k in ("first_length", "final_length", "kicks_kept", "kicks_improved", "segments_swapped"):
        assert per[k][0] == it[k][0], k
    assert per["passes_kept"][0] == 1 and per["windows_searched"][0] == 1 and per["closing_sweeps"][0] == 0


@pytest.mark.parametrize("name", ["uniform", "clustered", "lattice"])
def test_both_parities_a_skipped_and_a_short_window(dev, name):
    """n = 197, W = 64, R = 2: windows of 64, 64, 64, 5 (skipped), then 32, 64, 64, 37."""
    tour, per = solo(dev, name, 197, 64, 2, 3)
    assert per["windows_searched"][0] == 7


@pytest.mark.parametrize("name", ["uniform", "clustered", "lattice"])
def test_window_descents_alone(dev, name):
    tour, per = solo(dev, name, 197, 64, 2, 0)
    assert per["kicks_kept"][0] == per["segments_swapped"][0] == 0


@pytest.mark.parametrize("name", ["uniform", "clustered", "lattice"])
def test_kicks_and_keeps_alone(dev, name):
    """max_iterations = 0: no descent moves a tour, so a kicked window is kept only on a plateau or by luck."""
    tour, per = solo(dev, name, 197, 64, 2, 3, cap=0)
    assert per["window_sweeps"][0] == per["window_moves"][0] == per["closing_sweeps"][0] == 0


@pytest.mark.parametrize("select_rounds", [1, 4])
@pytest.mark.parametrize("name", ["uniform", "clustered", "lattice"])
def test_select_rounds(dev, name, select_rounds):
    solo(dev, name, 197, 64, 2, 3, select_rounds=select_rounds)


@pytest.mark.parametrize("select_rounds", [1, 4])
@pytest.mark.parametrize("name", ["uniform", "lattice"])
def test_crowded_selection(dev, name, select_rounds):
    """Descents capped at three sweeps leave the windows far from an optimum: most rows propose and their ranges meet, so the
    rounds of the selection decide who moves."""
    solo(dev, name, 197, 64, 2, 3, cap=3, select_rounds=select_rounds)


def test_the_largest_window(dev):
    """n = 1100, W = 1024: a window of 1024 edges - every thread a row, every LDS array at its last entry - and one of 76."""
    tour, per = solo(dev, "near", 1100, 1024, 1, 1, cap=1000)
    assert per["windows_searched"][0] == 2


def test_ragged_and_grouped_calls_equal_solo_calls(dev):
    from difusco_amd.decode import batched_window_search_grouped, batched_window_search_ragged, batched_window_search_torch
    sizes, counts = (50, 197, 300), (2, 1, 3)
    kw = dict(kicks=2, kick_size=2, span=5, window=64, passes=2)
    rng = np.random.default_rng(77)
    pts = [rng.random((n, 2)) for n in sizes]
    starts = [np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)]) for n, P in zip(sizes, counts)]
    total = sum(counts)
    seeds, offsets = [100 + t for t in range(total)], [(1 << 62) + (t << 32) for t in range(total)]
    per = {}
    tours, stats = batched_window_search_ragged(pts, starts, 200, dev, seeds=seeds, offsets=offsets, stats=per, **kw)
    again = {}
    tours2, stats2 = batched_window_search_ragged(pts, starts, 200, dev, seeds=seeds, offsets=offsets, stats=again, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(tours, tours2))               # two calls with the same seeds
    assert all(np.array_equal(per[k], again[k]) for k in PER) and all(np.array_equal(stats[k], stats2[k]) for k in KEYS)
    t = 0
    for g, (n, P) in enumerate(zip(sizes, counts)):
        for p in range(P):
            one = {}
            alone, _ = batched_window_search_torch(pts[g], starts[g][p][None], 200, dev, seeds=[seeds[t]], offsets=[offsets[t]],
                                                   stats=one, **kw)
            assert np.array_equal(tours[g][p], alone[0]), (g, p)
            assert all(per[k][t] == one[k][0] for k in PER), (g, p)
            check_invariants(pts[g], starts[g][p], tours[g][p], per, t)
            t += 1
    other, _ = batched_window_search_torch(pts[1], starts[1], 200, dev, seeds=[seeds[2] + 1], offsets=[offsets[2]], **kw)
    assert not np.array_equal(other[0], tours[1][0])                              # another seed, another tour
    # the grouped form: two instances of one size, two tours each
    gp = np.stack([pts[1], rng.random((197, 2))])
    gs = np.concatenate([starts[1], starts[1][:, ::-1], starts[1], starts[1][:, ::-1]])
    gper = {}
    gt, _ = batched_window_search_grouped(gp, gs, 200, dev, seeds=seeds[:4], offsets=offsets[:4], stats=gper, **kw)
    for b in range(4):
        one = {}
        alone, _ = batched_window_search_torch(gp[b // 2], gs[b][None], 200, dev, seeds=[seeds[b]], offsets=[offsets[b]], stats=one, **kw)
        assert np.array_equal(gt[b], alone[0]) and all(gper[k][b] == one[k][0] for k in PER), b


def test_refused_inputs_leave_the_tours_alone(dev):
    import ctypes
    from difusco_amd import _lib
    L = _lib.lib()
    n = 40
    pts, start = instance("uniform", n)
    starts = np.stack([start] * 3)
    d_pts = torch.from_numpy(pts.reshape(-1)).to(dev)
    d_tours = torch.from_numpy(starts.astype(np.int32).reshape(-1)).to(dev)
    d_keys = torch.zeros(3, dtype=torch.int64, device=dev)
    group_n, group_tours = np.array([n], dtype=np.int32), np.array([3], dtype=np.int32)
    nbytes = ctypes.c_size_t()
    assert L.difusco_tsp_window_search_ragged_workspace_bytes(1, group_n.ctypes.data, group_tours.ctypes.data, 16, ctypes.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    o = [np.zeros(3, np.int64) for _ in range(15)]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    ok = [1, group_n.ctypes.data, group_tours.ctypes.data, vp(d_pts), vp(d_tours), 100, 16, 4, 3, 4, 16, vp(d_keys), vp(d_keys), 16, 2,
          vp(ws), nbytes.value] + [x.ctypes.data for x in o] + [None]
    for i, v in ((8, -1), (8, 1025), (9, 0), (9, 65), (10, 0), (11, None), (12, None), (13, 15), (13, 1025), (14, 0), (14, 2 ** 31 - 1),
                 (16, nbytes.value - 1), (22, None), (31, None), (6, 0), (7, 0)):
        bad = list(ok)
        bad[i] = v
        assert L.difusco_tsp_window_search_ragged(*bad) == -1, i
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_tours.cpu().numpy().reshape(3, n + 1), starts)


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
INFO = {"merge_iterations", "two_opt_iterations", "merged_costs", "two_opt_moves", "or_opt_iterations", "or_opt_moves",
        "local_search_rounds", "local_search_kicks_improved", "local_search_closing_sweeps", "local_search_passes_kept",
        "local_search_window", "local_search_passes"}


def test_solve_tsp_batch_matches_solo(dev):
    from difusco_amd import TSPModel
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    from difusco_amd.synthetic import random_state_dict
    sd = random_state_dict(64, 2, 2, seed=0)
    B, n, P = 2, 200, 2
    pts = np.random.default_rng(12).random((B, n, 2))
    mixed = [pts[0], pts[1][:150]]
    seeds = [21, 22]
    model = lambda seed: TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=seed)
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(B)]
    kw = dict(parallel_sampling=P, two_opt_iterations=100, local_search="multi2opt+oropt")
    win = dict(kw, local_search_window=64, local_search_passes=2, local_search_kicks=2, local_search_kick_size=2,
               local_search_kick_span=5)
    res = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), **win)
    mix = solve_tsp_batch(model(0), mixed, -1, seeds=seeds, generators=gens(), **win)
    base = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), **kw)
    off = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), local_search_window=0, local_search_passes=1, **kw)
    assert off == base                                                            # window = 0: today's records exactly
    for b in range(B):
        solo_ = solve_tsp(model(seeds[b]), pts[b], -1, generator=torch.Generator().manual_seed(b), **win)
        assert res[b] == solo_, b
        assert set(solo_[3]) == INFO and len(solo_[3]["local_search_passes_kept"]) == P
        assert (solo_[3]["local_search_window"], solo_[3]["local_search_passes"]) == (64, 2)
        assert solo_[3]["merged_costs"] == base[b][3]["merged_costs"]             # the same decoded tours went in
        assert sorted(solo_[0][:-1]) == list(range(n)) and solo_[0][0] == solo_[0][-1] == 0
        assert len(solo_[2]) == P and all(x <= y + 1e-9 for x, y in zip(solo_[2], base[b][2]))   # numpy's sums of the two tours
    assert mix[0] == res[0]
    assert mix[1] == solve_tsp(model(seeds[1]), mixed[1], -1, generator=torch.Generator().manual_seed(1), **win)


def test_evaluate_with_the_flags(dev, tmp_path):
    from difusco_amd import evaluate as EV
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 3, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "3",
                 "--local_search", "multi2opt+oropt")
    flags = ["--tsp_local_search_window", "32", "--tsp_local_search_passes", "2", "--tsp_local_search_kicks", "2",
             "--tsp_local_search_kick_size", "2", "--tsp_local_search_kick_span", "5"]
    lines, recs = EV.run(argv + flags)
    full_lines, full = EV.run(argv)
    assert len(recs) == len(full) == 3
    settings = {"tsp_local_search_window": 32, "tsp_local_search_passes": 2, "tsp_local_search_kicks": 2,
                "tsp_local_search_kick_size": 2, "tsp_local_search_kick_span": 5}
    assert all(lines[0][k] == v for k, v in settings.items()) and not set(settings) & set(full_lines[0])
    for r, p in zip(recs, full):
        assert set(r) == set(p) | set(settings) | {"kicks_improved", "passes_kept", "closing_sweeps"}
        assert all(r[k] == v for k, v in settings.items())
        assert r["merged_costs"] == p["merged_costs"] and len(r["passes_kept"]) == len(r["closing_sweeps"]) == 1
        assert 0 <= r["passes_kept"][0] <= 2
    one = EV.run(argv + flags + ["--instances_per_call", "1"])[1]                 # another chunking: the same records
    assert {x["index"]: x for x in one} == {x["index"]: x for x in recs}
