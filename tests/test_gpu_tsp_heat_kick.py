"""The heat-biased kicks of the iterated TSP search on the GPU (``difusco_tsp_guided_search_ragged``): tours, the five group
counters and the per-tour arrays equal the numpy restatement of the rule (tests/tsp_heat_kick_emulation.py) bit for bit, for
both descents: over a size ladder with a different heat per tour, on dense heat, on the corners of heat and graph, where the
draws concentrate on two cold edges, where the running weights pass 2^32, in ragged and grouped calls against solo calls; the
refusals; then through ``solve_tsp`` / ``solve_tsp_batch`` and the evaluation runner."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tsp_heat_kick_emulation as H
import tsp_iterated_search_emulation as T
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp
from test_tsp_heat_kick_host import CONC_OFFSET, CONC_SEED, concentration_case, tour_graph

pytestmark = pytest.mark.gpu
KEYS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")
PER = ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length")
KW = dict(kick_size=4, span=16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def edge_index_of(rp, col):
    """[2, E] of a CSR: the row of every entry over its column."""
    return np.stack([np.repeat(np.arange(len(rp) - 1), np.diff(rp)), col]).astype(np.int64)


def keys_of(n, P):
    return [1000 * n + 17 * p + 1 for p in range(P)], [(1 << 62) + (p << 32) for p in range(P)]


@functools.lru_cache(maxsize=None)
def group(n, P, kicks, descent="full", compact=1024):
    """Points, P random-permutation start tours, the k-NN graph (self included, K = min(n, 8)), one uniform heat per tour, the keys
    and the emulation's result, computed once per session."""
    rng = np.random.default_rng(7000 + n)
    pts = rng.random((n, 2))
    starts = np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)])
    rp, col = H.knn_csr(pts, 8)
    heat = rng.random((P, len(col))).astype(np.float32)
    seeds, offsets = keys_of(n, P)
    want = H.guided_search(pts, starts, rp, col, heat, seeds, offsets, kicks=kicks, descent=descent, compact_select_max=compact,
                           **KW)
    return pts, starts, edge_index_of(rp, col), heat, seeds, offsets, want


def _same(tours, stats, per, g, first, want, focused):
    """Group ``g`` of a call, whose tours start at ``first`` of the per-tour arrays, against the emulation's (tours, c, per)."""
    ref, c, p = want
    assert np.array_equal(tours, ref)
    assert set(stats) == set(KEYS)
    assert {k: int(np.asarray(stats[k]).reshape(-1)[g]) for k in KEYS} == c
    names = PER + (("closing_sweeps",) if focused else ())
    assert set(per) == set(names) | {"host_syncs"} and set(p) == set(names)
    for k in names:
        got = np.asarray(per[k])[first:first + len(ref)]
        assert got.dtype == (np.float64 if k.endswith("length") else np.int64 if k == "segments_swapped" else np.int32)
        assert got.tolist() == list(p[k]), k                      # the lengths: the same float64 bits


def solo(dev, g, kicks, descent="full", compact=1024, cap=1000):
    from difusco_amd.decode import batched_iterated_search_torch
    pts, starts, ei, heat, seeds, offsets, _ = g
    per = {}
    tours, stats = batched_iterated_search_torch(pts, starts, cap, device=dev, kicks=kicks, seeds=seeds, offsets=offsets, stats=per,
                                                 descent=descent, compact_select_max=compact, kick_bias="heat", heat=heat,
                                                 edge_index=ei, **KW)
    return tours, stats, per


@pytest.mark.parametrize("descent", ["full", "focused"])
@pytest.mark.parametrize("kicks", [1, 7])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n", [4, 5, 8, 16, 17, 33, 64, 65, 200])
def test_solo_call_equals_emulation(dev, n, P, kicks, descent):
    g = group(n, P, kicks, descent)
    tours, stats, per = solo(dev, g, kicks, descent)
    assert tours.dtype == np.int64 and tours.shape == (P, n + 1)
    _same(tours, {k: [v] for k, v in stats.items()}, per, 0, 0, g[6], descent == "focused")
    assert per["host_syncs"] >= 3


@pytest.mark.parametrize("compact", [0, 1024])
def test_compact_select_max_changes_nothing(dev, compact):
    g = group(64, 3, 7, "focused", compact)
    tours, stats, per = solo(dev, g, 7, "focused", compact)
    _same(tours, {k: [v] for k, v in stats.items()}, per, 0, 0, g[6], True)
    assert np.array_equal(g[6][0], group(64, 3, 7, "focused")[6][0])


@pytest.mark.parametrize("descent", ["full", "focused"])
@pytest.mark.parametrize("n", [8, 16])
def test_dense_heat(dev, n, descent):
    """[P, N, N] with no edge_index: the complete graph, entry (i, j) at i N + j - and as a device tensor."""
    from difusco_amd.decode import batched_iterated_search_torch
    P = 2
    pts, starts, _, _, seeds, offsets, _ = group(n, P, 7, descent)
    heat = np.random.default_rng(n).random((P, n, n)).astype(np.float32)
    rp, col = np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n)
    want = H.guided_search(pts, starts, rp, col, heat.reshape(P, -1), seeds, offsets, kicks=7, descent=descent, **KW)
    for h in (heat, torch.from_numpy(heat).to(dev)):
        per = {}
        tours, stats = batched_iterated_search_torch(pts, starts, device=dev, kicks=7, seeds=seeds, offsets=offsets, stats=per,
                                                     descent=descent, kick_bias="heat", heat=h, **KW)
        _same(tours, {k: [v] for k, v in stats.items()}, per, 0, 0, want, descent == "focused")


@pytest.mark.parametrize("descent", ["full", "focused"])
def test_heat_corners_in_one_call(dev, descent):
    """Six groups over the same 33 points: heat all zeros, all ones, outside [0, 1] and NaN, a graph with empty rows, duplicate
    entries, and a graph that holds hardly any edge of the tours.  The edge lists are given unsorted: the layer sorts them."""
    from difusco_amd.decode import batched_iterated_search_ragged
    n, P = 33, 2
    pts, starts, ei, _, seeds, offsets, _ = group(n, P, 7, descent)
    rng = np.random.default_rng(33)
    E = ei.shape[1]
    wild = rng.random((P, E)).astype(np.float32) * 4 - 2
    wild[:, ::5] = np.nan
    wild[:, 1::7] = np.inf
    wild[:, 2::11] = -np.inf
    keep = ei[0] % 3 != 0                                        # rows 0, 3, 6, .. are empty
    dup = np.concatenate([ei, ei[:, ::2]], axis=1)                # every second entry twice, with another heat
    few = np.array([[0, 5, 5, 32], [1, 5, 6, 0]], dtype=np.int64)
    cases = [(ei, np.zeros((P, E), np.float32)), (ei, np.ones((P, E), np.float32)), (ei, wild),
             (ei[:, keep], rng.random((P, int(keep.sum()))).astype(np.float32)),
             (dup, rng.random((P, dup.shape[1])).astype(np.float32)), (few, rng.random((P, 4)).astype(np.float32))]
    shuffled = []
    for e, h in cases:
        order = rng.permutation(e.shape[1])
        shuffled.append((e[:, order], h[:, order]))
    per = {}
    tours, stats = batched_iterated_search_ragged([pts] * 6, [starts] * 6, device=dev, kicks=7, seeds=seeds * 6, offsets=offsets * 6,
                                                  stats=per, descent=descent, kick_bias="heat", heat=[h for _, h in shuffled],
                                                  edge_index=[e for e, _ in shuffled], **KW)
    for g, (e, h) in enumerate(shuffled):
        order = np.argsort(e[0], kind="stable")
        rp = np.concatenate([[0], np.cumsum(np.bincount(e[0], minlength=n))]).astype(np.int32)
        want = H.guided_search(pts, starts, rp, e[1][order], h[:, order], seeds, offsets, kicks=7, descent=descent, **KW)
        _same(tours[g], stats, per, g, g * P, want, descent == "focused")


def test_concentration(dev):
    """The case of the host test, kicks alone: every draw falls behind position 20 or 40, so at most two are kept."""
    from difusco_amd.decode import batched_iterated_search_torch
    pts, tour, rp, col, heat = concentration_case()
    kw = dict(kicks=1, kick_size=16, span=3, seeds=[CONC_SEED], offsets=[CONC_OFFSET])
    ref, c, p = H.search_tour(pts, tour, rp, col, heat, CONC_SEED, CONC_OFFSET, kicks=1, kick_size=16, span=3, max_iterations=0)
    per, uni = {}, {}
    tours, stats = batched_iterated_search_torch(pts, tour[None], 0, device=dev, stats=per, kick_bias="heat", heat=heat[None],
                                                 edge_index=edge_index_of(rp, col), **kw)
    assert np.array_equal(tours[0], ref) and {k: int(stats[k]) for k in KEYS} == c
    assert per["segments_swapped"].tolist() == [p["segments_swapped"]] and p["segments_swapped"] in (1, 2)
    assert per["first_length"].tolist() == [p["first_length"]] and per["final_length"].tolist() == [p["final_length"]]
    batched_iterated_search_torch(pts, tour[None], 0, device=dev, stats=uni, **kw)
    assert uni["segments_swapped"][0] > per["segments_swapped"][0]


def test_64_bit_prefix(dev):
    """n = 70001 with all heat 0: W_M > 2^32.  Kicks alone (max_iterations = 0), a one-edge-per-row graph."""
    from difusco_amd import _lib
    from difusco_amd.decode import batched_iterated_search_torch
    n = 70001
    group_n, group_tours, nbytes = np.array([n], dtype=np.int32), np.array([1], dtype=np.int32), ctypes.c_size_t()
    assert _lib.lib().difusco_tsp_guided_search_ragged_workspace_bytes(1, group_n.ctypes.data, group_tours.ctypes.data,
                                                                       group_n.ctypes.data, ctypes.byref(nbytes)) == 0
    assert nbytes.value <= 1 << 30
    pts = np.random.default_rng(n).random((n, 2))
    tour = np.concatenate([np.arange(n), [0]])
    rp, col, _ = tour_graph(tour)
    heat = np.zeros(n, dtype=np.float32)
    kw = dict(kicks=2, kick_size=16, span=30)
    log = []
    ref, c, p = H.search_tour(pts, tour, rp, col, heat, 9, 5, max_iterations=0, draws_log=log, **kw)
    assert any(a * 65536 > 2 ** 32 for d in log for a, _, _ in d)
    per = {}
    tours, stats = batched_iterated_search_torch(pts, tour[None], 0, device=dev, seeds=[9], offsets=[5], stats=per, kick_bias="heat",
                                                 heat=heat[None], edge_index=edge_index_of(rp, col), **kw)
    assert np.array_equal(tours[0], ref) and {k: int(stats[k]) for k in KEYS} == c
    assert all(per[k].tolist() == [p[k]] for k in PER)
    assert p["segments_swapped"] == sum(sum(T.apply_kick(tour, d)[1]) for d in log) > 0


@pytest.mark.parametrize("descent", ["full", "focused"])
def test_ragged_call_equals_solo_calls(dev, descent):
    from difusco_amd.decode import batched_iterated_search_ragged
    gs = [group(12, 2, 7, descent), group(40, 1, 7, descent), group(200, 3, 7, descent)]
    per = {}
    tours, stats = batched_iterated_search_ragged([g[0] for g in gs], [g[1] for g in gs], device=dev, kicks=7,
                                                  seeds=sum((g[4] for g in gs), []), offsets=sum((g[5] for g in gs), []), stats=per,
                                                  descent=descent, kick_bias="heat", heat=[g[3] for g in gs],
                                                  edge_index=[g[2] for g in gs], **KW)
    first = 0
    for i, g in enumerate(gs):
        t1, s1, p1 = solo(dev, g, 7, descent)
        assert np.array_equal(tours[i], t1) and all(int(stats[k][i]) == s1[k] for k in KEYS)
        assert all(np.array_equal(per[k][first:first + len(t1)], p1[k]) for k in p1 if k != "host_syncs")
        _same(tours[i], stats, per, i, first, g[6], descent == "focused")
        first += len(t1)


def test_grouped_call_equals_solo_calls(dev):
    from difusco_amd.decode import batched_iterated_search_grouped
    a = group(64, 3, 7)
    heat_b = a[3][::-1].copy()                                   # the second group: the same points, starts and keys, another heat
    per = {}
    tours, stats = batched_iterated_search_grouped(np.stack([a[0], a[0]]), np.concatenate([a[1], a[1]]), device=dev, kicks=7,
                                                   seeds=a[4] * 2, offsets=a[5] * 2, stats=per, kick_bias="heat",
                                                   heat=[a[3], heat_b], edge_index=[a[2], a[2]], **KW)
    _same(tours[:3], stats, per, 0, 0, a[6], False)
    tb, sb, pb = solo(dev, a[:3] + (heat_b,) + a[4:], 7)
    assert np.array_equal(tours[3:], tb) and all(int(stats[k][1]) == sb[k] for k in KEYS)
    assert all(np.array_equal(per[k][3:], pb[k]) for k in PER)


def test_a_finished_group_next_to_a_working_one(dev):
    from difusco_amd.decode import batched_iterated_search_ragged
    small, big = group(4, 1, 7, "focused"), group(200, 3, 7, "focused")
    gs = [small, big, small]
    per = {}
    tours, stats = batched_iterated_search_ragged([g[0] for g in gs], [g[1] for g in gs], device=dev, kicks=7,
                                                  seeds=sum((g[4] for g in gs), []), offsets=sum((g[5] for g in gs), []), stats=per,
                                                  descent="focused", kick_bias="heat", heat=[g[3] for g in gs],
                                                  edge_index=[g[2] for g in gs], **KW)
    _same(tours[0], stats, per, 0, 0, small[6], True)
    _same(tours[1], stats, per, 1, 1, big[6], True)
    _same(tours[2], stats, per, 2, 4, small[6], True)


@pytest.mark.parametrize("descent", ["full", "focused"])
def test_kicks_zero_is_the_multi_move_search(dev, descent):
    from difusco_amd.decode import batched_multi_local_search_torch
    g = group(65, 3, 7)
    for cap in (0, 3, 1000):
        want_t, want_s = batched_multi_local_search_torch(g[0], g[1], cap, device=dev)
        tours, stats, per = solo(dev, g, 0, descent, cap=cap)
        assert np.array_equal(tours, want_t) and stats == want_s
        assert not per["kicks_kept"].any() and not per["segments_swapped"].any()
        assert per["first_length"].tolist() == per["final_length"].tolist() == [T.tour_length(g[0], t) for t in tours]


def test_refused_inputs_leave_the_tours_alone(dev):
    from difusco_amd import _lib
    from difusco_amd.decode import batched_iterated_search_grouped, batched_iterated_search_torch
    L = _lib.lib()
    n = 16
    pts, starts, ei, heat, seeds, offsets, _ = group(n, 3, 7)
    rp, col = H.knn_csr(pts, 8)
    d_pts = torch.from_numpy(pts.reshape(-1)).to(dev)
    d_tours = torch.from_numpy(starts.astype(np.int32).reshape(-1)).to(dev)
    d_keys = torch.zeros(3, dtype=torch.int64, device=dev)
    d_rp, d_col, d_heat = (torch.from_numpy(x).to(dev) for x in (rp, col, heat.reshape(-1)))
    group_n, group_tours, group_edges = (np.array([v], dtype=np.int32) for v in (n, 3, len(col)))
    nbytes = ctypes.c_size_t()
    assert L.difusco_tsp_guided_search_ragged_workspace_bytes(1, group_n.ctypes.data, group_tours.ctypes.data,
                                                              group_edges.ctypes.data, ctypes.byref(nbytes)) == 0
    assert L.difusco_tsp_guided_search_ragged_workspace_bytes(1, group_n.ctypes.data, group_tours.ctypes.data, None,
                                                              ctypes.byref(nbytes)) == -1
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    o = [np.zeros(3, np.int64) for _ in range(11)]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(**over):
        a = dict(edges=group_edges.ctypes.data, rp=vp(d_rp), col=vp(d_col), heat=vp(d_heat), descent=0, closing=o[10].ctypes.data,
                 kick_size=4, ws=nbytes.value)
        a.update(over)
        return L.difusco_tsp_guided_search_ragged(1, group_n.ctypes.data, group_tours.ctypes.data, vp(d_pts), vp(d_tours), 100, 16, 4,
                                                  3, a["kick_size"], 16, vp(d_keys), vp(d_keys), 1024, a["descent"], a["edges"],
                                                  a["rp"], a["col"], a["heat"], vp(ws), a["ws"], *[x.ctypes.data for x in o[:10]],
                                                  a["closing"], None)
    bad_rp = [rp.copy() for _ in range(4)]
    bad_rp[0][0] = 1                                             # row_ptr[0] != 0
    bad_rp[1][n] = len(col) - 1                                  # row_ptr[n] != E
    bad_rp[2][5], bad_rp[2][6] = rp[6], rp[5]                    # not rising
    bad_rp[3][3] = -4
    bad_col = [col.copy() for _ in range(2)]
    bad_col[0][7] = n
    bad_col[1][len(col) - 1] = -1
    negative = np.array([-1], dtype=np.int32)
    refused = [dict(heat=None), dict(rp=None), dict(col=None), dict(edges=None), dict(edges=negative.ctypes.data), dict(descent=2),
               dict(descent=-1), dict(descent=1, closing=None), dict(kick_size=65), dict(ws=nbytes.value - 1)]
    tensors = [torch.from_numpy(x).to(dev) for x in bad_rp + bad_col]
    refused += [dict(rp=vp(t)) for t in tensors[:4]] + [dict(col=vp(t)) for t in tensors[4:]]
    for over in refused:
        assert call(**over) == -1, over
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_tours.cpu().numpy().reshape(3, n + 1), starts), over
    assert b"CSR" in L.difusco_last_error()
    # the Python layer, before any library call
    kw = dict(device=dev, kicks=3, kick_bias="heat")
    for h, e in ((heat[:, :-1], ei), (heat[:2], ei), (heat, ei[:, :-1]), (heat, ei[0]), (heat, None),
                 (np.zeros((3, n, n - 1), np.float32), None)):
        with pytest.raises(ValueError):
            batched_iterated_search_torch(pts, starts, heat=h, edge_index=e, **kw)
    out_of_range = ei.copy()
    out_of_range[1, 3] = n
    with pytest.raises(ValueError, match="outside"):
        batched_iterated_search_torch(pts, starts, heat=heat, edge_index=out_of_range, **kw)
    with pytest.raises(ValueError):
        batched_iterated_search_grouped(pts[None], starts, heat=[heat, heat], edge_index=[ei, ei], **kw)
    with pytest.raises(ValueError, match="only with kick_bias='heat'"):
        batched_iterated_search_torch(pts, starts, device=dev, kicks=3, heat=heat, edge_index=ei)
    with pytest.raises(ValueError, match="kick_bias"):
        batched_iterated_search_torch(pts, starts, device=dev, kicks=3, kick_bias="warm", heat=heat, edge_index=ei)
    # descent = 0 takes a null closing_sweeps_out, and the valid call runs
    assert call(closing=None) == 0
    assert call(descent=1) == 0


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
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
    kw = dict(parallel_sampling=P, sequential_sampling=2, two_opt_iterations=100, local_search="multi2opt+oropt",
              local_search_kicks=10, local_search_kick_size=4, local_search_kick_span=16)
    heat = dict(kw, local_search_kick_bias="heat")
    res = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), **heat)
    mix = solve_tsp_batch(model(0), mixed, -1, seeds=seeds, generators=gens(), merge_method="batched", **heat)
    uniform = solve_tsp_batch(model(0), pts, -1, seeds=seeds, generators=gens(), **kw)
    for b in range(B):
        solo_b = solve_tsp(model(seeds[b]), mixed[b], -1, generator=torch.Generator().manual_seed(b), **heat)
        assert mix[b] == solo_b, b
        if b != 1:
            assert res[b] == solo_b, b
        assert solo_b[3]["local_search_kick_bias"] == "heat" and "local_search_kick_bias" not in uniform[b][3]
        assert sorted(solo_b[0][:-1]) == list(range(len(mixed[b]))) and solo_b[0][0] == solo_b[0][-1] == 0
        assert res[b][3]["merged_costs"] == uniform[b][3]["merged_costs"]         # the same decoded tours went in
    focused = solve_tsp_batch(model(0), pts[:1], -1, seeds=seeds[:1], generators=gens()[:1], local_search_descent="focused", **heat)
    solo_f = solve_tsp(model(seeds[0]), pts[0], -1, generator=torch.Generator().manual_seed(0), local_search_descent="focused", **heat)
    assert focused[0] == solo_f and "local_search_closing_sweeps" in solo_f[3]


def test_sparse_pipeline_matches_solo(dev):
    """The k-NN path: the sample's heat in the edge order of the instance's own graph."""
    from difusco_amd import TSPModel
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    from difusco_amd.synthetic import random_state_dict
    sd = random_state_dict(64, 2, 2, seed=0)
    pts = np.random.default_rng(13).random((2, 50, 2))
    model = lambda seed: TSPModel(_model_args(sparse_factor=8, hidden_dim=64, n_layers=2), sd, device=dev, seed=seed)
    kw = dict(parallel_sampling=2, two_opt_iterations=100, local_search="multi2opt+oropt", local_search_kicks=5,
              local_search_kick_size=4, local_search_kick_span=16, local_search_kick_bias="heat")
    res = solve_tsp_batch(model(0), pts, 8, seeds=[5, 6], generators=[torch.Generator().manual_seed(b) for b in range(2)], **kw)
    for b in range(2):
        assert res[b] == solve_tsp(model(5 + b), pts[b], 8, generator=torch.Generator().manual_seed(b), **kw)


def test_evaluate_with_the_flag(dev, tmp_path):
    from difusco_amd import TSPModel, evaluate as EV
    from difusco_amd.datasets import read_tsp_split
    from difusco_amd.pipeline import solve_tsp
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 3, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "3",
                 "--local_search", "multi2opt+oropt", "--tsp_local_search_kicks", "10", "--tsp_local_search_kick_size", "4",
                 "--tsp_local_search_kick_span", "16")
    lines, recs = EV.run(argv + ["--tsp_local_search_kick_bias", "heat"])
    plain_lines, plain = EV.run(argv)
    assert lines[0]["tsp_local_search_kick_bias"] == "heat" and "tsp_local_search_kick_bias" not in plain_lines[0]
    examples = read_tsp_split(split)
    for r, p in zip(recs, plain):
        assert set(r) == set(p) | {"tsp_local_search_kick_bias"} and r["merged_costs"] == p["merged_costs"]
        m = TSPModel(_model_args(sparse_factor=-1, hidden_dim=64, n_layers=2), sd, device=dev, seed=r["seed"])
        one = solve_tsp(m, examples[r["index"]].points, -1, two_opt_iterations=100, generator=torch.Generator().manual_seed(r["seed"]),
                        local_search="multi2opt+oropt", local_search_kicks=10, local_search_kick_size=4, local_search_kick_span=16,
                        local_search_kick_bias="heat")
        want = EV.tsp_record("val", r["index"], examples[r["index"]], r["seed"], one)
        assert {k: v for k, v in r.items() if not k.startswith("tsp_local_search")} == want
