"""The heatmap-guided sampled k-opt search on the GPU (``difusco_tsp_kopt_search_ragged``): tours, the four counters and both
lengths equal the python restatement of the rule (tests/tsp_kopt_search_emulation.py) bit for bit over the cases of
tests/tsp_kopt_search_cases.py - a size ladder, the sample counts around a block and around the round kernel's stride, depths 1,
2 and 10, the corners of graph and heat, tours that stall next to tours that run on, offsets that cross 2^32 and 2^64, a begin
position n - 1, no round at all -; solo, grouped and ragged calls agree; the refusals; the pipeline and the runner with the
stage off."""
import ctypes

import numpy as np
import pytest
import torch

import tsp_kopt_search_cases as C
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu
PER = ("rounds", "actions", "depth_sum", "reverted", "first_length", "final_length")
DTYPES = dict(rounds=np.int32, actions=np.int32, depth_sum=np.int64, reverted=np.int32, first_length=np.float64,
              final_length=np.float64)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def ragged(dev, groups, kw):
    from difusco_amd.decode import batched_kopt_search_ragged
    per = {}
    tours = batched_kopt_search_ragged([g[0] for g in groups], [g[1] for g in groups], heat=[g[4] for g in groups],
                                       edge_index=[C.edge_index_of(g[2], g[3]) for g in groups], samples=kw["samples"],
                                       depth=kw["depth"], rounds=kw["max_rounds"], patience=kw["patience"], alpha=C.ALPHA,
                                       beta=C.BETA, seeds=sum((g[5] for g in groups), []), offsets=sum((g[6] for g in groups), []),
                                       stats=per, device=dev)
    return tours, per


def same(tours, per, first, want):
    """The tours of one group, which start at ``first`` of the per-tour arrays, against the emulation's (tours, per)."""
    ref, p = want
    assert tours.dtype == np.int64 and np.array_equal(tours, ref)
    assert set(per) == set(PER) | {"host_syncs"}
    for k in PER:
        got = np.asarray(per[k])[first:first + len(ref)]
        assert got.dtype == DTYPES[k]
        assert got.tolist() == list(p[k]), k                      # the lengths: the same float64 bits


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_ragged_call_equals_emulation(dev, name):
    groups, kw = C.cases()[name]
    want, _ = C.expected(name)
    tours, per = ragged(dev, groups, kw)
    first = 0
    for g, t, w in zip(groups, tours, want):
        assert t.shape == g[1].shape
        same(t, per, first, w)
        first += len(t)
    assert (per["final_length"] <= per["first_length"]).all() and not per["reverted"].any()
    # the setup and the counters, and one poll per 8 rounds while tours are running
    assert 2 <= per["host_syncs"] <= 2 + -(-kw["max_rounds"] // 8)
    if name == "R0":
        assert per["host_syncs"] == 2 and all(np.array_equal(t, g[1]) for g, t in zip(groups, tours))


def test_solo_grouped_and_ragged_calls_agree(dev):
    from difusco_amd.decode import batched_kopt_search_grouped, batched_kopt_search_torch
    a, kw = C.group(65, 3), dict(samples=64, depth=10, rounds=9, patience=10, alpha=C.ALPHA, beta=C.BETA)
    want = C.expected("ladder-n65")[0][0]
    ei = C.edge_index_of(a[2], a[3])
    per = {}
    solo = batched_kopt_search_torch(a[0], a[1], heat=a[4], edge_index=ei, seeds=a[5], offsets=a[6], stats=per, device=dev, **kw)
    same(solo, per, 0, want)
    for b in range(3):                                           # one tour alone
        one = {}
        t = batched_kopt_search_torch(a[0], a[1][b:b + 1], heat=a[4][b:b + 1], edge_index=ei, seeds=a[5][b:b + 1],
                                      offsets=a[6][b:b + 1], stats=one, device=dev, **kw)
        assert np.array_equal(t[0], solo[b]) and all(one[k][0] == per[k][b] for k in PER)
    heat_b = a[4][::-1].copy()                                   # a second group: the same points, tours and keys, another heat
    both = {}
    tours = batched_kopt_search_grouped(np.stack([a[0], a[0]]), np.concatenate([a[1], a[1]]), heat=[a[4], heat_b],
                                        edge_index=[ei, ei], seeds=a[5] * 2, offsets=a[6] * 2, stats=both, device=dev, **kw)
    same(tours[:3], both, 0, want)
    other = {}
    tb = batched_kopt_search_torch(a[0], a[1], heat=heat_b, edge_index=ei, seeds=a[5], offsets=a[6], stats=other, device=dev, **kw)
    assert np.array_equal(tours[3:], tb) and all(np.array_equal(both[k][3:], other[k]) for k in PER)
    assert not np.array_equal(tb, solo)                          # the heat decides where the search goes
    # in a ragged call next to groups of other sizes
    gs = [C.group(7, 3), a, C.group(200, 1)]
    tr, pr = ragged(dev, gs, dict(samples=64, depth=10, max_rounds=9, patience=10))
    same(tr[1], pr, 3, want)
    same(tr[0], pr, 0, C.expected("ladder-n7")[0][0])
    same(tr[2], pr, 6, C.expected("ladder-n200")[0][0])


def test_dense_heat(dev):
    """[P, N, N] with no edge_index: the complete graph, entry (i, j) at i N + j, the diagonal no candidate."""
    import tsp_kopt_search_emulation as K
    from difusco_amd.decode import batched_kopt_search_torch
    n, P = 16, 2
    pts, starts, _, _, _, seeds, offsets = C.group(n, 3)
    heat = np.random.default_rng(n).random((P, n, n)).astype(np.float32)
    rp, col = np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n)
    want = K.kopt_search(pts, starts[:P], rp, col, heat.reshape(P, -1), seeds[:P], offsets[:P], samples=32, depth=5, max_rounds=6,
                         beta=C.BETA, explore=C.explore(32, 6))
    assert sum(want[1]["actions"]) > 0
    per = {}
    tours = batched_kopt_search_torch(pts, starts[:P], heat=torch.from_numpy(heat).to(dev), samples=32, depth=5, rounds=6,
                                      seeds=seeds[:P], offsets=offsets[:P], stats=per, device=dev)
    same(tours, per, 0, want)


def test_refused_inputs_leave_the_tours_alone(dev):
    from difusco_amd import _lib
    from difusco_amd.decode import batched_kopt_search_grouped, batched_kopt_search_torch
    L = _lib.lib()
    n = 16
    pts, starts, rp, col, heat, seeds, offsets = C.group(n, 3)
    d_pts = torch.from_numpy(pts.reshape(-1)).to(dev)
    d_tours = torch.from_numpy(starts.astype(np.int32).reshape(-1)).to(dev)
    d_keys = torch.zeros(3, dtype=torch.int64, device=dev)
    d_rp, d_col, d_heat = (torch.from_numpy(x).to(dev) for x in (rp, col, heat.reshape(-1)))
    group_n, group_tours, group_edges = (np.array([v], dtype=np.int32) for v in (n, 3, len(col)))
    negative = np.array([-1], dtype=np.int32)
    nbytes = ctypes.c_size_t()
    size = lambda edges, S, D: L.difusco_tsp_kopt_search_ragged_workspace_bytes(1, group_n.ctypes.data, group_tours.ctypes.data, edges,
                                                                                S, D, ctypes.byref(nbytes))
    assert size(None, 64, 10) == size(negative.ctypes.data, 64, 10) == size(group_edges.ctypes.data, 0, 10) == -1
    assert size(group_edges.ctypes.data, 4097, 10) == size(group_edges.ctypes.data, 64, 0) == size(group_edges.ctypes.data, 64, 11) == -1
    assert size(group_edges.ctypes.data, 64, 10) == 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    o = [np.zeros(3, np.int64) for _ in range(6)]
    explore = C.explore(64, 4)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(**over):
        a = dict(edges=group_edges.ctypes.data, rp=vp(d_rp), col=vp(d_col), heat=vp(d_heat), seeds=vp(d_keys), S=64, D=10, R=4, H=10,
                 beta=10.0, explore=explore.ctypes.data, ws=nbytes.value, out5=o[5].ctypes.data, tours=vp(d_tours))
        a.update(over)
        return L.difusco_tsp_kopt_search_ragged(1, group_n.ctypes.data, group_tours.ctypes.data, vp(d_pts), a["tours"], a["edges"],
                                                a["rp"], a["col"], a["heat"], a["seeds"], vp(d_keys), a["S"], a["D"], a["R"], a["H"],
                                                a["beta"], a["explore"], vp(ws), a["ws"], *[x.ctypes.data for x in o[:5]], a["out5"],
                                                None)
    bad_rp = [rp.copy() for _ in range(4)]
    bad_rp[0][0] = 1                                             # row_ptr[0] != 0
    bad_rp[1][n] = len(col) - 1                                  # row_ptr[n] != E
    bad_rp[2][5], bad_rp[2][6] = rp[6], rp[5]                    # not rising
    bad_rp[3][3] = -4
    bad_col = [col.copy() for _ in range(2)]
    bad_col[0][7] = n
    bad_col[1][len(col) - 1] = -1
    bad_explore = [explore.copy() for _ in range(3)]
    bad_explore[0][1], bad_explore[1][2], bad_explore[2][3] = -1.0, np.nan, np.inf
    refused = [dict(heat=None), dict(rp=None), dict(col=None), dict(edges=None), dict(edges=negative.ctypes.data), dict(seeds=None),
               dict(tours=None), dict(S=0), dict(S=4097), dict(D=0), dict(D=11), dict(R=-1), dict(H=0), dict(beta=-1.0),
               dict(beta=float("nan")), dict(beta=float("inf")), dict(explore=None), dict(out5=None), dict(ws=nbytes.value - 1)]
    refused += [dict(explore=x.ctypes.data) for x in bad_explore]
    tensors = [torch.from_numpy(x).to(dev) for x in bad_rp + bad_col]
    refused += [dict(rp=vp(t)) for t in tensors[:4]] + [dict(col=vp(t)) for t in tensors[4:]]
    for over in refused:
        assert call(**over) == -1, over
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_tours.cpu().numpy().reshape(3, n + 1), starts), over
    assert b"CSR" in L.difusco_last_error()
    assert call(R=0, explore=None) == 0                          # no round reads no explore
    assert np.array_equal(d_tours.cpu().numpy().reshape(3, n + 1), starts)
    assert call() == 0
    # the Python layer, before any library call
    ei = C.edge_index_of(rp, col)
    for h, e in ((heat[:, :-1], ei), (heat[:2], ei), (heat, ei[:, :-1]), (heat, None), (None, ei)):
        with pytest.raises(ValueError):
            batched_kopt_search_torch(pts, starts, heat=h, edge_index=e, device=dev)
    for bad in (dict(samples=0), dict(samples=4097), dict(depth=0), dict(depth=11), dict(rounds=-1), dict(patience=0),
                dict(alpha=-1.0), dict(beta=float("nan")), dict(seeds=[1, 2])):
        with pytest.raises(ValueError):
            batched_kopt_search_torch(pts, starts, heat=heat, edge_index=ei, device=dev, **bad)
    with pytest.raises(ValueError):
        batched_kopt_search_grouped(pts[None], starts, heat=[heat, heat], edge_index=[ei, ei], device=dev)
    with pytest.raises(_lib.DifuscoHipError):
        batched_kopt_search_torch(pts, starts, heat=heat, edge_index=ei, device="cpu")


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
def _model(dev, seed, sparse_factor=-1):
    from difusco_amd import TSPModel
    from difusco_amd.synthetic import random_state_dict
    return TSPModel(_model_args(sparse_factor=sparse_factor, hidden_dim=64, n_layers=2), random_state_dict(64, 2, 2, seed=0), device=dev,
                    seed=seed)


def test_kopt_rounds_zero_is_the_call_without_the_option(dev, tmp_path):
    import json
    from difusco_amd import evaluate as EV
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    pts = np.random.default_rng(12).random((2, 50, 2))
    kw = dict(parallel_sampling=2, sequential_sampling=2, two_opt_iterations=100, local_search="multi2opt+oropt", local_search_kicks=3,
              local_search_kick_size=4, local_search_kick_span=16)
    gen = lambda b: torch.Generator().manual_seed(b)
    dump = lambda r: json.dumps(r, sort_keys=False)
    for more in ({}, dict(kopt_samples=7, kopt_depth=3)):
        assert dump(solve_tsp(_model(dev, 5), pts[0], -1, generator=gen(0), kopt_rounds=0, **more, **kw)) == \
            dump(solve_tsp(_model(dev, 5), pts[0], -1, generator=gen(0), **kw))
        assert dump(solve_tsp_batch(_model(dev, 0), pts, -1, seeds=[5, 6], generators=[gen(0), gen(1)], kopt_rounds=0, **more, **kw)) == \
            dump(solve_tsp_batch(_model(dev, 0), pts, -1, seeds=[5, 6], generators=[gen(0), gen(1)], **kw))
        mixed = [pts[0], pts[1][:40]]
        assert dump(solve_tsp_batch(_model(dev, 0), mixed, -1, seeds=[5, 6], generators=[gen(0), gen(1)], kopt_rounds=0, **more, **kw)) == \
            dump(solve_tsp_batch(_model(dev, 0), mixed, -1, seeds=[5, 6], generators=[gen(0), gen(1)], **kw))
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 2, seed=1)
    ckpt, _ = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples", "2")
    (args, _), (off, _) = EV.parse_args(argv), EV.parse_args(argv + ["--tsp_kopt_rounds", "0"])
    assert vars(args) == vars(off) and args.tsp_kopt_rounds == 0 and args.tsp_kopt_samples == 1024 and args.tsp_kopt_depth == 10
    lines, recs = EV.run(argv)
    lines0, recs0 = EV.run(argv + ["--tsp_kopt_rounds", "0", "--tsp_kopt_samples", "9"])
    timing = ("wall_s", "instances_per_s", "stages_s")
    assert dump(recs) == dump(recs0)
    assert dump([{k: v for k, v in l.items() if k not in timing} for l in lines]) == \
        dump([{k: v for k, v in l.items() if k not in timing} for l in lines0])
    for bad in (["--tsp_kopt_rounds", "-1"], ["--tsp_kopt_samples", "0"], ["--tsp_kopt_depth", "11"]):
        with pytest.raises(SystemExit):
            EV.parse_args(argv + bad)


@pytest.mark.parametrize("sparse_factor", [-1, 8])
def test_the_stage_through_the_pipeline(dev, sparse_factor):
    """With the stage on an instance gets what its solo call gets, alone, in a batch and in a mixed batch; no tour is longer than
    without the stage, and the stage moves some: the local search is capped at two sweeps, so it leaves work."""
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    pts = np.random.default_rng(13).random((2, 50, 2))
    mixed = [pts[0], pts[1][:40]]
    kw = dict(parallel_sampling=2, sequential_sampling=2, two_opt_iterations=2, local_search="multi2opt+oropt")
    on = dict(kw, kopt_rounds=6, kopt_samples=64, kopt_depth=6)
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(2)]
    res = solve_tsp_batch(_model(dev, 0, sparse_factor), pts, sparse_factor, seeds=[5, 6], generators=gens(), **on)
    mix = solve_tsp_batch(_model(dev, 0, sparse_factor), mixed, sparse_factor, seeds=[5, 6], generators=gens(), **on)
    off = solve_tsp_batch(_model(dev, 0, sparse_factor), pts, sparse_factor, seeds=[5, 6], generators=gens(), **kw)
    for b in range(2):
        one = solve_tsp(_model(dev, 5 + b, sparse_factor), mixed[b], sparse_factor, generator=torch.Generator().manual_seed(b), **on)
        assert mix[b] == one, b
        info = one[3]
        assert (info["kopt_rounds"], info["kopt_samples"], info["kopt_depth"]) == (6, 64, 6)
        assert len(info["kopt_actions"]) == len(info["kopt_rounds_run"]) == 2 and max(info["kopt_rounds_run"]) <= 6
        assert sorted(one[0][:-1]) == list(range(len(mixed[b]))) and one[0][0] == one[0][-1] == 0
    assert res[0] == mix[0]
    for r, o in zip(res, off):
        assert "kopt_actions" not in o[3] and r[3]["merged_costs"] == o[3]["merged_costs"]
        assert all(a <= c + 1e-12 for a, c in zip(r[2], o[2]))   # per copy: the stage returns no longer tour than it got
    assert sum(sum(r[3]["kopt_actions"]) for r in res) > 0
