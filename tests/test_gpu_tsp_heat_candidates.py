"""The heat-ranked candidate lists on the GPU (``difusco_tsp_heat_candidates_ragged``): ``neighbors_out``, ``listed`` and ``pads``
equal the numpy restatement of the rule (tests/tsp_heat_candidates_emulation.py) bit for bit over the groups of
tests/tsp_heat_candidates_cases.py - a group of 3, complete and dense graphs with K = n - 1, k-NN graphs, hub cities whose gathered
entries pass a wave, two waves and a block of 1024 threads, empty rows, a city nobody names, duplicate and self edges, heat
outside [0, 1] and NaN, saturated ties, K = 1 and K = 128 -, in a ragged call against the solo calls, twice in a row, with the
entries and tours permuted; then through the neighbour-list searches, ``solve_tsp`` / ``solve_tsp_batch`` and the evaluation runner
against the same searches on the emulated lists; under chosen workspace contents and behind memory fences; and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import memory_fence as MF
import tsp_heat_candidates_cases as C
import tsp_heat_candidates_emulation as E
import workspace_poison as WP
from test_gpu_evaluate import _argv, _ckpt, _model_args, _write_tsp

pytestmark = pytest.mark.gpu
RAGGED = ("n3", "knn37-P4", "hub200", "dense14")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def solo(dev, group, K, stats=None):
    from difusco_amd.decode import tsp_heat_candidate_lists
    pts, rp, col, heat = group
    return tsp_heat_candidate_lists(pts, heat, C.edge_index_of(rp, col), K, device=dev, stats=stats)


def ragged(dev, groups, K, stats=None):
    from difusco_amd.decode import tsp_heat_candidate_lists
    return tsp_heat_candidate_lists([g[0] for g in groups], [g[3] for g in groups], [C.edge_index_of(g[1], g[2]) for g in groups], K,
                                    device=dev, stats=stats)


def same(got, stats, want, g=None):
    lists, listed, pads = want
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.device.type == "cuda" and tuple(got.shape) == lists.shape
    assert np.array_equal(got.cpu().numpy(), lists)
    pick = (lambda v: int(v)) if g is None else (lambda v: int(v[g]))
    assert (pick(stats["listed"]), pick(stats["pads"])) == (listed, pads)


@pytest.mark.parametrize("name,K", C.PAIRS)
def test_solo_call_equals_emulation(dev, name, K):
    st = {}
    same(solo(dev, C.case(name), K, st), st, C.expected(name, K))
    assert set(st) == {"listed", "pads"} and isinstance(st["listed"], int)


@pytest.mark.parametrize("name,K", [("dense14", 13), ("complete5", 4), ("saturated", 9)])
def test_dense_heat(dev, name, K):
    """[P, N, N] with no edge_index: the complete graph, entry (i, j) at i N + j - as numpy and as a device tensor."""
    from difusco_amd.decode import tsp_heat_candidate_lists
    pts, _, _, heat = C.case(name)
    n = len(pts)
    for h in (heat.reshape(-1, n, n), torch.from_numpy(heat.reshape(-1, n, n)).to(dev)):
        st = {}
        same(tsp_heat_candidate_lists(pts, h, None, K, device=dev, stats=st), st, C.expected(name, K))


def test_ragged_call_equals_solo_calls_and_repeats(dev):
    groups = [C.case(name) for name in RAGGED]
    K = 5
    st = {}
    first = ragged(dev, groups, K, st)
    assert st["listed"].dtype == np.int64 and st["pads"].dtype == np.int64 and len(first) == len(RAGGED)
    for g, name in enumerate(RAGGED):
        same(first[g], st, C.expected(name, K), g)
        one = {}
        alone = solo(dev, groups[g], K, one)
        assert torch.equal(alone, first[g]) and (one["listed"], one["pads"]) == (int(st["listed"][g]), int(st["pads"][g]))
    again_st = {}
    again = ragged(dev, groups, K, again_st)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert np.array_equal(st["listed"], again_st["listed"]) and np.array_equal(st["pads"], again_st["pads"])
    # the order of the groups does not matter to a group either
    back = ragged(dev, groups[::-1], K)
    assert all(torch.equal(a, b) for a, b in zip(first, back[::-1]))


@pytest.mark.parametrize("name,K", [("knn37-P4", 5), ("duplicates", 6), ("corners", 5), ("hub200", 8), ("dense14", 13), ("saturated", 9)])
def test_entry_and_tour_order_do_not_matter(dev, name, K):
    st = {}
    same(solo(dev, C.permuted(name, seed=5), K, st), st, C.expected(name, K))


# ---- under chosen workspace contents and behind fences ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", WP.FILLS)
def test_results_do_not_depend_on_the_workspace(dev, monkeypatch, how):
    arena = WP.Arena(dev, 8 << 20)
    WP.patch_decode(monkeypatch, arena)
    arena.set("random")
    solo(dev, C.case("hub1100"), 5)                              # the residue donor: a different, larger case
    arena.set(how, whole=how != "residue")
    for name, K in (("hub200", 8), ("duplicates", 6), ("empty-rows", 4), ("n3", 5)):
        st = {}
        same(solo(dev, C.case(name), K, st), st, C.expected(name, K))
    st = {}
    got = ragged(dev, [C.case(name) for name in RAGGED], 5, st)
    for g, name in enumerate(RAGGED):
        same(got[g], st, C.expected(name, 5), g)
    arena.check_used(calls=5)


def test_writes_only_its_lists_and_declared_workspace(dev, monkeypatch):
    from difusco_amd import _lib, decode
    fence = MF.Fence(dev)
    made = MF.fence_allocations(monkeypatch, fence)
    uploads = MF.fence_uploads(monkeypatch, fence)
    handed, plain_ptr = [], decode._ptr

    def _ptr(t):
        handed.append((t, MF.snapshot(t)))
        return plain_ptr(t)
    monkeypatch.setattr(decode, "_ptr", _ptr)
    declared, plain_workspace = [], decode._workspace

    def _workspace(size_fn, *sizes, device):
        ws, nbytes = plain_workspace(size_fn, *sizes, device=device)
        declared.append((size_fn.__name__, ws, nbytes))
        return ws, nbytes
    monkeypatch.setattr(decode, "_workspace", _workspace)
    runs = [lambda st: [solo(dev, C.case("hub1100"), 5, st)], lambda st: [solo(dev, C.case("n3"), 5, st)],
            lambda st: [solo(dev, C.case("hub200"), 128, st)], lambda st: ragged(dev, [C.case(name) for name in RAGGED], 5, st)]
    wants = [[("hub1100", 5)], [("n3", 5)], [("hub200", 128)], [(name, 5) for name in RAGGED]]
    for run, want in zip(runs, wants):
        del handed[:], declared[:]
        st = {}
        got = run(st)
        fence.check(str(want))
        for g, (name, K) in enumerate(want):
            same(got[g], st, C.expected(name, K), g if len(want) > 1 else None)
        ((fn, ws, nbytes),) = declared
        assert fn == "difusco_tsp_heat_candidates_ragged_workspace_bytes" and fence.buffer_of(ws).nbytes == nbytes == ws.numel() > 0
        assert len(handed) == 6                                  # points, row_ptr, col, heat, neighbors_out, workspace
        const = 0
        for t, snap in handed:
            if any(t is m for m in made):                        # the two allocations of the call: its output and its scratch
                continue
            assert MF.unchanged(t, snap), f"{want}: a const argument ({t.dtype} {list(t.shape)}) was changed by the call"
            const += 1
        assert const == 4
    assert uploads and all(bool(torch.equal(MF._bytes_of(rec.tensor).cpu(), rec.host)) for rec in uploads)


def test_error_returns_leave_the_lists_alone(dev):
    from difusco_amd import _lib
    L = _lib.lib()
    pts, rp, col, heat = C.case("knn37-P4")
    n, P, E_, K = len(pts), len(heat), len(col), 5
    d_pts = torch.from_numpy(pts.reshape(-1)).to(dev)
    d_rp, d_col, d_heat = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rp, col, heat.reshape(-1)))
    marker = torch.full((n * K,), -7, dtype=torch.int32, device=dev)
    group_n, group_tours, group_edges = (np.array([v], dtype=np.int32) for v in (n, P, E_))
    nbytes = ctypes.c_size_t()
    size = lambda k, edges=group_edges.ctypes.data: L.difusco_tsp_heat_candidates_ragged_workspace_bytes(
        1, group_n.ctypes.data, group_tours.ctypes.data, edges, k, ctypes.byref(nbytes))
    assert size(0) == -1 and size(129) == -1 and size(K, None) == -1 and size(K) == 0 and nbytes.value > 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    listed, pads = np.zeros(1, np.int64), np.zeros(1, np.int64)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(**over):
        a = dict(K=K, out=vp(marker), ws=nbytes.value, rp=vp(d_rp), col=vp(d_col), heat=vp(d_heat), pts=vp(d_pts),
                 listed=listed.ctypes.data, edges=group_edges.ctypes.data, n=group_n.ctypes.data)
        a.update(over)
        return L.difusco_tsp_heat_candidates_ragged(1, a["n"], group_tours.ctypes.data, a["edges"], a["pts"], a["rp"], a["col"],
                                                    a["heat"], a["K"], a["out"], vp(ws), a["ws"], a["listed"], pads.ctypes.data, None)
    short_rp = rp.copy()
    short_rp[n] = E_ - 1                                         # row_ptr does not end at E
    bad_col = col.copy()
    bad_col[3] = n
    tensors = [torch.from_numpy(x).to(dev) for x in (short_rp, bad_col)]
    negative, zero_n = np.array([-1], dtype=np.int32), np.array([0], dtype=np.int32)
    refused = [dict(K=0), dict(K=129), dict(K=-1), dict(out=None), dict(ws=nbytes.value - 1), dict(rp=None), dict(col=None),
               dict(heat=None), dict(pts=None), dict(listed=None), dict(edges=None), dict(edges=negative.ctypes.data),
               dict(n=zero_n.ctypes.data), dict(rp=vp(tensors[0])), dict(col=vp(tensors[1]))]
    for over in refused:
        assert call(**over) == -1, over
        torch.cuda.synchronize(dev)
        assert bool((marker == -7).all()), over
    assert b"CSR" in L.difusco_last_error()
    assert call() == 0
    torch.cuda.synchronize(dev)
    want = C.expected("knn37-P4", K)
    assert np.array_equal(marker.cpu().numpy().reshape(n, K), want[0]) and (int(listed[0]), int(pads[0])) == want[1:]
    # the Python layer, before any library call
    from difusco_amd.decode import tsp_heat_candidate_lists
    ei = C.edge_index_of(rp, col)
    out_of_range = ei.copy()
    out_of_range[1, 3] = n
    with pytest.raises(ValueError, match="outside"):
        tsp_heat_candidate_lists(pts, heat, out_of_range, K, device=dev)
    for k in (0, 129, 2.0):
        with pytest.raises(ValueError):
            tsp_heat_candidate_lists(pts, heat, ei, k, device=dev)
    with pytest.raises(ValueError):
        tsp_heat_candidate_lists(pts, heat[:, :-1], ei, K, device=dev)


# ---- the searches on the lists -------------------------------------------------------------------------------------------------
def test_complete_lists_give_the_full_search(dev):
    """Dense n = 14, K = 13: every list names every other city, in an order the heat decides - the neighbour-list search is the
    multi-move local search, whatever the heat."""
    from difusco_amd.decode import batched_multi_local_search_torch, batched_nbr_local_search_torch, tsp_heat_candidate_lists
    pts, _, _, heat = C.case("dense14")
    n = len(pts)
    rng = np.random.default_rng(1400)
    starts = np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(3)])
    want = batched_multi_local_search_torch(pts, starts, device=dev)
    for h in (heat, np.zeros_like(heat), np.ones_like(heat), rng.random(heat.shape).astype(np.float32)):
        lists = tsp_heat_candidate_lists(pts, h.reshape(-1, n, n), None, n - 1, device=dev)
        assert all(sorted(row) == [b for b in range(n) if b != a] for a, row in enumerate(lists.cpu().tolist()))
        for closing in (True, False):
            got = batched_nbr_local_search_torch(pts, starts, device=dev, neighbors=lists, closing=closing)
            assert np.array_equal(got[0], want[0]) and {k: got[1][k] for k in want[1]} == want[1] and got[1]["full_sweeps"] == 0


SF, HIDDEN, LAYERS, K5 = 8, 64, 2, 5


def _model(dev, sd, seed, sparse_factor=SF):
    from difusco_amd import TSPModel
    return TSPModel(_model_args(sparse_factor=sparse_factor, hidden_dim=HIDDEN, n_layers=LAYERS), sd, device=dev, seed=seed)


def _by_emulation(dev, sd, seed, pts64, sparse_factor, P, gen, local_search, closing=True):
    """What ``solve_tsp`` must return with the heat lists: the stages of one round by hand - graph, sampling, merge - then the
    neighbour-list search of ``local_search`` on the EMULATED lists of that heat.  -> (tour, cost, costs, the search's counters)."""
    from difusco_amd.decode import batched_nbr_local_search_torch, batched_nbr_two_opt_torch, merge_tours
    from difusco_amd.graph import knn_edge_index_gpu
    from difusco_amd.pipeline import tour_length
    model = _model(dev, sd, seed, sparse_factor)
    n = len(pts64)
    sparse = sparse_factor > 0
    pts32 = torch.from_numpy(pts64.astype(np.float32)).to(dev)
    pts = pts32.cpu().numpy().astype(np.float64)
    if sparse:
        ei = knn_edge_index_gpu(pts64, sparse_factor, device=dev)
        heat = model.sample(pts32.repeat(P, 1), model.duplicate_edge_index(ei, n, dev, copies=P) if P > 1 else ei, generator=gen)
        rp, col = E.csr(n, ei[0].cpu().numpy(), ei[1].cpu().numpy())
    else:
        ei = None
        heat = model.sample(pts32.reshape(1, n, 2).repeat(P, 1, 1), None, generator=gen)
        rp, col = np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n)
    tours, _ = merge_tours(heat, pts32, ei, sparse_graph=sparse, parallel_sampling=P, device=dev)
    lists, listed, _ = E.lists(pts, rp, col, heat.cpu().numpy().reshape(P, -1), K5)
    tours = np.asarray(tours, dtype=np.int64)
    if local_search == "nbr2opt+oropt":
        solved, st = batched_nbr_local_search_torch(pts, tours, 100, device=dev, neighbors=lists, closing=closing)
        counters = dict(two_opt_iterations=st["two_opt_sweeps"], two_opt_moves=st["two_opt_moves"], or_opt_iterations=st["or_opt_sweeps"],
                        or_opt_moves=st["or_opt_moves"], local_search_rounds=st["rounds"], local_search_full_sweeps=st["full_sweeps"],
                        local_search_full_rounds=st["full_rounds"])
    else:
        st = {}
        solved, sweeps = batched_nbr_two_opt_torch(pts, tours, 100, device=dev, neighbors=lists, closing=closing, stats=st)
        counters = dict(two_opt_iterations=sweeps, two_opt_moves=st["moves"], two_opt_full_sweeps=st["full_sweeps"])
    costs = [tour_length(pts, t) for t in solved]
    best = int(np.argmin(costs))
    counters.update(local_search_candidates=K5, local_search_closing=closing, local_search_candidate_source="heat",
                    local_search_heat_listed=listed / (n * K5))
    return solved[best].tolist(), costs[best], costs, {k: (v if isinstance(v, (bool, str, float)) else int(v)) for k, v in counters.items()}


def _matches(result, want):
    tour, cost, costs, info = result
    assert (tour, cost, costs) == want[:3]
    assert {k: info[k] for k in want[3]} == want[3]
    assert sorted(tour[:-1]) == list(range(len(tour) - 1)) and tour[0] == tour[-1] == 0


@pytest.fixture(scope="module")
def weights():
    from difusco_amd.synthetic import random_state_dict
    return random_state_dict(HIDDEN, LAYERS, 2, seed=0)


@pytest.mark.parametrize("local_search", ["nbr2opt+oropt", "multi2opt"])
@pytest.mark.parametrize("sparse_factor", [SF, -1])
def test_solve_tsp_runs_the_search_on_the_emulated_lists(dev, weights, local_search, sparse_factor):
    from difusco_amd.pipeline import solve_tsp
    pts = np.random.default_rng(37).random((37, 2))
    kw = dict(parallel_sampling=2, two_opt_iterations=100, local_search=local_search, local_search_candidates=K5)
    got = solve_tsp(_model(dev, weights, 3, sparse_factor), pts, sparse_factor, generator=torch.Generator().manual_seed(1),
                    local_search_candidate_source="heat", **kw)
    _matches(got, _by_emulation(dev, weights, 3, pts, sparse_factor, 2, torch.Generator().manual_seed(1), local_search))
    assert 0.0 <= got[3]["local_search_heat_listed"] <= 1.0
    # the default source: the keyword spelled out changes nothing
    plain = solve_tsp(_model(dev, weights, 3, sparse_factor), pts, sparse_factor, generator=torch.Generator().manual_seed(1), **kw)
    spelled = solve_tsp(_model(dev, weights, 3, sparse_factor), pts, sparse_factor, generator=torch.Generator().manual_seed(1),
                        local_search_candidate_source="knn", **kw)
    assert plain == spelled and "local_search_candidate_source" not in plain[3] and "local_search_heat_listed" not in plain[3]
    assert plain[3]["merged_costs"] == got[3]["merged_costs"]                   # the same decoded tours went in


def test_sequential_rounds_build_their_own_lists(dev, weights):
    """Two rounds: the second samples on, so the emulation of its round needs its heat - checked through the batch, which must
    equal the solo call, and through ``local_search_heat_listed`` of the LAST round differing from a one-round call's."""
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    pts = np.random.default_rng(38).random((37, 2))
    kw = dict(parallel_sampling=2, two_opt_iterations=100, local_search="nbr2opt+oropt", local_search_candidates=K5,
              local_search_candidate_source="heat", local_search_closing=False)
    two = solve_tsp(_model(dev, weights, 4), pts, SF, generator=torch.Generator().manual_seed(2), sequential_sampling=2, **kw)
    one = solve_tsp(_model(dev, weights, 4), pts, SF, generator=torch.Generator().manual_seed(2), **kw)
    assert len(two[2]) == 4 and two[2][:2] == one[2] and two[3]["local_search_closing"] is False
    batch = solve_tsp_batch(_model(dev, weights, 0), pts[None], SF, seeds=[4], generators=[torch.Generator().manual_seed(2)],
                            sequential_sampling=2, **kw)
    assert batch[0] == two


@pytest.mark.parametrize("local_search", ["nbr2opt+oropt", "multi2opt"])
def test_ragged_solve_tsp_batch(dev, weights, local_search):
    from difusco_amd.pipeline import solve_tsp_batch
    rng = np.random.default_rng(39)
    mixed = [rng.random((37, 2)), rng.random((30, 2)), rng.random((37, 2))]
    seeds = [11, 12, 13]
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(3)]
    kw = dict(parallel_sampling=2, two_opt_iterations=100, local_search=local_search, local_search_candidates=K5)
    for sparse_factor, merge in ((SF, "loop"), (-1, "batched")):
        got = solve_tsp_batch(_model(dev, weights, 0, sparse_factor), mixed, sparse_factor, seeds=seeds, generators=gens(),
                              merge_method=merge, local_search_candidate_source="heat", **kw)
        for b in range(3):
            _matches(got[b], _by_emulation(dev, weights, seeds[b], mixed[b], sparse_factor, 2, torch.Generator().manual_seed(b),
                                           local_search))
    same_size = [mixed[0], mixed[2]]
    got = solve_tsp_batch(_model(dev, weights, 0), np.stack(same_size), SF, seeds=seeds[:2], generators=gens()[:2],
                          local_search_candidate_source="heat", **kw)
    for b in range(2):
        _matches(got[b], _by_emulation(dev, weights, seeds[b], same_size[b], SF, 2, torch.Generator().manual_seed(b), local_search))
    plain = solve_tsp_batch(_model(dev, weights, 0), mixed, SF, seeds=seeds, generators=gens(), **kw)
    spelled = solve_tsp_batch(_model(dev, weights, 0), mixed, SF, seeds=seeds, generators=gens(), local_search_candidate_source="knn", **kw)
    assert plain == spelled and all("local_search_candidate_source" not in r[3] for r in plain)


def test_evaluate_with_the_flag(dev, tmp_path):
    from difusco_amd import evaluate as EV
    from difusco_amd.datasets import read_tsp_split
    split = _write_tsp(tmp_path / "tsp.txt", [37] * 3, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", HIDDEN, LAYERS)
    argv = _argv(tmp_path, "tsp", split, ckpt, HIDDEN, LAYERS, "--two_opt_iterations", "100", "--do_valid_only", "--validation_examples",
                 "3", "--local_search", "nbr2opt+oropt", "--tsp_local_search_candidates", str(K5))
    lines, recs = EV.run(argv + ["--tsp_local_search_candidate_source", "heat"])
    plain_lines, plain = EV.run(argv)
    again_lines, again = EV.run(argv + ["--tsp_local_search_candidate_source", "knn"])
    assert again == plain and "tsp_local_search_candidate_source" not in plain_lines[0] and "tsp_local_search_candidate_source" not in again_lines[0]
    assert lines[0]["tsp_local_search_candidate_source"] == "heat"
    examples = read_tsp_split(split)
    for r, p in zip(recs, plain):
        assert set(r) == set(p) | {"tsp_local_search_candidate_source", "heat_listed"} and r["merged_costs"] == p["merged_costs"]
        want = _by_emulation(dev, sd, r["seed"], examples[r["index"]].points, -1, 1, torch.Generator().manual_seed(r["seed"]),
                             "nbr2opt+oropt")
        assert (r["tour"], r["solved_cost"], r["all_costs"]) == want[:3]
        assert r["heat_listed"] == want[3]["local_search_heat_listed"] and r["2opt_iterations"] == want[3]["two_opt_iterations"]
        for k in ("two_opt_moves", "or_opt_iterations", "or_opt_moves", "local_search_rounds", "local_search_full_sweeps",
                  "local_search_full_rounds"):
            assert r[k] == want[3][k], k
