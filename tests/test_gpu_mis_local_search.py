"""The MIS swap local search on the GPU (``difusco_mis_local_search``): the set and the three counters equal the numpy restatement
of the rule (tests/mis_local_search_emulation.py, pinned by tests/test_mis_local_search_host.py) bit for bit - on the hand cases,
the decode fixtures (n = 750: degrees above 64, several rounds with conflicts), from maximal, empty and non-maximal start sets,
capped, on a star that needs the lane stride, with isolated nodes and self loops, on one node, in a union of graphs next to a
component that is done in round 0; a dependent input is refused with the device array unchanged, duplicate entries never give a
dependent set; then through ``solve_mis`` / ``solve_mis_batch`` and the evaluation runner."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mis_local_search_emulation as M
from test_gpu_evaluate import _argv, _ckpt, _write_mis
from test_mis_local_search_host import FIXTURES, GNP, HAND, fixture, gnp, sym

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _same(dev, n, ei, scores, start, cap=None):
    """One GPU call against the emulation at the same cap: the set and (rounds, swaps, inserts)."""
    from difusco_amd.decode import mis_local_search_np
    want = M.local_search(n, ei, scores, start, cap)
    stats = {}
    got = mis_local_search_np(scores, start, edge_index=ei, device=dev, stats=stats, **({} if cap is None else {"max_rounds": cap}))
    assert got.shape == (n,) and got.dtype == int
    assert np.array_equal(got, want[0])
    assert (stats["rounds"], stats["swaps"], stats["inserts"]) == tuple(want[1:])
    return got


def _thinned(sol):
    out = np.array(sol).copy()
    out[np.flatnonzero(out)[::2]] = 0                        # every second chosen node dropped: independent, not maximal
    return out


@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases_equal_emulation(dev, name):
    n, pairs, scores, (want, rounds, swaps, inserts) = HAND[name]
    got = _same(dev, n, sym(n, pairs), np.array(scores, dtype=np.float32), np.zeros(n, dtype=int))
    assert got.tolist() == want


@pytest.mark.parametrize("start", ["decoded", "empty", "thinned"])
@pytest.mark.parametrize("name", ["mis_decode_n60_p15", "mis_decode_n300_p05"])
def test_small_fixtures_equal_emulation(dev, name, start):
    ei, scores, decoded = fixture(name)
    n = len(scores)
    s = {"decoded": decoded, "empty": np.zeros(n, dtype=int), "thinned": _thinned(decoded)}[start]
    got = _same(dev, n, ei, scores, s)
    if start == "decoded":
        assert int(got.sum()) == FIXTURES[name][0][1]
    for cap in (0, 1):
        _same(dev, n, ei, scores, s, cap)


def test_n750_fixture_equals_emulation(dev):
    """84,996 entries, mean degree 112: every neighbour list takes the lane stride; three rounds with conflicts."""
    ei, scores, decoded = fixture("mis_decode_n750_p15")
    got = _same(dev, len(scores), ei, scores, decoded)
    assert int(got.sum()) == 36


def test_star_takes_the_lane_stride(dev):
    n, pairs, scores, (want, *_) = HAND["star"]
    ei, sc = sym(n, pairs, self_loops=True), np.array(scores, dtype=np.float32)
    centre = np.zeros(n, dtype=int)
    centre[0] = 1                                            # the decode's answer: 70 candidates of one owner, none adjacent
    assert _same(dev, n, ei, sc, centre).tolist() == want
    _same(dev, n, ei, sc, centre, 0)


def test_isolated_nodes_self_loops_and_one_node(dev):
    n = 12
    ei = sym(n, [(0, 1), (1, 2), (4, 5), (5, 6), (5, 7)], self_loops=True)      # 3, 8, 9, 10, 11 are isolated
    sc = np.random.default_rng(5).random(n).astype(np.float32)
    got = _same(dev, n, ei, sc, np.zeros(n, dtype=int))
    assert got[[3, 8, 9, 10, 11]].tolist() == [1] * 5
    _same(dev, n, ei[:, : -n], sc, np.zeros(n, dtype=int))   # the same graph without the self loops: empty rows
    for loops in (np.zeros((2, 0), dtype=np.int64), np.zeros((2, 1), dtype=np.int64)):
        assert _same(dev, 1, loops, np.array([.3], dtype=np.float32), np.zeros(1, dtype=int)).tolist() == [1]
        assert _same(dev, 1, loops, np.array([.3], dtype=np.float32), np.ones(1, dtype=int)).tolist() == [1]


def test_a_graph_without_any_entry(dev):
    """No col array at all: every node ends in the set, with 0 swaps, from the empty set and from a partial one."""
    from difusco_amd.decode import mis_local_search_np
    none = np.zeros((2, 0), dtype=np.int64)
    sc = np.array([.5, 0, -0.0, 1, .5, 0, .25], dtype=np.float32)
    for start in (np.zeros(7, dtype=int), np.array([0, 1, 0, 0, 1, 0, 0])):
        stats = {}
        got = mis_local_search_np(sc, start, edge_index=none, device=dev, stats=stats)
        assert got.tolist() == [1] * 7 and stats["swaps"] == 0 and stats["inserts"] == 7 - int(start.sum())
        _same(dev, 7, none, sc, start)


def test_nan_scores_rank_last_as_in_the_decode(dev):
    """The rank is the decode's: NaN of either sign after everything else, the two zeros one value (tests/mis_decode_cases.py)."""
    import mis_decode_cases as Z
    for structure, kind in (("sparse_257", "with_nan"), ("union_40", "with_nan"), ("sparse_255", "mixed_zero_signs")):
        c = Z.case(structure, kind)
        got = _same(dev, c["n"], c["edge_index"], c["scores"], np.zeros(c["n"], dtype=int), 0)      # the insertion phase alone
        assert np.array_equal(got, c["want"])                # from the empty set that is the greedy decode
        _same(dev, c["n"], c["edge_index"], c["scores"], c["want"])


@pytest.mark.parametrize("cap", [None, 1, 2])
def test_union_equals_solo_calls(dev, cap):
    from difusco_amd.decode import mis_local_search_np
    n4, pairs4, scores4, _ = HAND["k4"]                      # done in round 0
    graphs = [gnp(n, p, seed=n) for n, p in GNP] + [(sym(n4, pairs4), np.array(scores4, dtype=np.float32))]
    ns = [n for n, _ in GNP] + [n4]
    off = np.concatenate([[0], np.cumsum(ns)])
    union = np.concatenate([ei + off[g] for g, (ei, _) in enumerate(graphs)], axis=1)
    scores = np.concatenate([s for _, s in graphs])
    kw = {} if cap is None else {"max_rounds": cap}
    sol = _same(dev, int(off[-1]), union, scores, np.zeros(int(off[-1]), dtype=int), cap)
    for g, n in enumerate(ns):
        solo = mis_local_search_np(graphs[g][1], np.zeros(n, dtype=int), edge_index=graphs[g][0], device=dev, **kw)
        assert np.array_equal(sol[off[g]:off[g + 1]], solo), g


def test_a_dependent_input_is_refused_and_left_alone(dev):
    from difusco_amd import _lib
    from difusco_amd.decode import mis_local_search_np
    from difusco_amd.graph import build_csr
    ei, scores, decoded = fixture("mis_decode_n60_p15")
    n = len(scores)
    a, b = next((int(p), int(q)) for p, q in ei.T if p != q)
    bad = np.zeros(n, dtype=np.int32)
    bad[[a, b]] = 1
    with pytest.raises(_lib.DifuscoHipError, match="not independent"):
        mis_local_search_np(scores, bad, edge_index=ei, device=dev)
    # the library call itself: the device array is what went in
    L = _lib.lib()
    g = build_csr(torch.from_numpy(ei), n, dev)
    d_sol, d_sc = torch.from_numpy(bad).to(dev), torch.from_numpy(scores).to(dev)
    nbytes = ctypes.c_size_t()
    _lib.check(L.difusco_mis_local_search_workspace_bytes(n, int(g.col.shape[0]), ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counters = (ctypes.c_int32 * 3)()
    args = [n, ctypes.c_void_p(g.rowptr.data_ptr()), ctypes.c_void_p(g.col.data_ptr()), ctypes.c_void_p(d_sc.data_ptr()),
            ctypes.c_void_p(d_sol.data_ptr()), 1000, ctypes.c_void_p(ws.data_ptr()), nbytes.value, counters,
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)]
    assert L.difusco_mis_local_search(*args) == -1 and b"not independent" in L.difusco_last_error()      # DIFUSCO_EINVAL
    assert np.array_equal(d_sol.cpu().numpy(), bad)
    for i, v in ((5, -1), (0, 0), (1, None), (8, None)):     # max_rounds < 0, n_nodes < 1, a null array, null counters
        broken = list(args)
        broken[i] = v
        assert L.difusco_mis_local_search(*broken) == -1
    assert np.array_equal(d_sol.cpu().numpy(), bad)
    assert L.difusco_mis_local_search_workspace_bytes(0, 0, ctypes.byref(nbytes)) == -1


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
def _mis_model(dev, golden_dir, seed):
    from difusco_amd import MISModel
    z = np.load(os.path.join(golden_dir, "weights_h64_l2.npz"))
    w = {k: torch.from_numpy(z[k]) for k in z.files if k != "provenance" and not k.startswith("gaussian_")}
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=-1, n_layers=2,
                hidden_dim=64, inference_trick="ddim", inference_diffusion_steps=5, inference_schedule="cosine")
    return MISModel(args, w, device=dev, seed=seed)


def test_solve_mis_and_batch_with_the_swap_search(dev, golden_dir):
    from difusco_amd.pipeline import solve_mis, solve_mis_batch
    from difusco_amd.synthetic import er_mis_edge_index
    inst = [(n, er_mis_edge_index(n, 0.1, seed=40 + i)) for i, n in enumerate((60, 57))]
    seeds, P, S = [51, 52], 3, 2
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(2)]
    kw = dict(parallel_sampling=P, sequential_sampling=S)
    bstats = []
    res = solve_mis_batch(_mis_model(dev, golden_dir, 0), inst, seeds=seeds, generators=gens(), local_search="swap", stats=bstats, **kw)
    none = solve_mis_batch(_mis_model(dev, golden_dir, 0), inst, seeds=seeds, generators=gens(), local_search="none", **kw)
    plain = solve_mis_batch(_mis_model(dev, golden_dir, 0), inst, seeds=seeds, generators=gens(), **kw)
    assert len(bstats) == 2 and all(bstats[0][k] == bstats[1][k] for k in ("rounds", "swaps", "inserts"))
    for b, (n, ei) in enumerate(inst):
        adj = M.adjacency(n, ei)
        stats = {}
        sol, size, sizes = solve_mis(_mis_model(dev, golden_dir, seeds[b]), n, ei, generator=torch.Generator().manual_seed(b),
                                     local_search="swap", stats=stats, **kw)
        base = solve_mis(_mis_model(dev, golden_dir, seeds[b]), n, ei, generator=torch.Generator().manual_seed(b), **kw)
        assert np.array_equal(res[b][0], sol) and res[b][1] == size and res[b][2] == sizes, b      # the solo answer
        assert stats["decoded_sizes"] == bstats[b]["decoded_sizes"] == base[2] and len(sizes) == P * S
        assert all(s >= d for s, d in zip(sizes, stats["decoded_sizes"])) and size == max(sizes)
        assert M.is_independent(adj, sol) and M.is_maximal(adj, sol) and int(sol.sum()) == size
        for r, p in ((none[b], plain[b]), (base, plain[b])):                                       # "none" is today's path
            assert np.array_equal(r[0], p[0]) and r[1:] == p[1:]
    assert sum(bstats[0][k] for k in ("swaps", "inserts")) == sum(sum(r[2]) - sum(s["decoded_sizes"]) for r, s in zip(res, bstats))


def test_evaluate_with_and_without_the_flag(dev, tmp_path):
    from difusco_amd import evaluate as EV
    pattern = _write_mis(tmp_path / "mis", [60, 75], seed=3)
    ckpt, _ = _ckpt(tmp_path / "mis.ckpt", 64, 2)
    argv = _argv(tmp_path, "mis", pattern, ckpt, 64, 2, "--parallel_sampling", "2", "--do_valid_only")
    lines, recs = EV.run(argv + ["--mis_local_search", "swap"])
    plain_lines, plain = EV.run(argv)
    keys = ["split", "index", "source", "n_nodes", "gt_cost", "solved_cost", "all_costs", "seed", "mis"]
    header = ["task", "split", "val/gt_cost", "val/solved_cost", "val/gap_pct", "non_reference_keys", "instances", "wall_s",
              "instances_per_s", "stages_s", "world_size", "precision", "instances_per_call", "chunks", "chunk_lengths", "seed",
              "two_opt_method", "graph_build", "ignored_args"]
    assert list(plain_lines[0]) == header and list(lines[0]) == header + ["mis_local_search"]
    assert lines[0]["mis_local_search"] == "swap" and len(recs) == len(plain) == 2
    assert set(plain_lines[0]["stages_s"]) == {"parse", "sampling", "decode"}
    assert set(lines[0]["stages_s"]) == {"parse", "sampling", "decode", "local_search"}
    for r, p in zip(recs, plain):
        assert list(p) == keys and list(r) == keys + ["decoded_costs"]
        assert r["decoded_costs"] == p["all_costs"] and r["solved_cost"] >= max(r["decoded_costs"])
        assert all(a >= d for a, d in zip(r["all_costs"], r["decoded_costs"]))
    assert plain == EV.run(argv + ["--mis_local_search", "none"])[1]
    # one instance per call gives the same records: the search never crosses a component
    assert recs == EV.run(argv + ["--mis_local_search", "swap", "--instances_per_call", "1"])[1]


def test_duplicate_entries_never_give_a_dependent_set(dev):
    """Duplicate neighbour-list entries may cost swaps, never independence or maximality (no equality with the emulation asked)."""
    from difusco_amd.decode import mis_local_search_np
    ei, scores, decoded = fixture("mis_decode_n300_p05")
    n = len(scores)
    rng = np.random.default_rng(9)
    for symmetric in (True, False):
        extra = ei[:, rng.choice(ei.shape[1], ei.shape[1] // 3, replace=False)]
        dup = np.concatenate([ei, extra, extra[::-1]] if symmetric else [ei, extra], axis=1)
        adj = M.adjacency(n, ei)
        for start in (decoded, np.zeros(n, dtype=int)):
            stats = {}
            sol = mis_local_search_np(scores, start, edge_index=dup, device=dev, stats=stats)
            assert M.is_independent(adj, sol) and M.is_maximal(adj, sol)
            assert int(sol.sum()) == int(start.sum()) + stats["swaps"] + stats["inserts"] >= int(decoded.sum())
