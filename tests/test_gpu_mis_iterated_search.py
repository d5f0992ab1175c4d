"""The iterated MIS swap search on the GPU (``difusco_mis_iterated_search``): the set, the three call counters and the four
per-instance counters equal the numpy restatement of the rule (tests/mis_iterated_search_emulation.py, pinned by
tests/test_mis_iterated_search_host.py) bit for bit, with the draws of the host Philox (tests/philox_reference.py) - on the hand
cases, on empty rows, isolated nodes, self loops, duplicate entries and an empty instance in the middle of the table, on the
decode fixtures from their decoded and from the empty set, capped and not, and on a union of the fixtures with two copies each,
where every table row equals its solo call.  ``kicks = 0`` is ``difusco_mis_local_search``; refused inputs leave the buffer
alone; then through ``solve_mis`` / ``solve_mis_batch`` and the evaluation runner."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mis_iterated_search_emulation as I
import mis_local_search_emulation as M
from test_gpu_evaluate import _argv, _ckpt, _write_mis
from test_gpu_mis_local_search import _mis_model
from test_mis_iterated_search_host import CASES, K4, union_of
from test_mis_local_search_host import FIXTURES, fixture, sym

pytestmark = pytest.mark.gpu

KICK_OFFSET = 1 << 62
SEEDS = {"mis_decode_n60_p15": 60, "mis_decode_n300_p05": 300, "mis_decode_n750_p15": 750}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _gpu(dev, ei, scores, start, rows, seeds, offsets, kicks, kick_size, cap):
    from difusco_amd.decode import mis_iterated_search_np
    stats = {}
    sol = mis_iterated_search_np(scores, start, edge_index=ei, device=dev, instance_rows=rows, seeds=seeds, offsets=offsets,
                                 kicks=kicks, kick_size=kick_size, stats=stats, **({} if cap is None else {"max_rounds": cap}))
    per = np.array([stats[k] for k in ("entered", "accepted", "size_before", "size_after")]).T
    return sol, (stats["rounds"], stats["swaps"], stats["inserts"]), per, stats["host_syncs"]


def _same(dev, n, ei, scores, start, *, rows=None, seeds=None, offsets=None, kicks, kick_size=4, cap=None, want=None):
    """One GPU call against the restatement: the set, (rounds, swaps, inserts) and the per-instance counters; no instance ends
    below its descent."""
    rows = [0, n] if rows is None else rows
    B = len(rows) - 1
    seeds, offsets = [0] * B if seeds is None else seeds, [0] * B if offsets is None else offsets
    if want is None:
        want = I.iterated_search(n, ei, scores, start, rows, seeds, offsets, kicks, kick_size, cap)
    sol, counters, per, syncs = _gpu(dev, ei, scores, start, rows, seeds, offsets, kicks, kick_size, cap)
    assert sol.shape == (n,) and sol.dtype == int
    assert np.array_equal(sol, want[0])
    assert counters == tuple(want[1])
    assert per.tolist() == want[2].tolist()
    assert all(after >= before for _, _, before, after in per.tolist())
    return sol, per, syncs


@pytest.mark.parametrize("name", list(CASES))
def test_hand_cases_equal_emulation(dev, name):
    n, pairs, scores, start, cap, kick_size, _ = CASES[name]
    start = np.zeros(n, dtype=int) if start is None else np.array(start)
    for kicks, seed in ((1, 5), (6, 77)):
        _same(dev, n, sym(n, pairs), np.array(scores, dtype=np.float32), start, seeds=[seed], offsets=[3], kicks=kicks,
              kick_size=kick_size, cap=cap)


def test_empty_rows_isolated_nodes_self_loops_and_one_node(dev):
    n = 12
    ei = sym(n, [(0, 1), (1, 2), (4, 5), (5, 6), (5, 7)], self_loops=True)      # 3, 8, 9, 10, 11 are isolated
    sc = np.random.default_rng(5).random(n).astype(np.float32)
    for graph in (ei, ei[:, : -n]):                          # with the self loops, and without them: empty rows
        sol, per, _ = _same(dev, n, graph, sc, np.zeros(n, dtype=int), seeds=[8], kicks=10, kick_size=2)
        assert sol[[3, 8, 9, 10, 11]].tolist() == [1] * 5
    for loops in (np.zeros((2, 0), dtype=np.int64), np.zeros((2, 1), dtype=np.int64)):
        for start in (0, 1):
            sol, per, _ = _same(dev, 1, loops, np.array([.3], dtype=np.float32), np.full(1, start), seeds=[2], kicks=3)
            assert sol.tolist() == [1] and per.tolist() == [[0, 0, 1, 1]]


def test_a_graph_without_any_entry(dev):
    """No col array at all: every node ends in the set, with 0 swaps, from the empty set and from a partial one; the kicks find
    every node in the set already."""
    none = np.zeros((2, 0), dtype=np.int64)
    sc = np.array([.5, 0, -0.0, 1, .5, 0, .25], dtype=np.float32)
    for start in (np.zeros(7, dtype=int), np.array([0, 1, 0, 0, 1, 0, 0])):
        from difusco_amd.decode import mis_iterated_search_np
        stats = {}
        mis_iterated_search_np(sc, start, edge_index=none, device=dev, seeds=[3], kicks=4, kick_size=2, stats=stats)
        assert stats["swaps"] == 0 and stats["inserts"] == 7 - int(start.sum())
        sol, per, _ = _same(dev, 7, none, sc, start, seeds=[3], kicks=4, kick_size=2)
        assert sol.tolist() == [1] * 7 and per[0, 2:].tolist() == [7, 7]


def test_duplicate_neighbour_entries(dev):
    """Every entry twice.  The descent counts a doubled member twice (a node next to it is never a candidate), so only graphs on
    which that changes nothing can equal the restatement: in K4 the candidates of the member are pairwise adjacent either way,
    and a graph without edges has no candidates.  The kick steps themselves do not count, they only ask "is there one"."""
    ei = sym(4, K4, self_loops=True)
    _same(dev, 4, np.concatenate([ei, ei], axis=1), np.array([.9, .5, .4, .3], dtype=np.float32), np.zeros(4, dtype=int),
          seeds=[4], kicks=6, kick_size=1)
    loops = sym(5, [], self_loops=True)
    _same(dev, 5, np.concatenate([loops, loops], axis=1), np.arange(5, dtype=np.float32), np.zeros(5, dtype=int), seeds=[4], kicks=2)


def test_an_empty_instance_in_the_middle_of_the_table(dev):
    graphs = [(fixture(name)[0], fixture(name)[1]) for name in ("mis_decode_n60_p15", "mis_decode_n300_p05")]
    n, union, scores, rows = union_of(graphs, empty_after=0)
    assert rows == [0, 60, 60, 360]
    sol, per, _ = _same(dev, n, union, scores, np.zeros(n, dtype=int), rows=rows, seeds=[1, 2, 3], offsets=[0, 5, 2 ** 64 - 3],
                        kicks=6)                              # the third offset wraps at kick 3
    assert per[1].tolist() == [0, 0, 0, 0] and per[:, 0].min() == 0 < per[[0, 2], 0].min()


@functools.lru_cache(maxsize=None)
def _reference(name, start, kicks, kick_size, cap, seed=None, offset=0):
    """The restatement on a fixture, computed once per module run and shared."""
    ei, scores, decoded = fixture(name)
    n = len(scores)
    s = decoded if start == "decoded" else np.zeros(n, dtype=int)
    return I.iterated_search(n, ei, scores, s, None, [SEEDS[name] if seed is None else seed], [offset], kicks, kick_size, cap)


@pytest.mark.parametrize("cap", [1, 1000])
@pytest.mark.parametrize("kick_size", [1, 4])
@pytest.mark.parametrize("start", ["decoded", "empty"])
@pytest.mark.parametrize("name", ["mis_decode_n60_p15", "mis_decode_n300_p05"])
def test_small_fixtures_equal_emulation(dev, name, start, kick_size, cap):
    from difusco_amd.decode import mis_local_search_np
    ei, scores, decoded = fixture(name)
    n = len(scores)
    s = decoded if start == "decoded" else np.zeros(n, dtype=int)
    descent = mis_local_search_np(scores, s, edge_index=ei, device=dev, max_rounds=cap)
    *_, base_syncs = _same(dev, n, ei, scores, s, seeds=[SEEDS[name]], kicks=0, kick_size=kick_size, cap=cap,
                           want=_reference(name, start, 0, kick_size, cap))
    for kicks in (1, 8, 20):
        sol, per, syncs = _same(dev, n, ei, scores, s, seeds=[SEEDS[name]], kicks=kicks, kick_size=kick_size, cap=cap,
                                want=_reference(name, start, kicks, kick_size, cap))
        assert per[0, 2] == int(descent.sum()) <= per[0, 3] == int(sol.sum())
        assert syncs <= base_syncs + kicks                   # at most one more host synchronisation per kick


@pytest.mark.parametrize("start", ["decoded", "empty"])
def test_n750_fixture_equals_emulation_and_grows(dev, start):
    """84,996 entries, mean degree 112: every neighbour list takes the lane stride.  With key 750 the restatement takes the set
    from the descent's 36 nodes to 39 in 20 kicks (7 of them kept), from either start set."""
    name = "mis_decode_n750_p15"
    ei, scores, decoded = fixture(name)
    want = _reference(name, start, 20, 4, 1000)
    assert want[2].tolist() == [[20, 7, 36, 39]]
    s = decoded if start == "decoded" else np.zeros(len(scores), dtype=int)
    sol, per, syncs = _same(dev, len(scores), ei, scores, s, seeds=[750], kicks=20, kick_size=4, cap=1000, want=want)
    assert int(sol.sum()) == 39 > FIXTURES[name][0][1] == 36


def _union_call():
    names = list(SEEDS)
    graphs = [(fixture(name)[0], fixture(name)[1]) for name in names for _ in range(2)]       # P = 2 copies of every fixture
    n, union, scores, rows = union_of(graphs)
    seeds = [SEEDS[name] for name in names for _ in range(2)]
    offsets = [KICK_OFFSET + (p << 32) for _ in names for p in range(2)]
    start = np.concatenate([fixture(name)[2] for name in names for _ in range(2)])
    return names, n, union, scores, rows, seeds, offsets, start


def test_union_of_the_fixtures_equals_the_solo_calls_and_repeats(dev):
    names, n, union, scores, rows, seeds, offsets, start = _union_call()
    kicks = 8
    first = _gpu(dev, union, scores, start, rows, seeds, offsets, kicks, 4, None)
    again = _gpu(dev, union, scores, start, rows, seeds, offsets, kicks, 4, None)
    assert np.array_equal(first[0], again[0]) and first[1] == again[1] and first[2].tolist() == again[2].tolist()
    sol, counters, per, _ = first
    swaps = inserts = 0
    for b in range(len(rows) - 1):
        name, p = names[b // 2], b % 2
        ei, sc, decoded = fixture(name)
        want = _reference(name, "decoded", kicks, 4, None, seeds[b], offsets[b])
        solo, solo_per, _ = _same(dev, len(sc), ei, sc, decoded, seeds=[seeds[b]], offsets=[offsets[b]], kicks=kicks, want=want)
        assert np.array_equal(sol[rows[b]:rows[b + 1]], solo) and per[b].tolist() == solo_per[0].tolist(), b
        swaps, inserts = swaps + want[1][1], inserts + want[1][2]
    assert counters[1:] == (swaps, inserts)
    assert per[0::2].tolist() != per[1::2].tolist()          # the two copies of a fixture were kicked differently


def test_kicks_zero_is_the_local_search_bit_for_bit(dev):
    from difusco_amd import _lib
    from difusco_amd.decode import mis_local_search_np
    L = _lib.lib()
    names, n, union, scores, rows, seeds, offsets, start = _union_call()
    for s in (start, np.zeros(n, dtype=int)):
        for cap in (0, 1, 1000):
            stats = {}
            want = mis_local_search_np(scores, s, edge_index=union, device=dev, max_rounds=cap, stats=stats)
            local_syncs = int(L.difusco_mis_search_host_syncs())
            sol, counters, per, syncs = _gpu(dev, union, scores, s, rows, seeds, offsets, 0, 4, cap)
            assert np.array_equal(sol, want) and counters == (stats["rounds"], stats["swaps"], stats["inserts"])
            assert 1 <= syncs <= local_syncs
            sizes = [int(want[rows[b]:rows[b + 1]].sum()) for b in range(len(rows) - 1)]
            assert per.tolist() == [[0, 0, v, v] for v in sizes]


def _raw_call(dev, ei, scores, solution, rows, kicks=3, kick_size=4, shave=0):
    """The library call itself -> (status, error text, the device solution afterwards)."""
    from difusco_amd import _lib
    from difusco_amd.graph import build_csr
    L = _lib.lib()
    n, B = len(scores), len(rows) - 1
    g = build_csr(torch.from_numpy(ei), n, dev)
    d_sol, d_sc = torch.from_numpy(np.asarray(solution, dtype=np.int32)).to(dev), torch.from_numpy(scores).to(dev)
    d_rows = torch.tensor(rows, dtype=torch.int64, device=dev)
    d_seeds, d_offs = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
    nbytes = ctypes.c_size_t()
    _lib.check(L.difusco_mis_iterated_search_workspace_bytes(n, int(g.col.shape[0]), B, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counters, per = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * (4 * B))()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.difusco_mis_iterated_search(n, vp(g.rowptr), vp(g.col), vp(d_sc), vp(d_sol), B, vp(d_rows), vp(d_seeds), vp(d_offs),
                                       kicks, kick_size, 1000, vp(ws), nbytes.value - shave, counters, per,
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return rc, L.difusco_last_error(), d_sol.cpu().numpy()


def test_refused_inputs_leave_the_buffer_alone(dev):
    from difusco_amd import _lib
    from difusco_amd.decode import mis_iterated_search_np
    ei, scores, decoded = fixture("mis_decode_n60_p15")
    n = len(scores)
    a, b = next((int(p), int(q)) for p, q in ei.T if p != q)
    bad = np.zeros(n, dtype=np.int32)
    bad[[a, b]] = 1
    with pytest.raises(_lib.DifuscoHipError, match="not independent"):
        mis_iterated_search_np(scores, bad, edge_index=ei, device=dev, kicks=3)
    rc, err, after = _raw_call(dev, ei, scores, bad, [0, n])
    assert rc == -1 and b"not independent" in err and np.array_equal(after, bad)                     # DIFUSCO_EINVAL
    good = decoded.astype(np.int32)
    for rows in ([0, 30, 20, n], [1, 30, n], [0, 30, n - 1], [0, 30, n + 1]):                         # malformed tables
        rc, err, after = _raw_call(dev, ei, scores, good, rows)
        assert rc == -1 and b"instance_rows" in err and np.array_equal(after, good), rows
    rc, err, after = _raw_call(dev, ei, scores, good, [0, n], shave=1)                               # one byte short
    assert rc == -1 and b"workspace" in err and np.array_equal(after, good)
    for kw in (dict(kicks=-1), dict(kick_size=0)):
        rc, err, after = _raw_call(dev, ei, scores, good, [0, n], **kw)
        assert rc == -1 and np.array_equal(after, good)
    rc, err, after = _raw_call(dev, ei, scores, good, [0, 30, n])                                    # and the call that is fine
    assert rc == 0 and after.sum() >= FIXTURES["mis_decode_n60_p15"][0][1]


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
def test_solve_mis_and_batch_with_kicks(dev, golden_dir):
    from difusco_amd.pipeline import solve_mis, solve_mis_batch
    from difusco_amd.synthetic import er_mis_edge_index
    inst = [(n, er_mis_edge_index(n, 0.1, seed=40 + i)) for i, n in enumerate((60, 57))]
    seeds, P, S = [51, 52], 3, 2
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(2)]
    kw = dict(parallel_sampling=P, sequential_sampling=S, local_search="swap")
    kick = dict(local_search_kicks=8, local_search_kick_size=2)
    stats_all, stats_one = [], []
    res = solve_mis_batch(_mis_model(dev, golden_dir, 0), inst, seeds=seeds, generators=gens(), stats=stats_all, **kw, **kick)
    # step_offset=0: every chunk starts its sampling steps at Philox offset 0, as a fresh solo model does (the runner's setting)
    one = solve_mis_batch(_mis_model(dev, golden_dir, 0), inst, seeds=seeds, generators=gens(), stats=stats_one,
                          instances_per_call=1, step_offset=0, **kw, **kick)
    swap_stats, zero_stats = [], []
    swap = solve_mis_batch(_mis_model(dev, golden_dir, 0), inst, seeds=seeds, generators=gens(), stats=swap_stats, **kw)
    zero = solve_mis_batch(_mis_model(dev, golden_dir, 0), inst, seeds=seeds, generators=gens(), stats=zero_stats,
                           local_search_kicks=0, **kw)
    assert swap_stats == zero_stats and "swap_sizes" not in zero_stats[0]
    per_instance = ("decoded_sizes", "swap_sizes", "kicks_entered", "kicks_accepted")
    for b, (n, ei) in enumerate(inst):
        adj = M.adjacency(n, ei)
        stats = {}
        sol, size, sizes = solve_mis(_mis_model(dev, golden_dir, seeds[b]), n, ei, generator=torch.Generator().manual_seed(b),
                                     stats=stats, **kw, **kick)
        for r in (res[b], one[b]):                                                                 # any chunking, and solo
            assert np.array_equal(r[0], sol) and r[1] == size and r[2] == sizes, b
        for k in per_instance:
            assert stats[k] == stats_all[b][k] == stats_one[b][k] and len(stats[k]) == P * S, k
        assert stats["swap_sizes"] == swap[b][2]                                                   # the first descent is today's
        assert all(a >= s for a, s in zip(sizes, stats["swap_sizes"])) and size == max(sizes)
        assert all(0 <= a <= e <= 8 for a, e in zip(stats["kicks_accepted"], stats["kicks_entered"]))
        assert M.is_independent(adj, sol) and M.is_maximal(adj, sol) and int(sol.sum()) == size
        assert np.array_equal(zero[b][0], swap[b][0]) and zero[b][1:] == swap[b][1:]
    assert sum(sum(s["kicks_entered"]) for s in stats_all) > 0


def test_evaluate_with_kicks(dev, tmp_path):
    from difusco_amd import evaluate as EV
    pattern = _write_mis(tmp_path / "mis", [60, 75], seed=3)
    ckpt, _ = _ckpt(tmp_path / "mis.ckpt", 64, 2)
    argv = _argv(tmp_path, "mis", pattern, ckpt, 64, 2, "--parallel_sampling", "2", "--do_valid_only", "--mis_local_search", "swap")
    flags = ["--mis_local_search_kicks", "8", "--mis_local_search_kick_size", "2"]
    lines, recs = EV.run(argv + flags)
    swap_lines, swap = EV.run(argv)
    assert list(lines[0]) == list(swap_lines[0]) + ["mis_local_search_kicks", "mis_local_search_kick_size"]
    assert (lines[0]["mis_local_search_kicks"], lines[0]["mis_local_search_kick_size"]) == (8, 2)
    extra = ["swap_costs", "kicks_entered", "kicks_accepted", "mis_local_search_kicks", "mis_local_search_kick_size"]
    for r, s in zip(recs, swap):
        assert list(r) == list(s) + extra and (r["mis_local_search_kicks"], r["mis_local_search_kick_size"]) == (8, 2)
        assert r["swap_costs"] == s["all_costs"] and r["decoded_costs"] == s["decoded_costs"]
        assert all(a >= b for a, b in zip(r["all_costs"], r["swap_costs"]))
    assert swap == EV.run(argv + ["--mis_local_search_kicks", "0"])[1]
    assert recs == EV.run(argv + flags + ["--instances_per_call", "1"])[1]
