"""The resident MIS search on the GPU (``difusco_mis_resident_search``: one block per instance, the per-node state in LDS, one
host synchronisation per call).  It must return what the launched search (``difusco_mis_iterated_search``) returns, so every case
here compares the set, the three call counters and the four per-instance counters of ``mode="resident"`` with the numpy
restatement of the rule (tests/mis_iterated_search_emulation.py) AND with ``mode="launches"`` on the same input: hand cases,
degenerate graphs, the decode fixtures capped and not, a union whose ``rounds`` needs the per-descent maximum, state carried
across launches, a hub longer than a block, an instance of exactly the limit and one above it, refused inputs, and the option
through ``solve_mis`` / ``solve_mis_batch`` and the evaluation runner."""
import ctypes

import numpy as np
import pytest
import torch

import mis_iterated_search_emulation as I
from test_gpu_evaluate import _argv, _ckpt, _write_mis
from test_gpu_mis_iterated_search import SEEDS, _reference, _union_call
from test_gpu_mis_local_search import _mis_model
from test_mis_iterated_search_host import CASES, K4, union_of
from test_mis_local_search_host import FIXTURES, fixture, sym

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _call(dev, mode, ei, scores, start, rows, seeds, offsets, kicks, kick_size, cap, kicks_per_launch=0):
    from difusco_amd.decode import mis_iterated_search_np
    stats = {}
    sol = mis_iterated_search_np(scores, start, edge_index=ei, device=dev, instance_rows=rows, seeds=seeds, offsets=offsets,
                                 kicks=kicks, kick_size=kick_size, stats=stats, mode=mode,
                                 **({} if cap is None else {"max_rounds": cap}),
                                 **({} if mode == "launches" else {"kicks_per_launch": kicks_per_launch}))
    per = np.array([stats[k] for k in ("entered", "accepted", "size_before", "size_after")]).T
    return sol, (stats["rounds"], stats["swaps"], stats["inserts"]), per, stats["host_syncs"]


def _equal(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert tuple(got[1]) == tuple(want[1]), (what, got[1], want[1])
    assert np.asarray(got[2]).tolist() == np.asarray(want[2]).tolist(), what


def _same(dev, n, ei, scores, start, *, rows=None, seeds=None, offsets=None, kicks, kick_size=4, cap=None, want=None,
          kicks_per_launch=0, emulate=True):
    """One resident call against the restatement (unless ``emulate`` is off) and against the launched search on the same input.
    -> what the resident call returned: (set, counters, per-instance counters, host synchronisations)."""
    rows = [0, n] if rows is None else rows
    B = len(rows) - 1
    seeds, offsets = [0] * B if seeds is None else seeds, [0] * B if offsets is None else offsets
    got = _call(dev, "resident", ei, scores, start, rows, seeds, offsets, kicks, kick_size, cap, kicks_per_launch)
    assert got[0].shape == (n,) and got[0].dtype == int and got[3] <= 2
    if emulate:
        if want is None:
            want = I.iterated_search(n, ei, scores, start, rows, seeds, offsets, kicks, kick_size, cap)
        _equal(got, want, "restatement")
    _equal(got, _call(dev, "launches", ei, scores, start, rows, seeds, offsets, kicks, kick_size, cap), "launches")
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_hand_cases(dev, name):
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
        sol, *_ = _same(dev, n, graph, sc, np.zeros(n, dtype=int), seeds=[8], kicks=10, kick_size=2)
        assert sol[[3, 8, 9, 10, 11]].tolist() == [1] * 5
    for loops in (np.zeros((2, 0), dtype=np.int64), np.zeros((2, 1), dtype=np.int64)):
        for start in (0, 1):
            sol, _, per, _ = _same(dev, 1, loops, np.array([.3], dtype=np.float32), np.full(1, start), seeds=[2], kicks=3)
            assert sol.tolist() == [1] and per.tolist() == [[0, 0, 1, 1]]


def test_a_graph_without_any_entry(dev):
    none = np.zeros((2, 0), dtype=np.int64)
    sc = np.array([.5, 0, -0.0, 1, .5, 0, .25], dtype=np.float32)
    for start in (np.zeros(7, dtype=int), np.array([0, 1, 0, 0, 1, 0, 0])):
        sol, counters, per, _ = _same(dev, 7, none, sc, start, seeds=[3], kicks=4, kick_size=2)
        assert sol.tolist() == [1] * 7 and per[0, 2:].tolist() == [7, 7] and counters == (0, 0, 7 - int(start.sum()))


def test_duplicate_neighbour_entries(dev):
    """Every entry twice: the doubled-entry K4 and the doubled self loops (the graphs on which the launched search's own test
    can equal the restatement).  Duplicates count per entry and self entries are ignored, as in the launched search."""
    ei = sym(4, K4, self_loops=True)
    _same(dev, 4, np.concatenate([ei, ei], axis=1), np.array([.9, .5, .4, .3], dtype=np.float32), np.zeros(4, dtype=int),
          seeds=[4], kicks=6, kick_size=1)
    loops = sym(5, [], self_loops=True)
    _same(dev, 5, np.concatenate([loops, loops], axis=1), np.arange(5, dtype=np.float32), np.zeros(5, dtype=int), seeds=[4], kicks=2)


@pytest.mark.parametrize("cap", [1, 1000])
@pytest.mark.parametrize("kick_size", [1, 4])
@pytest.mark.parametrize("start", ["decoded", "empty"])
@pytest.mark.parametrize("name", ["mis_decode_n60_p15", "mis_decode_n300_p05"])
def test_small_fixtures(dev, name, start, kick_size, cap):
    """cap = 1: the incumbent need not be a local optimum, so an instance into which nothing entered still descends."""
    ei, scores, decoded = fixture(name)
    n = len(scores)
    s = decoded if start == "decoded" else np.zeros(n, dtype=int)
    for kicks in (0, 1, 8, 20):
        _same(dev, n, ei, scores, s, seeds=[SEEDS[name]], kicks=kicks, kick_size=kick_size, cap=cap,
              want=_reference(name, start, kicks, kick_size, cap))


@pytest.mark.parametrize("start", ["decoded", "empty"])
def test_n750_fixture(dev, start):
    """Mean degree 112: every neighbour list takes the lane stride."""
    name = "mis_decode_n750_p15"
    ei, scores, decoded = fixture(name)
    want = _reference(name, start, 20, 4, 1000)
    assert want[2].tolist() == [[20, 7, 36, 39]]
    s = decoded if start == "decoded" else np.zeros(len(scores), dtype=int)
    sol, _, per, _ = _same(dev, len(scores), ei, scores, s, seeds=[750], kicks=20, kick_size=4, cap=1000, want=want)
    assert per.tolist() == [[20, 7, 36, 39]] and int(sol.sum()) == 39


def test_union_of_the_fixtures_equals_the_solo_calls_and_repeats(dev):
    """``rounds`` of the union is, per descent, the rounds of the instance that descended longest: neither the sum nor the
    maximum of the solo totals."""
    names, n, union, scores, rows, seeds, offsets, start = _union_call()
    kicks = 8
    first = _call(dev, "resident", union, scores, start, rows, seeds, offsets, kicks, 4, None)
    again = _call(dev, "resident", union, scores, start, rows, seeds, offsets, kicks, 4, None)
    _equal(first, again, "second call")
    launched = _call(dev, "launches", union, scores, start, rows, seeds, offsets, kicks, 4, None)
    _equal(first, launched, "launches")
    assert first[1][0] == launched[1][0] > 0
    sol, counters, per, _ = first
    swaps = inserts = 0
    solo_rounds = []
    for b in range(len(rows) - 1):
        name = names[b // 2]
        ei, sc, decoded = fixture(name)
        want = _reference(name, "decoded", kicks, 4, None, seeds[b], offsets[b])
        solo = _call(dev, "resident", ei, sc, decoded, [0, len(sc)], [seeds[b]], [offsets[b]], kicks, 4, None)
        _equal(solo, want, b)
        assert np.array_equal(sol[rows[b]:rows[b + 1]], solo[0]) and per[b].tolist() == solo[2][0].tolist(), b
        swaps, inserts = swaps + solo[1][1], inserts + solo[1][2]
        solo_rounds.append(solo[1][0])
    assert counters[1:] == (swaps, inserts)
    assert max(solo_rounds) <= counters[0] <= sum(solo_rounds)


def test_an_empty_instance_in_the_middle_and_an_offset_that_wraps(dev):
    graphs = [(fixture(name)[0], fixture(name)[1]) for name in ("mis_decode_n60_p15", "mis_decode_n300_p05")]
    n, union, scores, rows = union_of(graphs, empty_after=0)
    assert rows == [0, 60, 60, 360]
    _, _, per, _ = _same(dev, n, union, scores, np.zeros(n, dtype=int), rows=rows, seeds=[1, 2, 3], offsets=[0, 5, 2 ** 64 - 3],
                         kicks=6)                             # the third offset wraps at kick 3
    assert per[1].tolist() == [0, 0, 0, 0] and per[[0, 2], 0].min() > 0


def test_state_is_carried_across_launches(dev):
    """kicks = 8 in launches of 1, 3 (the last one shorter), 8 and the default: the incumbent, the counters and the kick index
    live in the workspace between launches."""
    names, n, union, scores, rows, seeds, offsets, start = _union_call()
    rows, seeds, offsets = rows[:5], seeds[:4], offsets[:4]                      # the two small fixtures, two copies each
    n = rows[-1]
    keep = (union[0] < n) & (union[1] < n)
    union, scores, start = union[:, keep], scores[:n], start[:n]
    want = I.iterated_search(n, union, scores, start, rows, seeds, offsets, 8, 4, 2)
    for per_launch in (1, 3, 8, 0):
        got = _call(dev, "resident", union, scores, start, rows, seeds, offsets, 8, 4, 2, per_launch)
        _equal(got, want, per_launch)
        assert got[3] <= 2


def test_no_poll_in_the_kick_loop(dev):
    ei, scores, decoded = fixture("mis_decode_n60_p15")
    n = len(scores)
    resident = [_call(dev, "resident", ei, scores, decoded, [0, n], [60], [0], kicks, 4, None)[3] for kicks in (0, 8, 64)]
    assert resident[0] == resident[1] == resident[2] <= 2
    launched = [_call(dev, "launches", ei, scores, decoded, [0, n], [60], [0], kicks, 4, None)[3] for kicks in (0, 64)]
    assert launched[1] > launched[0] >= 1                     # what the resident search changes


@pytest.mark.parametrize("centre", ["highest", "lowest"])
def test_a_hub_longer_than_a_block(dev, centre):
    """A star with 1,500 leaves: one neighbour list longer than a block has threads, and a tight count of 1,500."""
    leaves = 1500
    n = leaves + 1
    ei = sym(n, [(0, v) for v in range(1, n)])
    sc = np.random.default_rng(15).random(n).astype(np.float32) * .5 + .25
    sc[0] = 1.0 if centre == "highest" else 0.0
    for start in (np.zeros(n, dtype=int), np.array([1] + [0] * leaves)):
        sol, *_ = _same(dev, n, ei, sc, start, seeds=[9], kicks=4, kick_size=4)
        assert int(sol.sum()) == leaves


def _limit_graph(m):
    rng = np.random.default_rng(4096)
    chords = [(int(a), int(b)) for a, b in rng.integers(0, m, size=(m, 2)) if a != b]
    return sym(m, [(v, (v + 1) % m) for v in range(m)] + chords), rng.random(m).astype(np.float32)


def _raw_call(dev, ei, scores, solution, rows, kicks=3, kick_size=4, shave=0, kicks_per_launch=0):
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
    _lib.check(L.difusco_mis_resident_search_workspace_bytes(n, int(g.col.shape[0]), B, max(kicks, 0), ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counters, per = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * (4 * B))()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.difusco_mis_resident_search(n, vp(g.rowptr), vp(g.col), vp(d_sc), vp(d_sol), B, vp(d_rows), vp(d_seeds), vp(d_offs),
                                       kicks, kick_size, 1000, kicks_per_launch, vp(ws), nbytes.value - shave, counters, per,
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return rc, L.difusco_last_error(), d_sol.cpu().numpy()


def test_an_instance_of_exactly_the_limit_and_one_above_it(dev):
    from difusco_amd import _lib
    m = int(_lib.lib().difusco_mis_resident_max_nodes())
    ei, sc = _limit_graph(m)
    sol, _, per, _ = _same(dev, m, ei, sc, np.zeros(m, dtype=int), seeds=[7], kicks=3, emulate=False)
    assert per[0, 3] == int(sol.sum()) >= per[0, 2] > 0
    # one isolated node more: DIFUSCO_EUNSUPPORTED, the text names the instance and the limit, the buffer is unchanged
    sc1 = np.concatenate([sc, np.array([.5], dtype=np.float32)])
    start = np.zeros(m + 1, dtype=np.int32)
    start[m] = 1
    rc, err, after = _raw_call(dev, ei, sc1, start, [0, m + 1])
    assert rc == -4 and b"instance 0" in err and str(m).encode() in err and str(m + 1).encode() in err
    assert np.array_equal(after, start)
    # in a two-instance table an oversize second instance refuses the whole call
    small = sym(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    union = np.concatenate([small, ei + 5], axis=1)
    sc2 = np.concatenate([np.array([.5, .9, .4, .8, .3], dtype=np.float32), sc1])
    start = np.zeros(m + 6, dtype=np.int32)
    start[[1, 3]] = 1
    rc, err, after = _raw_call(dev, union, sc2, start, [0, 5, m + 6])
    assert rc == -4 and b"instance 1" in err and str(m).encode() in err and np.array_equal(after, start)
    with pytest.raises(_lib.DifuscoHipError, match="limit"):
        _call(dev, "resident", union, sc2, start, [0, 5, m + 6], [0, 0], [0, 0], 1, 4, None)


def test_refused_inputs_leave_the_buffer_alone(dev):
    from difusco_amd import _lib
    ei, scores, decoded = fixture("mis_decode_n60_p15")
    n = len(scores)
    a, b = next((int(p), int(q)) for p, q in ei.T if p != q)
    bad = np.zeros(n, dtype=np.int32)
    bad[[a, b]] = 1
    with pytest.raises(_lib.DifuscoHipError, match="not independent"):
        _call(dev, "resident", ei, scores, bad, [0, n], [0], [0], 3, 4, None)
    rc, err, after = _raw_call(dev, ei, scores, bad, [0, n])
    assert rc == -1 and b"not independent" in err and np.array_equal(after, bad)                     # DIFUSCO_EINVAL
    good = decoded.astype(np.int32)
    for rows in ([0, 30, 20, n], [1, 30, n], [0, 30, n - 1], [0, 30, n + 1]):                         # malformed tables
        rc, err, after = _raw_call(dev, ei, scores, good, rows)
        assert rc == -1 and b"instance_rows" in err and np.array_equal(after, good), rows
    rc, err, after = _raw_call(dev, ei, scores, good, [0, n], shave=1)                               # one byte short
    assert rc == -1 and b"workspace" in err and np.array_equal(after, good)
    for kw in (dict(kicks=-1), dict(kick_size=0), dict(kicks_per_launch=-1)):
        rc, err, after = _raw_call(dev, ei, scores, good, [0, n], **kw)
        assert rc == -1 and np.array_equal(after, good), kw
    rc, err, after = _raw_call(dev, ei, scores, good, [0, 30, n])                                    # and the call that is fine
    assert rc == 0 and after.sum() >= FIXTURES["mis_decode_n60_p15"][0][1]


# ---- pipeline and runner -----------------------------------------------------------------------------------------------------
def test_solve_mis_and_batch_in_resident_mode(dev, golden_dir):
    from difusco_amd.pipeline import solve_mis, solve_mis_batch
    from difusco_amd.synthetic import er_mis_edge_index
    inst = [(n, er_mis_edge_index(n, 0.1, seed=40 + i)) for i, n in enumerate((60, 57))]
    seeds, P, S = [51, 52], 3, 2
    gens = lambda: [torch.Generator().manual_seed(b) for b in range(2)]
    kw = dict(parallel_sampling=P, sequential_sampling=S, local_search="swap")
    kick = dict(local_search_kicks=8, local_search_kick_size=2)
    res = dict(local_search_mode="resident")

    def batch(**more):
        stats = []
        out = solve_mis_batch(_mis_model(dev, golden_dir, 0), inst, seeds=seeds, generators=gens(), stats=stats, **kw, **more)
        return [(r[0].tolist(), r[1], r[2]) for r in out], stats

    launched = batch(**kick)
    assert batch(**kick, **res) == launched
    # the call counters of the stats belong to a chunk: one instance per call is held against the launched run chunked alike
    one = batch(**kick, **res, instances_per_call=1, step_offset=0)
    assert one == batch(**kick, instances_per_call=1, step_offset=0) and one[0] == launched[0]
    for b, (n, ei) in enumerate(inst):
        solo = []
        for more in ({}, res):
            stats = {}
            sol, size, sizes = solve_mis(_mis_model(dev, golden_dir, seeds[b]), n, ei, generator=torch.Generator().manual_seed(b),
                                         stats=stats, **kw, **kick, **more)
            solo.append((sol.tolist(), size, sizes, stats))
        assert solo[0] == solo[1]
        assert solo[1][:3] == launched[0][b]
        for k in ("decoded_sizes", "swap_sizes", "kicks_entered", "kicks_accepted"):
            assert solo[1][3][k] == launched[1][b][k], k
    # kicks = 0 in resident mode is the plain swap search, stats included
    assert batch(**res) == batch() == batch(local_search_kicks=0, **res)
    assert "swap_sizes" not in batch(**res)[1][0]


def test_evaluate_in_resident_mode(dev, tmp_path):
    from difusco_amd import evaluate as EV
    pattern = _write_mis(tmp_path / "mis", [60, 75], seed=3)
    ckpt, _ = _ckpt(tmp_path / "mis.ckpt", 64, 2)
    argv = _argv(tmp_path, "mis", pattern, ckpt, 64, 2, "--parallel_sampling", "2", "--do_valid_only", "--mis_local_search", "swap",
                 "--mis_local_search_kicks", "8", "--mis_local_search_kick_size", "2")
    lines, recs = EV.run(argv + ["--mis_local_search_mode", "resident"])
    launched_lines, launched = EV.run(argv)
    assert lines[0]["mis_local_search_mode"] == "resident" and "mis_local_search_mode" not in launched_lines[0]
    assert list(lines[0]) == list(launched_lines[0]) + ["mis_local_search_mode"]
    assert all(r["mis_local_search_mode"] == "resident" for r in recs)
    drop = lambda rs: [{k: v for k, v in r.items() if k != "mis_local_search_mode"} for r in rs]
    assert drop(recs) == launched and all("mis_local_search_mode" not in r for r in launched)
    assert recs == EV.run(argv + ["--mis_local_search_mode", "resident", "--instances_per_call", "1"])[1]
