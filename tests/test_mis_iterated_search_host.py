"""The numpy restatement of the iterated MIS swap search (tests/mis_iterated_search_emulation.py) held against hand cases with
injected draws, the exact-integer kicked test, its own invariants and the union = solo contract, so that the GPU tests compare
against something checked; and the argument checks of the Python entry points that need no GPU."""
import numpy as np
import pytest

import mis_iterated_search_emulation as I
import mis_local_search_emulation as M
from test_mis_local_search_host import GNP, HAND, STAR_LEAVES, fixture, gnp, sym

TOP = (1 << 24) - 1                                          # the largest draw: kicked only when m_b <= kick_size


def constant_draw(*per_kick):
    """draw hook: kick t of every instance takes ``per_kick[t % len]`` (a list of 24-bit values, one per node)."""
    return lambda b, t, n_b: np.array(per_kick[t % len(per_kick)][:n_b], dtype=np.int64)


# name -> (n, undirected pairs, scores, start set or None (empty), max_rounds, kick_size, draws per kick)
K4 = [(a, b) for a in range(4) for b in range(a + 1, 4)]
CASES = {
    # the descent ends in {1, 3}; node 2 is forced in, 1 and 3 leave, the insertion phase adds 0 and 4: the optimum
    "path5": (5, [(0, 1), (1, 2), (2, 3), (3, 4)], (.5, .9, .4, .8, .3), None, None, 1, [[TOP, TOP, 0, TOP, TOP]]),
    # capped at 0 rounds the leaves stay; the centre is the one outside node (m = 1: always kicked), all leaves leave, the capped
    # descent cannot bring them back, so the kick is restored
    "star_restored": (STAR_LEAVES + 1, HAND["star"][1], HAND["star"][2], [0] + [1] * STAR_LEAVES, 0, 1, [[TOP] * (STAR_LEAVES + 1)]),
    # uncapped the swap round brings the leaves back: a plateau move that is kept
    "star_plateau": (STAR_LEAVES + 1, HAND["star"][1], HAND["star"][2], [0] + [1] * STAR_LEAVES, None, 1, [[TOP] * (STAR_LEAVES + 1)]),
    # m = 3, every outside node is kicked, the smallest (w, node) replaces the member: every kick is a plateau move
    "k4": (4, K4, (.9, .5, .4, .3), None, None, 3, [[9, 5, 3, 7], [1, 1, 1, 1], [2, 8, 8, 2]]),
    "edgeless": (6, [], (.1, .2, .3, .4, .5, .6), None, None, 4, [[0] * 6]),
    # I = {0, 3}; 1 and 2 are adjacent and both kicked with equal draws: only node 1 enters
    "adjacent_pair": (4, [(0, 1), (1, 2), (2, 3)], (.9, .1, .2, .8), None, None, 2, [[0, 7, 7, 0]]),
}


def run_case(name, kicks):
    n, pairs, scores, start, cap, kick_size, draws = CASES[name]
    ei = sym(n, pairs)
    start = np.zeros(n, dtype=int) if start is None else np.array(start)
    sc = np.array(scores, dtype=np.float32)
    return n, ei, sc, start, cap, kick_size, I.iterated_search(n, ei, sc, start, kicks=kicks, kick_size=kick_size, max_rounds=cap,
                                                              draw=constant_draw(*draws))


def check_properties(n, ei, scores, start, cap, rows, result, kicks):
    """Independent, maximal, every instance no smaller than the descent alone, the counters consistent with the sets."""
    sol, (rounds, swaps, inserts), per = result
    adj = M.adjacency(n, ei)
    assert M.is_independent(adj, sol) and M.is_maximal(adj, sol)
    descent, *_ = M.local_search(n, adj, scores, start, cap)
    for b in range(len(rows) - 1):
        lo, hi = rows[b], rows[b + 1]
        entered, accepted, before, after = per[b].tolist()
        assert before == int(descent[lo:hi].sum()) and after == int(sol[lo:hi].sum()) >= before
        assert 0 <= accepted <= entered <= kicks
        if accepted == 0:
            assert after == before or cap is not None        # without a kept kick only a capped descent can still grow
    assert int(per[:, 3].sum() - per[:, 2].sum()) == int(sol.sum()) - int(descent.sum())


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kicks", [0, 1, 3])
def test_hand_cases_keep_the_properties(name, kicks):
    n, ei, sc, start, cap, kick_size, result = run_case(name, kicks)
    check_properties(n, ei, sc, start, cap, [0, n], result, kicks)


def test_kicks_zero_is_the_descent():
    for name in ("mis_decode_n60_p15", "mis_decode_n300_p05"):
        ei, scores, decoded = fixture(name)
        n = len(scores)
        for start in (decoded, np.zeros(n, dtype=int)):
            for cap in (None, 1):
                want = M.local_search(n, ei, scores, start, cap)
                sol, counters, per = I.iterated_search(n, ei, scores, start, kicks=0, max_rounds=cap, seeds=[3], offsets=[9])
                assert np.array_equal(sol, want[0]) and counters == tuple(want[1:])
                assert per.tolist() == [[0, 0, int(sol.sum()), int(sol.sum())]]


def test_path_of_five_reaches_the_optimum():
    *_, (sol, counters, per) = run_case("path5", 1)
    assert sol.tolist() == [1, 0, 1, 0, 1] and per.tolist() == [[1, 1, 2, 3]]


def test_star_kick_is_restored_when_capped_and_kept_as_a_plateau_when_not():
    *_, (sol, counters, per) = run_case("star_restored", 2)
    assert sol.tolist() == [0] + [1] * STAR_LEAVES and per.tolist() == [[2, 0, STAR_LEAVES, STAR_LEAVES]]
    *_, (sol, counters, per) = run_case("star_plateau", 2)
    assert sol.tolist() == [0] + [1] * STAR_LEAVES and per.tolist() == [[2, 2, STAR_LEAVES, STAR_LEAVES]]
    assert counters == (2, 2, 2 * (STAR_LEAVES - 2))         # one swap round per kick: two leaves by the swap, the rest inserted


def test_k4_every_kick_is_a_kept_plateau_move():
    *_, (sol, counters, per) = run_case("k4", 3)
    # kick 0: 1, 2, 3 are kicked (0 is the member), (3, 2) is the smallest key; kick 1: 0, 1, 3 tie at w = 1, node 0 enters;
    # kick 2: 1, 2, 3 with draws 8, 8, 2: node 3 enters
    assert sol.tolist() == [0, 0, 0, 1] and per.tolist() == [[3, 3, 1, 1]] and counters == (0, 0, 1)


def test_edgeless_graph_kicks_nothing():
    *_, (sol, counters, per) = run_case("edgeless", 3)
    assert sol.tolist() == [1] * 6 and per.tolist() == [[0, 0, 6, 6]]


def test_of_two_adjacent_kicked_nodes_the_smaller_key_enters():
    assert I.entered_nodes(M.adjacency(4, sym(4, [(0, 1), (1, 2), (2, 3)])), {1: 7, 2: 7}) == [1]
    assert I.entered_nodes(M.adjacency(4, sym(4, [(0, 1), (1, 2), (2, 3)])), {1: 7, 2: 6}) == [2]
    assert I.entered_nodes(M.adjacency(4, sym(4, [(0, 1), (1, 2), (2, 3)])), {0: 7, 2: 7, 3: 9}) == [0, 2]
    *_, (sol, counters, per) = run_case("adjacent_pair", 1)
    assert sol.tolist() == [0, 1, 0, 1] and per.tolist() == [[1, 1, 2, 2]]


def test_the_kicked_test_is_exact_at_the_boundary():
    assert I.is_kicked((1 << 22) - 1, 4, 1) and not I.is_kicked(1 << 22, 4, 1)              # w m == kick_size 2^24: not kicked
    assert I.is_kicked(TOP, 3, 3) and not I.is_kicked(TOP, 4, 3) and I.is_kicked(0, 2 ** 31 - 1, 1)
    # through the search: K5, one member, m = 4, kick_size 1: a draw of 2^22 kicks nobody, 2^22 - 1 everybody
    k5 = sym(5, [(a, b) for a in range(5) for b in range(a + 1, 5)])
    sc = np.array([.9, .5, .4, .3, .2], dtype=np.float32)
    for w, entered in ((1 << 22, 0), ((1 << 22) - 1, 1)):
        _, _, per = I.iterated_search(5, k5, sc, np.zeros(5, dtype=int), kicks=1, kick_size=1, draw=constant_draw([w] * 5))
        assert per.tolist() == [[entered, entered, 1, 1]]


def union_of(graphs, empty_after=None):
    """(n, edge_index, scores, instance_rows) of the disjoint union; ``empty_after``: an empty instance after that graph."""
    ns = [len(s) for _, s in graphs]
    off = np.concatenate([[0], np.cumsum(ns)]).astype(int)
    union = np.concatenate([ei + off[g] for g, (ei, _) in enumerate(graphs)], axis=1)
    rows = off.tolist()
    if empty_after is not None:
        rows.insert(empty_after + 1, rows[empty_after + 1])
    return int(off[-1]), union, np.concatenate([s for _, s in graphs]), rows


@pytest.mark.parametrize("cap", [None, 1])
def test_union_of_three_instances_equals_the_solo_runs(cap):
    graphs = [gnp(n, p, seed=n) for n, p in GNP]
    n, union, scores, rows = union_of(graphs, empty_after=0)           # rows: graph 0, an empty instance, graph 1, graph 2
    seeds, offsets, kicks = [11, 99, 2 ** 63 + 5, 7], [0, 1, 2 ** 64 - 2, 1 << 62], 6     # an offset that wraps at kick 2
    result = I.iterated_search(n, union, scores, np.zeros(n, dtype=int), rows, seeds, offsets, kicks, 2, cap)
    sol, counters, per = result
    check_properties(n, union, scores, np.zeros(n, dtype=int), cap, rows, result, kicks)
    assert per[1].tolist() == [0, 0, 0, 0]
    total, most = np.zeros(3, dtype=int), 0
    for g, b in enumerate((0, 2, 3)):
        m = len(graphs[g][1])
        solo, c, p = I.iterated_search(m, graphs[g][0], graphs[g][1], np.zeros(m, dtype=int), None, [seeds[b]], [offsets[b]],
                                       kicks, 2, cap)
        assert np.array_equal(sol[rows[b]:rows[b + 1]], solo) and per[b].tolist() == p[0].tolist(), g
        total += c
        most = max(most, c[0])
    # swaps and inserts add up; a round of the union is a round of every instance that still moves
    assert tuple(total[1:]) == counters[1:] and most <= counters[0] <= total[0]
    assert per[:, 0].sum() > 0                               # the Philox draws did kick something


def test_different_seeds_give_different_kicks_and_the_same_seed_the_same():
    ei, scores = gnp(64, .15, seed=64)
    runs = [I.iterated_search(64, ei, scores, np.zeros(64, dtype=int), seeds=[s], offsets=[o], kicks=4)[2].tolist()
            for s, o in ((1, 0), (1, 0), (2, 0), (1, 4))]
    assert runs[0] == runs[1]
    draws = [I.philox_draw([s], [o])(0, 0, 64).tolist() for s, o in ((1, 0), (2, 0), (1, 4))]
    assert draws[0] != draws[1] != draws[2] != draws[0]
    assert I.philox_draw([1], [0])(0, 4, 64).tolist() == draws[2]      # kick t draws at offset + t


# ---- argument checks of the Python entry points (no GPU) ---------------------------------------------------------------------
def test_kicks_without_the_swap_search_are_refused():
    from difusco_amd import decode, pipeline
    assert decode.MIS_LOCAL_SEARCHES == ("none", "swap")
    assert decode.check_mis_kicks("swap", 8, 4) == (8, 4) and decode.check_mis_kicks("none", 0, 4) == (0, 4)
    for bad in (("none", 1, 4), ("swap", -1, 4), ("swap", 1, 0), ("swap", 1.5, 4)):
        with pytest.raises(ValueError):
            decode.check_mis_kicks(*bad)
    none = np.zeros((2, 0), dtype=np.int64)
    with pytest.raises(ValueError, match="swap"):
        pipeline.solve_mis(None, 3, none, local_search_kicks=2)
    with pytest.raises(ValueError, match="swap"):
        pipeline.solve_mis_batch(None, [(3, none)], local_search="none", local_search_kicks=2)
    with pytest.raises(ValueError):
        pipeline.solve_mis(None, 3, none, local_search="swap", local_search_kicks=2, local_search_kick_size=0)


def test_evaluate_refuses_kicks_without_swap(capsys):
    from difusco_amd import evaluate as EV
    argv = ["--storage_path", "x", "--do_test", "--ckpt_path", "c", "--task", "mis"]
    args, _ = EV.parse_args(argv + ["--mis_local_search", "swap", "--mis_local_search_kicks", "30"])
    assert (args.mis_local_search_kicks, args.mis_local_search_kick_size) == (30, 4)
    args, _ = EV.parse_args(argv)
    assert (args.mis_local_search_kicks, args.mis_local_search_kick_size) == (0, 4)
    with pytest.raises(SystemExit) as e:
        EV.parse_args(argv + ["--mis_local_search_kicks", "30"])
    assert e.value.code == 2 and "--mis_local_search swap" in capsys.readouterr().err
    for bad in (["--mis_local_search_kicks", "-1"], ["--mis_local_search_kick_size", "0"]):
        with pytest.raises(SystemExit):
            EV.parse_args(argv + ["--mis_local_search", "swap"] + bad)


def test_a_cpu_device_and_bad_tables_are_refused():
    from difusco_amd import _lib
    from difusco_amd.decode import mis_iterated_search_np
    sc, ei = np.array([.5, .9, .4], dtype=np.float32), sym(3, [(0, 1), (1, 2)])
    with pytest.raises(_lib.DifuscoHipError):
        mis_iterated_search_np(sc, [0, 1, 0], edge_index=ei, kicks=2, device="cpu")
    with pytest.raises(ValueError):
        mis_iterated_search_np(sc, [0, 1, 0], edge_index=ei, kicks=-1, device="cuda:0")
    with pytest.raises(ValueError):
        mis_iterated_search_np(sc, [0, 1, 0], edge_index=ei, kicks=1, kick_size=0, device="cuda:0")


def test_library_argument_checks_come_before_any_gpu_work():
    import ctypes
    from difusco_amd import _lib
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    counters = (ctypes.c_int32 * 3)()
    for bad in ((0, 0, 1), (5, -1, 1), (5, 8, 0)):
        assert L.difusco_mis_iterated_search_workspace_bytes(*bad, ctypes.byref(nbytes)) < 0
    assert L.difusco_mis_iterated_search_workspace_bytes(5, 8, 1, None) < 0
    assert L.difusco_mis_iterated_search_workspace_bytes(5, 8, 2, ctypes.byref(nbytes)) == 0
    local = ctypes.c_size_t()
    assert L.difusco_mis_local_search_workspace_bytes(5, 8, ctypes.byref(local)) == 0 and nbytes.value > local.value
    #     n  rowptr col scores sol B rows seeds offsets kicks kick_size max_rounds ws bytes counters per stream
    ok = [5, p, p, p, p, 2, p, p, p, 3, 4, 10, p, 1 << 20, counters, None, None]
    for i, v in ((0, 0), (1, None), (2, None), (3, None), (4, None), (5, 0), (6, None), (7, None), (8, None), (12, None),
                 (14, None), (13, nbytes.value - 1)):
        bad = list(ok)
        bad[i] = v
        assert L.difusco_mis_iterated_search(*bad) == -1, i
    for i, word in ((9, b"kicks"), (10, b"kick_size"), (11, b"max_rounds")):
        bad = list(ok)
        bad[i] = -1 if i != 10 else 0
        assert L.difusco_mis_iterated_search(*bad) == -1 and word in L.difusco_last_error()
