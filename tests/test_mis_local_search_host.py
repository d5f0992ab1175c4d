"""The numpy restatement of the MIS swap local search (tests/mis_local_search_emulation.py) held against hand cases, the committed
decode fixtures and its own invariants, so that the GPU tests compare against something checked; and the argument checks of the
Python entry points that need no GPU."""
import functools
import os

import numpy as np
import pytest

import graph_zoo as Z
import mis_local_search_emulation as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sym(n, pairs, self_loops=False):
    """int64 [2, E]: both directions of every undirected pair, optionally a self loop on every node (the dataset's layout)."""
    a = np.array([[p, q] for p, q in pairs] + [[q, p] for p, q in pairs] + ([[v, v] for v in range(n)] if self_loops else []),
                 dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(a.T)


STAR_LEAVES = 70
# name -> (n, undirected pairs, scores, (solution or None, rounds, swaps, inserts) from the empty start set)
HAND = {
    "path": (3, [(0, 1), (1, 2)], (.5, .9, .4), ([1, 0, 1], 1, 1, 1)),
    "k4": (4, [(a, b) for a in range(4) for b in range(a + 1, 4)], (.9, .5, .4, .3), ([1, 0, 0, 0], 0, 0, 1)),
    "claw": (4, [(0, 1), (0, 2), (0, 3)], (.9, .5, .4, .3), ([0, 1, 1, 1], 1, 1, 2)),
    "bridged_paths": (6, [(0, 1), (1, 2), (3, 4), (4, 5), (0, 3)], (.5, .9, .4, .45, .8, .3), ([1, 0, 1, 0, 1, 0], 1, 1, 2)),
    "star": (STAR_LEAVES + 1, [(0, v) for v in range(1, STAR_LEAVES + 1)], (1.0,) + (.5,) * STAR_LEAVES,
             ([0] + [1] * STAR_LEAVES, 1, 1, STAR_LEAVES - 1)),
    "tied_path": (3, [(0, 1), (1, 2)], (.5, .5, .5), ([1, 0, 1], 0, 0, 2)),
}
# fixture -> (decoded size, final size, (rounds, swaps, inserts)), then size and counters with max_rounds = 1
FIXTURES = {
    "mis_decode_n60_p15": ((16, 19, (1, 1, 2)), (19, (1, 1, 2))),
    "mis_decode_n300_p05": ((58, 63, (2, 5, 0)), (62, (1, 4, 0))),
    "mis_decode_n750_p15": ((28, 36, (3, 7, 1)), (30, (1, 2, 0))),
}
GNP = ((40, .2), (64, .15), (90, .1))


def gnp(n, p, seed):
    """(edge_index int64 [2, E] both directions plus self loops, float32 scores) of one G(n, p)."""
    rng = np.random.default_rng(seed)
    r, c = np.nonzero(np.triu(rng.random((n, n)) < p, 1))
    return sym(n, list(zip(r.tolist(), c.tolist())), self_loops=True), rng.random(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["edge_index"].astype(np.int64), z["predictions"].astype(np.float32), z["solution"].astype(np.int64)


def symmetric_zoo():
    out = []
    for name in Z.ZOO:
        deg, ei = Z.zoo_graph(name)
        pairs = set(zip(ei[0].tolist(), ei[1].tolist()))
        if all((b, a) in pairs for a, b in pairs):
            out.append(name)
    return out


@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(name):
    n, pairs, scores, (want, rounds, swaps, inserts) = HAND[name]
    sol, *counters = M.local_search(n, sym(n, pairs), np.array(scores, dtype=np.float32), np.zeros(n, dtype=int))
    assert sol.tolist() == want and tuple(counters) == (rounds, swaps, inserts)
    assert int(sol.sum()) == swaps + inserts
    if name == "star":
        assert int(sol.sum()) == STAR_LEAVES


@pytest.mark.parametrize("name", list(FIXTURES))
def test_decode_fixtures(name):
    ei, scores, decoded = fixture(name)
    n = len(scores)
    (size0, size, counters), (size1, counters1) = FIXTURES[name]
    adj = M.adjacency(n, ei)
    assert int(decoded.sum()) == size0
    sol, *got = M.local_search(n, adj, scores, decoded)
    assert (int(sol.sum()), tuple(got)) == (size, counters)
    sol1, *got1 = M.local_search(n, adj, scores, decoded, max_rounds=1)
    assert (int(sol1.sum()), tuple(got1)) == (size1, counters1)
    empty, *_ = M.local_search(n, adj, scores, np.zeros(n, dtype=int))
    assert np.array_equal(empty, sol)


def _invariants(n, ei, scores, start):
    adj = M.adjacency(n, ei)
    sol, rounds, swaps, inserts = M.local_search(n, adj, scores, start)
    assert M.is_independent(adj, sol) and M.is_maximal(adj, sol)
    assert M.remaining_swaps(adj, sol) == []
    assert int(sol.sum()) == int(np.sum(start)) + swaps + inserts
    return sol


@pytest.mark.parametrize("n,p", GNP)
def test_invariants_on_gnp(n, p):
    ei, scores = gnp(n, p, seed=n)
    sol = _invariants(n, ei, scores, np.zeros(n, dtype=int))
    half = sol.copy()
    half[np.flatnonzero(sol)[::2]] = 0                       # a non-maximal independent start set
    _invariants(n, ei, scores, half)


def test_the_zoo_has_symmetric_graphs():
    assert {"ones_96", "no_edges"} <= set(symmetric_zoo())


@pytest.mark.parametrize("name", symmetric_zoo())
def test_invariants_on_the_symmetric_zoo_graphs(name):
    deg, ei = Z.zoo_graph(name)
    n = len(deg)
    _invariants(n, ei, np.random.default_rng(n).random(n).astype(np.float32), np.zeros(n, dtype=int))


@pytest.mark.parametrize("cap", [None, 1, 2])
def test_union_equals_solo(cap):
    graphs = [gnp(n, p, seed=n) for n, p in GNP]
    off = np.concatenate([[0], np.cumsum([n for n, _ in GNP])])
    union = np.concatenate([ei + off[g] for g, (ei, _) in enumerate(graphs)], axis=1)
    scores = np.concatenate([s for _, s in graphs])
    sol, *_ = M.local_search(int(off[-1]), union, scores, np.zeros(int(off[-1]), dtype=int), cap)
    for g, (n, _) in enumerate(GNP):
        solo, *_ = M.local_search(n, graphs[g][0], graphs[g][1], np.zeros(n, dtype=int), cap)
        assert np.array_equal(sol[off[g]:off[g + 1]], solo), g


def test_a_dependent_start_set_is_refused():
    with pytest.raises(AssertionError):
        M.local_search(3, sym(3, [(0, 1), (1, 2)]), np.array([.5, .9, .4], dtype=np.float32), [1, 1, 0])


# ---- argument checks of the Python entry points (no GPU) ---------------------------------------------------------------------
def test_unknown_local_search_is_refused():
    from difusco_amd import decode, pipeline
    assert decode.MIS_LOCAL_SEARCHES == ("none", "swap")
    assert decode.check_mis_local_search("swap") == "swap"
    with pytest.raises(ValueError):
        decode.check_mis_local_search("2opt")
    with pytest.raises(ValueError):
        pipeline.solve_mis(None, 3, np.zeros((2, 0), dtype=np.int64), local_search="flip")
    with pytest.raises(ValueError):
        pipeline.solve_mis_batch(None, [(3, np.zeros((2, 0), dtype=np.int64))], local_search="flip")


def test_evaluate_refuses_the_flag_for_tsp(capsys):
    from difusco_amd import evaluate as EV
    argv = ["--storage_path", "x", "--do_test", "--ckpt_path", "c"]
    args, _ = EV.parse_args(["--task", "mis", "--mis_local_search", "swap"] + argv)
    assert args.mis_local_search == "swap"
    assert EV.parse_args(["--task", "mis"] + argv)[0].mis_local_search == "none"
    with pytest.raises(SystemExit) as e:
        EV.parse_args(["--task", "tsp", "--mis_local_search", "swap"] + argv)
    assert e.value.code == 2 and "--mis_local_search" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        EV.parse_args(["--task", "mis", "--mis_local_search", "2opt"] + argv)


def test_a_cpu_device_is_refused():
    from difusco_amd import _lib
    from difusco_amd.decode import mis_local_search_np
    with pytest.raises(_lib.DifuscoHipError):
        mis_local_search_np(np.array([.5, .9, .4], dtype=np.float32), [0, 1, 0], edge_index=sym(3, [(0, 1), (1, 2)]), device="cpu")


def test_library_argument_checks_come_before_any_gpu_work():
    import ctypes
    from difusco_amd import _lib
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    p = ctypes.c_void_p(0x1000)
    counters = (ctypes.c_int32 * 3)()
    assert L.difusco_mis_local_search_workspace_bytes(0, 0, ctypes.byref(nbytes)) < 0
    assert L.difusco_mis_local_search_workspace_bytes(5, -1, ctypes.byref(nbytes)) < 0
    assert L.difusco_mis_local_search_workspace_bytes(5, 8, None) < 0
    ok = [5, p, p, p, p, 10, p, 1 << 20, counters, None]
    for i, v in ((0, 0), (1, None), (2, None), (3, None), (4, None), (6, None), (8, None)):
        bad = list(ok)
        bad[i] = v
        assert L.difusco_mis_local_search(*bad) == -1, i
    bad = list(ok)
    bad[5] = -1
    assert L.difusco_mis_local_search(*bad) == -1 and b"max_rounds" in L.difusco_last_error()
