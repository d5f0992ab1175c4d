"""The groups the heat-ranked candidate lists are held to (tests/test_tsp_heat_candidates_host.py on the emulation,
tests/test_gpu_tsp_heat_candidates.py on the GPU), with the emulation's result of every (case, K) computed once per session.  TEST
INFRASTRUCTURE ONLY (a helper module like tests/graph_zoo.py: nothing is collected from it).

A case is (points float64 [n, 2], row_ptr int32 [n + 1], col int32 [E], heat float32 [P, E]).  The sizes are the smallest at
which the kernels take another path: a city with more gathered entries than a wave has lanes (64), than two waves, than a block
of 1024 threads; rows of degree 0; a city nobody names; K below, at and above the number of candidates; K = 1 and K = 128."""
import functools

import numpy as np

import tsp_heat_candidates_emulation as E


def _knn(n, k, seed, P, heat="random"):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    rp, col, _ = E.knn_graph(pts, k)
    h = rng.random((P, len(col))).astype(np.float32) if heat == "random" else np.zeros((P, len(col)), dtype=np.float32)
    return pts, rp, col, h


def _complete(n, seed, P):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    rp = np.arange(0, n * n + 1, n, dtype=np.int32)
    col = np.tile(np.arange(n, dtype=np.int32), n)
    return pts, rp, col, rng.random((P, n * n)).astype(np.float32)


def _from_rows(pts, rows, P, seed):
    """A graph from a list of per-city column lists."""
    n = len(pts)
    r = np.concatenate([np.full(len(c), u, dtype=np.int64) for u, c in enumerate(rows)] + [np.zeros(0, dtype=np.int64)])
    c = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows] + [np.zeros(0, dtype=np.int64)])
    rp, col = E.csr(n, r, c)
    return pts, rp, col, np.random.default_rng(seed).random((P, len(col))).astype(np.float32)


def _hub(n, P, seed, extra):
    """Every row lists city 0 and ``extra`` of its nearest other cities: city 0 has in-degree n - 1 (its own row lists itself)."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    _, col, _ = E.knn_graph(pts, extra + 1)
    near = col.reshape(n, extra + 1)[:, 1:]
    return _from_rows(pts, [[0] + list(near[u]) for u in range(n)], P, seed + 1)


def _empty_rows():
    """n = 12: row 5 is empty; city 7 has an empty row and no row names it (its list is all pads)."""
    rng = np.random.default_rng(12)
    pts = rng.random((12, 2))
    _, col, _ = E.knn_graph(pts, 5)
    rows = [[int(c) for c in col.reshape(12, 5)[u] if c != 7] for u in range(12)]
    rows[5], rows[7] = [], []
    return _from_rows(pts, rows, 2, 13)


def _duplicates():
    """n = 20, k = 5 with the self edges kept; every third entry a second and every seventh a third time, each with its own heat."""
    pts, rp, col, _ = _knn(20, 5, 20, 1)
    r = E.rows_of(rp)
    r = np.concatenate([r, r[::3], r[::7]])
    c = np.concatenate([col, col[::3], col[::7]])
    order = np.argsort(r, kind="stable")
    rp2, col2 = E.csr(20, r[order], c[order])
    return pts, rp2, col2, np.random.default_rng(21).random((3, len(col2))).astype(np.float32)


def _corners():
    """Heat that holds NaN, -1, 2.0 and 1e-6 (q = 0), a different pattern per tour."""
    pts, rp, col, h = _knn(16, 6, 16, 4)
    h[0, ::7] = np.nan
    h[1, ::3] = -1.0
    h[2, ::4] = 2.0
    h[3, ::2] = 1e-6
    h[3, 1::5] = np.inf
    return pts, rp, col, h


def _saturated():
    """The complete graph on 10 cities, two of them at one place, every heat 1.0: d2 ties between 3 and 4 for every city, so the
    index decides; from 3 and from 4 the other is at d2 = 0."""
    pts, rp, col, h = _complete(10, 10, 2)
    pts[4] = pts[3]
    return pts, rp, col, np.ones_like(h)


def _n3():
    pts = np.array([[0.1, 0.2], [0.7, 0.3], [0.4, 0.9]])
    return _from_rows(pts, [[1, 2], [0], []], 2, 3)


CASES = {
    "n3": (_n3, (1, 2, 5)),
    "complete5": (lambda: _complete(5, 5, 2), (4,)),
    "dense14": (lambda: _complete(14, 14, 3), (13, 128)),
    "knn37-P1": (lambda: _knn(37, 7, 37, 1), (1, 5, 6)),
    "knn37-P4": (lambda: _knn(37, 7, 37, 4), (5,)),
    "knn37-zero": (lambda: _knn(37, 7, 37, 2, heat="zero"), (6,)),
    "hub200": (lambda: _hub(200, 2, 200, 2), (8, 128)),
    "hub1100": (lambda: _hub(1100, 1, 1100, 2), (5,)),
    "empty-rows": (_empty_rows, (4,)),
    "duplicates": (_duplicates, (6,)),
    "corners": (_corners, (5,)),
    "saturated": (_saturated, (9,)),
}
PAIRS = [(name, K) for name, (_, Ks) in CASES.items() for K in Ks]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def expected(name, K):
    """The emulation's (lists, listed, pads)."""
    pts, rp, col, heat = case(name)
    return E.lists(pts, rp, col, heat, K)


def edge_index_of(rp, col):
    """[2, E] of a CSR: the row of every entry over its column."""
    return np.stack([E.rows_of(rp), np.asarray(col, dtype=np.int64)]).astype(np.int64)


def permuted(name, seed=0):
    """The case with the entries of every row permuted and the tours reversed: the same graph and heat."""
    pts, rp, col, heat = case(name)
    rng = np.random.default_rng(seed)
    order = np.concatenate([rp[u] + rng.permutation(int(rp[u + 1] - rp[u])) for u in range(len(pts))] + [np.zeros(0, dtype=np.int64)])
    order = order.astype(np.int64)
    return pts, rp, col[order], np.ascontiguousarray(heat[::-1, order])
