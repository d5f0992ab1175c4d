"""CPU restatement of the heat-ranked candidate lists (difusco_amd/csrc/tsp_heat_candidates.hip,
``difusco_tsp_heat_candidates_ragged``; the rule: include/difusco_hip.h) in numpy, on dense n x n tables.  TEST INFRASTRUCTURE
ONLY: nothing in the package imports it.

``lists(points, row_ptr, col, heat, K)`` -> (int32 [n, K] with -1 pads, listed, pads) of ONE group: ``heat`` float32 [P, E] in
the entry order of the CSR.  ``csr(n, rows, cols)`` turns a row-sorted COO into ``row_ptr``; ``knn_graph`` is the k-NN graph in
(d2, index) order that the zero-heat property speaks of."""
import numpy as np


def quantise(heat):
    """q(e): float32 product, round to nearest even, a NaN counts as 0 (fminf(fmaxf(h, 0), 1) drops it)."""
    h = np.asarray(heat, dtype=np.float32)
    h = np.where(np.isnan(h), np.float32(0), h)
    return np.rint(np.clip(h, np.float32(0), np.float32(1)) * np.float32(65535.0)).astype(np.uint32)


def d2_table(points):
    """d2 = dx dx + dy dy in float64, every operation rounded on its own."""
    p = np.asarray(points, dtype=np.float64)
    d = p[:, None, :] - p[None, :, :]
    sq = d * d
    return sq[..., 0] + sq[..., 1]


def csr(n, rows, cols):
    """(row_ptr int32 [n + 1], col int32 [E]) of a COO whose rows are sorted."""
    rows = np.asarray(rows, dtype=np.int64)
    assert np.all(rows[1:] >= rows[:-1])
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return row_ptr, np.asarray(cols, dtype=np.int32)


def rows_of(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def knn_graph(points, k):
    """The k nearest cities of every city, itself included, in (d2, index) order: (row_ptr, col, d2 table)."""
    d2 = d2_table(points)
    n = len(d2)
    idx = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d2), axis=1)[:, :k]
    row_ptr, col = csr(n, np.repeat(np.arange(n), k), idx.reshape(-1))
    return row_ptr, col, d2


def score_table(n, row_ptr, col, heat):
    """(S int64 [n, n], A bool [n, n]): the score and the candidate relation, diagonal of A cleared."""
    rows, col = rows_of(row_ptr), np.asarray(col, dtype=np.int64)
    heat = np.asarray(heat, dtype=np.float32).reshape(-1, len(col))
    s = np.zeros((n, n), dtype=np.int64)
    for t in range(heat.shape[0]):
        m = np.zeros((n, n), dtype=np.int64)
        np.maximum.at(m, (rows, col), quantise(heat[t]).astype(np.int64))       # q_t(u, v): the largest over the duplicates
        s += m
    adj = np.zeros((n, n), dtype=bool)
    adj[rows, col] = True
    A = adj | adj.T
    np.fill_diagonal(A, False)
    return s + s.T, A


def lists(points, row_ptr, col, heat, K):
    n = len(points)
    d2 = d2_table(points)
    S, A = score_table(n, row_ptr, col, heat)
    out = -np.ones((n, K), dtype=np.int32)
    listed = 0
    for a in range(n):
        c = np.nonzero(A[a])[0]
        order = c[np.lexsort((c, d2[a, c], -S[a, c]))][:K]                      # (S descending, d2 ascending, b ascending)
        out[a, :len(order)] = order
        listed += int((S[a, order] > 0).sum())
    return out, listed, int((out < 0).sum())
