"""CPU restatement of the HEAT-BIASED kicks of the iterated TSP search (difusco_amd/csrc/or_opt_heat.h,
``difusco_tsp_guided_search_ragged``; the rule: include/difusco_hip.h) in numpy, on top of ``tsp_iterated_search_emulation``,
``tsp_focused_search_emulation`` and ``philox_reference``.  TEST INFRASTRUCTURE ONLY.

Everything is the iterated search's (``descent="full"``) or the focused search's (``descent="focused"``) except how draw c of
kick t gets ``a``.  The group carries a directed graph in CSR (``row_ptr`` [n + 1], ``col`` [E]; any degrees, duplicates and self
edges allowed), the tour one ``heat`` float32 [E]:

* ``q(e) = rint(clamp(heat_e, 0, 1) * 65535)`` in float32, a NaN counts as 0; ``q(u, v)`` = the largest q(e) over the entries of
  row u with ``col[e] == v``, 0 if there is none;
* with the incumbent I when the kick is drawn, ``w_k = 65536 - max(q(I[k], I[k+1]), q(I[k+1], I[k]))``, ``W_0 = 0``,
  ``W_k+1 = W_k + w_k`` (python ints);
* ``l1``, ``l2`` from w1, w2 as before, ``M = n - l1 - l2``, ``r = (w0 << 32 | w3) % W_M``, p with ``W_p <= r < W_p+1``,
  ``a = p + 1``.

Deliberately simple: python ints and loops, no prefix-sum tricks."""
import bisect

import numpy as np

import multi_local_search_emulation as E
import tsp_focused_search_emulation as F
import tsp_iterated_search_emulation as I
from philox_reference import philox4x32_10

MASK64 = I.MASK64
COUNTERS = I.COUNTERS


def quantise(heat):
    """``q(e)`` of every entry: uint32 numpy array."""
    h = np.asarray(heat, dtype=np.float32)
    c = np.fmin(np.fmax(h, np.float32(0.0)), np.float32(1.0))       # fmax / fmin drop a NaN: it counts as 0
    return np.rint(c * np.float32(65535.0)).astype(np.uint32)


def edge_table(row_ptr, col, heat):
    """dict ``(u, v) -> q(u, v)`` of the entries of the graph (an absent pair has q = 0)."""
    rp, cl, q = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64), quantise(heat)
    assert rp[0] == 0 and rp[-1] == len(cl) == len(q) and (np.diff(rp) >= 0).all()
    table = {}
    for u in range(len(rp) - 1):
        for e in range(rp[u], rp[u + 1]):
            key = (u, int(cl[e]))
            table[key] = max(table.get(key, 0), int(q[e]))
    return table


def position_weights(tour, table):
    """``w_k``, k = 0 .. n-1, of the closed tour: python ints in 1 .. 65536."""
    t = [int(c) for c in tour]
    return [65536 - max(table.get((t[k], t[k + 1]), 0), table.get((t[k + 1], t[k]), 0)) for k in range(len(t) - 1)]


def prefix(weights):
    W = [0]
    for w in weights:
        W.append(W[-1] + w)
    return W


def heat_kick_draws(seed, offset, t, n, kick_size, span, W):
    """The draws ``(a, l1, l2)`` of kick ``t`` under the running weights ``W`` [n + 1] of the incumbent."""
    Lc = min(int(span), (n - 1) // 2)
    out = []
    for c in range(kick_size):
        w0, w1, w2, w3 = (int(x) for x in philox4x32_10(int(seed) & MASK64, (int(offset) + t) & MASK64, c))
        l1, l2 = 1 + w1 % Lc, 1 + w2 % Lc
        M = n - l1 - l2
        r = ((w0 << 32) | w3) % W[M]
        p = bisect.bisect_right(W, r, 0, M + 1) - 1                  # W_p <= r < W_p+1
        assert 0 <= p < M and W[p] <= r < W[p + 1]
        out.append((p + 1, l1, l2))
    return out


def search_tour(points, tour, row_ptr, col, heat, seed=0, offset=0, *, kicks=0, kick_size=16, span=30, max_iterations=1000,
                max_rounds=16, select_rounds=4, descent="full", compact_select_max=1024, draws_log=None):
    """The guided search of ONE tour.  Returns ``(tour int64 [n + 1], counters, per)`` as
    ``tsp_iterated_search_emulation.search_tour`` / ``tsp_focused_search_emulation.search_tour`` (``closing_sweeps`` only when
    focused).  ``draws_log`` (a list) receives the draws of every kick."""
    assert descent in ("full", "focused")
    focused = descent == "focused"
    pts = np.asarray(points, dtype=np.float64)
    n = len(tour) - 1
    table = edge_table(row_ptr, col, heat)
    inc, c = E.search_tour(pts, tour, max_iterations, max_rounds, select_rounds)
    length = I.tour_length(pts, inc)
    per = {"kicks_kept": 0, "kicks_improved": 0, "segments_swapped": 0, "first_length": length, "final_length": length}
    if focused:
        per["closing_sweeps"] = 0

    def add(cc):
        for k in COUNTERS:
            c[k] = max(c[k], cc[k]) if k == "rounds" else c[k] + cc[k]

    for t in range(kicks):
        d = heat_kick_draws(seed, offset, t, n, kick_size, span, prefix(position_weights(inc, table)))
        if draws_log is not None:
            draws_log.append(d)
        K, kept = I.apply_kick(inc, d)
        per["segments_swapped"] += sum(kept)
        if focused:
            C, cc = F.focused_descent(pts, K, F.kick_marks(K, d, kept), max_iterations, max_rounds, select_rounds,
                                      compact_select_max)
        else:
            C, cc = E.search_tour(pts, K, max_iterations, max_rounds, select_rounds)
        add(cc)
        lc = I.tour_length(pts, C)
        if lc <= length:
            per["kicks_kept"] += 1
            per["kicks_improved"] += lc < length
            inc, length = C, lc
    if focused and kicks > 0 and max_iterations > 0:                 # the closing full descent, kept iff it is not longer
        C, cc = E.search_tour(pts, inc, max_iterations, max_rounds, select_rounds)
        add(cc)
        per["closing_sweeps"] = cc["two_opt_sweeps"] + cc["or_opt_sweeps"]
        lc = I.tour_length(pts, C)
        if lc <= length:
            inc, length = C, lc
    per["final_length"] = length
    return np.asarray(inc, dtype=np.int64), c, per


def guided_search(points, tours, row_ptr, col, heats, seeds, offsets, **kw):
    """The search of one group (tours int [P, n + 1], heats [P, E], seeds / offsets [P]), combined as
    ``tsp_iterated_search_emulation.iterated_search`` does."""
    out, cs, ps = [], [], []
    for t, h, s, o in zip(np.asarray(tours), heats, seeds, offsets):
        a, c, p = search_tour(points, t, row_ptr, col, h, s, o, **kw)
        out.append(a)
        cs.append(c)
        ps.append(p)
    counters = {k: (max if k in ("two_opt_sweeps", "or_opt_sweeps", "rounds") else sum)(c[k] for c in cs) for k in cs[0]}
    return np.stack(out), counters, {k: [p[k] for p in ps] for k in ps[0]}


def knn_csr(points, K):
    """The k-NN graph of the tests, self included: row u holds the K nearest cities of u (ties to the lower id)."""
    P = np.asarray(points, dtype=np.float64)
    n = len(P)
    K = min(n, K)
    d = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    col = np.argsort(d, axis=1, kind="stable")[:, :K].astype(np.int32).reshape(-1)
    return np.arange(0, n * K + 1, K, dtype=np.int32), col
