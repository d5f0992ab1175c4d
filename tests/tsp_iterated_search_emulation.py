"""CPU restatement of the iterated multi-move local search (difusco_amd/csrc/or_opt_multi.hip,
``difusco_tsp_iterated_search_ragged``; the rule: include/difusco_hip.h) in numpy, on top of
``multi_local_search_emulation.search_tour`` and ``philox_reference.philox4x32_10``.  TEST INFRASTRUCTURE ONLY.

Every tour runs on its own, with a Philox key ``seed`` and a first offset ``offset``:

1. the incumbent I is ``search_tour`` of the input tour;
2. kick t = 0 .. kicks-1: with ``Lc = min(span, (n-1) // 2)``, draw c = 0 .. kick_size-1 takes the words w0, w1, w2 of
   ``philox4x32_10(seed, offset + t, c)`` and sets ``l1 = 1 + w1 % Lc``, ``l2 = 1 + w2 % Lc``, ``a = 1 + w0 % (n - l1 - l2)``,
   ``b = a + l1 + l2``; in rising c a draw is kept iff ``[a, b)`` intersects the range of no kept draw before it; a kept draw
   sets ``C[a:b] = I[a+l1:b] ++ I[a:a+l1]``;
3. C is descended with ``search_tour`` (fresh caps);
4. I <- C iff ``tour_length(C) <= tour_length(I)``, the length summed in ONE association (``tour_length`` below).

Deliberately simple: python loops over draws and kicks."""
import numpy as np

import multi_local_search_emulation as E
from or_opt_emulation import dist
from philox_reference import philox4x32_10

PARTS = 1024
MASK64 = (1 << 64) - 1
COUNTERS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves")


def tour_length(points, tour):
    """The length of the closed tour in the association of the kernel: d_k = |P_k P_k+1| (two products, one sum, one square
    root); 1024 strided partial sums, each accumulated in rising k from 0.0; then a halving tree over the partial sums."""
    P = np.asarray(points, dtype=np.float64)[np.asarray(tour, dtype=np.int64)]
    d = dist(P[:-1], P[1:])
    rows = -(-len(d) // PARTS)
    padded = np.zeros(rows * PARTS)                              # x + 0.0 is x: a missing term changes no bit
    padded[:len(d)] = d
    s = np.zeros(PARTS)
    for row in padded.reshape(rows, PARTS):
        s = s + row
    h = PARTS // 2
    while h:
        s = s[:h] + s[h:2 * h]
        h //= 2
    return float(s[0])


def kick_draws(seed, offset, t, n, kick_size, span):
    """The draws ``(a, l1, l2)`` of kick ``t`` of a tour of n nodes, c = 0 .. kick_size-1, python ints."""
    Lc = min(int(span), (n - 1) // 2)
    out = []
    for c in range(kick_size):
        w0, w1, w2, _ = (int(x) for x in philox4x32_10(int(seed) & MASK64, (int(offset) + t) & MASK64, c))
        l1, l2 = 1 + w1 % Lc, 1 + w2 % Lc
        out.append((1 + w0 % (n - l1 - l2), l1, l2))
    return out


def apply_kick(tour, draws):
    """The kicked copy of ``tour`` and the kept flag of every draw."""
    I = np.asarray(tour, dtype=np.int64)
    C = I.copy()
    ranges, kept = [], []
    for a, l1, l2 in draws:
        b = a + l1 + l2
        assert 1 <= a and b <= len(I) - 1 and l1 >= 1 and l2 >= 1
        ok = all(not (a < kb and ka < b) for ka, kb in ranges)
        kept.append(ok)
        if ok:
            ranges.append((a, b))
            C[a:b] = np.concatenate([I[a + l1:b], I[a:a + l1]])
    return C, kept


def search_tour(points, tour, seed=0, offset=0, *, kicks=0, kick_size=16, span=30, max_iterations=1000, max_rounds=16,
                select_rounds=4, draws=None, trace=None):
    """The iterated search of ONE tour.  Returns ``(tour int64 [n + 1], counters, per)``: ``counters`` as
    ``multi_local_search_emulation.search_tour`` (sweeps and moves summed over the descents, ``rounds`` the most rounds of a
    descent), ``per`` = dict of ``kicks_kept``, ``kicks_improved``, ``segments_swapped``, ``first_length``, ``final_length``.
    ``draws`` (a function of t) replaces the Philox draws; ``trace`` (a list) receives ``(kicked tour, descended tour, its
    length, taken)`` of every kick."""
    pts = np.asarray(points, dtype=np.float64)
    n = len(tour) - 1
    I, c = E.search_tour(pts, tour, max_iterations, max_rounds, select_rounds)
    length = tour_length(pts, I)
    per = {"kicks_kept": 0, "kicks_improved": 0, "segments_swapped": 0, "first_length": length, "final_length": length}
    for t in range(kicks):
        d = draws(t) if draws is not None else kick_draws(seed, offset, t, n, kick_size, span)
        K, kept = apply_kick(I, d)
        per["segments_swapped"] += sum(kept)
        C, cc = E.search_tour(pts, K, max_iterations, max_rounds, select_rounds)
        for k in COUNTERS:
            c[k] = max(c[k], cc[k]) if k == "rounds" else c[k] + cc[k]
        lc = tour_length(pts, C)
        take = lc <= length
        if trace is not None:
            trace.append((K, C, lc, take))
        if take:
            per["kicks_kept"] += 1
            per["kicks_improved"] += lc < length
            I, length = C, lc
    per["final_length"] = length
    return I, c, per


def iterated_search(points, tours, seeds, offsets, **kw):
    """The search of one group (tours int [P, n + 1], seeds / offsets [P]).  Returns ``(tours int64 [P, n + 1], counters,
    per)``: the counters combined over the tours as ``multi_local_search_emulation.multi_local_search`` does, ``per`` a dict of
    lists [P]."""
    out, cs, ps = [], [], []
    for t, s, o in zip(np.asarray(tours), seeds, offsets):
        a, c, p = search_tour(points, t, s, o, **kw)
        out.append(a)
        cs.append(c)
        ps.append(p)
    counters = {k: (max if k in ("two_opt_sweeps", "or_opt_sweeps", "rounds") else sum)(c[k] for c in cs) for k in cs[0]}
    return np.stack(out), counters, {k: [p[k] for p in ps] for k in ps[0]}
