"""CPU restatement of the windowed iterated search (difusco_amd/csrc/tsp_window_search.hip, ``difusco_tsp_window_search_ragged``;
the rule: include/difusco_hip.h) in numpy, on top of ``tsp_iterated_search_emulation.search_tour`` and
``multi_local_search_emulation.search_tour``.  TEST INFRASTRUCTURE ONLY.

Every tour runs on its own, with a Philox key ``seed`` and a first offset ``offset``:

1. T is ``multi_local_search_emulation.search_tour`` of the input tour;
2. pass r = 0 .. passes-1: the cuts are 0, n and every ``o + w W`` strictly between them, ``o = 0`` on even passes and
   ``W // 2`` on odd ones.  Window w is the open path ``T[c_w .. c_w+1]`` of ``m = c_w+1 - c_w`` edges; with ``m < 8`` it is
   copied, else it is ``tsp_iterated_search_emulation.search_tour`` of that path (which indexes ``points[path]`` by position and
   never moves its two end positions, so it takes an open path as it is) with ``kicks`` kicks at the first offset
   ``offset + (r C + w) kicks``, ``C = ceil(n / W) + 1``.  The candidate is the windows' results one after the other; it
   replaces T iff ``tour_length(candidate) <= tour_length(T)``;
3. one closing ``multi_local_search_emulation.search_tour`` of T, kept iff not longer.

Deliberately simple: python loops over passes and windows."""
import numpy as np

import multi_local_search_emulation as E
import tsp_iterated_search_emulation as T

SKIP = 8
GROUP_COUNTERS = T.COUNTERS


def cuts(n, window, r):
    """The cuts ``c_0 = 0 < .. < c_M = n`` of pass r."""
    o = 0 if r % 2 == 0 else window // 2
    inner = [c for c in range(o, n, window) if 0 < c < n]
    return [0] + inner + [n]


def search_tour(points, tour, seed=0, offset=0, *, window, passes=1, kicks=0, kick_size=16, span=30, max_iterations=1000,
                max_rounds=16, select_rounds=4, trace=None):
    """The windowed search of ONE tour.  Returns ``(tour int64 [n + 1], first, closing, per)``: ``first`` / ``closing`` the
    counters of the first and the closing descent, ``per`` = dict of ``first_length``, ``final_length``, ``passes_kept``,
    ``windows_searched``, ``kicks_kept``, ``kicks_improved``, ``segments_swapped``, ``window_sweeps``, ``window_moves``,
    ``closing_sweeps``.  ``trace`` (a list) receives ``(candidate, its length, taken)`` of every pass."""
    pts = np.asarray(points, dtype=np.float64)
    n = len(tour) - 1
    cur, first = E.search_tour(pts, tour, max_iterations, max_rounds, select_rounds)
    length = T.tour_length(pts, cur)
    per = {"first_length": length, "final_length": length, "passes_kept": 0, "windows_searched": 0, "kicks_kept": 0,
           "kicks_improved": 0, "segments_swapped": 0, "window_sweeps": 0, "window_moves": 0, "closing_sweeps": 0}
    C = -(-n // window) + 1
    for r in range(passes):
        c = cuts(n, window, r)
        cand = cur.copy()
        for w in range(len(c) - 1):
            lo, hi = c[w], c[w + 1]
            if hi - lo < SKIP:
                continue
            path, cc, pp = T.search_tour(pts, cur[lo:hi + 1], seed, int(offset) + (r * C + w) * kicks, kicks=kicks,
                                         kick_size=kick_size, span=span, max_iterations=max_iterations, max_rounds=max_rounds,
                                         select_rounds=select_rounds)
            assert path[0] == cur[lo] and path[-1] == cur[hi]
            cand[lo:hi + 1] = path
            per["windows_searched"] += 1
            for k in ("kicks_kept", "kicks_improved", "segments_swapped"):
                per[k] += int(pp[k])
            per["window_sweeps"] += cc["two_opt_sweeps"] + cc["or_opt_sweeps"]
            per["window_moves"] += cc["two_opt_moves"] + cc["or_opt_moves"]
        lc = T.tour_length(pts, cand)
        take = lc <= length
        if trace is not None:
            trace.append((cand, lc, take))
        if take:
            cur, length = cand, lc
            per["passes_kept"] += 1
    closed, closing = E.search_tour(pts, cur, max_iterations, max_rounds, select_rounds)
    per["closing_sweeps"] = closing["two_opt_sweeps"] + closing["or_opt_sweeps"]
    lc = T.tour_length(pts, closed)
    if lc <= length:
        cur, length = closed, lc
    per["final_length"] = length
    return cur, first, closing, per


def window_search(points, tours, seeds, offsets, **kw):
    """The search of one group (tours int [P, n + 1], seeds / offsets [P]).  Returns ``(tours int64 [P, n + 1], counters,
    per)``: the group counters are those of the first descent combined over the tours as
    ``multi_local_search_emulation.multi_local_search`` does, plus those of the closing descent combined in the same way (the
    rounds: the larger of the two); ``per`` a dict of lists [P]."""
    out, fs, cs, ps = [], [], [], []
    for t, s, o in zip(np.asarray(tours), seeds, offsets):
        a, f, c, p = search_tour(points, t, s, o, **kw)
        out.append(a)
        fs.append(f)
        cs.append(c)
        ps.append(p)
    counters = {}
    for k in GROUP_COUNTERS:
        if k in ("two_opt_sweeps", "or_opt_sweeps"):
            counters[k] = max(f[k] for f in fs) + max(c[k] for c in cs)
        elif k == "rounds":
            counters[k] = max(max(f[k] for f in fs), max(c[k] for c in cs))
        else:
            counters[k] = sum(f[k] for f in fs) + sum(c[k] for c in cs)
    return np.stack(out), counters, {k: [p[k] for p in ps] for k in ps[0]}


def lattice_instance(n, s):
    """The first n points of the smallest integer grid that holds them, row by row, and a random-permutation start: many equal
    changes and deltas, at any n."""
    k = int(np.ceil(np.sqrt(n)))
    rng = np.random.default_rng(9000 + 10 * n + s)
    g = np.arange(k, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    tour = np.array([0] + list(rng.permutation(n - 1) + 1) + [0], dtype=np.int64)
    return pts, tour
