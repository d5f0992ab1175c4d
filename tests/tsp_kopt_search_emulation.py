"""CPU restatement of the heatmap-guided sampled k-opt search (difusco_amd/csrc/tsp_kopt_search.hip,
``difusco_tsp_kopt_search_ragged``; the rule: include/difusco_hip.h) in python floats and ints, on top of ``philox_reference``
and the tour length of ``tsp_iterated_search_emulation``.  TEST INFRASTRUCTURE ONLY.

A tour carries an incumbent I, per candidate entry of its group's CSR graph a weight ``w`` (100 x the clamped heat at first) and
a count ``C``, per city the row sum ``sw``.  Every round, S simulations read that state as it stood at the start of the round:
each opens the tour at a drawn position, then up to D times draws a new edge from the head of the open path among the PROMISING
candidate entries (weight over the row average plus an exploration term, at least 1) and reverses the path prefix that closes
it.  The best closing gain of the round, ties to the lowest simulation, is applied if it is above 1e-6, and the weights of the
edges it added grow.  A tour stops after ``max_rounds`` rounds or ``patience * n`` simulations in a row without an applied action.

Deliberately simple: python loops, an explicit path list per simulation, dictionaries for the entries.  Python float arithmetic
is IEEE float64 with correctly rounded + - * / and ``math.sqrt``, which is what the rule asks for."""
import math

import numpy as np

from philox_reference import philox4x32_10
from tsp_iterated_search_emulation import tour_length

MASK64 = (1 << 64) - 1
IMPROVE = 1e-6
PER_TOUR = ("rounds", "actions", "depth_sum", "reverted", "first_length", "final_length")


def explore_table(alpha, samples, rounds):
    """What the Python layer passes as ``explore``: ``alpha * sqrt(log1p(r * S))``, float64 [rounds]."""
    return np.array([alpha * math.sqrt(math.log1p(r * samples)) for r in range(rounds)], dtype=np.float64)


def clamp_weight(h):
    """``100.0 * (double) fminf(fmaxf(h, 0), 1)``: a NaN counts as 0."""
    c = np.fmin(np.fmax(np.float32(h), np.float32(0.0)), np.float32(1.0))
    return 100.0 * float(c)


def candidates(row_ptr, col):
    """Per city the candidate entries of its row in rising e: ``col[e] != u`` and no earlier entry of the row has that column."""
    rp = [int(v) for v in row_ptr]
    out = []
    for u in range(len(rp) - 1):
        seen, row = set(), []
        for e in range(rp[u], rp[u + 1]):
            c = int(col[e])
            if c != u and c not in seen:
                row.append(e)
            seen.add(c)
        out.append(row)
    return out


def dist(P, a, b):
    dx, dy = P[a][0] - P[b][0], P[a][1] - P[b][1]
    return math.sqrt(dx * dx + dy * dy)


def step_word(words, i, s):
    """The word of step ``i`` of simulation ``s``: word ``i mod 4`` of call ``i div 4`` (``words[j]`` holds call j, [S, 4])."""
    return int(words[i // 4][s, i % 4])


def round_words(seed, offset, r, samples, depth):
    """The Philox calls of round ``r``: key ``seed``, offset ``offset + r`` modulo 2^64, call j at index ``(j << 32) | s``."""
    off = (int(offset) + r) & MASK64
    s = np.arange(samples, dtype=np.uint64)
    return [philox4x32_10(int(seed) & MASK64, off, (np.uint64(j) << np.uint64(32)) | s) for j in range(depth // 4 + 1)]


class State:
    """The state of one tour."""

    def __init__(self, points, tour, row_ptr, col, heat):
        self.P = [(float(x), float(y)) for x, y in np.asarray(points, dtype=np.float64)]
        self.n = len(tour) - 1
        self.I = [int(c) for c in tour[:-1]]
        self.col = [int(c) for c in col]
        self.cand = candidates(row_ptr, col)
        self.w = {e: clamp_weight(heat[e]) for row in self.cand for e in row}
        self.C = {e: 0 for row in self.cand for e in row}
        self.entry = {(u, self.col[e]): e for u, row in enumerate(self.cand) for e in row}
        self.sw = []
        for row in self.cand:
            s = 0.0
            for e in row:
                s = s + self.w[e]
            self.sw.append(s)
        self.length = tour_length(points, list(self.I) + [self.I[0]])


def simulate(st, s, words, depth, explore_r):
    """One simulation on the frozen state.  Returns ``(value or None, i*, steps)``: ``steps`` lists, per step taken,
    ``(entry, b_i, c, y, path after the step)``."""
    n, P = st.n, st.P
    p = step_word(words, 0, s) % n
    a1 = st.I[p]
    path = [st.I[(p + 1 + x) % n] for x in range(n)]
    gain = dist(P, a1, path[0])
    best, best_i, steps = None, 0, []
    for i in range(1, depth + 1):
        b = path[0]
        avg = st.sw[b] / float(n - 1)
        if not avg > 0:
            break
        promising = []
        for e in st.cand[b]:
            c = st.col[e]
            if c == a1 or c == path[1]:
                continue
            pot = st.w[e] / avg + explore_r / math.sqrt(float(st.C[e] + 1))
            if pot >= 1.0:
                promising.append((e, pot))
        if not promising:
            break
        tot = 0.0
        for _, pot in promising:
            tot = tot + pot
        draw = step_word(words, i, s) % 1000
        cum, chosen = 0, None
        for k, (e, pot) in enumerate(promising):
            cum = 1000 if k == len(promising) - 1 else cum + int((1000.0 * pot) / tot)
            if draw < cum:
                chosen = e
                break
        c = st.col[chosen]
        y = path.index(c)
        assert 2 <= y <= n - 2
        nb = path[y - 1]
        gain = gain - dist(P, b, c) + dist(P, c, nb)
        real = gain - dist(P, nb, a1)
        path = path[:y][::-1] + path[y:]
        assert path[0] == nb and path[-1] == a1
        steps.append((chosen, b, c, y, list(path)))
        if best is None or real > best:
            best, best_i = real, i
        if real > IMPROVE:
            break
    return best, best_i, steps


def search_tour(points, tour, row_ptr, col, heat, seed=0, offset=0, *, samples=64, depth=10, max_rounds=0, patience=10, beta=10.0,
                explore=None, alpha=1.0, log=None):
    """The search of ONE tour.  ``explore``: float64 [max_rounds] (default: ``explore_table(alpha, samples, max_rounds)``).
    Returns ``(tour int64 [n + 1], per)`` with ``per`` the six values of ``PER_TOUR``.  ``log`` (a list) receives, per applied
    action, ``(round, s, value, i*, p, incumbent before, steps, incumbent after, length before, length after)``."""
    tour = [int(c) for c in tour]
    n = len(tour) - 1
    assert n >= 4 and tour[-1] == tour[0]
    ex = explore_table(alpha, samples, max_rounds) if explore is None else np.asarray(explore, dtype=np.float64)
    assert len(ex) >= max_rounds
    st = State(points, tour, row_ptr, col, heat)
    first = st.length
    per = {"rounds": 0, "actions": 0, "depth_sum": 0, "reverted": 0, "first_length": first, "final_length": first}
    stall = 0
    for r in range(max_rounds):
        words = round_words(seed, offset, r, samples, depth)
        sims = [simulate(st, s, words, depth, float(ex[r])) for s in range(samples)]
        per["rounds"] += 1
        for _, _, steps in sims:                                     # the counts, after every simulation has read them
            for e, b, c, _, _ in steps:
                st.C[e] += 1
                m = st.entry.get((c, b))
                if m is not None:
                    st.C[m] += 1
        best, best_s = None, -1
        for s, (v, _, _) in enumerate(sims):
            if v is not None and (best is None or v > best):
                best, best_s = v, s
        if best is not None and best > IMPROVE:
            _, istar, steps = sims[best_s]
            p = step_word(words, 0, best_s) % n
            before = list(st.I)
            a1 = before[p]
            path = steps[istar - 1][4]
            z = path.index(tour[0])
            st.I = [path[(z + k) % n] for k in range(n)]
            x = best / st.length
            inc = beta * (x + (0.5 * x) * x)
            added = [(b, c) for _, b, c, _, _ in steps[:istar]] + [(path[0], a1)]
            for u, v in added:
                for a, b in ((u, v), (v, u)):
                    e = st.entry.get((a, b))
                    if e is not None:
                        st.w[e] = st.w[e] + inc
                    st.sw[a] = st.sw[a] + inc
            old = st.length
            st.length = tour_length(points, st.I + [st.I[0]])
            stall = 0
            per["actions"] += 1
            per["depth_sum"] += istar
            if log is not None:
                log.append((r, best_s, best, istar, p, before, steps[:istar], list(st.I), old, st.length))
        else:
            stall += samples
            if stall >= patience * n:
                break
    out = st.I + [st.I[0]]
    if st.length > first:
        per["reverted"], out = 1, tour
    else:
        per["final_length"] = st.length
    return np.asarray(out, dtype=np.int64), per


def kopt_search(points, tours, row_ptr, col, heats, seeds, offsets, **kw):
    """The search of one group (tours int [P, n + 1], heats [P, E], seeds / offsets [P]).  Returns ``(tours int64 [P, n + 1],
    dict of lists [P])``."""
    out, ps = [], []
    for t, h, s, o in zip(np.asarray(tours), heats, seeds, offsets):
        a, p = search_tour(points, t, row_ptr, col, h, s, o, **kw)
        out.append(a)
        ps.append(p)
    return np.stack(out), {k: [p[k] for p in ps] for k in PER_TOUR}
