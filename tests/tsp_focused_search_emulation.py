"""CPU restatement of the iterated multi-move local search with FOCUSED descents after the kicks
(difusco_amd/csrc/or_opt_multi.hip, ``difusco_tsp_focused_search_ragged``; the rule: include/difusco_hip.h) in numpy, on top of
``multi_local_search_emulation`` and ``tsp_iterated_search_emulation``.  TEST INFRASTRUCTURE ONLY.

The search of ``tsp_iterated_search_emulation.search_tour`` except that

* the descent after a kick evaluates only candidates next to a MARKED edge.  A tour keeps two sets of cities, S (current) and T
  (touched since the kick); position k = 0 .. n-1 is ACTIVE iff ``tour[k]`` and ``tour[k+1]`` are both in S.  After a kick T is the
  six end cities of the three new edges of every kept draw.  A phase begins with S := T.  A 2-opt sweep evaluates (i, j) iff
  position i or position j is active; an Or-opt sweep evaluates (v, i, j) iff one of the positions i .. i+3 (clipped to n-1) or
  position j is active.  Everything else of a sweep is ``multi_local_search_emulation``'s.  After a sweep, with the tour as it was
  before the moves, S := the end cities of the removed edges of EVERY proposal and T := T + those of the winners;
* with kicks > 0 one FULL descent of the incumbent closes the call, kept iff it is not longer; ``closing_sweeps`` are the
  sweeps in which it moved (0: the focused descents missed nothing).

``select_compact`` restates the selection rule per proposal, one against all: what the kernels do when a sweep has few
proposals.  It returns the winners of ``multi_local_search_emulation.select_ranges``."""
import numpy as np

import multi_local_search_emulation as E
import multi_two_opt_emulation as M
import tsp_iterated_search_emulation as I
from or_opt_emulation import THRESHOLD, VARIANTS, apply_or_opt_move

COUNTERS = I.COUNTERS


def select_compact(value, row, a, b, select_rounds):
    """The winners among proposals of key ``(value, row)`` and range ``[a, b)``, as indices into them, per round in key order.
    Per round: a live proposal wins iff no live proposal whose range meets its own has a lower key; the winners leave; live
    proposals that meet a winner are dropped.  Python loops, one proposal against all."""
    m = len(row)
    key = [(float(value[p]), int(row[p])) for p in range(m)]
    meets = lambda p, q: a[p] < b[q] and a[q] < b[p]
    live = [True] * m
    winners = []
    for _ in range(select_rounds):
        if not any(live):
            break
        won = [p for p in range(m) if live[p] and not any(live[q] and meets(p, q) and key[q] < key[p] for q in range(m))]
        for p in won:
            live[p] = False
        for p in range(m):
            if live[p] and any(meets(p, q) for q in won):
                live[p] = False
        winners.extend(sorted(won, key=lambda p: key[p]))
    return winners


def _select(value, row, a, b, select_rounds, compact_select_max):
    if len(row) <= compact_select_max:
        return select_compact(value, row, a, b, select_rounds)
    return E.select_ranges(value, row, a, b, select_rounds)


def active_positions(tour, S):
    """bool [n]: position k is active iff both its cities are in S (bool [n] over the cities)."""
    t = np.asarray(tour, dtype=np.int64)
    return S[t[:-1]] & S[t[1:]]


def row_active(act):
    """bool [n]: row i is row-active iff one of the positions i .. i+3 (clipped to n-1) is active."""
    n = len(act)
    out = act.copy()
    for k in (1, 2, 3):
        out[:n - k] |= act[k:]
    return out


def two_opt_sweep(points, tour, S, select_rounds, compact_select_max=1024, block=256, count=None):
    """One focused 2-opt sweep of one tour.  Returns ``(tour after, winners [(change, i, j)], proposals [(i, j)])``."""
    t = np.array(tour, dtype=np.int64, copy=True)
    n = len(t) - 1
    act = active_positions(t, S)
    cs, js = [], []
    for lo in range(0, n - 2, block):
        hi = min(lo + block, n - 2)
        c = M.row_changes(points, t, lo, hi)
        mask = act[lo:hi, None] | act[None, :]
        c = np.where(mask, c, np.inf)
        if count is not None:
            count[0] += int(np.isfinite(c).sum())
        j = c.argmin(axis=1)                                     # first occurrence = lowest j
        cs.append(c[np.arange(len(j)), j])
        js.append(j)
    c, j = np.concatenate(cs), np.concatenate(js)
    i = np.flatnonzero(c < THRESHOLD)
    c, j = c[i], j[i]
    applied = []
    for w in _select(c, i, i, j + 1, select_rounds, compact_select_max):
        t[i[w] + 1:j[w] + 1] = t[i[w] + 1:j[w] + 1][::-1].copy()
        applied.append((float(c[w]), int(i[w]), int(j[w])))
    return t, applied, list(zip(i.tolist(), j.tolist()))


def or_opt_sweep(points, tour, S, select_rounds, compact_select_max=1024, block=128, count=None):
    """One focused Or-opt sweep of one tour.  Returns ``(tour after, winners [(delta, v, i, j)], proposals [(v, i, j)])``."""
    t = np.array(tour, dtype=np.int64, copy=True)
    n = len(t) - 1
    act = active_positions(t, S)
    ract = row_active(act)
    ds, vs, js = [], [], []
    for lo in range(0, n - 1, block):
        hi = min(lo + block, n - 1)
        c = E.or_opt_row_deltas(points, t, lo, hi)
        mask = ract[lo:hi, None] | act[None, :]
        c = np.where(mask[:, None, :], c, np.inf)
        if count is not None:
            count[0] += int(np.isfinite(c).any(axis=1).sum())
        flat = c.reshape(len(c), -1).argmin(axis=1)              # first occurrence = lowest v, then lowest j
        ds.append(c.reshape(len(c), -1)[np.arange(len(flat)), flat])
        vs.append(flat // n)
        js.append(flat % n)
    delta, v, j = np.concatenate(ds), np.concatenate(vs), np.concatenate(js)
    i = np.flatnonzero(delta < THRESHOLD)
    delta, v, j = delta[i], v[i], j[i]
    a, b = E.or_opt_range(i, v, j)
    applied = []
    for w in _select(delta, i, a, b, select_rounds, compact_select_max):
        t = apply_or_opt_move(t, int(v[w]), int(i[w]), int(j[w]))
        applied.append((float(delta[w]), int(v[w]), int(i[w]), int(j[w])))
    return t, applied, list(zip(v.tolist(), i.tolist(), j.tolist()))


def _ends(kind, move):
    """The positions at the ends of the edges a move removes."""
    if kind == "2opt":
        i, j = move
        return [i, i + 1, j, j + 1]
    v, i, j = move
    L = VARIANTS[v][0]
    return [i, i + 1, i + L, i + L + 1, j, j + 1]


def focused_descent(points, tour, T, max_iterations=1000, max_rounds=16, select_rounds=4, compact_select_max=1024, log=None,
                    count=None):
    """The focused descent of ONE kicked tour; ``T`` (bool [n] over the cities, updated in place) holds the cities the kick
    touched.  Returns ``(tour, counters)`` as ``multi_local_search_emulation.search_tour``.  ``log`` (a list) receives ``(kind,
    proposals, winners)`` of every sweep, the last one of a phase (no proposal) included; ``count`` (a list of one int) is
    advanced by the pairs evaluated."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.array(tour, dtype=np.int64, copy=True)
    c = {"two_opt_sweeps": 0, "or_opt_sweeps": 0, "rounds": 1, "two_opt_moves": 0, "or_opt_moves": 0}
    total = 0
    if max_iterations == 0:
        return t, c
    for r in range(max_rounds):
        c["rounds"] = r + 1
        moved = [0, 0]
        for k, (kind, fn) in enumerate((("2opt", two_opt_sweep), ("oropt", or_opt_sweep))):
            S = T.copy()                                         # a phase begins with S := T
            while True:
                after, applied, props = fn(pts, t, S, select_rounds, compact_select_max, count=count)
                if log is not None:
                    log.append((kind, len(props), len(applied)))
                if not props:                                    # no proposal: the phase ends
                    break
                S = np.zeros_like(T)
                for p in props:
                    S[t[_ends(kind, p)]] = True                  # the tour before the moves
                for w in applied:
                    T[t[_ends(kind, w[1:])]] = True
                t = after
                total += 1
                moved[k] += 1
                c["two_opt_sweeps" if k == 0 else "or_opt_sweeps"] += 1
                c["two_opt_moves" if k == 0 else "or_opt_moves"] += len(applied)
                if total >= max_iterations:
                    return t, c
        if moved[1] == 0:
            break
    return t, c


def kick_marks(kicked, draws, kept):
    """T after a kick: the cities the kicked tour holds at a-1, a, a+l2-1, a+l2, b-1 and b of every kept draw."""
    K = np.asarray(kicked, dtype=np.int64)
    T = np.zeros(len(K) - 1, dtype=bool)
    for (a, l1, l2), ok in zip(draws, kept):
        if ok:
            b = a + l1 + l2
            T[K[[a - 1, a, a + l2 - 1, a + l2, b - 1, b]]] = True
    return T


def search_tour(points, tour, seed=0, offset=0, *, kicks=0, kick_size=16, span=30, max_iterations=1000, max_rounds=16,
                select_rounds=4, compact_select_max=1024, draws=None, log=None, count=None):
    """The focused search of ONE tour.  Returns ``(tour int64 [n + 1], counters, per)`` as
    ``tsp_iterated_search_emulation.search_tour`` (the counters sum all descents, the closing one included); ``per`` gains
    ``closing_sweeps``.  ``log`` / ``count``: those of ``focused_descent``, over all focused descents."""
    pts = np.asarray(points, dtype=np.float64)
    n = len(tour) - 1
    inc, c = E.search_tour(pts, tour, max_iterations, max_rounds, select_rounds)
    length = I.tour_length(pts, inc)
    per = {"kicks_kept": 0, "kicks_improved": 0, "segments_swapped": 0, "first_length": length, "final_length": length,
           "closing_sweeps": 0}

    def add(cc):
        for k in COUNTERS:
            c[k] = max(c[k], cc[k]) if k == "rounds" else c[k] + cc[k]

    for t in range(kicks):
        d = draws(t) if draws is not None else I.kick_draws(seed, offset, t, n, kick_size, span)
        K, kept = I.apply_kick(inc, d)
        per["segments_swapped"] += sum(kept)
        C, cc = focused_descent(pts, K, kick_marks(K, d, kept), max_iterations, max_rounds, select_rounds, compact_select_max,
                                log=log, count=count)
        add(cc)
        lc = I.tour_length(pts, C)
        if lc <= length:
            per["kicks_kept"] += 1
            per["kicks_improved"] += lc < length
            inc, length = C, lc
    if kicks > 0:                                                # the closing full descent, kept iff it is not longer
        C, cc = E.search_tour(pts, inc, max_iterations, max_rounds, select_rounds)
        add(cc)
        per["closing_sweeps"] = cc["two_opt_sweeps"] + cc["or_opt_sweeps"]
        lc = I.tour_length(pts, C)
        if lc <= length:
            inc, length = C, lc
    per["final_length"] = length
    return inc, c, per


def focused_search(points, tours, seeds, offsets, **kw):
    """The search of one group (tours int [P, n + 1], seeds / offsets [P]), combined as
    ``tsp_iterated_search_emulation.iterated_search`` does."""
    out, cs, ps = [], [], []
    for t, s, o in zip(np.asarray(tours), seeds, offsets):
        a, c, p = search_tour(points, t, s, o, **kw)
        out.append(a)
        cs.append(c)
        ps.append(p)
    counters = {k: (max if k in ("two_opt_sweeps", "or_opt_sweeps", "rounds") else sum)(c[k] for c in cs) for k in cs[0]}
    return np.stack(out), counters, {k: [p[k] for p in ps] for k in ps[0]}
