"""CPU restatement of the neighbour-list multi-move 2-opt + Or-opt search (difusco_amd/csrc/or_opt_multi.hip with or_opt_nbr.h,
``difusco_tsp_nbr_local_search_ragged``) in numpy float64.  TEST INFRASTRUCTURE ONLY.  Deltas, ranges, selection and apply are
those of ``multi_local_search_emulation``, the 2-opt neighbour sweep is ``nbr_two_opt_emulation.sweep``; this file adds the
candidate mask of an Or-opt neighbour sweep, the per-tour stage and the counters.

``neighbors`` is int [n, K] with the pads of ``nbr_two_opt_emulation``; ``S[x, y]`` iff ``y in N(x)`` or ``x in N(y)``.  For the
Or-opt candidate ``(v, i, j)``, ``(L, reversed) = VARIANTS[v]``, let ``a`` and ``b`` be the cities at positions ``i+1`` and
``i+L``, swapped when reversed: the move creates the edges ``(tour[j], a)`` and ``(b, tour[j+1])`` (``tour[n] == tour[0]``).
Column ``j`` is a candidate of ``(v, i)`` iff ``S[tour[j], a]`` or ``S[tour[j+1], b]``.  A neighbour sweep is an Or-opt sweep of
``multi_local_search_emulation`` whose rows see their candidates only.

Every tour runs on its own.  Neighbour stage: the rounds of ``multi_local_search_emulation.search_tour`` with neighbour sweeps in
both phases.  A round whose Or-opt phase applied nothing ends the stage: the tour is done (``closing`` false) or goes on, under
the same round number, with a full 2-opt phase and a full Or-opt phase, and full rounds after them until the Or-opt phase of one
applies nothing.  ``max_iterations`` (sweeps in which the tour moved) and ``max_rounds`` (rounds started) count over both stages.

This file computes the full delta table of a block of rows and masks it with the dense [n, n] matrix of listed pairs: quadratic,
and obviously the rule.  It does not walk the lists the way the kernels do."""
import numpy as np

import multi_local_search_emulation as M
import nbr_two_opt_emulation as N2
from or_opt_emulation import THRESHOLD, VARIANTS, apply_or_opt_move

all_others, knn_lists, listed = N2.all_others, N2.knn_lists, N2.listed

COUNTERS = ("two_opt_sweeps", "or_opt_sweeps", "rounds", "two_opt_moves", "or_opt_moves", "full_sweeps", "full_rounds")


def or_candidate_mask(S, tour, lo, hi):
    """bool [hi - lo, 5, n]: the candidate columns of ``(v, i)`` for rows ``lo <= i < hi`` of the closed tour; rows on which
    variant v does not fit (``i > n-1-L``) are all False."""
    t = np.asarray(tour, dtype=np.int64)
    n = len(t) - 1
    out = np.zeros((hi - lo, len(VARIANTS), n), dtype=bool)
    for v, (L, rev) in enumerate(VARIANTS):
        i = np.arange(lo, min(hi, n - L))                        # i <= n - 1 - L
        if len(i) == 0:
            continue
        a, b = (t[i + L], t[i + 1]) if rev else (t[i + 1], t[i + L])
        out[:len(i), v] = S[t[:n][None, :], a[:, None]] | S[t[1:][None, :], b[:, None]]
    return out


def or_opt_proposals(points, tour, S, block=128):
    """The row proposals of one Or-opt neighbour sweep: ``(delta float64 [m], i, v, j int64 [m])``, rows rising."""
    n = len(tour) - 1
    ds, vs, js = [], [], []
    for lo in range(0, n - 1, block):
        hi = min(lo + block, n - 1)
        c = np.where(or_candidate_mask(S, tour, lo, hi), M.or_opt_row_deltas(points, tour, lo, hi), np.inf)
        flat = c.reshape(len(c), -1).argmin(axis=1)              # first occurrence = lowest v, then lowest j
        ds.append(c.reshape(len(c), -1)[np.arange(len(flat)), flat])
        vs.append(flat // n)
        js.append(flat % n)
    delta, v, j = np.concatenate(ds), np.concatenate(vs), np.concatenate(js)
    rows = np.flatnonzero(delta < THRESHOLD)
    return delta[rows], rows, v[rows], j[rows]


def or_opt_sweep(points, tour, select_rounds, S=None):
    """One Or-opt sweep of one tour, the rows seeing their candidates only (``S`` None: the full sweep).  Returns what
    ``multi_local_search_emulation.or_opt_sweep`` returns."""
    if S is None:
        return M.or_opt_sweep(points, tour, select_rounds)
    delta, i, v, j = or_opt_proposals(points, tour, S)
    a, b = M.or_opt_range(i, v, j)
    t = np.array(tour, dtype=np.int64, copy=True)
    applied = []
    for w in M.select_ranges(delta, i, a, b, select_rounds):
        t = apply_or_opt_move(t, int(v[w]), int(i[w]), int(j[w]))
        applied.append((float(delta[w]), int(v[w]), int(i[w]), int(j[w])))
    return t, applied, len(i)


def search_tour(points, tour, neighbors, closing=True, max_iterations=1000, max_rounds=16, select_rounds=4, log=None):
    """The search of ONE tour.  Returns ``(tour int64 [n + 1], counters)``, counters = a dict of ``COUNTERS``.  ``log`` (a list)
    receives ``(stage, kind, tour before, winners)`` of every sweep that moved the tour: stage "nbr" or "full", kind "2opt" or
    "oropt"."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.array(tour, dtype=np.int64, copy=True)
    c = dict.fromkeys(COUNTERS, 0)
    c["rounds"] = 1
    if max_iterations == 0:
        return t, c
    L = listed(neighbors, len(pts))
    S = L | L.T
    total, r, full = 0, 0, False
    while True:
        c["rounds"] = r + 1
        or_moved = False
        mask = None if full else S
        for kind, fn in (("2opt", N2.sweep), ("oropt", or_opt_sweep)):
            while True:
                after, applied, _ = fn(pts, t, select_rounds, mask)
                if not applied:                                  # no proposal: the phase ends
                    break
                if log is not None:
                    log.append(("full" if full else "nbr", kind, t.copy(), applied))
                t = after
                total += 1
                c["full_sweeps"] += full
                c["two_opt_sweeps" if kind == "2opt" else "or_opt_sweeps"] += 1
                c["two_opt_moves" if kind == "2opt" else "or_opt_moves"] += len(applied)
                or_moved |= kind == "oropt"
                if total >= max_iterations:
                    return t, c
        if not full and not or_moved and closing:                # the neighbour stage ends: full phases under this round
            full = True
            c["full_rounds"] = 1
            continue
        if not or_moved or r + 1 >= max_rounds:
            return t, c
        r += 1
        c["full_rounds"] += full


def nbr_local_search(points, tours, neighbors, closing=True, max_iterations=1000, max_rounds=16, select_rounds=4):
    """The search of one group (tours int [P, n + 1], neighbors int [n, K]).  Returns ``(tours int64 [P, n + 1], counters)``:
    the sweeps and rounds are the maxima over the tours, the moves the sums."""
    out, cs = [], []
    for t in np.asarray(tours):
        a, c = search_tour(points, t, neighbors, closing, max_iterations, max_rounds, select_rounds)
        out.append(a)
        cs.append(c)
    counters = {k: (sum if k in ("two_opt_moves", "or_opt_moves") else max)(c[k] for c in cs) for k in COUNTERS}
    return np.stack(out), counters
