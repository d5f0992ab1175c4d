"""CPU restatement of the neighbour-list multi-move 2-opt (difusco_amd/csrc/two_opt_multi.hip, ``difusco_tsp_nbr_two_opt_ragged``)
in numpy float64.  TEST INFRASTRUCTURE ONLY.  Changes, selection and apply are those of ``multi_two_opt_emulation``; this file
adds the candidate mask of a neighbour sweep, the per-tour phase and the counters.

``neighbors`` is int [n, K]: row ``a`` lists cities; an entry outside ``0 .. n-1`` or equal to ``a`` is a pad.  ``N(a)`` = the
non-pad entries.  Column ``j`` (``i+2 <= j <= n-1``) is a candidate of row ``i`` iff ``tour[j] in N(tour[i])`` or ``tour[i] in
N(tour[j])`` or ``tour[j+1] in N(tour[i+1])`` or ``tour[i+1] in N(tour[j+1])`` (``tour[n] == tour[0]``).  A neighbour sweep is a
``multi_two_opt_emulation.sweep`` whose rows see their candidate columns only.  A tour whose neighbour sweep has no proposal is
done (``closing`` false) or goes on with full sweeps until one has no proposal.  A sweep counts for a group if one of its tours
moved, as a full sweep too if one that moved was in the full phase; the group stops when all tours are done or after
``max_iterations`` counted sweeps.

This file builds the dense [n, n] matrix of listed pairs and masks all changes of a row with it: quadratic, and obviously the
rule."""
import numpy as np

import multi_two_opt_emulation as emu

THRESHOLD = emu.THRESHOLD


def listed(neighbors, n):
    """bool [n, n]: ``L[a, c]`` iff ``c`` is a non-pad entry of city ``a``."""
    nb = np.asarray(neighbors, dtype=np.int64).reshape(n, -1)
    L = np.zeros((n, n), dtype=bool)
    a = np.repeat(np.arange(n), nb.shape[1])
    c = nb.reshape(-1)
    ok = (c >= 0) & (c < n) & (c != a)
    L[a[ok], c[ok]] = True
    return L


def candidate_mask(S, tour, lo=0, hi=None):
    """bool [hi - lo, n]: the candidate columns of rows ``lo <= i < hi`` (default: all rows ``0 .. n-3``) of the closed tour;
    ``S`` = ``L | L.T``, listed in either direction."""
    t = np.asarray(tour, dtype=np.int64)
    n = len(t) - 1
    hi = n - 2 if hi is None else hi
    i = np.arange(lo, hi)
    head = S[t[i][:, None], t[:n][None, :]]                      # (tour[i], tour[j])
    tail = S[t[i + 1][:, None], t[1:][None, :]]                  # (tour[i+1], tour[j+1]), position n is position 0
    return (head | tail) & (np.arange(n)[None, :] >= (i + 2)[:, None])


def proposals(points, tour, S=None, block=256):
    """The row proposals of one tour, the rows seeing their candidates only (``S`` None: every column, the full sweep):
    ``(change float64 [m], i int64 [m], j int64 [m])``, rows rising."""
    if S is None:
        return emu.proposals(points, tour)
    n = len(tour) - 1
    cs, js = [], []
    for lo in range(0, n - 2, block):
        hi = min(lo + block, n - 2)
        c = np.where(candidate_mask(S, tour, lo, hi), emu.row_changes(points, tour, lo, hi), np.inf)
        j = c.argmin(axis=1)                                     # first occurrence = lowest j
        cs.append(c[np.arange(len(j)), j])
        js.append(j)
    c, j = np.concatenate(cs), np.concatenate(js)
    rows = np.flatnonzero(c < THRESHOLD)
    return c[rows], rows, j[rows]


def sweep(points, tour, select_rounds, S=None):
    """One sweep of one tour.  Returns ``(tour after, [(change, i, j) of every winner in selection order], proposals)``."""
    change, i, j = proposals(points, tour, S)
    t = np.array(tour, dtype=np.int64, copy=True)
    applied = []
    for w in emu.select(change, i, j, select_rounds):
        t[i[w] + 1:j[w] + 1] = t[i[w] + 1:j[w] + 1][::-1].copy()
        applied.append((float(change[w]), int(i[w]), int(j[w])))
    return t, applied, len(i)


def nbr_two_opt(points, tours, neighbors, closing=True, max_iterations=1000, select_rounds=4, log=None):
    """The search of one group (tours int [P, n + 1], neighbors int [n, K]).  Returns ``(tours int64 [P, n + 1], sweeps,
    full_sweeps, moves)``.  ``log`` (a list) receives ``(tour index, phase, winners)`` of every sweep that moved a tour."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.array(tours, dtype=np.int64, copy=True)
    L = listed(neighbors, len(pts))
    S = L | L.T
    done, full = [False] * len(t), [False] * len(t)
    sweeps = full_sweeps = moves = 0
    while sweeps < max_iterations:
        moved = moved_full = running = False
        for p in range(len(t)):
            if done[p]:
                continue
            after, applied, _ = sweep(pts, t[p], select_rounds, None if full[p] else S)
            if not applied:
                if not full[p] and closing:
                    full[p] = running = True
                else:
                    done[p] = True
                continue
            if log is not None:
                log.append((p, int(full[p]), applied))
            t[p] = after
            moves += len(applied)
            moved = running = True
            moved_full |= full[p]
        sweeps += moved
        full_sweeps += moved_full
        if not running:
            break
    return t, int(sweeps), int(full_sweeps), moves


def all_others(n):
    """Lists that name every other city: int32 [n, n - 1]."""
    return np.array([[c for c in range(n) if c != a] for a in range(n)], dtype=np.int32)


def knn_lists(points, K):
    """The K nearest other cities of every city by float64 distance, nearest first (ties: the lowest index): int32 [n, K]."""
    pts = np.asarray(points, dtype=np.float64)
    d = emu.dist(pts[:, None, :], pts[None, :, :])
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :K].astype(np.int32)
