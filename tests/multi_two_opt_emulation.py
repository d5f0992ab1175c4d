"""CPU restatement of the multi-move 2-opt (difusco_amd/csrc/two_opt_multi.hip, ``difusco_tsp_multi_two_opt_ragged``) in numpy
float64, in the operation order of the kernels.  TEST INFRASTRUCTURE ONLY.

A tour is ``tour[0..n]`` with ``tour[n] == tour[0]``, ``P_k = points[tour[k]]``, ``d_k = |P_k P_k+1|``; a distance is
``sqrt(dx * dx + dy * dy)`` (two products, one sum, no fused multiply-add).  One sweep of one tour:

1. row ``i`` in ``0 .. n-3`` evaluates ``change(i, j) = ((|P_i P_j| + |P_i+1 P_j+1|) - d_i) - d_j`` for ``i+2 <= j <= n-1``,
   keeps its lowest change (ties: the lowest ``j``) and proposes ``(i, j_i)`` if that change is ``< -1e-6``.  Key ``(change, i)``,
   range ``[i, j_i + 1)``;
2. at most ``select_rounds`` rounds: a live proposal wins if its key is lower than that of every other live proposal whose range
   intersects its own; the winners leave, and every live proposal whose range intersects a winner's is dropped;
3. every winner reverses ``tour[i+1 .. j_i]``;
4. a tour without a proposal is done; a sweep counts for a group if one of its tours moved; the group stops when all its tours
   are done or after ``max_iterations`` counted sweeps.

This file compares every pair of live proposals (in row blocks): quadratic in their number, and obviously the rule."""
import numpy as np

THRESHOLD = -1e-6


def dist(p, q):
    d = p - q
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def tour_length(points, tour):
    t = np.asarray(tour)
    return float(dist(points[t[:-1]], points[t[1:]]).sum())


def row_changes(points, tour, lo, hi):
    """change(i, j) of rows ``lo <= i < hi`` of one tour: float64 [hi - lo, n], +inf where ``j < i + 2``."""
    t = np.asarray(tour, dtype=np.int64)
    n = len(t) - 1
    P = np.asarray(points, dtype=np.float64)[t]                  # [n + 1, 2]
    d = dist(P[:-1], P[1:])                                      # [n]
    i = np.arange(lo, hi)
    a = dist(P[i][:, None, :], P[None, :n, :])                   # |P_i P_j|
    b = dist(P[i + 1][:, None, :], P[None, 1:, :])               # |P_i+1 P_j+1|
    change = ((a + b) - d[i][:, None]) - d[None, :]
    return np.where(np.arange(n)[None, :] >= (i + 2)[:, None], change, np.inf)


def proposals(points, tour, block=256):
    """The row proposals of one tour: ``(change float64 [m], i int64 [m], j int64 [m])``, rows rising."""
    n = len(tour) - 1
    cs, js = [], []
    for lo in range(0, n - 2, block):
        c = row_changes(points, tour, lo, min(lo + block, n - 2))
        j = c.argmin(axis=1)                                     # first occurrence = lowest j
        cs.append(c[np.arange(len(j)), j])
        js.append(j)
    c, j = np.concatenate(cs), np.concatenate(js)
    rows = np.flatnonzero(c < THRESHOLD)
    return c[rows], rows, j[rows]


def select(change, i, j, select_rounds, block=1024):
    """The winners among the proposals, as indices into them: per round in key order, the rounds in order."""
    m = len(i)
    rank = np.empty(m, dtype=np.int64)
    rank[np.lexsort((i, change))] = np.arange(m)                 # key (change, i): distinct, i is
    a, b = i, j + 1
    live = np.ones(m, dtype=bool)
    winners = []
    for _ in range(min(select_rounds, m)):
        idx = np.flatnonzero(live)
        if len(idx) == 0:
            break
        la, lb, lr = a[idx], b[idx], rank[idx]
        win = np.zeros(len(idx), dtype=bool)
        for lo in range(0, len(idx), block):
            s = slice(lo, lo + block)
            meet = (la[s, None] < lb[None, :]) & (la[None, :] < lb[s, None])     # itself included
            win[s] = np.where(meet, lr[None, :], m).min(axis=1) == lr[s]
        hit = np.zeros(len(idx), dtype=bool)
        wa, wb = la[win], lb[win]
        for lo in range(0, len(idx), block):
            s = slice(lo, lo + block)
            hit[s] = ((la[s, None] < wb[None, :]) & (wa[None, :] < lb[s, None])).any(axis=1)
        won = idx[win]
        winners.extend(won[np.argsort(rank[won])].tolist())
        live[idx[hit]] = False                                   # the winners hit themselves
    return winners


def sweep(points, tour, select_rounds):
    """One sweep of one tour.  Returns ``(tour after, [(change, i, j) of every winner in selection order], proposals)``."""
    change, i, j = proposals(points, tour)
    t = np.array(tour, dtype=np.int64, copy=True)
    applied = []
    for w in select(change, i, j, select_rounds):
        t[i[w] + 1:j[w] + 1] = t[i[w] + 1:j[w] + 1][::-1].copy()
        applied.append((float(change[w]), int(i[w]), int(j[w])))
    return t, applied, len(i)


def multi_two_opt(points, tours, max_iterations=1000, select_rounds=4, log=None):
    """The search of one group (tours int [P, n + 1]).  Returns ``(tours int64 [P, n + 1], sweeps, moves)``.  ``log`` (a list)
    receives ``(tour index, tour before, winners, proposals)`` of every sweep that moved a tour."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.array(tours, dtype=np.int64, copy=True)
    done = [False] * len(t)
    sweeps = moves = 0
    while sweeps < max_iterations:
        moved = False
        for p in range(len(t)):
            if done[p]:
                continue
            after, applied, m = sweep(pts, t[p], select_rounds)
            if not applied:
                done[p] = True
                continue
            if log is not None:
                log.append((p, t[p].copy(), applied, m))
            t[p] = after
            moves += len(applied)
            moved = True
        if not moved:
            break
        sweeps += 1
    return t, sweeps, moves


def instance(n, s):
    """The instance recipe of the tests: points and one closed random-permutation start tour."""
    rng = np.random.default_rng(1000 * n + s)
    pts = rng.random((n, 2))
    tour = np.array([0] + list(rng.permutation(n - 1) + 1) + [0], dtype=np.int64)
    return pts, tour


def nearest_neighbour_tour(points):
    pts = np.asarray(points, dtype=np.float64)
    n = len(pts)
    left = np.ones(n, dtype=bool)
    tour = [0]
    left[0] = False
    for _ in range(n - 1):
        d = dist(pts, pts[tour[-1]])
        d[~left] = np.inf
        tour.append(int(d.argmin()))
        left[tour[-1]] = False
    return np.array(tour + [0], dtype=np.int64)
