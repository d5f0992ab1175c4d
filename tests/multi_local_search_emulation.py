"""CPU restatement of the multi-move local search (difusco_amd/csrc/or_opt_multi.hip, ``difusco_tsp_multi_local_search_ragged``)
in numpy float64, in the operation order of the kernels.  TEST INFRASTRUCTURE ONLY.

Conventions: those of ``multi_two_opt_emulation`` and ``or_opt_emulation``.  Every tour runs on its own: rounds of

* a 2-opt phase - ``multi_two_opt_emulation.sweep`` until a sweep has no proposal;
* an Or-opt phase - sweeps of (1) row proposals: row ``i`` in ``0 .. n-2`` keeps the lowest delta of the candidates ``(v, i, j)``
  of ``or_opt_emulation`` that start at ``i`` (ties: the lowest ``v``, then the lowest ``j``) and proposes if it is ``< -1e-6``,
  key ``(delta, i)``, range ``[min(i, j), hi + 1)`` with ``hi = j`` for ``j > i + L`` and ``i + L`` for ``j < i``; (2) the
  selection of the multi-move 2-opt over these keys and ranges; (3) every winner applies its move - until a sweep has no
  proposal.

A tour is done after a round whose Or-opt phase applied nothing, after ``max_rounds`` rounds, or when it has moved in
``max_iterations`` sweeps (both kinds together).  ``select_ranges`` compares every pair of live proposals: quadratic in their
number, and obviously the rule."""
import numpy as np

import multi_two_opt_emulation as M
from or_opt_emulation import THRESHOLD, VARIANTS, apply_or_opt_move, dist


def _dist_to(P, rows, cols):
    """``dist`` between the points ``P[rows]`` (down) and ``P[cols]`` (across), coordinate by coordinate: the same two
    products, one sum and square root on contiguous arrays."""
    dx = P[rows, 0][:, None] - P[cols, 0][None, :]
    dy = P[rows, 1][:, None] - P[cols, 1][None, :]
    return np.sqrt(dx * dx + dy * dy)


def or_opt_row_deltas(points, tour, lo, hi):
    """delta of the candidates of rows ``lo <= i < hi`` of one tour: float64 [hi - lo, 5, n], +inf where (v, i, j) is no
    candidate.  The arithmetic of ``or_opt_emulation.or_opt_deltas``, a block of rows at a time; |P_j P_i+k| and |P_i+k P_j+1|
    (k = 1 .. 3) are computed once for the five variants (a difference is squared, so |pq| and |qp| are the same bits)."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.asarray(tour, dtype=np.int64)
    n = len(t) - 1
    P = pts[t]                                                   # [n + 1, 2]
    d = dist(P[:-1], P[1:])                                      # [n]
    jj = np.arange(n)
    out = np.full((hi - lo, len(VARIANTS), n), np.inf)
    to_j, to_j1 = {}, {}
    for k in (1, 2, 3):
        i = np.arange(lo, min(hi, n - k))
        to_j[k], to_j1[k] = _dist_to(P, i + k, jj), _dist_to(P, i + k, jj + 1)
    for v, (L, rev) in enumerate(VARIANTS):
        i = np.arange(lo, min(hi, n - L))                        # i <= n - 1 - L
        if len(i) == 0:
            continue
        ka, kb = (L, 1) if rev else (1, L)                       # a = P_i+ka, b = P_i+kb
        close = dist(P[i], P[i + L + 1])
        add = (close[:, None] + to_j[ka][:len(i)]) + to_j1[kb][:len(i)]
        rem = (d[i] + d[i + L])[:, None] + d[None, :]
        delta = add - rem
        ok = (jj[None, :] < i[:, None]) | (jj[None, :] > (i + L)[:, None])
        out[:len(i), v] = np.where(ok, delta, np.inf)
    return out


def or_opt_proposals(points, tour, block=128):
    """The row proposals of one tour: ``(delta float64 [m], i, v, j int64 [m])``, rows rising."""
    n = len(tour) - 1
    ds, vs, js = [], [], []
    for lo in range(0, n - 1, block):
        c = or_opt_row_deltas(points, tour, lo, min(lo + block, n - 1))
        flat = c.reshape(len(c), -1).argmin(axis=1)              # first occurrence = lowest v, then lowest j
        ds.append(c.reshape(len(c), -1)[np.arange(len(flat)), flat])
        vs.append(flat // n)
        js.append(flat % n)
    delta, v, j = np.concatenate(ds), np.concatenate(vs), np.concatenate(js)
    rows = np.flatnonzero(delta < THRESHOLD)
    return delta[rows], rows, v[rows], j[rows]


def or_opt_range(i, v, j):
    """The position range ``[a, b)`` of the proposals ``(v, i, j)`` (arrays)."""
    L = np.array([VARIANTS[k][0] for k in v], dtype=np.int64) if len(v) else np.zeros(0, dtype=np.int64)
    hi = np.where(j > i + L, j, i + L)
    return np.minimum(i, j), hi + 1


def select_ranges(value, row, a, b, select_rounds, block=1024):
    """The winners among proposals of key ``(value, row)`` and range ``[a, b)``, as indices into them: per round in key order,
    the rounds in order.  ``multi_two_opt_emulation.select`` over arbitrary ranges."""
    m = len(row)
    rank = np.empty(m, dtype=np.int64)
    rank[np.lexsort((row, value))] = np.arange(m)                # key (value, row): distinct, the row is
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


def or_opt_sweep(points, tour, select_rounds):
    """One Or-opt sweep of one tour.  Returns ``(tour after, [(delta, v, i, j) of every winner in selection order],
    proposals)``.  The winners' ranges are disjoint and a move rewrites positions inside its range only, so applying them one
    after the other with their positions of the tour BEFORE the sweep is applying them all at once."""
    delta, i, v, j = or_opt_proposals(points, tour)
    a, b = or_opt_range(i, v, j)
    t = np.array(tour, dtype=np.int64, copy=True)
    applied = []
    for w in select_ranges(delta, i, a, b, select_rounds):
        t = apply_or_opt_move(t, int(v[w]), int(i[w]), int(j[w]))
        applied.append((float(delta[w]), int(v[w]), int(i[w]), int(j[w])))
    return t, applied, len(i)


def search_tour(points, tour, max_iterations=1000, max_rounds=16, select_rounds=4, log=None, phases=None):
    """The search of ONE tour.  Returns ``(tour int64 [n + 1], counters)``, counters = dict of ``two_opt_sweeps``,
    ``or_opt_sweeps``, ``rounds``, ``two_opt_moves``, ``or_opt_moves``.  ``log`` (a list) receives ``(kind, tour before, winners,
    proposals)`` of every sweep that moved the tour, kind "2opt" or "oropt"; ``phases`` (a list) receives ``(2-opt sweeps, Or-opt
    sweeps)`` of every round."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.array(tour, dtype=np.int64, copy=True)
    c = {"two_opt_sweeps": 0, "or_opt_sweeps": 0, "rounds": 1, "two_opt_moves": 0, "or_opt_moves": 0}
    total = 0
    if max_iterations == 0:
        return t, c
    for r in range(max_rounds):
        c["rounds"] = r + 1
        ph = [0, 0]
        for k, (kind, fn) in enumerate((("2opt", M.sweep), ("oropt", or_opt_sweep))):
            while True:
                after, applied, m = fn(pts, t, select_rounds)
                if not applied:                                  # no proposal: the phase ends
                    break
                if log is not None:
                    log.append((kind, t.copy(), applied, m))
                t = after
                total += 1
                ph[k] += 1
                c["two_opt_sweeps" if k == 0 else "or_opt_sweeps"] += 1
                c["two_opt_moves" if k == 0 else "or_opt_moves"] += len(applied)
                if total >= max_iterations:
                    if phases is not None:
                        phases.append(tuple(ph))
                    return t, c
        if phases is not None:
            phases.append(tuple(ph))
        if ph[1] == 0:
            break
    return t, c


def multi_local_search(points, tours, max_iterations=1000, max_rounds=16, select_rounds=4):
    """The search of one group (tours int [P, n + 1]).  Returns ``(tours int64 [P, n + 1], counters)``: the sweeps and rounds
    are the maxima over the tours, the moves the sums."""
    out, cs = [], []
    for t in np.asarray(tours):
        a, c = search_tour(points, t, max_iterations, max_rounds, select_rounds)
        out.append(a)
        cs.append(c)
    counters = {k: (max if k in ("two_opt_sweeps", "or_opt_sweeps", "rounds") else sum)(c[k] for c in cs) for k in cs[0]}
    return np.stack(out), counters


def clustered_instance(n, s):
    """Points in five tight clusters and a random-permutation start: here a 2-opt phase after round 1 can still move."""
    rng = np.random.default_rng(s * 977 + n)
    c = rng.random((5, 2))
    pts = c[rng.integers(0, 5, n)] + 0.02 * rng.standard_normal((n, 2))
    tour = np.array([0] + list(rng.permutation(n - 1) + 1) + [0], dtype=np.int64)
    return pts, tour


LATTICE_SEEDS = {6: 7, 8: 0}    # of seeds 0 .. 7: Or-opt sweeps with equal lowest deltas of two rows AND equal candidates in a row


def lattice_instance(k, s):
    """The k x k integer grid and a random-permutation start: many equal deltas."""
    rng = np.random.default_rng(7000 + 10 * k + s)
    g = np.arange(k, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    n = k * k
    tour = np.array([0] + list(rng.permutation(n - 1) + 1) + [0], dtype=np.int64)
    return pts, tour
