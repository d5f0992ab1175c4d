"""CPU restatement of the 2-opt + Or-opt local search (difusco_amd/csrc/or_opt.hip, ``difusco_tsp_local_search_ragged``) in numpy
float64, in the operation order of the kernels.  TEST INFRASTRUCTURE ONLY.

A tour is ``tour[0..n]`` with ``tour[n] == tour[0]``, ``P_k = points[tour[k]]``, ``d_k = |P_k P_k+1|``; a distance is
``sqrt(dx * dx + dy * dy)`` (two products, one sum, no fused multiply-add).  An Or-opt candidate ``(v, i, j)`` moves the segment
at positions ``i+1 .. i+L`` (``0 <= i <= n-1-L``) between ``P_j`` and ``P_j+1`` (``0 <= j <= n-1``, ``j`` outside ``[i, i+L]``),
``(L, reversed) = VARIANTS[v]``:

    add   = (|P_i P_i+L+1| + |P_j a|) + |b P_j+1|        (a, b) = (P_i+1, P_i+L), swapped when reversed
    rem   = (d_i + d_i+L) + d_j
    delta = add - rem

The best move of a tour is the lowest delta, ties to the lowest flat index ``(v n + i) n + j``; it is applied if
``delta < -1e-6``.  The 2-opt phases are ``oracle.tsp_decode_oracle.batched_two_opt``."""
import numpy as np

from oracle.tsp_decode_oracle import batched_two_opt

VARIANTS = ((1, False), (2, False), (2, True), (3, False), (3, True))
THRESHOLD = -1e-6


def dist(p, q):
    d = p - q
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def tour_length(points, tour):
    t = np.asarray(tour)
    return float(dist(points[t[:-1]], points[t[1:]]).sum())


def or_opt_deltas(points, tour):
    """delta of every candidate of one tour: float64 [5, n, n], +inf where (v, i, j) is no candidate."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.asarray(tour, dtype=np.int64)
    n = len(t) - 1
    P = pts[t]                                                   # [n + 1, 2]
    d = dist(P[:-1], P[1:])                                      # [n]
    jj = np.arange(n)
    out = np.full((len(VARIANTS), n, n), np.inf)
    for v, (L, rev) in enumerate(VARIANTS):
        rows = n - L                                             # i = 0 .. n - 1 - L
        if rows < 1:
            continue
        i = np.arange(rows)
        first, last = P[i + 1], P[i + L]
        a, b = (last, first) if rev else (first, last)
        close = dist(P[i], P[i + L + 1])                         # [rows]
        to_a = dist(P[jj][None, :, :], a[:, None, :])            # |P_j a|   [rows, n]
        from_b = dist(b[:, None, :], P[jj + 1][None, :, :])      # |b P_j+1|
        add = (close[:, None] + to_a) + from_b
        rem = (d[i] + d[i + L])[:, None] + d[None, :]
        delta = add - rem
        ok = (jj[None, :] < i[:, None]) | (jj[None, :] > (i + L)[:, None])
        out[v, :rows] = np.where(ok, delta, np.inf)
    return out


def best_or_opt_move(points, tour):
    """(delta, v, i, j) of the tour's best move (lowest delta, then lowest flat index), or None if it has no candidate."""
    deltas = or_opt_deltas(points, tour)
    flat = int(np.argmin(deltas.reshape(-1)))                    # first occurrence = lowest flat index
    n = deltas.shape[1]
    v, i, j = flat // (n * n), (flat // n) % n, flat % n
    if not np.isfinite(deltas[v, i, j]):
        return None
    return float(deltas[v, i, j]), v, i, j


def apply_or_opt_move(tour, v, i, j):
    L, rev = VARIANTS[v]
    t = list(tour)
    seg = t[i + 1:i + L + 1]
    if rev:
        seg = seg[::-1]
    if j > i + L:
        new = t[:i + 1] + t[i + L + 1:j + 1] + seg + t[j + 1:]
    else:
        assert j < i
        new = t[:j + 1] + seg + t[j + 1:i + 1] + t[i + L + 1:]
    return np.asarray(new, dtype=np.int64)


def or_opt_phase(points, tours, max_iterations, moves=None):
    """The Or-opt phase of one group (tours int [P, n + 1], changed in place): every tour applies its own best move per iteration;
    an iteration counts if a tour moved; ends after an iteration without a move or after ``max_iterations`` counted ones.
    ``moves`` (a list) receives ``(tour index, delta, v, i, j)`` of every applied move.  Returns the counted iterations."""
    count = 0
    while count < max_iterations:
        moved = False
        for p in range(len(tours)):
            best = best_or_opt_move(points, tours[p])
            if best is not None and best[0] < THRESHOLD:
                tours[p] = apply_or_opt_move(tours[p], *best[1:])
                moved = True
                if moves is not None:
                    moves.append((p,) + best)
        if not moved:
            break
        count += 1
    return count


def local_search(points, tours, max_iterations=1000, max_rounds=16, moves=None, phases=None):
    """The local search of one group: rounds of (2-opt phase, Or-opt phase) until an Or-opt phase applies nothing or
    ``max_rounds`` rounds ran.  Returns ``(tours int64 [P, n + 1], two_opt_iterations, or_opt_iterations, rounds)``.
    ``phases`` (a list) receives ``(a, b)`` of every round."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.array(tours, dtype=np.int64, copy=True)
    two = orr = rounds = 0
    for _ in range(max_rounds):
        rounds += 1
        t, a = batched_two_opt(pts, t, max_iterations)
        b = or_opt_phase(pts, t, max_iterations, moves)
        two, orr = two + a, orr + b
        if phases is not None:
            phases.append((a, b))
        if b == 0:
            break
    return t, two, orr, rounds


def instance(n, s):
    """The instance recipe of the tests: points and one closed start tour."""
    rng = np.random.default_rng(1000 * n + s)
    pts = rng.random((n, 2))
    tour = np.array([0] + list(rng.permutation(n - 1) + 1) + [0], dtype=np.int64)
    return pts, tour
