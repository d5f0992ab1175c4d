"""The inputs that the CPU and the GPU tests of the sampled k-opt search share (tests/test_tsp_kopt_emulation.py,
tests/test_gpu_tsp_kopt_search.py), with the emulation's result of every case computed once per session.  TEST INFRASTRUCTURE
ONLY.

A case is one ragged call: a list of groups (points, start tours [P, n + 1], row_ptr, col, heat [P, E], seeds, offsets) and the
arguments of the search.  ``explore`` is the table the Python layer computes, so that the emulation reads the same float64."""
import functools

import numpy as np

import tsp_kopt_search_emulation as K
from multi_two_opt_emulation import nearest_neighbour_tour
from oracle import tsp_decode_oracle as O
from tsp_heat_kick_emulation import knn_csr

ALPHA, BETA = 1.0, 10.0


def explore(samples, rounds, alpha=ALPHA):
    return alpha * np.sqrt(np.log1p(np.arange(rounds, dtype=np.float64) * float(samples)))


def edge_index_of(rp, col):
    """[2, E] of a CSR: the row of every entry over its column."""
    return np.stack([np.repeat(np.arange(len(rp) - 1), np.diff(rp)), col]).astype(np.int64)


def keys_of(n, P, base=1 << 62):
    return [1000 * n + 17 * p + 1 for p in range(P)], [base + (p << 33) for p in range(P)]


@functools.lru_cache(maxsize=None)
def group(n, P, base=1 << 62):
    """Points, P start tours closed on a random city, the k-NN graph (self included, K = min(n, 8)), one uniform heat per tour and
    the keys.  From 6 to 65 cities the even tours are random tours at their 2-opt optimum (where the search is meant to start: its
    simulations run deep there) and the odd ones random tours (almost every first step already improves); above, the nearest-neighbour
    tour from city 0 rotated to a random city, up to 200 cities at its 2-opt optimum."""
    rng = np.random.default_rng(8100 + n)
    pts = rng.random((n, 2))
    if n <= 65:
        starts = np.stack([(lambda t: np.concatenate([t, t[:1]]))(rng.permutation(n)) for _ in range(P)])
        if n == 4:                                               # the three tours of four cities: at most one is the optimum
            starts = np.array([[0, 1, 2, 3, 0], [2, 0, 1, 3, 2], [1, 0, 3, 2, 1]])[:P]
        elif n > 5:
            starts[::2] = O.batched_two_opt(pts, starts[::2], 10000)[0]
    else:
        nn = nearest_neighbour_tour(pts)[:-1]
        starts = np.stack([(lambda t: np.concatenate([t, t[:1]]))(np.roll(nn, -f)) for f in rng.integers(0, n, P)])
        if n <= 200:
            starts = O.batched_two_opt(pts, starts, 10000)[0]
    rp, col = knn_csr(pts, 8)
    heat = rng.random((P, len(col))).astype(np.float32)
    seeds, offsets = keys_of(n, P, base)
    return pts, starts, rp, col, heat, seeds, offsets


def corner_groups():
    """Five groups over the same 33 points: rows with self entries, duplicates (another heat each) and degree 0; heat with NaN,
    values outside [0, 1] and infinities; heat with all-zero and all-NaN rows; all heat zero; a graph of four entries."""
    n, P = 33, 2
    pts, starts, rp, col, _, seeds, offsets = group(n, P)
    rng = np.random.default_rng(33)
    ei = edge_index_of(rp, col)
    E = ei.shape[1]
    wild = rng.random((P, E)).astype(np.float32) * 4 - 2
    wild[:, ::5] = np.nan
    wild[:, 1::7] = np.inf
    wild[:, 2::11] = -np.inf
    rows = rng.random((P, E)).astype(np.float32)
    rows[:, np.isin(ei[0], [1, 4, 7, 10])] = 0.0                  # all-zero rows
    rows[:, np.isin(ei[0], [2, 5, 8, 11])] = np.nan               # all-NaN rows
    keep = ei[0] % 3 != 0                                        # rows 0, 3, 6, .. have degree 0
    dup = np.concatenate([ei[:, keep], ei[:, keep][:, ::2]], axis=1)   # every second entry twice; the self entries stay
    order = np.argsort(dup[0], kind="stable")
    dup = dup[:, order]
    few = np.array([[0, 5, 5, 32], [1, 5, 6, 0]], dtype=np.int64)
    out = []
    for e, h in ((dup, rng.random((P, dup.shape[1])).astype(np.float32)), (ei, wild), (ei, rows), (ei, np.zeros((P, E), np.float32)),
                 (few, rng.random((P, 4)).astype(np.float32))):
        r = np.concatenate([[0], np.cumsum(np.bincount(e[0], minlength=n))]).astype(np.int32)
        out.append((pts, starts, r, e[1].astype(np.int32), h, seeds, offsets))
    return out


@functools.lru_cache(maxsize=None)
def last_position_seed(n=7, samples=4, depth=3):
    """The first seed under which the emulation APPLIES an action whose begin position is p = n - 1 (round 0 or later)."""
    pts, starts, rp, col, heat, _, _ = random_tour_of(group(n, 3))
    for seed in range(1000):
        log = []
        K.search_tour(pts, starts[0], rp, col, heat[0], seed, 0, samples=samples, depth=depth, max_rounds=4,
                      explore=explore(samples, 4), log=log)
        if any(a[4] == n - 1 for a in log):
            return seed
    raise AssertionError("no seed begins an applied action at p = n - 1")


def random_tour_of(g):
    """The group with its second tour alone: a random tour, no 2-opt optimum."""
    return g[:1] + (g[1][1:2],) + g[2:4] + (g[4][1:2], g[5][1:2], g[6][1:2])


def with_keys(g, seeds, offsets):
    return g[:5] + (list(seeds), list(offsets))


def cases():
    """name -> (groups, arguments)."""
    out = {}
    for n, P in ((4, 3), (5, 1), (7, 3), (64, 1), (65, 3), (200, 1)):
        out[f"ladder-n{n}"] = ([group(n, P)], dict(samples=64, depth=10, max_rounds=9, patience=10))
    out["S1-D10"] = ([group(65, 3)], dict(samples=1, depth=10, max_rounds=40, patience=10))
    out["S65-D2"] = ([group(65, 3)], dict(samples=65, depth=2, max_rounds=9, patience=10))
    out["S1030-D1"] = ([group(65, 3)], dict(samples=1030, depth=1, max_rounds=3, patience=10))
    out["S1030-D10"] = ([group(200, 1)], dict(samples=1030, depth=10, max_rounds=2, patience=10))
    out["n1025"] = ([group(1025, 1)], dict(samples=130, depth=10, max_rounds=3, patience=10))
    out["corners"] = (corner_groups(), dict(samples=64, depth=10, max_rounds=9, patience=10))
    # patience 1: the small tours stall and stop, the tour of 64 cities in the same call runs on to the cap
    out["stall"] = ([group(5, 1), group(64, 3), group(7, 1)], dict(samples=64, depth=10, max_rounds=40, patience=1))
    out["offset-2^32"] = ([with_keys(group(65, 3), [5, 6, 7], [(1 << 32) - 2, (1 << 32) - 5, (1 << 64) - 3])],
                          dict(samples=64, depth=10, max_rounds=9, patience=10))
    g = random_tour_of(group(7, 3))
    out["begin-at-n-1"] = ([with_keys(g, [last_position_seed()], [0])], dict(samples=4, depth=3, max_rounds=4, patience=10))
    out["R0"] = ([group(65, 3)], dict(samples=64, depth=10, max_rounds=0, patience=10))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The emulation's result of a case: per group ``(tours int64 [P, n + 1], dict of lists [P])``, and the action logs, one list
    per tour of the call."""
    groups, kw = cases()[name]
    ex = explore(kw["samples"], kw["max_rounds"])
    out, logs = [], []
    for pts, starts, rp, col, heat, seeds, offsets in groups:
        ts, ps = [], []
        for t, h, s, o in zip(starts, heat, seeds, offsets):
            log = []
            a, p = K.search_tour(pts, t, rp, col, h, s, o, beta=BETA, explore=ex, log=log, **kw)
            ts.append(a)
            ps.append(p)
            logs.append(log)
        out.append((np.stack(ts), {k: [p[k] for p in ps] for k in K.PER_TOUR}))
    return out, logs
