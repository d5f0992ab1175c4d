"""The zoo of the greedy MIS decode (``difusco_mis_decode``, difusco_amd/csrc/mis_decode.hip): graph structures, score classes, the
pairs of them that the tests run, and a sequential reference.  A helper module like tests/graph_zoo.py: no GPU use, no conftest,
nothing collected from it.  tests/test_mis_decode_host.py pins it on the CPU (against oracle/tsp_decode_oracle.mis_decode and the
reference's own outputs in tests/golden/mis_decode_*.npz); tests/test_gpu_mis_decode_zoo.py holds the kernel against it.

The rule: the nodes are visited by ``np.argsort(-scores.astype(np.float32), kind="stable")`` - decreasing score, -0.0 and +0.0
equal, every NaN after everything else including -inf, equal scores (and the NaNs among themselves) by increasing node id.  A
visited node that no earlier taken node excluded is taken and excludes the entries of its own row; a self entry does not exclude
the node itself.  The kernel decides the same set in parallel rounds ("IN iff all higher-priority neighbours are OUT") by reading
a node's OWN row, so the two agree on symmetric adjacencies only; every structure here is symmetric.

The round bound.  ``level(v) = 1 + max level(u)`` over the neighbours ``u != v`` that rank before ``v`` (1 without one).  By
induction a node of level l has decided by the end of round l: its higher-priority neighbours have levels below l, so they were
decided when round l started, and a stale read of their state can only delay a decision to that round, not past it.  The host loop
runs groups of four rounds and stops after the first group whose last round leaves nobody undecided, so
``rounds <= 4 * ceil(Lmax / 4)``, and at least one group runs.  This follows from the kernel's code, not from a measurement.
"""
import functools
import math

import numpy as np

F32 = np.float32


# ---- the reference -------------------------------------------------------------------------------------------------------------
def visiting_order(scores):
    return np.argsort(-np.asarray(scores).reshape(-1).astype(F32), kind="stable")


def rows_of(edge_index, n):
    """(rowptr, col) of the adjacency: the entries of every row in the order ``edge_index`` lists them."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    at = np.argsort(ei[0], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))]).astype(np.int64)
    return rowptr, ei[1][at]


def reference(scores, edge_index, n):
    """``mis_utils.mis_decode_np`` restated sequentially: 0/1 int array [n].  The scores are taken AFTER the float32 cast (the
    wrapper casts), so float64 scores that collapse to one float32 value are a tie by node id."""
    rowptr, col = rows_of(edge_index, n)
    sol = np.zeros(n, dtype=int)
    for i in visiting_order(scores).tolist():
        if sol[i] == -1:
            continue
        sol[col[rowptr[i]:rowptr[i + 1]]] = -1
        sol[i] = 1
    return (sol == 1).astype(int)


def levels(scores, edge_index, n):
    """Lmax: the longest priority-decreasing dependency chain, counted in nodes."""
    rowptr, col = rows_of(edge_index, n)
    lev = np.zeros(n, dtype=np.int64)                  # 0: not visited yet, i.e. ranks later
    for v in visiting_order(scores).tolist():
        nb = col[rowptr[v]:rowptr[v + 1]]
        nb = nb[nb != v]
        lev[v] = 1 + (int(lev[nb].max()) if nb.size else 0)
    return int(lev.max())


def round_bound(lmax):
    return 4 * math.ceil(lmax / 4)


# ---- structures: name -> (n, edge_index int64 [2, E]) ----------------------------------------------------------------------------
def sym(pairs):
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([p.T, p.T[::-1]], axis=1)


def path(n, first=0):
    return [(first + i, first + i + 1) for i in range(n - 1)]


def star(d, decreasing=False):
    """Hub 0, leaves 1..d; the hub's row lists them in increasing or decreasing id order."""
    leaves = list(range(d, 0, -1) if decreasing else range(1, d + 1))
    return d + 1, sym([(0, v) for v in leaves])


def sparse_random(n, seed):
    """Mean degree 4: 2 n distinct random pairs a != b, both directions."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, 2 * n), rng.integers(0, n - 1, 2 * n)
    b = b + (b >= a)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    pairs = np.unique(np.stack([lo, hi], axis=1), axis=0)
    return sym(rng.permutation(pairs))


def with_loops(n, ei, nodes):
    nodes = np.asarray(nodes, dtype=np.int64)
    return np.concatenate([ei, np.stack([nodes, nodes])], axis=1)


def union_of(graphs):
    """Disjoint union of [(n, ei)] -> (n, ei, offsets [G + 1])."""
    off = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    return int(off[-1]), np.concatenate([ei + off[g] for g, (_, ei) in enumerate(graphs)], axis=1), off


def _union_40():
    """40 graphs of 1-9 nodes (paths, cycles, cliques, stars by turns), one-node members in the middle."""
    sizes = [((7 * g + 3) % 9) + 1 for g in range(40)]
    sizes[19] = sizes[20] = sizes[21] = 1
    out = []
    for g, k in enumerate(sizes):
        if k == 1:
            pairs = []
        elif g % 4 == 0:
            pairs = path(k)
        elif g % 4 == 1:
            pairs = path(k) + ([(k - 1, 0)] if k > 2 else [])
        elif g % 4 == 2:
            pairs = [(a, b) for a in range(k) for b in range(a + 1, k)]
        else:
            pairs = [(0, v) for v in range(1, k)]
        out.append((k, sym(pairs)))
    return out


UNION_40 = _union_40()
SORT_SIZES = (255, 256, 257, 4095, 4097, 300_000)      # across rocPRIM's switch from the single-block to the multi-pass sort
STAR_DEGREES = (63, 64, 65, 128, 129, 300)             # the lane-stride boundaries of the one-wavefront-per-node round kernel


def _structures():
    s = {}
    for n in (5, 257, 1000):
        s[f"path_{n}"] = (n, sym(path(n)))
    s["cycle_64"] = (64, sym(path(64) + [(63, 0)]))
    for d in STAR_DEGREES:
        s[f"star_{d}_inc"] = star(d)
        s[f"star_{d}_dec"] = star(d, decreasing=True)
    s["k_70"] = (70, sym([(a, b) for a in range(70) for b in range(a + 1, 70)]))
    s["k_40_90"] = (130, sym([(a, 40 + b) for a in range(40) for b in range(90)]))
    s["isolated_33"] = (60, sym(path(27, first=16)))                 # 0..15 and 43..59 are isolated
    base = sparse_random(50, seed=50)
    s["loops_all"] = (50, with_loops(50, base, np.arange(50)))       # the dataset layout
    s["loops_some"] = (50, with_loops(50, base, np.arange(0, 50, 3)))
    s["loops_only"] = (12, with_loops(12, sym(path(8)), [8, 10, 11]))      # 8, 10, 11: a self loop and nothing else; 9: empty row
    s["duplicates"] = (50, np.concatenate([base, base], axis=1))
    s["one_node"] = (1, np.zeros((2, 0), dtype=np.int64))
    s["one_node_loop"] = (1, np.zeros((2, 1), dtype=np.int64))
    s["edgeless_7"] = (7, np.zeros((2, 0), dtype=np.int64))
    s["union_40"] = union_of(UNION_40)[:2]
    for n in SORT_SIZES:
        s[f"sparse_{n}"] = (n, sparse_random(n, seed=n))
    return s


STRUCTURES = _structures()
FIXTURE_STRUCTURES = tuple(k for k, (n, _) in STRUCTURES.items() if n <= 4097)      # tests/golden/mis_decode_zoo.npz


# ---- score classes (float32, but for float64_collapsing) -------------------------------------------------------------------------
NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(F32)      # both signs, quiet and not


def sixteen_levels(n, rng):
    return (rng.integers(0, 17, n) / 16).astype(F32)


def make_scores(kind, n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    ids = np.arange(n)
    if kind == "distinct":
        return rng.permutation(ids / n).astype(F32)
    if kind == "increasing_id":
        return (ids / n).astype(F32)
    if kind == "decreasing_id":
        return ((n - 1 - ids) / n).astype(F32)
    if kind == "alternating_id":                       # every even node above every odd node: on a path the chain is 2
        return np.where(ids % 2 == 0, 1.0 - ids / (2 * n), 0.5 - ids / (2 * n)).astype(F32)
    if kind == "all_zero":
        return np.zeros(n, dtype=F32)
    if kind == "all_one":
        return np.ones(n, dtype=F32)
    if kind == "mixed_zero_signs":
        return np.where((ids // 3) % 2 == 0, F32(0.0), F32(-0.0)).astype(F32)
    if kind == "two_level":
        return rng.integers(0, 2, n).astype(F32)
    if kind == "sixteen_levels":
        return sixteen_levels(n, rng)
    if kind == "one_ulp":                              # np.nextafter steps: on positive floats one step is one more in the bits
        base = np.array([0.5, 1.0, np.finfo(F32).tiny], dtype=F32).view(np.int32)
        return (base[rng.integers(0, 3, n)] + rng.integers(-2, 3, n).astype(np.int32)).view(F32)
    if kind == "denormal":                             # distinct subnormals of both signs
        bits = (1 + rng.permutation(n)).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
        assert n < (1 << 23)
        return bits.view(F32)
    if kind == "gaussian_range":                       # x * 0.5 + 0.5 of the Gaussian path
        return rng.uniform(-0.7, 1.6, n).astype(F32)
    if kind == "infinities":
        s = rng.permutation(ids / n).astype(F32)
        k = max(2, n // 10)
        where = rng.choice(n, size=min(n, k), replace=False)
        s[where] = np.where(np.arange(len(where)) % 2 == 0, np.inf, -np.inf).astype(F32)
        return s
    if kind == "with_nan":                             # 5 % NaN (one at least), all four patterns, among sixteen_levels
        s = sixteen_levels(n, rng)
        where = rng.choice(n, size=max(1, round(0.05 * n)), replace=False)
        s[where] = NANS[np.arange(len(where)) % 4]
        return s
    if kind == "float64_collapsing":                   # pairwise distinct float64, 8 float32 values; as float64 a HIGHER id ranks first
        assert n <= 5000                               # n * 1e-13 stays below half a float32 ulp of 0.125
        s = (1 + rng.integers(0, 8, n)) / 8 + ids * 1e-13
        assert len(np.unique(s)) == n and len(np.unique(s.astype(F32))) <= 8
        return s
    raise ValueError(kind)


SCORE_CLASSES = ("distinct", "increasing_id", "decreasing_id", "alternating_id", "all_zero", "all_one", "mixed_zero_signs",
                 "two_level", "sixteen_levels", "one_ulp", "denormal", "gaussian_range", "infinities", "with_nan",
                 "float64_collapsing")


def _pairs():
    p = [(s, "distinct") for s in FIXTURE_STRUCTURES]
    p += [(f"path_{n}", k) for n in (5, 257, 1000) for k in ("increasing_id", "decreasing_id", "alternating_id", "all_zero", "all_one")]
    p += [("cycle_64", k) for k in ("increasing_id", "all_zero", "two_level", "with_nan")]
    p += [(f"star_{d}_{o}", k) for d in STAR_DEGREES for o in ("inc", "dec")
          for k in ("all_zero", "decreasing_id", "two_level", "mixed_zero_signs")]
    p += [("k_70", k) for k in ("all_one", "increasing_id", "decreasing_id", "two_level", "one_ulp", "with_nan")]
    p += [("k_40_90", k) for k in ("all_zero", "two_level", "sixteen_levels")]
    p += [("isolated_33", k) for k in ("all_zero", "with_nan", "infinities")]
    p += [(s, k) for s in ("loops_all", "loops_some", "loops_only") for k in ("all_zero", "two_level", "with_nan")]
    p += [("duplicates", k) for k in ("two_level", "sixteen_levels", "all_one")]
    p += [(s, k) for s in ("one_node", "one_node_loop") for k in ("all_zero", "with_nan")]
    p += [("edgeless_7", k) for k in ("all_zero", "mixed_zero_signs", "with_nan", "infinities")]
    p += [("union_40", k) for k in ("all_zero", "two_level", "sixteen_levels", "with_nan", "mixed_zero_signs")]
    p += [(f"sparse_{n}", k) for n in SORT_SIZES[:-1]
          for k in ("all_zero", "mixed_zero_signs", "two_level", "sixteen_levels", "one_ulp", "denormal", "gaussian_range",
                    "infinities", "with_nan", "float64_collapsing")]
    p += [("sparse_300000", "sixteen_levels")]         # the only case above 5000 nodes
    return p


PAIRS = _pairs()
BIG = ("sparse_300000", "sixteen_levels")


# ---- star placement: the one neighbour that matters sits at a chosen position of the hub's list -----------------------------------
def star_placement(d, pos, kind):
    """Hub 0 with leaves 1..d listed by increasing id, so leaf ``pos + 1`` is entry ``pos`` of the hub's row; every other leaf
    ranks after the hub.  ``kind="in"``: that leaf ranks before the hub and is IN from round 1, so the hub is OUT.
    ``kind="undecided"``: it also hangs on a tail leaf - w - x with x > w > leaf > hub, so it is IN but undecided until round 3; a
    hub that does not see it goes IN in round 1.  -> (n, edge_index, scores)."""
    n, ei = star(d)
    leaf = pos + 1
    scores = np.full(n, 0.25, dtype=F32)
    scores[0], scores[leaf] = 0.5, 0.75
    if kind == "undecided":
        w, x = n, n + 1
        ei = np.concatenate([ei, sym([(leaf, w), (w, x)])], axis=1)
        scores = np.concatenate([scores, np.array([0.8, 0.9], dtype=F32)])
        n += 2
    elif kind != "in":
        raise ValueError(kind)
    return n, ei, scores


STAR_PLACEMENTS = [(d, pos, kind) for d in STAR_DEGREES for pos in sorted({0, 63, 64, d - 1}) if pos < d
                   for kind in ("in", "undecided")]


# ---- one case, computed once -------------------------------------------------------------------------------------------------------
def case_id(pair):
    return f"{pair[0]}-{pair[1]}"


@functools.lru_cache(maxsize=None)
def case(structure, kind):
    """-> dict(n, edge_index, scores, want, lmax): the arrays are shared between the tests that need them and stay unchanged."""
    n, ei = STRUCTURES[structure]
    scores = make_scores(kind, n, seed=sum(map(ord, structure)))
    return dict(n=n, edge_index=ei, scores=scores, want=reference(scores, ei, n), lmax=levels(scores, ei, n))


# ---- properties --------------------------------------------------------------------------------------------------------------------
def is_independent(n, edge_index, sol):
    a, b = np.asarray(edge_index).reshape(2, -1)
    off = a != b
    return not np.any((sol[a] == 1) & (sol[b] == 1) & off)


def is_maximal(n, edge_index, sol):
    a, b = np.asarray(edge_index).reshape(2, -1)
    off = a != b
    covered = np.zeros(n, dtype=bool)
    covered[a[off & (sol[b] == 1)]] = True
    return bool(np.all(covered | (sol == 1)))
