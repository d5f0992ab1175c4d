"""The zoo of the TSP merge decode (``difusco_tsp_merge_tours`` / ``difusco_tsp_merge_batch``, difusco_amd/csrc/decode.hip): small
instances with coincident cities, heat classes with non-finite and signed-zero values, the pairs of them that the tests run, and
the reference.  A helper module like tests/mis_decode_cases.py: no GPU use, no conftest, nothing collected from it.
tests/test_tsp_merge_cases_host.py pins it on the CPU (the cases discriminate; the oracle reproduces the reference's own recorded
outputs in tests/golden/tsp_merge_zoo.npz); tests/test_gpu_tsp_merge_zoo.py holds the library against it.

The rule is the reference's, as ``oracle.tsp_decode_oracle.merge_tours`` computes it: a stable ascending sort of
``-(A + A^T) / dist`` over the dense N x N list, A + A^T added in float32, dist in float64 on the FLOAT32-CAST points (what the
library sees).  With ``score = (A + A^T) / dist`` the candidates of one sample are visited in this order:

  1. scores ``> 0`` by decreasing score, ``+inf`` first (positive heat at distance 0, or ``+inf`` heat);
  2. the zero block: ``S == +-0`` and all non-edges, in flat-index order;
  3. negative scores by decreasing score;
  4. score ``-inf`` (negative heat at distance 0, or ``-inf`` heat);
  5. NaN (``0/0``, NaN heat, ``inf + -inf``).

Equal scores, and the NaNs among themselves, follow flat index (i, j) with i < j.  ``completed`` is True exactly when the n - 1
insertions all came from block 1.  ``merge_iterations`` counts the entries of the dense list up to the terminating one (the
positive self entries rank with block 1, both orientations of a pair are entries); an entry of block 5 is never counted before a
terminating entry of block 1.  (A pair of coincident cities that is NOT an edge is 0/0 in the dense list, block 5, not a zero; a
k-NN list makes coincident cities each other's neighbours, and the host test asserts that every coincident pair here is a candidate.)

Two predicates on a case, both worked out by ``analyse`` with a walk of its own (which also cross-checks the oracle's walk):

``tie_free``    no two distinct pairs among the entries visited have equal scores.  Then the dense list keeps (i, j) and (j, i)
                adjacent and the library's two-entries-per-pair count equals the reference's: the rule of
                test_gpu_merge_batch.test_ties_keep_flat_index_order for comparing ``merge_iterations``.
``order_free``  the result cannot depend on how a sort orders equal keys (numpy's default argsort, which the reference uses, is
                unstable).  Holds when the case completed and, in every run of equal keys the walk visited, no two distinct
                pairs were insertable when the run began - or every distinct pair of the run was inserted, so that any order
                inserts them all - and the terminating run is one pair's two orientations and nothing else.  Rejection is
                monotone (degrees only grow, two ends of one path stay the two ends of one path), so a pair that is not
                insertable when its run begins is rejected in every order.  Only ``order_free`` cases are recorded from the
                reference.
"""
import functools

import numpy as np

from oracle import tsp_decode_oracle as D

F32 = np.float32
SIZES = (5, 8, 33, 64, 65, 129)          # directed list lengths K * n: from 20 and 56 (inside one 64-lane block) to 16512
SPARSE_K = 8
TRIO, TRIO_PAIR = (3, 7, 20), (11, 30)   # the coincident groups of the seeded n = 33 instance


# ---- structures: name -> (points float64 [n, 2], edge_index int64 [2, E] or None for the dense form) ------------------------------
def knn(points, k):
    """Row i lists the k nearest nodes of i (itself among them, at distance 0), ties by node id: a full stable sort, so the list does
    not depend on how a partial sort breaks the ties that coincident cities create."""
    d = ((points[:, None, :] - points[None, :, :]) ** 2).sum(-1)
    cols = np.argsort(d, axis=1, kind="stable")[:, :k]
    n = points.shape[0]
    return np.stack([np.repeat(np.arange(n, dtype=np.int64), k), cols.reshape(-1).astype(np.int64)])


def _points(n, groups=(), seed=None):
    pts = np.random.default_rng(1000 + n if seed is None else seed).random((n, 2))
    for g in groups:
        for v in g[1:]:
            pts[v] = pts[g[0]]
    return pts


def _structures():
    s = {}
    for n in SIZES:
        s[f"knn_{n}_full"] = (_points(n), n - 1)
        if n > SPARSE_K + 1:
            s[f"knn_{n}_k8"] = (_points(n), SPARSE_K)
    s["dense_33"] = (_points(33), None)
    pair = [(4, 17)]
    for n in (33, 65):
        s[f"pair_{n}_full"] = (_points(n, pair), n - 1)
        s[f"pair_{n}_k8"] = (_points(n, pair), SPARSE_K)
    s["pair_5_full"] = (_points(5, [(1, 3)]), 4)
    s["pair_129_k8"] = (_points(129, [(64, 128)]), SPARSE_K)
    s["pair_33_dense"] = (_points(33, pair), None)
    s["trio_33_full"] = (_points(33, [TRIO, TRIO_PAIR]), 32)
    s["trio_33_k8"] = (_points(33, [TRIO, TRIO_PAIR]), SPARSE_K)
    s["all_8_full"] = (_points(8, [tuple(range(8))]), 7)
    s["all_8_k8"] = (_points(8, [tuple(range(8))]), 8)           # every directed pair and every self loop: 64 entries, one block
    # distinct in float64 (1e-12 apart, far below half a float32 ulp of a coordinate in [0.25, 1)), one point after the cast
    cast = _points(65, seed=7)
    cast[9] = 0.25 + 0.75 * cast[9]
    cast[40] = cast[9] + 1e-12
    s["cast_65_full"] = (cast, 64)
    s["cast_65_k8"] = (cast, SPARSE_K)
    out = {}
    for name, (pts, k) in s.items():
        ei = None if k is None else knn(pts, k)
        out[name] = (pts, ei)
        if k is not None and name in ("knn_33_full", "knn_65_k8", "pair_33_full", "pair_33_k8", "trio_33_k8", "cast_65_k8", "knn_129_k8"):
            perm = np.random.default_rng(sum(map(ord, name))).permutation(ei.shape[1])
            out[name + "_perm"] = (pts, ei[:, perm])
    return out


STRUCTURES = _structures()


def points32(structure):
    return STRUCTURES[structure][0].astype(F32)


def directed_edges(structure):
    """(row, col) of the list the heat follows; the dense form lists entry (i, j) at i * n + j."""
    pts, ei = STRUCTURES[structure]
    if ei is not None:
        return ei[0], ei[1]
    n = pts.shape[0]
    idx = np.arange(n, dtype=np.int64)
    return np.repeat(idx, n), np.tile(idx, n)


def coincident_edges(structure):
    """bool [E]: directed edges between two different nodes whose float32 coordinates are equal."""
    row, col = directed_edges(structure)
    p = points32(structure)
    return (row != col) & np.all(p[row] == p[col], axis=1)


# ---- heat classes: float32 [E] on top of a seeded positive base ---------------------------------------------------------------
HEAT_CLASSES = ("base", "coincident_positive", "coincident_zero", "coincident_negative_zero", "coincident_negative", "nan_edges",
                "inf_edges", "inf_opposed", "negative_zero_edges", "gaussian_negative", "subnormal", "overflowing_sum", "all_nan")
NAN_PATTERNS = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fc00000], dtype=np.uint32).view(F32)


def _pick_directed(row, col, rng, count, need_reverse_first):
    """``count`` directed edges between different nodes, of ``count`` different pairs; the first one has its reverse in the list."""
    n = int(max(row.max(), col.max())) + 1
    listed = set((row * n + col).tolist())
    off = np.flatnonzero(row != col)
    order = off[rng.permutation(len(off))]
    chosen, pairs = [], set()
    for e in order.tolist():
        i, j = int(row[e]), int(col[e])
        if (min(i, j), max(i, j)) in pairs:
            continue
        if need_reverse_first and not chosen and (j * n + i) not in listed:
            continue
        chosen.append(e)
        pairs.add((min(i, j), max(i, j)))
        if len(chosen) == count:
            return np.array(chosen)
    raise AssertionError("too few pairs")


# seeds chosen until the case tells a wrong rule from the right one (tests/test_tsp_merge_cases_host.py): NaN ranked into the zero
# block (a pair of the zero block is inserted only if it is the first open partner of its first node in flat-index order, so few
# seeds show it), and -inf scores dropped; every other case draws from its own name
SEEDS = {("knn_5_full", "nan_edges"): 0, ("knn_65_k8", "nan_edges"): 43, ("knn_33_k8", "inf_opposed"): 52,
         ("trio_33_k8", "coincident_zero"): 35, ("trio_33_k8", "coincident_negative_zero"): 35, ("cast_65_k8", "coincident_zero"): 13,
         ("trio_33_k8", "coincident_negative"): 35, ("knn_65_k8", "inf_edges"): 7, ("cast_65_k8", "coincident_negative"): 13}


def make_heat(kind, structure, seed=None):
    row, col = directed_edges(structure)
    E = len(row)
    if seed is None:
        seed = SEEDS.get((structure, kind), sum(map(ord, structure + kind)))
    rng = np.random.default_rng(seed)
    heat = (rng.random(E) + 1e-3).astype(F32)
    co = coincident_edges(structure)
    if kind in ("base", "coincident_positive"):
        assert kind == "base" or co.any()
    elif kind == "coincident_zero":
        heat[co] = F32(0.0)
    elif kind == "coincident_negative_zero":
        heat[co] = F32(-0.0)
    elif kind == "coincident_negative":
        heat[co] = -heat[co]
    elif kind == "nan_edges":                          # one direction only; the first edge's reverse is listed and stays finite
        where = _pick_directed(row, col, rng, 5, True)
        heat[where] = NAN_PATTERNS
    elif kind == "inf_edges":
        where = _pick_directed(row, col, rng, 6, False)
        heat[where[:3]], heat[where[3:]] = F32(np.inf), F32(-np.inf)
    elif kind == "inf_opposed":                        # +inf one way, -inf the other: the pair sums to NaN
        e = int(_pick_directed(row, col, rng, 1, True)[0])
        back = np.flatnonzero((row == col[e]) & (col == row[e]))
        assert len(back) == 1
        heat[e], heat[back[0]] = F32(np.inf), F32(-np.inf)
    elif kind == "negative_zero_edges":
        heat[rng.random(E) < 0.3] = F32(-0.0)
    elif kind == "gaussian_negative":                  # P(0.3 + 0.7 z < 0) = 0.33; coincident pairs negative in both directions
        heat = (F32(0.3) + F32(0.7) * rng.standard_normal(E).astype(F32)).astype(F32)
        heat[co] = -np.abs(heat[co]) - F32(1e-3)
    elif kind == "subnormal":
        heat = rng.integers(1, 1 << 23, E).astype(np.uint32).view(F32)
    elif kind == "overflowing_sum":                    # every value finite; two directions above 1.7e38 add up to +inf in float32
        heat = (heat * F32(3.0e38)).astype(F32)
    elif kind == "all_nan":
        heat = NAN_PATTERNS[np.arange(E) % len(NAN_PATTERNS)].copy()
    else:
        raise ValueError(kind)
    assert heat.dtype == F32 and heat.shape == (E,)
    return heat


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _key_map(nan_rank, ninf_absent):
    if nan_rank not in ("last", "first", "zero"):
        raise ValueError(nan_rank)
    if nan_rank == "last" and not ninf_absent:
        return None

    def key_map(key):
        key = np.array(key, dtype=np.float64, copy=True)
        if ninf_absent:
            key[np.isposinf(key)] = 0.0                # key = -score: a -inf score read as "no edge"
        if nan_rank == "first":
            key[np.isnan(key)] = -np.inf
        elif nan_rank == "zero":
            key[np.isnan(key)] = 0.0
        return key
    return key_map


def reference(points, edge_index, heat, nan_rank="last", ninf_absent=False):
    """``oracle.tsp_decode_oracle.merge_tours`` on the float32-cast points; ``edge_index`` None for the dense form, ``heat`` [E] or
    [P, E].  -> [(tour, iterations, completed)] per sample.  ``nan_rank`` / ``ninf_absent`` are for the tests of the cases only:
    ``"first"`` ranks NaN scores with +inf, ``"zero"`` puts them into the zero block, ``ninf_absent`` reads a -inf score as no edge.
    Only the defaults are the rule."""
    pts = np.asarray(points).astype(F32)
    n = pts.shape[0]
    heat = np.asarray(heat, dtype=F32)
    heat = heat.reshape(1, -1) if heat.ndim == 1 else heat.reshape(heat.shape[0], -1)
    out = []
    for h in heat:
        adj = h if edge_index is not None else h.reshape(1, n, n)
        tours, it, done = D.merge_tours(adj, pts, edge_index, sparse_graph=edge_index is not None, parallel_sampling=1,
                                        key_map=_key_map(nan_rank, ninf_absent))
        out.append((tours[0], int(it), bool(done[0])))
    return out


def scores_of(points, edge_index, heat):
    """The dense score matrix (A + A^T) / dist as the rule states it: float32 sums, float64 distances of the float32 points."""
    pts = np.asarray(points).astype(F32).astype(np.float64)
    n = pts.shape[0]
    with np.errstate(all="ignore"):
        a = np.zeros((n, n), dtype=F32)
        if edge_index is None:
            a = np.asarray(heat, dtype=F32).reshape(n, n)
        else:
            np.add.at(a, (edge_index[0], edge_index[1]), np.asarray(heat, dtype=F32))
        return (a + a.T).astype(np.float64) / np.linalg.norm(pts[:, None] - pts, axis=-1)


def analyse(points, edge_index, heat):
    """A second walk over the dense list, kept as path end points and degrees: -> dict(edges, iterations, completed, tie_free,
    order_free, nan_scores, ninf_scores) - see the module docstring."""
    sc = scores_of(points, edge_index, heat)
    n = sc.shape[0]
    key = (-sc).flatten()
    order = np.argsort(key, kind="stable")
    far, deg = list(range(n)), [0] * n
    can = lambda i, j: i != j and deg[i] < 2 and deg[j] < 2 and far[i] != j      # noqa: E731
    edges, it, completed, tie_free, order_free = [], 0, True, True, True
    pos, total = 0, n * n
    while pos < total and len(edges) < n - 1:
        k0 = key[order[pos]]
        end = pos
        while end < total and (key[order[end]] == k0 or (np.isnan(k0) and np.isnan(key[order[end]]))):
            end += 1
        run = [(int(e) // n, int(e) % n) for e in order[pos:end]]
        distinct = {(min(i, j), max(i, j)) for i, j in run if i != j}
        insertable = {p for p in distinct if can(*p)}
        inserted = set()
        for i, j in run:
            it += 1
            if not can(i, j):
                continue
            if not k0 < 0:
                completed = False
            ti, tj = far[i], far[j]
            far[ti], far[tj] = tj, ti
            deg[i] += 1
            deg[j] += 1
            edges.append((min(i, j), max(i, j)))
            inserted.add((min(i, j), max(i, j)))
            if len(edges) == n - 1:
                break
        if len(distinct) > 1:
            tie_free = False
        if len(insertable) > 1 and inserted != distinct:
            order_free = False
        if len(edges) == n - 1 and len(run) != 2:
            order_free = False
        pos = end
    off = ~np.eye(n, dtype=bool)
    return dict(edges=edges, iterations=it, completed=completed, tie_free=tie_free, order_free=order_free and completed,
                nan_scores=int(np.isnan(sc[off]).sum()) // 2, ninf_scores=int(np.isneginf(sc[off]).sum()) // 2,
                pinf_scores=int(np.isposinf(sc[off]).sum()) // 2)


def tour_edges(tour):
    return sorted((min(a, b), max(a, b)) for a, b in zip(tour[:-1], tour[1:]))


# ---- the pairs that the tests run ------------------------------------------------------------------------------------------------
COINCIDENT = tuple(s for s in STRUCTURES if coincident_edges(s).any())
PLAIN = tuple(s for s in STRUCTURES if s not in COINCIDENT)


def _pairs():
    p = [(s, "base") for s in STRUCTURES]
    p += [(s, k) for s in COINCIDENT
          for k in ("coincident_positive", "coincident_zero", "coincident_negative_zero", "coincident_negative", "gaussian_negative")]
    everywhere = ("nan_edges", "inf_edges", "inf_opposed", "all_nan")
    p += [(s, k) for s in PLAIN for k in everywhere]
    p += [(s, k) for s in ("pair_33_full", "pair_33_k8", "trio_33_k8", "trio_33_full", "all_8_full", "all_8_k8", "cast_65_k8",
                           "pair_33_dense", "pair_33_k8_perm") for k in everywhere]
    rest = ("negative_zero_edges", "gaussian_negative", "subnormal", "overflowing_sum")
    p += [(s, k) for s in ("knn_5_full", "knn_8_full", "knn_33_full", "knn_33_k8", "knn_64_k8", "knn_65_full", "knn_65_k8_perm",
                           "knn_129_k8", "dense_33") for k in rest]
    p += [(s, k) for s in ("pair_33_k8", "trio_33_full", "cast_65_full") for k in ("negative_zero_edges", "subnormal", "overflowing_sum")]
    assert len(set(p)) == len(p)
    return p


PAIRS = _pairs()

# the cases recorded from the reference's own merge_tours + merge_cython (tests/golden/tsp_merge_zoo.npz): completed, order_free
FIXTURE_PAIRS = [("pair_33_full", "coincident_positive"), ("pair_33_full", "coincident_zero"), ("pair_33_full", "coincident_negative"),
                 ("pair_33_full_perm", "coincident_negative_zero"), ("pair_65_full", "coincident_positive"),
                 ("cast_65_full", "coincident_positive"), ("cast_65_full", "coincident_zero"), ("pair_5_full", "coincident_positive"),
                 ("knn_33_full", "nan_edges"), ("knn_65_full", "nan_edges"), ("knn_33_full_perm", "inf_edges"),
                 ("knn_64_full", "inf_edges"), ("knn_129_full", "nan_edges"), ("knn_33_full", "inf_opposed"),
                 ("pair_33_full", "gaussian_negative"), ("knn_65_full", "negative_zero_edges"), ("knn_33_full", "subnormal")]


def case_id(pair):
    return f"{pair[0]}-{pair[1]}"


@functools.lru_cache(maxsize=None)
def case(structure, kind):
    """-> dict(points float32, edge_index, heat, want=(tour, iterations, completed), info=analyse(...)): computed once, shared between
    the tests that need it, never changed."""
    pts, ei = points32(structure), STRUCTURES[structure][1]
    heat = make_heat(kind, structure)
    want = reference(pts, ei, heat)[0]
    info = analyse(pts, ei, heat)
    assert info["edges"] and sorted(info["edges"] + [_closing(info["edges"], len(pts))]) == tour_edges(want[0]), (structure, kind)
    assert (info["iterations"], info["completed"]) == want[1:], (structure, kind)
    return dict(points=pts, edge_index=ei, heat=heat, want=want, info=info)


def _closing(edges, n):
    deg = np.zeros(n, dtype=int)
    for a, b in edges:
        deg[a] += 1
        deg[b] += 1
    a, b = np.flatnonzero(deg < 2) if n > 2 else (0, 1)
    return (int(a), int(b))


def recorded_case(structure, kind):
    """A case of FIXTURE_PAIRS: its result cannot depend on the reference's unstable argsort."""
    c = case(structure, kind)
    assert c["want"][2] and c["info"]["order_free"], (structure, kind)
    return c


# ---- the completed flag of every case, checked on the CPU oracle -------------------------------------------------------------------
# Positive scores suffice on every K = n - 1, dense and all-coincident structure unless every score is NaN, and run out at K = 8;
# the exceptions are listed.  The smallest graphs lose too many of their few pairs to five NaN (or to -0.0 on a third of the
# edges); all-coincident cities have no positive score left once the coincident heat is not positive; the negative trio and pair
# cut the Gaussian case short.  At K = 8 three +inf edges, or one pair at +inf, can make a seeded instance complete.
def well_connected(structure):
    return "_full" in structure or "dense" in structure or structure.startswith("all_8")


NOT_COMPLETED_THOUGH_WELL_CONNECTED = frozenset(
    [("knn_5_full", "nan_edges"), ("knn_5_full", "negative_zero_edges"), ("knn_8_full", "nan_edges"), ("trio_33_full", "gaussian_negative"),
     ("pair_33_full_perm", "gaussian_negative")]
    + [(s, k) for s in ("all_8_full", "all_8_k8")
       for k in ("coincident_zero", "coincident_negative_zero", "coincident_negative", "gaussian_negative")])
COMPLETED_THOUGH_SPARSE = frozenset([("knn_33_k8", "inf_edges"), ("pair_33_k8", "subnormal"), ("pair_33_k8", "overflowing_sum"),
                                     ("pair_33_k8_perm", "coincident_zero")])


def expected_completed(structure, kind):
    if well_connected(structure):
        return kind != "all_nan" and (structure, kind) not in NOT_COMPLETED_THOUGH_WELL_CONNECTED
    return (structure, kind) in COMPLETED_THOUGH_SPARSE
