"""CPU restatement of the device graph build (difusco_amd/csrc/graph_build.hip, ``difusco_graph_build``) in numpy, pass by pass,
and the graphs both the host and the GPU tests run it on (a helper module like tests/two_opt_screen_emulation.py: nothing is
collected from it).

``emulate`` follows the kernels, not graph.py: the per-node spans as integer maxima on the two 32-bit halves of one 64-bit word
(the low half holds n-1-lo of the REVERSED node, so that one forward max-scan of both halves gives ``reach`` and ``back``), the
cuts from the scanned words, their sum scan, the composite key ``(block << 32) | morton`` sorted stably ON THE BITS THE LIBRARY
SORTS ON (``32 + bits(n)``), ``inv``, the stable sort of the edge ids by ``inv[centre]`` on ``bits(n)`` bits, ``col`` through
``inv`` and ``rowptr`` by a lower-bound search.  ``host`` is graph.py's ``build_csr`` on the CPU (the C helper plus
``locality_node_order``)."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


def bits(values):
    """gb_bits: the bits that hold every value of 0..values-1, at least 1."""
    b = 1
    while b < 63 and (1 << b) < values:
        b += 1
    return b


def morton(points):
    """gb_quantise / gb_spread: float64 from the first operation on, fmax / fmin for the clip, truncation."""
    p = np.asarray(points).astype(np.float64).reshape(-1, 2)
    mn, mx = p.min(axis=0), p.max(axis=0)
    span = np.fmax(mx - mn, 1e-30)
    q = np.fmin(np.fmax((p - mn) / span * 65535.0, 0.0), 65535.0).astype(np.uint64)

    def spread(v):
        v = (v | (v << np.uint64(8))) & np.uint64(0x00FF00FF)
        v = (v | (v << np.uint64(4))) & np.uint64(0x0F0F0F0F)
        v = (v | (v << np.uint64(2))) & np.uint64(0x33333333)
        return (v | (v << np.uint64(1))) & np.uint64(0x55555555)

    return spread(q[:, 0]) | (spread(q[:, 1]) << np.uint64(1))


def blocks(r, c, n):
    """Passes 1, 2, 4 and 5: spans, the scan of both halves, the cuts, their sum scan."""
    hi = np.arange(n, dtype=np.int64)
    rlo = np.arange(n, dtype=np.int64)               # word k: n-1-lo of node n-1-k; initially n-1-(n-1-k) = k
    np.maximum.at(hi, r, c)
    np.maximum.at(rlo, n - 1 - r, n - 1 - c)
    S = (hi.astype(np.uint64) << np.uint64(32)) | rlo.astype(np.uint64)
    T = (np.maximum.accumulate(S >> np.uint64(32)) << np.uint64(32)) | np.maximum.accumulate(S & M32)
    b = np.arange(1, n, dtype=np.int64)
    reach_prev = (T[b - 1] >> np.uint64(32)).astype(np.int64)
    back = n - 1 - (T[n - 1 - b] & M32).astype(np.int64)
    cut = np.zeros(n, dtype=np.uint32)
    cut[1:] = (reach_prev < b) & (back >= b)
    return np.cumsum(cut, dtype=np.uint32)


def emulate(edge_index, n, points=None):
    """-> dict(rowptr, col, row, perm int32; perm_identity; node_order int64 or None): what difusco_graph_build leaves."""
    ei = np.asarray(edge_index, dtype=np.int64)
    r, c = ei[0], ei[1]
    E = ei.shape[1]
    assert E == 0 or (r.min() >= 0 and c.min() >= 0 and r.max() < n and c.max() < n)
    order = None
    inv = np.arange(n, dtype=np.int64)
    if points is not None and n > 1 and E > 0:
        key = (blocks(r, c, n).astype(np.uint64) << np.uint64(32)) | morton(np.asarray(points).reshape(-1, 2)[:n])
        used = key & np.uint64((1 << (32 + bits(n))) - 1)
        assert np.array_equal(used, key)                              # the sorted bits hold the whole key
        order = np.argsort(used, kind="stable").astype(np.int64)
        inv = np.empty(n, dtype=np.int64)
        inv[order] = np.arange(n, dtype=np.int64)
    ekey = inv[r]
    used = ekey & ((1 << bits(n)) - 1)
    assert np.array_equal(used, ekey)
    perm = np.argsort(used, kind="stable")
    row = ekey[perm]
    out = dict(rowptr=np.searchsorted(row, np.arange(n + 1), side="left").astype(np.int32), col=inv[c[perm]].astype(np.int32),
               row=row.astype(np.int32), perm=perm.astype(np.int32), perm_identity=bool((perm == np.arange(E)).all()),
               node_order=None if order is None or (order == np.arange(n)).all() else order)
    return out


def host(edge_index, n, points=None):
    """graph.build_csr(method="host") on the CPU, in the form of ``emulate``'s result."""
    from difusco_amd.graph import build_csr
    g = build_csr(torch.from_numpy(np.asarray(edge_index, dtype=np.int64)), n, "cpu", points=points)
    E = g.n_edges
    return dict(rowptr=g.rowptr.numpy(), col=g.col.numpy(), row=g.row.numpy(),
                perm=np.arange(E, dtype=np.int32) if g.perm is None else g.perm.numpy(), perm_identity=g.perm is None,
                node_order=None if g.node_order is None else g.node_order.numpy())


def assert_same(a, b):
    for k in ("rowptr", "col", "row", "perm"):
        assert a[k].dtype == b[k].dtype == np.int32 and np.array_equal(a[k], b[k]), k
    assert a["perm_identity"] == b["perm_identity"]
    assert (a["node_order"] is None) == (b["node_order"] is None)
    if a["node_order"] is not None:
        assert np.array_equal(a["node_order"], b["node_order"])


# ---- the graphs ------------------------------------------------------------------------------------------------------------
def numpy_knn(points, k):
    from difusco_amd.synthetic import knn_edge_index
    return knn_edge_index(np.asarray(points, dtype=np.float64), k)


def tsp_points(n, seed):
    return np.random.default_rng(seed).random((n, 2)).astype(np.float32)


def tie_points():
    """40 points of which 12 coincide pairwise (28..39 repeat 0..11): equal keys inside one block keep id order."""
    p = tsp_points(40, 77)
    p[28:] = p[:12]
    return p


def line_points():
    """All points on one vertical line: the bounding box is degenerate on the x axis."""
    p = tsp_points(37, 78)
    p[:, 0] = np.float32(0.3)
    return p


def er_edge_index(n, p, seed, isolated=0, duplicate=False):
    """An Erdos-Renyi graph in the MIS dataset's layout (co_datasets/mis_dataset.py:43-48): the undirected edges, their reversed
    copies, then one self loop per node; not row-sorted.  ``isolated``: that many nodes keep their self loop only;
    ``duplicate``: one undirected edge is listed twice."""
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(n, k=1)
    keep = rng.random(iu[0].shape[0]) < p
    e = np.stack([iu[0][keep], iu[1][keep]]).astype(np.int64)
    if isolated:
        alone = rng.choice(n, size=isolated, replace=False)
        e = e[:, ~(np.isin(e[0], alone) | np.isin(e[1], alone))]
    if duplicate:
        e = np.concatenate([e, e[:, 5:6]], axis=1)
    e = e[:, rng.permutation(e.shape[1])]
    loops = np.arange(n, dtype=np.int64)
    return np.concatenate([e, e[::-1], np.stack([loops, loops])], axis=1)


def single_cases(knn=numpy_knn):
    """[(name, edge_index int64 numpy [2, E], n_nodes, points or None)]: the single-graph cases of the issue's list.  ``knn``
    builds the k-NN edge_index of float32 points (the GPU tests pass ``knn_edge_index_gpu``)."""
    from graph_zoo import ZOO, zoo_graph
    out = []
    for n, k in [(50, 10), (64, 63), (65, 8), (2000, 100)]:
        pts = tsp_points(n, n)
        out.append((f"tsp-{n}-k{k}", knn(pts, k), n, pts))
    # one instance, parallel_sampling 3 (duplicate_edge_index): equal Morton keys, different blocks
    pts = tsp_points(30, 5)
    ei = knn(pts, 8)
    out.append(("tsp-duplicated-x3", np.concatenate([ei + s * 30 for s in range(3)], axis=1), 90, np.tile(pts, (3, 1))))
    out.append(("ties-coincident", knn(tie_points(), 8), 40, tie_points()))
    out.append(("ties-vertical-line", knn(line_points(), 6), 37, line_points()))
    ei = knn(tsp_points(45, 9), 7)
    out.append(("nopoints-sorted", ei, 45, None))
    out.append(("nopoints-shuffled", ei[:, np.random.default_rng(3).permutation(ei.shape[1])], 45, None))
    out.append(("mis-er300", er_edge_index(300, 0.05, 11), 300, None))
    out.append(("mis-er300-isolated-duplicate", er_edge_index(300, 0.05, 12, isolated=10, duplicate=True), 300, None))
    for name in ZOO:
        deg, ei = zoo_graph(name)
        out.append((f"zoo-{name}", ei, len(deg), None))
        out.append((f"zoo-{name}-points", ei, len(deg), tsp_points(len(deg), len(deg))))      # hubs and empty rows, renumbered
    out.append(("tiny-n1-loop", np.zeros((2, 1), dtype=np.int64), 1, np.zeros((1, 2), dtype=np.float32)))
    out.append(("tiny-n2", np.array([[1, 0, 1], [0, 1, 1]], dtype=np.int64), 2, tsp_points(2, 1)))
    out.append(("tiny-n2-nopoints", np.array([[1, 0, 1], [0, 1, 1]], dtype=np.int64), 2, None))
    out.append(("tiny-no-edges", np.zeros((2, 0), dtype=np.int64), 3, tsp_points(3, 2)))
    return out


def tsp_union_case(knn=numpy_knn, sizes=(20, 33, 64), k=8):
    """-> (edge_indices per instance, node counts, points of the union): TSP instances of different sizes."""
    pts = [tsp_points(n, 100 + n) for n in sizes]
    return [knn(p, k) for p in pts], list(sizes), np.concatenate(pts)


def mis_union_case():
    """Three ER graphs (n = 300, p = 0.05) with 10 isolated nodes and a duplicated edge each, for task_rows="nodes"."""
    return [er_edge_index(300, 0.05, 20 + g, isolated=10, duplicate=True) for g in range(3)], [300] * 3
