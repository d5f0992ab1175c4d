"""Graph layout: COO ``edge_index`` (reference contract) -> CSR over the centre node, int32, on device.

Input contract: ``edge_index[0]`` = centre node i, ``edge_index[1]`` = neighbour
j; TSP k-NN graphs are row-sorted with constant degree and include the self edge
(``co_datasets/tsp_graph_dataset.py:53-62``); MIS graphs are undirected edges + reversed copy + self
loops, not row-sorted (``co_datasets/mis_dataset.py:43-48``); a batch is the disjoint union with node
ids offset per graph (``pl_meta_model.py:177-184``).  The conversion runs once per instance, outside
the denoising loop: on the host by default (C helper ``difusco_csr_from_coo_host``), or with ``method="device"`` on the GPU
(``difusco_graph_build``, csrc/graph_build.hip: the same arrays bit for bit, the graph never leaves the device).
"""
import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib


def _workspace(nbytes: int, device) -> torch.Tensor:
    """The scratch buffer of one library call of this module or of ``formats``: ``nbytes`` uninitialised bytes on ``device``."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


@dataclass
class CsrGraph:
    n_nodes: int
    n_edges: int
    rowptr: torch.Tensor            # int32 [n_nodes+1], device
    col: torch.Tensor               # int32 [n_edges], device
    perm: Optional[torch.Tensor]    # int32 [n_edges] CSR slot -> caller edge id; None = identity
    row: Optional[torch.Tensor] = None       # int32 [n_edges] centre node of each CSR slot, device
    seg_ptr: Optional[torch.Tensor] = None   # int32 [S+1] device; GroupNorm statistic segments
    n_segments: int = 1
    # internal node id -> caller node id (int64, device) when the nodes were renumbered for locality (TSP: Morton order
    # of the coordinates inside every graph of the batch); None = caller numbering.  Only node-indexed INPUTS (points)
    # have to be gathered with it; outputs of a TSP step are per edge and go through ``perm``.
    node_order: Optional[torch.Tensor] = None


def csr_from_coo_host(edge_index: np.ndarray, n_nodes: int):
    """numpy int64 [2,E] -> (rowptr, col, row, perm, identity) int32 numpy arrays."""
    ei = np.ascontiguousarray(edge_index, dtype=np.int64)
    assert ei.ndim == 2 and ei.shape[0] == 2
    E = ei.shape[1]
    rowptr = np.empty(n_nodes + 1, dtype=np.int32)
    col = np.empty(E, dtype=np.int32)
    row = np.empty(E, dtype=np.int32)
    perm = np.empty(E, dtype=np.int32)
    ident = ctypes.c_int(0)
    _lib.check(_lib.lib().difusco_csr_from_coo_host(
        ei.ctypes.data, E, n_nodes, rowptr.ctypes.data, col.ctypes.data, row.ctypes.data, perm.ctypes.data,
        ctypes.byref(ident)))
    return rowptr, col, row, perm, bool(ident.value)


def _id_blocks(rowptr: np.ndarray, col: np.ndarray, n_nodes: int) -> np.ndarray:
    """Block id per node of the finest partition of 0..n-1 into CONTIGUOUS id ranges that no edge crosses - for a
    disjoint-union batch (``pl_meta_model.py:177-184``) these are the graphs of the batch (or unions of them)."""
    deg = np.diff(rowptr)
    ids = np.arange(n_nodes, dtype=np.int64)
    lo, hi = ids.copy(), ids.copy()
    nz = np.flatnonzero(deg > 0)
    if nz.size:
        starts = rowptr[nz].astype(np.int64)
        lo[nz] = np.minimum(lo[nz], np.minimum.reduceat(col, starts))
        hi[nz] = np.maximum(hi[nz], np.maximum.reduceat(col, starts))
    reach = np.maximum.accumulate(hi)                  # furthest id touched by the nodes 0..i
    back = np.minimum.accumulate(lo[::-1])[::-1]       # lowest id touched by the nodes i..n-1
    cut = np.zeros(n_nodes, dtype=np.int64)            # cut[b] = 1: a block starts at node b
    if n_nodes > 1:
        cut[1:] = (reach[:-1] < ids[1:]) & (back[1:] >= ids[1:])
    return np.cumsum(cut)


def _morton_keys(points: np.ndarray) -> np.ndarray:
    """Z-order key of 2-D points (16 bits per axis over the bounding box)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    mn, mx = p.min(axis=0), p.max(axis=0)
    q = np.clip((p - mn) / np.maximum(mx - mn, 1e-30) * 65535.0, 0, 65535).astype(np.uint64)

    def spread(v):
        v = (v | (v << 8)) & np.uint64(0x00FF00FF)
        v = (v | (v << 4)) & np.uint64(0x0F0F0F0F)
        v = (v | (v << 2)) & np.uint64(0x33333333)
        return (v | (v << 1)) & np.uint64(0x55555555)

    return spread(q[:, 0]) | (spread(q[:, 1]) << np.uint64(1))


def locality_node_order(rowptr: np.ndarray, col: np.ndarray, points: np.ndarray) -> np.ndarray:
    """new -> old node numbering: inside every graph of the batch (see :func:`_id_blocks`) the nodes are sorted along
    the Morton curve of their coordinates.  Spatially close centre nodes then sit in neighbouring CSR rows, and since
    k-NN neighbours are spatially close too, the rows A h[j], V h[j] gathered by consecutive 32-edge tiles are a small
    compact set (L2-resident per XCD with the XCD-contiguous tile ranges of the fused kernel)."""
    n = rowptr.shape[0] - 1
    return np.lexsort((_morton_keys(points), _id_blocks(rowptr, col, n))).astype(np.int64)


GRAPH_BUILDS = ("host", "device")


def check_graph_build(method):
    if method not in GRAPH_BUILDS:
        raise ValueError(f"graph build {method!r}: one of {GRAPH_BUILDS}")
    return method


def _build_csr_device(edge_index, n_nodes: int, device, points=None) -> CsrGraph:
    """``build_csr`` through ``difusco_graph_build``: ``edge_index`` / ``points`` from any device (moved to ``device`` if
    needed), outputs and workspace torch tensors, the current stream.  One small readback (the flags) inside the library."""
    L = _lib.lib()
    device = torch.device(device)
    n_nodes = int(n_nodes)
    if not isinstance(edge_index, torch.Tensor):
        edge_index = torch.from_numpy(np.asarray(edge_index))
    ei = edge_index.detach().to(device=device, dtype=torch.int64).contiguous()
    assert ei.dim() == 2 and ei.shape[0] == 2
    E = int(ei.shape[1])
    pts = None
    if points is not None and n_nodes > 1 and E > 0:
        pts = points.detach() if isinstance(points, torch.Tensor) else torch.from_numpy(np.asarray(points))
        # float32 coordinates are widened on the device; everything else is widened here, as np.asarray(.., float64) would
        pts = pts.to(device=device, dtype=torch.float32 if pts.dtype == torch.float32 else torch.float64)
        pts = pts.reshape(-1, 2)[:n_nodes].contiguous()
        if pts.shape[0] != n_nodes:
            raise ValueError(f"points holds {pts.shape[0]} nodes, the graph has {n_nodes}")
    i32 = dict(dtype=torch.int32, device=device)
    rowptr, col, row, perm = (torch.empty(n_nodes + 1, **i32), torch.empty(E, **i32), torch.empty(E, **i32),
                              torch.empty(E, **i32))
    order = torch.empty(n_nodes, dtype=torch.int64, device=device) if pts is not None else None
    nbytes = ctypes.c_size_t()
    _lib.check(L.difusco_graph_build_workspace_bytes(n_nodes, E, int(pts is not None), ctypes.byref(nbytes)))
    ws = _workspace(nbytes.value, device)
    flags = (ctypes.c_uint32 * 2)()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None      # noqa: E731
    _lib.check(L.difusco_graph_build(n_nodes, E, ptr(ei), ptr(pts), int(pts is not None and pts.dtype == torch.float64),
                                     ptr(rowptr), ptr(col), ptr(row), ptr(perm), ptr(order), flags, ptr(ws), nbytes.value,
                                     ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    return CsrGraph(n_nodes=n_nodes, n_edges=E, rowptr=rowptr, col=col,
                    perm=None if flags[0] & _lib.GRAPH_PERM_IDENTITY else perm, row=row,
                    node_order=None if flags[0] & _lib.GRAPH_ORDER_IDENTITY else order)


def build_csr(edge_index: torch.Tensor, n_nodes: int, device, seg_rows: Optional[np.ndarray] = None,
              points=None, method: str = "host") -> CsrGraph:
    """edge_index int64 [2,E] (any device).  ``seg_rows``: boundaries [S+1] of the head-GroupNorm
    statistic segments over output rows (None = one segment = the reference's sparse behaviour).
    ``points`` ([n_nodes,2], optional): renumber the nodes for locality (``locality_node_order``); invisible to the
    caller - edge outputs keep the caller's edge order through ``perm``, ``node_order`` gathers the point input.
    ``method``: ``"host"`` (C helper + numpy) or ``"device"`` (``difusco_graph_build``: equal arrays, built on the GPU)."""
    if check_graph_build(method) == "device":
        g = _build_csr_device(edge_index, n_nodes, device, points)
        if seg_rows is not None and len(seg_rows) > 2:
            g.seg_ptr = torch.from_numpy(np.asarray(seg_rows, dtype=np.int32)).to(device)
            g.n_segments = len(seg_rows) - 1
        return g
    ei = edge_index.detach().cpu().numpy()
    rowptr, col, _row, perm, ident = csr_from_coo_host(ei, n_nodes)
    order = None
    if points is not None and n_nodes > 1 and col.shape[0] > 0:
        pts = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
        order = locality_node_order(rowptr, col, pts.reshape(-1, 2)[:n_nodes])
        if np.array_equal(order, np.arange(n_nodes)):
            order = None
        else:
            inv = np.empty(n_nodes, dtype=np.int64)
            inv[order] = np.arange(n_nodes, dtype=np.int64)
            rowptr, col, _row, perm, ident = csr_from_coo_host(inv[np.ascontiguousarray(ei, dtype=np.int64)], n_nodes)
    g = CsrGraph(
        n_nodes=n_nodes, n_edges=int(col.shape[0]),
        rowptr=torch.from_numpy(rowptr).to(device), col=torch.from_numpy(col).to(device),
        perm=None if ident else torch.from_numpy(perm).to(device), row=torch.from_numpy(_row).to(device),
        node_order=None if order is None else torch.from_numpy(order).to(device))
    if seg_rows is not None and len(seg_rows) > 2:
        g.seg_ptr = torch.from_numpy(np.asarray(seg_rows, dtype=np.int32)).to(device)
        g.n_segments = len(seg_rows) - 1
    return g


def union_rows(edge_counts, node_counts, task_rows: str):
    """Boundaries of the instances of a disjoint-union batch: ``(node_offsets [B+1], instance_rows [B+1])`` int64 numpy, the
    instance rows counting output rows (``"edges"`` for TSP, ``"nodes"`` for MIS) in caller order."""
    node_off = np.concatenate([[0], np.cumsum(np.asarray(node_counts, dtype=np.int64))])
    edge_off = np.concatenate([[0], np.cumsum(np.asarray(edge_counts, dtype=np.int64))])
    return node_off, (edge_off if task_rows == "edges" else node_off)


def _build_union_csr_device(edge_indices, node_counts, device, points, task_rows):
    """``build_union_csr`` without per-instance host round trips: the union is concatenated and checked on the device, and ONE
    readback carries both checks (the first instance with an edge outside its nodes, the CSR slot at every instance start)."""
    device = torch.device(device)
    eis = [e if isinstance(e, torch.Tensor) else torch.from_numpy(np.asarray(e)) for e in edge_indices]
    eis = [e.detach().to(device, torch.int64) for e in eis]
    counts = [int(e.shape[1]) for e in eis]
    node_off, inst_rows = union_rows(counts, node_counts, task_rows)
    n, B = int(node_off[-1]), len(eis)
    off_d = torch.from_numpy(node_off).to(device)
    union = torch.cat([e + int(node_off[b]) for b, e in enumerate(eis)], dim=1)
    if union.shape[1]:
        inst = torch.repeat_interleave(torch.arange(B, device=device), torch.tensor(counts, device=device),
                                       output_size=union.shape[1])
        outside = ((union < off_d[inst]) | (union >= off_d[inst + 1])).any(dim=0)
        first_bad = torch.where(outside, inst, B).min().reshape(1)
    else:
        first_bad = torch.full((1,), B, dtype=torch.int64, device=device)

    def refuse(b):
        if b < B:
            raise ValueError(f"edge_index of instance {b} refers to nodes outside 0..{int(node_counts[b]) - 1}")

    try:
        g = build_csr(union, n, device, seg_rows=node_off if (B > 1 and task_rows != "edges") else None, points=points,
                      method="device")
    except _lib.DifuscoHipError:      # an endpoint outside the whole union: name the instance, as the host method does
        refuse(int(first_bad.cpu()))
        raise
    if task_rows == "edges":
        back = torch.cat([first_bad, g.rowptr[off_d].to(torch.int64)]).cpu().numpy()
        refuse(int(back[0]))
        if not np.array_equal(back[1:], inst_rows):
            raise RuntimeError("instance edges are not contiguous in CSR-slot order (an edge leaves its instance?)")
        if B > 1:
            g.seg_ptr = torch.from_numpy(inst_rows.astype(np.int32)).to(device)
            g.n_segments = B
    else:
        refuse(int(first_bad.cpu()))
    return g, union, inst_rows


def build_union_csr(edge_indices, node_counts, device, points=None, task_rows: str = "edges", method: str = "host"):
    """Disjoint union of B instances (``pl_meta_model.py:177-184``), each given by its own ``edge_index`` [2, E_b] over its
    own nodes 0..n_b-1, with ONE head-GroupNorm statistic segment per instance - what the solo call of each instance
    normalises over.  Returns ``(graph, union_edge_index, instance_rows)``: ``instance_rows`` [B+1] int64 numpy, the output
    rows (``"edges"``: TSP, ``"nodes"``: MIS) of every instance in caller order.  ``points`` [sum n_b, 2]: node renumbering
    for locality as in :func:`build_csr`; it never crosses an instance (``_id_blocks``), which is checked: the CSR slots of
    every instance must stay one contiguous range (otherwise a segment would mix instances).
    ``method="device"``: the same graph, errors and ``instance_rows`` through ``difusco_graph_build``; the union is concatenated
    and checked on the device (one synchronising readback for both checks) and ``union_edge_index`` stays there."""
    if check_graph_build(method) == "device":
        return _build_union_csr_device(edge_indices, node_counts, device, points, task_rows)
    eis = [e if isinstance(e, torch.Tensor) else torch.from_numpy(np.asarray(e)) for e in edge_indices]
    eis = [e.detach().to("cpu", torch.int64) for e in eis]
    node_off, inst_rows = union_rows([e.shape[1] for e in eis], node_counts, task_rows)
    for b, e in enumerate(eis):
        if e.numel() and (int(e.min()) < 0 or int(e.max()) >= int(node_counts[b])):
            raise ValueError(f"edge_index of instance {b} refers to nodes outside 0..{int(node_counts[b]) - 1}")
    union = torch.cat([e + int(node_off[b]) for b, e in enumerate(eis)], dim=1)
    n = int(node_off[-1])
    B = len(eis)
    if task_rows == "edges":
        # CSR slots are ordered by centre node: instance b holds the slots rowptr[node_off[b]] .. rowptr[node_off[b+1]]
        seg = None
        g = build_csr(union, n, device, points=points)
        rowptr = g.rowptr.cpu().numpy().astype(np.int64)
        seg = rowptr[node_off]
        if not np.array_equal(seg, inst_rows):
            raise RuntimeError("instance edges are not contiguous in CSR-slot order (an edge leaves its instance?)")
        if B > 1:
            g.seg_ptr = torch.from_numpy(seg.astype(np.int32)).to(device)
            g.n_segments = B
    else:
        g = build_csr(union, n, device, seg_rows=node_off if B > 1 else None, points=points)
    return g, union, inst_rows


def complete_graph_batch(batch: int, n: int, device) -> CsrGraph:
    """Dense mode (``gnn_encoder.py:350-381``): B graphs with all n*n ordered pairs, edge (b,i,j) at slot
    b*n*n + i*n + j - exactly the flattening of the reference's [B,V,V] tensors.  One GroupNorm
    statistic segment per sample (the dense head normalises a (B,H,V,V) tensor)."""
    rowptr = (torch.arange(batch * n + 1, dtype=torch.int64) * n).to(torch.int32)
    col = (torch.arange(n, dtype=torch.int32).repeat(batch * n)
           + torch.arange(batch, dtype=torch.int32).repeat_interleave(n * n) * n)
    row = torch.arange(batch * n, dtype=torch.int32).repeat_interleave(n)
    g = CsrGraph(n_nodes=batch * n, n_edges=batch * n * n, rowptr=rowptr.to(device), col=col.to(device), perm=None,
                 row=row.to(device))
    if batch > 1:
        g.seg_ptr = (torch.arange(batch + 1, dtype=torch.int64) * n * n).to(torch.int32).to(device)
        g.n_segments = batch
    return g


def complete_graph_union(sample_sizes, device) -> CsrGraph:
    """:func:`complete_graph_batch` for samples of different n: sample s holds all n_s * n_s ordered pairs of its own nodes
    ``node_off_s .. node_off_s + n_s - 1``, edge (s, i, j) at slot ``off_s + i * n_s + j`` (``off_s`` = the sum of n^2 over the
    samples before it), one GroupNorm statistic segment per sample.  Equal sizes give the arrays of ``complete_graph_batch``."""
    ns = np.asarray(list(sample_sizes), dtype=np.int64)
    if ns.ndim != 1 or ns.size < 1 or (ns < 1).any():
        raise ValueError("sample_sizes: at least one sample, every n >= 1")
    if int((ns * ns).sum()) >= 2 ** 31:
        raise ValueError("the union has 2^31 edges or more")
    node_off = np.concatenate([[0], np.cumsum(ns)])
    deg = np.repeat(ns, ns)                                       # node -> its degree = the n of its sample
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    row = np.repeat(np.arange(node_off[-1], dtype=np.int64), deg)
    first = np.repeat(np.repeat(node_off[:-1], ns), deg)          # slot -> first node of its sample
    col = first + (np.arange(rowptr[-1], dtype=np.int64) - rowptr[row])
    g = CsrGraph(n_nodes=int(node_off[-1]), n_edges=int(rowptr[-1]), rowptr=torch.from_numpy(rowptr.astype(np.int32)).to(device),
                 col=torch.from_numpy(col.astype(np.int32)).to(device), perm=None,
                 row=torch.from_numpy(row.astype(np.int32)).to(device))
    if ns.size > 1:
        g.seg_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(ns * ns)]).astype(np.int32)).to(device)
        g.n_segments = int(ns.size)
    return g


def edge_tiled_offsets(n_edges: int) -> torch.Tensor:
    """Flat offsets [E_pad, 256] (int64) of the tiled edge-feature layout the fused path keeps ``e`` in
    (``csrc/kernels.h: edge_tiled_offset``): rows padded to a multiple of 256 edges, tile = 32 edges,
    [slab f/16][(f/8)%2][((f/4)%2)*32 + s%32][f%4].  Test / debugging helper."""
    e_pad = (n_edges + 255) // 256 * 256
    s = torch.arange(e_pad, dtype=torch.int64)[:, None]
    f = torch.arange(256, dtype=torch.int64)[None, :]
    return (s >> 5) * 8192 + (f >> 4) * 512 + ((f >> 3) & 1) * 256 + ((((f >> 2) & 1) * 32) + (s & 31)) * 4 + (f & 3)


def to_tiled(e: torch.Tensor) -> torch.Tensor:
    """[E, 256] row-major -> flat tiled buffer of E_pad*256 floats (pad rows zero)."""
    off = edge_tiled_offsets(e.shape[0]).to(e.device)
    out = torch.zeros(off.shape[0] * 256, dtype=e.dtype, device=e.device)
    out[off[: e.shape[0]].reshape(-1)] = e.reshape(-1)
    return out


def from_tiled(buf: torch.Tensor, n_edges: int) -> torch.Tensor:
    off = edge_tiled_offsets(n_edges).to(buf.device)
    return buf[off[:n_edges].reshape(-1)].reshape(n_edges, 256)


def knn_edge_index_gpu(points, k: int, device="cuda:0", graphs: int = 1, sizes=None) -> torch.Tensor:
    """``edge_index`` int64 [2, G*n*k] on ``device`` in the reference's layout (``co_datasets/tsp_graph_dataset.py:
    53-62``; batch = disjoint union with node ids offset by g*n, ``pl_meta_model.py:177-184``), built by
    ``difusco_knn_graph``.  ``points``: float64 [G*n, 2] (numpy or tensor), G graphs of n points each.
    ``sizes=[n_0, ...]``: graphs of different sizes instead, ``points`` their concatenation [sum n_g, 2]; graph g holds the
    ``n_g * k`` columns after those of the graphs before it, its node ids offset by ``n_0 + ... + n_{g-1}``."""
    import ctypes
    L = _lib.lib()
    device = torch.device(device)
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64))
    if sizes is None:
        n = points.shape[0] // graphs
        if n * graphs != points.shape[0]:
            raise ValueError("points must hold `graphs` instances of equal size")
        sizes = [n] * graphs
    else:
        sizes = [int(n) for n in sizes]
        if graphs != 1:
            raise ValueError("give either `graphs` (equal sizes) or `sizes`")
        if len(sizes) < 1 or sum(sizes) != points.shape[0]:
            raise ValueError(f"sizes sum to {sum(sizes)}, points holds {points.shape[0]}")
        for g, n in enumerate(sizes):
            if n < k:
                raise ValueError(f"instance {g} has {n} nodes, fewer than k = {k}")
    pts = points.to(device=device, dtype=torch.float64).contiguous()
    ei = torch.empty((2, sum(sizes) * k), dtype=torch.int64, device=device)
    nbytes, need = ctypes.c_size_t(), 0
    for n in sorted(set(sizes)):                                  # one workspace, large enough for every size of the call
        _lib.check(L.difusco_knn_graph_workspace_bytes(n, k, ctypes.byref(nbytes)))
        need = max(need, nbytes.value)
    ws = _workspace(need, device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    node, col = 0, 0
    for n in sizes:
        _lib.check(L.difusco_knn_graph(n, k, ctypes.c_void_p(pts[node:].data_ptr()), node,
                                       ctypes.c_void_p(ei[0, col:].data_ptr()),
                                       ctypes.c_void_p(ei[1, col:].data_ptr()),
                                       ctypes.c_void_p(ws.data_ptr()), need, stream))
        node, col = node + n, col + n * k
    return ei
