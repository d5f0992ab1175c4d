"""Heatmap -> tour on the GPU box: drop-in for ``merge_tours`` of the reference
(``difusco/utils/tsp_utils.py:89-145``), sparse (k-NN) and dense heatmaps.

Same signature and return value as the reference function: ``(tours, merge_iterations)`` with one closed tour
(list starting and ending at node 0) per parallel sample and the mean of the per-sample iteration counters.  The
work goes through ``difusco_tsp_merge_tours`` of libdifusco_hip.so (pair keys, scores and the two sorts on the GPU,
the reference's route bookkeeping on the host); there is no CPU fallback.  Keyword-only extensions: ``device``,
``return_completed`` (adds the per-sample flag that says whether the tour was assembled from positive-score
candidate pairs, the regime pinned against the reference)."""
import ctypes

import numpy as np
import torch

from . import _lib


def _dev(x, dtype, device):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=device, dtype=dtype).contiguous()


def _ptr(t):
    """The address of a tensor's first element, as the library takes it."""
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _gpu_only(who, device):
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DifuscoHipError(f"{who} runs on the GPU only (no CPU fallback)")
    return device


def _workspace(size_fn, *sizes, device):
    """The workspace of one call: (uint8 device tensor, its bytes), sized by the entry's ``_workspace_bytes``."""
    nbytes = ctypes.c_size_t()
    _lib.check(size_fn(*sizes, ctypes.byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device), nbytes.value


def _philox_table(seeds, offsets, count, noun, device):
    """The Philox keys and first offsets of ``count`` streams (default 0; masked to 64 bits) as two int64 device tensors.  Both
    lengths are checked before either is uploaded."""
    mask = (1 << 64) - 1
    table = []
    for name, v in (("seeds", seeds), ("offsets", offsets)):
        v = [0] * count if v is None else [int(x) & mask for x in v]
        if len(v) != count:
            raise ValueError(f"{name}: {len(v)} entries for {count} {noun}")
        table.append(np.array(v, dtype=np.uint64).view(np.int64))
    return [torch.from_numpy(t).to(device) for t in table]


def merge_tours(adj_mat, np_points, edge_index_np, sparse_graph=False, parallel_sampling=1, *, device="cuda:0",
                return_completed=False):
    """``adj_mat``: [parallel_sampling * E] (or [parallel_sampling, E]) heat values in the edge order of
    ``edge_index_np`` ([2, E], the ONE graph's edges); ``np_points`` [N, 2].  numpy arrays or torch tensors.

    Candidate pairs are visited as a stable ascending sort of ``-(A + A^T) / dist`` visits them: scores ``> 0`` by decreasing
    score (``+inf`` first: positive heat between coincident cities, ``+inf`` heat); then the zero block (``S == +-0`` and
    every pair that is no edge) in flat-index order; then negative scores by decreasing score; then ``-inf`` (negative heat
    between coincident cities, ``-inf`` heat); NaN of either sign (``0/0``, NaN heat, ``inf + -inf``) last.  Equal scores,
    and the NaNs among themselves, by flat index.  ``completed`` is True exactly when all N - 1 insertions came from the
    scores ``> 0``; a NaN is never counted by ``merge_iterations`` before such a terminating entry."""
    device = torch.device(device)
    L = _lib.lib()
    pts = _dev(np_points, torch.float32, device)
    n = pts.shape[0]
    if not sparse_graph:
        # dense heatmaps [parallel_sampling, N, N] (tsp_utils.py:105-108: adj_mat[0] + adj_mat[0].T): the same greedy
        # insertion over the complete directed edge list - entry (i, j) at i * N + j, so that the pair sums
        # fl32(A_ij + A_ji), the doubled diagonal and the order of equal keys are those of the dense matrix
        idx = torch.arange(n, dtype=torch.int32, device=device)
        ei = torch.stack([idx.repeat_interleave(n), idx.repeat(n)])
    else:
        ei = _dev(edge_index_np, torch.int32, device)
    heat = _dev(adj_mat, torch.float32, device).reshape(parallel_sampling, -1)
    E = ei.shape[1]
    if heat.shape[1] != E:
        raise ValueError(f"adj_mat holds {heat.shape[1]} values per sample for {E} edges")
    ws, nbytes = _workspace(L.difusco_tsp_merge_workspace_bytes, E, device=device)
    row, col = ei[0].contiguous(), ei[1].contiguous()
    # one C call for all samples of the graph (the pair-key sort is shared; the per-sample loop of tsp_utils.py:100-145 runs
    # inside the library)
    tours_np = np.empty((parallel_sampling, n + 1), dtype=np.int32)
    iters = np.zeros(parallel_sampling, dtype=np.int64)
    done_np = np.zeros(parallel_sampling, dtype=np.int32)
    _lib.check(L.difusco_tsp_merge_tours(n, E, _ptr(row), _ptr(col), _ptr(heat), _ptr(pts), parallel_sampling, _ptr(ws), nbytes,
                                         tours_np.ctypes.data_as(ctypes.c_void_p), iters.ctypes.data_as(ctypes.c_void_p),
                                         done_np.ctypes.data_as(ctypes.c_void_p), _stream(device)))
    tours = [t.tolist() for t in tours_np]
    done = [bool(v) for v in done_np]
    merge_iterations = float(np.mean(iters))
    return (tours, merge_iterations, done) if return_completed else (tours, merge_iterations)


MERGE_METHODS = ("loop", "batched")
MERGE_STATES = ("auto", "global")
MERGE_STATE_GLOBAL = 1          # DIFUSCO_MERGE_STATE_GLOBAL


def check_merge_method(method):
    if method not in MERGE_METHODS:
        raise ValueError(f"merge method {method!r}: one of {MERGE_METHODS}")
    return method


def merge_tours_batch(heats, points, edge_indices, sparse_graph=False, parallel_sampling=1, *, device="cuda:0",
                      return_completed=False, state="auto"):
    """``merge_tours`` of G instances of ANY sizes in one library call (``difusco_tsp_merge_batch``: one launch sequence, the
    greedy insertion on the GPU, one wave per sample).  One entry per instance: ``heats[g]`` as ``sample_batch`` returns it
    ([P * E_g] sparse, [P, n_g, n_g] dense), ``points[g]`` [n_g, 2], ``edge_indices[g]`` [2, E_g] with node ids 0..n_g-1
    (``edge_indices=None`` for dense heatmaps: no index arrays are built).  ``parallel_sampling``: P, or one P per instance.
    ``state``: ``"auto"`` keeps a sample's path state in LDS when it fits, ``"global"`` in the workspace at any size (same
    results).  Returns, per instance, what ``merge_tours`` returns for it."""
    if state not in MERGE_STATES:
        raise ValueError(f"merge state {state!r}: one of {MERGE_STATES}")
    heats, points = list(heats), list(points)
    G = len(heats)
    if G < 1 or len(points) != G:
        raise ValueError(f"{len(points)} point arrays for {G} heatmaps (at least one instance)")
    if sparse_graph:
        if edge_indices is None or len(edge_indices) != G:
            raise ValueError(f"sparse heatmaps need one edge_index per instance ({G})")
    elif edge_indices is not None and any(e is not None for e in edge_indices):
        raise ValueError("dense heatmaps take edge_indices=None")
    par = [int(parallel_sampling)] * G if np.ndim(parallel_sampling) == 0 else [int(v) for v in parallel_sampling]
    if len(par) != G or min(par) < 1:
        raise ValueError(f"parallel_sampling: one value >= 1, or one per instance ({G})")
    device = torch.device(device)
    L = _lib.lib()
    pts = [_dev(p, torch.float32, device).reshape(-1, 2) for p in points]
    ns = [int(p.shape[0]) for p in pts]
    if sparse_graph:
        eis = [_dev(e, torch.int32, device) for e in edge_indices]
        Es = [int(e.shape[1]) for e in eis]
    else:
        Es = [n * n for n in ns]
    hs = [_dev(h, torch.float32, device).reshape(par[g], -1) for g, h in enumerate(heats)]
    for g in range(G):
        if hs[g].shape[1] != Es[g]:
            raise ValueError(f"heats[{g}] holds {hs[g].shape[1]} values per sample for {Es[g]} edges")
    graph_n, graph_e, graph_p = np.array(ns, dtype=np.int32), np.array(Es, dtype=np.int64), np.array(par, dtype=np.int32)
    heat = torch.cat([h.reshape(-1) for h in hs])
    pts_all = torch.cat(pts).contiguous()
    if sparse_graph:
        row, col = torch.cat([e[0] for e in eis]).contiguous(), torch.cat([e[1] for e in eis]).contiguous()
        row_p, col_p = _ptr(row), _ptr(col)
    else:
        row_p = col_p = None
    ws, nbytes = _workspace(L.difusco_tsp_merge_batch_workspace_bytes, G, graph_n.ctypes.data, graph_e.ctypes.data,
                            graph_p.ctypes.data, device=device)
    S = int(graph_p.sum())
    tours_np = np.empty(int(((graph_n.astype(np.int64) + 1) * graph_p).sum()), dtype=np.int32)
    iters, done_np = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int32)
    _lib.check(L.difusco_tsp_merge_batch(G, graph_n.ctypes.data, graph_e.ctypes.data, graph_p.ctypes.data, row_p, col_p,
                                         _ptr(heat), _ptr(pts_all), MERGE_STATE_GLOBAL if state == "global" else 0, _ptr(ws),
                                         nbytes, tours_np.ctypes.data, iters.ctypes.data, done_np.ctypes.data, _stream(device)))
    out, t0, s0 = [], 0, 0
    for g in range(G):
        t1, s1 = t0 + par[g] * (ns[g] + 1), s0 + par[g]
        tours = [t.tolist() for t in tours_np[t0:t1].reshape(par[g], ns[g] + 1)]
        merge_iterations = float(np.mean(iters[s0:s1]))
        done = [bool(v) for v in done_np[s0:s1]]
        out.append((tours, merge_iterations, done) if return_completed else (tours, merge_iterations))
        t0, s0 = t1, s1
    return out


TWO_OPT_METHODS = ("exact", "screened")


def check_two_opt_method(method):
    if method not in TWO_OPT_METHODS:
        raise ValueError(f"two-opt method {method!r}: one of {TWO_OPT_METHODS}")
    return method


def two_opt_screen_bound(max_abs_coord):
    """The margin ``eps`` of the screened 2-opt for an instance whose largest |coordinate| is ``max_abs_coord``: the float32
    evaluation of a move's change is proven to lie within ``eps`` of the float64 one (``difusco_tsp_two_opt_screen_bound``, a
    host function: no GPU).  None when no bound exists (non-finite, or so large or small that float32 over- or underflows); a
    screened call then runs the exact sweep."""
    eps = ctypes.c_double()
    rc = _lib.lib().difusco_tsp_two_opt_screen_bound(float(max_abs_coord), ctypes.byref(eps))
    if rc < 0:
        _lib.check(rc)
    return float(eps.value) if rc == 1 else None


TWO_OPT_MODES = ("launches", "resident")


def check_two_opt_mode(local_search, mode):
    """``two_opt_mode`` of ``solve_tsp``, ``solve_tsp_batch`` and the runner: ``"resident"`` runs the single-move 2-opt with one
    GPU block per instance, so it needs ``local_search="2opt"``; the 2-opt phases of the other searches have no resident form."""
    if mode not in TWO_OPT_MODES:
        raise ValueError(f"two-opt mode {mode!r}: one of {TWO_OPT_MODES}")
    if mode == "resident" and local_search != "2opt":
        raise ValueError(f"two_opt_mode='resident' runs the single-move 2-opt: it needs local_search='2opt', not {local_search!r}")
    return mode


def two_opt_resident_max_cells():
    """The largest group ``mode="resident"`` takes: ``P * (n + 1)`` entries of closed tours (a constant of the build, >= 2048)."""
    return int(_lib.lib().difusco_tsp_two_opt_resident_max_cells())


# The tour searches come in three forms.  ``_torch``: the tours [B, N + 1] of ONE instance; ``_grouped``: G instances of one
# size, points [G, N, 2] and tours [G * P, N + 1]; ``_ragged``: lists of G instances of any sizes.  All three run one ``_ragged``
# library entry on per-group arrays (``_per_group``, ``_RaggedBatch``) and differ in how they hand the results back (``_as_form``).


def _grouped_arrays(points, tours):
    """The arguments of a ``_grouped`` function as numpy arrays: (points [G, N, 2] float64, tours [G * P, N + 1], P)."""
    pts, t = np.asarray(points, dtype=np.float64), np.asarray(tours)
    if pts.ndim != 3 or pts.shape[2] != 2 or pts.shape[0] < 1:
        raise ValueError("points must be [groups, N, 2]")
    G, n = pts.shape[0], pts.shape[1]
    if t.ndim != 2 or t.shape[1] != n + 1 or t.shape[0] % G != 0 or t.shape[0] == 0:
        raise ValueError("tours must be [groups * P, N + 1] closed tours over the N points of their group")
    return pts, t, t.shape[0] // G


def _per_group(form, points, tours):
    """The arguments of a form as (float64 point arrays, int32 tour arrays), one of each per group."""
    if form == "torch":
        return [np.ascontiguousarray(points, dtype=np.float64)], [np.ascontiguousarray(tours, dtype=np.int32)]
    if form == "grouped":
        pts, t, P = _grouped_arrays(points, tours)
        return ([np.ascontiguousarray(p) for p in pts],
                [np.ascontiguousarray(t[g * P:(g + 1) * P], dtype=np.int32) for g in range(pts.shape[0])])
    return [np.ascontiguousarray(p, dtype=np.float64) for p in points], [np.ascontiguousarray(t, dtype=np.int32) for t in tours]


def _as_form(form, tours, stats):
    """(int64 tours per group, a dict of per-group arrays) as a form returns them: the one instance and ints; one array of all
    tours and the arrays; as they are."""
    if form == "torch":
        return tours[0], {k: int(v[0]) for k, v in stats.items()}
    if form == "grouped":
        return np.concatenate(tours, axis=0), stats
    return tours, stats


class _RaggedBatch:
    """Checked per-group point and tour arrays as every ``_ragged`` library entry takes them: the group tables on the host,
    all points and all tours as one device tensor each.  The library refines the tours in place."""

    def __init__(self, pts, trs, device):
        self.shapes = [t.shape for t in trs]
        self.groups = len(pts)
        self.group_n = np.array([p.shape[0] for p in pts], dtype=np.int32)
        self.group_tours = np.array([t.shape[0] for t in trs], dtype=np.int32)
        self.d_pts = _dev(np.concatenate([p.reshape(-1) for p in pts]), torch.float64, device)
        self.d_tours = _dev(np.concatenate([t.reshape(-1) for t in trs]), torch.int32, device)

    @property
    def sizes(self):
        """The first arguments of every ``_ragged_workspace_bytes``."""
        return self.groups, self.group_n.ctypes.data, self.group_tours.ctypes.data

    @property
    def head(self):
        """The first arguments of every ``_ragged`` entry."""
        return (*self.sizes, _ptr(self.d_pts), _ptr(self.d_tours))

    def group_stats(self):
        """The per-group counters of the multi-move entries, in the order of their arguments."""
        G = self.groups
        return {"two_opt_sweeps": np.zeros(G, dtype=np.int64), "or_opt_sweeps": np.zeros(G, dtype=np.int64),
                "rounds": np.zeros(G, dtype=np.int32), "two_opt_moves": np.zeros(G, dtype=np.int64),
                "or_opt_moves": np.zeros(G, dtype=np.int64)}

    def read_tours(self):
        """The tours as they are on the device now: int64 numpy, one array per group."""
        flat = self.d_tours.cpu().numpy().astype(np.int64)
        cuts = np.cumsum([rows * width for rows, width in self.shapes])[:-1]
        return [f.reshape(shape) for f, shape in zip(np.split(flat, cuts), self.shapes)]


def _two_opt_resident(form, points, tours, max_iterations, device, method, stats, moves_per_launch):
    """``batched_two_opt_<form>`` with ``mode="resident"``: one ``difusco_tsp_two_opt_resident`` call on the per-group arrays."""
    pts, trs = _per_group(form, points, tours)
    if len(pts) < 1 or len(trs) != len(pts):
        raise ValueError(f"{len(trs)} tour arrays for {len(pts)} instances (at least one instance)")
    for g, (p, t) in enumerate(zip(pts, trs)):
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"points of instance {g} must be [n, 2]")
        if t.ndim != 2 or t.shape[1] != p.shape[0] + 1 or t.shape[0] < 1:
            raise ValueError(f"tours of instance {g} must be [P, {p.shape[0] + 1}] closed tours over the {p.shape[0]} points, P >= 1")
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    code = TWO_OPT_METHODS.index(method)
    ws, nbytes = _workspace(L.difusco_tsp_two_opt_resident_workspace_bytes, *batch.sizes, code, device=device)
    its = np.zeros(batch.groups, dtype=np.int64)
    pairs, syncs = ctypes.c_int64(), ctypes.c_int32()
    _lib.check(L.difusco_tsp_two_opt_resident(*batch.head, int(max_iterations), code, int(moves_per_launch), _ptr(ws), nbytes,
                                              its.ctypes.data, ctypes.byref(pairs), ctypes.byref(syncs), _stream(device)))
    if stats is not None:
        stats["exact_pairs"], stats["host_syncs"] = int(pairs.value), int(syncs.value)
    out, st = _as_form(form, batch.read_tours(), {"iterations": its})
    return out, st["iterations"]


def batched_two_opt_torch(points, tour, max_iterations=1000, device="cuda:0", *, method="exact", stats=None, mode="launches",
                          moves_per_launch=0):
    """Drop-in for ``batched_two_opt_torch`` of the reference (``difusco/utils/tsp_utils.py:12-49``): ``points``
    float64 [N,2] numpy, ``tour`` int [B, N+1] numpy (closed tours over the same points); returns
    ``(tour int64 numpy [B, N+1], iterator)``.  Runs ``difusco_tsp_two_opt``; GPU only.  ``method="screened"`` runs
    ``difusco_tsp_two_opt_screened``: the same tours and iterator, float64 only for the moves a float32 screen cannot rule out;
    ``stats`` (a dict) then receives ``exact_pairs``, the number of pairs that took the float64 path.  ``mode="resident"`` runs
    ``difusco_tsp_two_opt_resident`` instead: one GPU block keeps the tours in LDS and applies move after move without a launch
    or a host read per move (at most ``moves_per_launch`` per launch, 0 = the library's default); the same tours and iterator
    with either ``method``, for at most ``two_opt_resident_max_cells()`` tour entries (``B * (N + 1)``; more raises
    ``DifuscoHipError``, there is no fallback); ``stats`` receives ``exact_pairs`` and ``host_syncs``."""
    method = check_two_opt_method(method)
    device = _gpu_only("batched_two_opt_torch of difusco_amd", device)
    if check_two_opt_mode("2opt", mode) == "resident":
        return _two_opt_resident("torch", points, tour, max_iterations, device, method, stats, moves_per_launch)
    pts, tours = np.asarray(points, dtype=np.float64), np.asarray(tour)
    if tours.ndim != 2 or tours.shape[1] != pts.shape[0] + 1:
        raise ValueError("tour must be [batch, N + 1] over the N points")
    n, batch = pts.shape[0], tours.shape[0]
    pts, tours = _dev(pts, torch.float64, device), _dev(tours, torch.int32, device)
    L = _lib.lib()
    screened = method == "screened"
    ws, nbytes = _workspace(L.difusco_tsp_two_opt_screened_workspace_bytes if screened else L.difusco_tsp_two_opt_workspace_bytes,
                            n, batch, device=device)
    it, pairs = ctypes.c_int64(), ctypes.c_int64()
    head = (n, batch, _ptr(pts), _ptr(tours), int(max_iterations), _ptr(ws), nbytes, ctypes.byref(it))
    if screened:
        _lib.check(L.difusco_tsp_two_opt_screened(*head, ctypes.byref(pairs), _stream(device)))
        if stats is not None:
            stats["exact_pairs"] = int(pairs.value)
    else:
        _lib.check(L.difusco_tsp_two_opt(*head, _stream(device)))
    return tours.cpu().numpy().astype(np.int64), int(it.value)


def batched_two_opt_grouped(points, tours, max_iterations=1000, device="cuda:0", *, method="exact", stats=None, mode="launches",
                            moves_per_launch=0):
    """``batched_two_opt_torch`` of G instances at once: ``points`` float64 [G, N, 2], ``tours`` int [G * P, N + 1] with the P
    tours of instance g at rows g P .. g P + P - 1.  Every instance gets exactly what ``batched_two_opt_torch(points[g],
    tours[g P:(g+1) P])`` returns (its own stop test and iteration count); runs ``difusco_tsp_two_opt_grouped``, GPU only.
    Returns ``(tours int64 numpy [G * P, N + 1], iterations int64 numpy [G])``.  ``method`` / ``stats``: as
    ``batched_two_opt_torch`` (``difusco_tsp_two_opt_grouped_screened``).  ``mode`` / ``moves_per_launch``: as
    ``batched_two_opt_torch``, one block per instance; the limit holds for every instance (``P * (N + 1)`` entries)."""
    method = check_two_opt_method(method)
    device = _gpu_only("batched_two_opt_grouped", device)
    if check_two_opt_mode("2opt", mode) == "resident":
        return _two_opt_resident("grouped", points, tours, max_iterations, device, method, stats, moves_per_launch)
    pts, t, P = _grouped_arrays(points, tours)
    G, n = pts.shape[0], pts.shape[1]
    pts, t = _dev(pts, torch.float64, device), _dev(t, torch.int32, device)
    L = _lib.lib()
    screened = method == "screened"
    ws, nbytes = _workspace(L.difusco_tsp_two_opt_grouped_screened_workspace_bytes if screened
                            else L.difusco_tsp_two_opt_grouped_workspace_bytes, n, G, P, device=device)
    its = np.zeros(G, dtype=np.int64)
    pairs = ctypes.c_int64()
    head = (n, G, P, _ptr(pts), _ptr(t), int(max_iterations), _ptr(ws), nbytes, its.ctypes.data)
    if screened:
        _lib.check(L.difusco_tsp_two_opt_grouped_screened(*head, ctypes.byref(pairs), _stream(device)))
        if stats is not None:
            stats["exact_pairs"] = int(pairs.value)
    else:
        _lib.check(L.difusco_tsp_two_opt_grouped(*head, _stream(device)))
    return t.cpu().numpy().astype(np.int64), its


def batched_two_opt_ragged(points_list, tours_list, max_iterations=1000, device="cuda:0", *, method="exact", stats=None,
                           mode="launches", moves_per_launch=0):
    """``batched_two_opt_torch`` of G instances of ANY sizes at once: ``points_list[g]`` float64 [n_g, 2], ``tours_list[g]`` int
    [P_g, n_g + 1] closed tours over them.  Every instance gets exactly what ``batched_two_opt_torch(points_list[g],
    tours_list[g])`` returns (its own stop test, iteration count and tie rule); runs ``difusco_tsp_two_opt_ragged``, GPU only.
    Returns ``(list of int64 numpy [P_g, n_g + 1], iterations int64 numpy [G])``.  ``method`` / ``stats``: as
    ``batched_two_opt_torch``; with ``method="exact"`` ``exact_pairs`` counts every pair of every sweep.  ``mode`` /
    ``moves_per_launch``: as ``batched_two_opt_torch``, one block per instance (``P_g * (n_g + 1)`` entries each); an instance
    without a screen bound then takes the exact sweep for itself only."""
    method = check_two_opt_method(method)
    device = _gpu_only("batched_two_opt_ragged", device)
    if check_two_opt_mode("2opt", mode) == "resident":
        return _two_opt_resident("ragged", points_list, tours_list, max_iterations, device, method, stats, moves_per_launch)
    pts, trs = _per_group("ragged", points_list, tours_list)
    G = len(pts)
    if G < 1 or len(trs) != G:
        raise ValueError(f"{len(trs)} tour arrays for {G} instances (at least one instance)")
    for g, (p, t) in enumerate(zip(pts, trs)):
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"points_list[{g}] must be [n, 2]")
        if t.ndim != 2 or t.shape[1] != p.shape[0] + 1 or t.shape[0] < 1:
            raise ValueError(f"tours_list[{g}] must be [P, {p.shape[0] + 1}] closed tours over the {p.shape[0]} points, P >= 1")
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    code = TWO_OPT_METHODS.index(method)
    ws, nbytes = _workspace(L.difusco_tsp_two_opt_ragged_workspace_bytes, *batch.sizes, code, device=device)
    its = np.zeros(G, dtype=np.int64)
    pairs = ctypes.c_int64()
    _lib.check(L.difusco_tsp_two_opt_ragged(*batch.head, int(max_iterations), code, _ptr(ws), nbytes, its.ctypes.data,
                                            ctypes.byref(pairs), _stream(device)))
    if stats is not None:
        stats["exact_pairs"] = int(pairs.value)
    return batch.read_tours(), its


LOCAL_SEARCHES = ("2opt", "2opt+oropt", "multi2opt", "multi2opt+oropt", "nbr2opt+oropt")


def check_local_search(local_search, two_opt_method="exact"):
    if local_search not in LOCAL_SEARCHES:
        raise ValueError(f"local search {local_search!r}: one of {LOCAL_SEARCHES}")
    if local_search != "2opt" and two_opt_method != "exact":
        raise ValueError(f"local_search={local_search!r} runs the exact 2-opt sweep: two_opt_method={two_opt_method!r} is not built")
    return local_search


def _local_search_checked(who, pts, trs, max_iterations, max_rounds, device):
    """The argument checks of the local-search functions (before any library call) on float64 point arrays ``pts`` and int32
    tour arrays ``trs``, one per group."""
    device = _gpu_only(who, device)
    if int(max_iterations) != max_iterations or max_iterations < 0:
        raise ValueError(f"max_iterations = {max_iterations!r}: an integer >= 0")
    if int(max_rounds) != max_rounds or max_rounds < 1:
        raise ValueError(f"max_rounds = {max_rounds!r}: an integer >= 1")
    if len(pts) < 1 or len(trs) != len(pts):
        raise ValueError(f"{len(trs)} tour arrays for {len(pts)} instances (at least one instance)")
    for g, (p, t) in enumerate(zip(pts, trs)):
        if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 4:
            raise ValueError(f"points of instance {g} must be [n, 2] with n >= 4")
        if t.ndim != 2 or t.shape[1] != p.shape[0] + 1 or t.shape[0] < 1:
            raise ValueError(f"tours of instance {g} must be [P, {p.shape[0] + 1}] closed tours over the {p.shape[0]} points, P >= 1")
    return device


TSP_LOCAL_SEARCH_MODES = ("launches", "resident")


def check_tsp_local_search_mode(local_search, mode):
    """``local_search_mode`` of ``solve_tsp``, ``solve_tsp_batch`` and the runner: ``"resident"`` runs the 2-opt + Or-opt search
    with one GPU block per instance, so it needs ``local_search="2opt+oropt"``; the other searches have no such form (the
    single-move 2-opt has its own, ``two_opt_mode``)."""
    if mode not in TSP_LOCAL_SEARCH_MODES:
        raise ValueError(f"local search mode {mode!r}: one of {TSP_LOCAL_SEARCH_MODES}")
    if mode == "resident" and local_search != "2opt+oropt":
        raise ValueError(f"local_search_mode={mode!r} runs the 2-opt + Or-opt search: it needs local_search='2opt+oropt', "
                         f"not {local_search!r}")
    return mode


def local_search_resident_max_cells():
    """The largest group ``batched_local_search_*(mode="resident")`` takes: ``P * (n + 1)`` entries of closed tours (a constant
    of the build, >= 2048)."""
    return int(_lib.lib().difusco_tsp_local_search_resident_max_cells())


def _local_search(form, points, tours, max_iterations, device, max_rounds, stats, mode="launches", steps_per_launch=0):
    """``batched_local_search_<form>``: the checks and one ``difusco_tsp_local_search_ragged`` call, or with ``mode="resident"``
    one ``difusco_tsp_local_search_resident`` call, on the per-group arrays."""
    resident = check_tsp_local_search_mode("2opt+oropt", mode) == "resident"
    pts, trs = _per_group(form, points, tours)
    device = _local_search_checked(f"batched_local_search_{form}", pts, trs, max_iterations, max_rounds, device)
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    G = batch.groups
    st = {"two_opt_iterations": np.zeros(G, dtype=np.int64), "or_opt_iterations": np.zeros(G, dtype=np.int64),
          "rounds": np.zeros(G, dtype=np.int32)}
    if resident:
        ws, nbytes = _workspace(L.difusco_tsp_local_search_resident_workspace_bytes, *batch.sizes, device=device)
        syncs = ctypes.c_int32()
        _lib.check(L.difusco_tsp_local_search_resident(*batch.head, int(max_iterations), int(max_rounds), int(steps_per_launch),
                                                       _ptr(ws), nbytes, *(v.ctypes.data for v in st.values()), ctypes.byref(syncs),
                                                       _stream(device)))
    else:
        ws, nbytes = _workspace(L.difusco_tsp_local_search_ragged_workspace_bytes, *batch.sizes, device=device)
        _lib.check(L.difusco_tsp_local_search_ragged(*batch.head, int(max_iterations), int(max_rounds), _ptr(ws), nbytes,
                                                     *(v.ctypes.data for v in st.values()), _stream(device)))
    out, st = _as_form(form, batch.read_tours(), st)
    if stats is not None:
        stats["or_opt_iterations"], stats["rounds"] = st["or_opt_iterations"], st["rounds"]
        if resident:
            stats["host_syncs"] = int(syncs.value)
    return out, st["two_opt_iterations"]


def batched_local_search_torch(points, tour, max_iterations=1000, device="cuda:0", *, max_rounds=16, stats=None, mode="launches",
                               steps_per_launch=0):
    """2-opt + Or-opt local search of the tours of ONE instance, the arguments of ``batched_two_opt_torch``: rounds of a 2-opt
    phase (exactly ``batched_two_opt_torch`` with ``max_iterations``) and an Or-opt phase (every tour moves its best segment of
    1-3 cities, forwards or reversed, while that shortens it by more than 1e-6; at most ``max_iterations`` iterations) until an
    Or-opt phase applies nothing or ``max_rounds`` rounds ran (``difusco_tsp_local_search_ragged``, include/difusco_hip.h; GPU
    only).  No tour ends longer than 2-opt alone leaves it.  Returns ``(tour int64 numpy [B, N+1], two_opt_iterations)``;
    ``stats`` (a dict) receives ``or_opt_iterations`` and ``rounds``.  ``mode="resident"`` runs
    ``difusco_tsp_local_search_resident`` instead: one GPU block keeps the tours in LDS through both phases and all rounds,
    without a launch or a host read per step (at most ``steps_per_launch`` 2-opt moves and Or-opt iterations per launch, 0 =
    the library's default); the same tours and counters, for at most ``local_search_resident_max_cells()`` tour entries
    (``B * (N + 1)``; more raises ``DifuscoHipError``, there is no fallback); ``stats`` also receives ``host_syncs``."""
    return _local_search("torch", points, tour, max_iterations, device, max_rounds, stats, mode, steps_per_launch)


def batched_local_search_grouped(points, tours, max_iterations=1000, device="cuda:0", *, max_rounds=16, stats=None, mode="launches",
                                 steps_per_launch=0):
    """``batched_local_search_torch`` of G instances at once, the arguments of ``batched_two_opt_grouped``: ``points`` float64
    [G, N, 2], ``tours`` int [G * P, N + 1].  Every instance gets what its own ``batched_local_search_torch`` call returns.
    Returns ``(tours int64 numpy [G * P, N + 1], two_opt_iterations int64 numpy [G])``; ``stats`` receives ``or_opt_iterations``
    (int64 [G]) and ``rounds`` (int32 [G]).  ``mode`` / ``steps_per_launch``: as ``batched_local_search_torch``, one block per
    instance; the limit holds for every instance (``P * (N + 1)`` entries)."""
    return _local_search("grouped", points, tours, max_iterations, device, max_rounds, stats, mode, steps_per_launch)


def batched_local_search_ragged(points_list, tours_list, max_iterations=1000, device="cuda:0", *, max_rounds=16, stats=None,
                                mode="launches", steps_per_launch=0):
    """``batched_local_search_torch`` of G instances of ANY sizes at once, the arguments of ``batched_two_opt_ragged``.  Returns
    ``(list of int64 numpy [P_g, n_g + 1], two_opt_iterations int64 numpy [G])``; ``stats``: as ``batched_local_search_grouped``.
    ``mode`` / ``steps_per_launch``: as ``batched_local_search_torch`` (``P_g * (n_g + 1)`` entries per instance)."""
    return _local_search("ragged", points_list, tours_list, max_iterations, device, max_rounds, stats, mode, steps_per_launch)


def _multi_move_checked(who, pts, trs, max_iterations, max_rounds, select_rounds, device):
    """The argument checks of the multi-move functions (before any library call)."""
    if int(select_rounds) != select_rounds or select_rounds < 1:
        raise ValueError(f"select_rounds = {select_rounds!r}: an integer >= 1")
    return _local_search_checked(who, pts, trs, max_iterations, max_rounds, device)


def _multi_two_opt(form, points, tours, max_iterations, device, select_rounds, stats):
    """``batched_multi_two_opt_<form>``: the checks and one ``difusco_tsp_multi_two_opt_ragged`` call."""
    pts, trs = _per_group(form, points, tours)
    device = _multi_move_checked(f"batched_multi_two_opt_{form}", pts, trs, max_iterations, 1, select_rounds, device)
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    ws, nbytes = _workspace(L.difusco_tsp_multi_two_opt_ragged_workspace_bytes, *batch.sizes, device=device)
    st = {"sweeps": np.zeros(batch.groups, dtype=np.int64), "moves": np.zeros(batch.groups, dtype=np.int64)}
    _lib.check(L.difusco_tsp_multi_two_opt_ragged(*batch.head, int(max_iterations), int(select_rounds), _ptr(ws), nbytes,
                                                  st["sweeps"].ctypes.data, st["moves"].ctypes.data, _stream(device)))
    out, st = _as_form(form, batch.read_tours(), st)
    if stats is not None:
        stats["moves"] = st["moves"]
    return out, st["sweeps"]


def batched_multi_two_opt_torch(points, tour, max_iterations=1000, device="cuda:0", *, select_rounds=4, stats=None):
    """Multi-move 2-opt of the tours of ONE instance, the arguments of ``batched_two_opt_torch``: every sweep of all pairs applies
    a set of improving 2-opt moves with pairwise disjoint position ranges, chosen in at most ``select_rounds`` rounds (the rule:
    ``difusco_tsp_multi_two_opt_ragged``, include/difusco_hip.h; GPU only; not the reference's one move per sweep, so another
    2-opt optimum).  Every tour runs on its own; at most ``max_iterations`` sweeps.  Returns ``(tour int64 numpy [B, N+1],
    sweeps)``; ``stats`` (a dict) receives ``moves``, the moves applied over all tours."""
    return _multi_two_opt("torch", points, tour, max_iterations, device, select_rounds, stats)


def batched_multi_two_opt_grouped(points, tours, max_iterations=1000, device="cuda:0", *, select_rounds=4, stats=None):
    """``batched_multi_two_opt_torch`` of G instances at once, the arguments of ``batched_two_opt_grouped``: ``points`` float64
    [G, N, 2], ``tours`` int [G * P, N + 1].  Every instance gets what its own ``batched_multi_two_opt_torch`` call returns.
    Returns ``(tours int64 numpy [G * P, N + 1], sweeps int64 numpy [G])``; ``stats`` receives ``moves`` (int64 [G])."""
    return _multi_two_opt("grouped", points, tours, max_iterations, device, select_rounds, stats)


def batched_multi_two_opt_ragged(points_list, tours_list, max_iterations=1000, device="cuda:0", *, select_rounds=4, stats=None):
    """``batched_multi_two_opt_torch`` of G instances of ANY sizes at once, the arguments of ``batched_two_opt_ragged``.  Returns
    ``(list of int64 numpy [P_g, n_g + 1], sweeps int64 numpy [G])``; ``stats``: as ``batched_multi_two_opt_grouped``."""
    return _multi_two_opt("ragged", points_list, tours_list, max_iterations, device, select_rounds, stats)


TSP_CLOSINGS = ("full", "none")           # --tsp_local_search_closing of the runner: closing=True / False


def check_tsp_candidates(local_search, candidates, kicks=0, window=0, two_opt_mode="launches"):
    """``local_search_candidates`` of ``solve_tsp``, ``solve_tsp_batch`` and the runner (0: off): the neighbour-list sweeps are
    a mode of the multi-move 2-opt (``local_search="multi2opt"`` with K > 0) and the search ``local_search="nbr2opt+oropt"``,
    which needs K >= 1; the kicked, windowed and resident searches have no neighbour-list form.  The neighbour-list 2-opt +
    Or-opt search has a NAME OF ITS OWN instead of being ``"multi2opt+oropt"`` with K > 0, because that combination is refused,
    and the host tests of the neighbour-list 2-opt (``check_tsp_candidates``, the runner's parser) pin the refusal."""
    if int(candidates) != candidates or candidates < 0:
        raise ValueError(f"local_search_candidates = {candidates!r}: an integer >= 0")
    if local_search == "nbr2opt+oropt":
        # a name of its own: "multi2opt+oropt" with candidates stays refused below, as the host tests of the neighbour-list 2-opt pin
        if candidates < 1:
            raise ValueError("local_search='nbr2opt+oropt' runs the neighbour-list 2-opt + Or-opt search: it needs "
                             "local_search_candidates = K >= 1, not 0")
        if kicks > 0 or window > 0:
            raise ValueError(f"local_search='nbr2opt+oropt' combines with neither kicks nor windows")
        if two_opt_mode == "resident":
            raise ValueError("local_search='nbr2opt+oropt' does not combine with two_opt_mode='resident'")
        return int(candidates)
    if candidates > 0:
        if local_search != "multi2opt":
            raise ValueError(f"local_search_candidates = {candidates} runs the neighbour-list multi-move 2-opt: it needs "
                             f"local_search='multi2opt', not {local_search!r}")
        if kicks > 0 or window > 0:
            raise ValueError(f"local_search_candidates = {candidates} combines with neither kicks nor windows")
        if two_opt_mode == "resident":
            raise ValueError(f"local_search_candidates = {candidates} does not combine with two_opt_mode='resident'")
    return int(candidates)


def tsp_candidate_lists(edge_index, sizes, candidates):
    """The candidate lists of ``batched_nbr_two_opt_*`` from a k-NN ``edge_index`` ([2, sum n_g k], the layout of
    ``knn_edge_index_gpu``: the k neighbours of a node in a row, nearest first, node ids offset by the sizes before; or a list of
    one [2, n_g k] per graph with local node ids): per node
    its first ``candidates`` neighbours that are not the node itself, order kept, local to the graph.  Needs ``candidates <=
    k - 1``.  Returns one int32 device tensor [n_g, candidates] per graph."""
    sizes = [int(n) for n in sizes]
    total = sum(sizes)
    local = isinstance(edge_index, (list, tuple))
    cols = torch.cat([e[1] for e in edge_index]) if local else edge_index[1]
    if cols.ndim != 1 or cols.shape[0] % total != 0:
        raise ValueError(f"edge_index must be [2, {total} k]")
    k = cols.shape[0] // total
    if not 1 <= candidates <= k - 1:
        raise ValueError(f"candidates = {candidates}: 1 .. {k - 1} of a graph with k = {k}")
    nb = cols.reshape(total, k)
    first = torch.repeat_interleave(torch.tensor(np.cumsum([0] + sizes[:-1]), device=nb.device),
                                    torch.tensor(sizes, device=nb.device)).reshape(total, 1)
    if not local:
        nb = nb - first
    me = torch.arange(total, device=nb.device).reshape(total, 1) - first
    order = torch.argsort((nb == me).to(torch.int8), dim=1, stable=True)                 # the node itself last, the rest as they were
    lists = torch.gather(nb, 1, order)[:, :candidates].to(torch.int32)
    return list(torch.split(lists, sizes))


def _nbr_lists(form, pts, neighbors, candidates, device):
    """The checked lists of ``batched_nbr_two_opt_<form>`` as one flat int32 device tensor and their K."""
    sizes = [p.shape[0] for p in pts]
    if neighbors is None:
        if int(candidates) != candidates or candidates < 1:
            raise ValueError(f"candidates = {candidates!r}: an integer >= 1")
        for g, n in enumerate(sizes):
            if candidates > n - 1:
                raise ValueError(f"candidates = {candidates}: instance {g} has {n} points, at most {n - 1} other cities")
        from .graph import knn_edge_index_gpu
        ei = knn_edge_index_gpu(np.concatenate(pts), int(candidates) + 1, device=device, sizes=sizes)
        per = tsp_candidate_lists(ei, sizes, int(candidates))
    else:
        if form == "torch":
            per = [neighbors]
        elif form == "grouped":
            if len(neighbors) != len(pts):
                raise ValueError(f"neighbors holds {len(neighbors)} instances for {len(pts)}")
            per = list(neighbors)
        else:
            per = list(neighbors)
            if len(per) != len(pts):
                raise ValueError(f"{len(per)} neighbour arrays for {len(pts)} instances")
        per = [nb if isinstance(nb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(nb)) for nb in per]
        K = per[0].shape[1] if per[0].ndim == 2 else 0
        for g, (nb, n) in enumerate(zip(per, sizes)):
            if nb.ndim != 2 or nb.shape[0] != n or nb.shape[1] != K or K < 1:
                raise ValueError(f"neighbors of instance {g} must be [{n}, K] with one K >= 1 for the call")
            if nb.dtype.is_floating_point or nb.dtype.is_complex or nb.dtype == torch.bool:
                raise ValueError(f"neighbors of instance {g} must be integers, not {nb.dtype}")
    K = int(per[0].shape[1])
    flat = torch.cat([nb.to(device=device, dtype=torch.int32).reshape(-1) for nb in per]).contiguous()
    return flat, K


def _nbr_two_opt(form, points, tours, max_iterations, device, candidates, neighbors, closing, select_rounds, stats):
    """``batched_nbr_two_opt_<form>``: the checks and one ``difusco_tsp_nbr_two_opt_ragged`` call."""
    pts, trs = _per_group(form, points, tours)
    device = _multi_move_checked(f"batched_nbr_two_opt_{form}", pts, trs, max_iterations, 1, select_rounds, device)
    lists, K = _nbr_lists(form, pts, neighbors, candidates, device)
    closing = int(bool(closing))
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    ws, nbytes = _workspace(L.difusco_tsp_nbr_two_opt_ragged_workspace_bytes, *batch.sizes, K, closing, device=device)
    G = batch.groups
    st = {"sweeps": np.zeros(G, dtype=np.int64), "full_sweeps": np.zeros(G, dtype=np.int64), "moves": np.zeros(G, dtype=np.int64)}
    _lib.check(L.difusco_tsp_nbr_two_opt_ragged(*batch.head, _ptr(lists), K, closing, int(max_iterations), int(select_rounds),
                                                _ptr(ws), nbytes, *(v.ctypes.data for v in st.values()), _stream(device)))
    out, st = _as_form(form, batch.read_tours(), st)
    if stats is not None:
        stats.update(st)
    return out, st["sweeps"]


def batched_nbr_two_opt_torch(points, tour, max_iterations=1000, device="cuda:0", *, candidates=8, neighbors=None, closing=True,
                              select_rounds=4, stats=None):
    """Neighbour-list multi-move 2-opt of the tours of ONE instance, the arguments of ``batched_multi_two_opt_torch``: a sweep
    evaluates only the pairs whose new head or tail edge joins a city to one of its listed neighbours, O(N K) instead of all
    pairs, and applies the disjoint improving moves it selects; a tour whose neighbour sweep finds nothing stops
    (``closing=False``) or goes on with the full sweeps of ``batched_multi_two_opt_torch`` until one finds nothing
    (``closing=True``: the end tour is a full 2-opt optimum).  The rule: ``difusco_tsp_nbr_two_opt_ragged``,
    include/difusco_hip.h; GPU only.  ``neighbors``: int [N, K], row a the listed cities of a (an entry outside 0 .. N-1 or
    equal to a is a pad), numpy or a tensor; None builds the ``candidates`` nearest other cities of every city with
    ``knn_edge_index_gpu`` (``candidates <= N - 1``).  At most ``max_iterations`` sweeps over both phases.  Returns ``(tour
    int64 numpy [B, N+1], sweeps)``; ``stats`` (a dict) receives ``sweeps``, ``full_sweeps`` (those counted in the closing
    phase) and ``moves``."""
    return _nbr_two_opt("torch", points, tour, max_iterations, device, candidates, neighbors, closing, select_rounds, stats)


def batched_nbr_two_opt_grouped(points, tours, max_iterations=1000, device="cuda:0", *, candidates=8, neighbors=None, closing=True,
                                select_rounds=4, stats=None):
    """``batched_nbr_two_opt_torch`` of G instances at once, the arguments of ``batched_multi_two_opt_grouped``; ``neighbors``:
    int [G, N, K] or None.  Every instance gets what its own ``batched_nbr_two_opt_torch`` call returns.  Returns ``(tours int64
    numpy [G * P, N + 1], sweeps int64 numpy [G])``; ``stats`` receives ``sweeps``, ``full_sweeps`` and ``moves`` (int64 [G])."""
    return _nbr_two_opt("grouped", points, tours, max_iterations, device, candidates, neighbors, closing, select_rounds, stats)


def batched_nbr_two_opt_ragged(points_list, tours_list, max_iterations=1000, device="cuda:0", *, candidates=8, neighbors=None,
                               closing=True, select_rounds=4, stats=None):
    """``batched_nbr_two_opt_torch`` of G instances of ANY sizes at once, the arguments of ``batched_multi_two_opt_ragged``;
    ``neighbors``: a list of int [n_g, K] with one K, or None.  Returns ``(list of int64 numpy [P_g, n_g + 1], sweeps int64
    numpy [G])``; ``stats``: as ``batched_nbr_two_opt_grouped``."""
    return _nbr_two_opt("ragged", points_list, tours_list, max_iterations, device, candidates, neighbors, closing, select_rounds,
                        stats)


def _multi_local_search(form, points, tours, max_iterations, device, max_rounds, select_rounds):
    """``batched_multi_local_search_<form>``: the checks and one ``difusco_tsp_multi_local_search_ragged`` call."""
    pts, trs = _per_group(form, points, tours)
    device = _multi_move_checked(f"batched_multi_local_search_{form}", pts, trs, max_iterations, max_rounds, select_rounds, device)
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    ws, nbytes = _workspace(L.difusco_tsp_multi_local_search_ragged_workspace_bytes, *batch.sizes, device=device)
    st = batch.group_stats()
    _lib.check(L.difusco_tsp_multi_local_search_ragged(*batch.head, int(max_iterations), int(max_rounds), int(select_rounds),
                                                       _ptr(ws), nbytes, *(v.ctypes.data for v in st.values()), _stream(device)))
    return _as_form(form, batch.read_tours(), st)


def batched_multi_local_search_torch(points, tour, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4):
    """Multi-move 2-opt + Or-opt local search of the tours of ONE instance, the arguments of ``batched_two_opt_torch``: every
    tour runs rounds of a multi-move 2-opt phase (the sweeps of ``batched_multi_two_opt_torch``) and a multi-move Or-opt phase
    (every sweep moves a set of segments of 1-3 cities, forwards or reversed, with pairwise disjoint position ranges) until an
    Or-opt phase applies nothing, ``max_rounds`` rounds ran or the tour moved in ``max_iterations`` sweeps (the rule:
    ``difusco_tsp_multi_local_search_ragged``, include/difusco_hip.h; GPU only).  No tour ends longer than the multi-move 2-opt
    leaves it.  Returns ``(tour int64 numpy [B, N+1], stats)``: ``stats`` holds ``two_opt_sweeps``, ``or_opt_sweeps``, ``rounds``
    (the maxima over the tours) and ``two_opt_moves``, ``or_opt_moves`` (the sums over the tours), ints."""
    return _multi_local_search("torch", points, tour, max_iterations, device, max_rounds, select_rounds)


def batched_multi_local_search_grouped(points, tours, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4):
    """``batched_multi_local_search_torch`` of G instances at once, the arguments of ``batched_two_opt_grouped``: ``points``
    float64 [G, N, 2], ``tours`` int [G * P, N + 1].  Every instance gets what its own ``batched_multi_local_search_torch`` call
    returns.  Returns ``(tours int64 numpy [G * P, N + 1], stats)``; the entries of ``stats`` are numpy arrays [G]."""
    return _multi_local_search("grouped", points, tours, max_iterations, device, max_rounds, select_rounds)


def batched_multi_local_search_ragged(points_list, tours_list, max_iterations=1000, device="cuda:0", *, max_rounds=16,
                                      select_rounds=4):
    """``batched_multi_local_search_torch`` of G instances of ANY sizes at once, the arguments of ``batched_two_opt_ragged``.
    Returns ``(list of int64 numpy [P_g, n_g + 1], stats)``; ``stats``: as ``batched_multi_local_search_grouped``."""
    return _multi_local_search("ragged", points_list, tours_list, max_iterations, device, max_rounds, select_rounds)


def _nbr_local_search(form, points, tours, max_iterations, device, max_rounds, select_rounds, candidates, neighbors, closing):
    """``batched_nbr_local_search_<form>``: the checks and one ``difusco_tsp_nbr_local_search_ragged`` call."""
    pts, trs = _per_group(form, points, tours)
    device = _multi_move_checked(f"batched_nbr_local_search_{form}", pts, trs, max_iterations, max_rounds, select_rounds, device)
    lists, K = _nbr_lists(form, pts, neighbors, candidates, device)
    closing = int(bool(closing))
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    ws, nbytes = _workspace(L.difusco_tsp_nbr_local_search_ragged_workspace_bytes, *batch.sizes, K, closing, device=device)
    st = batch.group_stats()
    st["full_sweeps"] = np.zeros(batch.groups, dtype=np.int64)
    st["full_rounds"] = np.zeros(batch.groups, dtype=np.int32)
    _lib.check(L.difusco_tsp_nbr_local_search_ragged(*batch.head, _ptr(lists), K, closing, int(max_iterations), int(max_rounds),
                                                     int(select_rounds), _ptr(ws), nbytes, *(v.ctypes.data for v in st.values()),
                                                     _stream(device)))
    return _as_form(form, batch.read_tours(), st)


def batched_nbr_local_search_torch(points, tour, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4,
                                   candidates=8, neighbors=None, closing=True):
    """Neighbour-list multi-move 2-opt + Or-opt local search of the tours of ONE instance, the arguments of
    ``batched_multi_local_search_torch`` plus the lists of ``batched_nbr_two_opt_torch`` (``candidates`` / ``neighbors``): the
    rounds of ``batched_multi_local_search_torch``, but a sweep of either phase evaluates only the moves one of whose new edges -
    the head or tail edge of a 2-opt move, one of the two insertion edges of an Or-opt move - joins a city to one of its listed
    neighbours, O(N K) instead of all pairs.  A tour whose round applied no Or-opt move stops (``closing=False``) or goes on
    with the full rounds of ``batched_multi_local_search_torch`` until one applies no Or-opt move (``closing=True``: a tour
    that stops below the caps has no improving 2-opt or Or-opt move left).  The rule: ``difusco_tsp_nbr_local_search_ragged``,
    include/difusco_hip.h; GPU only.  The caps count over both stages.  Returns ``(tour int64 numpy [B, N+1], stats)``: the
    five counters of ``batched_multi_local_search_torch`` and ``full_sweeps``, ``full_rounds`` (the maxima over the tours of the
    sweeps in which a tour moved in, and the rounds it ran in, the full stage), ints."""
    return _nbr_local_search("torch", points, tour, max_iterations, device, max_rounds, select_rounds, candidates, neighbors, closing)


def batched_nbr_local_search_grouped(points, tours, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4,
                                     candidates=8, neighbors=None, closing=True):
    """``batched_nbr_local_search_torch`` of G instances at once, the arguments of ``batched_multi_local_search_grouped``;
    ``neighbors``: int [G, N, K] or None.  Every instance gets what its own ``batched_nbr_local_search_torch`` call returns.
    Returns ``(tours int64 numpy [G * P, N + 1], stats)``; the entries of ``stats`` are numpy arrays [G]."""
    return _nbr_local_search("grouped", points, tours, max_iterations, device, max_rounds, select_rounds, candidates, neighbors,
                             closing)


def batched_nbr_local_search_ragged(points_list, tours_list, max_iterations=1000, device="cuda:0", *, max_rounds=16,
                                    select_rounds=4, candidates=8, neighbors=None, closing=True):
    """``batched_nbr_local_search_torch`` of G instances of ANY sizes at once, the arguments of
    ``batched_multi_local_search_ragged``; ``neighbors``: a list of int [n_g, K] with one K, or None.  Returns ``(list of int64
    numpy [P_g, n_g + 1], stats)``; ``stats``: as ``batched_nbr_local_search_grouped``."""
    return _nbr_local_search("ragged", points_list, tours_list, max_iterations, device, max_rounds, select_rounds, candidates,
                             neighbors, closing)


TSP_KICK_SIZE, TSP_KICK_SPAN = 16, 30     # the pair of scripts/tsp_iterated_search_table.py


def check_tsp_kicks(local_search, kicks, kick_size=TSP_KICK_SIZE, span=TSP_KICK_SPAN):
    """``kicks`` / ``kick_size`` / ``span`` of ``solve_tsp`` and the runner: kicks iterate the multi-move local search, so they
    need it."""
    if int(kicks) != kicks or kicks < 0:
        raise ValueError(f"local_search_kicks = {kicks!r}: an integer >= 0")
    if int(kick_size) != kick_size or not 1 <= kick_size <= 64:
        raise ValueError(f"local_search_kick_size = {kick_size!r}: an integer in 1 .. 64")
    if int(span) != span or not 1 <= span < 2 ** 31:
        raise ValueError(f"local_search_kick_span = {span!r}: an integer >= 1")
    if kicks > 0 and local_search != "multi2opt+oropt":
        raise ValueError(f"local_search_kicks = {kicks} iterates the multi-move local search: it needs "
                         f"local_search='multi2opt+oropt', not {local_search!r}")
    return int(kicks), int(kick_size), int(span)


TSP_KICK_STATS = ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length")


TSP_DESCENTS = ("full", "focused")
TSP_COMPACT_SELECT_MAX = 1024             # proposals the focused search selects one per thread (difusco_tsp_focused_search_ragged)


def check_tsp_descent(descent, kicks=None):
    """``descent`` of the iterated search; for ``solve_tsp`` and the runner (``kicks`` given) the focused descents follow
    kicks, so they need some."""
    if descent not in TSP_DESCENTS:
        raise ValueError(f"local_search_descent = {descent!r}: one of {TSP_DESCENTS}")
    if kicks is not None and descent == "focused" and not kicks > 0:
        raise ValueError("local_search_descent = 'focused' restricts the descents after the kicks of the multi-move local "
                         "search: it needs local_search_kicks > 0")
    return descent


TSP_KICK_BIASES = ("uniform", "heat")


def check_tsp_kick_bias(kick_bias, kicks=None):
    """``kick_bias`` of the iterated search; for ``solve_tsp`` and the runner (``kicks`` given) the bias is one of the kicks, so
    it needs some."""
    if kick_bias not in TSP_KICK_BIASES:
        raise ValueError(f"local_search_kick_bias = {kick_bias!r}: one of {TSP_KICK_BIASES}")
    if kicks is not None and kick_bias == "heat" and not kicks > 0:
        raise ValueError("local_search_kick_bias = 'heat' draws the kicks of the multi-move local search from the heatmap: it "
                         "needs local_search_kicks > 0")
    return kick_bias


def _heat_graph(who, pts, trs, heat, edge_index, device):
    """The candidate graphs and heat of a guided call, on the device: per group ``heat[g]`` ([P_g, E_g] with ``edge_index[g]``
    [2, E_g]; [P_g, n_g, n_g] with ``edge_index=None``: the complete graph, entry (i, j) at i n + j as ``merge_tours`` lists it),
    numpy arrays or tensors (a device tensor never visits the host).  Edges that are not sorted by row are sorted (stable), the
    heat alike.  Returns (group_edges int32 numpy [G], row_ptr int32, col int32, heat float32 device tensors).  Every shape is
    checked here, before any library call."""
    G = len(pts)
    heat = list(heat)
    if len(heat) != G:
        raise ValueError(f"{who}: {len(heat)} heat arrays for {G} groups")
    dense = edge_index is None
    if not dense:
        edge_index = list(edge_index)
        if len(edge_index) != G or any(e is None for e in edge_index):
            raise ValueError(f"{who}: sparse heat needs one edge_index [2, E] per group ({G}); dense heat takes edge_index=None")
    rps, cols, hs, ne = [], [], [], []
    for g in range(G):
        n, P = pts[g].shape[0], trs[g].shape[0]
        h = _dev(heat[g], torch.float32, device)
        if dense:
            if h.numel() != P * n * n:
                raise ValueError(f"{who}: heat[{g}] holds {h.numel()} values, a dense heatmap of {P} tours has [{P}, {n}, {n}]")
            if n * n >= 2 ** 31:
                raise ValueError(f"{who}: a dense heatmap of n = {n} has more than 2^31 - 1 edges")
            idx = torch.arange(n, dtype=torch.int32, device=device)
            rp, cl, E = torch.arange(0, n * n + 1, n, dtype=torch.int32, device=device), idx.repeat(n), n * n
        else:
            ei = _dev(edge_index[g], torch.int64, device)
            if ei.ndim != 2 or ei.shape[0] != 2:
                raise ValueError(f"{who}: edge_index[{g}] must be [2, E], got {list(ei.shape)}")
            E = int(ei.shape[1])
            if h.numel() != P * E:
                raise ValueError(f"{who}: heat[{g}] holds {h.numel()} values for {P} tours of {E} edges")
            if E >= 2 ** 31:
                raise ValueError(f"{who}: edge_index[{g}] has more than 2^31 - 1 edges")
            row, cl = ei[0], ei[1]
            h = h.reshape(P, E)
            if E > 0:
                if int(row.min()) < 0 or int(row.max()) >= n or int(cl.min()) < 0 or int(cl.max()) >= n:
                    raise ValueError(f"{who}: edge_index[{g}] names a city outside 0 .. {n - 1}")
                if not bool((row[1:] >= row[:-1]).all()):
                    order = torch.sort(row, stable=True).indices
                    row, cl, h = row[order], cl[order], h[:, order]
            counts = torch.bincount(row, minlength=n)
            rp = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), torch.cumsum(counts, 0)]).to(torch.int32)
            cl = cl.to(torch.int32)
        rps.append(rp)
        cols.append(cl)
        hs.append(h.reshape(-1))
        ne.append(E)
    pad = lambda t, dt: t if t.numel() else torch.zeros(1, dtype=dt, device=device)      # never a null pointer
    return (np.array(ne, dtype=np.int32), torch.cat(rps).contiguous(), pad(torch.cat(cols).contiguous(), torch.int32),
            pad(torch.cat(hs).contiguous(), torch.float32))


TSP_CANDIDATE_SOURCES = ("knn", "heat")
TSP_HEAT_CANDIDATES_MAX = 128             # K of difusco_tsp_heat_candidates_ragged


def check_tsp_candidate_source(source, candidates):
    """``local_search_candidate_source`` of ``solve_tsp``, ``solve_tsp_batch`` and the runner: "knn" (default; the lists of
    ``check_tsp_candidates`` as they are) or "heat" (``tsp_heat_candidate_lists`` on the round's heatmaps), which is a source of
    neighbour lists and so needs ``local_search_candidates`` = K >= 1 (at most 128)."""
    if source not in TSP_CANDIDATE_SOURCES:
        raise ValueError(f"local_search_candidate_source = {source!r}: one of {TSP_CANDIDATE_SOURCES}")
    if source == "heat" and not 1 <= candidates <= TSP_HEAT_CANDIDATES_MAX:
        raise ValueError("local_search_candidate_source = 'heat' draws the neighbour lists from the heatmaps: it needs "
                         f"local_search_candidates = K in 1 .. {TSP_HEAT_CANDIDATES_MAX}, not {candidates!r}")
    return source


class _Samples:
    """What ``_heat_graph`` reads of a group's tours: how many there are."""

    def __init__(self, count):
        self.shape = (int(count),)


def tsp_heat_candidate_lists(points, heat, edge_index=None, candidates=8, *, device="cuda:0", stats=None):
    """Neighbour lists for ``batched_nbr_two_opt_*`` / ``batched_nbr_local_search_*`` (``neighbors=``) ranked by HEAT instead of
    distance (the rule: ``difusco_tsp_heat_candidates_ragged``, include/difusco_hip.h; GPU only).  One instance: ``points``
    [N, 2], ``heat`` [P, E] with ``edge_index`` [2, E], or ``heat`` [P, N, N] with ``edge_index=None`` (the complete graph) - the
    P heatmaps of the instance's samples on its directed candidate graph, as ``batched_iterated_search_torch`` with
    ``kick_bias="heat"`` takes them.  City a lists the cities its row names or whose row names it, first by the quantised heat
    of both orientations summed over the P samples (descending), then by squared distance, then by index; the first
    ``candidates`` = K (1 .. 128) are kept and a city with fewer gets -1 pads at the end.  Sequences of instances (lists of
    ``points``, ``heat`` and - unless all are dense - ``edge_index``) run as one library call; an instance gets the lists of its
    own call.  Returns one int32 device tensor [N, K] (a list of them for sequences); ``stats`` (a dict) receives ``listed`` -
    the list entries with a score above 0 - and ``pads``, ints (int64 arrays [G] for sequences).  Every shape and value is checked
    before any library call."""
    who = "tsp_heat_candidate_lists"
    single = isinstance(points, (np.ndarray, torch.Tensor))
    if single:
        points, heat, edge_index = [points], [heat], None if edge_index is None else [edge_index]
    if isinstance(candidates, bool) or not isinstance(candidates, (int, np.integer)) or not 1 <= candidates <= TSP_HEAT_CANDIDATES_MAX:
        raise ValueError(f"candidates = {candidates!r}: an integer in 1 .. {TSP_HEAT_CANDIDATES_MAX}")
    K = int(candidates)
    pts = [np.ascontiguousarray(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p, dtype=np.float64) for p in points]
    heat = list(heat)
    G = len(pts)
    if G < 1:
        raise ValueError(f"{who}: needs at least one instance")
    if len(heat) != G or (edge_index is not None and len(edge_index) != G):
        raise ValueError(f"{who}: {G} point arrays, {len(heat)} heat arrays" +
                         ("" if edge_index is None else f", {len(edge_index)} edge_index arrays"))
    samples = []
    for g in range(G):
        if pts[g].ndim != 2 or pts[g].shape[1] != 2 or pts[g].shape[0] < 1:
            raise ValueError(f"{who}: points[{g}] must be [N, 2] with N >= 1, got {list(pts[g].shape)}")
        shape = lambda x: tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))
        n, hs = pts[g].shape[0], shape(heat[g])
        if edge_index is None:
            if len(hs) != 3 or hs[0] < 1 or hs[1:] != (n, n):
                raise ValueError(f"{who}: heat[{g}] must be a dense [P, {n}, {n}] without edge_index, got {list(hs)}")
        else:
            es = shape(edge_index[g]) if edge_index[g] is not None else None
            if es is None or len(es) != 2 or es[0] != 2:
                raise ValueError(f"{who}: edge_index[{g}] must be [2, E], got {es and list(es)}")
            if len(hs) != 2 or hs[0] < 1 or hs[1] != es[1]:
                raise ValueError(f"{who}: heat[{g}] must be [P, {es[1]}] for the {es[1]} edges of edge_index[{g}], got {list(hs)}")
        samples.append(_Samples(hs[0]))
    device = _gpu_only(who, device)
    group_edges, row_ptr, col, d_heat = _heat_graph(who, pts, samples, heat, edge_index, device)
    group_n = np.array([p.shape[0] for p in pts], dtype=np.int32)
    group_tours = np.array([s.shape[0] for s in samples], dtype=np.int32)
    d_pts = _dev(np.concatenate([p.reshape(-1) for p in pts]), torch.float64, device)
    out = torch.empty(int(group_n.sum()) * K, dtype=torch.int32, device=device)
    L = _lib.lib()
    sizes = (G, group_n.ctypes.data, group_tours.ctypes.data, group_edges.ctypes.data)
    ws, nbytes = _workspace(L.difusco_tsp_heat_candidates_ragged_workspace_bytes, *sizes, K, device=device)
    listed, pads = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    _lib.check(L.difusco_tsp_heat_candidates_ragged(*sizes, _ptr(d_pts), _ptr(row_ptr), _ptr(col), _ptr(d_heat), K, _ptr(out),
                                                    _ptr(ws), nbytes, listed.ctypes.data, pads.ctypes.data, _stream(device)))
    per = [t.reshape(int(n), K) for t, n in zip(torch.split(out, [int(n) * K for n in group_n]), group_n)]
    if stats is not None:
        stats.update(listed=int(listed[0]), pads=int(pads[0])) if single else stats.update(listed=listed, pads=pads)
    return per[0] if single else per


def _iterated_search(form, points, tours, max_iterations, device, max_rounds, select_rounds, kicks, kick_size, span, seeds, offsets,
                     stats, descent, compact_select_max, kick_bias, heat, edge_index):
    """``batched_iterated_search_<form>``: the checks (before any library call) and one ``difusco_tsp_iterated_search_ragged``
    call - ``descent="focused"``: one ``difusco_tsp_focused_search_ragged`` call; ``kick_bias="heat"``: one
    ``difusco_tsp_guided_search_ragged`` call, either descent.  ``stats`` receives the per-tour arrays and ``host_syncs``."""
    who = f"batched_iterated_search_{form}"
    pts, trs = _per_group(form, points, tours)
    if form == "torch":                             # one instance: its heat and graph are the one entry of the per-group lists
        heat, edge_index = None if heat is None else [heat], None if edge_index is None else [edge_index]
    if int(kicks) != kicks or kicks < 0 or kicks >= 2 ** 31:
        raise ValueError(f"kicks = {kicks!r}: an integer >= 0")
    focused = check_tsp_descent(descent) == "focused"
    guided = check_tsp_kick_bias(kick_bias) == "heat"
    if guided and heat is None:
        raise ValueError(f"{who}: kick_bias='heat' needs heat= (and edge_index= unless the heat is dense)")
    if not guided and (heat is not None or edge_index is not None):
        raise ValueError(f"{who}: heat= / edge_index= are read only with kick_bias='heat'")
    if int(compact_select_max) != compact_select_max or not 0 <= compact_select_max <= TSP_COMPACT_SELECT_MAX:
        raise ValueError(f"compact_select_max = {compact_select_max!r}: an integer in 0 .. {TSP_COMPACT_SELECT_MAX}")
    _, kick_size, span = check_tsp_kicks("multi2opt+oropt", 0, kick_size, span)
    device = _multi_move_checked(who, pts, trs, max_iterations, max_rounds, select_rounds, device)
    graph = _heat_graph(who, pts, trs, heat, edge_index, device) if guided else None
    T = sum(t.shape[0] for t in trs)
    table = _philox_table(seeds, offsets, T, "tours", device)
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    if guided:
        ws, nbytes = _workspace(L.difusco_tsp_guided_search_ragged_workspace_bytes, *batch.sizes, graph[0].ctypes.data, device=device)
    else:
        ws, nbytes = _workspace(L.difusco_tsp_focused_search_ragged_workspace_bytes if focused
                                else L.difusco_tsp_iterated_search_ragged_workspace_bytes, *batch.sizes, device=device)
    out = batch.group_stats()
    per = {"kicks_kept": np.zeros(T, dtype=np.int32), "kicks_improved": np.zeros(T, dtype=np.int32),
           "segments_swapped": np.zeros(T, dtype=np.int64), "first_length": np.zeros(T, dtype=np.float64),
           "final_length": np.zeros(T, dtype=np.float64)}
    head = (*batch.head, int(max_iterations), int(max_rounds), int(select_rounds), int(kicks), kick_size, span, _ptr(table[0]),
            _ptr(table[1]))
    tail = (_ptr(ws), nbytes, *(v.ctypes.data for v in out.values()), *(per[k].ctypes.data for k in TSP_KICK_STATS))
    if focused:
        per["closing_sweeps"] = np.zeros(T, dtype=np.int32)
    if guided:
        group_edges, row_ptr, col, d_heat = graph
        _lib.check(L.difusco_tsp_guided_search_ragged(
            *head, int(compact_select_max), int(focused), group_edges.ctypes.data, _ptr(row_ptr), _ptr(col), _ptr(d_heat), *tail,
            per["closing_sweeps"].ctypes.data if focused else None, _stream(device)))
    elif focused:
        _lib.check(L.difusco_tsp_focused_search_ragged(*head, int(compact_select_max), *tail, per["closing_sweeps"].ctypes.data,
                                                       _stream(device)))
    else:
        _lib.check(L.difusco_tsp_iterated_search_ragged(*head, *tail, _stream(device)))
    if stats is not None:
        stats.update(per, host_syncs=int(L.difusco_tsp_search_host_syncs()))
    return _as_form(form, batch.read_tours(), out)


def batched_iterated_search_torch(points, tour, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4, kicks=0,
                                  kick_size=TSP_KICK_SIZE, span=TSP_KICK_SPAN, seeds=None, offsets=None, stats=None,
                                  descent="full", compact_select_max=TSP_COMPACT_SELECT_MAX, kick_bias="uniform", heat=None,
                                  edge_index=None):
    """``batched_multi_local_search_torch`` iterated with seeded segment kicks (the rule: ``difusco_tsp_iterated_search_ragged``,
    include/difusco_hip.h; GPU only; not in the reference): after its descent every tour, ``kicks`` times, swaps up to
    ``kick_size`` disjoint pairs of adjacent random segments of at most ``span`` cities each, descends again (the caps are per
    descent) and keeps the result unless it is longer.  ``seeds`` / ``offsets`` [B]: the Philox key and first offset of every
    tour (default 0; kick t draws at ``offsets[b] + t``); a tour gets the same answer alone or in any call.  ``kicks=0`` is
    ``batched_multi_local_search_torch``.  Returns ``(tour int64 numpy [B, N+1], stats)`` as that function (sweeps and moves
    summed over a tour's descents, ``rounds`` the most rounds of a descent); ``stats`` (a dict) receives the per-tour numpy
    arrays [B] ``kicks_kept``, ``kicks_improved``, ``segments_swapped``, ``first_length``, ``final_length`` and ``host_syncs``.
    ``descent="focused"`` (the rule: ``difusco_tsp_focused_search_ragged``): a descent after a kick evaluates only the candidates
    next to an edge that the kick or a move since has touched, and one full descent closes the call; ``stats`` gains
    ``closing_sweeps`` [B], the sweeps in which that descent still moved (0: the focused descents missed nothing).
    ``compact_select_max`` (0 .. 1024) changes the cost of a focused sweep's selection alone, never its result.
    ``kick_bias``: ``"uniform"`` (default: the cuts of a kick fall anywhere alike) or ``"heat"`` (the rule:
    ``difusco_tsp_guided_search_ragged``): the first cut of every draw falls on a tour edge with a probability that rises as the
    heat of that edge falls, either descent.  It reads ``heat`` and ``edge_index`` in the shapes ``merge_tours`` takes - sparse:
    ``heat`` [B, E] (or [B * E]), one row per tour, in the edge order of ``edge_index`` [2, E]; dense: ``heat`` [B, N, N] with
    ``edge_index=None`` -, numpy arrays or device tensors; edges not sorted by their first row are sorted (stable).  An edge
    absent from the graph counts as heat 0.  ``ValueError`` before any library call: ``"heat"`` without ``heat``, shapes that do
    not match, ``heat`` with ``"uniform"``, an unknown ``kick_bias``.  Constant heat does not reproduce ``"uniform"``."""
    return _iterated_search("torch", points, tour, max_iterations, device, max_rounds, select_rounds, kicks, kick_size, span, seeds,
                            offsets, stats, descent, compact_select_max, kick_bias, heat, edge_index)


def batched_iterated_search_grouped(points, tours, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4,
                                    kicks=0, kick_size=TSP_KICK_SIZE, span=TSP_KICK_SPAN, seeds=None, offsets=None, stats=None,
                                    descent="full", compact_select_max=TSP_COMPACT_SELECT_MAX, kick_bias="uniform", heat=None,
                                    edge_index=None):
    """``batched_iterated_search_torch`` of G instances at once, the arguments of ``batched_multi_local_search_grouped``;
    ``seeds`` / ``offsets`` [G * P] in the order of ``tours``.  Every tour gets what its own call returns.  Returns ``(tours int64
    numpy [G * P, N + 1], stats)``; the entries of the returned stats are numpy arrays [G], the per-tour arrays [G * P].
    ``kick_bias="heat"``: ``heat`` and ``edge_index`` are lists with one entry per instance, as ``merge_tours_batch`` takes them
    (``heat[g]`` [P, E_g] with ``edge_index[g]`` [2, E_g]; [P, N, N] with ``edge_index=None``)."""
    return _iterated_search("grouped", points, tours, max_iterations, device, max_rounds, select_rounds, kicks, kick_size, span, seeds,
                            offsets, stats, descent, compact_select_max, kick_bias, heat, edge_index)


def batched_iterated_search_ragged(points_list, tours_list, max_iterations=1000, device="cuda:0", *, max_rounds=16,
                                   select_rounds=4, kicks=0, kick_size=TSP_KICK_SIZE, span=TSP_KICK_SPAN, seeds=None,
                                   offsets=None, stats=None, descent="full", compact_select_max=TSP_COMPACT_SELECT_MAX,
                                   kick_bias="uniform", heat=None, edge_index=None):
    """``batched_iterated_search_torch`` of G instances of ANY sizes at once, the arguments of
    ``batched_multi_local_search_ragged``; ``seeds`` / ``offsets``: one per tour, group after group.  Returns ``(list of int64
    numpy [P_g, n_g + 1], stats)``; ``stats``: as ``batched_iterated_search_grouped``.  ``kick_bias``, ``heat``, ``edge_index``:
    as there."""
    return _iterated_search("ragged", points_list, tours_list, max_iterations, device, max_rounds, select_rounds, kicks, kick_size, span,
                            seeds, offsets, stats, descent, compact_select_max, kick_bias, heat, edge_index)


TSP_KOPT_MAX_SAMPLES, TSP_KOPT_MAX_DEPTH = 4096, 10       # difusco_tsp_kopt_search_ragged
TSP_KOPT_SAMPLES, TSP_KOPT_DEPTH, TSP_KOPT_ROUNDS, TSP_KOPT_PATIENCE, TSP_KOPT_ALPHA, TSP_KOPT_BETA = 1024, 10, 64, 10, 1.0, 10.0
TSP_KOPT_STATS = ("rounds", "actions", "depth_sum", "reverted", "first_length", "final_length")


def check_tsp_kopt(rounds, samples=TSP_KOPT_SAMPLES, depth=TSP_KOPT_DEPTH):
    """``rounds`` / ``samples`` / ``depth`` of the sampled k-opt search (``rounds = 0``: the stage is off)."""
    if int(rounds) != rounds or not 0 <= rounds < 2 ** 31:
        raise ValueError(f"kopt rounds = {rounds!r}: an integer >= 0")
    if int(samples) != samples or not 1 <= samples <= TSP_KOPT_MAX_SAMPLES:
        raise ValueError(f"kopt samples = {samples!r}: an integer in 1 .. {TSP_KOPT_MAX_SAMPLES}")
    if int(depth) != depth or not 1 <= depth <= TSP_KOPT_MAX_DEPTH:
        raise ValueError(f"kopt depth = {depth!r}: an integer in 1 .. {TSP_KOPT_MAX_DEPTH}")
    return int(rounds), int(samples), int(depth)


def kopt_explore(alpha, samples, rounds):
    """The ``explore`` table of ``difusco_tsp_kopt_search_ragged``: ``alpha * sqrt(log1p(r * samples))``, float64 [rounds]."""
    return alpha * np.sqrt(np.log1p(np.arange(rounds, dtype=np.float64) * float(samples)))


def _kopt_search(form, points, tours, heat, edge_index, samples, depth, rounds, patience, alpha, beta, seeds, offsets, stats, device):
    """``batched_kopt_search_<form>``: the checks (before any library call) and one ``difusco_tsp_kopt_search_ragged`` call."""
    who = f"batched_kopt_search_{form}"
    pts, trs = _per_group(form, points, tours)
    if form == "torch":
        heat, edge_index = None if heat is None else [heat], None if edge_index is None else [edge_index]
    if heat is None:
        raise ValueError(f"{who}: needs heat= (and edge_index= unless the heat is dense)")
    rounds, samples, depth = check_tsp_kopt(rounds, samples, depth)
    if int(patience) != patience or not 1 <= patience < 2 ** 31:
        raise ValueError(f"patience = {patience!r}: an integer >= 1")
    if not (np.isfinite(alpha) and alpha >= 0) or not (np.isfinite(beta) and beta >= 0):
        raise ValueError(f"alpha = {alpha!r}, beta = {beta!r}: finite values >= 0")
    device = _local_search_checked(who, pts, trs, 0, 1, device)
    ex = np.ascontiguousarray(kopt_explore(alpha, samples, rounds), dtype=np.float64)
    graph = _heat_graph(who, pts, trs, heat, edge_index, device)
    T = sum(t.shape[0] for t in trs)
    table = _philox_table(seeds, offsets, T, "tours", device)
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    group_edges, row_ptr, col, d_heat = graph
    ws, nbytes = _workspace(L.difusco_tsp_kopt_search_ragged_workspace_bytes, *batch.sizes, group_edges.ctypes.data, samples, depth,
                            device=device)
    per = {"rounds": np.zeros(T, dtype=np.int32), "actions": np.zeros(T, dtype=np.int32), "depth_sum": np.zeros(T, dtype=np.int64),
           "reverted": np.zeros(T, dtype=np.int32), "first_length": np.zeros(T, dtype=np.float64),
           "final_length": np.zeros(T, dtype=np.float64)}
    _lib.check(L.difusco_tsp_kopt_search_ragged(
        *batch.head, group_edges.ctypes.data, _ptr(row_ptr), _ptr(col), _ptr(d_heat), _ptr(table[0]), _ptr(table[1]), samples, depth,
        rounds, int(patience), float(beta), ex.ctypes.data if rounds else None, _ptr(ws), nbytes,
        *(per[k].ctypes.data for k in TSP_KOPT_STATS), _stream(device)))
    if stats is not None:
        stats.update(per, host_syncs=int(L.difusco_tsp_search_host_syncs()))
    out = batch.read_tours()
    return out[0] if form == "torch" else np.concatenate(out, axis=0) if form == "grouped" else out


def batched_kopt_search_torch(points, tours, *, heat, edge_index=None, samples=TSP_KOPT_SAMPLES, depth=TSP_KOPT_DEPTH,
                              rounds=TSP_KOPT_ROUNDS, patience=TSP_KOPT_PATIENCE, alpha=TSP_KOPT_ALPHA, beta=TSP_KOPT_BETA,
                              seeds=None, offsets=None, stats=None, device="cuda:0"):
    """Heatmap-guided sampled k-opt search of B tours of one instance (the rule: ``difusco_tsp_kopt_search_ragged``,
    include/difusco_hip.h; GPU only; a parallel restatement of the reference's heatmap + MCTS stage, not a port).  Per round
    every tour runs ``samples`` simulations: each opens the tour at a drawn position and, up to ``depth`` times, draws a new edge
    among the candidate entries of the open end whose learned weight (100 x heat at first) plus an exploration term
    (``alpha * sqrt(log1p(r * samples))`` over the entry's use count) stands out of its row, and closes it with a prefix
    reversal - a sequential k-opt move, k up to ``depth + 1``.  The best closing gain of the round is applied when it is above
    1e-6 and raises the weights of its new edges by ``beta * (x + x^2 / 2)``, x the relative gain.  A tour stops after ``rounds``
    rounds or ``patience * N`` simulations in a row without an applied action.  Run the local search first: the search has no
    2-opt stage of its own.  ``heat`` / ``edge_index``: as ``batched_iterated_search_torch`` with ``kick_bias="heat"`` takes
    them; ``seeds`` / ``offsets`` [B]: the Philox key and first offset of every tour (round r draws at ``offsets[b] + r``); a
    tour gets the same answer alone or in any call.  Returns the tours, int64 numpy [B, N + 1], none longer than its input;
    ``stats`` (a dict) receives the per-tour numpy arrays [B] ``rounds``, ``actions``, ``depth_sum``, ``reverted``,
    ``first_length``, ``final_length`` and ``host_syncs``.  ``rounds=0`` returns the input."""
    return _kopt_search("torch", points, tours, heat, edge_index, samples, depth, rounds, patience, alpha, beta, seeds, offsets, stats,
                        device)


def batched_kopt_search_grouped(points, tours, *, heat, edge_index=None, samples=TSP_KOPT_SAMPLES, depth=TSP_KOPT_DEPTH,
                                rounds=TSP_KOPT_ROUNDS, patience=TSP_KOPT_PATIENCE, alpha=TSP_KOPT_ALPHA, beta=TSP_KOPT_BETA,
                                seeds=None, offsets=None, stats=None, device="cuda:0"):
    """``batched_kopt_search_torch`` of G instances at once: ``points`` [G, N, 2], ``tours`` [G * P, N + 1]; ``heat`` and
    ``edge_index`` are lists with one entry per instance (``heat[g]`` [P, E_g] with ``edge_index[g]`` [2, E_g]; [P, N, N] with
    ``edge_index=None``); ``seeds`` / ``offsets`` [G * P].  Every tour gets what its own call returns."""
    return _kopt_search("grouped", points, tours, heat, edge_index, samples, depth, rounds, patience, alpha, beta, seeds, offsets,
                        stats, device)


def batched_kopt_search_ragged(points_list, tours_list, *, heat, edge_index=None, samples=TSP_KOPT_SAMPLES, depth=TSP_KOPT_DEPTH,
                               rounds=TSP_KOPT_ROUNDS, patience=TSP_KOPT_PATIENCE, alpha=TSP_KOPT_ALPHA, beta=TSP_KOPT_BETA,
                               seeds=None, offsets=None, stats=None, device="cuda:0"):
    """``batched_kopt_search_torch`` of G instances of ANY sizes at once: one point array [n_g, 2] and one tour array
    [P_g, n_g + 1] per instance, ``heat`` / ``edge_index`` as ``batched_kopt_search_grouped``; ``seeds`` / ``offsets``: one per
    tour, group after group.  Returns a list of int64 numpy [P_g, n_g + 1]."""
    return _kopt_search("ragged", points_list, tours_list, heat, edge_index, samples, depth, rounds, patience, alpha, beta, seeds,
                        offsets, stats, device)


TSP_WINDOW_MIN, TSP_WINDOW_MAX, TSP_WINDOW_MAX_KICKS = 16, 1024, 1024
# the recommended window mode: the lowest row of scripts/tsp_window_search_table.py
TSP_WINDOW, TSP_WINDOW_KICK_SIZE, TSP_WINDOW_KICK_SPAN = 128, 8, 30
TSP_WINDOW_STATS = ("kicks_kept", "kicks_improved", "segments_swapped", "first_length", "final_length", "passes_kept",
                    "windows_searched", "window_sweeps", "window_moves", "closing_sweeps")


def check_tsp_window(local_search, window, passes=1, kicks=0, descent="full", kick_bias="uniform"):
    """``window`` / ``passes`` of ``solve_tsp`` and the runner.  ``window = 0``: the mode is off (``passes`` must be 1 then).
    ``window > 0`` runs the windowed iterated search (``batched_window_search_torch``): it needs
    ``local_search='multi2opt+oropt'``, reads ``kicks`` as the kicks per window and pass, and combines with neither focused
    descents nor heat-biased kicks."""
    if int(window) != window or not (window == 0 or TSP_WINDOW_MIN <= window <= TSP_WINDOW_MAX):
        raise ValueError(f"local_search_window = {window!r}: 0 (off) or an integer in {TSP_WINDOW_MIN} .. {TSP_WINDOW_MAX}")
    if int(passes) != passes or passes < 1 or passes >= 2 ** 31:
        raise ValueError(f"local_search_passes = {passes!r}: an integer >= 1")
    if window == 0:
        if passes != 1:
            raise ValueError(f"local_search_passes = {passes} counts the passes of the windowed search: it needs local_search_window > 0")
        return 0, 1
    if local_search != "multi2opt+oropt":
        raise ValueError(f"local_search_window = {window} runs the multi-move local search on tour windows: it needs "
                         f"local_search='multi2opt+oropt', not {local_search!r}")
    if kicks > TSP_WINDOW_MAX_KICKS:
        raise ValueError(f"local_search_kicks = {kicks} with local_search_window > 0 is per window and pass: at most "
                         f"{TSP_WINDOW_MAX_KICKS}")
    if descent != "full":
        raise ValueError(f"local_search_window = {window} does not combine with local_search_descent = {descent!r}")
    if kick_bias != "uniform":
        raise ValueError(f"local_search_window = {window} does not combine with local_search_kick_bias = {kick_bias!r}")
    return int(window), int(passes)


def _window_search(form, points, tours, max_iterations, device, max_rounds, select_rounds, kicks, kick_size, span, seeds, offsets,
                   stats, window, passes):
    """``batched_window_search_<form>``: the checks (before any library call) and one ``difusco_tsp_window_search_ragged`` call.
    ``stats`` receives the per-tour arrays."""
    who = f"batched_window_search_{form}"
    pts, trs = _per_group(form, points, tours)
    if int(kicks) != kicks or not 0 <= kicks <= TSP_WINDOW_MAX_KICKS:
        raise ValueError(f"kicks = {kicks!r}: an integer in 0 .. {TSP_WINDOW_MAX_KICKS}")
    if int(window) != window or not TSP_WINDOW_MIN <= window <= TSP_WINDOW_MAX:
        raise ValueError(f"window = {window!r}: an integer in {TSP_WINDOW_MIN} .. {TSP_WINDOW_MAX}")
    if int(passes) != passes or passes < 1 or passes >= 2 ** 31:
        raise ValueError(f"passes = {passes!r}: an integer >= 1")
    _, kick_size, span = check_tsp_kicks("multi2opt+oropt", 0, kick_size, span)
    device = _multi_move_checked(who, pts, trs, max_iterations, max_rounds, select_rounds, device)
    for p in pts:
        if int(passes) * (-(-p.shape[0] // int(window)) + 1) * max(int(kicks), 1) >= 2 ** 32:
            raise ValueError(f"{who}: passes = {passes} with {-(-p.shape[0] // int(window)) + 1} windows and {kicks} kicks each "
                             "needs 2^32 or more Philox offsets per tour")
    T = sum(t.shape[0] for t in trs)
    table = _philox_table(seeds, offsets, T, "tours", device)
    batch = _RaggedBatch(pts, trs, device)
    L = _lib.lib()
    ws, nbytes = _workspace(L.difusco_tsp_window_search_ragged_workspace_bytes, *batch.sizes, int(window), device=device)
    out = batch.group_stats()
    i32s, f64s = ("kicks_kept", "kicks_improved", "passes_kept", "windows_searched", "closing_sweeps"), ("first_length", "final_length")
    per = {k: np.zeros(T, dtype=np.int32 if k in i32s else np.float64 if k in f64s else np.int64) for k in TSP_WINDOW_STATS}
    _lib.check(L.difusco_tsp_window_search_ragged(
        *batch.head, int(max_iterations), int(max_rounds), int(select_rounds), int(kicks), kick_size, span, _ptr(table[0]),
        _ptr(table[1]), int(window), int(passes), _ptr(ws), nbytes, *(v.ctypes.data for v in out.values()),
        *(per[k].ctypes.data for k in TSP_WINDOW_STATS), _stream(device)))
    if stats is not None:
        stats.update(per)
    return _as_form(form, batch.read_tours(), out)


def batched_window_search_torch(points, tour, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4, kicks=0,
                                kick_size=TSP_KICK_SIZE, span=TSP_KICK_SPAN, seeds=None, offsets=None, stats=None, window,
                                passes=1):
    """The iterated search of ``batched_iterated_search_torch`` on the WINDOWS of every tour, all windows of a pass at once (the
    rule: ``difusco_tsp_window_search_ragged``, include/difusco_hip.h; GPU only; not in the reference): after its descent every
    tour runs ``passes`` passes; a pass cuts the tour every ``window`` positions (16 .. 1024; odd passes shifted by half a
    window), runs ``kicks`` kicks (0 .. 1024, per window and pass) of the iterated search on every window as an open path whose
    ends stay, one GPU block per window with no host poll, and keeps the result unless the tour got longer; one full descent
    closes the call.  ``seeds`` / ``offsets`` [B]: as there; window w of pass r draws at ``offsets[b] + (r C + w) kicks``,
    ``C = ceil(N / window) + 1``.  A tour gets the same answer alone or in any call.  Returns ``(tour int64 numpy [B, N+1],
    stats)``, the stats of ``batched_multi_local_search_torch`` over the first and the closing descent; ``stats`` (a dict)
    receives the per-tour numpy arrays [B] ``first_length``, ``final_length``, ``passes_kept``, ``windows_searched``,
    ``kicks_kept``, ``kicks_improved``, ``segments_swapped``, ``window_sweeps``, ``window_moves`` and ``closing_sweeps``."""
    return _window_search("torch", points, tour, max_iterations, device, max_rounds, select_rounds, kicks, kick_size, span, seeds,
                          offsets, stats, window, passes)


def batched_window_search_grouped(points, tours, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4, kicks=0,
                                  kick_size=TSP_KICK_SIZE, span=TSP_KICK_SPAN, seeds=None, offsets=None, stats=None, window,
                                  passes=1):
    """``batched_window_search_torch`` of G instances at once, the arguments of ``batched_iterated_search_grouped``.  Every tour
    gets what its own call returns.  Returns ``(tours int64 numpy [G * P, N + 1], stats)``; the entries of the returned stats
    are numpy arrays [G], the per-tour arrays [G * P]."""
    return _window_search("grouped", points, tours, max_iterations, device, max_rounds, select_rounds, kicks, kick_size, span, seeds,
                          offsets, stats, window, passes)


def batched_window_search_ragged(points_list, tours_list, max_iterations=1000, device="cuda:0", *, max_rounds=16, select_rounds=4,
                                 kicks=0, kick_size=TSP_KICK_SIZE, span=TSP_KICK_SPAN, seeds=None, offsets=None, stats=None,
                                 window, passes=1):
    """``batched_window_search_torch`` of G instances of ANY sizes at once, the arguments of ``batched_iterated_search_ragged``.
    Returns ``(list of int64 numpy [P_g, n_g + 1], stats)``; ``stats``: as ``batched_window_search_grouped``."""
    return _window_search("ragged", points_list, tours_list, max_iterations, device, max_rounds, select_rounds, kicks, kick_size, span,
                          seeds, offsets, stats, window, passes)


def _numel(x):
    return x.numel() if isinstance(x, torch.Tensor) else x.size


def _mis_graph(predictions, adj_matrix, graph, edge_index, graph_build, device):
    """What the three MIS entries read, on the device: (float32 scores [N], the ``CsrGraph`` - built from ``edge_index`` or the
    scipy ``adj_matrix`` unless given -, its col array)."""
    from .graph import build_csr
    scores = _dev(predictions, torch.float32, device).reshape(-1)
    if graph is None:
        if edge_index is None:
            coo = adj_matrix.tocoo()
            edge_index = np.stack([coo.row, coo.col]).astype(np.int64)
        graph = build_csr(edge_index if isinstance(edge_index, torch.Tensor) else torch.from_numpy(np.asarray(edge_index)),
                          scores.shape[0], device, method=graph_build)
    # a graph without any entry has no col array to point at; the kernels read none (every row is empty)
    col = graph.col if graph.col.numel() else torch.zeros(1, dtype=torch.int32, device=device)
    return scores, graph, col


def _mis_solution(solution, n):
    """``solution`` of a search as an array or tensor of ``n`` entries: checked on the host, before any upload."""
    solution = solution if isinstance(solution, torch.Tensor) else np.asarray(solution)
    if _numel(solution) != n:
        raise ValueError(f"solution holds {_numel(solution)} entries for {n} scores")
    return solution


def _mis_solution_on_device(solution, device):
    """int32 [N] on the device and never the caller's tensor: the library refines in place."""
    sol = _dev(solution, torch.int32, device).reshape(-1)
    return sol.clone() if isinstance(solution, torch.Tensor) else sol


def _mis_counters(stats, counters):
    stats["rounds"], stats["swaps"], stats["inserts"] = int(counters[0]), int(counters[1]), int(counters[2])


def mis_decode_np(predictions, adj_matrix=None, *, graph=None, edge_index=None, device="cuda:0", graph_build="host", stats=None):
    """Drop-in for ``mis_decode_np`` of the reference (``difusco/utils/mis_utils.py:3-18``): ``predictions`` [N] node
    scores (numpy or tensor), ``adj_matrix`` a scipy sparse adjacency (as built at ``pl_mis_model.py:152-154``).
    Returns the 0/1 int numpy array.  Instead of a scipy matrix the caller may pass the ``CsrGraph`` of the denoise
    steps (``graph=``, no host round trip) or the ``edge_index`` the adjacency was built from (``graph_build``: the method of
    ``graph.build_csr`` for it).  The nodes are visited as by ``np.argsort(-scores, kind="stable")`` on the scores AFTER their
    cast to float32: decreasing score, -0.0 and +0.0 equal, NaN after everything else, equal scores by increasing node id - so
    float64 scores that collapse to one float32 value are a tie by id.  The adjacency must be symmetric (self loops and
    duplicate entries are allowed, a graph without any entry gives all ones).  ``stats`` (a dict) receives ``rounds``, the
    parallel rounds the decode ran.  GPU only."""
    device = torch.device(device)
    L = _lib.lib()
    scores, graph, col = _mis_graph(predictions, adj_matrix, graph, edge_index, graph_build, device)
    n = scores.shape[0]
    ws, nbytes = _workspace(L.difusco_mis_decode_workspace_bytes, n, device=device)
    sol = torch.empty(n, dtype=torch.int32, device=device)
    rounds = ctypes.c_int32()
    _lib.check(L.difusco_mis_decode(n, _ptr(graph.rowptr), _ptr(col), _ptr(scores), _ptr(sol), _ptr(ws), nbytes,
                                    ctypes.byref(rounds), _stream(device)))
    if stats is not None:
        stats["rounds"] = int(rounds.value)
    return sol.cpu().numpy().astype(int)


MIS_LOCAL_SEARCHES = ("none", "swap")


def check_mis_local_search(local_search):
    if local_search not in MIS_LOCAL_SEARCHES:
        raise ValueError(f"MIS local search {local_search!r}: one of {MIS_LOCAL_SEARCHES}")
    return local_search


def mis_local_search_np(predictions, solution, adj_matrix=None, *, graph=None, edge_index=None, device="cuda:0",
                        graph_build="host", max_rounds=1000, stats=None):
    """(1,2)-swap local search on a MIS solution (``difusco_mis_local_search``, include/difusco_hip.h; not in the reference):
    the arguments of ``mis_decode_np`` plus ``solution``, a 0/1 array [N] that is an independent set (e.g. what
    ``mis_decode_np`` returned; all zeros is allowed).  Rounds of "one chosen node out, two of its neighbours in", each followed
    by the greedy insertion of the nodes that became free, in the score order of the decode, until no such swap is left or
    ``max_rounds`` rounds ran; never a smaller set, always independent and maximal.  Returns the 0/1 int numpy array; ``stats``
    (a dict) receives ``rounds``, ``swaps`` and ``inserts``.  A set that is not independent raises ``DifuscoHipError``.  GPU only."""
    device = _gpu_only("mis_local_search_np", device)
    if int(max_rounds) != max_rounds or max_rounds < 0:
        raise ValueError(f"max_rounds = {max_rounds!r}: an integer >= 0")
    n = _numel(predictions)
    solution = _mis_solution(solution, n)
    L = _lib.lib()
    scores, graph, col = _mis_graph(predictions, adj_matrix, graph, edge_index, graph_build, device)
    sol = _mis_solution_on_device(solution, device)
    ws, nbytes = _workspace(L.difusco_mis_local_search_workspace_bytes, n, int(graph.col.shape[0]), device=device)
    counters = (ctypes.c_int32 * 3)()
    _lib.check(L.difusco_mis_local_search(n, _ptr(graph.rowptr), _ptr(col), _ptr(scores), _ptr(sol), int(max_rounds), _ptr(ws),
                                          nbytes, counters, _stream(device)))
    if stats is not None:
        _mis_counters(stats, counters)
    return sol.cpu().numpy().astype(int)


MIS_KICK_OFFSET = 1 << 62        # first Philox offset of the kick streams: far above the step counters the sampling draws at


def check_mis_kicks(local_search, kicks, kick_size):
    """``kicks`` / ``kick_size`` of ``solve_mis`` and the runner: kicks iterate the swap search, so they need it."""
    if int(kicks) != kicks or kicks < 0:
        raise ValueError(f"local_search_kicks = {kicks!r}: an integer >= 0")
    if int(kick_size) != kick_size or kick_size < 1:
        raise ValueError(f"local_search_kick_size = {kick_size!r}: an integer >= 1")
    if kicks > 0 and local_search != "swap":
        raise ValueError(f"local_search_kicks = {kicks} iterates the swap search: it needs local_search='swap', not {local_search!r}")
    return int(kicks), int(kick_size)


MIS_SEARCH_MODES = ("launches", "resident")


def check_mis_search_mode(local_search, mode):
    """``local_search_mode`` of ``solve_mis`` and the runner: ``"resident"`` runs the swap search, with any ``kicks >= 0``, one GPU
    block per instance, so it needs that search."""
    if mode not in MIS_SEARCH_MODES:
        raise ValueError(f"MIS local search mode {mode!r}: one of {MIS_SEARCH_MODES}")
    if mode == "resident" and local_search != "swap":
        raise ValueError(f"local_search_mode='resident' runs the swap search: it needs local_search='swap', not {local_search!r}")
    return mode


def mis_iterated_search_np(predictions, solution, adj_matrix=None, *, graph=None, edge_index=None, instance_rows=None, seeds=None,
                           offsets=None, kicks, kick_size=4, max_rounds=1000, device="cuda:0", graph_build="host", stats=None,
                           mode="launches", kicks_per_launch=0):
    """The swap search of ``mis_local_search_np`` iterated with seeded random kicks (``difusco_mis_iterated_search``,
    include/difusco_hip.h; not in the reference): after the descent, ``kicks`` times: about ``kick_size`` random nodes of every
    instance are forced in, their neighbours leave, the descent runs again and every instance keeps the result unless it is
    smaller.  ``instance_rows`` [B + 1]: the node offsets of the instances of the call (default: one instance); no edge may
    join two instances.  ``seeds`` / ``offsets`` [B]: the Philox key and first offset of every instance (default 0; kick t
    draws at ``offsets[b] + t``); an instance gets the same answer alone or in any union.  ``kicks=0`` is
    ``mis_local_search_np``.  Returns the 0/1 int numpy array; ``stats`` (a dict) receives ``rounds``, ``swaps``, ``inserts``
    (all descents), ``host_syncs`` and the per-instance lists ``entered``, ``accepted``, ``size_before``, ``size_after``.
    A set that is not independent or a malformed table raises ``DifuscoHipError``.  ``mode``: ``"launches"`` (the default) runs
    every kick as a sequence of launches over the whole call; ``"resident"`` (``difusco_mis_resident_search``) runs one GPU block
    per instance with its state in LDS and synchronises with the host once per call: the same set, counters and ``stats`` keys
    bit for bit, for instances of at most ``difusco_mis_resident_max_nodes()`` nodes (a larger one raises ``DifuscoHipError``);
    ``kicks_per_launch`` bounds the kicks of one of its launches (0: the library's default).  GPU only."""
    device = _gpu_only("mis_iterated_search_np", device)
    if int(max_rounds) != max_rounds or max_rounds < 0:
        raise ValueError(f"max_rounds = {max_rounds!r}: an integer >= 0")
    kicks, kick_size = check_mis_kicks("swap", kicks, kick_size)
    check_mis_search_mode("swap", mode)
    if int(kicks_per_launch) != kicks_per_launch or kicks_per_launch < 0:
        raise ValueError(f"kicks_per_launch = {kicks_per_launch!r}: an integer >= 0")
    n = _numel(predictions)
    solution = _mis_solution(solution, n)
    rows = np.array([0, n], dtype=np.int64) if instance_rows is None else np.asarray(instance_rows, dtype=np.int64).reshape(-1)
    B = len(rows) - 1
    if B < 1:
        raise ValueError("instance_rows must hold n_instances + 1 >= 2 offsets")
    table = _philox_table(seeds, offsets, B, "instances", device)
    L = _lib.lib()
    scores, graph, col = _mis_graph(predictions, adj_matrix, graph, edge_index, graph_build, device)
    sol = _mis_solution_on_device(solution, device)
    d_rows = torch.from_numpy(rows).to(device)
    counters = (ctypes.c_int32 * 3)()
    per = (ctypes.c_int32 * (4 * B))()
    if mode == "resident":
        ws, nbytes = _workspace(L.difusco_mis_resident_search_workspace_bytes, n, int(graph.col.shape[0]), B, kicks, device=device)
        _lib.check(L.difusco_mis_resident_search(n, _ptr(graph.rowptr), _ptr(col), _ptr(scores), _ptr(sol), B, _ptr(d_rows),
                                                 _ptr(table[0]), _ptr(table[1]), kicks, kick_size, int(max_rounds),
                                                 int(kicks_per_launch), _ptr(ws), nbytes, counters, per, _stream(device)))
    else:
        ws, nbytes = _workspace(L.difusco_mis_iterated_search_workspace_bytes, n, int(graph.col.shape[0]), B, device=device)
        _lib.check(L.difusco_mis_iterated_search(n, _ptr(graph.rowptr), _ptr(col), _ptr(scores), _ptr(sol), B, _ptr(d_rows),
                                                 _ptr(table[0]), _ptr(table[1]), kicks, kick_size, int(max_rounds), _ptr(ws), nbytes,
                                                 counters, per, _stream(device)))
    if stats is not None:
        _mis_counters(stats, counters)
        stats["host_syncs"] = int(L.difusco_mis_search_host_syncs())
        p = np.array(per[:], dtype=np.int64).reshape(B, 4)
        for k, name in enumerate(("entered", "accepted", "size_before", "size_after")):
            stats[name] = p[:, k].tolist()
    return sol.cpu().numpy().astype(int)
