"""Host-side checks of the mixed-size TSP batch: the dense union graph, the mixed chunk planner, the refusals of the ragged
2-opt entries (all raised before any GPU work) and the argument errors of the list form of ``solve_tsp_batch``.  No GPU."""
import ctypes
import types

import numpy as np
import pytest
import torch

from difusco_amd import _lib
from difusco_amd import evaluate as E
from difusco_amd.graph import build_csr, complete_graph_batch, complete_graph_union

EINVAL = -1


def _graph_arrays(g):
    return {k: (None if getattr(g, k) is None else getattr(g, k).tolist()) for k in ("rowptr", "col", "row", "perm", "seg_ptr")}


# ---- complete_graph_union ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,n", [(1, 7), (3, 5), (4, 1)])
def test_union_of_equal_sizes_is_complete_graph_batch(batch, n):
    a, b = complete_graph_union([n] * batch, "cpu"), complete_graph_batch(batch, n, "cpu")
    assert _graph_arrays(a) == _graph_arrays(b)
    assert (a.n_nodes, a.n_edges, a.n_segments) == (b.n_nodes, b.n_edges, b.n_segments)
    for k in ("rowptr", "col", "row"):
        assert getattr(a, k).dtype == getattr(b, k).dtype == torch.int32
    assert (a.seg_ptr is None) == (b.seg_ptr is None) and (a.seg_ptr is None or a.seg_ptr.dtype == b.seg_ptr.dtype)


def test_union_of_mixed_sizes_is_the_csr_of_the_explicit_edge_list():
    sizes = [3, 5, 4]
    edges, off = [], 0
    for n in sizes:                                              # slot of (s, i, j) = off_s + i * n_s + j: this order
        edges += [(off + i, off + j) for i in range(n) for j in range(n)]
        off += n
    seg = np.concatenate([[0], np.cumsum([n * n for n in sizes])])
    ref = build_csr(torch.tensor(edges, dtype=torch.int64).T, off, "cpu", seg_rows=seg)
    g = complete_graph_union(sizes, "cpu")
    assert ref.perm is None                                      # the explicit list is already in CSR-slot order
    assert _graph_arrays(g) == _graph_arrays(ref)
    assert (g.n_nodes, g.n_edges, g.n_segments) == (12, 50, 3) and g.seg_ptr.tolist() == [0, 9, 34, 50]


def test_union_refuses_empty_and_non_positive_sizes():
    for bad in ([], [3, 0]):
        with pytest.raises(ValueError, match="sample_sizes"):
            complete_graph_union(bad, "cpu")


# ---- the mixed chunk planner ------------------------------------------------------------------------------------------------
def test_mixed_chunks_of_a_hand_checked_split():
    # dense, P = 1: rows n^2 = 40000, 90000, 160000, 250000, 10000, 10000, 262144, 1; budget 2^18 = 262144
    sizes = [200, 300, 400, 500, 100, 100, 512, 1]
    assert E.mixed_size_chunks(sizes) == [(0, 2), (2, 3), (3, 5), (5, 6), (6, 7), (7, 8)]
    # 130000 fit, + 160000 would not; 250000 + 10000 fit (260000), + 10000 would not; 262144 fills a run exactly


def test_row_budget_closes_a_run_and_an_oversize_instance_stands_alone():
    assert E.ROWS_PER_CALL == 1 << 18
    k50 = [500] * 12                                             # sparse K = 50: 25000 rows each, 10 fit 2^18
    assert E.mixed_size_chunks(k50, sparse_factor=50) == [(0, 10), (10, 12)]
    assert E.mixed_size_chunks(k50, sparse_factor=50, parallel_sampling=4) == [(i, i + 2) for i in range(0, 12, 2)]
    assert E.mixed_size_chunks([20, 1000, 20]) == [(0, 1), (1, 2), (2, 3)]      # 10^6 rows: over the budget on its own
    rows = [E.tsp_rows(n, 50, 1) for n in k50]
    for lo, hi in E.mixed_size_chunks(k50, sparse_factor=50):
        assert sum(rows[lo:hi]) <= E.ROWS_PER_CALL


def test_mixed_chunks_close_at_64_instances_or_instances_per_call():
    sizes = [20, 30] * 70                                        # 140 tiny instances: the row budget never binds
    assert E.mixed_size_chunks(sizes) == [(0, 64), (64, 128), (128, 140)]
    assert E.mixed_size_chunks(sizes, instances_per_call=50) == [(0, 50), (50, 100), (100, 140)]
    assert E.mixed_size_chunks(sizes, instances_per_call=100) == [(0, 100), (100, 140)]
    assert E.mixed_size_chunks(sizes, instances_per_call=1) == [(i, i + 1) for i in range(140)]
    with pytest.raises(ValueError, match="instances_per_call"):
        E.mixed_size_chunks(sizes, instances_per_call=0)
    assert E.mixed_size_chunks([]) == []


def test_mixed_chunks_do_not_depend_on_the_world_size():
    sizes = [20, 30] * 9 + [500, 40]
    chunks = E.mixed_size_chunks(sizes, instances_per_call=4)
    assert [i for lo, hi in chunks for i in range(lo, hi)] == list(range(len(sizes)))
    for world in (1, 2, 3, 8):
        shards = [E.shard_chunks(chunks, r, world) for r in range(world)]
        assert [c for s in shards for c in s] == chunks          # ranks take whole chunks of the one list


def test_split_chunks_and_the_parser_default_are_unchanged_without_the_flag():
    ex = [types.SimpleNamespace(points=np.zeros((n, 2))) for n in [20, 30, 20, 30, 30, 30]]
    assert E.split_chunks("tsp", ex) == [(0, 1), (1, 2), (2, 3), (3, 6)]
    assert E.split_chunks("tsp", ex, instances_per_call=2) == [(0, 1), (1, 2), (2, 3), (3, 5), (5, 6)]
    base = ["--task", "tsp", "--storage_path", "x", "--do_test", "--ckpt_path", "c"]
    assert E.parse_args(base)[0].mixed_size_chunks is False
    assert E.parse_args(base + ["--mixed_size_chunks"])[0].mixed_size_chunks is True


# ---- the ragged 2-opt entries: refusals before any GPU work -----------------------------------------------------------------
def _i32(v):
    return np.asarray(v, dtype=np.int32)


def _workspace_bytes(L, n, tours, method):
    nbytes = ctypes.c_size_t()
    gn, gt = _i32(n), _i32(tours)                                # named: the arrays must outlive the call
    rc = L.difusco_tsp_two_opt_ragged_workspace_bytes(len(n), gn.ctypes.data, gt.ctypes.data, method, ctypes.byref(nbytes))
    return rc, nbytes.value


def _ragged(L, n, tours, *, groups=None, points=True, tour_arr=True, ws=True, ws_bytes=1 << 40, its=True, method=0, max_it=10,
            n_null=False, tours_null=False):
    """A call whose device pointers are never touched: every case here must be refused by the host checks."""
    fake = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(fake)
    gn, gt = _i32(n), _i32(tours)
    out = np.zeros(max(1, len(n)), dtype=np.int64)
    return L.difusco_tsp_two_opt_ragged(len(n) if groups is None else groups, None if n_null else gn.ctypes.data,
                                        None if tours_null else gt.ctypes.data, addr if points else None,
                                        addr if tour_arr else None, max_it, method, addr if ws else None, ws_bytes,
                                        out.ctypes.data if its else None, None, None)


def _refused(L, rc, *words):
    assert rc == EINVAL
    msg = L.difusco_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_ragged_two_opt_refusals_name_their_reason():
    L = _lib.lib()
    _refused(L, _ragged(L, [], [], groups=0), "groups")
    _refused(L, _ragged(L, [10], [1], groups=-3), "groups")
    _refused(L, _ragged(L, [10, 3, 12], [1, 1, 1]), "group 1", "n = 3")
    _refused(L, _ragged(L, [10, 12], [1, 0]), "group 1", "0 tours")
    _refused(L, _ragged(L, [10, 12], [2, -1]), "group 1", "tours")
    _refused(L, _ragged(L, [10, 12], [65535, 1]), "65535 tours")
    _refused(L, _ragged(L, [10] * 3, [30000] * 3), "65535 tours")
    _refused(L, _ragged(L, [10, 65535 * 16 + 1], [1, 1]), "group 1", str(65535 * 16))
    _refused(L, _ragged(L, [10], [1], n_null=True), "null")
    _refused(L, _ragged(L, [10], [1], tours_null=True), "null")
    for hole in ("points", "tour_arr", "ws", "its"):
        _refused(L, _ragged(L, [10], [1], **{hole: False}), "non-null")
    _refused(L, _ragged(L, [10], [1], max_it=-1), "max_iterations")
    _refused(L, _ragged(L, [10], [1], method=2), "method")
    for method in (0, 1):
        rc, need = _workspace_bytes(L, [10, 12], [2, 3], method)
        assert rc == 0 and need > 0
        _refused(L, _ragged(L, [10, 12], [2, 3], method=method, ws_bytes=need - 1), "workspace", str(need))
        _refused(L, _ragged(L, [10, 12], [2, 3], method=method, ws_bytes=0), "workspace")


def test_ragged_workspace_bytes_refusals():
    L = _lib.lib()
    _refused(L, _workspace_bytes(L, [10, 3], [1, 1], 0)[0], "group 1")
    _refused(L, _workspace_bytes(L, [10], [0], 0)[0], "group 0")
    _refused(L, _workspace_bytes(L, [10, 10], [40000, 40000], 1)[0], "65535 tours")
    _refused(L, _workspace_bytes(L, [10], [1], 7)[0], "method")
    gn, gt = _i32([10]), _i32([1])
    _refused(L, L.difusco_tsp_two_opt_ragged_workspace_bytes(1, gn.ctypes.data, gt.ctypes.data, 0, None), "null")
    _refused(L, L.difusco_tsp_two_opt_ragged_workspace_bytes(0, None, None, 0, ctypes.byref(ctypes.c_size_t())), "groups")
    # the 65535th tour and the largest n are still accepted
    assert _workspace_bytes(L, [4, 4], [65534, 1], 1)[0] == 0
    assert _workspace_bytes(L, [65535 * 16], [1], 0)[0] == 0


@pytest.mark.parametrize("n,G,P", [(4, 1, 1), (50, 64, 1), (500, 16, 4), (1025, 3, 2)])
def test_ragged_workspace_covers_the_grouped_entries_for_equal_groups(n, G, P):
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    assert L.difusco_tsp_two_opt_grouped_workspace_bytes(n, G, P, ctypes.byref(nbytes)) == 0
    rc, ragged = _workspace_bytes(L, [n] * G, [P] * G, 0)
    assert rc == 0 and ragged >= nbytes.value
    assert L.difusco_tsp_two_opt_grouped_screened_workspace_bytes(n, G, P, ctypes.byref(nbytes)) == 0
    rc, ragged1 = _workspace_bytes(L, [n] * G, [P] * G, 1)
    assert rc == 0 and ragged1 >= nbytes.value and ragged1 > ragged


def test_abi_version_is_unchanged():
    assert _lib.lib().difusco_abi_version() == 13 == _lib.ABI_VERSION      # additive: no ABI bump


# ---- argument errors of the Python layer, before any library call ------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library entry {name} reached")


def test_solve_tsp_batch_list_form_argument_errors(monkeypatch):
    from difusco_amd.pipeline import solve_tsp_batch
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    model = types.SimpleNamespace(device=torch.device("cpu"))
    rng = np.random.default_rng(0)
    pts = [rng.random((20, 2)), rng.random((31, 2)), rng.random((8, 2))]
    with pytest.raises(ValueError, match=r"points\[1\] must be \[n, 2\]"):
        solve_tsp_batch(model, [pts[0], rng.random((31, 3))], 5)
    with pytest.raises(ValueError, match=r"points\[0\] must be \[n, 2\]"):
        solve_tsp_batch(model, [rng.random(20), pts[1]], 5)
    with pytest.raises(ValueError, match="seeds"):
        solve_tsp_batch(model, pts, 5, seeds=[1, 2])
    with pytest.raises(ValueError, match="generators"):
        solve_tsp_batch(model, pts, 5, generators=[None])
    with pytest.raises(ValueError, match=r"points\[2\] has 8 nodes, fewer than sparse_factor = 10"):
        solve_tsp_batch(model, pts, 10)
    with pytest.raises(ValueError, match="at least one"):
        solve_tsp_batch(model, [], 5)
    with pytest.raises(ValueError, match="instances_per_call"):
        solve_tsp_batch(model, pts, 5, instances_per_call=0)
    with pytest.raises(ValueError, match="two-opt method"):
        solve_tsp_batch(model, pts, 5, two_opt_method="bogus")


def test_ragged_python_entries_check_their_arguments(monkeypatch):
    from difusco_amd.decode import batched_two_opt_ragged
    from difusco_amd.graph import knn_edge_index_gpu
    pts = [np.zeros((5, 2)), np.zeros((6, 2))]
    with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
        batched_two_opt_ragged(pts, [np.zeros((1, 6), np.int64), np.zeros((2, 7), np.int64)], device="cpu")
    with pytest.raises(ValueError, match="instance 1 has 8 nodes, fewer than k = 10"):      # before anything reaches the device
        knn_edge_index_gpu(np.zeros((58, 2)), 10, sizes=[50, 8])
    with pytest.raises(ValueError, match="sizes sum to"):
        knn_edge_index_gpu(np.zeros((58, 2)), 10, sizes=[50, 10])
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    with pytest.raises(ValueError, match=r"tours_list\[1\]"):
        batched_two_opt_ragged(pts, [np.zeros((1, 6), np.int64), np.zeros((2, 6), np.int64)])
    with pytest.raises(ValueError, match=r"points_list\[0\]"):
        batched_two_opt_ragged([np.zeros((5, 3))], [np.zeros((1, 6), np.int64)])
    with pytest.raises(ValueError, match="tour arrays"):
        batched_two_opt_ragged(pts, [np.zeros((1, 6), np.int64)])
