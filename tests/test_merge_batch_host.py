"""Host-side checks of the batched merge (``difusco_tsp_merge_batch``): the symbols, the unchanged ABI version, every refusal of
the library entries (all raised before any GPU work: the device pointers here are fake) and the argument errors of the Python
layer.  No GPU."""
import ctypes
import types

import numpy as np
import pytest
import torch

from difusco_amd import _lib
from difusco_amd import evaluate as E

EINVAL = -1


def test_symbols_exist_and_abi_version_is_unchanged():
    L = _lib.lib()
    assert L.difusco_tsp_merge_batch_workspace_bytes is not None and L.difusco_tsp_merge_batch is not None
    assert L.difusco_abi_version() == 13 == _lib.ABI_VERSION      # additive: no ABI bump
    from difusco_amd import decode
    assert decode.MERGE_STATE_GLOBAL == 1 and decode.MERGE_METHODS == ("loop", "batched")


def _tables(n, edges, samples):
    return np.asarray(n, dtype=np.int32), np.asarray(edges, dtype=np.int64), np.asarray(samples, dtype=np.int32)


def _batch(L, n, edges, samples, *, graphs=None, row=True, col=True, heat=True, points=True, ws=True, ws_bytes=1 << 50,
           tours=True, flags=0, null_table=None):
    """A call whose device pointers are never touched: every case here must be refused by the host checks."""
    fake = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(fake)
    gn, ge, gp = _tables(n, edges, samples)                      # named: the arrays must outlive the call
    tabs = {"n": gn.ctypes.data, "edges": ge.ctypes.data, "samples": gp.ctypes.data}
    if null_table:
        tabs[null_table] = None
    out = np.zeros(1 << 12, dtype=np.int32)
    return L.difusco_tsp_merge_batch(len(n) if graphs is None else graphs, tabs["n"], tabs["edges"], tabs["samples"],
                                     addr if row else None, addr if col else None, addr if heat else None,
                                     addr if points else None, flags, addr if ws else None, ws_bytes,
                                     out.ctypes.data if tours else None, None, None, None)


def _refused(L, rc, *words):
    assert rc == EINVAL
    msg = L.difusco_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_merge_batch_refusals_name_their_reason():
    L = _lib.lib()
    _refused(L, _batch(L, [], [], [], graphs=0), "graphs")
    _refused(L, _batch(L, [10], [30], [1], graphs=-2), "graphs")
    for table in ("n", "edges", "samples"):
        _refused(L, _batch(L, [10], [30], [1], null_table=table), "null")
    for hole in ("heat", "points", "ws", "tours"):
        _refused(L, _batch(L, [10], [30], [1], **{hole: False}), "non-null")
    _refused(L, _batch(L, [10], [30], [1], row=False), "row and col")
    _refused(L, _batch(L, [10], [30], [1], col=False), "row and col")
    _refused(L, _batch(L, [10, 2, 12], [30, 4, 40], [1, 1, 1]), "graph 1", "n = 2")
    _refused(L, _batch(L, [10, 12], [30, 0], [1, 1]), "graph 1", "0 edges")
    _refused(L, _batch(L, [10, 12], [-5, 40], [1, 1]), "graph 0", "edges")
    _refused(L, _batch(L, [10, 12], [30, (1 << 32) + 1], [1, 1]), "graph 1", "2^32")
    _refused(L, _batch(L, [10, 12], [100, 143], [1, 1], row=False, col=False), "graph 1", "n^2 = 144")
    _refused(L, _batch(L, [10, 12], [30, 40], [1, 0]), "graph 1", "0 samples")
    _refused(L, _batch(L, [10, 12], [30, 40], [-1, 2]), "graph 0", "samples")
    _refused(L, _batch(L, [10], [30], [1], flags=2), "flag")
    _refused(L, _batch(L, [10], [30], [1], flags=1 | (1 << 31)), "flag")
    _refused(L, _batch(L, [10, 12], [30, 40], [2, 3], ws_bytes=0), "workspace")
    _refused(L, _batch(L, [10, 12], [30, 40], [2, 3], ws_bytes=1000), "workspace")
    _refused(L, _batch(L, [10, 12], [100, 144], [2, 3], row=False, col=False, ws_bytes=64), "workspace")


def test_merge_batch_workspace_bytes_refusals():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()

    def call(n, edges, samples, graphs=None, out=nbytes):
        gn, ge, gp = _tables(n, edges, samples)
        return L.difusco_tsp_merge_batch_workspace_bytes(len(n) if graphs is None else graphs, gn.ctypes.data, ge.ctypes.data,
                                                         gp.ctypes.data, None if out is None else ctypes.byref(out))

    _refused(L, call([10], [30], [1], out=None), "null")
    _refused(L, call([], [], [], graphs=0), "graphs")
    _refused(L, call([10, 2], [30, 4], [1, 1]), "graph 1", "n = 2")
    _refused(L, call([10], [0], [1]), "graph 0", "edges")
    _refused(L, call([10], [(1 << 32) + 1], [1]), "2^32")
    _refused(L, call([10], [30], [0]), "graph 0", "samples")
    _refused(L, L.difusco_tsp_merge_batch_workspace_bytes(1, None, None, None, ctypes.byref(nbytes)), "null")


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library entry {name} reached")


def test_python_layer_rejects_unknown_values_before_any_library_call(monkeypatch):
    from difusco_amd.decode import check_merge_method, merge_tours_batch
    from difusco_amd.pipeline import solve_tsp_batch
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    model = types.SimpleNamespace(device=torch.device("cpu"))
    rng = np.random.default_rng(0)
    pts = [rng.random((20, 2)), rng.random((31, 2))]
    with pytest.raises(ValueError, match="merge method"):
        solve_tsp_batch(model, pts, 5, merge_method="bogus")                       # list form
    with pytest.raises(ValueError, match="merge method"):
        solve_tsp_batch(model, np.stack([pts[0], pts[0]]), 5, merge_method="")     # array form
    assert check_merge_method("loop") == "loop" and check_merge_method("batched") == "batched"
    heats = [np.zeros(20 * 20, np.float32), np.zeros(31 * 31, np.float32)]
    with pytest.raises(ValueError, match="merge state"):
        merge_tours_batch(heats, pts, None, state="lds")
    with pytest.raises(ValueError, match="point arrays"):
        merge_tours_batch(heats, pts[:1], None)
    with pytest.raises(ValueError, match="edge_index per instance"):
        merge_tours_batch(heats, pts, None, sparse_graph=True)
    with pytest.raises(ValueError, match="parallel_sampling"):
        merge_tours_batch(heats, pts, None, parallel_sampling=[1, 0])


def test_solve_tsp_batch_default_merge_method_is_loop():
    import inspect
    from difusco_amd.pipeline import solve_tsp_batch
    assert inspect.signature(solve_tsp_batch).parameters["merge_method"].default == "loop"


def test_evaluate_accepts_merge_method():
    base = ["--task", "tsp", "--storage_path", "x", "--do_test", "--ckpt_path", "c"]
    args, ignored = E.parse_args(base + ["--merge_method", "batched"])
    assert args.merge_method == "batched" and ignored == []
    assert E.parse_args(base)[0].merge_method == "loop"
    assert "merge_method" not in E.TRAINING_ONLY
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--merge_method", "bogus"])
