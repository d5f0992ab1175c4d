"""Host-side checks of the device graph build (``difusco_graph_build``): the symbols, the unchanged ABI version, every refusal the
library raises before any GPU work (the device pointers here are fake), the argument errors of the Python layer, and the device
ALGORITHM restated in numpy (tests/graph_build_emulation.py) against the host build on the case list of the GPU tests.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import graph_build_emulation as G
from difusco_amd import _lib
from difusco_amd import evaluate as E

EINVAL = -1
INT32_MAX = 2 ** 31 - 1


def test_symbols_exist_and_abi_version_is_unchanged():
    L = _lib.lib()
    assert L.difusco_graph_build_workspace_bytes is not None and L.difusco_graph_build is not None
    assert L.difusco_abi_version() == 13 == _lib.ABI_VERSION      # additive: no ABI bump
    assert (_lib.GRAPH_PERM_IDENTITY, _lib.GRAPH_ORDER_IDENTITY, _lib.GRAPH_BAD_EDGE) == (1, 2, 4)


def _refused(L, rc, *words):
    assert rc == EINVAL
    msg = L.difusco_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def _build(L, n=10, e=30, *, ei=True, points=True, f64=0, rowptr=True, col=True, row=True, perm=True, order=True, flags=True,
           ws=True, ws_bytes=1 << 50):
    """A call whose device pointers are never touched: every case here must be refused by the host checks."""
    fake = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(fake)
    out = (ctypes.c_uint32 * 2)()
    p = lambda on: addr if on else None      # noqa: E731
    return L.difusco_graph_build(n, e, p(ei), p(points), f64, p(rowptr), p(col), p(row), p(perm), p(order),
                                 out if flags else None, p(ws), ws_bytes, None)


def test_graph_build_refusals_name_their_reason():
    L = _lib.lib()
    for hole in ("rowptr", "flags", "ws"):
        _refused(L, _build(L, **{hole: False}), "null")
    for hole in ("ei", "col", "row", "perm"):
        _refused(L, _build(L, **{hole: False}), "null")
    _refused(L, _build(L, order=False), "null", "node_order")
    _refused(L, _build(L, n=-1), "sizes")
    _refused(L, _build(L, e=-1), "sizes")
    _refused(L, _build(L, n=INT32_MAX), "sizes")
    _refused(L, _build(L, e=INT32_MAX + 1), "sizes")
    _refused(L, _build(L, n=1 << 40, e=1 << 40), "sizes")
    _refused(L, _build(L, f64=2), "points_f64")
    # the library's own arrays alone need more than this (the exact size is refused too: tests/test_gpu_graph_build.py; the
    # sort's share of it is a question to the device)
    for small in (0, 64, 1000):
        _refused(L, _build(L, ws_bytes=small), "workspace")
        _refused(L, _build(L, points=False, ws_bytes=small), "workspace")


def test_graph_build_workspace_bytes_refusals():
    L = _lib.lib()
    nbytes = ctypes.c_size_t()
    _refused(L, L.difusco_graph_build_workspace_bytes(10, 30, 1, None), "null")
    _refused(L, L.difusco_graph_build_workspace_bytes(-1, 30, 1, ctypes.byref(nbytes)), "sizes")
    _refused(L, L.difusco_graph_build_workspace_bytes(10, -1, 0, ctypes.byref(nbytes)), "sizes")
    _refused(L, L.difusco_graph_build_workspace_bytes(INT32_MAX, 30, 1, ctypes.byref(nbytes)), "sizes")
    _refused(L, L.difusco_graph_build_workspace_bytes(10, INT32_MAX + 1, 0, ctypes.byref(nbytes)), "sizes")
    # the limits themselves are no argument error (without a device the size of the sort storage cannot be asked: EHIP)
    assert L.difusco_graph_build_workspace_bytes(INT32_MAX - 1, INT32_MAX, 1, ctypes.byref(nbytes)) in (0, -3)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library entry {name} reached")


def test_python_layer_rejects_unknown_values_before_any_library_call(monkeypatch):
    from difusco_amd.decode import mis_decode_np
    from difusco_amd.graph import GRAPH_BUILDS, build_csr, build_union_csr, check_graph_build
    from difusco_amd.models import COMetaModel, MISModel, TSPModel
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    assert GRAPH_BUILDS == ("host", "device")
    assert check_graph_build("host") == "host" and check_graph_build("device") == "device"
    ei = torch.zeros((2, 3), dtype=torch.int64)
    for bad in ("bogus", "", None, "Device"):
        with pytest.raises(ValueError, match="graph build"):
            check_graph_build(bad)
        with pytest.raises(ValueError, match="graph build"):
            build_csr(ei, 4, "cpu", method=bad)
        with pytest.raises(ValueError, match="graph build"):
            build_union_csr([ei], [4], "cpu", method=bad)
        for cls in (COMetaModel, TSPModel, MISModel):
            with pytest.raises(ValueError, match="graph build"):
                cls({}, engine=object(), graph_build=bad)
        with pytest.raises(ValueError, match="graph build"):
            mis_decode_np(np.zeros(4, np.float32), edge_index=ei, device="cpu", graph_build=bad)


def test_defaults_stay_host():
    from difusco_amd.decode import mis_decode_np
    from difusco_amd.graph import build_csr, build_union_csr
    from difusco_amd.models import COMetaModel
    assert inspect.signature(build_csr).parameters["method"].default == "host"
    assert inspect.signature(build_union_csr).parameters["method"].default == "host"
    assert inspect.signature(COMetaModel.__init__).parameters["graph_build"].default == "host"
    assert inspect.signature(mis_decode_np).parameters["graph_build"].default == "host"


def test_evaluate_accepts_graph_build():
    base = ["--task", "tsp", "--storage_path", "x", "--do_test", "--ckpt_path", "c"]
    args, ignored = E.parse_args(base + ["--graph_build", "device"])
    assert args.graph_build == "device" and ignored == []
    assert E.parse_args(base)[0].graph_build == "host"
    assert "graph_build" not in E.TRAINING_ONLY
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--graph_build", "bogus"])


# ---- the device algorithm, in numpy, against the host build ------------------------------------------------------------------
CASES = G.single_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_emulated_device_algorithm_equals_host_build(case):
    _, ei, n, pts = case
    G.assert_same(G.emulate(ei, n, pts), G.host(ei, n, pts))


def test_case_list_reaches_the_paths_it_names():
    res = {name: G.host(ei, n, pts) for name, ei, n, pts in CASES}
    assert res["nopoints-sorted"]["perm_identity"] and not res["nopoints-shuffled"]["perm_identity"]
    assert res["tsp-2000-k100"]["node_order"] is not None and res["tsp-2000-k100"]["rowptr"][-1] == 200000
    assert not res["mis-er300"]["perm_identity"]
    assert res["tiny-no-edges"]["node_order"] is None and res["tiny-n1-loop"]["node_order"] is None
    # the copies of a duplicated instance differ only in their block: every copy gets the same order, shifted
    order = res["tsp-duplicated-x3"]["node_order"].reshape(3, 30)
    assert np.array_equal(order[1], order[0] + 30) and np.array_equal(order[2], order[0] + 60)
    # coincident points: equal keys stay in id order (i before i + 28 for the twelve repeated points)
    pos = np.empty(40, dtype=np.int64)
    pos[res["ties-coincident"]["node_order"]] = np.arange(40)
    assert all(pos[i + 28] == pos[i] + 1 for i in range(12))
    assert bool(G.bits(64) == 6 and G.bits(65) == 7 and G.bits(1) == 1 and G.bits(2) == 1)


def test_emulated_unions_equal_host_unions():
    from difusco_amd.graph import build_union_csr
    eis, ns, pts = G.tsp_union_case()
    g, union, rows = build_union_csr([torch.from_numpy(e) for e in eis], ns, "cpu", points=pts)
    assert g.n_segments == 3 and np.array_equal(rows, np.cumsum([0] + [e.shape[1] for e in eis]))
    G.assert_same(G.emulate(union.numpy(), sum(ns), pts), G.host(union.numpy(), sum(ns), pts))
    eis, ns = G.mis_union_case()
    g, union, rows = build_union_csr([torch.from_numpy(e) for e in eis], ns, "cpu", task_rows="nodes")
    assert g.n_segments == 3 and np.array_equal(rows, [0, 300, 600, 900])
    G.assert_same(G.emulate(union.numpy(), 900), G.host(union.numpy(), 900))
