"""The device graph build (``difusco_graph_build`` / ``graph.build_csr(method="device")``) on a real GPU: for every graph of the
case list (tests/graph_build_emulation.py) the ``CsrGraph`` equals the host method's in every field, exactly, the ``None``
fields included; the refusals return an error code and leave the device usable; and whole solves on a model built with
``graph_build="device"`` return exactly what the ``"host"`` model returns."""
import ctypes
import os

import numpy as np
import pytest
import torch

import graph_build_emulation as G
from difusco_amd import _lib

pytestmark = pytest.mark.gpu

FIELDS = ("rowptr", "col", "row", "perm", "node_order", "seg_ptr")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _gpu_knn(dev):
    from difusco_amd.graph import knn_edge_index_gpu
    return lambda pts, k: knn_edge_index_gpu(np.asarray(pts, dtype=np.float64), k, device=dev).cpu().numpy()


def _same_graph(a, b):
    assert (a.n_nodes, a.n_edges, a.n_segments) == (b.n_nodes, b.n_edges, b.n_segments)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert x.dtype == y.dtype and x.device == y.device and x.shape == y.shape and torch.equal(x, y), f


def _both(dev, ei, n, pts, **kw):
    from difusco_amd.graph import build_csr
    ei_d = torch.from_numpy(ei).to(dev)                          # the device method starts from the device
    p = None if pts is None else torch.from_numpy(pts)
    host = build_csr(ei_d, n, dev, points=p, method="host", **kw)
    device = build_csr(ei_d, n, dev, points=None if p is None else p.to(dev), method="device", **kw)
    _same_graph(device, host)
    return device, host


@pytest.fixture(scope="module")
def cases(dev):
    return {c[0]: c for c in G.single_cases(_gpu_knn(dev))}


NAMES = [c[0] for c in G.single_cases(lambda pts, k: np.zeros((2, 0), dtype=np.int64))]      # the names alone: no k-NN here


@pytest.mark.parametrize("name", NAMES)
def test_device_build_equals_host_build(dev, cases, name):
    _, ei, n, pts = cases[name]
    g, _ = _both(dev, ei, n, pts)
    if name == "nopoints-sorted":
        assert g.perm is None and g.node_order is None
    if name == "nopoints-shuffled":
        assert g.perm is not None
    if name == "tsp-2000-k100":
        assert g.n_edges == 200000 and g.node_order is not None
    if pts is not None and n > 1 and ei.shape[1]:
        # host points, float64 points and points with spare rows give the same graph
        from difusco_amd.graph import build_csr
        ei_d = torch.from_numpy(ei).to(dev)
        _same_graph(build_csr(ei_d, n, dev, points=pts, method="device"), g)
        wide = torch.from_numpy(np.concatenate([pts, pts[:1]]).astype(np.float64)).to(dev)
        _same_graph(build_csr(ei_d, n, dev, points=wide, method="device"), g)


def test_float64_points_are_used_as_float64(dev):
    """float64 coordinates j / 65535 over the box [0, 1]: every quantised value sits on an integer boundary, where the float64
    rounding of the division decides the truncation - and the float32 value of the same coordinate decides otherwise."""
    rng = np.random.default_rng(8)
    pts = rng.integers(0, 65536, (60, 2)) / 65535.0
    pts[0], pts[1] = 0.0, 1.0
    assert not np.array_equal(G.morton(pts), G.morton(pts.astype(np.float32)))
    ei = G.numpy_knn(pts, 6)
    g, _ = _both(dev, ei, 60, pts)
    assert g.node_order is not None


def test_tsp_union_of_different_sizes(dev):
    from difusco_amd.graph import build_union_csr
    eis, ns, pts = G.tsp_union_case(_gpu_knn(dev))
    eis_d = [torch.from_numpy(e).to(dev) for e in eis]
    gh, uh, rh = build_union_csr(eis_d, ns, dev, points=torch.from_numpy(pts))
    gd, ud, rd = build_union_csr(eis_d, ns, dev, points=torch.from_numpy(pts).to(dev), method="device")
    _same_graph(gd, gh)
    assert gd.n_segments == 3 and gd.seg_ptr is not None
    assert isinstance(rd, np.ndarray) and rd.dtype == rh.dtype and np.array_equal(rd, rh)
    assert ud.device.type == "cuda" and torch.equal(ud.cpu(), uh.cpu())
    # one instance: no segments, as the host method
    g1h, _, _ = build_union_csr(eis_d[:1], ns[:1], dev, points=pts[:20])
    g1d, _, _ = build_union_csr(eis_d[:1], ns[:1], dev, points=pts[:20], method="device")
    _same_graph(g1d, g1h)
    assert g1d.seg_ptr is None and g1d.n_segments == 1


def test_mis_union_in_node_rows(dev):
    from difusco_amd.graph import build_union_csr
    eis, ns = G.mis_union_case()
    gh, _, rh = build_union_csr([torch.from_numpy(e) for e in eis], ns, dev, task_rows="nodes")
    gd, _, rd = build_union_csr(eis, ns, dev, task_rows="nodes", method="device")          # numpy input, as the host takes it
    _same_graph(gd, gh)
    assert gd.n_segments == 3 and np.array_equal(rd, rh) and np.array_equal(rd, [0, 300, 600, 900])


def test_seg_rows_pass_through(dev):
    ei = G.numpy_knn(G.tsp_points(45, 9), 7)
    g, _ = _both(dev, ei[:, np.random.default_rng(3).permutation(ei.shape[1])], 45, None, seg_rows=np.array([0, 20, 45]))
    assert g.n_segments == 2 and g.seg_ptr.tolist() == [0, 20, 45]


# ---- refusals: an error code, and the device stays usable -------------------------------------------------------------------
def test_out_of_range_edge_is_refused_and_named(dev):
    from difusco_amd.graph import build_csr
    pts = G.tsp_points(50, 1)
    ei = G.numpy_knn(pts, 6)
    bad = ei.copy()
    bad[1, 211] = 50                                              # == n_nodes
    bad[0, 37] = 50
    bad[1, 120] = -1
    for p in (None, pts):
        with pytest.raises(_lib.DifuscoHipError, match=r"edge 37 = \(50,\d+\) out of range \[0,50\)"):
            build_csr(torch.from_numpy(bad).to(dev), 50, dev, points=p, method="device")
        with pytest.raises(_lib.DifuscoHipError, match=r"edge 37 = \(50,\d+\) out of range \[0,50\)"):
            build_csr(torch.from_numpy(bad), 50, dev, points=p, method="host")
        _both(dev, ei, 50, p)                                     # the next call on the same device succeeds
    huge = ei.copy()
    huge[1, 5] = 2 ** 40 + 3                                      # would pass a check made after a cast to int32
    with pytest.raises(_lib.DifuscoHipError, match=r"edge 5 = "):
        build_csr(torch.from_numpy(huge).to(dev), 50, dev, points=pts, method="device")
    _both(dev, ei, 50, pts)


def test_union_edge_leaving_its_instance_is_refused(dev):
    from difusco_amd.graph import build_union_csr
    eis, ns, pts = G.tsp_union_case()
    for b, value in [(0, 20), (1, -1), (2, 64)]:                  # inside the union, below it, past its end
        bad = [e.copy() for e in eis]
        bad[b][1, 3] = value
        msgs = []
        for method in ("host", "device"):
            with pytest.raises(ValueError) as info:
                build_union_csr([torch.from_numpy(e) for e in bad], ns, dev, points=pts, method=method)
            msgs.append(str(info.value))
        assert msgs[0] == msgs[1] and f"instance {b}" in msgs[0]
        with pytest.raises(ValueError, match=f"instance {b}"):
            build_union_csr([torch.from_numpy(e) for e in bad], ns, dev, task_rows="nodes", method="device")
    gd, _, _ = build_union_csr(eis, ns, dev, points=pts, method="device")
    gh, _, _ = build_union_csr([torch.from_numpy(e) for e in eis], ns, dev, points=pts)
    _same_graph(gd, gh)


def test_workspace_one_byte_short_is_refused(dev):
    L = _lib.lib()
    need = ctypes.c_size_t()
    _lib.check(L.difusco_graph_build_workspace_bytes(10, 30, 1, ctypes.byref(need)))
    without = ctypes.c_size_t()
    _lib.check(L.difusco_graph_build_workspace_bytes(10, 30, 0, ctypes.byref(without)))
    assert 0 < without.value < need.value
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    flags = (ctypes.c_uint32 * 2)()
    a = ctypes.c_void_p(ws.data_ptr())
    for points, size in [(a, need.value - 1), (None, without.value - 1)]:
        assert L.difusco_graph_build(10, 30, a, points, 0, a, a, a, a, a, flags, a, size, None) == -1
        assert "workspace" in L.difusco_last_error().decode()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _weights(golden_dir):
    z = np.load(os.path.join(golden_dir, "weights_h64_l2.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files if k != "provenance" and not k.startswith("gaussian_")}


def _models(cls_name, golden_dir, dev, sparse_factor):
    from difusco_amd import models
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=2, hidden_dim=64, inference_trick="ddim", inference_diffusion_steps=5, inference_schedule="cosine")
    return [getattr(models, cls_name)(args, _weights(golden_dir), device=dev, seed=7, graph_build=m) for m in ("host", "device")]


def test_solve_tsp_is_the_same(dev, golden_dir):
    from difusco_amd.pipeline import solve_tsp
    pts = np.random.default_rng(50).random((50, 2))
    runs = [solve_tsp(m, pts, 10, parallel_sampling=2, two_opt_iterations=100, generator=torch.Generator().manual_seed(3))
            for m in _models("TSPModel", golden_dir, dev, 10)]
    assert runs[0] == runs[1]


def test_solve_tsp_batch_of_different_sizes_is_the_same(dev, golden_dir):
    from difusco_amd.pipeline import solve_tsp_batch
    rng = np.random.default_rng(51)
    pts = [rng.random((n, 2)) for n in (30, 50, 41)]
    runs = [solve_tsp_batch(m, pts, 10, parallel_sampling=2, two_opt_iterations=100, seeds=[5, 6, 7],
                            generators=[torch.Generator().manual_seed(b) for b in range(3)], step_offset=0)
            for m in _models("TSPModel", golden_dir, dev, 10)]
    assert runs[0] == runs[1]


def test_solve_mis_batch_is_the_same(dev, golden_dir):
    from difusco_amd.pipeline import solve_mis_batch
    inst = [(60, G.er_edge_index(60, 0.1, 30 + g)) for g in range(2)]
    runs = []
    for m in _models("MISModel", golden_dir, dev, -1):
        res = solve_mis_batch(m, inst, parallel_sampling=2, seeds=[1, 2], generators=[torch.Generator().manual_seed(b) for b in range(2)],
                              step_offset=0)
        runs.append([(sol.tolist(), size, sizes) for sol, size, sizes in res])
    assert runs[0] == runs[1]


def test_mis_decode_builds_its_graph_on_the_device(dev):
    from difusco_amd.decode import mis_decode_np
    ei = G.er_edge_index(80, 0.1, 40)
    scores = np.random.default_rng(4).random(80).astype(np.float32)
    assert np.array_equal(mis_decode_np(scores, edge_index=ei, device=dev, graph_build="device"),
                          mis_decode_np(scores, edge_index=ei, device=dev))


def test_graphed_sampling_on_a_device_built_graph(dev, golden_dir):
    """Twin models (equal weights, seed and call counter), both with the device build: one graphed, one eager."""
    from difusco_amd import models
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=10, n_layers=2,
                hidden_dim=64, inference_trick="ddim", inference_diffusion_steps=5, inference_schedule="cosine")
    eager, graphed = [models.TSPModel(args, _weights(golden_dir), device=dev, seed=11, graph_build="device") for _ in range(2)]
    pts = torch.from_numpy(G.tsp_points(50, 9)).to(dev)
    ei = torch.from_numpy(_gpu_knn(dev)(pts.cpu().numpy(), 10)).to(dev)
    a = eager.sample(pts, ei, generator=torch.Generator(device=dev).manual_seed(2))
    b = graphed.sample(pts, ei, generator=torch.Generator(device=dev).manual_seed(2), graphed=True)
    assert eager.prepare_graph(ei, 50, points=pts).node_order is not None
    assert a.shape == b.shape and torch.equal(a, b)
