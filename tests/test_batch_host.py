"""CPU-only tests of batched instances (ABI 13): the argument block of the per-instance random streams, its validation, the
union graph with one statistic segment per instance, and the argument errors of the batch APIs."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from difusco_amd import _lib
from difusco_amd.graph import build_csr, build_union_csr
from oracle import difusco_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_struct_fields():
    hdr = open(os.path.join(ROOT, "include", "difusco_hip.h")).read()
    body = re.search(r"typedef struct difusco_step_args \{(.*?)\} difusco_step_args;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        parts = re.sub(r"\[[^\]]*\]", "", decl).split(",")      # "uint64_t seed, offset" declares two fields
        names.append(parts[0].split()[-1].lstrip("*"))
        names += [v.strip().lstrip("*") for v in parts[1:]]
    return names


def test_step_args_mirror_the_header_at_abi_13():
    assert _lib.ABI_VERSION == 13 and _lib.lib().difusco_abi_version() == 13
    assert [f[0] for f in _lib.StepArgs._fields_] == _header_struct_fields()
    assert _lib.RAND_PHILOX_INSTANCES == 3
    names = [f[0] for f in _lib.StepArgs._fields_]
    assert names[-3:] == ["n_instances", "instance_rows", "instance_seeds"]


def _args(**kw):
    a = _lib.StepArgs()
    a.struct_size, a.abi_version = ctypes.sizeof(_lib.StepArgs), _lib.ABI_VERSION
    a.hidden, a.n_layers, a.out_channels, a.task = 256, 12, 2, _lib.TASK_TSP
    a.diffusion, a.n_nodes, a.n_edges, a.n_segments = _lib.CATEGORICAL, 10, 20, 1
    for name in ("weights", "rowptr", "col", "xt", "xt_out", "workspace", "points"):
        setattr(a, name, 0x1000)            # never dereferenced: validation fails first
    a.precision = _lib.PRECISIONS["fp16x3"]
    a.post[4] = 1.0
    a.rand_mode = _lib.RAND_PHILOX_INSTANCES
    a.n_instances, a.instance_rows, a.instance_seeds = 2, 0x2000, 0x3000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad", [dict(n_instances=0), dict(n_instances=-1), dict(instance_rows=None),
                                 dict(instance_seeds=None), dict(rand_mode=4)])
def test_per_instance_mode_validated_before_gpu_work(bad):
    L = _lib.lib()
    rc = L.difusco_denoise_step(ctypes.byref(_args(**bad)))
    assert rc == -1        # DIFUSCO_EINVAL
    msg = L.difusco_last_error().decode()
    assert "PHILOX_INSTANCES" in msg or "unknown rand_mode" in msg, msg


def test_stand_alone_posteriors_refuse_the_per_instance_mode():
    L = _lib.lib()
    post = (ctypes.c_float * 8)(0, 0, 0, 0, 1, 0, 0, 0)
    p = ctypes.c_void_p(0x1000)
    assert L.difusco_categorical_posterior(p, p, post, 3, None, 0, 0, p, None, 16, None) == -1
    assert "rand_mode" in L.difusco_last_error().decode()
    assert L.difusco_gaussian_posterior(p, p, post, 3, None, 0, 0, p, 16, None) == -1


def _tsp_instances(sizes, k, copies=1):
    pts, eis = [], []
    for i, n in enumerate(sizes):
        p, ei = O.tsp_instance(n, k, seed=10 + i)
        shift = torch.arange(copies).view(1, -1, 1) * n
        eis.append((torch.from_numpy(ei).reshape(2, 1, -1) + shift).reshape(2, -1))
        pts.append(torch.from_numpy(np.tile(p, (copies, 1))))
    return pts, eis


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("copies", [1, 3])
def test_union_segments_are_contiguous_and_per_instance(reorder, copies):
    sizes, k = [40, 75, 52], 6
    pts, eis = _tsp_instances(sizes, k, copies)
    counts = [p.shape[0] for p in pts]
    g, union, rows = build_union_csr(eis, counts, "cpu", points=torch.cat(pts) if reorder else None)
    expect = np.concatenate([[0], np.cumsum([copies * n * k for n in sizes])])
    assert np.array_equal(rows, expect)                                # P x per-instance edges, caller order
    assert g.n_segments == len(sizes)
    assert np.array_equal(g.seg_ptr.numpy(), expect)                   # CSR-slot order: the same contiguous ranges
    assert (g.node_order is not None) == reorder
    # every CSR slot of segment b is an edge of instance b (through perm), with both ends among instance b's nodes
    perm = g.perm.numpy() if g.perm is not None else np.arange(g.n_edges)
    inst_of_edge = np.searchsorted(expect, perm, side="right") - 1
    seg_of_slot = np.searchsorted(expect, np.arange(g.n_edges), side="right") - 1
    assert np.array_equal(inst_of_edge, seg_of_slot)
    node_off = np.concatenate([[0], np.cumsum(counts)])
    order = g.node_order.numpy() if g.node_order is not None else np.arange(g.n_nodes)
    assert np.array_equal(np.searchsorted(node_off, order, side="right") - 1,
                          np.searchsorted(node_off, np.arange(g.n_nodes), side="right") - 1)
    # the union's edge list is the concatenation, node ids shifted per instance
    assert torch.equal(union, torch.cat([e + int(node_off[b]) for b, e in enumerate(eis)], dim=1))


def test_union_of_one_instance_is_the_plain_graph():
    pts, eis = _tsp_instances([50], 5, copies=2)
    g, _, rows = build_union_csr(eis, [100], "cpu", points=pts[0])
    ref = build_csr(eis[0], 100, "cpu", points=pts[0])
    assert g.n_segments == 1 and g.seg_ptr is None and list(rows) == [0, 500]
    for name in ("rowptr", "col", "perm", "row", "node_order"):
        assert torch.equal(getattr(g, name), getattr(ref, name)), name


def test_mis_union_segments_count_nodes():
    eis = [torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), torch.tensor([[0, 3], [3, 0]]), torch.tensor([[0], [0]])]
    g, union, rows = build_union_csr(eis, [3, 5, 2], "cpu", task_rows="nodes")
    assert list(rows) == [0, 3, 8, 10]
    assert g.n_segments == 3 and g.seg_ptr.tolist() == [0, 3, 8, 10]
    assert union[:, 4:].tolist() == [[3, 6, 8], [6, 3, 8]]


def test_union_rejects_edges_outside_their_instance():
    with pytest.raises(ValueError, match="outside"):
        build_union_csr([torch.tensor([[0, 1], [1, 3]])], [3], "cpu")


def test_batch_api_argument_errors():
    from difusco_amd.decode import batched_two_opt_grouped
    from difusco_amd.pipeline import solve_mis_batch, solve_tsp_batch
    model = types.SimpleNamespace(device=torch.device("cpu"))
    pts = np.random.default_rng(0).random((3, 20, 2))
    with pytest.raises(ValueError, match=r"\[B, N, 2\]"):
        solve_tsp_batch(model, pts[0], sparse_factor=5)
    with pytest.raises(ValueError, match="seeds"):
        solve_tsp_batch(model, pts, sparse_factor=5, seeds=[1, 2])
    with pytest.raises(ValueError, match="generators"):
        solve_tsp_batch(model, pts, sparse_factor=5, generators=[None])
    with pytest.raises(ValueError, match="instances_per_call"):
        solve_tsp_batch(model, pts, sparse_factor=5, instances_per_call=0)
    with pytest.raises(ValueError, match="at least one"):
        solve_mis_batch(model, [])
    with pytest.raises(ValueError, match="seeds"):
        solve_mis_batch(model, [(3, np.zeros((2, 0), np.int64))], seeds=[1, 2])
    with pytest.raises(_lib.DifuscoHipError, match="GPU only"):
        batched_two_opt_grouped(pts, np.zeros((3, 21), np.int64), device="cpu")
    with pytest.raises(ValueError, match="points"):
        batched_two_opt_grouped(pts[0], np.zeros((3, 21), np.int64), device="cuda:0")
    with pytest.raises(ValueError, match="tours"):
        batched_two_opt_grouped(pts, np.zeros((4, 21), np.int64), device="cuda:0")
    with pytest.raises(ValueError, match="tours"):
        batched_two_opt_grouped(pts, np.zeros((3, 20), np.int64), device="cuda:0")


def test_grouped_two_opt_entry_rejects_bad_arguments_without_gpu():
    L = _lib.lib()
    nb = ctypes.c_size_t()
    assert L.difusco_tsp_two_opt_grouped_workspace_bytes(3, 2, 2, ctypes.byref(nb)) == -1
    assert L.difusco_tsp_two_opt_grouped_workspace_bytes(10, 0, 2, ctypes.byref(nb)) == -1
    assert L.difusco_tsp_two_opt_grouped_workspace_bytes(10, 2, 0, ctypes.byref(nb)) == -1
    assert L.difusco_tsp_two_opt_grouped_workspace_bytes(10, 2, 3, ctypes.byref(nb)) == 0 and nb.value > 0
    its = (ctypes.c_int64 * 2)()
    p = ctypes.c_void_p(0x1000)
    assert L.difusco_tsp_two_opt_grouped(10, 2, 3, p, p, 5, p, 0, its, None) == -1      # workspace too small
    assert "workspace" in L.difusco_last_error().decode()
    assert L.difusco_tsp_two_opt_grouped(10, 2, 3, p, p, 5, p, nb.value, None, None) == -1      # no iterations_out
    assert L.difusco_tsp_two_opt_grouped(10, 2, 3, p, p, -1, p, nb.value, its, None) == -1
