"""Every GPU entry writes only its outputs and the scratch it declared, and leaves its inputs bit-identical.

The suite holds every entry's results to an oracle (the parity tests) and shows that they do not depend on what the scratch held
(test_gpu_workspace_contents.py).  This file checks WHERE a call writes: each entry runs on cases the suite already holds to an
expectation, with its memory fenced (tests/memory_fence.py): outputs, uploads and workspaces lie between guards of seeded random
bytes, every workspace has exactly the bytes its size function declared, and every ``const`` input is compared byte for byte
before and after.  Every run also asserts its case's own expectation (oracle bound, fixture, numpy restatement), so a fenced run
is a correct run.  Payloads hold seeded random bytes before the call; there is no ``fill`` dimension.

Only ``backend="ctypes"`` is in reach of the hooks (the torch custom ops allocate in C++), and an overrun from one carved piece of
a workspace into the next piece of the same workspace is invisible to a fence (tests/memory_fence.py says both at length).

The size functions of include/difusco_hip.h and the fenced case that reaches each (all through ctypes):

  difusco_workspace_bytes                                 test_step_writes_only_its_outputs_and_workspace (and the two tests after it)
  difusco_prepared_bytes                                  test_prepared_step_... (``engine.prepare``)
  difusco_gen_table_bytes                                 test_gen_table_build_..., test_edge_embed_... (table), every general-input TSP step
  difusco_fused_scratch_bytes                             test_standalone_fused_layer_...
  difusco_graph_build_workspace_bytes                     test_graph_build_...
  difusco_knn_graph_workspace_bytes                       test_knn_graph_... (LDS and global-scratch path), test_knn_graph_of_mixed_sizes_...
  difusco_mcts_heatmap_workspace_bytes                    test_mcts_heatmap_...
  difusco_tsp_merge_workspace_bytes                       test_decode_entry_...[tsp_merge_tours]
  difusco_tsp_merge_batch_workspace_bytes                 [tsp_merge_batch_auto], [tsp_merge_batch_global]
  difusco_tsp_two_opt_workspace_bytes                     [two_opt_plain]
  difusco_tsp_two_opt_screened_workspace_bytes            [two_opt_screened]
  difusco_tsp_two_opt_grouped_workspace_bytes             [two_opt_grouped]
  difusco_tsp_two_opt_grouped_screened_workspace_bytes    [two_opt_grouped_screened]
  difusco_tsp_two_opt_ragged_workspace_bytes              [two_opt_ragged_exact], [two_opt_ragged_screened]
  difusco_tsp_two_opt_resident_workspace_bytes            [two_opt_resident]
  difusco_tsp_local_search_ragged_workspace_bytes         [local_search_ragged]
  difusco_tsp_local_search_resident_workspace_bytes       [local_search_resident]
  difusco_tsp_multi_two_opt_ragged_workspace_bytes        [multi_two_opt_ragged]
  difusco_tsp_nbr_two_opt_ragged_workspace_bytes          [nbr_two_opt_ragged]
  difusco_tsp_multi_local_search_ragged_workspace_bytes   [multi_local_search_ragged]
  difusco_tsp_nbr_local_search_ragged_workspace_bytes     [nbr_local_search_ragged]
  difusco_tsp_iterated_search_ragged_workspace_bytes      [iterated_search_ragged] (and the first call of [multi_local_search_ragged])
  difusco_tsp_focused_search_ragged_workspace_bytes       [focused_search_ragged]
  difusco_tsp_guided_search_ragged_workspace_bytes        [guided_search_ragged]
  difusco_tsp_kopt_search_ragged_workspace_bytes          [kopt_search_ragged]
  difusco_tsp_window_search_ragged_workspace_bytes        [window_search_ragged]
  difusco_mis_decode_workspace_bytes                      [mis_decode]
  difusco_mis_local_search_workspace_bytes                [mis_local_search]
  difusco_mis_iterated_search_workspace_bytes             [mis_iterated_search] (and [mis_resident_search], whose helper runs both)
  difusco_mis_resident_search_workspace_bytes             [mis_resident_search]

None is left out.  (``test_decode_entry_...`` asserts, per entry, that the size functions named in ``SIZE_FUNCTIONS`` were the ones
called.)"""
import ctypes
import os

import numpy as np
import pytest
import torch

import memory_fence as MF
import philox_reference as P
import test_gpu_workspace_contents as W
from difusco_amd import _lib
from oracle import difusco_oracle as O
from test_gpu_parity import CLASS_TOL
from test_gpu_workspace_contents import (DECODE, DIFFUSIONS, GRAPHS, STEP_ENGINES, _assert_within_the_oracle_bound, _graph_build_cases,
                                         _knn_brute_force, _step)

pytestmark = pytest.mark.gpu

GEN_ROWS = 71 * 256          # floats of the generated-input table proper; the buffer's tail is build / flag scratch (difusco_hip.h)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class _Inputs:
    """Snapshots of the ``const`` inputs of a call; ``check`` after it: every one is bit-identical."""

    def __init__(self):
        self.items = []

    def add(self, name, t):
        if t is not None and isinstance(t, torch.Tensor):
            assert t.is_contiguous(), name
            self.items.append((name, t, MF.snapshot(t)))
        return t

    def check(self, what):
        assert self.items, what
        changed = [name for name, t, snap in self.items if not MF.unchanged(t, snap)]
        assert not changed, f"{what}: inputs changed by the call: {changed}"


# =========================================== the fence sees a kernel's store =====================================================
def test_fence_reports_a_kernel_store_past_a_misdescribed_output(dev):
    """``difusco_categorical_posterior`` with n = 40 on an ``xt_out`` that was fenced as 32 floats: the same situation the family
    exists to catch - a buffer smaller than what the call was told.  Every byte written lies inside the test's own backing
    allocation (the tail guard has 256 KiB): nothing is out of bounds for the device.  The eight floats past the payload are bytes
    +0 .. +31.  The kernel stores 0.0 or 1.0 there (bytes 0x00, 0x80, 0x3f); the guard's first 32 bytes hold none of those three
    values (shown first), so every stored byte differs from what it replaces."""
    n, fenced = 40, 32
    fence = MF.Fence(dev, seed=1)
    out = fence.alloc((fenced,), torch.float32, name="xt_out")
    prob = fence.alloc((n,), torch.float32, name="prob_out")
    guard = fence.buffers[0].guards[1][:4 * (n - fenced)].cpu().numpy()
    assert not np.isin(guard, [0x00, 0x80, 0x3f]).any()
    fence.check("before the call")
    logits = torch.zeros(n, 2, device=dev)
    xt = torch.zeros(n, device=dev)
    post = np.array([0, 0, 1, 1, 1, 0, 0, 0], dtype=np.float32)          # prob = softmax(l)[1] = 1/2
    _lib.check(_lib.lib().difusco_categorical_posterior(_p(logits), _p(xt), _fp(post), _lib.RAND_PHILOX, None, 11, 0, _p(out), _p(prob),
                                                        n, _stream()))
    torch.cuda.synchronize()
    u = P.uniform(11, 0, n)
    assert (np.abs(u.astype(np.float64) - 0.5) > 1e-5).all()              # (no draw at the tie)
    assert (np.abs(prob.cpu().numpy().astype(np.float64) - 0.5) <= 1e-6).all()
    assert np.array_equal(out.cpu().numpy(), (u[:fenced] < 0.5).astype(np.float32))
    assert fence.changed_offsets(out) == ([], list(range(4 * (n - fenced))))
    assert fence.changed_offsets(prob) == ([], [])
    with pytest.raises(MF.FenceError) as exc:
        fence.check("posterior, n = 40 into 32 floats")
    text = str(exc.value)
    print(text)
    assert "xt_out (128 bytes): 32 guard bytes changed, first at +0, +1, +2, +3," in text and "prob_out" not in text
    tail = fence.buffers[0].backing[fence.lead + 4 * fenced:fence.lead + 4 * n].view(torch.float32).cpu().numpy()
    assert np.array_equal(tail, (u[fenced:] < 0.5).astype(np.float32))   # (and what landed there is the rest of the result)


# =========================================== the denoise step =====================================================================
def _fenced_step(monkeypatch, dev, engine, diffusion, graph, prepared_path=False, two_phase=False):
    """One step of the workspace-contents matrix with its memory fenced: the workspace (exactly ``difusco_workspace_bytes``),
    ``xt_out`` / ``pred`` / ``prob``, the generated-input table (exactly ``difusco_gen_table_bytes``) and, on request, the prepared
    buffer, the time-bias rows and ``gn_sums``.  Held to the oracle bound of its case; every input bit-identical afterwards."""
    from difusco_amd.engine import DenoiseEngine
    c = W._graph_case(graph)
    categorical = diffusion.startswith("categorical")
    eng = W._engine(engine, 2 if categorical else 1)
    what = f"{engine} {diffusion} {graph}" + (" prepared" if prepared_path else "") + (" two-phase" if two_phase else "")
    fence = MF.Fence(dev)
    made = MF.fence_allocations(monkeypatch, fence)
    inputs, seen = _Inputs(), {}
    step = DenoiseEngine.step

    def spy(self, g, task, diff, xt, t, post, **kw):
        inputs.add("x_t", xt)
        for k, tab in enumerate(kw.get("instances") or ()):
            inputs.add(("instance_rows", "instance_seeds")[k], tab)
        if two_phase:
            kw["gn_reduce"] = lambda sums: seen.setdefault("gn_sums", sums)
        seen["made_before"] = len(made)
        return step(self, g, task, diff, xt, t, post, **kw)
    monkeypatch.setattr(DenoiseEngine, "step", spy)
    g = c["g"]
    for name in ("rowptr", "col", "row", "perm", "seg_ptr", "node_order"):
        inputs.add(name, getattr(g, name))
    inputs.add("points", c["pts"])
    inputs.add("weights", eng.blob)
    eng._gen_table = None
    eng._tbias.clear()
    MF.fresh_engine_workspace(eng)
    try:
        eng.use_gen_table = diffusion != "gaussian-ddim-no-table"
        table = eng.gen_table() if (c["task"] == _lib.TASK_TSP and diffusion != "categorical") else None
        if table is not None:                                           # built under the patch, at exactly the declared bytes
            assert fence.buffer_of(table).nbytes == _lib.lib().difusco_gen_table_bytes(256) == 4 * table.numel()
            torch.cuda.synchronize()
            inputs.add("gen_table rows", table[:GEN_ROWS])
        prepared = None
        if prepared_path:
            eng.prepare_times([W.T])
            prepared = eng.prepare(g, c["pts"])
            torch.cuda.synchronize()
            assert prepared is not None and fence.buffer_of(prepared).nbytes == _lib.lib().difusco_prepared_bytes(256, g.n_nodes)
            tbias = eng._tbias[float(W.T)][0]
            assert fence.buffer_of(tbias).nbytes == 4 * eng.n_layers * 256
            inputs.add("prepared", prepared)
            inputs.add("time-bias rows", tbias)
            fence.check(what + ": prepare_times and prepare")
        got = _step(engine, diffusion, graph, prepared=prepared)
        torch.cuda.synchronize()
        need = _lib.lib().difusco_workspace_bytes(eng.hidden, eng.n_layers, g.n_nodes, g.n_edges, g.n_segments)
        (ws,) = eng._ws.values()
        assert ws.numel() == need > 0 and fence.buffer_of(ws).nbytes == need
        outs = [t for t in got if t is not None]
        assert len(outs) == (3 if categorical else 2) and all(fence.buffer_of(t) is not None for t in outs)
        in_step = made[seen["made_before"]:]
        if two_phase:
            sums = seen["gn_sums"]
            assert sums.dtype == torch.float64 and fence.buffer_of(sums).nbytes == 65 * 8 and any(t is sums for t in in_step)
        print(f"{what}: {len(fence.buffers)} fenced buffers, {fence.nbytes} bytes (workspace {need})")
        _assert_within_the_oracle_bound(engine, diffusion, graph, got)
        fence.check(what)
        inputs.check(what)
    finally:
        eng._gen_table = None
        eng._tbias.clear()
        MF.fresh_engine_workspace(eng)


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("diffusion", DIFFUSIONS)
@pytest.mark.parametrize("engine", list(STEP_ENGINES))
def test_step_writes_only_its_outputs_and_workspace(dev, monkeypatch, engine, diffusion, graph):
    _fenced_step(monkeypatch, dev, engine, diffusion, graph)


FUSED_ENGINES = [name for name, v in STEP_ENGINES.items() if v[2] and v[0] == 256]
TSP_GRAPHS = [name for name in GRAPHS if not name.startswith("mis")]
ONE_SEGMENT = ["tsp-37-k7", "tsp-11-k3", "mis-er60", "mis-no-edges"]


@pytest.mark.parametrize("graph", TSP_GRAPHS)
@pytest.mark.parametrize("diffusion", ["categorical", "gaussian-ddim"])
@pytest.mark.parametrize("engine", FUSED_ENGINES)
def test_prepared_step_writes_only_its_outputs_and_workspace(dev, monkeypatch, engine, diffusion, graph):
    """``prepare_times``, ``prepare``, then the step: the prepared buffer (exactly ``difusco_prepared_bytes``) and the time-bias rows
    are fenced when built and bit-identical after the step that reads them."""
    _fenced_step(monkeypatch, dev, engine, diffusion, graph, prepared_path=True)


@pytest.mark.parametrize("graph", ONE_SEGMENT)
@pytest.mark.parametrize("diffusion", ["categorical", "gaussian-ddim"])
@pytest.mark.parametrize("engine", list(STEP_ENGINES))
def test_two_phase_step_writes_only_its_outputs_workspace_and_sums(dev, monkeypatch, engine, diffusion, graph):
    """``gn_reduce=lambda t: None``: phase 1, nothing added, phase 2 - the statistics of this call, so the oracle bound of the
    one-phase step holds.  The 65 doubles of ``gn_sums`` are fenced."""
    _fenced_step(monkeypatch, dev, engine, diffusion, graph, two_phase=True)


# =========================================== decode, search and MIS entries =======================================================
# The uploads an entry may change: its documented in/out buffers (include/difusco_hip.h), named by the function of decode.py that
# uploads them and their dtype.  ``__init__:int32`` is ``_RaggedBatch.d_tours`` ("tours: DEVICE ... refined in place" at every
# ``_ragged`` / ``_resident`` entry; the class's other upload, the float64 points, is const), ``batched_two_opt_torch:int32`` /
# ``batched_two_opt_grouped:int32`` the ``int32_t* tours`` of difusco_tsp_two_opt(_screened) / _grouped(_screened),
# ``_mis_solution_on_device:int32`` the ``int32_t* solution`` of the three MIS searches.  The merges and the MIS decode take only
# const device inputs (the decode's solution is an output it allocates, not an upload).
_TOURS, _SOLUTION = {"__init__:int32"}, {"_mis_solution_on_device:int32"}
MAY_CHANGE = {
    "two_opt_plain": {"batched_two_opt_torch:int32"}, "two_opt_screened": {"batched_two_opt_torch:int32"},
    "two_opt_grouped": {"batched_two_opt_grouped:int32"}, "two_opt_grouped_screened": {"batched_two_opt_grouped:int32"},
    "two_opt_ragged_exact": _TOURS, "two_opt_ragged_screened": _TOURS, "two_opt_resident": _TOURS, "local_search_resident": _TOURS,
    "local_search_ragged": _TOURS, "multi_two_opt_ragged": _TOURS, "nbr_two_opt_ragged": _TOURS, "nbr_local_search_ragged": _TOURS,
    "multi_local_search_ragged": _TOURS, "iterated_search_ragged": _TOURS, "focused_search_ragged": _TOURS,
    "guided_search_ragged": _TOURS, "kopt_search_ragged": _TOURS, "window_search_ragged": _TOURS,
    "tsp_merge_tours": set(), "tsp_merge_batch_auto": set(), "tsp_merge_batch_global": set(), "mis_decode": set(),
    "mis_local_search": _SOLUTION, "mis_iterated_search": _SOLUTION, "mis_resident_search": _SOLUTION,
}
_W = "_workspace_bytes"
SIZE_FUNCTIONS = {
    "two_opt_plain": {"difusco_tsp_two_opt" + _W}, "two_opt_screened": {"difusco_tsp_two_opt_screened" + _W},
    "two_opt_grouped": {"difusco_tsp_two_opt_grouped" + _W}, "two_opt_grouped_screened": {"difusco_tsp_two_opt_grouped_screened" + _W},
    "two_opt_ragged_exact": {"difusco_tsp_two_opt_ragged" + _W}, "two_opt_ragged_screened": {"difusco_tsp_two_opt_ragged" + _W},
    "two_opt_resident": {"difusco_tsp_two_opt_resident" + _W}, "local_search_resident": {"difusco_tsp_local_search_resident" + _W},
    "local_search_ragged": {"difusco_tsp_local_search_ragged" + _W}, "multi_two_opt_ragged": {"difusco_tsp_multi_two_opt_ragged" + _W},
    "nbr_two_opt_ragged": {"difusco_tsp_nbr_two_opt_ragged" + _W}, "nbr_local_search_ragged": {"difusco_tsp_nbr_local_search_ragged" + _W},
    "multi_local_search_ragged": {"difusco_tsp_multi_local_search_ragged" + _W, "difusco_tsp_iterated_search_ragged" + _W},
    "iterated_search_ragged": {"difusco_tsp_iterated_search_ragged" + _W},
    "focused_search_ragged": {"difusco_tsp_focused_search_ragged" + _W}, "guided_search_ragged": {"difusco_tsp_guided_search_ragged" + _W},
    "kopt_search_ragged": {"difusco_tsp_kopt_search_ragged" + _W}, "window_search_ragged": {"difusco_tsp_window_search_ragged" + _W},
    "tsp_merge_tours": {"difusco_tsp_merge" + _W}, "tsp_merge_batch_auto": {"difusco_tsp_merge_batch" + _W},
    "tsp_merge_batch_global": {"difusco_tsp_merge_batch" + _W}, "mis_decode": {"difusco_mis_decode" + _W},
    "mis_local_search": {"difusco_mis_local_search" + _W}, "mis_iterated_search": {"difusco_mis_iterated_search" + _W},
    "mis_resident_search": {"difusco_mis_resident_search" + _W, "difusco_mis_iterated_search" + _W},
}


def test_the_tables_name_every_decode_entry():
    assert set(MAY_CHANGE) == set(DECODE) == set(SIZE_FUNCTIONS)


@pytest.mark.parametrize("entry", list(DECODE))
def test_decode_entry_writes_only_its_outputs_and_workspace(dev, monkeypatch, entry):
    """Every asserted case of the entry (the residue donor is not needed) under ``fence_allocations`` + ``fence_uploads``: each
    workspace is a fenced buffer of exactly the bytes its size function reported, no guard byte changes, and every upload that is
    not one of the entry's documented in/out buffers (``MAY_CHANGE``) is bit-identical to what was uploaded - as is every other
    device argument of the library call (``decode._ptr``) that is neither an allocation of the call nor such an in/out buffer."""
    from difusco_amd import decode
    fence = MF.Fence(dev)
    made = MF.fence_allocations(monkeypatch, fence)
    uploads = MF.fence_uploads(monkeypatch, fence)
    declared = []
    plain_workspace = decode._workspace

    def _workspace(size_fn, *sizes, device):
        before = len(made)
        ws, nbytes = plain_workspace(size_fn, *sizes, device=device)
        declared.append((size_fn.__name__, nbytes))
        assert ws.numel() == nbytes
        if nbytes > 0:                                                   # the call went through the patched torch.empty
            assert len(made) == before + 1 and made[-1] is ws and fence.buffer_of(ws).nbytes == nbytes
        return ws, nbytes
    monkeypatch.setattr(decode, "_workspace", _workspace)
    handed, plain_ptr = [], decode._ptr

    def _ptr(t):                                                         # every device pointer a wrapper hands to the library
        assert t.is_contiguous()
        handed.append((t, MF.snapshot(t)))
        return plain_ptr(t)
    monkeypatch.setattr(decode, "_ptr", _ptr)
    for k, run in enumerate(DECODE[entry][1]):
        n_buffers, n_made, n_uploads, n_declared, n_bytes = len(fence.buffers), len(made), len(uploads), len(declared), fence.nbytes
        n_handed = len(handed)
        calls = run(dev)
        calls = calls[0] if isinstance(calls, tuple) else calls
        torch.cuda.synchronize()
        what = f"{entry} case {k}"
        fence.check(what)
        sizes, ups = declared[n_declared:], uploads[n_uploads:]
        # how many buffers the case fenced: one workspace per library call (each of > 0 bytes: no case here is so small that its
        # entry asks for none), at least one upload per call (every wrapper uploads its scores, points or heat), nothing else unseen
        assert len(sizes) == calls and all(nbytes > 0 for _, nbytes in sizes), (what, sizes, calls)
        assert len(ups) >= calls, (what, len(ups), calls)
        assert len(fence.buffers) - n_buffers == len(ups) + (len(made) - n_made) >= len(ups) + calls, what
        changed = []
        for rec in ups:
            if not bool(torch.equal(MF._bytes_of(rec.tensor).cpu(), rec.host)):
                changed.append(rec.label)
        stray = [label for label in changed if label.split("#")[0] not in MAY_CHANGE[entry]]
        assert not stray, f"{what}: const uploads changed by the call: {stray}"
        # and whatever else the library was handed - neighbour lists, Philox tables, CSR arrays, concatenated heat, which do not
        # come through ``_dev`` -: all but the allocations (workspace, the decode's solution) and the in/out uploads are const
        const = 0
        for t, snap in handed[n_handed:]:
            rec = fence.buffer_of(t)
            if any(t is m for m in made) or (rec is not None and rec.label and rec.label.split("#")[0] in MAY_CHANGE[entry]):
                continue
            assert MF.unchanged(t, snap), f"{what}: a const argument ({t.dtype} {list(t.shape)}) was changed by the call"
            const += 1
        assert const >= calls, (what, const, calls)
        print(f"{what}: {len(fence.buffers) - n_buffers} fenced buffers ({len(ups)} uploads, {len(changed)} of them refined in place), "
              f"{const} const arguments, "
              f"{fence.nbytes - n_bytes} bytes, workspaces {sizes}")
    assert {name for name, _ in declared} == SIZE_FUNCTIONS[entry], declared


# =========================================== graph entries =======================================================================
def _knn_numpy(pts, k):
    """Neighbours [n, k] by (float64 squared distance as numpy evaluates it, index): for sizes below ``_knn_brute_force``'s reach."""
    dx, dy = pts[:, None, 0] - pts[None, :, 0], pts[:, None, 1] - pts[None, :, 1]
    return np.argsort(dx * dx + dy * dy, axis=1, kind="stable")[:, :k]


@pytest.mark.parametrize("n", [300, 16001])
def test_knn_graph_writes_only_its_edge_index_and_workspace(dev, monkeypatch, n):
    """``difusco_knn_graph``.  n = 300 keeps its keys in LDS: the 256 declared bytes stay untouched.  n = 16001 is past what fits
    LDS: the workspace is exactly 1024 x 16001 x 8 bytes (131 MB, as in test_gpu_workspace_contents.py) and is written."""
    from difusco_amd.graph import knn_edge_index_gpu
    k = 8
    pts, want = _knn_brute_force(n, k, n)
    fence = MF.Fence(dev)
    made = MF.fence_allocations(monkeypatch, fence)
    inputs = _Inputs()
    pts_d = inputs.add("points", fence.put(torch.from_numpy(pts), name="points"))
    ei = knn_edge_index_gpu(pts_d, k, device=dev)
    torch.cuda.synchronize()
    assert len(made) == 2 and made[0] is ei and ei.shape == (2, n * k)
    need = ctypes.c_size_t()
    _lib.check(_lib.lib().difusco_knn_graph_workspace_bytes(n, k, ctypes.byref(need)))
    assert fence.buffer_of(made[1]).nbytes == need.value == (256 if n == 300 else 1024 * 16001 * 8)
    if n == 300:
        assert fence.untouched(made[1])
    print(f"knn_graph n {n}: {len(fence.buffers)} fenced buffers, {fence.nbytes} bytes (workspace {need.value})")
    got = ei.cpu().numpy()
    assert np.array_equal(got[0], np.repeat(np.arange(n), k)) and np.array_equal(got[1].reshape(n, k), want)
    fence.check(f"knn_graph n {n}")
    inputs.check(f"knn_graph n {n}")


def test_knn_graph_of_mixed_sizes_writes_only_its_own_columns(dev, monkeypatch):
    """``sizes=[50, 8, 64]`` (n = k = 8 in the middle): one call per instance writes the ``ei[0, col:]`` / ``ei[1, col:]`` slices of
    ONE fenced ``edge_index``; every instance's columns equal its solo call, offset by its first node, and the numpy restatement."""
    from difusco_amd.graph import knn_edge_index_gpu
    k, sizes = 8, [50, 8, 64]
    pts = np.random.default_rng(508).random((sum(sizes), 2))
    fence = MF.Fence(dev)
    made = MF.fence_allocations(monkeypatch, fence)
    inputs = _Inputs()
    pts_d = inputs.add("points", fence.put(torch.from_numpy(pts), name="points"))
    ei = knn_edge_index_gpu(pts_d, k, device=dev, sizes=sizes)
    torch.cuda.synchronize()
    assert len(made) == 2 and made[0] is ei and ei.shape == (2, sum(sizes) * k) and fence.buffer_of(made[1]).nbytes == 256
    fence.check("knn_graph sizes, the union call")
    got = ei.cpu().numpy()
    node = col = 0
    for n in sizes:
        solo = knn_edge_index_gpu(fence.put(torch.from_numpy(pts[node:node + n])), k, device=dev).cpu().numpy()
        assert np.array_equal(solo[0], np.repeat(np.arange(n), k)) and np.array_equal(solo[1].reshape(n, k), _knn_numpy(pts[node:node + n], k))
        assert np.array_equal(got[:, col:col + n * k], solo + node)
        node, col = node + n, col + n * k
    print(f"knn_graph sizes {sizes}: {len(fence.buffers)} fenced buffers, {fence.nbytes} bytes")
    fence.check("knn_graph sizes")
    inputs.check("knn_graph sizes")


def test_graph_build_writes_only_its_arrays_and_workspace(dev, monkeypatch):
    """``difusco_graph_build`` through ``method="device"``: the union of three instances, a graph with points and one without
    (test_gpu_workspace_contents.py's cases, each equal to the host build in every field).  rowptr / col / row / perm, the node
    order and the workspace (exactly ``difusco_graph_build_workspace_bytes``) are fenced; ``edge_index`` and the points as the
    entry receives them are bit-identical afterwards."""
    from difusco_amd import graph
    fence = MF.Fence(dev)
    made = MF.fence_allocations(monkeypatch, fence)
    build, seen = graph._build_csr_device, []

    def spy(edge_index, n_nodes, device, points=None):
        inputs = _Inputs()
        for name, t in (("edge_index", edge_index), ("points", points)):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                inputs.add(name, t)
        before = len(made)
        g = build(edge_index, n_nodes, device, points)
        torch.cuda.synchronize()
        E = g.n_edges
        need = ctypes.c_size_t()
        with_points = points is not None and n_nodes > 1 and E > 0
        _lib.check(_lib.lib().difusco_graph_build_workspace_bytes(n_nodes, E, int(with_points), ctypes.byref(need)))
        new = made[before:]
        assert len(new) == (6 if with_points else 5) and fence.buffer_of(new[-1]).nbytes == need.value
        assert [t.numel() for t in new[:4]] == [n_nodes + 1, E, E, E]
        fence.check(f"graph_build n {n_nodes} E {E}")
        inputs.check(f"graph_build n {n_nodes} E {E}")
        seen.append((n_nodes, E, len(new), need.value))
        return g
    monkeypatch.setattr(graph, "_build_csr_device", spy)
    for run in _graph_build_cases(dev)[1]:
        run()
    assert len(seen) == 3
    for n, E, count, need in seen:
        print(f"graph_build n {n} E {E}: {count} fenced buffers, workspace {need} bytes")
    fence.check("graph_build")


def test_mcts_heatmap_writes_only_its_rows_and_workspace(dev, monkeypatch, golden_dir, tmp_path):
    """``difusco_mcts_heatmap_prepare`` + ``_rows`` on the smallest fixture, seven rows per call (the last block has two): the
    workspace (exactly ``difusco_mcts_heatmap_workspace_bytes``) and the [7, 30] row block are fenced; the text equals the
    reference converter's."""
    from difusco_amd import formats
    z = np.load(os.path.join(golden_dir, "mcts_text_n30.npz"))
    n, prob = int(z["num_nodes"]), float(z["expected_valid_prob"])
    ei = z["edge_index"] if "edge_index" in z.files else None
    E = ei.shape[1] if ei is not None else int((z["heat"] != 0).sum())
    fence = MF.Fence(dev)
    made = MF.fence_allocations(monkeypatch, fence)
    path = formats.write_mcts_heatmap(z["heat"], z["points"], n, str(tmp_path), 0, expected_valid_prob=prob, edge_index=ei,
                                      block_rows=7, use_gpu=True)
    torch.cuda.synchronize()
    assert open(path).read() == bytes(z["text"]).decode()
    ws = [t for t in made if t.dtype == torch.uint8]
    rows = [t for t in made if t.dtype == torch.float32 and tuple(t.shape) == (7, n)]
    assert len(ws) == 1 and len(rows) == 1, [(t.dtype, tuple(t.shape)) for t in made]
    if ei is not None:
        need = ctypes.c_size_t()
        _lib.check(_lib.lib().difusco_mcts_heatmap_workspace_bytes(n, E, ctypes.byref(need)))
        assert ws[0].numel() == need.value
    print(f"mcts_heatmap n {n}: {len(fence.buffers)} fenced buffers, {fence.nbytes} bytes (workspace {ws[0].numel()})")
    fence.check("mcts_heatmap")


# =========================================== direct C entries with caller-owned outputs ==========================================
@pytest.mark.parametrize("n", [1, 255, 257])
def test_posterior_kernels_write_n_values(dev, n):
    """``difusco_categorical_posterior`` / ``difusco_gaussian_posterior`` on Philox draws, against tests/philox_reference.py:
    the bits of ``u < prob`` (prob = softmax(l)[1] to 1e-6, test_gpu_parity.py's bound for it) and z within the derived bound of
    test_gpu_philox_exact.py."""
    from test_gpu_philox_exact import _logits_at, _normal_bound
    seed, offset = 11, (1 << 32) - 1
    fence, inputs = MF.Fence(dev), _Inputs()
    q = np.random.default_rng(n).random(n)
    logits = inputs.add("logits", fence.put(torch.from_numpy(_logits_at(q)), name="logits"))
    xt = inputs.add("xt", fence.put(torch.zeros(n), name="xt"))
    out, prob = fence.alloc((n,), torch.float32, name="xt_out"), fence.alloc((n,), torch.float32, name="prob_out")
    post = np.array([0, 0, 1, 1, 1, 0, 0, 0], dtype=np.float32)
    _lib.check(_lib.lib().difusco_categorical_posterior(_p(logits), _p(xt), _fp(post), _lib.RAND_PHILOX, None, seed, offset, _p(out),
                                                        _p(prob), n, _stream()))
    torch.cuda.synchronize()
    pr = prob.cpu().numpy()
    np.testing.assert_allclose(pr, q, rtol=0, atol=1e-6)
    assert np.array_equal(out.cpu().numpy(), (P.uniform(seed, offset, n) < np.clip(pr, 0.0, 1.0)).astype(np.float32))
    fence.check(f"categorical posterior n {n}")
    inputs.check(f"categorical posterior n {n}")

    fence, inputs = MF.Fence(dev), _Inputs()
    zero = inputs.add("pred and xt", fence.put(torch.zeros(n), name="pred and xt"))
    out = fence.alloc((n,), torch.float32, name="xt_out")
    post = np.array([1, 0, 0, 1, 1, 0, 0, 0], dtype=np.float32)          # x_s = 1 (0 - 0) + 1 z
    _lib.check(_lib.lib().difusco_gaussian_posterior(_p(zero), _p(zero), _fp(post), _lib.RAND_PHILOX, None, seed, offset, _p(out), n,
                                                     _stream()))
    torch.cuda.synchronize()
    z_ref = P.normal(seed, offset, n)
    assert (np.abs(out.cpu().numpy().astype(np.float64) - z_ref) <= _normal_bound(z_ref)).all()
    fence.check(f"gaussian posterior n {n}")
    inputs.check(f"gaussian posterior n {n}")
    print(f"posteriors n {n}: 3 fenced outputs, {12 * n} bytes")


@pytest.mark.parametrize("n_t", [1, 65])
def test_time_bias_rows_write_n_t_blocks(dev, n_t):
    """``difusco_time_bias_rows`` for 1 and 65 times (one launch per 64) against the oracle's time MLP, to the 2e-5 of
    test_gpu_round4.py."""
    H, Lyr = 256, 3
    p = W._params(H, 2)
    from difusco_amd import weights
    fence, inputs = MF.Fence(dev), _Inputs()
    blob = inputs.add("weights", fence.put(weights.pack_state_dict(p), name="weights"))
    ts = [float(t) for t in np.linspace(1, 1000, n_t).round()]
    out = fence.alloc((n_t, Lyr, H), torch.float32, name="rows")
    _lib.check(_lib.lib().difusco_time_bias_rows(H, Lyr, 2, _p(blob), (ctypes.c_float * n_t)(*ts), n_t, _p(out), _stream()))
    torch.cuda.synchronize()
    got = out.cpu()
    for i, t in enumerate(ts):
        te = O.time_features(p, torch.tensor([t]), H)
        for l in range(Lyr):
            err = (got[i, l] - O._layer_time_bias(p, l, te).reshape(-1)).abs().max().item()
            assert err < 2e-5, (t, l, err)
    print(f"time_bias_rows n_t {n_t}: 2 fenced buffers, {fence.nbytes} bytes")
    fence.check(f"time_bias_rows n_t {n_t}")
    inputs.check(f"time_bias_rows n_t {n_t}")


def _fenced_gen_table(fence, blob, H=256, Lyr=1, C=1):
    need = _lib.lib().difusco_gen_table_bytes(H)
    assert need >= 4 * GEN_ROWS and need % 4 == 0
    tab = fence.alloc((need // 4,), torch.float32, name="gen_table")
    _lib.check(_lib.lib().difusco_gen_table_build(H, Lyr, C, _p(blob), _p(tab), need, _stream()))
    torch.cuda.synchronize()
    return tab


def test_gen_table_build_stays_inside_its_declared_bytes(dev):
    """``difusco_gen_table_build`` into exactly ``difusco_gen_table_bytes(256)``; the 71 rows to the 2e-6 of test_gpu_round6.py."""
    from difusco_amd import weights
    p = O.init_params(256, 1, 1, seed=124)
    fence, inputs = MF.Fence(dev), _Inputs()
    blob = inputs.add("weights", fence.put(weights.pack_state_dict(p), name="weights"))
    tab = _fenced_gen_table(fence, blob)
    xs = -8.0 + (torch.arange(71, dtype=torch.float32) - 3.0) / 4.0
    want = O._lin(p, "edge_embed", O.scalar_embedding_sine(xs, 256))
    assert (tab[:GEN_ROWS].reshape(71, 256).cpu() - want).abs().max().item() < 2e-6
    print(f"gen_table_build: 2 fenced buffers, {fence.nbytes} bytes (table {4 * tab.numel()})")
    fence.check("gen_table_build")
    inputs.check("gen_table_build")


@pytest.mark.parametrize("path,bound", [("gemm", CLASS_TOL), ("table", 3e-6)])
@pytest.mark.parametrize("E", [33, 129])
def test_edge_embed_writes_its_rows_and_workgroup_maxima(dev, E, path, bound):
    """``difusco_edge_embed`` (fp16x3) as test_gpu_round6.py runs it, with ``e_tiled`` fenced at ``E_pad`` rows and ``tile_max`` at
    exactly ``ceil(E / 128) * 4`` floats - what the header documents as written ("one float per 32-edge tile", whole 128-edge
    workgroups).  With the table, its buffer is fenced at ``difusco_gen_table_bytes`` and its 71 rows stay bit-identical (the tile
    flags live in the buffer's tail)."""
    from difusco_amd import graph, weights
    H, Lyr, C = 256, 1, 1
    p = O.init_params(H, Lyr, C, seed=123)
    fence, inputs = MF.Fence(dev), _Inputs()
    blob = inputs.add("weights", fence.put(weights.pack_state_dict(p), name="weights"))
    tab = _fenced_gen_table(fence, blob) if path == "table" else None
    if tab is not None:
        inputs.add("gen_table rows", tab[:GEN_ROWS])
    g = torch.Generator().manual_seed(E)
    x_slot = torch.rand(E, generator=g) * 12.0 - 6.0
    x_slot[0], x_slot[-1] = 6.0, -6.0
    perm = torch.randperm(E, generator=g).to(torch.int32)
    x_caller = torch.empty(E)
    x_caller[perm.long()] = x_slot
    ref = O._lin(p, "edge_embed", O.scalar_embedding_sine(x_slot, H))
    E_pad = (E + 255) // 256 * 256
    n_tiles, n_wg_tiles = (E + 31) // 32, (E + 127) // 128 * 4
    xc, pm = inputs.add("xt", fence.put(x_caller, name="xt")), inputs.add("perm", fence.put(perm, name="perm"))
    e_t = fence.alloc((E_pad * H,), torch.float32, name="e_tiled")
    tmax = fence.alloc((n_wg_tiles,), torch.float32, name="tile_max")
    before = e_t.clone()
    _lib.check(_lib.lib().difusco_edge_embed(H, Lyr, C, _p(blob), _lib.PRECISIONS["fp16x3"], _p(xc), _p(pm), E, _p(e_t), _p(tmax),
                                             _p(tab), _stream()))
    torch.cuda.synchronize()
    got = graph.from_tiled(e_t, E).cpu()
    assert (got - ref).abs().max().item() < bound
    off = graph.edge_tiled_offsets(E_pad).to(dev)[E:].reshape(-1)
    assert torch.equal(e_t[off].view(torch.int32), before[off].view(torch.int32))      # rows past E: never written
    tm = tmax.cpu()
    for tl in range(n_tiles):
        assert tm[tl].item() == got[tl * 32:min(E, tl * 32 + 32)].abs().max().item()
    assert bool((tm[n_tiles:] == 0.0).all())
    print(f"edge_embed {path} E {E}: {len(fence.buffers)} fenced buffers, {fence.nbytes} bytes")
    fence.check(f"edge_embed {path} E {E}")
    inputs.check(f"edge_embed {path} E {E}")


@pytest.mark.parametrize("prec", ["fp16x3", "bf16x3"])
def test_standalone_fused_layer_writes_only_e_h_and_scratch(dev, prec):
    """``difusco_edge_layer_fused_ex`` on the zoo graph whose rows straddle tiles, every aggregation, time placement and gather
    kind: ``e`` (``E_pad`` tiled rows) and ``h`` are its documented in/out buffers, the scratch has exactly
    ``difusco_fused_scratch_bytes(n, E)`` bytes; all three are fenced, every other argument is bit-identical afterwards, and the
    results have the bits of test_gpu_graph_structure.py's run (which that file holds to float64)."""
    import graph_zoo as Z
    import test_gpu_graph_structure as S
    from difusco_amd import graph
    st = S._graph("straddle")
    n, E = len(st["deg"]), len(st["col"])
    x = S._dev_inputs(S._inputs("straddle", "random", 0), dev, True)
    csr = S._csr_dev(st, dev)
    nbytes = _lib.lib().difusco_fused_scratch_bytes(n, E)
    assert nbytes > 0 and x["e"].numel() == (E + 255) // 256 * 256 * 256
    for agg in Z.AGGS:
        for toe in (1, 0):
            for rg in ((0,) if agg == "max" else (0, 1)):
                want_e, want_h, _ = S._run_fused(_lib, dev, prec, S._inputs("straddle", "random", 0), csr, n, E, agg, toe, rg)
                fence, inputs = MF.Fence(dev), _Inputs()
                e_d, h_d = fence.put(x["e"], name="e"), fence.put(x["h"], name="h")
                scratch = fence.alloc_bytes(nbytes, name="scratch")
                rp, row, col = (inputs.add(k, t) for k, t in zip(("rowptr", "row", "col"), csr))
                for k in ("node4", "pc", "po", "bc", "bo", "tb", "sc"):
                    inputs.add(k, x[k])
                for k, t in enumerate(x["prm"]):
                    inputs.add(f"ln[{k}]", t)
                _lib.check(_lib.lib().difusco_edge_layer_fused_ex(
                    _lib.PRECISIONS[prec], n, E, _p(rp), _p(row), _p(col), _p(x["node4"]), _p(e_d), _p(h_d), _p(x["pc"]), _p(x["po"]),
                    _p(x["bc"]), *[_p(t) for t in x["prm"]], _p(x["bo"]), _p(x["tb"]), toe, _p(x["sc"]), _p(scratch), S.AGG_ID[agg], rg,
                    _stream()))
                torch.cuda.synchronize()
                what = f"fused layer {prec} {agg} toe={toe} reg_gather={rg}"
                full = graph.from_tiled(e_d, (E + 255) // 256 * 256).cpu()
                assert torch.equal(full[:E], want_e) and torch.equal(h_d.cpu(), want_h), what
                assert not bool(full[E:].any()), what + ": pad rows of e are not zero"
                fence.check(what)
                inputs.check(what)
    print(f"fused layer {prec} n {n} E {E}: 3 fenced buffers, {4 * (x['e'].numel() + x['h'].numel()) + nbytes} bytes (scratch {nbytes})")
