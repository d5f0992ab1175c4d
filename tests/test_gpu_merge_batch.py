"""The batched merge (``difusco_tsp_merge_batch`` / ``decode.merge_tours_batch``) on a real GPU: every (graph, sample) of a
call must get exactly what the per-graph entry (``decode.merge_tours``) and the CPU oracle give it - tour, iteration count and
completion flag - in both regimes, with the path state in LDS and in the workspace, for ties, dense heatmaps, the reference's
fixtures, and through ``solve_tsp_batch`` / ``evaluate``."""
import ctypes

import numpy as np
import pytest
import torch

from difusco_amd import _lib
from difusco_amd import evaluate as E
from oracle import difusco_oracle as O
from oracle import tsp_decode_oracle as D
from test_decode_oracle import DENSE, GOLDEN, check_against_fixture

pytestmark = pytest.mark.gpu

STATES = ["auto", "global"]
KINDS = ("bits", "prob", "gauss")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _heat(kind, pts, ei, rng):                                   # the heat kinds of tests/test_gpu_decode.py
    d = np.linalg.norm(pts[ei[0]] - pts[ei[1]], axis=1)
    if kind == "bits":
        return ((rng.random(ei.shape[1]) < np.exp(-d / (0.6 * d.mean()))).astype(np.float32) + np.float32(1e-6))
    if kind == "prob":
        return (np.exp(-d / (0.5 * d.mean())) * rng.random(ei.shape[1])).astype(np.float32) + np.float32(1e-6)
    return (rng.standard_normal(ei.shape[1]).astype(np.float32) * np.float32(0.25) + np.float32(0.75))


def _instance(n, k, shuffle):
    """(points, edge_index, heat [3, E]): one sample of every kind, drawn in the order bits, prob, gauss."""
    from difusco_amd.synthetic import tsp_instance
    rng = np.random.default_rng(n * 1000 + k)
    pts, ei = tsp_instance(n, k, seed=n)
    heat = np.stack([_heat(kind, pts, ei, rng) for kind in KINDS])
    if shuffle:
        perm = rng.permutation(ei.shape[1])
        ei, heat = ei[:, perm], heat[:, perm]
    return pts, ei, heat


def _raw(dev, graphs, state="auto"):
    """difusco_tsp_merge_batch through ctypes.  graphs: (points [n, 2], edge_index [2, E] or None for dense, heat [P, E]) per
    graph.  Returns per graph (tours [P][n + 1], iterations [P], completed [P]) - the per-sample values."""
    L = _lib.lib()
    dense = graphs[0][1] is None
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=t)
    gn = np.array([g[0].shape[0] for g in graphs], dtype=np.int32)
    gp = np.array([np.asarray(g[2]).shape[0] for g in graphs], dtype=np.int32)
    ge = np.array([np.asarray(g[2]).reshape(p, -1).shape[1] for g, p in zip(graphs, gp)], dtype=np.int64)
    heat = d(np.concatenate([np.asarray(g[2], dtype=np.float32).reshape(-1) for g in graphs]), torch.float32)
    pts = d(np.concatenate([np.asarray(g[0], dtype=np.float32).reshape(-1) for g in graphs]), torch.float32)
    if dense:
        row_p = col_p = None
    else:
        row = d(np.concatenate([g[1][0] for g in graphs]), torch.int32)
        col = d(np.concatenate([g[1][1] for g in graphs]), torch.int32)
        row_p, col_p = ctypes.c_void_p(row.data_ptr()), ctypes.c_void_p(col.data_ptr())
    nbytes = ctypes.c_size_t()
    _lib.check(L.difusco_tsp_merge_batch_workspace_bytes(len(graphs), gn.ctypes.data, ge.ctypes.data, gp.ctypes.data,
                                                         ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    S = int(gp.sum())
    tours = np.full(int(((gn.astype(np.int64) + 1) * gp).sum()), -1, dtype=np.int32)
    iters, done = np.full(S, -1, dtype=np.int64), np.full(S, -1, dtype=np.int32)
    _lib.check(L.difusco_tsp_merge_batch(len(graphs), gn.ctypes.data, ge.ctypes.data, gp.ctypes.data, row_p, col_p,
                                         ctypes.c_void_p(heat.data_ptr()), ctypes.c_void_p(pts.data_ptr()),
                                         1 if state == "global" else 0, ctypes.c_void_p(ws.data_ptr()), nbytes.value,
                                         tours.ctypes.data, iters.ctypes.data, done.ctypes.data, None))
    out, t0, s0 = [], 0, 0
    for n, p in zip(gn.tolist(), gp.tolist()):
        out.append((tours[t0:t0 + p * (n + 1)].reshape(p, n + 1).tolist(), iters[s0:s0 + p].tolist(),
                    [bool(v) for v in done[s0:s0 + p]]))
        t0, s0 = t0 + p * (n + 1), s0 + p
    return out


def _existing(dev, pts, ei, heat):
    """The per-graph entry, sample by sample: (tours, iterations, completed) with per-sample iteration counts."""
    from difusco_amd.decode import merge_tours
    tours, its, done = [], [], []
    for h in np.asarray(heat):
        t, it, ok = merge_tours(h, pts, ei, sparse_graph=ei is not None, device=dev, return_completed=True)
        tours += t
        its.append(int(it))
        done += ok
    return tours, its, done


def _oracle(pts, ei, heat):
    tours, its, done = [], [], []
    for h in np.asarray(heat):
        t, it, ok = D.merge_tours(h, pts, ei, sparse_graph=ei is not None, parallel_sampling=1)
        tours += t
        its.append(it)
        done += ok
    return tours, its, done


def _check_equal(got, graphs, dev, oracle_iterations=True):
    """got (from _raw) against the existing entry and the CPU oracle, graph by graph: tours and flags always, iteration counts
    against the existing entry always and against the oracle where the sample completed."""
    for (tours, its, done), (pts, ei, heat) in zip(got, graphs):
        e_tours, e_its, e_done = _existing(dev, pts, ei, heat)
        o_tours, o_its, o_done = _oracle(pts, ei, heat)
        assert done == e_done == o_done
        assert tours == e_tours == o_tours
        assert its == e_its
        print("merge_iterations: batched", its, "existing", e_its, "oracle", o_its)
        for s, ok in enumerate(done):
            if ok and oracle_iterations:
                assert its[s] == o_its[s]


# ---- 1. one call over graphs of both regimes --------------------------------------------------------------------------------
BOTH = [(4, 3), (17, 16), (33, 8), (64, 63), (65, 12), (129, 20)]


def test_batch_with_both_regimes(dev):
    from difusco_amd.decode import merge_tours_batch
    graphs = [_instance(n, k, shuffle=bool(g % 2)) for g, (n, k) in enumerate(BOTH)]
    got = _raw(dev, graphs, "auto")
    _check_equal(got, graphs, dev)
    flags = {nk: done for nk, (_, _, done) in zip(BOTH, got)}
    print("completed per graph (bits, prob, gauss):", flags)
    assert all(flags[(4, 3)]) and all(flags[(17, 16)]) and all(flags[(64, 63)])      # checked on the CPU oracle
    assert flags[(33, 8)] == [False, False, True]
    assert not any(flags[(65, 12)]) and not any(flags[(129, 20)])
    every = [ok for done in flags.values() for ok in done]
    assert any(every) and not all(every)
    assert _raw(dev, graphs, "global") == got
    for state in STATES:                                          # the Python entry: per instance what merge_tours returns
        res = merge_tours_batch([g[2] for g in graphs], [g[0] for g in graphs], [g[1] for g in graphs], sparse_graph=True,
                                parallel_sampling=3, device=dev, return_completed=True, state=state)
        assert res == [(t, float(np.mean(i)), d) for t, i, d in got]
    short = merge_tours_batch([g[2] for g in graphs], [g[0] for g in graphs], [g[1] for g in graphs], sparse_graph=True,
                              parallel_sampling=3, device=dev)
    assert short == [(t, float(np.mean(i))) for t, i, _ in got]


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------
def _grid_instance(g, k):
    from difusco_amd.synthetic import knn_edge_index
    xs = np.arange(g) / g
    pts = np.stack(np.meshgrid(xs, xs, indexing="ij"), -1).reshape(-1, 2)
    ei = knn_edge_index(pts, k)
    pts = pts.astype(np.float32)                                 # as synthetic.tsp_instance: every entry sees float32 coordinates
    return pts, ei, np.full((1, ei.shape[1]), np.float32(1) + np.float32(1e-6), dtype=np.float32)


def test_ties_keep_flat_index_order(dev):
    """Grid points with constant heat: few distinct scores over many candidate pairs (on the float32 coordinates 6 x 6, K = 35:
    112 distinct scores over 628 pairs; 8 x 8, K = 12: 9 over 408; 10 x 10, K = 99: 590 over 4948).  The tour depends on the
    order inside every run of equal scores; it must be the flat-index order of the per-graph entry and of the oracle: tours and
    flags equal both.  merge_iterations equals the per-graph entry's.  It is not held against the oracle here: inside a run of
    equal scores the dense list does not keep (i, j) and (j, i) adjacent, so the oracle's count of entries differs from the
    per-graph entry's two-per-pair count (8 x 8: 283 against 285, 10 x 10: 8979 against 8981, 6 x 6: 581 both), and the batched
    entry reproduces the per-graph entry's count exactly, as it must."""
    graphs = [_grid_instance(6, 35), _grid_instance(8, 12), _grid_instance(10, 99)]
    assert [g[0].shape[0] for g in graphs] == [36, 64, 100] and [g[1].shape[1] for g in graphs] == [1260, 768, 9900]
    for state in STATES:
        got = _raw(dev, graphs, state)
        _check_equal(got, graphs, dev, oracle_iterations=False)
        assert all(done == [True] for _, _, done in got)


# ---- 3. dense ---------------------------------------------------------------------------------------------------------------
def test_dense_graphs_without_index_arrays(dev):
    from difusco_amd.decode import merge_tours, merge_tours_batch
    assert len(DENSE) >= 3
    zs = [np.load(p) for p in DENSE]
    heats = [z["heat"] for z in zs]
    points = [z["points"] for z in zs]
    par = [int(z["parallel_sampling"]) for z in zs]
    for n in (20, 50):
        rng = np.random.default_rng(n)
        pts = rng.random((n, 2))
        d = np.linalg.norm(pts[:, None] - pts[None], axis=-1)
        heats.append((np.exp(-d / (0.3 * d.mean())) * rng.random((2, n, n))).astype(np.float32) + np.float32(1e-6))
        points.append(pts)
        par.append(2)
    for state in STATES:
        res = merge_tours_batch(heats, points, None, sparse_graph=False, parallel_sampling=par, device=dev,
                                return_completed=True, state=state)
        for g, (tours, it, done) in enumerate(res):
            ref = merge_tours(heats[g], points[g], None, sparse_graph=False, parallel_sampling=par[g], device=dev,
                              return_completed=True)
            assert (tours, it, done) == ref, g
            if g < len(zs):
                assert all(done) and np.array_equal(np.asarray(tours), zs[g]["tours"]) and it == float(zs[g]["merge_iterations"])
    raw = _raw(dev, [(p, None, np.asarray(h).reshape(q, -1)) for p, h, q in zip(points, heats, par)])
    assert [r[0] for r in raw] == [r[0] for r in res]


# ---- 4. the reference's sparse fixtures, all in one call ---------------------------------------------------------------------
def test_sparse_reference_fixtures_in_one_call(dev):
    assert len(GOLDEN) >= 6
    zs = [np.load(p) for p in GOLDEN]
    graphs = [(z["points"], z["edge_index"], z["heat"].reshape(int(z["parallel_sampling"]), -1)) for z in zs]
    for state in STATES:
        got = _raw(dev, graphs, state)
        for z, (tours, its, done) in zip(zs, got):
            check_against_fixture(z, tours, its, done)
    done_all = [ok for _, _, done in got for ok in done]
    assert any(done_all) and not all(done_all)


# ---- 5. structure of a call ------------------------------------------------------------------------------------------------
def test_single_graph_single_sample_equals_merge_tour(dev):
    L = _lib.lib()
    pts, ei, heat = _instance(129, 20, shuffle=True)
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=t)
    row, col, p32 = d(ei[0], torch.int32), d(ei[1], torch.int32), d(pts, torch.float32)
    nbytes = ctypes.c_size_t()
    _lib.check(L.difusco_tsp_merge_workspace_bytes(ei.shape[1], ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    for s in range(3):
        h = d(heat[s], torch.float32)
        tour = np.empty(pts.shape[0] + 1, dtype=np.int32)
        it, ok = ctypes.c_int64(), ctypes.c_int32()
        _lib.check(L.difusco_tsp_merge_tour(pts.shape[0], ei.shape[1], row.data_ptr(), col.data_ptr(), ctypes.c_void_p(h.data_ptr()),
                                            ctypes.c_void_p(p32.data_ptr()), ws.data_ptr(), nbytes.value,
                                            tour.ctypes.data_as(ctypes.c_void_p), ctypes.byref(it), ctypes.byref(ok), None))
        for state in STATES:
            assert _raw(dev, [(pts, ei, heat[s:s + 1])], state) == [([tour.tolist()], [it.value], [bool(ok.value)])]


def test_duplicate_edges_and_self_loops(dev):
    """One directed edge listed three times (its heat values add up in list order) and explicit self loops with positive heat
    (counted by merge_iterations, never inserted): the per-graph entry's results."""
    graphs = []
    for n, k in [(17, 16), (33, 8)]:
        pts, ei, heat = _instance(n, k, shuffle=False)
        rng = np.random.default_rng(n)
        e = int(rng.integers(ei.shape[1]))
        loops = np.array([[2, 5, 2], [2, 5, 2]])
        ei = np.concatenate([ei, ei[:, [e, e]], loops], axis=1)
        extra = (rng.random((3, 5)) * np.float32(0.7)).astype(np.float32) + np.float32(0.1)
        heat = np.concatenate([heat, extra], axis=1)
        perm = rng.permutation(ei.shape[1])
        graphs.append((pts, ei[:, perm], heat[:, perm]))
    for state in STATES:
        got = _raw(dev, graphs, state)
        for (tours, its, done), (pts, ei, heat) in zip(got, graphs):
            assert (tours, its, done) == _existing(dev, pts, ei, heat)


def test_permuting_the_graphs_permutes_the_results_and_calls_repeat_bitwise(dev):
    graphs = [_instance(n, k, shuffle=bool(g % 2)) for g, (n, k) in enumerate(BOTH)]
    got = _raw(dev, graphs)
    assert _raw(dev, graphs) == got
    order = [3, 0, 5, 1, 4, 2]
    assert _raw(dev, [graphs[g] for g in order]) == [got[g] for g in order]
    # different numbers of samples per graph in one call
    ragged = [(p, e, h[:1 + g % 3]) for g, (p, e, h) in enumerate(graphs)]
    assert _raw(dev, ragged) == [(t[:1 + g % 3], i[:1 + g % 3], d[:1 + g % 3]) for g, (t, i, d) in enumerate(got)]


def test_state_moves_to_the_workspace_above_the_lds_budget(dev):
    """12 bytes of path state per node: n = 13653 is the last size whose state fits the 160 KiB LDS budget, n = 13654 the first
    that keeps it in the workspace.  Both in one call (with a small graph), two samples each: `prob` heat on the k-NN edges
    (the positive scores run out: the host finishes it from the saved state) and a sample that completes on the device - unit
    heat on the edges of a random Hamiltonian path appended to the list, 1e-6 on the k-NN edges.  Against the per-graph entry;
    the forced-workspace call gives the same."""
    from difusco_amd.graph import knn_edge_index_gpu
    graphs = []
    for n in (13653, 13654, 40):
        rng = np.random.default_rng(n)
        pts = rng.random((n, 2)).astype(np.float32)
        knn = knn_edge_index_gpu(pts.astype(np.float64), 8, device=dev).cpu().numpy()
        perm = rng.permutation(n)
        ei = np.concatenate([knn, np.stack([perm[:-1], perm[1:]])], axis=1)
        path = np.concatenate([np.full(knn.shape[1], 1e-6), np.ones(n - 1)]).astype(np.float32)
        graphs.append((pts, ei, np.stack([_heat("prob", pts, ei, rng), path])))
    got = _raw(dev, graphs, "auto")
    assert got[0][2] == got[1][2] == [False, True] and got[2][2][1]      # both regimes on either side of the budget
    for (tours, its, done), (pts, ei, heat) in zip(got, graphs):
        assert (tours, its, done) == _existing(dev, pts, ei, heat)
    assert _raw(dev, graphs, "global") == got


# ---- 6. the pipeline ---------------------------------------------------------------------------------------------------------
def _model(dev, seed, sparse_factor):
    from difusco_amd import TSPModel
    from difusco_amd.engine import DenoiseEngine
    args = dict(diffusion_type="categorical", diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=2, hidden_dim=64, inference_trick="ddim", inference_diffusion_steps=5, inference_schedule="cosine")
    return TSPModel(args, engine=DenoiseEngine(O.init_params(64, 2, 2, seed=0), device=dev), seed=seed)


@pytest.mark.parametrize("K,sizes", [(-1, [12, 20, 31, 12, 20, 31]), (10, [60, 90, 60, 90, 60, 90]), (-1, [20] * 6), (10, [60] * 6)],
                         ids=["dense-list", "sparse-list", "dense-array", "sparse-array"])
def test_solve_tsp_batch_batched_merge_equals_loop(dev, K, sizes):
    from difusco_amd.pipeline import solve_tsp_batch
    rng = np.random.default_rng(61)
    pts = [rng.random((n, 2)) for n in sizes]
    form = np.stack(pts) if len(set(sizes)) == 1 else pts
    runs = []
    for kw in ({}, {"merge_method": "loop"}, {"merge_method": "batched"}):
        timings = {}
        runs.append(solve_tsp_batch(_model(dev, 3, K), form, K, parallel_sampling=2, sequential_sampling=2, two_opt_iterations=100,
                                    seeds=list(range(40, 46)), generators=[torch.Generator().manual_seed(b) for b in range(6)],
                                    timings=timings, step_offset=0, **kw))
        assert set(timings) >= {"knn", "sampling", "merge", "two_opt"}
    assert runs[0] == runs[1] == runs[2]
    assert all(len(r[3]["merged_costs"]) == 4 for r in runs[2])


def _write_split(path, sizes, seed):
    rng = np.random.default_rng(seed)
    lines = []
    for n in sizes:
        pts, perm = rng.random((n, 2)), rng.permutation(n)
        tour = np.concatenate([perm, perm[:1]]) + 1
        lines.append(" ".join(str(float(v)) for v in pts.reshape(-1)) + " output " + " ".join(str(int(t)) for t in tour))
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_evaluate_with_batched_merge_gives_the_same_records(dev, tmp_path):
    from difusco_amd.synthetic import random_state_dict
    split = _write_split(tmp_path / "tsp.txt", [20, 30] * 4, seed=4)
    ckpt = str(tmp_path / "last.ckpt")
    torch.save({"epoch": 0, "global_step": 0, "optimizer_states": [], "lr_schedulers": [],
                "state_dict": {"model." + k: v for k, v in random_state_dict(64, 2, 2, seed=0).items()}}, ckpt)
    argv = ["--task", "tsp", "--do_test", "--do_valid_only", "--diffusion_type", "categorical", "--storage_path", str(tmp_path),
            "--validation_split", split, "--test_split", split, "--validation_examples", "8", "--inference_schedule", "cosine",
            "--inference_diffusion_steps", "5", "--ckpt_path", ckpt, "--hidden_dim", "64", "--n_layers", "2", "--sparse_factor", "8",
            "--parallel_sampling", "2", "--two_opt_iterations", "100", "--mixed_size_chunks"]
    _, recs_loop = E.run(argv)
    _, recs_batched = E.run(argv + ["--merge_method", "batched"])
    assert len(recs_loop) == 8 and recs_batched == recs_loop
