"""The evaluation runner on the GPU (``python -m difusco_amd.evaluate``): end to end on small splits written in the reference's
formats.  With one instance per call every record is bitwise what a solo ``solve_tsp`` / ``solve_mis`` call on a fresh model
returns for that instance's seed and generator; with chunks of several instances the records repeat, do not depend on what
the model ran before (``step_offset``) nor on the number of ranks; heatmap dumps equal a solo ``sample()``."""
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from difusco_amd import evaluate as E
from difusco_amd.synthetic import er_mis_edge_index, random_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _write_tsp(path, sizes, seed):
    rng = np.random.default_rng(seed)
    lines = []
    for n in sizes:
        pts = rng.random((n, 2))
        perm = rng.permutation(n)
        tour = np.concatenate([perm, perm[:1]]) + 1
        lines.append(" ".join(str(float(v)) for v in pts.reshape(-1)) + " output " + " ".join(str(int(t)) for t in tour))
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _write_mis(folder, sizes, seed):
    nx = pytest.importorskip("networkx")
    folder.mkdir()
    rng = np.random.default_rng(seed)
    for i, n in enumerate(sizes):
        ei = er_mis_edge_index(n, 0.1, seed=seed + i)
        und = ei[:, : (ei.shape[1] - n) // 2]
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from(und.T.tolist())
        if i % 2 == 0:
            nx.set_node_attributes(g, {v: int(rng.integers(2)) for v in range(n)}, "label")
        with open(folder / f"g{i:02d}.gpickle", "wb") as f:
            pickle.dump(g, f)
    return str(folder / "*gpickle")


def _ckpt(path, hidden, layers, diffusion="categorical", seed=0):
    sd = random_state_dict(hidden, layers, 2 if diffusion == "categorical" else 1, seed=seed)
    torch.save({"epoch": 0, "global_step": 0, "state_dict": {"model." + k: v for k, v in sd.items()},
                "optimizer_states": [], "lr_schedulers": []}, path)
    return str(path), sd


def _argv(tmp_path, task, split, ckpt, hidden, layers, *extra, diffusion="categorical"):
    return ["--task", task, "--do_test", "--diffusion_type", diffusion, "--storage_path", str(tmp_path),
            "--validation_split", split, "--test_split", split, "--validation_examples", "2", "--inference_schedule", "cosine",
            "--inference_diffusion_steps", str(STEPS), "--ckpt_path", ckpt, "--hidden_dim", str(hidden), "--n_layers",
            str(layers)] + list(extra)


def _model_args(**kw):
    return dict(dict(diffusion_type="categorical", inference_schedule="cosine", inference_diffusion_steps=STEPS), **kw)


def _check_lines(lines, recs, task, n_test):
    assert [l["split"] for l in lines] == ["val", "test"]
    assert lines[0]["instances"] == 2 and lines[1]["instances"] == n_test
    for line in lines:
        mine = [r for r in recs if r["split"] == line["split"]]
        assert [r["index"] for r in mine] == list(range(line["instances"]))
        for k, v in E.split_metrics(task, line["split"], mine).items():
            assert line[k] == v
        stages = {"parse", "knn", "sampling", "merge", "two_opt"} if task == "tsp" else {"parse", "sampling", "decode"}
        assert set(line["stages_s"]) == stages and line["world_size"] == 1 and line["precision"] == "fp16x3"


# ---- bitwise equal to solo calls --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_tsp_records_equal_solo_solve_tsp(dev, tmp_path, mode):
    from difusco_amd import TSPModel
    from difusco_amd.datasets import read_tsp_split
    from difusco_amd.pipeline import solve_tsp
    sizes, K, P, S = ([60, 60, 48, 60], 10, 2, 2) if mode == "sparse" else ([50] * 4, -1, 2, 1)
    split = _write_tsp(tmp_path / "tsp.txt", sizes, seed=1)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 256, 3)
    lines, recs = E.run(_argv(tmp_path, "tsp", split, ckpt, 256, 3, "--sparse_factor", str(K), "--parallel_sampling", str(P),
                              "--sequential_sampling", str(S), "--two_opt_iterations", "100", "--instances_per_call", "1"))
    _check_lines(lines, recs, "tsp", len(sizes))
    examples = read_tsp_split(split)
    for r in recs:
        ex = examples[r["index"]]
        assert r["seed"] == E.instance_seed(0, r["split"], r["index"]) and r["n_nodes"] == sizes[r["index"]]
        m = TSPModel(_model_args(sparse_factor=K, hidden_dim=256, n_layers=3), sd, device=dev, seed=r["seed"])
        tour, cost, costs, info = solve_tsp(m, ex.points, K, parallel_sampling=P, two_opt_iterations=100,
                                            generator=torch.Generator().manual_seed(r["seed"]), sequential_sampling=S)
        assert r["tour"] == tour and r["solved_cost"] == cost and r["all_costs"] == costs, r["index"]
        assert r["merged_costs"] == info["merged_costs"] and r["2opt_iterations"] == info["two_opt_iterations"]
        assert r["merge_iterations"] == info["merge_iterations"] and r["gt_cost"] == E.tsp_gt_cost(ex.points, ex.tour)


def test_mis_records_equal_solo_solve_mis(dev, tmp_path):
    from difusco_amd import MISModel
    from difusco_amd.datasets import read_mis_split
    from difusco_amd.pipeline import solve_mis
    pattern = _write_mis(tmp_path / "mis", [40, 75, 60, 90, 52], seed=3)
    ckpt, sd = _ckpt(tmp_path / "mis.ckpt", 64, 2)
    P, S = 2, 2
    lines, recs = E.run(_argv(tmp_path, "mis", pattern, ckpt, 64, 2, "--parallel_sampling", str(P), "--sequential_sampling",
                              str(S), "--instances_per_call", "1"))
    _check_lines(lines, recs, "mis", 5)
    examples = read_mis_split(pattern)
    for r in recs:
        ex = examples[r["index"]]
        assert r["gt_cost"] == float(ex.labels.sum()) and r["source"] == list(ex.source)
        m = MISModel(_model_args(hidden_dim=64, n_layers=2), sd, device=dev, seed=r["seed"])
        sol, size, sizes = solve_mis(m, ex.n_nodes, ex.edge_index, parallel_sampling=P, sequential_sampling=S,
                                     generator=torch.Generator().manual_seed(r["seed"]))
        assert r["mis"] == np.nonzero(sol)[0].tolist() and r["solved_cost"] == size and r["all_costs"] == sizes, r["index"]


# ---- chunks of several instances ----------------------------------------------------------------------------------------
def test_chunked_records_repeat_and_ignore_model_history(dev, tmp_path):
    from difusco_amd import TSPModel
    from difusco_amd.datasets import read_tsp_split
    split = _write_tsp(tmp_path / "tsp.txt", [60] * 5 + [45] * 2, seed=2)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 256, 3)
    argv = _argv(tmp_path, "tsp", split, ckpt, 256, 3, "--sparse_factor", "10", "--parallel_sampling", "2",
                 "--two_opt_iterations", "100", "--instances_per_call", "3")
    lines_a, a = E.run(argv)
    _, b = E.run(argv)
    assert a == b and lines_a[1]["chunk_lengths"] == [2, 3] and lines_a[1]["chunks"] == 3      # (0,3) (3,5) (5,7): N never mixed
    # a model that has already run other steps gives what the runner's fresh model gave
    m = TSPModel(_model_args(sparse_factor=10, hidden_dim=256, n_layers=3, parallel_sampling=2), sd, device=dev, seed=5)
    ex = read_tsp_split(split)
    m.sample(torch.from_numpy(ex[0].points).float().to(dev).reshape(1, 60, 2), None)      # dense call: other shapes too
    assert m.model.calls == STEPS
    chunks = E.split_chunks("tsp", ex, 10, 2, instances_per_call=3)
    recs = E.solve_split(m, "tsp", ex, "test", chunks, seed=0, sparse_factor=10, parallel_sampling=2, two_opt_iterations=100)
    assert recs == [r for r in a if r["split"] == "test"]


def test_solve_batch_step_offset_equals_engine_counter(dev):
    from difusco_amd import MISModel, TSPModel
    from difusco_amd.pipeline import solve_mis_batch, solve_tsp_batch
    sd = random_state_dict(64, 2, 2, seed=1)
    pts = np.random.default_rng(4).random((3, 40, 2))
    mis = [(n, er_mis_edge_index(n, 0.1, seed=n)) for n in (50, 70)]
    res = []
    for use_offset in (False, True):
        mt = TSPModel(_model_args(sparse_factor=8, hidden_dim=64, n_layers=2), sd, device=dev, seed=3)
        mm = MISModel(_model_args(hidden_dim=64, n_layers=2), sd, device=dev, seed=3)
        kw = dict(seeds=[7, 8, 9], sequential_sampling=2, parallel_sampling=2, two_opt_iterations=50)
        solve_tsp_batch(mt, pts, 8, **kw)                                        # history: the counter is not 0
        solve_mis_batch(mm, mis, seeds=[1, 2])
        gens = lambda k: [torch.Generator().manual_seed(i) for i in range(k)]
        off_t = mt.model.calls if use_offset else None
        off_m = mm.model.calls if use_offset else None
        assert mt.model.calls == 2 * STEPS and mm.model.calls == STEPS
        res.append((solve_tsp_batch(mt, pts, 8, generators=gens(3), step_offset=off_t, **kw),
                    solve_mis_batch(mm, mis, seeds=[1, 2], generators=gens(2), sequential_sampling=2, step_offset=off_m)))
    (t0, m0), (t1, m1) = res
    assert t0 == t1
    assert all(np.array_equal(x[0], y[0]) and x[1:] == y[1:] for x, y in zip(m0, m1))


# ---- several ranks ----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_ranks_on_one_gpu_give_the_one_process_records(dev, tmp_path):
    split = _write_tsp(tmp_path / "tsp.txt", [50] * 5, seed=6)
    ckpt, _ = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--sparse_factor", "8", "--two_opt_iterations", "100",
                 "--instances_per_call", "2", "--device", "cuda:0")
    E.run(argv + ["--records", str(tmp_path / "one.jsonl")])
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "--module", "difusco_amd.evaluate"]
                         + argv + ["--dist_backend", "gloo", "--records", str(tmp_path / "two.jsonl")],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    assert [l["split"] for l in lines] == ["val", "test"] and all(l["world_size"] == 2 for l in lines)
    one = (tmp_path / "one.jsonl").read_text().splitlines()
    two = (tmp_path / "two.jsonl").read_text().splitlines()
    assert len(one) == 7 and [json.loads(l) for l in one] == [json.loads(l) for l in two]


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_gaussian_split_and_fp16(dev, tmp_path):
    split = _write_tsp(tmp_path / "tsp.txt", [60, 60, 60], seed=7)
    ckpt, _ = _ckpt(tmp_path / "g.ckpt", 256, 3, diffusion="gaussian")
    lines, recs = E.run(_argv(tmp_path, "tsp", split, ckpt, 256, 3, "--sparse_factor", "10", "--two_opt_iterations", "100",
                              diffusion="gaussian"))
    assert [l["instances"] for l in lines] == [2, 3] and lines[0]["precision"] == "fp16x3"
    assert all(np.isfinite(l["test/solved_cost"]) and l["test/solved_cost"] > 0 for l in lines[1:])
    assert all(sorted(r["tour"][:-1]) == list(range(60)) for r in recs)
    ckpt, _ = _ckpt(tmp_path / "c.ckpt", 256, 3)
    lines, _ = E.run(_argv(tmp_path, "tsp", split, ckpt, 256, 3, "--sparse_factor", "10", "--two_opt_iterations", "100",
                           "--fp16", "--do_valid_only"))
    assert [l["split"] for l in lines] == ["val"] and lines[0]["precision"] == "fp16x1"


@pytest.mark.parametrize("K", [8, -1])
def test_save_numpy_heatmap_equals_solo_sample(dev, tmp_path, K):
    from difusco_amd import TSPModel
    from difusco_amd.datasets import read_tsp_split
    from difusco_amd.graph import knn_edge_index_gpu
    split = _write_tsp(tmp_path / "tsp.txt", [50, 50, 50], seed=9)
    ckpt, sd = _ckpt(tmp_path / "last.ckpt", 64, 2)
    argv = _argv(tmp_path, "tsp", split, ckpt, 64, 2, "--sparse_factor", str(K), "--save_numpy_heatmap", "--instances_per_call",
                 "1", "--heatmap_dir", str(tmp_path / "out"))
    _, recs = E.run(argv)
    for r in recs:
        ex = read_tsp_split(split)[r["index"]]
        heat = np.load(tmp_path / "out" / "numpy_heatmap" / f"{r['split']}-heatmap-{r['index']}.npy")
        pts = np.load(tmp_path / "out" / "numpy_heatmap" / f"{r['split']}-points-{r['index']}.npy")
        assert pts.dtype == np.float32 and np.array_equal(pts, ex.points.astype(np.float32))
        m = TSPModel(_model_args(sparse_factor=K, hidden_dim=64, n_layers=2), sd, device=dev, seed=r["seed"])
        p32 = torch.from_numpy(pts).to(dev)
        gen = torch.Generator().manual_seed(r["seed"])
        if K > 0:
            solo = m.sample(p32, knn_edge_index_gpu(ex.points, K, device=dev), generator=gen)
        else:
            solo = m.sample(p32.reshape(1, 50, 2), None, generator=gen)
        assert heat.dtype == np.float32 and np.array_equal(heat, solo.cpu().numpy())
    with pytest.raises(NotImplementedError, match="single sampling"):
        E.run(argv + ["--parallel_sampling", "2"])
