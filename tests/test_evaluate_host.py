"""CPU tests of the evaluation runner (``python -m difusco_amd.evaluate``): the split readers, checkpoint loading and the
configuration check, argument parsing of the reference's evaluation commands, chunking and sharding, the pinned per-instance
seeds and the metrics.  Every input is written into tmp_path."""
import argparse
import os
import pickle

import numpy as np
import pytest
import torch

from difusco_amd import evaluate as E
from difusco_amd.checkpoint import CheckpointError, check_config, load_checkpoint
from difusco_amd.datasets import SplitFormatError, read_mis_split, read_tsp_split
from difusco_amd.synthetic import random_state_dict


# ---- TSP reader ------------------------------------------------------------------------------------------------------------
def test_tsp_reader_tokens_are_float_and_tours_zero_based(tmp_path):
    lines = ["0.1 0.2 0.30000000000000004 1e-3 0.5 0.7 output 1 3 2 1",
             "  0.25 0.75 1 0.999999999999999999 output 2 1 2  ",
             "0.6241 0.1234 0.5 0.5 0.3333333333333333 0.7 0.1 0.9 output 4 2 3 1 4"]
    path = tmp_path / "tsp.txt"
    path.write_text("\n".join(lines) + "\n")
    out = read_tsp_split(str(path))
    assert len(out) == 3 and [ex.points.shape[0] for ex in out] == [3, 2, 4]
    for i, (ex, line) in enumerate(zip(out, lines)):
        toks = line.strip().split(" output ")[0].split(" ")
        want = np.array([float(t) for t in toks], dtype=np.float64).reshape(-1, 2)
        assert ex.points.dtype == np.float64 and ex.points.tobytes() == want.tobytes()      # bit-identical
        assert ex.tour.dtype == np.int64 and ex.source == (str(path), i + 1)
    assert out[0].tour.tolist() == [0, 2, 1, 0] and out[1].tour.tolist() == [1, 0, 1] and out[2].tour.tolist() == [3, 1, 2, 0, 3]
    assert len(read_tsp_split(str(path), limit=2)) == 2


@pytest.mark.parametrize("bad", ["0.1 0.2 0.3 output 1 1", "0.1 0.2 0.3 0.4", "0.1 0.2 0.3 0.4 output 1 2",
                                 "0.1 x 0.3 0.4 output 1 2 1", "0.1 0.2 0.3 0.4 output 1 3 1", ""])
def test_tsp_reader_names_the_malformed_line(tmp_path, bad):
    path = tmp_path / "bad.txt"
    path.write_text("0.1 0.2 0.3 0.4 output 1 2 1\n" + bad + "\n0.5 0.5 0.6 0.6 output 2 1 2\n")
    with pytest.raises(SplitFormatError, match=f"{path}:2"):
        read_tsp_split(str(path))


# ---- MIS reader ------------------------------------------------------------------------------------------------------------
def _graph(n, edges, labels=None):
    nx = pytest.importorskip("networkx")
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    if labels is not None:
        nx.set_node_attributes(g, {i: int(v) for i, v in enumerate(labels)}, "label")
    return g


def _dump(g, path):
    with open(path, "wb") as f:
        pickle.dump(g, f)


def _reference_layout(g):
    """mis_dataset.py:43-48 restated: the edges, their reversed copy, the self loops, transposed."""
    e = np.array(g.edges, dtype=np.int64)
    e = np.concatenate([e, e[:, ::-1]], axis=0)
    loops = np.arange(g.number_of_nodes()).reshape(-1, 1).repeat(2, axis=1)
    return np.concatenate([e, loops], axis=0).T


def test_mis_reader_edge_layout_labels_and_glob_order(tmp_path):
    import glob
    g0 = _graph(5, [(0, 1), (1, 2), (0, 4), (3, 4)], labels=[1, 0, 1, 1, 0])
    g1 = _graph(4, [(2, 3), (0, 3)])                                              # no label attribute: zeros
    g1.nodes[0]["other"] = 7
    _dump(g0, tmp_path / "a.gpickle")
    _dump(g1, tmp_path / "b.gpickle")
    pattern = str(tmp_path / "*gpickle")
    out = read_mis_split(pattern)
    assert [ex.source[0] for ex in out] == glob.glob(pattern)
    by_name = {os.path.basename(ex.source[0]): ex for ex in out}
    for name, g in (("a.gpickle", g0), ("b.gpickle", g1)):
        ex = by_name[name]
        assert ex.n_nodes == g.number_of_nodes()
        assert ex.edge_index.dtype == np.int64 and np.array_equal(ex.edge_index, _reference_layout(g))
        assert ex.edge_index.shape == (2, 2 * g.number_of_edges() + g.number_of_nodes())
    assert by_name["a.gpickle"].labels.tolist() == [1, 0, 1, 1, 0] and by_name["a.gpickle"].labels.dtype == np.int64
    assert by_name["b.gpickle"].labels.tolist() == [0, 0, 0, 0]
    # labels from <name>_unweighted.result
    (tmp_path / "labels").mkdir()
    (tmp_path / "labels" / "a_unweighted.result").write_text("0\n1\n0\n0\n1\n")
    (tmp_path / "labels" / "b_unweighted.result").write_text("1\n1\n0\n0\n")
    out = {os.path.basename(ex.source[0]): ex for ex in read_mis_split(pattern, label_dir=str(tmp_path / "labels"))}
    assert out["a.gpickle"].labels.tolist() == [0, 1, 0, 0, 1] and out["b.gpickle"].labels.tolist() == [1, 1, 0, 0]


class _Evil:
    def __reduce__(self):
        return (os.getcwd, ())


def test_mis_reader_refuses_disallowed_globals(tmp_path):
    g = _graph(3, [(0, 1)])
    g.graph["payload"] = _Evil()
    _dump(g, tmp_path / "evil.gpickle")
    with pytest.raises(SplitFormatError, match=r"getcwd.*not allowed"):
        read_mis_split(str(tmp_path / "evil.gpickle"))


# ---- checkpoints ----------------------------------------------------------------------------------------------------------
def _lightning(sd, **extra):
    return {"epoch": 3, "global_step": 120, "pytorch-lightning_version": "1.7.7",
            "state_dict": {"model." + k: v for k, v in sd.items()},
            "optimizer_states": [{"state": {}, "param_groups": [{"lr": 2e-4, "weight_decay": 1e-4, "params": [0, 1]}]}],
            "lr_schedulers": [{"last_epoch": 120}], "callbacks": {}, **extra}


def test_load_checkpoint_lightning_and_bare(tmp_path):
    sd = random_state_dict(64, 2, 2, seed=3)
    torch.save(_lightning(sd), tmp_path / "last.ckpt")
    torch.save(sd, tmp_path / "bare.pt")
    for name in ("last.ckpt", "bare.pt"):
        got = load_checkpoint(str(tmp_path / name))
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert check_config(got, 64, 2, "categorical") == (64, 2, 2)


def test_checkpoint_config_mismatch_names_both_values(tmp_path):
    sd = random_state_dict(64, 2, 2, seed=3)
    with pytest.raises(CheckpointError) as exc:
        check_config(sd, 256, 12, "gaussian")
    msg = str(exc.value)
    assert "hidden size 64" in msg and "--hidden_dim 256" in msg
    assert "2 layers" in msg and "--n_layers 12" in msg
    assert "2 output channels" in msg and "gaussian needs 1" in msg
    with pytest.raises(CheckpointError, match="--hidden_dim 128"):
        check_config(sd, 128, 2, "categorical")


def test_checkpoint_that_needs_unpickling_is_refused(tmp_path):
    sd = random_state_dict(64, 2, 1, seed=4)
    torch.save(_lightning(sd, hyper_parameters={"param_args": argparse.Namespace(task="tsp")}), tmp_path / "hp.ckpt")
    with pytest.raises(CheckpointError, match=r"argparse\.Namespace.*--unsafe_checkpoint_load"):
        load_checkpoint(str(tmp_path / "hp.ckpt"))
    got = load_checkpoint(str(tmp_path / "hp.ckpt"), allow_unsafe=True)
    assert all(torch.equal(got[k], sd[k]) for k in sd)


# ---- arguments -------------------------------------------------------------------------------------------------------------
# reproducing_scripts.md, "Evaluation": the five commands' flags as written there
REFERENCE_COMMANDS = [
    ["--task", "tsp", "--wandb_logger_name", "tsp_diffusion_graph_categorical_tsp100_test", "--diffusion_type", "categorical",
     "--do_test", "--learning_rate", "0.0002", "--weight_decay", "0.0001", "--lr_scheduler", "cosine-decay",
     "--storage_path", "/your/storage/path", "--training_split", "/your/tsp100_train_concorde.txt",
     "--validation_split", "/your/tsp100_valid_concorde.txt", "--test_split", "/your/tsp100_test_concorde.txt",
     "--batch_size", "32", "--num_epochs", "25", "--inference_schedule", "cosine", "--inference_diffusion_steps", "50",
     "--ckpt_path", "/your/tsp100_categorical/ckpt_path/last.ckpt", "--resume_weight_only"],
    ["--task", "tsp", "--wandb_logger_name", "tsp_diffusion_graph_gaussian_tsp500_test_parallel4", "--diffusion_type",
     "categorical", "--do_test", "--learning_rate", "0.0002", "--weight_decay", "0.0001", "--lr_scheduler", "cosine-decay",
     "--storage_path", "/your/storage/path", "--training_split", "/your/tsp500_train_concorde.txt",
     "--validation_split", "/your/tsp500_valid_concorde.txt", "--test_split", "/your/tsp500_test_concorde.txt",
     "--sparse_factor", "50", "--batch_size", "32", "--num_epochs", "25", "--validation_examples", "8",
     "--inference_schedule", "cosine", "--inference_diffusion_steps", "50", "--parallel_sampling", "4",
     "--ckpt_path", "/your/tsp500_categorical/ckpt_path/last.ckpt", "--resume_weight_only"],
    ["--task", "tsp", "--wandb_logger_name", "tsp_diffusion_graph_gaussian_tsp10k_test_sequential4", "--diffusion_type",
     "categorical", "--do_test", "--learning_rate", "0.0002", "--weight_decay", "0.0001", "--lr_scheduler", "cosine-decay",
     "--storage_path", "/your/storage/path", "--training_split", "/your/tsp10000_train_concorde.txt",
     "--validation_split", "/your/tsp10000_valid_concorde.txt", "--test_split", "/your/tsp10000_test_concorde.txt",
     "--sparse_factor", "100", "--batch_size", "1", "--num_epochs", "25", "--validation_examples", "8",
     "--inference_schedule", "cosine", "--inference_diffusion_steps", "50", "--sequential_sampling", "4",
     "--two_opt_iterations", "5000", "--ckpt_path", "/your/tsp10k_categorical/ckpt_path/last.ckpt", "--resume_weight_only"],
    ["--task", "mis", "--wandb_logger_name", "mis_diffusion_graph_categorical_sat_test", "--diffusion_type", "categorical",
     "--do_test", "--learning_rate", "0.0002", "--weight_decay", "0.0001", "--lr_scheduler", "cosine-decay",
     "--storage_path", "/your/storage/path", "--training_split", "/your/train_mis_sat/*gpickle",
     "--validation_split", "/your/test_mis_sat/*gpickle", "--test_split", "/your/test_mis_sat/*gpickle",
     "--batch_size", "16", "--num_epochs", "50", "--validation_examples", "8", "--inference_schedule", "cosine",
     "--inference_diffusion_steps", "50", "--ckpt_path", "/your/mis_sat_categorical/ckpt_path/last.ckpt", "--resume_weight_only"],
    ["--task", "mis", "--wandb_logger_name", "mis_diffusion_graph_gaussian_er_test", "--diffusion_type", "gaussian",
     "--do_test", "--learning_rate", "0.0002", "--weight_decay", "0.0001", "--lr_scheduler", "cosine-decay",
     "--storage_path", "/your/storage/path", "--training_split", "/your/data_er/train/*gpickle",
     "--training_split_label_dir", "/your/data_er/train_annotations/",
     "--validation_split", "/your/data_er/train/validation/*gpickle", "--test_split", "/your/data_er/train/test/*gpickle",
     "--batch_size", "4", "--num_epochs", "50", "--validation_examples", "8", "--inference_schedule", "cosine",
     "--inference_diffusion_steps", "50", "--parallel_sampling", "4", "--use_activation_checkpoint",
     "--ckpt_path", "/your/mis_er_gaussian/ckpt_path/last.ckpt", "--resume_weight_only"],
]


@pytest.mark.parametrize("i", range(5))
def test_reference_evaluation_commands_parse(i):
    args, ignored = E.parse_args(REFERENCE_COMMANDS[i])
    assert args.do_test and not args.do_train and args.inference_diffusion_steps == 50 and args.inference_schedule == "cosine"
    assert {"learning_rate", "weight_decay", "lr_scheduler", "training_split", "batch_size", "num_epochs",
            "wandb_logger_name", "resume_weight_only"} <= set(ignored) <= set(E.TRAINING_ONLY)
    assert args.seed == 0 and args.instances_per_call is None and args.records is None
    if i == 1:
        assert args.sparse_factor == 50 and args.parallel_sampling == 4 and args.validation_examples == 8
    if i == 2:
        assert args.sequential_sampling == 4 and args.two_opt_iterations == 5000
    if i == 4:
        assert args.diffusion_type == "gaussian" and {"training_split_label_dir", "use_activation_checkpoint"} <= set(ignored)


def test_reference_defaults_are_kept():
    args, ignored = E.parse_args(["--task", "tsp", "--storage_path", ".", "--do_test", "--ckpt_path", "x.ckpt"])
    assert ignored == [] and args.diffusion_type == "gaussian" and args.inference_diffusion_steps == 1000
    assert args.validation_examples == 64 and args.sparse_factor == -1 and args.hidden_dim == 256 and args.n_layers == 12
    assert args.test_split == "data/tsp/tsp50_test_concorde.txt" and args.two_opt_iterations == 1000 and not args.fp16


@pytest.mark.parametrize("mode", [["--do_train"], ["--do_train", "--do_test"], []])
def test_training_or_no_mode_exits_with_status_2(mode, capsys):
    with pytest.raises(SystemExit) as exc:
        E.main(["--task", "tsp", "--storage_path", ".", "--ckpt_path", "x.ckpt"] + mode)
    assert exc.value.code == 2
    assert ("training is out of scope" if mode else "nothing to do") in capsys.readouterr().err


def test_numpy_heatmap_with_several_samples_is_refused_first(tmp_path):
    argv = ["--task", "tsp", "--storage_path", str(tmp_path), "--do_test", "--ckpt_path", str(tmp_path / "missing.ckpt"),
            "--save_numpy_heatmap"]
    for extra in (["--parallel_sampling", "2"], ["--sequential_sampling", "2"]):
        with pytest.raises(NotImplementedError, match="single sampling"):
            E.run(argv + extra)


# ---- chunks, shards, seeds -------------------------------------------------------------------------------------------------
def test_default_chunk_length_rule():
    assert E.default_instances_per_call(E.tsp_rows(50, -1, 1)) == 64
    assert E.default_instances_per_call(E.tsp_rows(50, -1, 4)) == 26
    assert E.default_instances_per_call(E.tsp_rows(500, 50, 1)) == 10
    assert E.default_instances_per_call(E.tsp_rows(500, 50, 4)) == 2
    assert E.default_instances_per_call(E.tsp_rows(1000, 100, 1)) == 2
    assert E.default_instances_per_call(E.tsp_rows(1000, 100, 4)) == 1
    assert E.default_instances_per_call(E.tsp_rows(10000, 100, 1)) == 1
    assert E.default_instances_per_call(E.mis_rows(85000, 1)) == 3


def test_chunks_are_pure_never_mix_n_and_shard_whole():
    sizes = [50] * 7 + [60] * 3 + [50] * 2 + [100] * 5
    length = lambda n: {50: 3, 60: 5, 100: 2}[n]
    chunks = E.plan_chunks(sizes, length)
    assert chunks == E.plan_chunks(list(sizes), length)
    assert chunks == [(0, 3), (3, 6), (6, 7), (7, 10), (10, 12), (12, 14), (14, 16), (16, 17)]
    for lo, hi in chunks:
        assert len(set(sizes[lo:hi])) == 1 and hi - lo <= length(sizes[lo])
    assert [i for lo, hi in chunks for i in range(lo, hi)] == list(range(len(sizes)))
    for world in (1, 2, 3, 5, 11):
        shards = [E.shard_chunks(chunks, r, world) for r in range(world)]
        assert [c for s in shards for c in s] == chunks             # whole chunks, contiguous, in order
    # MIS: graphs of any size share a chunk
    assert E.plan_chunks([10, 20, 30, 40], lambda e: 3, equal_size=False) == [(0, 3), (3, 4)]


def test_split_chunks_follow_the_arguments():
    ex = [type("X", (), {"points": np.zeros((n, 2))})() for n in [50] * 70 + [40]]
    assert E.split_chunks("tsp", ex, -1, 1) == [(0, 64), (64, 70), (70, 71)]
    assert E.split_chunks("tsp", ex, -1, 1, instances_per_call=30) == [(0, 30), (30, 60), (60, 70), (70, 71)]
    with pytest.raises(ValueError, match="instances_per_call"):
        E.split_chunks("tsp", ex, -1, 1, instances_per_call=0)


def test_instance_seeds_are_pinned():
    assert E.instance_seed(0, "test", 0) == 8319404288669743651
    assert E.instance_seed(0, "test", 1) == 1343195265560397746
    assert E.instance_seed(0, "val", 0) == 1944610627291712254
    assert E.instance_seed(1234, "test", 7) == 4694615965415208788
    g1, g2 = E.instance_generator(E.instance_seed(0, "test", 0)), E.instance_generator(E.instance_seed(0, "test", 0))
    assert torch.equal(torch.randn(8, generator=g1), torch.randn(8, generator=g2))


# ---- per-instance values and metrics ---------------------------------------------------------------------------------------
def test_gt_cost_matches_tsp_evaluator():
    rng = np.random.default_rng(8)
    for n in (5, 37, 200):
        pts = rng.random((n, 2))
        tour = np.concatenate([rng.permutation(n), [0]])
        tour[-1] = tour[0]
        p32 = pts.astype(np.float32).astype(np.float64)                         # the reference's np_points
        dist = np.sqrt(((p32[:, None, :] - p32[None, :, :]) ** 2).sum(-1))      # TSPEvaluator: distance matrix, then a sum
        ref = 0.0
        for i in range(len(tour) - 1):
            ref += dist[tour[i], tour[i + 1]]
        assert abs(E.tsp_gt_cost(pts, tour) - ref) <= 1e-12 * ref


def test_metrics_are_the_means_of_the_records():
    rng = np.random.default_rng(2)
    recs = [{"gt_cost": float(g), "solved_cost": float(g * (1 + 0.1 * rng.random())), "2opt_iterations": int(rng.integers(100)),
             "merge_iterations": float(rng.random() * 50)} for g in rng.random(9) + 5]
    m = E.split_metrics("tsp", "test", recs)
    for k in ("gt_cost", "solved_cost", "2opt_iterations", "merge_iterations"):
        assert m[f"test/{k}"] == float(np.mean([r[k] for r in recs]))
    assert m["test/gap_pct"] == pytest.approx(np.mean([100 * (r["solved_cost"] - r["gt_cost"]) / r["gt_cost"] for r in recs]))
    mis = [{"gt_cost": 10.0, "solved_cost": 9.0}, {"gt_cost": 0.0, "solved_cost": 4.0}, {"gt_cost": 20.0, "solved_cost": 19.0}]
    m = E.split_metrics("mis", "val", mis)
    assert set(m) == {"val/gt_cost", "val/solved_cost", "val/gap_pct"}
    assert m["val/gt_cost"] == 10.0 and m["val/solved_cost"] == pytest.approx(32 / 3) and m["val/gap_pct"] == pytest.approx(7.5)
    assert E.split_metrics("mis", "val", mis[1:2])["val/gap_pct"] is None
