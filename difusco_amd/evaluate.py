"""Evaluate a checkpoint on the reference's test splits without Lightning - the flow of ``difusco/train.py --do_test``
(``train.py:135-138``) on the GPU stages of this package:

    python -m difusco_amd.evaluate --task tsp --diffusion_type categorical --do_test --storage_path DIR \\
        --validation_split tsp500_valid.txt --test_split tsp500_test.txt --sparse_factor 50 --validation_examples 8 \\
        --inference_schedule cosine --inference_diffusion_steps 50 --parallel_sampling 4 --ckpt_path last.ckpt

Every argument of ``train.py:19-68`` is accepted with its name and default, so the reference's evaluation commands run with
only the program name changed; training-only arguments are ignored and listed as ``ignored_args``.  ``--do_test`` validates on
the first ``--validation_examples`` instances of ``validation_split`` (split "val", ``pl_meta_model.py:200-205``), then tests
on all of ``test_split`` (split "test") unless ``--do_valid_only``; data paths are ``os.path.join(storage_path, split)``.
Every instance goes through ``pipeline.solve_tsp_batch`` / ``solve_mis_batch`` - k-NN, the sampling loop, merge, 2-opt / MIS
decode on the GPU; the runner does nothing per denoise step.

Per instance it records what ``test_step`` logs (``pl_tsp_model.py:240-256``, ``pl_mis_model.py:194-209``); per split it
prints one JSON line with the mean of every reference key over the split's instances (``pl_meta_model.py:49-60``) and
``{split}/gap_pct``, which is not a reference key.  ``--fp16`` selects ``precision="fp16x1"``.

Determinism: instance i of split s draws its Philox stream and its x_T from ``instance_seed(--seed, s, i)``,
every chunk starts its steps at offset 0, and the chunks (``plan_chunks``) are cut from the split alone - the records do not
depend on the world size, the rank an instance lands on, or what the model ran before.

Extensions: ``--seed``, ``--instances_per_call`` (chunk length; default ``default_instances_per_call``),
``--two_opt_method {exact,screened}`` (``decode.batched_two_opt_grouped``: same records either way), ``--two_opt_mode
{launches,resident}`` (TSP with ``--local_search 2opt``: ``resident`` runs that 2-opt with one GPU block per instance,
``mode="resident"`` of ``decode.batched_two_opt_grouped``; the records and the header gain ``two_opt_mode`` and are otherwise
the same), ``--tsp_local_search_mode {launches,resident}`` (TSP with ``--local_search 2opt+oropt``: ``resident`` runs that
search with one GPU block per instance, ``mode="resident"`` of ``decode.batched_local_search_grouped``; the records and the header
gain ``tsp_local_search_mode`` and are otherwise the same), ``--local_search
{2opt,2opt+oropt,multi2opt,multi2opt+oropt,nbr2opt+oropt}`` (``2opt+oropt``, ``decode.batched_local_search_grouped``: Or-opt moves after 2-opt, never a longer tour; the records gain
``or_opt_iterations`` and ``local_search_rounds``, the header ``local_search``; ``multi2opt``,
``decode.batched_multi_two_opt_grouped``: every sweep applies all disjoint improving 2-opt moves it selects, ``2opt_iterations``
counts sweeps and the records gain ``two_opt_moves``; ``multi2opt+oropt``, ``decode.batched_multi_local_search_grouped``: rounds
of multi-move 2-opt and multi-move Or-opt sweeps, ``2opt_iterations`` and ``or_opt_iterations`` count sweeps and the records gain
``two_opt_moves``, ``or_opt_moves`` and ``local_search_rounds``), ``--mis_local_search {none,swap}`` (MIS:
``decode.mis_local_search_np`` after every decode, never a smaller set; the records gain ``decoded_costs``, the greedy sizes in
the order of ``all_costs``, the header ``mis_local_search``; refused with ``--task tsp``), ``--mis_local_search_kicks N`` /
``--mis_local_search_kick_size K`` (N > 0 only with ``--mis_local_search swap``: the search iterated with N seeded kicks,
``decode.mis_iterated_search_np``, keyed by the instance seed; the records gain ``swap_costs``, ``kicks_entered``,
``kicks_accepted`` and the two settings, the header the two settings), ``--mis_local_search_mode {launches,resident}``
(resident only with ``--task mis --mis_local_search swap``, any N >= 0: the search runs one GPU block per instance,
``decode.mis_iterated_search_np(mode="resident")``; the records and the header gain ``mis_local_search_mode`` and are otherwise
those of ``launches``), ``--tsp_local_search_kicks N`` /
``--tsp_local_search_kick_size K`` / ``--tsp_local_search_kick_span S`` (N > 0 only with ``--local_search multi2opt+oropt``: that
search iterated with N seeded segment kicks, ``decode.batched_iterated_search_grouped``, every tour keyed by its instance seed;
the records gain ``kicks_improved``, one count per copy in the order of the last round, and the three settings, the header
the three settings), ``--tsp_local_search_descent {full,focused}`` (focused only with ``--tsp_local_search_kicks N`` > 0: the
descents after the kicks evaluate only the candidates next to a touched edge and one full descent closes the search,
``descent="focused"`` of ``decode.batched_iterated_search_grouped``, keyed as the kicks are; only when it is ``focused`` the
records gain the setting and ``closing_sweeps``, one count per copy, and the header the setting),
``--tsp_local_search_kick_bias {uniform,heat}`` (heat only with ``--tsp_local_search_kicks N`` > 0 and ``--task tsp``: the first cut
of every draw of a kick falls on a tour edge with a probability that rises as the heat of that edge falls,
``kick_bias="heat"`` of ``decode.batched_iterated_search_grouped`` on each sample's own heatmap; only when it is ``heat`` the
records and the header gain the setting), ``--tsp_local_search_window W`` / ``--tsp_local_search_passes R`` (W > 0 only with
``--local_search multi2opt+oropt``, a full descent and uniform kicks: the windowed iterated search,
``decode.batched_window_search_grouped``, R passes over windows of W positions with ``--tsp_local_search_kicks`` kicks (>= 0) per
window and pass, keyed as the kicks are; the records gain ``kicks_improved``, ``passes_kept`` and ``closing_sweeps``, one count per
copy, and with the header the two settings and the three kick settings), ``--tsp_local_search_candidates K`` /
``--tsp_local_search_closing {full,none}`` (K > 0 only with ``--local_search multi2opt``: the multi-move 2-opt on neighbour
lists of K cities, ``decode.batched_nbr_two_opt_grouped``, closed by full sweeps unless ``none``; the records gain
``two_opt_full_sweeps`` and with the header the two settings; without K every record is what it was; ``--local_search
nbr2opt+oropt`` needs K >= 1: the 2-opt + Or-opt search on these lists, ``decode.batched_nbr_local_search_grouped`` - a name of its
own because ``multi2opt+oropt`` with K > 0 stays refused -, the records of ``multi2opt+oropt`` plus, after every other field,
``local_search_full_sweeps`` and ``local_search_full_rounds``), ``--tsp_local_search_candidate_source {knn,heat}`` (``heat``
needs K in 1 .. 128: the neighbour lists come from the round's heatmaps, ``decode.tsp_heat_candidate_lists``; the records gain
``heat_listed`` and with the header the setting; with ``knn`` every record is what it was), ``--tsp_kopt_rounds R`` / ``--tsp_kopt_samples S`` /
``--tsp_kopt_depth D`` (R > 0 only with ``--task tsp``: up to R rounds of the heatmap-guided sampled k-opt search,
``decode.batched_kopt_search_grouped``, on every tour after the local search and on each sample's own heatmap, keyed by its
instance seed; the records gain ``kopt_actions``, one count per copy, and with the header the three settings; with R = 0 every
record is what it was), ``--merge_method {loop,batched}``
(``decode.merge_tours_batch``: one merge call per chunk, same records either way), ``--graph_build {host,device}``
(``graph.build_csr``: where ``edge_index`` becomes the CSR, same records either way), ``--mixed_size_chunks``
(TSP: chunks are runs of consecutive instances of any N, ``mixed_size_chunks``; off: runs of equal N), ``--device``,
``--dist_backend``, ``--records PATH`` (JSONL, one line per instance), ``--heatmap_dir`` (where ``--save_numpy_heatmap``
writes ``numpy_heatmap/{split}-heatmap-{idx}.npy``; default ``<storage_path>/models``), ``--unsafe_checkpoint_load`` (allow a
checkpoint that needs full unpickling - trusted files only).

Several GPUs: run under ``torch.distributed.run``.  Each rank takes ``cuda:LOCAL_RANK`` (or ``--device``) and whole chunks
(``dist.shard_range`` over the chunk list); records are gathered on rank 0, which alone prints and writes.  The metrics are the
mean over all instances of the split.  Lightning's ``sync_dist`` instead averages per-rank means over a ``DistributedSampler``
that pads the split to a multiple of the world size, so its figure differs when the split does not divide evenly.
``--dist_backend gloo`` lets ranks share one GPU (tests)."""
import argparse
import hashlib
import json
import os
import sys
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# difusco/train.py:19-68, in order
REFERENCE_ARGS = [
    ("--task", dict(type=str, required=True)),
    ("--storage_path", dict(type=str, required=True)),
    ("--training_split", dict(type=str, default="data/tsp/tsp50_train_concorde.txt")),
    ("--training_split_label_dir", dict(type=str, default=None)),
    ("--validation_split", dict(type=str, default="data/tsp/tsp50_test_concorde.txt")),
    ("--test_split", dict(type=str, default="data/tsp/tsp50_test_concorde.txt")),
    ("--validation_examples", dict(type=int, default=64)),
    ("--batch_size", dict(type=int, default=64)),
    ("--num_epochs", dict(type=int, default=50)),
    ("--learning_rate", dict(type=float, default=1e-4)),
    ("--weight_decay", dict(type=float, default=0.0)),
    ("--lr_scheduler", dict(type=str, default="constant")),
    ("--num_workers", dict(type=int, default=16)),
    ("--fp16", dict(action="store_true")),
    ("--use_activation_checkpoint", dict(action="store_true")),
    ("--diffusion_type", dict(type=str, default="gaussian")),
    ("--diffusion_schedule", dict(type=str, default="linear")),
    ("--diffusion_steps", dict(type=int, default=1000)),
    ("--inference_diffusion_steps", dict(type=int, default=1000)),
    ("--inference_schedule", dict(type=str, default="linear")),
    ("--inference_trick", dict(type=str, default="ddim")),
    ("--sequential_sampling", dict(type=int, default=1)),
    ("--parallel_sampling", dict(type=int, default=1)),
    ("--n_layers", dict(type=int, default=12)),
    ("--hidden_dim", dict(type=int, default=256)),
    ("--sparse_factor", dict(type=int, default=-1)),
    ("--aggregation", dict(type=str, default="sum")),
    ("--two_opt_iterations", dict(type=int, default=1000)),
    ("--save_numpy_heatmap", dict(action="store_true")),
    ("--project_name", dict(type=str, default="tsp_diffusion")),
    ("--wandb_entity", dict(type=str, default=None)),
    ("--wandb_logger_name", dict(type=str, default=None)),
    ("--resume_id", dict(type=str, default=None)),
    ("--ckpt_path", dict(type=str, default=None)),
    ("--resume_weight_only", dict(action="store_true")),
    ("--do_train", dict(action="store_true")),
    ("--do_test", dict(action="store_true")),
    ("--do_valid_only", dict(action="store_true")),
]
# read only by training, Lightning or W&B: accepted, ignored, listed as ignored_args when given
TRAINING_ONLY = ("training_split", "training_split_label_dir", "batch_size", "num_epochs", "learning_rate", "weight_decay",
                 "lr_scheduler", "num_workers", "use_activation_checkpoint", "project_name", "wandb_entity",
                 "wandb_logger_name", "resume_id", "resume_weight_only")
TSP_KICK_SIZE, TSP_KICK_SPAN = 16, 30     # decode.TSP_KICK_SIZE / TSP_KICK_SPAN (this module parses without torch)
TSP_KOPT_SAMPLES, TSP_KOPT_DEPTH = 1024, 10   # decode.TSP_KOPT_SAMPLES / TSP_KOPT_DEPTH
EXTENSION_ARGS = [
    ("--seed", dict(type=int, default=0, help="base of the per-instance seeds (instance_seed)")),
    ("--instances_per_call", dict(type=int, default=None, help="chunk length (default: default_instances_per_call)")),
    ("--two_opt_method", dict(type=str, default="exact", choices=("exact", "screened"),
                              help="2-opt sweep: exact (float64 for every pair) or screened (float32 screen, same moves)")),
    ("--two_opt_mode", dict(type=str, default="launches", choices=("launches", "resident"),
                            help="TSP: how the single-move 2-opt runs: launches (a launch sequence per move) or resident (one "
                                 "GPU block per instance keeps the tours in LDS, no launch or host read per move; same "
                                 "records; needs --local_search 2opt and P * (N + 1) within the library's limit)")),
    ("--tsp_local_search_mode", dict(type=str, default="launches", choices=("launches", "resident"),
                                     help="TSP: how the 2-opt + Or-opt search runs: launches (a launch sequence per iteration) or "
                                          "resident (one GPU block per instance keeps the tours in LDS through both phases and all "
                                          "rounds; same records; needs --local_search 2opt+oropt and P * (N + 1) within the "
                                          "library's limit)")),
    ("--local_search", dict(type=str, default="2opt", choices=("2opt", "2opt+oropt", "multi2opt", "multi2opt+oropt", "nbr2opt+oropt"),
                             help="tour refinement: 2opt (the reference's), 2opt+oropt (rounds of 2-opt and Or-opt segment moves; "
                                  "records gain or_opt_iterations and local_search_rounds) or multi2opt (every sweep applies all "
                                  "disjoint improving 2-opt moves it selects; 2opt_iterations counts sweeps, records gain "
                                  "two_opt_moves) or multi2opt+oropt (rounds of multi-move 2-opt and multi-move Or-opt "
                                  "sweeps; 2opt_iterations and or_opt_iterations count sweeps, records gain two_opt_moves, "
                                  "or_opt_moves and local_search_rounds) or nbr2opt+oropt (multi2opt+oropt on neighbour lists, "
                                  "needs --tsp_local_search_candidates K >= 1; records gain local_search_full_sweeps and "
                                  "local_search_full_rounds as well)")),
    ("--tsp_local_search_kicks", dict(type=int, default=0,
                                       help="TSP: iterate the multi-move local search with this many seeded segment kicks "
                                            "(needs --local_search multi2opt+oropt; 0: one descent)")),
    ("--tsp_local_search_kick_size", dict(type=int, default=TSP_KICK_SIZE, help="TSP: segment swaps drawn per kick (1 .. 64)")),
    ("--tsp_local_search_kick_span", dict(type=int, default=TSP_KICK_SPAN, help="TSP: longest segment of a swap, in cities")),
    ("--tsp_local_search_descent", dict(type=str, default="full", choices=("full", "focused"),
                                         help="TSP: the descents after the kicks: full (every pair of the tour) or focused (only "
                                              "the candidates next to an edge a kick or a move touched, and one full descent at "
                                              "the end; needs --tsp_local_search_kicks N > 0)")),
    ("--tsp_local_search_kick_bias", dict(type=str, default="uniform", choices=("uniform", "heat"),
                                           help="TSP: where the first cut of a kick's draws falls: uniform (anywhere alike) or "
                                                "heat (on a tour edge with a probability that rises as the sampled heat of the "
                                                "edge falls; needs --tsp_local_search_kicks N > 0)")),
    ("--tsp_kopt_rounds", dict(type=int, default=0,
                               help="TSP: R > 0 runs up to R rounds of the heatmap-guided sampled k-opt search on every tour after "
                                    "the local search, on each sample's own heatmap (0: off; records gain kopt_actions)")),
    ("--tsp_kopt_samples", dict(type=int, default=TSP_KOPT_SAMPLES, help="TSP: simulations per round of the k-opt search (1 .. 4096)")),
    ("--tsp_kopt_depth", dict(type=int, default=TSP_KOPT_DEPTH, help="TSP: new edges per simulated move of the k-opt search (1 .. 10)")),
    ("--tsp_local_search_window", dict(type=int, default=0,
                                        help="TSP: W > 0 runs the iterated search on windows of W tour positions (16 .. 1024), one "
                                             "GPU block per window, --tsp_local_search_kicks kicks (>= 0) per window and pass (needs "
                                             "--local_search multi2opt+oropt, a full descent and uniform kicks; 0: off)")),
    ("--tsp_local_search_passes", dict(type=int, default=1,
                                        help="TSP: passes of the windowed search, odd ones shifted by half a window (needs "
                                             "--tsp_local_search_window W > 0)")),
    ("--tsp_local_search_candidates", dict(type=int, default=0,
                                            help="TSP: K > 0 runs the multi-move 2-opt on neighbour lists of K cities, then closes "
                                                 "as --tsp_local_search_closing says (needs --local_search multi2opt, no kicks, no "
                                                 "window; 0: off; records gain two_opt_full_sweeps)")),
    ("--tsp_local_search_closing", dict(type=str, default="full", choices=("full", "none"),
                                         help="TSP: what follows the neighbour-list sweeps: full (full sweeps until one finds "
                                              "nothing: a 2-opt optimum) or none (needs --tsp_local_search_candidates K > 0)")),
    ("--tsp_local_search_candidate_source", dict(type=str, default="knn", choices=("knn", "heat"),
                                                  help="TSP: where the neighbour lists come from: knn (the K nearest cities) or "
                                                       "heat (the K cities whose edges the sampled heatmaps rate highest, built on "
                                                       "the GPU per round; needs --tsp_local_search_candidates K in 1 .. 128; "
                                                       "records gain heat_listed)")),
    ("--mis_local_search", dict(type=str, default="none", choices=("none", "swap"),
                                 help="MIS refinement after the greedy decode: none (the reference's) or swap ((1,2)-swap local "
                                      "search; records gain decoded_costs)")),
    ("--mis_local_search_kicks", dict(type=int, default=0,
                                       help="MIS: iterate the swap search with this many seeded random kicks (needs "
                                            "--mis_local_search swap; 0: one descent)")),
    ("--mis_local_search_kick_size", dict(type=int, default=4, help="MIS: nodes forced in per kick and instance, on average")),
    ("--mis_local_search_mode", dict(type=str, default="launches", choices=("launches", "resident"),
                                      help="MIS: how the swap search runs: launches (a launch sequence per round and kick) or "
                                           "resident (one GPU block per instance, one host synchronisation per call; same "
                                           "records; needs --mis_local_search swap)")),
    ("--merge_method", dict(type=str, default="loop", choices=("loop", "batched"),
                            help="heatmap -> tour merge: loop (one library call per instance) or batched (one per chunk, same tours)")),
    ("--graph_build", dict(type=str, default="host", choices=("host", "device"),
                           help="COO -> CSR and node order: host (C helper + numpy) or device (difusco_graph_build, same arrays)")),
    ("--mixed_size_chunks", dict(action="store_true",
                                 help="TSP: chunks are runs of consecutive instances of any N (default: runs of equal N)")),
    ("--device", dict(type=str, default=None, help="GPU of this process (default: cuda:LOCAL_RANK)")),
    ("--dist_backend", dict(type=str, default="nccl", help="process-group backend under torch.distributed.run")),
    ("--records", dict(type=str, default=None, help="write one JSON line per instance to this file")),
    ("--heatmap_dir", dict(type=str, default=None, help="--save_numpy_heatmap target (default: <storage_path>/models)")),
    ("--unsafe_checkpoint_load", dict(action="store_true",
                                      help="allow a checkpoint that needs full unpickling (trusted files only)")),
]
REFERENCE_KEYS = {"tsp": ("gt_cost", "solved_cost", "2opt_iterations", "merge_iterations"), "mis": ("gt_cost", "solved_cost")}


def build_parser(suppress_defaults: bool = False) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m difusco_amd.evaluate",
                                description="Evaluate a DIFUSCO checkpoint on test splits (train.py --do_test without Lightning).")
    for flag, kw in REFERENCE_ARGS + EXTENSION_ARGS:
        kw = dict(kw)
        if suppress_defaults:
            kw["default"] = argparse.SUPPRESS
            kw.pop("required", None)
        p.add_argument(flag, **kw)
    return p


def parse_args(argv=None):
    """-> (args, ignored_args): the namespace of ``train.py``'s parser plus the extensions, and the sorted names of the
    training-only arguments given on the command line.  Exits with status 2 on a usage error, ``--do_train`` or no mode."""
    parser = build_parser()
    args = parser.parse_args(argv)
    given = vars(build_parser(suppress_defaults=True).parse_args(argv))
    if args.do_train:
        parser.error("--do_train: training is out of scope; this runner evaluates (--do_test [--do_valid_only])")
    if not args.do_test:
        parser.error("nothing to do: pass --do_test (validate, then test) or --do_test --do_valid_only")
    if args.task not in ("tsp", "mis"):
        parser.error(f"--task {args.task}: tsp or mis")
    if args.ckpt_path is None:
        parser.error("--ckpt_path is required (the weights to evaluate)")
    if args.local_search != "2opt" and args.two_opt_method != "exact":
        parser.error(f"--local_search {args.local_search} runs the exact 2-opt sweep: --two_opt_method {args.two_opt_method} is not built")
    if args.two_opt_mode != "launches" and (args.task != "tsp" or args.local_search != "2opt"):
        parser.error(f"--two_opt_mode {args.two_opt_mode} runs the single-move 2-opt of TSP tours: pass --task tsp "
                     "--local_search 2opt")
    if args.tsp_local_search_mode != "launches" and (args.task != "tsp" or args.local_search != "2opt+oropt"):
        parser.error(f"--tsp_local_search_mode {args.tsp_local_search_mode} runs the 2-opt + Or-opt search of TSP tours: pass "
                     "--task tsp --local_search 2opt+oropt")
    if args.tsp_local_search_kicks < 0 or not 1 <= args.tsp_local_search_kick_size <= 64 or args.tsp_local_search_kick_span < 1:
        parser.error("--tsp_local_search_kicks must be >= 0, --tsp_local_search_kick_size in 1 .. 64 and "
                     "--tsp_local_search_kick_span >= 1")
    if args.tsp_local_search_kicks > 0 and args.local_search != "multi2opt+oropt":
        parser.error(f"--tsp_local_search_kicks {args.tsp_local_search_kicks} iterates the multi-move local search: pass "
                     "--local_search multi2opt+oropt")
    if args.tsp_local_search_kicks > 0 and args.task != "tsp":
        parser.error(f"--tsp_local_search_kicks {args.tsp_local_search_kicks} refines TSP tours: not with --task {args.task}")
    if args.tsp_local_search_descent == "focused" and not args.tsp_local_search_kicks > 0:
        parser.error("--tsp_local_search_descent focused restricts the descents after the kicks of the multi-move local search: "
                     "pass --tsp_local_search_kicks N > 0")
    if args.tsp_local_search_kick_bias == "heat" and not args.tsp_local_search_kicks > 0:
        parser.error("--tsp_local_search_kick_bias heat draws the kicks of the multi-move local search from the heatmap: pass "
                     "--tsp_local_search_kicks N > 0")
    if args.tsp_local_search_kick_bias == "heat" and args.task != "tsp":
        parser.error(f"--tsp_local_search_kick_bias heat biases the kicks of TSP tours: not with --task {args.task}")
    if args.tsp_kopt_rounds < 0 or not 1 <= args.tsp_kopt_samples <= 4096 or not 1 <= args.tsp_kopt_depth <= 10:
        parser.error("--tsp_kopt_rounds must be >= 0, --tsp_kopt_samples in 1 .. 4096 and --tsp_kopt_depth in 1 .. 10")
    if args.tsp_kopt_rounds > 0 and args.task != "tsp":
        parser.error(f"--tsp_kopt_rounds {args.tsp_kopt_rounds} refines TSP tours: not with --task {args.task}")
    W, R = args.tsp_local_search_window, args.tsp_local_search_passes
    if not (W == 0 or 16 <= W <= 1024) or R < 1:
        parser.error("--tsp_local_search_window must be 0 (off) or in 16 .. 1024 and --tsp_local_search_passes >= 1")
    if W == 0 and R != 1:
        parser.error(f"--tsp_local_search_passes {R} counts the passes of the windowed search: pass --tsp_local_search_window W > 0")
    if W > 0 and args.local_search != "multi2opt+oropt":
        parser.error(f"--tsp_local_search_window {W} runs the multi-move local search on tour windows: pass "
                     "--local_search multi2opt+oropt")
    if W > 0 and args.tsp_local_search_kicks > 1024:
        parser.error(f"--tsp_local_search_kicks {args.tsp_local_search_kicks} with --tsp_local_search_window is per window and "
                     "pass: at most 1024")
    if W > 0 and (args.tsp_local_search_descent != "full" or args.tsp_local_search_kick_bias != "uniform"):
        parser.error(f"--tsp_local_search_window {W} combines with neither --tsp_local_search_descent focused nor "
                     "--tsp_local_search_kick_bias heat")
    if args.tsp_local_search_window > 0 and args.task != "tsp":
        parser.error(f"--tsp_local_search_window {args.tsp_local_search_window} refines TSP tours: not with --task {args.task}")
    K = args.tsp_local_search_candidates
    if K < 0:
        parser.error("--tsp_local_search_candidates must be >= 0")
    if K > 0 and args.task != "tsp":
        parser.error(f"--tsp_local_search_candidates {K} refines TSP tours: not with --task {args.task}")
    if K > 0 and args.local_search not in ("multi2opt", "nbr2opt+oropt"):
        parser.error(f"--tsp_local_search_candidates {K} runs the neighbour-list multi-move 2-opt: pass --local_search multi2opt "
                     "(or nbr2opt+oropt, the neighbour-list 2-opt + Or-opt search)")
    if args.local_search == "nbr2opt+oropt" and args.task != "tsp":
        parser.error(f"--local_search nbr2opt+oropt refines TSP tours: not with --task {args.task}")
    if args.local_search == "nbr2opt+oropt" and K == 0:
        parser.error("--local_search nbr2opt+oropt runs on neighbour lists: pass --tsp_local_search_candidates K >= 1")
    if K == 0 and args.tsp_local_search_closing != "full":
        parser.error(f"--tsp_local_search_closing {args.tsp_local_search_closing} closes the neighbour-list sweeps: pass "
                     "--tsp_local_search_candidates K > 0")
    if args.tsp_local_search_candidate_source == "heat" and args.task != "tsp":
        parser.error(f"--tsp_local_search_candidate_source heat lists the neighbours of TSP cities: not with --task {args.task}")
    if args.tsp_local_search_candidate_source == "heat" and not 1 <= K <= 128:
        parser.error("--tsp_local_search_candidate_source heat draws the neighbour lists from the heatmaps: pass "
                     "--tsp_local_search_candidates K in 1 .. 128")
    if args.mis_local_search != "none" and args.task != "mis":
        parser.error(f"--mis_local_search {args.mis_local_search} refines MIS solutions: not with --task {args.task}")
    if args.mis_local_search_kicks < 0 or args.mis_local_search_kick_size < 1:
        parser.error("--mis_local_search_kicks must be >= 0 and --mis_local_search_kick_size >= 1")
    if args.mis_local_search_kicks > 0 and args.mis_local_search != "swap":
        parser.error(f"--mis_local_search_kicks {args.mis_local_search_kicks} iterates the swap search: pass --mis_local_search swap")
    if args.mis_local_search_mode != "launches" and (args.task != "mis" or args.mis_local_search != "swap"):
        parser.error(f"--mis_local_search_mode {args.mis_local_search_mode} runs the MIS swap search: pass --task mis "
                     "--mis_local_search swap")
    ignored = sorted(k for k in given if k in TRAINING_ONLY or (k == "save_numpy_heatmap" and args.task == "mis"))
    return args, ignored


# ---- determinism: seeds and chunks ----------------------------------------------------------------------------------------
def instance_seed(seed: int, split: str, index: int) -> int:
    """The seed of instance ``index`` of ``split`` ("val" / "test"): BLAKE2b with an 8-byte digest of the ASCII text
    ``"{seed}:{split}:{index}"``, read little-endian and masked to 63 bits.  It is both the Philox key of the instance
    (``seeds[b]``) and the seed of the CPU ``torch.Generator`` that draws its x_T (``generators[b]``).  Pinned by the tests."""
    digest = hashlib.blake2b(f"{int(seed)}:{split}:{int(index)}".encode("ascii"), digest_size=8).digest()
    return int.from_bytes(digest, "little") & (2 ** 63 - 1)


def instance_generator(s: int):
    import torch
    return torch.Generator().manual_seed(int(s))


ROWS_PER_CALL = 1 << 18           # output rows of one chunk's union that the default length aims at
MAX_INSTANCES_PER_CALL = 64


def tsp_rows(n: int, sparse_factor: int, parallel_sampling: int) -> int:
    """Output rows of one TSP instance in a step: P x its edges (n K sparse, n^2 dense)."""
    return int(parallel_sampling) * int(n) * (int(sparse_factor) if sparse_factor is not None and sparse_factor > 0 else int(n))


def mis_rows(n_edges: int, parallel_sampling: int) -> int:
    """Edge rows of one MIS graph in a step: P x (2|E| + n)."""
    return int(parallel_sampling) * int(n_edges)


def default_instances_per_call(rows: int) -> int:
    """Default chunk length for instances of ``rows`` rows each (``tsp_rows`` / ``mis_rows``): as many as fit
    ROWS_PER_CALL = 2^18 rows, at least 1, at most 64.  DESIGN §5b: batching pays up to ~10^5 rows per instance and no longer
    at 4 x 10^5.  TSP-50 dense: 64 (P = 1), 26 (P = 4); TSP-500 K=50: 10 / 2; TSP-1000 K=100: 2 / 1."""
    return max(1, min(MAX_INSTANCES_PER_CALL, ROWS_PER_CALL // max(1, int(rows))))


def plan_chunks(sizes: Sequence[int], length: Callable[[int], int], equal_size: bool = True) -> List[Tuple[int, int]]:
    """Cuts instances 0..B-1 into runs [lo, hi) of consecutive instances: a run starts at the first instance not yet taken and
    holds at most ``length(sizes[lo])`` instances, all of size ``sizes[lo]`` when ``equal_size`` (TSP: one N per k-NN and
    2-opt launch).  A function of the split alone, so every world size cuts the same chunks (ranks take whole chunks:
    ``shard_chunks``)."""
    chunks, lo = [], 0
    while lo < len(sizes):
        cap, hi = max(1, int(length(sizes[lo]))), lo + 1
        while hi < len(sizes) and hi - lo < cap and (not equal_size or sizes[hi] == sizes[lo]):
            hi += 1
        chunks.append((lo, hi))
        lo = hi
    return chunks


def split_chunks(task: str, examples, sparse_factor: int = -1, parallel_sampling: int = 1,
                 instances_per_call: Optional[int] = None) -> List[Tuple[int, int]]:
    """The chunks of a split: TSP runs of equal N, MIS runs of graphs of any size; length ``instances_per_call`` or the
    default for the run's first instance."""
    if instances_per_call is not None and int(instances_per_call) < 1:
        raise ValueError("--instances_per_call must be >= 1")
    if task == "tsp":
        return plan_chunks([ex.points.shape[0] for ex in examples],
                           lambda n: instances_per_call or default_instances_per_call(tsp_rows(n, sparse_factor, parallel_sampling)))
    return plan_chunks([ex.edge_index.shape[1] for ex in examples],
                       lambda e: instances_per_call or default_instances_per_call(mis_rows(e, parallel_sampling)), equal_size=False)


def mixed_size_chunks(sizes: Sequence[int], sparse_factor: int = -1, parallel_sampling: int = 1,
                      instances_per_call: Optional[int] = None) -> List[Tuple[int, int]]:
    """``--mixed_size_chunks``: greedy runs [lo, hi) of consecutive TSP instances of any N.  A run closes when the output rows
    of its instances (``tsp_rows``) would exceed ROWS_PER_CALL - an instance above the budget forms a run of its own - and at
    ``instances_per_call`` instances (default MAX_INSTANCES_PER_CALL).  Like ``plan_chunks`` a function of the split and the
    arguments alone, never of the world size."""
    if instances_per_call is not None and int(instances_per_call) < 1:
        raise ValueError("--instances_per_call must be >= 1")
    cap = int(instances_per_call) if instances_per_call else MAX_INSTANCES_PER_CALL
    chunks, lo, rows = [], 0, 0
    for i, n in enumerate(sizes):
        r = tsp_rows(n, sparse_factor, parallel_sampling)
        if i > lo and (rows + r > ROWS_PER_CALL or i - lo >= cap):
            chunks.append((lo, i))
            lo, rows = i, 0
        rows += r
    if len(sizes) > lo:
        chunks.append((lo, len(sizes)))
    return chunks


def shard_chunks(chunks: Sequence[Tuple[int, int]], rank: int, world: int) -> List[Tuple[int, int]]:
    """The whole chunks of ``rank``: a contiguous block of the chunk list (``dist.shard_range``)."""
    from .dist import shard_range
    lo, hi = shard_range(len(chunks), rank, world)
    return list(chunks[lo:hi])


# ---- per-instance values and metrics -------------------------------------------------------------------------------------
def tsp_gt_cost(points, tour) -> float:
    """``TSPEvaluator(np_points).evaluate(np_gt_tour)`` (``pl_tsp_model.py:241-242``): the closed tour's length over the
    float32-rounded coordinates the reference evaluates (``pipeline.tour_length``)."""
    from .pipeline import tour_length
    return tour_length(np.asarray(points).astype(np.float32).astype(np.float64), tour)


def tsp_record(split: str, index: int, ex, seed: int, result) -> dict:
    tour, cost, costs, info = result
    rec = {"split": split, "index": int(index), "source": list(ex.source), "n_nodes": int(ex.points.shape[0]),
           "gt_cost": tsp_gt_cost(ex.points, ex.tour), "solved_cost": float(cost), "all_costs": [float(c) for c in costs],
           "merged_costs": [float(c) for c in info["merged_costs"]], "2opt_iterations": int(info["two_opt_iterations"]),
           "merge_iterations": float(info["merge_iterations"]), "seed": int(seed), "tour": [int(v) for v in tour]}
    for k in ("or_opt_iterations", "local_search_rounds", "two_opt_moves", "or_opt_moves",      # --local_search other than 2opt
              "two_opt_full_sweeps"):                                                            # --tsp_local_search_candidates K > 0
        if k in info:
            rec[k] = int(info[k])
    if "local_search_kicks_improved" in info:      # --tsp_local_search_kicks N > 0
        rec["kicks_improved"] = [int(v) for v in info["local_search_kicks_improved"]]
    if "local_search_closing_sweeps" in info:      # --tsp_local_search_descent focused
        rec["closing_sweeps"] = [int(v) for v in info["local_search_closing_sweeps"]]
    if "kopt_actions" in info:                      # --tsp_kopt_rounds R > 0
        rec["kopt_actions"] = [int(v) for v in info["kopt_actions"]]
    if "local_search_passes_kept" in info:         # --tsp_local_search_window W > 0
        rec["passes_kept"] = [int(v) for v in info["local_search_passes_kept"]]
    for k in ("local_search_full_sweeps", "local_search_full_rounds"):      # --local_search nbr2opt+oropt
        if k in info:
            rec[k] = int(info[k])
    if "local_search_heat_listed" in info:         # --tsp_local_search_candidate_source heat
        rec["heat_listed"] = float(info["local_search_heat_listed"])
    return rec


def mis_record(split: str, index: int, ex, seed: int, result, stats: Optional[dict] = None) -> dict:
    sol, size, sizes = result
    rec = {"split": split, "index": int(index), "source": list(ex.source), "n_nodes": int(ex.n_nodes),
           "gt_cost": float(np.asarray(ex.labels).sum()), "solved_cost": float(size), "all_costs": [float(s) for s in sizes],
           "seed": int(seed), "mis": np.nonzero(np.asarray(sol))[0].tolist()}
    if stats is not None:      # --mis_local_search swap: the greedy sizes only (the call counters belong to a chunk, not an instance)
        rec["decoded_costs"] = [float(s) for s in stats["decoded_sizes"]]
        if "swap_sizes" in stats:      # --mis_local_search_kicks N > 0: the sizes after the first descent and the kick counters
            rec["swap_costs"] = [float(s) for s in stats["swap_sizes"]]
            rec["kicks_entered"] = [int(v) for v in stats["kicks_entered"]]
            rec["kicks_accepted"] = [int(v) for v in stats["kicks_accepted"]]
    return rec


def split_metrics(task: str, split: str, records: Sequence[dict]) -> Dict[str, Optional[float]]:
    """The mean over ``records`` of every key ``test_step`` logs (``{split}/gt_cost``, ``{split}/solved_cost``, and for TSP
    ``{split}/2opt_iterations``, ``{split}/merge_iterations``), and ``{split}/gap_pct``, not a reference key: TSP the mean of
    100 (solved - gt) / gt, MIS the mean of 100 (gt - solved) / gt over the instances with gt > 0 (None if there is none)."""
    if not records:
        raise ValueError(f"split {split}: no instances")
    out = {f"{split}/{k}": float(np.mean([r[k] for r in records])) for k in REFERENCE_KEYS[task]}
    if task == "tsp":
        gaps = [100.0 * (r["solved_cost"] - r["gt_cost"]) / r["gt_cost"] for r in records]
    else:
        gaps = [100.0 * (r["gt_cost"] - r["solved_cost"]) / r["gt_cost"] for r in records if r["gt_cost"] > 0]
    out[f"{split}/gap_pct"] = float(np.mean(gaps)) if gaps else None
    return out


# ---- solving ---------------------------------------------------------------------------------------------------------------
def solve_split(model, task: str, examples, split: str, chunks, *, seed: int = 0, sparse_factor: int = -1,
                parallel_sampling: int = 1, sequential_sampling: int = 1, two_opt_iterations: int = 1000,
                timings: Optional[Dict[str, float]] = None, heatmap_dir: Optional[str] = None,
                two_opt_method: str = "exact", merge_method: str = "loop", local_search: str = "2opt",
                mis_local_search: str = "none", mis_local_search_kicks: int = 0,
                mis_local_search_kick_size: int = 4, mis_local_search_mode: str = "launches", tsp_local_search_kicks: int = 0,
                tsp_local_search_kick_size: int = TSP_KICK_SIZE, tsp_local_search_kick_span: int = TSP_KICK_SPAN,
                tsp_local_search_descent: str = "full", tsp_local_search_kick_bias: str = "uniform",
                tsp_local_search_window: int = 0, tsp_local_search_passes: int = 1,
                two_opt_mode: str = "launches", tsp_local_search_candidates: int = 0,
                tsp_local_search_closing: str = "full", tsp_local_search_mode: str = "launches", tsp_kopt_rounds: int = 0,
                tsp_kopt_samples: int = TSP_KOPT_SAMPLES, tsp_kopt_depth: int = TSP_KOPT_DEPTH,
                tsp_local_search_candidate_source: str = "knn") -> List[dict]:
    """One ``solve_tsp_batch`` / ``solve_mis_batch`` call per chunk ``(lo, hi)`` of ``examples``, each starting its steps at
    offset 0, instance i with ``instance_seed(seed, split, i)`` and its generator.  Returns one record per instance
    (``tsp_record`` / ``mis_record``).  ``heatmap_dir`` (TSP): also writes the ``.npy`` pair ``test_step`` saves
    (``formats.save_numpy_heatmap``) per instance."""
    from .formats import save_numpy_heatmap
    from .pipeline import solve_mis_batch, solve_tsp_batch
    records = []
    for lo, hi in chunks:
        idx = list(range(lo, hi))
        seeds = [instance_seed(seed, split, i) for i in idx]
        gens = [instance_generator(s) for s in seeds]
        if task == "tsp":
            heats = [] if heatmap_dir is not None else None
            pts = [examples[i].points for i in idx]
            # a chunk of one N takes the array form, a mixed chunk (--mixed_size_chunks) the list form of solve_tsp_batch
            res = solve_tsp_batch(model, np.stack(pts) if len({p.shape[0] for p in pts}) == 1 else pts, sparse_factor,
                                  parallel_sampling=parallel_sampling, sequential_sampling=sequential_sampling,
                                  two_opt_iterations=two_opt_iterations, seeds=seeds, generators=gens, timings=timings,
                                  step_offset=0, heatmaps=heats, two_opt_method=two_opt_method,
                                  merge_method=merge_method, local_search=local_search,
                                  **(dict(local_search_kicks=tsp_local_search_kicks,
                                          local_search_kick_size=tsp_local_search_kick_size,
                                          local_search_kick_span=tsp_local_search_kick_span)
                                     if tsp_local_search_kicks > 0 or tsp_local_search_window > 0 else {}),
                                  **(dict(local_search_window=tsp_local_search_window, local_search_passes=tsp_local_search_passes)
                                     if tsp_local_search_window > 0 else {}),
                                  **(dict(local_search_descent="focused") if tsp_local_search_descent == "focused" else {}),
                                  **(dict(local_search_kick_bias="heat") if tsp_local_search_kick_bias == "heat" else {}),
                                  **(dict(kopt_rounds=tsp_kopt_rounds, kopt_samples=tsp_kopt_samples, kopt_depth=tsp_kopt_depth)
                                     if tsp_kopt_rounds > 0 else {}),
                                  **(dict(two_opt_mode="resident") if two_opt_mode == "resident" else {}),
                                  **(dict(local_search_mode="resident") if tsp_local_search_mode == "resident" else {}),
                                  **(dict(local_search_candidates=tsp_local_search_candidates,
                                          local_search_closing=tsp_local_search_closing == "full")
                                     if tsp_local_search_candidates > 0 else {}),
                                  **(dict(local_search_candidate_source="heat")
                                     if tsp_local_search_candidate_source == "heat" else {}))
            for k, i in enumerate(idx):
                records.append(tsp_record(split, i, examples[i], seeds[k], res[k]))
                if tsp_local_search_candidates > 0:
                    records[-1].update(tsp_local_search_candidates=tsp_local_search_candidates,
                                       tsp_local_search_closing=tsp_local_search_closing)
                if tsp_local_search_candidate_source == "heat":
                    records[-1].update(tsp_local_search_candidate_source="heat")
                if two_opt_mode == "resident":
                    records[-1].update(two_opt_mode="resident")
                if tsp_local_search_mode == "resident":
                    records[-1].update(tsp_local_search_mode="resident")
                if tsp_local_search_window > 0:
                    records[-1].update(tsp_local_search_window=tsp_local_search_window,
                                       tsp_local_search_passes=tsp_local_search_passes)
                if tsp_local_search_kicks > 0 or tsp_local_search_window > 0:
                    records[-1].update(tsp_local_search_kicks=tsp_local_search_kicks,
                                       tsp_local_search_kick_size=tsp_local_search_kick_size,
                                       tsp_local_search_kick_span=tsp_local_search_kick_span)
                if tsp_local_search_descent == "focused":
                    records[-1].update(tsp_local_search_descent="focused")
                if tsp_local_search_kick_bias == "heat":
                    records[-1].update(tsp_local_search_kick_bias="heat")
                if tsp_kopt_rounds > 0:
                    records[-1].update(tsp_kopt_rounds=tsp_kopt_rounds, tsp_kopt_samples=tsp_kopt_samples,
                                       tsp_kopt_depth=tsp_kopt_depth)
                if heats is not None:
                    save_numpy_heatmap(heats[k][-1], examples[i].points.astype(np.float32), heatmap_dir, i, split)
        else:
            swap = mis_local_search != "none"
            ls_stats = [] if swap else None
            res = solve_mis_batch(model, [(examples[i].n_nodes, examples[i].edge_index) for i in idx],
                                  parallel_sampling=parallel_sampling, sequential_sampling=sequential_sampling, seeds=seeds,
                                  generators=gens, timings=timings, step_offset=0,
                                  **(dict(local_search=mis_local_search, stats=ls_stats) if swap else {}),
                                  **(dict(local_search_kicks=mis_local_search_kicks,
                                          local_search_kick_size=mis_local_search_kick_size) if mis_local_search_kicks > 0 else {}),
                                  **(dict(local_search_mode="resident") if mis_local_search_mode == "resident" else {}))
            for k, i in enumerate(idx):
                rec = mis_record(split, i, examples[i], seeds[k], res[k], ls_stats[k] if swap else None)
                if mis_local_search_kicks > 0:
                    rec.update(mis_local_search_kicks=mis_local_search_kicks, mis_local_search_kick_size=mis_local_search_kick_size)
                if mis_local_search_mode == "resident":
                    rec.update(mis_local_search_mode="resident")
                records.append(rec)
    return records


def read_split(task: str, path: str, limit: Optional[int] = None):
    from .datasets import SplitFormatError, read_mis_split, read_tsp_split
    examples = read_tsp_split(path, limit) if task == "tsp" else read_mis_split(path, limit=limit)
    if limit is not None and len(examples) < limit:
        raise SplitFormatError(f"{path}: {len(examples)} instances, --validation_examples asks for {limit}")
    if not examples:
        raise SplitFormatError(f"{path}: no instances")
    return examples


def run(argv=None) -> Tuple[List[dict], List[dict]]:
    """The whole evaluation; returns (the JSON lines printed, all records) on rank 0 and ([], []) on the other ranks."""
    args, ignored = parse_args(argv)
    P, S = args.parallel_sampling, args.sequential_sampling
    if args.task == "tsp" and args.save_numpy_heatmap and (P > 1 or S > 1):
        raise NotImplementedError("Save numpy heatmap only support single sampling")      # pl_tsp_model.py:258-260
    import torch
    import torch.distributed as dist
    from .checkpoint import check_config, load_checkpoint
    from .models import MISModel, TSPModel

    state = load_checkpoint(args.ckpt_path, allow_unsafe=args.unsafe_checkpoint_load)
    check_config(state, args.hidden_dim, args.n_layers, args.diffusion_type)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), 0
    if world > 1:
        dist.init_process_group(backend=args.dist_backend)
        rank, world = dist.get_rank(), dist.get_world_size()
    try:
        dev = torch.device(args.device or f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
        torch.cuda.set_device(dev)
        cls = TSPModel if args.task == "tsp" else MISModel
        model = cls(vars(args), state, device=dev, graph_build=args.graph_build,
                    **(dict(precision="fp16x1") if args.fp16 else {}))
        heatmap_dir = None
        if args.task == "tsp" and args.save_numpy_heatmap:
            heatmap_dir = args.heatmap_dir or os.path.join(args.storage_path, "models")
        splits = [("val", args.validation_split, args.validation_examples)]
        if not args.do_valid_only:
            splits.append(("test", args.test_split, None))
        lines, all_records = [], []
        for split, rel, limit in splits:
            t_start = time.perf_counter()
            examples = read_split(args.task, os.path.join(args.storage_path, rel), limit)
            parse_s = time.perf_counter() - t_start
            mixed = args.task == "tsp" and args.mixed_size_chunks
            if mixed:
                chunks = mixed_size_chunks([ex.points.shape[0] for ex in examples], args.sparse_factor, P, args.instances_per_call)
            else:
                chunks = split_chunks(args.task, examples, args.sparse_factor, P, args.instances_per_call)
            timings = {}
            recs = solve_split(model, args.task, examples, split, shard_chunks(chunks, rank, world), seed=args.seed,
                               sparse_factor=args.sparse_factor, parallel_sampling=P, sequential_sampling=S,
                               two_opt_iterations=args.two_opt_iterations, timings=timings, heatmap_dir=heatmap_dir,
                               two_opt_method=args.two_opt_method, merge_method=args.merge_method,
                               local_search=args.local_search, mis_local_search=args.mis_local_search,
                               mis_local_search_kicks=args.mis_local_search_kicks,
                               mis_local_search_kick_size=args.mis_local_search_kick_size,
                               mis_local_search_mode=args.mis_local_search_mode,
                               tsp_local_search_kicks=args.tsp_local_search_kicks,
                               tsp_local_search_kick_size=args.tsp_local_search_kick_size,
                               tsp_local_search_kick_span=args.tsp_local_search_kick_span,
                               tsp_local_search_descent=args.tsp_local_search_descent,
                               tsp_local_search_kick_bias=args.tsp_local_search_kick_bias,
                               tsp_local_search_window=args.tsp_local_search_window,
                               tsp_local_search_passes=args.tsp_local_search_passes, two_opt_mode=args.two_opt_mode,
                               tsp_local_search_candidates=args.tsp_local_search_candidates,
                               tsp_local_search_closing=args.tsp_local_search_closing,
                               tsp_local_search_mode=args.tsp_local_search_mode, tsp_kopt_rounds=args.tsp_kopt_rounds,
                               tsp_kopt_samples=args.tsp_kopt_samples, tsp_kopt_depth=args.tsp_kopt_depth,
                               tsp_local_search_candidate_source=args.tsp_local_search_candidate_source)
            torch.cuda.synchronize(dev)
            gathered = [(recs, timings)]
            if world > 1:
                gathered = [None] * world
                dist.all_gather_object(gathered, (recs, timings))
            wall = time.perf_counter() - t_start
            if rank != 0:
                continue
            recs = sorted((r for g in gathered for r in g[0]), key=lambda r: r["index"])
            stages = {"parse": parse_s}
            for _, tm in gathered:
                for k, v in tm.items():
                    stages[k] = max(stages.get(k, 0.0), v)      # the slowest rank's time of each stage
            line = {"task": args.task, "split": split, **split_metrics(args.task, split, recs),
                    "non_reference_keys": [f"{split}/gap_pct"], "instances": len(recs), "wall_s": round(wall, 4),
                    "instances_per_s": round(len(recs) / wall, 3), "stages_s": {k: round(v, 4) for k, v in stages.items()},
                    "world_size": world, "precision": model.model.precision,
                    "instances_per_call": args.instances_per_call if args.instances_per_call else "auto",
                    "chunks": len(chunks), "chunk_lengths": sorted({hi - lo for lo, hi in chunks}), "seed": args.seed,
                    "two_opt_method": args.two_opt_method, "graph_build": model.graph_build, "ignored_args": ignored}
            if mixed:
                line["mixed_size_chunks"] = True
            if args.two_opt_mode == "resident":
                line["two_opt_mode"] = "resident"
            if args.tsp_local_search_mode == "resident":
                line["tsp_local_search_mode"] = "resident"
            if args.local_search != "2opt":
                line["local_search"] = args.local_search
            if args.mis_local_search != "none":
                line["mis_local_search"] = args.mis_local_search
            if args.tsp_local_search_window > 0:
                line["tsp_local_search_window"] = args.tsp_local_search_window
                line["tsp_local_search_passes"] = args.tsp_local_search_passes
            if args.tsp_local_search_kicks > 0 or args.tsp_local_search_window > 0:
                line["tsp_local_search_kicks"] = args.tsp_local_search_kicks
                line["tsp_local_search_kick_size"] = args.tsp_local_search_kick_size
                line["tsp_local_search_kick_span"] = args.tsp_local_search_kick_span
            if args.tsp_local_search_candidates > 0:
                line["tsp_local_search_candidates"] = args.tsp_local_search_candidates
                line["tsp_local_search_closing"] = args.tsp_local_search_closing
            if args.tsp_local_search_candidate_source == "heat":
                line["tsp_local_search_candidate_source"] = "heat"
            if args.tsp_local_search_descent == "focused":
                line["tsp_local_search_descent"] = "focused"
            if args.tsp_local_search_kick_bias == "heat":
                line["tsp_local_search_kick_bias"] = "heat"
            if args.tsp_kopt_rounds > 0:
                line["tsp_kopt_rounds"] = args.tsp_kopt_rounds
                line["tsp_kopt_samples"] = args.tsp_kopt_samples
                line["tsp_kopt_depth"] = args.tsp_kopt_depth
            if args.mis_local_search_kicks > 0:
                line["mis_local_search_kicks"] = args.mis_local_search_kicks
                line["mis_local_search_kick_size"] = args.mis_local_search_kick_size
            if args.mis_local_search_mode == "resident":
                line["mis_local_search_mode"] = "resident"
            print(json.dumps(line), flush=True)
            lines.append(line)
            all_records += recs
        if rank == 0 and args.records:
            with open(args.records, "w") as f:
                for r in all_records:
                    f.write(json.dumps(r) + "\n")
        return lines, all_records
    finally:
        if world > 1 and dist.is_initialized():
            dist.destroy_process_group()


def main(argv=None) -> int:
    run(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main())
