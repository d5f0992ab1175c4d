"""Drop-in host side of the denoise step: ``TSPModel`` / ``MISModel`` with the reference's method
names, argument order and argument meaning (``difusco/pl_tsp_model.py:122-151``,
``difusco/pl_mis_model.py:118-140``), backed by the gfx950 library instead of the PyTorch-Lightning
modules.  Only the inference path exists here (no training, data loading, tour decoding).

    model = TSPModel(param_args, state_dict)            # param_args: the reference's argparse namespace
    xt = model.categorical_denoise_step(points, xt, t, device, edge_index, target_t=target_t)

``t`` / ``target_t`` are numpy int arrays of shape (1,) exactly as the reference's ``test_step`` passes
them (``pl_tsp_model.py:209-210``); python ints are accepted too.  Returned tensors are new fp32
tensors on ``device``, flattened in sparse mode (``pl_meta_model.py:144-145``).

Extensions beyond the reference signature are keyword-only: ``uniform=`` / ``noise=`` inject the
random numbers (teacher-forced parity tests), ``return_aux=True`` also returns the network
prediction and the pre-sampling probability, ``sample(..., graphed=True)`` replays the whole
sampling loop as one captured HIP graph (``_GraphedSampler``).
"""
from collections import OrderedDict
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import _lib
from .engine import DenoiseEngine
from .graph import CsrGraph, build_csr, build_union_csr, check_graph_build, complete_graph_batch, complete_graph_union
from .schedules import CategoricalDiffusion, GaussianDiffusion, InferenceSchedule

_DEFAULTS = dict(  # difusco/train.py:19-68 (only what the inference path reads)
    diffusion_type="gaussian", diffusion_schedule="linear", diffusion_steps=1000,
    inference_diffusion_steps=1000, inference_schedule="linear", inference_trick="ddim",
    sequential_sampling=1, parallel_sampling=1, n_layers=12, hidden_dim=256, sparse_factor=-1,
    aggregation="sum")


def _as_int(t) -> int:
    if t is None:
        return None
    return int(np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t).reshape(-1)[0])


class _GraphedSampler:
    """One captured sampling loop (``sample(..., graphed=True)``) for one problem shape: the static device buffers the graph
    reads (CSR arrays with ``perm`` / ``node_order`` always materialised, points, x_T, the Philox offset shift), the graph, its
    static output, and strong references to every other buffer whose address the captured launches hold (weights,
    workspace, time-bias rows, generated-input table, prepared state) - evicting the model's own caches cannot free them."""

    def __init__(self, model, task: int, g: CsrGraph, xt_numel: int):
        dev = model.device
        i32 = dict(dtype=torch.int32, device=dev)
        tsp = task == _lib.TASK_TSP
        self.graph = CsrGraph(
            n_nodes=g.n_nodes, n_edges=g.n_edges, rowptr=torch.empty(g.n_nodes + 1, **i32), col=torch.empty(g.n_edges, **i32),
            perm=torch.empty(g.n_edges, **i32), row=torch.empty(g.n_edges, **i32),
            seg_ptr=torch.empty(g.n_segments + 1, **i32) if g.n_segments > 1 else None, n_segments=g.n_segments,
            node_order=torch.empty(g.n_nodes, dtype=torch.int64, device=dev) if tsp else None)
        self.ident_perm = torch.arange(g.n_edges, **i32)
        self.ident_order = torch.arange(g.n_nodes, dtype=torch.int64, device=dev) if tsp else None
        self.points = torch.empty((g.n_nodes, 2), dtype=torch.float32, device=dev) if tsp else None
        self.xt = torch.empty(xt_numel, dtype=torch.float32, device=dev)
        self.shift = torch.zeros(1, dtype=torch.int64, device=dev)
        self.src = None             # the CsrGraph whose arrays the static graph holds now (kept alive: its identity is the test)
        self.cuda_graph = None
        self.out = None
        self.base_calls = 0         # engine call counter the captured offsets start from
        self.keep = ()

    def load(self, g: CsrGraph, points, xt0: torch.Tensor):
        """Stream-ordered copies of one instance into the static inputs (the CSR arrays only when the graph changed)."""
        G = self.graph
        if self.src is not g:
            G.rowptr.copy_(g.rowptr)
            G.col.copy_(g.col)
            G.row.copy_(g.row)
            G.perm.copy_(g.perm if g.perm is not None else self.ident_perm)
            if G.seg_ptr is not None:
                G.seg_ptr.copy_(g.seg_ptr)
            if G.node_order is not None:
                G.node_order.copy_(g.node_order if g.node_order is not None else self.ident_order)
            self.src = g
        if self.points is not None:
            self.points.copy_(points.reshape(-1, 2))
        self.xt.copy_(xt0.reshape(-1))


class COMetaModel:
    """Inference-side state of the reference's ``COMetaModel`` (``pl_meta_model.py:16-47``): the
    diffusion tables, the denoiser weights (as a ``DenoiseEngine``) and the two posteriors."""

    graph_build = "host"      # (class default: the host build, also for a model assembled without the constructor)

    def __init__(self, param_args=None, state_dict=None, node_feature_only=False, device="cuda:0",
                 seed: Optional[int] = None, engine: Optional[DenoiseEngine] = None, precision: str = "fp16x3",
                 fused: bool = True, gn_reduce=None, reorder_nodes: bool = True, backend: Optional[str] = None, flags: int = 0,
                 prepare: bool = True, strict_binary_check: bool = False, graph_build: str = "host"):
        args = dict(_DEFAULTS)
        if param_args is not None:
            args.update(vars(param_args) if not isinstance(param_args, dict) else param_args)
        self.args = SimpleNamespace(**args)
        # where edge_index becomes the CSR: "host" or "device" (graph.build_csr: the same arrays either way)
        self.graph_build = check_graph_build(graph_build)
        self.diffusion_type = self.args.diffusion_type
        self.diffusion_schedule = self.args.diffusion_schedule
        self.diffusion_steps = self.args.diffusion_steps
        self.node_feature_only = node_feature_only
        self.sparse = self.args.sparse_factor > 0 or node_feature_only
        if self.args.aggregation not in ("sum", "mean", "max"):      # gnn_encoder.py:170-191 (every published run uses sum)
            raise ValueError(f"Unknown aggregation {self.args.aggregation}")
        if self.diffusion_type == "gaussian":
            self.diffusion = GaussianDiffusion(T=self.diffusion_steps, schedule=self.diffusion_schedule)
            out_channels = 1
        elif self.diffusion_type == "categorical":
            self.diffusion = CategoricalDiffusion(T=self.diffusion_steps, schedule=self.diffusion_schedule)
            out_channels = 2
        else:
            raise ValueError(f"Unknown diffusion type {self.diffusion_type}")
        if engine is None:
            if state_dict is None:
                raise ValueError("state_dict (reference GNNEncoder weights) or engine required")
            engine = DenoiseEngine(state_dict, device=device, precision=precision, fused=fused, backend=backend, flags=flags,
                                   aggregation=self.args.aggregation)
        elif engine.aggregation != self.args.aggregation:
            raise ValueError(f"the engine aggregates by {engine.aggregation}, the model arguments say {self.args.aggregation}")
        if engine.out_channels != out_channels:
            raise ValueError(f"weights have {engine.out_channels} output channels, "
                             f"{self.diffusion_type} diffusion needs {out_channels}")
        self.model = engine
        self.device = engine.device
        if seed is None:
            # default Philox key: torch's initial seed, made different per rank when torch.distributed runs (ranks of a
            # sharded batch must not draw the same Bernoulli / normal streams).  An explicit ``seed=`` is used as given:
            # callers that shard samples over ranks pass different seeds (bench.py: 1234 + rank).
            seed = torch.initial_seed()
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                seed ^= (torch.distributed.get_rank() + 1) * 0x9E3779B97F4A7C15
        self.seed = int(seed) & (2 ** 63 - 1)
        self._binary_out = None     # (tensor, version) of the last Bernoulli-sampled output: known to be exactly {0,1}
        self._graph_cache = {}
        # prepared state (difusco_step_args.prepared / .tbias): what a TSP step computes from (weights, graph, points) alone
        # is computed once per (graph, points) and reused by every step of a sampling loop; `prepare=False` = stateless steps
        self.prepare = bool(prepare)
        self._prep_cache = {}
        # always verify on the device that a categorical x_t is exactly {0,1} (one reduction + sync per step) instead of
        # trusting the identity of our own last Bernoulli output - see _xt_is_binary
        self.strict_binary_check = bool(strict_binary_check)
        self.reorder_nodes = reorder_nodes      # TSP: Morton-order the nodes of every graph for L2 locality (graph.py)
        # optional: shard-summing callable for the head GroupNorm statistics (difusco_amd.dist.gn_allreduce); None =
        # statistics of each call's own rows, the reference's behaviour for that call
        self.gn_reduce = gn_reduce
        # graphed sampling (sample(..., graphed=True)): an LRU of captured loops, one per problem shape
        self._graphs = OrderedDict()
        self._capture_stream = None
        self._graph_captures = 0
        self._graph_replays = 0

    # ---- graph handling --------------------------------------------------------------------------
    def prepare_graph(self, edge_index: torch.Tensor, num_nodes: int, points=None) -> CsrGraph:
        """COO -> CSR once per instance; cached on the identity of ``edge_index`` so the 50 calls of
        a sampling loop convert once.  ``points`` (TSP): lets the graph renumber its nodes along a space-filling
        curve (``graph.locality_node_order``) - a pure locality choice, valid for any coordinates, invisible outside.
        Tensors created under ``torch.inference_mode()`` (Lightning's default for ``trainer.test``) have no version
        counter: for those the key is the storage address alone, which the cache keeps alive."""
        version = 0 if edge_index.is_inference() else edge_index._version
        key = (edge_index.data_ptr(), tuple(edge_index.shape), version, int(num_nodes))
        g = self._graph_cache.get(key)
        if g is None:
            if len(self._graph_cache) > 8:
                self._graph_cache.clear()
                self._prep_cache.clear()      # (prepared buffers hold their graphs alive)
            g = build_csr(edge_index, int(num_nodes), self.device, points=points if self.reorder_nodes else None,
                          method=self.graph_build)
            self._graph_cache[key] = (g, edge_index)   # keep edge_index alive: data_ptr stays unique
            return g
        return g[0]

    def _dense_graph(self, batch: int, n: int) -> CsrGraph:
        key = ("dense", batch, n)
        g = self._graph_cache.get(key)
        if g is None:
            g = (complete_graph_batch(batch, n, self.device), None)
            self._graph_cache[key] = g
        return g[0]

    def _dense_union_graph(self, sample_sizes) -> CsrGraph:
        """Dense samples of different n (``sample_batch``), cached on the tuple of sizes; equal sizes keep ``_dense_graph``'s
        key and graph."""
        sizes = tuple(int(n) for n in sample_sizes)
        if len(set(sizes)) == 1:
            return self._dense_graph(len(sizes), sizes[0])
        key = ("dense_union", sizes)
        g = self._graph_cache.get(key)
        if g is None:
            if len(self._graph_cache) > 8:
                self._graph_cache.clear()
                self._prep_cache.clear()
            g = (complete_graph_union(sizes, self.device), None)
            self._graph_cache[key] = g
        return g[0]

    def _prepared(self, g: CsrGraph, points):
        """Prepared buffer of (this engine, graph ``g``, ``points``) or None; cached on the identity of ``points`` (the
        sampling loop passes the same tensor 50 times - same rule as ``prepare_graph``)."""
        if not self.prepare or points is None:
            return None
        version = 0 if points.is_inference() else points._version
        # (the buffer is produced asynchronously on the stream that is current at the miss: the entry carries an event, and a step on
        #  another stream waits for it once - engine._ReadyEvent; the key holds no stream handle)
        key = (id(g), points.data_ptr(), tuple(points.shape), version)
        hit = self._prep_cache.get(key)
        if hit is None:
            if len(self._prep_cache) >= 2:      # a sampling loop reuses ONE entry; each pins 5 N H floats + the graph + the points
                self._prep_cache.clear()
            buf = self.model.prepare(g, points)
            from .engine import _ReadyEvent
            hit = ((buf, _ReadyEvent(self.device)) if buf is not None else None, g, points)      # keep g / points alive: id() and data_ptr() stay unique
            self._prep_cache[key] = hit
        return hit[0]

    def prepare_schedule(self, times) -> None:
        """Precompute the time-bias rows of every diffusion time a sampling loop will visit (one launch; ``sample`` calls it
        with the schedule's ``t1`` values).  Steps at other times run the time MLP themselves."""
        if self.prepare:
            self.model.prepare_times([_as_int(t) for t in times])

    def duplicate_edge_index(self, edge_index, num_nodes, device, copies: Optional[int] = None):
        """Disjoint union of ``parallel_sampling`` replicas (pl_meta_model.py:177-184).  ``copies`` (extension): the number of
        replicas, instead of ``self.args.parallel_sampling`` - callers need not write to the args to ask for a batch."""
        P = self.args.parallel_sampling if copies is None else int(copies)
        shift = torch.arange(0, P, device=device).view(1, -1, 1) * num_nodes
        return (edge_index.reshape((2, 1, -1)).to(device) + shift).reshape((2, -1))

    # ---- the two step flavours -------------------------------------------------------------------
    def _next_offset(self) -> int:
        return self.model.calls

    def _xt_is_binary(self, xt: torch.Tensor) -> bool:
        """Is ``xt`` exactly {0,1}-valued?  The reference embeds whatever value arrives (``pl_tsp_model.py:127``:
        ``xt.float()``) and truncates with ``.long()`` in the posterior (``pl_meta_model.py:122``); the two-row embedding
        table and the table-input first layer are exact only for 0/1 inputs.  The sampling loop feeds our own Bernoulli
        outputs back, which are known without looking (same storage, unmodified); anything else is checked on the
        device (one small reduction + sync per call).  Values whose truncation is not 0/1 raise, like ``one_hot``."""
        # NOTE (tensors without a version counter, i.e. created under torch.inference_mode()): an in-place edit of the tensor
        # this model returned cannot be detected without looking at the data; such an x_t must not be mutated in place
        # between steps (or construct the model with strict_binary_check=True, which always looks).
        known = None if getattr(self, "strict_binary_check", False) else self._binary_out      # (tensor kept alive, version or None)
        if known is not None and known[0].data_ptr() == xt.data_ptr() and known[0].numel() == xt.numel() \
                and (known[1] is None) == xt.is_inference() and (known[1] is None or known[1] == xt._version):
            return True
        if bool(((xt == 0) | (xt == 1)).all()):
            return True
        tr = xt.long()
        if not bool(((tr == 0) | (tr == 1)).all()):
            raise ValueError("categorical x_t must truncate to 0/1 (F.one_hot(xt.long(), num_classes=2), "
                             "pl_meta_model.py:122-123)")
        return False

    # ---- batches of instances (sample_batch) -------------------------------------------------------
    def _instance_tables(self, inst_rows, seeds):
        """Device tables of the per-instance random streams: (instance_rows int64 [B+1], instance_seeds int64 [B]); the
        seeds are masked to 63 bits as ``seed=`` of the constructor is."""
        if seeds is None:
            seeds = [self.seed] * (len(inst_rows) - 1)
        seeds = [int(v) & (2 ** 63 - 1) for v in seeds]
        if len(seeds) != len(inst_rows) - 1:
            raise ValueError(f"{len(seeds)} seeds for {len(inst_rows) - 1} instances")
        if self.gn_reduce is not None and len(seeds) > 1:
            raise ValueError("global GroupNorm statistics (gn_reduce) need one statistic segment per call: "
                             "sample_batch with several instances cannot use them")
        rows = torch.as_tensor(np.asarray(inst_rows, dtype=np.int64)).to(self.device)
        return rows, torch.tensor(seeds, dtype=torch.int64).to(self.device)

    @staticmethod
    def _initial_noise(shapes, generators, xt0, device):
        """x_T of every instance, drawn as solo ``sample()`` draws it (``torch.randn(shape, generator=)``), or taken from ``xt0``."""
        B = len(shapes)
        if xt0 is not None:
            if len(xt0) != B:
                raise ValueError(f"{len(xt0)} xt0 tensors for {B} instances")
            out = [x.to(device).reshape(-1) for x in xt0]
            for b, (x, shp) in enumerate(zip(out, shapes)):
                if x.numel() != int(np.prod(shp)):
                    raise ValueError(f"xt0[{b}] has {x.numel()} elements, instance {b} needs {int(np.prod(shp))}")
            return out
        if generators is not None and len(generators) != B:
            raise ValueError(f"{len(generators)} generators for {B} instances")
        out = []
        for b, shp in enumerate(shapes):
            gen = None if generators is None else generators[b]
            out.append(torch.randn(shp, generator=gen, device=device if gen is None else gen.device).to(device).reshape(-1))
        return out

    def _sample_loop(self, step, xt):
        """The denoising loop of ``sample()`` over a whole union; ``step(xt, t1, t2)`` is one step of it."""
        steps = self.args.inference_diffusion_steps
        sched = InferenceSchedule(inference_schedule=self.args.inference_schedule, T=self.diffusion.T, inference_T=steps)
        if self.diffusion_type == "categorical":
            xt = (xt > 0).float()
        self.prepare_schedule([sched(i)[0] for i in range(steps)])
        for i in range(steps):
            t1, t2 = sched(i)
            xt = step(xt, np.array([t1]).astype(int), np.array([t2]).astype(int))
        return xt * 0.5 + 0.5 if self.diffusion_type == "gaussian" else xt + 1e-6

    def _union_step(self, g, task, points, instances, step_offset=None):
        """One step of the loop over a union.  ``step_offset``: the k-th step of the loop draws at Philox offset
        ``step_offset + k`` instead of the engine's call counter (which advances either way); None = the counter."""
        if step_offset is not None and int(step_offset) < 0:
            raise ValueError("step_offset must be >= 0")
        k = [0]

        def step(xt, t1, t2):
            off = None if step_offset is None else int(step_offset) + k[0]
            k[0] += 1
            if self.diffusion_type == "gaussian":
                return self._gaussian(g, task, points, xt, t1, t2, None, False, instances=instances, offset=off)
            return self._categorical(g, task, points, xt, t1, t2, None, False, instances=instances, offset=off)
        return step

    def _post_constants(self, t: int, target_t: int) -> np.ndarray:
        """``difusco_step_args.post`` of the step t -> target_t."""
        post = np.zeros(8, dtype=np.float32)
        if self.diffusion_type == "gaussian":
            post[:5] = self.diffusion.posterior_constants(t, target_t, self.args.inference_trick)
        else:
            post[:4] = self.diffusion.posterior_constants(t, target_t)
            post[4] = 1.0 if target_t > 0 else 0.0                        # pl_meta_model.py:139-142
        return post

    def _categorical(self, g, task, points, xt, t, target_t, uniform, return_aux, instances=None, offset=None):
        t, target_t = _as_int(t), _as_int(target_t)
        if target_t is None:
            target_t = t - 1                                              # pl_meta_model.py:108-109
        post = self._post_constants(t, target_t)
        out, pred, prob = self.model.step(
            g, task, _lib.CATEGORICAL, xt, float(t), post, points=points, xt_is_binary=self._xt_is_binary(xt),
            rand=uniform if target_t > 0 else None, seed=self.seed,
            offset=self._next_offset() if offset is None else offset,
            want_pred=return_aux, want_prob=return_aux, gn_reduce=self.gn_reduce,
            prepared=self._prepared(g, points) if task == _lib.TASK_TSP else None, instances=instances)
        # tensors created under torch.inference_mode() (Lightning's default for trainer.test) have no version counter:
        # for those the held reference + storage identity is the whole key (no host sync in the 50-step loop either way)
        self._binary_out = (out, None if out.is_inference() else out._version) if target_t > 0 else None
        return (out, pred, prob) if return_aux else out

    def _gaussian(self, g, task, points, xt, t, target_t, noise, return_aux, instances=None, offset=None):
        t, target_t = _as_int(t), _as_int(target_t)
        if target_t is None:
            target_t = t - 1
        post = self._post_constants(t, target_t)
        out, pred, _ = self.model.step(
            g, task, _lib.GAUSSIAN, xt, float(t), post, points=points, xt_is_binary=False,
            rand=noise if post[4] != 0 else None, seed=self.seed,
            offset=self._next_offset() if offset is None else offset, want_pred=return_aux,
            gn_reduce=self.gn_reduce, prepared=self._prepared(g, points) if task == _lib.TASK_TSP else None,
            instances=instances)
        return (out, pred) if return_aux else out

    # ---- graphed sampling (sample(..., graphed=True)) ------------------------------------------------
    GRAPH_POOL = 4      # captured loops kept per model (least recently used evicted first)

    @property
    def graph_captures(self) -> int:
        """Sampling loops captured so far (each first graphed call of a new problem shape captures one)."""
        return self._graph_captures

    @property
    def graph_replays(self) -> int:
        """Graphed calls served by replaying an already captured loop."""
        return self._graph_replays

    def clear_graphs(self) -> None:
        """Drop every captured loop with its static buffers, graph memory pool and capture-stream workspace."""
        if self._graphs:
            torch.cuda.synchronize(self.device)      # (a replay or an output copy may still read the pool)
            self._graphs.clear()
        if self._capture_stream is not None:
            self.model._ws.pop(self._capture_stream.cuda_stream, None)

    def _refuse_graphed(self):
        """The configurations a captured loop cannot serve (checked before any graph or GPU work of the call)."""
        if self.gn_reduce is not None:
            raise ValueError("graphed=True cannot be combined with gn_reduce: the collective between the two phases of a "
                             "step cannot sit inside a captured graph")
        if self.model.flags & _lib.FLAG_CHECK_FINITE:
            raise ValueError("graphed=True cannot be combined with FLAG_CHECK_FINITE: the finiteness check synchronises")
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("graphed=True inside a stream capture: sample() cannot capture its loop into another graph")

    def _graph_key(self, task: int, g: CsrGraph, dense_shape):
        """What fixes the launches of a captured loop.  seg_ptr is a function of the dense shape (sparse calls of ``sample``
        have one statistic segment); its values are copied into the static buffer with the other CSR arrays anyway."""
        e = self.model
        return (task, self.diffusion_type, self.diffusion_schedule, self.diffusion.T, self.args.inference_diffusion_steps,
                self.args.inference_schedule, self.args.inference_trick if self.diffusion_type == "gaussian" else None,
                dense_shape, g.n_nodes, g.n_edges, g.n_segments, e.precision, e.fused, e.backend, e.flags, e.aggregation,
                e.use_gen_table, self.prepare, self.seed)

    def _graphed_loop(self, s: _GraphedSampler, task: int):
        """The whole loop of ``sample()`` on the static buffers of ``s``, on the current stream: prepared state, the
        categorical cast, the steps (Philox offsets shifted by ``s.shift``), the final affine map.  Returns (output,
        prepared buffer)."""
        steps = self.args.inference_diffusion_steps
        sched = InferenceSchedule(inference_schedule=self.args.inference_schedule, T=self.diffusion.T, inference_T=steps)
        categorical = self.diffusion_type == "categorical"
        tsp = task == _lib.TASK_TSP
        prepared = self.model.prepare(s.graph, s.points) if (tsp and self.prepare) else None
        xt = (s.xt > 0).float() if categorical else s.xt
        binary = categorical         # x_T > 0 and every Bernoulli output are exactly {0,1}: no device check, no sync
        for i in range(steps):
            t1, t2 = sched(i)
            t1, t2 = _as_int(np.array([t1]).astype(int)), _as_int(np.array([t2]).astype(int))
            post = self._post_constants(t1, t2)
            xt, _, _ = self.model.step(
                s.graph, task, _lib.CATEGORICAL if categorical else _lib.GAUSSIAN, xt, float(t1), post,
                points=s.points, xt_is_binary=binary, seed=self.seed, offset=self._next_offset(), prepared=prepared,
                offset_shift=s.shift)
            binary = categorical and post[4] != 0
        return (xt + 1e-6 if categorical else xt * 0.5 + 0.5), prepared

    def _sample_graphed(self, task: int, g: CsrGraph, points, shape, xt0, generator, dense_shape):
        """``sample(..., graphed=True)``: bitwise what the eager loop returns at the same engine call counter, which it
        advances by the number of steps as the eager loop does.  x_T is drawn as the eager loop draws it.  The first call of a
        problem shape runs the loop eagerly on the capture stream (its result is the call's) and then captures it; later
        calls copy the instance into the static buffers, write the offset shift and replay."""
        dev = self.device
        if xt0 is None:
            xt0 = torch.randn(shape, generator=generator, device=dev if generator is None else generator.device)
        xt0 = xt0.to(dev)
        if xt0.numel() != int(np.prod(shape)):
            raise ValueError(f"xt0 has {xt0.numel()} elements, the call needs {int(np.prod(shape))}")
        if self.diffusion_type == "categorical" and xt0.dtype != torch.float32:
            xt0 = (xt0 > 0).float()      # (the eager cast compares in xt0's own dtype; a float32 copy could round a value to 0)
        steps = self.args.inference_diffusion_steps
        key = self._graph_key(task, g, dense_shape)
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(device=dev)
        cap, cur = self._capture_stream, torch.cuda.current_stream(dev)
        s = self._graphs.get(key)
        cap.wait_stream(cur)
        with torch.cuda.stream(cap):
            if s is not None:
                self._graphs.move_to_end(key)
                s.load(g, points, xt0)
                s.shift.fill_(self.model.calls - s.base_calls)
                s.cuda_graph.replay()
                self.model.calls += steps
                self._graph_replays += 1
                out = s.out
            else:
                while len(self._graphs) >= self.GRAPH_POOL:
                    torch.cuda.synchronize(dev)
                    self._graphs.popitem(last=False)
                s = _GraphedSampler(self, task, g, int(np.prod(shape)))
                s.load(g, points, xt0)
                # warm-up = this call's result: creates the capture stream's workspace, the time-bias rows and the
                # generated-input table on this stream (or waits for them once), so no foreign event lands in the capture
                sched = InferenceSchedule(inference_schedule=self.args.inference_schedule, T=self.diffusion.T, inference_T=steps)
                times = [sched(i)[0] for i in range(steps)]
                self.prepare_schedule(times)
                out, _ = self._graphed_loop(s, task)
                out.record_stream(cur)
                s.base_calls = self.model.calls
                s.cuda_graph = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(s.cuda_graph, stream=cap):
                        s.out, prepared = self._graphed_loop(s, task)
                finally:
                    self.model.calls = s.base_calls      # capturing launched nothing: the counter stays where eager leaves it
                e = self.model
                s.keep = (e.blob, e._ws[cap.cuda_stream], prepared, e._gen_table[0] if e._gen_table is not None else None,
                          [e._tbias[float(_as_int(t))][0] for t in times if float(_as_int(t)) in e._tbias])
                self._graphs[key] = s
                self._graph_captures += 1
        cur.wait_stream(cap)
        res = out.clone()
        return res.reshape(dense_shape) if dense_shape is not None else res


class TSPModel(COMetaModel):
    """Inference half of ``difusco/pl_tsp_model.py``."""

    def __init__(self, param_args=None, state_dict=None, **kw):
        super().__init__(param_args=param_args, state_dict=state_dict, node_feature_only=False, **kw)

    def _graph_and_inputs(self, points, xt, edge_index):
        if edge_index is not None:
            g = self.prepare_graph(edge_index, points.shape[0], points=points)
            return g, points.reshape(-1, 2), xt.reshape(-1), None
        if points.dim() != 3:
            raise ValueError("dense mode expects points [B,V,2] and xt [B,V,V]")
        B, V = points.shape[0], points.shape[1]
        return self._dense_graph(B, V), points.reshape(-1, 2), xt.reshape(-1), (B, V, V)

    def categorical_denoise_step(self, points, xt, t, device, edge_index=None, target_t=None, *,
                                 uniform=None, return_aux=False):
        g, pts, x, dense_shape = self._graph_and_inputs(points, xt, edge_index)
        res = self._categorical(g, _lib.TASK_TSP, pts, x.float(), t, target_t, uniform, return_aux)
        if dense_shape is None:
            return res
        if return_aux:
            out, pred, prob = res
            return out.reshape(dense_shape), pred.reshape(dense_shape + (2,)), prob.reshape(dense_shape)
        return res.reshape(dense_shape)

    def gaussian_denoise_step(self, points, xt, t, device, edge_index=None, target_t=None, *,
                              noise=None, return_aux=False):
        g, pts, x, dense_shape = self._graph_and_inputs(points, xt, edge_index)
        res = self._gaussian(g, _lib.TASK_TSP, pts, x.float(), t, target_t, noise, return_aux)
        if dense_shape is None:
            return res
        if return_aux:
            out, pred = res
            return out.reshape(dense_shape), pred.reshape(dense_shape)
        return res.reshape(dense_shape)

    def sample(self, points, edge_index=None, xt0=None, generator=None, *, graphed=False):
        """The sampling loop of ``test_step`` (``pl_tsp_model.py:185-222``) for ONE noise sample per
        graph of the call: returns the heatmap tensor (``+1e-6`` categorical, ``*0.5+0.5`` gaussian),
        still on the device.  ``points``/``edge_index`` already hold the (possibly duplicated) batch.
        ``graphed=True``: the same bits from one replay of a captured HIP graph of the whole loop (captured on the first
        call of a problem shape; see ``_sample_graphed``)."""
        if graphed:
            self._refuse_graphed()
            if edge_index is not None:
                g = self.prepare_graph(edge_index, points.shape[0], points=points)
                return self._sample_graphed(_lib.TASK_TSP, g, points, (edge_index.shape[1],), xt0, generator, None)
            if points.dim() != 3:
                raise ValueError("dense mode expects points [B,V,2] and xt [B,V,V]")
            B, V = points.shape[0], points.shape[1]
            return self._sample_graphed(_lib.TASK_TSP, self._dense_graph(B, V), points, (B, V, V), xt0, generator, (B, V, V))
        steps = self.args.inference_diffusion_steps
        sched = InferenceSchedule(inference_schedule=self.args.inference_schedule, T=self.diffusion.T,
                                  inference_T=steps)
        if xt0 is None:
            shape = (edge_index.shape[1],) if edge_index is not None else (points.shape[0], points.shape[1], points.shape[1])
            xt0 = torch.randn(shape, generator=generator, device=self.device if generator is None else generator.device)
        xt = xt0.to(self.device)
        if self.diffusion_type == "categorical":
            xt = (xt > 0).float()
        self.prepare_schedule([sched(i)[0] for i in range(steps)])
        for i in range(steps):
            t1, t2 = sched(i)
            t1, t2 = np.array([t1]).astype(int), np.array([t2]).astype(int)
            if self.diffusion_type == "gaussian":
                xt = self.gaussian_denoise_step(points, xt, t1, self.device, edge_index, target_t=t2)
            else:
                xt = self.categorical_denoise_step(points, xt, t1, self.device, edge_index, target_t=t2)
        return xt * 0.5 + 0.5 if self.diffusion_type == "gaussian" else xt + 1e-6

    def sample_batch(self, points, edge_index=None, seeds=None, generators=None, xt0=None, step_offset=None):
        """``sample()`` of B instances in ONE sampling loop over their disjoint union, every instance getting what its own
        ``sample()`` call returns.  ``points``: list of B tensors, each what ``sample()`` takes for that instance (sparse: [P n_b, 2]
        with ``edge_index[b]`` [2, P E_b] holding its P parallel samples; dense: [P_b, n_b, 2], ``edge_index=None``, any n_b:
        instance b returns [P_b, n_b, n_b]).  ``seeds[b]``: the Philox key of instance b (a solo model built with ``seed=seeds[b]`` draws the same; default:
        this model's seed for all); ``generators[b]`` / ``xt0[b]``: its initial noise, as in ``sample()``.  Each instance keeps
        its own head GroupNorm statistics (sparse: one segment per instance, the solo call's; dense: one per sample, as solo)
        and its own random streams (``DIFUSCO_RAND_PHILOX_INSTANCES``); the step offsets are this engine's call counter, as
        in ``sample()``, or ``step_offset``, ``step_offset + 1``, ... when given (``step_offset=0``: what a fresh engine draws,
        whatever this one ran before).  Returns the list of B heatmaps, each shaped like ``sample()``'s."""
        B = len(points)
        if B < 1:
            raise ValueError("sample_batch needs at least one instance")
        dev = self.device
        if edge_index is not None:
            if len(edge_index) != B:
                raise ValueError(f"{len(edge_index)} edge_index tensors for {B} instances")
            pts = [p.reshape(-1, 2) for p in points]
            on = dev if self.graph_build == "device" else "cpu"      # the device build reads the points where they are
            g, _, inst_rows = build_union_csr(edge_index, [p.shape[0] for p in pts], dev,
                                              points=torch.cat([p.detach().to(on) for p in pts]) if self.reorder_nodes else None,
                                              method=self.graph_build)
            union_pts = torch.cat([p.to(dev, torch.float32) for p in pts])
            shapes = [(int(e.shape[1]),) for e in edge_index]
            out_shapes = shapes
        else:
            if any(p.dim() != 3 or p.shape[2] != 2 for p in points):
                raise ValueError("dense mode expects points [P_b, n_b, 2] for every instance")
            # one statistic segment per sample, as solo; instances may differ in n
            g = self._dense_union_graph([int(p.shape[1]) for p in points for _ in range(int(p.shape[0]))])
            union_pts = torch.cat([p.to(dev, torch.float32).reshape(-1, 2) for p in points])
            shapes = [(int(p.shape[0]), int(p.shape[1]), int(p.shape[1])) for p in points]
            out_shapes = shapes
            inst_rows = np.concatenate([[0], np.cumsum([int(np.prod(s_)) for s_ in shapes])])
        instances = self._instance_tables(inst_rows, seeds)
        xt = torch.cat(self._initial_noise(shapes, generators, xt0, dev))
        heat = self._sample_loop(self._union_step(g, _lib.TASK_TSP, union_pts, instances, step_offset), xt)
        return [heat[int(inst_rows[b]):int(inst_rows[b + 1])].reshape(out_shapes[b]) for b in range(B)]


class MISModel(COMetaModel):
    """Inference half of ``difusco/pl_mis_model.py`` (node features only)."""

    def __init__(self, param_args=None, state_dict=None, **kw):
        super().__init__(param_args=param_args, state_dict=state_dict, node_feature_only=True, **kw)

    def categorical_denoise_step(self, xt, t, device, edge_index=None, target_t=None, *, uniform=None,
                                 return_aux=False):
        g = self.prepare_graph(edge_index, xt.reshape(-1).shape[0])
        return self._categorical(g, _lib.TASK_MIS, None, xt.reshape(-1).float(), t, target_t, uniform, return_aux)

    def gaussian_denoise_step(self, xt, t, device, edge_index=None, target_t=None, *, noise=None, return_aux=False):
        g = self.prepare_graph(edge_index, xt.reshape(-1).shape[0])
        return self._gaussian(g, _lib.TASK_MIS, None, xt.reshape(-1).float(), t, target_t, noise, return_aux)

    def sample(self, n_nodes, edge_index, xt0=None, generator=None, *, graphed=False):
        """``pl_mis_model.py:156-192`` for one noise sample per graph of the call.  ``graphed=True``: the same bits from one
        replay of a captured HIP graph of the whole loop (``TSPModel.sample``)."""
        if graphed:
            self._refuse_graphed()
            g = self.prepare_graph(edge_index, int(n_nodes))
            return self._sample_graphed(_lib.TASK_MIS, g, None, (int(n_nodes),), xt0, generator, None)
        steps = self.args.inference_diffusion_steps
        sched = InferenceSchedule(inference_schedule=self.args.inference_schedule, T=self.diffusion.T,
                                  inference_T=steps)
        if xt0 is None:
            xt0 = torch.randn((n_nodes,), generator=generator, device=self.device if generator is None else generator.device)
        xt = xt0.to(self.device)
        if self.diffusion_type == "categorical":
            xt = (xt > 0).float()
        self.prepare_schedule([sched(i)[0] for i in range(steps)])
        for i in range(steps):
            t1, t2 = sched(i)
            t1, t2 = np.array([t1]).astype(int), np.array([t2]).astype(int)
            if self.diffusion_type == "gaussian":
                xt = self.gaussian_denoise_step(xt, t1, self.device, edge_index, target_t=t2)
            else:
                xt = self.categorical_denoise_step(xt, t1, self.device, edge_index, target_t=t2)
        return xt * 0.5 + 0.5 if self.diffusion_type == "gaussian" else xt + 1e-6

    def sample_batch(self, n_nodes, edge_index, seeds=None, generators=None, xt0=None, step_offset=None):
        """``sample()`` of B graphs in ONE sampling loop over their disjoint union: ``n_nodes[b]`` / ``edge_index[b]`` are what
        ``sample()`` takes for graph b (its P parallel samples already duplicated), ``seeds`` / ``generators`` / ``xt0`` /
        ``step_offset`` as in ``TSPModel.sample_batch``.  One head statistic segment per graph (= its solo call).  Returns the B
        node-score tensors."""
        B = len(n_nodes)
        if B < 1 or len(edge_index) != B:
            raise ValueError("sample_batch needs one edge_index per graph and at least one graph")
        g, _, inst_rows = build_union_csr(edge_index, [int(v) for v in n_nodes], self.device, task_rows="nodes",
                                          method=self.graph_build)
        instances = self._instance_tables(inst_rows, seeds)
        xt = torch.cat(self._initial_noise([(int(v),) for v in n_nodes], generators, xt0, self.device))
        heat = self._sample_loop(self._union_step(g, _lib.TASK_MIS, None, instances, step_offset), xt)
        return [heat[int(inst_rows[b]):int(inst_rows[b + 1])] for b in range(B)]
