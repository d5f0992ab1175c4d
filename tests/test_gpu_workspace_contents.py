"""The outputs of a call are bit-identical whatever bytes its scratch held when the call began.

Every GPU entry works in caller-provided scratch that the Python layer allocates with ``torch.empty``; here the scratch is an arena
(tests/workspace_poison.py) filled with zeros, with 0xFF bytes (NaN as a float, -1 as an int), with seeded random bytes, or left
as a different, larger call of the same entry (for the step: another task and engine) left it.  A counter, flag, pad row or tile
maximum that is right only because the buffer happened to hold zeros - or the last run's values - changes a result here.

The denoise step: every poisoned run is ``torch.equal`` to the ``zeros`` run, and the ``zeros`` run is held to the oracle bound the
suite already uses for its engine (test_gpu_parity.py: TOL for a categorical step and for bf16x3, CLASS_TOL for the Gaussian and the
non-binary categorical step of the fp32-class engines; test_gpu_fp16x1.py: 2 d + 1e-5 against the fp32 oracle, d = the distance of
the emulated fp16x1 network from it), so the family is tied to an independent reference and not only to itself.  The decode, search,
MIS and graph entries: every run equals its case's own expectation - a recorded fixture or a numpy restatement.

The ``fill`` parameter is the outermost one: all ``zeros`` cases come first in the file's order."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import philox_reference as P
import workspace_poison as WP
from difusco_amd import _lib
from oracle import difusco_oracle as O
from test_gpu_parity import CLASS_TOL, TOL
from test_gpu_philox_exact import ENGINES as PHILOX_ENGINES

pytestmark = pytest.mark.gpu

ARENA_BYTES = 64 << 20
SEED, OFFSET = 0x299f31d0a4093822, (1 << 32) - 3
INSTANCE_SEEDS = [(1 << 62) + 5, (0x7fffffff << 32) | 7]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def arena(dev):
    return WP.Arena(dev, ARENA_BYTES)


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} values differ, first at " \
                                  f"{(a != b).reshape(-1).nonzero()[:8].reshape(-1).tolist()}"


# =========================================== the denoise step =====================================================================
# name -> (hidden, precision, fused, flags, aggregation): the engines of test_gpu_philox_exact.py, fp16x1 and the other aggregations
STEP_ENGINES = {name: v + ("sum",) for name, v in PHILOX_ENGINES.items()}
STEP_ENGINES.update({"fused-fp16x1": (256, "fp16x1", True, 0, "sum"), "fused-fp16x3-mean": (256, "fp16x3", True, 0, "mean"),
                     "fused-fp16x3-max": (256, "fp16x3", True, 0, "max")})
DIFFUSIONS = ("categorical", "categorical-nonbinary", "gaussian-ddim", "gaussian-ddim-no-table")
GRAPHS = ("tsp-37-k7", "tsp-32-k8", "tsp-11-k3", "tsp-union-37-20", "dense-b2-v14", "mis-er60", "mis-no-edges")
T, TARGET_T = 500, 450


def _layers(hidden):
    return 3 if hidden == 256 else 2


@functools.lru_cache(maxsize=None)
def _params(hidden, channels):
    return O.init_params(hidden, _layers(hidden), channels, seed=100 + hidden + channels)


@functools.lru_cache(maxsize=None)
def _engine(name, channels):
    from difusco_amd.engine import DenoiseEngine
    hidden, precision, fused, flags, agg = STEP_ENGINES[name]
    return DenoiseEngine(_params(hidden, channels), device="cuda:0", precision=precision, fused=fused, backend="ctypes", flags=flags,
                         aggregation=agg)


@functools.lru_cache(maxsize=None)
def _post(diffusion):
    from difusco_amd.schedules import CategoricalDiffusion, GaussianDiffusion
    post = np.zeros(8, dtype=np.float32)
    if diffusion.startswith("categorical"):
        post[:4] = CategoricalDiffusion(T=1000, schedule="linear").posterior_constants(T, TARGET_T)
        post[4] = 1.0                                                # the step draws its Bernoulli numbers on the device
    else:
        post[:5] = GaussianDiffusion(T=1000, schedule="linear").posterior_constants(T, TARGET_T, "ddim")
        assert post[4] == 0.0                                        # DDIM: no draw
    return post


@functools.lru_cache(maxsize=None)
def _graph_case(name):
    """-> dict(task, g, pts (device or None), rows, instances (rows, seeds) or None, parts): ``parts`` is what the oracle is called
    on, one entry per statistic segment family: ("tsp", points, edge_index, row slice), ("dense", points [B, V, 2], slice) or
    ("mis", edge_index, n, slice)."""
    from difusco_amd.graph import build_csr, build_union_csr, complete_graph_batch
    import graph_build_emulation as G
    import graph_zoo as Z
    dev = torch.device("cuda:0")
    if name.startswith("tsp-union"):
        sizes = [37, 20]
        inst = [O.tsp_instance(n, 7, seed=20 + i) for i, n in enumerate(sizes)]
        pts = [torch.from_numpy(p) for p, _ in inst]
        eis = [torch.from_numpy(e) for _, e in inst]
        g, _, rows = build_union_csr(eis, sizes, dev, points=torch.cat(pts))
        rows = [int(v) for v in rows]
        assert rows == [0, 259, 399] and g.n_segments == 2           # one statistic segment per instance; 259 is inside a tile
        parts = [("tsp", p, e, slice(rows[b], rows[b + 1])) for b, (p, e) in enumerate(zip(pts, eis))]
        return dict(task=_lib.TASK_TSP, g=g, pts=torch.cat(pts).to(dev), rows=rows[-1], instances=(rows, INSTANCE_SEEDS), parts=parts)
    if name.startswith("tsp-"):
        n, k = (int(v.lstrip("k")) for v in name.split("-")[1:])
        p, ei = O.tsp_instance(n, k, seed=n)
        pts, ei = torch.from_numpy(p), torch.from_numpy(ei)
        g = build_csr(ei, n, dev, points=pts)
        E = n * k
        # E = 259: a partial tile and whole pad tiles inside E_pad = 512; 256: no padding at all; 33: one full tile and one edge
        assert g.n_edges == E == {"tsp-37-k7": 259, "tsp-32-k8": 256, "tsp-11-k3": 33}[name]
        return dict(task=_lib.TASK_TSP, g=g, pts=pts.to(dev), rows=E, instances=None, parts=[("tsp", pts, ei, slice(0, E))])
    if name == "dense-b2-v14":
        B, V = 2, 14
        g = complete_graph_batch(B, V, dev)
        assert g.n_segments == B and g.n_edges == B * V * V and (V * V) % 32 != 0      # segments of 196 rows: not tile aligned
        pts = torch.rand(B, V, 2, generator=torch.Generator().manual_seed(8))
        return dict(task=_lib.TASK_TSP, g=g, pts=pts.reshape(-1, 2).to(dev), rows=B * V * V, instances=None,
                    parts=[("dense", pts, slice(0, B * V * V))])
    if name == "mis-er60":
        n = 60
        ei = G.er_edge_index(n, 0.1, 31)
        node = int(np.bincount(ei[0], minlength=n).argmax())                            # the best connected node loses every entry,
        ei = ei[:, (ei[0] != node) & (ei[1] != node)]                                   # its self loop too: an empty row in the middle
        assert 0 < node < n - 1 and not (ei == node).any()
    else:
        deg, ei = Z.zoo_graph("no_edges")
        n = len(deg)
        assert ei.shape[1] == 0 and n == 40
    ei = torch.from_numpy(ei)
    return dict(task=_lib.TASK_MIS, g=build_csr(ei, n, dev), pts=None, rows=n, instances=None, parts=[("mis", ei, n, slice(0, n))])


@functools.lru_cache(maxsize=None)
def _xt(graph, diffusion):
    rows = _graph_case(graph)["rows"]
    g = torch.Generator().manual_seed(5 + rows)
    if diffusion == "categorical":
        return (torch.randn(rows, generator=g) > 0).float()
    if diffusion == "categorical-nonbinary":                         # 0.3 and 0.7 act as class 0, 1.2 and 1.9 as class 1
        return torch.tensor([0.0, 0.3, 0.7, 1.0, 1.2, 1.9])[torch.randint(0, 6, (rows,), generator=g)]
    return torch.randn(rows, generator=g)


def _step(engine, diffusion, graph, xt=None, offset=OFFSET, prepared=None, t=float(T)):
    """One step through the C entry with every output: (xt_out, pred, prob)."""
    c = _graph_case(graph)
    categorical = diffusion.startswith("categorical")
    eng = _engine(engine, 2 if categorical else 1)
    eng.use_gen_table = diffusion != "gaussian-ddim-no-table"
    tables = None
    if c["instances"] is not None:
        dev = eng.device
        tables = (torch.tensor(c["instances"][0], dtype=torch.int64, device=dev), torch.tensor(c["instances"][1], dtype=torch.int64, device=dev))
    xt = _xt(graph, diffusion).to(eng.device) if xt is None else xt
    return eng.step(c["g"], c["task"], _lib.CATEGORICAL if categorical else _lib.GAUSSIAN, xt, t, _post(diffusion), points=c["pts"],
                    xt_is_binary=diffusion == "categorical", seed=SEED, offset=offset, want_pred=True, want_prob=True, instances=tables,
                    prepared=prepared)


def _uniform(graph):
    """The uniforms the step draws on the device, in caller row order (tests/philox_reference.py)."""
    c = _graph_case(graph)
    if c["instances"] is not None:
        return torch.from_numpy(P.instance_uniform(c["instances"][0], c["instances"][1], OFFSET))
    return torch.from_numpy(P.uniform(SEED, OFFSET, c["rows"]))


@functools.lru_cache(maxsize=None)
def _oracle(hidden, agg, diffusion, graph, emulate_fp16x1=False):
    """(xt_out, pred, prob or None) of the CPU oracle for the step, segment family by segment family; ``emulate_fp16x1``: with the
    linears of the emulated fp16x1 network (tests/fp16x1_emulation.py through test_gpu_fp16x1.py)."""
    if emulate_fp16x1:
        from test_gpu_fp16x1 import _emulated
        return _emulated(lambda: _oracle.__wrapped__(hidden, agg, diffusion, graph))
    c = _graph_case(graph)
    categorical = diffusion.startswith("categorical")
    p = _params(hidden, 2 if categorical else 1)
    xt, u = _xt(graph, diffusion), _uniform(graph)
    outs, preds, probs = [], [], []
    for part in c["parts"]:
        kind, sl = part[0], part[-1]
        if kind == "tsp":
            args = (part[1], xt[sl], T, part[2], TARGET_T)
        elif kind == "dense":
            B, V = part[1].shape[:2]
            args = (part[1], xt[sl].reshape(B, V, V), T, None, TARGET_T)
        else:
            args = (xt[sl], T, part[1], TARGET_T)
        if categorical:
            fn = O.mis_categorical_denoise_step if kind == "mis" else O.tsp_categorical_denoise_step
            out, logits, prob = fn(p, O.CategoricalTables(), *args, uniform=u[sl], return_aux=True, aggregation=agg)
            if kind == "dense":
                logits = logits.permute(0, 2, 3, 1)
            preds.append(logits.reshape(-1, 2))
            probs.append(prob.reshape(-1))
        else:
            fn = O.mis_gaussian_denoise_step if kind == "mis" else O.tsp_gaussian_denoise_step
            out, pred = fn(p, O.GaussianTables(), *args, inference_trick="ddim", return_aux=True, aggregation=agg)
            preds.append(pred.reshape(-1))
        outs.append(out.reshape(-1))
    return torch.cat(outs), torch.cat(preds), torch.cat(probs) if categorical else None


def _assert_within_the_oracle_bound(engine, diffusion, graph, got):
    hidden, precision, _, _, agg = STEP_ENGINES[engine]
    out, pred, prob = (None if t is None else t.cpu() for t in got)
    ref_out, ref_pred, ref_prob = _oracle(hidden, agg, diffusion, graph)
    categorical = diffusion.startswith("categorical")
    if precision == "fp16x1":
        # test_gpu_fp16x1.py::_check_class: 2 d + 1e-5.  prob = c0 p0 + c1 p1 of softmax(logits) and the DDIM map have Lipschitz
        # constants below 1 in the prediction at t = 500 -> 450, so the same bound holds for them
        emu = _oracle(hidden, agg, diffusion, graph, True)[1]
        bound = 2 * (emu.double() - ref_pred.double()).abs().max().item() + 1e-5
    elif diffusion == "categorical" or precision == "bf16x3":
        bound = TOL
    else:
        bound = CLASS_TOL
    e_pred = (pred.reshape(ref_pred.shape) - ref_pred).abs().max().item() if ref_pred.numel() else 0.0
    what = f"{engine} {diffusion} {graph}"
    if categorical:
        e_prob = (prob - ref_prob).abs().max().item() if ref_prob.numel() else 0.0
        print(f"{what}: logits L_inf {e_pred:.2e}, prob L_inf {e_prob:.2e}, bound {bound:.1e}")
        assert e_pred < bound and e_prob < bound, (what, e_pred, e_prob, bound)
        safe = (_uniform(graph) - ref_prob).abs() > max(1e-5, e_prob)      # the band of test_gpu_parity.py
        assert torch.equal(out[safe], ref_out[safe]), what
        assert set(np.unique(out.numpy()).tolist()) <= {0.0, 1.0}
    else:
        e_out = (out - ref_out).abs().max().item() if ref_out.numel() else 0.0
        print(f"{what}: eps L_inf {e_pred:.2e}, x_s L_inf {e_out:.2e}, bound {bound:.1e}")
        assert e_pred < bound and e_out < bound, (what, e_pred, e_out, bound)


_ZEROS = {}


def _zeros_run(arena, engine, diffusion, graph):
    """The step on an all-zero workspace, once per module run: what every poisoned run must equal."""
    key = (engine, diffusion, graph)
    if key not in _ZEROS:
        eng = _engine(engine, 2 if diffusion.startswith("categorical") else 1)
        WP.give_to_engine(eng, arena)
        arena.set("zeros")
        _ZEROS[key] = _step(engine, diffusion, graph)
        torch.cuda.synchronize()
    return _ZEROS[key]


def _leave_residue(arena, task):
    """Another task on another engine, over random bytes: a MIS step of the unfused H = 64 engine before a TSP case, the fused TSP
    union step before a MIS case."""
    donor = ("fused-fp16x3", "categorical", "tsp-union-37-20") if task == _lib.TASK_MIS else ("unfused-h64", "gaussian-ddim", "mis-er60")
    WP.give_to_engine(_engine(donor[0], 2 if donor[1] == "categorical" else 1), arena)
    arena.set("random")
    _step(*donor)
    arena.set("residue", whole=False)


def _poisoned_step(arena, fill, engine, diffusion, graph, **kw):
    c = _graph_case(graph)
    eng = _engine(engine, 2 if diffusion.startswith("categorical") else 1)
    if fill == "residue":
        _leave_residue(arena, c["task"])
    else:
        arena.set(fill)
    WP.give_to_engine(eng, arena)
    ws = eng._workspace(c["g"])
    assert ws.data_ptr() == arena.buf.data_ptr()                     # the step below works in the arena
    got = _step(engine, diffusion, graph, **kw)
    torch.cuda.synchronize()
    need = _lib.lib().difusco_workspace_bytes(eng.hidden, eng.n_layers, c["g"].n_nodes, c["g"].n_edges, c["g"].n_segments)
    assert 0 < need <= arena.nbytes
    if fill != "residue":
        assert not arena.still_filled(need), "the step did not write its workspace"
    return got


@pytest.mark.parametrize("fill", WP.FILLS)
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("diffusion", DIFFUSIONS)
@pytest.mark.parametrize("engine", list(STEP_ENGINES))
def test_step_does_not_depend_on_the_workspace_contents(dev, arena, engine, diffusion, graph, fill):
    base = _zeros_run(arena, engine, diffusion, graph)
    if fill == "zeros":
        _assert_within_the_oracle_bound(engine, diffusion, graph, base)
        return
    got = _poisoned_step(arena, fill, engine, diffusion, graph)
    for a, b, name in zip(got, base, ("xt_out", "pred", "prob")):
        _same(a, b, f"{engine} {diffusion} {graph} {fill}: {name}")


CHAINS = [("fused-fp16x3", "categorical", "tsp-37-k7"), ("fused-fp16x3", "gaussian-ddim", "tsp-union-37-20"),
          ("fused-fp16x3-max", "categorical", "dense-b2-v14"), ("unfused-h64", "categorical", "tsp-37-k7"),
          ("fused-bf16x3", "categorical", "mis-er60"), ("unfused-h128", "gaussian-ddim", "mis-er60")]


def _chain(arena, engine, diffusion, graph, fill):
    """Three consecutive steps, x_t fed forward, Philox offsets OFFSET, OFFSET + 1, OFFSET + 2.  ``fill`` None: the workspace is
    zeroed once and then left alone, so every step sees its predecessor's residue; otherwise it is refilled before each step."""
    eng = _engine(engine, 2 if diffusion.startswith("categorical") else 1)
    WP.give_to_engine(eng, arena)
    arena.set("zeros")
    xt, outs = None, []
    for k in range(3):
        if fill is not None:
            torch.cuda.synchronize()
            arena.set(fill)
        out = _step(engine, diffusion, graph, xt=xt, offset=OFFSET + k, t=float(T - 50 * k))
        xt = out[0]
        outs.append(out)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("fill", WP.FILLS[:3])
@pytest.mark.parametrize("engine,diffusion,graph", CHAINS)
def test_chain_of_steps_refilled_before_each_equals_the_chain_left_alone(dev, arena, engine, diffusion, graph, fill):
    alone = _chain(arena, engine, diffusion, graph, None)
    again = _chain(arena, engine, diffusion, graph, fill)
    for k, (a, b) in enumerate(zip(again, alone)):
        for x, y, name in zip(a, b, ("xt_out", "pred", "prob")):
            _same(x, y, f"{engine} {diffusion} {graph} {fill}: step {k} {name}")
    assert not torch.equal(alone[0][0], alone[2][0])                 # (the chain moves)


@pytest.mark.parametrize("fill", WP.FILLS)
@pytest.mark.parametrize("graph", ["tsp-37-k7", "tsp-union-37-20", "dense-b2-v14"])
@pytest.mark.parametrize("diffusion", ["categorical", "gaussian-ddim"])
@pytest.mark.parametrize("engine", ["fused-fp16x3", "fused-bf16x3", "fused-fp16x1", "fused-fp16x3-mean"])
def test_prepared_step_does_not_depend_on_the_workspace_contents(dev, arena, engine, diffusion, graph, fill):
    """``prepare_times``, then ``prepare``, then the workspace is poisoned, then the step: the bits of the unprepared step.
    include/difusco_hip.h at ``difusco_prepare``: "difusco_prepare(): fills it from args->{hidden, n_layers, out_channels, task
    (TSP), weights, precision, n_nodes, n_edges, points, workspace, stream}" and, at ``difusco_step_args.prepared``, "what does not
    depend on x_t or t is then computed ONCE and handed back in": the PREPARED buffer and the time-bias rows carry state between
    calls and are left alone; the workspace is scratch of ``difusco_prepare`` and of the step alike, and is what is poisoned - once
    before ``prepare`` and again between ``prepare`` and the step."""
    base = _zeros_run(arena, engine, diffusion, graph)
    c = _graph_case(graph)
    eng = _engine(engine, 2 if diffusion == "categorical" else 1)
    WP.give_to_engine(eng, arena)
    eng._tbias.clear()
    try:
        eng.prepare_times([T])
        arena.set("random" if fill == "residue" else fill)
        prepared = eng.prepare(c["g"], c["pts"])
        assert prepared is not None and eng._workspace(c["g"]).data_ptr() == arena.buf.data_ptr()
        torch.cuda.synchronize()
        got = _step(engine, diffusion, graph, prepared=prepared) if fill == "zeros" else \
            _poisoned_step(arena, fill, engine, diffusion, graph, prepared=prepared)
        torch.cuda.synchronize()
    finally:
        eng._tbias.clear()
    for a, b, name in zip(got, base, ("xt_out", "pred", "prob")):
        _same(a, b, f"prepared {engine} {diffusion} {graph} {fill}: {name}")


@pytest.mark.parametrize("diffusion", ["categorical", "gaussian"])
def test_graphed_sampling_with_a_poisoned_capture_workspace(dev, arena, diffusion):
    """A captured loop (test_gpu_graphed_sampling.py's twins): the capture stream's workspace - whose address the captured launches
    hold - is refilled between the replays; every replay equals the eager loop at the same call counter."""
    from test_gpu_graphed_sampling import _gen, _tsp, _twins
    g_m, e_m = _twins("TSPModel", diffusion, dev, L=3, steps=4, sparse_factor=7)
    pts, ei = _tsp(dev, 37, 7, seed=4)
    x0 = torch.randn(ei.shape[1], generator=_gen(dev, 3), device=dev)
    _same(g_m.sample(pts, ei, xt0=x0, graphed=True), e_m.sample(pts, ei, xt0=x0), "capture call")
    ws = g_m.model._ws[g_m._capture_stream.cuda_stream]
    need = _lib.lib().difusco_workspace_bytes(256, 3, 37, 259, 1)
    assert ws.numel() >= need > 0
    pattern = torch.from_numpy(np.random.default_rng(7).integers(0, 256, ws.numel(), dtype=np.uint8)).to(dev)
    for fill in WP.FILLS[:3]:
        torch.cuda.synchronize()
        if fill == "random":
            ws.copy_(pattern)
        else:
            ws.fill_(0 if fill == "zeros" else 0xFF)
        torch.cuda.synchronize()
        a = g_m.sample(pts, ei, xt0=x0, graphed=True)
        torch.cuda.synchronize()
        assert ws.data_ptr() == g_m.model._ws[g_m._capture_stream.cuda_stream].data_ptr()
        assert bool((ws[:need] != (pattern[:need] if fill == "random" else (0 if fill == "zeros" else 0xFF))).any())
        _same(a, e_m.sample(pts, ei, xt0=x0), f"replay over {fill}")
    assert g_m.graph_captures == 1 and g_m.graph_replays == 3


@pytest.mark.parametrize("fill", ["random", "residue"])
@pytest.mark.parametrize("prec", ["fp16x3", "bf16x3"])
def test_standalone_fused_layer_with_other_scratch_contents(dev, arena, prec, fill):
    """``difusco_edge_layer_fused_ex`` on the zoo graph whose rows straddle tiles: test_gpu_graph_structure.py runs it on 0xFF
    scratch and holds that result to float64; random bytes, and what the layer on the larger ``hub_first`` graph left, give the
    same bits."""
    import graph_zoo as Z
    import test_gpu_graph_structure as S
    from difusco_amd import graph

    def run(name, agg, toe, rg, scratch_of):
        st = S._graph(name)
        n, E = len(st["deg"]), len(st["col"])
        inp = S._inputs(name, "random", 0)
        x = S._dev_inputs(inp, dev, True)
        rp, row, col = S._csr_dev(st, dev)
        e_d, h_d = x["e"].clone(), x["h"].clone()
        nbytes = _lib.lib().difusco_fused_scratch_bytes(n, E)
        scratch = scratch_of(nbytes)
        _lib.check(_lib.lib().difusco_edge_layer_fused_ex(
            _lib.PRECISIONS[prec], n, E, S._p(rp), S._p(row), S._p(col), S._p(x["node4"]), S._p(e_d), S._p(h_d), S._p(x["pc"]),
            S._p(x["po"]), S._p(x["bc"]), *[S._p(t) for t in x["prm"]], S._p(x["bo"]), S._p(x["tb"]), toe, S._p(x["sc"]),
            S._p(scratch), S.AGG_ID[agg], rg, S._stream()))
        torch.cuda.synchronize()
        return graph.from_tiled(e_d, (E + 255) // 256 * 256).cpu(), h_d.cpu()

    st = S._graph("straddle")
    n, E = len(st["deg"]), len(st["col"])
    for agg in Z.AGGS:
        for toe in (1, 0):
            for rg in ((0,) if agg == "max" else (0, 1)):
                want_e, want_h, want_pad = S._run_fused(_lib, dev, prec, S._inputs("straddle", "random", 0), S._csr_dev(st, dev), n, E,
                                                        agg, toe, rg)
                if fill == "residue":
                    arena.set("random")
                    run("hub_first", agg, toe, rg, arena.take)
                    arena.set("residue", whole=False)
                else:
                    arena.set(fill)
                e, h = run("straddle", agg, toe, rg, arena.take)
                arena.check_used(calls=1)
                what = f"{prec} {agg} toe={toe} reg_gather={rg} {fill}"
                _same(e[:E], want_e, what + " e")
                _same(h, want_h, what + " h")
                assert not bool(e[E:].any()), what + ": pad rows of e are not zero"


# =========================================== decode, search, MIS and graph entries ===============================================
@functools.lru_cache(maxsize=None)
def _golden(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


def _equal_runs(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k] == want[k], (what, k)


@functools.lru_cache(maxsize=None)
def _big_groups():
    """Five groups with more and longer tours than any asserted case of the TSP search entries, for the residue fill: what they
    leave in the arena is all that matters, their results are not looked at."""
    rng = np.random.default_rng(4242)
    sizes, counts = (50, 197, 300, 64, 1100), (4, 2, 3, 5, 1)
    pts = [rng.random((n, 2)) for n in sizes]
    starts = [np.stack([np.concatenate([[0], rng.permutation(n - 1) + 1, [0]]) for _ in range(P)]) for n, P in zip(sizes, counts)]
    total = sum(counts)
    return pts, starts, [100 + t for t in range(total)], [(1 << 62) + (t << 32) for t in range(total)]


def _big_lists(K):
    """Neighbour lists of the big groups: the K nearest other cities."""
    out = []
    for p in _big_groups()[0]:
        d = np.linalg.norm(p[:, None] - p[None], axis=-1)
        out.append(np.ascontiguousarray(np.argsort(d, axis=1, kind="stable")[:, 1:K + 1].astype(np.int32)))
    return out


# ---- single-move 2-opt: tests/two_opt_entries_cases.py against tests/golden/two_opt_entries.json
def _two_opt(entry, shape, cap):
    import two_opt_entries_cases as C

    def run(dev):
        rec = _golden("two_opt_entries.json")
        _equal_runs(C.short_run(dev, rec["inputs"], entry, shape, cap), rec["runs"][C.run_name(entry, shape, cap)], C.run_name(entry, shape, cap))
        return len(C.groups_of(shape)) if entry in ("plain", "screened") else 1      # those two take one group per call
    return run


# ---- resident searches: tests/resident_entries_cases.py against tests/golden/resident_entries.json
def _resident(entry, call, cap, per_launch, variant):
    import resident_entries_cases as C

    def run(dev):
        rec = _golden("resident_entries.json")
        name = C.run_name(entry, C.CALLS.index(call), cap, per_launch, variant)
        _equal_runs(C.short_run(dev, rec["inputs"], entry, C.CALLS.index(call), cap, per_launch, variant), C.recorded_run(rec, name), name)
        return 1
    return run


def _local_search_launched(call, cap, rounds):
    """``difusco_tsp_local_search_ragged`` (the launched 2-opt + Or-opt search, which the resident one must equal) on the groups of
    the resident fixture, against the numpy restatement of the rule."""
    import resident_entries_cases as C

    def run(dev):
        from difusco_amd import decode
        inputs, idx = _golden("resident_entries.json")["inputs"], C.CALLS.index(call)
        groups = C.group_arrays(inputs, idx)
        stats = {}
        tours, two = decode.batched_local_search_ragged([p for p, _ in groups], [t for _, t in groups], max_iterations=cap, device=dev,
                                                        max_rounds=rounds, stats=stats)
        got = {"tours": [np.asarray(t).tolist() for t in tours], "two_opt_iterations": np.asarray(two).tolist(),
               "or_opt_iterations": np.asarray(stats["or_opt_iterations"]).tolist(), "rounds": np.asarray(stats["rounds"]).tolist()}
        _equal_runs(got, C.emulated_run(inputs, "local_search", idx, cap, rounds), f"local_search_ragged {call} cap {cap}")
        return 1
    return run


# ---- multi-move entries: tests/multi_move_entries_cases.py against tests/golden/multi_move_entries.json
def _multi_move(*run_args):
    import multi_move_entries_cases as C

    def run(dev):
        rec = _golden("multi_move_entries.json")
        _equal_runs(C.short_run(dev, rec["inputs"], *run_args), rec["runs"][C.run_name(*run_args)], C.run_name(*run_args))
        return 1
    return run


# ---- the four multi-move search entries: tests/tsp_search_entries_cases.py against tests/golden/tsp_search_entries.json
def _search(mode, kicks, cap):
    import tsp_search_entries_cases as C

    def run(dev):
        rec = _golden("tsp_search_entries.json")
        _equal_runs(C.short_run(dev, rec["inputs"], mode, kicks, cap), rec["runs"][C.run_name(mode, kicks, cap)], C.run_name(mode, kicks, cap))
        if mode == "plain":      # the plain run makes an iterated call of keeps only first; with a cap of 0 sweeps it returns unmoved
            return 2, cap > 0    # tours before it touches the device
        return 1
    return run


def _big(fn_name, **kw):
    """The residue donor of a TSP search entry: its ragged wrapper on the big groups."""
    def run(dev):
        from difusco_amd import decode
        pts, starts, seeds, offsets = _big_groups()
        extra = dict(kw)
        if extra.pop("keys", False):
            extra.update(seeds=seeds, offsets=offsets)
        if "K" in extra:
            extra["neighbors"] = _big_lists(extra.pop("K"))
        if extra.pop("heat", False):
            import tsp_heat_kick_emulation as H
            from tsp_kopt_search_cases import edge_index_of
            csr = [H.knn_csr(p, 8) for p in pts]
            rng = np.random.default_rng(5)
            extra["heat"] = [rng.random((len(s), len(c[1]))).astype(np.float32) for s, c in zip(starts, csr)]
            extra["edge_index"] = [edge_index_of(*c) for c in csr]
        getattr(decode, fn_name)(pts, starts, 50, device=dev, **extra)
        return 1
    return run


# ---- the sampled k-opt search: tests/tsp_kopt_search_cases.py (the emulation's result of every case)
def _kopt(name):
    def run(dev):
        import tsp_kopt_search_cases as C
        from test_gpu_tsp_kopt_search import ragged, same
        groups, kw = C.cases()[name]
        tours, per = ragged(dev, groups, kw)
        first = 0
        for t, w in zip(tours, C.expected(name)[0]):
            same(t, per, first, w)
            first += len(t)
        return 1
    return run


# ---- the windowed search: tests/tsp_window_search_emulation.py through the instances of test_gpu_tsp_window_search.py
def _window_solo(name, n, window, passes, kicks, **kw):
    def run(dev):
        from test_gpu_tsp_window_search import solo
        solo(dev, name, n, window, passes, kicks, **kw)
        return 1
    return run


def _window_ragged(dev):
    """Three groups of different sizes in one call, every tour against the emulation."""
    from difusco_amd.decode import batched_window_search_ragged
    from test_gpu_tsp_window_search import OFFSET as W_OFFSET, SEED as W_SEED, instance, reference, same_tour
    groups = [("uniform", 197), ("lattice", 197), ("uniform", 100)]
    inst = [instance(*g) for g in groups]
    per = {}
    tours, _ = batched_window_search_ragged([p for p, _ in inst], [s[None] for _, s in inst], 200, dev, select_rounds=4, kicks=3,
                                            kick_size=2, span=5, seeds=[W_SEED] * 3, offsets=[W_OFFSET] * 3, stats=per, window=64, passes=2)
    for b, (name, n) in enumerate(groups):
        same_tour(tours[b][0], per, b, reference(name, n, W_SEED, W_OFFSET, 64, 2, 3, 2, 5, 200, 4))
    return 1


# ---- focused and heat-biased descents: their emulations through the groups of the two GPU test files
def _focused(n, P, kicks):
    def run(dev):
        from test_gpu_tsp_focused_search import SELECT_PATHS, _solo, group
        pts, starts, seeds, offsets, want = group(n, P, kicks)
        _solo(dev, pts, starts, want, kicks=kicks, kick_size=4, span=16, seeds=seeds, offsets=offsets)
        return len(SELECT_PATHS)
    return run


def _heat_kick(n, P, kicks, descent):
    def run(dev):
        import test_gpu_tsp_heat_kick as T
        g = T.group(n, P, kicks, descent)
        tours, stats, per = T.solo(dev, g, kicks, descent)
        T._same(tours, {k: [v] for k, v in stats.items()}, per, 0, 0, g[6], descent == "focused")
        return 1
    return run


# ---- merge: tests/tsp_merge_cases.py (the reference walk of every case)
def _merge_tours(structure, kind):
    def run(dev):
        import tsp_merge_cases as Z
        from test_gpu_merge_batch import _existing
        c = Z.case(structure, kind)
        tour, iterations, completed = c["want"]
        tours, its, done = _existing(dev, c["points"], c["edge_index"], c["heat"][None])
        assert (tours, done) == ([tour], [completed]), (structure, kind)
        if completed and c["info"]["tie_free"]:
            assert its == [iterations], (structure, kind)
        return 1
    return run


MERGE_RAGGED = ("knn_5_full", "knn_33_k8", "pair_33_k8_perm", "knn_65_full", "trio_33_k8", "knn_129_k8")      # four different sizes
MERGE_KINDS = ("base", "all_nan", "inf_edges")
MERGE_DENSE = (("pair_33_dense", "coincident_zero"), ("dense_33", "nan_edges"), ("pair_33_dense", "coincident_negative"))


def _merge_batch(state, dense, structures=MERGE_RAGGED):
    def run(dev):
        import tsp_merge_cases as Z
        from difusco_amd.decode import merge_tours_batch
        if dense:
            cases = [[Z.case(*p)] for p in MERGE_DENSE]
            heats = [c[0]["heat"].reshape(1, 33, 33) for c in cases]
            res = merge_tours_batch(heats, [c[0]["points"] for c in cases], None, sparse_graph=False, parallel_sampling=1, device=dev,
                                    return_completed=True, state=state)
        else:
            cases = [[Z.case(s, k) for k in MERGE_KINDS] for s in structures]
            res = merge_tours_batch([np.stack([c["heat"] for c in cs]) for cs in cases], [cs[0]["points"] for cs in cases],
                                    [cs[0]["edge_index"] for cs in cases], sparse_graph=True, parallel_sampling=len(MERGE_KINDS),
                                    device=dev, return_completed=True, state=state)
        for cs, (tours, it, done) in zip(cases, res):
            assert tours == [c["want"][0] for c in cs] and done == [c["want"][2] for c in cs]
            if all(c["want"][2] and c["info"]["tie_free"] for c in cs):
                assert it == float(np.mean([c["want"][1] for c in cs]))
        return 1
    return run


# ---- MIS: tests/mis_decode_cases.py and the emulations behind the three search test files
def _mis_decode(structure, kind):
    def run(dev):
        import mis_decode_cases as Z
        from test_gpu_mis_decode_zoo import _decode
        c = Z.case(structure, kind)
        assert np.array_equal(_decode(dev, c["scores"], c["lmax"], edge_index=c["edge_index"]), c["want"])
        return 1
    return run


def _mis_local(name, start, cap=None):
    def run(dev):
        from test_gpu_mis_local_search import _same as same, _thinned
        from test_mis_local_search_host import fixture
        ei, scores, decoded = fixture(name)
        n = len(scores)
        same(dev, n, ei, scores, {"decoded": decoded, "empty": np.zeros(n, dtype=int), "thinned": _thinned(decoded)}[start], cap)
        return 1
    return run


def _mis_iterated(mode, name, start, kicks, kick_size=4, cap=1000):
    def run(dev):
        from test_gpu_mis_iterated_search import SEEDS, _reference, _same as launched
        from test_gpu_mis_resident_search import _same as resident
        from test_mis_local_search_host import fixture
        ei, scores, decoded = fixture(name)
        s = decoded if start == "decoded" else np.zeros(len(scores), dtype=int)
        want = _reference(name, start, kicks, kick_size, cap)
        if mode == "launches":
            launched(dev, len(scores), ei, scores, s, seeds=[SEEDS[name]], kicks=kicks, kick_size=kick_size, cap=cap, want=want)
            return 1
        resident(dev, len(scores), ei, scores, s, seeds=[SEEDS[name]], kicks=kicks, kick_size=kick_size, cap=cap, want=want)
        return 2                                                     # (the resident helper also runs the launched search)
    return run


def _mis_union(mode):
    """Two fixtures and an empty instance between them, three keys, the third offset wrapping 2^64."""
    def run(dev):
        from test_gpu_mis_iterated_search import _same as launched
        from test_gpu_mis_resident_search import _same as resident
        from test_mis_iterated_search_host import union_of
        from test_mis_local_search_host import fixture
        graphs = [(fixture(name)[0], fixture(name)[1]) for name in ("mis_decode_n60_p15", "mis_decode_n300_p05")]
        n, union, scores, rows = union_of(graphs, empty_after=0)
        assert rows == [0, 60, 60, 360]
        (launched if mode == "launches" else resident)(dev, n, union, scores, np.zeros(n, dtype=int), rows=rows, seeds=[1, 2, 3],
                                                       offsets=[0, 5, 2 ** 64 - 3], kicks=6)
        return 1 if mode == "launches" else 2
    return run


# entry -> (the residue donor: a larger case of the same entry, the asserted cases).  Every case runs more than one sweep or round.
_U = ("plain", "screened", "grouped", "grouped_screened")
DECODE = {f"two_opt_{e}": (_two_opt(e, 1025, 1000), [_two_opt(e, 17, 1000), _two_opt(e, 17, 3), _two_opt(e, 4, 1000)]) for e in _U}
DECODE["two_opt_grouped_screened"][1].append(_two_opt("grouped_screened", "17_scaled", 1000))
DECODE.update({f"two_opt_{e}": (_two_opt(e, 1025, 1000), [_two_opt(e, "mixed", 1000), _two_opt(e, 17, 1000), _two_opt(e, "mixed", 3)])
               for e in ("ragged_exact", "ragged_screened")})
_R3 = ("n4x20", "poly7", "n33x3")
DECODE.update({
    "two_opt_resident": (_resident("two_opt", ("n43x5",), 1000, 1, "exact"),
                         [_resident("two_opt", _R3, 1000, 1, "exact"), _resident("two_opt", _R3, 1000, 0, "screened"),
                          _resident("two_opt", ("n33x3", "tiny33"), 1000, 2, "screened"), _resident("two_opt", ("n65",), 3, 1, "exact")]),
    "local_search_resident": (_resident("local_search", ("n43x5",), 1000, 1, 16),
                              [_resident("local_search", _R3, 1000, 1, 16), _resident("local_search", _R3, 1000, 0, 16),
                               _resident("local_search", ("n65",), 1000, 2, 16), _resident("local_search", ("n33x3",), 3, 1, 1)]),
    "local_search_ragged": (_local_search_launched(("n43x5",), 1000, 16),
                            [_local_search_launched(_R3, 1000, 16), _local_search_launched(("n65",), 1000, 16),
                             _local_search_launched(("n33x3",), 3, 1)]),
    "multi_two_opt_ragged": (_big("batched_multi_two_opt_ragged"),
                             [_multi_move("multi_two_opt", None, None, 1000, None, 4), _multi_move("multi_two_opt", None, None, 1000, None, 1),
                              _multi_move("multi_two_opt", None, None, 2, None, 4)]),
    "nbr_two_opt_ragged": (_big("batched_nbr_two_opt_ragged", K=5),
                           [_multi_move("nbr_two_opt", 3, 1, 1000, None, 4), _multi_move("nbr_two_opt", 3, 0, 1000, None, 4),
                            _multi_move("nbr_two_opt", 1, 1, 2, None, 4), _multi_move("nbr_two_opt", 3, 1, 1000, None, 1)]),
    "nbr_local_search_ragged": (_big("batched_nbr_local_search_ragged", K=5),
                                [_multi_move("nbr_local_search", 3, 1, 1000, 16, 4), _multi_move("nbr_local_search", 3, 0, 1000, 16, 4),
                                 _multi_move("nbr_local_search", 1, 1, 2, 16, 4), _multi_move("nbr_local_search", 3, 1, 1000, 16, 1)]),
    "multi_local_search_ragged": (_big("batched_multi_local_search_ragged"), [_search("plain", None, 1000), _search("plain", None, 0)]),
    "iterated_search_ragged": (_big("batched_iterated_search_ragged", kicks=2, keys=True),
                               [_search("iterated_full", 3, 1000), _search("iterated_full", 3, 0), _search("iterated_full", 0, 1000)]),
    "focused_search_ragged": (_big("batched_iterated_search_ragged", kicks=2, keys=True, descent="focused"),
                              [_search("iterated_focused", 3, 1000), _search("iterated_focused", 3, 0), _focused(33, 3, 7), _focused(65, 3, 1)]),
    "guided_search_ragged": (_big("batched_iterated_search_ragged", kicks=2, keys=True, kick_bias="heat", heat=True),
                             [_search("guided_full", 3, 1000), _search("guided_focused", 3, 1000), _heat_kick(33, 3, 7, "full"),
                              _heat_kick(65, 3, 7, "focused")]),
    "kopt_search_ragged": (_kopt("ladder-n200"), [_kopt("stall"), _kopt("corners"), _kopt("ladder-n7")]),
    "window_search_ragged": (_big("batched_window_search_ragged", kicks=2, keys=True, window=64, passes=2, kick_size=2, span=5),
                             [_window_ragged, _window_solo("uniform", 197, 64, 2, 3), _window_solo("lattice", 197, 64, 2, 3, cap=3)]),
    "tsp_merge_tours": (_merge_tours("knn_129_k8", "subnormal"),
                        [_merge_tours("knn_65_k8_perm", "nan_edges"), _merge_tours("pair_33_k8", "base"), _merge_tours("dense_33", "nan_edges"),
                         _merge_tours("knn_5_full", "base")]),
    "tsp_merge_batch_auto": (_merge_batch("auto", False), [_merge_batch("auto", False, MERGE_RAGGED[:3]), _merge_batch("auto", True)]),
    "tsp_merge_batch_global": (_merge_batch("global", False), [_merge_batch("global", False, MERGE_RAGGED[:3]), _merge_batch("global", True)]),
    "mis_decode": (_mis_decode("sparse_4097", "with_nan"),
                   [_mis_decode("path_1000", "increasing_id"), _mis_decode("union_40", "two_level"), _mis_decode("star_129_dec", "two_level")]),
    "mis_local_search": (_mis_local("mis_decode_n750_p15", "decoded"),
                         [_mis_local("mis_decode_n300_p05", "empty"), _mis_local("mis_decode_n60_p15", "thinned"),
                          _mis_local("mis_decode_n300_p05", "thinned", 1)]),
    "mis_iterated_search": (_mis_iterated("launches", "mis_decode_n750_p15", "decoded", 20),
                            [_mis_iterated("launches", "mis_decode_n300_p05", "empty", 8), _mis_union("launches"),
                             _mis_iterated("launches", "mis_decode_n60_p15", "decoded", 20, 1, 1)]),
    "mis_resident_search": (_mis_iterated("resident", "mis_decode_n750_p15", "decoded", 20),
                            [_mis_iterated("resident", "mis_decode_n300_p05", "empty", 8), _mis_union("resident"),
                             _mis_iterated("resident", "mis_decode_n60_p15", "decoded", 20, 1, 1)]),
})


@pytest.mark.parametrize("fill", WP.FILLS)
@pytest.mark.parametrize("entry", list(DECODE))
def test_decode_entry_does_not_depend_on_the_workspace_contents(dev, arena, monkeypatch, entry, fill):
    """Every case equals its own expectation (fixture or numpy restatement), whatever its workspace held.  ``residue``: the donor, a
    larger case of the same entry, runs first over random bytes; the cases then run one after the other without a refill."""
    WP.patch_decode(monkeypatch, arena)
    donor, cases = DECODE[entry]
    if fill == "residue":
        arena.set("random")
        donor(dev)
        arena.check_used()
        arena.set("residue", whole=False)
    else:
        arena.set(fill)
    sizes = []
    for run in cases:
        arena.calls = []
        calls = run(dev)
        calls, written = calls if isinstance(calls, tuple) else (calls, True)
        arena.check_used(calls=calls, written=written)
        sizes += arena.calls
    print(f"{entry} {fill}: workspace bytes per call {sizes}")
    # (no case here is so small that its entry reports 0 bytes: the resident entries take 512 bytes for their group table and state)
    assert min(sizes) > 0, "a call of the entry reported a workspace of 0 bytes: no poison was in play there"


# ---- the device graph build: tests/graph_build_emulation.py, against the host build
def _graph_build_cases(dev):
    import graph_build_emulation as G
    from test_gpu_graph_build import _both, _same_graph
    from difusco_amd.graph import build_union_csr

    def union():
        eis, ns, pts = G.tsp_union_case()
        eis_d = [torch.from_numpy(e).to(dev) for e in eis]
        gh, uh, rh = build_union_csr(eis_d, ns, dev, points=torch.from_numpy(pts))
        gd, ud, rd = build_union_csr(eis_d, ns, dev, points=torch.from_numpy(pts).to(dev), method="device")
        _same_graph(gd, gh)
        assert gd.n_segments == 3 and np.array_equal(rd, rh) and torch.equal(ud.cpu(), uh.cpu())

    def single(n, k, seed, points):
        pts = G.tsp_points(n, seed)
        g, _ = _both(dev, G.numpy_knn(pts, k), n, pts if points else None)
        assert (g.node_order is not None) == points
    return (lambda: single(2000, 100, 2000, True)), [union, lambda: single(65, 8, 65, True), lambda: single(45, 7, 9, False)]


@pytest.mark.parametrize("fill", WP.FILLS)
def test_graph_build_does_not_depend_on_the_workspace_contents(dev, arena, monkeypatch, fill):
    """``difusco_graph_build`` through ``build_csr(method="device")``: a union of three instances and a graph with points (Morton
    order), and one without, equal the host build in every field."""
    WP.patch_graph(monkeypatch, arena)
    donor, cases = _graph_build_cases(dev)
    if fill == "residue":
        arena.set("random")
        donor()
        arena.check_used(calls=1)
        arena.set("residue", whole=False)
    else:
        arena.set(fill)
    for run in cases:
        arena.calls = []
        run()
        arena.check_used(calls=1)                                    # the device build; the host build takes no workspace


@functools.lru_cache(maxsize=None)
def _knn_brute_force(n, k, seed):
    """(points float64 [n, 2], neighbours int64 [n, k]) of a chunked float64 brute force: (dx dx) + (dy dy) as numpy evaluates it -
    two rounded products and one rounded sum, no fused multiply-add -, the k smallest by (distance, index)."""
    pts = np.random.default_rng(seed).random((n, 2))
    out = np.empty((n, k), dtype=np.int64)
    for lo in range(0, n, 1000):
        hi = min(n, lo + 1000)
        dx, dy = pts[lo:hi, None, 0] - pts[None, :, 0], pts[lo:hi, None, 1] - pts[None, :, 1]
        d = dx * dx + dy * dy
        cand = np.argpartition(d, k + 8, axis=1)[:, :k + 9]          # the k-th distance is inside the first k + 9 of the partition
        cd = np.take_along_axis(d, cand, axis=1)
        order = np.lexsort((cand, cd), axis=1)[:, :k]
        out[lo:hi] = np.take_along_axis(cand, order, axis=1)
        kth = np.take_along_axis(cd, order[:, -1:], axis=1)
        assert ((d <= kth).sum(axis=1) == k).all()                   # no tie at the k-th distance: the selection is unambiguous
    return pts, out


@pytest.mark.parametrize("fill", WP.FILLS[:3])
def test_knn_graph_does_not_depend_on_the_workspace_contents(dev, monkeypatch, fill):
    """``difusco_knn_graph``.  n = 300 keeps its distance keys in LDS: 256 bytes of workspace are asked for and none is written,
    which is shown.  n = 16001 is past the 16000 points that fit LDS: every block keeps its keys in the workspace
    (1024 x n x 8 bytes)."""
    from difusco_amd.graph import knn_edge_index_gpu
    k = 8
    big = ctypes.c_size_t()
    _lib.check(_lib.lib().difusco_knn_graph_workspace_bytes(16001, k, ctypes.byref(big)))
    assert big.value == 1024 * 16001 * 8
    arena = WP.Arena(dev, big.value)
    WP.patch_graph(monkeypatch, arena)
    for n in (300, 16001):
        pts, want = _knn_brute_force(n, k, n)
        arena.set(fill)
        ei = knn_edge_index_gpu(pts, k, device=dev)
        torch.cuda.synchronize()
        assert len(arena.calls) == 1
        if n == 300:
            assert arena.calls == [256] and arena.still_filled(256)  # the LDS path leaves its workspace alone
        else:
            assert arena.calls == [big.value] and not arena.still_filled(big.value)
        ei = ei.cpu().numpy()
        assert np.array_equal(ei[0], np.repeat(np.arange(n), k)) and np.array_equal(ei[1].reshape(n, k), want)
        assert np.array_equal(want[:, 0], np.arange(n))              # self first


def test_knn_graph_on_the_residue_of_a_larger_call(dev, monkeypatch):
    """n = 16001 over what n = 16500 left in the same bytes."""
    from difusco_amd.graph import knn_edge_index_gpu
    k = 8
    arena = WP.Arena(dev, 1024 * 16500 * 8)
    WP.patch_graph(monkeypatch, arena)
    arena.set("random")
    knn_edge_index_gpu(np.random.default_rng(3).random((16500, 2)), k, device=dev)
    arena.check_used(calls=1)
    arena.set("residue", whole=False)
    pts, want = _knn_brute_force(16001, k, 16001)
    ei = knn_edge_index_gpu(pts, k, device=dev).cpu().numpy()
    assert arena.calls == [1024 * 16001 * 8]
    assert np.array_equal(ei[0], np.repeat(np.arange(16001), k)) and np.array_equal(ei[1].reshape(16001, k), want)


@pytest.mark.parametrize("fill", WP.FILLS)
def test_mcts_heatmap_does_not_depend_on_the_workspace_contents(dev, arena, monkeypatch, golden_dir, tmp_path, fill):
    """``difusco_mcts_heatmap_prepare`` then ``difusco_mcts_heatmap_rows`` on the smallest fixture, seven rows per ``rows`` call: the
    workspace is poisoned BEFORE ``prepare`` and then left alone - it carries the prepared state (threshold, row top 3, transposed
    entries) into every ``rows`` call.  The text equals what the reference's converter wrote, the rows the host numpy sweeps."""
    from difusco_amd import formats
    WP.patch_graph(monkeypatch, arena)
    z = np.load(os.path.join(golden_dir, "mcts_text_n30.npz"))
    n, prob = int(z["num_nodes"]), float(z["expected_valid_prob"])
    if fill == "residue":
        big = np.load(os.path.join(golden_dir, "mcts_text_n64.npz"))
        arena.set("random")
        formats.write_mcts_heatmap(big["heat"], big["points"], int(big["num_nodes"]), str(tmp_path / "donor"), 0,
                                   expected_valid_prob=float(big["expected_valid_prob"]),
                                   edge_index=big["edge_index"] if "edge_index" in big.files else None, use_gpu=True)
        arena.check_used(calls=1)
        arena.set("residue", whole=False)
    else:
        arena.set(fill)
    ei = z["edge_index"] if "edge_index" in z.files else None
    path = formats.write_mcts_heatmap(z["heat"], z["points"], n, str(tmp_path), 0, expected_valid_prob=prob, edge_index=ei,
                                      block_rows=7, use_gpu=True)
    arena.check_used(calls=1)
    assert open(path).read() == bytes(z["text"]).decode()
    heat, ei = (z["heat"], ei) if ei is not None else formats.sparsify(z["heat"].astype(np.float32, copy=False))
    host = np.stack(list(formats.mcts_heatmap_rows(heat, ei, z["points"], n, prob)))
    arena.calls = []
    got = np.stack(list(formats.mcts_heatmap_rows_gpu(heat, ei, z["points"], n, prob, block_rows=7, device=dev)))
    arena.check_used(calls=1)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), host.view(np.uint32))
