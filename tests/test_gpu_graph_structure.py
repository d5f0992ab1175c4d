"""The neighbour aggregation on adversarial graph structures (``-m gpu``).

The fused edge layer cuts the CSR edge list into 32-edge tiles and hands the per-node pieces of the neighbour sum from
``edge_layer_fused_kernel`` to ``node_finalize_kernel`` through part[tile][0|1] / direct[node]; which place holds which piece is
decided by where a row starts and ends relative to the tiles.  tests/graph_zoo.py holds graphs, defined by degree sequences, that
reach every case of that protocol (tests/test_graph_zoo_host.py asserts it, and that the inputs used here are sensitive enough: one
lost hub edge moves the float64 reference by 50 - 100 x the bound asserted).

Part 1 compares ONE layer (difusco_edge_layer_fused_ex / difusco_edge_gate_aggregate_ex) with a float64 torch evaluation, row by
row, and names the protocol case of the worst row when it fails.  A whole step cannot see a lost edge: with one hub edge dropped
from the reference the logits of a 3-layer step move by 2e-5 .. 7e-5 (sum), 7e-5 (mean), 0.0 (max) - at or below the step bounds.
Part 2 runs whole MIS / TSP steps on the same graphs against the oracle, at the bounds the suite already uses for steps.

Bounds.  Random inputs on graphs without a hub: what test_gpu_parity.py::test_edge_layer_fused / ::test_edge_gate_aggregate and
test_gpu_fp16x1.py::test_edge_layer_fused_fp16x1 assert.  Marker inputs and hubs (other magnitudes, sums of up to 1000 terms): the
calibration rule of test_gpu_round6.py - max(that bound, 4 x d32), d32 = distance of a plain fp32 torch evaluation of the same
layer from the float64 one, computed here from the reference alone.  Every case prints d32 and the observed errors
(profiles/graph_structure/ keeps one run).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import difusco_oracle as O
from tests import fp16x1_emulation as EMU
from tests import graph_zoo as Z

pytestmark = pytest.mark.gpu

TOL = 1e-4          # north_star's bound (bf16x3 steps)
CLASS_TOL = 1e-5    # the default engine's class (fp16x3 steps)
LAYER_GRAPHS = [n for n in Z.ZOO if n != "no_edges"]      # (E = 0: nothing for a layer entry to do; the step test runs it)
AGG_ID = {"sum": 0, "mean": 1, "max": 2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from difusco_amd import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- shared per-graph state (one graph at a time: the float64 references of the larger graphs are tens of MB) --------------------------
_STATE = {"name": None}


def _graph(name):
    if _STATE["name"] != name:
        from difusco_amd import graph
        _STATE.clear()
        deg, ei = Z.zoo_graph(name)
        rowptr, col, row, perm, ident = graph.csr_from_coo_host(ei, len(deg))
        assert ident
        _STATE.update(name=name, deg=deg, ei=ei, rowptr=rowptr, col=col, row=row, inputs={}, refs={})
    return _STATE


def _inputs(name, kind, phase, hidden=256):
    st = _graph(name)
    key = (kind, phase, hidden)
    if key not in st["inputs"]:
        st["inputs"][key] = Z.layer_inputs(st["ei"], len(st["deg"]), seed=Z.input_seed(hidden), kind=kind, phase=phase, hidden=hidden)
    return st["inputs"][key]


def _refs(name, kind, phase, variant, hidden=256):
    """{(agg, toe): (e64, h64, act64, d32_e, d32_h, d32_act)}; variant: "fused" | "unfused" (starts from C e + b_C) | "fp16x1"."""
    st = _graph(name)
    key = (kind, phase, variant, hidden)
    if key not in st["refs"]:
        inp = _inputs(name, kind, phase, hidden)
        kw = dict(from_ce=variant == "unfused", gemm=EMU.linear_fp16x1 if variant == "fp16x1" else None)
        aggs = ("sum",) if variant == "fp16x1" else Z.AGGS
        t64 = Z.layer_reference_all(inp, st["ei"], torch.float64, aggs=aggs, **kw)
        t32 = Z.layer_reference_all(inp, st["ei"], torch.float32, aggs=aggs, **kw)
        dist = lambda a, b: (a.double() - b).abs().max().item() if b.numel() else 0.0      # noqa: E731
        out = {k: t64[k] + tuple(dist(t32[k][i], t64[k][i]) for i in range(3)) for k in t64}
        if variant == "fp16x1":      # + the plain float64 layer: what the one-product result must NOT be close to
            plain = Z.layer_reference_all(inp, st["ei"], torch.float64, aggs=aggs)
            out = {k: out[k] + (plain[k][0],) for k in out}
        st["refs"][key] = out
    return st["refs"][key]


def _cases_of(name, deg):
    """(kind, phase) input sets of a graph: random inputs everywhere, the marker phases on the hubs."""
    out = [("random", 0)]
    if name in Z.HUBS:
        out += [("marker", ph) for ph in range(Z.n_phases(max(deg)))]
    return out


def _worst(st, per_row, rows_are_edges, over=0.0):
    """The worst row of a per-row error vector, as text that names the node, its CSR range and its protocol cases (+ the number of
    rows whose error exceeds ``over``)."""
    per_row = torch.nan_to_num(per_row, nan=float("inf"))
    r = int(per_row.argmax())
    slot = int(st["slot_of"][r]) if (rows_are_edges and "slot_of" in st) else r      # (TSP steps: output rows in caller order)
    node = int(st["row"][slot]) if rows_are_edges else r
    a, b = int(st["rowptr"][node]), int(st["rowptr"][node + 1])
    what = f"edge slot {slot} (tile {slot >> 5} row {slot & 31}) of " if rows_are_edges else ""
    return (f"{per_row[r].item():.3e} at {what}node {node}, (a, b) = ({a}, {b}), tiles {a >> 5}..{(b - 1) >> 5 if b > a else '-'}, "
            f"cases {sorted(Z.node_cases(st['rowptr'], node, len(st['col'])))}; {int((per_row > over).sum())} of {len(per_row)} rows over {over:.1e}")


def _bound(project, d32, deg, kind):
    return Z.calibrated(project, d32) if Z.uses_calibrated_bound(deg, kind) else project


def _dev_inputs(inp, dev, fused):
    """Device copies of a layer's inputs (cached in the input dict)."""
    from difusco_amd import graph, weights
    key = ("dev", fused)
    if key not in inp:
        d = lambda t: t.to(dev).contiguous()      # noqa: E731
        out = dict(node4=d(inp["node4"]), prm=[d(t) for t in inp["prm"]], tb=d(inp["tb"]))
        if fused:
            out.update(e=graph.to_tiled(d(inp["e"])), pc=d(weights.split_planes(inp["Wc"])), po=d(weights.split_planes(inp["Wo"])),
                       sc=d(weights.fused_scales(inp["Wc"], inp["Wo"], inp["prm"][4], inp["prm"][5])), bc=d(inp["bc"]), bo=d(inp["bo"]))
        else:
            out.update(ce=d(inp["ce"]))
        out["h"] = d(inp["h"])
        inp[key] = out
    return inp[key]


def _csr_dev(st, dev):
    if "csr_dev" not in st:
        st["csr_dev"] = tuple(torch.from_numpy(st[k]).to(dev) for k in ("rowptr", "row", "col"))
    return st["csr_dev"]


def _run_fused(L, dev, prec, inp, csr, n, E, agg, toe, reg_gather, expect=0):
    """difusco_edge_layer_fused_ex on fresh copies of e and h; the scratch starts as NaN bytes, so a piece that node_finalize
    reads and the kernel never wrote shows.  -> (e [E, 256], h, the pad rows of e) on the CPU."""
    from difusco_amd import graph
    x = _dev_inputs(inp, dev, True)
    rp, row, col = csr
    e_d, h_d = x["e"].clone(), x["h"].clone()
    scratch = torch.full((L.lib().difusco_fused_scratch_bytes(n, E),), 0xFF, dtype=torch.uint8, device=dev)
    code = L.lib().difusco_edge_layer_fused_ex(
        L.PRECISIONS[prec], n, E, _p(rp), _p(row), _p(col), _p(x["node4"]), _p(e_d), _p(h_d), _p(x["pc"]), _p(x["po"]), _p(x["bc"]),
        *[_p(t) for t in x["prm"]], _p(x["bo"]), _p(x["tb"]), toe, _p(x["sc"]), _p(scratch), AGG_ID[agg], reg_gather, _stream())
    if expect != 0:
        return code
    L.check(code)
    torch.cuda.synchronize()
    E_pad = (E + 255) // 256 * 256
    full = graph.from_tiled(e_d, E_pad).cpu()
    return full[:E], h_d.cpu(), full[E:]


def _run_unfused(L, dev, inp, csr, n, agg, toe):
    x = _dev_inputs(inp, dev, False)
    rp, _, col = csr
    ce_d, h_d = x["ce"].clone(), x["h"].clone()
    L.check(L.lib().difusco_edge_gate_aggregate_ex(inp["H"], n, _p(rp), _p(col), _p(x["node4"]), _p(ce_d), _p(h_d),
                                                   *[_p(t) for t in x["prm"]], _p(x["tb"]), toe, AGG_ID[agg], _stream()))
    torch.cuda.synchronize()
    return ce_d.cpu(), h_d.cpu()


def _compare(label, st, kind, got, ref, d32, project, rows_are_edges, failures):
    """L_inf of got against the float64 ref, held to the (calibrated) bound; a failure names the worst row's protocol case."""
    if ref.numel() == 0:
        return 0.0, project
    per_row = (got.double() - ref).abs().amax(dim=1)
    err = torch.nan_to_num(per_row, nan=float("inf")).max().item()
    bound = _bound(project, d32, st["deg"], kind)
    if not err < bound:
        failures.append(f"{label}: {err:.3e} >= bound {bound:.3e} (d32 {d32:.2e}); worst {_worst(st, per_row, rows_are_edges, bound)}")
    return err, bound


# ============================================ part 1: one layer ================================================================
@pytest.mark.parametrize("prec", ["fp16x3", "bf16x3"])
@pytest.mark.parametrize("name", LAYER_GRAPHS)
def test_fused_layer_on_zoo(dev, L, name, prec):
    """Fused kernel + node_finalize, {sum, mean, max} x time_on_edge x {full-line, register gathers}: h row by row and e edge by edge
    against float64, pad lanes still zero, two runs bit-identical (the pieces are combined in tile order, no atomics)."""
    st = _graph(name)
    n, E = len(st["deg"]), len(st["col"])
    csr = _csr_dev(st, dev)
    failures = []
    for kind, phase in _cases_of(name, st["deg"]):
        inp, refs = _inputs(name, kind, phase), _refs(name, kind, phase, "fused")
        for agg in Z.AGGS:
            for toe in (1, 0):
                e64, h64, _, d32_e, d32_h, _ = refs[(agg, toe)]
                for rg in ((0,) if agg == "max" else (0, 1)):      # (max has no register-gather instantiation)
                    label = f"fused {prec} {name} {kind}{phase} {agg} toe={toe} reg_gather={rg}"
                    e, h, pad = _run_fused(L, dev, prec, inp, csr, n, E, agg, toe, rg)
                    err_h, b_h = _compare(label + " h", st, kind, h, h64, d32_h, Z.H_BOUND[prec], False, failures)
                    err_e, b_e = _compare(label + " e", st, kind, e, e64, d32_e, Z.E_BOUND[prec], True, failures)
                    print(f"{label}: E={E} h L_inf {err_h:.2e} (d32 {d32_h:.2e}, bound {b_h:.1e}); e L_inf {err_e:.2e} "
                          f"(d32 {d32_e:.2e}, bound {b_e:.1e})")
                    if pad.numel() and not bool((pad == 0).all()):
                        failures.append(f"{label}: pad rows of e are not zero")
                    if toe == 0:      # repeat determinism (one time_on_edge per case keeps the run short)
                        e2, h2, _ = _run_fused(L, dev, prec, inp, csr, n, E, agg, toe, rg)
                        if not (torch.equal(e, e2) and torch.equal(h, h2)):
                            failures.append(f"{label}: two runs differ, h rows: {_worst(st, (h - h2).abs().amax(dim=1), False)}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("hidden", [256, 128, 64])
@pytest.mark.parametrize("name", LAYER_GRAPHS)
def test_unfused_layer_on_zoo(dev, L, name, hidden):
    """edge_gate_aggregate_kernel through difusco_edge_gate_aggregate_ex, {sum, mean, max} x time_on_edge (marker inputs at
    H = 256, where 256 consecutive hub edges own 256 distinct features)."""
    st = _graph(name)
    n = len(st["deg"])
    csr = _csr_dev(st, dev)
    failures = []
    for kind, phase in _cases_of(name, st["deg"]):
        if kind == "marker" and hidden != 256:
            continue
        inp, refs = _inputs(name, kind, phase, hidden), _refs(name, kind, phase, "unfused", hidden)
        for agg in Z.AGGS:
            for toe in (1, 0):
                _, h64, act64, _, d32_h, d32_a = refs[(agg, toe)]
                label = f"unfused H={hidden} {name} {kind}{phase} {agg} toe={toe}"
                act, h = _run_unfused(L, dev, inp, csr, n, agg, toe)
                err_h, b_h = _compare(label + " h", st, kind, h, h64, d32_h, Z.H_BOUND["unfused"], False, failures)
                err_a, b_a = _compare(label + " act", st, kind, act, act64, d32_a, Z.E_BOUND["unfused"], True, failures)
                print(f"{label}: h L_inf {err_h:.2e} (d32 {d32_h:.2e}, bound {b_h:.1e}); act L_inf {err_a:.2e} (d32 {d32_a:.2e}, "
                      f"bound {b_a:.1e})")
                if toe == 0:
                    act2, h2 = _run_unfused(L, dev, inp, csr, n, agg, toe)
                    if not (torch.equal(act, act2) and torch.equal(h, h2)):
                        failures.append(f"{label}: two runs differ")
    assert not failures, "\n".join(failures)


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


@pytest.mark.parametrize("name", LAYER_GRAPHS)
def test_fused_layer_fp16x1_on_zoo(dev, L, name):
    """fp16x1 (sum): against the layer whose two products are emulated (tests/fp16x1_emulation.py), with the class check of
    test_gpu_fp16x1.py::test_edge_layer_fused_fp16x1 - e is much closer to the emulation than to the plain layer."""
    st = _graph(name)
    n, E = len(st["deg"]), len(st["col"])
    csr = _csr_dev(st, dev)
    failures = []
    for kind, phase in _cases_of(name, st["deg"]):
        inp, refs = _inputs(name, kind, phase), _refs(name, kind, phase, "fp16x1")
        for toe in (1, 0):
            e_emu, h_emu, _, d32_e, d32_h, _, e_plain = refs[("sum", toe)]
            for rg in (0, 1):
                label = f"fused fp16x1 {name} {kind}{phase} sum toe={toe} reg_gather={rg}"
                e, h, pad = _run_fused(L, dev, "fp16x1", inp, csr, n, E, "sum", toe, rg)
                err_h, b_h = _compare(label + " h", st, kind, h, h_emu, d32_h, Z.H_BOUND["fp16x1"], False, failures)
                err_e, b_e = _compare(label + " e", st, kind, e, e_emu, d32_e, Z.E_BOUND["fp16x1"], True, failures)
                far_e = (e.double() - e_plain).abs().max().item()
                rms_emu, rms_plain = _rms(e.double() - e_emu), _rms(e_emu - e_plain)
                print(f"{label}: h L_inf {err_h:.2e} (d32 {d32_h:.2e}, bound {b_h:.1e}); e L_inf {err_e:.2e} (vs plain {far_e:.2e}), "
                      f"RMS vs emulation {rms_emu:.2e}, emulation vs plain {rms_plain:.2e}")
                if not (far_e > 2 * err_e and rms_plain > 10 * rms_emu):
                    failures.append(f"{label}: not in the one-product class: {(far_e, err_e, rms_plain, rms_emu)}")
                if pad.numel() and not bool((pad == 0).all()):
                    failures.append(f"{label}: pad rows of e are not zero")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("engine", ["fp16x3", "bf16x3", "fp16x1", "unfused"])
@pytest.mark.parametrize("name", ["straddle", "ones_95", "tiny_33", "hub256"])
def test_empty_rows_are_invisible(dev, L, name, engine):
    """Empty rows inserted before, between and after the rows of a graph leave every edge in its CSR slot: e and the h rows of the
    other nodes are bit-identical; the inserted rows get h + ReLU(LN(Uh)) (+ tbias when time_on_edge = 0), at the layer bound."""
    from difusco_amd import graph
    st = _graph(name)
    deg, ei = st["deg"], st["ei"]
    deg2, where = Z.with_empty_rows(deg)
    n, n2, E = len(deg), len(deg2), ei.shape[1]
    ei2 = where[ei]
    rowptr2, col2, row2, _, ident = graph.csr_from_coo_host(ei2, n2)
    assert ident and np.array_equal(rowptr2[where], st["rowptr"][:-1])
    csr, csr2 = _csr_dev(st, dev), tuple(torch.from_numpy(a).to(dev) for a in (rowptr2, row2, col2))
    inp = _inputs(name, "random", 0)
    g = torch.Generator().manual_seed(5)
    inp2 = {k: v for k, v in inp.items() if not (isinstance(k, tuple) and k[0] == "dev")}
    inp2["n"] = n2
    for key, width in (("node4", 4 * Z.H), ("h", Z.H)):
        big = torch.randn(n2, width, generator=g)
        big[torch.from_numpy(where)] = inp[key]
        inp2[key] = big
    st2 = dict(deg=deg2, rowptr=rowptr2, row=row2, col=col2)
    inserted = np.setdiff1d(np.arange(n2), where)
    variant = "unfused" if engine == "unfused" else ("fp16x1" if engine == "fp16x1" else "fused")
    aggs = Z.AGGS if engine == "unfused" else ("sum", "max")
    kw = dict(from_ce=variant == "unfused", gemm=EMU.linear_fp16x1 if variant == "fp16x1" else None)
    ref2 = Z.layer_reference_all(inp2, ei2, torch.float64, aggs=aggs, **kw)
    failures = []
    for agg in aggs:
        for toe in (1, 0):
            label = f"empty rows {engine} {name} {agg} toe={toe}"
            if engine == "unfused":
                e_a, h_a = _run_unfused(L, dev, inp, csr, n, agg, toe)
                e_b, h_b = _run_unfused(L, dev, inp2, csr2, n2, agg, toe)
            else:
                e_a, h_a, _ = _run_fused(L, dev, engine, inp, csr, n, E, agg, toe, 0)
                e_b, h_b, _ = _run_fused(L, dev, engine, inp2, csr2, n2, E, agg, toe, 0)
            if not torch.equal(e_a, e_b):
                failures.append(f"{label}: e changed: {_worst(st, (e_a - e_b).abs().amax(dim=1), True)}")
            if not torch.equal(h_a, h_b[where]):
                failures.append(f"{label}: h changed: {_worst(st, (h_a - h_b[where]).abs().amax(dim=1), False)}")
            h64 = ref2[(agg, toe)][1]
            err = (h_b.double() - h64)[inserted].abs().max().item()
            print(f"{label}: {len(inserted)} inserted rows, h L_inf {err:.2e}")
            if not err < Z.H_BOUND[engine]:
                failures.append(f"{label}: inserted rows off by {err:.3e}: {_worst(st2, (h_b.double() - h64).abs().amax(dim=1), False)}")
    assert not failures, "\n".join(failures)


def test_layer_entries_arguments(dev, L):
    """difusco_edge_layer_fused is difusco_edge_layer_fused_ex(SUM, n_nodes >= 2^20); max with register gathers and unknown
    aggregations are refused, as the step refuses them."""
    st = _graph("straddle")
    n, E = len(st["deg"]), len(st["col"])
    csr = _csr_dev(st, dev)
    inp = _inputs("straddle", "random", 0)
    assert _run_fused(L, dev, "fp16x3", inp, csr, n, E, "max", 1, 1, expect=-1) == -1
    assert "register-gather" in L.lib().difusco_last_error().decode()
    x = _dev_inputs(inp, dev, True)
    args = [_p(csr[0]), _p(csr[1]), _p(csr[2]), _p(x["node4"])]
    tail = [_p(x["pc"]), _p(x["po"]), _p(x["bc"]), *[_p(t) for t in x["prm"]], _p(x["bo"]), _p(x["tb"]), 1, _p(x["sc"])]
    scratch = torch.zeros(L.lib().difusco_fused_scratch_bytes(n, E), dtype=torch.uint8, device=dev)
    for bad in (-1, 3):
        e_d, h_d = x["e"].clone(), x["h"].clone()
        assert L.lib().difusco_edge_layer_fused_ex(L.PREC_FP16X3, n, E, *args, _p(e_d), _p(h_d), *tail, _p(scratch), bad, 0, _stream()) == -1
        assert "aggregation" in L.lib().difusco_last_error().decode()
        u = _dev_inputs(inp, dev, False)
        assert L.lib().difusco_edge_gate_aggregate_ex(256, n, _p(csr[0]), _p(csr[2]), _p(u["node4"]), _p(u["ce"].clone()), _p(h_d),
                                                      *[_p(t) for t in u["prm"]], _p(u["tb"]), 1, bad, _stream()) == -1
        assert "aggregation" in L.lib().difusco_last_error().decode()
    e_d, h_d = x["e"].clone(), x["h"].clone()
    L.check(L.lib().difusco_edge_layer_fused(L.PREC_FP16X3, n, E, *args, _p(e_d), _p(h_d), *tail, _p(scratch), _stream()))
    torch.cuda.synchronize()
    from difusco_amd import graph
    e_ex, h_ex, _ = _run_fused(L, dev, "fp16x3", inp, csr, n, E, "sum", 1, 0)
    assert torch.equal(graph.from_tiled(e_d, E).cpu(), e_ex) and torch.equal(h_d.cpu(), h_ex)
    u = _dev_inputs(inp, dev, False)
    ce_d, h_d = u["ce"].clone(), u["h"].clone()
    L.check(L.lib().difusco_edge_gate_aggregate(256, n, _p(csr[0]), _p(csr[2]), _p(u["node4"]), _p(ce_d), _p(h_d),
                                                *[_p(t) for t in u["prm"]], _p(u["tb"]), 1, _stream()))
    torch.cuda.synchronize()
    a_ex, h_ex = _run_unfused(L, dev, inp, csr, n, "sum", 1)
    assert torch.equal(ce_d.cpu(), a_ex) and torch.equal(h_d.cpu(), h_ex)


# ============================================ part 2: whole steps =================================================================
HID, LAYERS = 256, 3      # layer 0 from the table (kind 1), a middle layer (kind 0), the tail (kind 2 TSP / kind 3 MIS)
T, TT = 500, 469
_MODELS, _PARAMS = {}, {}


def _args(kind, sparse_factor, aggregation):
    return dict(diffusion_type=kind, diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=LAYERS, hidden_dim=HID, inference_trick="ddim", aggregation=aggregation)


def _params(C):
    if C not in _PARAMS:
        _PARAMS[C] = O.init_params(HID, LAYERS, C, seed=11)
    return _PARAMS[C]


def _model(task, diffusion, agg, dev, **kw):
    from difusco_amd import MISModel, TSPModel
    key = (task, diffusion, agg) + tuple(sorted(kw.items()))
    if key not in _MODELS:
        cls, sf = (MISModel, -1) if task == "mis" else (TSPModel, 8)
        _MODELS[key] = cls(_args(diffusion, sf, agg), _params(2 if diffusion == "categorical" else 1), device=dev, **kw)
    return _MODELS[key]


def _no_folds():
    from difusco_amd import _lib
    return _lib.FLAG_NO_L0_FOLD | _lib.FLAG_NO_TAIL_FOLD


def _step_check(label, prec, st, rows_are_edges, got, ref, truth, e_ref_true, failures, prob=None, ref_prob=None, out_x=None,
                ref_x=None, u=None):
    """The rule of test_gpu_round6.py::test_default_engine_on_trained_like_weights (fp16x3) / the 1e-4 bound (bf16x3)."""
    got = got.cpu().reshape(ref.shape)
    per_true = (got.double() - truth).abs().reshape(len(ref), -1).amax(dim=1)
    e_hip_true = torch.nan_to_num(per_true, nan=float("inf")).max().item() if len(ref) else 0.0
    e_hip_ref = (got - ref).abs().max().item() if len(ref) else 0.0
    print(f"{label}: HIP vs fp32 oracle {e_hip_ref:.2e}; fp32 oracle vs float64 (e_ref_true) {e_ref_true:.2e}; HIP vs float64 "
          f"{e_hip_true:.2e}")
    bound = max(CLASS_TOL, 4.0 * e_ref_true) if prec == "fp16x3" else TOL
    if not e_hip_true < bound:
        failures.append(f"{label}: vs float64 {e_hip_true:.3e} >= {bound:.3e}; worst {_worst(st, per_true, rows_are_edges, bound)}")
    direct = CLASS_TOL if prec == "fp16x3" else TOL
    if prec != "fp16x3" or e_ref_true < CLASS_TOL / 3:      # the fp32 oracle is a usable arbiter at the class
        if not e_hip_ref < direct:
            failures.append(f"{label}: vs fp32 oracle {e_hip_ref:.3e} >= {direct:.0e}")
        if prob is not None and len(ref):
            e_prob = (prob.cpu().reshape(-1) - ref_prob.reshape(-1)).abs().max().item()
            safe = (u - ref_prob.reshape(-1)).abs() > direct      # tie band = the bound asserted on prob
            if not (e_prob < direct and torch.equal(out_x.cpu().reshape(-1)[safe], ref_x.reshape(-1)[safe])):
                failures.append(f"{label}: prob off by {e_prob:.3e} or sampled bits differ outside the tie band")
    return got


@pytest.mark.parametrize("agg", Z.AGGS)
@pytest.mark.parametrize("name", list(Z.ZOO))
def test_mis_step_on_zoo(dev, name, agg):
    """MISModel.categorical_denoise_step on every zoo graph (no_edges included: E = 0 takes the unfused sequence, every launch over
    edges is skipped, every row is h + ReLU(LN(Uh)) + t): fused with and without the layer-0 / tail folds and unfused, fp16x3 and
    bf16x3, against the fp32 oracle and float64; fused against unfused at the bounds of test_log2e_domain_fused_equals_unfused."""
    st = _graph(name)
    n = len(st["deg"])
    p = _params(2)
    g = torch.Generator().manual_seed(17)
    ei = torch.from_numpy(st["ei"])
    xt = (torch.randn(n, generator=g) > 0).float()
    u = torch.rand(n, generator=g)
    ref_x, ref, ref_prob = O.mis_categorical_denoise_step(p, O.CategoricalTables(), xt, T, ei, TT, uniform=u, return_aux=True,
                                                          aggregation=agg)
    truth = O.encoder_sparse_f64(p, None, xt, torch.tensor([float(T)]), ei, node_feature_only=True, aggregation=agg)
    e_ref_true = (ref.double() - truth).abs().max().item()
    failures, ei_d = [], ei.to(dev)
    for prec, fu_bound in (("fp16x3", 1e-5), ("bf16x3", 1e-4)):
        got = {}
        for cfg, kw in (("fused", {}), ("fused/no folds", dict(flags=_no_folds())), ("unfused", dict(fused=False))):
            m = _model("mis", "categorical", agg, dev, precision=prec, **kw)
            out_x, logits, prob = m.categorical_denoise_step(xt.to(dev), np.array([T]), dev, ei_d, target_t=np.array([TT]), uniform=u,
                                                             return_aux=True)
            torch.cuda.synchronize()
            got[cfg] = _step_check(f"mis {name} {agg} {prec} {cfg}", prec, st, False, logits, ref, truth, e_ref_true, failures,
                                   prob, ref_prob, out_x, ref_x, u)
        for cfg in ("fused", "fused/no folds"):
            d = (got[cfg] - got["unfused"]).abs().max().item()
            print(f"mis {name} {agg} {prec}: {cfg} vs unfused {d:.2e}")
            if not d < fu_bound:
                failures.append(f"mis {name} {agg} {prec}: {cfg} vs unfused {d:.3e} >= {fu_bound:.0e}; worst "
                                f"{_worst(st, (got[cfg] - got['unfused']).abs().amax(dim=1), False)}")
    assert not failures, "\n".join(failures)


def test_mis_step_without_edges_on_both_bindings(dev):
    """E = 0 through the ctypes and the torch.ops binding: same bits, and the oracle's value."""
    st = _graph("no_edges")
    n = len(st["deg"])
    p = _params(2)
    g = torch.Generator().manual_seed(17)
    ei = torch.from_numpy(st["ei"])
    xt = (torch.randn(n, generator=g) > 0).float()
    u = torch.rand(n, generator=g)
    ref = O.mis_categorical_denoise_step(p, O.CategoricalTables(), xt, T, ei, TT, uniform=u, return_aux=True)[1]
    outs = []
    for backend in ("ctypes", "torch"):
        m = _model("mis", "categorical", "sum", dev, backend=backend)
        outs.append(m.categorical_denoise_step(xt.to(dev), np.array([T]), dev, ei.to(dev), target_t=np.array([TT]), uniform=u,
                                               return_aux=True)[1].cpu())
    assert torch.equal(outs[0], outs[1])
    assert (outs[0] - ref).abs().max().item() < CLASS_TOL


@pytest.mark.parametrize("task", ["mis", "tsp"])
@pytest.mark.parametrize("name", ["hub_middle", "zipf"])
def test_step_repeat_and_backend_determinism(dev, name, task):
    """Two runs of the same step, and the ctypes and torch.ops bindings, give the same bits (sum and max, fused)."""
    st = _graph(name)
    n = len(st["deg"])
    for agg in ("sum", "max"):
        outs = []
        for backend in ("ctypes", "ctypes", "torch"):
            if task == "mis":
                g = torch.Generator().manual_seed(17)
                xt, u = (torch.randn(n, generator=g) > 0).float(), torch.rand(n, generator=g)
                m = _model("mis", "categorical", agg, dev, backend=backend)
                res = m.categorical_denoise_step(xt.to(dev), np.array([T]), dev, torch.from_numpy(st["ei"]).to(dev),
                                                 target_t=np.array([TT]), uniform=u, return_aux=True)
            else:
                pts, ei, xt, u, _ = _tsp_inputs(st, "categorical")
                m = _model("tsp", "categorical", agg, dev, backend=backend, reorder_nodes=False)
                res = _tsp_run(m, "categorical", pts, ei.to(dev), xt, u, dev)
            outs.append([t.cpu() for t in res])
        for other in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], other)), (name, task, agg)


def _tsp_inputs(st, diffusion):
    n, E = len(st["deg"]), len(st["col"])
    g = torch.Generator().manual_seed(23)
    pts = torch.rand(n, 2, generator=g)
    sh = torch.randperm(E, generator=g)
    ei = torch.from_numpy(st["ei"])[:, sh].contiguous()      # the caller's edge order shuffled: perm is not the identity
    xt = (torch.randn(E, generator=g) > 0).float() if diffusion == "categorical" else torch.randn(E, generator=g)
    u = torch.rand(E, generator=g)
    return pts, ei, xt, u, sh


def _tsp_reference(p, diffusion, pts, ei, xt, u, agg):
    if diffusion == "categorical":
        # (O.tsp_categorical_denoise_step views the logits as [1, N, E / N, 2] like pl_tsp_model.py:135, which needs a constant
        #  degree; the posterior is element-wise, so the same functions are applied to a [1, 1, E, 2] view here)
        ref = O.encoder_sparse_edge(p, pts, xt.float(), torch.tensor([float(T)]), ei, aggregation=agg)
        ref_x, ref_prob = O.categorical_posterior(O.CategoricalTables(), T, TT, ref.reshape(1, 1, -1, 2).softmax(dim=-1), xt, True, u)
    else:
        ref_x, ref = O.tsp_gaussian_denoise_step(p, O.GaussianTables(), pts, xt, T, ei, TT, return_aux=True, aggregation=agg)[:2]
        ref_prob = None
    truth = O.encoder_sparse_f64(p, pts, xt, torch.tensor([float(T)]), ei, aggregation=agg).reshape(ref.shape)
    return ref_x, ref, ref_prob, truth


def _tsp_run(m, diffusion, pts, ei_d, xt, u, dev):
    if diffusion == "categorical":
        return m.categorical_denoise_step(pts.to(dev), xt.to(dev), np.array([T]), dev, ei_d, target_t=np.array([TT]), uniform=u,
                                          return_aux=True)
    out_x, pred = m.gaussian_denoise_step(pts.to(dev), xt.to(dev), np.array([T]), dev, ei_d, target_t=np.array([TT]), return_aux=True)
    return out_x, pred, None


# (aggregation, diffusion): the categorical step with binary x_t folds layer 0; the Gaussian step generates its edge input in the
# embedding kernel and has no layer-0 fold.  mean differs from sum in node_finalize only, which the MIS steps cover per graph.
@pytest.mark.parametrize("agg,diffusion", [("sum", "categorical"), ("max", "categorical"), ("mean", "categorical"), ("sum", "gaussian")])
@pytest.mark.parametrize("name", LAYER_GRAPHS)
def test_tsp_step_on_zoo(dev, name, agg, diffusion):
    """TSPModel on the zoo's edge lists with random points, the caller's edge order shuffled, reorder_nodes=False (the designed tile
    placement is kept); zipf and hub_empties also with the default reorder_nodes=True, at the same bounds."""
    st = _graph(name)
    p = _params(2 if diffusion == "categorical" else 1)
    pts, ei, xt, u, sh = _tsp_inputs(st, diffusion)
    ref_x, ref, ref_prob, truth = _tsp_reference(p, diffusion, pts, ei, xt, u, agg)
    e_ref_true = (ref.double() - truth).abs().max().item()
    st_rows = dict(st, slot_of=sh.numpy())      # per-row reports: output row r is the caller's edge r = CSR slot sh[r]
    failures, ei_d = [], ei.to(dev)
    configs = [("fp16x3", "fused", dict(reorder_nodes=False)), ("fp16x3", "fused/no folds", dict(reorder_nodes=False, flags=_no_folds())),
               ("fp16x3", "unfused", dict(reorder_nodes=False, fused=False))]
    if agg == "sum":
        configs += [("bf16x3", "fused", dict(reorder_nodes=False)), ("bf16x3", "unfused", dict(reorder_nodes=False, fused=False))]
    if name in ("zipf", "hub_empties"):
        configs.append(("fp16x3", "fused/reordered", {}))
    got = {}
    for prec, cfg, kw in configs:
        m = _model("tsp", diffusion, agg, dev, precision=prec, **kw)
        out_x, pred, prob = _tsp_run(m, diffusion, pts, ei_d, xt, u, dev)
        torch.cuda.synchronize()
        label = f"tsp {diffusion} {name} {agg} {prec} {cfg}"
        got[(prec, cfg)] = _step_check(label, prec, st_rows, True, pred, ref, truth, e_ref_true, failures, prob, ref_prob, out_x,
                                       ref_x, u)
        if prob is None and (prec != "fp16x3" or e_ref_true < CLASS_TOL / 3):
            d = (out_x.cpu().reshape(-1) - ref_x.reshape(-1)).abs().max().item()
            if not d < (CLASS_TOL if prec == "fp16x3" else TOL):
                failures.append(f"{label}: x_next off by {d:.3e}")
    for (prec, cfg), val in got.items():
        if cfg == "unfused":
            continue
        d = (val - got[(prec, "unfused")]).abs().max().item()
        print(f"tsp {diffusion} {name} {agg} {prec}: {cfg} vs unfused {d:.2e}")
        if not d < (1e-5 if prec == "fp16x3" else 1e-4):
            failures.append(f"tsp {diffusion} {name} {agg} {prec}: {cfg} vs unfused {d:.3e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("task", ["mis", "tsp"])
@pytest.mark.parametrize("name", ["hub_middle", "straddle", "zipf"])
def test_step_fp16x1_on_zoo(dev, name, task):
    """fp16x1 steps, default flags, through the class check of test_gpu_fp16x1.py (distance from the fp32 oracle between d / 4 and
    2 d + 1e-5, d = the emulated network's own distance)."""
    from tests.test_gpu_fp16x1 import _check_class, _emulated
    st = _graph(name)
    n = len(st["deg"])
    p = _params(2)
    if task == "mis":
        g = torch.Generator().manual_seed(17)
        ei = torch.from_numpy(st["ei"])
        xt = (torch.randn(n, generator=g) > 0).float()
        ref = lambda: O.mis_categorical_denoise_step(p, O.CategoricalTables(), xt, T, ei, 0, return_aux=True)[1]      # noqa: E731
        m = _model("mis", "categorical", "sum", dev, precision="fp16x1")
        got = m.categorical_denoise_step(xt.to(dev), np.array([T]), dev, ei.to(dev), target_t=np.array([0]), return_aux=True)[1]
    else:
        pts, ei, xt, _, _ = _tsp_inputs(st, "categorical")
        ref = lambda: O.encoder_sparse_edge(p, pts, xt.float(), torch.tensor([float(T)]), ei)      # noqa: E731
        m = _model("tsp", "categorical", "sum", dev, precision="fp16x1", reorder_nodes=False)
        got = m.categorical_denoise_step(pts.to(dev), xt.to(dev), np.array([T]), dev, ei.to(dev), target_t=np.array([0]),
                                         return_aux=True)[1]
    _check_class(f"fp16x1 {task} {name}", got.cpu(), _emulated(ref), ref())
