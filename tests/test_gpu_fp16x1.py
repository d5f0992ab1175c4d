"""Precision fp16x1 on the GPU (DIFUSCO_PREC_FP16X1): the edge-row GEMMs (layers.{l}.C, per_layer_out.{l}.2) take ONE fp16 product
of power-of-two-scaled operands; everything else runs as fp16x3.  "Emulation" is a CPU float64 sum of the fp16-rounded operands
(tests/fp16x1_emulation.py); for a whole network it is the fp32 oracle with ``_lin`` of those two Linears replaced (monkeypatch,
the oracle file is unchanged).

Rounding to fp16 is discontinuous: where an operand lies within fp32 noise of a rounding midpoint, the GPU and the CPU round it to
neighbouring fp16 values.  Inside one GEMM on shared inputs (the split linear) that never happens and the match is ~1e-7 relative.
Behind fp32 arithmetic (the stand-alone layer's GEMM 2 operand) a few operands in ten thousand flip, which shows in the L_inf over
millions of outputs but not in the RMS.  Across layers the flips feed into the next layer's operands, and after a few layers a
step is one more independent sample of the fp16x1 rounding: whole steps are held to the class bound of the contract instead -
their distance from the fp32 oracle is at most 2 d + 1e-5 and at least d / 4, d = the emulated network's own distance from it
(measured on the CPU; DESIGN.md records the values).  fp16x3, or any silent fall-back to it, is ~1e-6 from the oracle."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import difusco_oracle as O
from tests import fp16x1_emulation as EMU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _args(kind, sparse_factor=8, trick="ddim", H=256, L=3, aggregation="sum"):
    return dict(diffusion_type=kind, diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=L, hidden_dim=H, inference_trick=trick, aggregation=aggregation)


# ---- 1. the split linear, one product ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,n_out", [(1000, 256, 256), (300, 256, 1024), (333, 128, 128), (517, 64, 64), (2, 256, 256)])
def test_linear_rows_split_fp16x1(dev, m, k, n_out):
    from difusco_amd import _lib, weights
    g = torch.Generator().manual_seed(m + k + n_out)
    x = torch.randn(m, k, generator=g) * 3.0
    w = torch.randn(n_out, k, generator=g) / 16 + torch.arange(n_out).float()[:, None] * 1e-4
    b = torch.randn(n_out, generator=g)
    emu = EMU.linear_fp16x1(x, w, b)
    exact = x.double() @ w.double().t() + b.double()
    xd, pd, bd = x.to(dev), weights.split_planes(w).to(dev), b.to(dev)
    y = torch.full((m, n_out), float("nan"), device=dev)
    scratch = torch.empty(m, device=dev)
    _lib.check(_lib.lib().difusco_linear_rows_split(_p(xd), _p(pd), _lib.PREC_FP16X1, _p(bd), None, _p(y), m, k, n_out, n_out,
                                                    _p(scratch), _stream()))
    torch.cuda.synchronize()
    yc = y.cpu().double()
    e_emu, e_fp32 = (yc - emu).abs().max().item(), (yc - exact).abs().max().item()
    scale = exact.abs().max().item()
    print(f"linear fp16x1 {m}x{k}x{n_out}: L_inf vs emulation {e_emu:.2e}, vs fp32 {e_fp32:.2e}, max |y| {scale:.1f}")
    assert e_emu <= 1e-6 * scale, (e_emu, scale)
    assert e_fp32 >= 20 * e_emu, (e_fp32, e_emu)


# ---- 2. the fused edge layer, stand-alone entry ----------------------------------------------------------------------------
@pytest.mark.parametrize("time_on_edge", [1, 0])
@pytest.mark.parametrize("n,p_edge,seed", [(150, 0.35, 0), (300, 0.02, 2)])
def test_edge_layer_fused_fp16x1(dev, time_on_edge, n, p_edge, seed):
    """As test_gpu_parity.py::test_edge_layer_fused, against a reference layer whose two GEMMs are emulated."""
    import torch.nn.functional as F
    from difusco_amd import _lib, graph, weights
    H = 256
    g = torch.Generator().manual_seed(seed)
    ei = O.er_mis_instance(n, p_edge, seed=seed)
    ei = ei[:, ei[0] != 5]                                   # node 5: no edges at all
    rowptr, col, row, perm, _ = graph.csr_from_coo_host(ei, n)
    E = col.shape[0]
    node4 = torch.randn(n, 4 * H, generator=g)
    e = torch.randn(E, H, generator=g) * 2.0
    h = torch.randn(n, H, generator=g)
    Wc = (torch.rand(H, H, generator=g) * 2 - 1) / 16 + torch.arange(H).float()[:, None] * 1e-4
    Wo = (torch.rand(H, H, generator=g) * 2 - 1) / 16 + torch.arange(H).float()[None, :] * 1e-4
    bc, bo = torch.randn(H, generator=g) * 0.1, torch.randn(H, generator=g) * 0.1
    prm = [1 + 0.1 * torch.randn(H, generator=g) if i % 2 == 0 else 0.1 * torch.randn(H, generator=g) for i in range(6)]
    tb = torch.randn(H, generator=g)
    rowt, colt = torch.from_numpy(row).long(), torch.from_numpy(col).long()
    Uh, Vh, Ah, Bh = node4[:, :H], node4[:, H:2 * H], node4[:, 2 * H:3 * H], node4[:, 3 * H:]

    def layer(gemm):
        e1 = Ah[colt] + Bh[rowt] + gemm(e, Wc).float() + bc
        agg = O.segment_sum(torch.sigmoid(e1) * Vh[colt], rowt, n)
        hn = F.relu(F.layer_norm(Uh + agg, (H,), prm[0], prm[1], 1e-5))
        en = F.relu(F.layer_norm(e1, (H,), prm[2], prm[3], 1e-5))
        if time_on_edge:
            en = en + tb
        else:
            hn = hn + tb
        act = F.silu(F.layer_norm(en, (H,), prm[4], prm[5], 1e-5))
        return e + gemm(act, Wo).float() + bo, h + hn
    e_emu, h_emu = layer(EMU.linear_fp16x1)
    e_ref, h_ref = layer(lambda x, w: x.double() @ w.double().t())

    d = lambda t: t.to(dev).contiguous()
    e_d, h_d, n4_d = graph.to_tiled(d(e)), d(h), d(node4)
    pc, po = d(weights.split_planes(Wc)), d(weights.split_planes(Wo))
    sc_d = d(weights.fused_scales(Wc, Wo, prm[4], prm[5]))
    bc_d, bo_d, tb_d = d(bc), d(bo), d(tb)
    prm_d = [d(t) for t in prm]
    rp_d, row_d, col_d = d(torch.from_numpy(rowptr)), d(torch.from_numpy(row)), d(torch.from_numpy(col))
    scratch = torch.zeros(_lib.lib().difusco_fused_scratch_bytes(n, E), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().difusco_edge_layer_fused(_lib.PREC_FP16X1, n, E, _p(rp_d), _p(row_d), _p(col_d), _p(n4_d), _p(e_d),
                                                   _p(h_d), _p(pc), _p(po), _p(bc_d), _p(prm_d[0]), _p(prm_d[1]), _p(prm_d[2]),
                                                   _p(prm_d[3]), _p(prm_d[4]), _p(prm_d[5]), _p(bo_d), _p(tb_d), time_on_edge,
                                                   _p(sc_d), _p(scratch), _stream()))
    torch.cuda.synchronize()
    e_out = graph.from_tiled(e_d, E).cpu()
    err_e, err_h = (e_out - e_emu).abs().max().item(), (h_d.cpu() - h_emu).abs().max().item()
    far_e = (e_out - e_ref).abs().max().item()
    rms_emu, rms_fp32 = _rms(e_out - e_emu), _rms(e_emu.double() - e_ref.double())
    assert graph.from_tiled(e_d, (E + 255) // 256 * 256)[E:].abs().max().item() == 0.0      # pad lanes stay zero
    print(f"fused fp16x1 toe={time_on_edge} n={n} E={E}: e L_inf {err_e:.2e} (vs fp32 {far_e:.2e}), RMS vs emulation "
          f"{rms_emu:.2e}, emulation vs fp32 {rms_fp32:.2e}; h L_inf {err_h:.2e}")
    assert err_e < 5e-4 and err_h < 3e-5, (err_e, err_h)      # |e| ~ 10; h: the gate reads the GEMM 1 result only
    assert far_e > 2 * err_e and rms_fp32 > 10 * rms_emu, (far_e, err_e, rms_fp32, rms_emu)


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


def _check_class(label, got, emu, r32):
    """got (GPU, fp16x1) against the emulated network emu and the fp32 oracle r32 (see the module notes)."""
    got, emu, r32 = got.double().reshape(r32.shape), emu.double().reshape(r32.shape), r32.double()
    e_emu, e_fp32, d = (got - emu).abs().max().item(), (got - r32).abs().max().item(), (emu - r32).abs().max().item()
    print(f"{label}: logits L_inf vs emulation {e_emu:.2e}, vs fp32 {e_fp32:.2e} (emulation vs fp32 {d:.2e}); RMS vs emulation "
          f"{_rms(got - emu):.2e}, vs fp32 {_rms(got - r32):.2e} (emulation vs fp32 {_rms(emu - r32):.2e}); "
          f"max |logit| {emu.abs().max().item():.2f}")
    assert e_fp32 <= 2 * d + 1e-5, (e_fp32, d)
    assert e_fp32 >= d / 4, (e_fp32, d)
    assert e_emu <= 2 * d + 1e-5, (e_emu, d)


# ---- 3. whole steps against the emulated network ----------------------------------------------------------------------------
def _case(name, Lyr, H=256):
    """-> (reference(p) -> logits on the CPU, run(model kwargs) -> logits from the GPU, model args, params)."""
    from difusco_amd import MISModel, TSPModel
    dev = torch.device("cuda:0")
    if name.startswith("tsp_cat"):
        agg = "max" if name.endswith("max") else "sum"
        p = O.init_params(H, Lyr, 2, seed=40 + Lyr)
        pts, ei = O.tsp_instance(100, 20, seed=6)
        pts, ei = torch.from_numpy(pts), torch.from_numpy(ei)
        xt = (torch.randn(ei.shape[1], generator=torch.Generator().manual_seed(1)) > 0).float()
        ref = lambda: O.tsp_categorical_denoise_step(p, O.CategoricalTables(), pts, xt, 500, ei, 0, return_aux=True,
                                                     aggregation=agg)[1]
        run = lambda **kw: TSPModel(_args("categorical", 20, H=H, L=Lyr, aggregation=agg), p, device=dev, **kw) \
            .categorical_denoise_step(pts.to(dev), xt.to(dev), np.array([500]), dev, ei.to(dev), target_t=np.array([0]),
                                      return_aux=True)[1]
    elif name == "tsp_gau":
        p = O.init_params(H, Lyr, 1, seed=50 + Lyr)
        pts, ei = O.tsp_instance(80, 12, seed=5)
        pts, ei = torch.from_numpy(pts), torch.from_numpy(ei)
        xt = torch.randn(ei.shape[1], generator=torch.Generator().manual_seed(3))
        ref = lambda: O.tsp_gaussian_denoise_step(p, O.GaussianTables(), pts, xt, 600, ei, 560, return_aux=True)[1]
        run = lambda **kw: TSPModel(_args("gaussian", 12, H=H, L=Lyr), p, device=dev, **kw) \
            .gaussian_denoise_step(pts.to(dev), xt.to(dev), np.array([600]), dev, ei.to(dev), target_t=np.array([560]),
                                   return_aux=True)[1]
    elif name == "mis_cat":
        p = O.init_params(H, Lyr, 2, seed=60 + Lyr)
        ei = torch.from_numpy(O.er_mis_instance(120, 0.15, seed=4))
        xt = (torch.randn(120, generator=torch.Generator().manual_seed(2)) > 0).float()
        ref = lambda: O.mis_categorical_denoise_step(p, O.CategoricalTables(), xt, 500, ei, 0, return_aux=True)[1]
        run = lambda **kw: MISModel(_args("categorical", -1, H=H, L=Lyr), p, device=dev, **kw) \
            .categorical_denoise_step(xt.to(dev), np.array([500]), dev, ei.to(dev), target_t=np.array([0]), return_aux=True)[1]
    elif name == "tsp50_dense":
        p = O.init_params(H, Lyr, 2, seed=70 + Lyr)
        pts = torch.rand(1, 50, 2, generator=torch.Generator().manual_seed(8))
        xt = (torch.randn(1, 50, 50, generator=torch.Generator().manual_seed(9)) > 0).float()
        ref = lambda: O.tsp_categorical_denoise_step(p, O.CategoricalTables(), pts, xt, 500, None, 0,
                                                     return_aux=True)[1].permute(0, 2, 3, 1).contiguous()
        run = lambda **kw: TSPModel(_args("categorical", -1, H=H, L=Lyr), p, device=dev, **kw) \
            .categorical_denoise_step(pts.to(dev), xt.to(dev), np.array([500]), dev, None, target_t=np.array([0]),
                                      return_aux=True)[1]
    else:
        raise ValueError(name)
    return ref, run


def _emulated(ref):
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(O, "_lin", EMU.emulating_lin(O._lin))
        return ref()


@pytest.mark.parametrize("Lyr", [3, 12])
@pytest.mark.parametrize("name", ["tsp_cat", "tsp_gau", "mis_cat", "tsp50_dense", "tsp_cat_max"])
def test_step_fp16x1_against_emulated_network(dev, name, Lyr):
    """Every fused kind end to end: layer 0 from the two-row table (TSP categorical, MIS), the middle layers, the TSP tail with the
    GroupNorm partials, the MIS tail, max aggregation; Gaussian TSP takes the generated-input embedding and no layer-0 fold."""
    ref, run = _case(name, Lyr)
    _check_class(f"{name} L={Lyr}", run(precision="fp16x1").cpu(), _emulated(ref), ref())


def test_l0_fold_and_no_fold_agree(dev):
    """The layer-0 fold (C on the two table rows) and the unfolded first layer (C on every e tile) share the contract."""
    from difusco_amd import _lib
    ref, run = _case("tsp_cat", 3)
    r32, emu = ref(), _emulated(ref)
    a = run(precision="fp16x1").cpu()
    b = run(precision="fp16x1", flags=_lib.FLAG_NO_L0_FOLD).cpu()
    _check_class("tsp_cat L=3 no L0 fold", b, emu, r32)
    d = (emu.double() - r32.double()).abs().max().item()
    print(f"fold vs no fold L_inf {(a - b).abs().max().item():.2e}")
    assert (a - b).abs().max().item() <= 2 * d + 1e-5


# ---- 4. the unfused kernel sequence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tsp_cat", "mis_cat", "tsp_gau"])
def test_unfused_equals_fused_fp16x1(dev, name):
    ref, run = _case(name, 3)
    r32, emu = ref(), _emulated(ref)
    a = run(precision="fp16x1").cpu()
    b = run(precision="fp16x1", fused=False).cpu()
    _check_class(f"{name} L=3 unfused", b, emu, r32)
    d = (emu.double() - r32.double()).abs().max().item()
    print(f"{name}: fused vs unfused fp16x1 L_inf {(a - b).abs().max().item():.2e}")
    assert (a - b).abs().max().item() <= 2 * d + 1e-5


@pytest.mark.parametrize("name", ["tsp_cat", "mis_cat"])
def test_h64_unfused_fp16x1_against_emulated_network(dev, name):
    ref, run = _case(name, 2, H=64)
    _check_class(f"H=64 {name} L=2", run(precision="fp16x1").cpu(), _emulated(ref), ref())


# ---- 5. / 6. bindings, determinism, graph capture -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tsp_cat", "mis_cat", "tsp_gau"])
def test_backends_and_repeats_are_bitwise_equal(dev, name):
    _, run = _case(name, 3)
    a, b = run(precision="fp16x1", backend="ctypes"), run(precision="fp16x1", backend="torch")
    c = run(precision="fp16x1", backend="torch")
    assert torch.equal(a, b) and torch.equal(b, c)


def test_fp16x1_step_is_graph_capturable(dev):
    from difusco_amd import TSPModel
    H, Lyr = 256, 3
    p = O.init_params(H, Lyr, 2, seed=131)
    pts, ei = O.tsp_instance(96, 12, seed=14)
    pts, ei = torch.from_numpy(pts).to(dev), torch.from_numpy(ei).to(dev)
    m = TSPModel(_args("categorical", 12, H=H, L=Lyr), p, device=dev, precision="fp16x1")
    g = torch.Generator().manual_seed(5)
    u = torch.rand(ei.shape[1], generator=g).to(dev)
    x0 = (torch.randn(ei.shape[1], generator=g) > 0).float().to(dev)
    step = lambda x: m.categorical_denoise_step(pts, x, np.array([700]), dev, ei, target_t=np.array([650]), uniform=u,
                                                return_aux=True)
    x1, _, _ = step(x0)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        out, logits, prob = step(x1)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    ref_out, ref_logits, ref_prob = step(x1)
    assert torch.equal(logits, ref_logits) and torch.equal(prob, ref_prob) and torch.equal(out, ref_out)


# ---- 7. batched instances keep their solo results ------------------------------------------------------------------------------
def _model(cls, diffusion, hidden, dev, seed, sparse_factor=8):
    from difusco_amd.engine import DenoiseEngine
    p = O.init_params(hidden, 2, 2 if diffusion == "categorical" else 1, seed=0)
    eng = DenoiseEngine(p, device=dev, precision="fp16x1")
    args = dict(diffusion_type=diffusion, diffusion_schedule="linear", diffusion_steps=1000, sparse_factor=sparse_factor,
                n_layers=2, hidden_dim=hidden, inference_trick="ddim", inference_diffusion_steps=5, inference_schedule="cosine")
    return cls(args, engine=eng, seed=seed)


def test_tsp_sample_batch_fp16x1_matches_solo(dev):
    from difusco_amd import TSPModel
    seeds, P, sizes = [3, 4, 5], 2, [60, 90, 76]
    pts_rep, ei_rep = [], []
    for i, n in enumerate(sizes):
        p, e = O.tsp_instance(n, 8, seed=20 + i)
        p, e = torch.from_numpy(p), torch.from_numpy(e)
        pts_rep.append(p.repeat(P, 1).to(dev))
        ei_rep.append((e.reshape(2, 1, -1) + torch.arange(P).view(1, -1, 1) * n).reshape(2, -1).to(dev))
    gens = [torch.Generator().manual_seed(100 + b) for b in range(3)]
    heats = _model(TSPModel, "categorical", 256, dev, 0).sample_batch(pts_rep, ei_rep, seeds=seeds, generators=gens)
    for b in range(3):
        hs = _model(TSPModel, "categorical", 256, dev, seeds[b]).sample(pts_rep[b], ei_rep[b],
                                                                       generator=torch.Generator().manual_seed(100 + b))
        d = (heats[b] - hs).abs()
        print(f"TSP instance {b}: max |batched - solo| {d.max().item():.2e}")
        assert int((d > 1e-5).sum()) <= max(2, hs.numel() // 1000)      # the standard of test_gpu_batch_solve.py


def test_mis_sample_batch_fp16x1_matches_solo(dev):
    from difusco_amd import MISModel
    from difusco_amd.synthetic import er_mis_edge_index
    inst = [(n, torch.from_numpy(er_mis_edge_index(n, 0.08, seed=30 + i))) for i, n in enumerate([150, 260, 90])]
    seeds = [9, 10, 11]
    xt0 = [torch.randn(n, generator=torch.Generator().manual_seed(7 + b)) for b, (n, _) in enumerate(inst)]
    heats = _model(MISModel, "categorical", 64, dev, 0).sample_batch([n for n, _ in inst], [e.to(dev) for _, e in inst],
                                                                     seeds=seeds, xt0=xt0)
    for b, (n, e) in enumerate(inst):
        hs = _model(MISModel, "categorical", 64, dev, seeds[b]).sample(n, e.to(dev), xt0=xt0[b])
        d = (heats[b] - hs).abs()
        print(f"MIS instance {b}: max |batched - solo| {d.max().item():.2e}")
        assert int((d > 1e-5).sum()) <= max(2, hs.numel() // 1000)      # the standard of test_gpu_batch_solve.py


def test_solve_tsp_batch_fp16x1_matches_solo(dev):
    from difusco_amd import TSPModel
    from difusco_amd.pipeline import solve_tsp, solve_tsp_batch
    B, n, P = 3, 50, 2
    pts = np.random.default_rng(12).random((B, n, 2))
    seeds = [21, 22, 23]
    res = solve_tsp_batch(_model(TSPModel, "categorical", 256, dev, 0), pts, 8, parallel_sampling=P, sequential_sampling=2,
                          two_opt_iterations=100, seeds=seeds, generators=[torch.Generator().manual_seed(b) for b in range(B)])
    for b in range(B):
        tour, cost, costs, info = solve_tsp(_model(TSPModel, "categorical", 256, dev, seeds[b]), pts[b], 8, parallel_sampling=P,
                                            sequential_sampling=2, two_opt_iterations=100,
                                            generator=torch.Generator().manual_seed(b))
        assert res[b][0] == tour and res[b][1] == cost and res[b][2] == costs, b
