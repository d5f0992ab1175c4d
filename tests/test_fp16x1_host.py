"""CPU tests of precision fp16x1 (DIFUSCO_PREC_FP16X1): the binding and the header agree, unknown precisions are still refused
before any GPU work, and the test-side emulation of the contract (tests/fp16x1_emulation.py) is itself right."""
import ctypes
import os
import re

import pytest
import torch

from difusco_amd import _lib
from oracle import difusco_oracle as O
from tests import fp16x1_emulation as EMU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_enum(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difusco_hip.h")).read(), flags=re.S)
    return int(re.search(rf"\b{name}\s*=\s*(\d+)", hdr).group(1))


def test_binding_and_header_agree_on_fp16x1():
    assert _lib.PRECISIONS["fp16x1"] == _lib.PREC_FP16X1 == 4
    assert _header_enum("DIFUSCO_PREC_FP16X1") == 4
    for name, v in _lib.PRECISIONS.items():
        assert _header_enum("DIFUSCO_PREC_" + name.upper()) == v
    assert "fp16x1" in _lib.FUSED_PRECISIONS
    assert _lib.ABI_VERSION == 13 and _lib.lib().difusco_abi_version() == 13      # additive: no ABI bump


def test_default_precision_is_unchanged():
    import inspect
    from difusco_amd import engine, models
    assert inspect.signature(engine.DenoiseEngine.__init__).parameters["precision"].default == "fp16x3"
    assert inspect.signature(models.COMetaModel.__init__).parameters["precision"].default == "fp16x3"
    assert "fp16" not in models._DEFAULTS      # the reference's --fp16 is not read: fp16x1 is opt-in through precision=


def _step_args(precision):
    a = _lib.StepArgs()
    a.struct_size, a.abi_version = ctypes.sizeof(_lib.StepArgs), _lib.ABI_VERSION
    a.hidden, a.n_layers, a.out_channels, a.task = 256, 12, 2, _lib.TASK_TSP
    a.diffusion, a.n_nodes, a.n_edges, a.n_segments = _lib.CATEGORICAL, 10, 20, 1
    for name in ("weights", "rowptr", "col", "xt", "xt_out", "workspace", "points", "row"):
        setattr(a, name, 0x1000)            # never dereferenced: validation fails first
    a.workspace_bytes = 1 << 40
    a.precision = precision
    a.post[4] = 1.0
    a.rand_mode = _lib.RAND_PHILOX
    return a


@pytest.mark.parametrize("bad", [5, -1])
def test_unknown_precision_is_refused(bad):
    L = _lib.lib()
    assert L.difusco_denoise_step(ctypes.byref(_step_args(bad))) == -1      # DIFUSCO_EINVAL
    assert "unknown precision" in L.difusco_last_error().decode()
    p = ctypes.c_void_p(0x1000)
    assert L.difusco_linear_rows_split(p, p, bad, None, None, p, 4, 256, 256, 256, None, None) == -1
    assert "precision" in L.difusco_last_error().decode()
    args = [p] * 4
    assert L.difusco_edge_layer_fused(bad, 10, 20, *args, p, p, p, p, p, p, p, p, p, p, p, p, p, 1, p, p, None) == -1
    assert "precision" in L.difusco_last_error().decode()


def test_edge_embed_still_refuses_fp16x1():
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    assert L.difusco_edge_embed(256, 2, 2, p, _lib.PREC_FP16X1, p, None, 32, p, None, None, None) == -1
    assert "precision" in L.difusco_last_error().decode()


def test_scaled_rne_rounding_matches_torch_float16():
    g = torch.Generator().manual_seed(0)
    # normal fp16 values: magnitudes 2^-14 .. 2^15, random significands, plus exact halfway cases (ties to even)
    x = (torch.rand(200000, generator=g) * 29 - 14).exp2() * torch.sign(torch.randn(200000, generator=g))
    ties = (torch.randint(1024, 2048, (1000,), generator=g).float() + 0.5) * 2.0 ** -10
    x = torch.cat([x, ties, -ties]).float()
    ref = x.to(torch.float16).double()
    assert torch.equal(EMU.fp16_round(x), ref)
    # power-of-two scales move the exponent only: the rounding of x 2^k, undone, is the same rounding
    for k in (-20, -3, 0, 7, 30):
        y = x * 2.0 ** -k
        assert torch.equal(EMU.fp16_round_scaled(y, 2.0 ** k), EMU.fp16_round(y))
    # the weight scale of weights.split_planes: its fp16 hi plane is that rounding of w 2^k
    from difusco_amd import weights
    w = torch.randn(64, 64, generator=g) / 8
    s = weights.pow2_scale(w.abs().amax().reshape(1))[0]
    assert torch.equal(EMU.fp16_round_scaled(w, s), EMU.fp16_round(w))


def test_products_of_rounded_operands_are_exact_in_fp32():
    g = torch.Generator().manual_seed(1)
    a = EMU.fp16_round(torch.randn(100000, generator=g) * 1000)
    b = EMU.fp16_round(torch.randn(100000, generator=g) / 1000)
    assert torch.equal((a.float() * b.float()).double(), a * b)      # 11 + 11 significand bits fit the 24 of fp32


def test_emulating_lin_rounds_the_edge_gemms_only(monkeypatch):
    assert EMU.is_edge_gemm("layers.3.C") and EMU.is_edge_gemm("per_layer_out.11.2")
    assert not any(EMU.is_edge_gemm(n) for n in ("layers.3.A", "edge_embed", "node_embed", "per_layer_out.1.0",
                                                  "time_embed_layers.2.1", "layers.0.U"))
    p = O.init_params(64, 2, 2, seed=3)
    pts, ei = O.tsp_instance(30, 5, seed=1)
    pts, ei = torch.from_numpy(pts), torch.from_numpy(ei)
    xt = (torch.randn(ei.shape[1], generator=torch.Generator().manual_seed(2)) > 0).float()
    t = torch.tensor([500.0])
    ref = O.encoder_sparse_edge(p, pts, xt, t, ei)
    monkeypatch.setattr(O, "_lin", EMU.emulating_lin(O._lin))
    emu = O.encoder_sparse_edge(p, pts, xt, t, ei)
    d = (emu - ref).abs().max().item()
    assert 1e-6 < d < 0.05 * ref.abs().max().item(), d      # a real, small difference: fp16 operands in two Linears per layer
