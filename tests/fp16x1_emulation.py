"""CPU emulation of the DIFUSCO_PREC_FP16X1 contract (include/difusco_hip.h): each operand of an edge-row GEMM product is scaled
by a power of two, rounded once to fp16 (round to nearest even) and multiplied exactly; the sum is taken in float64 here.

A power-of-two scale changes the exponent only, so for every operand that stays a normal fp16 number after scaling (all but
elements more than 2^28 below the largest of their scaling group) the rounded value is the operand rounded to 11 significand
bits with an unbounded exponent: ``fp16_round`` below, which needs no scale at all."""
import torch
import torch.nn.functional as F



def fp16_round(x: torch.Tensor) -> torch.Tensor:
    """float64 tensor: x rounded to 11 significand bits (RNE), exponent unbounded."""
    m, e = torch.frexp(x.double())                      # x = m 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)     # torch.round: half to even


def fp16_round_scaled(x: torch.Tensor, scale) -> torch.Tensor:
    """float64 tensor: x * scale rounded to torch.float16, divided by scale again (scale: a power of two)."""
    s = torch.as_tensor(scale, dtype=torch.float32)
    return (x.float() * s).to(torch.float16).double() / s.double()


def linear_fp16x1(x: torch.Tensor, w: torch.Tensor, b=None) -> torch.Tensor:
    """y = fp16(x) fp16(w)^T (+ b) in float64 (the value a one-product fp16 GEMM approximates up to fp32 accumulation)."""
    y = fp16_round(x) @ fp16_round(w).t()
    return y if b is None else y + b.double()


def is_edge_gemm(name: str) -> bool:
    """True for the two Linears whose products FP16X1 rounds: layers.{l}.C and per_layer_out.{l}.2."""
    parts = name.split(".")
    return (len(parts) == 3 and parts[0] == "layers" and parts[2] == "C") or \
           (len(parts) == 3 and parts[0] == "per_layer_out" and parts[2] == "2")


def emulating_lin(orig):
    """A replacement for oracle.difusco_oracle._lin that rounds the operands of the edge-row GEMMs only (monkeypatch it in)."""
    def _lin(p, name, x):
        if not is_edge_gemm(name):
            return orig(p, name, x)
        return linear_fp16x1(x, p[name + ".weight"], p[name + ".bias"]).to(x.dtype)
    return _lin
