"""CPU reference of the MXFP8 format the opt-in DiT linears use (OCP MX v1.0, e4m3fn elements, E8M0 scales per 32 k of a row).

    X = floor(log2(amax of the block)) - 8, scale byte X + 127 clamped to 0..254 (all-zero block: byte 127, elements 0)
    element = RNE(clamp(x / 2^X, -448, 448)) as e4m3fn
    a block that holds a NaN or an infinity: scale byte 0xFF (the E8M0 NaN: the whole block is NaN), elements 0

Used by tests/test_mxfp8_cpu.py (pinned on hand cases) and tests/test_mxfp8_gpu.py (the HIP quantiser must match it bitwise, and the
fake-quantised fp32 DiT oracle is built from it).
"""
from __future__ import annotations

import torch

BLOCK = 32
SCALE_NAN = 0xFF  # E8M0 has no infinity and one NaN


def e8m0_values() -> torch.Tensor:
    """fp64 value of each of the 256 scale bytes: 2^(b - 127), byte 0xFF is NaN."""
    v = torch.pow(2.0, torch.arange(256).double() - 127.0)
    v[SCALE_NAN] = float("nan")
    return v


def e4m3_values() -> torch.Tensor:
    """fp64 value of each of the 256 e4m3fn codes (0x80 is -0.0, 0x7F and 0xFF are NaN; no infinities)."""
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()


def quant_mxfp8_ref(x: torch.Tensor):
    """x [M, K] (any float dtype) -> (q [M, K] float8_e4m3fn, scales [M, K/32] uint8), on the CPU."""
    M, K = x.shape
    assert K % BLOCK == 0
    xb = x.detach().cpu().double().reshape(M, K // BLOCK, BLOCK)
    bad = ~torch.isfinite(xb).all(-1)  # a NaN or an infinity anywhere in the block
    xb = torch.where(bad.unsqueeze(-1), torch.zeros_like(xb), xb)
    amax = xb.abs().amax(-1)
    _, ex = torch.frexp(amax)  # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1 (exact for subnormals too)
    X = torch.where(amax > 0, (ex - 1 - 8).clamp(-127, 127), torch.zeros_like(ex))
    y = (xb * torch.pow(2.0, -X.double()).unsqueeze(-1)).clamp(-448.0, 448.0)  # exact in fp64: at most 8 significant bits
    y = torch.where((amax > 0).unsqueeze(-1), y, torch.zeros_like(y))
    q = y.float().to(torch.float8_e4m3fn).reshape(M, K)  # fp64 -> fp32 is exact wherever the e4m3 result is not zero anyway
    return q, torch.where(bad, torch.full_like(X, SCALE_NAN), X + 127).to(torch.uint8)


def dequant_mxfp8(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Exact fp32 value of an MXFP8 matrix (also exactly representable in bf16 for |X| <= 110); a block with scale byte 0xFF is NaN."""
    M, K = q.shape
    s = torch.pow(2.0, scales.to(torch.float32) - 127.0)
    s = torch.where(scales == SCALE_NAN, torch.full_like(s, float("nan")), s)
    return (q.float().reshape(M, K // BLOCK, BLOCK) * s.unsqueeze(-1).to(q.device)).reshape(M, K)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """dequant(quant(x)) in fp32 on x's device: what an MXFP8 linear sees of x."""
    q, s = quant_mxfp8_ref(x.reshape(-1, x.shape[-1]))
    return dequant_mxfp8(q, s).reshape(x.shape).to(x.device)
