"""CPU reference of the MXFP6 format the opt-in DiT linears use (OCP MX v1.0, e2m3 elements, E8M0 scales per 32 k of a row), in fp64.

    e2m3: 1 sign, 2 exponent, 3 mantissa bits, bias 1: subnormals m/8, normals 2^(e-1)(1 + m/8), maximum 7.5, no Inf / NaN codes
    X = floor(log2(amax of the block)) - 2, scale byte X + 127 clamped to 0..254 (all-zero block: byte 127, codes 0)
    a block that holds a NaN or an infinity: scale byte 0xFF (the E8M0 NaN: the whole block is NaN), codes 0
    code = RNE(clamp(x / 2^X, -7.5, 7.5)); the sign bit is the sign bit of x, so a negative value that rounds to zero is the code 0x20 (-0)
    storage: q [M, 3K/4] uint8, block b of a row = bytes [24 b, 24 b + 24), element i = bits [6 i, 6 i + 6) of that 192-bit little-endian string

Used by tests/test_mxfp6_cpu.py (pinned on hand cases) and the GPU tests (the HIP quantiser must match it bitwise, and the fake-quantised fp32
DiT oracle is built from it).
"""
from __future__ import annotations

import torch

BLOCK = 32
E2M3_MAX = 7.5
SCALE_NAN = 0xFF


def e2m3_values() -> torch.Tensor:
    """fp64 value of each of the 64 codes (code 0x20 is -0.0)."""
    c = torch.arange(64)
    e, m = (c >> 3) & 3, (c & 7).double()
    mag = torch.where(e == 0, m / 8.0, torch.pow(2.0, (e - 1).double()) * (1.0 + m / 8.0))
    return torch.where((c & 0x20) != 0, -mag, mag)


def e2m3_encode(y: torch.Tensor) -> torch.Tensor:
    """uint8 codes of RNE(y) for fp64 y with |y| <= 7.5; the sign bit of y is kept (also for results that round to zero)."""
    a = y.abs()
    _, ex = torch.frexp(a)  # a = m 2^ex, m in [0.5, 1)
    e = (ex - 1).clamp(min=0)  # max(floor(log2 a), 0); a = 0 gives ex = 0 -> e = 0
    q = torch.round(a * torch.pow(2.0, (3 - e).double()))  # torch.round is half-to-even; a 2^(3-e) is exact in fp64
    code = (8 * e + q.long()).to(torch.uint8)  # q = 16 carries into the next exponent by itself
    return code | (torch.signbit(y).to(torch.uint8) << 5)


def quant_mxfp6_codes(x: torch.Tensor):
    """x [M, K] (any float dtype) -> (codes [M, K] uint8 in 0..63, scales [M, K/32] uint8), on the CPU."""
    M, K = x.shape
    assert K % BLOCK == 0
    xb = x.detach().cpu().double().reshape(M, K // BLOCK, BLOCK)
    bad = ~torch.isfinite(xb).all(-1)  # a NaN or an infinity anywhere in the block
    xb = torch.where(bad.unsqueeze(-1), torch.zeros_like(xb), xb)
    amax = xb.abs().amax(-1)
    _, ex = torch.frexp(amax)  # floor(log2 amax) = ex - 1 (exact for subnormals too)
    X = torch.where(amax > 0, (ex - 1 - 2).clamp(-127, 127), torch.zeros_like(ex))
    y = (xb * torch.pow(2.0, -X.double()).unsqueeze(-1)).clamp(-E2M3_MAX, E2M3_MAX)  # exact in fp64: at most 8 significant bits
    codes = e2m3_encode(y)
    codes = torch.where((amax > 0).unsqueeze(-1), codes, torch.zeros_like(codes))  # an all-zero block has zero codes, whatever its signs
    return codes.reshape(M, K), torch.where(bad, torch.full_like(X, SCALE_NAN), X + 127).to(torch.uint8)


def pack_e2m3(codes: torch.Tensor) -> torch.Tensor:
    """codes [M, K] uint8 (0..63) -> [M, 3K/4] uint8: 4 codes c0..c3 are the 24-bit little-endian integer c0 | c1 << 6 | c2 << 12 | c3 << 18,
    which is element i at bits [6 i, 6 i + 6) of every 24-byte block."""
    M, K = codes.shape
    assert K % 4 == 0
    c = codes.to(torch.int64).reshape(M, K // 4, 4)
    v = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return torch.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], dim=-1).to(torch.uint8).reshape(M, K // 4 * 3)


def unpack_e2m3(q: torch.Tensor) -> torch.Tensor:
    """[M, 3K/4] uint8 -> codes [M, K] uint8."""
    M, B = q.shape
    assert B % 3 == 0
    b = q.to(torch.int64).reshape(M, B // 3, 3)
    v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack([(v >> (6 * i)) & 0x3F for i in range(4)], dim=-1).to(torch.uint8).reshape(M, B // 3 * 4)


def quant_mxfp6_ref(x: torch.Tensor):
    """x [M, K] -> (q [M, 3K/4] uint8 packed, scales [M, K/32] uint8), on the CPU."""
    codes, s = quant_mxfp6_codes(x)
    return pack_e2m3(codes), s


def dequant_mxfp6(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Exact fp32 value of a packed MXFP6 matrix [M, 3K/4] (also exactly representable in bf16 for |X| <= 120); a block with scale byte 0xFF is NaN."""
    codes = unpack_e2m3(q.cpu())
    M, K = codes.shape
    v = e2m3_values()[codes.long()].reshape(M, K // BLOCK, BLOCK)
    s = torch.pow(2.0, scales.cpu().double() - 127.0)
    s = torch.where(scales.cpu() == SCALE_NAN, torch.full_like(s, float("nan")), s)  # the E8M0 NaN
    return (v * s.unsqueeze(-1)).reshape(M, K).float().to(q.device)


def fake_quant6(x: torch.Tensor) -> torch.Tensor:
    """dequant(quant(x)) in fp32 on x's device: what an MXFP6 linear sees of x."""
    q, s = quant_mxfp6_ref(x.reshape(-1, x.shape[-1]))
    return dequant_mxfp6(q, s).reshape(x.shape).to(x.device)
