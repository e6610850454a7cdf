"""The deferred-epilogue GEMM's K loop on v_mfma_f32_16x16x32_bf16 (g3_set_option("gemm_mfma16", 1): gemm_bf16_nt_w4e16_kernel, csrc/gemm_w4e.hpp +
gemm_w4e16_gen.hpp) against the 32x32x16 body and against the non-persistent one-wave kernel (gemm_deferred = 0): the same bits, at the smallest
shapes where the body can go wrong - the minimum of 38 K tiles with two tiles per workgroup, two or three tiles per workgroup, and 528 tiles on 8 and on
248 workgroups (66 carried epilogues in a row; a flush behind a carry) - for the three epilogue classes, gate_rows 1 / 2 / 4 and both piece orders.
Every launch is made twice; every output is a column view of a wider buffer of NaNs, which must stay NaN around it."""
import math

import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

# (M, N, K, gemm_deferred_grid)
SHAPES = [(8192, 4096, 2432, 0), (8448, 4096, 4096, 0), (8448, 4096, 2560, 8), (8448, 4096, 2560, 248)]
EPILOGUES = [(0, 1), (1, 1), (2, 1), (2, 2), (2, 4)]
PAD = 128  # guard columns on either side of an output


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _restore(ops, mfma16):
    ops.set_option("gemm_mfma16", mfma16)
    ops.set_option("gemm_deferred", 1)
    ops.set_option("gemm_deferred_grid", 0)
    ops.set_option("gemm_tokens_first", 2)


def _guarded(M, N, dev):
    buf = torch.full((M, N + 2 * PAD), float("nan"), device=dev, dtype=torch.bfloat16)
    return buf, buf[:, PAD:PAD + N]


def _run(ops, a, w, epi, kw, what):
    """One launch into a fresh guarded view, twice; -> the output (a copy), checked finite, reproducible and inside its view."""
    M, N = a.shape[0], w.shape[0]
    outs = []
    for _ in range(2):
        buf, out = _guarded(M, N, a.device)
        ops.gemm_nt(a, w, out=out, epilogue=epi, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:, :PAD]).all()) and bool(torch.isnan(buf[:, PAD + N:]).all()), f"{what}: wrote outside its view"
        assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).sum())} elements not written or not finite"
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1]), f"{what}: not reproducible"
    return outs[0]


def _same(got, ref, what):
    bad = gr.bits_of(got) != gr.bits_of(ref)
    n = int(bad.sum())
    assert n == 0, (f"{what}: {n} of {got.numel()} elements differ, first at row {int(bad.any(dim=1).nonzero()[0])} column {int(bad.any(dim=0).nonzero()[0])}, "
                    f"max |diff| {float((got.float() - ref.float()).abs().max()):.3e}")


@pytest.mark.parametrize("M,N,K,grid", SHAPES)
@pytest.mark.parametrize("epi,gate_rows", EPILOGUES)
def test_mfma16_body_equals_the_wide_body_and_the_plain_kernel_bitwise(M, N, K, grid, epi, gate_rows):
    from gen3c_amd import _lib, ops
    dev = _dev()
    assert _lib.load().g3_gemm_kernel_name(M, N, K, epi).decode() == "gemm_bf16_nt_w4e_kernel<EPI>"
    default = ops.option("gemm_mfma16")
    g = torch.Generator(device=dev).manual_seed(16 + M + 3 * N + 7 * K + 11 * grid + epi + gate_rows)
    a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    kw = dict(gate=torch.randn(gate_rows, N, device=dev, generator=g).to(torch.bfloat16),
              residual=torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)) if epi == 2 else {}
    try:
        ops.set_option("gemm_deferred", 0)
        plain = _run(ops, a, w, epi, kw, "gemm_deferred = 0")
        ops.set_option("gemm_deferred", 1)
        ops.set_option("gemm_deferred_grid", grid)
        for tf in (0, 1):
            ops.set_option("gemm_tokens_first", tf)
            for m16 in (0, 1):
                ops.set_option("gemm_mfma16", m16)
                what = f"gemm_mfma16 = {m16}, gemm_tokens_first = {tf}, grid {grid}"
                _same(_run(ops, a, w, epi, kw, what), plain, what + " against gemm_deferred = 0")
    finally:
        _restore(ops, default)


def test_mfma16_body_in_place_residual_and_column_views():
    """The DiT's gated residual writes x in place (out aliases the residual), x and the activations being column views of wider buffers."""
    from gen3c_amd import ops
    dev = _dev()
    M, N, K = 8192, 4096, 2432
    default = ops.option("gemm_mfma16")
    g = torch.Generator(device=dev).manual_seed(1677)
    a = torch.randn(M, K + 256, device=dev, generator=g).to(torch.bfloat16)[:, 128:128 + K]
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(2, N, device=dev, generator=g).to(torch.bfloat16)
    x0 = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    outs = {}
    try:
        for key, (deferred, m16) in {"plain": (0, 0), "wide": (1, 0), "narrow": (1, 1)}.items():
            ops.set_option("gemm_deferred", deferred)
            ops.set_option("gemm_mfma16", m16)
            for rep in range(2):
                buf, x = _guarded(M, N, dev)
                x.copy_(x0)
                ops.gemm_nt(a, w, out=x, epilogue=2, gate=gate, residual=x)
                torch.cuda.synchronize()
                assert bool(torch.isnan(buf[:, :PAD]).all()) and bool(torch.isnan(buf[:, PAD + N:]).all()) and bool(torch.isfinite(x).all()), key
                if rep:
                    assert torch.equal(outs[key], x), f"{key}: not reproducible"
                outs[key] = x.clone()
    finally:
        _restore(ops, default)
    _same(outs["narrow"], outs["plain"], "in place, gemm_mfma16 = 1 against gemm_deferred = 0")
    _same(outs["narrow"], outs["wide"], "in place, gemm_mfma16 = 1 against gemm_mfma16 = 0")


def test_mfma16_body_is_exact_on_small_integers():
    """Operands in {-3 .. 3} x {-2 .. 2}: every partial sum is an integer below 2^24, so every fp32 sum is exact in any order and the output is the
    bf16 of the exact product (gemm_ref.linear_ref, fp64): a wrong lane, row or k in the fragment map shows whatever the rounding. Two tiles per workgroup:
    the second tile's first K = 32 step must start from C = 0 and the first tile's values leave through the carried epilogue."""
    from gen3c_amd import ops
    dev = _dev()
    M, N, K = 8192, 4096, 2432
    default = ops.option("gemm_mfma16")
    g = torch.Generator(device=dev).manual_seed(1632)
    a = torch.randint(-3, 4, (M, K), device=dev, generator=g).to(torch.bfloat16)
    w = torch.randint(-2, 3, (N, K), device=dev, generator=g).to(torch.bfloat16)
    ref, _ = gr.linear_ref(a, w)
    assert float(ref.abs().max()) < 2 ** 24
    try:
        ops.set_option("gemm_mfma16", 1)
        for tf in (0, 1):
            ops.set_option("gemm_tokens_first", tf)
            _same(_run(ops, a, w, 0, {}, f"small integers, gemm_tokens_first = {tf}"), ref.float().to(torch.bfloat16), "small integers against the exact product")
    finally:
        _restore(ops, default)
