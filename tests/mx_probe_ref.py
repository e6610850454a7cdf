"""Exact probes for the MX quantisers and block-scaled GEMMs (gemm_mx.hip, mx_quant.hpp), their fp64 references, the bars and a numpy model
of the kernels' index bookkeeping (TEST INFRASTRUCTURE - a plain helper module; tests/test_mx_probe_ref_cpu.py checks it,
tests/test_mx_kernels_gpu.py uses it).

An operand is (codes [R][K] uint8, scales [R][K / 32] uint8): one e4m3fn code (MXFP8) or one e2m3 code 0..63 (MXFP6, unpacked) per element and
one E8M0 byte per 32 k of a row. Its value is table[code] * 2^(byte - 127), byte 0xFF = NaN (tests/mxfp8_ref.py, tests/mxfp6_ref.py). Every
probe below is built so that its expected output is a closed form, stated with the builder, and - the accumulation family E apart - so that
the sum of the absolute terms of every output stays below 2^24 units of its smallest term: every partial sum in every order is then exact in
fp32, and the kernel has exactly one right answer, bf16_round(exact).

Families (the GPU file runs each for both formats):
  A census_codes      one non-zero code per row (row r holds code r mod 256 / 64 at k = r mod 128), the other operand 1.0: the decode table.
  B scale_grid        1.5 x 1.0 at k = 0 under the scale bytes (m, n): 1.5 * 2^(m + n - 254) on the whole 256 x 256 grid of byte pairs.
  C census_position   weight row n one-hot at k = n (K <= 512), or 1.0 over block n / one-hot inside block n (K = 16384): which k meets which
                      k under which scale pair, with scale bytes 127 +- 40 that a neighbour's byte cannot imitate.
  D dense_integers    integers in [-4, 4], scale bytes 127 +- 2, every element non-zero work: every epilogue and the MXFP8 output.
  E align_probe       one product 2^p beside 63 (or 32) products of 1, cancelled by -2^p later: what the matrix core keeps of small addends;
    gaussian          Gaussian data with outlier channels through the reference quantiser, every output against fp64.
  F quant_sweep       every finite bf16 value under five planted block maxima; non-finite inputs.

The bars that are not "bitwise": the GELU epilogue is held with gemm_ref's check (C_GELU); family E's Gaussian cases with
|out - ref| <= 0.5 bf16_ulp(ref) + C_ACC * sum |a w|, C_ACC twice the worst figure measured against fp64 on those seeded cases (c_acc below)."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from tests import mxfp6_ref, mxfp8_ref
from tests.gemm_ref import (C_GELU, EPI_GATED_RESIDUAL, EPI_GELU, EPI_NONE, bits_of, check, check_sweep, gated_fp32, gated_ref,  # noqa: F401
                            gelu_fast32, gelu_ref)
from tests.tokenizer_kernel_ref import bf16_round, bf16_ulp  # noqa: F401

bf16 = torch.bfloat16
BLOCK = 32
BK = 128                 # k per K tile of the kernels
BM = BN = 256            # the workgroup tile
SCALE_ONE = 127
SCALE_NAN = 0xFF

# (M, N, K) of the GPU suite: the smallest shape of each mechanism
ONE_TILE = (256, 256, 128)       # one tile, one K tile, no stage reuse
ONE_ROW = (1, 256, 128)          # every token row clamps to row 0
ROW_TAIL = (257, 256, 256)       # a one-row second M tile
ODD_KTILES = (300, 512, 384)     # an odd number of K tiles
TAIL_GROUP = (1100, 768, 512)    # 15 tiles: no multiple of 8 (the XCD remap's remainder), and a one-tile tail group of token tiles
DEEP = (64, 512, 16384)          # 128 K tiles: the w2 depth
SHAPES = [ONE_TILE, ONE_ROW, ROW_TAIL, ODD_KTILES, TAIL_GROUP, DEEP]


# =================================================================================================================================
# formats and code tables
# =================================================================================================================================
@dataclasses.dataclass(frozen=True)
class Fmt:
    name: str
    ncodes: int
    one: int        # code of 1.0
    one_half: int   # code of 1.5
    neg_zero: int
    pad: int        # the hostile byte behind every operand row: an e4m3 NaN code / the byte 0x1F
    nan_codes: tuple

    def values(self) -> torch.Tensor:
        return mxfp8_ref.e4m3_values() if self.ncodes == 256 else mxfp6_ref.e2m3_values()

    def row_bytes(self, K: int) -> int:
        return K if self.ncodes == 256 else K // 4 * 3

    def pack(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [R][K] uint8 -> the bytes of the rows in memory [R][row_bytes(K)] uint8"""
        return codes if self.ncodes == 256 else mxfp6_ref.pack_e2m3(codes)

    def encode_ints(self, v: torch.Tensor) -> torch.Tensor:
        """codes of values that the format holds exactly (0 is code 0)"""
        tab = self.values()
        keep = [c for c in range(self.ncodes) if not math.isnan(float(tab[c])) and c != self.neg_zero]
        vals, order = torch.sort(tab[keep])
        idx = torch.searchsorted(vals, v.double().reshape(-1)).clamp(max=len(keep) - 1)
        assert bool((vals[idx] == v.double().reshape(-1)).all()), "a value the format does not hold"
        return torch.tensor(keep, dtype=torch.uint8)[order][idx].reshape(v.shape)


FP8 = Fmt("mxfp8", 256, 0x38, 0x3C, 0x80, 0x7F, (0x7F, 0xFF))
FP6 = Fmt("mxfp6", 64, 0x08, 0x0C, 0x20, 0x1F, ())
FMTS = {"mxfp8": FP8, "mxfp6": FP6}

e8m0_values = mxfp8_ref.e8m0_values


def dequant(codes: torch.Tensor, scales: torch.Tensor, fmt: Fmt) -> torch.Tensor:
    """fp64 value of an operand [R][K]"""
    R, K = codes.shape
    v = fmt.values()[codes.long()].reshape(R, K // BLOCK, BLOCK)
    return (v * e8m0_values()[scales.long()].unsqueeze(-1)).reshape(R, K)


# =================================================================================================================================
# the fp64 GEMM reference and its epilogues
# =================================================================================================================================
def gemm_ref64(a: torch.Tensor, w: torch.Tensor):
    """a [M][K], w [N][K] fp64 operand values -> (a @ w^T, sum_k |a w|) in fp64"""
    return a @ w.t(), a.abs() @ w.abs().t()


def epilogue_expect(y: torch.Tensor, epilogue: int, gate=None, residual=None):
    """What follows the Linear's rounded output y (bf16, the EPI_NONE result): -> (bitwise expectation or None, (ref, E) of the fp64 stage).
    NONE: y itself. GATED_RESIDUAL: bf16(fp32(R + g y)) - g y is exact in fp32, one right answer. GELU: no bitwise answer; gelu_ref's bound."""
    if epilogue == EPI_NONE:
        return y, None
    if epilogue == EPI_GATED_RESIDUAL:
        return gated_fp32(y, gate, residual), gated_ref(y, gate, residual)
    return None, gelu_ref(y)


def mxout_expect(y: torch.Tensor):
    """the MXFP8-output form: the reference quantiser on the bf16 tensor the plain entry stores -> (codes uint8, scales uint8)"""
    q, s = mxfp8_ref.quant_mxfp8_ref(y)
    return q.view(torch.uint8), s


# =================================================================================================================================
# probes
# =================================================================================================================================
@dataclasses.dataclass
class Probe:
    name: str
    fmt: Fmt
    ac: torch.Tensor   # [M][K] codes
    as_: torch.Tensor  # [M][K / 32]
    wc: torch.Tensor   # [N][K]
    ws: torch.Tensor   # [N][K / 32]
    expect: torch.Tensor        # fp64 [M][N]: the closed form
    statement: str              # why `expect` is exact
    rounded: bool = False       # the closed form is not a bf16 value; the expectation is its one rounding
    asserted: torch.Tensor | None = None  # bool [M][N]: the outputs held bitwise (None: all)
    order_free: bool = True     # sum |terms| < 2^24 units of the smallest term (family E's alignment probe is the exception, on purpose)

    @property
    def shape(self):
        return self.ac.shape[0], self.wc.shape[0], self.ac.shape[1]

    def values(self):
        return dequant(self.ac, self.as_, self.fmt), dequant(self.wc, self.ws, self.fmt)

    def expect_bits(self) -> torch.Tensor:
        """uint16 patterns of the expected bf16 output; every NaN is 0x7FC0 (compare with same_bits)"""
        e = bf16_round(self.expect)
        e = torch.where(e == 0, torch.zeros_like(e), e)  # a sum of +0 products and one -0 is +0 in round-to-nearest
        return canon_bits(e)


def canon_bits(t: torch.Tensor) -> torch.Tensor:
    b = bits_of(t.cpu())
    return torch.where(torch.isnan(t.cpu().float()), torch.full_like(b, 0x7FC0), b)


def _ones(fmt: Fmt, R: int, K: int):
    return torch.full((R, K), fmt.one, dtype=torch.uint8), torch.full((R, K // BLOCK), SCALE_ONE, dtype=torch.uint8)


def _rng(*key) -> torch.Generator:
    return torch.Generator().manual_seed(7919 + sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)))


def census_codes(fmt: Fmt, side: str, shape=ONE_TILE) -> Probe:
    """Family A. Row r of the census operand holds code (r + r // ncodes) mod ncodes at k = r mod 128 (+ 128 (r // 128 mod K tiles)) - every k of
    a K tile meets a non-zero code, every code a row - under the scale byte
    127 + (r mod 7) - 3, every other element code 0; the other operand is 1.0 everywhere under scale 127. One non-zero product per output:
    table[code] * 2^(byte - 127), an e4m3 / e2m3 value times a power of two - exactly a bf16 value. NaN codes give NaN, -0 gives +0."""
    M, N, K = shape
    R, O = (M, N) if side == "a" else (N, M)
    r = torch.arange(R)
    codes = torch.zeros(R, K, dtype=torch.uint8)
    code = (r + r // fmt.ncodes) % fmt.ncodes
    codes[r, (r % BK + BK * (r // BK)) % K] = code.to(torch.uint8)
    scales = torch.full((R, K // BLOCK), SCALE_ONE, dtype=torch.uint8)
    byte = (SCALE_ONE + r % 7 - 3).to(torch.uint8)
    scales[:] = byte.unsqueeze(1)
    row = fmt.values()[code] * e8m0_values()[byte.long()]
    oc, os_ = _ones(fmt, O, K)
    if side == "a":
        return Probe(f"census_codes[a] {fmt.name}", fmt, codes, scales, oc, os_, row.unsqueeze(1).expand(M, N).clone(), "one product per output")
    return Probe(f"census_codes[w] {fmt.name}", fmt, oc, os_, codes, scales, row.unsqueeze(0).expand(M, N).clone(), "one product per output")


def scale_grid(fmt: Fmt) -> Probe:
    """Family B. a[m][0] = 1.5 under scale byte m, w[n][0] = 1.0 under scale byte n, everything else code 0 under byte 127: output (m, n) is the
    one product 1.5 * 2^(m + n - 254). Asserted bitwise where that is a normal bf16 value and neither byte is 0xFF; column n = 127 and row
    m = 127 are the census of one operand's scale byte alone. The rest - the two ends beyond bf16's normal range and byte 0xFF - is reported."""
    M, N, K = ONE_TILE
    ac, wc = torch.zeros(M, K, dtype=torch.uint8), torch.zeros(N, K, dtype=torch.uint8)
    ac[:, 0], wc[:, 0] = fmt.one_half, fmt.one
    as_, ws = torch.full((M, K // BLOCK), SCALE_ONE, dtype=torch.uint8), torch.full((N, K // BLOCK), SCALE_ONE, dtype=torch.uint8)
    as_[:, 0] = torch.arange(M).to(torch.uint8)
    ws[:, 0] = torch.arange(N).to(torch.uint8)
    e = torch.arange(M).view(-1, 1) + torch.arange(N).view(1, -1) - 254
    expect = 1.5 * torch.pow(2.0, e.double())
    nan = (torch.arange(M).view(-1, 1) == SCALE_NAN) | (torch.arange(N).view(1, -1) == SCALE_NAN)
    expect = torch.where(nan, torch.full_like(expect, math.nan), expect)
    return Probe(f"scale_grid {fmt.name}", fmt, ac, as_, wc, ws, expect, "one product per output", asserted=~nan & (e >= -126) & (e <= 127))


def _hostile_scales(R: int, nb: int, *key) -> torch.Tensor:
    return (SCALE_ONE + torch.randint(-40, 41, (R, nb), generator=_rng(*key))).to(torch.uint8)


def _int_operand(fmt: Fmt, R: int, K: int, *key):
    v = torch.randint(-4, 5, (R, K), generator=_rng(*key)).double()
    return v, fmt.encode_ints(v)


def census_position(fmt: Fmt, shape, mode: str = "k") -> Probe:
    """Family C. Tokens: random integers in [-4, 4], scale bytes 127 +- 40 per (row, block) on BOTH operands.
    mode "k" (K <= N): weight row n is 1.0 at k = n (rows n >= K are zero): output (m, n) = a[m][n] 2^(sa[m][n / 32] + sw[n][n / 32] - 254), one product.
    mode "block" (K / 32 <= N): weight row n is 1.0 over block n: the 32-term integer sum of that block (|sum| <= 128, a bf16 value) times the one
    scale pair; all 32 terms share the scale, so the sum is exact in any order, whatever the other blocks' scales are.
    mode "in_block": weight row n is 1.0 at position 7 n mod 32 of block n: one product."""
    M, N, K = shape
    nb = K // BLOCK
    av, ac = _int_operand(fmt, M, K, M, N, K, 1)
    as_, ws = _hostile_scales(M, nb, M, K, 2), _hostile_scales(N, nb, N, K, 3)
    wv = torch.zeros(N, K, dtype=torch.float64)
    n = torch.arange(N)
    if mode == "k":
        assert K <= N
        wv[n[:K], n[:K]] = 1.0
    elif mode == "block":
        assert nb <= N
        wv.view(N, nb, BLOCK)[n[:nb], n[:nb], :] = 1.0
    else:
        assert nb <= N
        wv.view(N, nb, BLOCK)[n[:nb], n[:nb], (7 * n[:nb]) % BLOCK] = 1.0
    wc = fmt.encode_ints(wv)
    expect = (av * e8m0_values()[as_.long()].repeat_interleave(BLOCK, 1)) @ (wv * e8m0_values()[ws.long()].repeat_interleave(BLOCK, 1)).t()
    return Probe(f"census_position[{mode}] {fmt.name} {shape}", fmt, ac, as_, wc, ws, expect, "terms of one block under one scale pair per output")


def dense_integers(fmt: Fmt, shape) -> Probe:
    """Family D. Integers in [-4, 4] on both operands (w[:, 0] += n mod 3, clamped: no symmetry between rows), scale bytes 127 +- 2 per (row,
    block): every term is a multiple of 2^-4 and at most 2^8, so K terms stay below 2^24 units for every K of the suite (the CPU test asserts
    it on the actual sums). The result is not a bf16 value in general: the expectation is its one rounding."""
    M, N, K = shape
    g = _rng(M, N, K, 4)
    a = torch.randint(-4, 5, (M, K), generator=g).double()
    w = torch.randint(-4, 5, (N, K), generator=g).double()
    w[:, 0] = (w[:, 0] + torch.arange(N).double() % 3).clamp(-4, 4)
    as_ = (SCALE_ONE + torch.randint(-2, 3, (M, K // BLOCK), generator=g)).to(torch.uint8)
    ws = (SCALE_ONE + torch.randint(-2, 3, (N, K // BLOCK), generator=g)).to(torch.uint8)
    p = Probe(f"dense_integers {fmt.name} {shape}", fmt, fmt.encode_ints(a), as_, fmt.encode_ints(w), ws, torch.empty(0), "integer terms", rounded=True)
    ad, wd = p.values()
    p.expect = ad @ wd.t()
    return p


POSITION_CASES = [((64, 512, 128), "k"), ((257, 512, 256), "k"), (ODD_KTILES, "k"), ((64, 512, 512), "k"), (DEEP, "block"), (DEEP, "in_block")]


@functools.lru_cache(maxsize=None)
def exact_probes(fmt: Fmt):
    """every probe of the GPU suite with one right answer (families A - D); built once, not to be written to"""
    return ([census_codes(fmt, "a"), census_codes(fmt, "w"), scale_grid(fmt)] + [census_position(fmt, shape, mode) for shape, mode in POSITION_CASES]
            + [dense_integers(fmt, shape) for shape in SHAPES])


def epilogue_operands(M: int, N: int):
    """gate [2][N] (the first `rows` rows are a call's gate) and residual [M][N], bf16"""
    g = _rng(M, N, 5)
    return (torch.rand(2, N, generator=g) + 0.1).to(bf16), torch.randn(M, N, generator=g).to(bf16)


# ---- family E --------------------------------------------------------------------------------------------------------------------
ALIGN_P = 31          # p = 0 .. 30
ALIGN_VARIANTS = ("same_step", "earlier_step", "earlier_tile")
ALIGN_SHAPE = (128, 256, 512)


def _pow2_code(fmt: Fmt, e: int, neg: bool = False) -> int:
    return int(fmt.encode_ints(torch.tensor([-(2.0 ** e) if neg else 2.0 ** e]))[0])


def align_probe(fmt: Fmt, ones: int = 63) -> Probe:
    """Family E, the matrix core's alignment. Output (m, n) with m = 32 v + pa (variant v, pa = 0 .. 15) and pw = n mod 16 holds, for p = pa + pw:
        + 2^p   at k = 0,
        + 1     `ones` times: k = 1 .. 63 of the SAME 64-deep step (same_step), of the NEXT step (k = 64 ..: earlier_step: 2^p arrives through
                the accumulator) or of the next K tile (k = 128 ..: earlier_tile),
        - 2^p   alone in a later step (k = 64 / 128 / 256),
    exactly `ones`. ones = 63 splits p over the element codes of both operands (a 2^xa beside 2^-ya under one block scale; p <= 30 for e4m3,
    <= 10 for e2m3: rows / columns beyond that are left zero); ones = 32 puts 2^p alone in block 0 and the ones in block 1, p by the scale byte.
    fp32 itself holds 2^p + 63 only for p <= 23 (2^p + 32 for p <= 28): the probe is NOT order-free, it measures; see largest_exact_p."""
    M, N, K = ALIGN_SHAPE
    emax, emin = (8, -9) if fmt is FP8 else (2, -3)
    half = (emax - emin) if ones == 63 else 15      # the largest pa / pw
    half = min(half, 15)
    ac, wc = torch.zeros(M, K, dtype=torch.uint8), torch.zeros(N, K, dtype=torch.uint8)
    as_, ws = torch.full((M, K // BLOCK), SCALE_ONE, dtype=torch.uint8), torch.full((N, K // BLOCK), SCALE_ONE, dtype=torch.uint8)
    expect = torch.zeros(M, N, dtype=torch.float64)
    asserted = torch.zeros(M, N, dtype=torch.bool)
    ones_at = {"same_step": 0, "earlier_step": 64, "earlier_tile": 128}
    minus_at = {"same_step": 64, "earlier_step": 128, "earlier_tile": 256}

    def split(p):  # 2^x big, 2^-y small, x + y = p
        x = min(p, emax)
        return x, p - x

    for n in range(N):
        pw = n % 16
        if pw > half:
            continue
        if ones == 63:
            x, y = split(pw)
            for k0 in (0, 64, 128, 256):
                wc[n, k0] = _pow2_code(fmt, x)
            for k0 in (0, 64, 128):
                wc[n, k0 + 1:k0 + 64] = _pow2_code(fmt, -y)
            ws[n, :] = SCALE_ONE + y  # the small elements are 1 after the scale
        else:
            for k0 in (0, 64, 128, 256):
                wc[n, k0] = fmt.one
                ws[n, k0 // BLOCK] = SCALE_ONE + pw
            for k0 in (0, 64, 128):
                wc[n, k0 + 32:k0 + 64] = fmt.one
    for v, variant in enumerate(ALIGN_VARIANTS):
        for pa in range(half + 1):
            m = 32 * v + pa
            o, mi = ones_at[variant], minus_at[variant]
            if ones == 63:
                x, y = split(pa)
                ac[m, 0], ac[m, mi] = _pow2_code(fmt, x), _pow2_code(fmt, x, neg=True)
                ac[m, o + 1:o + 64] = _pow2_code(fmt, -y)
                as_[m, :] = SCALE_ONE + y  # the small elements are 1 after the scale
            else:
                ac[m, 0], ac[m, mi] = fmt.one, _pow2_code(fmt, 0, neg=True)
                as_[m, 0], as_[m, mi // BLOCK] = SCALE_ONE + pa, SCALE_ONE + pa
                ac[m, o + 32:o + 64] = fmt.one
            asserted[m] = (torch.arange(N) % 16) <= half
    p = Probe(f"align_probe[{ones} ones] {fmt.name}", fmt, ac, as_, wc, ws, expect, "2^p + ones - 2^p", asserted=asserted, order_free=False)
    ad, wd = p.values()
    # exact in fp64: every term is a power of two within 2^31 of the smallest
    p.expect = torch.where(asserted, ad @ wd.t(), torch.zeros_like(expect))
    assert bool((p.expect[asserted] == ones).all()), "align_probe: the closed form is `ones`"
    return p


def align_p_of(M: int = ALIGN_SHAPE[0], N: int = ALIGN_SHAPE[1]):
    """-> (variant index [M][N], p [M][N]) of the alignment probe's outputs"""
    m, n = torch.arange(M).view(-1, 1), torch.arange(N).view(1, -1)
    return (m // 32).expand(M, N), (m % 32 + n % 16).expand(M, N)


def largest_exact_p(out: torch.Tensor, probe: Probe) -> dict:
    """per variant: the largest P such that every asserted output with p <= P came back exactly `ones`"""
    v, p = align_p_of()
    ok = (out.cpu().double() == probe.expect) | ~probe.asserted
    res = {}
    for i, name in enumerate(ALIGN_VARIANTS):
        sel = (v == i) & probe.asserted
        bad = p[sel & ~ok]
        res[name] = int(bad.min()) - 1 if bad.numel() else int(p[sel].max())
    return res


# What the alignment probe measured on an MI355X (profiles/mx_parity_measured.txt) - a statement about the hardware, asserted by the GPU test so
# that a change is loud: the largest p at which 2^p + ones - 2^p still comes back as `ones`, per variant, [63 ones, 32 ones].
ALIGN_MEASURED = {
    "mxfp8": {"same_step": (13, 27), "earlier_step": (23, 27), "earlier_tile": (23, 27)},
    "mxfp6": {"same_step": (10, 27), "earlier_step": (10, 27), "earlier_tile": (10, 27)},  # 10: every p the e2m3 codes of one block reach
}

# The accumulation bar of the Gaussian cases: |out - ref| <= 0.5 bf16_ulp(ref) + C_ACC sum |a w|. Measured worst (|err| - 0.5 ulp) / sum |a w|
# against fp64 on the seeded cases below (profiles/mx_parity_measured.txt), doubled and rounded up to a power of two, never above 2^-12.
C_ACC_MEASURED = 5.524e-05  # = 2^-14.14: MXFP8 at (300, 512, 384); (64, 512, 16384): 2^-15.76; MXFP6: no output off bf16_round(fp64) on either shape
C_ACC_CAP = 2.0 ** -12


def c_acc() -> float:
    assert C_ACC_MEASURED is not None
    return min(2.0 ** math.ceil(math.log2(2.0 * C_ACC_MEASURED)), C_ACC_CAP)


GAUSS_SHAPES = [ODD_KTILES, DEEP]


@functools.lru_cache(maxsize=4)
def gaussian_bf16(shape):
    """a [M][K] randn with outlier channels (every 97th from 3 scaled by 30), w [N][K] randn / sqrt(K) with outlier channels too, as bf16"""
    M, N, K = shape
    g = _rng(M, N, K, 6)
    a = torch.randn(M, K, generator=g)
    a[:, 3::97] *= 30.0
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    w[:, 5::113] *= 8.0
    return a.to(bf16), w.to(bf16)


def quantise(x: torch.Tensor, fmt: Fmt):
    """the reference quantiser -> (codes [R][K] uint8, scales)"""
    if fmt is FP8:
        q, s = mxfp8_ref.quant_mxfp8_ref(x)
        return q.view(torch.uint8), s
    return mxfp6_ref.quant_mxfp6_codes(x)


def gaussian(fmt: Fmt, shape) -> Probe:
    a, w = gaussian_bf16(shape)
    ac, as_ = quantise(a, fmt)
    wc, ws = quantise(w, fmt)
    p = Probe(f"gaussian {fmt.name} {shape}", fmt, ac, as_, wc, ws, torch.empty(0), "fp64", rounded=True, order_free=False)
    ad, wd = p.values()
    p.expect = ad @ wd.t()
    return p


def acc_excess(out: torch.Tensor, probe: Probe) -> float:
    """worst (|err| - 0.5 ulp) / sum |a w| of an output against the probe's fp64 result"""
    ad, wd = probe.values()
    ref, absum = gemm_ref64(ad, wd)
    err = (out.cpu().double() - ref).abs() - 0.5 * bf16_ulp(ref)
    return float((err / absum.clamp(min=1e-300)).max())


# ---- family F --------------------------------------------------------------------------------------------------------------------
def _bf16_from_bits(b: int) -> float:
    return float(torch.tensor([b], dtype=torch.int32).to(torch.int16).view(bf16).float())


QUANT_ANCHORS = {  # the planted block maxima
    "1.0": _bf16_from_bits(0x3F80), "1.9921875": _bf16_from_bits(0x3FFF), "2^-126": _bf16_from_bits(0x0080),
    "subnormal": _bf16_from_bits(0x0013), "largest": _bf16_from_bits(0x7F7F),
}


@functools.lru_cache(maxsize=None)
def quant_sweep(anchor: str) -> torch.Tensor:
    """x [R][32] bf16: one block per finite bf16 value v with |v| <= the anchor; the anchor sits at position 7 i mod 32 of block i, v at another
    position that moves with i, zeros elsewhere - the anchor stays the block's amax, v meets every lane of the quad."""
    from tests.norm_rope_ref import all_bf16
    amax = QUANT_ANCHORS[anchor]
    v = all_bf16()
    v = v[torch.isfinite(v.float()) & (v.float().abs() <= amax)]
    R = v.numel()
    i = torch.arange(R)
    x = torch.zeros(R, BLOCK, dtype=bf16)
    pa = (7 * i) % BLOCK
    x[i, pa] = amax
    x[i, (pa + 1 + i % 31) % BLOCK] = v
    return x


def nonfinite_input(K: int = 256, rows: int = 48) -> torch.Tensor:
    """bf16 [rows][K] randn with planted non-finite values: row r < 32 holds one at k = 37 r mod K - NaN, +inf, -inf in turn, so every lane
    of a quad and every element of a lane meets one -, rows 32 .. 39 two in different blocks, rows 40 .. are finite."""
    g = _rng(K, rows, 8)
    x = torch.randn(rows, K, generator=g)
    bad = (math.nan, math.inf, -math.inf)
    for r in range(32):
        x[r, (37 * r) % K] = bad[r % 3]
    for r in range(32, 40):
        x[r, r] = bad[r % 3]
        x[r, K - 1 - r] = bad[(r + 1) % 3]
    return x.to(bf16)


# =================================================================================================================================
# exactness of a probe (what the CPU test asserts)
# =================================================================================================================================
def _lsb(x: torch.Tensor) -> torch.Tensor:
    """the largest power of two that divides each fp64 value (inf for 0)"""
    m, e = torch.frexp(x.abs())
    mi = (m * 2.0 ** 53).long()
    low = (mi & -mi).double()
    return torch.where(x == 0, torch.full_like(x, math.inf), low * torch.pow(2.0, (e - 53).double()))


def order_free_margin(p: Probe) -> float:
    """max over outputs of sum |terms| / unit, unit = a lower bound of the smallest power of two dividing every term of that output: the
    minimum over the blocks in which both operands are non-zero of lsb(a's block) lsb(w's block). Below 2^24 every partial sum, in any order
    and grouping, is an integer multiple of `unit` below 2^24 unit: exact in fp32."""
    ad, wd = p.values()
    ad, wd = torch.nan_to_num(ad, nan=0.0), torch.nan_to_num(wd, nan=0.0)
    M, K = ad.shape
    N = wd.shape[0]
    nb = K // BLOCK
    la = _lsb(ad).reshape(M, nb, BLOCK).amin(-1)  # inf where the block is all zero
    lw = _lsb(wd).reshape(N, nb, BLOCK).amin(-1)
    absum = ad.abs() @ wd.abs().t()
    unit = torch.full((M, N), math.inf, dtype=torch.float64)
    for b0 in range(0, nb, 16):
        u = la[:, None, b0:b0 + 16] * lw[None, :, b0:b0 + 16]
        unit = torch.minimum(unit, torch.nan_to_num(u, nan=math.inf).amin(-1))
    live = absum > 0
    return float((absum[live] / unit[live]).max()) if bool(live.any()) else 0.0


def expect_is_exact(p: Probe) -> bool:
    """`expect` is the fp64 product of the operands (exact there: the sums are far below 2^53 units), and - unless the probe says `rounded` -
    every asserted value is a bf16 value"""
    ad, wd = p.values()
    ref = ad @ wd.t()
    held = p.asserted if p.asserted is not None else torch.ones_like(ref, dtype=torch.bool)
    same = (ref == p.expect) | (torch.isnan(ref) & torch.isnan(p.expect))
    if not bool(same[held].all()):
        return False
    if p.rounded:
        return True
    e = p.expect[held]
    e = e[~torch.isnan(e)]
    return bool((bf16_round(e).double() == e).all())


# =================================================================================================================================
# the device model: indices only
# =================================================================================================================================
DEFECTS = ("scale_pair_swapped", "half_bytes_swapped", "fp6_bits_reversed", "fp6_second_chunk_16", "stale_stage", "stale_scale", "scale_shift_omitted",
           "xcd_remap", "tail_group")
DEFECT_FMT = {"half_bytes_swapped": "mxfp8", "fp6_bits_reversed": "mxfp6", "fp6_second_chunk_16": "mxfp6"}


def _rev6(c: np.ndarray) -> np.ndarray:
    r = np.zeros_like(c)
    for i in range(6):
        r |= ((c >> i) & 1) << (5 - i)
    return r


def model_seen(codes: torch.Tensor, scales: torch.Tensor, fmt: Fmt, defect: str = "") -> torch.Tensor:
    """What the matrix core multiplies, row by row, for an operand as the kernels stage and read it: fp64 [R][K] in the order of the MFMA's k
    index (K tile t, 64-deep step s, k' = 0 .. 63), value = table[code the lane maps put at k'] * 2^(the scale byte op_sel names for k' / 32).

    Bookkeeping modelled (gemm_mxfp8_nt_kernel / gemm_mxfp6_nt_kernel): K tile t sits in stage t & 1 with its scale dword (bytes = blocks
    4 t .. 4 t + 3); lane half h keeps dword >> 8 h; step s names byte 2 s, so MFMA block b of the step takes the byte of the lanes with h = b.
    MXFP8: lane half h holds tile bytes [64 s + 16 h, + 16) as operand bytes 0 .. 15 = k' 16 h .., and [64 s + 32 + 16 h, + 16) as bytes 16 .. 31 =
    k' 32 + 16 h ... MXFP6: lane half h holds the 24-byte block 2 s + h, assembled from the chunks at byte 24 b and 24 b + 8 of the packed row
    (registers 0 .. 3 from the first, 4 .. 5 from the upper half of the second); element i = bits [6 i, 6 i + 6) is k' = 32 h + i."""
    c = codes.numpy().astype(np.int64)
    s = scales.numpy().astype(np.int64)
    R, K = c.shape
    nk = K // BK
    tab = fmt.values().numpy()
    e8 = e8m0_values().numpy()
    seen = np.zeros((R, K), dtype=np.float64)
    if fmt is FP6:  # the packed rows, and what lies behind a row's last byte
        ext = np.concatenate([fmt.pack(codes).numpy().astype(np.int64), np.full((R, 64), fmt.pad, dtype=np.int64)], axis=1)
    for t in range(nk):
        td = t - 2 if (defect == "stale_stage" and t >= 2) else t      # the stage holds what was put there two tiles ago
        ts = t - 2 if (defect == "stale_scale" and t >= 2) else t
        dword = s[:, 4 * ts:4 * ts + 4]                                  # [R][4]
        for st in range(2):
            kk = np.zeros((R, 64), dtype=np.int64)                       # codes at k'
            sc = np.zeros((R, 2), dtype=np.int64)                        # scale byte of MFMA block 0 / 1
            for h in range(2):
                shift = 0 if defect == "scale_shift_omitted" else h
                byte = 2 * st + shift
                if defect == "scale_pair_swapped":
                    byte = 2 * st + (1 - h)
                sc[:, h] = dword[:, byte]
                if fmt is FP8:
                    tile = c[:, BK * td:BK * td + BK]
                    lo = tile[:, 64 * st + 16 * h:64 * st + 16 * h + 16]
                    h2 = 1 - h if defect == "half_bytes_swapped" else h
                    hi = tile[:, 64 * st + 32 + 16 * h2:64 * st + 32 + 16 * h2 + 16]
                    kk[:, 16 * h:16 * h + 16] = lo
                    kk[:, 32 + 16 * h:32 + 16 * h + 16] = hi
                else:
                    blk = 2 * st + h
                    row0 = 96 * td + 24 * blk
                    second = 16 if defect == "fp6_second_chunk_16" else 8
                    b24 = np.concatenate([ext[:, row0:row0 + 16], ext[:, row0 + second + 8:row0 + second + 16]], axis=1)  # [R][24]
                    v = b24.reshape(R, 8, 3)
                    v = v[..., 0] | (v[..., 1] << 8) | (v[..., 2] << 16)
                    el = np.stack([(v >> (6 * i)) & 0x3F for i in range(4)], axis=-1).reshape(R, 32)
                    if defect == "fp6_bits_reversed":
                        el = _rev6(el)[:, ::-1]
                    kk[:, 32 * h:32 * h + 32] = el
            val = tab[kk] * np.repeat(e8[sc], 32, axis=1)
            seen[:, BK * t + 64 * st:BK * t + 64 * st + 64] = val
    return torch.from_numpy(seen)


def model_tiles(M: int, N: int, defect: str = ""):
    """blockIdx -> (tile_m, tile_n), the kernels' order: a contiguous run of the global order per XCD (8), token tiles in super-rows of 4.
    defect "xcd_remap": the remainder of tiles / 8 forgotten in the run starts; "tail_group": gm = 4 also in a shorter last super-row, the
    token tile clamped to the last one."""
    tiles_m, tiles_n = -(-M // BM), N // BN
    nblk = tiles_m * tiles_n
    out = []
    for bid in range(nblk):
        q, r = nblk >> 3, nblk & 7
        xcd, slot = bid & 7, bid >> 3
        if defect == "xcd_remap":
            b = xcd * q + slot
        else:
            b = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot
        per_group = 4 * tiles_n
        grp = b // per_group
        within = b - grp * per_group
        gm = 4 if defect == "tail_group" else min(4, tiles_m - grp * 4)
        tile_n = within // gm
        tile_m = min(grp * 4 + (within - tile_n * gm), tiles_m - 1)
        out.append((tile_m, min(tile_n, tiles_n - 1)))
    return out


def model_output(p: Probe, defect: str = "", side: str = "a") -> torch.Tensor:
    """the fp64 output of the modelled kernel on a probe: seen(a) @ seen(w)^T on the tiles some workgroup owns, NaN (the guard's fill) elsewhere.
    An operand defect sits in the reads of one operand (`side`): the same permutation of k on both would pair the same elements again."""
    M, N, K = p.shape
    d = defect if DEFECT_FMT.get(defect, p.fmt.name) == p.fmt.name else ""
    a = model_seen(p.ac, p.as_, p.fmt, d if side == "a" else "")
    w = model_seen(p.wc, p.ws, p.fmt, d if side == "w" else "")
    full = a @ w.t()
    out = torch.full((M, N), math.nan, dtype=torch.float64)
    for tm, tn in model_tiles(M, N, defect):
        out[BM * tm:BM * tm + BM, BN * tn:BN * tn + BN] = full[BM * tm:BM * tm + BM, BN * tn:BN * tn + BN]
    return out


def same_values(a: torch.Tensor, b: torch.Tensor, held=None) -> bool:
    eq = (a == b) | (torch.isnan(a) & torch.isnan(b))
    return bool(eq.all() if held is None else eq[held].all())
