"""fp64 references of the block GEMM's epilogues, one stage at a time (TEST INFRASTRUCTURE - a plain helper module).

Written from the reference model's definitions (nn.Linear(bias=False) in bf16; GPT2FeedForward: gelu(layer1(x)), attention.py:86, 94-99; the
block's x + gate * block(...), blocks.py:455-471) and the ABI header (include/gen3c_hip.h, G3_EPI_NONE .. G3_EPI_BIAS_RESIDUAL), in float64 on
the very bf16 values a kernel reads - never from the kernels. tests/test_gemm_ref_cpu.py pins this module against fp64 torch and
oracle/dit_oracle.py; tests/test_gemm_epilogue_kernels_gpu.py holds the five epilogue copies against it.

Two stages, each one rounding to bf16:
  1  the Linear: a @ w^T (+ bias[m % rows]) (+ R), E = 2^-24 (|a| @ |w|^T + |s + bias| + |(s + bias) + R|): one fp32 rounding per product sum
     term and one per fp32 add of the epilogue; bound 0.5 bf16_ulp(ref) + C_GEMM E.
  2  what acts on the Linear's ROUNDED output y (the bitwise EPI_NONE output of the same kernel on the same operands):
     GELU 0.5 y erfc(-y / sqrt 2), E = 2^-24 |y|, bound 0.5 ulp + C_GELU E; gated residual R + g y: g y is exact in fp32, so there is exactly
     one right answer, bf16(fp32(R + g y)) - bitwise - which also lies within 0.5 ulp + 2^-24 |ref| of the fp64 value.

The fp32 restatements say what a correct kernel can deliver (the evidence behind C and the yardstick of the share bar, tests/norm_rope_ref.py):
gelu_fast32 is the erf form the kernels evaluate (Abramowitz-Stegun 7.1.26 with the 0.5 folded into the coefficients, exp through exp2),
operation by operation in fp32 with correctly rounded 1/x and exp2; linear_fp32 accumulates in fp32 over K in 16-wide chunks (an 8-wide one
last where K % 16 == 8: the tail the register-staged path zero-fills). Each takes ONE defect by name (the mutants the CPU test must see caught).

C = 4 x the restatement's worst (err - 0.5 ulp) / E rounded up to a power of two; tests/test_gemm_ref_cpu.py re-derives and asserts both.
"""
from __future__ import annotations

import functools
import math

import torch

from tests.norm_rope_ref import HALF_ULP_SHARE, SHARE_FLOOR, U24, all_bf16, check, half_ulp_share, measure, pow2_ceil  # noqa: F401  (re-exported)
from tests.tokenizer_kernel_ref import bf16_round, bf16_ulp  # noqa: F401

bf16 = torch.bfloat16
EPI_NONE, EPI_GELU, EPI_GATED_RESIDUAL, EPI_BIAS, EPI_BIAS_RESIDUAL = 0, 1, 2, 3, 4  # include/gen3c_hip.h

C_GEMM, C_GELU = 16.0, 1.0  # asserted against the restatements' worst by the CPU test

MUTANTS_GELU = ["gelu_tanh", "gelu_no_round", "gelu_no_log2e", "gelu_coef_sign"]
MUTANTS_GATE = ["gate_no_round", "gate_row_div"]
MUTANTS_LINEAR = ["bias_late", "k_tail_dropped", "bf16_partials"]


def _rows(M: int, rows: int, device=None, div: bool = False) -> torch.Tensor:
    m = torch.arange(M, device=device)
    return (m // rows) % rows if div else m % rows


# =================================================================================================================================
# stage 1: the Linear (+ bias) (+ residual)
# =================================================================================================================================
def linear_ref(a: torch.Tensor, w: torch.Tensor, bias=None, residual=None):
    """a [M][K], w [N][K], bias [rows][N] (row m % rows), residual [M][N], all bf16, on any one device -> (ref, E) in fp64 there"""
    ad, wd = a.double(), w.double()
    ref = ad @ wd.t()
    E = U24 * (ad.abs() @ wd.abs().t())
    if bias is not None:
        ref = ref + bias.double()[_rows(a.shape[0], bias.shape[0], a.device)]
        E = E + U24 * ref.abs()
    if residual is not None:
        assert bias is not None, "G3_EPI_BIAS_RESIDUAL is (a @ w^T + bias) + R"
        ref = ref + residual.double()
        E = E + U24 * ref.abs()
    return ref, E


def linear_acc32(a: torch.Tensor, w: torch.Tensor, mutant: str = "") -> torch.Tensor:
    """the fp32 accumulator of a @ w^T: K in 16-wide chunks one after the other (a chunk's 16 products are added exactly, the running sum is
    rounded to fp32 once per chunk), the last chunk 8 wide where K % 16 == 8. mutant: "k_tail_dropped" (the last 8 k are not added where
    K % 64 != 0), "bf16_partials" (the running sum is rounded to bf16 after every chunk)."""
    K = a.shape[1]
    if mutant == "k_tail_dropped" and K % 64:
        K -= 8
    ad, wd = a.double(), w.double()
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32, device=a.device)
    for k0 in range(0, K, 16):
        k1 = min(k0 + 16, K)
        acc = (acc.double() + ad[:, k0:k1] @ wd[:, k0:k1].t()).float()
        if mutant == "bf16_partials":
            acc = acc.to(bf16).float()
    return acc


def linear_fp32(a, w, bias=None, residual=None, mutant: str = "", acc=None) -> torch.Tensor:
    """stage 1 as a kernel delivers it: bf16((acc + bias) + R) with fp32 adds (acc: linear_acc32(a, w, mutant) where the caller has it already).
    mutant: those of linear_acc32, "bias_late" (the bias is added to the rounded product)."""
    if acc is None:
        acc = linear_acc32(a, w, mutant)
    if bias is None:
        return acc.to(bf16)
    b = bias.float()[_rows(a.shape[0], bias.shape[0], a.device)]
    v = acc.to(bf16).float() + b if mutant == "bias_late" else acc + b
    if residual is not None:
        v = v + residual.float()
    return v.to(bf16)


# =================================================================================================================================
# stage 2: GELU and the gated residual on the Linear's rounded output y
# =================================================================================================================================
def gelu64(y: torch.Tensor) -> torch.Tensor:
    yd = y.double()
    return 0.5 * yd * torch.special.erfc(-yd * math.sqrt(0.5))


def gelu_ref(y: torch.Tensor):
    """-> (0.5 y erfc(-y / sqrt 2), E = 2^-24 |y|): the result is the difference max(y, 0) - 0.5 |y| q of two terms of magnitude <= |y|"""
    return gelu64(y), U24 * y.double().abs()


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def _fma32(x: torch.Tensor, y: torch.Tensor, c: float) -> torch.Tensor:
    """fp32 fma(x, y, c): the product of two fp32 values is exact in fp64, so this is the sum rounded to fp64 and then to fp32"""
    return (x.double() * y.double() + c).float()


def gelu_fast32(x: torch.Tensor, mutant: str = "") -> torch.Tensor:
    """erf-form GELU in fp32, operation by operation (x: fp32 values, the Linear's rounded output unless a mutant says otherwise) -> bf16:
        t = 1 / fma(p / sqrt 2, |x|, 1);  poly = Horner in t over 0.5 a5 .. 0.5 a1 (fma);  ex = exp2(x x (-0.5 log2 e))
        result = max(x, 0) - ((poly t) ex) |x|
    with 1 / u and exp2 correctly rounded (evaluated in fp64, rounded once: the same on every host, tests/norm_rope_ref.py _rsqrt32).
    Where x x overflows (|x| > 1.8e19) the exponent is -inf and ex = 0.
    mutant: "gelu_tanh" (the tanh form), "gelu_no_log2e" (ex = exp2(-x x / 2)), "gelu_coef_sign" (a4's sign lost with its 0.5)."""
    x = x.float()
    if mutant == "gelu_tanh":
        xd = x.double()
        return (0.5 * xd * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (xd + 0.044715 * xd ** 3)))).float().to(bf16)
    ax = x.abs()
    p = _f32(_f32(0.3275911) * _f32(math.sqrt(0.5)))
    a = [0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429]
    if mutant == "gelu_coef_sign":
        a[3] = -a[3]
    h = [_f32(0.5 * _f32(c)) for c in a]
    t = (1.0 / _fma32(ax, torch.full_like(ax, p), 1.0).double()).float()
    poly = _fma32(torch.full_like(t, h[4]), t, h[3])
    for c in (h[2], h[1], h[0]):
        poly = _fma32(poly, t, c)
    k = _f32(-0.5) if mutant == "gelu_no_log2e" else _f32(-0.5 * _f32(1.44269504088896340736))
    ex = torch.exp2(((x * x) * k).double()).float()
    return (x.clamp(min=0.0) - ((poly * t) * ex) * ax).to(bf16)


def gelu_fp32(y: torch.Tensor, acc=None, mutant: str = "") -> torch.Tensor:
    """the GELU epilogue on y; mutant "gelu_no_round" evaluates it on the unrounded accumulator `acc` instead"""
    if mutant == "gelu_no_round":
        return gelu_fast32(acc)
    return gelu_fast32(y, mutant)


@functools.lru_cache(maxsize=None)
def gelu_near_tie():
    """bool [65536] by bit pattern: finite values whose gelu64 lies within 2^-10 bf16 ulp of a rounding tie. An approximate rcp / exp2 may round
    those either way; every other finite value has one right answer, bf16_round(gelu64(y))."""
    y = all_bf16()
    fin = torch.isfinite(y.float())
    s = gelu64(torch.where(fin, y, torch.zeros_like(y)))
    q = s / bf16_ulp(s)
    near = ((q - torch.floor(q)) - 0.5).abs() < 2.0 ** -10
    return near & fin


def bits_of(t: torch.Tensor) -> torch.Tensor:
    return (t.view(torch.int16).to(torch.int32) & 0xFFFF).long()


def gated_ref(y: torch.Tensor, gate: torch.Tensor, residual: torch.Tensor):
    """y, residual [M][N], gate [rows][N] (row m % rows) -> (R + g y, E = 2^-24 |ref|) in fp64"""
    ref = residual.double() + gate.double()[_rows(y.shape[0], gate.shape[0], y.device)] * y.double()
    return ref, U24 * ref.abs()


def gated_fp32(y, gate, residual, acc=None, mutant: str = "") -> torch.Tensor:
    """bf16(fp32(R + g y)): g y has at most 16 significant bits, exact in fp32, so the sum is rounded to fp32 once and to bf16 once.
    mutant: "gate_no_round" (g times the unrounded accumulator `acc`), "gate_row_div" (gate row m / rows)."""
    g = gate.float()[_rows(y.shape[0], gate.shape[0], y.device, div=mutant == "gate_row_div")]
    v = acc if mutant == "gate_no_round" else y.float()
    return (residual.float() + g * v).to(bf16)


# =================================================================================================================================
# input families (bf16, seeded, built on the CPU) and the shapes of the GPU suite
# =================================================================================================================================
FAMILIES = ("randn", "same_sign", "scale4_rows")
SCALE4_EVERY = 7  # family "scale4_rows": every 7th row of a is scaled by 4
GATE_ROWS_MAX = 4
# (M, N, K): the smallest shape of each epilogue copy (K = 64: classic / ping-pong; K = 128: one wave per SIMD) and the ragged ones
SMALL, K128 = (256, 256, 64), (256, 256, 128)
RAGGED = [(300, 260, 136), (257, 264, 192), (56, 1024, 4096)]
DEFERRED_NK = (4096, 2432)  # N, K of the deferred-epilogue shape; its M depends on the device's CU count


@functools.lru_cache(maxsize=8)
def inputs(M: int, N: int, K: int, family: str):
    """-> a [M][K], w [N][K], gate [4][N] (the first `rows` rows are a call's gate / bias), residual [M][N].
    "randn": randn activations, randn / sqrt(K) weights. "same_sign": |randn| and |randn| / sqrt(K) - the reference is as large as the sum of
    the magnitudes, so a biased accumulation shows. "scale4_rows": every 7th row of a scaled by 4, so that its a @ w^T has standard deviation 4
    and fills GELU's tails to |y| = 18. (Every row scaled by 4 puts 16 % of a case's pre-activations below -4, where Phi(y) < 2^-15 and the
    allowance C_GELU E exceeds half an ulp: past the 5 % such elements a case may hold. One row in 7 leaves 2.3 %.)"""
    g = torch.Generator().manual_seed(4000 + 31 * M + 7 * N + K + 1000003 * FAMILIES.index(family))
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    if family == "same_sign":
        a, w = a.abs(), w.abs()
    elif family == "scale4_rows":
        a[::SCALE4_EVERY] *= 4.0
    gate = torch.randn(GATE_ROWS_MAX, N, generator=g)
    res = torch.randn(M, N, generator=g)
    return a.to(bf16), w.to(bf16), gate.to(bf16), res.to(bf16)


def tile_rows(M: int, limit: int = 256) -> torch.Tensor:
    """the rows a case is checked on: every row where M <= 1024; else at most `limit`: the first and last row of the first, a middle and the
    last 256-row tile, and an even spread over the rest"""
    if M <= 1024:
        return torch.arange(M)
    tiles = -(-M // 256)
    must = [r for t in (0, tiles // 2, tiles - 1) for r in (256 * t, min(256 * t + 255, M - 1))]
    spread = torch.linspace(0, M - 1, limit - len(must)).long().tolist()
    return torch.tensor(sorted(set(must + spread)))


# ---- the sweep: every finite bf16 value through the epilogue as a one-term product -----------------------------------------------
@functools.lru_cache(maxsize=None)
def finite_bf16():
    """the 65 280 finite bf16 values in bit-pattern order"""
    v = all_bf16()
    return v[torch.isfinite(v.float())]


def sweep_inputs(M: int, N: int, K: int):
    """a[m][k] = the finite bf16 values in bit-pattern order, wrapped; w[n][k] = 1 where k == n % K, else 0: output (m, n) is a[m][n % K] times
    1 plus zeros. 256 x 256 x 256 holds every value once (and the first 256 again)."""
    v = finite_bf16()
    a = v[torch.arange(M * K) % v.numel()].reshape(M, K)
    w = torch.zeros(N, K, dtype=bf16)
    w[torch.arange(N), torch.arange(N) % K] = 1.0
    return a, w


def mx_sweep_inputs():
    """Every bf16 value x = +-1.m x 2^e with e >= -120 (63 488 values) as MXFP8 operands without a quantiser: block b of a row holds
    hi = (8 + m[6:4]) 16 and lo = m[3:0] as e4m3 elements 0 and 1 (both with x's sign) under the E8M0 scale 2^(e - 7) - hi + lo = 128 + m -,
    eight values per row at K = 256; w[n] is 1.0 at those two positions of block n % 8, scale 2^0.
    -> x [7936][8] bf16, aq [7936][256] e4m3fn, as [7936][8] u8, wq [256][256] e4m3fn, ws [256][8] u8"""
    v = all_bf16()
    bits = torch.arange(65536)
    ex, man = (bits >> 7) & 0xFF, bits & 0x7F
    ok = (ex >= 127 - 120) & (ex <= 254)
    x, ex, man, neg = v[ok], ex[ok], man[ok], (bits[ok] >> 15) == 1
    assert x.numel() == 63488
    sign = torch.where(neg, -1.0, 1.0)
    rows = x.numel() // 8
    aq = torch.zeros(rows, 8, 32)
    aq[:, :, 0] = (sign * (8 + (man >> 4)) * 16).reshape(rows, 8)
    aq[:, :, 1] = (sign * (man & 15)).reshape(rows, 8)
    as_ = (ex - 7).to(torch.uint8).reshape(rows, 8)  # byte = (e - 7) + 127 with e = ex - 127
    wq = torch.zeros(256, 8, 32)
    n = torch.arange(256)
    wq[n, n % 8, 0] = 1.0
    wq[n, n % 8, 1] = 1.0
    f8 = torch.float8_e4m3fn
    return x.reshape(rows, 8), aq.reshape(rows, 256).to(f8), as_, wq.reshape(256, 256).to(f8), torch.full((256, 8), 127, dtype=torch.uint8)


SWEEP_TAIL, SWEEP_ZERO = -4.0, -14.0


def check_sweep(what: str, y: torch.Tensor, out: torch.Tensor):
    """The bars of a GELU output `out` on swept pre-activations y (finite bf16 values, CPU), against gelu64(y):
      - |out - ref| <= 0.5 bf16_ulp(ref) + C_GELU 2^-24 |y| on EVERY element, and the share of elements != bf16_round(ref) at most
        max(10 x the restatement's share, 1e-3) (kr.check's first two bars);
      - C E > 0.5 ulp on at most 5 % of the elements with y >= -4. Below -4, Phi(y) < 2^-15 and the allowance is the larger term on every
        element - a quarter of the bit patterns -, so the 5 % condition cannot hold for the sweep as a whole; what holds the far tail instead:
      - y <= -14: exactly 0 (|gelu64| < 2^-134, half the smallest bf16 subnormal);
      - |y| <= 2 and not within 2^-10 ulp of a rounding tie (gelu_near_tie): exactly bf16_round(ref).
    Prints the figures, then asserts; returns (worst, share, share_r, frac)."""
    y, out = y.reshape(-1), out.reshape(-1)
    ref, E = gelu_ref(y)
    restated = gelu_fast32(y)
    worst, share = measure(out, ref, E)
    _, share_r = measure(restated, ref, E)
    yf = y.float()
    body = yf >= SWEEP_TAIL
    frac = half_ulp_share(ref[body], E[body], C_GELU)
    must = (yf.abs() <= 2.0) & ~gelu_near_tie()[bits_of(y)]
    wrong = int((out[must] != bf16_round(ref)[must]).sum())
    far = yf <= SWEEP_ZERO
    nonzero = int((out[far].float() != 0).sum())
    print(f"[{what}] {y.numel()} values: worst (err - 0.5 ulp) / E = {worst:.3f} (C = {C_GELU:g}), share != bf16(ref) {share:.2e} (restatement {share_r:.2e}), "
          f"C E > 0.5 ulp on {frac:.2%} of y >= -4; {int(must.sum())} values |y| <= 2 off the near-tie list: {wrong} != bf16(ref); {int(far.sum())} values y <= -14: {nonzero} != 0")
    assert worst <= C_GELU, f"{what}: (err - 0.5 ulp) / E = {worst} > C = {C_GELU}"
    assert share <= max(10 * share_r, SHARE_FLOOR), f"{what}: share {share} > max(10 x {share_r}, {SHARE_FLOOR})"
    assert frac <= HALF_ULP_SHARE, f"{what}: the allowance exceeds half an ulp on {frac:.2%} of the elements with y >= -4"
    assert wrong == 0, f"{what}: {wrong} values with |y| <= 2 are not bf16_round(gelu64(y))"
    assert nonzero == 0, f"{what}: {nonzero} values with y <= -14 are not 0"
    return worst, share, share_r, frac


def format_row(what: str, kernel: str, worst: float, share: float, share_r: float, frac: float) -> str:
    """one line of profiles/gemm_epilogue_parity_measured.txt"""
    return f"{what:<58} {kernel:<46} worst {worst:>8.3f}  share {share:.2e}  restatement {share_r:.2e}  C E > 0.5 ulp {frac:.2%}"


# =================================================================================================================================
# kernel selectors shared by the kernel-level GPU files (what g3_gemm_plan_bf16 must name, {e} = the epilogue's numeral)
# =================================================================================================================================
CLASSIC, PP2, PP4 = "gemm_bf16_nt_kernel<{e}, true, false, false>", "gemm_bf16_nt_pp_kernel<{e}, 2, false>", "gemm_bf16_nt_pp_kernel<{e}, 4, false>"
W4, W4P = "gemm_bf16_nt_w4_kernel<{e}, false>", "gemm_bf16_nt_w4_kernel<{e}, true>"
W4E, W4E_TF = "gemm_bf16_nt_w4e_kernel<{e}, false>", "gemm_bf16_nt_w4e_kernel<{e}, true>"
REG = "gemm_bf16_nt_kernel<{e}, false, false, false>"  # register staging: what K % 64 != 0 runs
TWO_TILES = "two tiles per workgroup"  # M of the persistent shapes: from the device's CU count (two_tiles_m)
# the options the GEMM / convolution choice reads, and their defaults (csrc/api.hip)
OPTION_DEFAULTS = {"gemm_pingpong": 3, "gemm_regstage": 0, "gemm_unpinned": 1, "gemm_persistent": 0, "gemm_tokens_first": 2, "gemm_wide_store": 1,
                   "gemm_deferred": 1, "conv_w4": 1}


def two_tiles_m(cus: int) -> int:
    """with N = 4096 (16 tiles): the smallest M that gives each workgroup of the persistent grid (one per CU, a multiple of 8) two tiles"""
    return 256 * -(-2 * (cus // 8 * 8) // 16)
