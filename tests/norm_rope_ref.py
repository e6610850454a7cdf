"""fp64 references of the kernels of gen3c_amd/csrc/norm_rope.hip, one operation at a time (TEST INFRASTRUCTURE - a plain helper module).

Written from the reference model's definitions (nn.LayerNorm without affine + AdaLN modulate, blocks.py:339-341, 408; te.pytorch.RMSNorm and
apply_rotary_pos_emb(fused=True), attention.py:262-280; the SiLU -> Linear of the timestep MLP and the AdaLN-LoRA, blocks.py:60-80, 411-415),
in float64 on the very bf16 values a kernel reads - never from the kernels. tests/test_norm_rope_ref_cpu.py pins this module against
oracle/dit_oracle.py and fp64 torch; tests/test_norm_rope_kernels_gpu.py holds the HIP kernels against it.

Per operation: the reference, the per-element bound 0.5 bf16_ulp(ref) + C E (one correct rounding of the result plus C times the first-order
fp32 error E of the terms that make it), a restatement in fp32 that sums in the kernel's order (what a correct kernel can deliver: the
evidence behind C, and the yardstick of the share bar), and restatements with ONE defect each (the mutants the CPU test must see caught).

C = 4 x the restatement's worst (err - 0.5 ulp) / E over the suite's input families, rounded up to a power of two (the margin covers the
device's approximate rsqrt / rcp / exp); tests/test_norm_rope_ref_cpu.py re-derives every C below from the restatements and asserts it.
"""
from __future__ import annotations

import functools
import math

import torch

from tests.tokenizer_kernel_ref import bf16_round, bf16_ulp, ulp_error  # noqa: F401  (re-exported for the two test files)

bf16 = torch.bfloat16
EPS = 1e-6
U24 = 2.0 ** -24

C_LN, C_RMS, C_ROPE, C_GEMV = 4.0, 8.0, 8.0, 2.0  # asserted against the restatements' worst by the CPU test
SHARE_FLOOR = 1e-3      # the GroupNorm test's bar: share of elements != bf16(ref) <= max(10 x the restatement's share, this)
HALF_ULP_SHARE = 0.05   # C E may exceed 0.5 bf16_ulp(ref) on at most this share of a case: for the rest the bound is a half-ulp bound


def _d(t):
    return t.detach().cpu().double()


def _f(t):
    return t.detach().cpu().float()


# =================================================================================================================================
# the checker both test files use
# =================================================================================================================================
def measure(out: torch.Tensor, ref: torch.Tensor, E: torch.Tensor):
    """-> (worst (err - 0.5 ulp) / E, share of elements != bf16_round(ref)). Where E is 0 (a result that is exactly 0 because every term is)
    the quotient is -inf if the element is within half an ulp and +inf if not. A NaN anywhere makes the worst NaN."""
    o = _d(out)
    excess = (o - ref).abs() - 0.5 * bf16_ulp(ref)
    q = torch.where(E > 0, excess / E.clamp(min=1e-300), torch.where(excess <= 0, -math.inf, math.inf).to(torch.float64))
    q = torch.where(torch.isnan(o), torch.full_like(q, math.nan), q)
    worst = float("nan") if bool(torch.isnan(q).any()) else float(q.max())
    return worst, float((out.detach().cpu() != bf16_round(ref)).double().mean())


def half_ulp_share(ref: torch.Tensor, E: torch.Tensor, C: float) -> float:
    """share of elements on which the allowance C E is larger than the rounding term"""
    return float((C * E > 0.5 * bf16_ulp(ref)).double().mean())


def check(what: str, out: torch.Tensor, ref: torch.Tensor, E: torch.Tensor, C: float, restated: torch.Tensor):
    """The bars of a checked output: |out - ref| <= 0.5 bf16_ulp(ref) + C E on every element; share of elements != bf16_round(ref) at most
    max(10 x the share of `restated` (the fp32 restatement's output on the same input), 1e-3); and C E > 0.5 ulp on at most 5 % of the
    elements. Prints the figures, then asserts; returns them."""
    worst, share = measure(out, ref, E)
    _, share_r = measure(restated, ref, E)
    frac = half_ulp_share(ref, E, C)
    print(f"[{what}] worst (err - 0.5 ulp) / E = {worst:.3f} (C = {C:g}), share != bf16(ref) {share:.2e} (restatement {share_r:.2e}), C E > 0.5 ulp on {frac:.2%}")
    assert worst <= C, f"{what}: (err - 0.5 ulp) / E = {worst} > C = {C}"
    assert share <= max(10 * share_r, SHARE_FLOOR), f"{what}: share {share} > max(10 x {share_r}, {SHARE_FLOOR})"
    assert frac <= HALF_ULP_SHARE, f"{what}: the allowance exceeds half an ulp on {frac:.2%} of the elements"
    return worst, share, share_r, frac


def pow2_ceil(v: float) -> float:
    return 2.0 ** math.ceil(math.log2(v))


def _rsqrt32(v: torch.Tensor) -> torch.Tensor:
    """the correctly rounded fp32 rsqrt (evaluated in fp64, rounded once), so that the restatements and the constants derived from them are the
    same on every host: torch's vectorised fp32 sqrt / rsqrt differ between CPUs in the last bit (seen between two AVX-512 hosts)"""
    return (1.0 / torch.sqrt(v.double())).float()


def _butterfly(s: torch.Tensor, width: int) -> torch.Tensor:
    """s += shfl_xor(s, o) for o = width/2 .. 1 over the last axis (length `width`): every lane ends with the same fp32 sum, lane 0 is returned"""
    idx = torch.arange(width)
    o = width // 2
    while o:
        s = s + s[..., idx ^ o]
        o //= 2
    return s[..., 0]


# =================================================================================================================================
# LayerNorm + AdaLN modulate
# =================================================================================================================================
def ln_ref(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float = EPS):
    """x [rows][D], shift / scale [B][D] (modulation row = row % B) -> (ref, E) in fp64.
    E = 2^-24 (|xn| |1 + scale| + |shift| + |1 + scale| (|mean| + max_row |x - mean|) / sqrt(var + eps)): one fp32 rounding of each term of the
    result, and the fp32 rounding of the mean (2^-24 |mean|) and of x - mean carried into xn."""
    xd, rows = _d(x), x.shape[0]
    m = torch.arange(rows) % shift.shape[0]
    sh, sc1 = _d(shift)[m], 1.0 + _d(scale)[m]
    mean = xd.mean(dim=1, keepdim=True)
    cen = xd - mean
    std = torch.sqrt((cen * cen).mean(dim=1, keepdim=True) + eps)
    xn = cen / std
    E = U24 * (xn.abs() * sc1.abs() + sh.abs() + sc1.abs() * (mean.abs() + cen.abs().amax(dim=1, keepdim=True)) / std)
    return xn * sc1 + sh, E


def ln_fp32(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float = EPS, wave: bool = False, mutant: str = "") -> torch.Tensor:
    """LayerNorm + modulate in fp32, two passes, summed in the kernels' order: a thread owns the 8-element chunks tid + 256 c (one workgroup per
    row) or lane + 64 c (one wave per row, D = 4096), adds its elements one by one, then a 64-lane xor butterfly and (workgroup form) the four
    waves' sums in turn. mutant: "no_eps", "var_dm1" (variance over D - 1), "mod_div" (modulation row = row // (rows / B))."""
    xf = _f(x)
    rows, D = xf.shape
    B = shift.shape[0]
    lanes, nc = (64, 8) if wave else (256, 4)
    assert D % 8 == 0 and D <= lanes * nc * 8 and (not wave or D == 4096)
    v = torch.zeros(rows, nc * lanes * 8)
    v[:, :D] = xf
    v = v.view(rows, nc, lanes, 8)
    live = (torch.arange(nc * lanes * 8) < D).view(1, nc, lanes, 8)

    def reduce(t):  # t [rows][nc][lanes][8]: per thread in (c, e) order, butterfly, waves
        s = torch.zeros(rows, lanes)
        for c in range(nc):
            for e in range(8):
                s = s + t[:, c, :, e]
        w = _butterfly(s.view(rows, lanes // 64, 64), 64)
        tot = torch.zeros(rows)
        for i in range(w.shape[1]):
            tot = tot + w[:, i]
        return tot if not wave else w[:, 0]

    mean = (reduce(v) / float(D)).view(rows, 1, 1, 1)
    d = v - mean
    sq = reduce(torch.where(live, d * d, torch.zeros(())))
    var = sq / float(D - 1 if mutant == "var_dm1" else D)
    rstd = _rsqrt32(var + (0.0 if mutant == "no_eps" else torch.tensor(eps, dtype=torch.float32))).view(rows, 1)
    m = torch.arange(rows) // max(rows // B, 1) if mutant == "mod_div" else torch.arange(rows) % B
    m = m.clamp(max=B - 1)
    dd = d.reshape(rows, -1)[:, :D]
    return (dd * rstd * (1.0 + _f(scale)[m]) + _f(shift)[m]).to(bf16)


LN_ROWS = 17  # == 1 (mod 4): the last workgroup of the one-wave-per-row form holds one row
LN_CONST_ROW, LN_ONEHOT_ROW = 15, 16
# (D, mod_rows, one wave per row): every D leaves another pass of the 256 x 8 chunk loop partly filled (8: one chunk; 136, 520: 17 and 65 chunks;
# 2056: a 2049th element; 8184: one chunk short of full) or exactly full (512, 2048, 4096, 8192)
LN_CASES = [(8, 2, 0), (136, 3, 0), (512, 1, 0), (512, 3, 0), (520, 2, 0), (2048, 3, 0), (2056, 1, 0), (4096, 2, 0), (4096, 2, 1), (4096, 3, 1),
            (8184, 3, 0), (8192, 2, 0)]


def ln_scale_m1_cols(D: int) -> torch.Tensor:
    return torch.arange(D) % 5 == 3


@functools.lru_cache(maxsize=None)
def ln_inputs(D: int, B: int):
    """-> x [17][D], mod [B][3 D] bf16 (shift = mod[:, :D], scale = mod[:, D:2 D]: column views, ldmod = 3 D). Rows: 0-5 randn * 2 + 0.5; 6-10
    per-row magnitudes 2^-14, 2^-9, 2^-4, 2^1, 2^6 (variance from 4e-9, far below eps, to 4e3); 11-12 randn + 100; 13-14 4 randn + 1000;
    15 constant 0.75 (its fp32 sums are exact: the output is bf16(shift) exactly); 16 one-hot at the last element. scale = -1 on every fifth
    column (the output is shift exactly there); elsewhere modulation row 0's shift is minus row 0's modulated value, so row 0 cancels to
    within a rounding of the shift."""
    g = torch.Generator().manual_seed(1000 + 7 * D + B)
    x = torch.empty(LN_ROWS, D)
    x[0:6] = torch.randn(6, D, generator=g) * 2 + 0.5
    x[6:11] = torch.randn(5, D, generator=g) * (2.0 ** torch.tensor([-14.0, -9.0, -4.0, 1.0, 6.0])).view(5, 1)
    x[11:13] = torch.randn(2, D, generator=g) + 100
    x[13:15] = 4 * torch.randn(2, D, generator=g) + 1000
    x[LN_CONST_ROW] = 0.75
    x[LN_ONEHOT_ROW] = 0
    x[LN_ONEHOT_ROW, D - 1] = 8.0
    x = x.to(bf16)
    mod = torch.randn(B, 3 * D, generator=g)
    mod[:, D:2 * D] *= 0.5
    mod = mod.to(bf16)
    cols = ln_scale_m1_cols(D)
    mod[:, D:2 * D][:, cols] = -1.0
    x0 = _d(x[0])
    xn0 = (x0 - x0.mean()) / torch.sqrt(((x0 - x0.mean()) ** 2).mean() + EPS)
    cancel = bf16_round(-(xn0 * (1.0 + _d(mod[0, D:2 * D]))))
    mod[0, :D] = torch.where(cols, mod[0, :D], cancel)
    return x, mod


# =================================================================================================================================
# per-head RMSNorm and RoPE. Tensors are [rows][H][128]; weights [H][128] (one row per head: the q and k regions of the pair entry differ)
# =================================================================================================================================
def rms_ref(x: torch.Tensor, w: torch.Tensor, eps: float = EPS):
    """ref = x / sqrt(mean(x^2) + eps) * w, E = 2^-24 |ref|"""
    xd = _d(x)
    ref = xd / torch.sqrt((xd * xd).mean(dim=-1, keepdim=True) + eps) * _d(w)
    return ref, U24 * ref.abs()


def _rope_tables(cos: torch.Tensor, sin: torch.Tensor, rows: int, B: int, by_mod: bool = False):
    S = cos.shape[0]
    pos = torch.arange(rows) % S if by_mod else torch.arange(rows) // B  # rows are (s, b), b fastest
    return cos[pos].unsqueeze(1), sin[pos].unsqueeze(1)  # [rows][1][128]


def rope_ref(y: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, B: int):
    """y [rows][H][128] (the normalised bf16 values), cos / sin fp32 [S][128] -> (ref, E): first half y_a cos - y_b sin, second half
    y_b cos + y_a sin (t cos + rotate_half(t) sin, rotate_half(t) = cat(-t[64:], t[:64])); E = 2^-24 (|y cos| + |y' sin|)."""
    yd = _d(y)
    c, s = _rope_tables(_d(cos), _d(sin), y.shape[0], B)
    rot = torch.cat([-yd[..., 64:], yd[..., :64]], dim=-1)
    return yd * c + rot * s, U24 * ((yd * c).abs() + (rot * s).abs())


def rms_rope_fp32(x: torch.Tensor, w: torch.Tensor, cos, sin, B: int, eps: float = EPS, mutant: str = ""):
    """-> (no-RoPE output, RoPE output or None) as a kernel delivers them, in fp32 in the kernel's order: lane sl of a head's 8 adds
    a[e]^2 + b[e]^2 over its 8 + 8 dims (a = dims 8 sl .. 8 sl + 7, b = the same 64 further), then a 3-step xor butterfly;
    y = bf16(x * rsqrt(ss / 128 + eps) * w); the rotation on y. mutant: "rms_127", "no_round" (the RoPE stage reads the unrounded y),
    "rot_sign", "w_first_half" (second-half weights read from the first half), "pos_mod" (table row = row % S)."""
    xf, wf = _f(x), _f(w)
    rows, H, _ = xf.shape
    a, b = xf[..., :64].reshape(rows, H, 8, 8), xf[..., 64:].reshape(rows, H, 8, 8)
    ss = torch.zeros(rows, H, 8)
    for e in range(8):
        ss = ss + (a[..., e] * a[..., e] + b[..., e] * b[..., e])
    ss = _butterfly(ss, 8).view(rows, H, 1)
    rinv = _rsqrt32(ss * torch.tensor(1.0 / (127.0 if mutant == "rms_127" else 128.0), dtype=torch.float32) + torch.tensor(eps, dtype=torch.float32))
    if mutant == "w_first_half":
        wf = torch.cat([wf[..., :64], wf[..., :64]], dim=-1)
    y32 = xf * rinv * wf
    y = y32.to(bf16)
    if cos is None:
        return y, None
    return y, rope_fp32(y32 if mutant == "no_round" else y, cos, sin, B, mutant=mutant)


def rope_fp32(y: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, B: int, mutant: str = "") -> torch.Tensor:
    """the rotation alone, in fp32 as the kernel writes it, on given normalised values y [rows][H][128]"""
    yy = _f(y)
    c, s = _rope_tables(_f(cos), _f(sin), yy.shape[0], B, by_mod=mutant == "pos_mod")
    ya, yb = yy[..., :64], yy[..., 64:]
    if mutant == "rot_sign":
        oa, ob = ya * c[..., :64] + yb * s[..., :64], yb * c[..., 64:] - ya * s[..., 64:]
    else:
        oa, ob = ya * c[..., :64] - yb * s[..., :64], yb * c[..., 64:] + ya * s[..., 64:]
    return torch.cat([oa, ob], dim=-1).to(bf16)


RMS_FAMILIES = 6  # a row's family is row % 6
RMS_ZERO_FAMILY = 5
# (S, B, H_q, H_k): H_k = 0 is the one-region entry. rows = S B; rows H and (octet form) rows H / 8 are no multiples of 32 and fill more than one
# workgroup: 37 pairs; 117 pairs; 35 octets / 280 pairs; 42 octets / 336 pairs; pair entry 45 octets / 120 + 240 pairs; 66 + 110 pairs
RMS_CASES = [(37, 1, 1, 0), (13, 3, 3, 0), (35, 1, 8, 0), (7, 2, 24, 0), (5, 3, 8, 16), (11, 2, 3, 5)]


@functools.lru_cache(maxsize=None)
def rms_inputs(S: int, B: int, H_q: int, H_k: int):
    """-> x [S B][H][128] bf16, w [H][128] (H = H_q + H_k; w_q on the first H_q heads, w_k on the rest), cos, sin fp32 [S][128] (every position
    and both halves differ). Families by row % 6: randn; 2^-12 randn (mean(x^2) = 6e-8, eps dominates); 256 randn; a per-row magnitude
    2^-16 .. 2^8; one-hot heads (the hot dim moves with row and head); all-zero heads (padded context tokens)."""
    H, rows = H_q + H_k, S * B
    g = torch.Generator().manual_seed(2000 + 101 * S + 11 * B + H_q + 3 * H_k)
    x = torch.randn(rows, H, 128, generator=g)
    r = torch.arange(rows)
    fam = r % RMS_FAMILIES
    x[fam == 1] *= 2.0 ** -12
    x[fam == 2] *= 256.0
    spread = 2.0 ** (torch.rand(rows, generator=g) * 24 - 16)
    x[fam == 3] *= spread[fam == 3].view(-1, 1, 1)
    hot = torch.zeros(rows, H, 128)
    hd = (r.view(-1, 1) * 37 + torch.arange(H).view(1, -1) * 29) % 128
    hot.scatter_(2, hd.unsqueeze(-1), 1.0)
    x[fam == 4] = (hot * x.abs().clamp(min=0.25))[fam == 4] * 3
    x[fam == RMS_ZERO_FAMILY] = 0
    wq = (torch.rand(128, generator=g) + 0.5).to(bf16)
    wk = (torch.rand(128, generator=g) + 0.5).to(bf16)
    w = torch.stack([wq] * H_q + [wk] * H_k)
    freqs = torch.randn(S, 128, generator=g) * 3
    return x.to(bf16), w, torch.cos(freqs).contiguous(), torch.sin(freqs).contiguous()


# =================================================================================================================================
# small-M GEMV, SiLU
# =================================================================================================================================
def silu64(a: torch.Tensor) -> torch.Tensor:
    ad = _d(a)
    return ad / (1.0 + torch.exp(-ad))


@functools.lru_cache(maxsize=None)
def all_bf16():
    """every bf16 bit pattern, indexed by its unsigned 16-bit value"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(bf16)


@functools.lru_cache(maxsize=None)
def silu_near_tie():
    """bool [65536] by bit pattern: finite values whose silu64 lies within 2^-10 bf16 ulp of a rounding tie (the middle between two bf16
    neighbours). An approximate exp may round those either way; every other finite value has one right answer, bf16_round(silu64(a))."""
    a = all_bf16()
    s = silu64(a)
    q = s / bf16_ulp(s)
    near = ((q - torch.floor(q)) - 0.5).abs() < 2.0 ** -10
    return near & torch.isfinite(a.float())


def silu_safe(a: torch.Tensor) -> torch.Tensor:
    """a with every near-tie value moved to its next bf16 neighbour away from 0 that is not one (bit pattern + 1, repeated)"""
    near = silu_near_tie()
    bits = a.view(torch.int16).to(torch.int32) & 0xFFFF
    for _ in range(8):
        bits = torch.where(near[bits.long()], bits + 1, bits)
    assert not bool(near[bits.long()].any())
    return bits.to(torch.int16).view(bf16)


def gemv_act(a: torch.Tensor, act_in: int) -> torch.Tensor:
    """fp64 act(a): identity, or nn.SiLU in bf16 = bf16_round(silu64(a))"""
    return _d(a) if act_in == 0 else bf16_round(silu64(a)).double()


def gemv_ref(a: torch.Tensor, w: torch.Tensor, act_in: int):
    """a [M][K], w [N][K] -> (ref = act(a) @ w^T, E = 2^-24 |act(a)| @ |w|^T) in fp64"""
    x = gemv_act(a, act_in)
    return x @ _d(w).t(), U24 * (x.abs() @ _d(w).abs().t())


def gemv_fp32(a: torch.Tensor, w: torch.Tensor, add=None, act_in: int = 0, mutant: str = "") -> torch.Tensor:
    """The kernel's order in fp32: lane l owns k = 8 l + 512 j, adds x w element by element, pass by pass, then a 64-lane butterfly;
    x = bf16(silu(a)) in fp32 for act_in = 1; with add: bf16(float(bf16(s)) + add).
    mutant: "add_early" (add applied to the unrounded sum), "silu_no_round"."""
    af, wf = _f(a), _f(w)
    M, K = af.shape
    N = wf.shape[0]
    if act_in == 1:
        af = af / (1.0 + torch.exp(-af))
        if mutant != "silu_no_round":
            af = af.to(bf16).float()
    Kp = (K + 511) // 512 * 512
    ap, wp = torch.zeros(M, Kp), torch.zeros(N, Kp)
    ap[:, :K], wp[:, :K] = af, wf
    ap, wp = ap.view(M, 1, Kp // 512, 64, 8), wp.view(1, N, Kp // 512, 64, 8)
    acc = torch.zeros(M, N, 64)
    for j in range(Kp // 512):
        for e in range(8):
            acc = acc + ap[:, :, j, :, e] * wp[:, :, j, :, e]
    s = _butterfly(acc, 64)
    if add is None:
        return s.to(bf16)
    if mutant == "add_early":
        return (s + _f(add)).to(bf16)
    return (s.to(bf16).float() + _f(add)).to(bf16)


def add_bf16(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """bf16(float(x) + float(y)): exact in fp32, one rounding (what add_inplace and the GEMV's `+ add` must deliver bit for bit)"""
    return (x.float() + y.float()).to(bf16)


# (M, N, K): K = 8 one lane of one pass; 72: 9 lanes; 520: a second pass with one lane, M = 8; 4096: 8 full passes (the timestep MLP);
# 1032: a third pass with one lane, M = 8, N no multiple of the 4 features of a workgroup
GEMV_CASES = [(1, 64, 8), (3, 101, 72), (8, 64, 520), (2, 256, 4096), (8, 100, 1032)]


@functools.lru_cache(maxsize=None)
def gemv_inputs(M: int, N: int, K: int, act_in: int):
    """-> a [M][K] (randn; for act_in = 1 moved off the SiLU near-tie values), w [N][K] (randn / sqrt(K)), add [M][N], all bf16"""
    g = torch.Generator().manual_seed(3000 + 13 * M + N + 5 * K + act_in)
    a = torch.randn(M, K, generator=g).to(bf16)
    if act_in == 1:
        a = silu_safe(a)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(bf16)
    add = torch.randn(M, N, generator=g).to(bf16)
    return a, w, add
