"""fp64 references of the tokenizer's kernels, one operation at a time (TEST INFRASTRUCTURE - a plain helper module).

Every function restates what the reference's module computes (tokenizer/modules/layers3d.py, utils.py, patching.py), with explicit padding
followed by a stock torch operator in float64 - never the kernels' (ot, oh, ow) tap arithmetic, so that a mistake in that arithmetic cannot
be shared by the kernel and its reference. tests/test_tokenizer_kernel_ref_cpu.py pins this module against oracle/tokenizer_oracle.py;
tests/test_tokenizer_kernels_gpu.py holds the HIP kernels against it.

Layouts: activations channels-last [T][H][W][C] (what the kernels take); convolution weights in torch's [N][K][kt][kh][kw].
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import tokenizer_oracle as tok

# kind -> (kernel size, stride) of the convolution that follows the padding written out in `conv_pad`
CONV_KINDS = {
    "s3": ((1, 3, 3), (1, 1, 1)),
    "t3": ((3, 1, 1), (1, 1, 1)),
    "p1": ((1, 1, 1), (1, 1, 1)),
    "s3s2": ((1, 3, 3), (1, 2, 2)),
    "t3s2": ((3, 1, 1), (2, 1, 1)),
}

GAMMA = 2.0 ** -21  # fp32-accumulation allowance of the convolution bound, relative to the absolute-value companion


def _cf(x: torch.Tensor) -> torch.Tensor:
    """[T][H][W][C] -> float64 [1][C][T][H][W]"""
    return x.detach().cpu().double().permute(3, 0, 1, 2).unsqueeze(0)


def _cl(y: torch.Tensor) -> torch.Tensor:
    """[1][C][T][H][W] -> [T][H][W][C]"""
    return y[0].permute(1, 2, 3, 0).contiguous()


def conv_pad(kind: str, x: torch.Tensor) -> torch.Tensor:
    """The padding each convolution of the network sees, on a channels-first [1][C][T][H][W] tensor."""
    if kind == "s3":      # CausalConv3d (1,3,3), padding 1: zeros on all four sides of a frame
        return F.pad(x, (1, 1, 1, 1, 0, 0))
    if kind == "t3":      # CausalConv3d (3,1,1): the first frame twice in front
        return torch.cat([x[:, :, :1], x[:, :, :1], x], dim=2)
    if kind == "p1":
        return x
    if kind == "s3s2":    # hybrid down-sampling: one zero column right, one zero row below, then stride (1,2,2) without further padding
        return F.pad(x, (0, 1, 0, 1, 0, 0))
    if kind == "t3s2":    # hybrid down-sampling: the first frame once by the block, once more by the stride-2 CausalConv3d
        return torch.cat([x[:, :, :1], x[:, :, :1], x], dim=2)
    raise KeyError(kind)


def conv_out_shape(kind: str, T: int, H: int, W: int):
    if kind == "s3s2":
        return T, (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
    if kind == "t3s2":
        return (T + 2 - 3) // 2 + 1, H, W
    return T, H, W


def conv_ref(kind: str, x: torch.Tensor, w: torch.Tensor, b=None, r=None, absolute: bool = False) -> torch.Tensor:
    """x [T][H][W][K], w [N][K][kt][kh][kw], b [N] or None, r [To][Ho][Wo][N] or None -> float64 [To][Ho][Wo][N].
    absolute=True: the companion A = conv(|x|, |w|) + |b| + |r| that scales the accumulation allowance."""
    ksize, stride = CONV_KINDS[kind]
    assert tuple(w.shape[2:]) == ksize, f"{kind}: weight {tuple(w.shape)}"
    fx = (lambda t: t.abs()) if absolute else (lambda t: t)
    xp = conv_pad(kind, fx(_cf(x)))
    y = _cl(F.conv3d(xp, fx(w.detach().cpu().double()), None, stride=stride))
    if b is not None:
        y = y + fx(b.detach().cpu().double())
    if r is not None:
        y = y + fx(r.detach().cpu().double())
    return y


def pack_taps(w: torch.Tensor, ldw: int = 0, fill: float = float("nan")) -> torch.Tensor:
    """[N][K][kt][kh][kw] -> the library's tap-major [kt*kh*kw][N][ldw] (K contiguous), padding columns = fill."""
    N, K = w.shape[:2]
    t = w.permute(2, 3, 4, 0, 1).reshape(-1, N, K)
    ldw = ldw or K
    out = torch.full((t.shape[0], N, ldw), fill, dtype=w.dtype)
    out[:, :, :K] = t
    return out


def groupnorm_ref(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, swish: bool, eps: float = 1e-6):
    """CausalNormalize with one group: x [frames][rows][C] -> (float64 y, float64 stats [frames][2] = sum, sum of squares).
    Two-pass mean and (biased) variance per frame."""
    xd = x.detach().cpu().double()
    mean = xd.mean(dim=(1, 2), keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=(1, 2), keepdim=True)
    y = (xd - mean) / torch.sqrt(var + eps) * gamma.detach().cpu().double() + beta.detach().cpu().double()
    if swish:
        y = y * torch.sigmoid(y)
    stats = torch.stack([xd.sum(dim=(1, 2)), (xd * xd).sum(dim=(1, 2))], dim=1)
    return y, stats


def groupnorm_fp32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, swish: bool, eps: float = 1e-6, fp64_stats: bool = True) -> torch.Tensor:
    """GroupNorm in fp32 with one final rounding to bf16: what a careful fp32 kernel can deliver. Used only to measure, on the CPU, how far fp32
    arithmetic alone is from the fp64 reference (the evidence behind the GroupNorm bounds).
    fp64_stats=True (what the kernels do): mean and variance from fp64 sums, the mean subtracted as two floats (its fp32 rounding and the
    remainder), everything after that in fp32. fp64_stats=False: both passes in fp32 - its mean is off by up to 2^-25 |mean|, which costs
    several ulps wherever a frame far from 0 has pixels next to its mean."""
    xf = x.detach().cpu().float()
    if fp64_stats:
        xd = x.detach().cpu().double()
        mean_d = xd.mean(dim=(1, 2), keepdim=True)
        var = ((xd - mean_d) ** 2).mean(dim=(1, 2), keepdim=True).float()
        mean_hi = mean_d.float()
        mean_lo = (mean_d - mean_hi.double()).float()
        d = (xf - mean_hi) - mean_lo
    else:
        mean = xf.mean(dim=(1, 2), keepdim=True)
        var = ((xf - mean) ** 2).mean(dim=(1, 2), keepdim=True)
        d = xf - mean
    y = d * torch.rsqrt(var + eps) * gamma.detach().cpu().float() + beta.detach().cpu().float()
    if swish:
        y = y * torch.sigmoid(y)
    return y.to(torch.bfloat16)


def resample_out_shape(mode: int, T: int, H: int, W: int):
    return {0: (T, (H + 1) // 2, (W + 1) // 2), 1: ((T + 1) // 2, H, W), 2: (2 * T - 1 if T > 1 else 1, H, W), 3: (T, 2 * H, 2 * W)}[mode]


def resample_ref(mode: int, x: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """The four resampling steps of CausalHybridDownsample3d / CausalHybridUpsample3d on x [T][H][W][C] -> `dtype` [To][Ho][Wo][C]."""
    v = x.detach().cpu().to(dtype).permute(3, 0, 1, 2).unsqueeze(0)
    if mode == 0:    # zeros right and below, then the (1,2,2) average
        v = F.avg_pool3d(F.pad(v, (0, 1, 0, 1, 0, 0)), (1, 2, 2), (1, 2, 2))
    elif mode == 1:  # the first frame once in front, then the (2,1,1) average
        v = F.avg_pool3d(torch.cat([v[:, :, :1], v], dim=2), (2, 1, 1), (2, 1, 1))
    elif mode == 2:  # every frame twice, without the first copy; a single frame (an image) is left alone
        v = v.repeat_interleave(2, dim=2)[:, :, 1:] if v.shape[2] > 1 else v
    elif mode == 3:
        v = v.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    else:
        raise KeyError(mode)
    return _cl(v)


def haar_patch_ref(video: torch.Tensor) -> torch.Tensor:
    """video [3][T][H][W] -> float64 coefficients [Tp][Hp][Wp][192] (Patcher3D, patch size 4)."""
    return _cl(tok.haar_patch3d(video.detach().cpu().double().unsqueeze(0)))


def haar_unpatch_ref(coef: torch.Tensor) -> torch.Tensor:
    """coef [Tp][Hp][Wp][192] -> float64 video [3][4 Tp - 3][4 Hp][4 Wp] (UnPatcher3D)."""
    return tok.haar_unpatch3d(_cf(coef))[0]


def bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at ref: 2^(floor(log2 |ref|) - 7), in fp64; the subnormal spacing 2^-133 below the smallest normal (and at 0)."""
    ref = ref.double()
    _, ex = torch.frexp(ref.abs())  # |ref| = m 2^ex with m in [0.5, 1): floor(log2 |ref|) = ex - 1
    e = torch.where(ref == 0, torch.full_like(ex, -126), ex - 1).clamp(min=-126)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 7).double())


def bf16_round(ref: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even of an fp64 tensor to bf16 in ONE step (torch's double -> bfloat16 goes through fp32: two roundings)."""
    u = bf16_ulp(ref)
    return (torch.round(ref.double() / u) * u).to(torch.bfloat16)  # torch.round: half to even; both scalings are exact


def ulp_error(out: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """|out - ref| in units of bf16_ulp(ref), elementwise, fp64."""
    return (out.detach().cpu().double() - ref).abs() / bf16_ulp(ref)


def conv_bound(ref: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """Per element: one correct rounding of an fp32-accumulated sum, 0.5 ulp + GAMMA * A."""
    return 0.5 * bf16_ulp(ref) + GAMMA * A


# ---- seeded inputs shared by the CPU evidence and the GPU tests (bf16, built on the CPU) ----------------------------------------------
def randn_bf16(shape, seed: int, mean: float = 0.0, std: float = 1.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std + mean).to(torch.bfloat16)


def uniform_bf16(shape, seed: int) -> torch.Tensor:
    """uniform in [-1, 1], as video is"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(torch.bfloat16)


def conv_operands(kind: str, K: int, N: int, T: int, H: int, W: int, seed: int):
    """x [T][H][W][K], w [N][K][kt][kh][kw] (fan-in scaled), b [N], r [To][Ho][Wo][N]: all bf16."""
    kt, kh, kw = CONV_KINDS[kind][0]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, W, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, kt, kh, kw, generator=g) / (K * kt * kh * kw) ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g).to(torch.bfloat16)
    r = torch.randn(*conv_out_shape(kind, T, H, W), N, generator=g).to(torch.bfloat16)
    return x, w, b, r


def groupnorm_operands(C: int, frames: int, rows: int, offset: bool, seed: int, shift: bool = False):
    """x [frames][rows][C]: N(0,1), or mean 6 / std 0.25 (stresses E[x^2] - mean^2 and fp32 partial sums); gamma in [0.5, 1.5].

    beta: an output bound counted in ulps OF THE RESULT cannot hold, in any fp32 evaluation, where (x - mean) rstd gamma and beta cancel to a
    result far smaller than either (the fp32 rounding of the two terms is then many ulps of their difference; with beta ~ 0.05 N(0,1) the fp32
    restatement itself is 2 ulp off at a handful of 3 M elements). So beta is either 0 (shift=False: every error in the mean, the variance,
    gamma or the activation shows at full sensitivity) or of magnitude 9..12 with a random sign (shift=True: |normalised x| gamma stays
    below 8.3 for these sizes, the result never comes near 0, and a wrong or misplaced beta is off by whole units)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(frames, rows, C, generator=g)
    x = (x * 0.25 + 6.0 if offset else x).to(torch.bfloat16)
    gamma = (torch.rand(C, generator=g) + 0.5).to(torch.bfloat16)
    beta = (torch.rand(C, generator=g) * 3 + 9) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    beta = (beta if shift else torch.zeros(C)).to(torch.bfloat16)
    return x, gamma, beta


RESAMPLE_CASES = [  # (mode, T, H, W)
    (0, 3, 7, 9), (0, 1, 1, 1), (0, 2, 8, 8),
    (1, 1, 3, 5), (1, 4, 3, 5), (1, 5, 3, 5),
    (2, 1, 3, 5), (2, 3, 3, 5),
    (3, 2, 3, 5),
]
RESAMPLE_CHANNELS = (8, 64, 192)


def resample_input(mode: int, T: int, H: int, W: int, C: int) -> torch.Tensor:
    return randn_bf16((T, H, W, C), seed=1000 * mode + 100 * T + 10 * H + W + C)


# =================================================================================================================================
# the convolution cases of the kernel-level GPU files (tests/test_tokenizer_kernels_gpu.py, tests/test_far_operands_gpu.py)
# =================================================================================================================================
CONV_GEOM = {  # what the library is told: kt, kh, kw, st, sh, sw, ot, oh, ow  (gen3c_amd/tokenizer.py). The REFERENCE never sees these numbers.
    "s3": (1, 3, 3, 1, 1, 1, 0, -1, -1), "t3": (3, 1, 1, 1, 1, 1, -2, 0, 0), "p1": (1, 1, 1, 1, 1, 1, 0, 0, 0),
    "s3s2": (1, 3, 3, 1, 2, 2, 0, 0, 0), "t3s2": (3, 1, 1, 2, 1, 1, -2, 0, 0),
}

# name: (kind, K, N, T, H, W, epilogue, pad of ld_in, ldw, ld_out, ldr, entry, meant for the one-wave kernel)
CONV_CASES = {
    "ragged_m_n": ("s3", 128, 136, 2, 9, 31, "res", 8, 8, 8, 8, "stats", True),       # M = 558: two whole M tiles and 46 rows; N = 136 of a 256 tile
    "one_tile": ("s3", 64, 256, 1, 16, 16, "bias", 0, 0, 0, 0, "plain", True),        # M = 256, N = 256 exactly, dense as the network calls it
    "one_tile_padded": ("s3", 64, 256, 1, 16, 16, "res", 8, 8, 8, 16, "stats", True),  # the same tile with every leading dimension padded
    "t3_image": ("t3", 64, 16, 1, 5, 7, "none", 8, 0, 16, 0, "plain", True),          # T = 1: all three taps read frame 0; production N = 16
    "t3_video": ("t3", 192, 192, 4, 6, 10, "res", 0, 8, 0, 8, "stats", True),
    "t3s2_image": ("t3s2", 64, 12, 1, 4, 6, "bias", 8, 8, 8, 0, "plain", False),      # N % 8 == 4: narrow store
    "t3s2_T2": ("t3s2", 16, 192, 2, 5, 9, "res", 8, 8, 8, 8, "plain", False),         # K = 16 (the decoder's first convolution) - direct loads
    "t3s2_T5": ("t3s2", 192, 16, 5, 6, 10, "none", 0, 0, 8, 0, "stats", True),
    "s3_W1": ("s3", 64, 16, 2, 5, 1, "bias", 8, 8, 8, 0, "plain", True),              # both horizontal neighbours are padding
    "s3_W2": ("s3", 72, 4, 1, 6, 2, "bias", 8, 8, 8, 0, "plain", False),              # K = 72: a ragged second K tile; N = 4
    "s3s2_odd": ("s3s2", 128, 260, 1, 7, 9, "bias", 8, 8, 8, 0, "plain", False),      # N = 260: second N tile of 4 columns, narrow store
    "s3s2_even": ("s3s2", 512, 16, 2, 8, 10, "res", 8, 8, 8, 8, "stats", True),       # bottom row / right column of windows half outside
    "s3s2_mixed": ("s3s2", 64, 192, 1, 7, 10, "none", 0, 0, 0, 0, "plain", True),
    "p1_tiny": ("p1", 8, 4, 1, 3, 5, "none", 8, 8, 8, 0, "plain", False),
    "p1_wide": ("p1", 512, 192, 2, 9, 15, "res", 8, 8, 8, 8, "plain", True),          # M = 270
    "ldr_mod8_4": ("s3", 64, 16, 2, 6, 7, "res", 0, 0, 0, 4, "plain", False),         # residual rows not 16-byte addressable: wide stores off
}
CONV_PATHS = {
    "w4_gaps": dict(conv_w4=1),                      # one wave per SIMD, tap change in the MFMA gaps
    "w4_stmt": dict(conv_w4=2),                      # one wave per SIMD, tap change between statements
    "pingpong": dict(conv_w4=0, gemm_pingpong=3),
    "lds_dma": dict(conv_w4=0, gemm_pingpong=0),     # gemm_bf16_nt_kernel, LDS-DMA staging
    "direct": dict(gemm_regstage=1),                 # gemm_bf16_nt_kernel, register staging (also what K % 64 != 0 takes under any options)
}
