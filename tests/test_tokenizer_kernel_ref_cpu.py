"""Pins tests/tokenizer_kernel_ref.py, the fp64 references the tokenizer's kernel-level GPU tests compare against, so that a wrong test
reference cannot hide a wrong kernel - and reproduces on the CPU the evidence behind the tolerances of tests/test_tokenizer_kernels_gpu.py
(fp32 restatements against fp64; run with -s to see the measured values)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import tokenizer_oracle as tok
from tests import tokenizer_kernel_ref as kr


def _cf(x):
    return x.double().permute(3, 0, 1, 2).unsqueeze(0)


def _cl(y):
    return y[0].permute(1, 2, 3, 0)


@pytest.mark.parametrize("kind,T,H,W", [("s3", 2, 5, 7), ("s3", 1, 4, 1), ("s3", 1, 3, 2), ("t3", 1, 3, 4), ("t3", 4, 3, 4), ("p1", 2, 3, 5),
                                         ("s3s2", 2, 7, 9), ("s3s2", 1, 8, 10), ("s3s2", 1, 7, 10), ("t3s2", 1, 3, 4), ("t3s2", 2, 3, 4), ("t3s2", 5, 3, 4)])
def test_conv_reference_equals_the_oracles_causal_conv3d(kind, T, H, W):
    """Each kind against CausalConv3d as the oracle states it, with the F.pad / cat that hybrid_downsample puts around the two strided ones."""
    x, w, b, r = kr.conv_operands(kind, 16, 12, T, H, W, seed=T + H + W)
    sd = {"c.conv3d.weight": w.double(), "c.conv3d.bias": b.double()}
    xc = _cf(x)
    if kind == "s3":
        want = tok.causal_conv3d(xc, sd, "c", spatial_pad=1)
    elif kind in ("t3", "p1"):
        want = tok.causal_conv3d(xc, sd, "c")
    elif kind == "s3s2":
        want = tok.causal_conv3d(F.pad(xc, (0, 1, 0, 1, 0, 0)), sd, "c", stride=(1, 2, 2))
    else:
        want = tok.causal_conv3d(torch.cat([xc[:, :, :1], xc], dim=2), sd, "c", stride=(2, 1, 1))
    got = kr.conv_ref(kind, x, w, b)
    assert tuple(got.shape) == (*kr.conv_out_shape(kind, T, H, W), 12)
    assert got.dtype == torch.float64 and float((got - _cl(want)).abs().max()) <= 1e-12
    # residual and the absolute-value companion
    assert torch.equal(kr.conv_ref(kind, x, w, b, r), got + r.double())
    A = kr.conv_ref(kind, x, w, b, r, absolute=True)
    assert torch.equal(A, kr.conv_ref(kind, x.abs(), w.abs(), b.abs(), r.abs())) and bool((A >= kr.conv_ref(kind, x, w, b, r).abs()).all())


def test_pack_taps_is_the_layout_the_network_loads():
    w = torch.arange(2 * 8 * 1 * 3 * 3, dtype=torch.float32).reshape(2, 8, 1, 3, 3).to(torch.bfloat16)
    p = kr.pack_taps(w, ldw=16)
    assert p.shape == (9, 2, 16) and torch.isnan(p[:, :, 8:].float()).all()
    for dy in range(3):
        for dx in range(3):
            assert torch.equal(p[dy * 3 + dx, :, :8], w[:, :, 0, dy, dx])


@pytest.mark.parametrize("swish", [False, True])
def test_groupnorm_reference_equals_causal_normalize(swish):
    x, gamma, beta = kr.groupnorm_operands(24, 3, 35, offset=True, seed=1)
    y, stats = kr.groupnorm_ref(x, gamma, beta, swish)
    xc = x.double().reshape(3, 5, 7, 24).permute(3, 0, 1, 2).unsqueeze(0)
    want = tok.causal_normalize(xc, {"n.norm.weight": gamma.double(), "n.norm.bias": beta.double()}, "n")
    want = tok.swish(want) if swish else want
    assert float((y - _cl(want).reshape(3, 35, 24)).abs().max()) <= 1e-12
    assert torch.equal(stats[:, 0], x.double().reshape(3, -1).sum(1)) and torch.equal(stats[:, 1], (x.double() ** 2).reshape(3, -1).sum(1))


def _identity_convs(pre, names, C):
    """conv1 / conv2 contribute nothing, conv3 is the identity: the hybrid blocks reduce to their resampling lines."""
    sd = {}
    for n, k in names:
        sd[f"{pre}.{n}.conv3d.weight"] = torch.zeros(C, C, *k, dtype=torch.float64)
        sd[f"{pre}.{n}.conv3d.bias"] = torch.zeros(C, dtype=torch.float64)
    sd[f"{pre}.conv3.conv3d.weight"] = torch.eye(C, dtype=torch.float64).reshape(C, C, 1, 1, 1)
    sd[f"{pre}.conv3.conv3d.bias"] = torch.zeros(C, dtype=torch.float64)
    return sd


@pytest.mark.parametrize("T,H,W", [(3, 7, 9), (1, 1, 1), (2, 8, 8), (4, 3, 5), (5, 4, 6)])
def test_resample_references_equal_the_hybrid_blocks_lines(T, H, W):
    C = 8
    x = kr.uniform_bf16((T, H, W, C), seed=T * H * W)
    xc = _cf(x)
    # the lines themselves (layers3d.py:217-227, 170-178 as oracle/tokenizer_oracle.py restates them)
    assert torch.equal(kr.resample_ref(0, x), _cl(F.avg_pool3d(F.pad(xc, (0, 1, 0, 1, 0, 0)), (1, 2, 2), (1, 2, 2))))
    assert torch.equal(kr.resample_ref(1, x), _cl(F.avg_pool3d(torch.cat([xc[:, :, :1], xc], dim=2), (2, 1, 1), (2, 1, 1))))
    tf = 2 if T > 1 else 1
    assert torch.equal(kr.resample_ref(2, x), _cl(xc.repeat_interleave(tf, dim=2)[:, :, tf - 1:]))
    assert torch.equal(kr.resample_ref(3, x), _cl(xc.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)))
    for mode in range(4):
        assert tuple(kr.resample_ref(mode, x).shape) == (*kr.resample_out_shape(mode, T, H, W), C)
    # and through the oracle's blocks with their convolutions switched off: down = mode 1 after mode 0, up = mode 3 after mode 2
    if H % 2 or W % 2:  # (the block adds a convolution and a pool of the same padded tensor: their sizes agree for even frames only)
        return
    down = tok.hybrid_downsample(xc, _identity_convs("d", (("conv1", (1, 3, 3)), ("conv2", (3, 1, 1))), C), "d")
    assert float((_cl(down) - kr.resample_ref(1, kr.resample_ref(0, x))).abs().max()) <= 1e-6  # the oracle pools in fp32
    up = tok.hybrid_upsample(xc, _identity_convs("u", (("conv1", (3, 1, 1)), ("conv2", (1, 3, 3))), C), "u")
    assert torch.equal(_cl(up), kr.resample_ref(3, kr.resample_ref(2, x)))


def test_resample_mode0_by_hand():
    """A 3 x 3 frame: the right column and the bottom row average with zeros (count_include_pad), the corner keeps a quarter."""
    x = torch.arange(1, 10, dtype=torch.float32).reshape(1, 3, 3, 1).repeat(1, 1, 1, 8).to(torch.bfloat16)
    y = kr.resample_ref(0, x)[0, :, :, 0]
    assert torch.equal(y, torch.tensor([[(1 + 2 + 4 + 5) / 4, (3 + 6) / 4], [(7 + 8) / 4, 9 / 4]], dtype=torch.float64))


def test_haar_references_are_the_oracles_and_invert_each_other():
    v = kr.uniform_bf16((3, 5, 8, 12), seed=3)
    c = kr.haar_patch_ref(v)
    assert tuple(c.shape) == (2, 2, 3, 192) and c.dtype == torch.float64
    assert torch.equal(c, tok.haar_patch3d(v.double().unsqueeze(0))[0].permute(1, 2, 3, 0))
    back = kr.haar_unpatch_ref(c)
    assert tuple(back.shape) == (3, 5, 8, 12) and float((back - v.double()).abs().max()) <= 1e-12
    # a constant video: every level keeps the constant in its lowest band (8 c / sqrt(2)^3 / (2 sqrt 2) = c) and zero elsewhere
    k = kr.haar_patch_ref(torch.full((3, 1, 4, 4), 0.5, dtype=torch.bfloat16))
    assert float((k[0, 0, 0, :3] - 0.5).abs().max()) <= 1e-12 and float(k[0, 0, 0, 3:].abs().max()) <= 1e-12


def test_bf16_ulp_and_one_step_rounding():
    ref = torch.tensor([1.0, 1.9999, 2.0, -3.0, 0.75, 2.0 ** -126, 0.0, 1e-45], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133], dtype=torch.float64)
    assert torch.equal(kr.bf16_ulp(ref), want)
    # neighbouring bf16 values are one ulp apart
    a = torch.tensor([1.0, 1.5, -2.5, 100.0], dtype=torch.bfloat16)
    nxt = (a.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - a.double()).abs(), kr.bf16_ulp(a.double()))
    # a value that fp32 rounds UP onto a bf16 tie and bf16 then rounds to even the wrong way: 1 + 2^-8 - 2^-40 must go down to 1
    tricky = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)
    assert torch.equal(kr.bf16_round(tricky).double(), torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6], dtype=torch.float64))
    g = torch.Generator().manual_seed(0)
    v = torch.randn(4096, generator=g)
    assert torch.equal(kr.bf16_round(v.double()), v.to(torch.bfloat16))  # fp32 values: one rounding either way
    assert float(kr.ulp_error(kr.bf16_round(v.double()), v.double()).max()) <= 0.5


# ---- the evidence behind the GPU tolerances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K", [("t3", 16), ("t3", 512), ("s3", 16), ("s3", 72), ("s3", 192), ("s3", 512), ("s3s2", 128), ("t3s2", 64)])
def test_evidence_conv_gamma_covers_fp32_accumulation(kind, K):
    """An fp32 F.conv3d against the fp64 one, as a fraction of the absolute-value companion A: the GPU bound's GAMMA = 2^-21 = 4.8e-7 has to
    stay a few times above it (the MFMA sums in another order). Measured 2e-8 to 1e-7 over K = 16..512 and 3..9 taps."""
    x, w, b, r = kr.conv_operands(kind, K, 16, 3, 9, 11, seed=K)
    ref = kr.conv_ref(kind, x, w, b, r)
    A = kr.conv_ref(kind, x, w, b, r, absolute=True)
    ksize, stride = kr.CONV_KINDS[kind]
    y32 = F.conv3d(kr.conv_pad(kind, _cf(x)).float(), w.float(), None, stride=stride)
    y32 = (_cl(y32) + b.float()) + r.float()
    ratio = float(((y32.double() - ref).abs() / A).max())
    print(f"[evidence conv {kind} K={K}] fp32 vs fp64 max |err| / A = {ratio:.2e}  (GAMMA = {kr.GAMMA:.2e})")
    assert ratio * 4 <= kr.GAMMA
    # and the bound passes a correctly rounded fp32 result while a dropped tap misses it by orders of magnitude
    bound = kr.conv_bound(ref, A)
    assert bool(((y32.to(torch.bfloat16).double() - ref).abs() <= bound).all())
    if ksize != (1, 1, 1):
        w_bad = w.clone()
        w_bad[:, :, -1, -1, -1] = 0
        worst = float(((kr.conv_ref(kind, x, w_bad, b, r) - ref).abs() / bound).max())
        assert worst > 50


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("swish", [False, True])
@pytest.mark.parametrize("shift", [False, True])
def test_evidence_groupnorm_fp32_restatement_stays_inside_one_ulp(offset, swish, shift):
    """GroupNorm in fp32, rounded once, against fp64: the worst element in bf16 ulps and the share of elements that differ from the correctly
    rounded reference, for the restatement that shares the kernels' fp64 statistics and two-float mean (the GPU test allows 1.0 ulp and ten
    times THIS share, floor 1e-3) and, printed beside it, for the one whose two passes are fp32 throughout.
    Measured: fp64 statistics 0.50 ulp everywhere, share <= 1e-4; fp32 throughout 0.93 ulp on the offset input at 1024 x 1000 and 15 ulp at
    512 x 1000 (a frame whose mean lies 6e-5 from a bf16 value many pixels take), share up to 4e-2 - the mean alone does that."""
    worst, share_worst = 0.0, 0.0
    for C, rows in ((64, 1000), (192, 77), (1024, 1000), (16, 5), (512, 1000)):
        x, gamma, beta = kr.groupnorm_operands(C, 3, rows, offset, seed=C + rows, shift=shift)
        ref, _ = kr.groupnorm_ref(x, gamma, beta, swish)
        want = kr.bf16_round(ref)
        line = f"[evidence groupnorm C={C} rows={rows} offset={offset} swish={swish} shift={shift}]"
        for fp64_stats in (True, False):
            y32 = kr.groupnorm_fp32(x, gamma, beta, swish, fp64_stats=fp64_stats)
            err, share = float(kr.ulp_error(y32, ref).max()), float((y32 != want).double().mean())
            line += f"  {'fp64 statistics' if fp64_stats else 'fp32 throughout'}: max {err:.3f} ulp, share != bf16(ref) {share:.2e};"
            if fp64_stats:
                worst, share_worst = max(worst, err), max(share_worst, share)
        print(line)
    assert worst <= 1.0 and share_worst <= 1e-3


def test_evidence_resample_fp32_average_is_exact_for_the_committed_inputs():
    """Up to four bf16 values summed in fp32 and scaled by a power of two: exact, so the rounded fp64 reference is the only right answer.
    Zero mismatches on every input the GPU test uses."""
    total = 0
    for mode, T, H, W in kr.RESAMPLE_CASES:
        for C in kr.RESAMPLE_CHANNELS:
            x = kr.resample_input(mode, T, H, W, C)
            got = kr.resample_ref(mode, x, dtype=torch.float32).to(torch.bfloat16)
            total += int((got != kr.bf16_round(kr.resample_ref(mode, x))).sum())
    print(f"[evidence resample] fp32 restatement vs bf16(fp64 reference): {total} mismatches")
    assert total == 0
