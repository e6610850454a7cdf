"""The tokenizer's HIP kernels one by one, through the C ABI, against the fp64 references of tests/tokenizer_kernel_ref.py (which
tests/test_tokenizer_kernel_ref_cpu.py pins against the oracle): the convolutions on every kernel path, their GroupNorm statistics, GroupNorm,
the resampling modes, the Haar patcher and its inverse, the 2-D transpose, and the documented refusals.

Rules every test here keeps: inputs are bf16 tensors built on the CPU from a seeded generator and feed kernel and reference alike; every
output lives in a NaN-filled buffer with padding columns (where the entry takes a leading dimension; three convolution cases keep the
network's own dense ld_out = N beside padded twins of the same kind) and 64 guard rows on both sides, which must come back bit for bit
untouched around a finite payload; convolution inputs sit between NaN guard rows (at least Wi + 2 positions) with
NaN in their padding channels, so a tap that reads a neighbour instead of the zero page, or the wrong frame past the tensor, surfaces as a
NaN. Options are restored to the library's defaults in try / finally.

Measured on an MI355X (profiles/tokenizer_kernel_parity_measured.txt): see the docstrings."""
import functools
from contextlib import contextmanager

import pytest
import torch

from tests import tokenizer_kernel_ref as kr
from tests.guarded import GUARD, Guarded, _dev

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEFAULTS = {"conv_w4": 1, "gemm_pingpong": 3, "gemm_regstage": 0, "gemm_wide_store": 1}


def _lib():
    from gen3c_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextmanager
def _options(**kw):
    from gen3c_amd import ops
    try:
        for k, v in kw.items():
            ops.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            ops.set_option(k, v)


def _err_names(entry):
    L, lib = _lib()
    msg = L.last_error()
    assert entry in msg, f"g3_last_error does not name {entry}: {msg!r}"


# =================================================================================================================================
# convolutions
# =================================================================================================================================
_GEOM, _CONV_CASES, _CONV_PATHS = kr.CONV_GEOM, kr.CONV_CASES, kr.CONV_PATHS  # (shared with tests/test_far_operands_gpu.py)


def _conv_params():
    out = []
    for name, c in _CONV_CASES.items():
        K, w4 = c[1], c[12]
        for path in _CONV_PATHS:
            if path.startswith("w4") and not w4:
                continue
            if path in ("pingpong", "lds_dma") and K % 64:
                continue
            out.append(pytest.param(name, path, id=f"{name}-{path}"))
    return out


def _one_wave_kernel_applies(K, N, taps, ld_out, ldr, has_res, opts):
    """conv_w4_applies of gemm.hip, restated (pointers here are 16-byte aligned, the tensors far below 2^31 rows)."""
    o = {**DEFAULTS, **opts}
    wide = o["gemm_wide_store"] and N % 8 == 0 and ld_out % 8 == 0 and (not has_res or ldr % 8 == 0)
    return bool(o["conv_w4"] and K % 64 == 0 and not o["gemm_regstage"] and wide and (K // 64) * taps >= 2 and K * 2 <= 8192)


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    """operands and fp64 reference of a case, computed once and shared by its kernel paths (never modified)"""
    kind, K, N, T, H, W, epi = _CONV_CASES[name][:7]
    x, w, b, r = kr.conv_operands(kind, K, N, T, H, W, seed=sum(map(ord, name)))
    b_, r_ = (b if epi != "none" else None), (r if epi == "res" else None)
    return x, w, b_, r_, kr.conv_ref(kind, x, w, b_, r_), kr.conv_ref(kind, x, w, b_, r_, absolute=True)


def _run_conv(kind, x, w, b, r, pads, entry, stats_start=0.0, gn_rows=None):
    """One library call on guarded buffers -> (output [To][Ho][Wo][N] bf16 on the CPU, statistics [To][2] fp64 on the CPU or None)."""
    L, lib = _lib()
    T, H, W, K = x.shape
    N = w.shape[0]
    To, Ho, Wo = kr.conv_out_shape(kind, T, H, W)
    M = To * Ho * Wo
    p_in, p_w, p_out, p_r = pads
    xin = Guarded(T * H * W, K, K + p_in, guard=max(GUARD, W + 2), data=x)
    wt = kr.pack_taps(w, K + p_w).to(_dev())
    bias = b.to(_dev()) if b is not None else None
    res = Guarded(M, N, N + p_r, data=r) if r is not None else None
    out = Guarded(M, N, N + p_out)
    args = [xin.ptr, K + p_in, wt.data_ptr(), K + p_w, bias.data_ptr() if bias is not None else None, res.ptr if res is not None else None,
            N + p_r, out.ptr, N + p_out, K, N, T, H, W, To, Ho, Wo, *_GEOM[kind]]
    stats = None
    if entry == "stats":
        stats = torch.full((To + 2, 2), float(stats_start), dtype=torch.float64, device=_dev())  # one sentinel pair in front and behind
        rc = lib.g3_conv3d_cl_gnstats_bf16(*args, stats[1:].data_ptr(), gn_rows or Ho * Wo, _stream())
    else:
        rc = lib.g3_conv3d_cl_bf16(*args, _stream())
    L.check(rc, f"g3_conv3d_cl ({entry})")
    torch.cuda.synchronize()
    out.assert_only_payload_written(f"conv {kind} K={K} N={N}")
    if stats is not None:
        stats = stats.cpu()
        assert torch.equal(stats[[0, -1]], torch.full((2, 2), float(stats_start), dtype=torch.float64)), "statistics written outside [frames][2]"
        stats = stats[1:-1]
    return out.cpu().reshape(To, Ho, Wo, N), stats


def _conv_ratio(out, ref, A):
    return float(((out.double() - ref).abs() / kr.conv_bound(ref, A)).max())


def _stats_err(stats, out, start=0.0):
    """the project's bound on delivered GroupNorm statistics: against fp64 sums of the STORED bf16 output, relative to |ref| + 1"""
    of = out.double().reshape(out.shape[0], -1)
    ref = torch.stack([of.sum(1), (of * of).sum(1)], dim=1) + start
    return float(((stats - ref).abs() / (ref.abs() + 1.0)).max())


@pytest.mark.parametrize("name,path", _conv_params())
def test_conv_every_kernel_path_against_fp64_reference(name, path):
    """Five kinds x five kernel paths x three epilogues x both entries, at the smallest shapes that reach each edge of the 256 x 256 x 64 tile
    (see _CONV_CASES). Per element |out - ref| <= 0.5 bf16_ulp(ref) + 2^-21 A with A = conv(|x|, |w|) + |b| + |r|: one correct rounding of
    (acc + bias) + residual accumulated in fp32 - the allowance is ~5x what an fp32 F.conv3d shows against fp64 on the CPU (2e-8 .. 1e-7 of A,
    tests/test_tokenizer_kernel_ref_cpu.py) and ~1e-5 |ref|, while a missing, misplaced or wrongly padded tap misses by orders of magnitude.
    Measured: worst err / bound over all cases and paths 1.000 (0.981 .. 1.000: the rounding term alone) (profiles/tokenizer_kernel_parity_measured.txt)."""
    kind, K, N, T, H, W, epi, p_in, p_w, p_out, p_r, entry, w4 = _CONV_CASES[name]
    opts = _CONV_PATHS[path] if not (path == "direct" and K % 64) else {}
    taps = _GEOM[kind][0] * _GEOM[kind][1] * _GEOM[kind][2]
    applies = _one_wave_kernel_applies(K, N, taps, N + p_out, N + p_r, epi == "res", opts)
    assert applies == path.startswith("w4"), f"{name}/{path}: the case does not reach the kernel it is meant for"
    assert w4 == _one_wave_kernel_applies(K, N, taps, N + p_out, N + p_r, epi == "res", {})
    x, w, b, r, ref, A = _conv_case(name)
    with _options(**opts):
        out, stats = _run_conv(kind, x, w, b, r, (p_in, p_w, p_out, p_r), entry)
    ratio = _conv_ratio(out, ref, A)
    print(f"[conv {name} {path}] {kind} K={K} N={N} ({T},{H},{W}) {epi}/{entry}: max err / (0.5 ulp + 2^-21 A) = {ratio:.3f}")
    assert ratio <= 1.0
    if stats is not None:
        e = _stats_err(stats, out)
        print(f"[conv {name} {path}] statistics rel err {e:.2e}")
        assert e < 2e-6


def test_conv_residual_without_bias_is_refused():
    L, lib = _lib()
    x, w, b, r = kr.conv_operands("p1", 64, 16, 1, 4, 4, seed=1)
    xin, wt, res, out = Guarded(16, 64, data=x), kr.pack_taps(w).to(_dev()), Guarded(16, 16, data=r), Guarded(16, 16)
    rc = lib.g3_conv3d_cl_bf16(xin.ptr, 64, wt.data_ptr(), 64, None, res.ptr, 16, out.ptr, 16, 64, 16, 1, 4, 4, 1, 4, 4, *_GEOM["p1"], _stream())
    torch.cuda.synchronize()
    assert rc != 0
    _err_names("g3_conv3d_cl_bf16")
    assert bool(torch.isnan(out.buf.float()).all()), "a refused call wrote output"


@functools.lru_cache(maxsize=None)
def _stats_case(H, W):
    x, w, b, r = kr.conv_operands("s3", 64, 64, 3, H, W, seed=H * W)
    return x, w, b, r, kr.conv_ref("s3", x, w, b, r), kr.conv_ref("s3", x, w, b, r, absolute=True)


@pytest.mark.parametrize("start", [0.0, 1000.5])
@pytest.mark.parametrize("producer", ["default", "pingpong"])
@pytest.mark.parametrize("H,W", [(8, 12), (8, 16), (10, 16), (12, 19)])
def test_conv_groupnorm_statistics_are_added_by_both_producers(H, W, producer, start):
    """g3_conv3d_cl_gnstats_bf16 with Ho Wo = 96 (below a wave quadrant: the statistics pass even under default options), 128 (exactly one
    quadrant per frame), 160 and 228 (frames straddle quadrants and tiles), three frames. The epilogue of the one-wave kernel ('default') and the
    separate pass behind any other kernel ('pingpong': conv_w4 = 0) must both ADD sum and sum of squares of the stored bf16 output to what the
    buffer held. Bound: the project's |stat - ref| / (|ref| + 1) < 2e-6 against fp64 sums. Measured: worst 4.3e-8."""
    x, w, b, r, ref, A = _stats_case(H, W)
    opts = {} if producer == "default" else {"conv_w4": 0}
    # which producer runs, restated from conv3d_cl: the epilogue where the one-wave kernel applies and a frame is at least 128 rows
    fused = _one_wave_kernel_applies(64, 64, 9, 72, 72, True, opts) and H * W >= 128
    assert fused == (producer == "default" and H * W >= 128), "the case does not reach the producer it is meant for"
    with _options(**opts):
        out, stats = _run_conv("s3", x, w, b, r, (8, 8, 8, 8), "stats", stats_start=start)
    assert _conv_ratio(out, ref, A) <= 1.0
    e = _stats_err(stats, out, start)
    print(f"[conv statistics Ho*Wo={H * W} {producer} start={start}] rel err {e:.2e}")
    assert e < 2e-6


# =================================================================================================================================
# GroupNorm
# =================================================================================================================================
def _gn_cases():
    out = [pytest.param(C, rows, offset, False, id=f"C{C}-rows{rows}-{'offset' if offset else 'centred'}")
           for C in (16, 64, 192, 512, 1024) for rows in (1, 5, 77, 1000) for offset in (False, True)]
    out += [pytest.param(C, 77, offset, True, id=f"C{C}-rows77-{'offset' if offset else 'centred'}-beta") for C in (16, 64, 192, 512, 1024) for offset in (False, True)]
    return out


@pytest.mark.parametrize("C,rows,offset,shift", _gn_cases())
def test_groupnorm_fused_and_two_call_forms_against_fp64_reference(C, rows, offset, shift):
    """g3_groupnorm_swish_cl_bf16 and the pair g3_groupnorm_stats_cl_bf16 + g3_groupnorm_apply_cl_bf16, swish off and on, three frames.
    C / 8 = 2, 8, 24 (does not divide 256: gn_apply_generic_kernel), 64 and 128 chunks per row; 1 and 5 rows are fewer than the row step, 1000
    rows at C = 64 reach the four-rows-in-flight loop and its tail. Inputs N(0,1), or mean 6 / std 0.25 (E[x^2] - mean^2 loses 2.5 digits; fp32
    partial sums in gn_stats_kernel); beta is 0, or 9..12 in magnitude in the '-beta' cases (kr.groupnorm_operands says why nothing between).
    Statistics: |stat - ref| / (|ref| + 1) < 2e-6 against fp64 sums (also when ADDED to a buffer that held 3.5).
    Output: |out - ref| <= 1.0 bf16_ulp(ref) on every element - 0.5 for the rounding, 0.5 for fp32 arithmetic and the approximate rsqrt / exp2 /
    rcp - and the share of elements that differ from bf16(ref) at most ten times the share an fp32 restatement shows on the same input on the
    CPU (floor 1e-3). That restatement (kr.groupnorm_fp32) takes mean and variance from fp64 sums and subtracts the mean as two floats, as the
    kernels do: 0.50 ulp and a share <= 1e-4 on every input here. With both passes in fp32 it is 0.93 ulp off on the offset input at C = 1024
    and 15 ulp at C = 512, rows = 1000, where the frame's mean lies 6e-5 from a bf16 value many pixels take - the case that needs the mean
    kept as two floats in gn_apply_kernel / gn_apply_generic_kernel.
    Measured (profiles/tokenizer_kernel_parity_measured.txt): centred and -beta cases 0.50 ulp, share <= 3.5e-4, statistics 8.3e-8; the offset
    cases there are those of the one-float mean: 3.44 ulp at C = 512, rows = 1000, at most 0.93 elsewhere."""
    L, lib = _lib()
    frames = 3
    x, gamma, beta = kr.groupnorm_operands(C, frames, rows, offset, seed=C + rows, shift=shift)
    xin = Guarded(frames * rows, C, C + 8, data=x)
    g_d, b_d = gamma.to(_dev()), beta.to(_dev())
    _, stats_ref = kr.groupnorm_ref(x, gamma, beta, False)

    def check_stats(stats, start, what):
        e = float(((stats.cpu() - (stats_ref + start)).abs() / ((stats_ref + start).abs() + 1.0)).max())
        print(f"[groupnorm C={C} rows={rows} offset={offset} {what}] statistics rel err {e:.2e}")
        assert e < 2e-6, what

    for swish in (0, 1):
        ref, _ = kr.groupnorm_ref(x, gamma, beta, bool(swish))
        want = kr.bf16_round(ref)
        share_fp32 = float((kr.groupnorm_fp32(x, gamma, beta, bool(swish)) != want).double().mean())
        for form in ("fused", "pair"):
            out = Guarded(frames * rows, C, C + 16)
            stats = torch.full((frames, 2), float("nan") if form == "fused" else 0.0, dtype=torch.float64, device=_dev())  # the fused entry zeroes them itself
            if form == "fused":
                L.check(lib.g3_groupnorm_swish_cl_bf16(xin.ptr, C + 8, g_d.data_ptr(), b_d.data_ptr(), stats.data_ptr(), out.ptr, C + 16, frames, rows, C, 1e-6,
                                                       swish, _stream()), "g3_groupnorm_swish_cl_bf16")
            else:
                added = torch.full((frames, 2), 3.5, dtype=torch.float64, device=_dev())
                L.check(lib.g3_groupnorm_stats_cl_bf16(xin.ptr, C + 8, stats.data_ptr(), frames, rows, C, _stream()), "g3_groupnorm_stats_cl_bf16")
                L.check(lib.g3_groupnorm_stats_cl_bf16(xin.ptr, C + 8, added.data_ptr(), frames, rows, C, _stream()), "g3_groupnorm_stats_cl_bf16")
                L.check(lib.g3_groupnorm_apply_cl_bf16(xin.ptr, C + 8, g_d.data_ptr(), b_d.data_ptr(), stats.data_ptr(), out.ptr, C + 16, frames, rows, C, 1e-6,
                                                       swish, _stream()), "g3_groupnorm_apply_cl_bf16")
                torch.cuda.synchronize()
                check_stats(added, 3.5, "pair, added to 3.5")
            torch.cuda.synchronize()
            what = f"{form} swish={swish}"
            out.assert_only_payload_written(f"groupnorm {what}")
            check_stats(stats, 0.0, what)
            got = out.cpu().reshape(frames, rows, C)
            ulps = float(kr.ulp_error(got, ref).max())
            share = float((got != want).double().mean())
            print(f"[groupnorm C={C} rows={rows} offset={offset} beta={shift} {what}] max {ulps:.3f} ulp, share != bf16(ref) {share:.2e} (fp32 restatement {share_fp32:.2e})")
            assert ulps <= 1.0, what
            assert share <= max(10 * share_fp32, 1e-3), what


# =================================================================================================================================
# resampling
# =================================================================================================================================
def _run_resample(x, mode):
    L, lib = _lib()
    T, H, W, C = x.shape
    To, Ho, Wo = kr.resample_out_shape(mode, T, H, W)
    xin = Guarded(T * H * W, C, data=x)
    out = Guarded(To * Ho * Wo, C)
    L.check(lib.g3_resample_cl_bf16(xin.ptr, out.ptr, T, H, W, C, mode, _stream()), "g3_resample_cl_bf16")
    torch.cuda.synchronize()
    out.assert_only_payload_written(f"resample mode {mode}")
    return out


@pytest.mark.parametrize("C", kr.RESAMPLE_CHANNELS)
@pytest.mark.parametrize("mode,T,H,W", kr.RESAMPLE_CASES)
def test_resample_modes_against_the_reference_lines(mode, T, H, W, C):
    """Modes 2 and 3 copy: bitwise equal to the torch index expression. Modes 0 and 1 average up to four bf16 values - exact in fp32 - so the
    correctly rounded fp64 reference is the only right answer: no element may differ (the CPU test holds the fp32 restatement to the same 0
    mismatches on these very inputs). Odd H / W (zero column and row), a single pixel, T = 1 (both temporal modes) are in kr.RESAMPLE_CASES."""
    x = kr.resample_input(mode, T, H, W, C)
    got = _run_resample(x, mode).cpu().reshape(*kr.resample_out_shape(mode, T, H, W), C)
    if mode >= 2:
        assert torch.equal(got, kr.resample_ref(mode, x, dtype=bf16))
        return
    ref = kr.resample_ref(mode, x)
    ulps = float(kr.ulp_error(got, ref).max())
    mismatches = int((got != kr.bf16_round(ref)).sum())
    print(f"[resample mode {mode} ({T},{H},{W}) C={C}] max {ulps:.3f} ulp, {mismatches} elements != bf16(ref)")
    assert ulps <= 1.0 and mismatches == 0


def test_resample_grid_stride_loop_beyond_the_grid_cap():
    """Mode 3 on (2, 96, 128, 512): 6.3 M 16-byte chunks of output against the 8192 x 256 threads the grid is capped at - every thread goes
    round its loop three times. Bitwise against the index expression (evaluated on the device: 100 MB of output)."""
    x = kr.randn_bf16((2, 96, 128, 512), seed=96)
    out = _run_resample(x, 3)
    want = x.to(_dev()).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).reshape(-1, 512)
    assert out.rows * (512 // 8) > 8192 * 256
    assert torch.equal(out.payload, want)


# =================================================================================================================================
# Haar patcher / unpatcher
# =================================================================================================================================
class GuardedFlat(Guarded):
    """a contiguous tensor of n elements between two NaN guards (rows of one element would waste the allocator): n x 1 with 4096 guard 'rows'"""

    def __init__(self, n, data=None):
        super().__init__(n, 1, 1, guard=4096, data=data)


def _run_patch(video):
    L, lib = _lib()
    _, T, H, W = video.shape
    rows = (T + 3) // 4 * (H // 4) * (W // 4)
    vin = GuardedFlat(video.numel(), data=video)
    out = Guarded(rows, 192)
    L.check(lib.g3_haar3d_patch_bf16(vin.ptr, out.ptr, T, H, W, _stream()), "g3_haar3d_patch_bf16")
    torch.cuda.synchronize()
    out.assert_only_payload_written("haar patch")
    return out


def _run_unpatch(coef, ld, base_offset=0):
    """coef [Tp][Hp][Wp][192] (CPU); the device copy has leading dimension ld and starts base_offset elements into its buffer."""
    L, lib = _lib()
    Tp, Hp, Wp, _ = coef.shape
    rows = Tp * Hp * Wp
    cin = torch.full((GUARD * ld + base_offset + rows * ld + GUARD * ld,), float("nan"), dtype=bf16, device=_dev())
    start = GUARD * ld + base_offset
    cin[start:start + rows * ld].view(rows, ld)[:, :192] = coef.reshape(rows, 192).to(_dev())
    Tout = 4 * Tp - 3
    vid = GuardedFlat(3 * Tout * 16 * Hp * Wp)
    L.check(lib.g3_haar3d_unpatch_bf16(cin.data_ptr() + 2 * start, ld, vid.ptr, Tp, Hp, Wp, _stream()), "g3_haar3d_unpatch_bf16")
    torch.cuda.synchronize()
    vid.assert_only_payload_written("haar unpatch")
    return vid.cpu().reshape(3, Tout, 4 * Hp, 4 * Wp)


_UNPATCH_LAYOUTS = [(192, 0), (200, 0), (196, 0), (192, 4)]  # (ld, base offset in elements): vector loads; vector loads, padded rows; scalar loads (ld % 8); scalar loads (base 8 bytes off)


@pytest.mark.parametrize("T,H,W", [(1, 4, 4), (5, 20, 28), (9, 36, 44)])
def test_haar_patch_unpatch_against_fp64_oracle(T, H, W):
    """Patcher3D / UnPatcher3D on uniform [-1, 1] video: 1 row; 70 rows; 297 rows = two whole 128-row blocks and a ragged one of 41. The inverse
    on every coefficient layout (_UNPATCH_LAYOUTS: both the 16-byte and the scalar load path), Tp = 1, 2, 3 -> 4 Tp - 3 frames.
    Each direction within 1.0 bf16_ulp(ref) of the fp64 oracle evaluated on the very bf16 values the kernel read; measured 0.50 / 0.50.
    Round trip: every direction rounds once, so unpatch(patch(x)) is x up to 2 bf16 ulp - of the video's range, 2 x 2^-8: counted in ulps of each
    pixel's own magnitude no implementation can keep that (a pixel of 1e-3 is rebuilt from 64 coefficients rounded at the size of the block's
    mean: the fp64 oracle with one correct rounding per direction is itself up to 9.5e3 ulp(x) off there, and 1.0 x 2^-8 at worst). Measured 1.0."""
    video = kr.uniform_bf16((3, T, H, W), seed=T + H + W)
    Tp, Hp, Wp = (T + 3) // 4, H // 4, W // 4
    out = _run_patch(video)
    coef = out.cpu().reshape(Tp, Hp, Wp, 192)
    e_patch = float(kr.ulp_error(coef, kr.haar_patch_ref(video)).max())
    print(f"[haar patch ({T},{H},{W})] {out.rows} rows, max {e_patch:.3f} ulp")
    assert e_patch <= 1.0
    ref_back = kr.haar_unpatch_ref(coef)
    assert tuple(ref_back.shape) == (3, 4 * Tp - 3, H, W) and 4 * Tp - 3 == T
    backs = []
    for ld, off in _UNPATCH_LAYOUTS:
        back = _run_unpatch(coef, ld, off)
        e_un = float(kr.ulp_error(back, ref_back).max())
        e_rt = float((back.double() - video.double()).abs().max() / 2.0 ** -8)
        print(f"[haar unpatch ({T},{H},{W}) ld={ld} base+{off}] max {e_un:.3f} ulp; round trip {e_rt:.3f} x 2^-8")
        assert e_un <= 1.0 and e_rt <= 2.0
        backs.append(back)
    assert all(torch.equal(backs[0], b) for b in backs[1:]), "the load paths of haar_unpatch_kernel disagree"


# =================================================================================================================================
# transpose
# =================================================================================================================================
@pytest.mark.parametrize("R,C", [(1, 1), (64, 64), (65, 130), (300, 77)])
def test_transpose2d_bitwise(R, C):
    L, lib = _lib()
    x = kr.randn_bf16((R, C), seed=R + C)
    xin, out = Guarded(R, C, C + 3, data=x), Guarded(C, R, R + 5)
    L.check(lib.g3_transpose2d_bf16(xin.ptr, C + 3, out.ptr, R + 5, R, C, _stream()), "g3_transpose2d_bf16")
    torch.cuda.synchronize()
    out.assert_only_payload_written("transpose2d")
    assert torch.equal(out.cpu(), x.t())


# =================================================================================================================================
# refusals
# =================================================================================================================================
def test_documented_refusals_name_their_entry_and_launch_nothing():
    L, lib = _lib()
    a, b = Guarded(256, 64), Guarded(256, 64)  # operands large enough for every shape named below
    vec = torch.zeros(64, dtype=bf16, device=_dev())
    st = torch.zeros(16, 2, dtype=torch.float64, device=_dev())
    s = _stream()
    calls = [
        ("g3_groupnorm_swish_cl_bf16", lambda: lib.g3_groupnorm_swish_cl_bf16(a.ptr, 16, vec.data_ptr(), vec.data_ptr(), st.data_ptr(), b.ptr, 16, 2, 4, 12, 1e-6, 1, s)),
        ("g3_groupnorm_stats_cl_bf16", lambda: lib.g3_groupnorm_stats_cl_bf16(a.ptr, 16, st.data_ptr(), 2, 4, 12, s)),
        ("g3_groupnorm_apply_cl_bf16", lambda: lib.g3_groupnorm_apply_cl_bf16(a.ptr, 16, vec.data_ptr(), vec.data_ptr(), st.data_ptr(), b.ptr, 16, 2, 4, 12, 1e-6, 0, s)),
        ("g3_resample_cl_bf16", lambda: lib.g3_resample_cl_bf16(a.ptr, b.ptr, 2, 3, 4, 12, 0, s)),                 # C % 8
        ("g3_resample_cl_bf16", lambda: lib.g3_resample_cl_bf16(a.ptr, b.ptr, 2, 3, 4, 8, 4, s)),                  # unknown mode
        ("g3_haar3d_patch_bf16", lambda: lib.g3_haar3d_patch_bf16(a.ptr, b.ptr, 1, 6, 8, s)),                      # H % 4
        ("g3_conv3d_cl_bf16", lambda: lib.g3_conv3d_cl_bf16(a.ptr, 12, a.ptr, 12, None, None, 0, b.ptr, 16, 12, 16, 1, 2, 2, 1, 2, 2, *_GEOM["p1"], s)),  # K % 8
        ("g3_conv3d_cl_gnstats_bf16", lambda: lib.g3_conv3d_cl_gnstats_bf16(a.ptr, 16, a.ptr, 16, None, None, 0, b.ptr, 16, 16, 16, 2, 3, 3, 2, 3, 3, *_GEOM["p1"],
                                                                            st.data_ptr(), 7, s)),                # 7 does not divide 18 rows
    ]
    for entry, call in calls:
        rc = call()
        assert rc != 0, entry
        _err_names(entry)
    torch.cuda.synchronize()
    st_cpu = st.cpu()
    assert bool(torch.isnan(b.buf.float()).all()) and bool((st_cpu == 0).all()), "a refused call wrote output"
