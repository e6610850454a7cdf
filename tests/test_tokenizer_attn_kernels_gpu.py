"""GPU: the tokenizer's three attention entries against exact fp64 probes, element by element - g3_spatial_attn_d512_bf16
(csrc/attention_d512.hip), g3_temporal_attn_cl_bf16 and g3_softmax_rows_bf16 (csrc/tokenizer.hip), and the score-matrix fallback of
CausalVideoTokenizerNet._spatial_attn at HW % 8 != 0. Probes, references, restatements and bars: tests/tokenizer_attn_ref.py; their own checks
and the proof that every listed defect is caught: tests/test_tokenizer_attn_ref_cpu.py. tests/test_tokenizer_gpu.py keeps its aggregate rel-L2 bars.

Every input is a bf16 tensor built on the CPU from a seeded generator and feeds kernel and reference alike; every output is a NaN-guarded payload
(tests/guarded.py) checked with assert_only_payload_written; every element is checked, no outliers on the probes.

d = 512 kernel, through the C ABI. Q and K are NaN-guarded payloads (guard rows directly behind the last row of the last frame), V^T in the
network's layout ([512][frames * hw], ld_vt = frames * hw, vt_frame = hw) and in a per-frame layout (ld_vt = hw + 8, vt_frame = 512 ld_vt, NaN in
the 8 padding columns). Bars, those of tests/attn_probe_ref.py:
 * census, uniform and threshold probes - P is exactly 1 or a power of two, only the output rounding is left: |out - ref| <= 2^-8 ref where
   ref >= 2^-20, |out| <= 2^-18 elsewhere;
 * the staircases, the mixed rows and everything at the default scale 512^-0.5: 2^-7 (bf16 rounds P and the output, 2^-9 each of the binade's
   upper end; the factor 2 covers the hardware exp2 and reciprocal). All 64 keys of a tile share one P, so its rounding does not average out
   inside a column - as at d = 128, where the CPU emulation reaches 6.5e-3 of the 7.8e-3; at d = 512 the emulation's worst staircase figure over
   every shape run here is 2.5e-3 (the reference point follows the staircase, P stays within 2^+-8 of 1), asserted on the CPU: the bar carries over;
 * Gaussian operands (the recipe of tests/test_tokenizer_gpu.py, dominant keys included) at the default scale, every element against the fp64
   softmax: |out - ref| <= 0.5 bf16_ulp(ref) + C_GAUSS E, E = 2^-9 sum_j p_j |v_j|. C_GAUSS = 4: twice the emulation's worst
   (err - 0.5 ulp) / E on these very inputs, 1.105, rounded up to a power of two (re-derived and asserted by the CPU test).

Temporal attention: both kernels where both apply (option tok_tattn_px 1 and 0; T <= 16, C <= 512, 16-byte aligned operands), bitwise equal, each
against the reference's dtype chain in fp64. Probes (exact integer scores): every element within 0.5 bf16 ulp + 2^-16 |ref|, the causality columns
bitwise +0. Gaussian operands: the same bar, except on a share of elements at most min(10 x the fp32 restatement's share on the same inputs, 1e-3),
each of them within what ONE score rounded to the other bf16 neighbour can move it by (tokenizer_attn_ref.temporal_flip_allowance). The
restatement (temporal_fp32) sums in the kernels' order from elementwise fp32 operations, so its share is the same on every host.
The misaligned case offsets every operand by 4 elements: 8 bytes. (8 elements are 16 bytes - a pointer that far from a 16-byte boundary is on the
next one, and the one-wave-per-pixel kernel would run.)

Row softmax: both paths, |out - ref| <= 0.5 ulp + 2^-16 ref against softmax(bf16 x * fp32 scale) in fp64, an -inf entry exactly 0, row sums of the
bf16 output within n 2^-9 max p of 1, padding columns and guard rows bitwise untouched. Which path a case takes is not observable in the result
(both meet the same bar; they differ in the order of an fp32 sum); every case names the path the launcher's rule sends it to. (The row-sum
bound is the stated one; a correctly rounded row of equal values can exceed it - 0.5 ulp reaches 2^-8 relative at the low end of a binade, n = 104
does - but none of the sizes here.)

The fallback seam: _spatial_attn with the flash switch off at HW = 35 (ldp = 40: the softmax streams over a strided row) and HW = 72, against the
fp64 chain (scores rounded to bf16, softmax, P rounded to bf16, P.V) on the q / k / v the HIP path itself produced; with the switch on the result
must be bitwise the same (C = 512 with HW % 64 != 0 never reaches the flash kernel).

No defect was found in the three kernels. The seam test found one in the fallback: at HW % 4 != 0 the scores GEMM refused N = HW (it stores 4
columns at a time) and _spatial_attn raised; gen3c_amd/tokenizer.py now takes the scores against k padded with zero rows to the next multiple of 4
(test_spatial_attn_fallback_seam). Measured on an MI355X (the tests print these per case; profiles/tokenizer_attn_parity_measured.txt):
MEASURED below."""
import functools
import math

import pytest
import torch

from tests import tokenizer_attn_ref as A
from tests.guarded import Guarded
from tests.tokenizer_kernel_ref import bf16_round, bf16_ulp

pytestmark = pytest.mark.gpu

# Largest figures over all cases of a family on an MI355X.
MEASURED = {
    "d512 probes at 2^-5 / log2 e, P exact (bar 2^-8): relative element error": 3.323e-03,
    "d512 staircases and mixed rows (bar 2^-7): relative element error": 2.505e-03,
    "d512 default scale (bar 2^-7): relative element error": 2.492e-03,
    "d512 Gaussian: (err - 0.5 ulp) / E of the kernel, of the emulation (C_GAUSS = 4)": (1.1047, 1.1047),
    "temporal probes: (err - 0.5 ulp) / |ref| (bar 2^-16 = 1.53e-5)": 0.0,
    "temporal Gaussian: share outside the bar, kernel / fp32 restatement": (4.492e-05, 4.492e-05),
    "row softmax: worst error in bf16 ulp of the reference; (err - 0.5 ulp) / ref (bar 2^-16)": (0.5001, 7.423e-07),
    "fallback seam: attention branch rel-L2 vs the fp64 chain, kernel / fp32 restatement": {35: (2.351e-03, 1.737e-03), 72: (2.352e-03, 1.749e-03)},
}

bf16 = torch.bfloat16
NAN_BITS = torch.full((1,), float("nan"), dtype=bf16).view(torch.int16).item()


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _untouched(g):
    return bool((g.buf.view(torch.int16) == NAN_BITS).all())


# ---- 1. the d = 512 kernel -----------------------------------------------------------------------------------------------------------------------------------

class Case512:
    """device operands of one probe, built once and never written"""

    def __init__(self, p, softmax_scale):
        self.p, self.F, self.hw = p, p.F, p.hw
        n = p.F * p.hw
        self.q = Guarded(n, A.D, data=p.q.reshape(n, A.D).to(bf16))
        self.k = Guarded(n, A.D, data=p.k.reshape(n, A.D).to(bf16))
        v = p.v.to(bf16).to(_dev())
        self.vt_net = v.reshape(n, A.D).t().contiguous()  # [512][F hw]
        self.vt_frame = torch.full((p.F, A.D, p.hw + 8), float("nan"), dtype=bf16, device=_dev())
        self.vt_frame[:, :, :p.hw] = v.transpose(1, 2)
        self.ref = A.reference(p, softmax_scale)

    def launch(self, layout, softmax_scale):
        """-> the Guarded output"""
        from gen3c_amd import _lib
        o = Guarded(self.F * self.hw, A.D)
        if layout == "net":
            vt, ld, fs = self.vt_net, self.F * self.hw, self.hw
        else:
            vt, ld, fs = self.vt_frame, self.hw + 8, A.D * (self.hw + 8)
        _lib.check(_lib.load().g3_spatial_attn_d512_bf16(self.q.ptr, self.k.ptr, vt.data_ptr(), ld, fs, o.ptr, self.F, self.hw, softmax_scale, _stream()),
                   "g3_spatial_attn_d512_bf16")
        torch.cuda.synchronize()
        return o

    def out(self, o):
        return o.payload.float().cpu().view(self.F, self.hw, A.D)


LAYOUTS = ("net", "per-frame")


@functools.lru_cache(maxsize=None)
def _case512(kind, F, hw, default_scale=False):
    if default_scale:
        return Case512(A.make(kind, F, hw, A.fp32_scale_log2(A.DEFAULT_SCALE_512)), A.DEFAULT_SCALE_512)
    return Case512(A.make(kind, F, hw), A.SOFTMAX_SCALE_512)


def _run_probes(F, hw, kinds, default_scale):
    scale = A.DEFAULT_SCALE_512 if default_scale else A.SOFTMAX_SCALE_512
    worst, fails = {}, []
    for kind in kinds:
        c = _case512(kind, F, hw, default_scale)
        rel = A.REL_BF16 if default_scale else c.p.rel
        for layout in LAYOUTS:
            tag = f"d512 {c.p.name} frames={F} hw={hw} V^T {layout}{' default scale' if default_scale else ''}"
            o = c.launch(layout, scale)
            o.assert_only_payload_written(tag)
            for g in (c.q, c.k):
                g.assert_only_payload_written(tag + " (an input)")
            out = c.out(o)
            ok, relmax, _small = A.out_errors(out, c.ref, rel)
            worst[rel] = max(worst.get(rel, 0.0), relmax)
            if not ok:
                fails.append(f"{tag}: bar {rel:.3e}, worst relative error {relmax:.3e}; {A.first_bad512(out, c.ref, rel)}")
    print(f"[tok attn d512{' default scale' if default_scale else ''}] frames={F} hw={hw}: {len(kinds)} probes x 2 layouts, worst relative element error per bar "
          + ", ".join(f"{b:.3e}: {w:.3e}" for b, w in sorted(worst.items())))
    assert not fails, f"{len(fails)} checks failed:\n" + "\n".join(fails)


@pytest.mark.parametrize("F,hw,kinds", A.PLAN_512, ids=[f"{F}x{hw}" for F, hw, _ in A.PLAN_512])
def test_d512_probes(F, hw, kinds):
    """frames % 8 == 0 takes the frame-per-XCD workgroup mapping (8: one frame per XCD, 16: two); hw = 64 has one tile and no next-K fetch; 192, 320
    and 448 end in a half-empty query block; 1088 has 17 tiles. The mixed-rows staircases make rows of one 32-row group, and 32-row groups of one
    128-row block, move their reference point in different tiles (asserted on the emulation's trace by the CPU test)."""
    _run_probes(F, hw, kinds, False)


@pytest.mark.parametrize("F,hw,kinds", A.PLAN_512_DEFAULT_SCALE, ids=[f"{F}x{hw}" for F, hw, _ in A.PLAN_512_DEFAULT_SCALE])
def test_d512_probes_at_the_default_scale(F, hw, kinds):
    """The kernel applies the scale in fp32 behind the MFMA, so at 512^-0.5 the probes keep their closed forms (a match scores 65.3, the staircase's
    s_j is rounded to bf16 and the reference uses the rounded value)."""
    _run_probes(F, hw, kinds, True)


@pytest.mark.parametrize("F,hw", A.GAUSS_SHAPES)
def test_d512_gaussian_every_element(F, hw):
    p = A.gaussian(F, hw)
    c = Case512(p, A.DEFAULT_SCALE_512)
    ref, absum = A.reference(p, A.DEFAULT_SCALE_512, with_abs=True)
    emu = A.gauss_excess(A.emulate(p, softmax_scale=A.DEFAULT_SCALE_512), ref, absum)
    sc = torch.einsum("id,jd->ij", p.q[0], p.k[0]) * A.DEFAULT_SCALE_512
    worst = -math.inf
    for layout in LAYOUTS:
        tag = f"d512 gaussian frames={F} hw={hw} V^T {layout}"
        o = c.launch(layout, A.DEFAULT_SCALE_512)
        o.assert_only_payload_written(tag)
        worst = max(worst, A.gauss_excess(c.out(o), ref, absum))
    print(f"[tok attn d512 gaussian] frames={F} hw={hw} (score std {float(sc.std()):.2f}): worst (err - 0.5 ulp) / E kernel {worst:.4f}, emulation {emu:.4f}, "
          f"C_GAUSS {A.C_GAUSS:g}")
    assert emu <= A.C_GAUSS / 2
    assert worst <= A.C_GAUSS, f"(err - 0.5 ulp) / E = {worst} > {A.C_GAUSS}"


def test_d512_refusals():
    """every refused call returns G3_ERR_ARG, names the entry in g3_last_error and leaves the guarded output untouched"""
    from gen3c_amd import _lib
    lib = _lib.load()
    c = _case512("census-position", 1, 64)
    q, k, vt, hw = c.q.ptr, c.k.ptr, c.vt_net.data_ptr(), 64
    o = Guarded(hw, A.D)
    calls = {
        "hw % 64 != 0": (q, k, vt, 96, 96, o.ptr, 1, 96),
        "ld_vt < hw": (q, k, vt, 56, 56, o.ptr, 1, hw),
        "ld_vt % 8": (q, k, vt, hw + 4, hw + 4, o.ptr, 1, hw),
        "vt_frame % 8": (q, k, vt, hw, hw + 4, o.ptr, 1, hw),
        "null q": (None, k, vt, hw, hw, o.ptr, 1, hw),
        "null k": (q, None, vt, hw, hw, o.ptr, 1, hw),
        "null vt": (q, k, None, hw, hw, o.ptr, 1, hw),
        "null o": (q, k, vt, hw, hw, None, 1, hw),
        "frames = 0": (q, k, vt, hw, hw, o.ptr, 0, hw),
        "frames < 0": (q, k, vt, hw, hw, o.ptr, -1, hw),
        "8 * ld_vt * 2 >= 2^32": (q, k, vt, 1 << 28, hw, o.ptr, 1, hw),
    }
    for what, a in calls.items():
        rc = lib.g3_spatial_attn_d512_bf16(*a, A.SOFTMAX_SCALE_512, _stream())
        torch.cuda.synchronize()
        assert rc == _lib.G3_ERR_ARG, (what, rc)
        assert "g3_spatial_attn_d512_bf16" in _lib.last_error(), (what, _lib.last_error())
        assert _untouched(o), f"{what}: the refused call wrote to the output"
    # ... and the same operands are accepted once the arguments are right
    _lib.check(lib.g3_spatial_attn_d512_bf16(q, k, vt, hw, hw, o.ptr, 1, hw, A.SOFTMAX_SCALE_512, _stream()), "g3_spatial_attn_d512_bf16")
    torch.cuda.synchronize()
    o.assert_only_payload_written("d512 after the refusals")


# ---- 2. temporal attention -----------------------------------------------------------------------------------------------------------------------------------

def _offset(x, off):
    """x [T, HW, C] fp64 -> a bf16 device tensor whose storage begins `off` elements into an allocation"""
    buf = torch.full((x.numel() + off + 8,), float("nan"), dtype=bf16, device=_dev())
    view = buf[off:off + x.numel()].view(x.shape)
    view.copy_(x.to(bf16))
    return view


def _assert_flat_written(g, start, numel, what):
    """the output began `start` elements into the Guarded payload: exactly [start, start + numel) of it was written"""
    flat = g.buf.view(-1).view(torch.int16)
    lo = g.guard * g.ld + start
    outside = torch.ones_like(flat, dtype=torch.bool)
    outside[lo:lo + numel] = False
    touched = int((flat[outside] != NAN_BITS).sum())
    assert touched == 0, f"{what}: {touched} elements outside the output were written"
    assert bool(torch.isfinite(g.buf.view(-1)[lo:lo + numel].float()).all()), f"{what}: non-finite values in the output"


def _temporal_launch(q, k, v, T, HW, C, scale, px, off=0):
    """-> the output [T, HW, C] bf16 on the CPU, from a guarded buffer (off: elements the output pointer is offset by)"""
    from gen3c_amd import _lib, ops
    g = Guarded(T * HW + (1 if off else 0), C)
    ops.set_option("tok_tattn_px", px)
    try:
        _lib.check(_lib.load().g3_temporal_attn_cl_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), g.ptr_at(off), T, HW, C, scale, _stream()), "g3_temporal_attn_cl_bf16")
        torch.cuda.synchronize()
    finally:
        ops.set_option("tok_tattn_px", 1)
    what = f"temporal T={T} HW={HW} C={C} px={px} offset {off}"
    if off:
        _assert_flat_written(g, off, T * HW * C, what)
        return g.buf[g.guard:].reshape(-1)[off:off + T * HW * C].view(T, HW, C).cpu()
    g.assert_only_payload_written(what)
    return g.payload.view(T, HW, C).cpu()


def _temporal_probe_case(T, HW, C, off):
    worst = -math.inf
    for scale in A.temporal_scales(C):
        for kind in A.TEMPORAL_KINDS:
            q, k, v = A.temporal_probe(kind, T, HW, C)
            ref = A.temporal_reference(q, k, v, scale)
            dq, dk, dv = (_offset(x, off) for x in (q, k, v))
            outs = [_temporal_launch(dq, dk, dv, T, HW, C, scale, px, off) for px in (1, 0)]
            tag = f"temporal {kind} T={T} HW={HW} C={C} scale {scale:.4g} offset {off}"
            assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{tag}: tok_tattn_px 1 and 0 differ"
            if off:  # the fallback agrees with the aligned launch of the same values, bit for bit
                aligned = _temporal_launch(*(_offset(x, 0) for x in (q, k, v)), T, HW, C, scale, 0)
                assert torch.equal(outs[0].view(torch.int16), aligned.view(torch.int16)), f"{tag}: differs from the aligned launch"
            o = outs[0].double()
            err = (o - ref).abs()
            bad = ~(err <= A.temporal_bar(ref))
            assert not bool(bad.any()), f"{tag}: {int(bad.sum())} elements outside 0.5 ulp + 2^-16 |ref|, first {tuple(int(i) for i in bad.nonzero()[0])}"
            nz = ref != 0
            worst = max(worst, float(((err - 0.5 * bf16_ulp(ref))[nz] / ref[nz].abs()).max()))
            if kind == "causality":
                future = (torch.arange(C)[None, :] > torch.arange(T)[:, None])[:, None, :].expand(T, HW, C)
                assert bool((outs[0].view(torch.int16)[future] == 0).all()), f"{tag}: a future frame's column is not bitwise +0"
    print(f"[tok attn temporal probes] T={T} HW={HW} C={C} offset {off}: both kernels{'' if A.px_applies(T, C) and not off else ' (one form serves both options)'}, "
          f"worst (err - 0.5 ulp) / |ref| = {worst:.3e} (bar {A.U16:.3e})")


@pytest.mark.parametrize("T,HW,C", A.TEMPORAL_SHAPES)
def test_temporal_probes(T, HW, C):
    """(5, 9, 520) and (3, 6, 1024): C > 512, a lane loops twice; T = 17, 33, 64: beyond the per-pixel kernel - the first form alone serves these,
    under either option. HW values that are no multiple of 4 leave a ragged last workgroup."""
    _temporal_probe_case(T, HW, C, 0)


def test_temporal_misaligned_operands_fall_back_and_agree():
    """(16, 6, 512) with q, k, v and o 8 bytes off a 16-byte boundary: the launcher must take the first form under either option; the results are
    bitwise those of the aligned launch."""
    _temporal_probe_case(16, 6, 512, 4)


def test_temporal_gaussian():
    T, HW, C = A.TEMPORAL_GAUSS
    q, k, v = A.temporal_gaussian(T, HW, C)
    scale = float(C) ** -0.5
    ref, absum, s, _w = A.temporal_reference(q, k, v, scale, detail=True)
    share_r, ok_r = A.temporal_outliers(A.temporal_fp32(q, k, v, scale), ref, absum, s, scale)
    dq, dk, dv = (_offset(x, 0) for x in (q, k, v))
    outs = [_temporal_launch(dq, dk, dv, T, HW, C, scale, px) for px in (1, 0)]
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "tok_tattn_px 1 and 0 differ"
    share, ok = A.temporal_outliers(outs[0], ref, absum, s, scale)
    print(f"[tok attn temporal gaussian] T={T} HW={HW} C={C}: share of elements outside 0.5 ulp + 2^-16 |ref|: kernel {share:.3e}, fp32 restatement {share_r:.3e}")
    assert ok_r and ok, "an element outside the bar is further off than one score's rounding to the other bf16 neighbour explains"
    assert share <= min(10 * share_r, 1e-3), f"share {share} > min(10 x {share_r}, 1e-3)"


def test_temporal_refusals():
    from gen3c_amd import _lib
    lib = _lib.load()
    x = torch.zeros(65 * 2 * 16, dtype=bf16, device=_dev())
    o = Guarded(65 * 2, 16)
    for what, (T, HW, C) in {"T = 65": (65, 2, 16), "C % 8 != 0": (2, 2, 12)}.items():
        rc = lib.g3_temporal_attn_cl_bf16(x.data_ptr(), x.data_ptr(), x.data_ptr(), o.ptr, T, HW, C, 0.25, _stream())
        torch.cuda.synchronize()
        assert rc == _lib.G3_ERR_ARG and "g3_temporal_attn_cl_bf16" in _lib.last_error(), (what, rc, _lib.last_error())
        assert _untouched(o), f"{what}: the refused call wrote to the output"


# ---- 3. row softmax ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(A.SOFTMAX_CASES)), ids=["{}x{}_ld{}_off{}".format(*c) for c in A.SOFTMAX_CASES])
def test_softmax_rows(i):
    from gen3c_amd import _lib
    rows, n, ld, off = A.SOFTMAX_CASES[i]
    x, names = A.softmax_rows_input(rows, n, first=i)
    ref = A.softmax_reference(x, A.SOFTMAX_SCALE_ROWS)
    g = Guarded(rows, off + n, ld=ld, data=torch.cat([torch.full((rows, off), 1.5, dtype=bf16), x], dim=1))
    ptr = g.ptr_at(off)
    path = "register" if A.softmax_reg_path(n, ld, ptr) else "streaming"
    assert (path == "register") == (n <= 16384 and n % 8 == 0 and ld % 8 == 0 and off == 0), "the case is meant for the other path"
    _lib.check(_lib.load().g3_softmax_rows_bf16(ptr, ld, rows, n, A.SOFTMAX_SCALE_ROWS, _stream()), "g3_softmax_rows_bf16")
    torch.cuda.synchronize()
    tag = f"softmax rows={rows} n={n} ld={ld} offset {off} ({path} path)"
    g.assert_only_payload_written(tag)
    got = g.payload.cpu()
    assert bool((got[:, :off] == 1.5).all()), f"{tag}: the columns in front of the base were written"
    out = got[:, off:].double()
    err = (out - ref).abs()
    bad = ~(err <= A.softmax_bar(ref))
    ulps = float((err / bf16_ulp(ref)).max())
    pos = ref > 0
    excess = float(((err - 0.5 * bf16_ulp(ref))[pos] / ref[pos]).max())
    sums = (out.sum(-1) - 1).abs()
    print(f"[tok attn softmax] {tag}, rows {names}: worst error {ulps:.4f} ulp, (err - 0.5 ulp) / ref {excess:.3e} (bar {A.U16:.3e}), |row sum - 1| {float(sums.max()):.3e}")
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} elements outside 0.5 ulp + 2^-16 ref, first {tuple(int(j) for j in bad.nonzero()[0])}"
    assert bool((out[ref == 0] == 0).all()), f"{tag}: an -inf entry is not exactly 0"
    assert bool((sums <= n * 2.0 ** -9 * ref.max(dim=-1).values).all()), f"{tag}: a row sum is off by {float(sums.max())}"
    for r, name in enumerate(names):
        if name == "all-equal":
            assert bool((got[r, off:] == bf16_round(torch.tensor(1.0 / n, dtype=torch.float64))).all()), f"{tag}: an all-equal row is not bf16(1 / n) throughout"


# ---- 4. the fallback seam -------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net():
    from gen3c_amd.tokenizer import CausalVideoTokenizerNet
    net = CausalVideoTokenizerNet(channels=128, device=_dev())
    net.init_random(seed=9)
    for n in ("q", "k"):  # a realistic score spread (std ~2.5), as in tests/test_tokenizer_gpu.py
        key = f"encoder.mid.attn_1.0.{n}.conv3d.weight"
        net._w[key] = (net._w[key].float() * 1.6).to(bf16)
    return net


@pytest.mark.parametrize("T,H,W", [(3, 5, 7), (2, 9, 8)])
def test_spatial_attn_fallback_seam(T, H, W, monkeypatch):
    """scores GEMM -> g3_softmax_rows_bf16 -> P.V GEMM over the zero-padded ldp. HW = 35: ldp = 40, the softmax takes the streaming path over a
    strided row and the P.V GEMM runs over 5 zero columns; HW = 72: a multiple of 8, not of 64. The attention branch (output minus residual)
    against the fp64 chain pushed through the same projection; tolerance = 2 x the rel-L2 of the three-kernel chain restated in torch fp32.
    Found by this test, now fixed in gen3c_amd/tokenizer.py: at HW = 35 the scores GEMM refused N = 35 (N % 4 != 0) and _spatial_attn raised."""
    from gen3c_amd import tokenizer as tkmod
    net, name, C, HW = _net(), "encoder.mid.attn_1.0", 512, H * W
    # (x at 1/8: GroupNorm takes the scale out of the branch, and the rounding of branch + residual - common to kernels and restatement - stays small beside it)
    x = (0.125 * torch.randn(T, H, W, C, generator=torch.Generator().manual_seed(100 * T + HW))).to(bf16).to(_dev())
    monkeypatch.setattr(tkmod, "_FLASH_SPATIAL_ATTN", False)
    y = net._spatial_attn(x, name)
    net._pending_stats = None
    monkeypatch.setattr(tkmod, "_FLASH_SPATIAL_ATTN", True)
    y_on = net._spatial_attn(x, name)
    net._pending_stats = None
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y_on.view(torch.int16)), "C = 512 with HW % 64 != 0 must take the score-matrix path under either switch"
    hn = net._gn(x, f"{name}.norm", False)
    q, k, v = (net._conv(hn, f"{name}.{n}", "p1").view(T, HW, C).cpu() for n in ("q", "k", "v"))
    net._pending_stats = None
    scale = torch.tensor(float(C) ** -0.5, dtype=torch.float32)
    s = bf16_round(torch.einsum("fid,fjd->fij", q.double(), k.double())).double()
    o64 = bf16_round(torch.einsum("fij,fjd->fid", bf16_round(torch.softmax(s * float(scale), dim=-1)).double(), v.double()))
    s32 = torch.einsum("fid,fjd->fij", q.float(), k.float()).to(bf16).float()
    o32 = torch.einsum("fij,fjd->fid", torch.softmax(s32 * scale, dim=-1).to(bf16).float(), v.float()).to(bf16)
    proj = lambda o: net._conv(o.to(_dev()).view(T, H, W, C).contiguous(), f"{name}.proj_out", "p1").float().cpu()
    xf = x.float().cpu()
    b64 = proj(o64)
    b32 = (proj(o32) + xf).to(bf16).float() - xf  # the restated chain ends as the kernels' does: branch + residual, rounded to bf16
    net._pending_stats = None
    got = y.float().cpu() - xf
    rel = lambda a, b: float((a - b).norm() / b.norm())
    r, r32 = rel(got, b64), rel(b32, b64)
    print(f"[tok attn fallback seam] T={T} HW={HW} ldp={(HW + 7) // 8 * 8}: score std {float((s * float(scale)).std()):.2f}, attention branch rel-L2 vs the fp64 chain: "
          f"kernels {r:.3e}, fp32 restatement {r32:.3e}; |branch| / |x| = {float(b64.norm() / xf.norm()):.3f}")
    assert torch.isfinite(y.float()).all()
    assert r <= 2.0 * r32
