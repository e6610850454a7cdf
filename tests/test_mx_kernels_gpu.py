"""GPU: the MX quantisers and block-scaled GEMMs (gemm_mx.hip, mx_quant.hpp) code by code, scale by scale and k by k against fp64.

Probes, closed forms and bars: tests/mx_probe_ref.py (pinned by tests/test_mx_probe_ref_cpu.py, which also shows every modelled index defect
caught). Every GEMM operand is a strided view with hostile padding - e4m3 NaN codes (MXFP6: byte 0x1F) behind every row, scale byte 254 behind
every scale row, lda / ldw = row bytes + 16, ldas / ldws = K / 32 + 4 -, every bf16 output is a NaN-guarded payload (tests/guarded.py), every
MXFP8 output sits in a 0xAA-filled buffer, and the kernel name is asserted for every launch. What the tests print is the record
profiles/mx_parity_measured.txt."""
import math

import pytest
import torch

from tests import mx_probe_ref as R
from tests.guarded import Guarded
from tests.mxfp6_ref import quant_mxfp6_ref
from tests.mxfp8_ref import quant_mxfp8_ref

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
FMT = [R.FP8, R.FP6]
FMT_IDS = ["mxfp8", "mxfp6"]
PAD_SCALE = 254


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _lib():
    from gen3c_amd import _lib
    return _lib.load()


def _poisoned(fmt, codes, scales):
    """-> (operand view [R][row bytes], scale view [R][K / 32]) on the device inside padded allocations full of hostile bytes"""
    dev = _dev()
    Rr, K = codes.shape
    rb, nb = fmt.row_bytes(K), K // R.BLOCK
    q = torch.full((Rr, rb + 16), fmt.pad, dtype=torch.uint8, device=dev)
    s = torch.full((Rr, nb + 4), PAD_SCALE, dtype=torch.uint8, device=dev)
    q[:, :rb] = fmt.pack(codes).to(dev)
    s[:, :nb] = scales.to(dev)
    qv = q[:, :rb]
    return (qv.view(F8) if fmt is R.FP8 else qv), s[:, :nb]


def _guards_untouched(g, what):
    fill = torch.full((1,), float("nan"), dtype=torch.bfloat16, device=g.buf.device).view(torch.int16)
    outside = torch.ones_like(g.buf, dtype=torch.bool)
    outside[g.guard:g.guard + g.rows, :g.C] = False
    touched = int((g.buf.view(torch.int16)[outside] != fill).sum())
    assert touched == 0, f"{what}: {touched} elements of the guard rows / padding columns were written"


class Operands:
    """a probe's operands on the device, staged once for several launches"""

    def __init__(self, p):
        self.p, self.fmt = p, p.fmt
        self.M, self.N, self.K = p.shape
        self.a, self.as_ = _poisoned(p.fmt, p.ac, p.as_)
        self.w, self.ws = _poisoned(p.fmt, p.wc, p.ws)

    def gemm(self, epilogue=0, gate=None, residual=None, inplace=False, finite=True):
        """one launch into a guarded output -> the payload on the CPU (bf16). inplace: the output buffer holds the residual."""
        from gen3c_amd import ops
        lib = _lib()
        name_of = lib.g3_gemm_mxfp8_kernel_name if self.fmt is R.FP8 else lib.g3_gemm_mxfp6_kernel_name
        stem = "gemm_mxfp8_nt_kernel" if self.fmt is R.FP8 else "gemm_mxfp6_nt_kernel"
        assert name_of(self.M, self.N, self.K, epilogue) == b"%s<%d>" % (stem.encode(), epilogue)
        what = f"{self.p.name} epilogue {epilogue}"
        g = Guarded(self.M, self.N, ld=self.N + 64, data=residual if inplace else None)
        kw = {}
        if epilogue == R.EPI_GATED_RESIDUAL:
            kw = dict(gate=gate.to(_dev()), residual=g.payload if inplace else residual.to(_dev()))
        fn = ops.gemm_mxfp8_nt if self.fmt is R.FP8 else ops.gemm_mxfp6_nt
        fn(self.a, self.as_, self.w, self.ws, out=g.payload, epilogue=epilogue, **kw)
        torch.cuda.synchronize()
        _guards_untouched(g, what)
        if finite:
            assert bool(torch.isfinite(g.payload.float()).all()), f"{what}: non-finite values in the payload"
        return g.cpu()

    def gemm_mxout(self, epilogue=0):
        """the MXFP8-output entry into 0xAA-padded buffers -> (codes, scales) on the CPU"""
        from gen3c_amd import ops
        dev = _dev()
        assert self.fmt is R.FP8
        assert _lib().g3_gemm_mxfp8_mxout_kernel_name(self.M, self.N, self.K, epilogue) == b"gemm_mxfp8_nt_kernel<%d>" % (256 + epilogue)
        M, N = self.M, self.N
        qb = torch.full((M + 8, N + 64), 0xAA, dtype=torch.uint8, device=dev)
        sb = torch.full((M + 8, N // 32 + 4), 0xAA, dtype=torch.uint8, device=dev)
        ops.gemm_mxfp8_nt(self.a, self.as_, self.w, self.ws, epilogue=epilogue, out_mx=(qb[:M, :N].view(F8), sb[:M, :N // 32]))
        torch.cuda.synchronize()
        assert bool((qb[:M, N:] == 0xAA).all()) and bool((sb[:M, N // 32:] == 0xAA).all()) and bool((qb[M:] == 0xAA).all()) and bool((sb[M:] == 0xAA).all()), \
            f"{self.p.name}: the MXFP8 output wrote outside [M, N] / [M, N / 32]"
        return qb[:M, :N].cpu(), sb[:M, :N // 32].cpu()


def _assert_bits(p, out, held=None):
    got, want = R.canon_bits(out), p.expect_bits()
    if held is None:
        held = p.asserted if p.asserted is not None else torch.ones_like(got, dtype=torch.bool)
    bad = ((got != want) & held).nonzero()
    print(f"[{p.name}] {int(held.sum())} outputs held bitwise: {bad.shape[0]} differ")
    assert bad.shape[0] == 0, (f"{p.name}: {bad.shape[0]} of {int(held.sum())} outputs differ, first at {bad[:4].tolist()}: got "
                               f"{[hex(int(got[i, j])) for i, j in bad[:4].tolist()]} want {[hex(int(want[i, j])) for i, j in bad[:4].tolist()]}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. code census
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["a", "w"])
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_code_census(fmt, side):
    """every e4m3 / e2m3 code through the token operand and through the weight operand (the two MFMA operands decode separately): the decode
    table times the row's scale, bit for bit; the e4m3 NaN codes give NaN; -0 comes back as +0 (the sum of one -0 and 127 +0 products)"""
    p = R.census_codes(fmt, side)
    out = Operands(p).gemm(finite=False)
    _assert_bits(p, out)
    line = out[:, 0] if side == "a" else out[0, :]
    for c in fmt.nan_codes:
        assert bool(torch.isnan(line[c].float())), f"e4m3 NaN code {c:#x} in operand {side} came back as {float(line[c])}"
    assert int(R.bits_of(line)[fmt.neg_zero]) == 0x0000, "-0 code: the project's record says +0"
    assert int(torch.isnan(line.float()).sum()) == len(fmt.nan_codes) * (256 // fmt.ncodes if fmt.nan_codes else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. scale census
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_scale_census(fmt):
    """every pair of scale bytes: bitwise inside bf16's normal range; beyond it and for byte 0xFF the observation is printed (the record)"""
    p = R.scale_grid(fmt)
    out = Operands(p).gemm(finite=False)
    _assert_bits(p, out)
    o = out.double()
    m, n = torch.arange(256).view(-1, 1), torch.arange(256).view(1, -1)
    e = m + n - 254
    fin = (m != 255) & (n != 255)
    lo, hi, ff = fin & (e < -126), fin & (e > 127), ~fin
    exact = 1.5 * torch.pow(2.0, e.double())
    as_bf16 = R.bf16_round(exact).double()  # the subnormal (or zero) bf16 nearest to the exact product
    print(f"[scale census {fmt.name}] below 2^-126: {int(lo.sum())} pairs, {int((o[lo] == as_bf16[lo]).sum())} equal bf16_round(exact) "
          f"({int((o[lo] == 0).sum())} zero); above 2^127: {int(hi.sum())} pairs, {int(torch.isinf(o[hi]).sum())} +inf; "
          f"a 0xFF byte in either operand: {int(ff.sum())} pairs, {int(torch.isnan(o[ff]).sum())} NaN")


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. position census
# ---------------------------------------------------------------------------------------------------------------------------------------
POSITION_CASES = R.POSITION_CASES


@pytest.mark.parametrize("shape,mode", POSITION_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{m}" for s, m in POSITION_CASES])
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_position_census(fmt, shape, mode):
    """which k meets which k under which scale pair, with scale bytes 127 +- 40 on both operands; at K = 16384 a stale stage or scale dword in
    any of the 128 K tiles moves an output by a factor of up to 2^80"""
    p = R.census_position(fmt, shape, mode)
    _assert_bits(p, Operands(p).gemm())


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. dense exact, every epilogue
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in R.SHAPES])
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_dense_exact_every_epilogue(fmt, shape):
    p = R.dense_integers(fmt, shape)
    M, N, K = shape
    ops_ = Operands(p)
    y = ops_.gemm()
    _assert_bits(p, y)
    gate, res = R.epilogue_operands(M, N)
    # GELU on the Linear's rounded output: gemm_ref's bars for arbitrary pre-activations (most of these lie in the tails, where GELU is y or 0)
    act = ops_.gemm(R.EPI_GELU)
    R.check_sweep(f"{p.name} GELU", y, act)
    # gated residual: g y is exact in fp32 - one right answer; gate rows 1 and 2, out of place and in place
    for rows in (1, 2):
        want = R.gated_fp32(y, gate[:rows], res)
        for inplace in (False, True):
            got = ops_.gemm(R.EPI_GATED_RESIDUAL, gate=gate[:rows], residual=res, inplace=inplace)
            bad = int((R.bits_of(got) != R.bits_of(want)).sum())
            assert bad == 0, f"{p.name} gated residual, {rows} gate rows{', in place' if inplace else ''}: {bad} outputs differ"
    if fmt is R.FP8:  # the MXFP8-output form: the reference quantiser on what the bf16 entry stores
        for epi, stored in ((R.EPI_NONE, y), (R.EPI_GELU, act)):
            q, s = ops_.gemm_mxout(epi)
            wq, ws = R.mxout_expect(stored)
            assert torch.equal(s, ws), f"{p.name} MXFP8 output, epilogue {epi}: scale bytes differ"
            assert torch.equal(q, wq), f"{p.name} MXFP8 output, epilogue {epi}: e4m3 codes differ"


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. accumulation: measured, then pinned
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_matrix_core_alignment(fmt):
    """2^p + ones - 2^p: the largest p that still comes back exact, per arrival of the 2^p. A statement about the hardware that the Gaussian
    bar rests on (the core keeps about 2^-(that p) of the largest addend); asserted so that a change is loud."""
    got = {}
    for j, ones in enumerate((63, 32)):
        p = R.align_probe(fmt, ones)
        out = Operands(p).gemm()
        res = R.largest_exact_p(out, p)
        v, pp = R.align_p_of()
        first_bad = {}
        for i, name in enumerate(R.ALIGN_VARIANTS):
            sel = (v == i) & p.asserted & (pp == res[name] + 1)
            first_bad[name] = sorted(set(out.double()[sel].tolist()))[:4]
        print(f"[alignment {fmt.name}, 2^p beside {ones} ones] largest exact p: {res}; outputs at the first inexact p: {first_bad}")
        got[ones] = res
    for name in R.ALIGN_VARIANTS:
        assert (got[63][name], got[32][name]) == R.ALIGN_MEASURED[fmt.name][name], \
            f"{fmt.name} {name}: largest exact p {(got[63][name], got[32][name])}, the record says {R.ALIGN_MEASURED[fmt.name][name]}"


@pytest.mark.parametrize("shape", R.GAUSS_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in R.GAUSS_SHAPES])
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_gaussian_against_fp64(fmt, shape):
    """|out - ref| <= 0.5 bf16_ulp(ref) + C_ACC sum |a w| on EVERY element, no outlier allowance"""
    p = R.gaussian(fmt, shape)
    out = Operands(p).gemm()
    worst = R.acc_excess(out, p)
    share = float((out != R.bf16_round(p.expect)).double().mean())
    print(f"[{p.name}] worst (|err| - 0.5 ulp) / sum |a w| = {worst:.3e} = 2^{math.log2(max(worst, 1e-300)):.2f}, share != bf16(ref) {share:.2e}")
    print(f"[{p.name}] C_ACC = 2^{math.log2(R.c_acc()):.0f}")
    assert worst <= R.c_acc(), f"{p.name}: (|err| - 0.5 ulp) / sum |a w| = {worst} > C_ACC = {R.c_acc()}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# F. quantisers
# ---------------------------------------------------------------------------------------------------------------------------------------
def _quant(fmt, x, ld_extra=0):
    """the device quantiser on x (CPU bf16) -> (bytes [R][row bytes], scales) on the CPU"""
    from gen3c_amd import ops
    xd = x.to(_dev())
    q, s = ops.quant_mxfp8(xd) if fmt is R.FP8 else ops.quant_mxfp6(xd)
    torch.cuda.synchronize()
    return q.view(torch.uint8).cpu(), s.cpu()


def _quant_ref(fmt, x):
    q, s = quant_mxfp8_ref(x) if fmt is R.FP8 else quant_mxfp6_ref(x)
    return q.view(torch.uint8), s


@pytest.mark.parametrize("anchor", list(R.QUANT_ANCHORS))
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_quantiser_every_bf16_value(fmt, anchor):
    """every finite bf16 value not above the planted block maximum, one block each: every tie and every saturation, bitwise"""
    x = R.quant_sweep(anchor)
    q, s = _quant(fmt, x)
    rq, rs = _quant_ref(fmt, x)
    bad_s, bad_q = int((s != rs).sum()), int((q != rq).any(-1).sum())
    print(f"[quantiser sweep {fmt.name}, amax {anchor}] {x.shape[0]} blocks: {bad_s} scale bytes, {bad_q} blocks of codes differ")
    assert bad_s == 0 and bad_q == 0


@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_quantiser_nonfinite_rule(fmt):
    """a NaN or an infinity anywhere in a block: scale byte 0xFF and zero codes; every other block bitwise what the finite rule gives"""
    x = R.nonfinite_input()
    q, s = _quant(fmt, x)
    rq, rs = _quant_ref(fmt, x)
    assert torch.equal(s, rs) and torch.equal(q, rq)
    bad = ~torch.isfinite(x.float()).reshape(x.shape[0], -1, R.BLOCK).all(-1)
    assert bool((s[bad] == R.SCALE_NAN).all()) and bool((s[~bad] != R.SCALE_NAN).all()) and int(bad.sum()) == 48
    clean = torch.where(torch.isfinite(x.float()), x.float(), torch.zeros(())).to(torch.bfloat16)
    cq, cs = _quant(fmt, clean)
    bb = fmt.row_bytes(R.BLOCK)
    assert torch.equal(s[~bad], cs[~bad]) and torch.equal(q.reshape(x.shape[0], -1, bb)[~bad], cq.reshape(x.shape[0], -1, bb)[~bad]), \
        "a finite block changed because a neighbour is not finite"
    assert bool((q.reshape(x.shape[0], -1, bb)[bad] == 0).all())


@pytest.mark.parametrize("D,wave", [(256, 0), (4096, 0), (4096, 1)], ids=["256", "4096", "4096-one-wave-per-row"])
def test_layernorm_producers_nonfinite_rule(D, wave):
    """the fused LayerNorm producers (one workgroup per row and, at D = 4096 under the "ln_wave_rows" option, one wave per row): a non-finite
    shift poisons its own block only, a non-finite x its whole row - as the bf16 chain (layernorm_modulate, then the reference quantiser) says"""
    import os
    from gen3c_amd import ops
    dev = _dev()
    ops.set_option("ln_wave_rows", wave)
    try:
        _layernorm_nonfinite_case(D, ops, dev)
    finally:
        ops.set_option("ln_wave_rows", int(os.environ.get("G3_LN_WAVE_ROWS", "0")))  # what the library starts with (csrc/api.hip)


def _layernorm_nonfinite_case(D, ops, dev):
    T, Hp, Wp, B = 2, 3, 2, 2
    rows = T * Hp * Wp * B
    g = torch.Generator().manual_seed(11)
    x = torch.randn(rows, D, generator=g).to(torch.bfloat16)
    shift = (0.5 * torch.randn(B, D, generator=g)).to(torch.bfloat16)
    scale = (0.5 * torch.randn(B, D, generator=g)).to(torch.bfloat16)
    shift[0, 37], shift[1, 200], scale[1, 70] = float("nan"), float("inf"), float("-inf")
    x[5, 100], x[8, 3] = float("inf"), float("nan")
    pe = (0.3 * torch.randn(T * Hp * Wp, D, generator=g)).to(torch.bfloat16).to(dev)
    x, shift, scale = x.to(dev), shift.to(dev), scale.to(dev)
    h = ops.layernorm_modulate(x, shift, scale)
    q, s = ops.layernorm_modulate_mxfp8(x, shift, scale)
    xc, xf = x.clone(), x.clone()
    hp = ops.posemb_layernorm_modulate(xc, pe, None, None, None, T, Hp, Wp, B, shift, scale)
    qp, sp = ops.posemb_layernorm_modulate_mxfp8(xf, pe, None, None, None, T, Hp, Wp, B, shift, scale)
    torch.cuda.synchronize()
    for what, hh, qq, ss in (("layernorm", h, q, s), ("posemb layernorm", hp, qp, sp)):
        rq, rs = quant_mxfp8_ref(hh.cpu())
        assert torch.equal(ss.cpu(), rs) and torch.equal(qq.view(torch.uint8).cpu(), rq.view(torch.uint8)), f"{what}: differs from the chain"
        nan_blocks = ss.cpu() == R.SCALE_NAN
        assert bool(nan_blocks[5].all()) and bool(nan_blocks[8].all()), f"{what}: a non-finite x must poison its row"
        assert nan_blocks[0].nonzero().flatten().tolist() == [1] and nan_blocks[1].nonzero().flatten().tolist() == [2, 6], f"{what}: {nan_blocks[:2]}"


def _nonfinite_gemm_case():
    """the Gaussian operands of ODD_KTILES and a copy of the activations with three poisoned token rows: -> a0, a, w (bf16, CPU), rows"""
    a0, w = R.gaussian_bf16(R.ODD_KTILES)
    a = a0.clone()
    a[7, 5], a[256, 383], a[299, 200] = float("nan"), float("inf"), float("-inf")
    return a0, a, w, [7, 256, 299]


@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_nonfinite_end_to_end(fmt):
    """quantiser, then GEMM, through ops: a NaN or an infinity in an activation block makes every output of its token row non-finite, one
    in a weight block every output of its feature column - as the bf16 linears do -; every other output is bitwise what it is without"""
    from gen3c_amd import ops
    dev = _dev()
    a0, a, w, rows = _nonfinite_gemm_case()
    quant = ops.quant_mxfp8 if fmt is R.FP8 else ops.quant_mxfp6
    gemm = ops.gemm_mxfp8_nt if fmt is R.FP8 else ops.gemm_mxfp6_nt
    name_of = _lib().g3_gemm_mxfp8_kernel_name if fmt is R.FP8 else _lib().g3_gemm_mxfp6_kernel_name
    M, N, K = R.ODD_KTILES
    assert name_of(M, N, K, 0) is not None
    wbad = w.clone()
    wbad[300, 100] = float("nan")
    wq, ws = quant(w.to(dev))
    wbq, wbs = quant(wbad.to(dev))
    base = gemm(*quant(a0.to(dev)), wq, ws).cpu()
    for epi in (0, 1, 2):
        kw = {}
        if epi == 2:
            gate, res = R.epilogue_operands(M, N)
            kw = dict(gate=gate[:1].to(dev), residual=res.to(dev))
        out = gemm(*quant(a.to(dev)), wbq, wbs, epilogue=epi, **kw).float().cpu()
        assert bool((~torch.isfinite(out[rows])).all()), f"{fmt.name} epilogue {epi}: a poisoned token row has finite outputs"
        assert bool((~torch.isfinite(out[:, 300])).all()), f"{fmt.name} epilogue {epi}: the poisoned weight row has finite outputs"
        if epi == 0:
            keep = torch.ones(M, N, dtype=torch.bool)
            keep[rows] = False
            keep[:, 300] = False
            assert torch.equal(R.bits_of(out.to(torch.bfloat16))[keep], R.bits_of(base)[keep]), "a finite output changed"
    if fmt is R.FP8:  # the MXFP8-output form: the poisoned rows' blocks leave as the E8M0 NaN, and the next GEMM carries it on
        assert _lib().g3_gemm_mxfp8_mxout_kernel_name(M, N, K, 1) == b"gemm_mxfp8_nt_kernel<257>"
        q, s = ops.gemm_mxfp8_nt(*quant(a.to(dev)), wq, ws, epilogue=1, out_mx=True)
        torch.cuda.synchronize()
        s = s.cpu()
        assert bool((s[rows] == R.SCALE_NAN).all()) and int((s == R.SCALE_NAN).sum()) == len(rows) * (N // 32)
        assert bool((q.view(torch.uint8).cpu()[rows] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals: the alignment clauses of mx_check_operands the older refusal tests do not reach
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["g3_gemm_mxfp8_nt", "g3_gemm_mxfp6_nt", "g3_gemm_mxfp8_nt_mxout"])
def test_refusals_of_operand_alignment_write_nothing(entry):
    from gen3c_amd import _lib
    lib = _lib.load()
    dev = _dev()
    M, N, K = 256, 256, 256
    rb = K if entry != "g3_gemm_mxfp6_nt" else K // 4 * 3
    ld = rb + 64
    aq = torch.zeros(M, ld, dtype=torch.uint8, device=dev)
    wq = torch.zeros(N, ld, dtype=torch.uint8, device=dev)
    sa = torch.full((M, 64), 127, dtype=torch.uint8, device=dev)
    sw = torch.full((N, 64), 127, dtype=torch.uint8, device=dev)
    c = torch.full((M, N + 64), 7.0, dtype=torch.bfloat16, device=dev)
    qo = torch.full((M, N + 64), 0xAA, dtype=torch.uint8, device=dev)
    so = torch.full((M, 64), 0xAA, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(aq_p=None, lda=ld, as_p=None, ldas=64, wq_p=None, ldw=ld, ws_p=None, ldws=64):
        ptr = lambda v, t: 0 if v == 0 else (v or t.data_ptr())
        head = (ptr(aq_p, aq), lda, ptr(as_p, sa), ldas, ptr(wq_p, wq), ldw, ptr(ws_p, sw), ldws)
        if entry == "g3_gemm_mxfp8_nt_mxout":
            return lib.g3_gemm_mxfp8_nt_mxout(*head, qo.data_ptr(), N + 64, so.data_ptr(), 64, M, N, K, 0, stream)
        return getattr(lib, entry)(*head, c.data_ptr(), N + 64, M, N, K, 0, 0, 1, 0, 0, 0, stream)

    cases = {
        "lda no multiple of 16": dict(lda=ld + 8),
        "ldw no multiple of 16": dict(ldw=ld + 8),
        "ldw below the row bytes": dict(ldw=rb - 16),
        "ldws no multiple of 4": dict(ldws=62),
        "weight scales off by 2 bytes": dict(ws_p=sw.data_ptr() + 2),
        "activation scales off by 1 byte": dict(as_p=sa.data_ptr() + 1),
        "weights off by 8 bytes": dict(wq_p=wq.data_ptr() + 8),
        "null activations": dict(aq_p=0),
        "null activation scales": dict(as_p=0),
        "null weights": dict(wq_p=0),
        "null weight scales": dict(ws_p=0),
    }
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == _lib.G3_ERR_ARG, f"{entry}, {what}: rc {rc}"
        assert _lib.last_error().startswith(entry), f"{entry}, {what}: {_lib.last_error()}"
    torch.cuda.synchronize()
    assert bool((c == 7.0).all()) and bool((qo == 0xAA).all()) and bool((so == 0xAA).all()), f"{entry}: a refused call wrote its output"
    assert call() == _lib.G3_OK  # the same buffers are accepted as they are
    torch.cuda.synchronize()
    if entry == "g3_gemm_mxfp8_nt_mxout":
        assert bool((qo[:, :N] == 0).all()) and bool((so[:, :N // 32] == 127).all()) and bool((qo[:, N:] == 0xAA).all())
    else:
        assert bool((c[:, :N] == 0).all()) and bool((c[:, N:] == 7.0).all())
