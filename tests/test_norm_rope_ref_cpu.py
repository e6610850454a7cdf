"""Pins tests/norm_rope_ref.py, the fp64 references the kernel-level GPU tests of norm_rope.hip compare against, so that a wrong test reference
cannot hide a wrong kernel - and shows on the CPU, on the GPU suite's own inputs, that (1) a correct fp32 evaluation in the kernels' summation
order passes the very checker the GPU test uses, (2) each constant C is 4 x that evaluation's worst figure rounded up to a power of two, and
(3) every one-defect mutant of the module fails that checker on at least one case (run with -s to see the figures)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import dit_oracle
from tests import norm_rope_ref as kr

bf16 = torch.bfloat16


def _caught(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


# =================================================================================================================================
# the references against the oracle and fp64 torch
# =================================================================================================================================
@pytest.mark.parametrize("D,B,wave", kr.LN_CASES)
def test_layernorm_reference_equals_fp64_torch_and_the_oracle(D, B, wave):
    x, mod = kr.ln_inputs(D, B)
    shift, scale = mod[:, :D], mod[:, D:2 * D]
    ref, E = kr.ln_ref(x, shift, scale)
    m = torch.arange(x.shape[0]) % B
    want = F.layer_norm(x.double(), (D,), None, None, 1e-6) * (1 + scale.double()[m]) + shift.double()[m]
    assert ref.dtype == torch.float64 and float(((ref - want).abs() / (want.abs() + 1)).max()) <= 1e-12
    oracle = dit_oracle._layernorm(x.float()) * (1 + scale.float()[m]) + shift.float()[m]  # fp32: to fp32 precision of the terms
    assert bool(((ref - oracle.double()).abs() <= 64 * E + 1e-30).all())
    assert bool((E >= 0).all()) and bool(torch.isfinite(E).all())
    # what the inputs promise
    cols = kr.ln_scale_m1_cols(D)
    assert torch.equal(kr.bf16_round(ref[:, cols]), shift[m][:, cols]), "scale = -1 columns: the result is the shift"
    assert torch.equal(kr.bf16_round(ref[kr.LN_CONST_ROW]), shift[kr.LN_CONST_ROW % B]), "constant row: the result is the shift"
    assert float(ref[0, ~cols].abs().max()) <= float(shift[0, ~cols].float().abs().max()) * 2.0 ** -8, "row 0 cancels to a rounding of the shift"


@pytest.mark.parametrize("S,B,Hq,Hk", kr.RMS_CASES)
def test_rmsnorm_and_rope_references_equal_the_oracle(S, B, Hq, Hk):
    x, w, cos, sin = kr.rms_inputs(S, B, Hq, Hk)
    H = Hq + Hk
    ref, E = kr.rms_ref(x, w)
    want32 = dit_oracle.te_rmsnorm(x.float(), w.float())  # the oracle computes in fp32 whatever it is given: to fp32 precision
    assert bool(((ref - want32.double()).abs() <= 64 * E).all())
    xd = x.double()
    want = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double()  # its line, in fp64
    assert float(((ref - want).abs() / (want.abs() + 1e-300)).max()) <= 1e-12
    zero = torch.arange(S * B) % kr.RMS_FAMILIES == kr.RMS_ZERO_FAMILY
    assert bool(zero.any()) and bool((ref[zero] == 0).all()) and bool((E[zero] == 0).all())
    # RoPE on bf16 values: freqs whose cos / sin are the tables. The oracle takes angles, so recover them: atan2(sin, cos)
    y = kr.bf16_round(ref)
    rref, rE = kr.rope_ref(y, cos, sin, B)
    freqs = torch.atan2(sin.double(), cos.double()).view(S, 1, 1, 128)
    want = dit_oracle.te_rope_fused(y.double().reshape(S, B, H, 128), freqs).reshape(S * B, H, 128)
    assert float((rref - want).abs().max()) <= 1e-5 * float(y.float().abs().max())  # the tables are fp32 roundings of cos / sin of the angles
    assert bool((rE >= rref.abs() * kr.U24 - 1e-300).all())


def test_bf16_rounding_helpers_and_silu_list():
    a = kr.all_bf16()
    fin = torch.isfinite(a.float())
    assert int(fin.sum()) == 65280
    assert torch.equal(kr.bf16_round(a[fin].double()), a[fin])
    near = kr.silu_near_tie()
    assert 0 < int(near.sum()) < 400 and not bool(near[~fin].any())
    g = torch.Generator().manual_seed(5)
    safe = kr.silu_safe(torch.randn(100000, generator=g).to(bf16))
    assert not bool(near[(safe.view(torch.int16).to(torch.int32) & 0xFFFF).long()].any())


def test_silu_fp32_rounds_to_the_reference_outside_the_near_tie_list():
    """x / (1 + exp(-x)) in fp32, rounded to bf16, on every finite bf16 value: equal to bf16_round(silu64(a)) wherever the reference does not
    list the value as a near tie and |silu64(a)| > 2^-100 (below that the fp32 exp overflows: -0 for about -1e-37); within one ulp on the list."""
    a = kr.all_bf16()
    fin = torch.isfinite(a.float())
    s64 = kr.silu64(a)
    got = (a.float() / (1.0 + torch.exp(-a.float()))).to(bf16)
    want = kr.bf16_round(s64)
    must = fin & ~kr.silu_near_tie() & (s64.abs() > 2.0 ** -100)
    assert int(must.sum()) > 40000  # the rest: |silu| below 2^-100 (tiny a, or a < -75)
    assert int((got[must] != want[must]).sum()) == 0
    listed = fin & kr.silu_near_tie()
    assert float(kr.ulp_error(got[listed], s64[listed]).max()) <= 1.0


# =================================================================================================================================
# the fp32 restatements pass the GPU test's checker; C is derived from them
# =================================================================================================================================
def _ln_case(D, B, wave, mutant=""):
    x, mod = kr.ln_inputs(D, B)
    shift, scale = mod[:, :D], mod[:, D:2 * D]
    ref, E = kr.ln_ref(x, shift, scale)
    good = kr.ln_fp32(x, shift, scale, wave=bool(wave))
    out = kr.ln_fp32(x, shift, scale, wave=bool(wave), mutant=mutant) if mutant else good
    return kr.check(f"layernorm D={D} B={B} wave={wave} {mutant or 'restatement'}", out, ref, E, kr.C_LN, good)


def _rms_case(S, B, Hq, Hk, mutant=""):
    """both stages, as the GPU test runs them -> worst of each"""
    x, w, cos, sin = kr.rms_inputs(S, B, Hq, Hk)
    y_good, r_good = kr.rms_rope_fp32(x, w, cos, sin, B)
    y, r = kr.rms_rope_fp32(x, w, cos, sin, B, mutant=mutant) if mutant else (y_good, r_good)
    what = f"S={S} B={B} H={Hq}+{Hk} {mutant or 'restatement'}"
    ref, E = kr.rms_ref(x, w)
    w1 = kr.check(f"rmsnorm {what}", y, ref, E, kr.C_RMS, y_good)[0]
    ref, E = kr.rope_ref(y, cos, sin, B)  # on the no-RoPE output delivered: the stage's own input
    w2 = kr.check(f"rope {what}", r, ref, E, kr.C_ROPE, kr.rope_fp32(y, cos, sin, B))[0]
    return w1, w2


def _gemv_case(M, N, K, act, mutant=""):
    a, w, add = kr.gemv_inputs(M, N, K, act)
    ref, E = kr.gemv_ref(a, w, act)
    good = kr.gemv_fp32(a, w, None, act)
    out = kr.gemv_fp32(a, w, None, act, mutant=mutant) if mutant else good
    worst = kr.check(f"gemv {M}x{N}x{K} act={act} {mutant or 'restatement'}", out, ref, E, kr.C_GEMV, good)[0]
    with_add = kr.gemv_fp32(a, w, add, act, mutant=mutant)
    assert torch.equal(with_add, kr.add_bf16(out, add)), "gemv + add != bf16(float(out without add) + float(add))"
    return worst


def test_restatements_pass_the_checker_on_every_case_of_the_gpu_suite():
    for c in kr.LN_CASES:
        _ln_case(*c)
    for c in kr.RMS_CASES:
        _rms_case(*c)
    for c in kr.GEMV_CASES:
        for act in (0, 1):
            _gemv_case(*c, act)


def test_constants_are_four_times_the_restatements_worst():
    """C = 4 x the worst (err - 0.5 ulp) / E of the fp32 restatement, rounded up to a power of two. The figure is the tail of a distribution: it
    is positive only where the reference lies within a few E of a rounding tie, one element in about 2^16, so the cases of the GPU suite (a few
    thousand to 1e5 elements each) are too few to show it for the per-head kernels and the GEMV (their worst there is below 0.5 or negative).
    It is therefore taken over the suite's own input FAMILIES - the same builders - at 6 M elements (RMSNorm, RoPE: 3072 rows x 16 heads) and
    160 k outputs per shape (GEMV: N = 20000); LayerNorm over the suite's cases themselves (0.57 M elements, rows of every family).
    Measured: layernorm 0.624 -> 4, rmsnorm 1.736 -> 8, rope 1.139 -> 8, gemv 0.379 -> 2."""
    worst_ln = max(_ln_case(*c)[0] for c in kr.LN_CASES)
    S, B, Hq, Hk = 1024, 3, 8, 8
    x, w, cos, sin = kr.rms_inputs(S, B, Hq, Hk)
    y, r = kr.rms_rope_fp32(x, w, cos, sin, B)
    worst_rms = kr.measure(y, *kr.rms_ref(x, w))[0]
    worst_rope = kr.measure(r, *kr.rope_ref(y, cos, sin, B))[0]
    worst_gemv = -1.0
    for M, N, K in ((8, 20000, 8), (8, 20000, 72), (8, 20000, 520)):
        for act in (0, 1):
            a, wt, _ = kr.gemv_inputs(M, N, K, act)
            worst_gemv = max(worst_gemv, kr.measure(kr.gemv_fp32(a, wt, None, act), *kr.gemv_ref(a, wt, act))[0])
    print(f"restatements' worst (err - 0.5 ulp) / E: layernorm {worst_ln:.3f}, rmsnorm {worst_rms:.3f}, rope {worst_rope:.3f}, gemv {worst_gemv:.3f}")
    for name, worst, C in (("layernorm", worst_ln, kr.C_LN), ("rmsnorm", worst_rms, kr.C_RMS), ("rope", worst_rope, kr.C_ROPE), ("gemv", worst_gemv, kr.C_GEMV)):
        assert kr.pow2_ceil(4 * worst) == C, f"{name}: C = {C} is not 4 x {worst:.3f} rounded up to a power of two"


def test_exact_operations_restated():
    x = torch.tensor([1.0, 256.0, -3.0], dtype=bf16)
    y = torch.tensor([2.0 ** -8, 1.0, 3.0], dtype=bf16)
    assert kr.add_bf16(x, y).tolist() == [1.0, 256.0, 0.0]  # 1 + 2^-8 is a tie between 1 and 1 + 2^-7, 257 one between 256 and 258: to even


# =================================================================================================================================
# every mutant is caught on the GPU suite's inputs
# =================================================================================================================================
@pytest.mark.parametrize("mutant", ["no_eps", "var_dm1", "mod_div"])
def test_layernorm_mutants_are_caught(mutant):
    caught = [c for c in kr.LN_CASES if _caught(lambda: _ln_case(*c, mutant=mutant))]
    print(f"layernorm mutant {mutant}: caught on {len(caught)} of {len(kr.LN_CASES)} cases")
    assert caught


@pytest.mark.parametrize("mutant", ["rms_127", "no_round", "rot_sign", "w_first_half", "pos_mod"])
def test_rmsnorm_rope_mutants_are_caught(mutant):
    caught = [c for c in kr.RMS_CASES if _caught(lambda: _rms_case(*c, mutant=mutant))]
    print(f"rmsnorm / rope mutant {mutant}: caught on {len(caught)} of {len(kr.RMS_CASES)} cases")
    assert caught


@pytest.mark.parametrize("mutant", ["add_early", "silu_no_round"])
def test_gemv_mutants_are_caught(mutant):
    caught = [c for c in kr.GEMV_CASES if _caught(lambda: _gemv_case(*c, 1, mutant=mutant))]
    print(f"gemv mutant {mutant}: caught on {len(caught)} of {len(kr.GEMV_CASES)} cases")
    assert caught
