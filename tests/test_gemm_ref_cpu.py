"""Pins tests/gemm_ref.py, the fp64 references the kernel-level GPU tests of the GEMM epilogues compare against, so that a wrong test reference
cannot hide a wrong kernel - and shows on the CPU, on the GPU suite's own inputs, that (1) a correct fp32 evaluation passes the very checker the
GPU test uses at every family and shape, (2) C_GEMM and C_GELU are 4 x that evaluation's worst figure rounded up to a power of two, (3) the
allowance C E exceeds half an ulp on at most 5 % of every case, and (4) every one-defect mutant fails that checker on at least one case
(run with -s to see the figures; profiles/gemm_epilogue_parity_measured.txt holds them)."""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import dit_oracle
from tests import gemm_ref as gr

bf16 = torch.bfloat16
# the shapes of the GPU suite; the deferred-epilogue shape (M from the device's CU count, N = 4096, K = 2432) on 64 of its rows
SHAPES = [gr.SMALL, gr.K128] + gr.RAGGED + [(64,) + gr.DEFERRED_NK]
CASES = [(s, f) for f in gr.FAMILIES for s in SHAPES]
ROWS = 3  # gate / bias rows of the CPU cases: m % 3 and m / 3 differ from the second row on, and no shape's M is a multiple


def _caught(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


# =================================================================================================================================
# the references against fp64 torch and what the oracle calls
# =================================================================================================================================
@pytest.mark.parametrize("family", gr.FAMILIES)
def test_references_equal_fp64_torch_and_the_calls_of_the_oracle(family):
    """oracle/dit_oracle.py evaluates the MLP and the gated residual inline (F.linear(F.gelu(F.linear(h, w1)), w2); xs + gate * y), with no
    function of its own to call: the references are pinned against those torch calls in fp64, and the oracle's source against the erf form."""
    M, N, K = gr.RAGGED[0]
    a, w, gate, res = gr.inputs(M, N, K, family)
    src = inspect.getsource(dit_oracle.dit_forward)
    assert "F.gelu(F.linear(" in src and "approximate" not in src and "xs + gate * y" in src
    ref, E = gr.linear_ref(a, w)
    want = F.linear(a.double(), w.double())
    assert ref.dtype == torch.float64 and float(((ref - want).abs() / (want.abs() + 1)).max()) <= 1e-12
    assert bool((E >= gr.U24 * ref.abs() - 1e-300).all()) and bool(torch.isfinite(E).all())
    m = torch.arange(M) % ROWS
    refb, Eb = gr.linear_ref(a, w, gate[:ROWS])
    assert float((refb - (want + gate.double()[m])).abs().max()) <= 1e-12 and bool((Eb >= E).all())
    refr, Er = gr.linear_ref(a, w, gate[:ROWS], res)
    assert float((refr - ((want + gate.double()[m]) + res.double())).abs().max()) <= 1e-12 and bool((Er >= Eb).all())
    y = gr.bf16_round(ref)
    g64, Eg = gr.gelu_ref(y)
    assert float((g64 - F.gelu(y.double())).abs().max()) <= 1e-15 * float(y.float().abs().max())
    erfc_form = 0.5 * y.double() * torch.special.erfc(-y.double() / math.sqrt(2.0))
    assert bool(((g64 - erfc_form).abs() <= 1e-12 * erfc_form.abs()).all()) and torch.equal(Eg, gr.U24 * y.double().abs())
    gref, gE = gr.gated_ref(y, gate[:ROWS], res)
    assert torch.equal(gref, res.double() + gate.double()[m] * y.double()) and torch.equal(gE, gr.U24 * gref.abs())
    # the gated residual has one right answer: g y is exact in fp32, so fp32(R + g y) is the fp64 sum rounded once
    one = (res.double() + gate.double()[m] * y.double()).float().to(bf16)
    assert torch.equal(gr.gated_fp32(y, gate[:ROWS], res).view(torch.int16), one.view(torch.int16))
    assert bool(((one.double() - gref).abs() <= 0.5 * gr.bf16_ulp(gref) + gE).all())


def test_gelu_tails_of_the_reference():
    y = torch.tensor([0.0, -0.0, 2.0 ** -133, -(2.0 ** -126), 1.0, -1.0, 40.0, -40.0, 3.0e38, -3.0e38], dtype=bf16)
    g = gr.gelu64(y)
    assert g[0] == 0 and g[1] == 0 and g[2] == 2.0 ** -134 and g[3] == -(2.0 ** -127)
    assert abs(float(g[4]) - 0.8413447460685429) < 1e-15 and abs(float(g[5]) + 0.15865525393145707) < 1e-15
    assert g[6] == 40.0 and g[7] == 0 and g[8] == float(y[8]) and g[9] == 0  # erfc underflows: exactly y and exactly 0
    assert bool(torch.isfinite(g).all())


# =================================================================================================================================
# the sweep: every finite bf16 value through the restated GELU
# =================================================================================================================================
def test_restated_gelu_over_every_finite_bf16_value():
    """gelu_fast32 on all 65 280 finite bf16 values passes the sweep's checker; measured: worst (err - 0.5 ulp) / E 0.243, 167 values differ
    from bf16_round(gelu64), all below -2 (144 below -6); 260 values lie within 2^-10 ulp of a rounding tie, 259 of them with |y| <= 2 - so
    the GPU sweep excludes the near-tie list from its exact bar - and the restatement rounds even those as the reference does."""
    y = gr.finite_bf16()
    assert y.numel() == 65280
    out = gr.gelu_fast32(y)
    worst, share, share_r, frac = gr.check_sweep("restated gelu, every finite bf16 value", y, out)
    ref = gr.gelu64(y)
    diff = out != gr.bf16_round(ref)
    near = gr.gelu_near_tie()[gr.bits_of(y)]
    print(f"differ from bf16_round(ref): {int(diff.sum())} (y < -2: {int((diff & (y.float() < -2)).sum())}, y < -6: {int((diff & (y.float() < -6)).sum())}); "
          f"near-tie values {int(near.sum())}, with |y| <= 2: {int((near & (y.float().abs() <= 2)).sum())}")
    assert int(diff.sum()) == 167 and not bool((diff & (y.float() >= -2)).any())
    assert 0 < int(near.sum()) < 400
    assert gr.pow2_ceil(4 * worst) == gr.C_GELU
    # the whole sweep against the 5 % condition: it cannot hold (every y < -4 has C E > 0.5 ulp), which is why check_sweep applies it to y >= -4
    assert gr.half_ulp_share(ref, gr.U24 * y.double().abs(), gr.C_GELU) > 0.2
    # an input the kernels' form rests on: x x overflows, the exponent is -inf, exp2 gives 0
    big = torch.tensor([3.0e38, -3.0e38, 2.0e19, -2.0e19], dtype=bf16)
    assert gr.gelu_fast32(big).tolist() == [float(big[0]), 0.0, float(big[2]), 0.0]


def test_sweep_operands_carry_every_value_as_a_one_term_product():
    a, w = gr.sweep_inputs(256, 256, 256)
    assert torch.equal(a.reshape(-1)[:65280].view(torch.int16), gr.finite_bf16().view(torch.int16)) and bool(torch.isfinite(a.float()).all())
    assert torch.equal(w.float(), torch.eye(256))
    a, w = gr.sweep_inputs(512, 4096, 2432)
    assert int((w != 0).sum()) == 4096 and bool((w.float().sum(1) == 1).all()) and bool((w[torch.arange(4096), torch.arange(4096) % 2432] == 1).all())
    assert set(gr.bits_of(a.reshape(-1)).tolist()) == set(gr.bits_of(gr.finite_bf16()).tolist())


def test_mxfp8_sweep_operands_dequantise_to_the_values():
    from tests.mxfp8_ref import dequant_mxfp8
    x, aq, as_, wq, ws = gr.mx_sweep_inputs()
    assert x.shape == (7936, 8) and aq.shape == (7936, 256) and float(x.float().abs().min()) == 2.0 ** -120
    deq = dequant_mxfp8(aq, as_).double().reshape(7936, 8, 32)
    assert bool((deq[:, :, 2:] == 0).all()) and torch.equal(deq.sum(-1), x.double()), "dequant(hi) + dequant(lo) must be x exactly"
    wd = dequant_mxfp8(wq, ws).double()
    assert torch.equal((deq.reshape(7936, 256) @ wd.t())[:, :8], x.double()) and torch.equal(wd[:8], wd[8:16])


# =================================================================================================================================
# the restatements pass the GPU test's checker at every family and shape; the 5 % condition; C derived from them
# =================================================================================================================================
def _case(shape, family, mutant=""):
    """both stages as the GPU test runs them, on the restatement (or a one-defect mutant of it) -> the worst of each checked output"""
    M, N, K = shape
    a, w, gate4, res = gr.inputs(M, N, K, family)
    gate = gate4[:ROWS]
    what = f"{M}x{N}x{K} {family} {mutant or 'restatement'}"
    lin = mutant if mutant in gr.MUTANTS_LINEAR else ""
    acc = gr.linear_acc32(a, w, lin)
    y = acc.to(bf16)  # the Linear's rounded output: the input of stage 2
    worst = {}
    for name, bias, r in (("none", None, None), ("bias", gate, None), ("bias_residual", gate, res)):
        ref, E = gr.linear_ref(a, w, bias, r)
        out = y if bias is None else gr.linear_fp32(a, w, bias, r, mutant=lin)
        worst[name] = gr.check(f"{name} {what}", out, ref, E, gr.C_GEMM, y if bias is None and not lin else gr.linear_fp32(a, w, bias, r))[0]
    ref, E = gr.gelu_ref(y)
    worst["gelu"] = gr.check(f"gelu {what}", gr.gelu_fp32(y, acc, mutant if mutant in gr.MUTANTS_GELU else ""), ref, E, gr.C_GELU, gr.gelu_fast32(y))[0]
    gm = mutant if mutant in gr.MUTANTS_GATE else ""
    got = gr.gated_fp32(y, gate, res, acc, gm)
    assert torch.equal(got.view(torch.int16), gr.gated_fp32(y, gate, res).view(torch.int16)), f"gated residual {what}: not bitwise bf16(fp32(R + g y))"
    ref, E = gr.gated_ref(y, gate, res)
    gr.check(f"gated residual {what}", got, ref, E, 1.0, gr.gated_fp32(y, gate, res))
    return worst


@pytest.mark.parametrize("family", gr.FAMILIES)
def test_restatements_pass_the_checker_at_every_shape_and_the_allowance_stays_below_five_percent(family):
    """gr.check asserts all three bars per case, the 5 % condition (C E > 0.5 ulp on at most 5 % of the elements) among them, for EPI_NONE, BIAS,
    BIAS_RESIDUAL (C_GEMM), GELU (C_GELU) and the gated residual; the latter is bitwise besides."""
    for shape in SHAPES:
        _case(shape, family)


def test_constants_are_four_times_the_restatements_worst():
    """C = 4 x the worst (err - 0.5 ulp) / E of the fp32 restatement over the suite's families and shapes (2.3 M outputs per epilogue),
    rounded up to a power of two. Measured: the Linear 2.956 (same-sign operands at K = 2432: the running sum grows chunk by chunk and every
    fp32 add rounds at its size) -> 16; GELU 0.243 (the sweep; no case of the families is worse) -> 1."""
    w_gemm, w_gelu = -math.inf, gr.measure(gr.gelu_fast32(gr.finite_bf16()), *gr.gelu_ref(gr.finite_bf16()))[0]
    for shape, family in CASES:
        w = _case(shape, family)
        w_gemm = max(w_gemm, w["none"], w["bias"], w["bias_residual"])
        w_gelu = max(w_gelu, w["gelu"])
    print(f"restatements' worst (err - 0.5 ulp) / E: linear {w_gemm:.3f}, gelu {w_gelu:.3f}")
    assert gr.pow2_ceil(4 * w_gemm) == gr.C_GEMM, f"C_GEMM = {gr.C_GEMM} is not 4 x {w_gemm:.3f} rounded up to a power of two"
    assert gr.pow2_ceil(4 * w_gelu) == gr.C_GELU, f"C_GELU = {gr.C_GELU} is not 4 x {w_gelu:.3f} rounded up to a power of two"


# =================================================================================================================================
# every mutant is caught by the same checker on the same inputs
# =================================================================================================================================
@pytest.mark.parametrize("mutant", gr.MUTANTS_GELU + gr.MUTANTS_GATE + gr.MUTANTS_LINEAR)
def test_mutants_are_caught(mutant):
    caught = [(s, f) for s, f in CASES if _caught(lambda: _case(s, f, mutant))]
    print(f"mutant {mutant}: caught on {len(caught)} of {len(CASES)} cases: {caught}")
    assert caught


@pytest.mark.parametrize("mutant", ["gelu_tanh", "gelu_no_log2e", "gelu_coef_sign"])
def test_gelu_mutants_are_caught_by_the_sweep(mutant):
    y = gr.finite_bf16()
    assert _caught(lambda: gr.check_sweep(f"sweep, mutant {mutant}", y, gr.gelu_fast32(y, mutant)))


def test_tile_rows_hold_the_edges_of_the_first_a_middle_and_the_last_tile():
    for M in (8192, 7936, 257 + 1024):
        r = gr.tile_rows(M).tolist()
        tiles = -(-M // 256)
        assert len(r) <= 256 and r == sorted(set(r)) and r[-1] == M - 1
        for t in (0, tiles // 2, tiles - 1):
            assert 256 * t in r and min(256 * t + 255, M - 1) in r
    assert gr.tile_rows(1024).tolist() == list(range(1024))
