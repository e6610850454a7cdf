"""CPU: the MX probes of tests/mx_probe_ref.py are what they claim to be, and they have teeth.

 * the code tables (256 e4m3fn codes, 64 e2m3 codes, the E8M0 byte with 0xFF = NaN) against the formats' definitions, every element value a bf16
   value; the two CPU references' non-finite rule and 0xFF dequantisation;
 * every probe of families A - D: the closed form IS the fp64 product of the operands, every held output is exactly a bf16 value (or the
   probe says it is rounded once), and the sum of the absolute terms stays below 2^24 units of the smallest term - any summation order is exact
   in fp32, the kernel has one right answer;
 * the clean index model of the kernels reproduces every probe; each listed defect - in the token operand's reads or in the weight operand's -
   changes at least one held output of at least one probe (printed: which probes catch it);
 * the alignment probe's closed form, the derivation of C_ACC from the recorded measurement, the quantiser sweeps and the non-finite input."""
import math

import pytest
import torch

from tests import mx_probe_ref as R
from tests import mxfp6_ref, mxfp8_ref

FMT = [R.FP8, R.FP6]
FMT_IDS = ["mxfp8", "mxfp6"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# code tables and the references' non-finite rule
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_code_tables_against_the_format_definitions():
    t8 = mxfp8_ref.e4m3_values()
    for c in range(256):  # OCP e4m3fn: bias 7, subnormals m / 8 * 2^-6, S.1111.111 = NaN, no infinities
        e, m, neg = (c >> 3) & 15, c & 7, c >> 7
        if e == 15 and m == 7:
            assert math.isnan(float(t8[c])), c
            continue
        v = m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        assert float(t8[c]) == (-v if neg else v) and math.copysign(1.0, float(t8[c])) == (-1.0 if neg else 1.0), c
    assert float(t8.nan_to_num().abs().max()) == 448.0 and R.FP8.nan_codes == (0x7F, 0xFF)
    t6 = mxfp6_ref.e2m3_values()
    for c in range(64):  # e2m3: bias 1, subnormals m / 8, maximum 7.5, no NaN / infinity
        e, m, neg = (c >> 3) & 3, c & 7, c >> 5
        v = m / 8 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1)
        assert float(t6[c]) == (-v if neg else v), c
    assert float(t6.abs().max()) == 7.5 and bool(torch.isfinite(t6).all())
    s = mxfp8_ref.e8m0_values()
    assert s.shape == (256,) and math.isnan(float(s[255])) and float(s[127]) == 1.0 and float(s[0]) == 2.0 ** -127 and float(s[254]) == 2.0 ** 127
    for fmt in FMT:  # every element value is a bf16 value (so is its product with a power of two inside bf16's range)
        v = fmt.values()
        v = v[~torch.isnan(v)]
        assert torch.equal(v.to(torch.bfloat16).double(), v)
        assert float(fmt.values()[fmt.one]) == 1.0 and float(fmt.values()[fmt.one_half]) == 1.5
        assert float(fmt.values()[fmt.neg_zero]) == 0.0 and math.copysign(1.0, float(fmt.values()[fmt.neg_zero])) == -1.0


def test_scale_byte_0xff_dequantises_to_nan_in_both_references():
    q8 = torch.ones(2, 64).to(torch.float8_e4m3fn)
    s = torch.tensor([[127, 255], [255, 120]], dtype=torch.uint8)
    d = mxfp8_ref.dequant_mxfp8(q8, s)
    assert bool(torch.isnan(d[0, 32:]).all()) and bool(torch.isnan(d[1, :32]).all()) and bool((d[0, :32] == 1).all()) and bool((d[1, 32:] == 2.0 ** -7).all())
    q6 = mxfp6_ref.pack_e2m3(torch.full((2, 64), R.FP6.one, dtype=torch.uint8))
    d = mxfp6_ref.dequant_mxfp6(q6, s)
    assert bool(torch.isnan(d[0, 32:]).all()) and bool(torch.isnan(d[1, :32]).all()) and bool((d[0, :32] == 1).all()) and bool((d[1, 32:] == 2.0 ** -7).all())
    assert bool(torch.isnan(R.dequant(torch.zeros(1, 32, dtype=torch.uint8), torch.tensor([[255]], dtype=torch.uint8), R.FP8)).all()), "0 x NaN"


@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_reference_quantisers_non_finite_rule(fmt):
    """a block with a NaN or an infinity: byte 0xFF, zero codes; every other block what it is with the offender replaced by a finite value"""
    x = R.nonfinite_input()
    bad = ~torch.isfinite(x.float()).reshape(x.shape[0], -1, 32).all(-1)
    assert int(bad.sum()) == 48 and not bool(bad[40:].any())
    codes, s = R.quantise(x, fmt)
    clean = torch.where(torch.isfinite(x.float()), x.float(), torch.zeros(())).to(torch.bfloat16)
    cc, cs = R.quantise(clean, fmt)
    assert bool((s[bad] == 0xFF).all()) and bool((codes.reshape(x.shape[0], -1, 32)[bad] == 0).all())
    assert torch.equal(s[~bad], cs[~bad]) and torch.equal(codes.reshape(x.shape[0], -1, 32)[~bad], cc.reshape(x.shape[0], -1, 32)[~bad])
    assert not bool((cs == 0xFF).any()), "a finite block never has byte 0xFF (the clamp ends at 254)"
    d = R.dequant(codes, s, fmt).reshape(x.shape[0], -1, 32)
    assert bool(torch.isnan(d[bad]).all()) and bool(torch.isfinite(d[~bad]).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the probes: exact, order-free, reproduced by the clean model
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_probes_are_exact_order_free_and_the_clean_model_reproduces_them(fmt):
    worst = 0.0
    for p in R.exact_probes(fmt):
        M, N, K = p.shape
        assert N % 256 == 0 and K % 128 == 0 and M <= 1100, p.name
        assert R.expect_is_exact(p), f"{p.name}: the closed form is not the fp64 product / not a bf16 value"
        margin = R.order_free_margin(p)
        worst = max(worst, margin)
        assert margin < 2.0 ** 24, f"{p.name}: sum |terms| = 2^{math.log2(margin):.1f} units of the smallest term"
        held = p.asserted if p.asserted is not None else torch.ones(M, N, dtype=torch.bool)
        assert R.same_values(R.model_output(p), p.expect, held), f"{p.name}: the clean index model does not give the closed form"
        bits = p.expect_bits()
        fin = held & ~torch.isnan(p.expect)
        assert bool(((bits[fin] & 0x7F80) != 0x7F80).all()), f"{p.name}: a held expectation overflows bf16"
        if not p.rounded:  # the stated exactness: the bf16 expectation IS the closed form
            back = bits[fin].to(torch.int32).to(torch.int16).view(torch.bfloat16).double()
            assert torch.equal(back, torch.where(p.expect[fin] == 0, torch.zeros(()).double(), p.expect[fin]))
    print(f"[{fmt.name}] largest sum |terms| / unit over the exact probes: 2^{math.log2(worst):.1f} (< 2^24)")


def test_census_covers_every_code_and_every_k_of_a_tile():
    for fmt in FMT:
        for side in ("a", "w"):
            p = R.census_codes(fmt, side)
            codes = p.ac if side == "a" else p.wc
            nz = codes != 0
            assert bool((nz.sum(1) <= 1).all())
            assert set(codes[nz].tolist()) == set(range(1, fmt.ncodes)) and set(nz.nonzero()[:, 1].tolist()) >= set(range(128))
            other = p.wc if side == "a" else p.ac
            assert bool((other == fmt.one).all())
        g = R.scale_grid(fmt)
        assert int(g.asserted.sum()) == 48641 and sorted(set(g.as_[:, 0].tolist())) == list(range(256)) == sorted(set(g.ws[:, 0].tolist()))
    for shape, mode in R.POSITION_CASES:  # every k (every block) of every K tile owns an output column
        p = R.census_position(R.FP8, shape, mode)
        wd = R.dequant(p.wc, torch.full_like(p.ws, 127), p.fmt)
        owned = (wd != 0).any(0)
        K = shape[2]
        assert bool(owned.all()) if mode != "in_block" else bool(owned.reshape(K // 32, 32).any(1).all()), (shape, mode)
        assert int(p.as_.max()) - int(p.as_.min()) >= 70, "scale bytes 127 +- 40"


# ---------------------------------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------------------------------
TILE_DEFECTS = ("xcd_remap", "tail_group")  # the tile map has no operand side
DEFECT_CASES = [(d, side) for d in R.DEFECTS for side in (("a",) if d in TILE_DEFECTS else ("a", "w"))]


@pytest.mark.parametrize("defect,side", DEFECT_CASES, ids=[f"{d}-{s}" for d, s in DEFECT_CASES])
def test_each_defect_changes_an_expected_output(defect, side):
    caught = []
    for fmt in FMT:
        if R.DEFECT_FMT.get(defect, fmt.name) != fmt.name:
            continue
        for p in R.exact_probes(fmt):
            M, N, K = p.shape
            held = p.asserted if p.asserted is not None else torch.ones(M, N, dtype=torch.bool)
            if not R.same_values(R.model_output(p, defect, side), p.expect, held):
                caught.append(p.name)
    print(f"[{defect}{'' if defect in TILE_DEFECTS else ', operand ' + side}] caught by {len(caught)} probes, e.g. {caught[:3]}")
    assert caught, f"no probe sees the defect {defect} in operand {side}"
    if defect in ("stale_stage", "stale_scale"):  # the K = 16384 probes look into K tiles 5 .. 128
        assert any("16384" in name and "census_position" in name for name in caught)


def test_tile_map_is_a_permutation_and_its_defects_are_not():
    for M, N, _ in R.SHAPES + [(1100, 768, 512), (2048, 2048, 128), (1025, 256, 128)]:
        tiles = R.model_tiles(M, N)
        assert sorted(tiles) == [(m, n) for m in range(-(-M // 256)) for n in range(N // 256)], (M, N)
    M, N, _ = R.TAIL_GROUP
    for d in ("xcd_remap", "tail_group"):
        tiles = R.model_tiles(M, N, d)
        assert len(set(tiles)) < len(tiles), f"{d}: two workgroups must share a tile at the 15-tile shape"


# ---------------------------------------------------------------------------------------------------------------------------------------
# family E and F
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_alignment_probe_closed_form_and_reach(fmt):
    v, pp = R.align_p_of()
    for ones, top in ((63, 30 if fmt is R.FP8 else 10), (32, 30)):
        p = R.align_probe(fmt, ones)
        assert p.shape == R.ALIGN_SHAPE and R.expect_is_exact(p)
        assert bool((p.expect[p.asserted] == ones).all())
        ad, wd = p.values()
        for i, name in enumerate(R.ALIGN_VARIANTS):
            sel = p.asserted & (v == i)
            assert sorted(set(pp[sel].tolist())) == list(range(top + 1)), (fmt.name, ones, name)
        big = (ad.abs().unsqueeze(1) * wd.abs().unsqueeze(0)).amax(-1)  # the largest |term| of each output: 2^p
        assert torch.equal(big[p.asserted], torch.pow(2.0, pp[p.asserted].double()))
        # a clean kernel model returns `ones` everywhere; largest_exact_p then reports the probe's reach
        assert R.largest_exact_p(R.model_output(p).to(torch.bfloat16), p) == {name: top for name in R.ALIGN_VARIANTS}
        # and an output that loses the ones from p = 14 on is reported as 13
        out = torch.where(pp >= 14, torch.zeros(()).double(), p.expect)
        if top >= 14:
            assert R.largest_exact_p(out, p) == {name: 13 for name in R.ALIGN_VARIANTS}
    for name, pair in R.ALIGN_MEASURED[fmt.name].items():
        assert all(isinstance(x, int) and 0 <= x <= 30 for x in pair), "the record of the alignment measurement"


def test_c_acc_is_twice_the_measured_worst_rounded_up_and_capped():
    assert R.C_ACC_CAP == 2.0 ** -12
    c = R.c_acc()
    assert c == 2.0 ** math.ceil(math.log2(2.0 * R.C_ACC_MEASURED)) or c == R.C_ACC_CAP
    assert c <= R.C_ACC_CAP and 2.0 * R.C_ACC_MEASURED <= c < 4.0 * R.C_ACC_MEASURED or c == R.C_ACC_CAP
    # the measured figure is consistent with the alignment record: the core keeps about 13 bits below the largest product of a block
    assert 2.0 ** -(R.ALIGN_MEASURED["mxfp8"]["same_step"][0] + 3) < R.C_ACC_MEASURED < 2.0 ** -(R.ALIGN_MEASURED["mxfp8"]["same_step"][0] - 1)
    # a dropped 32-element block at K = 16384 is far outside the bar: |a w| of one block is 1 / 512 of sum |a w| = 2^-9 > 2^-13
    assert 32 / 16384 > 4 * c


@pytest.mark.parametrize("fmt", FMT, ids=FMT_IDS)
def test_gaussian_case_is_seeded_and_has_outlier_channels(fmt):
    p = R.gaussian(fmt, R.ODD_KTILES)
    q = R.gaussian(fmt, R.ODD_KTILES)
    assert torch.equal(p.ac, q.ac) and torch.equal(p.ws, q.ws) and not bool(torch.isnan(p.expect).any())
    a, _ = R.gaussian_bf16(R.ODD_KTILES)
    assert float(a[:, 3::97].float().std()) > 10 * float(a[:, 4::97].float().std())
    ref, absum = R.gemm_ref64(*p.values())
    assert torch.equal(ref, p.expect) and bool((absum >= ref.abs()).all())
    assert R.acc_excess(R.bf16_round(ref), p) <= 0.0, "the correctly rounded result is within half an ulp"
    drop = p.values()[0].clone()
    drop[:, 32:64] = 0  # one block of 12 dropped
    assert R.acc_excess(R.bf16_round(drop @ p.values()[1].t()), p) > R.c_acc(), "a dropped block must break the bar"


def test_quantiser_sweeps():
    from tests.norm_rope_ref import all_bf16
    total = 0
    for name, amax in R.QUANT_ANCHORS.items():
        x = R.quant_sweep(name)
        assert x.shape[1] == 32 and x.shape[0] <= 65280
        xf = x.float()
        assert bool((xf.abs().amax(1) == amax).all()), f"{name}: the planted value is not the block's amax"
        assert bool(((xf != 0).sum(1) <= 2).all())
        v = all_bf16()
        want = v[torch.isfinite(v.float()) & (v.float().abs() <= amax)]
        assert x.shape[0] == want.numel()
        total += x.shape[0]
    assert R.quant_sweep("largest").shape[0] == 65280 and R.QUANT_ANCHORS["subnormal"] < 2.0 ** -126 < R.QUANT_ANCHORS["1.0"]
    # the sweeps hold the ties and saturations they are there for: 1.9921875 under amax 1.9921875 (e4m3: 510 -> 448 saturates), and e2m3's 7.75 tie
    q, s = mxfp8_ref.quant_mxfp8_ref(R.quant_sweep("1.9921875"))
    assert int(s[0, 0]) == 127 - 8 and float(q.float().abs().max()) == 448.0
    codes, s6 = mxfp6_ref.quant_mxfp6_codes(R.quant_sweep("1.9921875"))
    assert int(s6[0, 0]) == 127 - 2 and int((codes & 0x1F).max()) == 0x1F


def test_epilogue_references():
    g = torch.Generator().manual_seed(3)
    y = torch.randn(5, 64, generator=g).to(torch.bfloat16)
    gate, res = R.epilogue_operands(5, 64)
    want, (ref, E) = R.epilogue_expect(y, R.EPI_GATED_RESIDUAL, gate[:2], res)
    assert bool(((want.double() - ref).abs() <= 0.5 * R.bf16_ulp(ref) + E).all())
    assert R.epilogue_expect(y, R.EPI_NONE)[0] is y
    none, (ref, E) = R.epilogue_expect(y, R.EPI_GELU)
    assert none is None and bool(((R.gelu_fast32(y.float()).double() - ref).abs() <= 0.5 * R.bf16_ulp(ref) + R.C_GELU * E).all())
    q, s = R.mxout_expect(y)
    assert q.dtype == torch.uint8 and torch.equal(mxfp8_ref.dequant_mxfp8(q.view(torch.float8_e4m3fn), s), mxfp8_ref.fake_quant(y))
