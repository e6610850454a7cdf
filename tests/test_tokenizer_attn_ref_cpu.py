"""CPU: tests/tokenizer_attn_ref.py checks itself - the probes' closed forms, that emulate() (the d = 512 kernel's arithmetic restated in torch)
stays inside every bar tests/test_tokenizer_attn_kernels_gpu.py uses on every probe and shape it runs, that each listed defect is caught by at least
one probe (and that moving the reference point AT the threshold is none), the mixed-rows trace conditions, the Gaussian constant, and the temporal
and row-softmax references against their fp32 restatements."""
import functools
import math

import pytest
import torch

from tests import tokenizer_attn_ref as A
from tests.norm_rope_ref import pow2_ceil


@functools.lru_cache(maxsize=None)
def _probe(kind, F, hw, default_scale=False):
    return A.make(kind, F, hw, A.fp32_scale_log2(A.DEFAULT_SCALE_512) if default_scale else A.SCALE_LOG2_512)


@functools.lru_cache(maxsize=None)
def _ref(kind, F, hw, default_scale=False):
    return A.reference(_probe(kind, F, hw, default_scale), A.DEFAULT_SCALE_512 if default_scale else A.SOFTMAX_SCALE_512)


def test_the_probe_scale_is_a_power_of_two_in_the_exp2_domain():
    c = torch.tensor(A.SOFTMAX_SCALE_512, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)
    assert float(c) == 2.0 ** -5
    assert A.fp32_scale_log2(A.SOFTMAX_SCALE_512) == 2.0 ** -5 and A.MATCH_LOG2_512 == 32.0
    assert A.RESCALE_THR / (A.D * A.SCALE_LOG2_512) == 0.5  # the threshold census' q scale: a match is 512 * 0.5 * 2^-5 = 8.0


@pytest.mark.parametrize("F,hw", [(1, 64), (1, 128), (1, 192), (1, 320), (1, 448), (3, 320), (8, 192), (1, 1088), (16, 192)])
def test_closed_forms(F, hw):
    C = min(512, hw)
    shifts = [A.frame_shift(f) % C for f in range(F)]
    assert len(set(shifts)) == F, "every frame has its own class shift"
    pos = A.census_position(F, hw)
    ref = A.reference(pos)
    want = torch.zeros_like(ref)
    for f in range(F):
        want[f, torch.arange(hw), pos.q_class[f]] = A.v_gain(f)
    assert float((ref - want).abs().max()) < 1e-6
    blk = A.census_block(F, hw)
    assert A.keys_all_owned(blk)
    uni = A.uniform(F, hw)
    cnt = torch.bincount(torch.arange(hw) // C, minlength=A.D).double() / hw
    for f in range(F):
        assert float((A.reference(uni)[f] - A.v_gain(f) * cnt[None, :]).abs().max()) < 1e-12
    thr = A.threshold_census(F, hw)
    sc = torch.einsum("fid,fjd->fij", thr.q, thr.k) * A.SCALE_LOG2_512
    assert set(sc.unique().tolist()) <= {0.0, 8.0} and bool((sc.max(dim=-1).values == 8.0).all())
    if hw > 64:  # rows whose first tile holds no match: their reference point stays at 0 and the match carries P = 2^8
        late = sc[:, :, :64].max(dim=-1).values == 0.0
        assert bool(late.any()) and bool((~late).any())
        trace = []
        A.emulate(thr, trace=trace)
        assert not bool(torch.stack(trace[1:]).any()), "no row moves its reference point on a jump of exactly 8"


@pytest.mark.parametrize("F,hw,kinds", A.PLAN_512)
def test_the_emulation_meets_every_bar(F, hw, kinds):
    """... and so does the emulation that moves AT the threshold (NOT_A_DEFECT): `>=` in place of `>` is no defect, P stays <= 2^8."""
    worst = {}
    for kind in kinds:
        p, ref = _probe(kind, F, hw), _ref(kind, F, hw)
        for defect in (None, A.NOT_A_DEFECT):
            out = A.emulate(p, defect=defect)
            ok, rel, small = A.out_errors(out, ref, p.rel)
            assert ok, f"{p.name} F={F} hw={hw} {defect}: {A.first_bad512(out, ref, p.rel)}"
            worst[p.rel] = max(worst.get(p.rel, 0.0), rel)
    print(f"[d512 emulation] F={F} hw={hw}: worst relative error per bar {worst}")


@pytest.mark.parametrize("F,hw,kinds", A.PLAN_512_DEFAULT_SCALE)
def test_the_emulation_meets_the_bar_at_the_default_scale(F, hw, kinds):
    worst = 0.0
    for kind in kinds:
        p, ref = _probe(kind, F, hw, True), _ref(kind, F, hw, True)
        out = A.emulate(p, softmax_scale=A.DEFAULT_SCALE_512)
        ok, rel, _ = A.out_errors(out, ref, A.REL_BF16)
        assert ok, f"{p.name} F={F} hw={hw}: {A.first_bad512(out, ref, A.REL_BF16)}"
        worst = max(worst, rel)
    print(f"[d512 emulation, default scale] F={F} hw={hw}: worst relative error {worst:.3e} of {A.REL_BF16:.3e}")


def test_the_staircase_bar_carries_over_from_d128():
    """tests/test_attn_probes_gpu.py reports 6.5e-3 of 7.8e-3 for d = 128 (no-max form); here the reference point follows the staircase, all 64 keys
    of a tile still share one P, and the emulation's worst staircase figure over every shape of the GPU plan stays under 2^-7."""
    worst = 0.0
    for F, hw, kinds in A.PLAN_512 + A.PLAN_512_DEFAULT_SCALE:
        dflt = (F, hw, kinds) in A.PLAN_512_DEFAULT_SCALE
        for kind in kinds:
            if isinstance(kind, str):
                continue
            p = _probe(kind, F, hw, dflt)
            out = A.emulate(p, softmax_scale=A.DEFAULT_SCALE_512 if dflt else A.SOFTMAX_SCALE_512)
            worst = max(worst, A.out_errors(out, _ref(kind, F, hw, dflt), A.REL_BF16)[1])
    print(f"[d512 emulation] worst staircase relative error {worst:.3e} of {A.REL_BF16:.3e}")
    assert 0.0 < worst <= A.REL_BF16


def _caught(defect):
    hits = []
    for F, hw, kinds in A.PLAN_512[:2] + ((1, 1088, A.ALL_KINDS),):
        for kind in kinds:
            p = _probe(kind, F, hw)
            if not A.out_errors(A.emulate(p, defect=defect), _ref(kind, F, hw), p.rel)[0]:
                hits.append(f"{p.name} ({F}, {hw})")
    return hits


@pytest.mark.parametrize("defect", A.DEFECTS)
def test_every_defect_is_caught(defect):
    hits = _caught(defect)
    print(f"[d512 defects] {defect}: caught by {len(hits)} probes, e.g. {hits[:4]}")
    assert hits, f"no probe sees {defect}"
    expected = {"drop_key": "census-block", "swap_vt_cols": "census-position", "skip_rescale_row": "staircase step 12 asc", "other_block_factor": "mixed rows",
                "next_frame_vt": "census", "ragged_rows_unwritten": "uniform"}[defect]
    assert any(h.startswith(expected) for h in hits), (defect, hits)


def test_moving_at_the_threshold_is_not_a_defect():
    assert _caught(A.NOT_A_DEFECT) == []


@pytest.mark.parametrize("F,hw", [(8, 192), (3, 320), (1, 1088)])
def test_mixed_rows_trace(F, hw):
    """In some tile (after the first) some rows of one 32-row group move their reference point while others of that group do not - the per-row
    factor array - and in some tile one 32-row group moves while another group of the same 128-row block does not - the per-block flags."""
    within, across = False, False
    for step, desc in A.MIXED_STAIRS:
        trace = []
        A.emulate(_probe(("mixed", step, desc), F, hw), trace=trace)
        for mv in trace[1:]:
            for b0 in range(0, hw, A.QB):
                groups = [mv[:, g0:g0 + A.GROUP] for g0 in range(b0, min(b0 + A.QB, hw), A.GROUP)]
                anym = [bool(g.any()) for g in groups]
                within |= any(bool(g.any()) and not bool(g.all()) for g in groups)
                across |= any(anym) and not all(anym)
    assert within and across


def test_gaussian_constant():
    """C_GAUSS = 2 x the emulation's worst (err - 0.5 ulp) / E on the GPU test's own inputs, rounded up to a power of two"""
    worst = -math.inf
    for F, hw in A.GAUSS_SHAPES:
        p = A.gaussian(F, hw)
        ref, absum = A.reference(p, A.DEFAULT_SCALE_512, with_abs=True)
        w = A.gauss_excess(A.emulate(p, softmax_scale=A.DEFAULT_SCALE_512), ref, absum)
        print(f"[d512 gaussian] F={F} hw={hw}: emulation's worst (err - 0.5 ulp) / E = {w:.4f}")
        worst = max(worst, w)
    assert worst > 0 and A.C_GAUSS == pow2_ceil(2.0 * worst), (worst, A.C_GAUSS)


# ---- temporal ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,HW,C", A.TEMPORAL_SHAPES + ((16, 6, 512),))
def test_temporal_probes(T, HW, C):
    margins = []
    for scale in A.temporal_scales(C):
        for kind in A.TEMPORAL_KINDS:
            q, k, v = A.temporal_probe(kind, T, HW, C)
            assert A.temporal_scores_exact(q, k)
            ref, _absum, s, w = A.temporal_reference(q, k, v, scale, detail=True)
            margins.append(A.tie_margin(w))
            if kind != "uniform" and HW > 1:  # a pixel mix-up shows: neighbouring pixels carry different classes
                assert not torch.equal(q[:, 0], q[:, 1])
            if kind == "causality":
                future = torch.arange(C)[None, :] > torch.arange(T)[:, None]  # [T, C]
                assert bool((ref[future[:, None, :].expand(T, HW, C)] == 0).all())
                assert float((ref.sum(-1) - 1).abs().max()) <= T * 2.0 ** -9
                if T > A.TEMPORAL_PERIOD:  # the weight sits on the frames congruent to the query's
                    ti = T - 1
                    assert bool((ref[ti, :, ti % A.TEMPORAL_PERIOD] > ref[ti, :, (ti + 1) % A.TEMPORAL_PERIOD]).all())
            if kind == "uniform":
                want = torch.cumsum(v, 0) / torch.arange(1, T + 1, dtype=torch.float64)[:, None, None]
                assert float((ref - want).abs().max()) <= 2.0 ** -8 * float(v.abs().max())
            out = A.temporal_fp32(q, k, v, scale)
            assert bool(((out.double() - ref).abs() <= A.temporal_bar(ref)).all()), (kind, scale)
    print(f"[temporal probes] T={T} HW={HW} C={C}: smallest distance of a weight from a bf16 tie {min(margins):.4f} ulp")
    assert min(margins) > 2.0 ** -10, "a probe weight sits on a bf16 rounding tie: an fp32 softmax may round it either way"


def test_temporal_gaussian_restatement():
    T, HW, C = A.TEMPORAL_GAUSS
    q, k, v = A.temporal_gaussian(T, HW, C)
    scale = float(C) ** -0.5
    ref, absum, s, _w = A.temporal_reference(q, k, v, scale, detail=True)
    share, ok = A.temporal_outliers(A.temporal_fp32(q, k, v, scale), ref, absum, s, scale)
    print(f"[temporal gaussian] T={T} HW={HW} C={C}: fp32 restatement's share of elements outside 0.5 ulp + 2^-16 |ref|: {share:.3e}")
    assert ok and 2e-5 <= share <= 5e-4  # (the GPU bar, min(10 x this, 1e-3), means something only while this is neither 0 nor near 1e-3)


# ---- row softmax -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(A.SOFTMAX_CASES)))
def test_softmax_reference_and_restatement(i):
    rows, n, ld, off = A.SOFTMAX_CASES[i]
    x, names = A.softmax_rows_input(rows, n, first=i)
    ref = A.softmax_reference(x, A.SOFTMAX_SCALE_ROWS)
    assert float((ref.sum(-1) - 1).abs().max()) < 1e-12
    for r, name in enumerate(names):
        if name == "all-equal":
            assert float((ref[r] - 1.0 / n).abs().max()) < 1e-15
        if name == "minus-inf" and n >= 2:
            assert int((ref[r] == 0).sum()) == 1
        if name == "dominant" and n >= 2:
            assert float(ref[r].max()) >= 1 - n * 1e-25
    out = A.softmax_fp32(x, A.SOFTMAX_SCALE_ROWS)
    assert bool(((out.double() - ref).abs() <= A.softmax_bar(ref)).all())
    assert bool(((out.double().sum(-1) - 1).abs() <= n * 2.0 ** -9 * ref.max(dim=-1).values).all())
    assert ld >= n and (off == 0 or A.softmax_reg_path(n, ld, 0))  # an offset base is what takes an otherwise register-path case to the streaming one


def test_all_five_row_contents_reach_both_softmax_paths():
    seen = {True: set(), False: set()}
    for i, (rows, n, ld, off) in enumerate(A.SOFTMAX_CASES):
        seen[A.softmax_reg_path(n, ld, 2 * off)] |= set(A.softmax_rows_input(rows, n, first=i)[1])
    assert seen[True] == seen[False] == set(A.SOFTMAX_CONTENTS)
