"""GPU: every attention kernel against exact fp64 probes, element by element (probes, references and bars: tests/attn_probe_ref.py; their own
checks and the proof that they have teeth: tests/test_attn_probe_ref_cpu.py).

Every launch passes tests/attn_probe_ref.py's SOFTMAX_SCALE, whose exp2-domain value is exactly 2^-3 (its docstring: most kernels round Q * scale to
bf16, which at 1 / sqrt(128) shifts every probe logit by +0.323 % and the LSE by 0.1055 - measured here - while at a power of two it is exact);
family 1b runs the default scale and holds every kernel to the exact function or to that one rounding of it.

Families: (1) ops.flash_attn with every attn_variant 1..11, bf16 and partial outputs, LSE, ops.attn_merge of two and three key parts; (2) segmented
V^T; (3) the cross form (kv_dense, in-kernel Q norm); (4) the no-max kernels (ops.self_attn_bounded, 32x32x16 and 16x16x32); (5) carry / kv_skip /
launch chains on variants 4 and 11 through both entries; (6) the two frame-window entries, no-max and running-max; (7) the range-table entry
(ops.self_attn_ranges), no-max and running-max, with the probes at 64 classes so that every (head, query block, tile) triple of a launch owns an
output element (shapes, tables and probes: R.range_shape; every launch made twice, bit for bit). Every launch's kernel name is asserted, so no
family can silently re-run another one's kernel.

Buffers: q is a column view of a wider buffer; K is a column view of a NaN-guarded buffer whose guard rows sit directly behind key Skv - 1; every
bf16 output (and the fp32 outputs of the carry entry) is a NaN-guarded payload, checked with assert_only_payload_written after the launch.

Bars (every element is checked, no tolerated outliers).
 * elements with ref >= 2^-20: |out - ref| <= 2^-7 ref. bf16 rounds to nearest with 8 significant bits, at most 2^-9 of the binade's upper end; the
   rounding of P (l is summed from the unrounded P) and the rounding of the output add, and the factor 2 covers the hardware exp2 and reciprocal.
   On the staircase all 64 keys of a tile share ONE P, so the rounding of P does not average out inside a column: the CPU emulation reaches
   6.5e-3 of the 7.8e-3 there (no-max form, step 12) and at most 3.9e-3 elsewhere.
   Elements with ref < 2^-20: |out| <= 2^-18. fp32 partial outputs have no output rounding: 2^-8.
 * running-max kernels on the census and uniform probes: P is exactly 1, only the final rounding is left: 2^-8.
 * LSE: |lse - fp64 logsumexp * log2 e| <= 1e-4, the bar of tests/test_attn_bounded_gpu.py; uniform probe: |2^lse - Skv| <= 0.25.
 * the staircase at step 12 needs a bound of 12 (tiles - 1) in the log2 domain: the no-max forms run it where that is within their limit of 60
   (an understated bound is a caller error), the running-max forms at every length.

Measured on an MI355X (the tests print these per case): MEASURED below; the whole file takes about 22 s, family 7 about 3 s of it (its five
cases 0.3 to 0.9 s each; every case of it passed on the first run, so the (1, 8) run of shape (b) stays). At the default scale (family 1b) the
partial launches of the folding kernels write an LSE 0.1055 (census) to 1.319 (staircase, step 12, 2 240 keys) above the fp64 value of the inputs
and agree with the fp64 value behind the fold to 1.5e-5; family 1b's docstring records the kernel defect it found."""
import functools
import math

import pytest
import torch

from tests import attn_probe_ref as R
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

# Largest figures over all cases of a family on an MI355X: (relative element error where ref >= 2^-20, |LSE - fp64|).
MEASURED = {
    "1 flash_attn (variants 1..11, merges)": (2.722e-03, 1.395e-05),
    "2 segmented V^T": (1.953e-03, None),
    "3 cross": (1.190e-07, None),
    "4 no-max (32x32x16 and 16x16x32)": (4.345e-03, 2.927e-06),
    "5 carry / kv_skip / chains": (3.663e-03, 1.311e-06),
    "6 window": (1.953e-03, None),
    "6 window cp": (1.953e-03, None),
    "7 ranges": (4.883e-03, None),  # (the no-max form, bar 2^-7; in every one of the five cases)
}

HD = R.HD
SKV_ALL = (64, 128, 192, 256, 320, 449, 2209, 2240)
SKV_NM = (64, 128, 192, 256, 320, 2240)
SQS = (64, 200, 300)
SQ_ONCE, SQ_ONCE_AT = 513, (320, 2, 3)  # two full query blocks and a one-row third: run once, at (Skv, B, H) = (320, 2, 3)
BHS = ((1, 8), (2, 3))
STAIRS = ((0.5, False), (0.5, True), (12.0, False), (12.0, True))
NM, W4C = "flash_attn_fwd_w4b_nm_kernel<true>", "flash_attn_fwd_w4c_nm_kernel"
NM_WIN, MAX_WIN = "flash_attn_fwd_w4b_nm_win_kernel<true>", "flash_attn_fwd_w4b_win_kernel<true>"
MAX_DENSE = "flash_attn_fwd_w4b_kernel<true>"
NM_RNG, MAX_RNG = "flash_attn_fwd_w4b_nm_rng_kernel<true>", "flash_attn_fwd_w4b_rng_kernel<true>"
WINDOWS = ((64, 768), (64, 640), (128, 768), (128, 640), (192, 768), (192, 576))
WS = ((0, 0), (1, 0), (0, 1), (1, 2))


def _dev():
    return torch.device("cuda:0")


def _lib():
    from gen3c_amd import _lib
    return _lib.load()


class Case:
    """Device operands of one probe, built once and never written: q (column view of a wider buffer), k (column view of a NaN-guarded buffer), v,
    plain V^T, and the fp64 reference / LSE under `mask`."""

    def __init__(self, p, mask=None, k_rows=None, zero_tail_from=None):
        from gen3c_amd import ops
        self.p, self.B, self.H, self.Sq, self.Skv = p, p.B, p.H, p.Sq, p.Skv
        D = p.H * HD
        self.D = D
        bf = torch.bfloat16
        qbuf = torch.full((p.Sq * p.B, 2 * D), 1.5, dtype=bf, device=_dev())
        qbuf[:, :D] = R.flat(p.q).to(bf)
        self.q = qbuf[:, :D]
        kk, vv = p.k, p.v
        if zero_tail_from is not None:  # the cross form's all-zero tail: K rows and V^T columns
            kk, vv = kk.clone(), vv.clone()
            kk[zero_tail_from:] = 0
            vv[zero_tail_from:] = 0
            p = R.Probe(p.name, p.q, kk, vv, None, None)
        if k_rows is not None:  # a compact buffer: these keys only, in this order
            kk, vv = kk[k_rows], vv[k_rows]
        n = kk.shape[0]
        self.kg = Guarded(n * p.B, 2 * D, data=torch.cat([torch.full((n * p.B, D), -2.5, dtype=bf), R.flat(kk).to(bf)], dim=1))
        self.k = self.kg.payload[:, D:]
        self.v = R.flat(vv).to(bf).to(_dev())
        self.n_keys = n
        self.vt = ops.transpose_v(self.v, n, p.B, p.H)
        assert not self.q.is_contiguous() and not self.k.is_contiguous()
        ref, lse = R.reference(p, mask, check_leak=zero_tail_from is None)
        self.ref, self.lse = ref.to(_dev()), lse.to(_dev())

    def out(self):
        return Guarded(self.Sq * self.B, self.D, ld=self.D + 64)

    def out32(self):
        return R.Guarded32(self.Sq * self.B, self.D, ld=self.D + 64)

    def key_rows(self, s0, s1):
        return slice(s0 * self.B, s1 * self.B)

    def vt_of(self, s0, s1):
        from gen3c_amd import ops
        return ops.transpose_v(self.v[self.key_rows(s0, s1)], s1 - s0, self.B, self.H)


PROBES = {"census-position": R.census_position, "census-block": R.census_block, "uniform": R.uniform}


@functools.lru_cache(maxsize=None)
def _case(kind, Sq, Skv, B, H):
    if kind in PROBES:
        return Case(PROBES[kind](Sq, Skv, B, H))
    step, desc = kind
    return Case(R.staircase(Sq, Skv, B, H, step, desc))


KINDS = tuple(PROBES) + STAIRS


def _scaled(name):
    """the ops entry `name` at the probes' softmax scale (tests/attn_probe_ref.py: why it is a power of two in the exp2 domain)"""
    def call(*a, **kw):
        from gen3c_amd import ops
        kw.setdefault("softmax_scale", R.SOFTMAX_SCALE)
        return getattr(ops, name)(*a, **kw)
    return call


_flash, _bounded, _window, _window_cp = (_scaled(n) for n in ("flash_attn", "self_attn_bounded", "self_attn_window", "self_attn_window_cp"))


def _launch(f):
    """(result, kernel names of the attention launches f made)"""
    from gen3c_amd import ops
    ops.enable_kernel_timers(True)
    try:
        res = f()
        names = [m["kernel"] for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    finally:
        ops.enable_kernel_timers(False)
    return res, names


class Stats:
    def __init__(self, family):
        self.family, self.rel, self.lse, self.n, self.fails = family, 0.0, 0.0, 0, []

    def check_out(self, tag, c, out2d, rel, ref=None):
        ref = c.ref if ref is None else ref
        o = R.unflat(out2d, c.B, c.H)
        ok, relmax, _small = R.out_errors(o, ref, rel)
        self.rel, self.n = max(self.rel, relmax), self.n + 1
        if not ok:
            self.fails.append(f"{tag}: bar {rel:.3e}, worst relative error {relmax:.3e}; {R.first_bad(o, ref, rel)}")

    def check_lse(self, tag, c, lse, ref=None):
        ref = c.lse if ref is None else ref
        err = float((lse.double() - ref).abs().max())
        self.lse = max(self.lse, err)
        if not err <= R.LSE_ABS:
            self.fails.append(f"{tag}: |LSE - fp64| {err:.3e} above {R.LSE_ABS}")
        if c.p.name == "uniform":
            d = float((torch.exp2(lse.double()) - torch.exp2(ref)).abs().max())
            if not d <= R.UNIFORM_L_ABS:
                self.fails.append(f"{tag}: |2^lse - keys| {d:.3e} above {R.UNIFORM_L_ABS}")

    def report(self, what):
        """prints the case's figures, then fails with EVERY check of the case that missed its bar (all checks run first: one miss does not hide the next)"""
        print(f"[attn probes {self.family}] {what}: {self.n} outputs, max relative element error {self.rel:.3e}, max |LSE - fp64| {self.lse:.3e}")
        assert not self.fails, f"{len(self.fails)} checks failed:\n" + "\n".join(self.fails)


def _sqs(Skv, B, H):
    return SQS + ((SQ_ONCE,) if (Skv, B, H) == SQ_ONCE_AT else ())


def _rel_for(c, running_max):
    return R.REL_EXACT_P if (running_max and not c.p.name.startswith("staircase")) else R.REL_BF16


def _splits(Skv, parts):
    nt = (Skv + 63) // 64
    if nt < parts:
        return None
    cuts = [0, 64 * max(1, nt // 2), Skv] if parts == 2 else [0, 64, 64 * (nt - 1), Skv]
    return list(zip(cuts[:-1], cuts[1:]))


def _partial_name(lib, Sq, Skv, B, H, variant):
    """kernel of a partial=True launch: the bf16 launch's, except that w4 (9, and 10 / 11 on ragged keys) has no partial epilogue and runs as 4"""
    name = lib.g3_flash_attn_kernel_name_ex(Sq, Skv, B, H, variant).decode()
    return lib.g3_flash_attn_kernel_name_ex(Sq, Skv, B, H, 4).decode() if "w4_kernel" in name else name


# ---- 1. ops.flash_attn, every variant ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H", BHS)
@pytest.mark.parametrize("Skv", SKV_ALL)
@pytest.mark.parametrize("variant", range(1, 12))
def test_flash_attn_every_variant(variant, Skv, B, H):
    from gen3c_amd import ops
    st = Stats("1 flash_attn")
    lib = _lib()
    for Sq in _sqs(Skv, B, H):
        want = lib.g3_flash_attn_kernel_name_ex(Sq, Skv, B, H, variant).decode()
        if variant >= 10 and Skv % 64:  # ragged keys: w4b resolves to w4 (9)
            assert want == lib.g3_flash_attn_kernel_name_ex(Sq, Skv, B, H, 9).decode() and "w4_kernel" in want
        for kind in KINDS:
            c = _case(kind, Sq, Skv, B, H)
            tag = f"flash_attn variant {variant} {c.p.name} Sq={Sq} Skv={Skv} B={B} H={H}"
            o = c.out()
            _, names = _launch(lambda: _flash(c.q, c.k, c.vt, Sq, Skv, B, H, out=o.payload, variant=variant))
            assert names == [want], (tag, names, want)
            o.assert_only_payload_written(tag)
            st.check_out(tag, c, o.payload, _rel_for(c, True))
            if variant < 3:  # no partial epilogue in the 64-bit-addressing kernels
                continue
            (o32, lse), names = _launch(lambda: _flash(c.q, c.k, c.vt, Sq, Skv, B, H, variant=variant, partial=True))
            assert names == [_partial_name(lib, Sq, Skv, B, H, variant)], (tag, names)
            st.check_out(tag + " partial", c, o32, R.REL_EXACT_P)
            st.check_lse(tag + " partial", c, lse)
        if variant >= 3:  # attn_merge of two and of three disjoint key parts against the one-call census
            c = _case("census-block", Sq, Skv, B, H)
            for n_parts in (2, 3):
                cuts = _splits(Skv, n_parts)
                if cuts is None:
                    continue
                parts, names = _launch(lambda: [_flash(c.q, c.k[c.key_rows(s0, s1)], c.vt_of(s0, s1), Sq, s1 - s0, B, H, variant=variant, partial=True)
                                                for s0, s1 in cuts])
                assert names == [_partial_name(lib, Sq, s1 - s0, B, H, variant) for s0, s1 in cuts], (variant, Sq, Skv, cuts, names)
                o = c.out()
                ops.attn_merge(parts, Sq, B, H, out=o.payload)
                tag = f"attn_merge of {n_parts} parts {cuts} variant {variant} Sq={Sq} Skv={Skv} B={B} H={H}"
                o.assert_only_payload_written(tag)
                st.check_out(tag, c, o.payload, R.REL_BF16)
    st.report(f"variant {variant} Skv={Skv} B={B} H={H}")


@functools.lru_cache(maxsize=None)
def _default_scale_case(kind, Sq, Skv, B, H):
    """(case, {False: (ref, lse) of the inputs, True: (ref, lse) of the inputs behind the fold's one rounding}) at the default scale 1 / sqrt(128)"""
    p = R.census_block(Sq, Skv, B, H) if kind == "census-block" else R.staircase(Sq, Skv, B, H, *kind, scale_log2=R.fp32_scale_log2(R.DEFAULT_SCALE))
    refs = {fold: tuple(t.to(_dev()) for t in R.reference(p, softmax_scale=R.DEFAULT_SCALE, fold_q=fold)) for fold in (False, True)}
    return Case(p), refs


@pytest.mark.parametrize("variant", range(1, 12))
def test_flash_attn_default_scale_is_exact_or_one_rounding_of_the_scaled_q(variant):
    """At the default scale the kernels that fold the scale into Q see bf16(q * scale * log2 e) (tests/attn_probe_ref.py). The bf16-output launches
    of a variant, and its partial launches (which may be another kernel), must each meet every bar against the fp64 softmax of the inputs or - all
    of them alike - against the fp64 softmax of those once-rounded inputs: the one documented rounding and nothing else (an LSE off by any other
    constant matches neither). The bars are the module's: every flash_attn kernel keeps a running maximum, under either reference every matching
    census logit is the row's exact maximum (an exact multiple of 2^-9) and every jump of the maximum is 32.65 or 32.75, far above the kernels'
    deferred-rescale threshold of 8, so P == 1 and the census is held to 2^-8. Every launch is made twice: the kernels have no atomics and no
    order-dependent sums, so the two results must be equal bit for bit.

    What this test found, now fixed in csrc/attention.hip (row_max of flash_attn_fwd_v3_kernel): the inline-asm v_max3 chain was scheduled two
    instructions behind the last QK^T MFMA of a key block without the wait states a VALU read of an MFMA result needs, and read scores 0, 1, 2, 4 of
    the block one accumulation step short (28.66 for 32.75). In the folded kernel <*, 6, 8, true> the row then kept a reference point 4.09 below
    its maximum - under the deferred-rescale threshold, so for good - and P = 2^4.09375 = 17.074 rounded to bf16 17.125: 27 .. 45 of 1 200 rows,
    others in every launch, 0.2973 % high in every column (bf16 census 4.395e-3 against the bar of 3.906e-3, LSE exact), two launches unequal.
    At the probes' scale P = 2^4 is bf16-exact, so only this test could see it."""
    Sq, B, H = 200, 2, 3
    lib = _lib()
    for Skv in (320, 2240):
        stats = {(fold, part): Stats(f"1b default scale, {'partial' if part else 'bf16'} launches, reference {'behind the fold' if fold else 'of the inputs'}")
                 for fold in (False, True) for part in (False, True)}
        unequal = []
        for kind in ("census-block",) + STAIRS:
            c, refs = _default_scale_case(kind, Sq, Skv, B, H)
            tag = f"flash_attn variant {variant} {c.p.name} Sq={Sq} Skv={Skv} default scale"
            o, o_again = c.out(), c.out()
            _, names = _launch(lambda: [_flash(c.q, c.k, c.vt, Sq, Skv, B, H, out=g.payload, variant=variant, softmax_scale=None) for g in (o, o_again)])
            assert names == [lib.g3_flash_attn_kernel_name_ex(Sq, Skv, B, H, variant).decode()] * 2, (tag, names)
            o.assert_only_payload_written(tag)
            if not torch.equal(o.payload, o_again.payload):
                unequal.append(tag)
            if variant >= 3:
                ((o32, lse), (o32_again, lse_again)), names = _launch(
                    lambda: [_flash(c.q, c.k, c.vt, Sq, Skv, B, H, variant=variant, partial=True, softmax_scale=None) for _ in range(2)])
                assert names == [_partial_name(lib, Sq, Skv, B, H, variant)] * 2, (tag, names)
                if not (torch.equal(o32, o32_again) and torch.equal(lse, lse_again)):
                    unequal.append(tag + " partial")
            for fold in (False, True):
                ref, ref_lse = refs[fold]
                stats[fold, False].check_out(tag, c, o.payload, _rel_for(c, True), ref=ref)
                if variant >= 3:
                    stats[fold, True].check_out(tag + " partial", c, o32, R.REL_EXACT_P, ref=ref)
                    stats[fold, True].check_lse(tag + " partial", c, lse, ref=ref_lse)
        for (fold, part), st in stats.items():
            if st.n:
                print(f"[attn probes {st.family}] variant {variant} Skv={Skv}: {len(st.fails)} checks missed, max relative element error {st.rel:.3e}, "
                      f"max |LSE - fp64| {st.lse:.3e}")
        print(f"[attn probes 1b default scale] variant {variant} Skv={Skv}: launches that do not repeat bit for bit: {unequal}")
        for part in (False, True):
            assert not stats[False, part].fails or not stats[True, part].fails, (
                f"variant {variant} Skv={Skv} {'partial' if part else 'bf16'} launches: neither the exact function nor its fold:\n" +
                "\n".join(stats[False, part].fails[:6] + stats[True, part].fails[:6]))
        assert not unequal, f"variant {variant} Skv={Skv}: two launches on the same inputs differ: {unequal}"


# ---- 2. segmented V^T ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H", BHS)
@pytest.mark.parametrize("n_seg,L", [(4, 64), (3, 128)])
def test_segmented_vt(n_seg, L, B, H):
    from gen3c_amd import ops
    st = Stats("2 segmented V^T")
    Skv = n_seg * L
    for Sq in SQS:
        c = _case("census-block", Sq, Skv, B, H)
        vseg = torch.stack([c.vt_of(r * L, (r + 1) * L) for r in range(n_seg)])
        calls = [("flash_attn variant 4", lambda o: _flash(c.q, c.k, vseg, Sq, Skv, B, H, out=o, variant=4), "v3_kernel", True),
                 ("flash_attn variant 11", lambda o: _flash(c.q, c.k, vseg, Sq, Skv, B, H, out=o, variant=11), MAX_DENSE, True),
                 ("self_attn_bounded variant 11", lambda o: _bounded(c.q, c.k, vseg, Sq, Skv, B, H, R.BOUND_NATS, out=o, variant=11), NM, False)]
        for what, f, kernel, running_max in calls:
            tag = f"{what} {n_seg} x {L} keys Sq={Sq} B={B} H={H}"
            o = c.out()
            _, names = _launch(lambda: f(o.payload))
            assert len(names) == 1 and kernel in names[0], (tag, names)
            o.assert_only_payload_written(tag)
            st.check_out(tag, c, o.payload, _rel_for(c, running_max))
    st.report(f"{n_seg} x {L} B={B} H={H}")


# ---- 3. the cross form -----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cross_case(kind, Sq, Skv, B, H, kv_dense, q_norm):
    p = PROBES[kind](Sq, Skv, B, H)
    c = Case(p, zero_tail_from=kv_dense or None)
    if q_norm:  # the kernel reads 3 Hd[...] and normalises it: rms 3, times w = 2 -> the reference's 2 Hd[...]
        qbuf = torch.full((Sq * B, 2 * c.D), 1.5, dtype=torch.bfloat16, device=_dev())
        qbuf[:, :c.D] = R.flat(p.q * 1.5).to(torch.bfloat16)
        c.q = qbuf[:, :c.D]
    return c


@pytest.mark.parametrize("B,H", BHS)
@pytest.mark.parametrize("Skv,kv_dense", [(256, 64), (256, 192), (512, 64), (512, 192)])
def test_cross_form(Skv, kv_dense, B, H):
    from gen3c_amd import ops
    st = Stats("3 cross")
    w = torch.full((HD,), 2.0, dtype=torch.bfloat16, device=_dev())
    for Sq in SQS:
        runs = [("uniform", kv_dense, False), ("census-position", 0, True), ("census-block", 0, True), ("census-position", kv_dense, True),
                ("census-block", kv_dense, True), ("census-block", kv_dense, False)]
        for kind, dense, q_norm in runs:
            c = _cross_case(kind, Sq, Skv, B, H, dense, q_norm)
            tag = f"cross {kind} kv_dense={dense} q_norm={q_norm} Sq={Sq} Skv={Skv} B={B} H={H}"
            o = c.out()
            _, names = _launch(lambda: _flash(c.q, c.k, c.vt, Sq, Skv, B, H, out=o.payload, kv_dense=dense, q_norm_weight=w if q_norm else None,
                                                      q_norm_eps=1e-6))
            assert len(names) == 1 and "v3_kernel" in names[0], (tag, names)
            o.assert_only_payload_written(tag)
            st.check_out(tag, c, o.payload, R.REL_EXACT_P)
    st.report(f"Skv={Skv} kv_dense={kv_dense} B={B} H={H}")


# ---- 4. the no-max kernels -------------------------------------------------------------------------------------------------------------------------------

def _stair_bound(kind, Skv):
    """natural-units bound of a probe for the no-max forms, or None where the staircase is beyond their range"""
    if kind in PROBES:
        return R.BOUND_NATS
    b = R.staircase_bound_nats(kind[0], Skv)
    return b if b * R.LOG2E <= 60.0 else None


@pytest.mark.parametrize("B,H", BHS)
@pytest.mark.parametrize("Skv", SKV_NM)
@pytest.mark.parametrize("mfma16", [False, True])
def test_self_attn_bounded(mfma16, Skv, B, H):
    from gen3c_amd import ops
    st = Stats("4 no-max")
    lib = _lib()
    kernel = W4C if mfma16 else NM
    for Sq in _sqs(Skv, B, H):
        for kind in KINDS:
            bound = _stair_bound(kind, Skv)
            if bound is None:
                continue
            name_of = lib.g3_self_attn16_kernel_name if mfma16 else lib.g3_self_attn_kernel_name
            assert name_of(Sq, Skv, B, H, float(bound), 11).decode() == kernel
            c = _case(kind, Sq, Skv, B, H)
            tag = f"self_attn_bounded mfma16={mfma16} {c.p.name} Sq={Sq} Skv={Skv} B={B} H={H}"
            o = c.out()
            _, names = _launch(lambda: _bounded(c.q, c.k, c.vt, Sq, Skv, B, H, bound, out=o.payload, variant=11, mfma16=mfma16))
            assert names == [kernel], (tag, names)
            o.assert_only_payload_written(tag)
            st.check_out(tag, c, o.payload, R.REL_BF16)
            (o32, lse), names = _launch(lambda: _bounded(c.q, c.k, c.vt, Sq, Skv, B, H, bound, variant=11, partial=True, mfma16=mfma16))
            assert names == [NM], (tag, names)  # (a partial output is the 32x32x16 kernel's under either flag)
            st.check_out(tag + " partial", c, o32, R.REL_EXACT_P)
            st.check_lse(tag + " partial", c, lse)
    st.report(f"mfma16={mfma16} Skv={Skv} B={B} H={H}")


# ---- 5. carry / kv_skip / chains -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _chain_case(kind, Sq, L, world, B, H):
    if kind == "census-block":
        return Case(R.census_block(Sq, world * L, B, H, classes=min(128, L)))
    return Case(R.staircase(Sq, world * L, B, H, *kind))


@functools.lru_cache(maxsize=None)
def _skip_ref(Sq, L, world, rank, B, H):
    c = _chain_case("census-block", Sq, L, world, B, H)
    ref, lse = R.reference(c.p, R.skip_mask(Sq, world * L, rank * L, L))
    return ref.to(_dev()), lse.to(_dev())


@pytest.mark.parametrize("B,H", BHS)
@pytest.mark.parametrize("world,L", [(w, L) for w in (2, 3) for L in (64, 128, 256)])
@pytest.mark.parametrize("entry", ["flash_attn", "self_attn_bounded"])
@pytest.mark.parametrize("variant", [4, 11])
def test_carry_skip_and_chains(variant, entry, world, L, B, H):
    from gen3c_amd import ops
    st = Stats("5 carry")
    lib = _lib()
    Sq, Skv = 200, world * L
    bounded = entry == "self_attn_bounded"
    no_max = bounded and variant == 11

    def call(bound, *a, **kw):
        if bounded:
            return _bounded(*a, bound, variant=variant, **kw)
        return _flash(*a, variant=variant, **kw)

    def name(n_keys, bound, cp_form):
        return lib.g3_self_attn_cp_kernel_name(Sq, n_keys, B, H, float(bound if bounded else 0.0), variant, 0, int(cp_form)).decode()

    # one rank's step under context parallelism: the own block as a partial, then ONE carry launch over every other block
    c = _chain_case("census-block", Sq, L, world, B, H)
    bound = R.BOUND_NATS
    skipped_cols = lambda rank: slice(rank * L // c.p.C, (rank + 1) * L // c.p.C)
    for rank in range(world):
        tag = f"{entry} variant {variant} world {world} L {L} rank {rank} B={B} H={H}"
        if rank == 0:
            kk, vv, skip = c.k[c.key_rows(L, Skv)], c.vt_of(L, Skv), None
        elif rank == world - 1:
            kk, vv, skip = c.k[c.key_rows(0, rank * L)], c.vt_of(0, rank * L), None
        else:
            kk, vv, skip = c.k, c.vt, (rank * L, L)
        interior = skip is not None
        # the remote keys alone, as a partial into a guarded fp32 buffer: the skipped block's columns exactly 0, every other key once
        g32 = c.out32()
        (_o, lse), names = _launch(lambda: call(bound, c.q, kk, vv, Sq, Skv - L, B, H, out=g32.payload, partial=True, kv_skip=skip))
        assert names == [name(Skv - L, bound, interior)], (tag, names)
        g32.assert_only_payload_written(tag + " remote part")
        ref, ref_lse = _skip_ref(Sq, L, world, rank, B, H)
        st.check_out(tag + " remote part", c, g32.payload, R.REL_EXACT_P, ref=ref)
        st.check_lse(tag + " remote part", c, lse, ref=ref_lse)
        assert bool((R.unflat(g32.payload, B, H)[..., skipped_cols(rank)] == 0).all()), f"{tag}: a skipped key reached the output"
        # own block, then the carry launch: the whole row
        own32 = c.out32()
        own = call(bound, c.q, c.k[c.key_rows(rank * L, (rank + 1) * L)], c.vt_of(rank * L, (rank + 1) * L), Sq, L, B, H, out=own32.payload, partial=True)
        o = c.out()
        _, names = _launch(lambda: call(bound, c.q, kk, vv, Sq, Skv - L, B, H, out=o.payload, carry=own, kv_skip=skip))
        assert names == [name(Skv - L, bound, True)], (tag, names)
        o.assert_only_payload_written(tag + " carry")
        own32.assert_only_payload_written(tag + " own part")
        st.check_out(tag + " carry", c, o.payload, R.REL_BF16)
    # a chain of `world` launches, one per key block: fp32 -> carry -> ... -> bf16; census and the staircases (a growing and a shrinking reference point)
    for kind in ("census-block",) + STAIRS:
        c = _chain_case(kind, Sq, L, world, B, H)
        bound = R.BOUND_NATS if kind == "census-block" else R.staircase_bound_nats(kind[0], Skv)
        if no_max and bound * R.LOG2E > 60.0:
            continue
        tag = f"{entry} variant {variant} chain of {world} x {L} keys {c.p.name} B={B} H={H}"
        state, bufs = None, []
        for r in range(world):
            last = r == world - 1
            g = c.out() if last else c.out32()
            bufs.append(g)
            res, names = _launch(lambda: call(bound, c.q, c.k[c.key_rows(r * L, (r + 1) * L)], c.vt_of(r * L, (r + 1) * L), Sq, L, B, H, out=g.payload,
                                              partial=not last, carry=state))
            assert names == [name(L, bound, state is not None)], (tag, r, names)
            state = None if last else res
            if not last:
                lse = res[1]
        for r, g in enumerate(bufs):
            g.assert_only_payload_written(f"{tag} launch {r}")
        st.check_out(tag, c, bufs[-1].payload, R.REL_BF16)
        # the state before the last launch is the attention over the first world - 1 blocks: its LSE against fp64
        sub = R.Probe(c.p.name, c.p.q, c.p.k[:(world - 1) * L], c.p.v[:(world - 1) * L], None, None)
        st.check_lse(tag + " state", c, lse, ref=R.reference(sub)[1].to(_dev()))
    st.report(f"{entry} variant {variant} world {world} L {L} B={B} H={H}")


# ---- 6. the frame-window entries -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _win_probe(kind, S, B, H):
    return PROBES[kind](S, S, B, H)


@functools.lru_cache(maxsize=None)
def _win_case(kind, S, B, H, fl, W, s):
    return Case(_win_probe(kind, S, B, H), mask=R.window_mask(S, fl, W, s))


@pytest.mark.parametrize("B,H", BHS)
@pytest.mark.parametrize("fl,S", WINDOWS)
def test_self_attn_window(fl, S, B, H):
    from gen3c_amd import ops
    st = Stats("6 window")
    T = S // fl
    for W, s in WS + ((T - 1, 0),):
        mask = R.window_mask(S, fl, W, s)
        assert torch.equal(mask, ops.window_attn_mask(S, fl, W, s))
        dense = W >= T - 1 or s >= T
        for kind in ("census-position", "census-block"):
            c = _win_case(kind, S, B, H, fl, W, s)
            for bound, kernel, running_max in ((R.BOUND_NATS, NM if dense else NM_WIN, False), (0.0, MAX_DENSE if dense else MAX_WIN, True)):
                tag = f"self_attn_window {kind} fl={fl} S={S} W={W} s={s} bound={bound} B={B} H={H}"
                o = c.out()
                _, names = _launch(lambda: _window(c.q, c.k, c.vt, S, B, H, bound, fl, W, s, out=o.payload))
                assert names == [kernel], (tag, names)
                o.assert_only_payload_written(tag)
                st.check_out(tag, c, o.payload, _rel_for(c, running_max))
    st.report(f"fl={fl} S={S} B={B} H={H}")


@functools.lru_cache(maxsize=None)
def _win_cp_case(kind, S, B, H, fl, W, s, world, r):
    from gen3c_amd import parallel
    T = S // fl
    a, b, cc = parallel.window_halo_plan(T, world, W, s)["buffers"][r]
    p = _win_probe(kind, S, B, H)
    Sl = S // world
    rows = slice(r * Sl, (r + 1) * Sl)
    sub = R.Probe(p.name, p.q[rows].contiguous(), p.k, p.v, p.q_class[rows], p.C)
    mask = R.window_mask(Sl, fl, W, s, q_row0=r * Sl, T_total=T)
    keys = torch.cat([torch.arange(0, a * fl), torch.arange(b * fl, cc * fl)])
    assert bool(mask[:, keys].sum() == mask.sum()), "the plan's buffer holds every attended key"
    return Case(sub, mask=mask, k_rows=keys), (a, b, cc)


@pytest.mark.parametrize("B,H", BHS)
@pytest.mark.parametrize("fl,T,world", [(128, 6, 3), (192, 4, 2), (192, 4, 4), (64, 12, 3), (64, 12, 4)])  # rank rows 256 (aligned), 384, 192, 256, 192
def test_self_attn_window_cp(fl, T, world, B, H):
    from gen3c_amd import ops
    st = Stats("6 window cp")
    S = fl * T
    Sl = S // world
    for W, s in WS:
        for r in range(world):
            assert torch.equal(R.window_mask(Sl, fl, W, s, q_row0=r * Sl, T_total=T), ops.window_attn_mask(Sl, fl, W, s, q_row0=r * Sl, T_total=T))
            for kind in ("census-position", "census-block"):
                c, (a, b, _cc) = _win_cp_case(kind, S, B, H, fl, W, s, world, r)
                for bound, kernel, running_max in ((R.BOUND_NATS, NM_WIN, False), (0.0, MAX_WIN, True)):
                    tag = f"self_attn_window_cp {kind} fl={fl} T={T} world={world} rank={r} W={W} s={s} bound={bound} B={B} H={H}"
                    o = c.out()
                    _, names = _launch(lambda: _window_cp(c.q, c.k, c.vt, Sl, c.n_keys, B, H, bound, fl, T, r * (T // world), a, b, W, s,
                                                                       out=o.payload))
                    assert names == [kernel], (tag, names)
                    o.assert_only_payload_written(tag)
                    st.check_out(tag, c, o.payload, _rel_for(c, running_max))
    st.report(f"fl={fl} T={T} world={world} B={B} H={H}")


# ---- 7. the range-table entry ----------------------------------------------------------------------------------------------------------------------------

_ranges = _scaled("self_attn_ranges")


@functools.lru_cache(maxsize=None)
def _rng_table(name, B, H):
    from gen3c_amd import ops
    sh = R.range_shape(name)
    return ops.attn_range_table(R.pack(sh["lists"], sh["max_ranges"]), sh["S"], head_pattern=list(R.RANGE_HEAD_PATTERNS[B, H]), H=H)


@functools.lru_cache(maxsize=None)
def _rng_case(name, kind, B, H):
    sh = R.range_shape(name)
    return Case(R.range_probe(kind, sh["S"], B, H), mask=R.head_masks(sh["lists"], R.RANGE_HEAD_PATTERNS[B, H], sh["S"]))


@pytest.mark.parametrize("name,B,H", R.range_cases())
def test_self_attn_ranges(name, B, H):
    """Family 7: g3_self_attn_fwd_ranges_bf16 at R.range_shape's shapes (what each is the smallest shape for is a comment there). All probes have 64
    classes, so every 64-key tile holds every class, the census-block V column of a key is its tile, and output element (i, d) is 1 / n iff tile d
    is in the list of row i's block under its head's pattern: every (head, query block, tile) triple of a launch owns an output element of its own.
    (a) also runs the four staircases at (B, H) = (2, 3) - the running-max form all four, the no-max form those within its limit of 60 (the 0.5-step
    pair) - so the reference point moves across range jumps. Every launch is made twice into two guarded outputs which must be equal bit for bit
    (no atomics, no order-dependent sums; the table load is retired before the first LDS-DMA). Measured on an MI355X: every case inside every bar
    on the first run, no kernel defect found; worst relative element error 4.883e-3 (no-max form), the CPU emulation's figure to the digit."""
    from gen3c_amd import ops
    st = Stats("7 ranges")
    sh = R.range_shape(name)
    S, lists, hp = sh["S"], sh["lists"], R.RANGE_HEAD_PATTERNS[B, H]
    table = _rng_table(name, B, H)
    for pat, blocks in enumerate(lists):
        assert torch.equal(R.ranges_mask(blocks, S), ops.ranges_attn_mask(table, S, pattern=pat)), (name, pat)
    assert (table.attended, table.dense) == R.ranges_counts(lists, hp, S)
    kinds = tuple(sh["probes"]) + (STAIRS if sh["stairs"] and (B, H) == R.RANGE_STAIRS_AT else ())
    for kind in kinds:
        c = _rng_case(name, kind, B, H)
        for bound, kernel, running_max in ((_stair_bound(kind, S), NM_RNG, False), (0.0, MAX_RNG, True)):
            if bound is None:  # a staircase beyond the no-max form's range
                continue
            tag = f"self_attn_ranges shape {name} {c.p.name} S={S} bound={bound} B={B} H={H}"
            o, o_again = c.out(), c.out()
            _, names = _launch(lambda: [_ranges(c.q, c.k, c.vt, S, B, H, bound, table, out=g.payload) for g in (o, o_again)])
            assert names == [kernel] * 2, (tag, names)
            o.assert_only_payload_written(tag)
            o_again.assert_only_payload_written(tag + " (second launch)")
            assert torch.equal(o.payload, o_again.payload), f"{tag}: two launches on the same inputs differ"
            st.check_out(tag, c, o.payload, _rel_for(c, running_max))
    st.report(f"shape {name} S={S} B={B} H={H}")
