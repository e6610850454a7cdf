"""CPU: the attention probes of tests/attn_probe_ref.py are what they claim to be, and they have teeth.

 * every probe tensor survives a bf16 round trip bit for bit, the Hadamard rows are orthogonal, all but 1e-6 of a row's weight lies on the keys of
   the query's class, and in the census-block probe every (attended) key of every GPU case owns a nonzero reference element;
 * a clean emulation of the kernels' arithmetic (64-key tiles, fp32 log2-domain scores, running maximum or constant bound, bf16 P, fp32 l from the
   unrounded P, bf16 output, LSE) meets every bar of tests/test_attn_probes_gpu.py at every shape that file runs;
 * each of twenty defects planted into the emulation fails at least one probe;
 * the same defects on Gaussian inputs at 2 209 and 4 160 keys against the rel-L2 < 1e-2 bar of the older attention tests: printed, not gated
   (the list of defects that bar lets through is why the probes exist);
 * the range-table family (family 7 of tests/test_attn_probes_gpu.py) at exactly its shapes, tables and probes (R.range_shape, R.range_probe): the
   probes at 64 classes are exact, leak-free under every head's mask, own every attended key, and census-block's element (i, d) is 1 / n iff tile d
   is in row i's list; the clean emulation meets every bar in both forms and its explicit walk gives the bits of its mask; each of the nine range
   defects (R.RANGE_DEFECTS: another walk) fails a named probe BY ITS OUTPUT, and is reported against the Gaussian rel-L2 bar of 4e-3 that
   tests/test_attn_ranges_gpu.py holds the range kernels to."""
import functools
import math

import pytest
import torch

from tests import attn_probe_ref as R

SKV_ALL = (64, 128, 192, 256, 320, 449, 2209, 2240)
SKV_NM = (64, 128, 192, 256, 320, 2240)
SQS = (64, 200, 300)
SQ_ONCE, SQ_ONCE_AT = 513, (320, 2, 3)  # two full query blocks and a one-row third, once - as tests/test_attn_probes_gpu.py
BHS = ((1, 8), (2, 3))
STAIRS = ((0.5, False), (0.5, True), (12.0, False), (12.0, True))
BOUND_LOG2 = R.BOUND_NATS * R.LOG2E
WINDOWS = ((64, 768), (64, 640), (128, 768), (128, 640), (192, 768), (192, 576))
WS = ((0, 0), (1, 0), (0, 1), (1, 2))


def _probes(Sq, Skv, B, H):
    yield R.census_position(Sq, Skv, B, H)
    yield R.census_block(Sq, Skv, B, H)
    yield R.uniform(Sq, Skv, B, H)
    for step, desc in STAIRS:
        yield R.staircase(Sq, Skv, B, H, step, desc)


def _bound_for(p):
    if p.name.startswith("staircase"):
        step = float(p.name.split()[2])
        return R.staircase_bound_nats(step, p.Skv) * R.LOG2E
    return BOUND_LOG2


def _passes(p, out, lse, ref, ref_lse, rel, check_lse=True):
    ok, _relmax, _small = R.out_errors(out, ref, rel)
    if check_lse:
        ok = ok and float((lse.double() - ref_lse).abs().max()) <= R.LSE_ABS
        if p.name == "uniform":
            ok = ok and float((torch.exp2(lse.double()) - torch.exp2(ref_lse)).abs().max()) <= R.UNIFORM_L_ABS
    return ok


def test_hadamard_rows_are_orthogonal():
    Hd = R.hadamard()
    assert Hd.shape == (128, 128) and bool((Hd.abs() == 1).all())
    assert torch.equal(Hd @ Hd.t(), 128.0 * torch.eye(128, dtype=torch.float64))
    for B, H in BHS:  # a different shift per (batch, head)
        assert len({R.shift(b, h, H) for b in range(B) for h in range(H)}) == B * H
    assert R.MATCH_LOG2 == 32.0 and R.MATCH_LOG2 < BOUND_LOG2 <= 60.0
    assert R.fp32_scale_log2(R.SOFTMAX_SCALE) == 2.0 ** -3  # the kernels' fp32 product: exactly a power of two, so Q * scale stays bf16-exact


@pytest.mark.parametrize("Skv", SKV_ALL)
def test_probes_are_exact_leak_free_and_every_key_is_owned(Skv):
    for B, H in BHS:
        for Sq in SQS + ((SQ_ONCE,) if (Skv, B, H) == SQ_ONCE_AT else ()):
            for p in _probes(Sq, Skv, B, H):  # (the constructor asserts the bf16 round trip)
                for t in (p.q, p.k, p.v):
                    assert torch.equal(t.to(torch.bfloat16).double(), t)
                out, lse = R.reference(p)  # (asserts the leakage)
                assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
                assert float((out.sum(-1) - 1).abs().max()) < 1e-12  # every V row is one-hot: a row of the output sums to 1
            assert R.keys_all_owned(R.census_block(Sq, Skv, B, H)), (Sq, Skv, B, H)


def test_window_and_skip_cases_own_every_attended_key():
    for fl, S in WINDOWS:
        for W, s in WS:
            mask = R.window_mask(S, fl, W, s)
            from gen3c_amd import ops
            assert torch.equal(mask, ops.window_attn_mask(S, fl, W, s, q_rows=R.Q_ROWS))
            assert R.keys_all_owned(R.census_block(S, S, 2, 3), mask), (fl, S, W, s)
            R.reference(R.census_position(S, S, 2, 3), mask)
    for world in (2, 3):
        for L in (64, 128, 256):
            for rank in range(world):
                mask = R.skip_mask(200, world * L, rank * L, L)
                assert R.keys_all_owned(R.census_block(200, world * L, 2, 3, classes=min(128, L)), mask), (world, L, rank)


def test_staircase_masses_are_the_documented_ones():
    out, _ = R.reference(R.staircase(64, 320, 1, 8, 0.5, False))
    row = out[0, 0, 0, :5]
    assert abs(float(row[0]) - 0.089) < 1e-3 and abs(float(row[4]) - 0.356) < 1e-3, row
    out, _ = R.reference(R.staircase(64, 320, 1, 8, 12.0, True))
    assert abs(float(out[0, 0, 0, 0]) - 1.0) < 1e-3 and 3e-15 < float(out[0, 0, 0, 4]) < 4.5e-15


@pytest.mark.parametrize("Skv", SKV_ALL)
def test_clean_emulation_meets_every_bar(Skv):
    worst = dict(rel=0.0, lse=0.0)
    for B, H in BHS:
        for Sq in SQS + ((SQ_ONCE,) if (Skv, B, H) == SQ_ONCE_AT else ()):
            for p in _probes(Sq, Skv, B, H):
                ref, ref_lse = R.reference(p)
                exact_p = not p.name.startswith("staircase")
                forms = [(None, R.REL_EXACT_P if exact_p else R.REL_BF16)]
                if Skv in SKV_NM and (not p.name.startswith("staircase") or _bound_for(p) <= 60.0):
                    forms.append((_bound_for(p), R.REL_BF16))
                for bound, rel in forms:
                    out, lse = R.emulate(p.q, p.k, p.v, bound_log2=bound)
                    assert _passes(p, out, lse, ref, ref_lse, rel), (p.name, Sq, Skv, B, H, bound, R.first_bad(R.unflat(out, B, H), ref, rel))
                    if Sq == 200:  # the scale folded into Q (the w4 / w4b / w4c and folded v3 kernels): exact at the probes' scale, the same bits
                        out_f, lse_f = R.emulate(p.q, p.k, p.v, bound_log2=bound, fold_q=True)
                        assert torch.equal(out_f, out) and torch.equal(lse_f, lse), (p.name, Sq, Skv, B, H, bound)
                    o32, _ = R.emulate(p.q, p.k, p.v, bound_log2=bound, partial=True)
                    assert R.out_errors(o32, ref, R.REL_EXACT_P)[0], (p.name, "fp32 partial", Sq, Skv, B, H, bound)
                    worst["rel"] = max(worst["rel"], R.out_errors(out, ref, rel)[1])
                    worst["lse"] = max(worst["lse"], float((lse.double() - ref_lse).abs().max()))
    print(f"[emulation Skv={Skv}] worst relative element error {worst['rel']:.3e}, worst |LSE - fp64| {worst['lse']:.3e}")


def test_clean_emulation_meets_the_bars_under_masks_and_across_launches():
    B, H = 2, 3
    for fl, S in WINDOWS:
        for W, s in WS:
            mask = R.window_mask(S, fl, W, s)
            for make in (R.census_position, R.census_block):
                p = make(S, S, B, H)
                ref, ref_lse = R.reference(p, mask)
                for bound, rel in ((None, R.REL_EXACT_P), (BOUND_LOG2, R.REL_BF16)):
                    out, lse = R.emulate(p.q, p.k, p.v, mask=mask, bound_log2=bound)
                    assert _passes(p, out, lse, ref, ref_lse, rel), (p.name, fl, S, W, s, bound)
    for world in (2, 3):
        for L in (64, 128, 256):
            Skv = world * L
            probes = [R.census_block(200, Skv, B, H, classes=min(128, L))] + [R.staircase(200, Skv, B, H, step, d) for step, d in STAIRS]
            for p in probes:
                ref, ref_lse = R.reference(p)
                for bound in (None, _bound_for(p)):
                    if bound is not None and bound > 60.0:
                        continue
                    state = None
                    for r in range(world):  # a chain: one launch per key block, each resuming from the state before
                        sl = slice(r * L, (r + 1) * L)
                        state = R.emulate(p.q, p.k[sl], p.v[sl], bound_log2=bound, partial=r < world - 1, carry=state)
                    assert _passes(p, state[0], state[1], ref, ref_lse, R.REL_BF16), (p.name, world, L, bound, R.first_bad(state[0], ref, R.REL_BF16))


def test_why_the_probes_do_not_run_at_the_default_scale():
    """The correction of the closed form's premise, with the emulation to back it: at 1 / sqrt(128) a kernel that rounds q * scale * log2(e) to bf16
    (the fold) shifts EVERY probe logit by +0.323 % - LSE 0.1055 above the fp64 value of the inputs, as measured on the GPU - while it meets every
    bar against the fp64 softmax of the once-rounded inputs, and a kernel that scales in fp32 meets them against the inputs' own."""
    Sq, Skv, B, H = 200, 320, 2, 3
    c32 = R.fp32_scale_log2(R.DEFAULT_SCALE)
    folded = float(torch.tensor(2.0 * c32).to(torch.bfloat16)) / (2.0 * c32)
    assert abs(folded - 1.003233) < 1e-5
    for p in (R.census_block(Sq, Skv, B, H), R.staircase(Sq, Skv, B, H, 12.0, False, scale_log2=c32)):
        refs = {fold: R.reference(p, softmax_scale=R.DEFAULT_SCALE, fold_q=fold) for fold in (False, True)}
        for fold in (False, True):
            out, lse = R.emulate(p.q, p.k, p.v, softmax_scale=R.DEFAULT_SCALE, fold_q=fold)
            assert _passes(p, out, lse, *refs[fold], R.REL_BF16), (p.name, fold)
            assert not _passes(p, out, lse, *refs[not fold], R.REL_BF16), (p.name, fold)
        _out, lse = R.emulate(p.q, p.k, p.v, softmax_scale=R.DEFAULT_SCALE, fold_q=True)
        d = float((lse.double() - refs[False][1]).max())
        print(f"[default scale, folded] {p.name}: LSE - fp64 of the inputs = {d:.4f}")
        if p.name == "census-block":
            assert abs(d - 0.1055) < 2e-4


# ---- range tables: family 7's probes, at its shapes ----------------------------------------------------------------------------------------------------

def _range_kinds(name, B, H):
    sh = R.range_shape(name)
    return tuple(sh["probes"]) + (STAIRS if sh["stairs"] and (B, H) == R.RANGE_STAIRS_AT else ())


def _range_forms(kind, S):
    """(log2-domain bound or None, bar) of the two kernel forms: the rule of tests/test_attn_probes_gpu.py (_rel_for, _stair_bound)"""
    stair = isinstance(kind, tuple)
    forms = [(None, R.REL_BF16 if stair else R.REL_EXACT_P)]
    bound = R.staircase_bound_nats(kind[0], S) * R.LOG2E if stair else BOUND_LOG2
    return forms + ([(bound, R.REL_BF16)] if bound <= 60.0 else [])


@functools.lru_cache(maxsize=None)
def _range_ref(name, B, H, kind):
    """(probe, per-head masks, fp64 reference, LSE): built once, shared, never written"""
    sh = R.range_shape(name)
    p = R.range_probe(kind, sh["S"], B, H)
    masks = R.head_masks(sh["lists"], R.RANGE_HEAD_PATTERNS[B, H], sh["S"])
    return (p, masks) + R.reference(p, masks)  # (asserts the leakage)


@pytest.mark.parametrize("name,B,H", R.range_cases())
def test_range_probes_are_exact_leak_free_and_every_tile_is_owned(name, B, H):
    from gen3c_amd import ops
    sh = R.range_shape(name)
    S, lists, hp = sh["S"], sh["lists"], R.RANGE_HEAD_PATTERNS[B, H]
    assert len(hp) == H and set(hp) == set(range(len(lists))) and list(hp) != sorted(hp)  # every pattern, the last one too, and not in order
    assert len(set(hp)) < H or H <= len(lists)  # two heads on one pattern wherever there are more heads than patterns
    for pat, blocks in enumerate(lists):  # the helper's mask, written from the header's definition, is the library's
        assert torch.equal(R.ranges_mask(blocks, S), ops.ranges_attn_mask(R.pack(lists, sh["max_ranges"]), S, pattern=pat))
    for kind in _range_kinds(name, B, H):
        p, masks, ref, lse = _range_ref(name, B, H, kind)
        for t in (p.q, p.k, p.v):
            assert torch.equal(t.to(torch.bfloat16).double(), t)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(lse).all())
        assert float((ref.sum(-1) - 1).abs().max()) < 1e-12
        if p.name != "census-block":
            continue
        assert p.C == R.RANGE_CLASSES and R.keys_all_owned(p, masks), (name, B, H)
        # the closed form: every (head, query block, tile) triple of the launch owns the element (row, tile) of every row of the block
        want = masks[:, :, ::R.KVB].double()  # [H, S, tiles]: tile d in row i's list
        want = (want / want.sum(-1, keepdim=True)).permute(1, 0, 2)[:, None].expand(S, B, H, S // R.KVB)
        assert float((ref[..., :S // R.KVB] - want).abs().max()) < 1e-6 and float(ref[..., S // R.KVB:].abs().max()) == 0.0


@pytest.mark.parametrize("name,B,H", R.range_cases())
def test_clean_range_emulation_meets_every_bar_and_its_walk_gives_the_bits_of_its_mask(name, B, H):
    sh = R.range_shape(name)
    walks = R.range_walks(sh["lists"], R.RANGE_HEAD_PATTERNS[B, H], B, sh["S"])
    worst = 0.0
    for kind in _range_kinds(name, B, H):
        p, masks, ref, ref_lse = _range_ref(name, B, H, kind)
        for bound, rel in _range_forms(kind, sh["S"]):
            out, lse = R.emulate(p.q, p.k, p.v, mask=masks, bound_log2=bound)
            assert _passes(p, out, lse, ref, ref_lse, rel), (name, p.name, B, H, bound, R.first_bad(out, ref, rel))
            out_w, lse_w = R.emulate_walks(p.q, p.k, p.v, walks, bound_log2=bound)
            assert torch.equal(out_w, out) and torch.equal(lse_w, lse), (name, p.name, B, H, bound)
            worst = max(worst, R.out_errors(out, ref, rel)[1])
    print(f"[range emulation {name} B={B} H={H}] worst relative element error {worst:.3e}")


def _range_defect_runs(defect):
    """shape (a) in both forms, (b) and (c) with a running maximum; a case whose defective walk IS the clean one (lanes >= 32 on a short table, the
    pair index at B = 1) is left out"""
    for name, B, H in R.range_cases():
        sh = R.range_shape(name)
        hp = R.RANGE_HEAD_PATTERNS[B, H]
        walks = R.range_walks(sh["lists"], hp, B, sh["S"], defect)
        if walks == R.range_walks(sh["lists"], hp, B, sh["S"]):
            continue
        for kind in _range_kinds(name, B, H):
            p, masks, ref, ref_lse = _range_ref(name, B, H, kind)
            for bound, _rel in _range_forms(kind, sh["S"])[:2 if name == "a" else 1]:
                yield p, masks, dict(walks=walks, bound_log2=bound, ref=(ref, ref_lse)), f"shape {name} "


# ---- teeth -------------------------------------------------------------------------------------------------------------------------------------------

def _defect_runs(defect):
    """(probe, mask the reference uses, emulation keyword arguments) of the cases on which a defect is tried"""
    if defect in R.RANGE_DEFECTS:
        yield from _range_defect_runs(defect)
        return
    if defect in ("window_short", "window_long"):
        fl, S, W, s = 64, 768, 1, 0
        bad = R.window_mask(S, fl, W, s, hi_shift=-R.KVB if defect == "window_short" else R.KVB)
        for make in (R.census_position, R.census_block):
            yield make(S, S, 2, 3), R.window_mask(S, fl, W, s), dict(mask=bad, bound_log2=BOUND_LOG2)
        return
    if defect == "skip_shifted":
        Sq, L = 200, 128
        for make in (R.census_position, R.census_block):
            yield make(Sq, 3 * L, 2, 3), R.skip_mask(Sq, 3 * L, L, L), dict(mask=R.skip_mask(Sq, 3 * L, L + R.KVB, L))
        return
    for Sq, Skv, B, H in ((200, 320, 2, 3), (64, 449, 1, 8)):
        for p in _probes(Sq, Skv, B, H):
            yield p, None, dict(defect=defect)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_fails_at_least_one_probe(defect):
    failed = []
    for p, mask, kw, *where in _defect_runs(defect):
        rel = R.REL_EXACT_P if (kw.get("bound_log2") is None and not p.name.startswith("staircase")) else R.REL_BF16
        if "walks" in kw:  # a range defect: the shared reference, and the OUTPUT alone (family 7's launches write no LSE)
            ref, ref_lse = kw["ref"]
            out, lse = R.emulate_walks(p.q, p.k, p.v, kw["walks"], bound_log2=kw["bound_log2"])
            caught = not _passes(p, out, lse, ref, ref_lse, rel, check_lse=False)
        else:
            ref, ref_lse = R.reference(p, mask)
            out, lse = R.emulate(p.q, p.k, p.v, **kw)
            caught = not _passes(p, out, lse, ref, ref_lse, rel)
        if caught:
            form = "" if "walks" not in kw else " no-max" if kw["bound_log2"] is not None else " running max"
            failed.append(f"{''.join(where)}{p.name}{form} Sq={p.Sq} Skv={p.Skv} B={p.B} H={p.H}")
    print(f"[defect {defect}] caught by: {failed}")
    assert failed, f"no probe notices the defect {defect}"


@functools.lru_cache(maxsize=None)
def _gaussian(Sq, Skv, B, H):
    g = torch.Generator().manual_seed(Skv)
    mk = lambda n: torch.randn(n, B, H, R.HD, generator=g).to(torch.bfloat16).double()
    return mk(Sq), mk(Skv), mk(Skv)


def test_report_defects_against_the_gaussian_rel_l2_bar():
    """Not a gate: which defects rel-L2 < 1e-2 on Gaussian inputs lets through (the older attention tests' bar). That bar looks at the output only,
    so a defect of the LSE alone (lse_without_log2_l) is outside it by construction and is listed apart."""
    Sq, B, H, fl = 256, 2, 3, 320
    errors = {}
    for Skv in (2209, 4160):
        q, k, v = _gaussian(Sq, Skv, B, H)
        p = R.Probe("gaussian", q, k, v, exact=False)
        for defect in R.DEFECTS:
            kw, mask = dict(defect=defect), None
            if defect in R.RANGE_DEFECTS:
                continue  # (self-attention under a table: reported below, at family 7's shapes and against the range kernels' own bar)
            if defect in ("window_short", "window_long", "skip_shifted") and Skv % 64:
                continue  # (whole tiles only, as the kernels with these forms)
            if defect in ("window_short", "window_long"):  # the query rows are the first rows of the sequence
                window = lambda shift_: R.window_mask(Skv, fl, 1, 0, hi_shift=shift_)[:Sq]
                mask, kw = window(0), dict(mask=window(-R.KVB if defect == "window_short" else R.KVB))
            elif defect == "skip_shifted":
                mask, kw = R.skip_mask(Sq, Skv, 1024, 1024), dict(mask=R.skip_mask(Sq, Skv, 1024 + R.KVB, 1024))
            ref, _ = R.reference(p, mask)
            out, _lse = R.emulate(q, k, v, **kw)
            errors.setdefault(defect, []).append((Skv, float((out.double() - ref).norm() / ref.norm())))
    for d, runs in errors.items():
        print(f"[gaussian rel-L2] {d}: " + ", ".join(f"Skv={s}: {e:.3e}" for s, e in runs))
    through = [d for d, runs in errors.items() if d != "lse_without_log2_l" and all(e < 1e-2 for _s, e in runs)]
    print(f"[gaussian rel-L2 < 1e-2 lets through] {through}; never looks at: ['lse_without_log2_l']")
    # the range defects, against the bar tests/test_attn_ranges_gpu.py holds the range kernels to: the worst (batch, head) rel-L2 < 4e-3 on Gaussian
    # inputs, at family 7's shapes (a) and (c) and tables, no-max form
    bar, rng_errors = 4e-3, {}
    for name, B, H in (("a", 2, 3), ("c", 1, 2)):
        sh = R.range_shape(name)
        S, hp = sh["S"], R.RANGE_HEAD_PATTERNS[B, H]
        q, k, v = _gaussian(S, S, B, H)
        ref, _ = R.reference(R.Probe("gaussian", q, k, v, exact=False), R.head_masks(sh["lists"], hp, S))
        clean = R.range_walks(sh["lists"], hp, B, S)
        for defect in (None,) + R.RANGE_DEFECTS:
            walks = R.range_walks(sh["lists"], hp, B, S, defect)
            if defect is not None and walks == clean:
                continue
            out, _lse = R.emulate_walks(q, k, v, walks, bound_log2=BOUND_LOG2)
            pair = lambda b, h: float((out[:, b, h].double() - ref[:, b, h]).norm() / ref[:, b, h].norm())
            rng_errors.setdefault(defect or "clean", []).append((name, max(pair(b, h) for b in range(B) for h in range(H))))
    for d, runs in rng_errors.items():
        print(f"[gaussian worst (batch, head) rel-L2, range table] {d}: " + ", ".join(f"shape {n}: {e:.3e}" for n, e in runs))
    assert all(e < bar for _n, e in rng_errors["clean"]), rng_errors["clean"]  # (the clean emulation is inside that bar: the report is about the defects)
    print(f"[gaussian rel-L2 < {bar} lets through] {[d for d, runs in rng_errors.items() if d != 'clean' and all(e < bar for _n, e in runs)]}")
