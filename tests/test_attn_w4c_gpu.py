"""GPU: flash_attn_fwd_w4c_nm_kernel, the no-max self-attention kernel on 16x16x32 MFMAs (g3_self_attn_fwd_bounded16_bf16,
ops.self_attn_bounded(mfma16=True)), in NaN-guarded buffers, B = 2, H = 2, q / k as column views of fused [S*B, 3*256] buffers as the DiT passes them.

Shapes (S_q, S_kv): (256, 64) one tile - prologue and last-tile path only; (320, 128) ragged last query block, one tile pair; (512, 192) odd tile count,
both stage parities; (256, 1024) the steady-state loop.
Inputs and bars are those of tests/test_attn_bounded_gpu.py: RMS-normalised rows, random / 8 keys equal to their query / 8 keys equal to the negated
query; unit weights: worst (batch, head) rel-L2 against the fp32 softmax < 4e-3; w_q = w_k = 1.85: error at most 1.5 x the max-tracking kernel's on the
same inputs. Beside each figure the existing no-max kernel's (flash_attn_fwd_w4b_nm_kernel) on the same inputs is printed, and in EVERY case - each shape,
each of the three input kinds, both weight settings - the two figures must agree within the spread the existing kernel's own error shows across five seeds
of that very case (same shape, kind and weights; measured here from the existing kernel alone; recorded in profiles/attn_mfma16_ab.txt). With more than
one tile the two kernels' outputs must also differ somewhere: the launch really takes the new table row.
Also: two calls are bitwise equal; nothing outside the payload is written; calls outside the kernel's form (a partial output, a bound above
60 / log2 e, S_kv % 64 != 0, the 8-wave variant, segmented V^T) are bitwise g3_self_attn_fwd_bounded_bf16's and report its kernel. (kv_dense belongs to
the cross-attention entry: the bounded entries do not take it, so no call through this entry can carry one.)"""
import math

import pytest
import torch

from tests.guarded import Guarded
from tests.test_attn_bounded_gpu import HD, NM, _bound, _fp32, _rel_l2, _rms, _worst_pair

pytestmark = pytest.mark.gpu

W4C = "flash_attn_fwd_w4c_nm_kernel"
B, H = 2, 2
D = H * HD
SHAPES = [(256, 64), (320, 128), (512, 192), (256, 1024)]


def _inputs(Sq, Skv, w, kind, seed):
    """q = columns [0, D) of a guarded [Sq*B, 3 D] buffer, k = columns [D, 2 D) of a guarded [Skv*B, 3 D] buffer, v, V^T, a guarded output."""
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    qraw = torch.randn(Sq * B, 3 * D, device=dev, generator=g)
    kraw = torch.randn(Skv * B, 3 * D, device=dev, generator=g)
    qn, kn = _rms(qraw[:, :D], w), _rms(kraw[:, D:2 * D], w)
    if kind != "random":  # query rows 0, Sq / 2, Sq - 1 of every (batch, head): 8 keys each are the query itself (or its negation)
        sign = 1.0 if kind == "pos" else -1.0
        keys = torch.randperm(Skv, device=dev, generator=g)[:24].view(3, 8)
        for i, r in enumerate((0, Sq // 2, Sq - 1)):
            for b in range(B):
                kn[keys[i] * B + b] = sign * qn[r * B + b]
    qbuf = Guarded(Sq * B, 3 * D, data=torch.cat([qn, qraw[:, D:]], dim=1).to(torch.bfloat16))
    kbuf = Guarded(Skv * B, 3 * D, data=torch.cat([kraw[:, :D], kn, kraw[:, 2 * D:]], dim=1).to(torch.bfloat16))
    v = torch.randn(Skv * B, D, device=dev, generator=g).to(torch.bfloat16)
    q, k = qbuf.payload[:, :D], kbuf.payload[:, D:2 * D]
    assert q.stride(0) == 3 * D and k.stride(0) == 3 * D and not q.is_contiguous() and not k.is_contiguous()
    return q, k, v, ops.transpose_v(v, Skv, B, H), Guarded(Sq * B, D, ld=D + 64)


def _run(q, k, vt, Sq, Skv, bound, out, mfma16, **kw):
    """(result, name of the kernel launched)"""
    from gen3c_amd import ops
    ops.enable_kernel_timers(True)
    try:
        res = ops.self_attn_bounded(q, k, vt, Sq, Skv, B, H, bound, out=out, variant=kw.pop("variant", 11), mfma16=mfma16, **kw)
        launched = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    finally:
        ops.enable_kernel_timers(False)
    return res, launched[-1]["kernel"]


def _err(out, ref, w):
    """The figure each bar of tests/test_attn_bounded_gpu.py is set on: unit weights - the worst (batch, head) pair; w = 1.85 - the whole tensor."""
    return _worst_pair(out, ref, B, H) if w == 1.0 else _rel_l2(out, ref)


@pytest.mark.parametrize("Sq,Skv", SHAPES)
def test_w4c_vs_fp32_and_vs_the_32x32x16_kernel(Sq, Skv):
    from gen3c_amd import _lib, ops
    lib = _lib.load()
    assert lib.g3_self_attn16_kernel_name(Sq, Skv, B, H, float(_bound(1.0)), 11).decode() == W4C
    assert lib.g3_self_attn_kernel_name(Sq, Skv, B, H, float(_bound(1.0)), 11).decode() == NM  # the plain entry's answer is unchanged
    differs = []
    for w in (1.0, 1.85):
        for kind in ("random", "pos", "neg"):
            seed0 = Sq + Skv + (1 if w != 1.0 else 0)
            # the yardstick for "the two kernels agree", measured per case: the spread of the EXISTING kernel's own error across five seeds of this
            # shape, input kind and weight (seed0 + 100 s; the kernel under test takes no part in it)
            e32_seeds = []
            for s in range(5):
                q, k, v, vt, _o = _inputs(Sq, Skv, w, kind, seed0 + 100 * s)
                e32_seeds.append(_err(ops.self_attn_bounded(q, k, vt, Sq, Skv, B, H, _bound(w), variant=11), _fp32(q, k, v, B, H), w))
            spread = max(e32_seeds) - min(e32_seeds)
            q, k, v, vt, o = _inputs(Sq, Skv, w, kind, seed0)
            _, name = _run(q, k, vt, Sq, Skv, _bound(w), o.payload, True)
            assert name == W4C
            o.assert_only_payload_written(f"w4c w={w} {kind} Sq={Sq} Skv={Skv}")
            out = o.payload.clone()
            o2 = Guarded(Sq * B, D, ld=D + 64)
            _run(q, k, vt, Sq, Skv, _bound(w), o2.payload, True)
            assert torch.equal(out, o2.payload), "two calls differ"
            out32, name32 = _run(q, k, vt, Sq, Skv, _bound(w), None, False)
            assert name32 == NM
            ref = _fp32(q, k, v, B, H)
            e16, e32 = _err(out, ref, w), _err(out32, ref, w)
            differs.append(not torch.equal(out, out32))
            line = (f"[w4c w={w} {kind} Sq={Sq} Skv={Skv}] rel-L2 vs fp32: 16x16x32 {e16:.4e}, 32x32x16 {e32:.4e} (its five seeds: "
                    f"{' '.join(f'{e:.3e}' for e in e32_seeds)}, spread {spread:.3e}); between the two kernels {_rel_l2(out, out32):.3e}")
            if w == 1.0:  # unit weights: the bar of the existing attention tests
                print(line)
                assert e16 < 4e-3, f"{kind}: rel-L2 {e16:.3e} vs fp32 softmax"
            else:  # weights 1.85: against the max-tracking kernel's own error on the same inputs
                e_max = _rel_l2(ops.flash_attn(q, k, vt, Sq, Skv, B, H, variant=11), ref)
                print(line + f"; max-tracking {e_max:.4e}, ratio {e16 / e_max:.3f}")
                assert e16 <= 1.5 * e_max, f"{kind}: 16x16x32 no-max {e16:.3e} vs max-tracking {e_max:.3e}"
            assert abs(e16 - e32) <= spread, f"w={w} {kind}: 16x16x32 {e16:.4e} vs 32x32x16 {e32:.4e}: apart by more than the five-seed spread {spread:.3e}"
    # the launch really ran another kernel: the scores and P are the same numbers in both, but with more than one tile the fp32 sums of a row run in
    # another order, and over six cases of >= 128 keys some output element rounds the other way (measured: 1e-6 .. 2e-5 rel-L2 between the two)
    if Skv >= 128:
        assert any(differs), "the 16x16x32 entry returned the 32x32x16 kernel's bits in every case"


def test_w4c_entry_falls_back_bitwise():
    from gen3c_amd import ops
    Sq, Skv = 320, 192
    q, k, v, vt, _o = _inputs(Sq, Skv, 1.0, "pos", seed=11)
    over = 60.5 / math.log2(math.e)
    # (keyword arguments of the call, kernel that must NOT be the new one)
    for kw in (dict(partial=True), dict(bound=over), dict(bound=0.0), dict(variant=4)):
        bound = kw.pop("bound", _bound(1.0))
        got, name = _run(q, k, vt, Sq, Skv, bound, None, True, **dict(kw))
        want, name_plain = _run(q, k, vt, Sq, Skv, bound, None, False, **dict(kw))
        assert name == name_plain and name != W4C, (kw, bound, name, name_plain)
        for a, b in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
            assert torch.equal(a, b), (kw, bound)
    # S_kv % 64 != 0: the ragged-tile kernel
    Skv2 = 200
    q, k, v, vt, _o = _inputs(Sq, Skv2, 1.0, "random", seed=12)
    got, name = _run(q, k, vt, Sq, Skv2, _bound(1.0), None, True)
    want, name_plain = _run(q, k, vt, Sq, Skv2, _bound(1.0), None, False)
    assert name == name_plain and name not in (W4C, NM) and torch.equal(got, want)
    # segmented V^T (two key segments): the key-sharded entry, which the flag does not touch
    Skv3, L = 256, 128
    q, k, v, vt, _o = _inputs(Sq, Skv3, 1.0, "random", seed=13)
    vseg = torch.stack([ops.transpose_v(v[:L * B], L, B, H), ops.transpose_v(v[L * B:], L, B, H)])
    got, name = _run(q, k, vseg, Sq, Skv3, _bound(1.0), None, True)
    want, name_plain = _run(q, k, vseg, Sq, Skv3, _bound(1.0), None, False)
    assert name == name_plain and name != W4C and torch.equal(got, want)
