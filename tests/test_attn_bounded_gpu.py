"""GPU: the no-max form of the one-wave-per-SIMD self-attention kernel (flash_attn_fwd_w4b_nm_kernel, g3_self_attn_fwd_bounded_bf16).

The caller bounds the logits (q, k behind a per-head RMSNorm: |q . k| / sqrt(128) <= sqrt(128) max|w_q| max|w_k|), the kernel takes the bound as the
constant reference point of the softmax instead of a running row maximum. Every launch here names variant 11 and head dim 128.

Shapes: S_kv 64 .. 320 = the prologue alone, both parities of the loop tail and one full loop pair; S_q 64 / 200 / 512 = one workgroup, a ragged
one, several; (B, H) = (1, 8) takes the XCD-local 1-D grid, (2, 3) the 3-D grid. q / k are column views of fused buffers, as the DiT passes them.
Inputs: RMS-normalised rows (norm sqrt(128) w), random / 8 keys equal to their query (logit ~ +bound) / 8 keys equal to the negated query (~ -bound).

Bars.
 * unit weights (bound 16.8 in the log2 domain): rel-L2 against an fp32 softmax < 4e-3, the bar of the existing attention tests.
 * w_q = w_k = 1.85 (bound 57.5, just under the limit of 60): the fp32 softmax is sharp and the max-tracking kernel itself sits near 4e-3, so the
   no-max form's error must be at most 1.5 x the max-tracking kernel's on the same inputs (the dominant P is no longer exactly 1: a CPU emulation gave
   ratios 1.05 .. 1.29; the margin covers other seeds).
 * split-KV: a bounded part and a max-form part over disjoint keys merge to the one-call result within 1e-3 - compared as the fp32 partials the
   kernels write (the bf16 rounding of an OUTPUT alone is 2^-9 relative), on inputs whose V is constant inside each part: the merged row is then
   (w_A v_A + w_B v_B) with the weights coming from the two parts' LSE alone, while the bf16 rounding of P (which separates ANY two attention
   results by ~3e-3 on random V, see tests/test_kernels_gpu.py: split-KV) averages out inside a part. Measured 1.6e-4 .. 4.5e-4.
 * a bound of 0, a bound beyond the limit and variant 4 run exactly what g3_flash_attn_fwd_ex_bf16 runs: bitwise equal outputs.
An understated bound is a caller error and is not tested."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 128
NM = "flash_attn_fwd_w4b_nm_kernel<true>"
MARGIN = 1.03


def _bound(w):  # natural units: 128 w_q w_k / sqrt(128), plus the margin for the bf16 roundings of q and k
    return HD * w * w / math.sqrt(HD) * MARGIN


def _rel_l2(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _rms(x, w):
    x = x.float().view(x.shape[0], -1, HD)
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True)) * w).reshape(x.shape[0], -1)


def _inputs(Sq, Skv, B, H, w, kind, seed):
    """q: [Sq*B, H*128] view of a [Sq*B, 2 H 128] buffer (first half), k: [Skv*B, H*128] view of a [Skv*B, 2 H 128] buffer (second half), v, V^T."""
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    D = H * HD
    qbuf = torch.randn(Sq * B, 2 * D, device=dev, generator=g)
    kbuf = torch.randn(Skv * B, 2 * D, device=dev, generator=g)
    qn, kn = _rms(qbuf[:, :D], w), _rms(kbuf[:, D:], w)
    if kind != "random":  # query rows 0, Sq / 2, Sq - 1 of every (batch, head): 8 keys each are the query itself (or its negation)
        sign = 1.0 if kind == "pos" else -1.0
        keys = torch.randperm(Skv, device=dev, generator=g)[:24].view(3, 8)
        for i, r in enumerate((0, Sq // 2, Sq - 1)):
            for b in range(B):
                kn[keys[i] * B + b] = sign * qn[r * B + b]
    qbuf = torch.cat([qn, qbuf[:, D:]], dim=1).to(torch.bfloat16)
    kbuf = torch.cat([kbuf[:, :D], kn], dim=1).to(torch.bfloat16)
    v = torch.randn(Skv * B, D, device=dev, generator=g).to(torch.bfloat16)
    q, k = qbuf[:, :D], kbuf[:, D:]
    assert q.stride(0) == 2 * D and k.stride(0) == 2 * D and not q.is_contiguous() and not k.is_contiguous()
    return q, k, v, ops.transpose_v(v, Skv, B, H)


def _fp32(q, k, v, B, H):
    out = torch.empty(q.shape[0], H * HD, device=q.device)
    for b in range(B):
        for h in range(H):
            sl = slice(h * HD, (h + 1) * HD)
            sc = (q[b::B, sl].float() @ k[b::B, sl].float().t()) / math.sqrt(HD)
            out[b::B, sl] = torch.softmax(sc, dim=-1) @ v[b::B, sl].float()
    return out


def _worst_pair(out, ref, B, H):
    return max(_rel_l2(out[b::B, h * HD:(h + 1) * HD], ref[b::B, h * HD:(h + 1) * HD]) for b in range(B) for h in range(H))


def _name(Sq, Skv, B, H, bound, variant=11):
    from gen3c_amd import _lib
    return _lib.load().g3_self_attn_kernel_name(Sq, Skv, B, H, float(bound), variant).decode()


@pytest.mark.parametrize("B,H", [(1, 8), (2, 3)])
@pytest.mark.parametrize("Sq", [64, 200, 512])
@pytest.mark.parametrize("Skv", [64, 128, 192, 256, 320])
def test_bounded_self_attention_vs_fp32(Skv, Sq, B, H):
    from gen3c_amd import ops
    assert _name(Sq, Skv, B, H, _bound(1.0)) == NM and _name(Sq, Skv, B, H, _bound(1.85)) == NM
    assert 57.0 < _bound(1.85) * math.log2(math.e) < 60.0
    for kind in ("random", "pos", "neg"):
        # unit weights: the bar of the existing attention tests
        q, k, v, vt = _inputs(Sq, Skv, B, H, 1.0, kind, seed=Skv + Sq + B)
        ops.enable_kernel_timers(True)
        out = ops.self_attn_bounded(q, k, vt, Sq, Skv, B, H, _bound(1.0), variant=11)
        launched = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
        ops.enable_kernel_timers(False)
        assert launched and launched[-1]["kernel"] == NM and {"Sq", "Skv", "H", "B", "kernel"} <= set(launched[-1])
        ref = _fp32(q, k, v, B, H)
        e1 = _worst_pair(out, ref, B, H)
        print(f"[bounded w=1 {kind} Sq={Sq} Skv={Skv} B={B} H={H}] worst (batch, head) rel-L2 vs fp32 = {e1:.3e}")
        assert torch.isfinite(out.float()).all()
        assert e1 < 4e-3, f"{kind}: rel-L2 {e1:.3e} vs fp32 softmax"
        # weights 1.85: against the max-tracking kernel's own error on the same inputs
        q, k, v, vt = _inputs(Sq, Skv, B, H, 1.85, kind, seed=Skv + Sq + B + 1)
        out = ops.self_attn_bounded(q, k, vt, Sq, Skv, B, H, _bound(1.85), variant=11)
        out_max = ops.flash_attn(q, k, vt, Sq, Skv, B, H, variant=11)
        ref = _fp32(q, k, v, B, H)
        e_nm, e_max = _rel_l2(out, ref), _rel_l2(out_max, ref)
        print(f"[bounded w=1.85 {kind} Sq={Sq} Skv={Skv} B={B} H={H}] rel-L2 vs fp32: no-max {e_nm:.3e}, max-tracking {e_max:.3e}, ratio {e_nm / e_max:.3f}")
        assert torch.isfinite(out.float()).all()
        assert e_nm <= 1.5 * e_max, f"{kind}: no-max {e_nm:.3e} vs max-tracking {e_max:.3e}"


@pytest.mark.parametrize("B,H", [(1, 8), (2, 3)])
@pytest.mark.parametrize("Sq,Skv,split", [(200, 320, 128), (64, 128, 64), (512, 256, 192)])
def test_bounded_partial_merges_with_a_max_form_part(Sq, Skv, split, B, H):
    """LSE of the no-max form (m_run = bound) is the same log-sum-exp the max-tracking kernel writes: keys [0, split) through the bounded entry,
    keys [split, Skv) through g3_flash_attn_fwd_ex_bf16, merged, against ONE bounded call over all keys - both sides as the fp32 partials the kernels
    write. V is one random row per part (see the module docstring), so a wrong LSE moves the mixing weights and nothing else hides it."""
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    q, k, v, _ = _inputs(Sq, Skv, B, H, 1.0, "pos", seed=Sq + split)
    g = torch.Generator(device=dev).manual_seed(split)
    va, vb = (torch.randn(1, H * HD, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    v = torch.cat([va.expand(split * B, -1), vb.expand((Skv - split) * B, -1)]).contiguous()
    vt = ops.transpose_v(v, Skv, B, H)
    o_one, lse_one = ops.self_attn_bounded(q, k, vt, Sq, Skv, B, H, _bound(1.0), variant=11, partial=True)  # ONE bounded call over all keys, fp32
    rows = split * B
    part_a = ops.self_attn_bounded(q, k[:rows], ops.transpose_v(v[:rows], split, B, H), Sq, split, B, H, _bound(1.0), variant=11, partial=True)
    part_b = ops.flash_attn(q, k[rows:], ops.transpose_v(v[rows:], Skv - split, B, H), Sq, Skv - split, B, H, variant=11, partial=True)
    # the merge in fp32 (w_i = 2^(lse_i - max)), so that no bf16 rounding of the OUTPUT (2^-9 relative, more than the bar) sits between the two sides
    rowsof = lambda lse: lse.permute(2, 0, 1).reshape(Sq * B, H)  # [B, H, Sq] -> [(s, b), H]
    la, lb = rowsof(part_a[1]), rowsof(part_b[1])
    mx = torch.maximum(la, lb)
    wa, wb = torch.exp2(la - mx), torch.exp2(lb - mx)
    exp_h = lambda w: w.repeat_interleave(HD, dim=1)
    merged32 = (exp_h(wa) * part_a[0] + exp_h(wb) * part_b[0]) / exp_h(wa + wb)
    r = _rel_l2(merged32, o_one)
    d_lse_merged = float((mx + torch.log2(wa + wb) - rowsof(lse_one)).abs().max())
    # the same keys through both forms: the same log-sum-exp (fp32 sums of the unrounded P: a few ulp of values below 32, 2e-6 each)
    lse_max = ops.flash_attn(q, k[:rows], ops.transpose_v(v[:rows], split, B, H), Sq, split, B, H, variant=11, partial=True)[1]
    d_lse = float((part_a[1] - lse_max).abs().max())
    # the merge kernel on the same two parts: merged32 rounded to bf16 (half an ulp = 2^-9 relative at most)
    merged = ops.attn_merge([part_a, part_b], Sq, B, H)
    r_kernel = _rel_l2(merged, merged32)
    ref = _fp32(q, k, v, B, H)
    print(f"[bounded split-kv Sq={Sq} Skv={Skv} split={split} B={B} H={H}] fp32 merge vs one call {r:.3e}, LSE merged - one call {d_lse_merged:.3e}, "
          f"max |LSE nm - LSE max| {d_lse:.3e}, merge kernel vs fp32 merge {r_kernel:.3e}, vs fp32 softmax {_rel_l2(merged, ref):.3e}")
    assert d_lse <= 1e-4 and d_lse_merged <= 1e-4
    assert r <= 1e-3
    assert r_kernel <= 2.0 ** -9 + 1e-5
    assert _rel_l2(merged, ref) < 4e-3


def test_bounded_entry_falls_back_bitwise():
    """Outside the no-max form's range the bounded entry IS g3_flash_attn_fwd_ex_bf16: bound 0, a bound beyond 60 in the log2 domain, the 8-wave kernel."""
    from gen3c_amd import _lib, ops
    Sq, Skv, B, H = 200, 320, 1, 8
    q, k, v, vt = _inputs(Sq, Skv, B, H, 1.0, "pos", seed=7)
    lib = _lib.load()
    plain11 = ops.flash_attn(q, k, vt, Sq, Skv, B, H, variant=11)
    plain4 = ops.flash_attn(q, k, vt, Sq, Skv, B, H, variant=4)
    over = 60.5 / math.log2(math.e)
    for bound, variant, plain in ((0.0, 11, plain11), (over, 11, plain11), (-1.0, 11, plain11), (_bound(1.0), 4, plain4)):
        name = _name(Sq, Skv, B, H, bound, variant)
        assert name == lib.g3_flash_attn_kernel_name_ex(Sq, Skv, B, H, variant).decode() and name != NM, (bound, variant, name)
        ops.enable_kernel_timers(True)
        out = ops.self_attn_bounded(q, k, vt, Sq, Skv, B, H, bound, variant=variant)
        launched = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
        ops.enable_kernel_timers(False)
        assert launched[-1]["kernel"] == name
        assert torch.equal(out, plain), (bound, variant)
    assert _name(Sq, Skv, B, H, 60.0 / math.log2(math.e) * 0.999) == NM  # the limit itself is inside
    # the no-max form really is another kernel: same function, not the same bits
    nm = ops.self_attn_bounded(q, k, vt, Sq, Skv, B, H, _bound(1.0), variant=11)
    assert _rel_l2(nm, plain11) < 6e-3
