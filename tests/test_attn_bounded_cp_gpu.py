"""GPU: the no-max self-attention kernels under key sharding (g3_self_attn_fwd_bounded_cp_bf16 through ops.self_attn_bounded with segmented V^T,
carry=, kv_skip=, partial=): flash_attn_fwd_w4b_nm_kernel<true> with segmented V^T, flash_attn_fwd_w4b_nm_carry_kernel<true> with a carry-in state or a
skipped key range. Every launch names variant 11 and head dim 128.

Inputs: the recipe of tests/test_attn_bounded_gpu.py (RMS-normalised q and k rows of norm sqrt(128) w, kinds random / pos / neg = 8 keys equal to
(minus) their query for three query rows, the bound 128 w^2 / sqrt(128) * 1.03, q / k column views of fused buffers); key layout of
tests/test_attn_carry_gpu.py (`world` blocks of L keys, plain V^T and rank segments, the queries of one rank, its own block skipped).

Shapes (Sq, L, world): (64, 64, 2), (200, 128, 3), (512, 192, 4), (200, 64, 5) - 64 / 256 / 576 / 256 remote keys = the prologue alone, both parities of
the loop tail, a full loop pair; a skip that starts at tile 1 (L = 64, rank 1) and later ones. (B, H) = (1, 8): XCD-local 1-D grid, (2, 3): 3-D grid.

Bars (all taken from the existing tests of the max form and of the plain no-max form, none from what this code gives).
 * address-only forms - segments against plain V^T, a skipped range against contiguous copies of the kept keys, an absent / empty carry, an in-place
   carry - are the same arithmetic on the same keys in the same tiles: bitwise.
 * chains: local_first (own shard + before + after through ops.attn_merge) and local_carry (own-shard partial + one carry launch with the skip), each
   < 1e-3 against the other (carry against merge, test_carry_small_shapes) and < 4e-3 against the fp32 softmax over all keys; the same for a three-launch
   chain where the keys make three blocks (world >= 3: 128 keys in 64-key tiles make two). The fp32 partial + LSE of a two-launch bounded chain against
   ONE bounded partial call over all keys: 1e-3 and |dLSE| <= 1e-4 (test_bounded_partial_merges_with_a_max_form_part). With the bound as the
   reference point of every launch a key's P does not depend on the split, so this difference should be fp32 summation order alone, far
   below the bar; the test prints it, and the bar stays the existing one (not tightened on a guess).
 * mixed chains: a bounded part and a max-form part of the same rows merge and carry within 1e-3 of ONE bounded call, as fp32 partials, on V constant
   inside each part (the merged row is w_A v_A + w_B v_B with the weights from the parts' LSE alone: a wrong LSE moves them and nothing hides it).
 * w = 1.85 (bound 57.5 in the log2 domain), kinds pos / neg: the bounded chain's error against fp32 <= 1.5 x the max-form chain's on the same inputs.
 * bound 0, beyond 60 / log2(e), negative, variant 4: bitwise g3_flash_attn_fwd_carry_bf16, and its kernel name; its refusals, nothing launched."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 128
NM = "flash_attn_fwd_w4b_nm_kernel<true>"
NMC = "flash_attn_fwd_w4b_nm_carry_kernel<true>"
CARRY = "flash_attn_fwd_w4b_carry_kernel<true>"
MARGIN = 1.03
SHAPES = [(64, 64, 2), (200, 128, 3), (512, 192, 4), (200, 64, 5)]
BH = [(1, 8), (2, 3)]
DEV = torch.device("cuda:0")


def _bound(w):  # natural units: 128 w_q w_k / sqrt(128), plus the margin for the bf16 roundings of q and k
    return HD * w * w / math.sqrt(HD) * MARGIN


def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _rms(x, w):
    x = x.float().view(x.shape[0], -1, HD)
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True)) * w).reshape(x.shape[0], -1)


def _fp32(q, k, v, B, H):
    out = torch.empty(q.shape[0], H * HD, device=q.device)
    for b in range(B):
        for h in range(H):
            sl = slice(h * HD, (h + 1) * HD)
            sc = (q[b::B, sl].float() @ k[b::B, sl].float().t()) / math.sqrt(HD)
            out[b::B, sl] = torch.softmax(sc, dim=-1) @ v[b::B, sl].float()
    return out


@functools.lru_cache(maxsize=None)
def _problem(Sq, L, world, B, H, w, kind, const_v=False):
    """q [Sq*B, H*128] / k [S*B, H*128] (S = world * L): column views of fused buffers; v; plain V^T [B,H,128,S]; rank segments [world,B,H,128,L]; the fp32
    softmax over all keys. Built once per case and shared (never written to). const_v: V is one random row for block 0 and another for the rest."""
    from gen3c_amd import ops
    S = world * L
    g = torch.Generator(device=DEV).manual_seed(1000 * Sq + 10 * L + world + B)
    D = H * HD
    qbuf = torch.randn(Sq * B, 2 * D, device=DEV, generator=g)
    kbuf = torch.randn(S * B, 2 * D, device=DEV, generator=g)
    qn, kn = _rms(qbuf[:, :D], w), _rms(kbuf[:, D:], w)
    if kind != "random":  # query rows 0, Sq / 2, Sq - 1 of every (batch, head): 8 keys each are the query itself (or its negation)
        sign = 1.0 if kind == "pos" else -1.0
        keys = torch.randperm(S, device=DEV, generator=g)[:24].view(3, 8)
        for i, r in enumerate((0, Sq // 2, Sq - 1)):
            for b in range(B):
                kn[keys[i] * B + b] = sign * qn[r * B + b]
    qbuf = torch.cat([qn, qbuf[:, D:]], dim=1).to(torch.bfloat16)
    kbuf = torch.cat([kbuf[:, :D], kn], dim=1).to(torch.bfloat16)
    if const_v:
        va, vb = (torch.randn(1, D, device=DEV, generator=g).to(torch.bfloat16) for _ in range(2))
        v = torch.cat([va.expand(L * B, -1), vb.expand((S - L) * B, -1)]).contiguous()
    else:
        v = torch.randn(S * B, D, device=DEV, generator=g).to(torch.bfloat16)
    q, k = qbuf[:, :D], kbuf[:, D:]
    assert q.stride(0) == 2 * D and k.stride(0) == 2 * D and not q.is_contiguous() and not k.is_contiguous()
    vt = ops.transpose_v(v, S, B, H)
    vseg = torch.stack([ops.transpose_v(v[r * L * B:(r + 1) * L * B], L, B, H) for r in range(world)])
    return q, k, v, vt, vseg, _fp32(q, k, v, B, H)


def _blocks(k, vseg, L, B, r0, r1):
    """key blocks [r0, r1): K rows (a row range of the strided view), segmented V^T"""
    return k[r0 * L * B:r1 * L * B], vseg[r0:r1]


def _remote(k, vseg, L, world, rank, B):
    """every key but the rank's own block: a sub-range on the first / last rank, the whole buffers with a skip on an interior one"""
    if rank == 0:
        return k[L * B:], vseg[1:], None
    if rank == world - 1:
        return k[:rank * L * B], vseg[:rank], None
    return k, vseg, (rank * L, L)


def _attn(bound):
    """the attention call of a chain: the bounded entry, or (bound None) the max form's"""
    from gen3c_amd import ops
    if bound is None:
        return lambda *a, **kw: ops.flash_attn(*a, variant=11, **kw)
    return lambda *a, **kw: ops.self_attn_bounded(*a, bound, variant=11, **kw)


def _local_first(q, k, vseg, Sq, L, world, rank, B, H, bound):
    """own shard + the blocks before + the blocks after, merged by ops.attn_merge"""
    from gen3c_amd import ops
    at = _attn(bound)
    parts = [at(q, *_blocks(k, vseg, L, B, rank, rank + 1), Sq, L, B, H, partial=True)]
    for r0, r1 in ((0, rank), (rank + 1, world)):
        if r1 > r0:
            parts.append(at(q, *_blocks(k, vseg, L, B, r0, r1), Sq, (r1 - r0) * L, B, H, partial=True))
    return ops.attn_merge(parts, Sq, B, H)


def _local_carry(q, k, vseg, Sq, L, world, rank, B, H, bound):
    """own-shard partial, then ONE carry launch over every remote key (an interior rank skips its own block)"""
    at = _attn(bound)
    own = at(q, *_blocks(k, vseg, L, B, rank, rank + 1), Sq, L, B, H, partial=True)
    kk, vv, skip = _remote(k, vseg, L, world, rank, B)
    return at(q, kk, vv, Sq, (world - 1) * L, B, H, carry=own, kv_skip=skip)


def _rowsof(lse, Sq, B, H):  # [B, H, Sq] -> [(s, b), H]
    return lse.permute(2, 0, 1).reshape(Sq * B, H)


def _merge32(pa, pb, Sq, B, H):
    """the merge of two (o_part, lse) in fp32: no bf16 rounding of an OUTPUT (2^-9 relative, more than the 1e-3 bar) between the two sides"""
    la, lb = _rowsof(pa[1], Sq, B, H), _rowsof(pb[1], Sq, B, H)
    mx = torch.maximum(la, lb)
    wa, wb = torch.exp2(la - mx), torch.exp2(lb - mx)
    e = lambda w: w.repeat_interleave(HD, dim=1)
    return (e(wa) * pa[0] + e(wb) * pb[0]) / e(wa + wb), mx + torch.log2(wa + wb)


def _launched(fn):
    from gen3c_amd import ops
    ops.enable_kernel_timers(True)
    try:
        r = fn()
        recs = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    finally:
        ops.enable_kernel_timers(False)
    assert recs
    return r, recs[-1]["kernel"]


def _cp_name(Sq, Skv, B, H, bound, variant, segmented, cp_form):
    from gen3c_amd import _lib
    return _lib.load().g3_self_attn_cp_kernel_name(Sq, Skv, B, H, float(bound), variant, int(segmented), int(cp_form)).decode()


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("Sq,L,world", SHAPES)
def test_kernel_names(Sq, L, world, B, H):
    """the name query and the timer record: the plain no-max kernel for a segmented call without skip or carry, the carry instantiation with either"""
    from gen3c_amd import ops
    q, k, v, vt, vseg, _ = _problem(Sq, L, world, B, H, 1.0, "random")
    bd, S = _bound(1.0), world * L
    for seg in (0, 1):
        assert _cp_name(Sq, S, B, H, bd, 11, seg, 0) == NM
        assert _cp_name(Sq, S, B, H, bd, 11, seg, 1) == NMC
    _, name = _launched(lambda: ops.self_attn_bounded(q, k, vseg, Sq, S, B, H, bd, variant=11))
    assert name == NM
    _, name = _launched(lambda: ops.self_attn_bounded(q, k, vseg, Sq, S, B, H, bd, variant=11, partial=True))
    assert name == NM
    for rank in range(world):
        own, name = _launched(lambda: ops.self_attn_bounded(q, *_blocks(k, vseg, L, B, rank, rank + 1), Sq, L, B, H, bd, variant=11, partial=True))
        assert name == NM
        kk, vv, skip = _remote(k, vseg, L, world, rank, B)
        _, name = _launched(lambda: ops.self_attn_bounded(q, kk, vv, Sq, (world - 1) * L, B, H, bd, variant=11, carry=own, kv_skip=skip))
        assert name == NMC
        _, name = _launched(lambda: ops.self_attn_bounded(q, kk, vv, Sq, (world - 1) * L, B, H, bd, variant=11, kv_skip=skip))
        assert name == (NMC if skip is not None else NM), (rank, name)  # a skip alone takes the carry instantiation too
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("Sq,L,world", SHAPES)
def test_address_only_forms_bitwise(Sq, L, world, B, H):
    from gen3c_amd import ops
    q, k, v, vt, vseg, _ = _problem(Sq, L, world, B, H, 1.0, "pos")
    bd, S = _bound(1.0), world * L
    sab = lambda *a, **kw: ops.self_attn_bounded(*a, bd, variant=11, **kw)
    # segments == plain V^T over the same keys (the plain call is g3_self_attn_fwd_bounded_bf16's)
    a, b = sab(q, k, vseg, Sq, S, B, H), sab(q, k, vt, Sq, S, B, H)
    ap, bp = sab(q, k, vseg, Sq, S, B, H, partial=True), sab(q, k, vt, Sq, S, B, H, partial=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(ap[0], bp[0]) and torch.equal(ap[1], bp[1])
    # a skipped range == contiguous copies of the kept blocks, plain and segmented V^T, every rank (L = 64, rank 1: the skip starts at tile 1;
    # rank 0 / the last rank: a skip at either end, which the entry point turns into a base offset / nothing)
    S_rem = (world - 1) * L
    for rank in range(world):
        b0 = rank * L
        k_kept = torch.cat([k[:b0 * B], k[(b0 + L) * B:]]).contiguous()
        own = sab(q, *_blocks(k, vseg, L, B, rank, rank + 1), Sq, L, B, H, partial=True)
        for segmented in (False, True):
            if segmented:
                vv, v_kept = vseg, torch.cat([vseg[:rank], vseg[rank + 1:]]).contiguous()
            else:
                vv, v_kept = vt, torch.cat([vt[..., :b0], vt[..., b0 + L:]], dim=-1).contiguous()
            a = sab(q, k, vv, Sq, S_rem, B, H, kv_skip=(b0, L))
            b = sab(q, k_kept, v_kept, Sq, S_rem, B, H, kv_skip=(0, 0))
            ap = sab(q, k, vv, Sq, S_rem, B, H, kv_skip=(b0, L), partial=True)
            bp = sab(q, k_kept, v_kept, Sq, S_rem, B, H, kv_skip=(0, 0), partial=True)
            ac = sab(q, k, vv, Sq, S_rem, B, H, kv_skip=(b0, L), carry=own)
            bc = sab(q, k_kept, v_kept, Sq, S_rem, B, H, kv_skip=(0, 0), carry=own)
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(ap[0], bp[0]) and torch.equal(ap[1], bp[1]) and torch.equal(ac, bc), (rank, segmented)
    # an empty carry (carry_lse = -inf, whatever carry_o holds) and no carry == the plain bounded call; an in-place carry == a fresh buffer
    k0, v0 = _blocks(k, vseg, L, B, 0, 1)
    k1, v1 = _blocks(k, vseg, L, B, 1, world)
    own = sab(q, k0, v0, Sq, L, B, H, partial=True)
    empty = (torch.full_like(own[0], float("nan")), torch.full_like(own[1], float("-inf")))
    plain, plain_p = sab(q, k1, v1, Sq, S_rem, B, H), sab(q, k1, v1, Sq, S_rem, B, H, partial=True)
    got, got_p = sab(q, k1, v1, Sq, S_rem, B, H, carry=empty), sab(q, k1, v1, Sq, S_rem, B, H, carry=empty, partial=True)
    none, none_p = sab(q, k1, v1, Sq, S_rem, B, H, kv_skip=(0, 0)), sab(q, k1, v1, Sq, S_rem, B, H, kv_skip=(0, 0), partial=True)
    torch.cuda.synchronize()
    assert torch.equal(got, plain) and torch.equal(got_p[0], plain_p[0]) and torch.equal(got_p[1], plain_p[1])
    assert torch.equal(none, plain) and torch.equal(none_p[0], plain_p[0]) and torch.equal(none_p[1], plain_p[1])
    fresh = sab(q, k1, v1, Sq, S_rem, B, H, carry=own, partial=True)
    o_alias = own[0].clone()
    inplace = sab(q, k1, v1, Sq, S_rem, B, H, carry=(o_alias, own[1]), out=o_alias, partial=True)
    torch.cuda.synchronize()
    assert inplace[0].data_ptr() == o_alias.data_ptr()
    assert torch.equal(inplace[0], fresh[0]) and torch.equal(inplace[1], fresh[1])


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("Sq,L,world", SHAPES)
def test_chains(Sq, L, world, B, H):
    """both remote schedules on every rank against each other and against fp32; a two-launch chain's fp32 state against ONE bounded call over all keys"""
    from gen3c_amd import ops
    bd, S = _bound(1.0), world * L
    for kind in ("random", "pos", "neg"):
        q, k, v, vt, vseg, ref = _problem(Sq, L, world, B, H, 1.0, kind)
        one = ops.self_attn_bounded(q, k, vseg, Sq, S, B, H, bd, variant=11, partial=True)  # ONE bounded call over all keys, fp32
        for rank in range(world):
            lf = _local_first(q, k, vseg, Sq, L, world, rank, B, H, bd)
            lc = _local_carry(q, k, vseg, Sq, L, world, rank, B, H, bd)
            own = ops.self_attn_bounded(q, *_blocks(k, vseg, L, B, rank, rank + 1), Sq, L, B, H, bd, variant=11, partial=True)
            kk, vv, skip = _remote(k, vseg, L, world, rank, B)
            two = ops.self_attn_bounded(q, kk, vv, Sq, (world - 1) * L, B, H, bd, variant=11, carry=own, kv_skip=skip, partial=True)
            torch.cuda.synchronize()
            r_cm, r_lf, r_lc = _rel(lc, lf), _rel(lf, ref), _rel(lc, ref)
            r_two = _rel(two[0], one[0])
            d_lse = float((two[1] - one[1]).abs().max())
            print(f"[bounded cp {kind} Sq={Sq} L={L} world={world} rank={rank} B={B} H={H}] carry vs merge {r_cm:.3e}, local_first vs fp32 {r_lf:.3e}, "
                  f"local_carry vs fp32 {r_lc:.3e}, two-launch fp32 state vs one call {r_two:.3e}, |dLSE| {d_lse:.3e}")
            assert torch.isfinite(lf.float()).all() and torch.isfinite(lc.float()).all()
            assert r_cm < 1e-3, (kind, rank, r_cm)
            assert r_lf < 4e-3 and r_lc < 4e-3, (kind, rank, r_lf, r_lc)
            assert r_two <= 1e-3 and d_lse <= 1e-4, (kind, rank, r_two, d_lse)


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("Sq,L,world", [s for s in SHAPES if s[2] >= 3])  # three key blocks need world >= 3 (L = 64 at world 2: 128 keys are two tiles)
def test_three_launch_chain(Sq, L, world, B, H):
    """partial -> partial with carry -> final with carry over the blocks [0], [1], [2, world) against the merge of the same three parts and fp32"""
    from gen3c_amd import ops
    bd = _bound(1.0)
    for kind in ("random", "pos", "neg"):
        q, k, v, vt, vseg, ref = _problem(Sq, L, world, B, H, 1.0, kind)
        sab = lambda *a, **kw: ops.self_attn_bounded(*a, bd, variant=11, **kw)
        spans = ((0, 1), (1, 2), (2, world))
        parts = [sab(q, *_blocks(k, vseg, L, B, r0, r1), Sq, (r1 - r0) * L, B, H, partial=True) for r0, r1 in spans]
        p2 = sab(q, *_blocks(k, vseg, L, B, 1, 2), Sq, L, B, H, carry=parts[0], partial=True)
        out = sab(q, *_blocks(k, vseg, L, B, 2, world), Sq, (world - 2) * L, B, H, carry=p2)
        merged = ops.attn_merge(parts, Sq, B, H)
        torch.cuda.synchronize()
        print(f"[bounded cp three launches {kind} Sq={Sq} L={L} world={world} B={B} H={H}] vs merge {_rel(out, merged):.3e}, vs fp32 {_rel(out, ref):.3e}")
        assert _rel(out, merged) < 1e-3 and _rel(out, ref) < 4e-3, (kind, _rel(out, merged), _rel(out, ref))


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("Sq,L,world", SHAPES)
def test_mixed_chains(Sq, L, world, B, H):
    """A bounded part and a max-form part of the same rows: LSE of the no-max form (m_run = bound) is the log-sum-exp the max form writes, so they merge
    and carry into each other. Part A = block 0, part B = the other blocks, V one random row per part (module docstring); everything is compared as the
    fp32 partials the kernels write, against ONE bounded call over all keys."""
    from gen3c_amd import ops
    q, k, v, vt, vseg, ref = _problem(Sq, L, world, B, H, 1.0, "pos", True)
    bd, S, S_b = _bound(1.0), world * L, (world - 1) * L
    one = ops.self_attn_bounded(q, k, vseg, Sq, S, B, H, bd, variant=11, partial=True)
    ka, va = _blocks(k, vseg, L, B, 0, 1)
    kb, vb = _blocks(k, vseg, L, B, 1, world)
    a_nm, a_mx = _attn(bd)(q, ka, va, Sq, L, B, H, partial=True), _attn(None)(q, ka, va, Sq, L, B, H, partial=True)
    b_nm, b_mx = _attn(bd)(q, kb, vb, Sq, S_b, B, H, partial=True), _attn(None)(q, kb, vb, Sq, S_b, B, H, partial=True)
    d_lse = max(float((a_nm[1] - a_mx[1]).abs().max()), float((b_nm[1] - b_mx[1]).abs().max()))
    res = {}
    for name, (pa, pb) in (("merge nm+max", (a_nm, b_mx)), ("merge max+nm", (a_mx, b_nm))):
        m32, l32 = _merge32(pa, pb, Sq, B, H)
        res[name] = (_rel(m32, one[0]), float((l32 - _rowsof(one[1], Sq, B, H)).abs().max()))
        assert _rel(ops.attn_merge([pa, pb], Sq, B, H), m32) <= 2.0 ** -9 + 1e-5  # the merge kernel on the same parts: m32 rounded to bf16
    c1 = _attn(bd)(q, kb, vb, Sq, S_b, B, H, carry=a_mx, partial=True)    # max-form state carried into a bounded launch
    c2 = _attn(None)(q, kb, vb, Sq, S_b, B, H, carry=a_nm, partial=True)  # bounded state carried into a max-form launch
    torch.cuda.synchronize()
    for name, c in (("carry max->nm", c1), ("carry nm->max", c2)):
        res[name] = (_rel(c[0], one[0]), float((c[1] - one[1]).abs().max()))
    print(f"[bounded cp mixed Sq={Sq} L={L} world={world} B={B} H={H}] max |LSE nm - LSE max| {d_lse:.3e}; "
          + "; ".join(f"{n}: {r:.3e}, |dLSE| {d:.3e}" for n, (r, d) in res.items()) + f"; one call vs fp32 softmax {_rel(one[0], ref):.3e}")
    assert d_lse <= 1e-4
    for n, (r, d) in res.items():
        assert r <= 1e-3 and d <= 1e-4, (n, r, d)


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("Sq,L,world", SHAPES)
def test_chains_near_the_bound_limit(Sq, L, world, B, H):
    """w_q = w_k = 1.85: bound 57.5 in the log2 domain. The fp32 softmax is sharp and the max form itself sits near 4e-3, so the bounded chains are held
    against the max-form chains on the same inputs (the ratio bar of test_bounded_self_attention_vs_fp32)."""
    bd = _bound(1.85)
    assert 57.0 < bd * math.log2(math.e) < 60.0
    for kind in ("pos", "neg"):
        q, k, v, vt, vseg, ref = _problem(Sq, L, world, B, H, 1.85, kind)
        for rank in range(world):
            for chain in (_local_first, _local_carry):
                out = chain(q, k, vseg, Sq, L, world, rank, B, H, bd)
                out_max = chain(q, k, vseg, Sq, L, world, rank, B, H, None)
                torch.cuda.synchronize()
                e_nm, e_max = _rel(out, ref), _rel(out_max, ref)
                print(f"[bounded cp w=1.85 {kind} {chain.__name__} Sq={Sq} L={L} world={world} rank={rank} B={B} H={H}] rel-L2 vs fp32: no-max {e_nm:.3e}, "
                      f"max form {e_max:.3e}, ratio {e_nm / e_max:.3f}")
                assert torch.isfinite(out.float()).all()
                assert e_nm <= 1.5 * e_max, (kind, rank, chain.__name__, e_nm, e_max)


def test_fallbacks_are_bitwise_the_carry_entry():
    """bound 0, beyond 60 / log2(e), negative, and variant 4: the call IS g3_flash_attn_fwd_carry_bf16 - outputs and kernel name"""
    from gen3c_amd import _lib, ops
    Sq, L, world, B, H, rank = 200, 128, 3, 1, 8, 1
    q, k, v, vt, vseg, _ = _problem(Sq, L, world, B, H, 1.0, "pos")
    S_rem = (world - 1) * L
    lib = _lib.load()
    over = 60.5 / math.log2(math.e)
    for bound, variant in ((0.0, 11), (over, 11), (-1.0, 11), (_bound(1.0), 4)):
        own = ops.flash_attn(q, *_blocks(k, vseg, L, B, rank, rank + 1), Sq, L, B, H, partial=True, out=None, kv_skip=(0, 0), variant=variant)
        calls = (dict(carry=own, kv_skip=(rank * L, L)), dict(carry=own, kv_skip=(rank * L, L), partial=True), dict(kv_skip=(rank * L, L)), dict(kv_skip=(0, 0)))
        for kw in calls:
            for vv in (vseg, vt):
                kk = k if kw["kv_skip"][1] else k[:S_rem * B]
                vx = vv if kw["kv_skip"][1] else (vv[:world - 1] if vv.dim() == 5 else vv[..., :S_rem].contiguous())
                want, name_c = _launched(lambda: ops.flash_attn(q, kk, vx, Sq, S_rem, B, H, variant=variant, **kw))
                got, name_b = _launched(lambda: ops.self_attn_bounded(q, kk, vx, Sq, S_rem, B, H, bound, variant=variant, **kw))
                torch.cuda.synchronize()
                cp_form = "carry" in kw or kw["kv_skip"][1] > 0
                assert name_b == name_c == _cp_name(Sq, S_rem, B, H, bound, variant, vv.dim() == 5, cp_form) and name_b not in (NM, NMC), (bound, variant, name_b, name_c)
                assert name_c == (CARRY if variant == 11 else "flash_attn_fwd_v3_kernel<3, 6, 8, false>")
                if isinstance(want, tuple):
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (bound, variant, kw.keys())
                else:
                    assert torch.equal(got, want), (bound, variant, kw.keys())
    assert _cp_name(Sq, S_rem, B, H, 60.0 / math.log2(math.e) * 0.999, 11, 1, 1) == NMC  # the limit itself is inside
    # the no-max form really is another kernel: same function, not the same bits as the max form's chain
    a = _local_carry(q, k, vseg, Sq, L, world, rank, B, H, _bound(1.0))
    b = _local_carry(q, k, vseg, Sq, L, world, rank, B, H, None)
    assert _rel(a, b) < 6e-3
    assert lib.g3_self_attn_kernel_name(Sq, S_rem, B, H, float(_bound(1.0)), 11).decode() == NM  # (the plain bounded entry's query is unchanged)


def test_refusals_do_not_launch():
    """the refusal cases of tests/test_attn_carry_gpu.py::test_refusals_do_not_launch through the bounded entry, with a usable bound: G3_ERR_ARG, output untouched"""
    from gen3c_amd import _lib, ops
    Sq, L, world, B, H = 128, 128, 3, 1, 2
    g = torch.Generator(device="cpu").manual_seed(2)
    S = world * L
    q = torch.randn(Sq * B, H * 128, generator=g).to(torch.bfloat16).to(DEV)
    k = torch.randn(S * B, H * 128, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(S * B, H * 128, generator=g).to(torch.bfloat16).to(DEV)
    vt = ops.transpose_v(v, S, B, H)
    vseg = torch.stack([ops.transpose_v(v[r * L * B:(r + 1) * L * B], L, B, H) for r in range(world)])
    bd = 40.0  # |q . k| / sqrt(128) of unnormalised N(0, 1) rows stays far below it; nothing here launches anyway
    own = ops.flash_attn(q, k[:L * B].contiguous(), vseg[:1].contiguous(), Sq, L, B, H, partial=True, variant=4)
    S_rem = 2 * L
    sab = lambda *a, **kw: ops.self_attn_bounded(*a, bd, **kw)

    def refused(fn, msg):
        out = torch.full((Sq * B, H * 128), 7.0, dtype=torch.bfloat16, device=DEV)
        torch.cuda.synchronize()
        with pytest.raises(_lib.Gen3cHipError, match=msg) as ei:
            fn(out)
        assert f"rc={_lib.G3_ERR_ARG}" in str(ei.value)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call must not launch"

    for variant in (4, 11):
        refused(lambda o: sab(q, k, vseg, Sq, S_rem, B, H, out=o, kv_skip=(32, 128), variant=variant), "multiples of 64")
        refused(lambda o: sab(q, k[:(S_rem + 64) * B], vt[..., :S_rem + 64].contiguous(), Sq, S_rem, B, H, out=o, kv_skip=(S_rem + 64, 64), variant=variant),
                "0 <= begin")
        refused(lambda o: sab(q, k, vseg, Sq, S_rem, B, H, out=o, kv_skip=(64, 128), variant=variant), "whole V\\^T segments")
    for bad in (1, 2, 9):
        refused(lambda o: sab(q, k, vseg, Sq, S_rem, B, H, out=o, carry=own, kv_skip=(L, L), variant=bad), "carry / key-skip form")
    # variant 11 on a ragged key count resolves to w4 (9): no carry form, bounded or not
    refused(lambda o: sab(q, k[:100 * B], ops.transpose_v(v[:100 * B], 100, B, H), Sq, 100, B, H, out=o, kv_skip=(0, 0), variant=11), "carry / key-skip form")
    # V^T leading dimension below ceil64 of the keys: only the 64-bit-addressing kernel could run it
    vt_short = torch.zeros(B, H, 128, 104, dtype=torch.bfloat16, device=DEV)
    for variant in (4, 11):
        refused(lambda o: sab(q, k[:100 * B], vt_short, Sq, 100, B, H, out=o, kv_skip=(0, 0), variant=variant), "64-bit-addressing")  # (checked ahead of the kernel choice)
    # misaligned carry_o (4 bytes off), same strides as the output
    wide = torch.zeros(Sq * B, H * 128 + 8, dtype=torch.float32, device=DEV)
    co = wide[:, 1:1 + H * 128]
    for variant in (4, 11):
        out32 = torch.full_like(wide, 7.0)
        torch.cuda.synchronize()
        with pytest.raises(_lib.Gen3cHipError, match="misaligned carry_o"):
            sab(q, k, vseg, Sq, S_rem, B, H, out=out32[:, :H * 128], partial=True, carry=(co, own[1]), kv_skip=(0, L), variant=variant)
        torch.cuda.synchronize()
        assert bool((out32 == 7.0).all())
    # K rows 256 MiB apart: the span exceeds the kernels' 32-bit byte offsets - refused, not run bounded (the operands are small: nothing reads them)
    q1 = torch.zeros(64, 128, dtype=torch.bfloat16, device=DEV)
    k1 = torch.zeros(128, 128, dtype=torch.bfloat16, device=DEV)
    vt1 = torch.zeros(1, 1, 128, 128, dtype=torch.bfloat16, device=DEV)
    out = torch.full((64, 128), 7.0, dtype=torch.bfloat16, device=DEV)
    lib = _lib.load()
    torch.cuda.synchronize()
    for variant in (4, 11):
        rc = lib.g3_self_attn_fwd_bounded_cp_bf16(q1.data_ptr(), 128, 128, 128, k1.data_ptr(), 1 << 27, 128, 128, vt1.data_ptr(), 128, 128 * 128, 128 * 128, 0, 0, 0, 0,
                                                  None, None, out.data_ptr(), None, None, 128, 128, 128, 64, 128, 1, 1, 128, 1.0 / math.sqrt(128), bd, variant,
                                                  torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.G3_ERR_ARG and "32-bit byte offsets" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
