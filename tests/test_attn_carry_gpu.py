"""GPU: the carry-in / skipped-key-range form of the self-attention kernels (g3_flash_attn_fwd_carry_bf16 through ops.flash_attn(carry=...,
kv_skip=...)) on both kernels that context parallelism launches - 11 (one wave per SIMD) and 4 (8 waves; its short- and long-context
instantiations). Layout as under context parallelism: `world` key blocks of S_local keys, the queries of one rank, its own block skipped."""
import pytest
import torch

from gen3c_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VARIANTS = (11, 4)


def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm())


def _problem(Sq, L, world, B, H, seed):
    """q [Sq*B, H*128]; k / v over world * L keys ([S*B, H*128], rows (s, b)); V^T plain [B,H,128,S] and in rank segments [world,B,H,128,L]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    S = world * L
    q = torch.randn(Sq * B, H * 128, generator=g).to(torch.bfloat16).to(DEV)
    k = torch.randn(S * B, H * 128, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(S * B, H * 128, generator=g).to(torch.bfloat16).to(DEV)
    vt = ops.transpose_v(v, S, B, H)
    vseg = torch.stack([ops.transpose_v(v[r * L * B:(r + 1) * L * B], L, B, H) for r in range(world)])
    return q, k, v, vt, vseg


def _blocks(k, vseg, L, B, r0, r1):
    """contiguous copies of key blocks [r0, r1): K rows, segmented V^T"""
    return k[r0 * L * B:r1 * L * B].contiguous(), vseg[r0:r1].contiguous()


def _ref_fp32(q, k, v, Sq, B, H, rows=None):
    """fp32 softmax attention of (a subset of) the query positions over all keys of k / v"""
    S = k.shape[0] // B
    qs = q.float().reshape(Sq, B, H, 128)
    if rows is not None:
        qs = qs[rows]
    k4 = k.float().reshape(S, B, H, 128).permute(1, 2, 3, 0)  # [B,H,128,S]
    v4 = v.float().reshape(S, B, H, 128).permute(1, 2, 0, 3)  # [B,H,S,128]
    out = []
    for b in range(B):
        sc = torch.einsum("shd,hdk->hsk", qs[:, b], k4[b]) / 128 ** 0.5
        out.append(torch.einsum("hsk,hkd->shd", torch.softmax(sc, dim=-1), v4[b]))
    return torch.stack(out, 1).reshape(-1, H * 128)


def _remote(k, vseg, L, world, rank, B):
    """every key but the rank's own block: a sub-range on the first / last rank, the whole buffers with a skip on an interior one"""
    if rank == 0:
        return k[L * B:], vseg[1:], None
    if rank == world - 1:
        return k[:rank * L * B], vseg[:rank], None
    return k, vseg, (rank * L, L)


def _cp_step(q, k, vseg, Sq, L, world, rank, B, H, variant):
    """own block -> fp32 partial, then ONE carry launch over every other block (skip of the own block on an interior rank)"""
    k_own, v_own = _blocks(k, vseg, L, B, rank, rank + 1)
    own = ops.flash_attn(q, k_own, v_own, Sq, L, B, H, partial=True, variant=variant)
    kk, vv, skip = _remote(k, vseg, L, world, rank, B)
    out = ops.flash_attn(q, kk, vv, Sq, (world - 1) * L, B, H, carry=own, kv_skip=skip, variant=variant)
    return own, out


def _merge_ref(q, k, vseg, Sq, L, world, rank, B, H, variant, own):
    """ops.attn_merge of the SAME two partials: the own block's and the remote launch's own part (same keys, same tiles, so the bf16 P
    fragments round alike and only the fold differs from the merge)"""
    kk, vv, skip = _remote(k, vseg, L, world, rank, B)
    rem = ops.flash_attn(q, kk, vv, Sq, (world - 1) * L, B, H, kv_skip=skip, partial=True, variant=variant)
    return ops.attn_merge([own, rem], Sq, B, H)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("Sq,L,world,B,H", [(200, 256, 3, 1, 2), (333, 512, 4, 2, 2), (450, 1536, 3, 1, 2)])  # remote 512 .. 3 072 keys
def test_carry_small_shapes(variant, Sq, L, world, B, H):
    q, k, v, vt, vseg = _problem(Sq, L, world, B, H, seed=Sq + L)
    for rank in range(world):
        own, out = _cp_step(q, k, vseg, Sq, L, world, rank, B, H, variant)
        merged = _merge_ref(q, k, vseg, Sq, L, world, rank, B, H, variant, own)
        ref = _ref_fp32(q, k, v, Sq, B, H)
        torch.cuda.synchronize()
        assert _rel(out, merged) < 1e-3, (rank, _rel(out, merged))
        assert _rel(out, ref) < 4e-3, (rank, _rel(out, ref))


@pytest.mark.parametrize("variant", VARIANTS)
def test_carry_cp8_rank_shape(variant):
    """the cp = 8 rank shape of the product: S_local = 7 040, B = 2, 8 heads per group, 49 280 remote keys"""
    L, world, B, H = 7040, 8, 2, 8
    q, k, v, vt, vseg = _problem(L, L, world, B, H, seed=8)
    del vt
    rows = torch.arange(0, L, 37, device=DEV)  # fp32 reference on a subset of the query positions (the full score matrix is 22 GB)
    for rank in (0, 3, 7):
        own, out = _cp_step(q, k, vseg, L, L, world, rank, B, H, variant)
        merged = _merge_ref(q, k, vseg, L, L, world, rank, B, H, variant, own)
        torch.cuda.synchronize()
        assert _rel(out, merged) < 1e-3, (rank, _rel(out, merged))
        ref = _ref_fp32(q, k, v, L, B, H, rows=rows)
        sub = out.view(L, B, H * 128)[rows].reshape(-1, H * 128)
        assert _rel(sub, ref) < 4e-3, (rank, _rel(sub, ref))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("segmented", [False, True])
def test_kv_skip_bitwise(variant, segmented):
    """a skipped range == the same kernel on a contiguous copy of the kept keys: same keys, same order, same tiles -> bit for bit"""
    Sq, L, world, B, H = 300, 256, 4, 2, 2
    q, k, v, vt, vseg = _problem(Sq, L, world, B, H, seed=5)
    for rank in (1, 2):
        b0, n = rank * L, L
        k_kept = torch.cat([k[:b0 * B], k[(b0 + n) * B:]]).contiguous()
        if segmented:
            vv, v_kept = vseg, torch.cat([vseg[:rank], vseg[rank + 1:]]).contiguous()
        else:
            vv, v_kept = vt, torch.cat([vt[..., :b0], vt[..., b0 + n:]], dim=-1).contiguous()
        S_rem = (world - 1) * L
        a = ops.flash_attn(q, k, vv, Sq, S_rem, B, H, kv_skip=(b0, n), variant=variant)
        b = ops.flash_attn(q, k_kept, v_kept, Sq, S_rem, B, H, kv_skip=(0, 0), variant=variant)
        ao, al = ops.flash_attn(q, k, vv, Sq, S_rem, B, H, kv_skip=(b0, n), partial=True, variant=variant)
        bo, bl = ops.flash_attn(q, k_kept, v_kept, Sq, S_rem, B, H, kv_skip=(0, 0), partial=True, variant=variant)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(ao, bo) and torch.equal(al, bl)
    # a skip at the front (a different base) and one at the very end (nothing skipped) are the same launch too
    a = ops.flash_attn(q, k, vseg if segmented else vt, Sq, 3 * L, B, H, kv_skip=(0, L), variant=variant)
    b = ops.flash_attn(q, k[L * B:].contiguous(), vseg[1:].contiguous() if segmented else vt[..., L:].contiguous(), Sq, 3 * L, B, H, kv_skip=(0, 0),
                       variant=variant)
    c = ops.flash_attn(q, k, vseg if segmented else vt, Sq, 3 * L, B, H, kv_skip=(3 * L, L), variant=variant)
    d = ops.flash_attn(q, k[:3 * L * B].contiguous(), vseg[:3].contiguous() if segmented else vt[..., :3 * L].contiguous(), Sq, 3 * L, B, H,
                       kv_skip=(0, 0), variant=variant)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(c, d)


@pytest.mark.parametrize("variant", VARIANTS)
def test_three_launch_chain(variant):
    """fp32 -> carry -> fp32 -> carry -> bf16 == the merge of the three parts"""
    Sq, L, B, H = 290, 512, 2, 2
    q, k, v, vt, vseg = _problem(Sq, L, 3, B, H, seed=3)
    parts = [ops.flash_attn(q, *_blocks(k, vseg, L, B, r, r + 1), Sq, L, B, H, partial=True, variant=variant) for r in range(3)]
    p1 = parts[0]
    p2 = ops.flash_attn(q, *_blocks(k, vseg, L, B, 1, 2), Sq, L, B, H, carry=p1, partial=True, variant=variant)
    out = ops.flash_attn(q, *_blocks(k, vseg, L, B, 2, 3), Sq, L, B, H, carry=p2, variant=variant)
    merged = ops.attn_merge(parts, Sq, B, H)
    ref = _ref_fp32(q, k, v, Sq, B, H)
    torch.cuda.synchronize()
    assert _rel(out, merged) < 1e-3 and _rel(out, ref) < 4e-3, (_rel(out, merged), _rel(out, ref))
    # the middle state is the merge of the first two parts, in fp32
    m2 = ops.attn_merge(parts[:2], Sq, B, H)
    assert _rel(p2[0], m2) < 1e-2


@pytest.mark.parametrize("variant", VARIANTS)
def test_in_place_and_empty_carry(variant):
    Sq, L, B, H = 257, 512, 1, 2
    q, k, v, vt, vseg = _problem(Sq, L, 2, B, H, seed=9)
    k0, v0 = _blocks(k, vseg, L, B, 0, 1)
    k1, v1 = _blocks(k, vseg, L, B, 1, 2)
    own = ops.flash_attn(q, k0, v0, Sq, L, B, H, partial=True, variant=variant)
    fresh = ops.flash_attn(q, k1, v1, Sq, L, B, H, carry=own, partial=True, variant=variant)
    o_alias = own[0].clone()
    inplace = ops.flash_attn(q, k1, v1, Sq, L, B, H, carry=(o_alias, own[1]), out=o_alias, partial=True, variant=variant)
    torch.cuda.synchronize()
    assert inplace[0].data_ptr() == o_alias.data_ptr()
    assert torch.equal(inplace[0], fresh[0]) and torch.equal(inplace[1], fresh[1])
    # carry_lse = -inf: no earlier keys - whatever carry_o holds, the result is the plain launch's, bit for bit
    empty = (torch.full_like(own[0], float("nan")), torch.full_like(own[1], float("-inf")))
    plain = ops.flash_attn(q, k1, v1, Sq, L, B, H, kv_skip=(0, 0), variant=variant)
    got = ops.flash_attn(q, k1, v1, Sq, L, B, H, carry=empty, variant=variant)
    plain_p = ops.flash_attn(q, k1, v1, Sq, L, B, H, kv_skip=(0, 0), partial=True, variant=variant)
    got_p = ops.flash_attn(q, k1, v1, Sq, L, B, H, carry=empty, partial=True, variant=variant)
    torch.cuda.synchronize()
    assert torch.equal(got, plain) and torch.equal(got_p[0], plain_p[0]) and torch.equal(got_p[1], plain_p[1])
    # and the carry-less launch through the carry entry point equals the existing entry point (the same arithmetic, bit for bit)
    ex = ops.flash_attn(q, k1, v1, Sq, L, B, H, variant=variant)
    torch.cuda.synchronize()
    assert torch.equal(plain, ex)


def test_refusals_do_not_launch():
    Sq, L, world, B, H = 128, 128, 3, 1, 2
    q, k, v, vt, vseg = _problem(Sq, L, world, B, H, seed=2)
    own = ops.flash_attn(q, *_blocks(k, vseg, L, B, 0, 1), Sq, L, B, H, partial=True, variant=4)
    S_rem = 2 * L

    def refused(fn, msg):
        out = torch.full((Sq * B, H * 128), 7.0, dtype=torch.bfloat16, device=DEV)
        torch.cuda.synchronize()
        with pytest.raises(_lib.Gen3cHipError, match=msg):
            fn(out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call must not launch"

    refused(lambda o: ops.flash_attn(q, k, vseg, Sq, S_rem, B, H, out=o, kv_skip=(32, 128), variant=4), "multiples of 64")
    refused(lambda o: ops.flash_attn(q, k[:(S_rem + 64) * B], vt[..., :S_rem + 64].contiguous(), Sq, S_rem, B, H, out=o, kv_skip=(S_rem + 64, 64), variant=4),
            "0 <= begin")
    refused(lambda o: ops.flash_attn(q, k, vseg, Sq, S_rem, B, H, out=o, kv_skip=(64, 128), variant=4), "whole V\\^T segments")
    for bad in (1, 2, 9):
        refused(lambda o: ops.flash_attn(q, k, vseg, Sq, S_rem, B, H, out=o, carry=own, kv_skip=(L, L), variant=bad), "carry / key-skip form")
    # variant 11 on a ragged key count resolves to w4 (9): no carry form either
    refused(lambda o: ops.flash_attn(q, k[:100 * B], ops.transpose_v(v[:100 * B], 100, B, H), Sq, 100, B, H, out=o, kv_skip=(0, 0), variant=11),
            "carry / key-skip form")
    # V^T leading dimension below ceil64 of the keys: only the 64-bit-addressing kernel could run it
    vt_short = torch.zeros(B, H, 128, 104, dtype=torch.bfloat16, device=DEV)
    refused(lambda o: ops.flash_attn(q, k[:100 * B], vt_short, Sq, 100, B, H, out=o, kv_skip=(0, 0), variant=4), "64-bit-addressing")
    # misaligned carry_o (4 bytes off), same strides as the output
    wide = torch.zeros(Sq * B, H * 128 + 8, dtype=torch.float32, device=DEV)
    co = wide[:, 1:1 + H * 128]
    out32 = torch.full_like(wide, 7.0)
    torch.cuda.synchronize()
    with pytest.raises(_lib.Gen3cHipError, match="misaligned carry_o"):
        ops.flash_attn(q, k, vseg, Sq, S_rem, B, H, out=out32[:, :H * 128], partial=True, carry=(co, own[1]), kv_skip=(0, L), variant=4)
    torch.cuda.synchronize()
    assert bool((out32 == 7.0).all())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("segmented", [False, True])
def test_kv_skip_from_tile_one_bitwise(variant, segmented):
    """S_local = 64: the skip starts at logical tile 1 (rank 1) or 2 (rank 2), where the w4b prologue / its first V^T walk step take the jump"""
    Sq, L, world, B, H = 200, 64, 4, 2, 2
    q, k, v, vt, vseg = _problem(Sq, L, world, B, H, seed=11)
    for rank in (1, 2):
        b0 = rank * L
        k_kept = torch.cat([k[:b0 * B], k[(b0 + L) * B:]]).contiguous()
        if segmented:
            vv, v_kept = vseg, torch.cat([vseg[:rank], vseg[rank + 1:]]).contiguous()
        else:
            vv, v_kept = vt, torch.cat([vt[..., :b0], vt[..., b0 + L:]], dim=-1).contiguous()
        own = ops.flash_attn(q, *_blocks(k, vseg, L, B, rank, rank + 1), Sq, L, B, H, partial=True, variant=variant)
        a = ops.flash_attn(q, k, vv, Sq, 3 * L, B, H, carry=own, kv_skip=(b0, L), variant=variant)
        b = ops.flash_attn(q, k_kept, v_kept, Sq, 3 * L, B, H, carry=own, kv_skip=(0, 0), variant=variant)
        torch.cuda.synchronize()
        assert torch.equal(a, b), rank


def test_refuses_span_beyond_32bit_offsets():
    """K rows 256 MiB apart: the K span the carry form would address exceeds 4 GiB - refused (no 64-bit-addressing carry kernel), not launched.
    The operands are small: the launcher refuses before anything reads them."""
    import math
    Sq, Skv, H = 64, 128, 1
    q = torch.zeros(Sq, H * 128, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros(Skv, H * 128, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(1, H, 128, Skv, dtype=torch.bfloat16, device=DEV)
    out = torch.full((Sq, H * 128), 7.0, dtype=torch.bfloat16, device=DEV)
    lib = _lib.load()
    torch.cuda.synchronize()
    for variant in VARIANTS:
        rc = lib.g3_flash_attn_fwd_carry_bf16(q.data_ptr(), H * 128, H * 128, 128, k.data_ptr(), 1 << 27, H * 128, 128, vt.data_ptr(), Skv, H * 128 * Skv,
                                              128 * Skv, 0, 0, 0, 0, None, None, out.data_ptr(), None, None, H * 128, H * 128, 128, Sq, Skv, 1, H, 128,
                                              1.0 / math.sqrt(128), variant, torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and "32-bit byte offsets" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
