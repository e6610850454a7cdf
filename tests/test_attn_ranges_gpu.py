"""GPU: range-table self-attention (g3_self_attn_fwd_ranges_bf16; flash_attn_fwd_w4b_nm_rng_kernel / flash_attn_fwd_w4b_rng_kernel): every workgroup of the
one-wave-per-SIMD kernel loads its block's list of key ranges in the pattern of its head, clamps it, and walks it with a cursor in scalar registers.
ops.ranges_attn_mask is the function.

Inputs as in tests/test_attn_window_gpu.py: q, k behind a per-head RMSNorm with unit weights (column views of fused buffers, as the DiT passes them),
random v; head dim 128; BOUND = sqrt(128) * 1.03. Both kernel forms run on every case and the kernel's name is asserted per launch. The hand-made
tables are for the kernel alone and do not depend on the builders; g3_attn_ranges_check is what tests/test_attn_ranges_cpu.py tests.

The element-level check of these kernels - exact fp64 probes in which every (head, query block, tile) triple owns an output element, guarded K and
O, every launch twice, the 64-range table, the staircases across range jumps - is family 7 of tests/test_attn_probes_gpu.py; operands spanning
2^31 / 2^32 bytes are the rng_* kinds of tests/test_far_operands_gpu.py. Here: the Gaussian bar, the bitwise oracles, and the one promise the
header makes about a table that breaks the rules (test_the_kernel_clamps_a_rule_breaking_table_to_the_operand).

 1. S 832, B = H = 1, max_ranges 8: block 0 = tile {0}; block 1 = tiles {0}, {2}; block 2 = tiles {1}, {5}, {12}; block 3 (64 rows) = [0, 2), {3}, [6, 13):
    nt = 1, 2, 3; the prologue's K(1) / V^T(1) out of a second range; the t + 2 clamp; the last tile of the operand.
 2. S 1920, B = H = 2 (3-D grid), 2 patterns, head_pattern [1, 0]: seeded random lists of 1 to 6 ranges of random lengths, some touching: range changes
    with and without a jump, the head-to-pattern lookup, batch strides.
 3. S 8256, B 1, H 8 (1-D XCD grid), max_ranges 64, 2 patterns, head_pattern [0, 1, 0, 1, 1, 0, 1, 0]: one block with 64 one-tile ranges on tiles 0, 2, ...,
    126, one with 63, the rest seeded random: a cursor step on every tile, table lanes >= 32, the 1-D grid's head decode.

Bars.
 * worst (batch, head) rel-L2 against an fp64 softmax masked by ops.ranges_attn_mask < 4e-3, the bar of the existing attention tests.
 * bit for bit, block by block (shapes 1, 2): the keys of every query block's list, gathered in list order into a contiguous copy, through the existing
   carry entry (variant 11) with an empty carry (the form that shares the epilogue) - concatenated, the outputs EQUAL the launch.
 * bit for bit, whole launch: ops.self_attn_ranges on sparse_attn.frame_ranges(...) EQUALS ops.self_attn_window, in both forms.
 * sparse_attn.radial_ranges(6, 1024, 0.25, 1) at S 6144: below 4e-3 against the masked fp64 softmax; tile_density = attended / dense = 0.646."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import attn_probe_ref as R

pytestmark = pytest.mark.gpu

HD = 128
BOUND = HD / math.sqrt(HD) * 1.03  # unit RMSNorm weights: |q . k| / sqrt(128) <= sqrt(128), plus the margin for the bf16 roundings of q and k
NM_RNG, MAX_RNG = "flash_attn_fwd_w4b_nm_rng_kernel<true>", "flash_attn_fwd_w4b_rng_kernel<true>"
NM_WIN, MAX_WIN = "flash_attn_fwd_w4b_nm_win_kernel<true>", "flash_attn_fwd_w4b_win_kernel<true>"
NM_CARRY, MAX_CARRY = "flash_attn_fwd_w4b_nm_carry_kernel<true>", "flash_attn_fwd_w4b_carry_kernel<true>"


def _rms(x):
    x = x.float().view(x.shape[0], -1, HD)
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True))).reshape(x.shape[0], -1)


@functools.lru_cache(maxsize=None)
def _problem(S, B, H):
    """q [S*B, H*128] = first half of a fused [S*B, 2 H 128] buffer, k = second half of another; v, V^T. Built once per shape, shared, never written."""
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(S + 7 * B + H)
    D = H * HD
    qbuf = torch.randn(S * B, 2 * D, device=dev, generator=g)
    kbuf = torch.randn(S * B, 2 * D, device=dev, generator=g)
    qbuf = torch.cat([_rms(qbuf[:, :D]), qbuf[:, D:]], dim=1).to(torch.bfloat16)
    kbuf = torch.cat([kbuf[:, :D], _rms(kbuf[:, D:])], dim=1).to(torch.bfloat16)
    v = torch.randn(S * B, D, device=dev, generator=g).to(torch.bfloat16)
    q, k = qbuf[:, :D], kbuf[:, D:]
    assert not q.is_contiguous() and not k.is_contiguous()
    return q, k, v, ops.transpose_v(v, S, B, H)


def _fp64(S, B, H, masks):
    """masks[h]: CPU bool [S, S] of head h -> the masked softmax in fp64, [S*B, H*128]"""
    q, k, v, _ = _problem(S, B, H)
    out = torch.empty(S * B, H * HD, device="cuda:0", dtype=torch.float64)
    dev_masks = {}
    for h in range(H):
        m = dev_masks.setdefault(id(masks[h]), masks[h].to("cuda:0"))
        sl = slice(h * HD, (h + 1) * HD)
        for b in range(B):
            sc = (q[b::B, sl].double() @ k[b::B, sl].double().t()) / math.sqrt(HD)
            out[b::B, sl] = torch.softmax(sc.masked_fill_(~m, -math.inf), dim=-1) @ v[b::B, sl].double()
    return out


def _worst_pair(out, ref, B, H):
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    return max(rel(out[b::B, h * HD:(h + 1) * HD], ref[b::B, h * HD:(h + 1) * HD]) for b in range(B) for h in range(H))


def _timed(f):
    """(result, metadata of the attention launches f made)"""
    from gen3c_amd import ops
    ops.enable_kernel_timers(True)
    try:
        out = f()
        metas = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    finally:
        ops.enable_kernel_timers(False)
    return out, metas


_pack, _random_list = R.pack, R.random_list  # (shared with family 7 of tests/test_attn_probes_gpu.py, so the seeded lists are the same lists)


@functools.lru_cache(maxsize=None)
def _shape(i):
    """(S, B, H, table array, head_pattern or None)"""
    if i == 1:
        return 832, 1, 1, _pack([[[(0, 1)], [(0, 1), (2, 1)], [(1, 1), (5, 1), (12, 1)], [(0, 2), (3, 1), (6, 7)]]], 8), None
    if i == 2:
        rng = np.random.RandomState(1920)
        lists = [[_random_list(rng, 30, 6) for _b in range(8)] for _p in range(2)]
        flat = [rl for p in lists for rl in p]
        assert any(a[0] + a[1] == b[0] for rl in flat for a, b in zip(rl, rl[1:])), "some ranges touch"
        assert any(a[0] + a[1] < b[0] for rl in flat for a, b in zip(rl, rl[1:])), "some ranges jump"
        assert {len(rl) for rl in flat} >= {1, 2} and max(len(rl) for rl in flat) >= 5
        return 1920, 2, 2, _pack(lists, 6), [1, 0]
    rng = np.random.RandomState(8256)
    lists = [[_random_list(rng, 129, 10) for _b in range(33)] for _p in range(2)]
    lists[0][3] = [(2 * r, 1) for r in range(64)]  # a cursor step on every tile, all 64 table lanes
    lists[1][32] = [(2 * r, 1) for r in range(63)]  # (the last block: 64 rows)
    lists[1][5] = [(2 * r, 1) for r in range(1, 65)]  # 64 more, up to the operand's last tile (128)
    lists[0][7] = [(0, 129)]  # every tile, one range
    return 8256, 1, 8, _pack(lists, 64), [0, 1, 0, 1, 1, 0, 1, 0]


@functools.lru_cache(maxsize=None)
def _table(i):
    from gen3c_amd import ops
    S, B, H, tab, hp = _shape(i)
    return ops.attn_range_table(tab, S, head_pattern=hp, H=H)


@pytest.mark.parametrize("shape", [1, 2, 3])
def test_ranges_attention_vs_masked_fp64(shape):
    from gen3c_amd import ops
    S, B, H, tab, hp = _shape(shape)
    table = _table(shape)
    q, k, v, vt = _problem(S, B, H)
    pmasks = [ops.ranges_attn_mask(table, S, pattern=p) for p in range(tab.shape[0])]
    ref = _fp64(S, B, H, [pmasks[hp[h] if hp else 0] for h in range(H)])
    for bound, kernel in ((BOUND, NM_RNG), (0.0, MAX_RNG)):
        out, metas = _timed(lambda: ops.self_attn_ranges(q, k, vt, S, B, H, bound, table))
        assert len(metas) == 1 and metas[0]["kernel"] == kernel and metas[0]["tile_density"] == table.attended / table.dense
        err = _worst_pair(out, ref, B, H)
        print(f"[ranges shape {shape}: S={S} B={B} H={H} {kernel}] tiles {table.attended}/{table.dense}, worst (batch, head) rel-L2 vs masked fp64 = {err:.3e}")
        assert torch.isfinite(out.float()).all()
        assert err < 4e-3, f"{kernel}: rel-L2 {err:.3e} vs the masked fp64 softmax"


@pytest.mark.parametrize("shape", [1, 2])
def test_ranges_launch_equals_the_carry_kernels_block_by_block(shape):
    from gen3c_amd import ops
    S, B, H, tab, hp = _shape(shape)
    table = _table(shape)
    q, k, v, vt = _problem(S, B, H)
    QR = ops.window_q_rows()
    forms = ((BOUND, NM_RNG, NM_CARRY, lambda *a, **kw: ops.self_attn_bounded(*a, BOUND, **kw)), (0.0, MAX_RNG, MAX_CARRY, ops.flash_attn))
    for bound, kernel, carry_kernel, oracle in forms:
        out, metas = _timed(lambda: ops.self_attn_ranges(q, k, vt, S, B, H, bound, table))
        assert metas[0]["kernel"] == kernel
        expect = torch.empty_like(out)
        for h in range(H):
            sl = slice(h * HD, (h + 1) * HD)
            for blk, r0 in enumerate(range(0, S, QR)):
                r1 = min(r0 + QR, S)
                keys = torch.cat([torch.arange(f, f + n) for f, n in tab[hp[h] if hp else 0, blk].tolist() if n])  # the block's keys, in list order
                rows = (keys[:, None] * B + torch.arange(B)[None, :]).flatten().to(q.device)  # k's rows are (key, batch), batch fastest
                kk = k[:, sl][rows].contiguous()
                vtt = vt[:, h:h + 1, :, keys.to(q.device)].contiguous()
                n = keys.numel()
                carry = (torch.zeros((r1 - r0) * B, HD, device=q.device), torch.full((B, 1, r1 - r0), -math.inf, device=q.device))  # "no earlier keys"
                part, m = _timed(lambda: oracle(q[r0 * B:r1 * B, sl], kk, vtt, r1 - r0, n, B, 1, variant=11, carry=carry))
                assert m[0]["kernel"] == carry_kernel, "the oracle must run the epilogue the range kernel runs"
                expect[r0 * B:r1 * B, sl] = part
        assert torch.equal(expect, out), f"{kernel} differs from the carry kernel's blocks"


@pytest.mark.parametrize("frame_len,S,W,s,B,H", [(320, 1920, 1, 1, 2, 2), (320, 1920, 0, 2, 2, 2), (320, 1920, 2, 0, 2, 2), (64, 832, 0, 1, 1, 1)])
def test_frame_ranges_launch_equals_the_window_launch(frame_len, S, W, s, B, H):
    from gen3c_amd import ops, sparse_attn
    q, k, v, vt = _problem(S, B, H)
    table = ops.attn_range_table(sparse_attn.frame_ranges(S // frame_len, frame_len, W, s), S, H=H)
    assert torch.equal(ops.ranges_attn_mask(table, S), ops.window_attn_mask(S, frame_len, W, s))
    assert (table.attended, table.dense) == tuple(H * x for x in ops.window_attn_tiles(S, frame_len, W, s)) and table.attended < table.dense
    for bound, kernel, win_kernel in ((BOUND, NM_RNG, NM_WIN), (0.0, MAX_RNG, MAX_WIN)):
        out, metas = _timed(lambda: ops.self_attn_ranges(q, k, vt, S, B, H, bound, table))
        win, wmetas = _timed(lambda: ops.self_attn_window(q, k, vt, S, B, H, bound, frame_len, W, s))
        assert metas[0]["kernel"] == kernel and wmetas[0]["kernel"] == win_kernel
        assert metas[0]["tile_density"] == wmetas[0]["tile_density"]
        assert torch.equal(out, win), f"{kernel} differs from {win_kernel} on the same tiles in the same order"


def test_the_kernel_clamps_a_rule_breaking_table_to_the_operand():
    """gen3c_hip.h: "the kernel clamps every range (and the pattern index) to the operand". ops.attn_range_table refuses such a table, so the
    library entry is called directly, once with a table that breaks the rules and once with the valid table the clamp must make of it -
    min(first_key, S), min(n_keys, S - first_key), a range of no keys ends the list, pattern n_patterns - 1 - and the two outputs must be EQUAL,
    in both forms, and finite. Ranges that overrun S by one and by two tiles, first_key == S and first_key == S + 64 (each behind a valid first
    range, with a valid-looking range behind it that must not be visited), and a head_pattern entry equal to n_patterns.
    No value here could fault even if the clamp were missing: the largest unclamped key is S + 127 - K has 128 B NaN guard rows behind key S - 1,
    V^T 128 NaN columns - and the table buffer holds a whole third pattern (the list {0}) behind the two the launch is told of. Negative or huge
    table values are deliberately not run: their unclamped addresses would leave the allocations; that part of the promise is read from the
    code (attention_w4b.hpp: the unsigned min in the table load)."""
    from gen3c_amd import _lib as L, ops
    from tests.guarded import Guarded
    lib = L.load()
    S, B, H, MR = 832, 2, 2, 4
    D = H * HD
    bad = np.zeros((3, 4, MR, 2), dtype=np.int32)
    bad[0, 0, :2] = [(0, 64), (704, 192)]              # over S by one tile
    bad[0, 1, :2] = [(128, 128), (768, 192)]           # by two
    bad[0, 2, :3] = [(64, 64), (S, 64), (320, 64)]     # first_key == S: no keys left, the list ends there
    bad[0, 3, :3] = [(0, 128), (S + 64, 64), (448, 64)]
    bad[1, 0, :1] = [(256, 640)]                       # by one, the only range
    bad[1, 1, :3] = [(0, 64), (192, 64), (704, 256)]   # by two
    bad[1, 2, :3] = [(512, 64), (S, 128), (704, 64)]
    bad[1, 3, :2] = [(768, 64), (S + 64, 64)]
    bad[2, :, 0] = (0, 64)                             # behind the launch's two patterns: what an unclamped pattern index would read
    assert int((bad[:2, :, :, 0] + bad[:2, :, :, 1]).max()) == S + 128
    good = bad.copy()
    first = np.minimum(good[..., 0], S)
    good[..., 1] = np.minimum(good[..., 1], S - first)
    good[..., 0] = first
    for p in range(2):
        for b in range(4):
            n = int(np.argmax(good[p, b, :, 1] == 0)) if (good[p, b, :, 1] == 0).any() else MR
            good[p, b, n:] = 0
    ops.attn_range_table(good[:2], S, head_pattern=[1, 0], H=H)  # (the clamped table keeps every rule)
    with pytest.raises(Exception):
        ops.attn_range_table(bad[:2], S, head_pattern=[1, 0], H=H)
    q, k, v, _ = _problem(S, B, H)
    dev = q.device
    kg = Guarded(S * B, 2 * D, guard=2 * 64 * B, data=torch.cat([torch.full((S * B, D), -2.5, dtype=torch.bfloat16, device=dev), k], dim=1))
    kk = kg.payload[:, D:]
    ldvt = S + 128
    vt = torch.full((B, H, HD, ldvt), float("nan"), dtype=torch.bfloat16, device=dev)
    vt[..., :S] = v.view(S, B, H, HD).permute(1, 2, 3, 0)
    tables = {name: (torch.from_numpy(t).to(dev), torch.tensor(hp, dtype=torch.int32, device=dev)) for name, t, hp in (("bad", bad, [2, 0]), ("good", good, [1, 0]))}
    for bound, kernel in ((BOUND, NM_RNG), (0.0, MAX_RNG)):
        outs = {}
        for name, (tab, hp) in tables.items():
            o = Guarded(S * B, D, ld=D + 64)
            args = (q.data_ptr(), q.stride(0) * B, q.stride(0), HD, kk.data_ptr(), kk.stride(0) * B, kk.stride(0), HD, vt.data_ptr(), ldvt, H * HD * ldvt, HD * ldvt,
                    o.payload.data_ptr(), o.ld * B, o.ld, HD, S, B, H, HD, 1.0 / math.sqrt(HD), bound, tab.data_ptr(), 2, MR, hp.data_ptr())
            assert lib.g3_attn_ranges_plan_bf16(*args).decode() == kernel
            L.check(lib.g3_self_attn_fwd_ranges_bf16(*args, torch.cuda.current_stream().cuda_stream), "g3_self_attn_fwd_ranges_bf16")
            torch.cuda.synchronize()
            o.assert_only_payload_written(f"{kernel} {name} table")  # (and the payload finite)
            outs[name] = o.payload.clone()
        assert torch.equal(outs["bad"], outs["good"]), f"{kernel}: the rule-breaking table does not give the launch of its clamped table"


def test_radial_ranges_vs_masked_fp64():
    from gen3c_amd import ops, sparse_attn
    T, fl, B, H = 6, 1024, 1, 2
    S = T * fl
    q, k, v, vt = _problem(S, B, H)
    table = ops.attn_range_table(sparse_attn.radial_ranges(T, fl, 0.25, 1), S, H=H)
    assert round(table.attended / table.dense, 3) == 0.646
    mask = ops.ranges_attn_mask(table, S)
    ref = _fp64(S, B, H, [mask] * H)
    for bound, kernel in ((BOUND, NM_RNG), (0.0, MAX_RNG)):
        out, metas = _timed(lambda: ops.self_attn_ranges(q, k, vt, S, B, H, bound, table))
        assert len(metas) == 1 and metas[0]["kernel"] == kernel and metas[0]["tile_density"] == table.attended / table.dense
        err = _worst_pair(out, ref, B, H)
        print(f"[radial 0.25, S={S} H={H} {kernel}] tiles {table.attended}/{table.dense}, worst (batch, head) rel-L2 vs masked fp64 = {err:.3e}")
        assert torch.isfinite(out.float()).all()
        assert err < 4e-3, f"{kernel}: rel-L2 {err:.3e} vs the masked fp64 softmax"
