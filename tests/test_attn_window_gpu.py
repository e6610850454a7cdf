"""GPU: frame-window self-attention (g3_self_attn_fwd_window_bf16; flash_attn_fwd_w4b_nm_win_kernel / flash_attn_fwd_w4b_win_kernel): every workgroup of
the one-wave-per-SIMD kernel derives its own key range - the frames within W of its 256 query rows' frames, plus the first s frames - in its prologue
and walks it as the carry kernels walk a launch-wide range with one skipped part. ops.window_attn_mask is the function.

Inputs: q, k behind a per-head RMSNorm with unit weights (column views of fused buffers, as the DiT passes them), random v; head dim 128.

Shapes, chosen for where this form can go wrong:
 * frame_len 64, S 832 (13 frames; the last block has 64 rows), W 0: the last workgroup walks ONE tile (the prologue's nt > 1 guards); with a sink of 1
   every block after the first skips from logical tile 1 (the V^T walk's special case).
 * frame_len 320, S 1920 (6 frames; blocks straddle frames, S is no multiple of 256, odd tile counts), W 0..2 x s 0..2, B = H = 2: a sink that touches or
   overlaps the window (no skip), skips of one and more tiles, first and last blocks clipped at both ends, both grid forms' strides.
 * frame_len 256, S 2048, W 1, s 1: blocks aligned to frames.

Bars.
 * worst (batch, head) rel-L2 against an fp64 softmax masked by ops.window_attn_mask < 4e-3, the bar of the existing attention tests - for the no-max form
   (the bound in range) and the running-maximum form (logit_bound 0).
 * bit for bit: every query block's rows through the existing carry entry (variant 11) over a contiguous copy of the block's physical key range, with the
   block's skip and an empty carry (lse = -inf, "no earlier keys": it forces the carry kernels, whose epilogue the window kernels share) - concatenated,
   the outputs EQUAL the window launch.
 * a window that covers everything (W = T - 1) is ops.self_attn_bounded(variant=11), bit for bit, and names the dense kernel.
 * g3_self_attn_window_tiles is the count of 64-key tiles with any attended key, per block, of ops.window_attn_mask."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 128
BOUND = HD / math.sqrt(HD) * 1.03  # unit RMSNorm weights: |q . k| / sqrt(128) <= sqrt(128), plus the margin for the bf16 roundings of q and k
NM_WIN, MAX_WIN = "flash_attn_fwd_w4b_nm_win_kernel<true>", "flash_attn_fwd_w4b_win_kernel<true>"
NM_DENSE, MAX_DENSE = "flash_attn_fwd_w4b_nm_kernel<true>", "flash_attn_fwd_w4b_kernel<true>"
NM_CARRY, MAX_CARRY = "flash_attn_fwd_w4b_nm_carry_kernel<true>", "flash_attn_fwd_w4b_carry_kernel<true>"


def _rms(x):
    x = x.float().view(x.shape[0], -1, HD)
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True))).reshape(x.shape[0], -1)


@functools.lru_cache(maxsize=None)
def _problem(S, B, H):
    """q [S*B, H*128] = first half of a fused [S*B, 2 H 128] buffer, k = second half of another; v, V^T; the fp64 logits and values per (batch, head).
    Built once per shape and shared by every case on it (nothing writes to them)."""
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
    logits = {}
    for b in range(B):
        for h in range(H):
            sl = slice(h * HD, (h + 1) * HD)
            logits[b, h] = (q[b::B, sl].double() @ k[b::B, sl].double().t()) / math.sqrt(HD), v[b::B, sl].double()
    return q, k, v, ops.transpose_v(v, S, B, H), logits


def _fp64(S, B, H, mask):
    logits = _problem(S, B, H)[4]
    out = torch.empty(S * B, H * HD, device="cuda:0", dtype=torch.float64)
    for (b, h), (sc, v) in logits.items():
        out[b::B, h * HD:(h + 1) * HD] = torch.softmax(sc.masked_fill(~mask, -math.inf), dim=-1) @ v
    return out


def _worst_pair(out, ref, B, H):
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    return max(rel(out[b::B, h * HD:(h + 1) * HD], ref[b::B, h * HD:(h + 1) * HD]) for b in range(B) for h in range(H))


def _timed(f):
    """(result, kernel names of the attention launches f made)"""
    from gen3c_amd import ops
    ops.enable_kernel_timers(True)
    try:
        out = f()
        metas = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    finally:
        ops.enable_kernel_timers(False)
    return out, metas


CASES = ([(64, 832, 0, 0, 1, 1), (64, 832, 0, 1, 1, 1)] + [(320, 1920, W, s, 2, 2) for W in (0, 1, 2) for s in (0, 1, 2)] + [(256, 2048, 1, 1, 1, 1)])


@pytest.mark.parametrize("frame_len,S,W,s,B,H", CASES)
def test_window_attention_vs_masked_fp64(frame_len, S, W, s, B, H):
    from gen3c_amd import ops
    q, k, v, vt, _ = _problem(S, B, H)
    mask = ops.window_attn_mask(S, frame_len, W, s)
    assert not bool(mask.all()), "every case here has keys to skip"
    ref = _fp64(S, B, H, mask.to("cuda:0"))
    attended, dense = ops.window_attn_tiles(S, frame_len, W, s)
    for bound, kernel in ((BOUND, NM_WIN), (0.0, MAX_WIN)):
        out, metas = _timed(lambda: ops.self_attn_window(q, k, vt, S, B, H, bound, frame_len, W, s))
        assert len(metas) == 1 and metas[0]["kernel"] == kernel and metas[0]["tile_density"] == attended / dense
        err = _worst_pair(out, ref, B, H)
        print(f"[window fl={frame_len} S={S} W={W} s={s} B={B} H={H} {kernel}] tiles {attended}/{dense}, worst (batch, head) rel-L2 vs masked fp64 = {err:.3e}")
        assert torch.isfinite(out.float()).all()
        assert err < 4e-3, f"{kernel}: rel-L2 {err:.3e} vs the masked fp64 softmax"


@pytest.mark.parametrize("frame_len,S,W,s,H", [(320, 1920, 1, 1, 2), (64, 832, 0, 1, 1)])
def test_window_launch_equals_the_carry_kernels_block_by_block(frame_len, S, W, s, H):
    from gen3c_amd import ops
    B, QR = 1, ops.window_q_rows()
    q, k, v, vt, _ = _problem(S, B, H)
    mask = ops.window_attn_mask(S, frame_len, W, s)
    forms = ((BOUND, NM_WIN, NM_CARRY, lambda *a, **kw: ops.self_attn_bounded(*a, BOUND, **kw)), (0.0, MAX_WIN, MAX_CARRY, ops.flash_attn))
    for bound, kernel, carry_kernel, oracle in forms:
        out, metas = _timed(lambda: ops.self_attn_window(q, k, vt, S, B, H, bound, frame_len, W, s))
        assert metas[0]["kernel"] == kernel
        parts, skips = [], set()
        for r0 in range(0, S, QR):
            r1 = min(r0 + QR, S)
            keys = mask[r0].nonzero().flatten()  # the block's key set: [0, sink_end) u [lo, hi), from the written-down function
            assert bool((mask[r0:r1] == mask[r0]).all())
            hi, n = int(keys[-1]) + 1, keys.numel()
            gap = (keys[1:] - keys[:-1] > 1).nonzero().flatten()
            assert gap.numel() <= 1
            if gap.numel():  # physical keys [0, hi), skipping [sink_end, lo)
                first, skip = 0, (int(keys[gap[0]]) + 1, int(keys[gap[0] + 1]) - int(keys[gap[0]]) - 1)
            else:            # physical keys [lo, hi)
                first, skip = int(keys[0]), None
            skips.add(None if skip is None else skip[0] // 64)
            kk, vtt = k[first:hi], vt[:, :, :, first:hi].contiguous()
            carry = (torch.zeros(r1 - r0, H * HD, device=q.device), torch.full((B, H, r1 - r0), -math.inf, device=q.device))  # "no earlier keys"
            part, m = _timed(lambda: oracle(q[r0:r1], kk, vtt, r1 - r0, n, B, H, variant=11, kv_skip=skip, carry=carry))
            assert m[0]["kernel"] == carry_kernel, "the oracle must run the epilogue the window kernel runs"
            parts.append(part)
        assert None in skips and len(skips) > 1, "blocks without a skip and blocks with one"
        assert frame_len != 64 or 1 in skips, "blocks that skip from logical tile 1"
        assert torch.equal(torch.cat(parts), out), f"{kernel} differs from the carry kernel's blocks"


@pytest.mark.parametrize("frame_len,S,B,H", [(320, 1920, 2, 2), (64, 832, 1, 1)])
def test_window_that_covers_everything_is_the_dense_launch(frame_len, S, B, H):
    from gen3c_amd import ops
    q, k, v, vt, _ = _problem(S, B, H)
    T = S // frame_len
    for bound, kernel in ((BOUND, NM_DENSE), (0.0, MAX_DENSE)):
        dense = ops.self_attn_bounded(q, k, vt, S, S, B, H, bound, variant=11)
        for W, s in ((T - 1, 0), (T + 3, 1), (0, T)):
            out, metas = _timed(lambda: ops.self_attn_window(q, k, vt, S, B, H, bound, frame_len, W, s))
            assert metas[0]["kernel"] == kernel and metas[0]["tile_density"] == 1.0
            assert torch.equal(out, dense)
        almost, metas = _timed(lambda: ops.self_attn_window(q, k, vt, S, B, H, bound, frame_len, T - 2, 0))
        assert metas[0]["kernel"] != kernel and not torch.equal(almost, dense)


@pytest.mark.parametrize("frame_len,S,W,s", sorted({c[:4] for c in CASES}))
def test_window_tile_count_is_the_masks(frame_len, S, W, s):
    from gen3c_amd import ops
    rows = ops.window_attn_mask(S, frame_len, W, s)[::ops.window_q_rows()]  # one row per query block (the key set is the block's)
    tiles = int(rows.view(rows.shape[0], S // 64, 64).any(dim=2).sum())
    assert ops.window_attn_tiles(S, frame_len, W, s) == (tiles, rows.shape[0] * (S // 64))
