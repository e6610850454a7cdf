"""CPU: the range-table self-attention's host side, without a launch - g3_attn_ranges_check (every rule of include/gen3c_hip.h, by its text), the
dry run g3_attn_ranges_plan_bf16 (placeholder pointers), ops.ranges_attn_mask, and the builders of gen3c_amd/sparse_attn.py against brute-force
restatements of their row-level definitions.

Product-shape figures (T = 16, sink 1, width1 0.25), worked out from the row-level definition when the pattern was specified: density 0.345 at 3 520
tokens per frame and 0.348 at 3 600, at most 16 ranges per block in both. The builder gives exactly these (0.34527, 0.34832; 16)."""
import math

import numpy as np
import pytest
import torch

from gen3c_amd import _lib

FN = "g3_self_attn_fwd_ranges_bf16"
CHECK = "g3_attn_ranges_check"
NM_RNG = "flash_attn_fwd_w4b_nm_rng_kernel<true>"
MAX_RNG = "flash_attn_fwd_w4b_rng_kernel<true>"
UNIT_BOUND = 128 / math.sqrt(128) * 1.03
ARGS = ["q", "q_row", "q_batch", "q_head", "k", "k_row", "k_batch", "k_head", "vt", "vt_row", "vt_batch", "vt_head", "o", "o_row", "o_batch", "o_head",
        "S", "B", "H", "head_dim", "softmax_scale", "logit_bound", "ranges", "n_patterns", "max_ranges", "head_pattern"]


def _canonical(S, B, H, n_patterns=1, max_ranges=8, bound=UNIT_BOUND):
    """Contiguous [S*B, H*128] q / k / o and V^T [B, H, 128, S] at placeholder addresses; the dry run dereferences nothing."""
    return dict(q=0x10000, q_row=B * H * 128, q_batch=H * 128, q_head=128, k=0x20000, k_row=B * H * 128, k_batch=H * 128, k_head=128,
                vt=0x30000, vt_row=S, vt_batch=H * 128 * S, vt_head=128 * S, o=0x40000, o_row=B * H * 128, o_batch=H * 128, o_head=128,
                S=S, B=B, H=H, head_dim=128, softmax_scale=1.0 / math.sqrt(128), logit_bound=bound, ranges=0x50000, n_patterns=n_patterns,
                max_ranges=max_ranges, head_pattern=0)


def _plan(lib, a):
    name = lib.g3_attn_ranges_plan_bf16(*[a[n] for n in ARGS])
    return (name.decode(), None) if name is not None else (None, lib.g3_last_error().decode())


def test_ranges_plan_names_the_kernel():
    lib = _lib.load()
    assert lib.g3_self_attn_ranges_max() == 64 and lib.g3_self_attn_window_q_rows() == 256
    a = _canonical(1920, 2, 2)
    assert _plan(lib, a) == (NM_RNG, None)
    assert _plan(lib, dict(a, logit_bound=0.0)) == (MAX_RNG, None)
    assert _plan(lib, dict(a, logit_bound=61.0 / math.log2(math.e))) == (MAX_RNG, None)  # beyond the no-max form's range
    assert _plan(lib, dict(a, head_pattern=0x60004, n_patterns=2, max_ranges=64)) == (NM_RNG, None)
    assert _plan(lib, _canonical(64, 1, 1, max_ranges=1)) == (NM_RNG, None)  # never demoted: one tile, one block
    big = _canonical(56320, 2, 32, max_ranges=16)
    assert _plan(lib, big) == (NM_RNG, None)
    lib.g3_set_option(b"attn_variant", 4)  # the entry always runs variant 11's family
    try:
        assert _plan(lib, big) == (NM_RNG, None) and _plan(lib, dict(big, logit_bound=0.0)) == (MAX_RNG, None)
    finally:
        lib.g3_set_option(b"attn_variant", 0)


def test_ranges_plan_refusals():
    lib = _lib.load()
    a = _canonical(1920, 2, 2)
    cases = [
        (dict(S=1900, vt_row=1920), FN + ": S 1900 must be a positive multiple of 64"),
        (dict(S=0), FN + ": S 0 must be a positive multiple of 64"),
        (dict(n_patterns=0), FN + ": n_patterns 0 must be >= 1"),
        (dict(max_ranges=0), FN + ": max_ranges 0 outside [1, 64]"),
        (dict(max_ranges=65), FN + ": max_ranges 65 outside [1, 64]"),
        (dict(ranges=0), FN + ": null or misaligned range table (8-byte alignment)"),
        (dict(ranges=0x50004), FN + ": null or misaligned range table (8-byte alignment)"),
        (dict(head_pattern=0x60002), FN + ": misaligned head_pattern (4-byte alignment)"),
        (dict(vt_row=1856), FN + ": V^T leading dim 1856 below ceil64(S) 1920"),
        (dict(q=0), FN + ": null operand"),
        (dict(o=0), FN + ": null operand"),
        (dict(head_dim=64), "g3_flash_attn_fwd_bf16: head_dim 64 unsupported (128 only)"),
        (dict(B=0), "g3_flash_attn_fwd_bf16: bad shape"),
        (dict(k=0x20008), "g3_flash_attn_fwd_bf16: misaligned pointer"),
        (dict(o=0x40004), "g3_flash_attn_fwd_bf16: misaligned pointer"),
        (dict(q_row=2 * 2 * 128 + 4), "g3_flash_attn_fwd_bf16: strides must keep 16-byte (q,k,vt) / 8-byte (o) alignment"),
        (dict(o_row=2 * 2 * 128 + 2), "g3_flash_attn_fwd_bf16: strides must keep 16-byte (q,k,vt) / 8-byte (o) alignment"),
    ]
    for over, text in cases:
        assert _plan(lib, dict(a, **over)) == (None, text), over
    # operands beyond the kernel's 32-bit byte offsets: the window's arithmetic over all S keys
    S, row = 1920, 1 << 21
    k_max = (S - 1 + 2 * 64) * row * 2 + 256
    v_max = 127 * S * 2 + (S + 64) * 2 + 256
    assert k_max > 0xFFFFFFFF
    assert _plan(lib, dict(a, k_row=row)) == (None, f"{FN}: K / V^T span exceeds the kernel's 32-bit byte offsets (k {k_max}, vt {v_max} bytes)")
    ld = 1 << 25
    v_max = 127 * ld * 2 + (S + 64) * 2 + 256
    k_max = (S - 1 + 2 * 64) * (2 * 2 * 128) * 2 + 256
    assert _plan(lib, dict(a, vt_row=ld, vt_head=128 * ld, vt_batch=2 * 128 * ld)) == \
        (None, f"{FN}: K / V^T span exceeds the kernel's 32-bit byte offsets (k {k_max}, vt {v_max} bytes)")
    # the dry run of the recorded entries does not know this entry
    assert lib.g3_attn_plan_bf16(9, *([0] * 35)) is None and lib.g3_last_error() == b"g3_attn_plan_bf16: unknown entry 9"


def _tab(lists, max_ranges, n_patterns=1):
    """lists[pattern][block] = [(first_key, n_keys), ...] -> int32 [n_patterns, n_qblk, max_ranges, 2]"""
    t = np.zeros((n_patterns, len(lists[0]), max_ranges, 2), dtype=np.int32)
    for p, blocks in enumerate(lists):
        for b, rl in enumerate(blocks):
            for r, e in enumerate(rl):
                t[p, b, r] = e
    return t


def test_ranges_check_accepts_and_counts():
    from gen3c_amd import ops
    S = 832  # 4 query blocks (the last of 64 rows), 13 tiles
    lists = [[[(0, 64)], [(0, 64), (128, 64)], [(64, 64), (320, 64), (768, 64)], [(0, 128), (192, 64), (384, 448)]],
             [[(0, 832)], [(0, 64), (64, 64)], [(768, 64)], [(0, 64)]]]  # (pattern 1 block 1: touching ranges stay two ranges)
    t = ops.attn_range_table(_tab(lists, 8, 2), S, head_pattern=[1, 0, 1], device="cpu")
    per_pattern = [1 + 2 + 3 + 10, 13 + 2 + 1 + 1]
    assert (t.attended, t.dense) == (2 * per_pattern[1] + per_pattern[0], 3 * 4 * 13)
    assert (t.S, t.n_patterns, t.max_ranges, t.H) == (S, 2, 8, 3)
    assert t.ranges.dtype == torch.int32 and t.ranges.shape == (2, 4, 8, 2) and t.ranges_dev.device.type == "cpu"
    assert t.head_pattern.tolist() == [1, 0, 1]
    t0 = ops.attn_range_table(_tab(lists[:1], 8), S, H=5, device="cpu")  # no head_pattern: pattern 0 for every head
    assert (t0.attended, t0.dense) == (5 * per_pattern[0], 5 * 4 * 13) and t0.head_pattern is None and t0.head_pattern_dev is None
    # the mask is the written-down function
    for p in (0, 1):
        mask = ops.ranges_attn_mask(t, S, pattern=p)
        assert mask.dtype == torch.bool and mask.shape == (S, S) and mask.device.type == "cpu"
        brute = torch.zeros(S, S, dtype=torch.bool)
        for b, rl in enumerate(lists[p]):
            for k0, n in rl:
                brute[256 * b:256 * b + 256, k0:k0 + n] = True
        assert torch.equal(mask, brute)
        assert sum(int(mask[256 * b].view(13, 64).any(dim=1).sum()) for b in range(4)) == per_pattern[p]
    assert torch.equal(ops.ranges_attn_mask(_tab(lists, 8, 2), S, pattern=1), ops.ranges_attn_mask(t, S, pattern=1))  # a bare array is taken too


def test_ranges_check_refusals():
    from gen3c_amd import ops
    S = 832
    good = [[[(0, 64)], [(0, 64), (128, 64)], [(64, 64), (320, 64), (768, 64)], [(0, 128), (192, 64), (384, 448)]]]

    def refused(text, lists=good, max_ranges=8, n_patterns=1, S=S, poke=None, **kw):
        t = _tab(lists, max_ranges, n_patterns)
        if poke:
            t[poke[0]] = poke[1]
        with pytest.raises(_lib.Gen3cHipError) as e:
            ops.attn_range_table(t, S, device="cpu", **kw)
        assert text in str(e.value), str(e.value)

    def with_block(b, rl, p=0):
        lists = [[list(x) for x in good[0]] for _ in range(p + 1)]
        lists[p][b] = rl
        return lists

    refused(f"{CHECK}: S 800 must be a positive multiple of 64", S=800)
    refused(f"{CHECK}: H 0 must be >= 1", H=0)
    refused(f"{CHECK}: head_pattern[1] = 1 outside [0, 1)", head_pattern=[0, 1])
    refused(f"{CHECK}: head_pattern[0] = -1 outside [0, 1)", head_pattern=[-1])
    refused(f"{CHECK}: pattern 0, block 2, range 0: the list is empty", lists=with_block(2, []))
    refused(f"{CHECK}: pattern 1, block 3, range 0: the list is empty", lists=with_block(3, [], p=1), n_patterns=2)
    refused(f"{CHECK}: pattern 0, block 1, range 1: first_key 100 and n_keys 64 must be multiples of 64, first_key >= 0 and n_keys > 0",
            lists=with_block(1, [(0, 64), (100, 64)]))
    refused(f"{CHECK}: pattern 0, block 1, range 0: first_key 0 and n_keys 96 must be multiples of 64, first_key >= 0 and n_keys > 0",
            lists=with_block(1, [(0, 96)]))
    refused(f"{CHECK}: pattern 0, block 0, range 0: first_key -64 and n_keys 64 must be multiples of 64, first_key >= 0 and n_keys > 0",
            lists=with_block(0, [(-64, 64)]))
    refused(f"{CHECK}: pattern 0, block 0, range 1: first_key 128 and n_keys -64 must be multiples of 64, first_key >= 0 and n_keys > 0",
            lists=with_block(0, [(0, 64), (128, -64)]))
    refused(f"{CHECK}: pattern 0, block 3, range 1: first_key 64 lies below the end 128 of range 0 (lists are ascending and disjoint)",
            lists=with_block(3, [(0, 128), (64, 128)]))
    refused(f"{CHECK}: pattern 0, block 3, range 2: first_key 0 lies below the end 256 of range 1 (lists are ascending and disjoint)",
            lists=with_block(3, [(0, 64), (128, 128), (0, 64)]))
    refused(f"{CHECK}: pattern 0, block 2, range 1: keys [768, 896) reach beyond S 832", lists=with_block(2, [(0, 64), (768, 128)]))
    refused(f"{CHECK}: pattern 0, block 0, range 0: keys [832, 896) reach beyond S 832", lists=with_block(0, [(832, 64)]))
    refused(f"{CHECK}: pattern 0, block 1, range 3: (192, 64) behind the terminator must be zero", lists=with_block(1, [(0, 64), (128, 64), (0, 0), (192, 64)]))
    refused(f"{CHECK}: pattern 0, block 0, range 1: (64, 0) behind the terminator must be zero", poke=((0, 0, 1, 0), 64))
    # what the Python surface refuses before the library sees it
    with pytest.raises(ValueError, match="int32 array"):
        ops.attn_range_table(np.zeros((1, 4, 8, 2), dtype=np.int64), S, device="cpu")
    with pytest.raises(ValueError, match=r"\[n_patterns, 4, max_ranges, 2\]"):
        ops.attn_range_table(np.zeros((1, 3, 8, 2), dtype=np.int32), S, device="cpu")
    with pytest.raises(ValueError, match=r"max_ranges 65 outside \[1, 64\]"):
        ops.attn_range_table(np.zeros((1, 4, 65, 2), dtype=np.int32), S, device="cpu")
    # the C function itself: null pointers
    lib = _lib.load()
    import ctypes
    att, dense = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.g3_attn_ranges_check(None, 1, S, 8, None, 1, ctypes.byref(att), ctypes.byref(dense)) != 0
    assert lib.g3_last_error() == f"{CHECK}: null table or result pointer".encode()


def _tiles_per_block(mask, S):
    return sum(int(mask[r0].view(S // 64, 64).any(dim=1).sum()) for r0 in range(0, S, 256))


@pytest.mark.parametrize("frame_len,S", [(64, 832), (320, 1920), (256, 2048)])
def test_frame_ranges_is_the_window_function(frame_len, S):
    from gen3c_amd import ops, sparse_attn
    for W in range(3):
        for s in range(3):
            tab = sparse_attn.frame_ranges(S // frame_len, frame_len, W, s)
            t = ops.attn_range_table(tab, S, device="cpu")
            mask = ops.ranges_attn_mask(t, S)
            assert torch.equal(mask, ops.window_attn_mask(S, frame_len, W, s)), (W, s)
            assert (t.attended, t.dense) == (_tiles_per_block(mask, S), -(-S // 256) * (S // 64)) == ops.window_attn_tiles(S, frame_len, W, s)
            assert tab.shape[2] <= 2


def test_frame_ranges_at_720p_contains_every_rows_window():
    from gen3c_amd import ops, sparse_attn
    fl, T = 3600, 4  # 45 x 80 tokens per latent frame: no multiple of 64, which the window entry refuses
    S = T * fl
    with pytest.raises(_lib.Gen3cHipError, match="must be positive multiples of 64"):
        ops.window_attn_tiles(S, fl, 1, 1)
    f = torch.arange(S) // fl
    for W, s in ((0, 0), (1, 1), (0, 2)):
        t = ops.attn_range_table(sparse_attn.frame_ranges(T, fl, W, s), S, device="cpu")
        mask = ops.ranges_attn_mask(t, S)
        per_row = ((f[None, :] - f[:, None]).abs() <= W) | (f[None, :] < s)
        assert bool((mask | ~per_row).all()), "every row's own window is inside its block's list"
        assert not bool(mask.all()) and t.attended == _tiles_per_block(mask, S)
        # nothing beyond the block-granular window rounded outward by one tile
        r0 = torch.arange(S) // 256 * 256
        f0, f1 = r0 // fl, (torch.clamp(r0 + 256, max=S) - 1) // fl
        k = torch.arange(S)
        lo, hi = torch.clamp(f0 - W, min=0) * fl // 64 * 64, -(-(torch.clamp(f1 + W + 1, max=T) * fl) // 64) * 64
        blockwise = ((k[None, :] >= lo[:, None]) & (k[None, :] < hi[:, None])) | (k[None, :] < -(-min(s, T) * fl // 64) * 64)
        assert torch.equal(mask, blockwise)


def _radial_rows(T, fl, width1, sink, min_width=64):
    """The row-level definition, brute force: bool [S, S]."""
    S = T * fl
    fq, pq = torch.arange(S) // fl, torch.arange(S) % fl
    d = (fq[:, None] - fq[None, :]).abs()
    hw = torch.zeros(T, dtype=torch.long)
    for dd in range(1, T):
        hw[dd] = max(min_width, math.ceil(fl * width1 / 2 ** math.floor(math.log2(dd))))
    return (fq[None, :] < sink) | (d == 0) | ((pq[:, None] - pq[None, :]).abs() < hw[d])


@pytest.mark.parametrize("T,fl,width1,sink", [(6, 1024, 0.25, 1), (8, 360, 0.5, 0), (7, 320, 0.125, 2)])
def test_radial_ranges_contains_its_definition_and_little_more(T, fl, width1, sink):
    from gen3c_amd import ops, sparse_attn
    S = T * fl
    tab = sparse_attn.radial_ranges(T, fl, width1, sink)
    t = ops.attn_range_table(tab, S, device="cpu")
    mask = ops.ranges_attn_mask(t, S)
    rows = _radial_rows(T, fl, width1, sink)
    assert bool((mask | ~rows).all()), "the table contains the row-level definition"
    # ... and is contained in the definition dilated by one query block (the union over the block's rows) and one key tile on each side
    n_blk, n_tile = -(-S // 256), S // 64
    pad = torch.zeros(n_blk * 256, S, dtype=torch.bool)
    pad[:S] = rows
    tiles = pad.view(n_blk, 256, n_tile, 64).any(dim=3).any(dim=1)  # [block, tile]: any row of the block attends any key of the tile
    wide = tiles.clone()  # one key tile on each side ...
    wide[:, 1:] |= tiles[:, :-1]
    wide[:, :-1] |= tiles[:, 1:]
    dil = wide.clone()    # ... and one query block on each side
    dil[1:] |= wide[:-1]
    dil[:-1] |= wide[1:]
    got = mask[::256].view(n_blk, n_tile, 64).all(dim=2)
    assert torch.equal(got, mask[::256].view(n_blk, n_tile, 64).any(dim=2)), "whole tiles"
    assert bool((dil | ~got).all())
    assert torch.equal(got, tiles), "exactly the tiles some row of the block attends (outward rounding adds no tile of its own)"
    assert t.attended == int(got.sum()) and t.dense == n_blk * n_tile
    assert not bool(mask.all())


def test_radial_ranges_product_figures():
    from gen3c_amd import sparse_attn
    for fl, density in ((3520, 0.345), (3600, 0.348)):
        tab = sparse_attn.radial_ranges(16, fl, 0.25, 1)
        S = 16 * fl
        assert tab.shape == (1, -(-S // 256), 16, 2), "at most 16 ranges per block"
        attended, dense = int(tab[0, :, :, 1].sum()) // 64, tab.shape[1] * (S // 64)
        assert round(attended / dense, 3) == density, attended / dense
    tab = sparse_attn.radial_ranges(6, 1024, 0.25, 1)
    assert round(int(tab[0, :, :, 1].sum()) // 64 / (tab.shape[1] * 96), 3) == 0.646
    with pytest.raises(ValueError, match="must be a positive multiple of 64 tokens"):
        sparse_attn.radial_ranges(3, 100)


def test_cli_flag_and_environment(monkeypatch):
    import argparse
    from gen3c_amd import cli_common
    monkeypatch.delenv("G3_SELF_ATTN_PATTERN", raising=False)
    parse = lambda *argv: cli_common.self_attn_pattern_requested(cli_common.add_common_args(argparse.ArgumentParser()).parse_args(list(argv)))
    assert parse() is None
    assert parse("--self_attn_pattern", "radial:0.25:1") == ("radial", 0.25, 1)
    assert parse("--self_attn_pattern", "frame:2:1") == ("frame", 2, 1)
    with pytest.raises(ValueError, match="expected radial:WIDTH1:SINK or frame:W:S"):
        parse("--self_attn_pattern", "radial:wide")
    monkeypatch.setenv("G3_SELF_ATTN_PATTERN", "frame:1:0")
    assert parse() == ("frame", 1, 0)
    assert parse("--self_attn_pattern", "radial:0.5:2") == ("radial", 0.5, 2)  # the flag wins
    monkeypatch.setenv("G3_SELF_ATTN_PATTERN", "ring")
    with pytest.raises(ValueError, match="expected radial:WIDTH1:SINK or frame:W:S"):
        parse()


def test_dit_pattern_option_and_refusals():
    from gen3c_amd.dit import VideoExtendGeneralDIT
    kw = dict(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=1, num_heads=2, adaln_lora_dim=32,
              crossattn_emb_channels=128, device="cpu", init_weights=False)
    net = VideoExtendGeneralDIT(**kw)
    assert net.self_attn_pattern is None and net._self_attn_table_for(6, 8, 8, "cpu") is None
    net = VideoExtendGeneralDIT(self_attn_pattern=("frame", 1, 1), **kw)
    assert net.self_attn_pattern == ("frame", 1, 1)
    t = net._self_attn_table_for(6, 8, 8, "cpu")
    assert t is not None and t.S == 384 and t.attended < t.dense and net._self_attn_table_for(6, 8, 8, "cpu") is t  # built once, cached
    assert net._self_attn_table_for(2, 8, 8, "cpu") is None  # covers every tile: the plain branch
    net.set_self_attn_pattern(("radial", 0.25, 1))
    assert net._self_attn_table_for(6, 8, 8, "cpu") is None  # 64 tokens per frame: min_width covers the frame at every distance
    t2 = net._self_attn_table_for(6, 16, 32, "cpu")
    assert t2 is not None and t2.S == 3072 and t2.attended < t2.dense
    net.set_self_attn_pattern("frame:0:6")
    assert net.self_attn_pattern == ("frame", 0, 6) and net._self_attn_table_for(6, 8, 8, "cpu") is None
    with pytest.raises(ValueError, match="self_attn_pattern"):
        net.set_self_attn_pattern(("spiral", 1, 1))
    net.set_self_attn_pattern(("frame", 1, 1))
    with pytest.raises(ValueError, match=r"self_attn_pattern=\('frame', 1, 1\): S = 5 x 8 x 12 = 480 tokens is not a multiple of 64"):
        net._self_attn_table_for(5, 8, 12, "cpu")
    net.set_self_attn_window(1, 1)
    with pytest.raises(ValueError, match="self_attn_pattern and self_attn_window are both set"):
        net._self_attn_table_for(6, 8, 8, "cpu")
    net.set_self_attn_window(None)
    net._cp_attn, net.cp_size = object(), 4  # (what enable_context_parallel leaves behind)
    with pytest.raises(ValueError, match="with context parallelism over 4 ranks: range tables under key sharding are out of scope"):
        net._self_attn_table_for(6, 8, 8, "cpu")
    net.set_self_attn_pattern(None)
    assert net._self_attn_table_for(6, 8, 8, "cpu") is None
