"""CPU: the frame-window self-attention's host side, without a launch - the dry run g3_attn_window_plan_bf16 (placeholder pointers), the tile count,
ops.window_attn_mask against a brute-force restatement of the function in include/gen3c_hip.h, the command-line / environment switch and the DiT's
refusals."""
import math

import pytest
import torch

from gen3c_amd import _lib

FN = "g3_self_attn_fwd_window_bf16"
NM_DENSE = "flash_attn_fwd_w4b_nm_kernel<true>"
MAX_DENSE = "flash_attn_fwd_w4b_kernel<true>"
NM_WIN = "flash_attn_fwd_w4b_nm_win_kernel<true>"
MAX_WIN = "flash_attn_fwd_w4b_win_kernel<true>"
UNIT_BOUND = 128 / math.sqrt(128) * 1.03
ARGS = ["q", "q_row", "q_batch", "q_head", "k", "k_row", "k_batch", "k_head", "vt", "vt_row", "vt_batch", "vt_head", "o", "o_row", "o_batch", "o_head",
        "S", "B", "H", "head_dim", "softmax_scale", "logit_bound", "frame_len", "window_frames", "sink_frames"]


def _canonical(S, B, H, frame_len, W, s, bound=UNIT_BOUND):
    """Contiguous [S*B, H*128] q / k / o and V^T [B, H, 128, S] at placeholder addresses."""
    return dict(q=0x10000, q_row=B * H * 128, q_batch=H * 128, q_head=128, k=0x20000, k_row=B * H * 128, k_batch=H * 128, k_head=128,
                vt=0x30000, vt_row=S, vt_batch=H * 128 * S, vt_head=128 * S, o=0x40000, o_row=B * H * 128, o_batch=H * 128, o_head=128,
                S=S, B=B, H=H, head_dim=128, softmax_scale=1.0 / math.sqrt(128), logit_bound=bound, frame_len=frame_len, window_frames=W, sink_frames=s)


def _plan(lib, a):
    name = lib.g3_attn_window_plan_bf16(*[a[n] for n in ARGS])
    return (name.decode(), None) if name is not None else (None, lib.g3_last_error().decode())


def test_window_plan_names_the_kernel_and_leaves_the_last_error_alone():
    lib = _lib.load()
    assert lib.g3_self_attn_window_q_rows() == 256
    assert _plan(lib, dict(_canonical(1920, 2, 2, 320, 1, 1), head_dim=64))[0] is None  # (some refusal: the text below must survive accepted calls)
    before = lib.g3_last_error()
    assert before
    a = _canonical(1920, 2, 2, 320, 1, 1)
    assert _plan(lib, a) == (NM_WIN, None)
    assert _plan(lib, dict(a, logit_bound=0.0)) == (MAX_WIN, None)
    assert _plan(lib, dict(a, logit_bound=61.0 / math.log2(math.e))) == (MAX_WIN, None)  # beyond the no-max form's range
    assert _plan(lib, dict(a, window_frames=0, sink_frames=0)) == (NM_WIN, None)
    # the window covers every key of every block (T = 6 frames): the dense kernels
    assert _plan(lib, dict(a, window_frames=5, sink_frames=0)) == (NM_DENSE, None)
    assert _plan(lib, dict(a, window_frames=1 << 30, sink_frames=1 << 30)) == (NM_DENSE, None)
    assert _plan(lib, dict(a, window_frames=0, sink_frames=6)) == (NM_DENSE, None)
    assert _plan(lib, dict(a, window_frames=5, logit_bound=0.0)) == (MAX_DENSE, None)
    assert _plan(lib, dict(a, window_frames=4, sink_frames=5)) == (NM_WIN, None)
    # the product shape, and the same under another process-wide kernel option: the entry always resolves to the one-wave-per-SIMD family
    big = _canonical(56320, 2, 32, 3520, 2, 1)
    assert _plan(lib, big) == (NM_WIN, None)
    lib.g3_set_option(b"attn_variant", 4)
    try:
        assert _plan(lib, big) == (NM_WIN, None) and _plan(lib, dict(big, window_frames=15)) == (NM_DENSE, None)
    finally:
        lib.g3_set_option(b"attn_variant", 0)
    assert lib.g3_last_error() == before


def test_window_plan_refusals():
    lib = _lib.load()
    a = _canonical(1920, 2, 2, 320, 1, 1)
    shape = ": S {} and frame_len {} must be positive multiples of 64, S a multiple of frame_len"
    cases = [
        (dict(S=1900, vt_row=1920), FN + shape.format(1900, 320)),                      # S % 64
        (dict(frame_len=96), FN + shape.format(1920, 96)),                              # frame_len % 64
        (dict(frame_len=0), FN + shape.format(1920, 0)),
        (dict(frame_len=256), FN + shape.format(1920, 256)),                            # S % frame_len
        (dict(S=0), FN + shape.format(0, 320)),
        (dict(window_frames=-1), FN + ": window_frames -1 and sink_frames 1 must be >= 0"),
        (dict(sink_frames=-2), FN + ": window_frames 1 and sink_frames -2 must be >= 0"),
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
        for degenerate in (False, True):  # a window that covers everything is refused for the same reasons
            args = dict(a, **over)
            if degenerate and "window_frames" not in over and "sink_frames" not in over:
                args["window_frames"] = 1 << 20
            assert _plan(lib, args) == (None, text), (over, degenerate)
    # operands beyond the kernel's 32-bit byte offsets: the carry entry's arithmetic over all S keys
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
    # the dry run of the recorded entries does not know the window entry
    assert lib.g3_attn_plan_bf16(7, *([0] * 35)) is None and lib.g3_last_error() == b"g3_attn_plan_bf16: unknown entry 7"


def _brute_mask(S, frame_len, W, s, q_rows=256):
    """include/gen3c_hip.h: block b = rows [256 b, min(256 b + 256, S)) lies in frames f0..f1 and attends frames [max(0, f0 - W), min(T, f1 + W + 1)) and
    [0, min(s, T))."""
    T = S // frame_len
    blocks = [((i // q_rows * q_rows) // frame_len, (min(i // q_rows * q_rows + q_rows, S) - 1) // frame_len) for i in range(S)]  # (f0, f1) of row i's block
    frames = torch.tensor([[max(0, f0 - W) <= f < min(T, f1 + W + 1) or f < min(s, T) for f in range(T)] for f0, f1 in blocks])  # [row, key frame]
    return frames.repeat_interleave(frame_len, dim=1)


@pytest.mark.parametrize("S,frame_len,W,s", [(832, 64, 0, 0), (832, 64, 0, 1), (832, 64, 2, 3), (832, 64, 12, 0), (832, 64, 0, 13),
                                             (1920, 320, 0, 0), (1920, 320, 1, 1), (1920, 320, 2, 2), (1920, 320, 0, 2), (1920, 320, 5, 0)])
def test_window_mask_is_the_stated_function_and_the_tile_count_follows_it(S, frame_len, W, s):
    from gen3c_amd import ops
    mask = ops.window_attn_mask(S, frame_len, W, s)
    assert mask.dtype == torch.bool and mask.shape == (S, S) and mask.device.type == "cpu"
    assert torch.equal(mask, _brute_mask(S, frame_len, W, s))
    # a superset of the per-row window, and equal to it for blocks inside one frame
    f = torch.arange(S) // frame_len
    per_row = ((f[None, :] - f[:, None]).abs() <= W) | (f[None, :] < s)
    assert bool((mask | ~per_row).all())
    n_blk = (S + 255) // 256
    tiles = sum(int(mask[256 * b].view(S // 64, 64).any(dim=1).sum()) for b in range(n_blk))
    assert ops.window_attn_tiles(S, frame_len, W, s) == (tiles, n_blk * (S // 64))


def test_window_tiles_at_the_product_shape_and_its_refusals():
    from gen3c_amd import ops
    att, dense = ops.window_attn_tiles(56320, 3520, 2, 1)
    assert dense == 220 * 880 and 0.34 < att / dense < 0.40  # frame-granular density 87 / 256 = 0.34, plus the straddling blocks' extra frames
    assert ops.window_attn_tiles(56320, 3520, 15, 0) == (dense, dense) and ops.window_attn_tiles(56320, 3520, 0, 16) == (dense, dense)
    with pytest.raises(_lib.Gen3cHipError, match="g3_self_attn_window_tiles: S 1900 and frame_len 320 must be positive multiples of 64"):
        ops.window_attn_tiles(1900, 320, 1, 1)
    with pytest.raises(_lib.Gen3cHipError, match="g3_self_attn_window_tiles: window_frames -1 and sink_frames 0 must be >= 0"):
        ops.window_attn_tiles(1920, 320, -1, 0)


def test_cli_flags_and_environment(monkeypatch):
    import argparse
    from gen3c_amd import cli_common
    monkeypatch.delenv("G3_SELF_ATTN_WINDOW", raising=False)
    parse = lambda *argv: cli_common.self_attn_window_requested(cli_common.add_common_args(argparse.ArgumentParser()).parse_args(list(argv)))
    assert parse() is None
    assert parse("--self_attn_window_frames", "2") == (2, 1)
    assert parse("--self_attn_window_frames", "4", "--self_attn_sink_frames", "0") == (4, 0)
    with pytest.raises(ValueError, match="--self_attn_sink_frames 2 needs --self_attn_window_frames"):
        parse("--self_attn_sink_frames", "2")
    with pytest.raises(ValueError, match="window frames -1 and sink frames 1 must be >= 0"):
        parse("--self_attn_window_frames", "-1")
    monkeypatch.setenv("G3_SELF_ATTN_WINDOW", "2,3")
    assert parse() == (2, 3)
    assert parse("--self_attn_window_frames", "1") == (1, 1)  # the flags win
    monkeypatch.setenv("G3_SELF_ATTN_WINDOW", "4")
    assert parse() == (4, 1)
    monkeypatch.setenv("G3_SELF_ATTN_WINDOW", "two")
    with pytest.raises(ValueError, match="G3_SELF_ATTN_WINDOW='two': expected"):
        parse()


def test_dit_window_option_and_refusals():
    from gen3c_amd.dit import VideoExtendGeneralDIT
    kw = dict(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=1, num_heads=2, adaln_lora_dim=32,
              crossattn_emb_channels=128, device="cpu", init_weights=False)
    net = VideoExtendGeneralDIT(**kw)
    assert net.self_attn_window is None and net._self_attn_window_for(6, 8, 8) is None
    net = VideoExtendGeneralDIT(self_attn_window=(2, 0), **kw)
    assert net.self_attn_window == (2, 0) and net._self_attn_window_for(6, 8, 8) == (64, 2, 0)
    net.set_self_attn_window(1)
    assert net.self_attn_window == (1, 1) and net._self_attn_window_for(6, 8, 16) == (128, 1, 1)
    assert net._self_attn_window_for(2, 8, 8) is None and net._self_attn_window_for(6, 8, 8) is not None  # W >= frames - 1: the dense launch
    net.set_self_attn_window(0, sink_frames=6)
    assert net._self_attn_window_for(6, 8, 8) is None and net._self_attn_window_for(7, 8, 8) == (64, 0, 6)
    with pytest.raises(ValueError, match="window_frames -1 and sink_frames 1 must be >= 0"):
        net.set_self_attn_window(-1)
    net.set_self_attn_window(1, 1)
    with pytest.raises(ValueError) as e:
        net._self_attn_window_for(6, 8, 12)
    assert str(e.value) == ("self_attn_window=(1, 1): 8 x 12 = 96 tokens per latent frame is not a multiple of 64, the kernel's key tile "
                            "(the product size is 44 x 80 = 3520 = 55 x 64)")
    net._cp_attn, net.cp_size = object(), 4  # (what enable_context_parallel leaves behind)
    with pytest.raises(ValueError) as e:
        net._self_attn_window_for(6, 8, 8)
    assert str(e.value) == ("self_attn_window=(1, 1) with context parallelism over 4 ranks: the window form is single-GPU only. Windows under key sharding "
                            "would also cut the K / V exchange; that is later work")
    net.set_self_attn_window(None)
    assert net._self_attn_window_for(6, 8, 8) is None
