"""CPU: the frame window under context parallelism, without a launch - parallel.window_halo_plan against brute force from ops.window_attn_mask, every
refusal of g3_self_attn_fwd_window_cp_bf16 through its dry run, the per-rank tile count against the mask, the "window_halo" schedule over gloo with
a stub backend (tests/_cp_window_worker.py), and the DiT / command-line switch."""
import math
import socket

import pytest
import torch
import torch.multiprocessing as mp

from gen3c_amd import _lib

FN = "g3_self_attn_fwd_window_cp_bf16"
NM_WIN = "flash_attn_fwd_w4b_nm_win_kernel<true>"
MAX_WIN = "flash_attn_fwd_w4b_win_kernel<true>"
UNIT_BOUND = 128 / math.sqrt(128) * 1.03
ARGS = ["q", "q_row", "q_batch", "q_head", "k", "k_row", "k_batch", "k_head", "vt", "vt_row", "vt_batch", "vt_head", "o", "o_row", "o_batch", "o_head",
        "Sq", "Skv_buf", "B", "H", "head_dim", "softmax_scale", "logit_bound", "frame_len", "total_frames", "q_frame0", "buf_head_frames", "buf_tail_frame0",
        "window_frames", "sink_frames"]

# (T, world, W, s, frame_len) and the remote frames summed over ranks
PLAN_CASES = [((8, 4, 1, 1, 256), 9), ((8, 4, 0, 2, 256), 6), ((8, 4, 2, 0, 256), 12), ((6, 6, 1, 1, 320), 14), ((6, 3, 1, 1, 320), 6),
              ((16, 8, 2, 1, 3520), 34), ((16, 2, 2, 1, 3520), 5)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_mask(T, world, W, s, fl, r, unit=1):
    """ops.window_attn_mask of rank r with 256-row query blocks. unit = 64 states the same mask in 64-token units (frame_len, the 256 rows and the
    rank's first row are all multiples of 64, so every division in the definition is exact): one row / key per 64 - what keeps the 3 520-token cases
    small."""
    from gen3c_amd import ops
    assert fl % unit == 0 and 256 % unit == 0
    Sl = T // world * fl
    return ops.window_attn_mask(Sl // unit, fl // unit, W, s, q_rows=256 // unit, q_row0=r * Sl // unit, T_total=T)


@pytest.mark.parametrize("case,remote_total", PLAN_CASES)
def test_halo_plan_is_the_masks_frame_set(case, remote_total):
    from gen3c_amd import parallel
    T, world, W, s, fl = case
    plan = parallel.window_halo_plan(T, world, W, s)
    fpr = T // world
    assert plan["fpr"] == fpr and len(plan["buffers"]) == world
    unit = 64 if fl > 1024 else 1
    for r in range(world):
        mask = _rank_mask(T, world, W, s, fl, r, unit)
        assert mask.shape == (fpr * fl // unit, T * fl // unit)
        per_frame = mask.view(mask.shape[0], T, fl // unit)
        assert bool((per_frame.any(dim=2) == per_frame.all(dim=2)).all())  # whole frames
        attended = [f for f in range(T) if bool(per_frame[:, f].any())]
        a, b, c = plan["buffers"][r]
        assert 0 <= a <= b <= c <= T
        buf = list(range(0, a)) + list(range(b, c))
        assert buf == attended, (r, plan["buffers"][r], attended)
        # what p sends to r is what r expects from p: the frames of p's shard in r's buffer; sender-major they are the buffer, ascending
        got = []
        for p in range(world):
            pieces = plan["sends"][(p, r)]
            frames = [f for f0, f1 in pieces for f in range(f0, f1)]
            assert frames == [f for f in buf if p * fpr <= f < (p + 1) * fpr], (p, r, pieces)
            assert all(f0 < f1 for f0, f1 in pieces) and len(pieces) <= 2
            got += frames
        assert got == buf
        assert plan["remote_frames"][r] == len([f for f in buf if not r * fpr <= f < (r + 1) * fpr])
    assert sum(plan["remote_frames"]) == remote_total


def test_halo_plan_refusals_and_the_product_fraction():
    from gen3c_amd import parallel
    for bad in ((7, 2, 1, 1), (8, 0, 1, 1), (8, 4, -1, 1), (8, 4, 1, -1), (0, 1, 1, 1)):
        with pytest.raises(ValueError, match="window_halo_plan"):
            parallel.window_halo_plan(*bad)
    # the product shape: 34 remote frames against the dense exchange's 8 x 14 = 112
    plan = parallel.window_halo_plan(16, 8, 2, 1)
    assert sum(plan["remote_frames"]) == 34 and max(a + c - b for a, b, c in plan["buffers"]) == 7
    # a window that covers everything: every rank holds every frame
    assert parallel.window_halo_plan(8, 4, 7, 0)["buffers"] == [(0, 0, 8)] * 4 and parallel.window_halo_plan(8, 4, 0, 8)["buffers"] == [(0, 0, 8)] * 4
    # no sink: one piece that starts at the window
    assert parallel.window_halo_plan(8, 4, 1, 0)["buffers"] == [(0, 0, 3), (0, 1, 5), (0, 3, 7), (0, 5, 8)]


def _canonical(Sq, Skv_buf, B, H, fl, T, q_frame0, a, b, W, s, bound=UNIT_BOUND):
    """Contiguous [Sq*B, H*128] q / o, [Skv_buf*B, H*128] k and V^T [B, H, 128, Skv_buf] at placeholder addresses."""
    return dict(q=0x10000, q_row=B * H * 128, q_batch=H * 128, q_head=128, k=0x20000, k_row=B * H * 128, k_batch=H * 128, k_head=128,
                vt=0x30000, vt_row=Skv_buf, vt_batch=H * 128 * Skv_buf, vt_head=128 * Skv_buf, o=0x40000, o_row=B * H * 128, o_batch=H * 128, o_head=128,
                Sq=Sq, Skv_buf=Skv_buf, B=B, H=H, head_dim=128, softmax_scale=1.0 / math.sqrt(128), logit_bound=bound, frame_len=fl, total_frames=T,
                q_frame0=q_frame0, buf_head_frames=a, buf_tail_frame0=b, window_frames=W, sink_frames=s)


def _plan(lib, a):
    name = lib.g3_attn_window_cp_plan_bf16(*[a[n] for n in ARGS])
    return (name.decode(), None) if name is not None else (None, lib.g3_last_error().decode())


def test_window_cp_plan_names_the_kernel():
    lib = _lib.load()
    # rank 2 of 4 at T = 8, fl = 256, W = 1, s = 1: own frames [4, 6), buffer [0, 1) ++ [3, 7)
    a = _canonical(512, 5 * 256, 2, 2, 256, 8, 4, 1, 3, 1, 1)
    assert _plan(lib, a) == (NM_WIN, None)
    assert _plan(lib, dict(a, logit_bound=0.0)) == (MAX_WIN, None)
    assert _plan(lib, dict(a, logit_bound=61.0 / math.log2(math.e))) == (MAX_WIN, None)
    # a window that covers everything still runs the window kernels (the whole sequence as the buffer)
    full = _canonical(512, 8 * 256, 2, 2, 256, 8, 4, 0, 0, 1 << 20, 0)
    assert _plan(lib, full) == (NM_WIN, None)
    # a wider buffer is allowed: unattended keys are skipped
    assert _plan(lib, _canonical(512, 8 * 256, 2, 2, 256, 8, 4, 2, 2, 1, 1)) == (NM_WIN, None)  # [0, 2) ++ [2, 8) around the tight [0, 1) ++ [3, 7)
    assert _plan(lib, _canonical(512, 5 * 256, 2, 2, 256, 8, 6, 1, 4, 1, 1)) == (NM_WIN, None)  # the last rank with [0, 1) ++ [4, 8) around [5, 8)
    # the product shape: an interior rank of cp = 8 holds 7 of 16 frames
    big = _canonical(2 * 3520, 7 * 3520, 2, 32, 3520, 16, 6, 1, 4, 2, 1)
    assert _plan(lib, big) == (NM_WIN, None)


def test_window_cp_plan_refusals():
    lib = _lib.load()
    a = _canonical(512, 5 * 256, 2, 2, 256, 8, 4, 1, 3, 1, 1)  # rank 2 of 4: frames [4, 6), buffer [0, 1) ++ [3, 7)
    S5 = 5 * 256
    held = "which the buffer of frames [0, {}) ++ [{}, {}) x 256 keys does not hold"
    cases = [
        (dict(frame_len=96), FN + ": Sq 512, Skv_buf 1280 and frame_len 96 must be positive, frame_len a multiple of 64"),
        (dict(frame_len=0), FN + ": Sq 512, Skv_buf 1280 and frame_len 0 must be positive, frame_len a multiple of 64"),
        (dict(Sq=0), FN + ": Sq 0, Skv_buf 1280 and frame_len 256 must be positive, frame_len a multiple of 64"),
        (dict(window_frames=-1), FN + ": window_frames -1 and sink_frames 1 must be >= 0"),
        (dict(sink_frames=-2), FN + ": window_frames 1 and sink_frames -2 must be >= 0"),
        (dict(Sq=448), FN + ": Sq 448 is not a multiple of frame_len 256 (a rank owns whole frames)"),
        (dict(total_frames=0), FN + ": total_frames 0 must be positive and q_frame0 4 >= 0"),
        (dict(q_frame0=-1), FN + ": total_frames 8 must be positive and q_frame0 -1 >= 0"),
        (dict(buf_head_frames=4), FN + ": buf_head_frames 4 and buf_tail_frame0 3 must satisfy 0 <= a <= b"),
        (dict(buf_head_frames=-1), FN + ": buf_head_frames -1 and buf_tail_frame0 3 must satisfy 0 <= a <= b"),
        (dict(q_frame0=7), FN + ": the queries' frames [7, 9) reach beyond total_frames 8"),
        (dict(Skv_buf=S5 + 64), FN + ": Skv_buf 1344 is not (a + c - b) * frame_len for a c in [b, total_frames]: a 1, b 3, frame_len 256, total_frames 8"),
        (dict(Skv_buf=7 * 256), FN + ": Skv_buf 1792 is not (a + c - b) * frame_len for a c in [b, total_frames]: a 1, b 3, frame_len 256, total_frames 8"),
        (dict(buf_head_frames=3, buf_tail_frame0=4, Skv_buf=2 * 256),
         FN + ": Skv_buf 512 is not (a + c - b) * frame_len for a c in [b, total_frames]: a 3, b 4, frame_len 256, total_frames 8"),
        # a buffer one frame short of a workgroup's key set: at the tail (block 1 = frame 5 attends [4, 7)), at the window's start (block 0 = frame 4
        # attends [3, 6)) and in the sink
        (dict(Skv_buf=4 * 256), FN + ": query block 1 attends keys [0, 256) u [1024, 1792), " + held.format(1, 3, 6)),
        (dict(buf_tail_frame0=4, Skv_buf=4 * 256), FN + ": query block 0 attends keys [0, 256) u [768, 1536), " + held.format(1, 4, 7)),
        (dict(buf_head_frames=0, Skv_buf=4 * 256), FN + ": query block 0 attends keys [0, 256) u [768, 1536), " + held.format(0, 3, 7)),
        (dict(vt_row=S5 - 64), FN + ": V^T leading dim 1216 below ceil64(S) 1280"),
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
    # a sink that reaches the window needs ONE range: a gap inside it is a missing key
    merged = _canonical(512, 5 * 256, 2, 2, 256, 8, 2, 0, 0, 1, 1)  # rank 1: frames [2, 4), window [1, 5) + sink [0, 1) = [0, 5)
    assert _plan(lib, merged) == (NM_WIN, None)
    assert _plan(lib, dict(merged, buf_head_frames=1, buf_tail_frame0=2, Skv_buf=4 * 256)) == \
        (None, FN + ": query block 0 attends keys [0, 256) u [256, 1024), " + held.format(1, 2, 5))
    # operands beyond the kernel's 32-bit byte offsets: the arithmetic over the buffer's keys
    row = 1 << 21
    k_max = (S5 - 1 + 2 * 64) * row * 2 + 256
    v_max = 127 * S5 * 2 + (S5 + 64) * 2 + 256
    assert k_max > 0xFFFFFFFF
    assert _plan(lib, dict(a, k_row=row)) == (None, f"{FN}: K / V^T span exceeds the kernel's 32-bit byte offsets (k {k_max}, vt {v_max} bytes)")


TILE_CASES = [(8, 4, 1, 1, 256), (8, 4, 0, 2, 256), (8, 4, 2, 0, 256), (6, 6, 1, 1, 320), (6, 3, 1, 1, 320), (6, 6, 0, 2, 320), (6, 3, 0, 2, 320),
              (13, 13, 0, 1, 64), (16, 8, 2, 1, 3520)]


@pytest.mark.parametrize("T,world,W,s,fl", TILE_CASES)
def test_window_cp_tiles_follow_the_mask(T, world, W, s, fl):
    from gen3c_amd import ops, parallel
    plan = parallel.window_halo_plan(T, world, W, s)
    Sl = T // world * fl
    unit = 64 if fl > 1024 else 1
    total = 0
    for r in range(world):
        a, b, c = plan["buffers"][r]
        att, dense = ops.window_attn_tiles_cp(Sl, (a + c - b) * fl, fl, T, r * T // world, a, b, W, s)
        mask = _rank_mask(T, world, W, s, fl, r, unit)
        n_blk = (Sl + 255) // 256
        tiles = sum(int(mask[256 // unit * blk].view(-1, 64 // unit).any(dim=1).sum()) for blk in range(n_blk))
        assert (att, dense) == (tiles, n_blk * (T * fl // 64)), (r, att, tiles)
        total += att
    if all((r * Sl) % 256 == 0 for r in range(world)):  # the ranks' blocks are the single-GPU blocks
        assert total == ops.window_attn_tiles(T * fl, fl, W, s)[0]
    with pytest.raises(_lib.Gen3cHipError, match="g3_self_attn_window_cp_tiles: Sq 448 is not a multiple of frame_len 256"):
        ops.window_attn_tiles_cp(448, 1280, 256, 8, 4, 1, 3, 1, 1)


def test_window_mask_default_call_is_unchanged_and_the_rank_form_slices_it():
    from gen3c_amd import ops
    S, fl, W, s = 2048, 256, 1, 1
    whole = ops.window_attn_mask(S, fl, W, s)
    assert torch.equal(whole, ops.window_attn_mask(S, fl, W, s, q_row0=0, T_total=8))
    for r in range(4):  # 256-aligned shards: a rank's mask is its rows of the single-GPU mask
        assert torch.equal(ops.window_attn_mask(512, fl, W, s, q_row0=512 * r, T_total=8), whole[512 * r:512 * (r + 1)])
    # misaligned shards (fl = 320, one frame per rank): blocks count from the rank's first row, so rank 1's rows differ from the single-GPU mask's
    whole = ops.window_attn_mask(1920, 320, 1, 1)
    r1 = ops.window_attn_mask(320, 320, 1, 1, q_row0=320, T_total=6)
    assert r1.shape == (320, 1920) and not torch.equal(r1, whole[320:640])
    assert bool(r1[:, :960].all()) and not bool(r1[:, 960:].any())  # frame 1 alone: frames [0, 3)
    with pytest.raises(ValueError, match="window_attn_mask"):
        ops.window_attn_mask(320, 320, 1, 1, q_row0=100, T_total=6)
    with pytest.raises(ValueError, match="window_attn_mask"):
        ops.window_attn_mask(640, 320, 1, 1, q_row0=1600, T_total=6)


@pytest.mark.parametrize("world", [2, 4])
def test_window_halo_schedule_over_gloo(tmp_path, world):
    from tests import _cp_window_worker
    mp.spawn(_cp_window_worker.worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


def test_window_halo_needs_its_numbers_and_its_backend(monkeypatch):
    from gen3c_amd import parallel
    monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 0)
    assert parallel.CP_SCHEDULES[:4] == ("gather_first", "local_first", "local_carry", "head_parallel") and parallel.CP_SCHEDULES[4] == "window_halo"
    k = torch.zeros(128, 256)
    cpa = parallel.ContextParallelAttention(object(), backend=dict(pack=None), schedule="window_halo")
    with pytest.raises(ValueError, match=r'schedule "window_halo" needs configure\(window=\(frame_len, W, s\)\)'):
        cpa.start(k, k, 128, 1, 2)
    cpa.configure(window=(64, 1, 1))
    with pytest.raises(ValueError, match='the backend has no "attention_window_cp"'):
        cpa.start(k, k, 128, 1, 2)
    cpa.backend = dict(attention_window_cp=None)
    cpa.configure(window=(96, 1, 1))
    with pytest.raises(ValueError, match="S_local 128 is not a multiple of frame_len 96"):
        cpa.start(k, k, 128, 1, 2)
    with pytest.raises(ValueError, match="window_halo: frame_len 0 must be positive"):
        cpa.configure(window=(0, 1, 1))
    cpb = parallel.ContextParallelAttention(object(), schedule="local_carry")
    assert cpb.configure(window=(64, 2, 1)).schedule == "window_halo" and cpb.window == (64, 2, 1)
    assert cpb.configure(head_groups=2).schedule == "window_halo"  # (other settings leave the window alone)
    assert cpb.configure(window=None).schedule == "local_carry" and cpb.window is None


def test_dit_switch_and_the_refusal_without_it(monkeypatch):
    from gen3c_amd import parallel
    from gen3c_amd.dit import VideoExtendGeneralDIT
    kw = dict(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=1, num_heads=2, adaln_lora_dim=32,
              crossattn_emb_channels=128, device="cpu", init_weights=False)
    monkeypatch.delenv("G3_CP_CONFIG", raising=False)
    monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 4)
    monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 1)
    net = VideoExtendGeneralDIT(self_attn_window=(1, 1), **kw)
    assert net.self_attn_window == (1, 1) and net.self_attn_window_cp is False
    net.enable_context_parallel(object())
    with pytest.raises(ValueError) as e:  # without the switch: the old text, word for word
        net._self_attn_window_for(2, 16, 16)
    assert str(e.value) == ("self_attn_window=(1, 1) with context parallelism over 4 ranks: the window form is single-GPU only. Windows under key sharding "
                            "would also cut the K / V exchange; that is later work")
    assert net._cp_attn.schedule == "local_first" and net._cp_attn.window is None
    for make in (lambda: VideoExtendGeneralDIT(self_attn_window=(1, 1), self_attn_window_cp=True, **kw),
                 lambda: (lambda n: (n.set_self_attn_window(1, 1, context_parallel=True), n)[1])(VideoExtendGeneralDIT(**kw))):
        net = make()
        assert net.self_attn_window == (1, 1) and net.self_attn_window_cp is True
        assert net._self_attn_window_for(8, 16, 16) == (256, 1, 1)  # a single GPU: the switch means nothing
        net.enable_context_parallel(object())
        # 2 local frames x 4 ranks = 8 global frames of 16 x 16 = 256 tokens
        assert net._self_attn_window_for(2, 16, 16) is None
        assert net._cp_attn.schedule == "window_halo" and net._cp_attn.window == (256, 1, 1)
        assert not net._cp_fused_qkv()  # K / V first: the exchange flies under the Q projection
        with pytest.raises(ValueError, match="8 x 12 = 96 tokens per latent frame is not a multiple of 64"):
            net._self_attn_window_for(2, 8, 12)
        # the window covers every frame of the WHOLE sequence (not just the rank's two): the rank's ordinary schedule
        net.set_self_attn_window(7, 0, context_parallel=True)
        assert net._self_attn_window_for(2, 16, 16) is None and net._cp_attn.schedule == "local_first" and net._cp_attn.window is None
        net.set_self_attn_window(1, 0, context_parallel=True)  # covers the rank's own two frames, not the sequence's eight
        assert net._self_attn_window_for(2, 16, 16) is None and net._cp_attn.window == (256, 1, 0)
        net.set_self_attn_window(None)
        assert net.self_attn_window_cp is False and net._self_attn_window_for(2, 16, 16) is None and net._cp_attn.schedule == "local_first"


def test_cli_flag_and_environment_field(monkeypatch):
    import argparse
    from gen3c_amd import cli_common
    monkeypatch.delenv("G3_SELF_ATTN_WINDOW", raising=False)
    args = lambda *argv: cli_common.add_common_args(argparse.ArgumentParser()).parse_args(list(argv))
    assert cli_common.self_attn_window_cp_requested(args()) is False
    assert cli_common.self_attn_window_cp_requested(args("--self_attn_window_frames", "2", "--self_attn_window_cp")) is True
    monkeypatch.setenv("G3_SELF_ATTN_WINDOW", "2,1,cp")
    assert cli_common.self_attn_window_requested(args()) == (2, 1) and cli_common.self_attn_window_cp_requested(args()) is True
    monkeypatch.setenv("G3_SELF_ATTN_WINDOW", "2,1")
    assert cli_common.self_attn_window_requested(args()) == (2, 1) and cli_common.self_attn_window_cp_requested(args()) is False
    monkeypatch.setenv("G3_SELF_ATTN_WINDOW", "2,1,3")
    with pytest.raises(ValueError, match="G3_SELF_ATTN_WINDOW='2,1,3': expected"):
        cli_common.self_attn_window_requested(args())
