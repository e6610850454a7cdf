"""Worker of tests/test_attn_window_cp_cpu.py (gloo, CPU tensors): ContextParallelAttention's "window_halo" schedule with a stub backend - an fp32
masked softmax over the compact buffer, which restates what g3_self_attn_fwd_window_cp_bf16 computes from the same arguments - against each rank's
rows of the masked dense softmax over the whole sequence."""
import math
import os

import torch
import torch.distributed as dist

# (frame_len, frames per rank, B, H, head_groups, W, s): blocks inside a frame, blocks that straddle, one group / several, a sink that reaches the window
CASES = ((256, 2, 1, 4, 2, 1, 1), (320, 1, 2, 2, 1, 1, 1), (64, 3, 1, 4, 4, 0, 2), (128, 2, 2, 2, 2, 2, 0), (64, 2, 1, 2, 1, 0, 0))


def masked_softmax(q, k, v, mask, Sq, B, H):
    """q [Sq*B, H*128], k / v [Skv*B, H*128] rows (s, b), mask bool [Sq, Skv] -> fp32 [Sq*B, H*128]."""
    q4 = q.reshape(Sq, B, H, 128).permute(1, 2, 0, 3).float()
    k4 = k.reshape(-1, B, H, 128).permute(1, 2, 0, 3).float()
    v4 = v.reshape(-1, B, H, 128).permute(1, 2, 0, 3).float()
    sc = (q4 @ k4.transpose(-1, -2) / math.sqrt(128.0)).masked_fill(~mask, float("-inf"))
    return (torch.softmax(sc, dim=-1) @ v4).permute(2, 0, 1, 3).reshape(Sq * B, H * 128)


def stub_backend(calls):
    from gen3c_amd import ops

    def transpose_v(v, S, B, H):
        return v.reshape(S, B, H, 128).permute(1, 2, 3, 0).contiguous()

    def attention_window_cp(q, k, vt, Sq, Skv_buf, B, H, logit_bound, out, frame_len, total_frames, q_frame0, buf_head, buf_tail0, W, s):
        calls.append((Sq, Skv_buf, H, q_frame0, buf_head, buf_tail0))
        assert k.shape[0] == Skv_buf * B and vt.shape == (B, H, 128, Skv_buf)
        full = ops.window_attn_mask(Sq, frame_len, W, s, q_rows=256, q_row0=q_frame0 * frame_len, T_total=total_frames)
        c = Skv_buf // frame_len - buf_head + buf_tail0
        keys = torch.cat([torch.arange(0, buf_head * frame_len), torch.arange(buf_tail0 * frame_len, c * frame_len)])
        held = torch.zeros(total_frames * frame_len, dtype=torch.bool)
        held[keys] = True
        assert not bool(full[:, ~held].any()), "the buffer misses a key some row attends"
        assert bool(full[:, held].view(Sq, -1, frame_len).any(dim=2).any(dim=0).all()), "the plan's buffer is tight: every frame in it is attended"
        v = vt.permute(3, 0, 1, 2).reshape(Skv_buf * B, H * 128)
        out.copy_(masked_softmax(q, k, v, full[:, keys], Sq, B, H).to(out.dtype))
        return out

    return dict(pack=lambda t: t.contiguous(), transpose_v=transpose_v, attention_window_cp=attention_window_cp)


def worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from gen3c_amd import ops, parallel
    parallel.init_distributed("gloo")
    parallel.parallel_state.initialize_model_parallel(context_parallel_size=world)
    group = parallel.parallel_state.get_context_parallel_group()
    try:
        g = torch.Generator().manual_seed(0)
        for fl, fpr, B, H, G, W, s in CASES:
            Sl, T = fl * fpr, fpr * world
            S, D = Sl * world, H * 128
            q, k, v = (torch.randn(S * B, D, generator=g) for _ in range(3))
            rows = slice(rank * Sl * B, (rank + 1) * Sl * B)
            mask = ops.window_attn_mask(Sl, fl, W, s, q_rows=256, q_row0=rank * Sl, T_total=T)
            ref = masked_softmax(q[rows], k, v, mask, Sl, B, H)
            qkv = torch.cat([q[rows], k[rows], v[rows]], dim=1)  # column views of one buffer, as in the DiT
            calls = []
            cpa = parallel.ContextParallelAttention(group, head_groups=G, backend=stub_backend(calls), schedule="window_halo")
            cpa.configure(window=(fl, W, s))
            cpa.stats = []
            out = cpa(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], Sl, B, H, logit_bound=3.0)
            torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
            assert cpa.effective == dict(schedule="window_halo", kernel="w4b", head_groups=G), cpa.effective
            plan = parallel.window_halo_plan(T, world, W, s)
            a, b, c = plan["buffers"][rank]
            assert calls == [(Sl, (a + c - b) * fl, H // G, rank * fpr, a, b)] * G, calls
            assert cpa.bytes_gathered == 2 * plan["remote_frames"][rank] * fl * B * D * q.element_size(), (cpa.bytes_gathered, plan["remote_frames"])
            # back to the schedule configured before the window
            assert cpa.configure(window=None).schedule == "gather_first" and cpa.window is None
        with open(os.path.join(tmp, f"ok{rank}"), "w") as f:
            f.write("ok")
    finally:
        dist.destroy_process_group()
