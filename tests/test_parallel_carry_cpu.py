"""CPU (gloo, world sizes 2, 3 and 8): the "local_carry" context-parallel schedule - own shard first into an fp32 partial, then ONE launch per
head group over every remote key that carries the partial in (an interior rank skips its own block inside the gathered buffers) - checked
against full attention over the gathered sequence. The HIP kernels cannot run here, so the attention callables are an oracle restated below,
with the semantics of g3_flash_attn_fwd_carry_bf16 (kv_skip, carry-in, partial output into a caller's fp32 view)."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _v_rows(vt, B, H):
    """V^T [B,H,128,S] or rank-major segments [n,B,H,128,S_seg] -> V [S,B,H,128]."""
    if vt.dim() == 5:
        n, S_seg = vt.shape[0], vt.shape[-1]
        return vt.permute(0, 4, 1, 2, 3).reshape(n * S_seg, B, H, 128)
    return vt.permute(3, 0, 1, 2)


def _part(q, k, v, Sq, B, H):
    """fp64 softmax part over the given keys: (normalised o [Sq*B, H*128], log2-domain lse [B,H,Sq])."""
    q4 = q.reshape(Sq, B, H, 128).permute(1, 2, 0, 3).double()
    k4 = k.reshape(-1, B, H, 128).permute(1, 2, 0, 3).double()
    v4 = v.permute(1, 2, 0, 3).double()
    sc = q4 @ k4.transpose(-1, -2) / math.sqrt(128.0)
    o = torch.softmax(sc, dim=-1) @ v4
    return o.permute(2, 0, 1, 3).reshape(Sq * B, H * 128), torch.logsumexp(sc, dim=-1) / math.log(2.0)


def _oracle_backend(with_carry=True):
    def transpose_v(v, S, B, H):
        return v.reshape(S, B, H, 128).permute(1, 2, 3, 0).contiguous()

    def attention(q, k, vt, Sq, Skv, B, H, out, variant=0):
        o, _ = _part(q, k, _v_rows(vt, B, H), Sq, B, H)
        out.copy_(o.to(out.dtype))
        return out

    def attention_partial(q, k, vt, Sq, Skv, B, H, variant=0):
        o, lse = _part(q, k, _v_rows(vt, B, H), Sq, B, H)
        return o.float(), lse.float().contiguous()

    def merge(parts, Sq, B, H, out):
        l = torch.stack([p[1].double() for p in parts])
        w = torch.softmax(l * math.log(2.0), dim=0)
        acc = 0
        for i, (o, _) in enumerate(parts):
            acc = acc + o.double().reshape(Sq, B, H, 128) * w[i].permute(2, 0, 1)[..., None]
        out.copy_(acc.reshape(Sq * B, H * 128).to(out.dtype))
        return out

    def attention_carry(q, k, vt, Sq, Skv, B, H, out=None, carry=None, kv_skip=None, partial=False, variant=0):
        v = _v_rows(vt, B, H)
        k3 = k.reshape(-1, B, H * 128)
        if kv_skip is not None:  # logical key j at physical j + (j >= begin ? len : 0)
            b0, n = kv_skip
            assert b0 % 64 == 0 and n % 64 == 0 and k3.shape[0] == Skv + n
            keep = torch.cat([torch.arange(0, b0), torch.arange(b0 + n, Skv + n)])
            k3, v = k3[keep], v[keep]
        assert k3.shape[0] == Skv and v.shape[0] == Skv
        o, lse = _part(q, k3.reshape(Skv * B, H * 128), v, Sq, B, H)
        if carry is not None:
            oc, lc = carry
            assert out is not None and oc.stride() == out.stride(), "carry_o has the output's strides"
            m = torch.maximum(lc.double(), lse)
            wc, wk = torch.exp2(lc.double() - m), torch.exp2(lse - m)
            per_row = lambda w: w.permute(2, 0, 1).reshape(Sq * B, H, 1)  # [B,H,Sq] -> rows (s, b), per head
            o = ((per_row(wc) * oc.double().reshape(Sq * B, H, 128) + per_row(wk) * o.reshape(Sq * B, H, 128)) / per_row(wc + wk)).reshape(Sq * B, H * 128)
            lse = m + torch.log2(wc + wk)
        if partial:
            out = torch.empty(Sq * B, H * 128) if out is None else out
            out.copy_(o.float())
            return out, lse.float().contiguous()
        out.copy_(o.to(out.dtype))
        return out

    be = dict(pack=lambda t: t.contiguous(), transpose_v=transpose_v, attention=attention, attention_partial=attention_partial, merge=merge)
    if with_carry:
        be["attention_carry"] = attention_carry
    return be


def _worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from gen3c_amd import parallel
    parallel.init_distributed("gloo")
    parallel.parallel_state.initialize_model_parallel(context_parallel_size=world)
    group = parallel.parallel_state.get_context_parallel_group()
    try:
        g = torch.Generator().manual_seed(0)
        # S_local = 64 / 128: V^T shards gathered as key segments (the carry schedule runs); S_local = 24: not segmented (local_first fallback)
        for Sl, B, H, G in ((64, 1, 4, 2), (128, 2, 4, 4), (24, 2, 4, 2)):
            S = Sl * world
            q = torch.randn(S * B, H * 128, generator=g)
            k = torch.randn(S * B, H * 128, generator=g)
            v = torch.randn(S * B, H * 128, generator=g)
            ref, _ = _part(q, k, v.reshape(S, B, H, 128), S, B, H)
            rows = slice(rank * Sl * B, (rank + 1) * Sl * B)
            D = H * 128
            qkv_local = torch.cat([q[rows], k[rows], v[rows]], dim=1)
            cpa = parallel.ContextParallelAttention(group, head_groups=G, backend=_oracle_backend(), schedule="local_carry")
            out = cpa(qkv_local[:, :D], qkv_local[:, D:2 * D], qkv_local[:, 2 * D:], Sl, B, H)
            torch.testing.assert_close(out, ref[rows].float(), rtol=1e-5, atol=1e-5)
            assert cpa.effective["schedule"] == ("local_carry" if Sl % 64 == 0 else "gather_first"), cpa.effective
            # a backend without the carry form: the same request runs local_first, and says so
            cpf = parallel.ContextParallelAttention(group, head_groups=G, backend=_oracle_backend(with_carry=False)).configure(schedule="local_carry")
            out2 = cpf(qkv_local[:, :D], qkv_local[:, D:2 * D], qkv_local[:, 2 * D:], Sl, B, H)
            torch.testing.assert_close(out2, ref[rows].float(), rtol=1e-5, atol=1e-5)
            assert cpf.effective["schedule"] == ("local_first" if Sl % 64 == 0 else "gather_first"), cpf.effective
        with open(os.path.join(tmp, f"ok{rank}"), "w") as f:
            f.write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])  # 3 and 8: interior ranks, whose remote keys sit on both sides of their own block
def test_local_carry_schedule_world(tmp_path, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


def test_local_carry_world_one_falls_back(tmp_path):
    """world = 1: nothing to exchange - the request runs as local_first would (gather_first with one rank), and effective says so."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    from gen3c_amd import parallel
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        g = torch.Generator().manual_seed(1)
        S, B, H = 64, 1, 2
        q, k, v = (torch.randn(S * B, H * 128, generator=g) for _ in range(3))
        cpa = parallel.ContextParallelAttention(dist.group.WORLD, head_groups=2, backend=_oracle_backend(), schedule="local_carry")
        out = cpa(q, k, v, S, B, H)
        ref, _ = _part(q, k, v.reshape(S, B, H, 128), S, B, H)
        torch.testing.assert_close(out, ref.float(), rtol=1e-5, atol=1e-5)
        assert cpa.effective["schedule"] == "gather_first"
    finally:
        if created:
            dist.destroy_process_group()


def test_schedule_names():
    from gen3c_amd import parallel
    assert "local_carry" in parallel.CP_SCHEDULES
    assert parallel.CP_SCHEDULES[:2] == ("gather_first", "local_first")


def test_cp_config_env_accepts_local_carry(monkeypatch):
    """G3_CP_CONFIG="4,auto,local_carry" reaches ContextParallelAttention through dit.enable_context_parallel (no GPU work: an unbuilt network
    object, only the CP plumbing), and the DiT then takes the ONE fused QKV projection for it, as for local_first (phase 1 waits for nothing)."""
    from gen3c_amd import parallel
    from gen3c_amd.dit import VideoExtendGeneralDIT
    monkeypatch.setenv("G3_CP_CONFIG", "4,auto,local_carry")
    monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 3)
    monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 1)
    net = VideoExtendGeneralDIT.__new__(VideoExtendGeneralDIT)
    net._tables = {}
    VideoExtendGeneralDIT.enable_context_parallel(net, object())
    assert net._cp_attn.schedule == "local_carry" and net._cp_attn.head_groups == 4 and net._cp_attn.kernel == "auto"
    assert net._cp_fused_qkv()
    for sched, fused in (("local_first", True), ("gather_first", False), ("local_carry", True)):
        net._cp_attn.configure(schedule=sched)
        assert net._cp_fused_qkv() == fused, sched
    net._cp_attn = None
    assert not net._cp_fused_qkv()
