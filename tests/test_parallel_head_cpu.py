"""CPU (gloo, world sizes 2, 4 and 8; 3 for the fallback): the "head_parallel" context-parallel schedule - per head group a scatter of q, k and v
by destination rank, three single-tensor all-to-alls, the ordinary full-length attention over this rank's heads, a fourth all-to-all and the
gather into the group's output columns - checked against full attention over the gathered sequence. The HIP kernels cannot run here, so the
backend callables are an fp64 oracle restated below, with the semantics of g3_cp_scatter_heads_bf16 / g3_cp_gather_heads_bf16."""
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


def _oracle_backend(with_exchange=True, calls=None):
    def transpose_v(v, S, B, H):
        return v.reshape(S, B, H, 128).permute(1, 2, 3, 0).contiguous()

    def attention(q, k, vt, Sq, Skv, B, H, out, variant=0):
        if calls is not None:
            calls.append(("attention", Sq, Skv, H))
        o, _ = _part(q, k, _v_rows(vt, B, H), Sq, B, H)
        out.copy_(o.to(out.dtype))
        return out

    def attention_bounded(q, k, vt, Sq, Skv, B, H, logit_bound, out, variant=0):
        assert logit_bound > 0 and vt.dim() == 4, "the bounded entry takes a bound and plain V^T"
        if calls is not None:
            calls.append(("attention_bounded", Sq, Skv, H))
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

    def scatter_heads(q, k, v, H, n_dest, head0, Hg):
        """x_out[d][r][j] = x[r][(d * (H / n_dest) + head0) * 128 + j]"""
        assert H % n_dest == 0 and head0 + Hg <= H // n_dest
        def one(x):
            if x is None:
                return None
            assert x.shape[1] == H * 128
            return torch.stack([x[:, (d * (H // n_dest) + head0) * 128:(d * (H // n_dest) + head0 + Hg) * 128] for d in range(n_dest)]).contiguous()
        return one(q), one(k), one(v)

    def gather_heads(x, out, H, head0):
        n_src, rows, W = x.shape
        assert H % n_src == 0 and head0 + W // 128 <= H // n_src and out.shape == (rows, H * 128)
        for s in range(n_src):
            c0 = (s * (H // n_src) + head0) * 128
            out[:, c0:c0 + W] = x[s]
        return out

    be = dict(pack=lambda t: t.contiguous(), transpose_v=transpose_v, attention=attention, attention_partial=attention_partial, merge=merge)
    if with_exchange:
        be.update(scatter_heads=scatter_heads, gather_heads=gather_heads, attention_bounded=attention_bounded)
    return be


CASES = ((64, 1, 8, 2), (24, 2, 8, 1), (128, 2, 16, 4))  # (S_local, B, H, head_groups)


def _worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from gen3c_amd import parallel
    parallel.init_distributed("gloo")
    parallel.parallel_state.initialize_model_parallel(context_parallel_size=world)
    group = parallel.parallel_state.get_context_parallel_group()
    try:
        g = torch.Generator().manual_seed(0)
        for ci, (Sl, B, H, G) in enumerate(CASES if world != 3 else ((64, 1, 4, 2),)):
            S = Sl * world
            q = torch.randn(S * B, H * 128, generator=g)
            k = torch.randn(S * B, H * 128, generator=g)
            v = torch.randn(S * B, H * 128, generator=g)
            rows = slice(rank * Sl * B, (rank + 1) * Sl * B)
            ref, _ = _part(q[rows], k, v.reshape(S, B, H, 128), Sl, B, H)  # this rank's query rows against every key
            D = H * 128
            qkv_local = torch.cat([q[rows], k[rows], v[rows]], dim=1)
            calls = []
            cpa = parallel.ContextParallelAttention(group, head_groups=G, backend=_oracle_backend(calls=calls), schedule="head_parallel")
            cpa.stats = []
            bound = 3.0 if ci % 2 else 0.0  # with a bound the bounded backend entry runs, without one the plain entry
            out = cpa(qkv_local[:, :D], qkv_local[:, D:2 * D], qkv_local[:, 2 * D:], Sl, B, H, logit_bound=bound)
            torch.testing.assert_close(out, ref.float(), rtol=1e-5, atol=1e-5)
            if world == 3:  # H = 4 heads do not divide over 3 ranks: the request runs local_first, and says so
                assert cpa.effective["schedule"] == "local_first", cpa.effective
                continue
            Hl = H // world
            Ge = max(d for d in range(1, G + 1) if Hl % d == 0)
            assert cpa.effective["schedule"] == "head_parallel" and cpa.effective["head_groups"] == Ge, cpa.effective
            # one full-length launch per group over this rank's heads of the group, through the entry the bound selects
            assert calls == [("attention_bounded" if bound else "attention", S, S, Hl // Ge)] * Ge, calls
            # received from the other ranks: q, k, v and o, (world - 1) row blocks of this rank's H / world heads each
            assert cpa.bytes_gathered == 4 * (world - 1) * (Sl * B) * Hl * 128 * q.element_size(), cpa.bytes_gathered
            if ci:
                continue
            # a backend without the exchange callables: the same request runs local_first, and says so
            cpf = parallel.ContextParallelAttention(group, head_groups=G, backend=_oracle_backend(with_exchange=False)).configure(schedule="head_parallel")
            out2 = cpf(qkv_local[:, :D], qkv_local[:, D:2 * D], qkv_local[:, 2 * D:], Sl, B, H)
            torch.testing.assert_close(out2, ref.float(), rtol=1e-5, atol=1e-5)
            assert cpf.effective["schedule"] == "local_first", cpf.effective
        with open(os.path.join(tmp, f"ok{rank}"), "w") as f:
            f.write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_head_parallel_schedule_world(tmp_path, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


def test_head_parallel_world_three_runs_local_first(tmp_path):
    mp.spawn(_worker, args=(3, _free_port(), str(tmp_path)), nprocs=3, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(3))


def test_head_parallel_world_one_self_exchange(tmp_path):
    """world = 1: the schedule still runs - scatter, the real all_to_all_single with itself, attention, return, gather."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    from gen3c_amd import parallel
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        g = torch.Generator().manual_seed(1)
        S, B, H = 72, 2, 4
        q, k, v = (torch.randn(S * B, H * 128, generator=g) for _ in range(3))
        cpa = parallel.ContextParallelAttention(dist.group.WORLD, head_groups=2, backend=_oracle_backend(), schedule="head_parallel")
        cpa.stats = []
        out = cpa(q, k, v, S, B, H)
        ref, _ = _part(q, k, v.reshape(S, B, H, 128), S, B, H)
        torch.testing.assert_close(out, ref.float(), rtol=1e-5, atol=1e-5)
        assert cpa.effective["schedule"] == "head_parallel" and cpa.effective["head_groups"] == 2
        assert cpa.bytes_gathered == 0
    finally:
        if created:
            dist.destroy_process_group()


def test_schedule_name_is_appended():
    from gen3c_amd import parallel
    assert "head_parallel" in parallel.CP_SCHEDULES
    assert parallel.CP_SCHEDULES[:3] == ("gather_first", "local_first", "local_carry")


def test_cp_config_env_accepts_head_parallel(monkeypatch):
    """G3_CP_CONFIG="4,auto,head_parallel" reaches ContextParallelAttention through dit.enable_context_parallel (no GPU work: an unbuilt network
    object, only the CP plumbing), and the DiT then takes the ONE fused QKV projection for it; the other schedules keep their projections."""
    from gen3c_amd import parallel
    from gen3c_amd.dit import VideoExtendGeneralDIT
    monkeypatch.setenv("G3_CP_CONFIG", "4,auto,head_parallel")
    monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 4)
    monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 1)
    net = VideoExtendGeneralDIT.__new__(VideoExtendGeneralDIT)
    net._tables = {}
    VideoExtendGeneralDIT.enable_context_parallel(net, object())
    assert isinstance(net._cp_attn, parallel.ContextParallelAttention)
    assert net._cp_attn.schedule == "head_parallel" and net._cp_attn.head_groups == 4 and net._cp_attn.kernel == "auto"
    assert net._cp_fused_qkv()
    for sched, fused in (("local_first", True), ("gather_first", False), ("local_carry", True), ("head_parallel", True)):
        net._cp_attn.configure(schedule=sched)
        assert net._cp_fused_qkv() == fused, sched
    monkeypatch.delenv("G3_CP_CONFIG")
    VideoExtendGeneralDIT.enable_context_parallel(net, object())
    assert net._cp_attn.schedule == "local_first"  # the DiT's default does not change
