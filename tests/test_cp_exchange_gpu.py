"""GPU: the head-parallel context-parallel schedule - its two layout kernels (g3_cp_scatter_heads_bf16, g3_cp_gather_heads_bf16), bitwise against
torch indexing; ContextParallelAttention(schedule="head_parallel") on a 1-rank group (a self-exchange through the real all_to_all_single), bitwise
against the single-GPU attention calls it must reduce to; and a DiT denoise step under it == the non-CP step (tools/cp_check.py) with 2 ranks
sharing the GPU over gloo and with 1 rank over RCCL.

Layout cases: rows = 6 (S_local 3, B 2: less than one workgroup) and 1030 (several workgroups, a ragged last one); (H, P, head0, Hg) = a group at the
start of a rank's heads, one in the middle, one rank with all heads, and the cp = 8 split of the 32-head model. The inputs are column views of one
[rows, 3 H 128 + 8] buffer, as the DiT's fused QKV projection leaves them."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NM = "flash_attn_fwd_w4b_nm_kernel<true>"
GUARD = 64  # elements (128 bytes: the guarded tensor stays 16-byte aligned)
SENTINEL = -7.0
LAYOUTS = [(8, 4, 0, 2), (8, 4, 1, 1), (4, 1, 0, 4), (32, 8, 3, 1)]


def _guarded(shape, dev):
    """A contiguous bf16 tensor of `shape` inside a flat sentinel-filled buffer -> (tensor, check) where check() asserts that the guards are intact."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.bfloat16, device=dev)
    def check():
        assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + n:] == SENTINEL).all()), "guard elements were written"
    return flat[GUARD:GUARD + n].view(shape), check


def _qkv(rows, H, dev, seed):
    D = H * 128
    g = torch.Generator(device=dev).manual_seed(seed)
    buf = torch.randn(rows, 3 * D + 8, device=dev, generator=g).to(torch.bfloat16)
    return buf, buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:3 * D]


def _expect_scatter(x, H, P, head0, Hg):
    Hl = H // P
    return torch.stack([x[:, (d * Hl + head0) * 128:(d * Hl + head0 + Hg) * 128] for d in range(P)])


@pytest.mark.parametrize("rows", [6, 1030])
@pytest.mark.parametrize("H,P,head0,Hg", LAYOUTS)
def test_scatter_and_gather_bitwise(rows, H, P, head0, Hg):
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    buf, q, k, v = _qkv(rows, H, dev, seed=rows + H)
    assert q.stride(0) == 3 * H * 128 + 8 and not q.is_contiguous()
    before = buf.clone()
    no_v = (H, P, head0, Hg) == (8, 4, 1, 1)  # one case without v: its output must not be touched (there is none)
    outs, checks = zip(*[_guarded((P, rows, Hg * 128), dev) for _ in range(3)])
    got = ops.cp_scatter_heads(q, k, None if no_v else v, H, P, head0, Hg, out=(outs[0], outs[1], None if no_v else outs[2]))
    torch.cuda.synchronize()
    for x, o, ret, skipped in ((q, outs[0], got[0], False), (k, outs[1], got[1], False), (v, outs[2], got[2], no_v)):
        if skipped:
            assert ret is None and bool((o == SENTINEL).all())
        else:
            assert ret is o and torch.equal(o, _expect_scatter(x, H, P, head0, Hg))
    for c in checks:
        c()
    assert torch.equal(buf, before)
    # gather: the inverse, into a column view of a wider sentinel-filled buffer; every other column and the guards stay
    D, Hl = H * 128, H // P
    wide, check = _guarded((rows, D + 8), dev)
    back = ops.cp_gather_heads(outs[0], wide[:, :D], H, head0)
    torch.cuda.synchronize()
    expect = torch.full((rows, D + 8), SENTINEL, dtype=torch.bfloat16, device=dev)
    for s in range(P):
        c0 = (s * Hl + head0) * 128
        expect[:, c0:c0 + Hg * 128] = q[:, c0:c0 + Hg * 128]  # gather(scatter(x)) restores x in the group's columns
    assert back.data_ptr() == wide.data_ptr() and torch.equal(wide, expect)
    check()


def test_gather_of_all_groups_restores_the_tensor():
    """Every head group of every rank, scattered and gathered back: the whole [rows, H*128] tensor again."""
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    rows, H, P, Hg = 70, 8, 2, 2
    _buf, q, k, v = _qkv(rows, H, dev, seed=5)
    out = torch.full((rows, H * 128), SENTINEL, dtype=torch.bfloat16, device=dev)
    for head0 in range(0, H // P, Hg):
        _, _, vs = ops.cp_scatter_heads(None, None, v, H, P, head0, Hg)
        ops.cp_gather_heads(vs, out, H, head0)
    assert torch.equal(out, v)


def test_refusals_return_err_arg_before_any_launch():
    from gen3c_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    rows, H, P, Hg = 6, 8, 4, 2
    D = H * 128
    buf = torch.zeros(rows, 3 * D + 8, dtype=torch.bfloat16, device=dev)
    ld = buf.stride(0)
    q, k, v = buf.data_ptr(), buf.data_ptr() + 2 * D, buf.data_ptr() + 4 * D
    outs = [torch.full((P, rows, Hg * 128), SENTINEL, dtype=torch.bfloat16, device=dev) for _ in range(3)]
    qo, ko, vo = (o.data_ptr() for o in outs)
    wide = torch.full((rows, D + 8), SENTINEL, dtype=torch.bfloat16, device=dev)

    def scatter(q=q, k=k, v=v, ld=ld, qo=qo, ko=ko, vo=vo, rows=rows, H=H, P=P, head0=0, Hg=Hg):
        return lib.g3_cp_scatter_heads_bf16(q, k, v, ld, qo, ko, vo, rows, H, P, head0, Hg, 0)

    def gather(src=qo, dst=wide.data_ptr(), ld=D + 8, rows=rows, H=H, P=P, head0=0, Hg=Hg):
        return lib.g3_cp_gather_heads_bf16(src, dst, ld, rows, H, P, head0, Hg, 0)

    assert scatter() == _lib.G3_OK and gather() == _lib.G3_OK  # the baseline the refusals below vary
    torch.cuda.synchronize()
    for o in outs:
        o.fill_(SENTINEL)
    wide.fill_(SENTINEL)
    for fn in (scatter, gather):
        assert fn(P=3) == _lib.G3_ERR_ARG  # H % n != 0
        assert fn(head0=1) == _lib.G3_ERR_ARG  # head0 + Hg > H / n
        assert fn(Hg=3) == _lib.G3_ERR_ARG
        assert fn(rows=0) == _lib.G3_ERR_ARG and fn(rows=-4) == _lib.G3_ERR_ARG
        assert fn(ld=D - 8) == _lib.G3_ERR_ARG  # below the width
        assert fn(ld=D + 4) == _lib.G3_ERR_ARG  # not a multiple of 8
        assert "g3_cp_" in _lib.last_error()
    for name in ("q", "k", "v", "qo", "ko", "vo"):  # each pointer 2 bytes off
        assert scatter(**{name: locals()[name] + 2}) == _lib.G3_ERR_ARG, name
    assert gather(src=qo + 2) == _lib.G3_ERR_ARG and gather(dst=wide.data_ptr() + 2) == _lib.G3_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs) and bool((wide == SENTINEL).all()), "a refused call launched"


# ---- the schedule on a 1-rank group: a self-exchange through the real all_to_all_single ---------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank_group():
    import socket
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1)
    yield dist.group.WORLD
    if created:
        dist.destroy_process_group()


def _rms(x):
    x = x.float().view(x.shape[0], -1, 128)
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True))).reshape(x.shape[0], -1)


def _attn_inputs(S, B, H, seed):
    """q, k, v: column views of one [S*B, 3 H 128] buffer; q and k RMS-normalised per head with unit weights, as behind the DiT's norms."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    D = H * 128
    x = torch.randn(S * B, 3 * D, device=dev, generator=g)
    qkv = torch.cat([_rms(x[:, :D]), _rms(x[:, D:2 * D]), x[:, 2 * D:]], dim=1).to(torch.bfloat16)
    return qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]


def _launched(fn):
    from gen3c_amd import ops
    ops.enable_kernel_timers(True)
    try:
        out = fn()
        return out, [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    finally:
        ops.enable_kernel_timers(False)


def test_head_parallel_one_rank_is_the_single_gpu_attention(one_rank_group):
    import math
    from gen3c_amd import _lib, ops, parallel
    S, B, H, G = 2112, 2, 4, 2
    q, k, v = _attn_inputs(S, B, H, seed=3)
    vt = ops.transpose_v(v, S, B, H)
    cpa = parallel.ContextParallelAttention(one_rank_group, head_groups=G, schedule="head_parallel", kernel="w4b")
    cpa.stats = []
    out, launches = _launched(lambda: cpa(q, k, v, S, B, H))
    assert cpa.effective == dict(schedule="head_parallel", kernel="w4b", head_groups=G), cpa.effective
    assert [(m["Sq"], m["Skv"], m["H"]) for m in launches] == [(S, S, H // G)] * G, launches  # one full-length launch per group, nothing else
    assert torch.equal(out, ops.flash_attn(q, k, vt, S, S, B, H, variant=11))
    assert [kind for (kind, _g, _tm) in cpa.stats] == ["wait"] * (4 * G) and sorted(g for (_k, g, _tm) in cpa.stats) == [0] * 4 + [1] * 4
    assert cpa.bytes_gathered == 0  # one rank: nothing comes from another

    # with the caller's logit bound (unit norm weights: sqrt(128), and the margin for the bf16 roundings of q and k) the no-running-max kernel runs
    bound = 128.0 / math.sqrt(128.0) * 1.03
    assert _lib.load().g3_self_attn_kernel_name(S, S, B, H // G, bound, 11).decode() == NM
    out_b, launches = _launched(lambda: cpa(q, k, v, S, B, H, logit_bound=bound))
    assert [m["kernel"] for m in launches] == [NM] * G, launches
    assert torch.equal(out_b, ops.self_attn_bounded(q, k, vt, S, S, B, H, bound, variant=11))
    assert cpa.effective["schedule"] == "head_parallel"


def test_head_parallel_one_rank_ragged_tokens_wave8(one_rank_group):
    from gen3c_amd import ops, parallel
    S, B, H, G = 200, 2, 4, 2
    q, k, v = _attn_inputs(S, B, H, seed=4)
    cpa = parallel.ContextParallelAttention(one_rank_group, head_groups=G, schedule="head_parallel", kernel="wave8")
    cpa.stats = []
    out = cpa(q, k, v, S, B, H)
    assert cpa.effective == dict(schedule="head_parallel", kernel="wave8", head_groups=G), cpa.effective
    assert torch.equal(out, ops.flash_attn(q, k, ops.transpose_v(v, S, B, H), S, S, B, H, variant=4))
    assert len(cpa.stats) == 4 * G


# ---- a DiT denoise step under the schedule == the non-CP step (tools/cp_check.py) ----------------------------------------------------------------
def _free_port() -> str:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


@pytest.mark.parametrize("ranks,backend", [(2, "gloo"), (1, "nccl")])
def test_head_parallel_step_matches_single_rank(ranks, backend):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(ROOT / "tools" / "cp_check.py")]
    env = dict(os.environ, G3_CP_CHECK_SCHEDULES="head_parallel", G3_CP_CHECK_BACKEND=backend)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(ROOT), env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[cp_check] OK" in r.stdout
    # (the ranks' prints may interleave on one line: the pattern is not anchored and stops at the schedule name)
    lines = re.findall(r"rank (\d)/%d: CP \(head_parallel\) vs non-CP denoise step rel_l2=(\S+) max_abs=\S+ effective=([a-z_]+)" % ranks, r.stdout)
    assert sorted(int(rk) for rk, _, _ in lines) == list(range(ranks)), r.stdout[-3000:]
    for rk, rel, eff in lines:
        assert eff == "head_parallel", f"rank {rk} ran {eff}"
        assert float(rel) < 5e-3
