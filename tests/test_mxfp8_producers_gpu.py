"""GPU: the producers that emit MXFP8 straight from their registers (mxfp8_producers="fused"): LayerNorm + AdaLN modulate
(g3_layernorm_modulate_mxfp8, g3_posemb_layernorm_modulate_mxfp8) and the MXFP8 GEMM with MXFP8 output (g3_gemm_mxfp8_nt_mxout).

The claim is bitwise: a fused producer rounds to bf16 where the separate chain (bf16 producer, then g3_quant_mxfp8_bf16) does and runs the same
quantiser arithmetic. Every comparison here is torch.equal on the uint8 views of q and on the scale bytes; there is no tolerance in this file.
"""
import os

import pytest
import torch

from tests._mxfp8_tiny_dit import _inputs, _net, _run  # the tiny DiT, shared with the CP worker process
from tests.mxfp8_ref import quant_mxfp8_ref

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
LN_WAVE_DEFAULT = int(os.environ.get("G3_LN_WAVE_ROWS", "0"))  # what the library starts with (csrc/api.hip)


def _dev():
    return torch.device("cuda:0")


def _u8(q):
    return q.view(torch.uint8)


def _padded_pair(rows, K, dev, guard_rows=0):
    """(q, scales) views [rows, K] / [rows, K/32] inside 0xAA-filled buffers with padded leading dimensions (and guard rows behind)."""
    qb = torch.full((rows + guard_rows, K + 64), 0xAA, dtype=torch.uint8, device=dev)
    sb = torch.full((rows + guard_rows, K // 32 + 4), 0xAA, dtype=torch.uint8, device=dev)
    return qb, sb, (qb[:rows, :K].view(F8), sb[:rows, :K // 32])


def _padding_untouched(qb, sb, rows, K):
    return (bool((qb[:rows, K:] == 0xAA).all()) and bool((sb[:rows, K // 32:] == 0xAA).all()) and bool((qb[rows:] == 0xAA).all())
            and bool((sb[rows:] == 0xAA).all()))


class _ln_wave:
    """The "ln_wave_rows" option for the duration of a block (None: leave it), restored afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from gen3c_amd import ops
        if self.value is not None:
            ops.set_option("ln_wave_rows", self.value)

    def __exit__(self, *exc):
        from gen3c_amd import ops
        if self.value is not None:
            ops.set_option("ln_wave_rows", LN_WAVE_DEFAULT)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. LayerNorm + modulate -> MXFP8
# ---------------------------------------------------------------------------------------------------------------------------------------

def _ln_inputs(rows, B, D, dev, seed):
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.linspace(-20.0, 10.0, rows)).reshape(rows, 1)  # per-row magnitude spread 2^-20 .. 2^10
    x = (torch.randn(rows, D, generator=g) * mag).to(torch.bfloat16).to(dev)
    shift = (0.5 * torch.randn(B, D, generator=g)).to(torch.bfloat16)
    scale = (0.5 * torch.randn(B, D, generator=g)).to(torch.bfloat16)
    scale[:, 32:96] = -1.0  # 1 + scale = 0: the normalised value drops out
    shift[:, 32:64] = 0.0   # block 1: every output exactly 0 -> scale byte 127, zero elements
    shift[:, 64:96] = 0.375  # block 2: a constant block
    return x, shift.to(dev), scale.to(dev)


@pytest.mark.parametrize("rows,B,D,wave", [
    (10, 2, 4096, 1),   # the one-wave-per-row form, last workgroup half empty
    (6, 2, 4096, 0),    # the generic form at the same D
    (5, 1, 256, None),
    (3, 1, 96, None),   # three quads, most threads idle
    (2, 2, 8192, None),  # four chunks per thread
])
def test_layernorm_mxfp8_bitwise_vs_chain_and_cpu_reference(rows, B, D, wave):
    from gen3c_amd import ops
    dev = _dev()
    x, shift, scale = _ln_inputs(rows, B, D, dev, seed=rows * 1000 + D)
    x0 = x.clone()
    with _ln_wave(wave):
        h = ops.layernorm_modulate(x, shift, scale)
        q_ref, s_ref = ops.quant_mxfp8(h)
        qb, sb, out = _padded_pair(rows, D, dev)
        q, s = ops.layernorm_modulate_mxfp8(x, shift, scale, out=out)
        q2, s2 = ops.layernorm_modulate_mxfp8(x, shift, scale)  # allocating form
        torch.cuda.synchronize()
    assert torch.equal(x, x0), "the plain form must not write x"
    assert torch.equal(_u8(q), _u8(q_ref)) and torch.equal(s, s_ref), "fused LayerNorm differs from layernorm_modulate + quant_mxfp8"
    assert torch.equal(_u8(q2), _u8(q_ref)) and torch.equal(s2, s_ref)
    q_cpu, s_cpu = quant_mxfp8_ref(h.cpu())
    assert torch.equal(_u8(q).cpu(), _u8(q_cpu)) and torch.equal(s.cpu(), s_cpu), "fused LayerNorm differs from the CPU reference"
    assert bool((s[:, 1] == 127).all()) and bool((_u8(q)[:, 32:64] == 0).all()), "an all-zero block must give byte 127 and zero elements"
    assert bool((_u8(q)[:, 64:96] == _u8(q)[:, 64:65]).all()), "constant block"
    assert _padding_untouched(qb, sb, rows, D), "wrote outside [rows, D] / [rows, D/32]"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the position-embedding form
# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,tables,wave", [(4096, 1, 1), (4096, 1, 0), (256, 1, None), (256, 3, None)])
def test_posemb_layernorm_mxfp8_bitwise_vs_chain(D, tables, wave):
    from gen3c_amd import ops
    dev = _dev()
    T, Hp, Wp, B = 2, 3, 2, 2
    rows = T * Hp * Wp * B
    x, shift, scale = _ln_inputs(rows, B, D, dev, seed=D + tables)
    g = torch.Generator().manual_seed(D * 7 + tables)
    rnd = lambda *shape: (0.3 * torch.randn(*shape, generator=g)).to(torch.bfloat16).to(dev)
    if tables == 1:  # POS 2: the materialised table
        pe = (rnd(T * Hp * Wp, D), None, None, None)
    else:            # POS 1: the three axis tables + the per-token normaliser
        pe = (rnd(T, D), rnd(Hp, D), rnd(Wp, D), (0.5 + torch.rand(T * Hp * Wp, generator=g)).to(torch.bfloat16).to(dev))
    x_chain, x_fused = x.clone(), x.clone()
    with _ln_wave(wave):
        h = ops.posemb_layernorm_modulate(x_chain, *pe, T, Hp, Wp, B, shift, scale)
        q_ref, s_ref = ops.quant_mxfp8(h)
        qb, sb, out = _padded_pair(rows, D, dev)
        q, s = ops.posemb_layernorm_modulate_mxfp8(x_fused, *pe, T, Hp, Wp, B, shift, scale, out=out)
        torch.cuda.synchronize()
    assert not torch.equal(x_chain, x), "the embedding was not added"
    assert torch.equal(x_fused, x_chain), "x after the fused call differs from what posemb_layernorm_modulate leaves"
    assert torch.equal(_u8(q), _u8(q_ref)) and torch.equal(s, s_ref)
    assert _padding_untouched(qb, sb, rows, D)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. MXFP8 GEMM with MXFP8 output
# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("M,N,K", [
    (64, 256, 128),    # one tile, mostly dead rows
    (300, 512, 256),   # a row tail inside the second tile row
    (513, 1024, 256),
])
def test_gemm_mxout_bitwise_vs_gemm_then_quant(M, N, K, epi):
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(M + N + K + epi)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (0.1 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    w[32:64] = 0  # a whole output block of zeros (GELU(0) = 0)
    w2 = (0.05 * torch.randn(256, N, generator=g)).to(torch.bfloat16).to(dev)
    aq, as_ = ops.quant_mxfp8(a)
    wq, ws = ops.quant_mxfp8(w.to(dev))
    w2q, w2s = ops.quant_mxfp8(w2)

    c = ops.gemm_mxfp8_nt(aq, as_, wq, ws, epilogue=epi)
    q_ref, s_ref = ops.quant_mxfp8(c)
    qb, sb, out = _padded_pair(M, N, dev, guard_rows=8)
    q, s = ops.gemm_mxfp8_nt(aq, as_, wq, ws, epilogue=epi, out_mx=out)
    q2, s2 = ops.gemm_mxfp8_nt(aq, as_, wq, ws, epilogue=epi, out_mx=True)
    y_ref = ops.gemm_mxfp8_nt(q_ref, s_ref, w2q, w2s)
    y = ops.gemm_mxfp8_nt(q, s, w2q, w2s)  # as w2 consumes w1's output: the padded pair goes straight into the next GEMM
    torch.cuda.synchronize()
    assert q.dtype == F8 and s.dtype == torch.uint8 and tuple(q2.shape) == (M, N) and tuple(s2.shape) == (M, N // 32)
    assert torch.equal(_u8(q), _u8(q_ref)) and torch.equal(s, s_ref), "GEMM with MXFP8 output differs from GEMM + quant_mxfp8"
    assert torch.equal(_u8(q2), _u8(q_ref)) and torch.equal(s2, s_ref)
    assert bool((s[:, 1] == 127).all()) and bool((_u8(q)[:, 32:64] == 0).all()), "an all-zero block must give byte 127 and zero elements"
    assert _padding_untouched(qb, sb, M, N), "wrote past row M or outside [M, N] / [M, N/32]"
    assert torch.equal(y, y_ref), "the second GEMM on the fused pair differs"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. refusals launch nothing
# ---------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from gen3c_amd import _lib, ops
    lib = _lib.load()
    dev = _dev()
    stream = torch.cuda.current_stream().cuda_stream
    ARG = _lib.G3_ERR_ARG

    # ---- the two LayerNorm entry points
    rows, D = 8, 256
    T, Hp, Wp, B = 2, 2, 2, 1
    x = torch.full((rows, D + 64), 3.0, dtype=torch.bfloat16, device=dev)
    mod = torch.zeros(1, D, dtype=torch.bfloat16, device=dev)
    pe = torch.ones(rows, D, dtype=torch.bfloat16, device=dev)
    q = torch.full((rows, D + 64), 0xAA, dtype=torch.uint8, device=dev)
    s = torch.full((rows, D // 32 + 4), 0xAA, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()

    def ln(x_p=None, ldx=D + 64, sh_p=None, ldmod=D, mod_rows=1, q_p=None, ldq=D + 64, s_p=None, lds=D // 32 + 4, n_rows=rows, d=D):
        null = lambda v, t: 0 if v == 0 else (v or p(t))
        return lib.g3_layernorm_modulate_mxfp8(null(x_p, x), ldx, null(sh_p, mod), p(mod), ldmod, mod_rows, null(q_p, q), ldq, null(s_p, s), lds,
                                               n_rows, d, 1e-6, stream)

    def pos(x_p=None, ldx=D + 64, pe_p=None, pe_h=0, t=T, ldmod=D, mod_rows=1, q_p=None, ldq=D + 64, s_p=None, lds=D // 32 + 4, d=D):
        null = lambda v, tt: 0 if v == 0 else (v or p(tt))
        return lib.g3_posemb_layernorm_modulate_mxfp8(null(x_p, x), ldx, null(pe_p, pe), pe_h, 0, 0, t, Hp, Wp, B, p(mod), p(mod), ldmod, mod_rows,
                                                      null(q_p, q), ldq, null(s_p, s), lds, d, 1e-6, stream)

    shared = {
        "null q": dict(q_p=0), "null scales": dict(s_p=0), "null x": dict(x_p=0),
        "D not a multiple of 32": dict(d=D - 8), "D not a multiple of 8": dict(d=D - 4), "D too large": dict(d=8192 + 32, ldq=8192 + 64, lds=300),
        "ldx not a multiple of 8": dict(ldx=D + 4), "ldmod not a multiple of 8": dict(ldmod=D + 4), "no modulation rows": dict(mod_rows=0),
        "ldq < D": dict(ldq=D - 8), "ldq not a multiple of 8": dict(ldq=D + 4), "lds < D/32": dict(lds=D // 32 - 1),
        "q not 8-byte aligned": dict(q_p=p(q) + 4),
    }
    for what, kw in shared.items():
        assert ln(**kw) == ARG, f"g3_layernorm_modulate_mxfp8, {what}"
        assert _lib.last_error().startswith("g3_layernorm_modulate_mxfp8"), what
        assert pos(**kw) == ARG, f"g3_posemb_layernorm_modulate_mxfp8, {what}"
        assert _lib.last_error().startswith("g3_posemb_layernorm_modulate_mxfp8"), what
    assert ln(sh_p=0) == ARG and ln(n_rows=0) == ARG
    assert pos(pe_p=0) == ARG and pos(t=0) == ARG
    assert pos(pe_h=p(pe)) == ARG, "axis tables without all three + the normaliser"
    with pytest.raises(_lib.Gen3cHipError):  # through the Python front end
        ops.layernorm_modulate_mxfp8(x[:, :D - 8], mod[:, :D - 8], mod[:, :D - 8], out=(q[:, :D - 8].view(F8), s[:, :7]))
    torch.cuda.synchronize()
    assert bool((q == 0xAA).all()) and bool((s == 0xAA).all()) and bool((x == 3.0).all()), "a refused LayerNorm call wrote something"
    assert ln() == _lib.G3_OK and pos() == _lib.G3_OK  # the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert bool((q[:, D:] == 0xAA).all()) and not bool((q[:, :D] == 0xAA).all())

    # ---- the GEMM with MXFP8 output
    M, N, K = 256, 512, 512
    aq = torch.zeros(M, K + 64, dtype=torch.uint8, device=dev)
    wq = torch.zeros(N + 256, K + 64, dtype=torch.uint8, device=dev)
    sa = torch.full((M, 64), 127, dtype=torch.uint8, device=dev)
    sw = torch.full((N + 256, 64), 127, dtype=torch.uint8, device=dev)
    qo = torch.full((M, N + 64), 0xAA, dtype=torch.uint8, device=dev)
    so = torch.full((M, N // 32 + 4), 0xAA, dtype=torch.uint8, device=dev)

    def gemm(aq_p=None, lda=K + 64, as_p=None, ldas=64, wq_p=None, ldw=K + 64, ws_p=None, ldws=64, q_p=None, ldq=N + 64, s_p=None, lds=N // 32 + 4,
             m=M, n=N, k=K, epi=0):
        null = lambda v, t: 0 if v == 0 else (v or p(t))
        return lib.g3_gemm_mxfp8_nt_mxout(null(aq_p, aq), lda, null(as_p, sa), ldas, null(wq_p, wq), ldw, null(ws_p, sw), ldws, null(q_p, qo), ldq,
                                          null(s_p, so), lds, m, n, k, epi, stream)

    cases = {
        # what g3_gemm_mxfp8_nt refuses of the operands
        "null activations": dict(aq_p=0), "null activation scales": dict(as_p=0), "null weights": dict(wq_p=0), "null weight scales": dict(ws_p=0),
        "M = 0": dict(m=0), "K not a multiple of 128": dict(k=K + 32), "N not a multiple of 256": dict(n=N + 128),
        "misaligned activations": dict(aq_p=p(aq) + 8), "misaligned weights": dict(wq_p=p(wq) + 4), "misaligned scales": dict(as_p=p(sa) + 2),
        "short activation scale stride": dict(ldas=K // 32 - 4), "short weight scale stride": dict(ldws=K // 32 - 4), "odd scale stride": dict(ldas=17),
        "short lda": dict(lda=K - 16), "lda not a multiple of 16": dict(lda=K + 8), "short ldw": dict(ldw=K - 16),
        # the MXFP8 output
        "null q_out": dict(q_p=0), "null s_out": dict(s_p=0), "ldq < N": dict(ldq=N - 8), "ldq not a multiple of 8": dict(ldq=N + 4),
        "lds < N/32": dict(lds=N // 32 - 1), "misaligned q_out": dict(q_p=p(qo) + 4),
        "gated residual": dict(epi=2), "bias epilogue": dict(epi=3), "negative epilogue": dict(epi=-1), "the MX_OUT flag as an epilogue": dict(epi=256),
    }
    for what, kw in cases.items():
        assert gemm(**kw) == ARG, f"g3_gemm_mxfp8_nt_mxout, {what}"
        assert _lib.last_error().startswith("g3_gemm_mxfp8_nt_mxout"), what
    with pytest.raises(_lib.Gen3cHipError):
        ops.gemm_mxfp8_nt(aq[:, :K].view(F8), sa[:, :K // 32], wq[:N, :K].view(F8), sw[:N, :K // 32], epilogue=ops.EPI_GATED_RESIDUAL, out_mx=True)
    torch.cuda.synchronize()
    assert bool((qo == 0xAA).all()) and bool((so == 0xAA).all()), "a refused GEMM call wrote its output"
    assert gemm() == _lib.G3_OK
    torch.cuda.synchronize()
    assert bool((qo[:, :N] == 0).all()) and bool((so[:, :N // 32] == 127).all()) and bool((qo[:, N:] == 0xAA).all()) and bool((so[:, N // 32:] == 0xAA).all())
    assert [lib.g3_gemm_mxfp8_mxout_kernel_name(M, N, K, e) for e in (0, 1)] == [b"gemm_mxfp8_nt_kernel<256>", b"gemm_mxfp8_nt_kernel<257>"]
    assert lib.g3_gemm_mxfp8_mxout_kernel_name(M, N, K, 2) is None and lib.g3_gemm_mxfp8_mxout_kernel_name(M, N + 128, K, 0) is None


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the DiT (the tiny net and inputs of tests/test_mxfp8_dit_gpu.py, re-stated in tests/_mxfp8_tiny_dit.py)
# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cross_q_norm_in_attention", [1, 0])
@pytest.mark.parametrize("B", [1, 2])
def test_dit_fused_equals_separate(B, cross_q_norm_in_attention, monkeypatch):
    from gen3c_amd import dit
    monkeypatch.setattr(dit, "_CROSS_Q_NORM_IN_ATTENTION", cross_q_norm_in_attention)
    dev = _dev()
    inp = _inputs(B)
    net = _net(dev, "mxfp8")
    assert net.mxfp8_producers == "separate"
    y_sep = _run(net, inp, dev)
    packed = net._packed
    net.set_mxfp8_producers("fused")
    y_fused = _run(net, inp, dev)
    assert net._packed is packed, "switching the producers dropped the packed weights"
    y_ctor = _run(_net(dev, "mxfp8", producers="fused"), inp, dev)
    assert torch.isfinite(y_sep).all()
    assert torch.equal(y_fused, y_sep), "mxfp8_producers='fused' changed the output"
    assert torch.equal(y_ctor, y_sep)


def test_dit_fused_quantiser_launch_counts_and_bf16_inert():
    from gen3c_amd import ops
    dev = _dev()
    inp = _inputs()
    calls = []
    real_q = ops.quant_mxfp8
    net = _net(dev, "mxfp8")
    y_sep = _run(net, inp, dev)  # packs (and quantises) the weights: not counted below
    ops.quant_mxfp8 = lambda *a, **k: calls.append("quant") or real_q(*a, **k)
    try:
        assert torch.equal(_run(net, inp, dev), y_sep)
        assert len(calls) == 12, f"separate: {len(calls)} activation quantiser launches, expected 6 per block"
        calls.clear()
        net.set_mxfp8_producers("fused")
        assert torch.equal(_run(net, inp, dev), y_sep)
        assert len(calls) == 4, f"fused: {len(calls)} activation quantiser launches, expected the two attention outputs per block"
        calls.clear()
        y_bf = _run(_net(dev), inp, dev)
        y_bf_fused = _run(_net(dev, "bf16", producers="fused"), inp, dev)
        assert calls == [], "bf16 + fused called the quantiser"
    finally:
        ops.quant_mxfp8 = real_q
    assert torch.equal(y_bf_fused, y_bf), "mxfp8_producers must have no effect under bf16"
    assert not torch.equal(y_bf, y_sep)


def test_dit_fused_follows_in_place_weight_edit():
    dev = _dev()
    inp = _inputs()
    with torch.no_grad():
        net = _net(dev, "mxfp8", producers="fused")
        y0 = _run(net, inp, dev)
        dict(net.named_parameters())["blocks.block0.blocks.2.block.layer1.weight"].mul_(-0.5)
        y1 = _run(net, inp, dev)
        fresh = _net(dev, "mxfp8")  # separate producers, built with the edited weights
        fresh.load_state_dict(net.state_dict())
        y2 = _run(fresh, inp, dev)
    assert not torch.equal(y0, y1), "the edit was not followed"
    assert torch.equal(y1, y2), "edited fused net differs from a separate-producers net built with the edited weights"


def test_dit_fused_context_parallel_one_rank_equals_single_rank():
    """tests/_cp_producers_worker.py under torchrun with one rank: the gather_first and the local_first branch of forward() with fused producers,
    bitwise against the single-rank output and against the separate arm."""
    import subprocess
    import sys
    from pathlib import Path
    import socket
    root = Path(__file__).resolve().parent.parent
    with socket.socket() as sock:  # a free rendezvous port: fixed ones collide on shared machines
        sock.bind(("127.0.0.1", 0))
        port = str(sock.getsockname()[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", port, str(root / "tests" / "_cp_producers_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(root), env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[cp_producers] OK" in r.stdout
