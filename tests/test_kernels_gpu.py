"""GPU parity tests of the individual HIP kernels (through the C ABI) against fp32 references.

Tolerances (stated per test): operands are bf16, accumulation fp32, outputs rounded once to bf16 - so the expected
error vs an fp32 evaluation of the same bf16 operands is ~2^-9 relative per output (one bf16 rounding) plus
accumulation-order noise.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _rel_l2(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def test_gemm_pingpong_bitwise_equals_classic_and_is_race_free():
    """The ping-pong kernels accumulate every output element over K in the same order as the one-barrier-per-tile kernel, so
    the three must agree BITWISE; repeated launches must reproduce themselves (a staging race - an LDS half-tile read before
    its DMA landed or restaged before its last read - shows up as a run-to-run or kernel-to-kernel difference)."""
    from gen3c_amd import ops
    dev = _dev()
    for (M, N, K, epi) in [(7040, 4096, 4096, 2), (2048, 12288, 4096, 0), (1000, 1024, 16384, 1), (513, 264, 192, 0), (256, 256, 64, 3)]:
        g = torch.Generator(device=dev).manual_seed(M + N + K)
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
        gate = torch.randn(1, N, device=dev, generator=g).to(torch.bfloat16)
        res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
        kw = dict(gate=gate, residual=res) if epi == 2 else (dict(gate=gate) if epi == 3 else {})
        outs = {}
        for variant in (0, 1, 2, 3):  # 3 = one wave per SIMD (gemm_w4.hpp); falls back to 2 where it does not apply (K < 128)
            ops.set_option("gemm_pingpong", variant)
            first = ops.gemm_nt(a, w, epilogue=epi, **kw).clone()
            for _ in range(8):
                again = ops.gemm_nt(a, w, epilogue=epi, **kw)
                assert torch.equal(first, again), f"variant {variant} not reproducible at {M}x{N}x{K}"
            outs[variant] = first
        ops.set_option("gemm_pingpong", 3)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.equal(outs[0], outs[3]), f"ping-pong / w4 != classic at {M}x{N}x{K} epi {epi}"


_GEMM_OPTION_DEFAULTS = {"gemm_pingpong": 3, "gemm_regstage": 0, "gemm_unpinned": 1, "gemm_persistent": 0, "gemm_tokens_first": 2}
_GEMM_ROW_FAMILIES = [  # (instantiation with {e} for the epilogue, the options that select it, the smallest shape that reaches it, its epilogues)
    ("gemm_bf16_nt_kernel<{e}, true, false, false>", {"gemm_pingpong": 0}, "small", range(5)),
    ("gemm_bf16_nt_kernel<{e}, true, false, true>", {"gemm_pingpong": 0, "gemm_unpinned": 0}, "small", range(5)),
    ("gemm_bf16_nt_kernel<{e}, false, false, false>", {"gemm_regstage": 1}, "small", range(5)),
    ("gemm_bf16_nt_kernel<{e}, false, false, true>", {"gemm_regstage": 1, "gemm_unpinned": 0}, "small", range(5)),
    ("gemm_bf16_nt_pp_kernel<{e}, 2, false>", {"gemm_pingpong": 2}, "small", range(5)),
    ("gemm_bf16_nt_pp_kernel<{e}, 4, false>", {"gemm_pingpong": 1}, "small", range(5)),
    ("gemm_bf16_nt_w4_kernel<{e}, false>", {}, "k128", range(5)),
    ("gemm_bf16_nt_w4_kernel<{e}, true>", {"gemm_persistent": 1}, "two_tiles_k128", range(5)),
    ("gemm_bf16_nt_w4e_kernel<{e}, false>", {"gemm_tokens_first": 0}, "two_tiles_k2432", range(3)),
    ("gemm_bf16_nt_w4e_kernel<{e}, true>", {"gemm_tokens_first": 1}, "two_tiles_k2432", range(3)),
]
_gemm_row_cache = {}


def _gemm_row_operands(shape, epi):
    """Operands of a shape (made once) and the output of the gemm_pingpong = 0 kernel on them per epilogue (computed once, never written again)."""
    from gen3c_amd import _lib, ops
    dev = _dev()
    if shape not in _gemm_row_cache:
        cus = C.c_int(0)
        _lib.check(_lib.load().g3_device_info(0, C.byref(cus), None, None, 0), "g3_device_info")
        m_two = 256 * -(-2 * (cus.value // 8 * 8) // 16)  # with N = 4096 (16 tiles): at least two tiles for each of the persistent grid's workgroups
        M, N, K = {"small": (256, 256, 64), "k128": (256, 256, 128), "two_tiles_k128": (m_two, 4096, 128), "two_tiles_k2432": (m_two, 4096, 2432)}[shape]
        g = torch.Generator(device=dev).manual_seed(M + N + K)
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
        _gemm_row_cache[shape] = (a, w, torch.randn(1, N, device=dev, generator=g).to(torch.bfloat16), torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16))
    a, w, gate, res = _gemm_row_cache[shape]
    kw = dict(gate=gate, residual=res) if epi in (2, 4) else (dict(gate=gate) if epi == 3 else {})
    if (shape, epi) not in _gemm_row_cache:
        ops.set_option("gemm_pingpong", 0)
        try:
            _gemm_row_cache[shape, epi] = ops.gemm_nt(a, w, epilogue=epi, **kw)
            torch.cuda.synchronize()
        finally:
            ops.set_option("gemm_pingpong", 3)
    return a, w, kw, _gemm_row_cache[shape, epi]


@pytest.mark.parametrize("name,options,shape,epi", [(n.format(e=e), o, s, e) for n, o, s, epis in _GEMM_ROW_FAMILIES for e in epis])
def test_gemm_launcher_launches_the_row_the_plan_names(name, options, shape, epi):
    """One case per kernel-table row of g3_gemm_bf16_nt, at the smallest shape that reaches the row: the dry run names that row for exactly the call made,
    the call runs, and the output is BITWISE that of the gemm_pingpong = 0 kernel on the same operands (every GEMM kernel accumulates over K in one order
    and rounds at the same points: the bar of test_gemm_pingpong_bitwise_equals_classic_and_is_race_free and test_gemm_deferred_epilogue_kernel)."""
    from gen3c_amd import _lib, ops
    lib = _lib.load()
    a, w, kw, ref = _gemm_row_operands(shape, epi)
    (M, K), N = a.shape, w.shape[0]
    gate, res = kw.get("gate"), kw.get("residual")
    out = torch.empty_like(ref)
    call = _lib.GemmCall(entry=0, A=a.data_ptr(), lda=K, W=w.data_ptr(), ldw=K, C=out.data_ptr(), ldc=N, M=M, N=N, K=K, epilogue=epi,
                         gate=gate.data_ptr() if gate is not None else 0, gate_rows=1, ldg=N, residual=res.data_ptr() if res is not None else 0, ldr=N)
    try:
        for k, v in options.items():
            ops.set_option(k, v)
        planned = lib.g3_gemm_plan_bf16(C.byref(call), 0, None, None)
        assert planned is not None and planned.decode() == name, (planned, _lib.last_error())
        ops.gemm_nt(a, w, out=out, epilogue=epi, **kw)
        torch.cuda.synchronize()
    finally:
        for k, v in _GEMM_OPTION_DEFAULTS.items():
            ops.set_option(k, v)
    assert torch.equal(out, ref), f"{name} != the gemm_pingpong = 0 kernel on {int((out != ref).sum())} of {M * N} elements"


@pytest.mark.parametrize("K,fused", [(128, True), (64, False)])
def test_gemm_qk_entry_launches_what_the_plan_says(K, fused):
    """g3_gemm_qk_norm_rope_bf16 on both sides of its kernel choice: K = 128 runs the norm / RoPE (+ V^T) epilogue of the one-wave kernel and nothing else,
    K = 64 the plain GEMM and the standalone norm / RoPE and transpose passes - as the dry run says; both against the unfused chain, at the bar of
    test_gemm_qk_norm_rope_epilogue_matches_unfused (the fallback IS that chain: bitwise)."""
    from gen3c_amd import _lib, ops
    dev = _dev()
    lib = _lib.load()
    S, B, D = 300, 2, 256
    g = torch.Generator(device=dev).manual_seed(S + K)
    a = torch.randn(S * B, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(3 * D, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    wq, wk = [(torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16) for _ in range(2)]
    ang = torch.randn(S, 128, device=dev, generator=g) * 3
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    vt = torch.zeros((B, D // 128, 128, ops.ceil_to(S, 64)), dtype=torch.bfloat16, device=dev)
    out = torch.full((S * B, 3 * D), 7.0, dtype=torch.bfloat16, device=dev)
    call = _lib.GemmCall(entry=1, A=a.data_ptr(), lda=K, W=w.data_ptr(), ldw=K, C=out.data_ptr(), ldc=3 * D, M=S * B, N=3 * D, K=K, n_q=D, n_k=D,
                         norm_q=wq.data_ptr(), norm_k=wk.data_ptr(), cos_table=cos.data_ptr(), sin_table=sin.data_ptr(), B=B, eps=1e-6, vt=vt.data_ptr(),
                         vt_ld=vt.shape[-1])
    grid, follow = C.c_int(0), C.c_uint(99)
    planned = lib.g3_gemm_plan_bf16(C.byref(call), 0, C.byref(grid), C.byref(follow))
    want = ("gemm_bf16_nt_w4_kernel<5, false>", 0) if fused else ("gemm_bf16_nt_pp_kernel<0, 2, false>", 1 | 2 | 4)  # THEN_NORM_Q | THEN_NORM_K | THEN_VT
    assert planned is not None and (planned.decode(), follow.value, grid.value) == (*want, 3 * 3), (planned, follow.value, grid.value, _lib.last_error())
    ops.gemm_qk_norm_rope(a, w, D, D, wq, wk, cos, sin, S, B, out=out, vt=vt)
    ref = ops.gemm_nt(a, w)
    ops.qk_rmsnorm_rope(ref[:, :D], wq, cos, sin, S, B, D // 128, out=ref[:, :D])
    ops.qk_rmsnorm_rope(ref[:, D:2 * D], wk, cos, sin, S, B, D // 128, out=ref[:, D:2 * D])
    torch.cuda.synchronize()
    assert torch.equal(vt, ops.transpose_v(ref[:, 2 * D:], S, B, D // 128))
    if fused:
        assert bool((out[:, 2 * D:] == 7.0).all()), "v columns of C must stay unwritten where the epilogue writes V^T"
        got, exp = out[:, :2 * D], ref[:, :2 * D]
        same, diff = float((got == exp).float().mean()), float((got.float() - exp.float()).abs().max())
        assert same > 0.995 and diff <= 2.0 ** -5 * float(exp.float().abs().max())  # at most one bf16 ulp, on a few elements
    else:
        assert torch.equal(out, ref)


def _report(name, got, ref):
    err = (got.float() - ref.float()).abs()
    print(f"[{name}] rel_l2={_rel_l2(got, ref):.3e} max_abs={float(err.max()):.3e} ref_absmax={float(ref.abs().max()):.3e}")


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (512, 768, 256), (300, 260, 136), (1000, 64, 328), (56, 1024, 4096),
                                   (2048, 4096, 1024), (300, 520, 128), (257, 264, 192), (640, 256, 320)])
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
@pytest.mark.parametrize("regstage", [0, 1, 2, 3, 4, 5])
def test_gemm_nt(M, N, K, epi, regstage):
    from gen3c_amd import ops
    dev = _dev()
    # regstage: 0 = LDS-DMA staging (default), 1 = register staging, 2 / 3 = ping-pong kernel with 4 / 2 phases per K tile
    if regstage >= 1 and K % 64 != 0:
        pytest.skip("K % 64 != 0 always takes the register-staged path")
    # 4 = the default kernel with the direct 8-byte-per-lane epilogue instead of the LDS-transposed full-line one
    ops.set_option("gemm_wide_store", 0 if regstage == 4 else 1)
    # 5 = the one-wave-per-SIMD kernel (gemm_w4.hpp; K >= 128, else the ping-pong kernel runs)
    label = regstage
    if regstage == 4:
        regstage = 3
    ops.set_option("gemm_regstage", 1 if regstage == 1 else 0)
    ops.set_option("gemm_pingpong", 3 if regstage == 5 else (regstage - 1 if regstage >= 2 else 0))
    g = torch.Generator(device=dev).manual_seed(M * 7 + N * 3 + K + epi)
    a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(1, N, device=dev, generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    ref = a.float() @ w.float().t()
    if epi == 1:
        ref = torch.nn.functional.gelu(ref)
        out = ops.gemm_nt(a, w, epilogue=ops.EPI_GELU)
    elif epi == 2:
        ref = res.float() + gate.float() * ref
        out = ops.gemm_nt(a, w, epilogue=ops.EPI_GATED_RESIDUAL, gate=gate, residual=res)
    elif epi == 3:
        ref = ref + gate.float()
        out = ops.gemm_nt(a, w, epilogue=ops.EPI_BIAS, gate=gate)
    else:
        out = ops.gemm_nt(a, w)
    torch.cuda.synchronize()
    ops.set_option("gemm_regstage", 0)
    ops.set_option("gemm_pingpong", 3)
    ops.set_option("gemm_wide_store", 1)
    _report(f"gemm {M}x{N}x{K} epi{epi} regstage{label}", out, ref)
    # one bf16 rounding of the output (2^-8 relative worst case) + fp32 accumulation noise
    torch.testing.assert_close(out.float(), ref, rtol=1.0 / 128, atol=2e-2)
    assert _rel_l2(out, ref) < 4e-3


@pytest.mark.parametrize("S,B,H,K,mode", [(512, 1, 4, 512, "qkv"), (300, 2, 2, 256, "qkv"), (1000, 1, 2, 1024, "kv"), (640, 1, 3, 384, "q"), (256, 2, 2, 256, "q_norope"),
                                          (7040, 1, 32, 4096, "qkv"), (333, 4, 2, 256, "qkv"), (200, 3, 2, 256, "kv"), (3520, 2, 32, 4096, "qkv")])
def test_gemm_qk_norm_rope_epilogue_matches_unfused(S, B, H, K, mode):
    """g3_gemm_qk_norm_rope_bf16 (RMSNorm + RoPE in the projection's epilogue, gemm_w4.hpp) against the same projection followed by the
    standalone qk_rmsnorm_rope kernel: identical rounding points; the only difference is the fp32 summation order of the 128 squares."""
    from gen3c_amd import ops
    dev = _dev()
    D = H * 128
    g = torch.Generator(device=dev).manual_seed(S + K + H)
    a = torch.randn(S * B, K, device=dev, generator=g).to(torch.bfloat16)
    n_q, n_k, n_v = {"qkv": (D, D, D), "kv": (0, D, D), "q": (D, 0, 0), "q_norope": (D, 0, 0)}[mode]
    N = n_q + n_k + n_v
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    wq = (torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    wk = (torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    cos = sin = None
    if mode != "q_norope":
        ang = torch.randn(S, 128, device=dev, generator=g) * 3
        cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    fused = ops.gemm_qk_norm_rope(a, w, n_q, n_k, wq if n_q else None, wk if n_k else None, cos, sin, S, B)
    if n_v:  # the same call with a V^T destination: v heads transposed into it (zero tail kept), their columns of `out` left alone
        vt = torch.zeros((B, n_v // 128, 128, ops.ceil_to(S, 64)), dtype=torch.bfloat16, device=dev)
        out2 = torch.full((S * B, N), 7.0, dtype=torch.bfloat16, device=dev)
        ops.gemm_qk_norm_rope(a, w, n_q, n_k, wq if n_q else None, wk if n_k else None, cos, sin, S, B, out=out2, vt=vt)
        torch.cuda.synchronize()
        assert torch.equal(out2[:, :n_q + n_k], fused[:, :n_q + n_k])
        assert torch.equal(vt, ops.transpose_v(fused[:, n_q + n_k:], S, B, n_v // 128)), "V^T written by the epilogue != transpose of the plain v columns"
        if K >= 128 and B in (1, 2, 4):
            assert bool((out2[:, n_q + n_k:] == 7.0).all()), "v columns of C must stay unwritten when V^T is requested"
    ref = ops.gemm_nt(a, w)
    if n_q:
        ops.qk_rmsnorm_rope(ref[:, :n_q], wq, cos, sin, S, B, n_q // 128, out=ref[:, :n_q])
    if n_k:
        ops.qk_rmsnorm_rope(ref[:, n_q:n_q + n_k], wk, cos, sin, S, B, n_k // 128, out=ref[:, n_q:n_q + n_k])
    torch.cuda.synchronize()
    if n_v:
        assert torch.equal(fused[:, n_q + n_k:], ref[:, n_q + n_k:]), "plain (v) features must be untouched"
    same = float((fused == ref).float().mean())
    diff = float((fused.float() - ref.float()).abs().max())
    print(f"[gemm_qk_norm_rope {mode} S={S} B={B} H={H} K={K}] identical {same * 100:.3f} % of elements, max abs diff {diff:.3e}")
    assert same > 0.995 and diff <= 2.0 ** -5 * float(ref.float().abs().max())  # at most one bf16 ulp, on a few elements


def test_gemm_inplace_residual_and_gate_rows():
    from gen3c_amd import ops
    dev = _dev()
    B, S, N, K = 2, 200, 512, 256
    g = torch.Generator(device=dev).manual_seed(5)
    a = torch.randn(S * B, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(B, 3 * N, device=dev, generator=g).to(torch.bfloat16)[:, N:2 * N]  # strided rows
    x = torch.randn(S * B, N, device=dev, generator=g).to(torch.bfloat16)
    ref = x.float() + gate.float().repeat(S, 1) * (a.float() @ w.float().t())
    ops.gemm_nt(a, w, out=x, epilogue=ops.EPI_GATED_RESIDUAL, gate=gate, residual=x)
    torch.cuda.synchronize()
    _report("gemm inplace", x, ref)
    torch.testing.assert_close(x.float(), ref, rtol=1.0 / 128, atol=2e-2)


def _attn_ref(q, k, v, Sq, Skv, B, H):
    qf = q.float().view(Sq, B, H, 128).permute(1, 2, 0, 3)
    kf = k.float().view(Skv, B, H, 128).permute(1, 2, 0, 3)
    vf = v.float().view(Skv, B, H, 128).permute(1, 2, 0, 3)
    p = torch.softmax(qf @ kf.transpose(-1, -2) / math.sqrt(128), dim=-1)
    return (p @ vf).permute(2, 0, 1, 3).reshape(Sq * B, H * 128)


@pytest.fixture(params=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], ids=["attn_v1", "attn_v2", "attn_v3", "attn_v3fold_long", "attn_v3fold_all", "attn_mw_default", "attn_mw_fold_all", "attn_mw_nofold_all", "attn_w4", "attn_w4b", "attn_w4b_xb"])
def attn_variant(request):
    from gen3c_amd import ops
    ops.set_option("attn_variant", request.param)
    yield request.param
    ops.set_option("attn_variant", 0)


@pytest.mark.parametrize("Sq,Skv,B,H", [(256, 256, 1, 1), (512, 512, 1, 2), (300, 200, 1, 2), (96, 40, 2, 3), (1024, 512, 1, 4),
                                         (2048, 2048, 1, 2), (64, 64, 1, 1), (64, 65, 1, 1), (100, 128, 1, 1), (70, 129, 1, 1),
                                         (512, 4160, 1, 1), (128, 192, 1, 1), (128, 250, 1, 1), (128, 320, 1, 2), (64, 449, 1, 1),
                                         # self-attention shapes, Sq = Skv odd (the token counts of tests/test_dit_shapes_gpu.py): below one tile, ragged, past 2048
                                         (25, 25, 1, 1), (189, 189, 2, 2), (2209, 2209, 2, 2)])
def test_flash_attn(Sq, Skv, B, H, attn_variant):
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(Sq + Skv + B + H)
    q = torch.randn(Sq * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    vt = ops.transpose_v(v, Skv, B, H)
    # check the re-layout itself, including the zero tail
    vt_ref = torch.zeros_like(vt)
    vt_ref[..., :Skv] = v.view(Skv, B, H, 128).permute(1, 2, 3, 0)
    torch.cuda.synchronize()
    assert torch.equal(vt, vt_ref), "transpose_v mismatch"
    out = ops.flash_attn(q, k, vt, Sq, Skv, B, H)
    torch.cuda.synchronize()
    ref = _attn_ref(q, k, v, Sq, Skv, B, H)
    _report(f"attn {Sq}x{Skv} B{B} H{H}", out, ref)
    # P is rounded to bf16 before PV (as in flash-attention / TE), output rounded once: ~1e-2 worst-case absolute on O(1) values
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)
    assert _rel_l2(out, ref) < 1e-2


def test_flash_attn_online_softmax_rescale(attn_variant):
    """A late key with a huge score forces the running-max rescale path (cdna guide rule 26); moderate growth
    (< the deferred-rescale threshold of the pipelined kernel) exercises the no-rescale path with P > 1."""
    from gen3c_amd import ops
    dev = _dev()
    Sq, Skv, B, H = 64, 320, 1, 1
    g = torch.Generator(device=dev).manual_seed(11)
    q = torch.randn(Sq, 128, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(Skv, 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(Skv, 128, device=dev, generator=g).to(torch.bfloat16)
    k[200] = (q[5].float() * 3.0).to(torch.bfloat16)   # spike for query 5 in the 4th tile
    k[300] = (q[17].float() * 6.0).to(torch.bfloat16)  # and for query 17 in the 5th
    k[130] = (q[40].float() * 0.5).to(torch.bfloat16)  # score ~ +5.6 (log2 domain ~ +8): around the defer threshold
    k[131] = (q[41].float() * 0.3).to(torch.bfloat16)  # below the threshold: stays on the deferred path
    vt = ops.transpose_v(v, Skv, B, H)
    out = ops.flash_attn(q, k, vt, Sq, Skv, B, H)
    torch.cuda.synchronize()
    ref = _attn_ref(q, k, v, Sq, Skv, B, H)
    _report("attn rescale", out, ref)
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)


def test_flash_attn_strided_views_and_zero_context_rows(attn_variant):
    """q/k/v as column views of a fused projection output; zero K/V rows (padded T5 tokens) stay unmasked."""
    from gen3c_amd import ops
    dev = _dev()
    Sq, Skv, B, H = 192, 128, 1, 2
    D = H * 128
    g = torch.Generator(device=dev).manual_seed(3)
    qkv = torch.randn(Sq, 3 * D, device=dev, generator=g).to(torch.bfloat16)
    kv = torch.randn(Skv, 2 * D, device=dev, generator=g).to(torch.bfloat16)
    kv[80:] = 0
    q, k, v = qkv[:, D:2 * D], kv[:, :D], kv[:, D:]
    vt = ops.transpose_v(v, Skv, B, H)
    out = ops.flash_attn(q, k, vt, Sq, Skv, B, H)
    torch.cuda.synchronize()
    ref = _attn_ref(q.contiguous(), k.contiguous(), v.contiguous(), Sq, Skv, B, H)
    _report("attn strided", out, ref)
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)


def test_flash_attn_folded_long_context_edges():
    """The folded kernel (scale on Q, running max as the MFMA C operand) on long contexts with the awkward cases: ragged last tile,
    a late key whose score jumps far above the running maximum (rescale branch shifts the pending scores), large-magnitude scores,
    batch > 1 and strided q/k/v views."""
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(99)
    for (Sq, Skv, B, H, qscale, spike) in [(200, 4161, 1, 2, 1.0, None), (256, 3000, 2, 2, 1.0, 2900), (96, 2600, 1, 1, 6.0, 2500), (320, 8256, 1, 3, 1.0, 40)]:
        W = H * 128
        big = torch.randn(max(Sq, Skv) * B, 3 * W, device=dev, generator=g).to(torch.bfloat16)
        q, k, v = big[:Sq * B, :W] * qscale, big[:Skv * B, W:2 * W], big[:Skv * B, 2 * W:]
        q = q.to(torch.bfloat16)
        if spike is not None:  # one key aligned with every query: its score towers over the rest
            k = k.clone()
            k.view(Skv, B, H, 128)[spike] = (q.view(Sq, B, H, 128).float().mean(0) * 4).to(torch.bfloat16)
        out = ops.flash_attn(q, k, ops.transpose_v(v, Skv, B, H), Sq, Skv, B, H)
        q4, k4, v4 = (t.float().reshape(-1, B, H, 128).permute(1, 2, 0, 3) for t in (q, k, v))
        ref = (torch.softmax(q4 @ k4.transpose(-1, -2) / math.sqrt(128), -1) @ v4).permute(2, 0, 1, 3).reshape(Sq * B, W)
        r = _rel_l2(out, ref)
        print(f"[attn folded edges Sq={Sq} Skv={Skv} B={B} H={H}] rel_l2={r:.3e}")
        assert torch.isfinite(out.float()).all() and r < 1e-2


def test_flash_attn_segmented_vt_matches_plain():
    """g3_flash_attn_fwd_kvseg_bf16: V^T handed over as n key segments (what a rank-major all-gather of per-rank V^T shards looks
    like) gives bit-identical output to one contiguous V^T - only the addressing of the V tiles differs."""
    from gen3c_amd import ops
    dev = _dev()
    for (Sq, S_loc, n, B, H) in [(320, 128, 4, 1, 2), (200, 64, 8, 2, 3), (7040, 7040, 2, 1, 2)]:
        Skv = S_loc * n
        g = torch.Generator(device=dev).manual_seed(Sq + Skv)
        q = torch.randn(Sq * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
        k = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
        ref = ops.flash_attn(q, k, ops.transpose_v(v, Skv, B, H), Sq, Skv, B, H)
        segs = torch.stack([ops.transpose_v(v[i * S_loc * B:(i + 1) * S_loc * B], S_loc, B, H) for i in range(n)])  # [n,B,H,128,ld]
        out = ops.flash_attn(q, k, segs.contiguous(), Sq, Skv, B, H)
        assert torch.equal(out, ref), (Sq, S_loc, n, B, H)


@pytest.mark.parametrize("variant", [9, 10, 11], ids=["attn_w4", "attn_w4b", "attn_w4b_xb"])
def test_flash_attn_one_wave_per_simd_long_context(variant):
    """The one-wave-per-SIMD kernels (attention_w4.hpp / attention_w4b.hpp) on what their hand-laid tile stream has to get right: many tiles
    (ring slots and LDS-DMA bases wrap), keys whose scores tower over the running maximum late in the context (rescale branch with fragment
    reads in flight), an odd and an even number of tiles, an odd key count (2209 = 47 x 47: ragged last tile), query counts that do not fill the last
    workgroup, batch > 1, strided views, and V^T handed over in key segments (bit-identical to the contiguous layout)."""
    from gen3c_amd import ops
    dev = _dev()
    ops.set_option("attn_variant", variant)
    try:
        g = torch.Generator(device=dev).manual_seed(1234 + variant)
        for (Sq, Skv, B, H, qscale, spikes) in [(300, 4160, 1, 2, 1.0, ()), (256, 3008, 2, 2, 1.0, (2900,)), (96, 2624, 1, 1, 6.0, (70, 2500)), (520, 8256, 1, 3, 1.0, (40, 8200)),
                                                (64, 64, 1, 1, 1.0, ()), (130, 128, 1, 2, 1.0, (100,)), (189, 2209, 2, 2, 1.0, (2150,))]:
            W = H * 128
            big = torch.randn(max(Sq, Skv) * B, 3 * W, device=dev, generator=g).to(torch.bfloat16)
            q, k, v = (big[:Sq * B, :W] * qscale).to(torch.bfloat16), big[:Skv * B, W:2 * W], big[:Skv * B, 2 * W:]
            if spikes:
                k = k.clone()
                for i, sp in enumerate(spikes):  # keys aligned with the queries: scores far above everything before them, growing
                    k.view(Skv, B, H, 128)[sp] = (q.view(Sq, B, H, 128).float().mean(0) * (4 + 3 * i)).to(torch.bfloat16)
            out = ops.flash_attn(q, k, ops.transpose_v(v, Skv, B, H), Sq, Skv, B, H)
            q4, k4, v4 = (t.float().reshape(-1, B, H, 128).permute(1, 2, 0, 3) for t in (q, k, v))
            ref = (torch.softmax(q4 @ k4.transpose(-1, -2) / math.sqrt(128), -1) @ v4).permute(2, 0, 1, 3).reshape(Sq * B, W)
            r = _rel_l2(out, ref)
            print(f"[attn variant {variant} Sq={Sq} Skv={Skv} B={B} H={H}] rel_l2={r:.3e}")
            assert torch.isfinite(out.float()).all() and r < 1e-2, (Sq, Skv, B, H, r)
        for (Sq, S_loc, n, B, H) in [(320, 128, 4, 1, 2), (200, 64, 8, 2, 3), (300, 1408, 3, 1, 2)]:
            Skv = S_loc * n
            g = torch.Generator(device=dev).manual_seed(Sq + Skv)
            q = torch.randn(Sq * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
            k = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
            v = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
            ref = ops.flash_attn(q, k, ops.transpose_v(v, Skv, B, H), Sq, Skv, B, H)
            segs = torch.stack([ops.transpose_v(v[i * S_loc * B:(i + 1) * S_loc * B], S_loc, B, H) for i in range(n)])
            out = ops.flash_attn(q, k, segs.contiguous(), Sq, Skv, B, H)
            assert torch.equal(out, ref), (Sq, S_loc, n, B, H)
            ops.set_option("attn_variant", 4)
            base = ops.flash_attn(q, k, ops.transpose_v(v, Skv, B, H), Sq, Skv, B, H)
            ops.set_option("attn_variant", variant)
            assert _rel_l2(out, base.float()) < 4e-3
    finally:
        ops.set_option("attn_variant", 0)


@pytest.mark.parametrize("rows,D,B", [(64, 128, 1), (1000, 256, 2), (4096, 4096, 1), (77, 8192, 1)])
def test_layernorm_modulate(rows, D, B):
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(rows + D)
    rows = rows // B * B
    x = (torch.randn(rows, D, device=dev, generator=g) * 2 + 0.5).to(torch.bfloat16)
    mod = torch.randn(B, 3 * D, device=dev, generator=g).to(torch.bfloat16)
    shift, scale = mod[:, :D], mod[:, D:2 * D]
    out = ops.layernorm_modulate(x, shift, scale)
    torch.cuda.synchronize()
    xn = torch.nn.functional.layer_norm(x.float(), (D,), None, None, 1e-6)
    ref = xn * (1 + scale.float().repeat(rows // B, 1)) + shift.float().repeat(rows // B, 1)
    _report(f"ln_mod {rows}x{D}", out, ref)
    torch.testing.assert_close(out.float(), ref, rtol=1.0 / 128, atol=1e-2)


@pytest.mark.parametrize("S,B,H,rope", [(64, 1, 1, True), (333, 2, 3, True), (512, 1, 32, False)])
def test_qk_rmsnorm_rope(S, B, H, rope):
    from gen3c_amd import ops
    from oracle import dit_oracle
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(S + H)
    D = H * 128
    qkv = torch.randn(S * B, 3 * D, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    freqs = torch.randn(S, 128, device=dev, generator=g) * 3
    x = qkv[:, D:2 * D]
    cos, sin = (torch.cos(freqs).contiguous(), torch.sin(freqs).contiguous()) if rope else (None, None)
    out = ops.qk_rmsnorm_rope(x, w, cos, sin, S, B, H)
    torch.cuda.synchronize()
    t = x.float().reshape(S, B, H, 128)
    ref = dit_oracle.te_rmsnorm(t, w.float())
    if rope:
        ref = dit_oracle.te_rope_fused(ref, freqs.view(S, 1, 1, 128))
    ref = ref.reshape(S * B, D)
    _report(f"qk_norm_rope S{S} B{B} H{H} rope={rope}", out, ref)
    torch.testing.assert_close(out.float(), ref, rtol=1.5 / 128, atol=2e-2)


@pytest.mark.parametrize("Sq,Skv,live,B,H", [(700, 512, 64, 2, 4), (512, 512, 100, 1, 2), (1000, 512, 300, 2, 2), (300, 256, 1, 2, 3), (513, 512, 449, 1, 2)])
def test_flash_attn_zero_tail_is_the_dense_softmax(Sq, Skv, live, B, H):
    """Round 6 (g3_cross_attn_fwd_bf16, kv_dense): keys [live, Skv) have all-zero K rows and V^T columns (zero-padded T5 tokens). The launch that runs its tile
    loop over ceil64(live) keys and adds the tail in closed form must give the softmax over ALL Skv keys - the padded tokens stay in the denominator
    (general_dit.py:407-410) - i.e. what the dense launch gives (same kernel, other summation order of the identical tail terms: <= 1 bf16 ulp apart) and
    what an fp32 softmax over all keys gives. Cases: scores well below and well above 0 (the tail's score) so that both branches of m' = max(m, 0) run;
    live = 449 -> ceil64 = 512 = Skv: nothing to skip (plain launch)."""
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(Sq + live)
    for qscale in (0.3, 3.0):
        q = (torch.randn(Sq * B, H * 128, device=dev, generator=g) * qscale).to(torch.bfloat16)
        k = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
        k[live * B:] = 0
        v[live * B:] = 0
        vt = ops.transpose_v(v, Skv, B, H)
        dense = ops.flash_attn(q, k, vt, Sq, Skv, B, H)
        short = ops.flash_attn(q, k, vt, Sq, Skv, B, H, kv_dense=live)
        torch.cuda.synchronize()
        qf = q.float().view(Sq, B, H, 128).permute(1, 2, 0, 3)
        kf = k.float().view(Skv, B, H, 128).permute(1, 2, 0, 3)
        vf = v.float().view(Skv, B, H, 128).permute(1, 2, 0, 3)
        ref = (torch.softmax(qf @ kf.transpose(-1, -2) / math.sqrt(128), dim=-1) @ vf).permute(2, 0, 1, 3).reshape(Sq * B, H * 128)
        r_d, r_s = _rel_l2(dense, ref), _rel_l2(short, ref)
        r_ds = _rel_l2(short, dense)
        print(f"[zero tail Sq{Sq} Skv{Skv} live{live} B{B} H{H} qscale {qscale}] dense vs fp32 {r_d:.2e}  shortcut vs fp32 {r_s:.2e}  shortcut vs dense {r_ds:.2e}")
        assert r_s < 6e-3 and r_s <= 1.2 * r_d + 1e-4
        assert r_ds < 2e-3
        # all-negative scores (every real key scores below the tail's 0): the tail dominates the denominator
        q2 = (-(k.float()[:B].repeat(Sq, 1)) * 0.5).to(torch.bfloat16)
        d2 = ops.flash_attn(q2, k, vt, Sq, Skv, B, H)
        s2 = ops.flash_attn(q2, k, vt, Sq, Skv, B, H, kv_dense=live)
        assert _rel_l2(s2, d2) < 2e-3


@pytest.mark.parametrize("Sq,Skv,B,H,live", [(700, 512, 2, 4, 0), (300, 77, 1, 2, 0), (1000, 512, 2, 2, 64)])
def test_cross_attention_q_norm_inside_the_kernel(Sq, Skv, B, H, live):
    """Round 6 (g3_cross_attn_fwd_bf16, q_norm_weight): the per-head RMSNorm of the cross-attention's Q applied in the attention kernel's Q load == the separate
    norm pass followed by the plain launch (same rounding points; the 128 squares are summed in another order -> an occasional 1-ulp bf16 flip of a normalised q),
    and == an fp32 evaluation (te_rmsnorm -> softmax). Also combined with the zero-tail form; strided q (a column view of a wider buffer); ragged Skv."""
    from gen3c_amd import ops
    from oracle import dit_oracle
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(Sq + Skv)
    wide = (torch.randn(Sq * B, 2 * H * 128, device=dev, generator=g) * 1.7).to(torch.bfloat16)
    q = wide[:, H * 128:]
    k = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    if live:
        k[live * B:] = 0
        v[live * B:] = 0
    w = (torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    vt = ops.transpose_v(v, Skv, B, H)
    qn = ops.qk_rmsnorm_rope(q, w, None, None, Sq, B, H)
    sep = ops.flash_attn(qn, k, vt, Sq, Skv, B, H)
    fused = ops.flash_attn(q, k, vt, Sq, Skv, B, H, q_norm_weight=w, kv_dense=live)
    torch.cuda.synchronize()
    qf = dit_oracle.te_rmsnorm(q.float().reshape(Sq, B, H, 128), w.float()).permute(1, 2, 0, 3)
    kf = k.float().view(Skv, B, H, 128).permute(1, 2, 0, 3)
    vf = v.float().view(Skv, B, H, 128).permute(1, 2, 0, 3)
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) / math.sqrt(128), dim=-1) @ vf).permute(2, 0, 1, 3).reshape(Sq * B, H * 128)
    r_sep, r_fused, r_both = _rel_l2(sep, ref), _rel_l2(fused, ref), _rel_l2(fused, sep)
    print(f"[cross-attn q-norm in kernel Sq{Sq} Skv{Skv} B{B} H{H} live{live}] separate vs fp32 {r_sep:.2e}  in-kernel vs fp32 {r_fused:.2e}  in-kernel vs separate {r_both:.2e}")
    assert r_fused < 6e-3 and r_fused <= 1.2 * r_sep + 1e-4 and r_both < 2e-3


@pytest.mark.parametrize("S,B,H,K", [(512, 2, 4, 512), (1000, 2, 2, 256), (4096, 1, 8, 1024), (2048, 2, 16, 4096), (180, 2, 2, 256)])
def test_v_projection_by_operand_swap_is_the_transposed_projection(S, B, H, K):
    """Round 6 (gen3c_amd/dit.py: _V_OPERAND_SWAP): V^T[b] = W_v . h[:, b]^T - the V projection with the GEMM's operands swapped, one launch per batch item,
    written straight into the V^T [B, H, 128, ld] buffer - is BITWISE the transpose pass applied to the fused projection's v columns (same products,
    same K order per element), on shapes that run the deferred-epilogue kernel (2048 x 2 x 16 heads x K 4096), the plain one-wave kernel and ragged tiles
    (180 tokens: S % 4 == 0 but no whole 64-key tile, so the V^T rows keep a zero tail the swapped GEMM must not touch)."""
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(S + H + K)
    D = H * 128
    h = torch.randn(S * B, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(3 * D, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    qkv = ops.gemm_nt(h, w)
    ld = ops.ceil_to(S, 64)
    ref = ops.transpose_v(qkv[:, 2 * D:], S, B, H, out=torch.zeros(B, H, 128, ld, device=dev, dtype=torch.bfloat16))
    vt = torch.zeros(B, H, 128, ld, device=dev, dtype=torch.bfloat16)
    hv = h.view(S, B, K)
    for b in range(B):
        ops.gemm_nt(w[2 * D:], hv[:, b], out=vt[b].view(D, ld)[:, :S])
    torch.cuda.synchronize()
    assert torch.equal(vt, ref)
    qk = ops.gemm_nt(h, w[:2 * D])
    assert torch.equal(qk, qkv[:, :2 * D]), "a row slice of the fused weight gives the same q | k columns"


def test_v_projection_by_operand_swap_is_refused_at_a_token_count_that_is_no_multiple_of_4():
    """The guard in gen3c_amd/dit.py (_v_by_operand_swap) relies on this: the swapped V GEMM at N = S with S % 4 != 0 raises (g3_gemm_bf16_nt stores 4
    columns at a time) instead of writing anything - the V^T buffer, tail included, is left as it was."""
    from gen3c_amd import _lib, ops
    dev = _dev()
    S, B, H, K = 189, 2, 2, 256
    D, ld = H * 128, ops.ceil_to(S, 64)
    g = torch.Generator(device=dev).manual_seed(S)
    h = torch.randn(S * B, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(D, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    vt = torch.full((B, H, 128, ld), 3.0, device=dev, dtype=torch.bfloat16)
    for b in range(B):
        with pytest.raises(_lib.Gen3cHipError, match=r"g3_gemm_bf16_nt: need .*N.* % 4"):
            ops.gemm_nt(w, h.view(S, B, K)[:, b], out=vt[b].view(D, ld)[:, :S])
    torch.cuda.synchronize()
    assert bool((vt == 3.0).all())


@pytest.mark.parametrize("S,B,Hq,Hk,rope", [(333, 2, 8, 8, True), (130, 1, 16, 8, True), (97, 2, 8, 24, False), (1000, 2, 32, 32, True)])
def test_qk_rmsnorm_rope_octet_and_pair(S, B, Hq, Hk, rope):
    """Round 6: the octet form (one 8-lane group keeps a row's cos / sin and the weights for 8 consecutive heads) and the two-region entry
    g3_qk_rmsnorm_rope_pair_bf16 (q | k of the fused QKV buffer in one in-place launch): vs the fp32 oracle, and BITWISE equal to the general
    one-group-per-head kernel run region by region (same arithmetic body). Row counts that leave ragged last workgroups."""
    from gen3c_amd import _lib, ops
    from oracle import dit_oracle
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(S + Hq + 3 * Hk)
    Dq, Dk = Hq * 128, Hk * 128
    qkv = torch.randn(S * B, Dq + Dk + 256, device=dev, generator=g).to(torch.bfloat16)  # a strided view with a plain tail (the v columns)
    wq = (torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    wk = (torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    freqs = torch.randn(S, 128, device=dev, generator=g) * 3
    cos, sin = (torch.cos(freqs).contiguous(), torch.sin(freqs).contiguous()) if rope else (None, None)
    lib = _lib.load()
    general = qkv.clone()
    assert lib.g3_set_option(b"norm_octets", 0) == 0
    try:
        ops.qk_rmsnorm_rope(general[:, :Dq], wq, cos, sin, S, B, Hq, out=general[:, :Dq])
        ops.qk_rmsnorm_rope(general[:, Dq:Dq + Dk], wk, cos, sin, S, B, Hk, out=general[:, Dq:Dq + Dk])
    finally:
        assert lib.g3_set_option(b"norm_octets", 1) == 0
    octet = qkv.clone()
    ops.qk_rmsnorm_rope(octet[:, :Dq], wq, cos, sin, S, B, Hq, out=octet[:, :Dq])
    ops.qk_rmsnorm_rope(octet[:, Dq:Dq + Dk], wk, cos, sin, S, B, Hk, out=octet[:, Dq:Dq + Dk])
    pair = qkv.clone()
    ops.qk_rmsnorm_rope_pair(pair[:, :Dq + Dk], wq, Hq, wk, Hk, cos, sin, S, B)
    separate = ops.qk_rmsnorm_rope(qkv[:, :Dq], wq, cos, sin, S, B, Hq)  # out of place, packed output
    torch.cuda.synchronize()
    assert torch.equal(octet, general), "octet form != general form"
    assert torch.equal(pair, general), "two-region launch != two launches"
    assert torch.equal(separate, general[:, :Dq])
    assert torch.equal(pair[:, Dq + Dk:], qkv[:, Dq + Dk:]), "the plain tail must be untouched"
    for x, w, H, got in ((qkv[:, :Dq], wq, Hq, pair[:, :Dq]), (qkv[:, Dq:Dq + Dk], wk, Hk, pair[:, Dq:Dq + Dk])):
        ref = dit_oracle.te_rmsnorm(x.float().reshape(S, B, H, 128), w.float())
        if rope:
            ref = dit_oracle.te_rope_fused(ref, freqs.view(S, 1, 1, 128))
        torch.testing.assert_close(got.float(), ref.reshape(S * B, H * 128), rtol=1.5 / 128, atol=2e-2)


@pytest.mark.parametrize("M,N,K,act", [(1, 256, 4096, 1), (1, 12288, 256, 0), (3, 100, 64, 1), (8, 384, 128, 0)])
def test_gemv(M, N, K, act):
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(N + K)
    a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    add = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    out = ops.gemv(a, w, add=add, act_in=act)
    torch.cuda.synchronize()
    af = a.float()
    if act:
        af = torch.nn.functional.silu(af).to(torch.bfloat16).float()
    ref = (af @ w.float().t()).to(torch.bfloat16).float() + add.float()
    _report(f"gemv {M}x{N}x{K}", out, ref)
    torch.testing.assert_close(out.float(), ref, rtol=1.5 / 128, atol=2e-2)


def test_add_inplace():
    from gen3c_amd import ops
    dev = _dev()
    x = torch.randn(1000, 256, device=dev).to(torch.bfloat16)
    y = torch.randn(1000, 256, device=dev).to(torch.bfloat16)
    ref = (x.float() + y.float()).to(torch.bfloat16)
    ops.add_inplace(x, y)
    torch.cuda.synchronize()
    assert torch.equal(x, ref)


@pytest.mark.parametrize("T,Hp,Wp,B,D", [(3, 4, 5, 1, 256), (2, 3, 7, 2, 4096), (1, 5, 2, 3, 512)])
def test_posemb_layernorm_modulate_equals_the_two_pass_path(T, Hp, Wp, B, D):
    """The fused top-of-block kernel (x += per-block absolute position embedding, then LayerNorm + AdaLN modulate) against the two
    separate passes over a MATERIALISED embedding built with torch in the reference's order (position_embedding.py:218-233, normalize
    attention.py:108-124): x after the add and the modulated output must both be bit-identical (same bf16 rounding points)."""
    import math
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(T * 100 + D)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    pe_t, pe_h, pe_w = ((rnd(n, D) * 0.02).to(torch.bfloat16) for n in (T + 2, Hp + 1, Wp + 3))  # tables longer than the used range
    emb = (pe_t[:T, None, None, :] + pe_h[None, :Hp, None, :]) + pe_w[None, None, :Wp, :]
    norm = torch.linalg.vector_norm(emb, dim=-1, keepdim=True, dtype=torch.float32)
    norm = torch.add(1e-6, norm, alpha=math.sqrt(1.0 / D))
    emb_n = emb / norm.to(emb.dtype)
    S = T * Hp * Wp
    table = emb_n.reshape(S, 1, D).expand(-1, B, -1).reshape(S * B, D).contiguous()
    x = rnd(S * B, D).to(torch.bfloat16)
    shift, scale = (rnd(B, 3 * D)[:, :D] * 0.3).to(torch.bfloat16), (rnd(B, 3 * D)[:, D:2 * D] * 0.3).to(torch.bfloat16)  # strided [B, D] views
    x_ref = x.clone()
    ops.add_inplace(x_ref, table)
    h_ref = ops.layernorm_modulate(x_ref, shift, scale)
    x_new = x.clone()
    h = ops.posemb_layernorm_modulate(x_new, pe_t[:T].contiguous(), pe_h[:Hp].contiguous(), pe_w[:Wp].contiguous(),
                                      norm.to(torch.bfloat16).reshape(S).contiguous(), T, Hp, Wp, B, shift, scale)
    torch.cuda.synchronize()
    assert torch.equal(x_new, x_ref), f"x differs on {int((x_new != x_ref).sum())} elements"
    assert torch.equal(h, h_ref), f"LN output differs on {int((h != h_ref).sum())} elements"
    assert not torch.equal(x_new, x)
    # the form the DiT uses: ONE materialised table [S, D] (the embedding above, not repeated over B) instead of the three axis tables
    x_mat = x.clone()
    h_mat = ops.posemb_layernorm_modulate(x_mat, emb_n.reshape(S, D).contiguous(), None, None, None, T, Hp, Wp, B, shift, scale)
    torch.cuda.synchronize()
    assert torch.equal(x_mat, x_ref) and torch.equal(h_mat, h_ref)


def test_errors_are_loud():
    from gen3c_amd import _lib, ops
    dev = _dev()
    a = torch.zeros(8, 12, device=dev, dtype=torch.bfloat16)  # K=12 not a multiple of 8
    w = torch.zeros(8, 12, device=dev, dtype=torch.bfloat16)
    with pytest.raises(_lib.Gen3cHipError):
        ops.gemm_nt(a, w)
    with pytest.raises(_lib.Gen3cHipError):
        ops.gemm_nt(a.cpu(), w.cpu())  # no CPU fallback


def test_dit_patchify_unpatchify_timestep_embedding():
    """csrc/embed.hip against the torch expressions they replace (general_dit_video_conditioned.py:77-101 + blocks.py:154-159;
    general_dit.py:348-357; blocks.py:38-57 + general_dit.py:173-177). Pure data movement must be exact."""
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(5)
    B, T, H, W, pt, ps = 2, 3, 8, 12, 1, 2
    x = torch.randn(B, 16, T, H, W, device=dev, generator=g).to(torch.bfloat16)
    m = torch.randn(B, 1, T, H, W, device=dev, generator=g).to(torch.bfloat16)
    pose = torch.randn(B, 64, T, H, W, device=dev, generator=g).to(torch.bfloat16)
    pad = torch.randn(B, 1, H, W, device=dev, generator=g).to(torch.bfloat16)
    got = ops.dit_patchify([(x, True), (m, True), (pose, True), (pad, False)], B, T, H, W, pt, ps)
    cat = torch.cat([x, m, pose, pad[:, :, None].expand(B, 1, T, H, W)], dim=1)
    Tp, Hp, Wp = T // pt, H // ps, W // ps
    ref = cat.view(B, -1, Tp, pt, Hp, ps, Wp, ps).permute(2, 4, 6, 0, 1, 3, 5, 7).reshape(Tp * Hp * Wp * B, -1)
    assert torch.equal(got, ref)
    Co = 16
    y = torch.randn(Tp * Hp * Wp * B, ps * ps * pt * Co, device=dev, generator=g).to(torch.bfloat16)
    got = ops.dit_unpatchify(y, B, Co, T, H, W, pt, ps)
    ref = y.view(Tp, Hp, Wp, B, ps, ps, pt, Co).permute(3, 7, 0, 6, 1, 4, 2, 5).reshape(B, Co, T, H, W)
    assert torch.equal(got, ref)
    D = 4096
    ts = torch.tensor([0.25 * math.log(80.0), 0.25 * math.log(0.002)], device=dev).to(torch.bfloat16).float()
    w = (1.0 + 0.1 * torch.randn(D, device=dev, generator=g)).to(torch.bfloat16)
    t_sin, emb = ops.timestep_embedding(ts.contiguous(), w, D)
    half = D // 2
    expo = -math.log(10000) * torch.arange(half, dtype=torch.float32, device=dev) / half
    ang = ts[:, None] * torch.exp(expo)[None]
    ref_sin = torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1).to(torch.bfloat16)
    assert float((t_sin.float() - ref_sin.float()).abs().max()) <= 2 ** -7  # one bf16 ulp at |x| <= 1 (libm cos/sin/exp ulps)
    tf = ref_sin.float()
    ref_emb = (tf * torch.rsqrt(tf.pow(2).mean(-1, keepdim=True) + 1e-6) * w.float()).to(torch.bfloat16)
    assert _rel_l2(emb, ref_emb) < 2e-3


def test_gemm_known_answer_constant_weights():
    """The reference's only numeric check near this path fills projection weights with 0.1 and expects q = in_features * 0.1
    (diffusion/training/utils/peft/lora_attn_test.py:73-250, model_channels = 256): same closed form through the MFMA GEMM."""
    from gen3c_amd import ops
    dev = _dev()
    for K in (256, 4096):
        x = torch.ones(300, K, device=dev, dtype=torch.bfloat16)
        w = torch.full((512, K), 0.1, device=dev, dtype=torch.bfloat16)
        out = ops.gemm_nt(x, w).float()
        expect = K * float(torch.tensor(0.1, dtype=torch.bfloat16))  # 0.1 is rounded to bf16 once, then summed exactly in fp32
        torch.testing.assert_close(out, torch.full_like(out, expect), rtol=1e-2, atol=0)  # rtol of the reference test
        assert float(out.std()) == 0.0


@pytest.mark.parametrize("variant", [4, 11])
@pytest.mark.parametrize("S_local,world,rank,B,H", [(3520, 4, 1, 1, 8), (1024, 8, 0, 2, 4), (704, 2, 1, 1, 2)])
def test_flash_attn_split_kv_partials_merge(variant, S_local, world, rank, B, H):
    """Split-KV attention: the keys of a row are covered by several launches that return a normalised fp32 partial +
    log-sum-exp each (g3_flash_attn_fwd_ex_bf16), merged by g3_attn_merge_partials_bf16. Layout as under context parallelism: K gathered
    rank-major, V^T in per-rank key segments; parts = this rank's own shard, the ranks before it, the ranks after it. Must match the
    single call over all keys and an fp32 softmax. Tolerances: vs fp32 <= 4e-3 - the bound the single call itself is held to
    (tests/test_fullsize_gpu.py; measured 2.9e-3 for both) - and no worse than the single call's own error + 10 %; vs the single call <= 4.5e-3:
    the two results carry INDEPENDENT bf16 roundings of P (each launch rounds relative to its own running maximum), so their distance is
    ~sqrt(2) x the distance of either to fp32 (measured 2.9e-3 .. 3.3e-3), exactly as for a permutation of the keys."""
    from gen3c_amd import ops
    dev = _dev()
    S_all = S_local * world
    g = torch.Generator(device=dev).manual_seed(S_local + world + rank)
    q = torch.randn(S_local * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(S_all * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(S_all * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    rows = S_local * B
    vt_seg = torch.stack([ops.transpose_v(v[r * rows:(r + 1) * rows], S_local, B, H) for r in range(world)])  # [world, B, H, 128, S_local]
    full = ops.flash_attn(q, k, vt_seg, S_local, S_all, B, H, variant=variant)
    parts = []
    for (r0, r1) in ((rank, rank + 1), (0, rank), (rank + 1, world)):
        if r1 > r0:
            parts.append(ops.flash_attn(q, k[r0 * rows:r1 * rows], vt_seg[r0:r1].contiguous(), S_local, (r1 - r0) * S_local, B, H, variant=variant, partial=True))
    merged = ops.attn_merge(parts, S_local, B, H)
    r_split = _rel_l2(merged, full)
    worst = worst_full = 0.0
    for b in range(B):
        for h in range(H):
            sl = slice(h * 128, (h + 1) * 128)
            sc = (q[b::B, sl].float() @ k[b::B, sl].float().t()) / math.sqrt(128)
            ref = torch.softmax(sc, dim=-1) @ v[b::B, sl].float()
            worst = max(worst, _rel_l2(merged[b::B, sl], ref))
            worst_full = max(worst_full, _rel_l2(full[b::B, sl], ref))
    print(f"[split-kv v{variant} S_local={S_local} world={world} rank={rank} B={B} H={H}] {len(parts)} parts: vs one call {r_split:.3e}, "
          f"vs fp32 {worst:.3e} (single call vs fp32 {worst_full:.3e})")
    assert r_split <= 4.5e-3 and worst <= 4e-3 and worst <= 1.1 * worst_full
    # a single part merged alone is the plain result (weights = 1): fp32 partial -> bf16 once
    one = ops.attn_merge([ops.flash_attn(q, k, vt_seg, S_local, S_all, B, H, variant=variant, partial=True)], S_local, B, H)
    assert _rel_l2(one, full) <= 1e-6 or torch.equal(one, full)


def test_flash_attn_per_call_variant_leaves_global_option_alone():
    """the context-parallel path used to toggle the process-global "attn_variant" around launches; the choice is now an argument."""
    from gen3c_amd import _lib, ops
    dev = _dev()
    lib = _lib.load()
    S, H = 4096, 8
    g = torch.Generator(device=dev).manual_seed(1)
    q, k, v = (torch.randn(S, H * 128, device=dev, generator=g).to(torch.bfloat16) for _ in range(3))
    vt = ops.transpose_v(v, S, 1, H)
    auto_name = lib.g3_flash_attn_kernel_name(S, S, 1, H)
    a = ops.flash_attn(q, k, vt, S, S, 1, H, variant=4)
    b = ops.flash_attn(q, k, vt, S, S, 1, H, variant=11)
    assert lib.g3_flash_attn_kernel_name(S, S, 1, H) == auto_name
    assert lib.g3_flash_attn_kernel_name_ex(S, S, 1, H, 4).decode().startswith("flash_attn_fwd_v3_kernel")
    assert lib.g3_flash_attn_kernel_name_ex(S, S, 1, H, 11).decode() == "flash_attn_fwd_w4b_kernel<true>"
    assert _rel_l2(a, b) < 6e-3


@pytest.mark.parametrize("case,kernel", [("partial_ragged_v11", "flash_attn_fwd_v3_kernel<1, 6, 8, false>"), ("short_vt_ld", "flash_attn_fwd_v2_kernel<1>"),
                                         ("cross_tail_qnorm", "flash_attn_fwd_v3_kernel<1, 6, 8, false>")])
def test_kernel_timer_records_the_kernel_that_ran_after_a_launcher_fallback(case, kernel):
    """The `kernel` of a kernel-timer entry is the dry run's answer (g3_attn_plan_bf16) for the arguments launched, launcher fallbacks included:
    split-KV partials on ragged keys under variant 11 (-> w4 -> the 8-wave kernel), a V^T leading dimension of ceil8 but below ceil64 of the keys
    (-> the 64-bit-addressing kernel), the cross-attention form (-> the v3 kernels). Outputs against the fp32 softmax at test_flash_attn's bar."""
    from gen3c_amd import ops
    from oracle import dit_oracle
    dev = _dev()
    Sq, B, H = 200, 2, 2
    Skv = 512 if case == "cross_tail_qnorm" else 100
    g = torch.Generator(device=dev).manual_seed(len(case))
    q = torch.randn(Sq * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(Skv * B, H * 128, device=dev, generator=g).to(torch.bfloat16)
    q_ref = q
    ops.enable_kernel_timers(True)
    try:
        if case == "partial_ragged_v11":
            out, _ = ops.flash_attn(q, k, ops.transpose_v(v, Skv, B, H), Sq, Skv, B, H, partial=True, variant=11)
        elif case == "short_vt_ld":
            vt = ops.transpose_v(v, Skv, B, H)[..., :104].contiguous()  # (the zero tail [100, 104) included)
            out = ops.flash_attn(q, k, vt, Sq, Skv, B, H)
        else:
            k[64 * B:] = 0
            v[64 * B:] = 0
            w = (torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16)
            out = ops.flash_attn(q, k, ops.transpose_v(v, Skv, B, H), Sq, Skv, B, H, kv_dense=64, q_norm_weight=w)
            q_ref = dit_oracle.te_rmsnorm(q.float().reshape(Sq, B, H, 128), w.float()).reshape(Sq * B, H * 128)
        torch.cuda.synchronize()
        timers = ops.collected_kernel_timers()
    finally:
        ops.enable_kernel_timers(False)
    (name, meta, _), = [t for t in timers if t[0] == "flash_attn_fwd"]
    print(f"[attn timer {case}] kernel={meta['kernel']}")
    assert meta["kernel"] == kernel
    ref = _attn_ref(q_ref, k, v, Sq, Skv, B, H)
    _report(f"attn fallback {case}", out, ref)
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)
    assert _rel_l2(out, ref) < 1e-2


def test_hip_dot_product_attention_operator_seam():
    """SURVEY 8b "Attention operator": the reference's Attention module calls attn_op(q, k, v, core_attention_bias_type="no_bias",
    core_attention_bias=None) on sbhd tensors and expects [S, B, H*d] (attention.py:282-297); general_dit.py:541 hands the operator a
    context-parallel group. gen3c_amd.attention_op.HipDotProductAttention on [S, B, 32, 128] inputs vs an fp32 softmax."""
    import os
    import torch.distributed as dist
    from gen3c_amd.attention_op import HipDotProductAttention
    dev = _dev()
    S, B, H = 1536, 2, 32
    g = torch.Generator(device=dev).manual_seed(77)
    q, k, v = (torch.randn(S, B, H, 128, device=dev, generator=g).to(torch.bfloat16) for _ in range(3))
    op = HipDotProductAttention(H, 128, num_gqa_groups=H, attention_dropout=0, qkv_format="sbhd", attn_mask_type="no_mask", tp_size=1,
                                tp_group=None, sequence_parallel=False)  # the reference's constructor call, attention.py:228-238
    out = op(q, k, v, core_attention_bias_type="no_bias", core_attention_bias=None)
    assert out.shape == (S, B, H * 128) and out.dtype == torch.bfloat16
    qf, kf, vf = (t.permute(1, 2, 0, 3).float() for t in (q, k, v))
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) / math.sqrt(128), dim=-1) @ vf).permute(2, 0, 1, 3).reshape(S, B, H * 128)
    r = _rel_l2(out, ref)
    print(f"[HipDotProductAttention sbhd S={S} B={B} H={H}] rel-L2 vs fp32 {r:.3e}")
    assert r < 4e-3
    with pytest.raises(NotImplementedError):
        op(q, k, v, core_attention_bias_type="post_scale_bias", core_attention_bias=torch.zeros(1, device=dev))
    # the context-parallel hook with a 1-rank group (gloo): every collective call of the CP path runs, result = the plain call
    created = False
    if not dist.is_initialized():
        import socket
        with socket.socket() as s_:
            s_.bind(("127.0.0.1", 0))
            port = s_.getsockname()[1]
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=0, world_size=1)
        created = True
    try:
        grp = dist.new_group([0])
        op.set_context_parallel_group(grp, [0], torch.cuda.Stream())
        out_cp = op(q, k, v, core_attention_bias_type="no_bias", core_attention_bias=None)
        torch.cuda.synchronize()
        assert _rel_l2(out_cp, out) < 3e-3  # (kernel choice per head group may differ from the single launch's)
        op.set_context_parallel_group(None, None, None)
        assert torch.equal(op(q, k, v), out)
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("M,N,K,epi,gate_rows", [(14080, 4096, 4096, 2, 2), (14080, 4096, 4096, 0, 1), (14080, 4096, 16384, 2, 2), (14080, 12288, 4096, 0, 1),
                                                 (14080, 16384, 4096, 1, 1), (28160, 4096, 4096, 2, 2), (28160, 4096, 16384, 2, 2)])
def test_gemm_deferred_epilogue_kernel_at_the_context_parallel_rank_shapes(M, N, K, epi, gate_rows):
    """the block GEMMs at ONE RANK's shapes under context parallelism - M = 2 x 7 040 (cp = 8: 55 x 16 = 880 tiles on 256 persistent workgroups,
    3.44 rounds: 112 workgroups walk four tiles, 144 three) and M = 2 x 14 080 (cp = 4) - deferred-epilogue kernel BITWISE equal to the non-persistent one-wave
    kernel, both piece orders, and within the fp32 bar on sampled rows (same body as test_gemm_deferred_epilogue_kernel)."""
    test_gemm_deferred_epilogue_kernel(M, N, K, epi, gate_rows)


@pytest.mark.parametrize("M,N,K", [(8192, 4096, 2432), (8448, 4096, 4096), (33792, 2048, 2560)])
@pytest.mark.parametrize("epi,gate_rows", [(0, 1), (1, 1), (2, 1), (2, 2), (2, 4)])
def test_gemm_deferred_epilogue_kernel(M, N, K, epi, gate_rows):
    """gemm_bf16_nt_w4e_kernel (csrc/gemm_w4e.hpp, round 5): persistent tile loop, a finished tile's epilogue rides in the next tile's K loop. Against the
    non-persistent one-wave kernel (same arithmetic, epilogue behind its own K loop): BITWISE equal, whatever a tile's position in its workgroup's list
    (carried epilogue / bare flush of the last tile); and against fp32. (8192, 4096, 2432): the minimum K (38 K tiles), exactly 2 tiles per workgroup;
    (8448, 4096, 4096): 528 tiles over 256 workgroups - 2 or 3 tiles each (carry into a carrying tile); (33792, 2048, 2560): 1056 tiles, 4-5 each.
    gate_rows 2 / 4: the conditional + unconditional branches of the DiT step share one launch (row m uses gate row m % gate_rows)."""
    from gen3c_amd import _lib, ops
    dev = _dev()
    name = _lib.load().g3_gemm_kernel_name(M, N, K, epi).decode()
    assert name == "gemm_bf16_nt_w4e_kernel<EPI>", name
    g = torch.Generator(device=dev).manual_seed(M + 3 * N + 7 * K + epi + gate_rows)
    a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(gate_rows, N, device=dev, generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    kw = dict(gate=gate, residual=res) if epi == 2 else {}
    outs = {}
    for deferred in (1, 0):
        ops.set_option("gemm_deferred", deferred)
        outs[deferred] = ops.gemm_nt(a, w, epilogue=epi, **kw).clone()
        for _ in range(2):
            assert torch.equal(outs[deferred], ops.gemm_nt(a, w, epilogue=epi, **kw)), f"deferred={deferred}: not reproducible"
    ops.set_option("gemm_deferred", 1)
    for tf in (0, 1):  # both LDS-DMA piece orders of the deferred kernel (weight rows / token rows two K tiles ahead; default: by shape)
        ops.set_option("gemm_tokens_first", tf)
        assert torch.equal(outs[1], ops.gemm_nt(a, w, epilogue=epi, **kw)), f"gemm_tokens_first={tf} changes the result"
    ops.set_option("gemm_tokens_first", 2)
    torch.cuda.synchronize()
    diff = (outs[1].float() - outs[0].float()).abs()
    bad = int((diff > 0).sum())
    assert bad == 0, f"deferred != plain one-wave kernel: {bad} of {M * N} elements, max |diff| {float(diff.max()):.3e}, first bad row {int((diff > 0).any(dim=1).nonzero()[0])}"
    rows = torch.arange(0, M, 61, device=dev)  # sampled rows vs fp32 (the full fp32 product of the largest case is 280 MB)
    ref = a[rows].float() @ w.float().t()
    if epi == 1:
        ref = torch.nn.functional.gelu(ref)
    elif epi == 2:
        ref = res[rows].float() + gate[rows % gate_rows].float() * ref
    _report(f"gemm deferred {M}x{N}x{K} epi{epi} gate_rows{gate_rows}", outs[1][rows], ref)
    assert _rel_l2(outs[1][rows], ref) < 4e-3


def test_gemm_deferred_epilogue_in_place_residual_and_strided_views():
    """The DiT's gated residual writes x IN PLACE (out aliases the residual) and its operands are column views of wider buffers."""
    from gen3c_amd import ops
    dev = _dev()
    M, N, K = 8192, 4096, 4096
    g = torch.Generator(device=dev).manual_seed(77)
    abuf = torch.randn(M, K + 256, device=dev, generator=g).to(torch.bfloat16)
    a = abuf[:, 128:128 + K]
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(2, N, device=dev, generator=g).to(torch.bfloat16)
    x0 = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    outs = {}
    for deferred in (1, 0):
        ops.set_option("gemm_deferred", deferred)
        x = x0.clone()
        ops.gemm_nt(a, w, out=x, epilogue=2, gate=gate, residual=x)
        outs[deferred] = x
    ops.set_option("gemm_deferred", 1)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref = x0.float() + gate[torch.arange(M, device=dev) % 2].float() * (a.float() @ w.float().t())
    assert _rel_l2(outs[1], ref) < 4e-3


@pytest.mark.parametrize("grid", [8, 72, 248])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_deferred_epilogue_long_and_uneven_tile_lists(grid, epi):
    """The deferred-epilogue kernel's tile loop on fewer workgroups than CUs (test option gemm_deferred_grid): 8 workgroups walk 66 tiles each (one per XCD:
    66 carried epilogues in a row, one flush), 72 walk 7 or 8, 248 walk 2 or 3 - every hand-over (carry into a carrying tile, last-tile flush behind a carry)
    at every position of the XCD-aware tile order. Bitwise equal to the non-persistent kernel."""
    from gen3c_amd import ops
    dev = _dev()
    M, N, K = 8448, 4096, 2560  # 33 x 16 = 528 tiles, 40 K tiles
    g = torch.Generator(device=dev).manual_seed(grid + epi)
    a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(2, N, device=dev, generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    kw = dict(gate=gate, residual=res) if epi == 2 else {}
    try:
        ops.set_option("gemm_deferred", 0)
        ref = ops.gemm_nt(a, w, epilogue=epi, **kw)
        ops.set_option("gemm_deferred", 1)
        ops.set_option("gemm_deferred_grid", grid)
        out = ops.gemm_nt(a, w, epilogue=epi, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_option("gemm_deferred", 1)
        ops.set_option("gemm_deferred_grid", 0)
    diff = (out.float() - ref.float()).abs()
    assert int((diff > 0).sum()) == 0, f"grid {grid}: {int((diff > 0).sum())} elements differ, max {float(diff.max()):.3e}"
