"""Thin torch-tensor front end over the C ABI (include/gen3c_hip.h).

torch is used for what it is good at here - device memory and streams. Every function hands raw device pointers,
shapes and the current HIP stream to libgen3c_hip.so; none of them computes anything in PyTorch.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional

import torch

from . import _lib

EPI_NONE, EPI_GELU, EPI_GATED_RESIDUAL, EPI_BIAS = 0, 1, 2, 3

# bench.py switches this to a list to collect (kernel, shape, HipTimer) triples for the dominant kernel: hipEvents are
# recorded on the launch stream right around the launch (a handful of events per step - no measurable overhead).
_KERNEL_TIMERS = None


def set_option(name: str, value: int):
    """Runtime A/B switch of the C library (g3_set_option)."""
    _lib.check(_lib.load().g3_set_option(name.encode(), int(value)), "g3_set_option")


def option(name: str) -> int:
    """The value of a switch in force in the C library (g3_get_option): its default, its environment variable or the last g3_set_option, whoever called it."""
    import ctypes as C
    v = C.c_int(0)
    _lib.check(_lib.load().g3_get_option(name.encode(), C.byref(v)), "g3_get_option")
    return int(v.value)


def enable_kernel_timers(on: bool = True):
    global _KERNEL_TIMERS
    _KERNEL_TIMERS = [] if on else None


def collected_kernel_timers():
    return list(_KERNEL_TIMERS or [])


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str, dtype=torch.bfloat16) -> int:
    if not t.is_cuda:
        raise _lib.Gen3cHipError(f"{name}: expected a GPU (HIP) tensor, got device {t.device}; gen3c_amd has no CPU path")
    if t.dtype != dtype:
        raise _lib.Gen3cHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t.data_ptr()


def _rowmajor2d(t: torch.Tensor, name: str):
    if t.dim() != 2 or t.stride(1) != 1:
        raise _lib.Gen3cHipError(f"{name}: expected a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


@contextlib.contextmanager
def _kernel_timer(kind: str, meta, on: bool = True):
    """The one kernel timer: with timers enabled (and `on`), a hipEvent pair around the launch inside the block, collected as (kind, meta, timer) -
    meta a dict, or a callable that makes it once the launch has returned. A launch that raises collects nothing."""
    if _KERNEL_TIMERS is None or not on:
        yield
        return
    timer = HipTimer()
    timer.start()
    yield
    timer.stop()
    _KERNEL_TIMERS.append((kind, meta() if callable(meta) else meta, timer))


def _gemm_timer(kind: str, M: int, N: int, K: int, epilogue: int):
    """The timer of the block GEMMs (M >= 4096); tiny ones (context K/V, embeddings of a few rows) are not worth an event pair."""
    return _kernel_timer(kind, dict(M=M, N=N, K=K, epilogue=epilogue), M >= 4096)


def _out_bf16(out: Optional[torch.Tensor], M: int, N: int, device):
    """The bf16 [M, N] output of an op: allocated, or the caller's (any row stride), checked. -> out, its row stride"""
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=device)
    Mo, No, ldc = _rowmajor2d(out, "out")
    assert (Mo, No) == (M, N)
    return out, ldc


def _gate_residual(gate: Optional[torch.Tensor], residual: Optional[torch.Tensor], M: int, N: int):
    """The epilogue operands of the GEMM entries: gate [rows, N], residual [M, N], either may be None. -> gate, gate_rows, ldg, residual, ldr"""
    gp, grows, ldg, rp, ldr = 0, 1, 0, 0, 0
    if gate is not None:
        grows, gn, ldg = _rowmajor2d(gate, "gate")
        assert gn == N
        gp = _dev(gate, "gate")
    if residual is not None:
        rm, rn, ldr = _rowmajor2d(residual, "residual")
        assert (rm, rn) == (M, N)
        rp = _dev(residual, "residual")
    return gp, grows, ldg, rp, ldr


def _rope_tables(cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], S: int):
    """The RoPE tables cos / sin, contiguous fp32 [S, 128], or None for no rotation. -> their pointers (0, 0 without)"""
    if cos is None:
        return 0, 0
    assert cos.shape == (S, 128) and sin.shape == (S, 128) and cos.is_contiguous() and sin.is_contiguous()
    return _dev(cos, "cos", torch.float32), _dev(sin, "sin", torch.float32)


def gemm_nt(a: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None, epilogue: int = EPI_NONE,
            gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = epi(a[M,K] @ w[N,K]^T).  gate: [rows, N] (row = m % rows); residual: [M, N]."""
    M, K, lda = _rowmajor2d(a, "a")
    N, Kw, ldw = _rowmajor2d(w, "w")
    if K != Kw:
        raise _lib.Gen3cHipError(f"gemm_nt: K mismatch {K} vs {Kw}")
    out, ldc = _out_bf16(out, M, N, a.device)
    epi = _gate_residual(gate, residual, M, N)
    with _gemm_timer("gemm_nt", M, N, K, epilogue):
        _lib.check(_lib.load().g3_gemm_bf16_nt(_dev(a, "a"), lda, _dev(w, "w"), ldw, _dev(out, "out"), ldc, M, N, K, epilogue, *epi, _stream()),
                   "g3_gemm_bf16_nt")
    return out


def quant_mxfp8(x: torch.Tensor, out=None):
    """MXFP8 (OCP MX, e4m3fn) of a bf16 [M, K] matrix: (q [M, K] torch.float8_e4m3fn, scales [M, K/32] torch.uint8 E8M0).
    out: an optional (q, scales) pair to write into. See g3_quant_mxfp8_bf16 for the rounding rule."""
    M, K, ldx = _rowmajor2d(x, "x")
    q, s, ldq, lds = _mx_out_pair(out, M, K, x.device, "quant_mxfp8", of=f"x {tuple(x.shape)}")
    _lib.check(_lib.load().g3_quant_mxfp8_bf16(_dev(x, "x"), ldx, _dev(q, "q", torch.float8_e4m3fn), ldq, _dev(s, "scales", torch.uint8), lds, M, K,
                                               _stream()), "g3_quant_mxfp8_bf16")
    return q, s


def _mx_operands(what: str, aq, as_, wq, ws):
    """Shapes and strides of the MX operands and their scales, checked against each other: MXFP8 (gemm_mxfp8_nt, both forms) or MXFP6
    (gemm_mxfp6_nt), whose K comes from the packed row bytes - 32 six-bit codes per 24. -> M, N, K, lda, ldas, ldw, ldws"""
    M, K, lda = _rowmajor2d(aq, "aq")
    N, Kw, ldw = _rowmajor2d(wq, "wq")
    if what == "gemm_mxfp6_nt":
        if K != Kw or K % 24:
            raise _lib.Gen3cHipError(f"gemm_mxfp6_nt: packed row bytes {K} vs {Kw} (must be equal and a multiple of 24)")
        K = K // 3 * 4
    elif K != Kw:
        raise _lib.Gen3cHipError(f"{what}: K mismatch {K} vs {Kw}")
    Ma, Ka, ldas = _rowmajor2d(as_, "as_")
    Nw, Kws, ldws = _rowmajor2d(ws, "ws")
    if (Ma, Nw) != (M, N) or Ka * 32 != K or Kws * 32 != K:
        raise _lib.Gen3cHipError(f"{what}: scale shapes {tuple(as_.shape)} / {tuple(ws.shape)} do not match operands [{M}, {K}] / [{N}, {K}]")
    return M, N, K, lda, ldas, ldw, ldws


def gemm_mxfp8_nt(aq: torch.Tensor, as_: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, out: Optional[torch.Tensor] = None,
                  epilogue: int = EPI_NONE, gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, out_mx=None):
    """out[M,N] = epi(dequant(aq, as_) @ dequant(wq, ws)^T) on the block-scaled matrix cores; operands as quant_mxfp8 returns them.
    Same epilogues and rounding points as gemm_nt (NONE, GELU, GATED_RESIDUAL; out may be the residual).
    out_mx: True or a (q, scales) pair to write into - the output leaves as MXFP8, bitwise quant_mxfp8 of the bf16 result, which is never
    written (g3_gemm_mxfp8_nt_mxout; NONE and GELU only); returns (q, scales)."""
    if out_mx is not None and out_mx is not False:
        return _gemm_mxfp8_nt_mxout(aq, as_, wq, ws, out_mx, epilogue, out, gate, residual)
    M, N, K, lda, ldas, ldw, ldws = _mx_operands("gemm_mxfp8_nt", aq, as_, wq, ws)
    out, ldc = _out_bf16(out, M, N, aq.device)
    epi = _gate_residual(gate, residual, M, N)
    f8 = torch.float8_e4m3fn
    with _gemm_timer("gemm_mxfp8_nt", M, N, K, epilogue):
        _lib.check(_lib.load().g3_gemm_mxfp8_nt(_dev(aq, "aq", f8), lda, _dev(as_, "as_", torch.uint8), ldas, _dev(wq, "wq", f8), ldw,
                                                _dev(ws, "ws", torch.uint8), ldws, _dev(out, "out"), ldc, M, N, K, epilogue, *epi, _stream()),
                   "g3_gemm_mxfp8_nt")
    return out


def quant_mxfp6(x: torch.Tensor, out=None):
    """MXFP6 (OCP MX, e2m3) of a bf16 [M, K] matrix: (q [M, 3K/4] torch.uint8 - 32 six-bit codes per 24 bytes -, scales [M, K/32] torch.uint8
    E8M0). out: an optional (q, scales) pair to write into. See g3_quant_mxfp6_bf16 for the rounding rule and the packing."""
    M, K, ldx = _rowmajor2d(x, "x")
    if out is None:
        out = (torch.empty((M, K // 4 * 3), dtype=torch.uint8, device=x.device), torch.empty((M, K // 32), dtype=torch.uint8, device=x.device))
    q, s = out
    Mq, Kq, ldq = _rowmajor2d(q, "q")
    Ms, Ks, lds = _rowmajor2d(s, "scales")
    if K % 32 or (Mq, Kq) != (M, K // 4 * 3) or (Ms, Ks) != (M, K // 32):
        raise _lib.Gen3cHipError(f"quant_mxfp6: output shapes {tuple(q.shape)} / {tuple(s.shape)} do not match x {tuple(x.shape)}")
    lib = _lib.load()
    _lib.check(lib.g3_quant_mxfp6_bf16(_dev(x, "x"), ldx, _dev(q, "q", torch.uint8), ldq, _dev(s, "scales", torch.uint8), lds, M, K,
                                       _stream()), "g3_quant_mxfp6_bf16")
    return q, s


def gemm_mxfp6_nt(aq: torch.Tensor, as_: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, out: Optional[torch.Tensor] = None,
                  epilogue: int = EPI_NONE, gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None):
    """out[M,N] = epi(dequant(aq, as_) @ dequant(wq, ws)^T) on the block-scaled matrix cores at the MXFP6 rate; operands as quant_mxfp6
    returns them. Same epilogues and rounding points as gemm_nt (NONE, GELU, GATED_RESIDUAL; out may be the residual)."""
    M, N, K, lda, ldas, ldw, ldws = _mx_operands("gemm_mxfp6_nt", aq, as_, wq, ws)
    out, ldc = _out_bf16(out, M, N, aq.device)
    epi = _gate_residual(gate, residual, M, N)
    u8 = torch.uint8
    with _gemm_timer("gemm_mxfp6_nt", M, N, K, epilogue):
        _lib.check(_lib.load().g3_gemm_mxfp6_nt(_dev(aq, "aq", u8), lda, _dev(as_, "as_", u8), ldas, _dev(wq, "wq", u8), ldw, _dev(ws, "ws", u8), ldws,
                                                _dev(out, "out"), ldc, M, N, K, epilogue, *epi, _stream()), "g3_gemm_mxfp6_nt")
    return out


def _mx_out_pair(out, M: int, K: int, device, what: str, of: Optional[str] = None):
    """The (q, scales) pair an MXFP8-producing op writes: allocated, or the caller's, checked against [M, K] (`of`: what the error text calls
    it). -> q, s, ldq, lds"""
    if out is None or out is True:
        out = (torch.empty((M, K), dtype=torch.float8_e4m3fn, device=device), torch.empty((M, K // 32), dtype=torch.uint8, device=device))
    q, s = out
    Mq, Kq, ldq = _rowmajor2d(q, "q")
    Ms, Ks, lds = _rowmajor2d(s, "scales")
    if (Mq, Kq) != (M, K) or (Ms, Ks) != (M, K // 32):
        raise _lib.Gen3cHipError(f"{what}: output shapes {tuple(q.shape)} / {tuple(s.shape)} do not match {of or f'[{M}, {K}]'}")
    return q, s, ldq, lds


def _gemm_mxfp8_nt_mxout(aq, as_, wq, ws, out_mx, epilogue, out, gate, residual):
    if out is not None or gate is not None or residual is not None:
        raise _lib.Gen3cHipError("gemm_mxfp8_nt: out_mx takes no bf16 out, gate or residual (epilogues NONE and GELU only)")
    M, N, K, lda, ldas, ldw, ldws = _mx_operands("gemm_mxfp8_nt", aq, as_, wq, ws)
    q, s, ldq, lds = _mx_out_pair(out_mx, M, N, aq.device, "gemm_mxfp8_nt")
    f8 = torch.float8_e4m3fn
    with _gemm_timer("gemm_mxfp8_nt_mxout", M, N, K, epilogue):
        _lib.check(_lib.load().g3_gemm_mxfp8_nt_mxout(_dev(aq, "aq", f8), lda, _dev(as_, "as_", torch.uint8), ldas, _dev(wq, "wq", f8), ldw,
                                                      _dev(ws, "ws", torch.uint8), ldws, _dev(q, "q", f8), ldq, _dev(s, "scales", torch.uint8), lds,
                                                      M, N, K, epilogue, _stream()), "g3_gemm_mxfp8_nt_mxout")
    return q, s


def gemv(a: torch.Tensor, w: torch.Tensor, add: Optional[torch.Tensor] = None, act_in: int = 0,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M<=8, N] = act_in(a) @ w^T (+ add)."""
    M, K, lda = _rowmajor2d(a, "a")
    N, Kw, ldw = _rowmajor2d(w, "w")
    assert K == Kw
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    ap, ldadd = 0, 0
    if add is not None:
        am, an, ldadd = _rowmajor2d(add, "add")
        assert (am, an) == (M, N)
        ap = _dev(add, "add")
    lib = _lib.load()
    _lib.check(lib.g3_gemv_bf16(_dev(a, "a"), lda, _dev(w, "w"), ldw, ap, ldadd, _dev(out, "out"), out.stride(0), M, N, K,
                                act_in, _stream()), "g3_gemv_bf16")
    return out


def _modulated(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor):
    """x [rows, D] and the AdaLN shift / scale [B, D] (one row stride) of a LayerNorm + modulate. -> rows, D, ldx, B, ldmod"""
    rows, D, ldx = _rowmajor2d(x, "x")
    B, Ds, ldmod = _rowmajor2d(shift, "shift")
    assert Ds == D and scale.shape == shift.shape and scale.stride(0) == ldmod
    return rows, D, ldx, B, ldmod


def _posemb_modulated(x, pe_t, pe_h, pe_w, pos_norm, T: int, Hp: int, Wp: int, B: int, shift, scale):
    """The operands both posemb_layernorm_modulate forms share, checked. -> rows, D, ldx, B of shift / scale, ldmod, the four table pointers"""
    rows, D, ldx, Bm, ldmod = _modulated(x, shift, scale)
    assert rows == T * Hp * Wp * B
    if pe_h is None:
        assert pe_w is None and pos_norm is None and pe_t.shape == (T * Hp * Wp, D) and pe_t.is_contiguous()
    else:
        for t, n in ((pe_t, T), (pe_h, Hp), (pe_w, Wp)):
            assert t.dim() == 2 and t.shape[0] >= n and t.shape[1] == D and t.is_contiguous()
        assert pos_norm.numel() == T * Hp * Wp and pos_norm.is_contiguous()
    tables = tuple(_dev(t, n) if t is not None else 0 for t, n in ((pe_t, "pe_t"), (pe_h, "pe_h"), (pe_w, "pe_w"), (pos_norm, "pos_norm")))
    return rows, D, ldx, Bm, ldmod, tables


def layernorm_modulate(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None,
                       eps: float = 1e-6) -> torch.Tensor:
    """x: [rows, D] (rows = (s, b), b fastest); shift/scale: [B, D]."""
    rows, D, ldx, B, ldmod = _modulated(x, shift, scale)
    if out is None:
        out = torch.empty((rows, D), dtype=torch.bfloat16, device=x.device)
    lib = _lib.load()
    _lib.check(lib.g3_layernorm_modulate_bf16(_dev(x, "x"), ldx, _dev(shift, "shift"), _dev(scale, "scale"), ldmod, B,
                                              _dev(out, "out"), out.stride(0), rows, D, eps, _stream()),
               "g3_layernorm_modulate_bf16")
    return out


def layernorm_modulate_mxfp8(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, out=None, eps: float = 1e-6):
    """layernorm_modulate with the result as MXFP8: returns (q [rows, D] float8_e4m3fn, scales [rows, D/32] uint8), bitwise
    quant_mxfp8(layernorm_modulate(x, shift, scale)) without the bf16 tensor in between. out: an optional (q, scales) pair to write into."""
    rows, D, ldx, B, ldmod = _modulated(x, shift, scale)
    q, s, ldq, lds = _mx_out_pair(out, rows, D, x.device, "layernorm_modulate_mxfp8")
    lib = _lib.load()
    _lib.check(lib.g3_layernorm_modulate_mxfp8(_dev(x, "x"), ldx, _dev(shift, "shift"), _dev(scale, "scale"), ldmod, B,
                                               _dev(q, "q", torch.float8_e4m3fn), ldq, _dev(s, "scales", torch.uint8), lds, rows, D, eps, _stream()),
               "g3_layernorm_modulate_mxfp8")
    return q, s


def posemb_layernorm_modulate(x: torch.Tensor, pe_t: torch.Tensor, pe_h: Optional[torch.Tensor], pe_w: Optional[torch.Tensor],
                              pos_norm: Optional[torch.Tensor], T: int, Hp: int, Wp: int, B: int, shift: torch.Tensor, scale: torch.Tensor,
                              out: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """x [T*Hp*Wp*B, D] += per-block absolute position embedding (IN PLACE), returns LayerNorm(x)*(1+scale)+shift.
    Either the three axis tables + norm (the kernel rebuilds every row), or pe_h = pe_w = pos_norm = None and pe_t the finished embedding
    [T*Hp*Wp, D] (one table read per row). See g3_posemb_layernorm_modulate_bf16."""
    rows, D, ldx, Bm, ldmod, tables = _posemb_modulated(x, pe_t, pe_h, pe_w, pos_norm, T, Hp, Wp, B, shift, scale)
    if out is None:
        out = torch.empty((rows, D), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().g3_posemb_layernorm_modulate_bf16(_dev(x, "x"), ldx, *tables, T, Hp, Wp, B, _dev(shift, "shift"), _dev(scale, "scale"), ldmod, Bm,
                                                             _dev(out, "out"), out.stride(0), D, eps, _stream()), "g3_posemb_layernorm_modulate_bf16")
    return out


def posemb_layernorm_modulate_mxfp8(x: torch.Tensor, pe_t: torch.Tensor, pe_h: Optional[torch.Tensor], pe_w: Optional[torch.Tensor],
                                    pos_norm: Optional[torch.Tensor], T: int, Hp: int, Wp: int, B: int, shift: torch.Tensor, scale: torch.Tensor,
                                    out=None, eps: float = 1e-6):
    """posemb_layernorm_modulate (x updated IN PLACE the same way) with the result as MXFP8: returns (q, scales) as layernorm_modulate_mxfp8."""
    rows, D, ldx, Bm, ldmod, tables = _posemb_modulated(x, pe_t, pe_h, pe_w, pos_norm, T, Hp, Wp, B, shift, scale)
    q, s, ldq, lds = _mx_out_pair(out, rows, D, x.device, "posemb_layernorm_modulate_mxfp8")
    _lib.check(_lib.load().g3_posemb_layernorm_modulate_mxfp8(_dev(x, "x"), ldx, *tables, T, Hp, Wp, B, _dev(shift, "shift"), _dev(scale, "scale"), ldmod, Bm,
                                                              _dev(q, "q", torch.float8_e4m3fn), ldq, _dev(s, "scales", torch.uint8), lds, D, eps, _stream()),
               "g3_posemb_layernorm_modulate_mxfp8")
    return q, s


def qk_rmsnorm_rope(x: torch.Tensor, weight: torch.Tensor, cos: Optional[torch.Tensor], sin: Optional[torch.Tensor],
                    S: int, B: int, H: int, out: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """x: [S*B, >=H*128] view (row stride arbitrary), per-head RMSNorm + optional RoPE -> out [S*B, H*128]."""
    rows, width, ld_in = _rowmajor2d(x, "x")
    assert rows == S * B and width == H * 128
    if out is None:
        out = torch.empty((rows, H * 128), dtype=torch.bfloat16, device=x.device)
    cp, sp = _rope_tables(cos, sin, S)
    lib = _lib.load()
    _lib.check(lib.g3_qk_rmsnorm_rope_bf16(_dev(x, "x"), ld_in, _dev(weight, "weight"), cp, sp, _dev(out, "out"),
                                           out.stride(0), S, B, H, 128, eps, _stream()), "g3_qk_rmsnorm_rope_bf16")
    return out


def qk_rmsnorm_rope_pair(x: torch.Tensor, weight_q: torch.Tensor, H_q: int, weight_k: torch.Tensor, H_k: int, cos: Optional[torch.Tensor],
                         sin: Optional[torch.Tensor], S: int, B: int, out: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """x: [S*B, (H_q + H_k)*128] view: heads [0, H_q) normalised with weight_q, the next H_k with weight_k, RoPE on all of them - q | k of the fused QKV
    buffer in ONE launch (g3_qk_rmsnorm_rope_pair_bf16). out=None: in place."""
    rows, width, ld_in = _rowmajor2d(x, "x")
    assert rows == S * B and width == (H_q + H_k) * 128
    if out is None:
        out = x
    cp, sp = _rope_tables(cos, sin, S)
    lib = _lib.load()
    _lib.check(lib.g3_qk_rmsnorm_rope_pair_bf16(_dev(x, "x"), ld_in, _dev(weight_q, "weight_q"), H_q, _dev(weight_k, "weight_k"), H_k, cp, sp, _dev(out, "out"),
                                                out.stride(0), S, B, 128, eps, _stream()), "g3_qk_rmsnorm_rope_pair_bf16")
    return out


def gemm_qk_norm_rope(a: torch.Tensor, w: torch.Tensor, n_q: int, n_k: int, norm_q: Optional[torch.Tensor], norm_k: Optional[torch.Tensor],
                      cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], S: int, B: int, out: Optional[torch.Tensor] = None,
                      eps: float = 1e-6, vt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = a @ w^T with per-head RMSNorm (+ RoPE) applied to the feature ranges [0, n_q) (weight norm_q) and [n_q, n_q+n_k) (norm_k)
    in the GEMM epilogue; the remaining features (v) are stored as they are - or, with `vt` ([B, H_v, 128, ld] bf16, ld >= S, tail zero),
    written transposed into it instead (their columns of `out` then stay unwritten). Replaces gemm_nt + qk_rmsnorm_rope (+ transpose_v)."""
    M, K, lda = _rowmajor2d(a, "a")
    N, Kw, ldw = _rowmajor2d(w, "w")
    assert K == Kw and M == S * B
    out, ldc = _out_bf16(out, M, N, a.device)
    cp, sp = _rope_tables(cos, sin, S)
    vtp, vt_ld = 0, 0
    if vt is not None:
        n_v = N - n_q - n_k
        assert n_v > 0 and vt.dim() == 4 and vt.shape[:3] == (B, n_v // 128, 128) and vt.shape[3] >= S and vt.is_contiguous()
        vtp, vt_ld = _dev(vt, "vt"), vt.shape[3]
    with _gemm_timer("gemm_nt", M, N, K, 5):  # (collected with the block GEMMs, under an epilogue number of its own)
        _lib.check(_lib.load().g3_gemm_qk_norm_rope_bf16(_dev(a, "a"), lda, _dev(w, "w"), ldw, _dev(out, "out"), ldc, M, N, K, n_q, n_k,
                                                         _dev(norm_q, "norm_q") if n_q else 0, _dev(norm_k, "norm_k") if n_k else 0, cp, sp, B, eps,
                                                         vtp, vt_ld, _stream()), "g3_gemm_qk_norm_rope_bf16")
    return out


def ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def transpose_v(v: torch.Tensor, S: int, B: int, H: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """v: [S*B, H*128] view -> V^T [B, H, 128, ceil64(S)] with a zero tail."""
    rows, width, ld_in = _rowmajor2d(v, "v")
    assert rows == S * B and width == H * 128
    ldvt = ceil_to(S, 64)
    if out is None:
        out = torch.empty((B, H, 128, ldvt), dtype=torch.bfloat16, device=v.device)
    assert out.shape == (B, H, 128, ldvt) and out.is_contiguous()
    lib = _lib.load()
    _lib.check(lib.g3_transpose_v_bf16(_dev(v, "v"), ld_in, _dev(out, "out"), ldvt, S, B, H, 128, _stream()),
               "g3_transpose_v_bf16")
    return out


def cp_scatter_heads(q: Optional[torch.Tensor], k: Optional[torch.Tensor], v: Optional[torch.Tensor], H: int, n_dest: int, head0: int, Hg: int,
                     out=None):
    """Send layout of the head-parallel exchange (g3_cp_scatter_heads_bf16). q, k, v: [rows, H*128] column views of ONE buffer (the same row
    stride; any of them None) -> per given tensor a contiguous [n_dest, rows, Hg*128]: destination d's block holds the heads
    d * (H / n_dest) + head0 .. + Hg of every row. Returns (q_out, k_out, v_out), None where the input is None. out: the same triple to write into."""
    given = [t for t in (q, k, v) if t is not None]
    if not given:
        raise _lib.Gen3cHipError("cp_scatter_heads: q, k and v are all None")
    rows, width, ld = _rowmajor2d(given[0], "q/k/v")
    for t in given:
        if _rowmajor2d(t, "q/k/v") != (rows, width, ld) or t.device != given[0].device:
            raise _lib.Gen3cHipError("cp_scatter_heads: q, k and v must be column views of one buffer (same shape, row stride and device)")
    if width != H * 128:
        raise _lib.Gen3cHipError(f"cp_scatter_heads: expected {H * 128} columns, got {width}")
    if out is None:
        out = tuple(None if t is None else torch.empty((n_dest, rows, Hg * 128), dtype=torch.bfloat16, device=t.device) for t in (q, k, v))
    for t, o in zip((q, k, v), out):
        if t is not None and (o is None or tuple(o.shape) != (n_dest, rows, Hg * 128) or not o.is_contiguous()):
            raise _lib.Gen3cHipError(f"cp_scatter_heads: every output must be a contiguous {(n_dest, rows, Hg * 128)} tensor")
    ptr = lambda t, name: 0 if t is None else _dev(t, name)
    _lib.check(_lib.load().g3_cp_scatter_heads_bf16(ptr(q, "q"), ptr(k, "k"), ptr(v, "v"), ld, *(ptr(o if t is not None else None, "out") for t, o in zip((q, k, v), out)),
                                                    rows, H, n_dest, head0, Hg, _stream()), "g3_cp_scatter_heads_bf16")
    return tuple(o if t is not None else None for t, o in zip((q, k, v), out))


def cp_gather_heads(x: torch.Tensor, out: torch.Tensor, H: int, head0: int) -> torch.Tensor:
    """Inverse of cp_scatter_heads for one tensor (g3_cp_gather_heads_bf16): x [n_src, rows, Hg*128] contiguous, as the returning all-to-all
    delivers it, into the columns (s * (H / n_src) + head0) * 128 .. of out [rows, H*128] (a view with any row stride); other columns stay."""
    if x.dim() != 3 or not x.is_contiguous() or x.shape[2] % 128:
        raise _lib.Gen3cHipError(f"cp_gather_heads: expected a contiguous [n_src, rows, Hg*128] tensor, got {tuple(x.shape)} strides {x.stride()}")
    n_src, rows, W = x.shape
    orows, width, ld = _rowmajor2d(out, "out")
    if (orows, width) != (rows, H * 128):
        raise _lib.Gen3cHipError(f"cp_gather_heads: out must be [{rows}, {H * 128}], got {tuple(out.shape)}")
    _lib.check(_lib.load().g3_cp_gather_heads_bf16(_dev(x, "x"), _dev(out, "out"), ld, rows, H, n_src, head0, W // 128, _stream()), "g3_cp_gather_heads_bf16")
    return out


def flash_attn(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, Sq: int, Skv: int, B: int, H: int,
               out: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None, variant: int = 0, partial: bool = False, kv_dense: int = 0,
               q_norm_weight: Optional[torch.Tensor] = None, q_norm_eps: float = 1e-6, carry=None, kv_skip=None):
    """q: [Sq*B, H*128], k: [Skv*B, H*128] (rows (s,b), b fastest), vt: [B, H, 128, ldvt] -> out [Sq*B, H*128].
    vt may also be 5-D [n_seg, B, H, 128, ld_seg]: V^T in key segments of Skv / n_seg keys each (a rank-major all-gather of
    per-rank V^T shards, see g3_flash_attn_fwd_kvseg_bf16).
    variant: per-call kernel choice (0 = library option / automatic; 4 = 8-wave kernel, 11 = one-wave-per-SIMD kernel) - no global state.
    partial=True: the keys are only PART of the rows' keys - returns (o_part fp32 [Sq*B, H*128], lse fp32 [B, H, Sq]) for attn_merge.
    kv_dense (0 < kv_dense < Skv): the CALLER guarantees all-zero K rows and V^T columns for keys [kv_dense, Skv) (zero-padded context tokens): they enter the
    softmax in closed form instead of through the tile loop; q_norm_weight ([128] bf16): q is the raw projection and its per-head RMSNorm runs inside the
    kernel's Q load (both: g3_cross_attn_fwd_bf16).
    carry=(o_part, lse): an earlier state of the same rows (what partial=True returns; o_part with the strides of this call's output) that the
    kernel folds into its own part - the result is the attention over both key sets, as bf16 or (partial=True) as a new (o_part, lse), so launches
    chain without a merge pass. kv_skip=(begin, len), multiples of 64: k / vt hold Skv + len keys and keys [begin, begin + len) are skipped (Skv
    counts the attended keys). partial=True may then also take `out`, an fp32 view to write the part into (it may be carry's o_part).
    Either one (or partial=True with `out`) runs g3_flash_attn_fwd_carry_bf16 - variant 0, 4 or 11 only; no fallback."""
    if carry is not None or kv_skip is not None or (partial and out is not None):
        return _attn_call("carry", q, k, vt, Sq, Skv, B, H, out, softmax_scale, variant, partial, carry=carry, kv_skip=kv_skip)
    if 0 < kv_dense < Skv or q_norm_weight is not None:
        assert not partial and vt.dim() == 4 and not variant, "the cross-attention form takes plain V^T, a bf16 output and the automatic kernel choice"
        return _attn_call("cross", q, k, vt, Sq, Skv, B, H, out, softmax_scale, 0, False, kv_dense=int(kv_dense) if 0 < kv_dense < Skv else 0,
                          q_norm_weight=q_norm_weight, q_norm_eps=q_norm_eps)
    return _attn_call("ex", q, k, vt, Sq, Skv, B, H, out, softmax_scale, variant, partial)


def self_attn_bounded(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, Sq: int, Skv: int, B: int, H: int, logit_bound: float,
                      out: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None, variant: int = 0, partial: bool = False, carry=None, kv_skip=None,
                      mfma16: bool = False):
    """flash_attn (operands, `out`, `variant` and `partial` as there) for callers that guarantee
    |q . k| * softmax_scale <= logit_bound for every query / key pair, e.g. q and k behind a per-head RMSNorm:
    |q . k| / sqrt(128) <= sqrt(128) * max|w_q| * max|w_k|. Where the one-wave-per-SIMD kernel (variant 11) is the choice and
    0 < logit_bound * log2(e) <= 60 it runs without its running row maximum (g3_self_attn_fwd_bounded_bf16); every other call is flash_attn's.
    The key-sharded forms of flash_attn - 5-D segmented V^T, carry=, kv_skip=, partial=True with `out` - go to g3_self_attn_fwd_bounded_cp_bf16:
    the no-max kernels where they apply (variant 11, the bound in range), else exactly flash_attn's carry call (variant 0, 4 or 11 only).
    mfma16=True: g3_self_attn_fwd_bounded16_bf16 - the no-max kernel's tile loop on 16x16x32 MFMAs where the plain no-max kernel would run with a bf16
    output (equal to rounding, not bit for bit); every other call, the key-sharded forms included, is the call without the flag."""
    if vt.dim() == 5 or carry is not None or kv_skip is not None or (partial and out is not None):
        return _attn_call("bounded_cp", q, k, vt, Sq, Skv, B, H, out, softmax_scale, variant, partial, carry=carry, kv_skip=kv_skip, logit_bound=logit_bound)
    return _attn_call("bounded16" if mfma16 else "bounded", q, k, vt, Sq, Skv, B, H, out, softmax_scale, variant, partial, logit_bound=logit_bound)


def self_attn_window(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, S: int, B: int, H: int, logit_bound: float, frame_len: int, window_frames: int,
                     sink_frames: int, out: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None):
    """Self-attention over a temporal frame window (opt-in local attention; g3_self_attn_fwd_window_bf16): q, k [S*B, H*128] with tokens ordered
    (t, h, w), frame_len tokens per latent frame, vt plain [B, H, 128, ldvt]. Each block of window_q_rows() query rows attends the keys of the frames
    within window_frames of its rows' frames and of the first sink_frames frames - window_attn_mask is the function - and the output is the exact
    softmax over those keys. logit_bound as for self_attn_bounded (out of range: the running-maximum form of the same kernel). A window that covers
    every key is self_attn_bounded(variant=11), bit for bit. The one-wave-per-SIMD kernel's operand rules; no fallback."""
    return _attn_call("window", q, k, vt, S, S, B, H, out, softmax_scale, 11, False, logit_bound=logit_bound,
                      window=(int(frame_len), int(window_frames), int(sink_frames)))


def self_attn_window_cp(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, Sq: int, Skv_buf: int, B: int, H: int, logit_bound: float, frame_len: int,
                        total_frames: int, q_frame0: int, buf_head_frames: int, buf_tail_frame0: int, window_frames: int, sink_frames: int,
                        out: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None):
    """self_attn_window for one rank under key sharding (g3_self_attn_fwd_window_cp_bf16): q [Sq*B, H*128] are the rank's own rows, global frames
    [q_frame0, q_frame0 + Sq / frame_len) of total_frames; k [Skv_buf*B, H*128] and plain vt [B, H, 128, ldvt] are a compact buffer of the global
    frames [0, buf_head_frames) ++ [buf_tail_frame0, c) in ascending order (parallel.window_halo_plan makes the tight one). The function is
    window_attn_mask(..., q_row0=q_frame0 * frame_len, T_total=total_frames): where q_frame0 * frame_len is a multiple of window_q_rows() the rows
    equal self_attn_window on the whole sequence, bit for bit. The launcher refuses a buffer that misses a key some block attends; no fallback."""
    return _attn_call("window_cp", q, k, vt, Sq, Skv_buf, B, H, out, softmax_scale, 11, False, logit_bound=logit_bound,
                      window=(int(frame_len), int(window_frames), int(sink_frames)),
                      window_cp=(int(total_frames), int(q_frame0), int(buf_head_frames), int(buf_tail_frame0)))


class AttnRangeTable:
    """A validated range table of self_attn_ranges (attn_range_table makes it): `ranges` int32 [n_patterns, n_qblk, max_ranges, 2] and `head_pattern`
    (int32 [H] or None) on the host, `ranges_dev` / `head_pattern_dev` their copies on the device, and (`attended`, `dense`): the (head, query
    block, 64-key tile) triples a launch with H heads visits and the dense launch's count."""
    __slots__ = ("ranges", "head_pattern", "ranges_dev", "head_pattern_dev", "S", "H", "n_patterns", "max_ranges", "attended", "dense", "profile")

    @property
    def tile_density(self) -> float:
        return self.attended / self.dense


def attn_range_table(ranges, S: int, head_pattern=None, H: Optional[int] = None, device=None) -> AttnRangeTable:
    """ranges: a HOST int32 array [n_patterns, ceil(S / window_q_rows()), max_ranges, 2] of (first_key, n_keys) pairs (numpy or torch; the rules:
    include/gen3c_hip.h, the builders: gen3c_amd/sparse_attn.py); head_pattern: the pattern of each of the H heads (default: pattern 0 for every
    head, H = 1 if not given - H only scales the tile counts). Validated by g3_attn_ranges_check - a table that breaks a rule raises with the
    pattern, block and range named - and uploaded ONCE to `device` (default: the current GPU); every self_attn_ranges launch reuses the copy."""
    import ctypes
    import numpy as np
    host = ranges.cpu() if isinstance(ranges, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ranges))
    if host.dtype != torch.int32:
        raise ValueError(f"attn_range_table: the table must be an int32 array, got {host.dtype}")
    n_qblk = -(-int(S) // window_q_rows()) if S > 0 else 0
    if host.dim() != 4 or host.shape[1] != n_qblk or host.shape[3] != 2:
        raise ValueError(f"attn_range_table: expected [n_patterns, {n_qblk}, max_ranges, 2] for S = {S}, got {tuple(host.shape)}")
    if not 1 <= host.shape[2] <= 64:
        raise ValueError(f"attn_range_table: max_ranges {host.shape[2]} outside [1, 64]")
    host = host.contiguous()
    hp = None
    if head_pattern is not None:
        hp = torch.as_tensor(head_pattern, dtype=torch.int32).cpu().contiguous().flatten()
        if H is not None and int(H) != hp.numel():
            raise ValueError(f"attn_range_table: head_pattern has {hp.numel()} entries, H is {H}")
        H = hp.numel()
    H = 1 if H is None else int(H)
    att, dense = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().g3_attn_ranges_check(host.data_ptr(), host.shape[0], int(S), host.shape[2], hp.data_ptr() if hp is not None else None, H,
                                                ctypes.byref(att), ctypes.byref(dense)), "g3_attn_ranges_check")
    t = AttnRangeTable()
    t.ranges, t.head_pattern, t.S, t.H, t.n_patterns, t.max_ranges = host, hp, int(S), H, host.shape[0], host.shape[2]
    t.attended, t.dense = att.value, dense.value
    t.profile = None  # (the DiT's auto mode hangs its AttnProfilePlan and per-block choices here)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    t.ranges_dev = host.to(dev)
    t.head_pattern_dev = hp.to(dev) if hp is not None else None
    return t


def self_attn_ranges(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, S: int, B: int, H: int, logit_bound: float, table: AttnRangeTable,
                     out: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None, head_pattern_dev: Optional[torch.Tensor] = None):
    """Self-attention over a range table (opt-in sparse attention; g3_self_attn_fwd_ranges_bf16): q, k [S*B, H*128] with tokens ordered (t, h, w), vt
    plain [B, H, 128, ldvt], table from attn_range_table for this S (and, with a head_pattern, this H). Every block of window_q_rows() query rows
    attends the keys of its list in the pattern of its head - ranges_attn_mask is the function - and the output is the exact softmax over those
    keys. logit_bound as for self_attn_bounded (out of range: the running-maximum form of the same kernel). The one-wave-per-SIMD kernel's
    operand rules; no fallback. head_pattern_dev: a DEVICE int32 [H] that takes the place of the table's own head_pattern_dev for this launch (what
    attn_pattern_profile wrote, in stream order; the kernel clamps its values to the table's patterns)."""
    if not isinstance(table, AttnRangeTable):
        raise ValueError("self_attn_ranges: table must come from ops.attn_range_table (which validates it)")
    if table.S != S or (table.head_pattern is not None and table.H != H):
        raise ValueError(f"self_attn_ranges: the table was made for S = {table.S}, H = {table.H}; the call has S = {S}, H = {H}")
    if table.ranges_dev.device != q.device:
        raise ValueError(f"self_attn_ranges: the table lives on {table.ranges_dev.device}, q on {q.device}")
    if head_pattern_dev is not None:
        if (head_pattern_dev.dtype != torch.int32 or head_pattern_dev.numel() != H or not head_pattern_dev.is_contiguous()
                or head_pattern_dev.device != q.device):
            raise ValueError(f"self_attn_ranges: head_pattern_dev must be a contiguous int32 [{H}] on {q.device}")
    return _attn_call("ranges", q, k, vt, S, S, B, H, out, softmax_scale, 11, False, logit_bound=logit_bound, ranges=table,
                      head_pattern_dev=head_pattern_dev)


class AttnProfilePlan:
    """What attn_pattern_profile needs besides q and k (attn_profile_plan makes it): the table, the n sample rows and the per-tile membership bytes
    [n, S / 64] on host and device, and - allocated at the first call for its (B, H, n_chunks) - the workspace and the results `recall` float32
    [B, H, n, n_patterns], `score` float32 [H, n_patterns] and `head_pattern` int32 [H], all on the device."""
    __slots__ = ("table", "n", "sample_rows", "sample_rows_dev", "member", "member_dev", "workspace", "recall", "score", "head_pattern", "n_chunks")


def attn_profile_plan(table: AttnRangeTable, n_samples: int = 64, sample_rows=None) -> AttnProfilePlan:
    """The sample rows (default: n_samples rows spread evenly, ((2i + 1) * S) // (2n)) and the bitmask g3_attn_profile_members makes of the table
    for them, built and uploaded ONCE to the table's device."""
    if not isinstance(table, AttnRangeTable):
        raise ValueError("attn_profile_plan: table must come from ops.attn_range_table (which validates it)")
    S = table.S
    if sample_rows is None:
        n = int(n_samples)
        if not 1 <= n <= min(64, S):
            raise ValueError(f"attn_profile_plan: n_samples {n} outside [1, min(64, S = {S})]")
        sample_rows = [((2 * i + 1) * S) // (2 * n) for i in range(n)]
    rows = torch.as_tensor(sample_rows, dtype=torch.int32).cpu().contiguous().flatten()
    n = rows.numel()
    member = torch.zeros((max(n, 1), S // 64), dtype=torch.uint8)
    _lib.check(_lib.load().g3_attn_profile_members(table.ranges.data_ptr(), table.n_patterns, S, table.max_ranges, rows.data_ptr(), n, member.data_ptr()),
               "g3_attn_profile_members")
    p = AttnProfilePlan()
    p.table, p.n, p.sample_rows, p.member = table, n, rows, member
    dev = table.ranges_dev.device
    p.sample_rows_dev, p.member_dev = rows.to(dev), member.to(dev)
    p.workspace = p.recall = p.score = p.head_pattern = None
    p.n_chunks = 0
    return p


def attn_profile_chunks(S: int, B: int, H: int) -> int:
    return _lib.load().g3_attn_profile_chunks(S, B, H)


def attn_pattern_profile(q: torch.Tensor, k: torch.Tensor, S: int, B: int, H: int, plan: AttnProfilePlan, softmax_scale: Optional[float] = None,
                         n_chunks: Optional[int] = None, head_pattern_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per head, the pattern of plan.table that keeps most of the softmax mass of the plan's sample rows (g3_attn_pattern_profile_bf16 +
    g3_attn_pattern_select; the function: include/gen3c_hip.h): q, k [S*B, H*128] as for self_attn_ranges (column views of a fused buffer are
    fine). Returns the DEVICE int32 [H] head_pattern (plan.head_pattern, or head_pattern_out where given) with plan.recall and plan.score filled -
    everything on the current stream, nothing read back."""
    if not isinstance(plan, AttnProfilePlan):
        raise ValueError("attn_pattern_profile: plan must come from ops.attn_profile_plan")
    t = plan.table
    if t.S != S:
        raise ValueError(f"attn_pattern_profile: the plan was made for S = {t.S}; the call has S = {S}")
    if t.ranges_dev.device != q.device:
        raise ValueError(f"attn_pattern_profile: the plan lives on {t.ranges_dev.device}, q on {q.device}")
    qr, qw, ldq = _rowmajor2d(q, "q")
    kr, kw, ldk = _rowmajor2d(k, "k")
    assert qr == S * B and kr == S * B and qw == H * 128 and kw == H * 128
    lib = _lib.load()
    nc = int(n_chunks) if n_chunks is not None else lib.g3_attn_profile_chunks(S, B, H)
    if plan.recall is None or tuple(plan.recall.shape[:2]) != (B, H) or plan.n_chunks < nc:
        plan.workspace = torch.empty(max(lib.g3_attn_profile_workspace_bytes(B, H, max(nc, 1)) // 4, 1), dtype=torch.float32, device=q.device)
        plan.recall = torch.empty((B, H, plan.n, t.n_patterns), dtype=torch.float32, device=q.device)
        plan.score = torch.empty((H, t.n_patterns), dtype=torch.float32, device=q.device)
        plan.head_pattern = torch.empty(H, dtype=torch.int32, device=q.device)
        plan.n_chunks = max(nc, 1)
    hp = plan.head_pattern if head_pattern_out is None else head_pattern_out
    if hp.dtype != torch.int32 or hp.numel() != H or not hp.is_contiguous() or hp.device != q.device:
        raise ValueError(f"attn_pattern_profile: head_pattern_out must be a contiguous int32 [{H}] on {q.device}")
    scale = float(1.0 / math.sqrt(128) if softmax_scale is None else softmax_scale)
    _lib.check(lib.g3_attn_pattern_profile_bf16(_dev(q, "q"), ldq * B, ldq, 128, _dev(k, "k"), ldk * B, ldk, 128, S, B, H, 128, scale,
                                                _dev(plan.sample_rows_dev, "sample_rows", torch.int32), plan.n,
                                                _dev(plan.member_dev, "tile_member", torch.uint8), t.n_patterns, nc,
                                                _dev(plan.workspace, "workspace", torch.float32), plan.workspace.numel() * 4,
                                                _dev(plan.recall, "recall", torch.float32), _stream()), "g3_attn_pattern_profile_bf16")
    _lib.check(lib.g3_attn_pattern_select(_dev(plan.recall, "recall", torch.float32), B, H, plan.n, t.n_patterns, _dev(plan.score, "score", torch.float32),
                                          _dev(hp, "head_pattern", torch.int32), _stream()), "g3_attn_pattern_select")
    return hp


def ranges_attn_mask(table_or_array, S: int, pattern: int = 0) -> torch.Tensor:
    """CPU bool [S, S]: mask[i, j] = query row i attends key j under self_attn_ranges with `pattern` - the written-down definition of the function
    (gen3c_hip.h): row i lies in query block i // window_q_rows(), whose list of (first_key, n_keys) ranges ends at the first n_keys == 0."""
    import numpy as np
    tab = table_or_array.ranges if isinstance(table_or_array, AttnRangeTable) else table_or_array
    tab = tab if isinstance(tab, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tab))
    q_rows = window_q_rows()
    mask = torch.zeros(S, S, dtype=torch.bool)
    for b, rl in enumerate(tab[pattern].tolist()):
        for first, n in rl:
            if n == 0:
                break
            mask[b * q_rows:(b + 1) * q_rows, first:first + n] = True
    return mask


def window_q_rows() -> int:
    """Query rows per block of the window form's key sets (the kernel's workgroup)."""
    return _lib.load().g3_self_attn_window_q_rows()


def window_attn_tiles(S: int, frame_len: int, window_frames: int, sink_frames: int):
    """(attended, dense): the (query block, 64-key tile) pairs a self_attn_window launch visits and the dense launch's count."""
    import ctypes
    att, dense = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().g3_self_attn_window_tiles(S, frame_len, window_frames, sink_frames, ctypes.byref(att), ctypes.byref(dense)), "g3_self_attn_window_tiles")
    return att.value, dense.value


def window_attn_tiles_cp(Sq: int, Skv_buf: int, frame_len: int, total_frames: int, q_frame0: int, buf_head_frames: int, buf_tail_frame0: int,
                         window_frames: int, sink_frames: int):
    """(attended, dense) of one rank's self_attn_window_cp launch: the (query block, 64-key tile) pairs it visits, and its query blocks times the
    tiles of the whole sequence. Raises on everything the launch refuses."""
    import ctypes
    att, dense = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().g3_self_attn_window_cp_tiles(Sq, Skv_buf, frame_len, total_frames, q_frame0, buf_head_frames, buf_tail_frame0, window_frames,
                                                        sink_frames, ctypes.byref(att), ctypes.byref(dense)), "g3_self_attn_window_cp_tiles")
    return att.value, dense.value


def window_attn_mask(S: int, frame_len: int, window_frames: int, sink_frames: int, q_rows: Optional[int] = None, q_row0: int = 0,
                     T_total: Optional[int] = None) -> torch.Tensor:
    """CPU bool [S, S]: mask[i, j] = query row i attends key j under self_attn_window - the written-down definition of the function (gen3c_hip.h).
    With T = S / frame_len frames, the block of q_rows (default window_q_rows()) query rows that holds row i lies in frames f0..f1 and attends the
    keys of frames [max(0, f0 - W), min(T, f1 + W + 1)) and of frames [0, min(s, T)): block-granular, a superset of row i's own window.
    With T_total (and q_row0, a multiple of frame_len): one rank's mask under key sharding, bool [S, T_total * frame_len] - the S query rows are the
    global rows [q_row0, q_row0 + S), blocked from the rank's own row 0, over the keys of all T_total frames (self_attn_window_cp)."""
    if T_total is not None or q_row0:
        if T_total is None:
            raise ValueError("window_attn_mask: q_row0 needs T_total")
        if S <= 0 or frame_len <= 0 or S % frame_len or q_row0 < 0 or q_row0 % frame_len or q_row0 + S > T_total * frame_len or window_frames < 0 or sink_frames < 0:
            raise ValueError(f"window_attn_mask: S {S} and q_row0 {q_row0} must be multiples of frame_len {frame_len} (S positive) within T_total {T_total} "
                             f"frames, window_frames {window_frames} and sink_frames {sink_frames} >= 0")
    elif S <= 0 or frame_len <= 0 or S % frame_len or window_frames < 0 or sink_frames < 0:
        raise ValueError(f"window_attn_mask: S {S} must be a positive multiple of frame_len {frame_len}, window_frames {window_frames} and sink_frames {sink_frames} >= 0")
    else:
        T_total = S // frame_len  # the single-GPU form: the rows are the whole sequence
    q_rows = window_q_rows() if q_rows is None else q_rows
    r0 = torch.arange(S) // q_rows * q_rows  # first row of every row's block
    f0 = (r0 + q_row0) // frame_len
    f1 = (torch.clamp(r0 + q_rows, max=S) - 1 + q_row0) // frame_len
    kf = torch.arange(T_total * frame_len) // frame_len  # frame of every key
    lo, hi = torch.clamp(f0 - window_frames, min=0), torch.clamp(f1 + window_frames + 1, max=T_total)
    return ((kf[None, :] >= lo[:, None]) & (kf[None, :] < hi[:, None])) | (kf[None, :] < min(sink_frames, T_total))


# The launching entry points ops uses: (enum g3_attn_entry, symbol, its arguments by name in call order - the stream follows -, the symbol of its dry run,
# that one's arguments). g3_attn_plan_bf16 takes the entry and the union of the arguments (_ATTN_PLAN), so the kernel a timer records is the dry run's
# answer for the very arguments launched ("bounded16": g3_attn_plan16_bf16, the dry run in which entry 4 stands for g3_self_attn_fwd_bounded16_bf16).
# The window and range-table entries have no value of enum g3_attn_entry: their dry runs take exactly the call's arguments.
_AQ, _AK, _AVT = ("q", "q_row", "q_batch", "q_head"), ("k", "k_row", "k_batch", "k_head"), ("vt", "vt_row", "vt_batch", "vt_head", "vt_seg_len", "vt_seg_stride")
_AOUT, _ASHAPE = ("o", "o_partial", "lse", "o_row", "o_batch", "o_head"), ("Sq", "Skv", "B", "H", "head_dim", "softmax_scale")
_ACP = ("kv_skip_begin", "kv_skip_len", "carry_o", "carry_lse")
_ATTN_PLAN = ("g3_attn_plan_bf16", ("entry",) + _AQ + ("q_norm_weight", "q_norm_eps") + _AK + _AVT + _ACP + _AOUT + ("Sq", "Skv", "kv_dense") + _ASHAPE[2:] +
              ("logit_bound", "variant"))
_ABOUNDED = _AQ + _AK + _AVT + _AOUT + _ASHAPE + ("logit_bound", "variant")
_AWINDOW = _AQ + _AK + _AVT[:4] + ("o", "o_row", "o_batch", "o_head", "Sq") + _ASHAPE[2:] + ("logit_bound", "frame_len", "window_frames", "sink_frames")
_AWINDOW_CP = _AQ + _AK + _AVT[:4] + ("o", "o_row", "o_batch", "o_head") + _ASHAPE + ("logit_bound", "frame_len", "total_frames", "q_frame0", "buf_head_frames",
                                                                                   "buf_tail_frame0", "window_frames", "sink_frames")
_ARANGES = _AQ + _AK + _AVT[:4] + ("o", "o_row", "o_batch", "o_head", "Sq") + _ASHAPE[2:] + ("logit_bound", "ranges", "n_patterns", "max_ranges", "head_pattern")
_ATTN_ENTRIES = {
    "cross": (2, "g3_cross_attn_fwd_bf16", _AQ + ("q_norm_weight", "q_norm_eps") + _AK + _AVT[:4] + ("o", "o_row", "o_batch", "o_head", "Sq", "Skv", "kv_dense") + _ASHAPE[2:]) + _ATTN_PLAN,
    "ex": (3, "g3_flash_attn_fwd_ex_bf16", _AQ + _AK + _AVT + _AOUT + _ASHAPE + ("variant",)) + _ATTN_PLAN,
    "bounded": (4, "g3_self_attn_fwd_bounded_bf16", _ABOUNDED) + _ATTN_PLAN,
    "bounded16": (4, "g3_self_attn_fwd_bounded16_bf16", _ABOUNDED, "g3_attn_plan16_bf16", _ATTN_PLAN[1]),
    "carry": (5, "g3_flash_attn_fwd_carry_bf16", _AQ + _AK + _AVT + _ACP + _AOUT + _ASHAPE + ("variant",)) + _ATTN_PLAN,
    "bounded_cp": (6, "g3_self_attn_fwd_bounded_cp_bf16", _AQ + _AK + _AVT + _ACP + _AOUT + _ASHAPE + ("logit_bound", "variant")) + _ATTN_PLAN,
    "window": (None, "g3_self_attn_fwd_window_bf16", _AWINDOW, "g3_attn_window_plan_bf16", _AWINDOW),
    "window_cp": (None, "g3_self_attn_fwd_window_cp_bf16", _AWINDOW_CP, "g3_attn_window_cp_plan_bf16", _AWINDOW_CP),
    "ranges": (None, "g3_self_attn_fwd_ranges_bf16", _ARANGES, "g3_attn_ranges_plan_bf16", _ARANGES),
}


def _attn_call(entry, q, k, vt, Sq, Skv, B, H, out, softmax_scale, variant, partial, kv_dense=0, q_norm_weight=None, q_norm_eps=0.0, carry=None, kv_skip=None,
               logit_bound=0.0, window=None, window_cp=None, ranges=None, head_pattern_dev=None):
    """The one marshaller of flash_attn, self_attn_bounded, self_attn_window, self_attn_window_cp and self_attn_ranges, which only choose the C entry point: shape checks, outputs, the entry's arguments, the
    launch and the kernel timer."""
    skip_begin, skip_len = (int(kv_skip[0]), int(kv_skip[1])) if kv_skip is not None else (0, 0)
    skv_all = Skv + skip_len  # keys the operands hold
    qr, qw, ldq = _rowmajor2d(q, "q")
    kr, kw, ldk = _rowmajor2d(k, "k")
    assert qr == Sq * B and kr == skv_all * B and qw == H * 128 and kw == H * 128
    assert vt.is_contiguous() and vt.dim() in (4, 5) and tuple(vt.shape[-4:-1]) == (B, H, 128)
    ldvt = vt.shape[-1]
    n_seg = vt.shape[0] if vt.dim() == 5 else 0
    if n_seg:
        assert skv_all % n_seg == 0
    lse = None
    if partial:
        if out is None:
            out = torch.empty((Sq * B, H * 128), dtype=torch.float32, device=q.device)
        assert out.dtype == torch.float32, "partial=True writes fp32"
        lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    out, ldo = _out_bf16(out, Sq * B, H * 128, q.device)  # (partial: the fp32 part from above, only checked)
    co = cl = 0
    if carry is not None:
        o_c, l_c = carry
        if o_c.dtype != torch.float32 or o_c.shape != (Sq * B, H * 128) or o_c.stride() != out.stride():
            raise ValueError(f"flash_attn: carry o_part must be fp32 {(Sq * B, H * 128)} with the output's strides {out.stride()} "
                             f"(got {o_c.dtype} {tuple(o_c.shape)} {o_c.stride()})")
        if l_c.dtype != torch.float32 or l_c.shape != (B, H, Sq) or not l_c.is_contiguous():
            raise ValueError(f"flash_attn: carry lse must be contiguous fp32 {(B, H, Sq)}")
        co, cl = _dev(o_c, "carry_o", torch.float32), _dev(l_c, "carry_lse", torch.float32)
    a = dict(q=_dev(q, "q"), q_row=ldq * B, q_batch=ldq, q_head=128, q_norm_weight=_dev(q_norm_weight, "q_norm_weight") if q_norm_weight is not None else 0,
             q_norm_eps=float(q_norm_eps), k=_dev(k, "k"), k_row=ldk * B, k_batch=ldk, k_head=128, vt=_dev(vt, "vt"), vt_row=ldvt, vt_batch=H * 128 * ldvt,
             vt_head=128 * ldvt, vt_seg_len=skv_all // n_seg if n_seg else 0, vt_seg_stride=B * H * 128 * ldvt if n_seg else 0, kv_skip_begin=skip_begin,
             kv_skip_len=skip_len, carry_o=co, carry_lse=cl, o=0 if partial else _dev(out, "out"), o_partial=_dev(out, "o_part", torch.float32) if partial else 0,
             lse=_dev(lse, "lse", torch.float32) if partial else 0, o_row=ldo * B, o_batch=ldo, o_head=128, Sq=Sq, Skv=Skv, kv_dense=kv_dense, B=B, H=H,
             head_dim=128, softmax_scale=float(1.0 / math.sqrt(128) if softmax_scale is None else softmax_scale), logit_bound=float(logit_bound), variant=int(variant))
    if window is not None:
        assert vt.dim() == 4 and (Sq == Skv or window_cp is not None), "the window form takes plain V^T and Sq == Skv"
        a.update(frame_len=window[0], window_frames=window[1], sink_frames=window[2])
    if window_cp is not None:
        a.update(total_frames=window_cp[0], q_frame0=window_cp[1], buf_head_frames=window_cp[2], buf_tail_frame0=window_cp[3])
    if ranges is not None:
        assert vt.dim() == 4 and Sq == Skv, "the range-table form takes plain V^T and Sq == Skv"
        hp_dev = head_pattern_dev if head_pattern_dev is not None else ranges.head_pattern_dev  # (a per-launch choice in place of the table's own)
        a.update(ranges=_dev(ranges.ranges_dev, "ranges", torch.int32), n_patterns=ranges.n_patterns, max_ranges=ranges.max_ranges,
                 head_pattern=_dev(hp_dev, "head_pattern", torch.int32) if hp_dev is not None else 0)
    a["entry"], symbol, names, plan, plan_names = _ATTN_ENTRIES[entry]
    lib = _lib.load()

    def timer_meta():
        meta = dict(Sq=Sq, Skv=Skv, B=B, H=H, partial=partial)
        if entry == "cross":
            meta.update(kv_dense=kv_dense, q_norm=q_norm_weight is not None)
        elif entry in ("carry", "bounded_cp"):
            meta.update(carry=carry is not None, kv_skip=skip_len)
        if entry == "window":
            attended, dense = window_attn_tiles(Sq, *window)
            meta.update(frame_len=window[0], window_frames=window[1], sink_frames=window[2], tile_density=attended / dense)
        elif entry == "window_cp":
            attended, dense = window_attn_tiles_cp(Sq, Skv, window[0], *window_cp, window[1], window[2])
            meta.update(frame_len=window[0], window_frames=window[1], sink_frames=window[2], total_frames=window_cp[0], q_frame0=window_cp[1],
                        buf_head_frames=window_cp[2], buf_tail_frame0=window_cp[3], tile_density=attended / dense)
        elif entry == "ranges":
            # (the table counts its own H heads; with no head_pattern every head runs pattern 0 and the density is the same for any H)
            meta.update(n_patterns=ranges.n_patterns, max_ranges=ranges.max_ranges, tile_density=ranges.attended / ranges.dense)
        # the kernel the launcher picked for THIS launch: every fallback, the per-call variant, else the library option in force
        meta["kernel"] = getattr(lib, plan)(*[a[n] for n in plan_names]).decode()
        return meta

    with _kernel_timer("flash_attn_fwd", timer_meta):
        _lib.check(getattr(lib, symbol)(*[a[n] for n in names], _stream()), symbol)
    return (out, lse) if partial else out


def attn_merge(parts, Sq: int, B: int, H: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """parts: list of (o_part fp32 [Sq*B, H*128], lse fp32 [B, H, Sq]) from flash_attn(partial=True) over disjoint key sets of the same
    queries -> bf16 [Sq*B, H*128] = attention over the union of the keys (g3_attn_merge_partials_bf16). `out` may be a column view."""
    import ctypes as C
    n = len(parts)
    assert 1 <= n <= 8
    ld = parts[0][0].stride(0)
    for o, l in parts:
        assert o.shape == (Sq * B, H * 128) and o.stride(1) == 1 and o.stride(0) == ld and l.shape == (B, H, Sq) and l.is_contiguous()
    out, ldo = _out_bf16(out, Sq * B, H * 128, parts[0][0].device)
    op = (C.c_void_p * n)(*[_dev(o, "o_part", torch.float32) for o, _ in parts])
    lp = (C.c_void_p * n)(*[_dev(l, "lse", torch.float32) for _, l in parts])
    _lib.check(_lib.load().g3_attn_merge_partials_bf16(op, lp, n, ld * B, ld, 128, _dev(out, "out"), ldo * B, ldo, 128, Sq, B, H, 128, _stream()),
               "g3_attn_merge_partials_bf16")
    return out


def add_inplace(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    lib = _lib.load()
    _lib.check(lib.g3_add_inplace_bf16(_dev(x, "x"), _dev(y, "y"), x.numel(), _stream()), "g3_add_inplace_bf16")
    return x


def dit_patchify(sources, B: int, T: int, H: int, W: int, patch_t: int, patch_s: int) -> torch.Tensor:
    """sources: list of (tensor, has_t) - bf16 contiguous [B,C_i,T,H,W] (has_t) or [B,C_i,H,W] broadcast over T.
    -> patches [(T/pt)*(H/ps)*(W/ps)*B, sum(C_i)*pt*ps*ps] bf16, rows (t h w b), columns (c r m n). See g3_dit_patchify_bf16."""
    import ctypes as C
    assert 1 <= len(sources) <= 4
    ptrs, chans, has_t = [], [], []
    for i, (t, ht) in enumerate(sources):
        assert t.is_contiguous() and t.shape[0] == B and tuple(t.shape[-2:]) == (H, W) and (t.dim() == 5 and t.shape[2] == T if ht else t.dim() == 4)
        ptrs.append(_dev(t, f"source{i}"))
        chans.append(int(t.shape[1]))
        has_t.append(1 if ht else 0)
    n = len(sources)
    ctot = sum(chans)
    out = torch.empty(((T // patch_t) * (H // patch_s) * (W // patch_s) * B, ctot * patch_t * patch_s * patch_s), dtype=torch.bfloat16,
                      device=sources[0][0].device)
    lib = _lib.load()
    _lib.check(lib.g3_dit_patchify_bf16((C.c_void_p * n)(*ptrs), (C.c_int * n)(*chans), (C.c_int * n)(*has_t), n, out.data_ptr(), B, T, H, W,
                                        patch_t, patch_s, _stream()), "g3_dit_patchify_bf16")
    return out


def dit_unpatchify(y: torch.Tensor, B: int, C_out: int, T: int, H: int, W: int, patch_t: int, patch_s: int) -> torch.Tensor:
    """y [(T/pt)(H/ps)(W/ps) B, ps*ps*pt*C_out] -> [B, C_out, T, H, W]. See g3_dit_unpatchify_bf16."""
    rows, cols, ldy = _rowmajor2d(y, "y")
    assert rows == (T // patch_t) * (H // patch_s) * (W // patch_s) * B and cols == patch_s * patch_s * patch_t * C_out
    out = torch.empty((B, C_out, T, H, W), dtype=torch.bfloat16, device=y.device)
    lib = _lib.load()
    _lib.check(lib.g3_dit_unpatchify_bf16(_dev(y, "y"), ldy, out.data_ptr(), B, C_out, T, H, W, patch_t, patch_s, _stream()), "g3_dit_unpatchify_bf16")
    return out


def timestep_embedding(timesteps: torch.Tensor, norm_weight: torch.Tensor, D: int):
    """timesteps f32 [B] -> (t_sin bf16 [B,D], emb bf16 [B,D]). See g3_timestep_embedding_bf16."""
    assert timesteps.dim() == 1 and timesteps.is_contiguous() and norm_weight.numel() == D
    Bn = timesteps.shape[0]
    t_sin = torch.empty((Bn, D), dtype=torch.bfloat16, device=timesteps.device)
    emb = torch.empty_like(t_sin)
    lib = _lib.load()
    _lib.check(lib.g3_timestep_embedding_bf16(_dev(timesteps, "timesteps", torch.float32), _dev(norm_weight, "norm_weight"), t_sin.data_ptr(),
                                              emb.data_ptr(), Bn, D, _stream()), "g3_timestep_embedding_bf16")
    return t_sin, emb


def edm_prepare_input(xt, gt_latent, noise, indicator, T: int, hw: int, augment_sigma: float, c_in_aug: float,
                      c_in_bf16: float, c_in_step: float):
    """-> (new_xt, new_xt_scaled), both bf16 like xt. See g3_edm_prepare_input_bf16."""
    assert xt.is_contiguous() and gt_latent.is_contiguous() and noise.is_contiguous() and indicator.is_contiguous()
    assert xt.shape == gt_latent.shape == noise.shape and indicator.numel() == T
    new_xt, new_xt_scaled = torch.empty_like(xt), torch.empty_like(xt)
    lib = _lib.load()
    _lib.check(lib.g3_edm_prepare_input_bf16(_dev(xt, "xt"), _dev(gt_latent, "gt_latent"), _dev(noise, "noise", torch.float32),
                                             _dev(indicator, "indicator", torch.float32), _dev(new_xt, "new_xt"),
                                             _dev(new_xt_scaled, "new_xt_scaled"), xt.numel(), T, hw, augment_sigma, c_in_aug,
                                             c_in_bf16, c_in_step, _stream()), "g3_edm_prepare_input_bf16")
    return new_xt, new_xt_scaled


def edm_cfg_euler_step(out_cond, out_uncond, new_xt, gt_latent, indicator, T: int, hw: int, guidance: float,
                       c_skip_bf16: float, c_out_bf16: float, c_skip: float, c_out: float, sigma: float, inv_sigma: float,
                       sigma_next: float):
    """-> xt_next (bf16). See g3_edm_cfg_euler_step_bf16."""
    for t in (out_cond, out_uncond, new_xt, gt_latent, indicator):
        assert t.is_contiguous()
    assert out_cond.shape == out_uncond.shape == new_xt.shape == gt_latent.shape
    xt_next = torch.empty_like(new_xt)
    lib = _lib.load()
    _lib.check(lib.g3_edm_cfg_euler_step_bf16(_dev(out_cond, "out_cond"), _dev(out_uncond, "out_uncond"), _dev(new_xt, "new_xt"),
                                              _dev(gt_latent, "gt_latent"), _dev(indicator, "indicator", torch.float32),
                                              _dev(xt_next, "xt_next"), new_xt.numel(), T, hw, guidance, c_skip_bf16, c_out_bf16,
                                              c_skip, c_out, sigma, inv_sigma, sigma_next, _stream()), "g3_edm_cfg_euler_step_bf16")
    return xt_next


def edm_cfg_2ab_step(out_cond, out_uncond, new_xt, gt_latent, indicator, T: int, hw: int, guidance: float,
                     c_skip_bf16: float, c_out_bf16: float, c_skip: float, c_out: float, sigma: float, inv_sigma: float,
                     sigma_next: float, x0_hist, have_prev: bool, a: float, cb1: float, cb2: float, x0_out=None):
    """-> xt_next (bf16). `x0_hist` (fp32, new_xt's shape) is the previous step's x0 prediction when have_prev, and is overwritten IN PLACE with
    this step's; x0_out (optional) receives it instead and leaves x0_hist as it was. See g3_edm_cfg_2ab_step_bf16."""
    x0_out = x0_hist if x0_out is None else x0_out
    for t in (out_cond, out_uncond, new_xt, gt_latent, indicator, x0_hist, x0_out):
        assert t.is_contiguous()
    assert out_cond.shape == out_uncond.shape == new_xt.shape == gt_latent.shape == x0_hist.shape == x0_out.shape
    assert indicator.numel() == T and new_xt.numel() % (T * hw) == 0
    xt_next = torch.empty_like(new_xt)
    lib = _lib.load()
    _lib.check(lib.g3_edm_cfg_2ab_step_bf16(_dev(out_cond, "out_cond"), _dev(out_uncond, "out_uncond"), _dev(new_xt, "new_xt"),
                                            _dev(gt_latent, "gt_latent"), _dev(indicator, "indicator", torch.float32),
                                            _dev(xt_next, "xt_next"), new_xt.numel(), T, hw, guidance, c_skip_bf16, c_out_bf16,
                                            c_skip, c_out, sigma, inv_sigma, sigma_next, _dev(x0_hist, "x0_hist", torch.float32),
                                            _dev(x0_out, "x0_out", torch.float32), int(bool(have_prev)), a, cb1, cb2, _stream()),
               "g3_edm_cfg_2ab_step_bf16")
    return xt_next


def edm_cond_euler_step(out_cond, new_xt, gt_latent, indicator, T: int, hw: int, c_skip_bf16: float, c_out_bf16: float, c_skip: float,
                        c_out: float, sigma: float, inv_sigma: float, sigma_next: float):
    """-> xt_next (bf16): the Euler step of a sigma outside the guidance interval, net_output = out_cond. See g3_edm_cond_euler_step_bf16."""
    for t in (out_cond, new_xt, gt_latent, indicator):
        assert t.is_contiguous()
    assert out_cond.shape == new_xt.shape == gt_latent.shape
    assert indicator.numel() == T and new_xt.numel() % (T * hw) == 0
    xt_next = torch.empty_like(new_xt)
    lib = _lib.load()
    _lib.check(lib.g3_edm_cond_euler_step_bf16(_dev(out_cond, "out_cond"), _dev(new_xt, "new_xt"), _dev(gt_latent, "gt_latent"),
                                               _dev(indicator, "indicator", torch.float32), _dev(xt_next, "xt_next"), new_xt.numel(), T, hw,
                                               c_skip_bf16, c_out_bf16, c_skip, c_out, sigma, inv_sigma, sigma_next, _stream()),
               "g3_edm_cond_euler_step_bf16")
    return xt_next


def edm_cond_2ab_step(out_cond, new_xt, gt_latent, indicator, T: int, hw: int, c_skip_bf16: float, c_out_bf16: float, c_skip: float,
                      c_out: float, sigma: float, inv_sigma: float, sigma_next: float, x0_hist, have_prev: bool, a: float, cb1: float,
                      cb2: float, x0_out=None):
    """-> xt_next (bf16): edm_cfg_2ab_step for a sigma outside the guidance interval, net_output = out_cond; x0_hist / x0_out as there.
    See g3_edm_cond_2ab_step_bf16."""
    x0_out = x0_hist if x0_out is None else x0_out
    for t in (out_cond, new_xt, gt_latent, indicator, x0_hist, x0_out):
        assert t.is_contiguous()
    assert out_cond.shape == new_xt.shape == gt_latent.shape == x0_hist.shape == x0_out.shape
    assert indicator.numel() == T and new_xt.numel() % (T * hw) == 0
    xt_next = torch.empty_like(new_xt)
    lib = _lib.load()
    _lib.check(lib.g3_edm_cond_2ab_step_bf16(_dev(out_cond, "out_cond"), _dev(new_xt, "new_xt"), _dev(gt_latent, "gt_latent"),
                                             _dev(indicator, "indicator", torch.float32), _dev(xt_next, "xt_next"), new_xt.numel(), T, hw,
                                             c_skip_bf16, c_out_bf16, c_skip, c_out, sigma, inv_sigma, sigma_next,
                                             _dev(x0_hist, "x0_hist", torch.float32), _dev(x0_out, "x0_out", torch.float32),
                                             int(bool(have_prev)), a, cb1, cb2, _stream()), "g3_edm_cond_2ab_step_bf16")
    return xt_next


class HipTimer:
    """hipEvent pair recorded on torch's current stream through the C ABI (used by bench.py for kernel timing)."""

    def __init__(self):
        import ctypes as C
        self._lib = _lib.load()
        self._a, self._b = C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.g3_event_create(C.byref(self._a)))
        _lib.check(self._lib.g3_event_create(C.byref(self._b)))

    def start(self):
        _lib.check(self._lib.g3_event_record(self._a, _stream()))

    def stop(self):
        _lib.check(self._lib.g3_event_record(self._b, _stream()))

    def elapsed_ms(self) -> float:
        import ctypes as C
        ms = C.c_float(0)
        _lib.check(self._lib.g3_event_elapsed_ms(self._a, self._b, C.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            self._lib.g3_event_destroy(self._a)
            self._lib.g3_event_destroy(self._b)
        except Exception:
            pass
