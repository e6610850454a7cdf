"""Race screen: every LDS hand-off of the MFMA kernels must be fenced, so results may not depend on wave timing. Runs the
product library against the same sources built with -DG3_AB_JITTER=<n> (pseudo-random waves sleep n*64 cycles at tile / phase
boundaries) and demands BITWISE equal outputs.
  build (here, before gpurun):  python tools/race_screen.py --build [n]
  run (GPU box):                python tools/race_screen.py [--no-tokenizer] [--mxfp8-producers-only: the last section alone]
                                                            [--bounded-cp-only: the no-max key-sharded attention section alone]
                                                            [--mfma16-only: the 16x16x32 no-max attention section alone]
                                                            [--ranges-only: the range-table attention section alone]
                                                            [--gemm-mfma16-only: the deferred GEMM's 16x16x32 body alone]"""
import ctypes as C
import math
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

if "--build" in sys.argv:
    from gen3c_amd import build
    n = [a for a in sys.argv[1:] if a.isdigit()]
    extra = tuple(a for a in sys.argv[1:] if a.startswith("-D"))  # e.g. -DG3_AB_OMIT_PROLOGUE_BARRIER: self-test of the screen
    # default perturbations: sleeping waves at tile / phase boundaries AND no static wave priorities (the variant that exposed the
    # attention prologue races of round 1; -DG3_AB_OMIT_PROLOGUE_BARRIER re-introduces one of them as a self-test of this screen)
    jit = () if "--no-jitter" in sys.argv else (f"-DG3_AB_JITTER={n[0] if n else 30}",)
    extra = extra + ("-DG3_AB_NO_ATTN_SETPRIO", "-DG3_AB_NO_GEMM_SETPRIO")
    print(build.build(extra_flags=jit + extra, suffix="_ab", force=True))
    sys.exit(0)

import torch  # noqa: E402
from gen3c_amd import _lib, ops  # noqa: E402

base = _lib.load()
alt = C.CDLL(str(ROOT / "gen3c_amd" / "lib" / "libgen3c_hip_ab.so"))
for name, argtypes in _lib.SIGNATURES.items():
    getattr(alt, name).argtypes = argtypes
    getattr(alt, name).restype = _lib._RESTYPES.get(name, C.c_int)
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(3)
bad = 0
ONLY_BCP = "--bounded-cp-only" in sys.argv  # run only the section of g3_self_attn_fwd_bounded_cp_bf16
ONLY_W4C = "--mfma16-only" in sys.argv  # run only the section of g3_self_attn_fwd_bounded16_bf16
ONLY_RNG = "--ranges-only" in sys.argv  # run only the section of g3_self_attn_fwd_ranges_bf16
ONLY_G16 = "--gemm-mfma16-only" in sys.argv  # run only the section of the deferred GEMM's 16x16x32 body
ONLY_MX = "--mxfp8-producers-only" in sys.argv or ONLY_BCP or ONLY_W4C or ONLY_RNG or ONLY_G16  # run only the last section (the launches that emit MXFP8)


def both(fn):
    outs = []
    for lib in (base, alt):
        outs.append(fn(lib))
    torch.cuda.synchronize()
    return outs


def report(what, a, b):
    global bad
    eq = bool(torch.equal(a, b))
    bad += not eq
    print(f"{'ok  ' if eq else 'DIFF'} {what}" + ("" if eq else f"  rel-l2 {float((a.float() - b.float()).norm() / a.float().norm()):.3e}"), flush=True)


# ---- attention (long and short contexts, ragged tails, segmented V^T)
for (Sq, Skv, H, segs) in [] if ONLY_MX else [(56320, 56320, 4, 1), (7040, 56320, 4, 8), (1000, 449, 3, 1), (56320, 512, 8, 1), (300, 128, 2, 2)]:
    q = torch.randn(Sq, H * 128, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    if segs == 1:
        vt = ops.transpose_v(v, Skv, 1, H)
    else:
        sl = Skv // segs
        vt = torch.stack([ops.transpose_v(v[i * sl:(i + 1) * sl], sl, 1, H) for i in range(segs)]).contiguous()
    ld = vt.shape[-1]
    for variant in (3, 4, 6, 8, 9, 10, 11):
        def run(lib):
            lib.g3_set_option(b"attn_variant", variant)
            o = torch.empty_like(q)
            args = (q.data_ptr(), H * 128, H * 128, 128, k.data_ptr(), H * 128, H * 128, 128, vt.data_ptr(), ld, H * 128 * ld, 128 * ld)
            tail = (o.data_ptr(), H * 128, H * 128, 128, Sq, Skv, 1, H, 128, 1.0 / math.sqrt(128), st)
            rc = lib.g3_flash_attn_fwd_kvseg_bf16(*args, Skv // segs, H * 128 * ld, *tail) if segs > 1 else lib.g3_flash_attn_fwd_bf16(*args, *tail)
            assert rc == 0, lib.g3_last_error()
            return o
        a, b = both(run)
        report(f"attention Sq={Sq} Skv={Skv} H={H} segs={segs} variant={variant}", a, b)
    del q, k, v, vt

# ---- cross-attention form (round 6): Q norm inside the Q load + zero key tail in closed form
for (Sq, Skv, H, live) in [] if ONLY_MX else [(56320, 512, 8, 64), (1000, 512, 3, 0), (3000, 256, 2, 100)]:
    q = torch.randn(Sq, H * 128, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    if live:
        k[live:] = 0
        v[live:] = 0
    wq = (torch.rand(128, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    vt = ops.transpose_v(v, Skv, 1, H)
    ld = vt.shape[-1]

    def run(lib):
        lib.g3_set_option(b"attn_variant", 0)
        o = torch.empty_like(q)
        rc = lib.g3_cross_attn_fwd_bf16(q.data_ptr(), H * 128, H * 128, 128, wq.data_ptr(), 1e-6, k.data_ptr(), H * 128, H * 128, 128, vt.data_ptr(), ld, H * 128 * ld, 128 * ld,
                                        o.data_ptr(), H * 128, H * 128, 128, Sq, Skv, live, 1, H, 128, 1.0 / math.sqrt(128), st)
        assert rc == 0, lib.g3_last_error()
        return o
    a, b = both(run)
    report(f"cross-attention form Sq={Sq} Skv={Skv} H={H} live={live} (q norm in the kernel)", a, b)
    del q, k, v, vt

# ---- carry-in form (g3_flash_attn_fwd_carry_bf16: the local_carry context-parallel schedule): an interior rank's ONE launch over every remote key,
# its own key block skipped inside the gathered buffers, the own block's fp32 partial carried in; bf16 and fp32-partial outputs
for (Sl, nseg, rank, H) in [] if ONLY_MX else [(7040, 8, 3, 4), (256, 3, 1, 2), (64, 4, 1, 2)]:
    Skv = Sl * nseg
    q = torch.randn(Sl, H * 128, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    vt = torch.stack([ops.transpose_v(v[i * Sl:(i + 1) * Sl], Sl, 1, H) for i in range(nseg)]).contiguous()
    ld = vt.shape[-1]
    for variant in (4, 11):
        own_o, own_l = ops.flash_attn(q, k[rank * Sl:(rank + 1) * Sl].contiguous(), vt[rank:rank + 1].contiguous(), Sl, Sl, 1, H, partial=True, variant=variant)
        torch.cuda.synchronize()
        for partial in (False, True):
            def run(lib):
                o = torch.empty_like(q)
                o32 = torch.empty(Sl, H * 128, device=dev, dtype=torch.float32)
                lse = torch.empty(1, H, Sl, device=dev, dtype=torch.float32)
                rc = lib.g3_flash_attn_fwd_carry_bf16(q.data_ptr(), H * 128, H * 128, 128, k.data_ptr(), H * 128, H * 128, 128, vt.data_ptr(), ld, H * 128 * ld, 128 * ld,
                                                      Sl, H * 128 * ld, rank * Sl, Sl, own_o.data_ptr(), own_l.data_ptr(), None if partial else o.data_ptr(),
                                                      o32.data_ptr() if partial else None, lse.data_ptr() if partial else None, H * 128, H * 128, 128,
                                                      Sl, Skv - Sl, 1, H, 128, 1.0 / math.sqrt(128), variant, st)
                assert rc == 0, lib.g3_last_error()
                return torch.cat([o32.flatten(), lse.flatten()]) if partial else o
            a, b = both(run)
            report(f"carry-in form S_local={Sl} segs={nseg} rank={rank} H={H} variant={variant} {'fp32 partial' if partial else 'bf16'}", a, b)
    del q, k, v, vt

# ---- no-max forms under key sharding (g3_self_attn_fwd_bounded_cp_bf16): flash_attn_fwd_w4b_nm_kernel over segmented V^T (every key, no carry) and
# flash_attn_fwd_w4b_nm_carry_kernel (an interior rank's remote keys, own block skipped, the own block's bounded partial carried in); q, k RMS-normalised
# per head so that the bound holds; bf16 and fp32-partial outputs
for (Sl, nseg, rank, H) in [(7040, 8, 3, 4), (256, 3, 1, 2), (64, 4, 1, 2)] if (ONLY_BCP or not ONLY_MX) else []:
    Skv = Sl * nseg
    rms = lambda x: (x.view(x.shape[0], H, 128) * torch.rsqrt(x.view(x.shape[0], H, 128).pow(2).mean(-1, keepdim=True))).reshape(x.shape[0], H * 128)
    q = rms(torch.randn(Sl, H * 128, device=dev, generator=g)).to(torch.bfloat16)
    k = rms(torch.randn(Skv, H * 128, device=dev, generator=g)).to(torch.bfloat16)
    v = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    vt = torch.stack([ops.transpose_v(v[i * Sl:(i + 1) * Sl], Sl, 1, H) for i in range(nseg)]).contiguous()
    ld = vt.shape[-1]
    bound = 128 / math.sqrt(128) * 1.03
    own_o, own_l = ops.self_attn_bounded(q, k[rank * Sl:(rank + 1) * Sl].contiguous(), vt[rank:rank + 1].contiguous(), Sl, Sl, 1, H, bound, partial=True, variant=11)
    torch.cuda.synchronize()
    for cp_form in (False, True):
        name = base.g3_self_attn_cp_kernel_name(Sl, Skv - Sl if cp_form else Skv, 1, H, bound, 11, 1, int(cp_form)).decode()
        assert name == ("flash_attn_fwd_w4b_nm_carry_kernel<true>" if cp_form else "flash_attn_fwd_w4b_nm_kernel<true>"), name
        for partial in (False, True):
            def run(lib):
                o = torch.empty_like(q)
                o32 = torch.empty(Sl, H * 128, device=dev, dtype=torch.float32)
                lse = torch.empty(1, H, Sl, device=dev, dtype=torch.float32)
                rc = lib.g3_self_attn_fwd_bounded_cp_bf16(q.data_ptr(), H * 128, H * 128, 128, k.data_ptr(), H * 128, H * 128, 128, vt.data_ptr(), ld, H * 128 * ld, 128 * ld,
                                                          Sl, H * 128 * ld, rank * Sl if cp_form else 0, Sl if cp_form else 0, own_o.data_ptr() if cp_form else None,
                                                          own_l.data_ptr() if cp_form else None, None if partial else o.data_ptr(),
                                                          o32.data_ptr() if partial else None, lse.data_ptr() if partial else None, H * 128, H * 128, 128,
                                                          Sl, Skv - Sl if cp_form else Skv, 1, H, 128, 1.0 / math.sqrt(128), bound, 11, st)
                assert rc == 0, lib.g3_last_error()
                return torch.cat([o32.flatten(), lse.flatten()]) if partial else o
            a, b = both(run)
            report(f"bounded {'carry-in + skip' if cp_form else 'segmented V^T'} form ({name}) S_local={Sl} segs={nseg} rank={rank} H={H} {'fp32 partial' if partial else 'bf16'}", a, b)
    del q, k, v, vt

# ---- the no-max kernel on 16x16x32 MFMAs (g3_self_attn_fwd_bounded16_bf16, flash_attn_fwd_w4c_nm_kernel): the DiT step's launch, an odd tile count with a
# ragged last query block, a single tile, and 4 / 5 / 6 tiles (K one tile ahead: the first K(3) fetched behind a barrier, both loop exits after a steady pair;
# the jitter build also sleeps between that barrier and the first piece into the stage it freed); q, k RMS-normalised per head so that the bound holds
for (Sq, Skv, H) in [(56320, 56320, 4), (320, 192, 2), (256, 64, 8), (320, 256, 2), (320, 320, 2), (320, 384, 2)] if (ONLY_W4C or not ONLY_MX) else []:
    rms = lambda x: (x.view(x.shape[0], H, 128) * torch.rsqrt(x.view(x.shape[0], H, 128).pow(2).mean(-1, keepdim=True))).reshape(x.shape[0], H * 128)
    q = rms(torch.randn(Sq, H * 128, device=dev, generator=g)).to(torch.bfloat16)
    k = rms(torch.randn(Skv, H * 128, device=dev, generator=g)).to(torch.bfloat16)
    v = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    vt = ops.transpose_v(v, Skv, 1, H)
    ld = vt.shape[-1]
    bound = 128 / math.sqrt(128) * 1.03
    name = base.g3_self_attn16_kernel_name(Sq, Skv, 1, H, bound, 11).decode()
    assert name == "flash_attn_fwd_w4c_nm_kernel", name

    def run(lib):
        o = torch.empty_like(q)
        rc = lib.g3_self_attn_fwd_bounded16_bf16(q.data_ptr(), H * 128, H * 128, 128, k.data_ptr(), H * 128, H * 128, 128, vt.data_ptr(), ld, H * 128 * ld, 128 * ld, 0, 0,
                                                 o.data_ptr(), None, None, H * 128, H * 128, 128, Sq, Skv, 1, H, 128, 1.0 / math.sqrt(128), bound, 11, st)
        assert rc == 0, lib.g3_last_error()
        return o
    a, b = both(run)
    report(f"no-max 16x16x32 form ({name}) Sq={Sq} Skv={Skv} H={H}", a, b)
    del q, k, v, vt

# ---- GEMM: every K-loop structure x epilogues x ragged shapes
for (M, N, K, epi) in [] if ONLY_MX else [(56320, 4096, 4096, 2), (7040, 12288, 4096, 0), (4096, 16384, 4096, 1), (3000, 4096, 16384, 2), (513, 264, 192, 3), (300, 520, 128, 0),
                       (256, 256, 64, 0), (8192, 12288, 4096, 0), (16384, 16384, 4096, 1), (8448, 4096, 2432, 2)]:
    a_ = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w_ = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(1, N, device=dev, generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    # 13 = one wave per SIMD as a persistent tile loop (round 3; runs where a workgroup gets >= 2 tiles); 23 = persistent with the DEFERRED epilogue
    # (round 5, gemm_w4e.hpp: where M, N are multiples of 256, K of 128 with >= 38 K tiles - the jitter hits its tile boundaries and period K tiles)
    for pp in (0, 1, 2, 3, 13, 23):
        def run(lib):
            lib.g3_set_option(b"gemm_pingpong", pp % 10)
            lib.g3_set_option(b"gemm_persistent", 1 if pp == 13 else 0)
            lib.g3_set_option(b"gemm_deferred", 1 if pp == 23 else 0)
            o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            rc = lib.g3_gemm_bf16_nt(a_.data_ptr(), K, w_.data_ptr(), K, o.data_ptr(), N, M, N, K, epi, gate.data_ptr() if epi >= 2 else None, 1, N,
                                     res.data_ptr() if epi in (2, 4) else None, N, st)
            assert rc == 0, lib.g3_last_error()
            return o
        x, y = both(run)
        report(f"gemm {M}x{N}x{K} epi{epi} pingpong={pp}", x, y)
    del a_, w_, gate, res

# ---- the deferred-epilogue GEMM with its K loop on 16x16x32 MFMAs (gemm_mfma16 = 1: gemm_bf16_nt_w4e16_kernel) at its launch forms: the three epilogue classes,
# both piece orders, two tiles per workgroup at the minimum of 38 K tiles, 66 carried epilogues in a row on 8 workgroups and a flush behind a carry on 248. Every
# fragment read lands in registers the quadrant before it multiplied, and the barrier sits between two quadrants: what the jitter stretches
for (M, N, K, epi, grid) in [] if (ONLY_MX and not ONLY_G16) else [(8192, 4096, 2432, 0, 0), (8192, 4096, 2432, 1, 0), (8192, 4096, 2432, 2, 0), (8448, 4096, 2560, 1, 8),
                                                                    (8448, 4096, 2560, 2, 248), (56320, 4096, 4096, 2, 0), (16384, 16384, 4096, 1, 0)]:
    a_ = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w_ = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(2, N, device=dev, generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    for tf in (0, 1):
        def run(lib):
            for opt, val in ((b"gemm_pingpong", 3), (b"gemm_persistent", 0), (b"gemm_deferred", 1), (b"gemm_mfma16", 1), (b"gemm_deferred_grid", grid), (b"gemm_tokens_first", tf)):
                lib.g3_set_option(opt, val)
            o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            rc = lib.g3_gemm_bf16_nt(a_.data_ptr(), K, w_.data_ptr(), K, o.data_ptr(), N, M, N, K, epi, gate.data_ptr() if epi == 2 else None, 2, N,
                                     res.data_ptr() if epi == 2 else None, N, st)
            assert rc == 0, lib.g3_last_error()
            lib.g3_set_option(b"gemm_deferred_grid", 0)
            lib.g3_set_option(b"gemm_tokens_first", 2)
            return o
        x, y = both(run)
        report(f"gemm 16x16x32 body {M}x{N}x{K} epi{epi} grid={grid or 'CUs'} tokens_first={tf}", x, y)
    del a_, w_, gate, res

# ---- implicit-GEMM convolutions (tokenizer geometries: 1x3x3, causal 3x1x1, strided)
for (C_in, C_out, T, Hh, Ww, kt, kh, kw, st_, sh, sw) in [] if ONLY_MX else [(128, 256, 5, 48, 64, 1, 3, 3, 1, 1, 1), (256, 256, 6, 40, 48, 3, 1, 1, 1, 1, 1), (128, 128, 5, 48, 64, 1, 3, 3, 1, 2, 2),
                                                           (256, 256, 7, 24, 32, 3, 1, 1, 2, 1, 1)]:
    x_ = torch.randn(T * Hh * Ww, C_in, device=dev, generator=g).to(torch.bfloat16)
    w_ = (torch.randn(kt * kh * kw, C_out, C_in, device=dev, generator=g) / math.sqrt(C_in * kt * kh * kw)).to(torch.bfloat16)
    bias = torch.randn(C_out, device=dev, generator=g).to(torch.bfloat16)
    To = (T + st_ - 1) // st_ if kt == 3 else T
    Ho, Wo = (Hh // sh, Ww // sw)
    ot, oh, ow = (-(kt - 1), 0 if sh == 2 else -(kh // 2), 0 if sw == 2 else -(kw // 2))
    if kt == 3 and st_ == 2:
        To = (T - 1) // 2 + 1
    resid = torch.randn(To * Ho * Wo, C_out, device=dev, generator=g).to(torch.bfloat16)
    for (pp, w4, with_res) in ((0, 0, False), (2, 0, False), (2, 1, False), (2, 1, True), (2, 0, True)):  # w4 = 1: gemm_w4_conv.hpp (round 3)
        def run(lib):
            lib.g3_set_option(b"gemm_pingpong", pp)
            lib.g3_set_option(b"conv_w4", w4)
            o = torch.empty(To * Ho * Wo, C_out, device=dev, dtype=torch.bfloat16)
            rc = lib.g3_conv3d_cl_bf16(x_.data_ptr(), C_in, w_.data_ptr(), C_in, bias.data_ptr(), resid.data_ptr() if with_res else None, C_out, o.data_ptr(), C_out,
                                       C_in, C_out, T, Hh, Ww, To, Ho, Wo, kt, kh, kw, st_, sh, sw, ot, oh, ow, st)
            assert rc == 0, lib.g3_last_error()
            return o
        x, y = both(run)
        report(f"conv {C_in}->{C_out} k=({kt},{kh},{kw}) s=({st_},{sh},{sw}) on {T}x{Hh}x{Ww} pingpong={pp} conv_w4={w4} residual={with_res}", x, y)
# ---- split-KV attention: partial outputs + merge (round 3)
for (Sq, Skv, H, variant) in [] if ONLY_MX else [(7040, 14080, 4, 11), (7040, 14080, 4, 4), (1000, 448, 2, 4)]:
    q = torch.randn(Sq, H * 128, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(Skv, H * 128, device=dev, generator=g).to(torch.bfloat16)
    vt = ops.transpose_v(v, Skv, 1, H)
    ld = vt.shape[-1]

    def run(lib):
        op = torch.empty(Sq, H * 128, device=dev, dtype=torch.float32)
        lse = torch.empty(1, H, Sq, device=dev, dtype=torch.float32)
        rc = lib.g3_flash_attn_fwd_ex_bf16(q.data_ptr(), H * 128, H * 128, 128, k.data_ptr(), H * 128, H * 128, 128, vt.data_ptr(), ld, H * 128 * ld, 128 * ld, 0, 0,
                                           None, op.data_ptr(), lse.data_ptr(), H * 128, H * 128, 128, Sq, Skv, 1, H, 128, 1.0 / math.sqrt(128), variant, st)
        assert rc == 0, lib.g3_last_error()
        return torch.cat([op.reshape(-1), lse.reshape(-1)])
    a, b = both(run)
    report(f"split-KV partial attention Sq={Sq} Skv={Skv} H={H} variant={variant}", a, b)
# ---- the whole tokenizer at the size bench.py times it (round 4): 121 x 704 x 1280, channels = 128 - the 1.79 GB activations, the spatial attention's frames
# on two streams with per-stream score buffers, GroupNorm statistics from conv epilogues, all 16 latent frames in the temporal attention
if "--no-tokenizer" not in sys.argv and not ONLY_MX:
    import bench  # noqa: E402
    from gen3c_amd.tokenizer import CausalVideoTokenizerNet  # noqa: E402
    for lib in (base, alt):
        lib.g3_set_option(b"attn_variant", 0)
        lib.g3_set_option(b"gemm_pingpong", 3)
        lib.g3_set_option(b"gemm_persistent", 0)
        lib.g3_set_option(b"gemm_deferred", 1)
        lib.g3_set_option(b"conv_w4", 1)
    tnet = CausalVideoTokenizerNet(channels=128, device=dev)
    tnet.init_random(seed=3)
    clip = bench.tokenizer_bench_clip(dev)
    outs = []
    for lib in (base, alt, base):
        _lib._lib = lib  # the product's loader hands out this handle
        z = tnet.encoder(clip)
        y = tnet.decoder(z)
        torch.cuda.synchronize()
        outs.append((z, y))
    _lib._lib = base
    # the fp64 atomics that collect GroupNorm statistics may add in any order: bitwise equality is expected in practice (measured), a last-bit
    # difference of a statistic would show as ~1e-7, a race as >= 1e-3
    for what, i in (("encode", 0), ("decode", 1)):
        report(f"tokenizer {what} 121x704x1280 channels=128, product vs jitter build", outs[0][i], outs[1][i])
        report(f"tokenizer {what} 121x704x1280 channels=128, product run twice", outs[0][i], outs[2][i])
    del outs, clip, tnet
# ---- range-table self-attention (g3_self_attn_fwd_ranges_bf16): both kernel forms on the three shapes of tests/test_attn_ranges_gpu.py (its hand-made tables:
# one to three tiles per block; random lists under a head-to-pattern lookup on the 3-D grid; 64 one-tile ranges on the 1-D grid) - the cursor's range changes
# sit between the statements whose LDS hand-offs the jitter stretches
if not (ONLY_BCP or ONLY_W4C or ONLY_G16 or "--mxfp8-producers-only" in sys.argv):
    from tests.test_attn_ranges_gpu import _shape as rng_shape
    for i in (1, 2, 3):
        S_, B_, H_, tab, hp = rng_shape(i)
        table = ops.attn_range_table(tab, S_, head_pattern=hp, H=H_)
        q = torch.randn(S_ * B_, H_ * 128, device=dev, generator=g).to(torch.bfloat16)
        k = torch.randn(S_ * B_, H_ * 128, device=dev, generator=g).to(torch.bfloat16)
        vt = ops.transpose_v(torch.randn(S_ * B_, H_ * 128, device=dev, generator=g).to(torch.bfloat16), S_, B_, H_)
        ld = vt.shape[-1]
        for bound in (20.0, 0.0):  # (q, k are not normalised here: |q . k| / sqrt(128) is N(0, 1), far below 20; 0: the running-maximum form)
            def run(lib):
                o = torch.zeros(S_ * B_, H_ * 128, device=dev, dtype=torch.bfloat16)
                rc = lib.g3_self_attn_fwd_ranges_bf16(q.data_ptr(), B_ * H_ * 128, H_ * 128, 128, k.data_ptr(), B_ * H_ * 128, H_ * 128, 128, vt.data_ptr(), ld,
                                                      H_ * 128 * ld, 128 * ld, o.data_ptr(), B_ * H_ * 128, H_ * 128, 128, S_, B_, H_, 128, 1.0 / math.sqrt(128),
                                                      bound, table.ranges_dev.data_ptr(), table.n_patterns, table.max_ranges,
                                                      table.head_pattern_dev.data_ptr() if table.head_pattern_dev is not None else None, st)
                assert rc == 0, lib.g3_last_error()
                return o
            a, b = both(run)
            report(f"self_attn_ranges shape {i}: S={S_} B={B_} H={H_} max_ranges={table.max_ranges} {'no-max' if bound else 'running-max'} form", a, b)
        del q, k, vt
# ---- the producers that emit MXFP8 from their registers (mxfp8_producers = "fused"): the GEMM with MXFP8 output (its K loop carries the jitter; the epilogue
# transposes through each wave's own LDS slice and quantises across lane quads) and the two LayerNorm forms, plain and with the position embedding
LN_WAVE_START = int(os.environ.get("G3_LN_WAVE_ROWS", "0"))  # what both libraries start with (csrc/api.hip); restored after each case
for (M, N, K, epi) in [] if (ONLY_BCP or ONLY_W4C or ONLY_RNG or ONLY_G16) else [(14080, 16384, 4096, 1), (7040, 4096, 4096, 0), (513, 1024, 256, 1), (300, 512, 256, 0)]:
    aq, as_ = ops.quant_mxfp8(torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16))
    wq, ws = ops.quant_mxfp8((torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16))

    def run(lib):
        q = torch.zeros(M, N, device=dev, dtype=torch.uint8)
        s = torch.zeros(M, N // 32, device=dev, dtype=torch.uint8)
        rc = lib.g3_gemm_mxfp8_nt_mxout(aq.data_ptr(), K, as_.data_ptr(), K // 32, wq.data_ptr(), K, ws.data_ptr(), K // 32, q.data_ptr(), N, s.data_ptr(), N // 32,
                                        M, N, K, epi, st)
        assert rc == 0, lib.g3_last_error()
        return torch.cat([q.flatten(), s.flatten()])
    a, b = both(run)
    report(f"gemm_mxfp8 with MXFP8 output {M}x{N}x{K} epi{epi}", a, b)
    del aq, as_, wq, ws
for (T_, Hp, Wp, B_, D_, wave) in [] if (ONLY_BCP or ONLY_W4C or ONLY_RNG or ONLY_G16) else [(4, 20, 22, 2, 4096, 1), (4, 20, 22, 2, 4096, 0), (3, 5, 7, 1, 2048, 0)]:
    rows = T_ * Hp * Wp * B_
    x_ = torch.randn(rows, D_, device=dev, generator=g).to(torch.bfloat16)
    pe = (0.3 * torch.randn(T_ * Hp * Wp, D_, device=dev, generator=g)).to(torch.bfloat16)
    sh_ = (0.5 * torch.randn(B_, D_, device=dev, generator=g)).to(torch.bfloat16)
    sc_ = (0.5 * torch.randn(B_, D_, device=dev, generator=g)).to(torch.bfloat16)
    for posemb in (False, True):
        def run(lib):
            lib.g3_set_option(b"ln_wave_rows", wave)
            xx = x_.clone()
            q = torch.zeros(rows, D_, device=dev, dtype=torch.uint8)
            s = torch.zeros(rows, D_ // 32, device=dev, dtype=torch.uint8)
            if posemb:
                rc = lib.g3_posemb_layernorm_modulate_mxfp8(xx.data_ptr(), D_, pe.data_ptr(), None, None, None, T_, Hp, Wp, B_, sh_.data_ptr(), sc_.data_ptr(), D_, B_,
                                                            q.data_ptr(), D_, s.data_ptr(), D_ // 32, D_, 1e-6, st)
            else:
                rc = lib.g3_layernorm_modulate_mxfp8(xx.data_ptr(), D_, sh_.data_ptr(), sc_.data_ptr(), D_, B_, q.data_ptr(), D_, s.data_ptr(), D_ // 32, rows, D_, 1e-6, st)
            assert rc == 0, lib.g3_last_error()
            lib.g3_set_option(b"ln_wave_rows", LN_WAVE_START)
            return torch.cat([q.flatten(), s.flatten(), xx.view(torch.uint8).flatten()])
        a, b = both(run)
        report(f"LayerNorm -> MXFP8 rows={rows} D={D_} {'wave' if wave else 'workgroup'} form{' + position embedding' if posemb else ''}", a, b)
    del x_, pe, sh_, sc_
for lib in (base, alt):
    lib.g3_set_option(b"attn_variant", 0)
    lib.g3_set_option(b"gemm_pingpong", 3)
    lib.g3_set_option(b"gemm_persistent", 0)
    lib.g3_set_option(b"conv_w4", 1)
print("RACE SCREEN", "CLEAN" if bad == 0 else f"FOUND {bad} DIFFERENCES")
sys.exit(1 if bad else 0)
