"""Strided kernel entries with ONE operand far away: its rows spread over more than 2^31 (P31) or 2^32 (P32) bytes, or - for the operands a kernel
addresses relative to a 256-row tile - row 255 more than 2^32 bytes behind the tile's first (PT), inside the sentinel-filled arena of
tests/far_operands.py (whose docstring says why a wrong 32-bit offset then shows as a NaN or as a written sentinel, not as a stray access).

Rules every case keeps: the operands are seeded tensors at the smallest shape of the family's kernel-level file; one operand is far, the others
compact; where the entry has a dry run (g3_gemm_plan_bf16, g3_attn_plan_bf16, the MX name functions) it must name the kernel the case is meant for
BEFORE the call, so a case cannot silently run another row of a kernel table; the oracle is THE SAME ENTRY ON THE SAME VALUES AT COMPACT PITCH on
the very kernel the far call was planned onto - forced there by the existing options (gemm_pingpong, gemm_deferred, conv_w4, variant) where the far
call is planned elsewhere than the compact one - and every output must be BITWISE equal; after the call every input is unchanged, every float
output finite and every other byte of the arena still the fill. Compact launches run once per kernel and are shared. No tolerance is introduced.

g3_gemm_bf16_nt: classic LDS-DMA, classic register staging, ping-pong 2 and 4, one wave per SIMD (plain and persistent) and the deferred-epilogue
kernel, selected as tests/test_gemm_epilogue_kernels_gpu.py selects them; A, W, C, residual and gate (two rows) far in turn at P31 and P32, A and W
at PT; epilogues NONE and BIAS_RESIDUAL on every kernel (NONE and GATED_RESIDUAL on the deferred one, which has no bias form), GATED_RESIDUAL on
one kernel per epilogue copy. The deferred kernel applies from two tiles per workgroup of a one-per-CU grid on (w4e_applies; gemm_deferred_grid
changes the grid, not that rule), so its shape is the epilogue file's 8192 x 4096 x 2432, as is the persistent kernel's 8192 x 4096 x 128; PT
would span 128 GiB there: the persistent kernel gets PT at 257 x 65 536 x 128 (A) and 65 536 x 264 x 128 (W) - two tiles per workgroup through
N and through M -, the deferred kernel's bound is held by tests/test_gemm_plan_cpu.py alone. A two-row gate that is far at all lies beyond the
deferred kernel's 4 ldg 2 < 2^31: those cases assert the one-wave kernel and compare with it (gemm_deferred = 0).

THE DEFECT THIS FILE FOUND. The one-wave-per-SIMD kernels keep a tile row's LDS-DMA source as a 32-bit byte offset from the tile's first row
(gemm_w4.hpp, gemm_w4e.hpp), and the parent commit's plan put a call with 255 lda 2 >= 2^32 (or ldw) on them all the same. Measured on the parent's
library: "w4-epi0-A-PT", "w4-epi4-A-PT" (264 of 67 848 outputs not finite: row 255 of A read 4 GiB short, from the sentinel), "w4-epi0-W-PT"
(257: column 255) and "w4p-epi0-A-PT" (65 536) fail, "w4-epi0-A-P32" passes. gemm_choose / w4e_applies now bound lda and ldw
(255 ld 2 + 128 < 2^32); such a call runs on the ping-pong kernel, which forms 64-bit row pointers, and g3_gemm_qk_norm_rope_bf16 on that kernel
plus the standalone norm / RoPE / V^T passes. The PT cases (and the fused projection's A at P32: 256 rows) assert that plan and compare with a
compact launch forced onto it. No other defect: every other case was bitwise on the first run.

Other families. g3_gemm_qk_norm_rope_bf16 (A, W, C, vt_ld); norm / RoPE family, GEMV, unpatchify, GroupNorm (statistics, apply, fused), Haar
unpatcher, softmax rows, 2-D transpose, MX quantisers, the three block-scaled GEMMs (codes and scales separately, PT on the codes of A), head
scatter / gather at rows = 6 and 1030, g3_attn_merge_partials_bf16 (both parts through one pair of strides): every operand that has a leading
dimension. g3_conv3d_cl_gnstats_bf16 on its five kernel paths, one s3 and one t3s2 case: input, output, residual; g3_conv3d_cl_bf16 (the same
launcher without statistics) once per case and path with the input at P32. g3_spatial_attn_d512_bf16: V^T far by its row pitch and by
vt_frame_stride alone (both below the entry's own bound, which caps 8 rows at 4 GiB: what goes far is the 64-bit base of a row).

Attention (ATTN_KINDS): the census probe at Skv = 320, (B, H) = (2, 3) through every launching entry and kernel family of
tests/test_attn_probes_gpu.py - (1) g3_flash_attn_fwd_ex_bf16 on every variant 1..11 with a bf16 output, and on 4 and 11 with o_partial + lse;
(3) g3_cross_attn_fwd_bf16 with the in-kernel Q norm; (4) the no-max kernels, 32x32x16 and 16x16x32, and the no-max partial output; (5) the
key-skip form of the carry entries on variants 4 and 11 and without running max; (6) both frame-window kernels and the window entry under key
sharding; (7) both range-table kernels (g3_self_attn_fwd_ranges_bf16) at S = 320 - a 256-row and a 64-row query block over 5 tiles, two patterns,
head_pattern [1, 0, 1], no block attending every tile - with the table and head_pattern placed in the arena like every other operand, so a stray
access of the table walk lands on sentinel too. Each gets Q and O (or o_partial: fp32 at the same element strides) by row, batch and head at P31 and P32, K by row at P31 (inside
k_max: same kernel), V^T by head and by batch at P31, and K by row at P32: the 64-bit-addressing kernels keep it, the bf16-output plain and
bounded entries are planned onto variant 2, every other form must refuse with G3_ERR_ARG, name an entry and leave the whole arena untouched.
lse is contiguous [B][H][Sq] by the ABI (no stride): it is written beside a far o_partial, never far itself. The carry entries run without a
carry-in STATE: carry_o takes o's element strides as fp32, so a state beside a far bf16 o at P32 would span 8 GiB; the carry kernels' Q / K / V^T /
O addressing is what the key-skip cases run.

Not covered here, and why. g3_transpose_v_bf16's V^T side: the entry zero-fills every row up to ldvt, so a far ldvt IS a multi-GiB payload (the
V^T of the fused projection, which stops at the last 32-row block, is covered). g3_spatial_attn_d512_bf16 one step below either bound: the
operands span 4 GiB (Q, K, O) or 256 GiB (V^T); its refusals are held by tests/test_attn_plan_cpu.py. Segmented V^T (family 2 of that file) is not launched far. Where 256 or 300 input rows are spread over 4 GiB the convolution's plan bounds
(ld_in 2 < 2^31, ...) are still far away: tests/test_gemm_plan_cpu.py holds them; what switches at P32 is the one-wave kernel's tap change
(test_conv3d_one_operand_far). The convolution's weights (ldw) stay compact.

MEASURED on an MI355X (profiles/far_operand_parity_measured.txt, made before the range kinds; the figures here are of the run with them): 794 cases,
21.4 s for the whole file (module wall time, arena included; the slowest case 0.6 s; the 32 range cases and their two compact launches 1.4 s) -
tests/test_gemm_epilogue_kernels_gpu.py takes 7.8 s for its 46 cases on the parent commit. Kernels named by a plan: 18 GEMM
instantiations, 8 convolution instantiations, 18 attention kernels. EVERY case is bitwise equal to its compact oracle; no case needed a bar
instead. The GroupNorm statistics (fp64 atomics, up to 5 workgroups per frame) and the convolution's fused statistics were bitwise repeatable
between two compact launches in every run - sums of a handful of fp32 partials are exact in fp64 - so the fallback to the bar of
tests/test_tokenizer_kernels_gpu.py (2e-6 of |sum| + 1 against fp64 sums) never ran. The far K at P32 of the 11 kinds planned onto variant 2
is ADDITIONALLY held to the fp64 census probe at REL_EXACT_P = 2^-8 (tests/attn_probe_ref.py): worst relative error 3.7e-8, largest element
that should be zero 3.5e-10; 12 kinds refuse it with the arena untouched, the two 64-bit-addressing variants keep their kernel."""
import ctypes as C
import functools
import time

import pytest
import torch

from contextlib import contextmanager

from tests import far_operands as fo
from tests import gemm_ref as gr
from tests import tokenizer_kernel_ref as kr
from tests.gemm_ref import CLASSIC, PP2, PP4, REG, TWO_TILES, W4, W4E, W4P

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def arena():
    t0 = time.time()
    a = fo.Arena()
    yield a
    a.buf = None
    del a
    torch.cuda.empty_cache()
    print(f"[far] module wall time {time.time() - t0:.1f} s")


def _bits(t):
    return t.view(torch.int16)


def _lib():
    from gen3c_amd import _lib as L
    return L, L.load()


@contextmanager
def _options(**kw):
    """the options of a case, the library's defaults (gr.OPTION_DEFAULTS) put back behind it"""
    from gen3c_amd import ops
    try:
        for k, v in kw.items():
            ops.set_option(k, v)
        yield
    finally:
        for k, v in gr.OPTION_DEFAULTS.items():
            ops.set_option(k, v)


def _cus():
    L, lib = _lib()
    cus = C.c_int(0)
    L.check(lib.g3_device_info(0, C.byref(cus), None, None, 0), "g3_device_info")
    return cus.value


# =================================================================================================================================
# g3_gemm_bf16_nt
# =================================================================================================================================
RAGGED = gr.RAGGED[1]  # 257 x 264 x 192
GATE_ROWS = 2          # the smallest gate that has a pitch
# kernel -> (template the plan must name, the options that select it, shape, shape for PT on A, shape for PT on W, what PT is planned onto)
GEMM_KERNELS = {
    "classic": (CLASSIC, {"gemm_pingpong": 0}, RAGGED, RAGGED, RAGGED, CLASSIC),
    "regstage": (REG, {"gemm_regstage": 1}, RAGGED, RAGGED, RAGGED, REG),
    "pp2": (PP2, {"gemm_pingpong": 2}, RAGGED, RAGGED, RAGGED, PP2),
    "pp4": (PP4, {"gemm_pingpong": 1}, RAGGED, RAGGED, RAGGED, PP4),
    "w4": (W4, {}, RAGGED, RAGGED, RAGGED, PP2),
    "w4p": (W4P, {"gemm_persistent": 1}, (TWO_TILES, 4096, 128), (257, TWO_TILES, 128), (TWO_TILES, 264, 128), PP2),
    "w4e": (W4E, {"gemm_tokens_first": 0}, (TWO_TILES,) + gr.DEFERRED_NK, None, None, None),
}
# the options that put a COMPACT call on a kernel the far call was rerouted to
FORCE = {PP2: {"gemm_pingpong": 2}, W4: {"gemm_deferred": 0}}
EPI_OPERANDS = {0: ("A", "W", "C"), 2: ("A", "W", "C", "residual", "gate"), 4: ("A", "W", "C", "residual", "gate")}


def _gemm_cases():
    for kernel, row in GEMM_KERNELS.items():
        epis = (0, 2) if kernel == "w4e" else (0, 4) + ((2,) if kernel in ("classic", "pp2", "w4") else ())
        for epi in epis:
            for operand in EPI_OPERANDS[epi]:
                for pitch in ("P31", "P32") + (("PT",) if operand in "AW" and row[3] else ()):
                    yield pytest.param(kernel, epi, operand, pitch, id=f"{kernel}-epi{epi}-{operand}-{pitch}")


def _resolve(shape):
    """TWO_TILES as M beside N = 4096: the epilogue file's (gr.two_tiles_m); as the one long dimension beside a two-tile one (PT): 256 x the grid"""
    if shape[0] == TWO_TILES and shape[1] == 4096:
        return (gr.two_tiles_m(_cus()),) + tuple(shape[1:])
    return tuple(256 * (_cus() // 8 * 8) if d == TWO_TILES else d for d in shape)


def _gemm_call(L, a, w, out, epi, gate, residual):
    (M, K), N = a.shape, w.shape[0]
    return L.GemmCall(entry=0, A=a.data_ptr(), lda=a.stride(0), W=w.data_ptr(), ldw=w.stride(0), C=out.data_ptr(), ldc=out.stride(0), M=M, N=N, K=K,
                      epilogue=epi, gate=gate.data_ptr() if gate is not None else 0, gate_rows=gate.shape[0] if gate is not None else 1,
                      ldg=gate.stride(0) if gate is not None else 0, residual=residual.data_ptr() if residual is not None else 0,
                      ldr=residual.stride(0) if residual is not None else 0)


def _gemm_in_arena(arena, shape, epi, far=None, pitch=None):
    """place the operands (the far one last), ask the plan, launch, check the arena -> (planned kernel, output)"""
    from gen3c_amd import ops
    L, lib = _lib()
    M, N, K = shape
    a, w, gate4, res = gr.inputs(M, N, K, "randn")
    data = {"A": a, "W": w, "gate": gate4[:GATE_ROWS].contiguous(), "residual": res, "C": (M, N)}
    names = ["A", "W", "C"] + (["residual", "gate"] if epi else [])
    arena.reset()
    v = {}
    for name in sorted(names, key=lambda n: n == far):
        p = None
        if name == far:
            rows = data[name][0] if name == "C" else data[name].shape[0]
            p = fo.PITCHES[pitch](rows)
        v[name] = arena.place_rows(name, data[name], p, role="out" if name == "C" else "in")
    call = _gemm_call(L, v["A"], v["W"], v["C"], epi, v.get("gate"), v.get("residual"))
    planned = lib.g3_gemm_plan_bf16(C.byref(call), 0, None, None)
    assert planned is not None, L.last_error()
    ops.gemm_nt(v["A"], v["W"], out=v["C"], epilogue=epi, gate=v.get("gate"), residual=v.get("residual"))
    torch.cuda.synchronize()
    what = f"g3_gemm_bf16_nt {M}x{N}x{K} epi {epi} {far or 'compact'} {pitch or ''} on {planned.decode()}"
    return planned.decode(), arena.check(what)["C"]


_COMPACT = {}  # (kernel name, shape, epilogue) -> the compact launch's output: computed once, shared, never changed


def _compact(arena, tmpl, options, shape, epi):
    key = (tmpl.format(e=epi), shape, epi)
    if key not in _COMPACT:
        with _options(**options):
            name, out = _gemm_in_arena(arena, shape, epi)
        assert name == key[0], f"the compact launch under {options} was planned onto {name}, not {key[0]}"
        _COMPACT[key] = out
    return _COMPACT[key]


@pytest.mark.parametrize("kernel, epi, operand, pitch", list(_gemm_cases()))
def test_gemm_bf16_nt_one_operand_far(arena, kernel, epi, operand, pitch):
    tmpl, options, shape, shape_pt_a, shape_pt_w, tmpl_pt = GEMM_KERNELS[kernel]
    expect = tmpl
    if pitch == "PT":
        shape, expect = (shape_pt_a if operand == "A" else shape_pt_w), tmpl_pt
    if kernel == "w4e" and operand == "gate":
        expect = W4  # w4e_applies: 4 ldg 2 < 2^31 - a two-row gate that is far at all lies beyond it; the one-wave kernel takes the call
    shape = _resolve(shape)
    with _options(**options):
        name, out = _gemm_in_arena(arena, shape, epi, operand, pitch)
    print(f"[far] g3_gemm_bf16_nt {kernel} {shape} epi {epi} {operand} {pitch}: {name}")
    assert name == expect.format(e=epi), f"planned onto {name}, the case is meant for {expect.format(e=epi)}"
    want = _compact(arena, expect, options if expect == tmpl else {**options, **FORCE[expect]}, shape, epi)
    bad = int((_bits(out) != _bits(want)).sum())
    assert bad == 0, f"{bad} of {out.numel()} outputs differ from the compact launch of {name}"


# =================================================================================================================================
# the row-wise entries: norm / RoPE family, tokenizer, MX quantisers and GEMMs, head exchange
# =================================================================================================================================
u8, f32, f64 = torch.uint8, torch.float32, torch.float64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _randn(*shape, seed=0, scale=1.0, dtype=bf16):
    g = torch.Generator().manual_seed(7000 + seed)
    return (scale * torch.randn(*shape, generator=g)).to(dtype)


def _codes(rows, cols, seed, top=0x77):
    """random e4m3 / e2m3 code bytes without the e4m3 NaN (0x7F, 0xFF): magnitude <= top, random sign"""
    g = torch.Generator().manual_seed(7100 + seed)
    return (torch.randint(0, top + 1, (rows, cols), generator=g) + 128 * torch.randint(0, 2, (rows, cols), generator=g)).to(u8)


def _scales(rows, cols, seed):
    g = torch.Generator().manual_seed(7200 + seed)
    return torch.randint(125, 130, (rows, cols), generator=g).to(u8)  # E8M0 bytes around 2^0


def _flat(t):
    return t.reshape(1, -1)


def _p(t, elements=0):
    return t.data_ptr() + elements * t.element_size()


def e_layernorm(place, lib, mx=False, posemb=False):
    rows, D, mod_rows = 6, 256, 2
    x = place("x", _randn(rows, D, seed=1), role="inout" if posemb else "in")
    mod = place("mod", _randn(mod_rows, 2 * D, seed=2, scale=0.5))  # shift | scale: column views of one buffer, as the DiT's modulation GEMV leaves them
    head = (_p(x), x.stride(0))
    if posemb:  # the finished-table form: T Hp Wp = 3 positions, B = 2
        pe_c = place("pe_dense", _flat(_randn(3, D, seed=3, scale=0.1)))
        head += (_p(pe_c), None, None, None, 1, 1, 3, 2)
    mods = (_p(mod), _p(mod, D), mod.stride(0), mod_rows)
    if mx:
        q, s = place("q", (rows, D), dtype=u8, role="out"), place("scales", (rows, D // 32), dtype=u8, role="out")
        tail = (_p(q), q.stride(0), _p(s), s.stride(0))
    else:
        out = place("out", (rows, D), role="out")
        tail = (_p(out), out.stride(0))
    if posemb:
        fn = lib.g3_posemb_layernorm_modulate_mxfp8 if mx else lib.g3_posemb_layernorm_modulate_bf16
        return fn(*head, *mods, *tail, D, 1e-6, _stream())
    fn = lib.g3_layernorm_modulate_mxfp8 if mx else lib.g3_layernorm_modulate_bf16
    return fn(*head, *mods, *tail, rows, D, 1e-6, _stream())


def e_qk_rmsnorm_rope(place, lib, H=2, pair=False):
    S, B = 3, 2
    x = place("in", _randn(S * B, H * 128, seed=4))
    wq, wk = place("wq", _flat(_randn(128, seed=5))), place("wk", _flat(_randn(128, seed=6)))
    g = torch.Generator().manual_seed(7007)
    ang = torch.rand(S, 128, generator=g) * 6.0
    cos, sin = place("cos", _flat(torch.cos(ang))), place("sin", _flat(torch.sin(ang)))
    out = place("out", (S * B, H * 128), role="out")
    if pair:
        return lib.g3_qk_rmsnorm_rope_pair_bf16(_p(x), x.stride(0), _p(wq), H // 2, _p(wk), H // 2, _p(cos), _p(sin), _p(out), out.stride(0), S, B, 128, 1e-6, _stream())
    return lib.g3_qk_rmsnorm_rope_bf16(_p(x), x.stride(0), _p(wq), _p(cos), _p(sin), _p(out), out.stride(0), S, B, H, 128, 1e-6, _stream())


def e_transpose_v(place, lib):
    S, B, H = 5, 2, 2  # ldvt = 8: three zero-filled positions per row
    v = place("v", _randn(S * B, H * 128, seed=8))
    vt = place("vt", (B * H * 128, 8), role="out", dense=True)  # the entry zero-fills a row up to ldvt: the rows are dense, ldvt = 8
    return lib.g3_transpose_v_bf16(_p(v), v.stride(0), _p(vt), vt.stride(0), S, B, H, 128, _stream())


def e_gemv(place, lib):
    M, N, K = 4, 24, 256
    a, w, add = place("a", _randn(M, K, seed=9)), place("w", _randn(N, K, seed=10, scale=1 / 16)), place("add", _randn(M, N, seed=11))
    out = place("out", (M, N), role="out")
    return lib.g3_gemv_bf16(_p(a), a.stride(0), _p(w), w.stride(0), _p(add), add.stride(0), _p(out), out.stride(0), M, N, K, 1, _stream())


def e_unpatchify(place, lib):
    B, Co, T, H, W, pt, ps = 2, 16, 2, 4, 4, 1, 2
    y = place("y", _randn((T // pt) * (H // ps) * (W // ps) * B, ps * ps * pt * Co, seed=12))
    out = place("out", (1, B * Co * T * H * W), role="out")
    return lib.g3_dit_unpatchify_bf16(_p(y), y.stride(0), _p(out), B, Co, T, H, W, pt, ps, _stream())


def _gn_operands(place, rows):
    frames, Cc = 3, 64
    xd = _randn(frames * rows, Cc, seed=13)
    x = place("x", xd)
    gamma, beta = place("gamma", _flat(_randn(Cc, seed=14))), place("beta", _flat(_randn(Cc, seed=15)))
    xf = xd.double().reshape(frames, -1)
    return frames, Cc, x, gamma, beta, torch.stack([xf.sum(1), (xf * xf).sum(1)], 1)


def e_gn_stats(place, lib, rows=5):
    frames, Cc, x, _, _, _ = _gn_operands(place, rows)
    stats = place("stats", torch.zeros(1, frames * 2, dtype=f64), role="inout")  # [frames][2] dense; the entry adds to what the buffer holds
    return lib.g3_groupnorm_stats_cl_bf16(_p(x), x.stride(0), _p(stats), frames, rows, Cc, _stream())


def e_gn_apply(place, lib, rows=5):
    frames, Cc, x, gamma, beta, sums = _gn_operands(place, rows)
    stats = place("stats", _flat(sums))
    out = place("out", (frames * rows, Cc), role="out")
    return lib.g3_groupnorm_apply_cl_bf16(_p(x), x.stride(0), _p(gamma), _p(beta), _p(stats), _p(out), out.stride(0), frames, rows, Cc, 1e-6, 1, _stream())


def e_gn_swish(place, lib, rows=5):
    frames, Cc, x, gamma, beta, _ = _gn_operands(place, rows)
    stats = place("stats", (1, frames * 2), dtype=f64, role="out")  # [frames][2] dense; the fused entry zeroes them itself
    out = place("out", (frames * rows, Cc), role="out")
    return lib.g3_groupnorm_swish_cl_bf16(_p(x), x.stride(0), _p(gamma), _p(beta), _p(stats), _p(out), out.stride(0), frames, rows, Cc, 1e-6, 1, _stream())


def e_haar_unpatch(place, lib):
    Tp, Hp, Wp = 2, 2, 3
    coef = place("coef", _randn(Tp * Hp * Wp, 192, seed=16))
    video = place("video", (1, 3 * (4 * Tp - 3) * 4 * Hp * 4 * Wp), role="out")
    return lib.g3_haar3d_unpatch_bf16(_p(coef), coef.stride(0), _p(video), Tp, Hp, Wp, _stream())


def e_softmax_rows(place, lib, n=40):
    x = place("x", _randn(6, n, seed=17, scale=3.0), role="inout")
    return lib.g3_softmax_rows_bf16(_p(x), x.stride(0), 6, n, 0.5, _stream())


def e_transpose2d(place, lib):
    R, Cc = 70, 10  # two row tiles of 64
    x = place("in", _randn(R, Cc, seed=18))
    out = place("out", (Cc, R), role="out")
    return lib.g3_transpose2d_bf16(_p(x), x.stride(0), _p(out), out.stride(0), R, Cc, _stream())


def e_quant_mx(place, lib, fp6=False):
    M, K = 6, 64
    x = place("x", _randn(M, K, seed=19, scale=4.0))
    q, s = place("q", (M, 3 * K // 4 if fp6 else K), dtype=u8, role="out"), place("scales", (M, K // 32), dtype=u8, role="out")
    fn = lib.g3_quant_mxfp6_bf16 if fp6 else lib.g3_quant_mxfp8_bf16
    return fn(_p(x), x.stride(0), _p(q), q.stride(0), _p(s), s.stride(0), M, K, _stream())


def e_gemm_mx(place, lib, form="mxfp8"):
    M, N, K = 257, 256, 128
    kb = 3 * K // 4 if form == "mxfp6" else K
    aq, as_ = place("aq", _codes(M, kb, 20, 0xFF if form == "mxfp6" else 0x77)), place("as", _scales(M, K // 32, 21))
    wq, ws = place("wq", _codes(N, kb, 22, 0xFF if form == "mxfp6" else 0x77)), place("ws", _scales(N, K // 32, 23))
    ops_ = (_p(aq), aq.stride(0), _p(as_), as_.stride(0), _p(wq), wq.stride(0), _p(ws), ws.stride(0))
    name = {"mxfp8": lib.g3_gemm_mxfp8_kernel_name, "mxout": lib.g3_gemm_mxfp8_mxout_kernel_name, "mxfp6": lib.g3_gemm_mxfp6_kernel_name}[form](M, N, K, 0)
    want = {"mxfp8": b"gemm_mxfp8_nt_kernel<0>", "mxout": b"gemm_mxfp8_nt_kernel<256>", "mxfp6": b"gemm_mxfp6_nt_kernel<0>"}[form]
    assert name == want, (name, want)
    if form == "mxout":
        q, s = place("q", (M, N), dtype=u8, role="out"), place("scales", (M, N // 32), dtype=u8, role="out")
        return lib.g3_gemm_mxfp8_nt_mxout(*ops_, _p(q), q.stride(0), _p(s), s.stride(0), M, N, K, 0, _stream())
    c = place("c", (M, N), role="out")
    fn = lib.g3_gemm_mxfp6_nt if form == "mxfp6" else lib.g3_gemm_mxfp8_nt
    return fn(*ops_, _p(c), c.stride(0), M, N, K, 0, None, 1, 0, None, 0, _stream())


def e_cp_scatter(place, lib, rows=6):
    H, n, head0, Hg = 8, 4, 0, 2
    qkv = place("qkv", _randn(rows, 3 * H * 128, seed=24))
    outs = [place(f"{x}_out", (1, n * rows * Hg * 128), role="out") for x in "qkv"]
    return lib.g3_cp_scatter_heads_bf16(_p(qkv), _p(qkv, H * 128), _p(qkv, 2 * H * 128), qkv.stride(0), *[_p(o) for o in outs], rows, H, n, head0, Hg, _stream())


def e_cp_gather(place, lib, rows=6):
    H, n, head0, Hg = 8, 4, 0, 2
    x = place("in", _flat(_randn(n * rows, Hg * 128, seed=25)))
    out = place("out", (rows, H * 128), role="out")
    return lib.g3_cp_gather_heads_bf16(_p(x), _p(out), out.stride(0), rows, H, n, head0, Hg, _stream())


def e_d512(place, lib, by_frame=False):
    """two frames of hw = 64 positions. V^T [frames][512][ld_vt]: far by its row pitch (1024 rows of one pitch, vt_frame_stride = 512 ld_vt), or -
    by_frame - by vt_frame_stride alone, the rows of a frame compact. Both stay below the entry's bound 8 ld_vt 2 < 2^32 (the pitch of 1024 rows
    spread over 4 GiB is 4 MiB): what goes far is the 64-bit base of a row, and a signed or truncated product in forming it would show."""
    frames, hw = 2, 64
    q, k = place("q", _randn(frames * hw, 512, seed=40, scale=0.5), dense=True), place("k", _randn(frames * hw, 512, seed=41, scale=0.5), dense=True)
    o = place("o", (frames * hw, 512), role="out", dense=True)
    vt_data = _randn(frames * 512, hw, seed=42)
    if by_frame:
        row = 2 * hw + 16
        frame = fo.PITCHES[place.pitch](frames) if place.far == "vt" else 512 * row + 16
        vt = place.arena.place("vt", (frames, 512, hw), (frame, row, 2), bf16, vt_data.reshape(frames, 512, hw))
        place.placed.append("vt")
        ld_vt, fs = row // 2, frame // 2
    else:
        vt = place("vt", vt_data)
        ld_vt, fs = vt.stride(0), 512 * vt.stride(0)
    return lib.g3_spatial_attn_d512_bf16(_p(q), _p(k), _p(vt), ld_vt, fs, _p(o), frames, hw, 2.0 ** -5 / 1.4426950408889634, _stream())


QK_FUSED, QK_UNFUSED = "gemm_bf16_nt_w4_kernel<5, false>", "gemm_bf16_nt_pp_kernel<0, 2, false>"


def e_gemm_qk(place, lib, rerouted=False):
    """One q, one k and one v head at 256 x 384 x 128, V^T written by the epilogue: the plan must name the one-wave kernel's norm / RoPE epilogue.
    rerouted: with 256 rows of A, P32 is PT - row 255 starts beyond 2^32 - and the plan must put the call on the ping-pong kernel followed by the
    standalone norm / RoPE and V^T passes; the compact oracle is forced onto that chain with gemm_pingpong = 2 (the fused and the unfused chain
    agree to a rounding, not bitwise: tests/test_kernels_gpu.py). The fused epilogue leaves C's v columns unwritten, the chain writes them."""
    L, _ = _lib()
    S, B, N, K = 128, 2, 384, 128
    M = S * B
    a, w = place("A", _randn(M, K, seed=30)), place("W", _randn(N, K, seed=31, scale=1 / 11))
    wq, wk = place("wq", _flat(_randn(128, seed=5))), place("wk", _flat(_randn(128, seed=6)))
    g = torch.Generator().manual_seed(7032)
    ang = torch.rand(S, 128, generator=g) * 6.0
    cos, sin = place("cos", _flat(torch.cos(ang))), place("sin", _flat(torch.sin(ang)))
    c = place("C", (M, N if rerouted else 256), role="out", min_pitch=2 * N + 16)
    vt = place("vt", (B * 128, S), role="out", dense=True)
    with _options(**({"gemm_pingpong": 2} if rerouted and not place.far else {})):
        call = L.GemmCall(entry=1, A=_p(a), lda=a.stride(0), W=_p(w), ldw=w.stride(0), C=_p(c), ldc=c.stride(0), M=M, N=N, K=K, n_q=128, n_k=128, norm_q=_p(wq),
                          norm_k=_p(wk), cos_table=_p(cos), sin_table=_p(sin), B=B, eps=1e-6, vt=_p(vt), vt_ld=vt.stride(0))
        follow = C.c_uint(0)
        planned = lib.g3_gemm_plan_bf16(C.byref(call), 0, None, C.byref(follow))
        assert planned is not None, L.last_error()
        print(f"[far] g3_gemm_qk_norm_rope_bf16: {planned.decode()} follow-up {follow.value}")
        assert planned.decode() == (QK_UNFUSED if rerouted else QK_FUSED) and bool(follow.value) == rerouted, (planned, follow.value)
        return lib.g3_gemm_qk_norm_rope_bf16(_p(a), a.stride(0), _p(w), w.stride(0), _p(c), c.stride(0), M, N, K, 128, 128, _p(wq), _p(wk), _p(cos), _p(sin), B, 1e-6,
                                             _p(vt), vt.stride(0), _stream())


P = functools.partial
# entry -> (the call, the operands that have a leading dimension, those of them that also get PT)
ROW_ENTRIES = {
    "g3_layernorm_modulate_bf16": (e_layernorm, ("x", "mod", "out"), ()),
    "g3_layernorm_modulate_mxfp8": (P(e_layernorm, mx=True), ("x", "mod", "q", "scales"), ()),
    "g3_posemb_layernorm_modulate_bf16": (P(e_layernorm, posemb=True), ("x", "mod", "out"), ()),
    "g3_posemb_layernorm_modulate_mxfp8": (P(e_layernorm, mx=True, posemb=True), ("x", "mod", "q", "scales"), ()),
    "g3_qk_rmsnorm_rope_bf16": (e_qk_rmsnorm_rope, ("in", "out"), ()),
    "g3_qk_rmsnorm_rope_bf16/octet": (P(e_qk_rmsnorm_rope, H=8), ("in", "out"), ()),
    "g3_qk_rmsnorm_rope_pair_bf16": (P(e_qk_rmsnorm_rope, H=2, pair=True), ("in", "out"), ()),
    "g3_qk_rmsnorm_rope_pair_bf16/octet": (P(e_qk_rmsnorm_rope, H=16, pair=True), ("in", "out"), ()),
    "g3_gemm_qk_norm_rope_bf16": (e_gemm_qk, ("A", "W", "C", "vt"), ()),
    "g3_gemm_qk_norm_rope_bf16/rerouted": (P(e_gemm_qk, rerouted=True), ("A",), ()),
    "g3_transpose_v_bf16": (e_transpose_v, ("v",), ()),
    "g3_gemv_bf16": (e_gemv, ("a", "w", "add", "out"), ()),
    "g3_dit_unpatchify_bf16": (e_unpatchify, ("y",), ()),
    "g3_groupnorm_stats_cl_bf16": (e_gn_stats, ("x",), ()),
    "g3_groupnorm_stats_cl_bf16/5 blocks": (P(e_gn_stats, rows=1030), ("x",), ()),
    "g3_groupnorm_apply_cl_bf16": (e_gn_apply, ("x", "out"), ()),
    "g3_groupnorm_apply_cl_bf16/1030 rows": (P(e_gn_apply, rows=1030), ("x", "out"), ()),
    "g3_groupnorm_swish_cl_bf16": (e_gn_swish, ("x", "out"), ()),
    "g3_haar3d_unpatch_bf16": (e_haar_unpatch, ("coef",), ()),
    "g3_softmax_rows_bf16": (e_softmax_rows, ("x",), ()),
    "g3_softmax_rows_bf16/generic": (P(e_softmax_rows, n=37), ("x",), ()),
    "g3_transpose2d_bf16": (e_transpose2d, ("in", "out"), ()),
    "g3_quant_mxfp8_bf16": (e_quant_mx, ("x", "q", "scales"), ()),
    "g3_quant_mxfp6_bf16": (P(e_quant_mx, fp6=True), ("x", "q", "scales"), ()),
    "g3_gemm_mxfp8_nt": (e_gemm_mx, ("aq", "as", "wq", "ws", "c"), ("aq",)),
    "g3_gemm_mxfp8_nt_mxout": (P(e_gemm_mx, form="mxout"), ("aq", "as", "wq", "ws", "q", "scales"), ("aq",)),
    "g3_gemm_mxfp6_nt": (P(e_gemm_mx, form="mxfp6"), ("aq", "as", "wq", "ws", "c"), ("aq",)),
    "g3_spatial_attn_d512_bf16": (e_d512, ("vt",), ()),
    "g3_spatial_attn_d512_bf16/frame stride": (P(e_d512, by_frame=True), ("vt",), ()),
    "g3_cp_scatter_heads_bf16": (e_cp_scatter, ("qkv",), ()),
    "g3_cp_scatter_heads_bf16/1030 rows": (P(e_cp_scatter, rows=1030), ("qkv",), ()),
    "g3_cp_gather_heads_bf16": (e_cp_gather, ("out",), ()),
    "g3_cp_gather_heads_bf16/1030 rows": (P(e_cp_gather, rows=1030), ("out",), ()),
}


def _row_cases():
    for entry, (_, operands, tiled) in ROW_ENTRIES.items():
        for operand in operands:
            for pitch in ("P31", "P32") + (("PT",) if operand in tiled else ()):
                if entry.startswith("g3_gemm_qk_norm_rope_bf16") and operand == "A" and (pitch == "P32") != entry.endswith("/rerouted"):
                    continue  # 256 rows of A: P32 is PT, where the plan leaves the fused kernel (e_gemm_qk); W's 384 rows are two tiles, each spanning less
                yield pytest.param(entry, operand, pitch, id=f"{entry}-{operand}-{pitch}")


def _run_entry(arena, entry, far=None, pitch=None):
    L, lib = _lib()
    arena.reset()
    placed = []

    def place(name, data_or_shape, role="in", dtype=bf16, dense=False, min_pitch=None):
        """dense: compact rows without sentinel behind them (an entry that fills a row up to its leading dimension); min_pitch: a column view"""
        rows, cols = data_or_shape.shape if isinstance(data_or_shape, torch.Tensor) else data_or_shape
        placed.append(name)
        p = fo.PITCHES[pitch](rows) if name == far else cols * torch.empty((), dtype=dtype).element_size() if dense else min_pitch
        return arena.place_rows(name, data_or_shape, p, dtype=dtype, role=role)

    place.far, place.pitch, place.arena, place.placed = far, pitch, arena, placed

    rc = ROW_ENTRIES[entry][0](place, lib)
    assert rc == 0, f"{entry}: rc {rc}: {L.last_error()}"
    torch.cuda.synchronize()
    assert far is None or far in placed
    return arena.check(f"{entry} {far or 'compact'} {pitch or ''}")


def got_rows(entry):
    return 1030 if entry.endswith(("5 blocks", "1030 rows")) else 5


_COMPACT_ROWS = {}  # entry -> (outputs of its compact launch, bitwise repeatable?): once, shared, never changed


def _bytes_equal(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(u8) == b.contiguous().view(u8)).all())


@pytest.mark.parametrize("entry, operand, pitch", list(_row_cases()))
def test_rowwise_entry_one_operand_far(arena, entry, operand, pitch):
    """Entries without a plan: one launcher, whose choice of kernel (where it has one) reads shapes and alignment, never a stride's size. The
    compact launch runs twice, once for all cases of an entry: were its result not bitwise repeatable (the GroupNorm statistics are added with
    fp64 atomics by up to 5 workgroups per frame in the '5 blocks' case; measured: repeatable, sums of fp32 partials are exact in fp64) the
    statistics would fall back to the bar of tests/test_tokenizer_kernels_gpu.py, |stat - fp64 sum| / (|sum| + 1) < 2e-6."""
    if entry not in _COMPACT_ROWS:
        first, second = _run_entry(arena, entry), _run_entry(arena, entry)
        _COMPACT_ROWS[entry] = (first, all(_bytes_equal(first[k], second[k]) for k in first))
    want, repeatable = _COMPACT_ROWS[entry]
    got = _run_entry(arena, entry, operand, pitch)
    print(f"[far] {entry} {operand} {pitch}: outputs {sorted(got)} {'bitwise' if repeatable else 'NOT REPEATABLE: bar'}")
    assert sorted(got) == sorted(want)
    for name in got:
        if repeatable or name != "stats":
            assert _bytes_equal(got[name], want[name]), f"output {name!r} differs from the compact launch"
        else:  # the cited bar: against the fp64 sums of the input (both statistics entries run e_gn's three frames of 64 channels)
            xf = _randn(3 * got_rows(entry), 64, seed=13).double().reshape(3, -1)
            ref = torch.stack([xf.sum(1), (xf * xf).sum(1)], 1).reshape(1, -1).to(got[name].device)
            assert float(((got[name] - ref).abs() / (ref.abs() + 1.0)).max()) < 2e-6


# =================================================================================================================================
# attention: every launching entry, every kernel family of tests/test_attn_probes_gpu.py (1, 3, 4, 5, 6, 7)
# =================================================================================================================================
from tests import attn_probe_ref as R  # noqa: E402

SQ, SKV, AB, AH = 200, 320, 2, 3  # the census probe of tests/test_attn_probes_gpu.py at Skv = 320, Sq = 200, (B, H) = (2, 3)
WIN = dict(frame_len=64, W=0, s=0)  # S = 320 = 5 frames of 64: block 0 (frames 0..3) attends 4 frames, block 1 the last one - never every key
# kind -> (entry, variant, Sq, what a far K at P32 must do: the "same" kernel (64-bit addressing already), the "v2" kernel, or be "refused")
ATTN_KINDS = {f"ex_v{v}": ("ex", v, SQ, "same" if v < 3 else "v2") for v in range(1, 12)}  # family 1: every variant, bf16 output
ATTN_KINDS.update({
    "partial_v4": ("ex_partial", 4, SQ, "refused"), "partial_v11": ("ex_partial", 11, SQ, "refused"),  # family 1: o_partial + lse
    "cross": ("cross", 0, SQ, "refused"),                                                              # family 3: in-kernel Q norm
    "nm": ("bounded", 11, SQ, "v2"), "nm16": ("bounded16", 11, SQ, "v2"), "nm_partial": ("bounded_partial", 11, SQ, "refused"),  # family 4
    "skip_v4": ("carry", 4, SQ, "refused"), "skip_v11": ("carry", 11, SQ, "refused"), "nm_skip": ("bounded_cp", 11, SQ, "refused"),  # family 5
    "win_nm": ("window", 11, SKV, "refused"), "win_max": ("window_max", 11, SKV, "refused"), "win_cp": ("window_cp", 11, 128, "refused"),  # family 6
    "rng_nm": ("ranges", 11, SKV, "refused"), "rng_max": ("ranges_max", 11, SKV, "refused"),                                              # family 7
})
# family 7: S = 320 is a 256-row and a 64-row query block over 5 tiles; two patterns in tiles, head_pattern [1, 0, 1], max_ranges 4, and no block
# attends every tile. The table and head_pattern are operands in the arena (8- and 4-byte aligned: the arena aligns to 16).
RNG_LISTS = [[[(0, 1), (2, 2)], [(1, 1), (4, 1)]], [[(1, 3)], [(0, 2), (3, 1), (4, 1)]]]
RNG_HEAD_PATTERN, RNG_MAX_RANGES = [1, 0, 1], 4
assert all(sum(n for _f, n in rl) < SKV // 64 for blocks in RNG_LISTS for rl in blocks)
SKIP = (64, 64)  # family 5: the keys [64, 128) of the 320 in K / V^T are skipped, S_kv = 256 attended
ATTN_DIMS = {"q": ("head", "batch", "row"), "o": ("head", "batch", "row"), "k": ("head", "batch", "row"), "vt": ("row", "head", "batch")}  # innermost first
# (operand, the dimension whose stride is far, pitch). K by row: P31 stays inside the kernels' 32-bit budget (k_max of attn_plan) - the same kernel
# must run and be right; P32 is beyond it. V^T by head / batch at P31. "o" is the bf16 output, or o_partial (fp32, the same element strides).
ATTN_FAR = [("q", d, p) for d in ("row", "batch", "head") for p in ("P31", "P32")] + [("o", d, p) for d in ("row", "batch", "head") for p in ("P31", "P32")] + \
           [("k", "row", "P31"), ("k", "row", "P32"), ("vt", "head", "P31"), ("vt", "batch", "P31")]
REFUSAL_NAMES = ("g3_flash_attn_fwd_ex_bf16:", "g3_cross_attn_fwd_bf16:", "g3_flash_attn_fwd_carry_bf16:", "g3_self_attn_fwd_window_bf16:",
                 "g3_self_attn_fwd_window_cp_bf16:", "g3_self_attn_fwd_ranges_bf16:")


@functools.lru_cache(maxsize=4)
def _attn_probe(Sq):
    p = R.census_position(Sq, SKV, AB, AH)
    ref, _ = R.reference(p) if Sq == SQ else (None, None)
    g = torch.Generator().manual_seed(7400)
    return {"q": p.q.to(bf16), "k": p.k.to(bf16), "vt": p.v.permute(1, 2, 3, 0).contiguous().to(bf16), "wq": (0.5 + torch.rand(1, R.HD, generator=g)).to(bf16)}, ref


def _attn_strides(operand, Sq, inner_bytes, far_dim=None, pitch=None):
    """byte strides by dimension name: compact nesting (16 bytes of sentinel behind every level), the far dimension outermost at its pitch"""
    n = {"head": AH, "batch": AB, "row": R.HD if operand == "vt" else SKV if operand == "k" else Sq}
    reach, strides = inner_bytes, {}
    for dim in [d for d in ATTN_DIMS[operand] if d != far_dim]:
        strides[dim] = reach + 16
        reach += strides[dim] * (n[dim] - 1)
    if far_dim:
        strides[far_dim] = fo.PITCHES[pitch](n[far_dim])
        assert strides[far_dim] >= reach
    return strides


def _attn_launch(lib, entry, variant, a):
    """-> (the dry run's answer, the launching entry's status); a: the placed operands as ABI arguments"""
    q, k, vt, o, o32, lse, os_, wq, Sq = a["q"], a["k"], a["vt"], a["o"], a["o32"], a["lse"], a["os"], a["wq"], a["Sq"]
    bound = R.BOUND_NATS if entry in ("bounded", "bounded16", "bounded_partial", "bounded_cp", "window", "window_cp", "ranges") else 0.0
    shape, sc, st = (AB, AH, R.HD), R.SOFTMAX_SCALE, _stream()
    if entry in ("window", "window_max"):
        args = (*q, *k, *vt, o, *os_, Sq, *shape, sc, bound, WIN["frame_len"], WIN["W"], WIN["s"])
        return lib.g3_attn_window_plan_bf16(*args), lib.g3_self_attn_fwd_window_bf16(*args, st)
    if entry in ("ranges", "ranges_max"):
        args = (*q, *k, *vt, o, *os_, Sq, *shape, sc, bound, a["ranges"], len(RNG_LISTS), RNG_MAX_RANGES, a["head_pattern"])
        return lib.g3_attn_ranges_plan_bf16(*args), lib.g3_self_attn_fwd_ranges_bf16(*args, st)
    if entry == "window_cp":  # this rank's queries: frames 3 and 4 of 5; the buffer holds all five (a = b = 0), W = 1: frames 2..4 attended
        args = (*q, *k, *vt, o, *os_, Sq, SKV, *shape, sc, bound, WIN["frame_len"], 5, 3, 0, 0, 1, 0)
        return lib.g3_attn_window_cp_plan_bf16(*args), lib.g3_self_attn_fwd_window_cp_bf16(*args, st)
    skip = SKIP if entry in ("carry", "bounded_cp") else (0, 0)
    Skv = SKV - skip[1]
    code = {"ex": 3, "ex_partial": 3, "cross": 2, "bounded": 4, "bounded16": 4, "bounded_partial": 4, "carry": 5, "bounded_cp": 6}[entry]
    plan = lib.g3_attn_plan16_bf16 if entry == "bounded16" else lib.g3_attn_plan_bf16
    planned = plan(code, *q, wq if entry == "cross" else None, 1e-6, *k, *vt, 0, 0, *skip, None, None, o, o32, lse, *os_, Sq, Skv, 0, *shape, sc, bound, variant)
    outs = (o, o32, lse, *os_, Sq, Skv)
    if entry == "cross":
        rc = lib.g3_cross_attn_fwd_bf16(*q, wq, 1e-6, *k, *vt, o, *os_, Sq, Skv, 0, *shape, sc, st)
    elif entry in ("ex", "ex_partial"):
        rc = lib.g3_flash_attn_fwd_ex_bf16(*q, *k, *vt, 0, 0, *outs, *shape, sc, variant, st)
    elif entry in ("bounded", "bounded_partial"):
        rc = lib.g3_self_attn_fwd_bounded_bf16(*q, *k, *vt, 0, 0, *outs, *shape, sc, bound, variant, st)
    elif entry == "bounded16":
        rc = lib.g3_self_attn_fwd_bounded16_bf16(*q, *k, *vt, 0, 0, *outs, *shape, sc, bound, variant, st)
    elif entry == "carry":
        rc = lib.g3_flash_attn_fwd_carry_bf16(*q, *k, *vt, 0, 0, *skip, None, None, *outs, *shape, sc, variant, st)
    else:
        rc = lib.g3_self_attn_fwd_bounded_cp_bf16(*q, *k, *vt, 0, 0, *skip, None, None, *outs, *shape, sc, bound, variant, st)
    return planned, rc


def _attn_in_arena(arena, entry, variant, Sq, far=None, refused=False):
    """-> (planned kernel, {output name: tensor}); refused: the call must return G3_ERR_ARG, name an entry and leave the whole arena untouched"""
    L, lib = _lib()
    data, _ = _attn_probe(Sq)
    partial = entry.endswith("_partial")
    arena.reset()
    v, es = {}, {}
    for operand in sorted(("q", "k", "vt", "o"), key=lambda n: bool(far) and n == far[0]):
        size, dt = (4, f32) if operand == "o" and partial else (2, bf16)
        s = _attn_strides(operand, Sq, size * (SKV if operand == "vt" else R.HD), *(far[1:] if far and far[0] == operand else ()))
        if operand == "vt":
            shape, order = (AB, AH, R.HD, SKV), ("batch", "head", "row")
        else:
            shape, order = (SKV if operand == "k" else Sq, AB, AH, R.HD), ("row", "batch", "head")
        v[operand] = arena.place(operand, shape, tuple(s[d] for d in order) + (size,), dt, data.get(operand), role="out" if operand == "o" else "in")
        es[operand] = tuple(s[d] // size for d in ("row", "batch", "head"))
    wq = arena.place_rows("wq", data["wq"])
    lse = arena.place_rows("lse", (1, AB * AH * Sq), dtype=f32, role="out") if partial else None
    a = {n: (_p(v[n]), *es[n]) for n in ("q", "k", "vt")}
    a.update(o=None if partial else _p(v["o"]), o32=_p(v["o"]) if partial else None, lse=_p(lse) if partial else None, os=es["o"], wq=_p(wq), Sq=Sq)
    if entry in ("ranges", "ranges_max"):
        tab = arena.place_rows("ranges", torch.from_numpy(R.pack(RNG_LISTS, RNG_MAX_RANGES)).reshape(1, -1))
        hp = arena.place_rows("head_pattern", torch.tensor([RNG_HEAD_PATTERN], dtype=torch.int32))
        assert _p(tab) % 8 == 0 and _p(hp) % 4 == 0
        a.update(ranges=_p(tab), head_pattern=_p(hp))
    planned, rc = _attn_launch(lib, entry, variant, a)
    torch.cuda.synchronize()
    what = f"attention {entry} variant {variant} {far or 'compact'}"
    if refused:
        assert planned is None and rc == L.G3_ERR_ARG and L.last_error().startswith(REFUSAL_NAMES), (planned, rc, L.last_error())
        arena.assert_untouched(what)
        return None, None
    assert planned is not None and rc == 0, (planned, rc, L.last_error())
    return planned.decode(), arena.check(f"{what} on {planned.decode()}")


_COMPACT_ATTN = {}  # kind -> (planned name, outputs): once, shared, never changed


def _compact_attn(arena, kind):
    if kind not in _COMPACT_ATTN:
        entry, variant, Sq, _ = ATTN_KINDS.get(kind, ("ex", 2, SQ, None))
        _COMPACT_ATTN[kind] = _attn_in_arena(arena, entry, variant, Sq)
    return _COMPACT_ATTN[kind]


def test_attention_kinds_reach_the_kernels_they_are_meant_for(arena):
    """the compact launches: one kernel per kind, the carry / window / no-max / 16x16x32 / cross forms among them, every variant of family 1"""
    names = {kind: _compact_attn(arena, kind)[0] for kind in ATTN_KINDS}
    print("[far] attention kinds: " + ", ".join(f"{k} = {n}" for k, n in names.items()))
    L, lib = _lib()
    for kind, (entry, variant, Sq, _) in ATTN_KINDS.items():
        if entry == "ex":
            assert names[kind] == lib.g3_flash_attn_kernel_name_ex(Sq, SKV, AB, AH, variant).decode(), kind
    assert names["skip_v4"] == "flash_attn_fwd_v3_kernel<3, 6, 8, false>" != names["ex_v4"] and names["skip_v11"] == "flash_attn_fwd_w4b_carry_kernel<true>", names
    assert names["nm_skip"] == "flash_attn_fwd_w4b_nm_carry_kernel<true>", names
    assert names["nm"] == names["nm_partial"] == "flash_attn_fwd_w4b_nm_kernel<true>" and names["nm16"] == "flash_attn_fwd_w4c_nm_kernel", names
    assert names["win_nm"] == names["win_cp"] == "flash_attn_fwd_w4b_nm_win_kernel<true>" and names["win_max"] == "flash_attn_fwd_w4b_win_kernel<true>", names
    assert names["rng_nm"] == "flash_attn_fwd_w4b_nm_rng_kernel<true>" and names["rng_max"] == "flash_attn_fwd_w4b_rng_kernel<true>", names
    assert names["partial_v11"] == names["ex_v11"] and names["partial_v4"] == names["ex_v4"] == names["cross"], names


@pytest.mark.parametrize("operand, dim, pitch", ATTN_FAR, ids=[f"{o}-by-{d}-{p}" for o, d, p in ATTN_FAR])
@pytest.mark.parametrize("kind", list(ATTN_KINDS))
def test_attention_one_operand_far(arena, kind, operand, dim, pitch):
    """K by row at P32: the plain and bounded entries with a bf16 output are planned onto the 64-bit-addressing kernel (variant 2), compared bitwise
    with a compact launch forced there (variant = 2) AND - the one case of this file that is also held to an fp64 reference - with the census
    probe's fp64 result at the bar tests/test_attn_probes_gpu.py gives the running-max kernels on that probe (REL_EXACT_P = 2^-8). Every form that
    has no 64-bit kernel (partial outputs, cross, carry / key skip, both window entries, the range-table entry) must refuse it, name an entry and write nothing; the
    refusals' texts are held by tests/test_attn_carry_gpu.py, test_attn_bounded_cp_gpu.py and test_attn_plan_cpu.py."""
    L, lib = _lib()
    entry, variant, Sq, k_p32 = ATTN_KINDS[kind]
    beyond = (operand, pitch) == ("k", "P32") and k_p32 != "same"
    if beyond and k_p32 == "refused":
        _attn_in_arena(arena, entry, variant, Sq, (operand, dim, pitch), refused=True)
        return
    name_c, want = _compact_attn(arena, kind)
    name, got = _attn_in_arena(arena, entry, variant, Sq, (operand, dim, pitch))
    print(f"[far] attention {kind} {operand} by {dim} {pitch}: {name}")
    if beyond:
        v2 = lib.g3_flash_attn_kernel_name_ex(Sq, SKV, AB, AH, 2).decode()
        assert name == v2 and "v2" in v2, (name, v2)
        name_c, want = _compact_attn(arena, "ex_v2")
        assert name_c == v2
        ref = _attn_probe(Sq)[1]
        ok, rel, small = R.out_errors(got["o"].cpu(), ref, R.REL_EXACT_P)
        print(f"[far] attention {kind} k by row P32 on {name}: against the fp64 census probe rel {rel:.3e}, small {small:.3e}")
        assert ok, R.first_bad(got["o"].cpu(), ref, R.REL_EXACT_P)
    else:
        assert name == name_c, f"planned onto {name}, the compact launch ran {name_c}"
    assert sorted(got) == sorted(want)
    for out in got:
        assert _bytes_equal(got[out], want[out]), f"output {out!r} differs from the compact launch of {name}"


# ---- g3_attn_merge_partials_bf16: two parts (one pair of strides for both) and the output far by row, batch and head -----------------------------------
MERGE_DIMS = {"parts": (("head", AH), ("batch", AB), ("part", 2), ("row", 6)), "out": (("head", AH), ("batch", AB), ("row", 6))}
MERGE_FAR = [(o, d, p) for o in ("parts", "out") for d in ("row", "batch", "head") for p in ("P31", "P32")]


def _merge_in_arena(arena, far=None):
    L, lib = _lib()
    Sq = 6
    arena.reset()
    g = torch.Generator().manual_seed(7300)
    parts = torch.rand(Sq, 2, AB, AH, R.HD, generator=g)
    lse = 4.0 * torch.randn(2, AB * AH * Sq, generator=g)
    v, st = {}, {}
    for operand, size, dt in (("parts", 4, f32), ("out", 2, bf16)):
        reach, s = size * R.HD, {}
        fd = far[1] if far and far[0] == operand else None
        for dim, n in [d for d in MERGE_DIMS[operand] if d[0] != fd]:
            s[dim] = reach + 16
            reach += s[dim] * (n - 1)
        if fd:
            s[fd] = fo.PITCHES[far[2]](dict(MERGE_DIMS[operand])[fd])
        st[operand] = s
        if operand == "parts":
            v[operand] = arena.place("parts", (Sq, 2, AB, AH, R.HD), (s["row"], s["part"], s["batch"], s["head"], 4), f32, parts)
        else:
            v[operand] = arena.place("out", (Sq, AB, AH, R.HD), (s["row"], s["batch"], s["head"], 2), bf16, role="out")
    lse_d = arena.place_rows("lse", lse)
    op = (C.c_void_p * 2)(_p(v["parts"]), _p(v["parts"]) + st["parts"]["part"])
    lp = (C.c_void_p * 2)(_p(lse_d), _p(lse_d, lse_d.stride(0)))
    p, o = st["parts"], st["out"]
    rc = lib.g3_attn_merge_partials_bf16(op, lp, 2, p["row"] // 4, p["batch"] // 4, p["head"] // 4, _p(v["out"]), o["row"] // 2, o["batch"] // 2, o["head"] // 2,
                                         Sq, AB, AH, R.HD, _stream())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    return arena.check(f"g3_attn_merge_partials_bf16 {far or 'compact'}")["out"]


@pytest.mark.parametrize("operand, dim, pitch", MERGE_FAR, ids=[f"{o}-by-{d}-{p}" for o, d, p in MERGE_FAR])
def test_attn_merge_partials_one_operand_far(arena, operand, dim, pitch):
    if "merge" not in _COMPACT_ROWS:
        _COMPACT_ROWS["merge"] = (_merge_in_arena(arena), True)
    out = _merge_in_arena(arena, (operand, dim, pitch))
    assert _bytes_equal(out, _COMPACT_ROWS["merge"][0]), "the output differs from the compact launch"


# =================================================================================================================================
# g3_conv3d_cl_gnstats_bf16 on its five kernel paths: input, output and residual far
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def _conv_operands(name):
    """the operands tests/test_tokenizer_kernels_gpu.py builds for the case (same seed), without its fp64 reference"""
    kind, K, N, T, H, W, epi = kr.CONV_CASES[name][:7]
    x, w, b, r = kr.conv_operands(kind, K, N, T, H, W, seed=sum(map(ord, name)))
    return x, w, (b if epi != "none" else None), (r if epi == "res" else None)


CONV_FAR = {"one_tile_padded": ("input", "output", "residual"), "t3s2_T5": ("input", "output")}  # one s3 and one t3s2 case of kr.CONV_CASES (the second has no residual)
CONV_KERNELS = {"w4_gaps": "gemm_bf16_nt_w4_conv_kernel<{e}>", "w4_stmt": "gemm_bf16_nt_w4_conv_kernel<{e}>", "pingpong": "gemm_bf16_nt_pp_kernel<{e}, 2, true>",
                "lds_dma": "gemm_bf16_nt_kernel<{e}, true, true, false>", "direct": "gemm_bf16_nt_kernel<{e}, false, true, false>"}


def _tap_in_gaps(rows_in, ld_in_bytes, opts):
    """gemm_w4_conv.hpp's condition for changing taps inside the K loop, restated: the 32-bit form needs the whole input inside 4 GiB"""
    return opts.get("conv_w4", 1) == 1 and rows_in < 1 << 24 and rows_in * ld_in_bytes + 128 < 1 << 32 and ld_in_bytes < 1 << 24


def _conv_in_arena(arena, name, opts, far=None, pitch=None, stats_entry=True):
    """-> (planned kernel, tap change in the gaps?, {output, stats}); stats_entry False: g3_conv3d_cl_bf16, the same launcher without statistics"""
    L, lib = _lib()
    kind, K, N, T, H, W, epi = kr.CONV_CASES[name][:7]
    x, w, b, r = _conv_operands(name)
    To, Ho, Wo = kr.conv_out_shape(kind, T, H, W)
    M = To * Ho * Wo
    arena.reset()
    pf = lambda op, rows: fo.PITCHES[pitch](rows) if far == op else None
    wt = arena.place_rows("w", kr.pack_taps(w, K + 8, fill=0.0).reshape(-1, K + 8)[:, :K].contiguous(), 2 * (K + 8))
    bias = arena.place_rows("bias", b.reshape(1, -1)) if b is not None else None
    res = arena.place_rows("residual", r.reshape(M, N), pf("residual", M)) if r is not None else None
    stats = arena.place_rows("stats", torch.zeros(1, To * 2, dtype=f64), role="inout" if stats_entry else "in")
    out = arena.place_rows("output", (M, N), pf("output", M), role="out")
    xin = arena.place_rows("input", x.reshape(T * H * W, K), pf("input", T * H * W))
    geom = kr.CONV_GEOM[kind]
    with _options(**opts):
        call = L.GemmCall(entry=3 if stats_entry else 2, A=_p(xin), lda=xin.stride(0), W=_p(wt), ldw=wt.stride(0), C=_p(out), ldc=out.stride(0), N=N, K=K, gate=_p(bias) if bias is not None else 0,
                          residual=_p(res) if res is not None else 0, ldr=res.stride(0) if res is not None else 0, Ti=T, Hi=H, Wi=W, To=To, Ho=Ho, Wo=Wo,
                          **dict(zip("kt kh kw st sh sw ot oh ow".split(), geom)), gn_stats=_p(stats), gn_rows=Ho * Wo)
        planned = lib.g3_gemm_plan_bf16(C.byref(call), 0, None, None)
        assert planned is not None, L.last_error()
        args = (_p(xin), xin.stride(0), _p(wt), wt.stride(0), _p(bias) if bias is not None else None, _p(res) if res is not None else None,
                res.stride(0) if res is not None else 0, _p(out), out.stride(0), K, N, T, H, W, To, Ho, Wo, *geom)
        rc = lib.g3_conv3d_cl_gnstats_bf16(*args, _p(stats), Ho * Wo, _stream()) if stats_entry else lib.g3_conv3d_cl_bf16(*args, _stream())
        assert rc == 0, L.last_error()
        torch.cuda.synchronize()
    gaps = b"w4_conv" in planned and _tap_in_gaps(T * H * W, 2 * xin.stride(0), opts)  # (the one-wave kernel's alone)
    return planned.decode(), gaps, arena.check(f"g3_conv3d_cl_gnstats_bf16 {name} {opts} {far or 'compact'} {pitch or ''}")


def _conv_cases():
    for name, operands in CONV_FAR.items():
        for path in kr.CONV_PATHS:
            for operand in operands:
                for pitch in ("P31", "P32"):
                    yield pytest.param(name, path, operand, pitch, id=f"{name}-{path}-{operand}-{pitch}")


_COMPACT_CONV = {}


@pytest.mark.parametrize("path", list(kr.CONV_PATHS))
@pytest.mark.parametrize("name", list(CONV_FAR))
def test_conv3d_plain_entry_input_far(arena, name, path):
    """g3_conv3d_cl_bf16 - the same launcher with no statistics buffer - once per case and path, the input at P32: the kernel the statistics
    entry names, and the output of the statistics entry's compact launch, bit for bit; the statistics buffer it is not given stays as it was."""
    opts = kr.CONV_PATHS[path]
    kernel, gaps, got = _conv_in_arena(arena, name, opts, "input", "P32", stats_entry=False)
    name_c, _, want = _conv_in_arena(arena, name, opts if not ("w4_conv" in kernel and opts.get("conv_w4") == 1) else kr.CONV_PATHS["w4_stmt"])
    print(f"[far] g3_conv3d_cl_bf16 {name} {path} input P32: {kernel}")
    assert kernel == name_c == CONV_KERNELS[path].format(e={"none": 0, "bias": 3, "res": 4}[kr.CONV_CASES[name][6]])
    assert _bytes_equal(got["output"], want["output"]), "the output differs from the statistics entry's compact launch"


@pytest.mark.parametrize("name, path, operand, pitch", list(_conv_cases()))
def test_conv3d_one_operand_far(arena, name, path, operand, pitch):
    """The bounds of conv_w4_applies (ld_in 2 < 2^31, rows < 2^31, N ldw 2 < 2^32) lie beyond what a 256- or 300-row input can be spread to
    inside the arena - tests/test_gemm_plan_cpu.py holds them -, so every far call keeps its compact call's kernel, asserted. What does switch is
    the one-wave kernel's tap change: in the MFMA gaps with 32-bit offsets while the whole input lies inside 4 GiB (P31), between statements
    with 64-bit addresses beyond (input at P32; the condition is restated in _tap_in_gaps) - the far launch is then compared with the compact
    launch of THAT form (conv_w4 = 2). Statistics: bitwise where the compact launch is bitwise repeatable (checked once per path), else the
    bar of tests/test_tokenizer_kernels_gpu.py (2e-6 of |sum| + 1 against fp64 sums of the stored output)."""
    opts = kr.CONV_PATHS[path]
    epi = {"none": 0, "bias": 3, "res": 4}[kr.CONV_CASES[name][6]]

    def compact(o):
        key = (name, tuple(sorted(o.items())))
        if key not in _COMPACT_CONV:
            n1, g1, first = _conv_in_arena(arena, name, o)
            _, _, second = _conv_in_arena(arena, name, o)
            assert _bytes_equal(first["output"], second["output"])
            _COMPACT_CONV[key] = (n1, g1, first, _bytes_equal(first["stats"], second["stats"]))
        return _COMPACT_CONV[key]

    kernel, gaps, got = _conv_in_arena(arena, name, opts, operand, pitch)
    assert kernel == CONV_KERNELS[path].format(e=epi), (kernel, path)
    oracle = opts
    if path == "w4_gaps":
        assert gaps == (not (operand == "input" and pitch == "P32")), "the restated tap_in_gaps condition does not switch where the case means it to"
        oracle = opts if gaps else kr.CONV_PATHS["w4_stmt"]
    name_c, gaps_c, want, repeatable = compact(oracle)
    assert name_c == kernel and gaps_c == gaps
    form = f" tap change {'in the gaps' if gaps else 'between statements'}," if "w4_conv" in kernel else ""
    print(f"[far] g3_conv3d_cl_gnstats_bf16 {name} {path} {operand} {pitch}: {kernel}{form} statistics {'bitwise' if repeatable else 'NOT REPEATABLE: bar'}")
    assert _bytes_equal(got["output"], want["output"]), "the output differs from the compact launch"
    if repeatable:
        assert _bytes_equal(got["stats"], want["stats"]), "the statistics differ from the compact launch"
    else:
        of = got["output"].double().reshape(got["stats"].numel() // 2, -1)
        ref = torch.stack([of.sum(1), (of * of).sum(1)], dim=1).reshape(1, -1)
        e = float(((got["stats"] - ref).abs() / (ref.abs() + 1.0)).max())
        print(f"[far] ... statistics rel err {e:.2e}")
        assert e < 2e-6
