"""The five copies of the block GEMM's epilogue - store_tile and store_tile_lds (gemm_epilogue.hpp), the one-wave-per-SIMD kernel's (gemm_w4.hpp),
the deferred one (gemm_w4e.hpp) and the block-scaled GEMM's (gemm_mx.hip) - through gen3c_amd.ops / the C ABI, against the fp64 references of
tests/gemm_ref.py (which tests/test_gemm_ref_cpu.py pins against fp64 torch, and whose mutants it shows caught on these very inputs).

Rules every test here keeps (those of tests/test_norm_rope_kernels_gpu.py): operands are bf16 tensors built on the CPU from seeded generators and
feed kernel and reference alike; A and W have NaN behind every row, gate and residual are column views of wider NaN-filled tensors; every output
lives in a NaN-guarded buffer (tests/guarded.py) that must come back untouched around a finite payload; before every call the dry run
g3_gemm_plan_bf16 must name the kernel the case is meant for; options are restored to the library's defaults in try / finally.

Two stages per case, each one rounding (gr.check: |out - ref| <= 0.5 bf16_ulp(ref) + C E per element, share of elements != bf16_round(ref) at most
max(10 x the fp32 restatement's, 1e-3), C E > 0.5 ulp on at most 5 %):
  1  EPI_NONE, EPI_BIAS, EPI_BIAS_RESIDUAL against a @ w^T (+ bias) (+ R) in fp64, C_GEMM = 16;
  2  on y = the kernel's own EPI_NONE output: EPI_GELU against 0.5 y erfc(-y / sqrt 2), C_GELU = 1; EPI_GATED_RESIDUAL bitwise bf16(fp32(R + g y))
     and within 0.5 ulp + 2^-24 |ref| of the fp64 value.
Cases above 1024 rows are checked on 256 of them (gr.tile_rows: the edges of the first, a middle and the last M tile and a spread), their
references evaluated in float64 on the device; the gated residual's bitwise bar always holds on every row.
Measured on an MI355X (profiles/gemm_epilogue_parity_measured.txt): the Linear's worst (err - 0.5 ulp) / E is 7.59 of C_GEMM = 16 (deferred kernel,
same-sign operands, K = 2432, 1 M outputs; below 3 in every other case); GELU's is 0.243 in every copy, the restatement's own figure; the swept
GELU differs from bf16_round(gelu64(y)) on 169 of 65 279 values (restatement: 167), none with |y| <= 2; the gated residual is bitwise
bf16(fp32(R + g y)) everywhere; bf16 subnormals pass the matrix core unflushed and -0 comes back as +0. No defect found."""
import ctypes as C
from contextlib import contextmanager

import pytest
import torch

from tests import gemm_ref as gr
from tests.gemm_ref import CLASSIC, PP2, PP4, REG, TWO_TILES, W4, W4E, W4E_TF, W4P  # (shared with tests/test_far_operands_gpu.py)
from tests.guarded import Guarded, _dev
from tests.test_kernels_gpu import _GEMM_OPTION_DEFAULTS

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEFAULTS = dict(_GEMM_OPTION_DEFAULTS, gemm_wide_store=1, gemm_deferred=1)
# epilogue copy -> (kernel the plan must name, the options that select it, its smallest shape, epilogues, gate rows, the sweep's shape)
COPIES = {
    "store_tile/pp2": (PP2, {"gemm_wide_store": 0}, gr.SMALL, range(5), (1, 2), (256, 256, 256)),
    "store_tile/classic": (CLASSIC, {"gemm_wide_store": 0, "gemm_pingpong": 0}, gr.SMALL, range(5), (1, 2), (256, 256, 256)),
    "store_tile_lds/classic": (CLASSIC, {"gemm_pingpong": 0}, gr.SMALL, range(5), (1, 2), (256, 256, 256)),
    "store_tile_lds/pp2": (PP2, {"gemm_pingpong": 2}, gr.SMALL, range(5), (1, 2), (256, 256, 256)),
    "store_tile_lds/pp4": (PP4, {"gemm_pingpong": 1}, gr.SMALL, range(5), (1, 2), (256, 256, 256)),
    "gemm_w4": (W4, {}, gr.K128, range(5), (1, 2), (256, 256, 256)),
    "gemm_w4/persistent": (W4P, {"gemm_persistent": 1}, (TWO_TILES, 4096, 128), range(5), (1, 2), (TWO_TILES, 4096, 128)),
    "gemm_w4e": (W4E, {"gemm_tokens_first": 0}, (TWO_TILES,) + gr.DEFERRED_NK, range(3), (1, 2, 4), (TWO_TILES,) + gr.DEFERRED_NK),
    "gemm_w4e/tokens_first": (W4E_TF, {"gemm_tokens_first": 1}, (TWO_TILES,) + gr.DEFERRED_NK, range(3), (1, 2, 4), (TWO_TILES,) + gr.DEFERRED_NK),
}
# the ragged and strided cases of the non-deferred kernels -> (kernel, options, shape, families)
RAGGED = {
    "300x260x136 ragged M, N % 8 == 4, K tail": (REG, {}, gr.RAGGED[0], gr.FAMILIES),
    "257x264x192 w4": (W4, {}, gr.RAGGED[1], gr.FAMILIES),
    "257x264x192 classic": (CLASSIC, {"gemm_pingpong": 0}, gr.RAGGED[1], gr.FAMILIES),
    "257x264x192 pp2": (PP2, {"gemm_pingpong": 2}, gr.RAGGED[1], gr.FAMILIES),
    "257x264x192 pp4": (PP4, {"gemm_pingpong": 1}, gr.RAGGED[1], gr.FAMILIES),
    "257x264x192 narrow": (PP2, {"gemm_wide_store": 0}, gr.RAGGED[1], gr.FAMILIES),
    "56x1024x4096 w4": (W4, {}, gr.RAGGED[2], gr.FAMILIES[:1]),
    "56x1024x4096 classic": (CLASSIC, {"gemm_pingpong": 0}, gr.RAGGED[2], gr.FAMILIES[:1]),
    "56x1024x4096 pp2": (PP2, {"gemm_pingpong": 2}, gr.RAGGED[2], gr.FAMILIES[:1]),
}


def _lib():
    from gen3c_amd import _lib as L
    return L, L.load()


@contextmanager
def _options(**kw):
    from gen3c_amd import ops
    try:
        for k, v in kw.items():
            ops.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            ops.set_option(k, v)


def _shape(shape):
    if shape[0] != TWO_TILES:
        return shape
    L, lib = _lib()
    cus = C.c_int(0)
    L.check(lib.g3_device_info(0, C.byref(cus), None, None, 0), "g3_device_info")
    return (gr.two_tiles_m(cus.value),) + tuple(shape[1:])


def _bits(t):
    return t.view(torch.int16)


def _view(t, pad, front=0):
    """t [R][C] (CPU) -> its device copy as a column view [:, front : front + C] of a NaN-filled [R][front + C + pad] tensor"""
    buf = torch.full((t.shape[0], front + t.shape[1] + pad), float("nan"), dtype=t.dtype, device=_dev())
    buf[:, front:front + t.shape[1]] = t.to(_dev())
    return buf[:, front:front + t.shape[1]]


def _gemm(tmpl, a, w, out, epi, gate=None, residual=None):
    """the dry run must name tmpl's instantiation for exactly this call; then the call"""
    from gen3c_amd import ops
    L, lib = _lib()
    (M, K), N = a.shape, w.shape[0]
    call = L.GemmCall(entry=0, A=a.data_ptr(), lda=a.stride(0), W=w.data_ptr(), ldw=w.stride(0), C=out.data_ptr(), ldc=out.stride(0), M=M, N=N, K=K,
                      epilogue=epi, gate=gate.data_ptr() if gate is not None else 0, gate_rows=gate.shape[0] if gate is not None else 1,
                      ldg=gate.stride(0) if gate is not None else 0, residual=residual.data_ptr() if residual is not None else 0,
                      ldr=residual.stride(0) if residual is not None else 0)
    planned = lib.g3_gemm_plan_bf16(C.byref(call), 0, None, None)
    assert planned is not None and planned.decode() == tmpl.format(e=epi), (planned, tmpl.format(e=epi), L.last_error())
    ops.gemm_nt(a, w, out=out, epilogue=epi, gate=gate, residual=residual)
    torch.cuda.synchronize()
    return planned.decode()


def _record(what, kernel, figures):
    print("[parity] " + gr.format_row(what, kernel, *figures))


def _run_case(label, tmpl, options, shape, family, epis, gate_rows, alias=False):
    M, N, K = _shape(shape)
    a, w, gate4, res = gr.inputs(M, N, K, family)
    narrow = bool(N % 8) or options.get("gemm_wide_store", 1) == 0
    ldc = N + (4 if narrow else 8)  # a narrow case may as well have an output row stride that is no multiple of 8
    a_d, w_d = _view(a, 8), _view(w, 8)
    gate_d = _view(gate4, N, front=N)      # columns [N, 2 N) of a [4][3 N] tensor
    res_d = _view(res, 8)
    sel = gr.tile_rows(M)
    on_dev = M > 1024
    sel_d = sel.to(_dev())
    what = f"{label} {M}x{N}x{K} {family}"

    def run(epi, rows=1, out=None, residual=None):
        out = out or Guarded(M, N, ldc)
        g = gate_d[:rows] if epi >= 2 else None
        r = (residual if residual is not None else res_d) if epi in (2, 4) else None
        name = _gemm(tmpl, a_d, w_d, out.payload, epi, g, r)
        out.assert_only_payload_written(f"{what} epi {epi} gate_rows {rows}")
        return out, name

    with _options(**options):
        y_g, name0 = run(0)
        # ---- stage 1 ----
        a_s, w_s = (a_d[sel_d].contiguous(), w_d.contiguous()) if on_dev else (a[sel], w)
        gate_s, res_s = (gate_d, res_d[sel_d]) if on_dev else (gate4, res[sel])
        acc = gr.linear_acc32(a_s, w_s)
        ref, E = gr.linear_ref(a_s, w_s)
        y = y_g.payload[sel_d].cpu()
        _record(f"{what} none", name0, gr.check(f"{what} EPI_NONE", y, ref.cpu(), E.cpu(), gr.C_GEMM, acc.to(bf16).cpu()))
        for epi in (3, 4):
            if epi not in epis:
                continue
            for rows in gate_rows:
                out, name = run(epi, rows)
                bias = gate_s[:rows][(sel_d if on_dev else sel) % rows]  # one bias row per checked row
                r = res_s if epi == 4 else None
                ref, E = gr.linear_ref(a_s, w_s, bias, r)
                fig = gr.check(f"{what} epi {epi} gate_rows {rows}", out.payload[sel_d].cpu(), ref.cpu(), E.cpu(), gr.C_GEMM, gr.linear_fp32(a_s, w_s, bias, r, acc=acc).cpu())
                _record(f"{what} {'bias' if epi == 3 else 'bias_residual'} rows {rows}", name, fig)
                if alias and epi == 4:
                    inplace = Guarded(M, N, ldc, data=res)
                    run(epi, rows, out=inplace, residual=inplace.payload)
                    assert torch.equal(_bits(inplace.payload), _bits(out.payload)), f"{what} epi 4: out aliasing the residual changes the result"
        # ---- stage 2, on the kernel's own EPI_NONE output ----
        if 1 in epis:
            out, name = run(1)
            ref, E = gr.gelu_ref(y)
            _record(f"{what} gelu", name, gr.check(f"{what} EPI_GELU", out.payload[sel_d].cpu(), ref, E, gr.C_GELU, gr.gelu_fast32(y)))
        if 2 in epis:
            for rows in gate_rows:
                out, name = run(2, rows)
                want = gr.gated_fp32(y_g.payload, gate_d[:rows], res_d)  # on the device, every row
                bad = int((_bits(out.payload) != _bits(want)).sum())
                assert bad == 0, f"{what} gate_rows {rows}: {bad} of {M * N} elements are not bf16(fp32(R + g y))"
                g_exp = gate4[:rows][sel % rows]
                ref, E = gr.gated_ref(y, g_exp, res[sel])
                fig = gr.check(f"{what} EPI_GATED_RESIDUAL gate_rows {rows}", out.payload[sel_d].cpu(), ref, E, 1.0, gr.gated_fp32(y, g_exp, res[sel]))
                _record(f"{what} gated_residual rows {rows} (bitwise)", name, fig)
                if alias:
                    inplace = Guarded(M, N, ldc, data=res)
                    run(2, rows, out=inplace, residual=inplace.payload)
                    assert torch.equal(_bits(inplace.payload), _bits(out.payload)), f"{what} epi 2: out aliasing the residual changes the result"


# =================================================================================================================================
# every epilogue copy at the smallest shape that reaches it
# =================================================================================================================================
@pytest.mark.parametrize("family", gr.FAMILIES)
@pytest.mark.parametrize("copy", list(COPIES))
def test_every_epilogue_copy_at_its_smallest_shape(copy, family):
    """Each copy of the epilogue under the selection of _GEMM_ROW_FAMILIES (tests/test_kernels_gpu.py) at the smallest shape that reaches it - the
    narrow store_tile under gemm_wide_store = 0, store_tile_lds in the classic and both ping-pong kernels at 256 x 256 x 64, gemm_w4.hpp plain at
    K = 128 and persistent at two tiles per workgroup, gemm_w4e.hpp in both piece orders at K = 2432 -, every epilogue it has, gate rows 1 and 2
    (1, 2, 4 on the deferred kernel), on randn, same-sign and tail-filling operands."""
    tmpl, options, shape, epis, gate_rows, _ = COPIES[copy]
    _run_case(copy, tmpl, options, shape, family, epis, gate_rows)


# =================================================================================================================================
# ragged and strided cases
# =================================================================================================================================
@pytest.mark.parametrize("case", list(RAGGED))
def test_ragged_shapes_strided_views_gate_rows_and_in_place_residual(case):
    """(300, 260, 136): a ragged second M tile, N % 8 == 4 (the narrow store with a ragged N tile) and K % 64 == 8 (register staging with an 8-wide
    zero-filled tail, NaN behind it); (257, 264, 192): one row in the second M tile, a wide store with a ragged N tile, in every kernel family;
    (56, 1024, 4096): 64 K tiles. All five epilogues; gate rows 1, 2, 3, 4 (row m % rows; the restated m / rows is a mutant the CPU test shows
    caught); out (ldc = N + 8, N + 4 where the store is narrow), gate (ldg = 3 N) and residual (ldr = N + 8) are column views; EPI_GATED_RESIDUAL
    and EPI_BIAS_RESIDUAL once more with out aliasing the residual, bitwise equal."""
    tmpl, options, shape, families = RAGGED[case]
    for family in families:
        _run_case(case, tmpl, options, shape, family, range(5), (1, 2, 3, 4), alias=True)


# =================================================================================================================================
# the sweep: every finite bf16 value through each copy's GELU
# =================================================================================================================================
def _sweep_figures(what, kernel, y_d, g_d, count):
    """y_d / g_d: the EPI_NONE and EPI_GELU outputs (device, same shape). The GELU output must be a function of y alone; then one value per
    distinct y goes through gr.check_sweep."""
    yb, gb = gr.bits_of(y_d.reshape(-1)), gr.bits_of(g_d.reshape(-1))
    lut = torch.full((65536,), -1, dtype=torch.int64, device=y_d.device)
    lut[yb] = gb
    spread = int((lut[yb] != gb).sum())
    assert spread == 0, f"{what}: {spread} outputs differ from another output with the same pre-activation"
    present = (lut >= 0).cpu()
    assert int(present.sum()) >= count, f"{what}: only {int(present.sum())} distinct pre-activations"
    y = gr.all_bf16()[present]
    g = lut.cpu()[present].to(torch.int16).view(bf16)
    fig = gr.check_sweep(what, y, g)
    _record(f"{what}: {y.numel()} values", kernel, fig)


@pytest.mark.parametrize("copy", list(COPIES))
def test_gelu_over_every_finite_bf16_value_per_epilogue_copy(copy):
    """A = the 65 280 finite bf16 values in bit-pattern order (wrapped), W[n][k] = (k == n % K): every output is one exact product plus zeros.
    Stage 1: EPI_NONE returns every normal value bit for bit; what comes back for -0 and the subnormals is recorded and used as y, not asserted.
    Stage 2 (gr.check_sweep): the GELU output against gelu64(y) per element with C_GELU = 1 and the restatement's share (167 of 65 280) as
    yardstick; exactly bf16_round(gelu64(y)) for |y| <= 2 off the near-tie list; exactly 0 for y <= -14."""
    tmpl, options, _, _, _, shape = COPIES[copy]
    M, N, K = _shape(shape)
    a, w = gr.sweep_inputs(M, N, K)
    a_d, w_d = _view(a, 8), _view(w, 8)
    ldc = N + (4 if options.get("gemm_wide_store", 1) == 0 else 8)
    what = f"{copy} sweep {M}x{N}x{K}"
    with _options(**options):
        y_g, g_g = Guarded(M, N, ldc), Guarded(M, N, ldc)
        _gemm(tmpl, a_d, w_d, y_g.payload, 0)
        kernel = _gemm(tmpl, a_d, w_d, g_g.payload, 1)
    y_g.assert_only_payload_written(what)
    g_g.assert_only_payload_written(what + " gelu")
    sent = a_d[:, torch.arange(N, device=_dev()) % K]
    normal = sent.float().abs() >= 2.0 ** -126
    bad = int((_bits(y_g.payload)[normal] != _bits(sent)[normal]).sum())
    assert bad == 0, f"{what}: {bad} normal values do not come back bit for bit from EPI_NONE"
    sub = ~normal
    back, went = gr.bits_of(y_g.payload[sub]), gr.bits_of(sent[sub])
    kept = int((back == went).sum())
    zeros = {f"{int(b):#06x}": int((back == b).sum()) for b in (0x0000, 0x8000)}
    neg0 = back[went == 0x8000]
    print(f"[parity] {what}: stage 1 returned {int(sub.sum())} outputs for +-0 and the subnormals: {kept} bit for bit, {zeros} as zeros; "
          f"-0 came back as {sorted({f'{int(b):#06x}' for b in neg0.unique()})}")
    _sweep_figures(what, kernel, y_g.payload, g_g.payload, 65000)


def test_mxfp8_gelu_over_every_bf16_value_above_2_pow_minus_120():
    """g3_gemm_mxfp8_nt (bf16 output) on hand-built operands, no quantiser: x = +-1.m x 2^e, e >= -120, as the e4m3 pair ((8 + m[6:4]) 16, m[3:0])
    under the E8M0 scale 2^(e - 7) against a weight of two ones - 63 488 values, eight per row at 7936 x 256 x 256. The host shows dequant of the
    operands to be x exactly (tests/test_gemm_ref_cpu.py too); stage 1 asserts the same of the device's EPI_NONE output; stage 2 is the sweep's."""
    from gen3c_amd import ops
    from tests.mxfp8_ref import dequant_mxfp8
    L, lib = _lib()
    x, aq, as_, wq, ws = gr.mx_sweep_inputs()
    M, N, K = aq.shape[0], wq.shape[0], aq.shape[1]
    assert torch.equal(dequant_mxfp8(aq, as_).double().reshape(M, 8, 32).sum(-1), x.double())
    names = [lib.g3_gemm_mxfp8_kernel_name(M, N, K, e) for e in (0, 1)]
    assert [n.decode() if n else n for n in names] == ["gemm_mxfp8_nt_kernel<0>", "gemm_mxfp8_nt_kernel<1>"], (names, L.last_error())
    dev = _dev()
    ops_in = [t.to(dev) for t in (aq, as_, wq, ws)]
    y_g, g_g = Guarded(M, N, N + 8), Guarded(M, N, N + 8)
    ops.gemm_mxfp8_nt(*ops_in, out=y_g.payload, epilogue=0)
    ops.gemm_mxfp8_nt(*ops_in, out=g_g.payload, epilogue=1)
    torch.cuda.synchronize()
    what = f"gemm_mx sweep {M}x{N}x{K}"
    y_g.assert_only_payload_written(what)
    g_g.assert_only_payload_written(what + " gelu")
    sent = x.to(dev)[:, torch.arange(N, device=dev) % 8]
    bad = int((_bits(y_g.payload) != _bits(sent)).sum())
    assert bad == 0, f"{what}: {bad} of {M * N} values do not come back bit for bit from EPI_NONE"
    _sweep_figures(what, names[1].decode(), y_g.payload, g_g.payload, 63488)
