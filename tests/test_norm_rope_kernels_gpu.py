"""The kernels of gen3c_amd/csrc/norm_rope.hip one by one, through gen3c_amd.ops / the C ABI, against the fp64 references of
tests/norm_rope_ref.py (which tests/test_norm_rope_ref_cpu.py pins against the oracle, and whose mutants it shows caught on these very inputs):
LayerNorm + AdaLN modulate in both forms, the per-head RMSNorm (+ RoPE) in its general, octet and pair forms, the small-M GEMV and its SiLU over
every finite bf16 value, add_inplace past the grid cap, the V -> V^T re-layout, and the documented refusals.

Rules every test here keeps (those of tests/test_tokenizer_kernels_gpu.py): inputs are bf16 tensors built on the CPU from seeded generators and
feed kernel and reference alike; every output lives in a NaN-filled buffer with padding columns and guard rows, which must come back bit for
bit untouched around a finite payload; options are restored to the library's defaults in try / finally.

Bars (kr.check): |out - ref| <= 0.5 bf16_ulp(ref) + C E per element, the share of elements != bf16_round(ref) at most max(10 x the fp32
restatement's share on the same input, 1e-3), and C E > 0.5 ulp on at most 5 % of a case. Measured on an MI355X:
profiles/norm_rope_kernel_parity_measured.txt."""
import os
from contextlib import contextmanager

import pytest
import torch

from tests import norm_rope_ref as kr
from tests.guarded import Guarded, _dev

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEFAULTS = {"ln_wave_rows": int(os.environ.get("G3_LN_WAVE_ROWS", "0")), "norm_octets": 1}


def _lib():
    from gen3c_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


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


def _bits(t):
    return t.view(torch.int16)


def _padded(t, pad, fill=float("nan")):
    """t [R][C] (CPU) -> its device copy as the [:, :C] view of a [R][C + pad] tensor filled with `fill`"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=_dev())
    buf[:, :t.shape[1]] = t.to(_dev())
    return buf[:, :t.shape[1]]


def _err_names(entry):
    L, lib = _lib()
    msg = L.last_error()
    assert entry in msg, f"g3_last_error does not name {entry}: {msg!r}"


# =================================================================================================================================
# LayerNorm + AdaLN modulate
# =================================================================================================================================
@pytest.mark.parametrize("D,B,wave", kr.LN_CASES)
def test_layernorm_modulate_against_fp64_reference(D, B, wave):
    """g3_layernorm_modulate_bf16, one launch of 17 rows per case (kr.ln_inputs: six input families from eps-dominated to 1000 +- 4, a constant
    row, a one-hot row, scale = -1 columns, a shift that cancels row 0), D from one chunk to 8192 with partly filled passes of the chunk loop,
    modulation rows 1 / 2 / 3 as column views of one [B][3 D] tensor, ldx and ldo padded; D = 4096 in the one-workgroup-per-row form and, with
    17 = 4 x 4 + 1 rows, the one-wave-per-row form with a ragged last workgroup. Bars: kr.check with C = 4 (the fp32 restatement in the kernel's
    summation order shows 0.62 at worst on these inputs). Exactly: the constant row and the scale = -1 columns equal the shift; x is unchanged.
    Measured: see profiles/norm_rope_kernel_parity_measured.txt."""
    from gen3c_amd import ops
    x, mod = kr.ln_inputs(D, B)
    xin = Guarded(kr.LN_ROWS, D, D + 8, data=x)
    before = _bits(xin.buf).clone()
    mod_d = mod.to(_dev())
    shift, scale = mod_d[:, :D], mod_d[:, D:2 * D]
    out = Guarded(kr.LN_ROWS, D, D + 16)
    with _options(ln_wave_rows=wave):
        ops.layernorm_modulate(xin.payload, shift, scale, out=out.payload)
        torch.cuda.synchronize()
    out.assert_only_payload_written(f"layernorm D={D}")
    assert torch.equal(_bits(xin.buf), before), "layernorm_modulate wrote to its input"
    got = out.cpu()
    sh_c, sc_c = mod[:, :D], mod[:, D:2 * D]
    ref, E = kr.ln_ref(x, sh_c, sc_c)
    kr.check(f"layernorm D={D} mod_rows={B} wave={wave} GPU", got, ref, E, kr.C_LN, kr.ln_fp32(x, sh_c, sc_c, wave=bool(wave)))
    m = torch.arange(kr.LN_ROWS) % B
    cols = kr.ln_scale_m1_cols(D)
    assert torch.equal(got[kr.LN_CONST_ROW], sh_c[kr.LN_CONST_ROW % B]), "a constant row must give bf16(shift) exactly"
    assert torch.equal(got[:, cols], sh_c[m][:, cols]), "scale = -1 must give the shift exactly"


# =================================================================================================================================
# per-head RMSNorm (+ RoPE)
# =================================================================================================================================
def _run_qk(x, w, cos, sin, S, B, Hq, Hk, layout, octets):
    """One form of the pass on x [rows][H][128] (CPU) -> output [rows][H][128] on the CPU. layout 'out': from a padded ld_in into a guarded
    buffer with another padded ld_out; 'inplace': on the leading columns of a guarded buffer whose 256 further columns must stay as they were."""
    from gen3c_amd import ops
    H, rows = Hq + Hk, S * B
    W = H * 128
    x2 = x.reshape(rows, W)
    wq, wk = w[0].to(_dev()), w[-1].to(_dev())
    cd, sd = (cos.to(_dev()), sin.to(_dev())) if cos is not None else (None, None)
    if layout == "out":
        src = _padded(x2, 8)
        dst = Guarded(rows, W, W + 24)
        src_before = src.clone()
        target, out_view = src, dst.payload
    else:
        g = torch.Generator().manual_seed(rows + W)
        tail = torch.randn(rows, 256, generator=g).to(bf16)
        dst = Guarded(rows, W + 256, W + 256 + 8, data=torch.cat([x2, tail], dim=1))
        target = out_view = dst.payload[:, :W]
    with _options(norm_octets=octets):
        if Hk:
            ops.qk_rmsnorm_rope_pair(target, wq, Hq, wk, Hk, cd, sd, S, B, out=out_view)
        else:
            ops.qk_rmsnorm_rope(target, wq, cd, sd, S, B, H, out=out_view)
        torch.cuda.synchronize()
    dst.assert_only_payload_written(f"qk norm {layout} octets={octets}")
    if layout == "out":
        assert torch.equal(src, src_before), "the out-of-place pass wrote to its input"
    else:
        assert torch.equal(dst.payload[:, W:].cpu(), tail), "the in-place pass touched the columns behind the heads"
    return out_view.cpu().reshape(rows, H, 128)


@pytest.mark.parametrize("S,B,Hq,Hk", kr.RMS_CASES)
def test_qk_rmsnorm_rope_every_form_against_fp64_reference(S, B, Hq, Hk):
    """g3_qk_rmsnorm_rope_bf16 at H = 1, 3 (general form) and 8, 24 (octet form, and general with norm_octets = 0), g3_qk_rmsnorm_rope_pair_bf16
    at (8, 16) (octet, and general) and (3, 5) (general), B = 1, 2, 3, row counts that leave the last workgroup of either form ragged, out of
    place between two padded leading dimensions and in place on a column view. Inputs kr.rms_inputs: randn, eps-dominated, 256 randn, a
    2^-16 .. 2^8 spread, one-hot heads, all-zero heads; cos / sin differ at every position and in both halves.
    Two stages, each one rounding: without RoPE against x / sqrt(mean(x^2) + eps) w (C = 8: the restatement shows 1.74 at worst over these
    families), then with RoPE against the rotation of the kernel's OWN no-RoPE output (C = 8: 1.14). Every form and layout is bitwise equal to
    the first; all-zero heads give exactly 0. Measured: see profiles/norm_rope_kernel_parity_measured.txt."""
    x, w, cos, sin = kr.rms_inputs(S, B, Hq, Hk)
    forms = [1, 0] if (Hq % 8 == 0 and Hk % 8 == 0) else [1]  # with H % 8 != 0 the option changes nothing: the general form either way
    what = f"S={S} B={B} H={Hq}+{Hk}"
    zero = torch.arange(S * B) % kr.RMS_FAMILIES == kr.RMS_ZERO_FAMILY
    stage = {}
    for rope in (False, True):
        c, s = (cos, sin) if rope else (None, None)
        outs = [_run_qk(x, w, c, s, S, B, Hq, Hk, layout, octets) for octets in forms for layout in ("out", "inplace")]
        if Hk:  # the two regions one by one through the one-region entry, general form
            from gen3c_amd import ops
            buf = _padded(x.reshape(S * B, -1), 8).clone()
            cd, sd = (c.to(_dev()), s.to(_dev())) if rope else (None, None)
            with _options(norm_octets=0):
                ops.qk_rmsnorm_rope(buf[:, :Hq * 128], w[0].to(_dev()), cd, sd, S, B, Hq, out=buf[:, :Hq * 128])
                ops.qk_rmsnorm_rope(buf[:, Hq * 128:], w[-1].to(_dev()), cd, sd, S, B, Hk, out=buf[:, Hq * 128:])
                torch.cuda.synchronize()
            outs.append(buf.cpu().reshape(S * B, Hq + Hk, 128))
        for i, o in enumerate(outs[1:]):
            assert torch.equal(_bits(o), _bits(outs[0])), f"{what} rope={rope}: form / layout {i + 1} differs bitwise from the first"
        stage[rope] = outs[0]
        assert bool((outs[0][zero] == 0).all()), "an all-zero head must give exactly 0"
    y = stage[False]
    ref, E = kr.rms_ref(x, w)
    kr.check(f"rmsnorm {what} GPU", y, ref, E, kr.C_RMS, kr.rms_rope_fp32(x, w, None, None, B)[0])
    ref, E = kr.rope_ref(y, cos, sin, B)
    kr.check(f"rope {what} GPU", stage[True], ref, E, kr.C_ROPE, kr.rope_fp32(y, cos, sin, B))


# =================================================================================================================================
# small-M GEMV
# =================================================================================================================================
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,N,K", kr.GEMV_CASES)
def test_gemv_with_and_without_add_against_fp64_reference(M, N, K, act):
    """g3_gemv_bf16 without `add` (what the timestep MLP calls) against act(a) @ w^T in fp64, C = 2 (the restatement in the kernel's order:
    0.38 at worst), and with `add` bitwise bf16(float(out without add) + float(add)). K from one lane of one 512-wide pass to eight full passes,
    with one lane live in the last pass at M = 8; lda, ldw, ldadd, ldo padded (NaN behind every row of a and w). act_in = 1 draws `a` off the
    reference's SiLU near-tie values, so that the approximate exp cannot flip bf16(silu(a))."""
    from gen3c_amd import ops
    a, w, add = kr.gemv_inputs(M, N, K, act)
    a_d, w_d, add_d = _padded(a, 8), _padded(w, 16), _padded(add, 3)
    out, out_add = Guarded(M, N, N + 5), Guarded(M, N, N + 7)
    ops.gemv(a_d, w_d, add=None, act_in=act, out=out.payload)
    ops.gemv(a_d, w_d, add=add_d, act_in=act, out=out_add.payload)
    torch.cuda.synchronize()
    out.assert_only_payload_written(f"gemv {M}x{N}x{K}")
    out_add.assert_only_payload_written(f"gemv {M}x{N}x{K} + add")
    got = out.cpu()
    ref, E = kr.gemv_ref(a, w, act)
    kr.check(f"gemv {M}x{N}x{K} act={act} GPU", got, ref, E, kr.C_GEMV, kr.gemv_fp32(a, w, None, act))
    assert torch.equal(out_add.cpu(), kr.add_bf16(got, add)), "gemv + add != bf16(float(out without add) + float(add))"


def test_gemv_silu_over_every_finite_bf16_value():
    """act_in = 1 with w the 4096 x 4096 identity and M = 8: two calls put all 65 280 finite bf16 values through the kernel's SiLU (x w is then
    exact and the sum has one non-zero term). The output must equal bf16_round(silu64(a)) on every value the reference does not list as a
    near tie (its silu64 within 2^-10 ulp of a rounding tie) with |silu64(a)| > 2^-100, and lie within 1 ulp on the listed ones. Below 2^-100
    the kernel's __expf overflows: -0 where the true value is about -1e-37 - recorded, not a defect."""
    from gen3c_amd import ops
    allv = kr.all_bf16()
    fin = torch.isfinite(allv.float())
    vals = torch.cat([allv[fin], torch.zeros(2 * 8 * 4096 - int(fin.sum()), dtype=bf16)]).reshape(2, 8, 4096)
    eye = torch.eye(4096, dtype=bf16, device=_dev())
    got = []
    for i in range(2):
        out = Guarded(8, 4096, 4096 + 8)
        ops.gemv(vals[i].to(_dev()), eye, add=None, act_in=1, out=out.payload)
        torch.cuda.synchronize()
        out.assert_only_payload_written("gemv silu sweep")
        got.append(out.cpu())
    got, a = torch.cat(got).reshape(-1), vals.reshape(-1)
    s64 = kr.silu64(a)
    want = kr.bf16_round(s64)
    near = kr.silu_near_tie()[(a.view(torch.int16).to(torch.int32) & 0xFFFF).long()]
    must = ~near & (s64.abs() > 2.0 ** -100)
    wrong = int((got[must] != want[must]).sum())
    near_ulp = float(kr.ulp_error(got[near], s64[near]).max())
    small = ~must & ~near
    print(f"[gemv silu sweep GPU] {int(must.sum())} values must equal bf16_round(silu64): {wrong} differ; {int(near.sum())} near-tie values: max {near_ulp:.3f} ulp; "
          f"{int(small.sum())} values with |silu64| <= 2^-100: max |out| {float(got[small].float().abs().max()):.3e}")
    assert wrong == 0
    assert near_ulp <= 1.0


# =================================================================================================================================
# add_inplace
# =================================================================================================================================
@pytest.mark.parametrize("n", [8, 2040, 8388608 + 8, 2 * 8388608 + 4104])
def test_add_inplace_bitwise_past_the_grid_cap(n):
    """x += y on one chunk, on 255 chunks, and past the 4096 x 256 x 8 = 8 388 608 elements the grid is capped at: one further chunk (thread 0
    alone goes round again) and two full rounds plus 513 chunks. Bitwise against bf16(float(x) + float(y)) evaluated by torch on the device;
    x and y lie between NaN guards; y is unchanged."""
    from gen3c_amd import ops
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, generator=g).to(bf16), (torch.randn(n, generator=g) * 3).to(bf16)
    xg, yg = Guarded(n, 1, 1, guard=4096, data=x), Guarded(n, 1, 1, guard=4096, data=y)
    want = (xg.payload.float() + yg.payload.float()).to(bf16)
    y_before = _bits(yg.buf).clone()
    ops.add_inplace(xg.payload, yg.payload)
    torch.cuda.synchronize()
    xg.assert_only_payload_written(f"add_inplace n={n}")
    assert torch.equal(_bits(yg.buf), y_before), "add_inplace wrote to y"
    assert torch.equal(_bits(xg.payload), _bits(want))


# =================================================================================================================================
# V -> V^T
# =================================================================================================================================
def _check_vt(vt, v_cpu, S, B, H, ldvt, what):
    vt.assert_only_payload_written(what)
    got = vt.cpu().reshape(B, H, 128, ldvt)
    want = v_cpu.reshape(S, B, H, 128).permute(1, 2, 3, 0)
    assert torch.equal(_bits(got[..., :S]), _bits(want)), f"{what}: payload"
    assert bool((_bits(got[..., S:]) == 0).all()), f"{what}: the tail [S, ldvt) must be +0"


def _v_view(S, B, H):
    g = torch.Generator().manual_seed(100 * S + 10 * B + H)
    v = torch.randn(S * B, H * 128, generator=g).to(bf16)
    buf = torch.full((S * B, 64 + H * 128 + 72), float("nan"), dtype=bf16, device=_dev())  # q-like columns in front, padding behind
    buf[:, 64:64 + H * 128] = v.to(_dev())
    return v, buf[:, 64:64 + H * 128]


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 200])
def test_transpose_v_into_a_prefilled_destination(S, B, H):
    """ops.transpose_v from a column view (ld_in = H 128 + 136) into a NaN-prefilled [B][H][128][ceil64(S)] inside a guarded allocation: the
    payload transposed, exactly 0 on [S, ldvt), nothing else written. S = 1, 63 (one ragged tile), 64 (exact), 65, 200 (a ragged second / fourth)."""
    from gen3c_amd import ops
    v, view = _v_view(S, B, H)
    ldvt = ops.ceil_to(S, 64)
    vt = Guarded(B * H * 128, ldvt)
    ops.transpose_v(view, S, B, H, out=vt.payload.view(B, H, 128, ldvt))
    torch.cuda.synchronize()
    _check_vt(vt, v, S, B, H, ldvt, f"transpose_v S={S} B={B} H={H}")


@pytest.mark.parametrize("ldvt", [72, 136])
def test_transpose_v_leading_dimension_beyond_ceil64(ldvt):
    """g3_transpose_v_bf16 with S = 70 and ldvt = 72 (the second tile stores one 8-wide chunk per row) or 136 (a third tile that reads nothing):
    leading dimensions the C ABI admits and ops.transpose_v cannot ask for."""
    L, lib = _lib()
    S, B, H = 70, 2, 3
    v, view = _v_view(S, B, H)
    vt = Guarded(B * H * 128, ldvt)
    L.check(lib.g3_transpose_v_bf16(view.data_ptr(), view.stride(0), vt.ptr, ldvt, S, B, H, 128, _stream()), "g3_transpose_v_bf16")
    torch.cuda.synchronize()
    _check_vt(vt, v, S, B, H, ldvt, f"transpose_v S={S} ldvt={ldvt}")


# =================================================================================================================================
# refusals
# =================================================================================================================================
def test_documented_refusals_name_their_entry_and_launch_nothing():
    L, lib = _lib()
    a, b = Guarded(256, 256, data=torch.zeros(256, 256, dtype=bf16)), Guarded(256, 256)  # operands large enough for every accepted prefix of the shapes below
    f32 = torch.zeros(64, 128, dtype=torch.float32, device=_dev())
    s = _stream()
    ln, qk, pair = "g3_layernorm_modulate_bf16", "g3_qk_rmsnorm_rope_bf16", "g3_qk_rmsnorm_rope_pair_bf16"
    calls = [
        (ln, lambda: lib.g3_layernorm_modulate_bf16(a.ptr, 256, a.ptr, a.ptr, 256, 1, b.ptr, 256, 4, 12, 1e-6, s)),        # D % 8
        (ln, lambda: lib.g3_layernorm_modulate_bf16(a.ptr, 8208, a.ptr, a.ptr, 8208, 1, b.ptr, 8208, 1, 8200, 1e-6, s)),  # D > 8192
        (ln, lambda: lib.g3_layernorm_modulate_bf16(a.ptr, 20, a.ptr, a.ptr, 256, 1, b.ptr, 256, 4, 16, 1e-6, s)),         # ldx % 8
        (ln, lambda: lib.g3_layernorm_modulate_bf16(a.ptr, 256, a.ptr, a.ptr, 256, 1, b.ptr, 252, 4, 16, 1e-6, s)),        # ldo % 8
        (ln, lambda: lib.g3_layernorm_modulate_bf16(a.ptr, 256, None, a.ptr, 256, 1, b.ptr, 256, 4, 16, 1e-6, s)),         # null shift
        ("g3_gemv_bf16", lambda: lib.g3_gemv_bf16(a.ptr, 256, a.ptr, 256, None, 0, b.ptr, 256, 9, 16, 64, 0, s)),           # M = 9
        ("g3_gemv_bf16", lambda: lib.g3_gemv_bf16(a.ptr, 256, a.ptr, 256, None, 0, b.ptr, 256, 4, 16, 12, 0, s)),           # K % 8
        ("g3_add_inplace_bf16", lambda: lib.g3_add_inplace_bf16(b.ptr, a.ptr, 12, s)),                                      # n % 8
        ("g3_transpose_v_bf16", lambda: lib.g3_transpose_v_bf16(a.ptr, 256, b.ptr, 64, 70, 1, 1, 128, s)),                  # ldvt < S
        ("g3_transpose_v_bf16", lambda: lib.g3_transpose_v_bf16(a.ptr, 256, b.ptr, 64, 64, 1, 1, 64, s)),                   # head_dim
        (qk, lambda: lib.g3_qk_rmsnorm_rope_bf16(a.ptr, 256, a.ptr, f32.data_ptr(), None, b.ptr, 256, 4, 1, 2, 128, 1e-6, s)),   # cos without sin
        (qk, lambda: lib.g3_qk_rmsnorm_rope_bf16(a.ptr, 256, a.ptr, None, f32.data_ptr(), b.ptr, 256, 4, 1, 2, 128, 1e-6, s)),   # sin without cos
        (qk, lambda: lib.g3_qk_rmsnorm_rope_bf16(a.ptr, 256, a.ptr, None, None, b.ptr, 256, 4, 1, 2, 64, 1e-6, s)),              # head_dim
        (pair, lambda: lib.g3_qk_rmsnorm_rope_pair_bf16(a.ptr, 256, a.ptr, 2, a.ptr, 0, None, None, b.ptr, 256, 4, 1, 128, 1e-6, s)),  # H_k = 0
    ]
    for entry, call in calls:
        rc = call()
        assert rc != 0, entry
        _err_names(entry)
    torch.cuda.synchronize()
    assert bool(torch.isnan(b.buf.float()).all()), "a refused call wrote output"
