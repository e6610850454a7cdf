"""The splat and gather kernels of gen3c_amd/csrc/render.hip texel by texel against the fp64 reference of tests/splat_ref.py, through the C ABI:
  A  g3_warp_splat_f32 with splat_tiled = 0 (warp_splat_kernel), then g3_warp_resolve_f32 (warp_resolve_kernel): all five accumulator channels, ring included,
     then frame, mask and depth;
  B  the same with splat_tiled = 1 (warp_splat_tiled_kernel);
  C  g3_warp_splat_resolve_f32 (warp_splat_windows_kernel<false>, warp_gather_resolve_kernel reading the accumulator per item);
  D  g3_render_items_f32 in four forms: planes (render_fused = 0: warp_project_kernel + the window splat), clamped (fused, render_full_extent = 0:
     warp_zmax_kernel, warp_splat_windows_kernel<true>), full_extent (fused, render_full_extent = 1: the gather pass reads the accumulator per texel) and
     exclusive (render_exclusive = 1: warp_extent_kernel, warp_splat_windows_kernel<true, true>, single-writer texels resolved by the splat) - always with
     n_src < n and a src_index that shares a source, group sizes 1 and 2 on `levels`, and a `scatter` / `stretch` render followed by a flat case on the same
     workspace (the accumulator must have cleaned itself). Foreground masking stays off.
The image is random and high in contrast (uniform in [-0.9, 0.9] per pixel and channel), so every single contribution is visible: tests/test_splat_ref_cpu.py
shows that a dropped, doubled or misplaced contribution misses the bar on the texel it touches.

Rules: operands are built on the CPU from seeded generators and feed kernel and reference alike; outputs live in guarded buffers that must come back
untouched around the payload; options are restored in `finally`.

Bars (tests/splat_ref.py, u = 2^-24): masks equal exactly; resolved values within ((n_t + 8) u + 2 delta_t) absnum / den per texel, accumulator channels
within ((n_t + 4) u + delta_t) absnum; no outlier allowance; non-finite positions coincide. delta_t is twice the sum of the named roundings of the depth
weight's operation chain (hardware log2 / exp2 / rcp at 1 ulp for the window kernels, libm for A and B) and 0 for the resolved value where every contributor
has the same z.

Cases (tests/splat_ref.py; tests/test_splat_ref_cpu.py asserts what each reaches): quarter, rows, fold, stretch, scatter, levels at 75 x 141 (3 x 5 tiles,
partial on both axes), tiny 1 x 1 / 1 x 7 / 7 x 1 / 33 x 32, nonfinite at 40 x 72 (flow-plane entries), and on C and the full_extent / exclusive forms of D the
two 1056 x 1024 frames of 33 x 32 source tiles: many_tiles (1053 rectangles in one destination tile: count in chunks, sum in chunks) and far_tiles (28 live
tiles; a list that fits and a pair of rectangles, each with tiles that only the second 1024-tile scan finds).

Measured on an MI355X (profiles/render_splat_parity_measured.txt), worst error as a fraction of its bar: A / B accumulator channels 0.065 (bitwise the
rounded fp64 sum on 6 % .. 69 % of the values), resolved 0.35 (frame) / 0.24 (depth; 0.28 in another run - the order of the float atomics differs from run to run); C 0.37 / 0.24; D 0.37 / 0.33, the same in all four forms; many_tiles
0.17, far_tiles 0.30. On `levels` the window kernels' error is at most 0.04 of the delta term alone (A / B 0.03): the hardware chain is far inside its bound.
Frame values bitwise the rounded reference on 36 % .. 86 % of the small cases. Masks exact everywhere; no defect found in render.hip. Six arithmetic mutants
of render.hip (built aside, not kept) each fail this file: see the profile's summary."""
import numpy as np
import pytest
import torch

from tests import attn_probe_ref as R
from tests import splat_ref as sr

pytestmark = pytest.mark.gpu
F32 = np.float32

FORMS_D = {"planes": (0, 0, 1), "clamped": (1, 0, 0), "full_extent": (1, 0, 1), "exclusive": (1, 1, 1)}  # render_fused, render_exclusive, render_full_extent
OPTS_D = ("render_fused", "render_exclusive", "render_full_extent")
FLOW_CASES = sr.SMALL_CASES + sr.TINY_CASES + ("nonfinite",)
POINT_CASES = sr.SMALL_CASES + sr.TINY_CASES


def _lib():
    from gen3c_amd import _lib as L
    return L, L.load()


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(_dev())  # (a copy: the cases' arrays are shared between the tests and read-only)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _outside_untouched(g, what):
    outside = torch.ones_like(g.buf, dtype=torch.bool)
    outside[g.guard:g.guard + g.rows, :g.C] = False
    touched = int((g.buf.view(torch.int32)[outside] != g.fill).sum())
    assert touched == 0, f"{what}: {touched} elements around the output were written"


class _Outputs:
    def __init__(self, n, h, w):
        self.n, self.h, self.w = n, h, w
        self.frame, self.mask, self.depth = R.Guarded32(n * 3 * h, w), R.Guarded32(n * h, w), R.Guarded32(n * h, w)

    def ptrs(self):
        return [g.payload.data_ptr() for g in (self.frame, self.mask, self.depth)]

    def check(self, what, ref, delta_note=False):
        """masks exactly the reference's; frame and depth within the per-texel bars; nothing written around the payloads"""
        n, h, w = self.n, self.h, self.w
        for g, nm in ((self.frame, "frame"), (self.mask, "mask"), (self.depth, "depth")):
            _outside_untouched(g, f"{what} {nm}")
        mask = self.mask.payload.cpu().numpy().reshape(n, h, w)
        frame = self.frame.payload.cpu().numpy().reshape(n, 3, h, w)
        depth = self.depth.payload.cpu().numpy().reshape(n, h, w)
        nd = int((mask != ref["mask"]).sum())
        assert nd == 0, f"{what}: mask differs on {nd} px"
        wf, ef = sr.compare(f"{what} frame", frame, ref["frame"], ref["frame_bar"])
        wd, ed = sr.compare(f"{what} depth", depth, ref["depth"], ref["depth_bar"])
        note = ""
        if delta_note:  # the error in units of the bar's delta term alone, on the texels whose contributors differ in z
            mixed = ~ref["same_z"][:, 1:-1, 1:-1] & (ref["mask"] > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                dterm = 2.0 * ref["delta"][:, 1:-1, 1:-1][:, None] * ref["absnum"][:, 1:-1, 1:-1, :3].transpose(0, 3, 1, 2) / ref["den"][:, 1:-1, 1:-1][:, None]
                fr = np.abs(frame - ref["frame"]) / dterm
            note = f"; worst error / delta term on the {int(mixed.sum())} mixed-z texels {float(fr[np.broadcast_to(mixed[:, None], fr.shape)].max()):.3f}"
        print(f"[{what}] mask exact ({int(mask.sum())} px valid); frame worst {wf:.3f} of the bar, bitwise fp32(ref) {ef:.4f}; depth worst {wd:.3f}, bitwise {ed:.4f}{note}")
        return wf, wd


def _flow_operands(c):
    ops = dict(image=_t(c["image"]), z=_t(c["z"]), flow=_t(c["flow"]), mask=_t(c["mask"]), gmax=_t(sr.gmax_bits(c["z"], c["group_size"]).view(np.int32)))
    return ops, {k: v.clone() for k, v in ops.items()}


def _inputs_untouched(ops, before, what):
    for k in ops:
        assert torch.equal(ops[k].view(torch.int32), before[k].view(torch.int32)), f"{what}: input {k} was written"


def _aligned_bytes(nbytes, align=256):
    buf = torch.full((nbytes + 2 * 4096 + align,), 0xEE, dtype=torch.uint8, device=_dev())
    off = 4096 + (-(buf.data_ptr() + 4096)) % align
    return buf, buf.data_ptr() + off, off


def _bytes_guards(buf, off, nbytes, what):
    assert bool((buf[:off] == 0xEE).all()) and bool((buf[off + nbytes:] == 0xEE).all()), f"{what}: bytes around the workspace were written"


# =================================================================================================================================
# A, B: splat into the accumulator, then resolve
# =================================================================================================================================
@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("name", FLOW_CASES)
def test_splat_accumulator_then_resolve(name, tiled):
    from gen3c_amd import ops as gops
    L, lib = _lib()
    c = sr.case(name)
    ref = sr.case_reference(name, "libm")
    n, h, w, gs = c["n"], c["h"], c["w"], c["group_size"]
    ops, before = _flow_operands(c)
    acc = R.Guarded32(n * (h + 2), (w + 2) * 5)
    acc.payload.zero_()
    out = _Outputs(n, h, w)
    what = f"{'B tiled' if tiled else 'A direct'} {name}"
    was = gops.option("splat_tiled")
    try:
        gops.set_option("splat_tiled", tiled)
        rc = lib.g3_warp_splat_f32(ops["image"].data_ptr(), ops["z"].data_ptr(), ops["flow"].data_ptr(), ops["mask"].data_ptr(), ops["gmax"].data_ptr(),
                                   acc.payload.data_ptr(), n, h, w, gs, _stream())
        torch.cuda.synchronize()
        assert rc == 0, L.last_error()
    finally:
        gops.set_option("splat_tiled", was)
    _outside_untouched(acc, what)
    _inputs_untouched(ops, before, what)
    if name != "nonfinite":  # (there the kernel's fmaxf(NaN, 0) = 0 and the reference's clamp of NaN differ by design in the ring)
        got = acc.payload.cpu().numpy().reshape(n, h + 2, w + 2, 5)
        wa, ea = sr.compare(f"{what} accumulator", got, ref["acc"], ref["acc_bar"])
        print(f"[{what}] accumulator (5 channels, ring included) worst {wa:.3f} of the bar, bitwise fp32(ref) {ea:.4f}")
    rc = lib.g3_warp_resolve_f32(acc.payload.data_ptr(), *out.ptrs(), n, h, w, _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()
    out.check(what, ref, delta_note=name == "levels")


# =================================================================================================================================
# C: window splat + gather pass
# =================================================================================================================================
@pytest.mark.parametrize("name", FLOW_CASES + sr.BIG_CASES)
def test_window_splat_and_gather(name):
    L, lib = _lib()
    c = sr.case(name)
    ref = sr.case_reference(name, "hw")
    n, h, w, gs = c["n"], c["h"], c["w"], c["group_size"]
    ops, before = _flow_operands(c)
    acc = R.Guarded32(n * (h + 2), (w + 2) * 5)
    acc.payload.zero_()
    nbytes = int(lib.g3_warp_windows_workspace_bytes(n, h, w))
    ntiles = ((h + 31) // 32) * ((w + 31) // 32)
    assert nbytes == n * ntiles * (40 * 40 * 5 * 4 + 16)
    buf, ws, off = _aligned_bytes(nbytes)
    out = _Outputs(n, h, w)
    what = f"C windows {name}"
    rc = lib.g3_warp_splat_resolve_f32(ops["image"].data_ptr(), ops["z"].data_ptr(), ops["flow"].data_ptr(), ops["mask"].data_ptr(), ops["gmax"].data_ptr(),
                                       acc.payload.data_ptr(), ws, *out.ptrs(), n, h, w, gs, _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()
    _outside_untouched(acc, what)
    _bytes_guards(buf, off, nbytes, what)
    _inputs_untouched(ops, before, what)
    out.check(what, ref, delta_note=name == "levels")


# =================================================================================================================================
# D: g3_render_items_f32
# =================================================================================================================================
class _Items:
    """device operands of one points_case and a prepared workspace"""

    def __init__(self, lib, L, p):
        self.p = p
        self.ops = dict(points=_t(p["points"]), image=_t(p["image_src"]), mask=_t(p["mask_src"]), src=_t(p["src_index"]), w2c=_t(p["w2c"]), K=_t(p["K"]))
        self.before = {k: v.clone() for k, v in self.ops.items()}
        n, h, w, gs = p["n"], p["h"], p["w"], p["group_size"]
        self.nbytes = int(lib.g3_render_workspace_bytes(n, h, w, gs))
        self.buf, self.ws, self.off = _aligned_bytes(self.nbytes)
        assert lib.g3_render_workspace_init(self.ws, n, h, w, gs, _stream()) == 0, L.last_error()

    def args(self, p, o, ws, out):
        return [o["points"].data_ptr(), o["image"].data_ptr(), o["mask"].data_ptr(), None, o["src"].data_ptr(), o["w2c"].data_ptr(), o["K"].data_ptr(), None, ws,
                *out.ptrs(), None, p["n"], p["n_src"], p["h"], p["w"], p["group_size"]]


def _render(lib, L, it, what, ref, workspace=None, delta_note=False):
    p = it.p
    ws_owner = workspace or it
    out = _Outputs(p["n"], p["h"], p["w"])
    rc = lib.g3_render_items_f32(*it.args(p, it.ops, ws_owner.ws, out), _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()
    _bytes_guards(ws_owner.buf, ws_owner.off, ws_owner.nbytes, what)
    _inputs_untouched({k: v for k, v in it.ops.items() if k != "src"}, it.before, what)
    assert torch.equal(it.ops["src"], it.before["src"])
    return out.check(what, ref, delta_note=delta_note)


class _form:
    def __init__(self, form):
        self.values = FORMS_D[form]

    def __enter__(self):
        from gen3c_amd import ops as gops
        self.was = [gops.option(o) for o in OPTS_D]
        for o, v in zip(OPTS_D, self.values):
            gops.set_option(o, v)
            assert gops.option(o) == v

    def __exit__(self, *exc):
        from gen3c_amd import ops as gops
        for o, v in zip(OPTS_D, self.was):
            gops.set_option(o, v)
        return False


@pytest.mark.parametrize("form", list(FORMS_D))
@pytest.mark.parametrize("name,gs", [(c, None) for c in POINT_CASES] + [("levels", 1)])
def test_render_items(name, gs, form):
    """every item of the case is a source view; one more item renders source 0 again from a shifted camera (n_src < n, a shared source)"""
    L, lib = _lib()
    p = sr.points_case(name, True, gs)
    assert p["n_src"] < p["n"] and len(set(p["src_index"].tolist())) < p["n"]
    ref = sr.points_reference(name, True, gs, "hw")
    with _form(form):
        _render(lib, L, _Items(lib, L, p), f"D {form} {name} group_size {p['group_size']}", ref, delta_note=name == "levels")


@pytest.mark.parametrize("form", list(FORMS_D))
@pytest.mark.parametrize("first", ["scatter", "stretch"])
def test_render_items_second_render_on_the_same_workspace(first, form):
    """`first` puts corners beyond the windows into the dense accumulator; the flat `quarter` case rendered next on the same workspace is held to the full bar"""
    L, lib = _lib()
    p1, p2 = sr.points_case(first), sr.points_case("quarter")
    assert (p1["n"], p1["h"], p1["w"], p1["group_size"]) == (p2["n"], p2["h"], p2["w"], p2["group_size"])
    with _form(form):
        a = _Items(lib, L, p1)
        _render(lib, L, a, f"D {form} {first} (first render)", sr.points_reference(first))
        b = _Items(lib, L, p2)
        _render(lib, L, b, f"D {form} quarter after {first}", sr.points_reference("quarter"), workspace=a)
        # the dense accumulator opens the workspace; its ring is never read (the resolve crops it) and so never cleaned
        n, h, w = p1["n"], p1["h"], p1["w"]
        acc = a.buf[a.off:a.off + n * (h + 2) * (w + 2) * 5 * 4].view(torch.float32).view(n, h + 2, w + 2, 5)
        left = int((acc[:, 1:-1, 1:-1].view(torch.int32) != 0).sum())
        assert left == 0, f"{left} non-zero values left inside the dense accumulator"


@pytest.mark.parametrize("form", ["full_extent", "exclusive"])
@pytest.mark.parametrize("name", sr.BIG_CASES)
def test_render_items_1056_source_tiles(name, form):
    """many_tiles: the rectangles of 1056 source tiles (a second 1024-tile scan) all meet in one 30 x 30 texel region: more than 256 per destination tile (count
    in chunks, sum in chunks). far_tiles: all but 28 source tiles empty; a list that fits and a pair of rectangles, each with tiles only the second scan finds"""
    L, lib = _lib()
    p = sr.points_case(name, False)
    with _form(form):
        _render(lib, L, _Items(lib, L, p), f"D {form} {name}", sr.points_reference(name, False))


# =================================================================================================================================
# refusals: nothing is launched, nothing is written
# =================================================================================================================================
def test_splat_and_resolve_refusals():
    L, lib = _lib()
    c = sr.case("tiny_1x7")
    n, h, w, gs = c["n"], c["h"], c["w"], c["group_size"]
    ops, before = _flow_operands(c)
    acc = R.Guarded32(n * (h + 2), (w + 2) * 5)
    out = _Outputs(n, h, w)
    fills = [g.buf.view(torch.int32).clone() for g in (acc, out.frame, out.mask, out.depth)]
    good = [ops["image"].data_ptr(), ops["z"].data_ptr(), ops["flow"].data_ptr(), ops["mask"].data_ptr(), ops["gmax"].data_ptr(), acc.payload.data_ptr(), n, h, w, gs]
    for i, v in [(i, None) for i in range(6)] + [(6, 0), (7, 0), (8, -1), (9, 0)]:
        a = list(good)
        a[i] = v
        assert lib.g3_warp_splat_f32(*a, _stream()) == L.G3_ERR_ARG and "g3_warp_splat_f32" in L.last_error()
    good = [acc.payload.data_ptr(), *out.ptrs(), n, h, w]
    for i, v in ((0, None), (1, None), (2, None), (4, 0), (5, -2), (6, 0)):
        a = list(good)
        a[i] = v
        assert lib.g3_warp_resolve_f32(*a, _stream()) == L.G3_ERR_ARG and "g3_warp_resolve_f32" in L.last_error()
    torch.cuda.synchronize()
    for g, f in zip((acc, out.frame, out.mask, out.depth), fills):
        assert torch.equal(g.buf.view(torch.int32), f), "a refused call wrote"
    _inputs_untouched(ops, before, "refusals")


def test_window_splat_refusals():
    L, lib = _lib()
    c = sr.case("tiny_1x7")
    n, h, w, gs = c["n"], c["h"], c["w"], c["group_size"]
    ops, before = _flow_operands(c)
    acc = R.Guarded32(n * (h + 2), (w + 2) * 5)
    out = _Outputs(n, h, w)
    nbytes = int(lib.g3_warp_windows_workspace_bytes(n, h, w))
    buf, ws, off = _aligned_bytes(nbytes)
    assert lib.g3_warp_windows_workspace_bytes(0, h, w) == 0 and lib.g3_warp_windows_workspace_bytes(n, -1, w) == 0
    fills = [g.buf.view(torch.int32).clone() for g in (acc, out.frame, out.mask, out.depth)]
    good = [ops["image"].data_ptr(), ops["z"].data_ptr(), ops["flow"].data_ptr(), ops["mask"].data_ptr(), ops["gmax"].data_ptr(), acc.payload.data_ptr(), ws,
            *out.ptrs(), n, h, w, gs]
    # null operands (the depth output, argument 9, is optional), non-positive shapes, a workspace off its 16-byte alignment, frames beyond the packed texel ids
    bad = [(i, None) for i in range(9)] + [(10, 0), (11, 0), (12, -1), (13, 0), (6, ws + 4), (6, ws + 8), (11, 32766), (12, 65534)]
    for i, v in bad:
        a = list(good)
        a[i] = v
        assert lib.g3_warp_splat_resolve_f32(*a, _stream()) == L.G3_ERR_ARG and "g3_warp_splat_resolve_f32" in L.last_error(), (i, v)
    torch.cuda.synchronize()
    for g, f in zip((acc, out.frame, out.mask, out.depth), fills):
        assert torch.equal(g.buf.view(torch.int32), f), "a refused call wrote"
    assert bool((buf == 0xEE).all()), "a refused call wrote into the workspace"
    _inputs_untouched(ops, before, "refusals")


@pytest.mark.parametrize("form", list(FORMS_D))
def test_render_items_refusals(form):
    L, lib = _lib()
    p = sr.points_case("tiny_1x7")
    it = _Items(lib, L, p)
    torch.cuda.synchronize()
    out = _Outputs(p["n"], p["h"], p["w"])
    ws_before = it.buf.clone()
    fills = [g.buf.view(torch.int32).clone() for g in (out.frame, out.mask, out.depth)]
    good = it.args(p, it.ops, it.ws, out)
    bnd = torch.ones(p["n_src"], p["h"], p["w"], dtype=torch.uint8, device=_dev())
    kinv = torch.eye(3, device=_dev()).repeat(p["n"], 1, 1).contiguous()
    assert lib.g3_render_workspace_bytes(0, 4, 4, 1) == 0 and lib.g3_render_workspace_bytes(1, 4, 4, 0) == 0
    # null operands (mask_src 2, boundary 3, Kinv 7, depth 11 and flow 12 are optional), non-positive shapes, a workspace off its 256-byte alignment, frames
    # beyond the packed texel ids, foreground masking without Kinv / without a depth output
    bad = [[(i, None)] for i in (0, 1, 4, 5, 6, 8, 9, 10)] + [[(13, 0)], [(14, 0)], [(15, 0)], [(16, -1)], [(17, 0)], [(8, it.ws + 16)], [(8, it.ws + 128)],
                                                             [(15, 32766)], [(16, 65534)], [(3, bnd.data_ptr())], [(3, bnd.data_ptr()), (7, kinv.data_ptr()), (11, None)]]
    with _form(form):
        for edits in bad:
            a = list(good)
            for i, v in edits:
                a[i] = v
            assert lib.g3_render_items_f32(*a, _stream()) == L.G3_ERR_ARG and "g3_render_items_f32" in L.last_error(), edits
    torch.cuda.synchronize()
    for g, f in zip((out.frame, out.mask, out.depth), fills):
        assert torch.equal(g.buf.view(torch.int32), f), "a refused call wrote"
    assert torch.equal(it.buf, ws_before), "a refused call wrote into the workspace"
    for bad_ws in (None, it.ws + 8):
        assert lib.g3_render_workspace_init(bad_ws, p["n"], p["h"], p["w"], p["group_size"], _stream()) == L.G3_ERR_ARG
    assert lib.g3_render_workspace_init(it.ws, p["n"], 0, p["w"], p["group_size"], _stream()) == L.G3_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(it.buf, ws_before)
