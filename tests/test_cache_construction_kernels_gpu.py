"""The kernels that run when the 3D cache is built or updated, at kernel level through the C ABI: unproject_kernel (g3_unproject_points_f32) and
reliable_mask_kernel (g3_reliable_depth_mask_f32) of gen3c_amd/csrc/render.hip against the fp64 references of tests/cache_construction_ref.py
(pinned, with the mutants of a transposed c2w and of item 0's matrices for every item, by tests/test_cache_construction_ref_cpu.py), and the
occlusion mesh (mesh_downsample_kernel, mesh_vertex, mesh_mark_kernel) against the oracle's brute force at frame sizes that are no multiple
of 4, where the bilinear weights of the mesh down-sampling are fractional and its nearest-sample index is not 4 i.

Rules: operands are built on the CPU from seeded generators and feed kernel and reference alike (the host inverses are taken in the test);
outputs live in guarded buffers that must come back untouched around the payload.

Bars. unproject: |out - ref| <= 8 * 2^-24 * S (S: the fp64 sum of the absolute values of every term; eight roundings), zeros exactly where
depth <= 0, non-finite positions coincide. Reliable mask: bitwise the oracle (same accumulation order) and equal to the fp64 decision wherever
|ratio - thr| > 1e-5 thr, at most 1 % of the pixels inside that band, 20 % .. 80 % true. Mesh: flow and masks bit-exact, colours / depths beyond
1e-4 + 1e-3 |ref| on a share below 1e-3, largest error below 5e-2.

Measured on an MI355X (profiles/cache_update_parity_measured.txt): unproject at worst 0.197 of its bar, 66 % / 37 % of the values bitwise the
rounded fp64 reference; the reliable mask differs from the oracle and from the fp64 decision on 0 pixels of all 34 cases, 0 pixels inside the
band (cap 1 %); the mesh cases have flow and masks bit-exact, 0 colour / depth outliers, largest errors 2.4e-07 / 1.4e-06."""
import numpy as np
import pytest
import torch

from tests import attn_probe_ref as R
from tests import cache_construction_ref as cr

pytestmark = pytest.mark.gpu
F32 = np.float32


def _lib():
    from gen3c_amd import _lib as L
    return L, L.load()


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _outside_untouched(g, what):
    outside = torch.ones_like(g.buf, dtype=torch.bool)
    outside[g.guard:g.guard + g.rows, :g.C] = False
    touched = int((g.buf.view(torch.int32)[outside] != g.fill).sum())
    assert touched == 0, f"{what}: {touched} elements around the output were written"


class GuardedBytes:
    """n payload bytes between two runs of 4096 bytes of 0xEE"""
    G = 4096

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * self.G,), 0xEE, dtype=torch.uint8, device=_dev())

    @property
    def payload(self):
        return self.buf[self.G:self.G + self.n]

    def assert_guards(self, what):
        assert bool((self.buf[:self.G] == 0xEE).all()) and bool((self.buf[self.G + self.n:] == 0xEE).all()), f"{what}: bytes around the output were written"


# =================================================================================================================================
# unproject
# =================================================================================================================================
@pytest.mark.parametrize("case", ["batch", "grid_stride"])
def test_unproject_against_fp64_reference(case):
    """batch: three 19 x 43 items under two general rotations with translation and an identity, three intrinsics with skew and off-centre
    principal points (a transposed or mis-indexed c2w, or item 0's matrices for every item, misses the bar: shown on the CPU); depth with 0, -0,
    negative, inf and NaN. grid_stride: one 257 x 1031 item, more pixels than the 1024 x 256 threads of the launch."""
    L, lib = _lib()
    d, c2w, Kinv = cr.unproject_inputs(case)
    b, h, w = d.shape
    d_d, c_d, k_d = _t(d), _t(c2w), _t(Kinv)
    out = R.Guarded32(b * h, w * 3)
    rc = lib.g3_unproject_points_f32(d_d.data_ptr(), c_d.data_ptr(), k_d.data_ptr(), out.payload.data_ptr(), b, h, w, _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()
    _outside_untouched(out, case)
    assert torch.equal(d_d.view(torch.int32), _t(d).view(torch.int32)) and torch.equal(c_d, _t(c2w)) and torch.equal(k_d, _t(Kinv)), "an input was written"
    got = out.payload.cpu().numpy().reshape(b, h, w, 3)
    ref, S = cr.unproject64(d, c2w, Kinv)
    worst, exact = cr.unproject_check(case, got, ref, S, d)
    print(f"[unproject {case}] worst error {worst:.3f} of the bar 8 * 2^-24 * S; bitwise fp32(ref) on {exact:.4f}; zero px {int((~(d > 0)).sum())}, "
          f"non-finite values {int((~np.isfinite(ref)).sum())}")


def test_unproject_refusals():
    L, lib = _lib()
    d, c2w, Kinv = cr.unproject_inputs("batch")
    b, h, w = d.shape
    d_d, c_d, k_d = _t(d), _t(c2w), _t(Kinv)
    out = R.Guarded32(b * h, w * 3)
    fill = out.buf.view(torch.int32).clone()
    good = [d_d.data_ptr(), c_d.data_ptr(), k_d.data_ptr(), out.payload.data_ptr(), b, h, w]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (6, -1)):
        a = list(good)
        a[i] = v
        assert lib.g3_unproject_points_f32(*a, _stream()) == L.G3_ERR_ARG and "g3_unproject_points_f32" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.buf.view(torch.int32), fill)


# =================================================================================================================================
# reliable depth mask
# =================================================================================================================================
_REL_IN = {}


@pytest.mark.parametrize("thr", cr.THRESHOLDS)
@pytest.mark.parametrize("case,window", [(c, wdw) for c in cr.RELIABLE_SHAPES for wdw in cr.RELIABLE_WINDOWS[c]])
def test_reliable_mask_against_oracle_and_fp64(case, window, thr):
    """B = 3 with different content per item at 19 x 43 and 257 x 1031 (the grid-stride loop), 1 x 7 and 7 x 1, windows 1 / 3 / 5 / 7 and 11 on a
    5 x 9 frame (wider than the frame), thresholds 0.05 and 0.3, depth with 0, negative, inf and NaN."""
    from oracle import warp_oracle as wo
    L, lib = _lib()
    if case not in _REL_IN:
        _REL_IN[case] = cr.reliable_inputs(case)
    d = _REL_IN[case]
    b, h, w = d.shape
    d_d = _t(d)
    out = GuardedBytes(b * h * w)
    rc = lib.g3_reliable_depth_mask_f32(d_d.data_ptr(), out.payload.data_ptr(), b, h, w, window, thr, float(cr.EPS), _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()
    out.assert_guards(f"{case} window {window}")
    raw = out.payload.cpu().numpy()
    assert set(np.unique(raw).tolist()) <= {0, 1}
    got = raw.reshape(b, h, w) != 0
    with np.errstate(all="ignore"):
        o = wo.reliable_depth_mask(d[:, None], window=window, ratio_thresh=thr, eps=float(cr.EPS))[:, 0]
    dec, band = cr.reliable64(d, window, thr)
    share = float(got.mean())
    n_or, n_64 = int((got != o).sum()), int(((got != dec) & ~band).sum())
    print(f"[reliable {case} window {window} thr {thr}] share true {share:.3f}; != oracle {n_or}; != fp64 outside the band {n_64}; inside the band {int(band.sum())}/{band.size} (cap 1 %)")
    assert n_or == 0 and n_64 == 0 and band.mean() <= 0.01
    if h * w > 100:
        assert 0.2 < share < 0.8
    else:
        assert 0 < got.sum() < got.size


def test_reliable_mask_refuses_an_even_window():
    L, lib = _lib()
    d = cr.reliable_inputs("batch")
    b, h, w = d.shape
    out = GuardedBytes(b * h * w)
    for window in (4, 0, -3):
        rc = lib.g3_reliable_depth_mask_f32(_t(d).data_ptr(), out.payload.data_ptr(), b, h, w, window, 0.05, float(cr.EPS), _stream())
        assert rc == L.G3_ERR_ARG and "g3_reliable_depth_mask_f32" in L.last_error()
    torch.cuda.synchronize()
    assert bool((out.buf == 0xEE).all()), "a refused call wrote"


# =================================================================================================================================
# occlusion mesh at frame sizes that are no multiple of 4
# =================================================================================================================================
def _mesh_bars(what, ref, frame, mask, depth, flow=None):
    removed = (ref["mask_plain"] != ref["mask"]).sum(axis=(1, 2, 3))
    assert np.all(removed > 0), f"{what}: mesh occlusion must remove pixels in every item: {removed}"
    assert max(ref["touching"]) >= 10, f"{what}: one camera plane must touch at least 10 triangles: {ref['touching']}"
    if flow is not None:
        assert int((flow != ref["flow"]).sum()) == 0, f"{what}: flow differs"
    nd = int((mask != ref["mask"]).sum())
    figs = [f"occluded px {removed.tolist()}, triangles touching a camera plane {ref['touching']}, mask px differing {nd}"]
    ok = nd == 0
    for name, got, want in (("colour", frame, ref["frame"]), ("depth", depth, ref["depth"])):
        err = np.abs(got - want)
        bad = err > (1e-4 + 1e-3 * np.abs(want))
        figs.append(f"{name} outliers {int(bad.sum())}/{bad.size} (cap 1e-3), max abs err {err.max():.3e} (cap 5e-2)")
        ok = ok and bad.mean() < 1e-3 and err.max() < 5e-2
    print(f"[mesh {what}] " + "; ".join(figs))
    assert ok, "; ".join(figs)


@pytest.mark.parametrize("hw", cr.MESH_SIZES)
def test_mesh_occlusion_through_forward_warp_vs_bruteforce_oracle(hw):
    """renderer.forward_warp (g3_mesh_occlusion_f32) at 42 x 70 and 41 x 75: h / 4 and w / 4 round down, the bilinear taps of the mesh vertices get
    weights other than 0.5 and the nearest mask sample is floor(i h / (h / 4)); two cameras, foreground masking on"""
    from gen3c_amd import renderer
    h, w = hw
    depth, img, K, pts, rel, bnd = cr.mesh_scene(h, w)
    w2cs = cr.mesh_cameras()
    n = len(w2cs)
    bc = lambda a, s: _t(np.broadcast_to(a, s).copy())
    Ks = bc(K[None], (n, 3, 3))
    frame, m2, d2, flow = renderer.forward_warp(bc(img[None], (n, 3, h, w)), bc(rel, (n, 1, h, w)), None, None, _t(w2cs), Ks, Ks, render_depth=True,
                                                world_points1=bc(pts, (n, h, w, 3)), foreground_masking=True, boundary_mask=bc(bnd[None], (n, h, w)))
    torch.cuda.synchronize()
    _mesh_bars(f"forward_warp {h}x{w}", cr.mesh_oracle(h, w), frame.cpu().numpy(), m2.cpu().numpy(), d2.cpu().numpy(), flow.cpu().numpy())


@pytest.mark.parametrize("hw", cr.MESH_SIZES)
def test_mesh_occlusion_through_render_cache_vs_bruteforce_oracle(hw):
    """Cache3D_Buffer.render_cache (g3_render_items_f32: patch list from mesh_mark_kernel, vertices recomputed by mesh_vertex) on the same cases;
    the cache's own mask and boundary mask (reliable-mask kernel at an odd size) must be the oracle's bit for bit, its points within 1e-6"""
    from gen3c_amd import renderer
    h, w = hw
    depth, img, K, pts, rel, bnd = cr.mesh_scene(h, w)
    w2cs = cr.mesh_cameras()
    n = len(w2cs)
    dev = _dev()
    cache = renderer.Cache3D_Buffer(frame_buffer_max=2, input_image=_t(img)[None], input_depth=_t(depth)[None, None], input_w2c=torch.eye(4, device=dev)[None],
                                    input_intrinsics=_t(K)[None], filter_points_threshold=0.05, foreground_masking=True, input_format=["B", "C", "H", "W"])
    np.testing.assert_allclose(cache.input_points.reshape(h, w, 3).cpu().numpy(), pts[0], rtol=1e-6, atol=1e-6)
    cache.input_points = _t(pts).reshape(cache.input_points.shape).to(cache.input_points.dtype)  # the host inverse of K may differ in the last bit between torch and numpy
    assert np.array_equal(cache.input_mask.reshape(h, w).cpu().numpy(), rel[0, 0]) and np.array_equal(cache.boundary_mask.reshape(h, w).cpu().numpy(), bnd)
    Ks = _t(K)[None, None].expand(1, n, 3, 3).contiguous()
    pix, msk = cache.render_cache(_t(w2cs)[None], Ks)
    dep, msk_d = cache.render_cache(_t(w2cs)[None], Ks, render_depth=True)
    torch.cuda.synchronize()
    assert torch.equal(msk, msk_d)
    _mesh_bars(f"render_cache {h}x{w}", cr.mesh_oracle(h, w), pix[0, :, 0].cpu().numpy(), msk[0, :, 0].cpu().numpy(), dep[0, :, 0].cpu().numpy())


@pytest.mark.parametrize("hw", [(7, 40), (40, 7), (4, 4)])
def test_mesh_occlusion_refuses_frames_without_a_2x2_mesh(hw):
    """h / 4 < 2 or w / 4 < 2: no patch exists; g3_mesh_occlusion_f32 returns G3_ERR_ARG and writes nothing"""
    L, lib = _lib()
    h, w = hw
    cam = torch.ones(1, h, w, 3, device=_dev())
    bm = torch.ones(1, h, w, dtype=torch.uint8, device=_dev())
    K = _t(np.array([[60, 0, w / 2], [0, 60, h / 2], [0, 0, 1]], F32))
    Kinv = torch.linalg.inv(K.cpu()).to(_dev())
    outs = [torch.full((4 * h * w,), 7.0, device=_dev()) for _ in range(6)]  # pts_ds, m_ds, tmin, frame, mask, depth: larger than any of them
    before = [o.clone() for o in outs]
    rc = lib.g3_mesh_occlusion_f32(cam.data_ptr(), bm.data_ptr(), K.data_ptr(), Kinv.data_ptr(), *[o.data_ptr() for o in outs], 1, h, w, 4, _stream())
    torch.cuda.synchronize()
    assert rc == L.G3_ERR_ARG and "g3_mesh_occlusion_f32" in L.last_error()
    assert all(torch.equal(a, b_) for a, b_ in zip(outs, before))
