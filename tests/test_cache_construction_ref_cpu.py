"""Pins tests/cache_construction_ref.py (the references of tests/test_cache_construction_kernels_gpu.py) on the CPU: the fp64 unproject and
reliable-mask references against oracle/warp_oracle.py under the GPU test's own bars, the listed mutants of unproject_kernel shown caught on the
GPU test's own inputs, the oracle's mesh down-sampling against F.interpolate at frame sizes that are no multiple of 4, and the conditions the
occlusion-mesh cases must meet."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import warp_oracle as wo
from tests import cache_construction_ref as cr

F32 = np.float32


def _oracle_unproject(d, c2w, Kinv):
    """warp_oracle.unproject_points takes w2c and K and inverts them in fp32; feed it matrices whose fp32 inverses are the test's c2w / Kinv by
    restating its body on the given inverses (same operations, same order)"""
    b, h, w = d.shape
    out = np.zeros((b, h, w, 3), F32)
    xs, ys = np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None]
    with np.errstate(all="ignore"):
        for i in range(b):
            Ki, Cm = Kinv[i], c2w[i]
            un = [((Ki[r, 0] * xs + Ki[r, 1] * ys) + Ki[r, 2] * F32(1.0)).astype(F32) for r in range(3)]
            camp = [(d[i] * un[r]).astype(F32) for r in range(3)]
            for r in range(3):
                val = (((Cm[r, 0] * camp[0] + Cm[r, 1] * camp[1]) + Cm[r, 2] * camp[2]) + Cm[r, 3] * F32(1.0)).astype(F32)
                out[i, :, :, r] = np.where(d[i] > 0, val, F32(0))
    return out


@pytest.mark.parametrize("case", ["batch", "grid_stride"])
def test_unproject_reference_and_mutants(case):
    d, c2w, Kinv = cr.unproject_inputs(case)
    ref, S = cr.unproject64(d, c2w, Kinv)
    got = _oracle_unproject(d, c2w, Kinv)
    worst, exact = cr.unproject_check(case, got, ref, S, d)
    print(f"[unproject ref {case}] fp32 restatement: worst {worst:.3f} of the bar, bitwise share {exact:.4f}")
    assert (~np.isfinite(ref)).any() and (ref == 0).any()
    mutants = [dict(transpose_c2w=True)] + ([dict(item0_matrices=True)] if case == "batch" else [])
    for mut in mutants:
        bad, _ = cr.unproject64(d, c2w, Kinv, **mut)
        with pytest.raises(AssertionError):
            cr.unproject_check(f"{case} {mut}", bad.astype(F32), ref, S, d)
    if case == "batch":  # the restatement above is the oracle's own arithmetic
        w2c = np.stack([np.linalg.inv(m.astype(np.float64)) for m in c2w]).astype(F32)
        with np.errstate(all="ignore"):
            o = wo.unproject_points(d[:, None], w2c, np.stack([np.linalg.inv(k.astype(np.float64)) for k in Kinv]).astype(F32))
        fin = np.isfinite(ref) & np.isfinite(o)
        assert np.abs(o - ref)[fin].max() < 1e-4


@pytest.mark.parametrize("case", list(cr.RELIABLE_SHAPES))
def test_reliable_mask_reference_against_oracle(case):
    d = cr.reliable_inputs(case)
    assert d.shape == cr.RELIABLE_SHAPES[case]
    if d[0].size > 100:
        assert np.isinf(d).any() and np.isnan(d).any() and (d == 0).any() and (d < 0).any()
        assert not np.array_equal(d[0], d[1]) and not np.array_equal(d[1], d[2])
    for win in cr.RELIABLE_WINDOWS[case]:
        for thr in cr.THRESHOLDS:
            with np.errstate(all="ignore"):
                o = wo.reliable_depth_mask(d[:, None], window=win, ratio_thresh=thr, eps=float(cr.EPS))[:, 0]
            dec, band = cr.reliable64(d, win, thr)
            share = o.mean()
            print(f"[reliable ref {case} window {win} thr {thr}] share true {share:.3f}, in band {band.mean():.5f}, oracle != fp64 outside the band {int(((o != dec) & ~band).sum())}")
            assert band.mean() <= 0.01 and np.array_equal(o[~band], dec[~band])
            if d[0].size > 100:
                assert 0.2 < share < 0.8
            else:
                assert 0 < o.sum() < o.size


@pytest.mark.parametrize("hw", [(42, 70), (41, 75), (11, 9), (8, 7), (7, 8)])
def test_mesh_downsample_against_interpolate(hw):
    h, w = hw
    rng = np.random.RandomState(h * 100 + w)
    pts = (rng.randn(h, w, 3) * [2, 2, 1] + [0, 0, 4]).astype(F32)
    mask = rng.rand(h, w) < 0.3
    got, gm = wo.downsample_points_mask(pts, mask, 4)
    nh, nw = h // 4, w // 4
    ref = F.interpolate(torch.from_numpy(pts).permute(2, 0, 1)[None], size=(nh, nw), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    rm = F.interpolate(torch.from_numpy(mask.astype(F32))[None, None], size=(nh, nw), mode="nearest")[0, 0].numpy() > 0
    assert got.shape == (nh, nw, 3) and np.array_equal(gm, rm)
    err = np.abs(got - ref)
    ulp = np.spacing(np.abs(pts).max().astype(F32))
    print(f"[downsample {h}x{w}] max err {err.max():.2e} = {err.max() / ulp:.2f} ulp of the largest tap")
    assert err.max() <= 2 * ulp
    if h % 4 and w % 4 and nh > 1 and nw > 1:  # fractional weights really occur
        sy = F32(h) / F32(nh)
        c = (np.arange(nh, dtype=F32) + F32(0.5)) * sy - F32(0.5)
        assert np.any(np.abs((c - np.floor(c)) - 0.5) > 0.01)


@pytest.mark.parametrize("hw", cr.MESH_SIZES)
def test_mesh_cases_meet_their_conditions(hw):
    ref = cr.mesh_oracle(*hw)
    removed = (ref["mask_plain"] != ref["mask"]).sum(axis=(1, 2, 3))
    print(f"[mesh case {hw}] occluded px {removed.tolist()}, triangles touching the camera plane {ref['touching']}, valid share {ref['mask'].mean():.3f}")
    assert np.all(removed > 0) and max(ref["touching"]) >= 10
