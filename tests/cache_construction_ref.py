"""Inputs and fp64 references for the kernel-level tests of the cache-construction kernels of gen3c_amd/csrc/render.hip (unproject_kernel,
reliable_mask_kernel) and the occlusion-mesh cases at frame sizes that are no multiple of 4 (TEST INFRASTRUCTURE - a plain helper module;
tests/test_cache_construction_ref_cpu.py pins it, tests/test_cache_construction_kernels_gpu.py uses it)."""
import numpy as np

F32 = np.float32
EPS32 = 2.0 ** -24
UNPROJECT_ROUNDINGS = 8  # (K0 x + K1 y) + K2: 4; d * un: 1; per output row ((C0 c0 + C1 c1) + C2 c2) + C3: the longest path to an output is 8
EPS = F32(1e-6)


# ---- unproject ------------------------------------------------------------------------------------------------------------------------------------------
def pose(a, b, t):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    Rm = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rm, t
    return M.astype(F32)


def unproject_inputs(case):
    """-> (depth [b,h,w], c2w [b,4,4], Kinv [b,3,3]): fp32, the host inverses taken here so that kernel and reference see the same matrices.
    'batch': 3 items of 19 x 43, two general rotations with translation and an identity, three intrinsics with skew and off-centre principal
    points, depth with 0, negative, inf and NaN. 'grid_stride': one 257 x 1031 item (more pixels than 1024 x 256 threads)."""
    if case == "batch":
        b, h, w = 3, 19, 43
        w2c = np.stack([pose(0.3, -0.2, [0.5, -1, 2]), pose(-1.1, 0.7, [3, 0.2, -4]), np.eye(4, dtype=F32)])
    else:
        b, h, w = 1, 257, 1031
        w2c = np.stack([pose(0.45, 0.25, [-0.7, 0.4, 1.5])])
    rng = np.random.RandomState(2 + b)
    d = (1 + 3 * rng.rand(b, h, w)).astype(F32)
    d[0, 3:6, 4:9] = 0
    d[-1, 0, 0] = -1
    d[-1, 7, 7] = np.inf
    d[-1, 12, 30] = np.nan
    d[0, h - 1, w - 1] = -0.0
    K = np.stack([np.array([[50 + 7 * i + w, 0.3 * (i + 1), w / 2 + i + 0.25], [0, 61 - 3 * i + w, h / 2 - i - 0.5], [0, 0, 1]], F32) for i in range(b)])
    c2w = np.stack([np.linalg.inv(m).astype(F32) for m in w2c])
    Kinv = np.stack([np.linalg.inv(k).astype(F32) for k in K])
    return d, c2w, Kinv


def unproject64(d, c2w, Kinv, transpose_c2w=False, item0_matrices=False):
    """fp64 on the fp32 operands -> (points [b,h,w,3], S [b,h,w,3] = the sum of the absolute values of every term of each output).
    Zeros where depth <= 0 (NaN depth included: NaN > 0 is false). The keyword arguments are the mutants the CPU test shows caught."""
    b, h, w = d.shape
    xs = np.arange(w, dtype=np.float64)[None, :]
    ys = np.arange(h, dtype=np.float64)[:, None]
    out, S = np.zeros((b, h, w, 3)), np.zeros((b, h, w, 3))
    with np.errstate(all="ignore"):
        for i in range(b):
            j = 0 if item0_matrices else i
            Ki, Cm = Kinv[j].astype(np.float64), c2w[j].astype(np.float64)
            if transpose_c2w:
                Cm = Cm.T
            di = d[i].astype(np.float64)
            un = [Ki[r, 0] * xs + Ki[r, 1] * ys + Ki[r, 2] for r in range(3)]
            una = [abs(Ki[r, 0]) * xs + abs(Ki[r, 1]) * ys + abs(Ki[r, 2]) for r in range(3)]
            ok = d[i] > 0
            for r in range(3):
                val = Cm[r, 0] * (di * un[0]) + Cm[r, 1] * (di * un[1]) + Cm[r, 2] * (di * un[2]) + Cm[r, 3]
                mag = sum(abs(Cm[r, k]) * np.abs(di) * una[k] for k in range(3)) + abs(Cm[r, 3])
                out[i, :, :, r] = np.where(ok, val, 0.0)
                S[i, :, :, r] = np.where(ok, mag, 0.0)
    return out, S


def unproject_check(what, got, ref, S, d):
    """the bars of the GPU test on one result; -> (worst error over the bar, share bitwise equal to fp32(ref)); raises AssertionError"""
    got = np.asarray(got)
    zero = ~(d > 0)
    assert np.all(got[zero] == 0), f"{what}: {(got[zero] != 0).sum()} non-zero values where depth <= 0"
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)].astype(F32)), f"{what}: non-finite positions differ"
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref)[fin]
    bar = UNPROJECT_ROUNDINGS * EPS32 * S[fin]
    bad = err > bar
    with np.errstate(all="ignore"):
        worst = float(np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0)).max())
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values beyond 8 * 2^-24 * S, worst {worst:.2f} of the bar"
    with np.errstate(all="ignore"):
        return worst, float((got[fin] == ref[fin].astype(F32)).mean())


# ---- reliable depth mask --------------------------------------------------------------------------------------------------------------------------------
RELIABLE_SHAPES = {"batch": (3, 19, 43), "grid_stride": (3, 257, 1031), "1x7": (1, 1, 7), "7x1": (1, 7, 1), "5x9": (1, 5, 9)}
RELIABLE_WINDOWS = {"batch": (1, 3, 5, 7), "grid_stride": (1, 3, 5, 7), "1x7": (1, 3, 5, 7), "7x1": (1, 3, 5, 7), "5x9": (11,)}
THRESHOLDS = (0.05, 0.3)


def reliable_inputs(case):
    """depth [b,h,w], different per item: a gently slanted plane times per-block steps of {1, 1.03, 1.12, 1.6} plus 0.1 % noise, a band of 22 % of
    the frame without depth (0 or negative; left, top, right for items 0, 1, 2), and single inf / NaN pixels - so that every window / threshold
    pair leaves between 20 % and 80 % true. The frames of a few pixels are near-constant with one pixel without depth."""
    b, h, w = RELIABLE_SHAPES[case]
    rng = np.random.RandomState(40 + h + w)
    ys, xs = np.mgrid[0:h, 0:w].astype(F32)
    out = np.zeros((b, h, w), F32)
    if h * w < 100:
        out[0] = (2 + 0.0005 * (xs + ys) + 0.0001 * rng.randn(h, w)).astype(F32)
        out[0, h - 1 if case != "5x9" else 1, w - 1] = 0 if case != "5x9" else -1
        return out
    bs = 10 if h * w < 5000 else 32
    for i in range(b):
        plane = 2 + (0.1 + 0.05 * i) * xs / w + 0.08 * ys / h
        nby, nbx = -(-h // bs), -(-w // bs)
        steps = rng.choice([1.0, 1.0, 1.0, 1.03, 1.12, 1.6], size=(nby, nbx))
        d = plane * np.kron(steps, np.ones((bs, bs)))[:h, :w] * (1 + 0.001 * rng.randn(h, w))
        hole = (xs < 0.22 * w, ys < 0.22 * h, xs >= 0.78 * w)[i]
        out[i] = np.where(hole, np.where(rng.rand(h, w) < 0.5, 0.0, -1.0), d).astype(F32)
    out[0, h // 2, w // 2] = np.inf
    out[-1, h // 3, w // 3] = np.nan
    return out


def reliable64(d, window, thr, eps=EPS):
    """fp64 decision on the fp32 depth: (max - min) / (mean + eps) < thr and depth > 0, max / min over the pixels inside the frame, mean over the
    full window with zero padding. -> (decision, in_band): in_band marks |ratio - thr| <= 1e-5 thr, where an fp32 evaluation may decide either way.
    A NaN in the window makes the ratio NaN (false), as max / min pooling and the sum all propagate it."""
    b, h, w = d.shape
    r = window // 2
    d64 = d.astype(np.float64)
    with np.errstate(all="ignore"):
        pmax = np.pad(d64, ((0, 0), (r, r), (r, r)), constant_values=-np.inf)
        pmin = np.pad(d64, ((0, 0), (r, r), (r, r)), constant_values=np.inf)
        p0 = np.pad(d64, ((0, 0), (r, r), (r, r)), constant_values=0)
        mx, mn, sm = np.full((b, h, w), -np.inf), np.full((b, h, w), np.inf), np.zeros((b, h, w))
        for dy in range(window):
            for dx in range(window):
                mx = np.maximum(mx, pmax[:, dy:dy + h, dx:dx + w])
                mn = np.minimum(mn, pmin[:, dy:dy + h, dx:dx + w])
                sm = sm + p0[:, dy:dy + h, dx:dx + w]
        ratio = (mx - mn) / (sm / float(window * window) + float(eps))
        t = float(F32(thr))
        return (ratio < t) & (d > 0), np.abs(ratio - t) <= 1e-5 * t


# ---- occlusion mesh at frame sizes that are no multiple of 4 ---------------------------------------------------------------------------------------------
MESH_SIZES = ((42, 70), (41, 75))


def mesh_cameras():
    """two target cameras (w2c): a lateral move that drags the foreground discs over the background, and a camera plane pushed into the skirt of
    boundary triangles between the near disc (z 1.6) and the background (z 4)"""
    from tests.test_render_gpu import _cam
    return np.stack([_cam(tx=-0.5, yaw=0.05), _cam(tx=-0.7, tz=-1.68)])


def mesh_scene(h, w):
    """_scene of tests/test_render_gpu.py with focal 60 -> (depth, image, K, world points, reliable mask as fp32, boundary mask)"""
    from oracle import warp_oracle as wo
    from tests.test_render_gpu import _scene
    depth, img, K = _scene(h, w)
    K = K.copy()
    K[0, 0] = K[1, 1] = 60.0
    pts = wo.unproject_points(depth[None, None], np.eye(4, dtype=F32)[None], K[None])
    rel = wo.reliable_depth_mask(depth[None, None], ratio_thresh=0.05).astype(F32)
    bnd = ~wo.reliable_depth_mask(depth[None, None])[0, 0]
    return depth, img, K, pts, rel, bnd


_MESH_REF = {}


def mesh_oracle(h, w):
    """the oracle's forward_warp with the brute-force ray x triangle depth, computed once per size and shared: dict(frame, mask, depth, flow,
    mask_plain (no occlusion), tris_touching_camera_plane per item)"""
    if (h, w) not in _MESH_REF:
        from oracle import warp_oracle as wo
        depth, img, K, pts, rel, bnd = mesh_scene(h, w)
        w2cs = mesh_cameras()
        n = len(w2cs)
        bc = lambda a, s: np.broadcast_to(a, s)
        Ks = bc(K[None], (n, 3, 3)).copy()
        with np.errstate(all="ignore"):
            fr, m, dp, flow, _ = wo.forward_warp(bc(img[None], (n, 3, h, w)), bc(rel, (n, 1, h, w)), bc(pts, (n, h, w, 3)), w2cs, Ks, render_depth=True,
                                                 foreground_masking=True, boundary_mask=bc(bnd[None], (n, h, w)), ray_triangle_fn=wo.ray_triangle_depth_c)
            _, m_plain, _, _, _ = wo.forward_warp(bc(img[None], (n, 3, h, w)), bc(rel, (n, 1, h, w)), bc(pts, (n, h, w, 3)), w2cs, Ks)
            _, camp = wo.project_points(bc(pts, (n, h, w, 3)), w2cs, Ks)
        touching = [int((wo.mesh_triangles(*wo.downsample_points_mask(camp[i], bnd, 4))[..., 2].min(1) <= 1e-4).sum()) for i in range(n)]
        _MESH_REF[(h, w)] = dict(frame=fr, mask=m, depth=dp, flow=flow, mask_plain=m_plain, touching=touching)
    return _MESH_REF[(h, w)]
