"""fp64 reference, seeded cases and tile model for the splat / gather kernels of gen3c_amd/csrc/render.hip (TEST INFRASTRUCTURE - a plain
helper module; pinned by tests/test_splat_ref_cpu.py, used on the GPU by tests/test_splat_kernels_gpu.py).

Geometry. Corner indices and the four bilinear weights are fp32 by construction: `geom_from_flow` is the arithmetic of
oracle.warp_oracle.splat_indices from `trans = flow + grid` on (the CPU test holds the two equal bit for bit). One statement differs on
purpose: the index clamp is taken on the float (floor / ceil, then clamp, NaN -> 0), which is what a saturating float -> int64 conversion
followed by the integer clamp gives and what the kernels do; numpy's conversion of +inf on x86 would give INT64_MIN instead.

Sums. Every contribution of a valid pixel's corner is c * b * m / dw with dw = exp(min(50 log1p(max(z, 0)) / (lmax + 1e-7), 80)) + 1e-7 in
fp64, lmax the fp64 log1p of the group's fp32 maximum of max(z, 0) (over every pixel of the group's items, masked or not). Per texel of the
(h + 2) x (w + 2) accumulator: num[4] (r g b z), den, absnum[4] = sum |c| w, the number n_t of non-zero contributions and the largest
exponent E_t = 50 log1p(z) / (lmax + 1e-7) among them (and n_pix, the number of distinct PIXELS that reach the texel with a bilinear weight of at least 1 / 16: corners of
one pixel that coincide on an integer coordinate are several contributions of one colour, and next to a neighbour of weight 1e-7 a contribution is alone
in its texel for every purpose - the resolved value of such a texel is that pixel's colour whatever happens to its weight).

Bars (u = 2^-24; derived, never fitted):
  resolved value   |out - ref| <= ((n_t + 8) u + 2 delta_t) absnum / den    (n_t - 1 additions, the product roundings, the division)
  accumulator      |acc - num| <= ((n_t + 4) u + delta_t) absnum            (den: the same with absnum = den)
delta_t bounds the relative error of ONE depth weight 1 / dw; hardware log2 / exp2 / rcp are taken at 1 ulp (= 2 u relative), and because
that figure is quoted from the ISA manual's instruction descriptions from memory, delta_t is TWICE the sum of its terms. A relative error of
the exponent's factors counts E_t times (d exp(E) / exp(E) = dE), an absolute error of the logarithm 50 / lmax times.
  window kernels (chain "hw": __logf(1 + z) * (1 / (lmax + 1e-7)) * 50, __expf, + 1e-7, v_rcp):
    rounding of 1 + z                  (50 / lmax) u     absolute u in the logarithm
    the log                            E (2 u + 2 u)     v_log_f32 at 1 ulp; the ln 2 constant and its product inside __logf
    the reciprocal of lmax             E (2 u + u + u)   lmax from libm log1pf at 1 ulp, + 1e-7, IEEE 1 / x
    product with it, product with 50   E (u + u)
    log2e product inside __expf        E (u + u)         the constant and the product
    the exp                            2 u               v_exp_f32 at 1 ulp
    + 1e-7                             u
    the reciprocal of dw               2 u               v_rcp_f32 at 1 ulp
    sum (12 E + 50 / lmax + 5) u; with E <= 50 and lmax >= log1p(1.5): 3.9e-5, delta <= 7.9e-5
  direct and tiled splat, and the fp32 oracle (chain "libm": log1pf(z) / (lmax + 1e-7) * 50, expf, + 1e-7, IEEE division):
    log1pf                             E 4 u             2 ulp (the OpenCL bound OCML is held to)
    lmax, + 1e-7                       E (2 u + u)
    division, product with 50          E (u + u)
    expf                               6 u               3 ulp (the OpenCL bound)
    + 1e-7, the division by dw         u + u
    sum (9 E + 8) u
Cases: `case(name)` builds the seeded cases in flow form (z, flow and validity planes), `points_case(name)` the same destinations as points under an
identity-rotation camera for the projection forms; what each case is for stands at its generator and, as asserted counts of the tile model, in
tests/test_splat_ref_cpu.py. `far_tiles` complements `many_tiles`: there every texel lies in a thousand rectangles, so a rectangle that one scan misses
changes no decision; here tiles from index 1024 on are one of two owners of a texel and ten of 26 entries of a list that fits.

Texels whose contributors all have the same z: bitwise equal dw, which cancels in the RESOLVED value up to its roundings: delta_t = 0 there.
It does not cancel in the accumulator channels (they are sums of c b m / dw themselves), so their bar keeps delta_t.
"""
from functools import lru_cache

import numpy as np

from oracle import warp_oracle as wo

F32 = np.float32
U = 2.0 ** -24
TS, WIN = 32, 40
FOCAL = 64.0     # intrinsics of the projection forms: f = 64, principal point (w / 2, h / 2)
FLAT_Z = 2.0     # z + 1e-7 == z in fp32 and the division by it is exact: quarter-pixel destinations survive the projection
SHIFT_PX = 2.0   # the item that shares source 0 looks from a camera moved by SHIFT_PX pixels (at FLAT_Z) along x


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------
def geom_from_flow(flow, h, w):
    """flow (n, 2, h, w) fp32 -> the dict of warp_oracle.splat_indices (fx cx fy cy int64, nw sw ne se fp32), same arithmetic from the flow on"""
    flow = np.asarray(flow, F32)
    gx = np.arange(w, dtype=F32)[None, None, :]
    gy = np.arange(h, dtype=F32)[None, :, None]
    with np.errstate(invalid="ignore"):
        tx, ty = (flow[:, 0] + gx).astype(F32), (flow[:, 1] + gy).astype(F32)
        ox, oy = (tx + F32(1.0)).astype(F32), (ty + F32(1.0)).astype(F32)

        def index(f, hi):
            return np.where(np.isnan(f), F32(0), np.clip(f, F32(0), F32(hi))).astype(np.int64)

        fx, cx = index(np.floor(ox), w + 1), index(np.ceil(ox), w + 1)
        fy, cy = index(np.floor(oy), h + 1), index(np.ceil(oy), h + 1)
        oxc = np.clip(ox, F32(0), F32(w + 1)).astype(F32)
        oyc = np.clip(oy, F32(0), F32(h + 1)).astype(F32)
        one = F32(1.0)
        wy_f = (one - (oyc - fy.astype(F32))).astype(F32)
        wy_c = (one - (cy.astype(F32) - oyc)).astype(F32)
        wx_f = (one - (oxc - fx.astype(F32))).astype(F32)
        wx_c = (one - (cx.astype(F32) - oxc)).astype(F32)
        return dict(fx=fx, cx=cx, fy=fy, cy=cy, nw=(wy_f * wx_f).astype(F32), sw=(wy_c * wx_f).astype(F32), ne=(wy_f * wx_c).astype(F32),
                    se=(wy_c * wx_c).astype(F32))


CORNERS = (("nw", "fy", "fx"), ("sw", "cy", "fx"), ("ne", "fy", "cx"), ("se", "cy", "cx"))


# ---- contributions and sums ------------------------------------------------------------------------------------------------------------------------
def group_lmax(z, group_size):
    """fp64 log1p of each group's fp32 maximum of max(z, 0) -> (lmax per item (n,), fp32 maximum z per group)"""
    n = z.shape[0]
    zm = np.array([np.fmax(np.nanmax(np.maximum(z[i], F32(0))), F32(0)) for i in range(n)], F32)
    ng = (n + group_size - 1) // group_size
    gz = np.array([zm[g * group_size:(g + 1) * group_size].max() for g in range(ng)], F32)
    return np.log1p(gz.astype(np.float64))[np.arange(n) // group_size], gz


def contributions(image, mask, z, flow, group_size):
    """The list of corner contributions of every pixel with mask != 0, as a dict of flat arrays (4 P entries, corner-major):
    tex (flat accumulator texel), w (fp64 b m / dw), b (bilinear weight), col (.., 4: r g b z), E, z, pix (index of the pixel among the P), corner"""
    image, mask, z = np.asarray(image, F32), np.asarray(mask, F32), np.asarray(z, F32)
    n, _, h, w = image.shape
    g = geom_from_flow(flow, h, w)
    lmax, _ = group_lmax(z, group_size)
    valid = mask != 0
    it, py, px = np.nonzero(valid)
    zz = z[valid].astype(np.float64)
    E = 50.0 * np.log1p(np.maximum(zz, 0.0)) / (lmax[it] + 1e-7)
    dw = np.exp(np.minimum(E, 80.0)) + 1e-7
    m = mask[valid].astype(np.float64)
    col = np.stack([image[it, c, py, px].astype(np.float64) for c in range(3)] + [zz], -1)
    P = len(it)
    out = dict(tex=[], w=[], b=[], corner=[])
    for ci, (key, yy, xx) in enumerate(CORNERS):
        out["tex"].append((it * (h + 2) + g[yy][valid]) * (w + 2) + g[xx][valid])
        b = g[key][valid].astype(np.float64)
        out["b"].append(b)
        out["w"].append(b * m / dw)
        out["corner"].append(np.full(P, ci))
    C = {k: np.concatenate(v) for k, v in out.items()}
    C.update(col=np.tile(col, (4, 1)), E=np.tile(E, 4), z=np.tile(zz, 4), pix=np.tile(np.arange(P), 4), item=np.tile(it, 4), py=np.tile(py, 4), px=np.tile(px, 4))
    C["shape"] = (n, h, w)
    C["lmax"] = lmax
    return C


def delta_terms(E, lmax, chain):
    """twice the sum of the named terms of the module docstring"""
    if chain == "hw":
        return 2.0 * (12.0 * E + 50.0 / lmax + 5.0) * U
    assert chain == "libm"
    return 2.0 * (9.0 * E + 8.0) * U


def accumulate(C, chain):
    """fp64 sums per accumulator texel, the resolved frame / mask / depth and the per-texel bars"""
    n, h, w = C["shape"]
    T = n * (h + 2) * (w + 2)
    tex, wgt = C["tex"], C["w"]
    nz = wgt != 0
    den = np.bincount(tex, wgt, T)
    num = np.stack([np.bincount(tex, C["col"][:, c] * wgt, T) for c in range(4)], -1)
    absnum = np.stack([np.bincount(tex, np.abs(C["col"][:, c]) * wgt, T) for c in range(4)], -1)
    n_t = np.bincount(tex[nz], minlength=T)
    big, P1 = nz & (C["b"] >= 1.0 / 16), int(C["pix"].max(initial=0)) + 1
    n_pix = np.bincount(np.unique(tex[big].astype(np.int64) * P1 + C["pix"][big]) // P1, minlength=T)
    E_t = np.zeros(T)
    np.maximum.at(E_t, tex[nz], C["E"][nz])
    zlo, zhi = np.full(T, np.inf), np.full(T, -np.inf)
    np.minimum.at(zlo, tex[nz], C["z"][nz])
    np.maximum.at(zhi, tex[nz], C["z"][nz])
    same_z = ~(zhi > zlo)
    lmax_t = np.repeat(np.maximum(C["lmax"], 1e-30), (h + 2) * (w + 2))
    delta = delta_terms(E_t, lmax_t, chain)
    shp = (n, h + 2, w + 2)
    R = dict(num=num.reshape(shp + (4,)), den=den.reshape(shp), absnum=absnum.reshape(shp + (4,)), n_t=n_t.reshape(shp), n_pix=n_pix.reshape(shp), E_t=E_t.reshape(shp),
             same_z=same_z.reshape(shp), delta=delta.reshape(shp), shape=C["shape"], chain=chain)
    R["acc_bar"] = (((R["n_t"] + 4) * U + R["delta"])[..., None] * np.concatenate([R["absnum"], R["den"][..., None]], -1))
    R["acc"] = np.concatenate([R["num"], R["den"][..., None]], -1)
    # resolve: crop the ring, mask = den > 0, fill -1 / 0, clamp the frame
    crop = lambda a: a[:, 1:-1, 1:-1]
    d, nu, ab = crop(R["den"]), crop(R["num"]), crop(R["absnum"])
    ok = d > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(ok[..., None], nu / d[..., None], 0.0)
        rel = ((crop(R["n_t"]) + 8) * U + 2.0 * np.where(crop(R["same_z"]), 0.0, crop(R["delta"])))
        bar = np.where(ok[..., None], rel[..., None] * ab / d[..., None], 0.0)
    R["mask"] = ok.astype(F32)
    R["frame"] = np.moveaxis(np.where(ok[..., None], np.clip(val[..., :3], -1.0, 1.0), -1.0), -1, 1)
    R["frame_bar"] = np.moveaxis(bar[..., :3], -1, 1)
    R["depth"] = val[..., 3]
    R["depth_bar"] = bar[..., 3]
    return R


def reference(image, mask, z, flow, group_size, chain):
    return accumulate(contributions(image, mask, z, flow, group_size), chain)


def compare(what, got, ref, bar):
    """|got - ref| <= bar everywhere (no allowance), non-finite positions coincide. Returns (worst error as a fraction of its bar, share of values
    bitwise equal to the reference rounded to fp32)."""
    got = np.asarray(got)
    assert got.shape == ref.shape == bar.shape, (what, got.shape, ref.shape, bar.shape)
    g, r, b = got.reshape(-1).astype(np.float64), ref.reshape(-1), bar.reshape(-1)
    fin = np.isfinite(r)
    assert np.array_equal(np.isfinite(g), fin), f"{what}: non-finite positions differ ({int((np.isfinite(g) != fin).sum())})"
    err = np.abs(g[fin] - r[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0, 0.0, err / b[fin])
    worst = float(frac.max()) if frac.size else 0.0
    exact = float((got.reshape(-1)[fin] == r[fin].astype(F32)).mean()) if frac.size else 1.0
    nbad = int((frac > 1).sum())
    assert nbad == 0, f"{what}: {nbad} of {frac.size} values beyond their bar, worst {worst:.3f} of it"
    return worst, exact


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------
FLAT_CASES = ("quarter", "rows", "fold", "stretch", "scatter", "many_tiles")
BIG_CASES = ("many_tiles", "far_tiles")  # 1056 x 1024 = 33 x 32 source tiles: the forms that own the list and scan code
SMALL_CASES = ("quarter", "rows", "fold", "stretch", "scatter", "levels")
TINY_CASES = ("tiny_1x1", "tiny_1x7", "tiny_7x1", "tiny_33x32")
ALL_CASES = SMALL_CASES + ("many_tiles",) + TINY_CASES + ("nonfinite", "far_tiles")


def _quarter_flow(rng, n, h, w, tx, ty):
    q = rng.integers(0, 4, (n, 2, h, w)).astype(F32) * F32(0.25)
    return (q + np.array([tx, ty], F32)[None, :, None, None]).astype(F32)


@lru_cache(maxsize=None)
def case(name):
    """dict(h, w, n, group_size, image (n,3,h,w), mask (n,h,w), z (n,h,w), flow (n,2,h,w)); the arrays are shared between the tests: read only"""
    seed = 1000 + ALL_CASES.index(name)
    rng = np.random.default_rng(seed)
    n, gs = 1, 1
    h, w = 75, 141
    if name in BIG_CASES:
        h, w = 1056, 1024
    elif name.startswith("tiny_"):
        h, w = (int(v) for v in name[5:].split("x"))
    elif name == "nonfinite":
        h, w = 40, 72
    elif name == "levels":
        n, gs = 2, 2
    image = rng.uniform(-0.9, 0.9, (n, 3, h, w)).astype(F32)
    mask = (rng.random((n, h, w)) >= 0.2).astype(F32)
    z = np.full((n, h, w), FLAT_Z, F32)
    gx = np.arange(w, dtype=np.float64)[None, None, :]
    gy = np.arange(h, dtype=np.float64)[None, :, None]
    if name in ("quarter", "levels"):
        flow = _quarter_flow(rng, n, h, w, 3.0, -2.0)
        if name == "levels":  # the weight ratio between an item's two levels is exp(50 (log1p(z_b) - log1p(z_a)) / log1p(3.0))
            lv = np.array([[2.0, 2.2], [2.7, 3.0]], F32)
            pick = rng.integers(0, 2, (n, h, w))
            z = np.stack([lv[i][pick[i]] for i in range(n)]).astype(F32)
    elif name == "rows":
        frac = rng.integers(1, 8, (n, h, 1)).astype(F32) * F32(0.125)
        fx = np.broadcast_to(F32(5.0) + frac, (n, h, w))
        fy = rng.integers(-2, 3, (n, h, w)).astype(F32) * np.spacing((np.arange(h, dtype=F32) + F32(1.0)))[None, :, None]
        flow = np.stack([fx, fy.astype(F32)], 1).astype(F32)
    elif name == "fold":
        xi = np.arange(w)
        u = (32 * (xi // 32) + (xi % 8) + 4).astype(np.float64)[None, None, :] + 0.25 * rng.integers(0, 4, (n, h, w))
        v = gy + 0.5 + 0 * gx
        flow = np.stack([u - gx, v - gy], 1).astype(F32)
    elif name == "stretch":
        u = 70.0 + 1.6 * (gx - 70.0) + 0 * gy
        v = 37.0 + 1.6 * (gy - 37.0) + 0 * gx
        flow = np.stack([u - gx, v - gy], 1).astype(F32)
    elif name == "scatter":
        u = rng.uniform(-4.0, w + 4.0, (n, h, w))
        v = rng.uniform(-4.0, h + 4.0, (n, h, w))
        flow = np.stack([u - gx, v - gy], 1).astype(F32)
    elif name == "many_tiles":
        mask = np.zeros((n, h, w), F32)
        ty, tx = np.meshgrid(np.arange(h // TS), np.arange(w // TS), indexing="ij")
        for _ in range(4):  # four valid pixels per 32 x 32 source tile (a repeated position only makes it three)
            mask[0, ty * TS + rng.integers(0, TS, ty.shape), tx * TS + rng.integers(0, TS, tx.shape)] = 1.0
        u = 40.0 + 0.25 * rng.integers(0, 29 * 4, (n, h, w))
        v = 40.0 + 0.25 * rng.integers(0, 29 * 4, (n, h, w))
        flow = np.stack([u - gx, v - gy], 1).astype(F32)
    elif name == "far_tiles":
        # many_tiles' frame with almost every source tile EMPTY: tiles 0 .. 15 and 1040 .. 1049 meet in one region (26 rectangles: the list fits, and its
        # second 1024-tile scan finds ten of them), tiles 20 and 1052 alone in another (texels in exactly two rectangles, one found by the second scan only)
        mask = np.zeros((n, h, w), F32)
        u, v = np.zeros((n, h, w)), np.zeros((n, h, w))
        tiles_x = w // TS
        for tiles, (ry, rx) in ((list(range(16)) + list(range(1040, 1050)), (40.0, 400.0)), ([20, 1052], (400.0, 40.0))):
            for t in tiles:
                y0, x0 = (t // tiles_x) * TS, (t % tiles_x) * TS
                ys, xs = y0 + rng.integers(0, TS, 12), x0 + rng.integers(0, TS, 12)
                mask[0, ys, xs] = 1.0
                u[0, ys, xs] = rx + 0.25 * rng.integers(0, 29 * 4, 12)
                v[0, ys, xs] = ry + 0.25 * rng.integers(0, 29 * 4, 12)
        u, v = np.where(mask != 0, u, gx + 0 * gy), np.where(mask != 0, v, gy + 0 * gx)
        flow = np.stack([u - gx, v - gy], 1).astype(F32)
    elif name.startswith("tiny_"):
        mask = np.ones((n, h, w), F32)
        flow = _quarter_flow(rng, n, h, w, 0.0, 0.0)
    elif name == "nonfinite":
        flow = _quarter_flow(rng, n, h, w, 3.0, -2.0)
        inf, nan = np.inf, np.nan
        bad = [(inf, 0.25), (0.5, inf), (-inf, 0.25), (0.25, -inf), (nan, nan), (inf, inf), (-inf, -inf), (inf, -inf), (-inf, inf), (nan, 0.25), (0.5, nan), (nan, inf)]
        ys, xs = rng.integers(0, h, len(bad)), rng.integers(0, w, len(bad))
        for (bx, by), y, x in zip(bad, ys, xs):
            flow[0, :, y, x] = (bx, by)
            mask[0, y, x] = 1.0
    else:
        raise KeyError(name)
    out = dict(name=name, h=h, w=w, n=n, group_size=gs, image=image, mask=mask, z=z, flow=np.ascontiguousarray(flow, F32))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def case_reference(name, chain):
    c = case(name)
    return reference(c["image"], c["mask"], c["z"], c["flow"], c["group_size"], chain)


def gmax_bits(z, group_size):
    """what warp_project_kernel leaves per group: the bit pattern of the fp32 log1p of the group's maximum of max(z, 0)"""
    _, gz = group_lmax(np.asarray(z, F32), group_size)
    return np.log1p(gz.astype(F32)).astype(F32).view(np.uint32)


# ---- the projection forms: points that project onto the case's destinations -----------------------------------------------------------------------
@lru_cache(maxsize=None)
def points_case(name, share=True, group_size=None):
    """Operands of g3_render_items_f32 for a case: every item of the case becomes a SOURCE view whose points project (identity rotation, so z stays
    what the case says) onto the case's destinations; with `share` one more item renders source 0 again from a camera moved SHIFT_PX pixels along x
    (n_src < n, src_index shares a source). The reference takes z and flow from oracle.warp_oracle.project_points / splat_indices on these very
    operands: the fp32 rounding of the projection is part of the case."""
    c = case(name)
    h, w, ns = c["h"], c["w"], c["n"]
    gs = group_size or c["group_size"]
    K1 = np.array([[FOCAL, 0, w / 2], [0, FOCAL, h / 2], [0, 0, 1]], F32)
    gx = np.arange(w, dtype=np.float64)[None, None, :]
    gy = np.arange(h, dtype=np.float64)[None, :, None]
    u, v, zz = c["flow"][:, 0].astype(np.float64) + gx, c["flow"][:, 1].astype(np.float64) + gy, c["z"].astype(np.float64)
    assert np.isfinite(u).all() and np.isfinite(v).all()
    pts = np.stack([(u - w / 2) * zz / FOCAL, (v - h / 2) * zz / FOCAL, zz], -1).astype(F32)
    src = np.arange(ns, dtype=np.int32)
    if share:
        src = np.concatenate([src, np.zeros(1, np.int32)])
    n = len(src)
    w2c = np.broadcast_to(np.eye(4, dtype=F32), (n, 4, 4)).copy()
    if share:
        w2c[-1, 0, 3] = SHIFT_PX * FLAT_Z / FOCAL
    K = np.broadcast_to(K1, (n, 3, 3)).copy()
    proj, _ = wo.project_points(pts[src], w2c, K)
    idx = wo.splat_indices(proj, h, w)
    z = idx["z"]
    mask = (c["mask"][src] * (z > 0)).astype(F32)
    out = dict(name=name, h=h, w=w, n=n, n_src=ns, group_size=gs, points=pts, image_src=c["image"], mask_src=c["mask"], src_index=src, w2c=w2c, K=K,
               image=c["image"][src], mask=mask, z=z, flow=idx["flow"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def points_reference(name, share=True, group_size=None, chain="hw"):
    p = points_case(name, share, group_size)
    return reference(p["image"], p["mask"], p["z"], p["flow"], p["group_size"], chain)


# ---- tile model -------------------------------------------------------------------------------------------------------------------------------------
def tile_model(mask, flow, h, w):
    """What the window kernels see per 32 x 32 SOURCE tile, in numpy: origin (smallest north-west corner of the valid pixels), extent (up to the largest
    south-east corner) and the thread -> pixel map (thread = 32 * ((y % 32) / 4) + x % 32 owns rows 4 * (thread / 32) .. + 3 of one column; a wave is 8 rows
    x 32 columns, its lanes >= 32 hold the rows 4 .. 7). Returns counts of the situations the merge phases, the owner map and the gather pass act on - for
    assertions on a case's geometry only, never for expected values."""
    n = mask.shape[0]
    g = geom_from_flow(flow, h, w)
    valid = mask != 0
    tiles_x, tiles_y = (w + TS - 1) // TS, (h + TS - 1) // TS
    ntiles = tiles_x * tiles_y
    Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    tile = np.broadcast_to(((Y // TS) * tiles_x + X // TS)[None], (n, h, w))
    item = np.broadcast_to(np.arange(n)[:, None, None], (n, h, w))
    slot = (item * ntiles + tile)[valid]
    big = np.iinfo(np.int64).max
    ox, oy = np.full(n * ntiles, big), np.full(n * ntiles, big)
    mx, my = np.full(n * ntiles, -1), np.full(n * ntiles, -1)
    np.minimum.at(ox, slot, g["fx"][valid])
    np.minimum.at(oy, slot, g["fy"][valid])
    np.maximum.at(mx, slot, g["cx"][valid])
    np.maximum.at(my, slot, g["cy"][valid])
    live = mx >= 0
    ex, ey = np.where(live, mx - ox + 1, 0), np.where(live, my - oy + 1, 0)
    out = {}
    # corner ids (y << 16 | x); -1 / -2 where the pixel is masked (two values, so that a dead west never equals a dead east)
    ident = lambda yy, xx, dead: np.where(valid, (g[yy] << 16) | g[xx], dead)
    tw = [ident("fy", "fx", -1), ident("cy", "fx", -1)]
    te = [ident("fy", "cx", -2), ident("cy", "cx", -2)]
    out["coinciding"] = int((valid & ((g["fy"] == g["cy"]) | (g["fx"] == g["cx"]))).sum())
    # east corner of (y, x - 1) meets a west corner of (y + d, x): same tile (x % 32 != 0), same thread (rows y and y + d in one group of four)
    for d, key in ((0, "ew_row_k"), (-1, "ew_row_k_minus_1"), (1, "ew_row_k_plus_1")):
        cnt = 0
        ys = np.arange(h)
        ok_y = (ys + d >= 0) & (ys + d < h) & ((ys + d) // 4 == ys // 4)
        ya = ys[ok_y]
        okx = (np.arange(1, w) % TS) != 0
        for e in te:
            for wv in tw:
                cnt += int(((e[:, ya][:, :, :-1] == wv[:, ya + d][:, :, 1:]) & okx[None, None, :]).sum())
        out[key] = cnt
    ys = np.arange(h - 1)
    ya = ys[ys % 4 != 3]
    col = sum(int(((a[:, ya] == b[:, ya + 1]) & (a[:, ya] >= 0)).sum()) for a in tw for b in tw)
    out["column"] = col
    cross = 0
    for j in (1, 2):
        ya = np.arange(h - j)
        ya = ya[ya % 8 == 3]
        cross += sum(int(((a[:, ya] == b[:, ya + j]) & (a[:, ya] >= 0)).sum()) for a in tw for b in tw)
    out["cross_half"] = cross
    # west corners of different COLUMNS never merge (phase 2 moves east corners, phase 3 runs down one column): two columns of a tile that aim at
    # one window texel compete for its owner
    keys = []
    for c in range(2):
        tid = tw[c][valid]
        lx, ly = (tid & 0xffff) - ox[slot], (tid >> 16) - oy[slot]
        inw = (lx < WIN) & (ly < WIN)
        keys.append(np.stack([slot[inw], tid[inw], np.broadcast_to(X[None], (n, h, w))[valid][inw]], 1))
    k = np.unique(np.concatenate(keys), axis=0)
    _, per_texel = np.unique(k[:, :2], axis=0, return_counts=True)
    out["competing_owner_texels"] = int((per_texel >= 2).sum())
    beyond = 0
    for _, yy, xx in CORNERS:
        beyond += int((((g[xx][valid] - ox[slot]) >= WIN) | ((g[yy][valid] - oy[slot]) >= WIN)).sum())
    out["corners_beyond_window"] = beyond
    out["rect_wider_than_window"] = int(((ex > WIN) | (ey > WIN)).sum())
    # how many (full) rectangles cover an accumulator texel
    cov = np.zeros((n, h + 3, w + 3), np.int64)
    for s in np.nonzero(live)[0]:
        i = s // ntiles
        y0, x0, y1, x1 = oy[s], ox[s], oy[s] + ey[s], ox[s] + ex[s]
        cov[i, y0, x0] += 1
        cov[i, y1, x0] -= 1
        cov[i, y0, x1] -= 1
        cov[i, y1, x1] += 1
    cov = cov.cumsum(1).cumsum(2)[:, :h + 2, :w + 2]
    out["texels_in_one_rect"] = int((cov == 1).sum())
    hi = np.zeros((n, h + 3, w + 3), np.int64)  # ... and how many of those rectangles belong to source tiles a first 1024-tile scan does not see
    for s in np.nonzero(live)[0]:
        if s % ntiles >= 1024:
            hi[s // ntiles, oy[s]:oy[s] + ey[s], ox[s]:ox[s] + ex[s]] += 1
    out["texels_in_two_rects_one_of_a_tile_from_1024_on"] = int(((cov == 2) & (hi[:, :h + 2, :w + 2] == 1)).sum())
    out["texels_in_two_or_more"] = int((cov >= 2).sum())
    ring = dict(north=0, south=0, west=0, east=0)
    for _, yy, xx in CORNERS:
        ring["north"] += int((g[yy][valid] == 0).sum())
        ring["south"] += int((g[yy][valid] == h + 1).sum())
        ring["west"] += int((g[xx][valid] == 0).sum())
        ring["east"] += int((g[xx][valid] == w + 1).sum())
    out.update({f"ring_{k_}": v for k_, v in ring.items()})
    # the gather pass: rectangles that meet a destination tile's texels [dy0 + 1, dy0 + 32] x [dx0 + 1, dx0 + 32] (its hit test), for item 0
    o_x, o_y, e_x, e_y, lv = ox[:ntiles], oy[:ntiles], ex[:ntiles], ey[:ntiles], live[:ntiles]
    dy0, dx0 = (np.arange(ntiles) // tiles_x) * TS, (np.arange(ntiles) % tiles_x) * TS
    hit = lv[None, :] & (o_x[None, :] <= dx0[:, None] + TS) & ((o_x + e_x)[None, :] > dx0[:, None] + 1) & (o_y[None, :] <= dy0[:, None] + TS) & \
        ((o_y + e_y)[None, :] > dy0[:, None] + 1)
    per_dest = hit.sum(1)
    densest = int(per_dest.argmax())
    out["source_tiles"] = ntiles
    out["most_rects_in_one_dest_tile"] = int(per_dest.max())
    out["largest_tile_index_there"] = int(np.nonzero(hit[densest])[0].max()) if per_dest.max() else -1
    out["fitting_lists_with_a_tile_from_1024_on"] = int(((per_dest <= 256) & hit[:, 1024:].any(1)).sum())
    out["empty_source_tiles"] = int((~live).sum())
    out["origins"] = np.stack([ox, oy, ex, ey], 1).reshape(n, ntiles, 4)
    return out
