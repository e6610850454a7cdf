"""Pins tests/splat_ref.py, the fp64 reference that tests/test_splat_kernels_gpu.py holds the splat and gather kernels to (no GPU needed).

  * geometry: geom_from_flow is oracle.warp_oracle.splat_indices bit for bit on the projected cases;
  * the fp32 oracle (warp_oracle.bilinear_splatting) lies within the per-texel bars on every case, masks equal. Measured: worst 0.35 of the bar (rows),
    0.30 on quarter, 0.18 on the 1056 x 1024 collapse (up to 41 contributions per texel), 0.29 on levels (depth 0.30);
  * mutants of the contribution list miss the bar on a texel they touch, at 20 seeded positions per flat case: one contribution of bilinear weight >= 1/16
    dropped, added twice, moved to the neighbouring texel, the north-east and south-west weights of one pixel swapped - and, on `levels`, the item's own
    maximum in place of the group's. Measured: the weakest of the 480 mutants misses by 3.8e3 bars (many_tiles, added twice), the own-maximum mutant misses
    on all 5 747 mixed-z texels of item 0, by at least 38 bars at the 20 seeded positions;
  * sensitivity (a condition): of the contributions with bilinear weight >= 1/16 in texels that have at least two, the share whose removal moves the
    reference by less than 16 bars (largest channel) is at most 1 %. "At least two" counts PIXELS that reach the texel with such a weight: corners of one
    pixel that coincide on an integer coordinate are two contributions of one colour, and beside a neighbour of weight 1e-7 (the `rows` case is made of
    those) a contribution is alone in its texel - no change of its weight moves a ratio it forms alone (counting contributions instead gave 3 % on quarter,
    5 % on rows, 53 % on stretch). Measured: 0 of 15 280 .. 33 694 in every flat case, smallest shift 224 bars (many_tiles);
  * the tile model's counts per case, flow form and projected form: each case still reaches what it was built for (floors are a tenth or less of the
    counts the generators give today, or the threshold itself where a path starts at one: 257 rectangles, tile 1024; every count is printed)."""
import numpy as np
import pytest

from oracle import warp_oracle as wo
from tests import splat_ref as sr

F32 = np.float32
POINT_CASES = sr.SMALL_CASES + sr.TINY_CASES


@pytest.mark.parametrize("name", POINT_CASES)
def test_geometry_is_the_oracles(name):
    p = sr.points_case(name)
    proj, _ = wo.project_points(p["points"][p["src_index"]], p["w2c"], p["K"])
    idx = wo.splat_indices(proj, p["h"], p["w"])
    g = sr.geom_from_flow(idx["flow"], p["h"], p["w"])
    for k in g:
        assert np.array_equal(g[k], idx[k]) and g[k].dtype == idx[k].dtype, k
    if name in sr.FLAT_CASES:
        assert np.all(p["z"] == F32(sr.FLAT_Z)), "an identity rotation keeps a flat depth flat"


@pytest.mark.parametrize("name", sr.ALL_CASES)
def test_fp32_oracle_within_the_bars(name):
    c = sr.case(name)
    ref = sr.case_reference(name, "libm")
    idx = sr.geom_from_flow(c["flow"], c["h"], c["w"])
    idx["z"] = c["z"]
    with np.errstate(all="ignore"):
        fr, m = wo.bilinear_splatting(c["image"], c["mask"][:, None], idx, True)
        dp, _ = wo.bilinear_splatting(c["z"][:, None], c["mask"][:, None], idx, False)
    assert np.array_equal(m[:, 0], ref["mask"])
    wf, ef = sr.compare(f"{name} frame", fr, ref["frame"], ref["frame_bar"])
    wd, ed = sr.compare(f"{name} depth", dp[:, 0], ref["depth"], ref["depth_bar"])
    print(f"[oracle {name}] frame worst {wf:.3f} of the bar, bitwise fp32(ref) {ef:.4f}; depth worst {wd:.3f}, bitwise {ed:.4f}; most contributions in a texel "
          f"{int(ref['n_t'].max())}, largest delta {ref['delta'].max():.2e}")
    assert ref["delta"].max() < 1e-4 and 0 < ref["mask"].mean()
    assert np.isfinite(ref["frame"]).all() and np.isfinite(ref["depth"]).all()


# ---- mutants -------------------------------------------------------------------------------------------------------------------------------------
def _texel_miss(C, tex, wgt, ref, t):
    """the resolved value of flat texel t under the mutated (tex, wgt), as the largest |value - ref| / bar over r g b (inf where the mask flips)"""
    n, h, w = C["shape"]
    i, rest = divmod(int(t), (h + 2) * (w + 2))
    y, x = divmod(rest, w + 2)
    if not (1 <= y <= h and 1 <= x <= w):
        return 0.0
    sel = tex == t
    den = wgt[sel].sum()
    if (den > 0) != bool(ref["mask"][i, y - 1, x - 1]):
        return np.inf
    if not den > 0:
        return 0.0
    val = np.clip((C["col"][sel, :3] * wgt[sel, None]).sum(0) / den, -1, 1)
    err = np.abs(val - ref["frame"][i, :, y - 1, x - 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / ref["frame_bar"][i, :, y - 1, x - 1]).max())


def _eligible(C, ref):
    n, h, w = C["shape"]
    rest = C["tex"] % ((h + 2) * (w + 2))
    y, x = rest // (w + 2), rest % (w + 2)
    inside = (y >= 1) & (y <= h) & (x >= 1) & (x <= w)
    return inside & (C["b"] >= 1.0 / 16) & (ref["n_pix"].reshape(-1)[C["tex"]] >= 2) & (C["w"] != 0)


@pytest.mark.parametrize("name", sr.FLAT_CASES)
def test_mutants_miss_the_bar(name):
    c = sr.case(name)
    C = sr.contributions(c["image"], c["mask"], c["z"], c["flow"], c["group_size"])
    ref = sr.case_reference(name, "hw")
    n, h, w = C["shape"]
    rng = np.random.default_rng(77)
    el = np.nonzero(_eligible(C, ref))[0]
    assert len(el) >= 20
    P = len(C["tex"]) // 4
    weakest = {}
    for kind in ("drop", "twice", "move", "swap"):
        misses = []
        if kind == "swap":  # pixels whose north-east and south-west weights differ, the north-east corner eligible
            ne, sw = np.arange(2 * P, 3 * P), np.arange(P, 2 * P)
            ok = (np.abs(C["b"][ne] - C["b"][sw]) >= 1.0 / 16) & _eligible(C, ref)[ne]
            pos = ne[ok]
        else:
            pos = el
        for i in rng.choice(pos, 20, replace=False):
            tex, wgt = C["tex"].copy(), C["w"].copy()
            touched = [tex[i]]
            if kind == "drop":
                wgt[i] = 0.0
            elif kind == "twice":
                wgt[i] *= 2.0
            elif kind == "move":
                x = tex[i] % (w + 2)
                tex[i] += 1 if x < w else -1
                touched.append(tex[i])
            else:
                j = i - P  # the same pixel's south-west corner
                wgt[i], wgt[j] = wgt[j], wgt[i]
                touched.append(tex[j])
            miss = max(_texel_miss(C, tex, wgt, ref, t) for t in touched)
            assert miss > 1.0, f"{name}: mutant '{kind}' of contribution {i} stays within the bar ({miss:.3f})"
            misses.append(miss)
        weakest[kind] = min(misses)
    print(f"[mutants {name}] 20 positions each, weakest miss in bars: " + ", ".join(f"{k} {v:.3g}" for k, v in weakest.items()))
    assert min(weakest.values()) > 16


def test_levels_item_maximum_mutant_misses_the_bar():
    """`levels`: two items in one group, two depth levels per item; the weight ratio between an item's levels lies in [4, 64]; the second item sets the group
    maximum. An implementation that takes the maximum per item changes item 0's ratio by far more than the bar."""
    c = sr.case("levels")
    assert c["group_size"] == 2 and c["z"][1].max() > c["z"][0].max()
    C = sr.contributions(c["image"], c["mask"], c["z"], c["flow"], 2)
    ratios = []
    for i in range(c["n"]):
        E = np.unique(C["E"][C["item"] == i])
        assert len(E) == 2
        ratios.append(float(np.exp(E[1] - E[0])))
        assert 4.0 <= ratios[-1] <= 64.0, ratios
    ref = sr.case_reference("levels", "hw")
    mut = sr.reference(c["image"], c["mask"], c["z"], c["flow"], 1, "hw")
    mixed = ~ref["same_z"][0, 1:-1, 1:-1] & (ref["mask"][0] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        miss = (np.abs(mut["frame"][0] - ref["frame"][0]) / ref["frame_bar"][0]).max(0)
    ys, xs = np.nonzero(mixed)
    pick = np.random.default_rng(78).choice(len(ys), 20, replace=False)
    at20 = miss[ys[pick], xs[pick]]
    print(f"[mutant levels] weight ratios between the levels {ratios[0]:.2f} / {ratios[1]:.2f}; the item's own maximum misses the bar on {float((miss[mixed] > 1).mean()):.4f} of "
          f"the {int(mixed.sum())} mixed-z texels of item 0, weakest of 20 seeded positions {at20.min():.3g} bars")
    assert np.all(at20 > 1.0) and mixed.sum() > 1000
    assert np.array_equal(mut["frame"][1], ref["frame"][1]), "item 1 holds the group maximum: its own maximum is the same number"


@pytest.mark.parametrize("name", sr.FLAT_CASES)
def test_every_contribution_is_visible(name):
    c = sr.case(name)
    C = sr.contributions(c["image"], c["mask"], c["z"], c["flow"], c["group_size"])
    ref = sr.case_reference(name, "hw")
    n, h, w = C["shape"]
    el = np.nonzero(_eligible(C, ref))[0]
    t = C["tex"][el]
    num, den = ref["num"].reshape(-1, 4)[t, :3], ref["den"].reshape(-1)[t]
    absn = ref["absnum"].reshape(-1, 4)[t, :3]
    bar = (((ref["n_t"].reshape(-1)[t] + 8) * sr.U + 2.0 * np.where(ref["same_z"].reshape(-1)[t], 0.0, ref["delta"].reshape(-1)[t]))[:, None] * absn / den[:, None])
    wi = C["w"][el]
    without = (num - C["col"][el, :3] * wi[:, None]) / (den - wi)[:, None]
    shift = (np.abs(without - num / den[:, None]) / bar).max(1)
    share = float((shift < 16).mean())
    print(f"[sensitivity {name}] {len(el)} contributions of bilinear weight >= 1/16 in texels with at least two; removal moves the reference by < 16 bars for "
          f"{int((shift < 16).sum())} of them (share {share:.5f}, cap 0.01); smallest shift {shift.min():.3g} bars")
    assert len(el) >= 1000 and share <= 0.01


# ---- what each case reaches ------------------------------------------------------------------------------------------------------------------------
FLOORS = {
    "quarter": dict(coinciding=300, ew_row_k=1000, ew_row_k_minus_1=300, ew_row_k_plus_1=300, texels_in_one_rect=900, texels_in_two_or_more=50),
    "rows": dict(ew_row_k=1000, ew_row_k_minus_1=400, ew_row_k_plus_1=400, column=400, cross_half=90),
    "fold": dict(competing_owner_texels=280),
    "stretch": dict(corners_beyond_window=600, rect_wider_than_window=8, texels_in_one_rect=1000, texels_in_two_or_more=20),
    "scatter": dict(ring_north=70, ring_south=70, ring_west=70, ring_east=70, corners_beyond_window=2900),
    "levels": dict(ew_row_k=1000, column=400, cross_half=90),
    "many_tiles": dict(source_tiles=1025, most_rects_in_one_dest_tile=257, largest_tile_index_there=1024, texels_in_two_or_more=90),
    "far_tiles": dict(source_tiles=1025, fitting_lists_with_a_tile_from_1024_on=1, texels_in_two_rects_one_of_a_tile_from_1024_on=100, empty_source_tiles=1000),
    "tiny_33x32": dict(source_tiles=2, cross_half=10),
    "nonfinite": dict(ring_north=1, ring_south=1, ring_west=1, ring_east=1, corners_beyond_window=300),
}


@pytest.mark.parametrize("variant", ["flow", "projected"])
@pytest.mark.parametrize("name", sr.ALL_CASES)
def test_tile_model_coverage(name, variant):
    if variant == "projected":
        if name == "nonfinite":
            return  # the projection forms take points: no flow planes to poison
        c = sr.points_case(name, name not in sr.BIG_CASES)
    else:
        c = sr.case(name)
    tm = sr.tile_model(c["mask"], c["flow"], c["h"], c["w"])
    org = tm.pop("origins")
    print(f"[coverage {name} {variant}] " + ", ".join(f"{k} {v}" for k, v in tm.items()))
    for k, floor in FLOORS.get(name, {}).items():
        assert tm[k] >= floor, f"{name} ({variant}): {k} = {tm[k]}, the case was built for at least {floor}"
    assert org.shape == (c["n"], ((c["h"] + 31) // 32) * ((c["w"] + 31) // 32), 4)
    if name == "nonfinite":  # the poisoned pixels' contributions land in the cropped ring and nowhere in the frame
        C = sr.contributions(c["image"], c["mask"], c["z"], c["flow"], c["group_size"])
        bad = ~np.isfinite(c["flow"][C["item"], :, C["py"], C["px"]]).all(1)
        rest = C["tex"][bad] % ((c["h"] + 2) * (c["w"] + 2))
        y, x = rest // (c["w"] + 2), rest % (c["w"] + 2)
        assert bad.sum() == 4 * 12 and np.all((y == 0) | (y == c["h"] + 1) | (x == 0) | (x == c["w"] + 1))
