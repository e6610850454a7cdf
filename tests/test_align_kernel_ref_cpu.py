"""Pins tests/align_kernel_ref.py (the references of tests/test_align_kernels_gpu.py) on the CPU: against torch.quantile, against the reference's
own results in tests/golden/align_edges.npz (tools/gen_golden_align_edges.py), against oracle/align_oracle.py - and shows that each listed
mutant of csrc/align.hip would miss a bar of the GPU tests on the GPU tests' own inputs."""
import numpy as np
import pytest
import torch

from oracle import align_oracle as ao
from tests import align_kernel_ref as kr

F32 = np.float32
TINY = [f"tiny_counts_{n}" for n in kr.TINY_COUNTS]


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def _inputs(name):
    if name == "grid_stride":
        return kr.build_grid_stride()
    if name in kr.FIXTURE_CASES:
        return kr.load_case(name)
    return kr.build_case(name)


@pytest.mark.parametrize("name", kr.FIXTURE_CASES)
def test_builders_reproduce_the_committed_inputs(name):
    for got, want in zip(kr.build_case(name), kr.load_case(name)):
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_camera_is_the_fixtures():
    K, c2w, _, _ = kr.camera(kr.H, kr.W)
    assert np.array_equal(K, kr.fixture()["K"]) and np.array_equal(c2w, kr.fixture()["c2w"])


def test_case_properties():
    """each case is the edge it claims to be"""
    r = kr.rigid_reference(*kr.load_case("ragged"))
    assert kr.H * kr.W == 851 and 0.7 < r["mask_count"] / 851 < 0.9
    r = kr.rigid_reference(*kr.load_case("plateaus"))
    assert len(np.unique(r["sorted"][0])) == 8 and all(p["a"] == p["b"] for a in r["parts"] for p in a)
    r = kr.rigid_reference(*kr.load_case("plateau_at_rank"))
    s, t = r["sorted"]
    assert kr.multiplicity(s, r["parts"][0][0]["a"]) == 185 and r["parts"][0][0]["a"] == r["parts"][0][0]["b"] == s[0]
    assert kr.multiplicity(t, r["parts"][1][1]["b"]) > 100 and r["parts"][1][1]["a"] == r["parts"][1][1]["b"] == t[-1]
    r = kr.rigid_reference(*kr.load_case("last_digit"))
    for a in range(2):
        k = r["sorted"][a].view(np.uint32)
        assert len(np.unique(k >> 8)) == 1 and len(np.unique(k & 255)) > 64
    r = kr.rigid_reference(*kr.load_case("top_digit"))
    for a in range(2):
        k = r["sorted"][a].view(np.uint32)
        assert all(len(np.unique((k >> sh) & 255)) > 32 for sh in (0, 8, 16)) and len(np.unique(k >> 24)) > 8
    src, tgt, mask = kr.load_case("nonfinite")
    r = kr.rigid_reference(src, tgt, mask)
    assert np.isinf(r["src_inv"]).sum() == 5 and np.isnan(r["src_inv"]).sum() == 3 and r["sorted"][0][-1] == np.inf
    assert 0 < r["sorted"][0][0] < np.finfo(F32).tiny, "a subnormal inverse depth must stay valid"
    assert r["mask_count"] == int(mask.sum()) == r["count"][1] + 4
    for n in kr.TINY_COUNTS:
        assert kr.rigid_reference(*kr.build_case(f"tiny_counts_{n}"))["count"][1] == n
    src, _, _ = kr.build_grid_stride()
    assert src.size == 264967 > 1024 * 256 and -(-src.size // 65536) == 5 and src.size % 5 != 0


@pytest.mark.parametrize("name", list(kr.FIXTURE_CASES) + TINY + ["grid_stride"])
def test_quantile_restatement_is_bitwise_torch_quantile(name):
    src, tgt, mask = _inputs(name)
    r = kr.rigid_reference(src, tgt, mask)
    si, ti, sv, tv, _ = kr.inverses(src, tgt, mask)
    for a, (arr, valid) in enumerate(((si, sv), (ti, tv))):
        tq = torch.quantile(torch.from_numpy(arr[valid]), torch.tensor([0.1, 0.9])).numpy()
        mine = np.array([r["qlo"][a], r["qhi"][a]], F32)
        assert np.array_equal(_bits(tq), _bits(mine)), (name, a, tq, mine)
        assert np.array_equal(_bits(mine), _bits([ao._quantile_linear(arr[valid], 0.1), ao._quantile_linear(arr[valid], 0.9)]))
        if name in kr.FIXTURE_CASES:
            assert np.array_equal(_bits(kr.fixture()[f"{name}_quantiles"][a]), _bits(mine))
        s = r["sorted"][a]  # order statistics: sorted, a permutation of the valid values, floor / ceil ranks
        assert np.all(s[:-1] <= s[1:]) and s.size == valid.sum()
        for qi in range(2):
            p = r["parts"][a][qi]
            assert 0 <= p["hi"] - p["lo"] <= 1 and 0 <= p["weight"] < 1 and p["a"] == s[p["lo"]] and p["b"] == s[p["hi"]]


@pytest.mark.parametrize("name", list(kr.FIT_CASES) + ["grid_stride", "1x7", "7x1", "2x2"])
def test_fp64_fit_is_well_conditioned_and_matches_reference_and_oracle(name):
    if "x" in name:
        src, tgt, mask = kr.build_small_frame(*map(int, name.split("x")))
    else:
        src, tgt, mask = _inputs(name)
    r = kr.rigid_reference(src, tgt, mask)
    print(f"[fit {name}] inliers {r['n_inliers']} cond {r['cond']:.1f} scale {r['scale64']:.7f} bias {r['bias64']:.7f}")
    assert r["n_inliers"] >= 2 and r["cond"] < 1e4
    with np.errstate(all="ignore"):
        mine = (F32(1) / (r["src_inv"] * F32(r["scale64"]) + F32(r["bias64"]))).astype(F32)
        o, so, bo = ao.align_inv_depth_to_depth(r["src_inv"], tgt, mask)
    assert so == F32(r["scale64"]) and bo == F32(r["bias64"])
    assert np.array_equal(_bits(mine), _bits(o))
    if name in kr.FIT_CASES:
        ref = kr.fixture()[f"{name}_rigid"]
        ok = np.isfinite(ref) & (ref != 0)
        assert np.array_equal(ok, np.isfinite(mine) & (mine != 0))
        # where |scale x| < |bias| the result is 1 / bias up to a correction: it shows the relative error of the reference's fp32 lstsq bias
        # (2.3e-6 here, |bias| = 0.05 against inverse depths of 0.3), not of this restatement - those pixels (source depth 3e38) are left out
        own = ok & (np.abs(r["src_inv"] * F32(r["scale64"])) >= np.abs(F32(r["bias64"])))
        assert (ok & ~own).sum() <= 3
        rel = np.abs(mine[own] / ref[own] - 1).max()
        print(f"[fit {name}] max rel vs the reference's lstsq {rel:.2e} ({int((ok & ~own).sum())} bias-dominated pixels left out)")
        assert rel <= 2e-6


def _nonrigid_setup(name):
    src, tgt, mask = kr.load_case(name)
    K, c2w, Kinv, T = kr.camera(kr.H, kr.W)
    with np.errstate(all="ignore"):
        d_s = ao.align_depth(src, tgt, mask)
    return d_s, tgt, mask, Kinv, T


@pytest.mark.parametrize("name", ["ragged", "plateaus", "plateau_at_rank"])
def test_adam_closed_forms_match_the_reference_trajectory(name):
    """steps 1 and 2 from the fp64 gradient against the reference's autograd + torch.optim.Adam (fixture), and the share of pixels the rounding
    margin leaves out (cap of the GPU test: 2 % of the masked pixels)"""
    d_s, tgt, mask, Kinv, T = _nonrigid_setup(name)
    z = kr.fixture()
    g1, _, und1 = kr.grad64(d_s, tgt, mask, Kinv, T, np.ones_like(d_s))
    sc1 = kr.adam_step1(g1)
    keep = ~und1
    ref1 = z[f"{name}_non_rigid_1"] / z[f"{name}_rigid"]
    e1 = np.abs(sc1 - ref1)[keep].max()
    g2, _, und2 = kr.grad64(d_s, tgt, mask, Kinv, T, sc1.astype(F32))
    m, v = kr.adam_step2(g1, g2)
    sc2 = sc1 - kr.LR / (1 - 0.81) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** 2) + 1e-8)
    ref2 = z[f"{name}_non_rigid_2"] / z[f"{name}_rigid"]
    keep2 = keep & ~und2
    e2 = np.abs(sc2 - ref2)[keep2]
    left = (und1 | und2).sum() / mask.sum()
    print(f"[adam {name}] step 1 max |sc - ref| {e1:.2e}; step 2 max {e2.max():.2e} mean {e2.mean():.2e}; left out {left:.4f} of the masked pixels")
    assert left <= 0.02
    assert e1 <= 2e-6
    assert e2.max() <= 2e-3 and e2.mean() <= 1e-5


@pytest.mark.parametrize("hw", [(1, 7), (7, 1)])
def test_small_frames_leave_no_pixel_inside_the_rounding_margin(hw):
    src, tgt, mask = kr.build_small_frame(*hw)
    K, c2w, Kinv, T = kr.camera(*hw)
    g, _, und = kr.grad64(ao.align_depth(src, tgt, mask), tgt, mask, Kinv, T, np.ones(hw, F32))
    assert not und.any() and np.all(g != 0)


def test_oracle_sign_of_nan_is_zero_like_torch():
    """2 steps on the non-finite case: a NaN of sc must not spread through the ARAP box filter (torch.sign(NaN) = 0)"""
    src, tgt, mask = kr.load_case("nonfinite")
    K, c2w, _, _ = kr.camera(kr.H, kr.W)
    with np.errstate(all="ignore"):
        o = ao.align_depth(src, tgt, mask, k=K, c2w=c2w, alignment_method="non_rigid", num_iters=2)
    ref = kr.fixture()["nonfinite_non_rigid_2"]
    ok = np.isfinite(ref) & (ref != 0)
    assert np.array_equal(ok, np.isfinite(o) & (o != 0)) and float(torch.sign(torch.tensor(float("nan")))) == 0.0
    rel = np.abs(o[ok] / ref[ok] - 1)
    assert rel.max() <= 2e-3 and rel.mean() <= 1e-5


def test_all_false_mask_leaves_only_the_border_term():
    d_s, tgt, mask, Kinv, T = _nonrigid_setup("ragged")
    g, _, und = kr.grad64(d_s, tgt, np.zeros_like(mask), Kinv, T, np.ones_like(d_s))
    assert not und.any() and np.all(g[2:-2, 2:-2] == 0) and np.all(g[0] != 0) and np.all(g[:, 0] != 0)


# ---- mutants: each must miss a bar of the GPU test on one of its inputs ---------------------------------------------------------------------------------
MUTANT_INPUTS = list(kr.FIXTURE_CASES) + TINY + ["grid_stride"]


def _state_differs(good, bad):
    """the GPU test's exact bars on the state: counts, order statistics, weights, quantiles"""
    return (good["mask_count"] != bad["mask_count"] or not np.array_equal(good["count"], bad["count"]) or not np.array_equal(_bits(good["stat"]), _bits(bad["stat"]))
            or not np.array_equal(_bits(good["weight"]), _bits(bad["weight"])) or not np.array_equal(_bits(good["qlo"]), _bits(bad["qlo"]))
            or not np.array_equal(_bits(good["qhi"]), _bits(bad["qhi"])))


def _fit_differs(good, bad):
    """the 1-ulp bar on scale / bias"""
    return (abs(bad["scale64"] - good["scale64"]) > kr.ulp32(good["scale64"]) or abs(bad["bias64"] - good["bias64"]) > kr.ulp32(good["bias64"]))


@pytest.mark.parametrize("mutant,expect_in", [
    (dict(rank_n_minus=0), "ragged"), (dict(floor_both=True), "ragged"), (dict(drop_last_digit=True), "last_digit"),
    (dict(mask_count_with_depth=True), "nonfinite")])
def test_state_mutants_are_caught(mutant, expect_in):
    caught = [n for n in MUTANT_INPUTS if _state_differs(kr.rigid_reference(*_inputs(n)), kr.rigid_reference(*_inputs(n), **mutant))]
    print(f"[mutant {mutant}] caught on {caught}")
    assert expect_in in caught


def test_inclusive_inlier_mutant_is_caught_by_the_fit_bar():
    caught = [n for n in kr.FIT_CASES if _fit_differs(kr.rigid_reference(*_inputs(n)), kr.rigid_reference(*_inputs(n), inclusive=True))]
    print(f"[mutant <=] caught on {caught}")
    assert "plateaus" in caught and "plateau_at_rank" in caught


def test_workspace_layout_helper():
    total, off = kr.workspace_layout(23, 37)
    assert off["src_inv"] == 18688 and off["e"] - off["v2"] == 3584 and total == 18688 + 8 * 3584
    raw = np.zeros(total, np.uint8)
    raw[104:108] = np.array([1.5], F32).view(np.uint8)
    st = kr.parse_workspace(raw, 23, 37)
    assert st["scale"][0] == F32(1.5) and st["hist"].size == 2048 and st["partial"].size == 1280 and st["sc"].shape == (23, 37)
