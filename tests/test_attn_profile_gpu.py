"""GPU: g3_attn_pattern_profile_bf16 + g3_attn_pattern_select (ops.attn_pattern_profile) against the fp64 restatement of tests/attn_profile_ref.py.

RECALL BAR, derived, not measured: every recall within 2e-4 ABSOLUTE of the fp64 reference. The tests normalise rows to ||q|| = ||k|| = sqrt(128), so
sum_i |q_i k_i| <= 128; accumulating 128 terms in fp32 errs by at most 128 * 2^-24 * 128 * scale (0.0884) = 8.6e-5 in a logit, which is the same
RELATIVE error in each exp term, and a ratio of two such sums errs by at most twice that. Each test prints its measured worst value."""
import math

import numpy as np
import pytest
import torch

from tests import attn_profile_ref as ref

pytestmark = pytest.mark.gpu

BAR = 2e-4
DEV = "cuda:0"


def _normalised(x: torch.Tensor, H: int, norm: float = math.sqrt(128.0)) -> torch.Tensor:
    """[rows, H*128] fp32 -> bf16 with every head's 128-vector scaled to `norm`."""
    v = x.reshape(x.shape[0], H, 128)
    return (v * (norm / v.norm(dim=2, keepdim=True))).reshape(x.shape[0], H * 128).to(torch.bfloat16)


_CACHE = {}


def _inputs_832():
    """S = 832, B = 1, H = 2: q, k (CPU bf16) and the fp64 recall of the hand-made 3-pattern table at the 13 sample rows - computed once."""
    if "832" not in _CACHE:
        g = torch.Generator().manual_seed(11)
        q = _normalised(torch.randn(832, 256, generator=g), 2)
        k = _normalised(torch.randn(832, 256, generator=g), 2)
        _CACHE["832"] = (q, k, ref.recall_ref(q, k, 832, 1, 2, ref.hand_table_832(), ref.SAMPLE_ROWS_832))
    return _CACHE["832"]


def _plan_832():
    from gen3c_amd import ops
    table = ops.attn_range_table(ref.hand_table_832(), 832, device=DEV)
    return ops.attn_profile_plan(table, sample_rows=ref.SAMPLE_ROWS_832)


def _check(plan, hp, want, bar, what):
    got = plan.recall.cpu().double().numpy()
    worst = float(np.abs(got - want).max())
    score, hp_want = ref.select_ref(want)
    margin = np.sort(score, axis=1)
    margin = float((margin[:, -1] - margin[:, -2]).min()) if score.shape[1] > 1 else float("inf")
    print(f"[attn profile {what}] worst |recall - fp64| = {worst:.3e} (bar {bar:.1e}); smallest fp64 score margin {margin:.3e}; head_pattern {hp.cpu().tolist()}")
    assert np.isfinite(got).all() and worst <= bar
    assert float(np.abs(plan.score.cpu().double().numpy() - score).max()) <= bar
    return hp_want, margin


@pytest.mark.parametrize("n_chunks", [1, 5, 13])
def test_hand_made_table_every_chunking(n_chunks):
    from gen3c_amd import ops
    q, k, want = _inputs_832()
    plan = _plan_832()
    assert plan.n == 13 and {0, 255, 256, 767, 768, 831} <= set(plan.sample_rows.tolist())
    qd, kd = q.to(DEV), k.to(DEV)
    hp = ops.attn_pattern_profile(qd, kd, 832, 1, 2, plan, n_chunks=n_chunks)
    hp_want, margin = _check(plan, hp, want, BAR, f"S=832 n=13 n_chunks={n_chunks}")
    if margin > 2 * BAR:
        assert hp.cpu().tolist() == hp_want.tolist()
    if n_chunks == 5:  # the same launch again: bit for bit
        r1, s1, h1 = plan.recall.clone(), plan.score.clone(), hp.clone()
        plan.recall.fill_(-1.0)
        hp2 = ops.attn_pattern_profile(qd, kd, 832, 1, 2, plan, n_chunks=5)
        assert torch.equal(plan.recall, r1) and torch.equal(plan.score, s1) and torch.equal(hp2, h1)


def _planted(n_seed=3):
    """S = 6 144 (T = 6 frames of 1 024), B = 2, H = 3: head 0 plants its frame's coordinate, head 1 coordinate 16 + p // 128, head 2 none."""
    S, B, H = 6144, 2, 3
    g = torch.Generator().manual_seed(n_seed)
    s = torch.arange(S).repeat_interleave(B)  # row s*B + b
    f, p = s // 1024, s % 1024

    def make():
        x = 0.3 * torch.randn(S * B, H, 128, generator=g)
        x[torch.arange(S * B), 0, f] += 4.0
        x[torch.arange(S * B), 1, 16 + p // 128] += 4.0
        return _normalised(x.reshape(S * B, H * 128), H)
    return S, B, H, make(), make()


@pytest.mark.parametrize("n", [64, 33])
def test_planted_heads_are_found(n):
    from gen3c_amd import ops, sparse_attn
    S, B, H, q, k = _planted()
    tab = sparse_attn.build_spec(("auto", ("frame", 0, 0), ("band", 0.0625, 0)), 6, 1024)
    dens = sparse_attn.tile_density(tab, S)
    assert abs(dens[0] - 0.167) < 1e-3 and abs(dens[1] - 0.344) < 1e-3
    table = ops.attn_range_table(tab, S, device=DEV)
    plan = ops.attn_profile_plan(table, n_samples=n)
    assert plan.sample_rows.tolist() == [((2 * i + 1) * S) // (2 * n) for i in range(n)]
    want = ref.recall_ref(q, k, S, B, H, tab, plan.sample_rows.tolist())
    score, hp_want = ref.select_ref(want)
    print(f"[attn profile planted heads n={n}] fp64 score per head (pattern 0, pattern 1): {np.round(score, 3).tolist()}")
    assert hp_want.tolist() == [0, 1, 1] and float(np.abs(score[:, 0] - score[:, 1]).min()) >= 0.05  # every head is asserted: none is a near-tie
    # q and k as column views of one fused [S*B, 3*H*128] buffer
    qkv = torch.zeros(S * B, 3 * H * 128, dtype=torch.bfloat16, device=DEV)
    qkv[:, :H * 128], qkv[:, H * 128:2 * H * 128] = q.to(DEV), k.to(DEV)
    hp = ops.attn_pattern_profile(qkv[:, :H * 128], qkv[:, H * 128:2 * H * 128], S, B, H, plan)
    _check(plan, hp, want, BAR, f"planted heads S=6144 B=2 H=3 n={n} (fused-buffer views)")
    assert hp.cpu().tolist() == [0, 1, 1]
    hp_c = ops.attn_pattern_profile(q.to(DEV), k.to(DEV), S, B, H, plan, n_chunks=7).clone()
    assert hp_c.cpu().tolist() == [0, 1, 1]


def test_cover_pattern_recall_is_exactly_one_and_ties_take_the_lower_index():
    from gen3c_amd import ops, sparse_attn
    S, B, H = 1920, 2, 2
    g = torch.Generator().manual_seed(23)
    q = _normalised(torch.randn(S * B, H * 128, generator=g), H).to(DEV)
    k = _normalised(torch.randn(S * B, H * 128, generator=g), H).to(DEV)
    cover, sparse = sparse_attn.frame_ranges(5, 384, 5, 0), sparse_attn.frame_ranges(5, 384, 0, 1)
    assert sparse_attn.tile_density(cover, S) == [1.0] and sparse_attn.tile_density(sparse, S)[0] < 0.5
    for tabs, hp_want, cover_at in (([sparse, cover], [1, 1], [1]), ([cover, sparse], [0, 0], [0]), ([sparse, cover, cover], [1, 1], [1, 2]),
                                    ([sparse, sparse], [0, 0], [])):
        tab = sparse_attn.stack_tables(tabs)
        plan = ops.attn_profile_plan(ops.attn_range_table(tab, S, device=DEV), n_samples=24)
        for n_chunks in (None, 1, 30):
            hp = ops.attn_pattern_profile(q, k, S, B, H, plan, n_chunks=n_chunks)
            for p in cover_at:
                assert bool((plan.recall[..., p] == 1.0).all()), "the cover's recall is 1.0f exactly for every (b, h, i)"
                assert bool((plan.score[:, p] == 1.0).all())
            assert hp.cpu().tolist() == hp_want
        if len(tabs) == 2 and tabs[0] is tabs[1]:
            assert torch.equal(plan.recall[..., 0], plan.recall[..., 1])
        want = ref.recall_ref(q.cpu(), k.cpu(), S, B, H, tab, plan.sample_rows.tolist())
        _check(plan, hp, want, BAR, f"cover S=1920 B=2 H=2, {len(tabs)} patterns")


def test_large_logits_stay_finite_and_accurate():
    from gen3c_amd import ops
    q, k, _ = _inputs_832()
    f = 14.0  # |l| log2(e) reaches about 80
    qs = (q.float() * f).to(torch.bfloat16)
    want = ref.recall_ref(qs, k, 832, 1, 2, ref.hand_table_832(), ref.SAMPLE_ROWS_832)
    peak = float(((qs.float()[ref.SAMPLE_ROWS_832].reshape(13, 2, 128).permute(1, 0, 2) @ k.float().reshape(832, 2, 128).permute(1, 2, 0)).abs().max())
                 / math.sqrt(128) * math.log2(math.e))
    assert 60.0 <= peak <= 110.0, peak
    grow = float(qs.float().reshape(832, 2, 128).norm(dim=2).max()) / math.sqrt(128.0)  # sum |q_i k_i| grew by this factor
    plan = _plan_832()
    for n_chunks in (1, 5, 13):
        hp = ops.attn_pattern_profile(qs.to(DEV), k.to(DEV), 832, 1, 2, plan, n_chunks=n_chunks)
        assert torch.isfinite(plan.recall).all() and torch.isfinite(plan.score).all()
        _check(plan, hp, want, BAR * grow, f"large logits (peak |l| log2e = {peak:.1f}, bar x {grow:.2f}) n_chunks={n_chunks}")


def test_selected_patterns_launch_as_the_host_uploaded_ones():
    from gen3c_amd import ops
    q, k, _ = _inputs_832()
    S, B, H = 832, 1, 2
    g = torch.Generator().manual_seed(2)
    v = torch.randn(S * B, H * 128, generator=g).to(torch.bfloat16).to(DEV)
    qd, kd = q.to(DEV), k.to(DEV)
    vt = ops.transpose_v(v, S, B, H)
    plan = _plan_832()
    selected = ops.attn_pattern_profile(qd, kd, S, B, H, plan)
    outs = []
    for hp_dev in (selected, torch.tensor([2, 0], dtype=torch.int32, device=DEV), torch.tensor([1, 2], dtype=torch.int32, device=DEV)):
        o_dev = ops.self_attn_ranges(qd, kd, vt, S, B, H, 0.0, plan.table, head_pattern_dev=hp_dev)
        host_table = ops.attn_range_table(ref.hand_table_832(), S, head_pattern=hp_dev.cpu().tolist(), device=DEV)
        assert torch.equal(o_dev, ops.self_attn_ranges(qd, kd, vt, S, B, H, 0.0, host_table))
        outs.append(o_dev)
    assert not torch.equal(outs[1], outs[2])  # (the keyword is read)
    assert torch.equal(ops.self_attn_ranges(qd, kd, vt, S, B, H, 0.0, plan.table),
                       ops.self_attn_ranges(qd, kd, vt, S, B, H, 0.0, plan.table, head_pattern_dev=torch.zeros(2, dtype=torch.int32, device=DEV)))
    with pytest.raises(ValueError, match="head_pattern_dev must be a contiguous int32"):
        ops.self_attn_ranges(qd, kd, vt, S, B, H, 0.0, plan.table, head_pattern_dev=torch.zeros(3, dtype=torch.int32, device=DEV))
