"""GPU: the DiT's per-head pattern selection (set_self_attn_pattern(("auto", ...))) on the tiny 2-block, 2-head net of tests/_mxfp8_tiny_dit.py with a
latent [1, 16, 6, 16, 16]: 6 latent frames of 8 x 8 = 64 tokens, S = 384 (tests/test_dit_ranges_gpu.py's shape and tolerances)."""
import math

import numpy as np
import pytest
import torch

from tests import attn_profile_ref as ref
from tests._mxfp8_tiny_dit import _inputs, _net, _run

pytestmark = pytest.mark.gpu

SHAPE = dict(B=1, T=6, H=16, W=16)


def test_auto_over_two_identical_candidates_is_the_single_pattern():
    dev = torch.device("cuda:0")
    inp = _inputs(**SHAPE)
    net = _net(dev)
    net.set_self_attn_pattern("frame:1:1")
    y_one = _run(net, inp, dev)
    assert net.self_attn_head_patterns() is None
    net.set_self_attn_pattern("auto=frame:1:1,frame:1:1")
    y_auto = _run(net, inp, dev)
    assert torch.equal(y_auto, y_one)
    assert net.self_attn_head_patterns() == [[0, 0], [0, 0]]  # ties: the lower index
    net.set_self_attn_pattern("auto=frame:5:0,frame:0:6")  # every candidate covers every tile: the plain branch
    y_cover = _run(net, inp, dev)
    net.set_self_attn_pattern(None)
    assert torch.equal(y_cover, _run(net, inp, dev))


def _masked_softmax_attention(calls):
    def attn(q, k, vt, S, B, H, logit_bound, table, out=None, softmax_scale=None, head_pattern_dev=None):
        from gen3c_amd import ops
        hp = head_pattern_dev.cpu().tolist()
        calls.append((q.clone().cpu(), k.clone().cpu(), hp, table))
        o = torch.empty(S * B, H * 128, device=q.device, dtype=torch.bfloat16)
        for h in range(H):
            mask = ops.ranges_attn_mask(table, S, pattern=hp[h]).to(q.device)
            sl = slice(h * 128, (h + 1) * 128)
            for b in range(B):
                sc = (q[b::B, sl].float() @ k[b::B, sl].float().t()) / math.sqrt(128)
                o[b::B, sl] = (torch.softmax(sc.masked_fill(~mask, -math.inf), dim=-1) @ vt[b, h, :, :S].float().t()).to(torch.bfloat16)
        return o
    return attn


def test_auto_picks_the_superset_and_matches_the_masked_softmax(monkeypatch):
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs(**SHAPE)
    net = _net(dev)
    lines = []
    net.self_attn_pattern_log = lines.append
    net.set_self_attn_pattern("auto=frame:0:0,frame:1:1")
    y = _run(net, inp, dev).float()
    assert net.self_attn_head_patterns() == [[1, 1], [1, 1]]  # the second candidate holds every key of the first
    assert len(lines) == 2 and "0 = frame:0:0 tile density 0.500, 1 = frame:1:1 tile density 0.750" in lines[0] and "warning" in lines[1]
    calls = []
    monkeypatch.setattr(ops, "self_attn_ranges", _masked_softmax_attention(calls))
    y_ref = _run(net, inp, dev).float()
    monkeypatch.undo()
    rel = float((y - y_ref).norm() / y_ref.norm())
    mx = float((y - y_ref).abs().max())
    print(f"[dit auto=frame:0:0,frame:1:1, 384 tokens] rel_l2={rel:.3e} max_abs={mx:.3e} ref_absmax={float(y_ref.abs().max()):.3e}")
    assert torch.isfinite(y).all() and rel <= 9e-3 and mx <= 1.0e-2 * float(y_ref.abs().max())
    assert len(calls) == 2 and len(lines) == 2  # one launch per block; the table (and its report) once
    for bi, (q, k, hp, table) in enumerate(calls):  # the captured q | k through the fp64 reference: the same choices
        plan = table.profile[0]
        score, hp_ref = ref.select_ref(ref.recall_ref(q, k, 384, 1, 2, table.ranges.numpy(), plan.sample_rows.tolist()))
        print(f"[dit auto block {bi}] fp64 score margins (pattern 1 - pattern 0) per head: {np.round(score[:, 1] - score[:, 0], 4).tolist()}")
        assert hp == hp_ref.tolist() == [1, 1]


def test_plain_specs_and_no_option_call_without_the_keyword(monkeypatch):
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs(**SHAPE)
    net = _net(dev)
    real, seen = ops.self_attn_ranges, []

    def old_signature(q, k, vt, S, B, H, logit_bound, table, out=None, softmax_scale=None):  # the function before the keyword existed
        seen.append(table.n_patterns)
        return real(q, k, vt, S, B, H, logit_bound, table, out=out, softmax_scale=softmax_scale)
    monkeypatch.setattr(ops, "self_attn_ranges", old_signature)
    _run(net, inp, dev)
    assert seen == []
    net.set_self_attn_pattern("frame:1:1")
    y = _run(net, inp, dev)
    assert seen == [1, 1]
    net.set_self_attn_pattern(("frame", 0, 1))
    _run(net, inp, dev)
    assert seen == [1, 1, 1, 1] and torch.isfinite(y).all()
