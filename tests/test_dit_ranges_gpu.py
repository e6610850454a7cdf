"""GPU: the DiT's opt-in range-table self-attention (VideoExtendGeneralDIT(self_attn_pattern=...) / set_self_attn_pattern) on the tiny 2-block net of
tests/_mxfp8_tiny_dit.py with a latent [1, 16, 6, 16, 16]: 6 latent frames of 8 x 8 = 64 tokens, S = 384. tests/test_dit_window_gpu.py's three tests
for this option.

 * self_attn_pattern=("frame", 1, 1): the forward against the SAME forward with ops.self_attn_ranges replaced by an fp32 torch softmax masked by
   ops.ranges_attn_mask - the tolerance tests/test_dit_gpu.py holds the HIP forward to against its oracle (rel-L2 <= 9e-3, max-abs <= 1e-2 max|y|).
 * a spec whose table covers every tile: the plain forward, bit for bit, with the same kernel list.
 * option unset: the forward's kernel-timer list names exactly what it named before the option existed (PARENT_KERNELS, recorded from that tree)."""
import math

import pytest
import torch

from tests._mxfp8_tiny_dit import _inputs, _net, _run

pytestmark = pytest.mark.gpu

SHAPE = dict(B=1, T=6, H=16, W=16)
# (timer, kernel) of every timed launch of one forward of the net below at SHAPE, recorded from the tree before this option existed
PARENT_KERNELS = [["flash_attn_fwd", "flash_attn_fwd_v3_kernel<1, 6, 8, false>"]] * 4  # per block: self-attention, cross-attention (384 tokens: the 8-wave kernel)


def _masked_softmax_attention(calls):
    def attn(q, k, vt, S, B, H, logit_bound, table, out=None, softmax_scale=None):
        from gen3c_amd import ops
        calls.append((S, table.n_patterns, table.attended, table.dense, logit_bound))
        mask = ops.ranges_attn_mask(table, S).to(q.device)
        o = torch.empty(S * B, H * 128, device=q.device, dtype=torch.bfloat16)
        for b in range(B):
            for h in range(H):
                sl = slice(h * 128, (h + 1) * 128)
                sc = (q[b::B, sl].float() @ k[b::B, sl].float().t()) / math.sqrt(128)
                o[b::B, sl] = (torch.softmax(sc.masked_fill(~mask, -math.inf), dim=-1) @ vt[b, h, :, :S].float().t()).to(torch.bfloat16)
        return o
    return attn


def _forward_kernels(net, inp, dev):
    from gen3c_amd import ops
    ops.enable_kernel_timers(True)
    try:
        y = _run(net, inp, dev)
        names = [[n, m.get("kernel")] for (n, m, _t) in ops.collected_kernel_timers()]
    finally:
        ops.enable_kernel_timers(False)
    return y, names


def test_dit_pattern_forward_vs_masked_softmax(monkeypatch):
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs(**SHAPE)
    net = _net(dev)
    net.set_self_attn_pattern(("frame", 1, 1))
    y, names = _forward_kernels(net, inp, dev)
    rng = [k for n, k in names if n == "flash_attn_fwd" and k and "_rng_" in k]
    assert rng == ["flash_attn_fwd_w4b_nm_rng_kernel<true>"] * 2, names  # one launch per block, the no-max form (the blocks' bound is in range)
    calls = []
    monkeypatch.setattr(ops, "self_attn_ranges", _masked_softmax_attention(calls))
    y_ref = _run(net, inp, dev)
    attended, dense = ops.window_attn_tiles(384, 64, 1, 1)  # the same function as the window's at this frame length
    assert len(calls) == 2 and all(c[:4] == (384, 1, attended, dense) and c[4] > 0 for c in calls)
    y, y_ref = y.float(), y_ref.float()
    rel = float((y - y_ref).norm() / y_ref.norm())
    mx = float((y - y_ref).abs().max())
    print(f"[dit pattern ('frame', 1, 1), 384 tokens] rel_l2={rel:.3e} max_abs={mx:.3e} ref_absmax={float(y_ref.abs().max()):.3e}")
    assert y.shape == y_ref.shape and torch.isfinite(y).all()
    assert rel <= 9e-3 and mx <= 1.0e-2 * float(y_ref.abs().max())
    monkeypatch.undo()
    net.set_self_attn_pattern(None)
    y_dense = _run(net, inp, dev).float()
    assert not torch.equal(y_dense, y), "the pattern changes the function"


def test_dit_pattern_that_covers_every_tile_is_the_plain_forward():
    dev = torch.device("cuda:0")
    inp = _inputs(**SHAPE)
    from gen3c_amd.dit import VideoExtendGeneralDIT
    plain = _net(dev)
    y_plain, names_plain = _forward_kernels(plain, inp, dev)
    net = VideoExtendGeneralDIT(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=2, num_heads=2, adaln_lora_dim=32,
                                crossattn_emb_channels=128, rope_t_extrapolation_ratio=2.0, device=dev, init_weights=False, self_attn_pattern=("frame", 5, 0))
    net.initialize_weights(randomize_adaln=True, seed=7)
    assert net.self_attn_pattern == ("frame", 5, 0)
    y, names = _forward_kernels(net, inp, dev)
    assert names == names_plain and torch.equal(y, y_plain)
    net.set_self_attn_pattern(("radial", 1.0, 0))  # half-width 64 = the whole frame at every distance
    assert torch.equal(_run(net, inp, dev), y_plain)
    net.set_self_attn_pattern("frame:0:6")
    assert torch.equal(_run(net, inp, dev), y_plain)


def test_dit_without_the_option_launches_what_it_launched_before():
    dev = torch.device("cuda:0")
    net = _net(dev)
    assert net.self_attn_pattern is None
    _y, names = _forward_kernels(net, _inputs(**SHAPE), dev)
    assert names == PARENT_KERNELS
