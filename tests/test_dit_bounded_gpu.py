"""GPU: the DiT forward with the self-attention logit bound on (dit._SELF_ATTN_LOGIT_BOUND, ops.self_attn_bounded) and off, against each other and
against the references the existing DiT tests use.

 * tests/golden/dit_tiny (48 tokens, the smallest DiT test shape): its self-attention is far too short for the one-wave-per-SIMD kernel, so the bounded
   entry must run exactly what the plain one runs - the two forwards are bitwise equal, and both clear the golden tolerance of tests/test_dit_gpu.py.
 * 2 304 tokens, 2 blocks (the shape of test_dit_forward_long_sequence_vs_oracle, the smallest DiT test shape made of whole 64-key tiles), with the
   one-wave kernel selected: the flag decides between flash_attn_fwd_w4b_nm_kernel and flash_attn_fwd_w4b_kernel. Bar on their distance: with unit
   norm weights, as here, one attention layer's result is 3e-3 rel-L2 from the fp32 softmax in the max-tracking form (2.7e-3 .. 3.1e-3 measured, the
   bf16 rounding of P) and at most 1.12 x that in the no-max form (the largest ratio tests/test_attn_bounded_gpu.py measured); the two roundings are
   independent, so the two results are sqrt(1 + 1.12^2) x 3e-3 = 4.5e-3 apart at most. The same 4.5e-3 is asked of the network's output (the
   attention output enters the residual stream through a gate, next to the cross-attention and MLP branches, which do not amplify it on these nets:
   the whole bf16 forward is within 5.2e-3 of the fp32 oracle). Both forwards must clear that test's oracle tolerance as well."""
import pytest
import torch

from tests.golden_io import load_dit_case

pytestmark = pytest.mark.gpu

NM = "flash_attn_fwd_w4b_nm_kernel<true>"


def _forward_on_off(net, kwargs, monkeypatch):
    """{flag: (output fp32 on the host, names of the self-attention kernels launched)}"""
    from gen3c_amd import dit, ops
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(dit, "_SELF_ATTN_LOGIT_BOUND", flag)
        ops.enable_kernel_timers(True)
        try:
            y = net(**kwargs)
            torch.cuda.synchronize()
            S = max(m["Skv"] for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd")
            names = [m["kernel"] for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd" and m["Skv"] == S and m["Sq"] == S]
        finally:
            ops.enable_kernel_timers(False)
        res[flag] = (y.float().cpu(), names)
    return res


def test_dit_tiny_golden_bound_on_and_off_are_the_same_launches():
    from tests.test_dit_gpu import build_net
    dev = torch.device("cuda:0")
    cfg, sd, inp, y_ref = load_dit_case("dit_tiny")
    net = build_net(cfg, sd, dev)
    bf = lambda t: t.to(dev).to(torch.bfloat16)
    kwargs = dict(x=bf(inp["x"]), timesteps=bf(inp["timesteps"]), crossattn_emb=bf(inp["ctx"]), crossattn_mask=None, fps=inp["fps"].to(dev),
                  padding_mask=bf(inp["padding_mask"]), condition_video_indicator=bf(inp["mask"][:, :, :, :1, :1]), condition_video_input_mask=bf(inp["mask"]),
                  condition_video_pose=bf(inp["pose"]))
    with pytest.MonkeyPatch.context() as mp:
        res = _forward_on_off(net, kwargs, mp)
    for flag, (y, names) in res.items():
        rel = float((y - y_ref).norm() / y_ref.norm())
        mx = float((y - y_ref).abs().max())
        print(f"[dit_tiny bound={'on' if flag else 'off'}] rel_l2={rel:.3e} max_abs={mx:.3e} kernels={sorted(set(names))}")
        assert len(names) == cfg["blocks"] and NM not in names
        assert torch.isfinite(y).all() and rel <= 9e-3 and mx <= 1.0e-2 * float(y_ref.abs().max())  # tests/test_dit_gpu.py
    assert res[True][1] == res[False][1]
    assert torch.equal(res[True][0], res[False][0])


def test_dit_2304_tokens_no_max_kernel_vs_max_tracking_and_oracle():
    from gen3c_amd import ops
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from oracle import dit_oracle
    dev = torch.device("cuda:0")
    net = VideoExtendGeneralDIT(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=2, num_heads=2,
                                adaln_lora_dim=32, crossattn_emb_channels=128, rope_t_extrapolation_ratio=2.0, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=21)
    B, T, H, W, M = 1, 4, 48, 48, 32   # 4 x 24 x 24 = 2304 tokens = 36 tiles of 64 keys
    g = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(B, 16, T, H, W).to(torch.bfloat16)
    mask = torch.zeros(B, 1, T, H, W, dtype=torch.bfloat16)
    mask[:, :, :1] = 1
    pose = (0.5 * rnd(B, 64, T, H, W)).to(torch.bfloat16)
    ctx = (0.2 * rnd(B, M, 128)).to(torch.bfloat16)
    ts = torch.tensor([0.7], dtype=torch.bfloat16)
    pad = torch.zeros(B, 1, 8 * H, 8 * W, dtype=torch.bfloat16)
    kwargs = dict(x=x.to(dev), timesteps=ts.to(dev), crossattn_emb=ctx.to(dev), crossattn_mask=None, fps=torch.tensor([24.0], device=dev),
                  padding_mask=pad.to(dev), condition_video_indicator=mask[:, :, :, :1, :1].to(dev), condition_video_input_mask=mask.to(dev),
                  condition_video_pose=pose.to(dev))
    ops.set_option("attn_variant", 11)  # 9 x 2 workgroups do not fill the chip: the automatic choice here is the 8-wave kernel
    try:
        with pytest.MonkeyPatch.context() as mp:
            res = _forward_on_off(net, kwargs, mp)
    finally:
        ops.set_option("attn_variant", 0)
    assert res[True][1] == [NM, NM], res[True][1]
    assert res[False][1] == ["flash_attn_fwd_w4b_kernel<true>"] * 2, res[False][1]
    sd = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    y_ref = dit_oracle.dit_forward(sd, x.float(), ts.float(), ctx.float(), mask.float(), pose.float(), pad.float(), torch.tensor([24.0]),
                                   num_blocks=2, num_heads=2)
    for flag, (y, _names) in res.items():
        rel = float((y - y_ref).norm() / y_ref.norm())
        mx = float((y - y_ref).abs().max())
        print(f"[dit 2304 tokens bound={'on' if flag else 'off'}] vs oracle rel_l2={rel:.3e} max_abs={mx:.3e} ref_absmax={float(y_ref.abs().max()):.3e}")
        assert y.shape == y_ref.shape and torch.isfinite(y).all()
        assert rel <= 9e-3 and mx <= 1.0e-2 * float(y_ref.abs().max())  # tests/test_dit_gpu.py: test_dit_forward_long_sequence_vs_oracle
    d = float((res[True][0] - res[False][0]).norm() / res[False][0].norm())
    print(f"[dit 2304 tokens] bound on vs off rel_l2={d:.3e}")
    assert d <= 4.5e-3
