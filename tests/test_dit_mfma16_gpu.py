"""GPU: the DiT forward with dit._SELF_ATTN_MFMA16 on and off - the 2 304-token, 2-block net of tests/test_dit_bounded_gpu.py (the smallest DiT test shape
made of whole 64-key tiles), the one-wave-per-SIMD kernel selected. The flag decides between flash_attn_fwd_w4c_nm_kernel (16x16x32 MFMAs) and
flash_attn_fwd_w4b_nm_kernel<true>; the "auto" default keeps the kernel an explicit "attn_variant" option names.
Bars: those of that file. The two kernels round P to bf16 at the same point but sum in a different order, so their results are two independent
roundings of one function: the same 4.5e-3 rel-L2 that file allows between its two forms is asked here, and both forwards must clear the fp32
oracle's tolerance (rel-L2 9e-3, max-abs 1e-2 of the reference's largest value)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NM = "flash_attn_fwd_w4b_nm_kernel<true>"
W4C = "flash_attn_fwd_w4c_nm_kernel"


def test_dit_2304_tokens_mfma16_on_vs_off_and_oracle():
    from gen3c_amd import dit, ops
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
    res = {}
    ops.set_option("attn_variant", 11)  # 9 x 2 workgroups do not fill the chip: the automatic choice here is the 8-wave kernel
    try:
        with pytest.MonkeyPatch.context() as mp:
            for flag in (True, False, "auto"):
                mp.setattr(dit, "_SELF_ATTN_MFMA16", flag)
                ops.enable_kernel_timers(True)
                try:
                    y = net(**kwargs)
                    torch.cuda.synchronize()
                    names = [m["kernel"] for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd" and m["Skv"] == 2304 and m["Sq"] == 2304]
                finally:
                    ops.enable_kernel_timers(False)
                res[flag] = (y.float().cpu(), names)
    finally:
        ops.set_option("attn_variant", 0)
    assert res[True][1] == [W4C, W4C], res[True][1]
    assert res[False][1] == [NM, NM], res[False][1]
    assert res["auto"][1] == [NM, NM] and torch.equal(res["auto"][0], res[False][0])  # an explicit variant keeps the kernel it names
    sd = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    y_ref = dit_oracle.dit_forward(sd, x.float(), ts.float(), ctx.float(), mask.float(), pose.float(), pad.float(), torch.tensor([24.0]),
                                   num_blocks=2, num_heads=2)
    for flag in (True, False):
        y = res[flag][0]
        rel = float((y - y_ref).norm() / y_ref.norm())
        mx = float((y - y_ref).abs().max())
        print(f"[dit 2304 tokens mfma16={'on' if flag else 'off'}] vs oracle rel_l2={rel:.3e} max_abs={mx:.3e} ref_absmax={float(y_ref.abs().max()):.3e}")
        assert y.shape == y_ref.shape and torch.isfinite(y).all()
        assert rel <= 9e-3 and mx <= 1.0e-2 * float(y_ref.abs().max())
    d = float((res[True][0] - res[False][0]).norm() / res[False][0].norm())
    print(f"[dit 2304 tokens] mfma16 on vs off rel_l2={d:.3e}")
    assert d <= 4.5e-3
