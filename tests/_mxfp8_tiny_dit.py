"""The tiny 2-block DiT and inputs of tests/test_mxfp8_dit_gpu.py, re-stated with the mxfp8_producers keyword, a batch size and a shape, and that
test's fake-quantised fp32 oracle: shared by tests/test_mxfp8_dit_gpu.py, tests/test_mxfp8_producers_gpu.py and its context-parallel worker process
(tests/_cp_producers_worker.py), and tests/test_dit_shapes_gpu.py."""
import types

import torch
import torch.nn.functional as F

from tests.mxfp8_ref import fake_quant

MX_KEYS = ("0.block.attn.to_q.0.weight", "0.block.attn.to_k.0.weight", "0.block.attn.to_v.0.weight", "0.block.attn.to_out.0.weight",
           "1.block.attn.to_q.0.weight", "1.block.attn.to_out.0.weight", "2.block.layer1.weight", "2.block.layer2.weight")


def _net(dev, precision=None, seed=7, producers=None):
    from gen3c_amd.dit import VideoExtendGeneralDIT
    kw = {} if precision is None else dict(linear_precision=precision)
    if producers is not None:
        kw["mxfp8_producers"] = producers
    net = VideoExtendGeneralDIT(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=2, num_heads=2,
                                adaln_lora_dim=32, crossattn_emb_channels=128, rope_t_extrapolation_ratio=2.0, device=dev, init_weights=False, **kw)
    net.initialize_weights(randomize_adaln=True, seed=seed)
    return net


def _inputs(B=1, T=4, H=16, W=24, M=32):
    g = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(B, 16, T, H, W).to(torch.bfloat16)
    mask = torch.zeros(B, 1, T, H, W, dtype=torch.bfloat16)
    mask[:, :, :1] = 1
    pose = (0.5 * rnd(B, 64, T, H, W)).to(torch.bfloat16)
    if B > 1:
        pose[1:] = 0  # the uncond half of a cond + uncond batch
    ctx = (0.2 * rnd(B, M, 128)).to(torch.bfloat16)
    return dict(x=x, timesteps=torch.tensor([0.7], dtype=torch.bfloat16), crossattn_emb=ctx, fps=torch.tensor([24.0]),
                padding_mask=torch.zeros(B, 1, 8 * H, 8 * W, dtype=torch.bfloat16), condition_video_indicator=mask[:, :, :, :1, :1],
                condition_video_input_mask=mask, condition_video_pose=pose)


def _run(net, inp, dev):
    y = net(crossattn_mask=None, **{k: v.to(dev) for k, v in inp.items()})
    torch.cuda.synchronize()
    return y


def _oracle(sd, inp, fake=False, bf16_inputs=False):
    """fp32 oracle; fake=True: the six block linears see MXFP8 fake-quantised inputs and weights (oracle/ untouched: its F is swapped here)."""
    from oracle import dit_oracle
    ids = {id(v) for k, v in sd.items() if k.startswith("blocks.") and k.split(".blocks.", 1)[-1] in MX_KEYS}

    def linear(x, w, b=None):
        if id(w) in ids:
            xin = x.to(torch.bfloat16).float() if bf16_inputs else x
            return F.linear(fake_quant(xin), fake_quant(w), b)
        return F.linear(x, w, b)

    saved = dit_oracle.F
    if fake:
        dit_oracle.F = types.SimpleNamespace(**{n: getattr(F, n) for n in dir(F) if not n.startswith("__")})
        dit_oracle.F.linear = linear
    try:
        f = lambda t: t.float()
        return dit_oracle.dit_forward(sd, f(inp["x"]), f(inp["timesteps"]), f(inp["crossattn_emb"]), f(inp["condition_video_input_mask"]),
                                      f(inp["condition_video_pose"]), f(inp["padding_mask"]), inp["fps"], num_blocks=2, num_heads=2)
    finally:
        dit_oracle.F = saved
