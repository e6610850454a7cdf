"""GPU: the DiT's opt-in MXFP8 mode (VideoExtendGeneralDIT(linear_precision="mxfp8") / set_linear_precision, --dit_precision).

Bars, set by CPU emulation with the fp32 oracle first (this tiny 2-block net and these inputs; `python -m tests.test_mxfp8_dit_gpu` prints
them): fake-quantising the six block linears moves the oracle by 2.86e-3 rel-L2 (the mode's own quantisation error on this net), and rounding
those linears' inputs to bf16 before the quantisation, as the product does, moves the fake-quantised oracle by 1.44e-3. The product's bf16
arithmetic adds its own distance r_bf16, measured in the same test as the bf16 net against the plain oracle. With at most 1.5x margin:
  (a) against the fake-quantised oracle: rel-L2 <= 1.5 (r_bf16 + 1.44e-3);
  (b) against the plain fp32 oracle (the recorded quality bar): rel-L2 <= 1.5 (r_bf16 + 2.86e-3).
"""
import pytest
import torch

from tests._mxfp8_tiny_dit import _oracle  # the fake-quantised oracle, shared with tests/test_dit_shapes_gpu.py

pytestmark = pytest.mark.gpu

EMU_FLIPS, EMU_QUANT = 1.44e-3, 2.86e-3


def _net(dev, precision=None, seed=7):
    from gen3c_amd.dit import VideoExtendGeneralDIT
    kw = {} if precision is None else dict(linear_precision=precision)
    net = VideoExtendGeneralDIT(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=2, num_heads=2,
                                adaln_lora_dim=32, crossattn_emb_channels=128, rope_t_extrapolation_ratio=2.0, device=dev, init_weights=False, **kw)
    net.initialize_weights(randomize_adaln=True, seed=seed)
    return net


def _inputs():
    B, T, H, W, M = 1, 4, 16, 24, 32
    g = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(B, 16, T, H, W).to(torch.bfloat16)
    mask = torch.zeros(B, 1, T, H, W, dtype=torch.bfloat16)
    mask[:, :, :1] = 1
    pose = (0.5 * rnd(B, 64, T, H, W)).to(torch.bfloat16)
    ctx = (0.2 * rnd(B, M, 128)).to(torch.bfloat16)
    return dict(x=x, timesteps=torch.tensor([0.7], dtype=torch.bfloat16), crossattn_emb=ctx, fps=torch.tensor([24.0]),
                padding_mask=torch.zeros(B, 1, 8 * H, 8 * W, dtype=torch.bfloat16), condition_video_indicator=mask[:, :, :, :1, :1],
                condition_video_input_mask=mask, condition_video_pose=pose)


def _run(net, inp, dev):
    y = net(crossattn_mask=None, **{k: v.to(dev) for k, v in inp.items()})
    torch.cuda.synchronize()
    return y


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def test_tiny_dit_mxfp8_against_fake_quant_and_plain_oracle():
    dev = torch.device("cuda:0")
    inp = _inputs()
    net = _net(dev, "mxfp8")
    y = _run(net, inp, dev)
    y_bf = _run(_net(dev), inp, dev)
    sd = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    plain = _oracle(sd, inp)
    r_bf16 = _rel(y_bf, plain)
    r_fake = _rel(y, _oracle(sd, inp, fake=True))
    r_plain = _rel(y, plain)
    bar_fake, bar_plain = 1.5 * (r_bf16 + EMU_FLIPS), 1.5 * (r_bf16 + EMU_QUANT)
    print(f"[mxfp8 tiny DiT] bf16 net vs plain oracle {r_bf16:.3e}; mxfp8 net vs fake-quantised oracle {r_fake:.3e} (bar {bar_fake:.3e}), "
          f"vs plain fp32 oracle {r_plain:.3e} (bar {bar_plain:.3e})")
    assert torch.isfinite(y).all()
    assert r_fake <= bar_fake
    assert r_plain <= bar_plain


def test_bf16_default_unchanged_and_launches_no_mxfp8():
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs()
    calls = []
    real_q, real_g = ops.quant_mxfp8, ops.gemm_mxfp8_nt
    ops.quant_mxfp8 = lambda *a, **k: calls.append("quant") or real_q(*a, **k)
    ops.gemm_mxfp8_nt = lambda *a, **k: calls.append("gemm") or real_g(*a, **k)
    try:
        y0 = _run(_net(dev), inp, dev)
        y1 = _run(_net(dev, "bf16"), inp, dev)
        assert calls == [], "the bf16 mode called an MXFP8 op"
        net = _net(dev, "mxfp8")
        ym = _run(net, inp, dev)
        assert "gemm" in calls and "quant" in calls
        net.set_linear_precision("bf16")
        calls.clear()
        y2 = _run(net, inp, dev)
        assert calls == []
    finally:
        ops.quant_mxfp8, ops.gemm_mxfp8_nt = real_q, real_g
    assert torch.equal(y0, y1) and torch.equal(y0, y2), "bf16 output changed"
    assert not torch.equal(y0, ym)


@pytest.mark.parametrize("inference", [False, True])
def test_mxfp8_follows_in_place_weight_edits(inference):
    dev = torch.device("cuda:0")
    inp = _inputs()
    ctx = torch.inference_mode() if inference else torch.no_grad()
    with ctx:
        net = _net(dev, "mxfp8")
        y0 = _run(net, inp, dev)
        P = dict(net.named_parameters())
        for name in ("blocks.block0.blocks.2.block.layer1.weight", "blocks.block1.blocks.0.block.attn.to_v.0.weight"):
            P[name].mul_(-0.5)
        y1 = _run(net, inp, dev)
        fresh = _net(dev, "mxfp8")
        fresh.load_state_dict(net.state_dict())
        y2 = _run(fresh, inp, dev)
    assert not torch.equal(y0, y1), "the edit was not followed"
    assert torch.equal(y1, y2), "edited net differs from a net built with the edited weights"


def test_mxfp8_context_parallel_one_rank_matches_single_rank():
    """tools/cp_check.py with the MXFP8 linears on both sides: the CP step through a 1-rank RCCL group against the non-CP step, within the
    bf16 CP test's bar (rel-L2 < 5e-3, tests/test_cp_gpu.py)."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    from tests.test_cp_gpu import _free_port
    root = Path(__file__).resolve().parent.parent
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(root / "tools" / "cp_check.py")]
    env = dict(os.environ, G3_CP_CHECK_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0", G3_CP_CHECK_PRECISION="mxfp8")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(root), env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[cp_check] OK" in r.stdout


if __name__ == "__main__":  # the CPU emulation behind the bars above
    torch.manual_seed(0)
    net = _net("cpu")
    sd = {k: v.detach().float() for k, v in net.state_dict().items()}
    inp = _inputs()
    plain, fake, fake_bf = _oracle(sd, inp), _oracle(sd, inp, fake=True), _oracle(sd, inp, fake=True, bf16_inputs=True)
    print(f"fake-quantised oracle vs plain oracle rel-L2 {_rel(fake, plain):.3e}; bf16-input fake-quantised vs fake-quantised {_rel(fake_bf, fake):.3e}")
