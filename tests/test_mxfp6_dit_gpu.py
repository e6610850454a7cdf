"""GPU: the DiT's opt-in MXFP6 mode (VideoExtendGeneralDIT(linear_precision="mxfp6") / set_linear_precision, --dit_precision mxfp6).

Bars, set by CPU emulation with the fp32 oracle first (the tiny 2-block net and inputs of tests/_mxfp8_tiny_dit.py; `python -m
tests.test_mxfp6_dit_gpu` prints them): fake-quantising the six block linears to MXFP6 e2m3 moves the oracle by 2.81e-3 rel-L2 (the mode's own
quantisation error on this net), and rounding those linears' inputs to bf16 before the quantisation, as the product does, moves the
fake-quantised oracle by 1.56e-3. The product's bf16 arithmetic adds its own distance r_bf16, measured in the same test as the bf16 net against
the plain oracle. With at most 1.5x margin:
  (a) against the MXFP6-fake-quantised oracle: rel-L2 <= 1.5 (r_bf16 + 1.56e-3);
  (b) against the plain fp32 oracle: rel-L2 <= 1.5 (r_bf16 + 2.81e-3).
"""
import contextlib

import pytest
import torch

from tests import _mxfp8_tiny_dit as tiny
from tests._mxfp8_tiny_dit import _inputs, _net, _run
from tests.mxfp6_ref import fake_quant6

pytestmark = pytest.mark.gpu

EMU_FLIPS, EMU_QUANT = 1.56e-3, 2.81e-3
MX6_OPS = ("quant_mxfp6", "gemm_mxfp6_nt")
MX8_PRODUCER_OPS = ("layernorm_modulate_mxfp8", "posemb_layernorm_modulate_mxfp8", "_gemm_mxfp8_nt_mxout")


def _oracle6(sd, inp, fake=False, bf16_inputs=False):
    """tests/_mxfp8_tiny_dit._oracle with its fake-quantiser swapped for the MXFP6 one (the file itself is left alone)."""
    saved = tiny.fake_quant
    tiny.fake_quant = fake_quant6
    try:
        return tiny._oracle(sd, inp, fake=fake, bf16_inputs=bf16_inputs)
    finally:
        tiny.fake_quant = saved


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


@contextlib.contextmanager
def _counted(names):
    """Count the calls of the named gen3c_amd.ops functions."""
    from gen3c_amd import ops
    calls, real = [], {n: getattr(ops, n) for n in names}
    for n in names:
        setattr(ops, n, (lambda n_: lambda *a, **k: calls.append(n_) or real[n_](*a, **k))(n))
    try:
        yield calls
    finally:
        for n in names:
            setattr(ops, n, real[n])


def test_tiny_dit_mxfp6_against_fake_quant_and_plain_oracle():
    dev = torch.device("cuda:0")
    inp = _inputs()
    net = _net(dev, "mxfp6")
    y = _run(net, inp, dev)
    y_bf = _run(_net(dev), inp, dev)
    sd = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    plain = _oracle6(sd, inp)
    r_bf16 = _rel(y_bf, plain)
    r_fake = _rel(y, _oracle6(sd, inp, fake=True))
    r_plain = _rel(y, plain)
    bar_fake, bar_plain = 1.5 * (r_bf16 + EMU_FLIPS), 1.5 * (r_bf16 + EMU_QUANT)
    print(f"[mxfp6 tiny DiT] bf16 net vs plain oracle {r_bf16:.3e}; mxfp6 net vs fake-quantised oracle {r_fake:.3e} (bar {bar_fake:.3e}), "
          f"vs plain fp32 oracle {r_plain:.3e} (bar {bar_plain:.3e})")
    assert torch.isfinite(y).all()
    assert r_fake <= bar_fake
    assert r_plain <= bar_plain


def test_modes_do_not_leak():
    dev = torch.device("cuda:0")
    inp = _inputs()
    with _counted(MX6_OPS) as calls:
        y_default = _run(_net(dev), inp, dev)
        y_bf = _run(_net(dev, "bf16"), inp, dev)
        assert calls == [], "the bf16 mode called an MXFP6 op"
        y_8 = _run(_net(dev, "mxfp8"), inp, dev)
        assert calls == [], "the mxfp8 mode called an MXFP6 op"
        y_6 = _run(_net(dev, "mxfp6"), inp, dev)
        assert set(calls) == set(MX6_OPS)
    assert torch.equal(y_default, y_bf), "bf16 output differs from a default net's"
    assert not torch.equal(y_6, y_bf) and not torch.equal(y_6, y_8)
    fresh = {"bf16": y_bf, "mxfp6": y_6, "mxfp8": y_8}
    net = _net(dev)
    for precision in ("bf16", "mxfp6", "mxfp8", "bf16"):
        net.set_linear_precision(precision)
        assert torch.equal(_run(net, inp, dev), fresh[precision]), f"after switching to {precision}: differs from a fresh {precision} net"


def test_mxfp8_producers_setting_is_inert_under_mxfp6():
    dev = torch.device("cuda:0")
    inp = _inputs()
    y_sep = _run(_net(dev, "mxfp6", producers="separate"), inp, dev)
    with _counted(MX8_PRODUCER_OPS + ("quant_mxfp8", "gemm_mxfp8_nt")) as calls:
        y_fused = _run(_net(dev, "mxfp6", producers="fused"), inp, dev)
    assert calls == [], f"mxfp6 with fused producers called {sorted(set(calls))}"
    assert torch.equal(y_sep, y_fused)


@pytest.mark.parametrize("inference", [False, True])
def test_mxfp6_follows_in_place_weight_edits(inference):
    dev = torch.device("cuda:0")
    inp = _inputs()
    ctx = torch.inference_mode() if inference else torch.no_grad()
    with ctx:
        net = _net(dev, "mxfp6")
        y0 = _run(net, inp, dev)
        P = dict(net.named_parameters())
        for name in ("blocks.block0.blocks.2.block.layer1.weight", "blocks.block1.blocks.0.block.attn.to_v.0.weight"):
            P[name].mul_(-0.5)
        y1 = _run(net, inp, dev)
        fresh = _net(dev, "mxfp6")
        fresh.load_state_dict(net.state_dict())
        y2 = _run(fresh, inp, dev)
    assert not torch.equal(y0, y1), "the edit was not followed"
    assert torch.equal(y1, y2), "edited net differs from a net built with the edited weights"


@pytest.mark.parametrize("shape", [dict(B=2), dict(B=2, T=3, H=10, W=14)], ids=["B2", "B2-ragged"])
def test_mxfp6_batch_two_and_ragged_shape(shape):
    """B = 2 and a ragged token count against the MXFP6-fake-quantised oracle, with bar (a) of the first test."""
    dev = torch.device("cuda:0")
    inp = _inputs(**shape)
    inp["timesteps"] = torch.tensor([0.7, 0.2], dtype=torch.bfloat16)  # one per batch item, as tests/test_dit_shapes_gpu.py
    net = _net(dev, "mxfp6")
    y = _run(net, inp, dev)
    y_bf = _run(_net(dev), inp, dev)
    sd = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    r_bf16 = _rel(y_bf, _oracle6(sd, inp))
    r_fake = _rel(y, _oracle6(sd, inp, fake=True))
    print(f"[mxfp6 tiny DiT {shape}] bf16 net vs plain oracle {r_bf16:.3e}; mxfp6 net vs fake-quantised oracle {r_fake:.3e}")
    assert torch.isfinite(y).all()
    assert r_fake <= 1.5 * (r_bf16 + EMU_FLIPS)


def test_mxfp6_context_parallel_one_rank_matches_single_rank():
    """tools/cp_check.py with the MXFP6 linears on both sides: the CP step through a 1-rank RCCL group against the non-CP step, within the
    bf16 CP test's bar (rel-L2 < 5e-3, tests/test_cp_gpu.py)."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    from tests.test_cp_gpu import _free_port
    root = Path(__file__).resolve().parent.parent
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(root / "tools" / "cp_check.py")]
    env = dict(os.environ, G3_CP_CHECK_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0", G3_CP_CHECK_PRECISION="mxfp6")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(root), env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[cp_check] OK" in r.stdout


if __name__ == "__main__":  # the CPU emulation behind the bars above
    torch.manual_seed(0)
    net = _net("cpu")
    sd = {k: v.detach().float() for k, v in net.state_dict().items()}
    inp = _inputs()
    plain, fake, fake_bf = _oracle6(sd, inp), _oracle6(sd, inp, fake=True), _oracle6(sd, inp, fake=True, bf16_inputs=True)
    print(f"MXFP6 fake-quantised oracle vs plain oracle rel-L2 {_rel(fake, plain):.3e}; bf16-input fake-quantised vs fake-quantised {_rel(fake_bf, fake):.3e}")
