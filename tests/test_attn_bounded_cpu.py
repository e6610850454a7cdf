"""CPU: host-side dispatch of the bounded self-attention entry (g3_self_attn_kernel_name; nothing launches) and the logit bound _pack() derives
from the q / k RMSNorm weights."""
import math

import torch

from gen3c_amd import _lib

NM = "flash_attn_fwd_w4b_nm_kernel<true>"
LOG2E = math.log2(math.e)


def _name(Sq, Skv, B, H, bound, variant=0):
    return _lib.load().g3_self_attn_kernel_name(Sq, Skv, B, H, float(bound), variant).decode()


def _plain(Sq, Skv, B, H, variant=0):
    return _lib.load().g3_flash_attn_kernel_name_ex(Sq, Skv, B, H, variant).decode()


def test_bounded_dispatch_table():
    lib = _lib.load()
    lib.g3_set_option(b"attn_variant", 0)
    unit = 128 / math.sqrt(128) * 1.03  # 11.65 natural units = 16.8 in the log2 domain
    assert abs(unit * LOG2E - 16.8) < 0.05
    # the benchmark's launch (and its batch-2 form): automatic choice 11 -> the no-max kernel
    assert _name(56320, 56320, 1, 32, unit) == NM
    assert _name(56320, 56320, 2, 32, unit) == NM
    assert _name(56320, 56320, 1, 32, unit, 11) == NM
    assert _name(320, 320, 1, 8, unit, 11) == NM
    # the bound's range: 0 < bound * log2(e) <= 60
    for bad in (0.0, -3.0, 60.01 / LOG2E, 1e9, float("nan"), float("inf")):
        assert _name(56320, 56320, 1, 32, bad) == "flash_attn_fwd_w4b_kernel<true>", bad
    assert _name(56320, 56320, 1, 32, 59.9 / LOG2E) == NM
    # every other kernel choice is g3_flash_attn_kernel_name_ex's: the 8-wave kernel (explicit, or chosen by the fill rule), ragged and short contexts,
    # the w4b form without the cross-barrier prefetch, the older kernels
    for (Sq, Skv, B, H, variant) in [(56320, 56320, 1, 32, 4), (28160, 56320, 1, 8, 0), (7040, 56320, 1, 8, 0), (56320, 56321, 1, 32, 0), (56320, 56321, 1, 32, 11),
                                     (56320, 512, 1, 32, 0), (56320, 56320, 1, 32, 10), (56320, 56320, 1, 32, 9), (56320, 56320, 1, 32, 3), (4096, 4096, 1, 8, 2)]:
        got = _name(Sq, Skv, B, H, unit, variant)
        assert got == _plain(Sq, Skv, B, H, variant) and got != NM, (Sq, Skv, B, H, variant, got)
    # the process-wide option resolves the same way
    lib.g3_set_option(b"attn_variant", 11)
    try:
        assert _name(7040, 56320, 1, 8, unit) == NM
        assert _name(7040, 56321, 1, 8, unit) == "flash_attn_fwd_w4_kernel<0>"
    finally:
        lib.g3_set_option(b"attn_variant", 0)


def test_plain_names_do_not_move():
    """What tests/test_dispatch_cpu.py asserts of the plain name function holds next to the new entry."""
    lib = _lib.load()
    lib.g3_set_option(b"attn_variant", 0)
    name = lambda *a: lib.g3_flash_attn_kernel_name(*a).decode()
    assert name(56320, 56320, 1, 32) == "flash_attn_fwd_w4b_kernel<true>"
    assert name(56320, 56320, 2, 32) == "flash_attn_fwd_w4b_kernel<true>"
    for sq in (28160, 14080, 7040):
        assert name(sq, 56320, 1, 8).startswith("flash_attn_fwd_v3_kernel<0")
    assert name(56320, 56321, 1, 32).startswith("flash_attn_fwd_v3_kernel<0")
    assert name(56320, 512, 1, 32).startswith("flash_attn_fwd_v3_kernel<1")
    assert _plain(56320, 56320, 1, 32, 11) == "flash_attn_fwd_w4b_kernel<true>"
    assert _plain(56320, 56320, 1, 32, 10) == "flash_attn_fwd_w4b_kernel<false>"


def test_pack_computes_the_logit_bound_per_block():
    from gen3c_amd import dit
    net = dit.VideoExtendGeneralDIT(max_img_h=16, max_img_w=16, max_frames=8, in_channels=81, model_channels=128, num_blocks=2, num_heads=1,
                                    adaln_lora_dim=8, crossattn_emb_channels=16, device="cpu", init_weights=True)
    P = dict(net.named_parameters())
    qn = [P[f"blocks.block{i}.blocks.0.block.attn.to_q.1.weight"] for i in range(2)]
    kn = [P[f"blocks.block{i}.blocks.0.block.attn.to_k.1.weight"] for i in range(2)]
    with torch.no_grad():
        qn[0].fill_(1.0); kn[0].fill_(1.0)
        qn[1].copy_(torch.linspace(-1.5, 0.75, 128)); kn[1].copy_(torch.linspace(0.25, 2.0, 128))
    blocks = net._pack()["blocks"]
    want = [128 * 1.0 * 1.0 / math.sqrt(128) * 1.03, 128 * 1.5 * 2.0 / math.sqrt(128) * 1.03]
    for blk, w in zip(blocks, want):
        assert isinstance(blk["fa_bound"], float) and abs(blk["fa_bound"] - w) <= 1e-5 * w, (blk["fa_bound"], w)  # (these weights are exact in bf16)
    assert _name(56320, 56320, 1, 32, blocks[0]["fa_bound"]) == NM and _name(56320, 56320, 1, 32, blocks[1]["fa_bound"]) == NM
    # a changed weight set is re-packed with its own bound; one beyond the kernel's range (max|w_q| max|w_k| above ~3.6) falls back by itself
    with torch.no_grad():
        qn[0].fill_(2.0); kn[0].fill_(2.0)
    b0 = net._pack()["blocks"][0]["fa_bound"]
    assert abs(b0 - 4 * want[0]) <= 1e-5 * 4 * want[0] and b0 * LOG2E > 60
    assert _name(56320, 56320, 1, 32, b0) == "flash_attn_fwd_w4b_kernel<true>"
