"""CPU: the mxfp8_producers switch ("separate" | "fused") of the DiT and its command-line flag. The kernels behind "fused" are pinned on the GPU
by tests/test_mxfp8_producers_gpu.py."""
import argparse

import pytest

KW = dict(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=1, num_heads=2, adaln_lora_dim=32,
          crossattn_emb_channels=128, device="cpu", init_weights=False)


def test_dit_mxfp8_producers_flag_parses():
    from gen3c_amd.cli_common import add_common_args
    ap = add_common_args(argparse.ArgumentParser())
    assert ap.parse_args([]).dit_mxfp8_producers == "separate"
    assert ap.parse_args(["--dit_mxfp8_producers", "fused"]).dit_mxfp8_producers == "fused"
    args = ap.parse_args(["--dit_precision", "mxfp8", "--dit_mxfp8_producers", "fused"])
    assert (args.dit_precision, args.dit_mxfp8_producers) == ("mxfp8", "fused")
    with pytest.raises(SystemExit):
        ap.parse_args(["--dit_mxfp8_producers", "inline"])


def test_constructor_and_setter_validation():
    from gen3c_amd.dit import MXFP8_PRODUCERS, VideoExtendGeneralDIT
    assert MXFP8_PRODUCERS == ("separate", "fused")
    net = VideoExtendGeneralDIT(**KW)
    assert net.mxfp8_producers == "separate"
    net.set_mxfp8_producers("fused")
    assert net.mxfp8_producers == "fused"
    net.set_mxfp8_producers("separate")
    assert net.mxfp8_producers == "separate"
    assert VideoExtendGeneralDIT(linear_precision="mxfp8", mxfp8_producers="fused", **KW).mxfp8_producers == "fused"
    for bad in ("Fused", "", "epilogue", None):
        with pytest.raises(ValueError):
            net.set_mxfp8_producers(bad)
        assert net.mxfp8_producers == "separate", "a refused value must leave the setting alone"
    with pytest.raises(ValueError):
        VideoExtendGeneralDIT(mxfp8_producers="both", **KW)


def test_setter_keeps_the_packed_weights():
    from gen3c_amd.dit import VideoExtendGeneralDIT
    net = VideoExtendGeneralDIT(linear_precision="mxfp8", **KW)
    sentinel = net._packed = dict(marker=True)  # stands in for a packed weight set (packing itself quantises on the GPU)
    net.set_mxfp8_producers("fused")
    assert net._packed is sentinel
    net.set_mxfp8_producers("separate")
    assert net._packed is sentinel
    net.set_linear_precision("bf16")  # the precision, by contrast, is part of the packed set
    assert net._packed is None


def test_bf16_with_fused_producers_constructs():
    from gen3c_amd.dit import VideoExtendGeneralDIT
    net = VideoExtendGeneralDIT(linear_precision="bf16", mxfp8_producers="fused", **KW)
    assert (net.linear_precision, net.mxfp8_producers) == ("bf16", "fused")
    assert net._packed is None


def test_new_entry_points_are_bound():
    from gen3c_amd import _lib, ops
    for name in ("g3_layernorm_modulate_mxfp8", "g3_posemb_layernorm_modulate_mxfp8", "g3_gemm_mxfp8_nt_mxout", "g3_gemm_mxfp8_mxout_kernel_name"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["g3_layernorm_modulate_mxfp8"]) == len(_lib.SIGNATURES["g3_layernorm_modulate_bf16"]) + 2
    assert len(_lib.SIGNATURES["g3_posemb_layernorm_modulate_mxfp8"]) == len(_lib.SIGNATURES["g3_posemb_layernorm_modulate_bf16"]) + 2
    for fn in ("layernorm_modulate_mxfp8", "posemb_layernorm_modulate_mxfp8"):
        assert callable(getattr(ops, fn))
