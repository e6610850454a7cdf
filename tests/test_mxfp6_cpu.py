"""CPU: the MXFP6 reference quantiser (tests/mxfp6_ref.py) pinned on hand cases, and the mxfp6 switch of the DiT and the command line."""
import pytest
import torch

from tests.mxfp6_ref import dequant_mxfp6, e2m3_encode, e2m3_values, fake_quant6, pack_e2m3, quant_mxfp6_codes, quant_mxfp6_ref, unpack_e2m3


def _block(vals):
    """One 32-wide block: the given values, then zeros."""
    row = torch.zeros(32, dtype=torch.float64)
    row[: len(vals)] = torch.tensor(vals, dtype=torch.float64)
    return row.reshape(1, 32)


def _values(codes, s):
    """fp64 values a (codes, scale bytes) pair stands for."""
    M, K = codes.shape
    return (e2m3_values()[codes.long()].reshape(M, K // 32, 32) * torch.pow(2.0, s.double() - 127).unsqueeze(-1)).reshape(M, K)


def test_value_table():
    v = e2m3_values()
    assert v[:9].tolist() == [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0]  # subnormals m/8, then the first normal
    assert v[31] == 7.5 and v[63] == -7.5 and v[24] == 4.0 and v[16] == 2.0 and v[15] == 1.875
    assert torch.isfinite(v).all()  # no Inf / NaN codes
    assert v[0x20] == 0 and torch.signbit(v[0x20])  # -0


def test_hand_cases_amax_8():
    codes, s = quant_mxfp6_codes(_block([7.5, 7.75, 8.0, 0.0625, 0.1875, 1.0625, -3.9, 5.25]))
    assert s.tolist() == [[128]]  # floor(log2 8) - 2 = 1
    assert _values(codes, s)[0, :8].tolist() == [7.5, 8.0, 8.0, 0.0, 0.25, 1.0, -4.0, 5.0]  # 5.25 / 2 = 2.625: tie between 2.5 and 2.75 -> even


def test_hand_cases_amax_below_8_saturates():
    codes, s = quant_mxfp6_codes(_block([7.9, 7.75, -7.9]))
    assert s.tolist() == [[127]]  # X = 0: the scaled amax lies in (7.5, 8)
    assert codes[0, :3].tolist() == [31, 31, 63]  # 7.75 is clamped to 7.5 before rounding: the tie never becomes 8
    assert _values(codes, s)[0, :3].tolist() == [7.5, 7.5, -7.5]


def test_all_64_codes_round_trip_and_negative_zero_policy():
    """decode then encode returns the code. -0 policy: the sign bit of the input is kept, so code 0x20 (-0) returns as 0x20, and a negative
    value that rounds to zero gives 0x20; only an all-zero BLOCK has all-zero codes whatever its signs."""
    c = torch.arange(64, dtype=torch.uint8)
    assert torch.equal(e2m3_encode(e2m3_values()), c)
    codes, s = quant_mxfp6_codes(_block([4.0, -0.01, -0.0, 0.01]))
    assert s.tolist() == [[127]] and codes[0, :4].tolist() == [24, 0x20, 0x20, 0]
    x = torch.zeros(1, 64, dtype=torch.float64)
    x[0, 3] = -0.0
    codes, s = quant_mxfp6_codes(x)
    assert s.tolist() == [[127, 127]] and codes.tolist() == [[0] * 64]


def test_every_midpoint_rounds_to_even():
    v = e2m3_values()[:32]  # the non-negative values, ascending with the code
    mid = (v[:-1] + v[1:]) / 2
    want = torch.where(torch.arange(31) % 2 == 0, torch.arange(31), torch.arange(1, 32)).to(torch.uint8)
    assert torch.equal(e2m3_encode(mid), want)
    assert torch.equal(e2m3_encode(-mid), want | 0x20)
    eps = 2.0 ** -20
    assert torch.equal(e2m3_encode(mid - eps), torch.arange(31, dtype=torch.uint8))
    assert torch.equal(e2m3_encode(mid + eps), torch.arange(1, 32, dtype=torch.uint8))


def test_subnormal_block_and_huge_block():
    codes, s = quant_mxfp6_codes(torch.full((1, 32), 2.0 ** -133, dtype=torch.float64))
    assert s.tolist() == [[0]] and codes.tolist() == [[0] * 32]  # X clamps to -127; 2^-133 / 2^-127 = 2^-6 rounds to 0
    codes, s = quant_mxfp6_codes(_block([-(2.0 ** 120), 2.0 ** 118, 2.0 ** 100]))
    assert s.tolist() == [[127 + 118]] and codes[0, :3].tolist() == [0x20 | 24, 8, 0]


def test_pack_bit_positions_and_round_trip():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 64, (5, 96), generator=g).to(torch.uint8)
    q = pack_e2m3(codes)
    assert q.shape == (5, 72) and q.dtype == torch.uint8
    assert torch.equal(unpack_e2m3(q), codes)
    for blk in range(3):  # elements 0, 1, 5 and 31 of every 24-byte block, by hand from the 192-bit little-endian string
        for row in range(5):
            big = int.from_bytes(bytes(q[row, 24 * blk: 24 * blk + 24].tolist()), "little")
            for i in (0, 1, 5, 31):
                assert (big >> (6 * i)) & 0x3F == int(codes[row, 32 * blk + i]), (row, blk, i)
    one = torch.zeros(1, 32, dtype=torch.uint8)
    one[0, 1], one[0, 5], one[0, 31] = 0x3F, 0x21, 0x3F
    p = pack_e2m3(one)[0].tolist()
    assert p[0] == 0xC0 and p[1] == 0x0F  # element 1: bits 6..11
    assert p[3] == 0x40 and p[4] == 0x08  # element 5 = 0b100001 at bits 30..35: bit 30 (byte 3 bit 6) and bit 35 (byte 4 bit 3)
    assert p[23] == 0xFC and p[22] == 0  # element 31: bits 186..191


def test_dequant_is_exact_in_bf16_and_close():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(16, 256, generator=g) * 0.02).to(torch.bfloat16)
    q, s = quant_mxfp6_ref(x)
    assert q.shape == (16, 192) and s.shape == (16, 8)
    d = dequant_mxfp6(q, s)
    assert torch.equal(d, d.to(torch.bfloat16).float())
    rel = float((d - x.float()).norm() / x.float().norm())
    assert rel < 0.04  # 3 mantissa bits, as e4m3
    assert torch.equal(fake_quant6(x.float()), d)


def test_dit_precision_flag_parses_mxfp6():
    import argparse
    from gen3c_amd.cli_common import add_common_args
    ap = add_common_args(argparse.ArgumentParser())
    assert ap.parse_args(["--dit_precision", "mxfp6"]).dit_precision == "mxfp6"
    assert ap.parse_args(["--dit_precision", "mxfp6", "--dit_mxfp8_producers", "fused"]).dit_mxfp8_producers == "fused"
    with pytest.raises(SystemExit):
        ap.parse_args(["--dit_precision", "fp6"])


def test_dit_linear_precision_mxfp6_switch_drops_packed_set():
    from gen3c_amd.dit import LINEAR_PRECISIONS, VideoExtendGeneralDIT
    assert LINEAR_PRECISIONS == ("bf16", "mxfp8", "mxfp6")
    kw = dict(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=1, num_heads=2, adaln_lora_dim=32,
              crossattn_emb_channels=128, device="cpu", init_weights=False)
    net = VideoExtendGeneralDIT(**kw)
    net.set_linear_precision("mxfp6")
    assert net.linear_precision == "mxfp6"
    assert VideoExtendGeneralDIT(linear_precision="mxfp6", **kw).linear_precision == "mxfp6"
    with pytest.raises(ValueError):
        net.set_linear_precision("fp6")
    for a, b in (("mxfp6", "mxfp8"), ("mxfp8", "mxfp6"), ("mxfp6", "bf16")):
        net.set_linear_precision(a)
        net._packed = "stale"
        net.set_linear_precision(b)
        assert net._packed is None, f"{a} -> {b} kept the packed weights"
    net.set_linear_precision("mxfp6")
    net.set_mxfp8_producers("fused")  # accepted and inert under mxfp6
    assert net.mxfp8_producers == "fused"
