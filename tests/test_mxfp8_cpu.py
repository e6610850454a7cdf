"""CPU: the MXFP8 reference quantiser (tests/mxfp8_ref.py) pinned on hand cases and against a brute-force nearest-value search."""
import math

import pytest
import torch

from tests.mxfp8_ref import dequant_mxfp8, fake_quant, quant_mxfp8_ref


def _e4m3_table():
    """(code, value) of every finite e4m3fn code."""
    out = []
    for code in range(256):
        if code & 0x7F == 0x7F:
            continue  # NaN
        s = -1.0 if code & 0x80 else 1.0
        e, m = (code >> 3) & 0xF, code & 7
        v = s * (m / 8.0) * 2.0 ** -6 if e == 0 else s * (1 + m / 8.0) * 2.0 ** (e - 7)
        out.append((code, v))
    return out


_TABLE = _e4m3_table()


def _brute_code(y: float) -> int:
    """RNE to e4m3fn by search: nearest finite value, ties to the even code; the sign of y is kept for zero."""
    best = min(abs(v - y) for _, v in _TABLE)
    cands = [(c, v) for c, v in _TABLE if abs(v - y) == best]
    if len(cands) > 1:
        even = [(c, v) for c, v in cands if c & 1 == 0]
        cands = even or cands
        if len({v for _, v in cands}) == 1 and cands[0][1] == 0.0:  # +0 / -0
            return 0x80 if math.copysign(1.0, y) < 0 else 0x00
    return cands[0][0]


def _block(vals):
    """One 32-wide block: the given values, then zeros."""
    row = torch.zeros(32, dtype=torch.float32)
    row[: len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return row


def _codes(q):
    return q.view(torch.uint8).tolist()


def test_powers_of_two():
    q, s = quant_mxfp8_ref(_block([1.0, 0.5, 2.0 ** -9, 0.25]).reshape(1, 32))
    assert s.tolist() == [[127 - 8]]  # amax 1 -> X = -8
    assert _codes(q)[0][:4] == [0x78, 0x70, 0x30, 0x68]  # 256, 128, 2^-1, 64


def test_block_amax_between_448_and_512_clamps():
    q, s = quant_mxfp8_ref(_block([480.0, -464.0, 256.0]).reshape(1, 32))
    assert s.tolist() == [[127]]  # floor(log2 480) = 8 -> X = 0
    assert _codes(q)[0][:3] == [0x7E, 0xFE, 0x78]  # +-448 (clamped, not NaN), 256
    q, s = quant_mxfp8_ref(_block([1.875]).reshape(1, 32))  # 1.875 * 2^8 = 480
    assert s.tolist() == [[119]] and _codes(q)[0][0] == 0x7E


def test_subnormals():
    q, s = quant_mxfp8_ref(_block([256.0, 2.0 ** -8, 3 * 2.0 ** -10, 2.0 ** -10, -(2.0 ** -9), 7 * 2.0 ** -9]).reshape(1, 32))
    assert s.tolist() == [[127]]
    assert _codes(q)[0][:6] == [0x78, 0x02, 0x02, 0x00, 0x81, 0x07]


def test_rne_ties():
    # X = 0: 1.0625 lies halfway between 1.0 (0x38) and 1.125 (0x39) -> even; 1.1875 between 1.125 and 1.25 (0x3A) -> even
    q, _ = quant_mxfp8_ref(_block([256.0, 1.0625, 1.1875, 272.0, 304.0]).reshape(1, 32))
    assert _codes(q)[0][:5] == [0x78, 0x38, 0x3A, 0x78, 0x7A]  # 272: 256 | 288 -> 256; 304: 288 | 320 -> 320


def test_all_zero_block_and_negative_zero():
    x = torch.zeros(2, 64)
    x[0, 5] = -0.0
    x[1, 40] = -3.0
    q, s = quant_mxfp8_ref(x)
    assert s.tolist() == [[127, 127], [127, 127 - 7]]
    codes = _codes(q)
    assert codes[0] == [0] * 64 and codes[1][:32] == [0] * 32
    assert codes[1][40] == 0xFC  # -3 * 2^7 = -384 = -1.5 * 2^8


def test_negative_values():
    q, s = quant_mxfp8_ref(_block([-256.0, -1.0, 300.0]).reshape(1, 32))
    assert _codes(q)[0][:3] == [0xF8, 0xB8, 0x79]


@pytest.mark.parametrize("seed", [0, 1])
def test_matches_brute_force_search(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(8, 128, generator=g) * torch.exp2(torch.randint(-12, 12, (8, 1), generator=g).float())
    x[2, :32] = 0.0
    x[3, 7] = 5000.0  # outlier: most of its block goes subnormal / zero
    x = x.to(torch.bfloat16)
    q, s = quant_mxfp8_ref(x)
    codes = _codes(q)
    for m in range(8):
        for b in range(4):
            X = int(s[m, b]) - 127
            blk = x[m, 32 * b: 32 * b + 32].double()
            amax = float(blk.abs().max())
            if amax == 0:
                assert X == 0 and codes[m][32 * b: 32 * b + 32] == [0] * 32
                continue
            assert X == max(-127, min(127, math.floor(math.log2(amax)) - 8))
            for k in range(32):
                y = max(-448.0, min(448.0, float(blk[k]) / 2.0 ** X))
                assert codes[m][32 * b + k] == _brute_code(y), (m, b, k, float(blk[k]), X)


def test_dequant_is_exact_in_bf16_and_close():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(16, 256, generator=g) * 0.02).to(torch.bfloat16)
    q, s = quant_mxfp8_ref(x)
    d = dequant_mxfp8(q, s)
    assert torch.equal(d, d.to(torch.bfloat16).float())
    rel = float((d - x.float()).norm() / x.float().norm())
    assert rel < 0.04  # e4m3: 3 mantissa bits
    assert torch.equal(fake_quant(x.float()), d)


def test_dit_precision_flag_parses():
    import argparse
    from gen3c_amd.cli_common import add_common_args
    ap = add_common_args(argparse.ArgumentParser())
    assert ap.parse_args([]).dit_precision == "bf16"
    assert ap.parse_args(["--dit_precision", "mxfp8"]).dit_precision == "mxfp8"
    with pytest.raises(SystemExit):
        ap.parse_args(["--dit_precision", "fp4"])


def test_dit_linear_precision_switch():
    from gen3c_amd.dit import VideoExtendGeneralDIT
    kw = dict(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=1, num_heads=2, adaln_lora_dim=32,
              crossattn_emb_channels=128, device="cpu", init_weights=False)
    net = VideoExtendGeneralDIT(**kw)
    assert net.linear_precision == "bf16"
    net.set_linear_precision("mxfp8")
    assert net.linear_precision == "mxfp8"
    assert VideoExtendGeneralDIT(linear_precision="mxfp8", **kw).linear_precision == "mxfp8"
    with pytest.raises(ValueError):
        net.set_linear_precision("fp8")
    with pytest.raises(ValueError):
        VideoExtendGeneralDIT(linear_precision="int8", **kw)
