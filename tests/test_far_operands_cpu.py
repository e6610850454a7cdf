"""CPU: the far-operand harness itself (tests/far_operands.py) on a small arena with the thresholds scaled down (2^15 for 2^31, 2^16 for 2^32, a
margin of 64 for 4096, tiles of 8 rows for 256): the pitch arithmetic, the placement, the sliced check - and mutants, "kernels" restated in Python
with the defects the harness exists for, which the check must catch: a signed and a truncated 32-bit row offset on the read and on the write side,
the same relative to a tile's first row, and a write one element outside a payload."""
import pytest
import torch

from tests import far_operands as fo

bf16 = torch.bfloat16
TH = fo.Thresholds(t31=1 << 15, t32=1 << 16, margin=64)
TILE = 8
ARENA = TH.headroom + TH.t32 + (1 << 14)
SLICE = 10000  # no divisor of the arena: the last slice is ragged


def arena():
    return fo.Arena(ARENA, device="cpu", th=TH, slice_bytes=SLICE)


def data(rows, cols, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g).to(bf16)


# ---- the offset a kernel forms from a row index: right, and the two defects (scaled: "32 bits" are 16 here) ----
def exact(off):
    return off


def truncated(off):
    return off % TH.t32


def signed(off):
    off %= TH.t32
    return off - TH.t32 if off >= TH.t31 else off


def double_rows(a, src, dst, read=exact, write=exact, tile=None, stray=None):
    """out[r] = 2 in[r], addressing the arena's bytes as a kernel does: base + offset(r * pitch) - or, with tile, a 64-bit tile base plus
    offset((r % tile) * pitch). stray = (row, elements): one more element written that far behind the row's end."""
    R, Cc = src.view.shape
    ps, pd = src.view.stride(0) * 2, dst.view.stride(0) * 2
    words = a.buf.view(torch.int16)
    for r in range(R):
        t0, rr = ((r // tile) * tile, r % tile) if tile else (0, r)
        s = src.base + t0 * ps + read(rr * ps)
        d = dst.base + t0 * pd + write(rr * pd)
        assert 0 <= s and s + 2 * Cc <= a.buf.numel() and 0 <= d and d + 2 * Cc <= a.buf.numel(), "the harness's promise: a wrong offset stays inside the arena"
        row = words[s // 2:s // 2 + Cc].clone().view(bf16)
        words[d // 2:d // 2 + Cc] = (2 * row.float()).to(bf16).view(torch.int16)
        if stray and stray[0] == r:
            words[d // 2 + Cc - 1 + stray[1]] = 0x3F80


def test_pitches_are_the_smallest_multiples_of_16_that_do_the_job():
    for th in (TH, fo.REAL):
        for rows in (2, 3, 5, 7, 257, 1030):
            p31, p32 = fo.pitch_p31(rows, th), fo.pitch_p32(rows, th)
            assert p31 % 16 == 0 and th.t31 < (rows - 1) * p31 < th.t32 and (rows - 1) * (p31 - 16) <= th.t31
            assert p32 % 16 == 0 and (rows - 1) * p32 > th.t32 + th.margin and (rows - 1) * (p32 - 16) <= th.t32 + th.margin
        pt = fo.pitch_pt(257, th)
        assert pt % 16 == 0 and 255 * pt > th.t32 + th.margin and 255 * (pt - 16) <= th.t32 + th.margin
    assert fo.pitch_pt(TILE + 1, TH, TILE) == fo.pitch_beyond(TILE, TH.t32 + TH.margin)
    with pytest.raises(AssertionError):
        fo.pitch_p31(1, TH)
    with pytest.raises(AssertionError):
        fo.pitch_pt(256, TH)
    # the real arena holds the widest case: headroom, the compact operands of the largest GEMM case (< 512 MiB), the PT span of a 257-row operand
    assert fo.ARENA_BYTES <= 7 << 30 and fo.REAL.headroom + (1 << 29) + 256 * fo.pitch_pt(257) + 65536 <= fo.ARENA_BYTES
    assert fo.SLICE_BYTES <= 1 << 30


def test_placement_bases_alignment_headroom_and_views():
    a = arena()
    x = data(5, 24)
    v = a.place_rows("x", x, fo.pitch_p32(5, TH))
    w = a.place_rows("w", data(3, 8, 1))
    o = a.place_rows("o", (5, 24), role="out")
    q = a.place("q", (2, 3, 4, 8), (4096, 1024, 64, 4), torch.float32, torch.arange(192, dtype=torch.float32).reshape(2, 3, 4, 8))
    s = a.place_rows("s", torch.arange(21, dtype=torch.uint8).reshape(3, 7), 32)
    for p in a.payloads:
        assert p.base % 16 == 0 and p.base >= TH.headroom and p.last <= ARENA and p.view.data_ptr() == a.buf.data_ptr() + p.base
    assert [p.base >= q.last for p, q in zip(a.payloads[1:], a.payloads)] == [True] * 4  # one after the other, never interleaved
    assert v.stride(0) * 2 == fo.pitch_p32(5, TH) and a["x"].last - a["x"].base == 4 * fo.pitch_p32(5, TH) + 48
    assert torch.equal(v, x) and w.stride(0) * 2 == 32 and q.stride() == (1024, 256, 16, 1) and s.stride() == (32, 1)
    assert bool(torch.isnan(o.float()).all()) and torch.equal(o.view(torch.int16), torch.full((5, 24), fo.FILL16, dtype=torch.int16))
    assert torch.equal(a["q"].bytes.view(torch.float32).reshape(2, 3, 4, 8), q)
    with pytest.raises(AssertionError):
        a.place_rows("big", (9, 8), fo.pitch_p32(9, TH), role="out")  # behind the others it no longer fits
    with pytest.raises(AssertionError):
        a.place("overlap", (4, 8), (8, 2), bf16, data(4, 8))  # rows that share bytes
    o.copy_(x)
    out = a.check("placement")
    assert torch.equal(out["o"], x) and a.payloads == [] and a.scan() == (0, None)


@pytest.mark.parametrize("pitch", ["P31", "P32"])
@pytest.mark.parametrize("side", ["read", "write"])
def test_a_right_kernel_passes_and_both_offset_defects_are_caught(side, pitch):
    R, Cc = 5, 24
    x = data(R, Cc)
    far = fo.PITCHES[pitch](R, TH)
    wrong = {"P31": [signed], "P32": [signed, truncated]}[pitch]  # (a truncated offset is still the right one below 2^32)
    for offset in [exact, truncated, signed]:
        a = arena()
        a.place_rows("x", x, far if side == "read" else None)
        a.place_rows("o", (R, Cc), far if side == "write" else None, role="out")
        double_rows(a, a["x"], a["o"], **{side: offset})
        if offset in wrong:  # the read delivers the sentinel; the write leaves its row of the output unwritten
            with pytest.raises(AssertionError, match="elements of the output 'o' are not finite"):
                a.check(f"{side} {pitch} {offset.__name__}")
        else:
            out = a.check(f"{side} {pitch} {offset.__name__}")
            assert torch.equal(out["o"], (2 * x.float()).to(bf16))


def test_misdirected_write_is_seen_as_written_sentinel_even_where_the_output_is_complete():
    """the write of row R - 1 goes astray AND the row is then written correctly: the output is finite, only the scan can tell"""
    R, Cc = 5, 24
    a = arena()
    x = data(R, Cc)
    a.place_rows("x", x)
    a.place_rows("o", (R, Cc), fo.pitch_p32(R, TH), role="out")
    double_rows(a, a["x"], a["o"], write=truncated)
    double_rows(a, a["x"], a["o"])
    with pytest.raises(AssertionError, match=r"outside the payloads were written, the first at byte \d+: \d+ bytes behind the base of 'o', between its rows"):
        a.check("astray and repaired")
    assert a.scan() == (0, None) and a.payloads == []  # a failed check leaves a fresh arena


def test_tile_relative_offsets_need_the_tile_pitch():
    """A kernel with a 64-bit tile base and a truncated offset inside the tile is right at P32 of a 9-row operand (no row starts 2^16 behind its
    tile's first) and wrong at PT - the case P31 / P32 alone would miss."""
    R, Cc = TILE + 1, 16
    x = data(R, Cc)
    for name, pitch, caught in (("P32", fo.pitch_p32(R, TH), False), ("PT", fo.pitch_pt(R, TH, TILE), True)):
        a = arena()
        a.place_rows("x", x, pitch)
        a.place_rows("o", (R, Cc), role="out")
        double_rows(a, a["x"], a["o"], read=truncated, tile=TILE)
        if caught:
            with pytest.raises(AssertionError, match="not finite"):
                a.check(name)
        else:
            assert torch.equal(a.check(name)["o"], (2 * x.float()).to(bf16))


@pytest.mark.parametrize("stray", [(0, 1), (4, 1), (2, -24 - 1)], ids=["behind row 0", "behind the last row", "before row 2"])
def test_a_write_one_element_outside_a_payload_is_caught(stray):
    R, Cc = 5, 24
    a = arena()
    a.place_rows("x", data(R, Cc))
    a.place_rows("o", (R, Cc), role="out")
    double_rows(a, a["x"], a["o"], stray=stray)
    with pytest.raises(AssertionError, match="1 2-byte words outside the payloads"):
        a.check("stray write")


def test_a_changed_input_and_a_refused_call_that_writes_are_caught():
    R, Cc = 5, 24
    a = arena()
    x = a.place_rows("x", data(R, Cc), fo.pitch_p31(R, TH))
    o = a.place_rows("o", (R, Cc), role="out")
    o.copy_(x)
    x[3, 5] = 1.0
    with pytest.raises(AssertionError, match="1 bytes of the input 'x' were changed|2 bytes of the input 'x' were changed"):
        a.check("input written")
    a.reset()
    a.place_rows("x", data(R, Cc))
    o = a.place_rows("o", (R, Cc), role="out")
    a.assert_untouched("refused, nothing written")
    a.place_rows("x", data(R, Cc))
    o = a.place_rows("o", (R, Cc), role="out")
    o[1, 1] = 0.0
    with pytest.raises(AssertionError, match="a refused call wrote 1 2-byte words"):
        a.assert_untouched("refused, output written")


def test_in_place_payloads_may_change_and_come_back():
    a = arena()
    x = data(5, 24)
    v = a.place_rows("x", x, fo.pitch_p32(5, TH), role="inout")
    v.mul_(2)
    assert torch.equal(a.check("in place")["x"], (2 * x.float()).to(bf16))
