"""Operands that lie FAR from each other inside one allocation (TEST INFRASTRUCTURE - a plain helper module, like tests/guarded.py).

The hot kernels address their operands with hand-built 32-bit byte offsets from a base pointer. Every other kernel-level test hands them operands
whose last byte lies a few MiB behind the base, so a signed 32-bit product (wrong from 2^31 on) or a truncated one (wrong from 2^32 on) never shows.
Here a small operand is spread over gigabytes: an as_strided view, one per operand, of one raw byte arena at a chosen byte pitch.

Why one arena with headroom. Let an operand's base sit H >= 2^31 bytes behind the arena's start and let the arena reach the operand's last byte. A
kernel that should touch base + off with 0 <= off < 2^32 + small and gets the offset wrong in one of the two ways under test touches instead
    base + off - 2^32                  (truncated to 32 bits: off >= 2^32, so this is >= base), or
    base + off - 2^32 >= base - 2^31   (read as signed: 2^31 <= off < 2^32),
and both addresses lie INSIDE THE SAME ALLOCATION: at or after arena start (base - 2^31 >= start) and before the operand's last byte. The whole
arena is filled with the bf16 NaN pattern 0x7FC0 (what tests/guarded.py uses; as fp32 0x7FC07FC0 is a NaN too), so a misdirected read delivers NaN
into an output that must be finite, and a misdirected write lands on sentinel bytes that must come back untouched - a defect of this class shows as
a failed assertion, never as an access outside the allocation.

Pitches (each the smallest multiple of 16 bytes that does the job; Thresholds scales them down for the CPU test of this module):
    P31  row R - 1 starts in (2^31, 2^32): a signed product is wrong, an unsigned one still right
    P32  row R - 1 starts beyond 2^32 + 4096: a 32-bit product of the row index is wrong
    PT   row 255 starts beyond 2^32 + 4096, with 257 rows (264 for a GEMM's W: N % 8 == 0): for kernels that form 32-bit offsets from a TILE's first row (256-row tiles)

check(): every input payload bit for bit unchanged; every output payload finite; then the payloads are blanked and the WHOLE arena is compared
with the fill, in slices (nothing near the arena's size is allocated besides it) - which also leaves the arena refilled for the next case."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import torch

FILL16 = 0x7FC0  # bf16 NaN, the pattern of torch.full(..., nan, dtype=bfloat16); little endian: bytes C0 7F
ALIGN = 16
TILE_ROWS = 256


@dataclass(frozen=True)
class Thresholds:
    t31: int = 1 << 31     # where a signed 32-bit byte offset goes wrong
    t32: int = 1 << 32     # where a truncated one does
    margin: int = 4096     # "beyond 2^32" means beyond 2^32 + margin: a whole row (and then some) on the far side

    @property
    def headroom(self) -> int:
        return self.t31


REAL = Thresholds()
ARENA_BYTES = REAL.headroom + REAL.t32 + (3 << 28)  # 6.75 GiB (<= 7 GiB): headroom + the PT span (4 GiB + 17 MiB) + the compact operands
SLICE_BYTES = 1 << 28


def _up(x: int, m: int = ALIGN) -> int:
    return -(-x // m) * m


def pitch_beyond(rows: int, start_beyond: int) -> int:
    """smallest multiple of 16 with (rows - 1) * pitch > start_beyond"""
    assert rows >= 2, "a one-row operand has no pitch to be far by"
    return _up(start_beyond // (rows - 1) + 1)


def pitch_p31(rows: int, th: Thresholds = REAL) -> int:
    p = pitch_beyond(rows, th.t31)
    assert th.t31 < (rows - 1) * p < th.t32, (rows, p)
    return p


def pitch_p32(rows: int, th: Thresholds = REAL) -> int:
    return pitch_beyond(rows, th.t32 + th.margin)


def pitch_pt(rows: int, th: Thresholds = REAL, tile_rows: int = TILE_ROWS) -> int:
    assert rows > tile_rows, "PT needs a full tile and at least one row of the next (257 rows; a few more where the row count must be a multiple of 8)"
    return pitch_beyond(tile_rows, th.t32 + th.margin)


PITCHES = {"P31": pitch_p31, "P32": pitch_p32, "PT": pitch_pt}


@dataclass
class Payload:
    name: str
    role: str                     # "in", "out" or "inout" (an entry working in place)
    base: int                     # byte offset of the first element in the arena
    last: int                     # one past its last byte
    view: torch.Tensor            # the operand as the kernel gets it
    bytes: torch.Tensor           # the same bytes as uint8 [..., row bytes]
    original: Optional[torch.Tensor] = field(default=None, repr=False)  # compact copy of an input's bytes


class Arena:
    """nbytes of raw memory on `device`, sentinel-filled; operands are placed behind `headroom` bytes, one after the other."""

    def __init__(self, nbytes: int = ARENA_BYTES, device="cuda:0", th: Thresholds = REAL, slice_bytes: int = SLICE_BYTES):
        assert nbytes % ALIGN == 0 and slice_bytes % 2 == 0
        self.th, self.slice_bytes = th, slice_bytes
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % ALIGN == 0
        self.payloads: list[Payload] = []
        self.cursor = th.headroom
        self.reset()

    # ---- filling and placing -----------------------------------------------------------------------------------------------------
    def reset(self):
        self.buf.view(torch.int16).fill_(FILL16)
        self.payloads, self.cursor = [], self.th.headroom

    def place(self, name: str, shape, byte_strides, dtype, data: Optional[torch.Tensor] = None, role: str = "in") -> torch.Tensor:
        """An as_strided view of dtype `dtype` and the given shape; byte_strides per dimension, the last dimension dense. data (any device, same
        shape) is copied in; without data the payload keeps the sentinel (an output)."""
        shape, byte_strides = tuple(int(s) for s in shape), tuple(int(s) for s in byte_strides)
        size = torch.empty((), dtype=dtype).element_size()
        assert role in ("in", "out", "inout") and len(shape) == len(byte_strides) and byte_strides[-1] == size and all(n > 0 for n in shape)
        row = shape[-1] * size
        outer = sorted(zip(byte_strides[:-1], shape[:-1]))
        reach = row
        for stride, n in outer:  # no two elements of the payload share a byte, every row starts on an even address (the fill is a 2-byte pattern)
            assert stride % 2 == 0 and stride >= reach, (name, shape, byte_strides)
            reach = stride * (n - 1) + reach
        base = _up(self.cursor)
        last = base + reach
        assert base >= self.th.headroom and last <= self.buf.numel(), f"{name}: [{base}, {last}) does not fit the arena of {self.buf.numel()} bytes"
        self.cursor = last
        typed = self.buf.view(dtype)
        view = typed.as_strided(shape, tuple(s // size for s in byte_strides), base // size)
        raw = self.buf.as_strided(shape[:-1] + (row,), byte_strides[:-1] + (1,), base)
        assert view.data_ptr() == self.buf.data_ptr() + base and view.data_ptr() % ALIGN == 0
        p = Payload(name, role, base, last, view, raw)
        if data is not None:
            assert tuple(data.shape) == shape and data.dtype == dtype, (name, data.shape, data.dtype)
            view.copy_(data.to(self.buf.device))
        if role != "out":
            assert data is not None, f"{name}: an input needs data"
            p.original = raw.clone()
        self.payloads.append(p)
        return view

    def place_rows(self, name: str, data_or_shape, pitch: Optional[int] = None, dtype=torch.bfloat16, role: str = "in") -> torch.Tensor:
        """a [R][C] operand at a byte pitch (None: dense rows padded to 16 bytes plus 16 - compact, with sentinel behind every row)"""
        data = data_or_shape if isinstance(data_or_shape, torch.Tensor) else None
        R, Cc = data.shape if data is not None else data_or_shape
        dtype = data.dtype if data is not None else dtype
        size = torch.empty((), dtype=dtype).element_size()
        if pitch is None:
            pitch = _up(Cc * size) + ALIGN
        assert pitch % ALIGN == 0
        return self.place(name, (R, Cc), (pitch, size), dtype, data, role)

    def __getitem__(self, name: str) -> Payload:
        return next(p for p in self.payloads if p.name == name)

    # ---- the check ---------------------------------------------------------------------------------------------------------------
    def _blank(self, p: Payload):
        row = p.bytes.shape[-1]
        pattern = torch.tensor([FILL16 & 0xFF, FILL16 >> 8] * (-(-row // 2)), dtype=torch.uint8, device=self.buf.device)[:row]
        p.bytes.copy_(pattern.expand_as(p.bytes))

    def scan(self):
        """(number of 2-byte words of the whole arena that differ from the fill, byte offset of the first) - slice by slice"""
        words = self.buf.view(torch.int16)
        step = self.slice_bytes // 2
        counts = [(words[s:s + step] != FILL16).sum() for s in range(0, words.numel(), step)]
        counts = torch.stack(counts).cpu()
        bad = int(counts.sum())
        first = None
        if bad:
            i = int((counts != 0).nonzero()[0])
            first = 2 * (i * step + int((words[i * step:(i + 1) * step] != FILL16).nonzero()[0]))
        return bad, first

    def where(self, offset: int) -> str:
        """a byte offset of the arena in terms of the payloads (for the assertion's message)"""
        if offset < self.th.headroom:
            return f"byte {offset}: in the headroom, {self.th.headroom - offset} bytes before the first operand"
        inside = [p for p in self.payloads if p.base <= offset < p.last]
        if inside:
            return f"byte {offset}: {offset - inside[0].base} bytes behind the base of {inside[0].name!r}, between its rows"
        return f"byte {offset}: outside every operand's span"

    def check(self, what: str) -> dict:
        """-> {name: compact copy} of the output (and in-place) payloads. Leaves the arena sentinel-filled and empty of payloads."""
        outputs = {}
        for p in self.payloads:
            if p.role == "in":
                changed = int((p.bytes != p.original).sum())
                assert changed == 0, f"{what}: {changed} bytes of the input {p.name!r} were changed"
            else:
                got = p.view.clone()
                if got.dtype.is_floating_point:
                    bad = int((~torch.isfinite(got.float())).sum())
                    assert bad == 0, f"{what}: {bad} of {got.numel()} elements of the output {p.name!r} are not finite"
                outputs[p.name] = got
        for p in self.payloads:
            self._blank(p)
        bad, first = self.scan()
        msg = f"{what}: {bad} 2-byte words outside the payloads were written, the first at {self.where(first)}" if bad else ""
        if bad:
            self.reset()
        else:
            self.payloads, self.cursor = [], self.th.headroom
        assert not bad, msg
        return outputs

    def assert_untouched(self, what: str):
        """after a refused launch: nothing written at all, the outputs included"""
        outs = [p for p in self.payloads if p.role == "out"]
        for p in self.payloads:
            if p.role != "out":
                changed = int((p.bytes != p.original).sum())
                assert changed == 0, f"{what}: {changed} bytes of {p.name!r} were changed by a refused call"
        for p in self.payloads:
            if p.role != "out":
                self._blank(p)
        bad, first = self.scan()  # the output payloads still hold the fill
        names = [p.name for p in outs]
        if bad:
            where = self.where(first)
            self.reset()
            raise AssertionError(f"{what}: a refused call wrote {bad} 2-byte words (outputs {names} included), the first at {where}")
        self.payloads, self.cursor = [], self.th.headroom
