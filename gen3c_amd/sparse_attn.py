"""Builders of range tables for ops.self_attn_ranges (g3_self_attn_fwd_ranges_bf16; the function and the table's rules: include/gen3c_hip.h).

Tokens are ordered (t, h, w): T latent frames of frame_len tokens, S = T * frame_len (a multiple of 64). Every builder returns a host int32 array
[1, n_qblk, max_ranges, 2] of (first_key, n_keys) pairs - one pattern, one ascending list of disjoint 64-key-aligned ranges per block of Q_ROWS query
rows, terminated by n_keys == 0 - for ops.attn_range_table, which validates and uploads it. A block's list is the union over its rows of what the
row-level definition attends, rounded OUTWARD to whole 64-key tiles, with overlapping and touching ranges merged: the kernel masks nothing, so a
row attends a superset of its own definition. No builder touches the GPU.

Picture quality under any of these patterns is unmeasured: no trained checkpoint exists in this project."""
from __future__ import annotations

import math

import numpy as np

Q_ROWS = 256    # query rows per block (g3_self_attn_window_q_rows(), the kernel's workgroup)
KEY_TILE = 64   # keys per tile
MAX_RANGES = 64  # g3_self_attn_ranges_max()


def _check_shape(name: str, T: int, frame_len: int) -> int:
    if T <= 0 or frame_len <= 0 or (T * frame_len) % KEY_TILE:
        raise ValueError(f"{name}: T {T} x frame_len {frame_len} must be a positive multiple of {KEY_TILE} tokens")
    return T * frame_len


def _merge_tiles(intervals, S: int):
    """[(k0, k1)) key intervals -> ascending disjoint (first_key, n_keys) with whole tiles, overlapping and touching ranges merged."""
    out = []
    for k0, k1 in sorted((k0 // KEY_TILE * KEY_TILE, min(S, -(-k1 // KEY_TILE) * KEY_TILE)) for k0, k1 in intervals if k1 > k0):
        if out and k0 <= out[-1][1]:
            out[-1][1] = max(out[-1][1], k1)
        else:
            out.append([k0, k1])
    return [(k0, k1 - k0) for k0, k1 in out]


def _table(name: str, lists) -> np.ndarray:
    n = max(len(rl) for rl in lists)
    if n > MAX_RANGES:
        raise ValueError(f"{name}: a query block needs {n} ranges, the kernel takes at most {MAX_RANGES}")
    tab = np.zeros((1, len(lists), n, 2), dtype=np.int32)
    for b, rl in enumerate(lists):
        tab[0, b, :len(rl)] = rl
    return tab


def _block_frames(b: int, S: int, frame_len: int):
    """The rows of query block b, split by frame: [(frame, first in-frame position, last in-frame position)]."""
    r0, r1 = b * Q_ROWS, min(b * Q_ROWS + Q_ROWS, S) - 1
    return [(f, max(r0, f * frame_len) - f * frame_len, min(r1, f * frame_len + frame_len - 1) - f * frame_len)
            for f in range(r0 // frame_len, r1 // frame_len + 1)]


def frame_ranges(T: int, frame_len: int, window_frames: int, sink_frames: int) -> np.ndarray:
    """The frame window of ops.self_attn_window at ANY frame length: the block whose rows lie in frames f0..f1 attends the keys of the frames
    [max(0, f0 - W), min(T, f1 + W + 1)) and of the frames [0, min(s, T)). Where frame_len % 64 == 0 the mask (ops.ranges_attn_mask) is
    ops.window_attn_mask exactly and the launch visits the window kernels' tiles in their order; at other frame lengths (720p: 45 x 80 = 3 600
    tokens, which the window entry refuses) every range is rounded outward to whole tiles."""
    S = _check_shape("frame_ranges", T, frame_len)
    W, s = int(window_frames), int(sink_frames)
    if W < 0 or s < 0:
        raise ValueError(f"frame_ranges: window_frames {W} and sink_frames {s} must be >= 0")
    lists = []
    for b in range(-(-S // Q_ROWS)):
        fr = _block_frames(b, S, frame_len)
        f0, f1 = fr[0][0], fr[-1][0]
        lists.append(_merge_tiles([(0, min(s, T) * frame_len), (max(0, f0 - W) * frame_len, min(T, f1 + W + 1) * frame_len)], S))
    return _table("frame_ranges", lists)


def radial_half_width(frame_len: int, d: int, width1: float, min_width: int) -> int:
    """hw(d), d >= 1: max(min_width, ceil(frame_len * width1 / 2^floor(log2 d)))"""
    return max(int(min_width), math.ceil(frame_len * width1 / (1 << (int(d).bit_length() - 1))))


def radial_ranges(T: int, frame_len: int, width1: float = 0.25, sink_frames: int = 1, min_width: int = 64) -> np.ndarray:
    """A spatial band that narrows with frame distance, IN THE STYLE OF radial attention (arXiv 2506.19852) - not an implementation of it: the
    half-width halves every time the frame distance doubles, as there, but frames are never subsampled here, and nothing is tuned on a model.
    Row-level definition: the query at in-frame position pq of frame fq attends the key at position pk of frame fk iff
        fk < sink_frames,  or  fk == fq,  or  |pq - pk| < hw(d),  d = |fq - fk|,  hw(d) = max(min_width, ceil(frame_len * width1 / 2^floor(log2 d))).
    The table holds, per query block, the union over its rows, rounded outward to 64-key tiles, touching ranges merged."""
    S = _check_shape("radial_ranges", T, frame_len)
    if not width1 > 0 or sink_frames < 0 or min_width < 1:
        raise ValueError(f"radial_ranges: width1 {width1} must be > 0, sink_frames {sink_frames} >= 0, min_width {min_width} >= 1")
    lists = []
    for b in range(-(-S // Q_ROWS)):
        iv = [(0, min(int(sink_frames), T) * frame_len)]
        for fq, p0, p1 in _block_frames(b, S, frame_len):
            for fk in range(T):
                if fk == fq:
                    iv.append((fk * frame_len, (fk + 1) * frame_len))
                else:
                    hw = radial_half_width(frame_len, abs(fq - fk), width1, min_width)
                    iv.append((fk * frame_len + max(0, p0 - hw + 1), fk * frame_len + min(frame_len, p1 + hw)))
        lists.append(_merge_tiles(iv, S))
    return _table("radial_ranges", lists)


def band_ranges(T: int, frame_len: int, width: float = 0.125, sink_frames: int = 1, min_width: int = 64) -> np.ndarray:
    """The temporal-head pattern of the per-head schemes (Sparse VideoGen's "temporal head", arXiv 2502.01776, in this token order): a spatial band
    of CONSTANT width across ALL frames, the query's own included - radial_ranges' band with a half-width that does not shrink,
        hw = max(min_width, ceil(frame_len * width)),
    and without its whole-own-frame clause (that is the spatial head's part). Row-level definition: the query at in-frame position pq of frame fq
    attends the key at position pk of frame fk iff  fk < sink_frames  or  |pq - pk| < hw.
    The table holds, per query block, the union over its rows, rounded outward to 64-key tiles, touching ranges merged."""
    S = _check_shape("band_ranges", T, frame_len)
    if not width > 0 or sink_frames < 0 or min_width < 1:
        raise ValueError(f"band_ranges: width {width} must be > 0, sink_frames {sink_frames} >= 0, min_width {min_width} >= 1")
    hw = max(int(min_width), math.ceil(frame_len * width))
    lists = []
    for b in range(-(-S // Q_ROWS)):
        iv = [(0, min(int(sink_frames), T) * frame_len)]
        for fq, p0, p1 in _block_frames(b, S, frame_len):
            iv += [(fk * frame_len + max(0, p0 - hw + 1), fk * frame_len + min(frame_len, p1 + hw)) for fk in range(T)]
        lists.append(_merge_tiles(iv, S))
    return _table("band_ranges", lists)


def stack_tables(tables) -> np.ndarray:
    """One-or-more-pattern tables for the same S -> one table [sum of n_patterns, n_qblk, max of max_ranges, 2], zero-padded behind every terminator."""
    tables = [np.asarray(t) for t in tables]
    if not tables or any(t.ndim != 4 or t.shape[3] != 2 or t.dtype != np.int32 or t.shape[1] != tables[0].shape[1] for t in tables):
        raise ValueError("stack_tables: expected int32 tables [n_patterns, n_qblk, max_ranges, 2] with one n_qblk")
    out = np.zeros((sum(t.shape[0] for t in tables), tables[0].shape[1], max(t.shape[2] for t in tables), 2), dtype=np.int32)
    p = 0
    for t in tables:
        out[p:p + t.shape[0], :, :t.shape[2]] = t
        p += t.shape[0]
    return out


AUTO_MAX = 8  # candidates of an "auto" spec: the bits of the profiler's membership byte
_EXPECTED = ("expected radial:WIDTH1:SINK or frame:W:S, or band:WIDTH:SINK, or auto=SPEC,SPEC[,...] with 2 to 8 of those (each head picks, per block and "
             "per forward, the candidate that keeps most of its sampled rows' softmax mass)")


def _parse_one(text: str):
    parts = text.split(":")
    try:
        if len(parts) == 3 and parts[0] in ("radial", "band"):
            return (parts[0], float(parts[1]), int(parts[2]))
        if len(parts) == 3 and parts[0] == "frame":
            return ("frame", int(parts[1]), int(parts[2]))
    except ValueError:
        pass
    return None


def parse_pattern(text):
    """'radial:WIDTH1:SINK' | 'frame:W:S' | 'band:WIDTH:SINK' | 'auto=SPEC,SPEC[,...]' (the command lines' --self_attn_pattern and
    G3_SELF_ATTN_PATTERN) -> the DiT's spec tuple; None / '' -> None."""
    if text is None or text == "":
        return None
    text = str(text)
    if text.startswith("auto="):
        cands = [_parse_one(t) for t in text[len("auto="):].split(",")]
        if all(c is not None for c in cands) and 2 <= len(cands) <= AUTO_MAX:
            return ("auto", *cands)
    elif _parse_one(text) is not None:
        return _parse_one(text)
    raise ValueError(f"self_attn_pattern {text!r}: {_EXPECTED}")


def _check_one(spec):
    try:
        if len(spec) == 3 and spec[0] in ("radial", "band") and float(spec[1]) > 0 and int(spec[2]) >= 0:
            return (spec[0], float(spec[1]), int(spec[2]))
        if len(spec) == 3 and spec[0] == "frame" and int(spec[1]) >= 0 and int(spec[2]) >= 0:
            return ("frame", int(spec[1]), int(spec[2]))
    except (TypeError, ValueError):
        pass
    return None


def check_spec(spec):
    """The DiT's spec tuple, normalised: ('radial', width1 > 0, sink_frames >= 0) | ('frame', W >= 0, s >= 0) | ('band', width > 0, sink_frames >= 0) |
    ('auto', spec, spec, ...) with 2 to 8 of the former | None."""
    if spec is None:
        return None
    if isinstance(spec, str):
        return check_spec(parse_pattern(spec))
    if len(spec) >= 1 and spec[0] == "auto":
        cands = [None if isinstance(c, str) else _check_one(c) for c in spec[1:]]
        if 2 <= len(cands) <= AUTO_MAX and all(c is not None for c in cands):
            return ("auto", *cands)
    elif _check_one(spec) is not None:
        return _check_one(spec)
    raise ValueError(f"self_attn_pattern {spec!r}: expected ('radial', width1 > 0, sink_frames >= 0), ('frame', W >= 0, s >= 0) or None - or "
                     f"('band', width > 0, sink_frames >= 0), or ('auto', spec, spec, ...) with 2 to 8 of those; as a string: {_EXPECTED}")


def is_auto(spec) -> bool:
    return spec is not None and spec[0] == "auto"


def build_spec(spec, T: int, frame_len: int) -> np.ndarray:
    """The table of a (checked) spec: one pattern, or for ('auto', ...) its candidates stacked in their order."""
    spec = check_spec(spec)
    if is_auto(spec):
        return stack_tables([build_spec(c, T, frame_len) for c in spec[1:]])
    kind, a, b = spec
    return {"radial": radial_ranges, "band": band_ranges, "frame": frame_ranges}[kind](T, frame_len, a, b)


def tile_density(table: np.ndarray, S: int) -> list:
    """Per pattern of a valid table: attended (query block, tile) pairs / all pairs."""
    table = np.asarray(table)
    return [float(table[p, :, :, 1].sum()) / KEY_TILE / (table.shape[1] * (S // KEY_TILE)) for p in range(table.shape[0])]


def spec_text(spec) -> str:
    """The command lines' string of a checked spec."""
    if is_auto(spec):
        return "auto=" + ",".join(spec_text(c) for c in spec[1:])
    return f"{spec[0]}:{spec[1]}:{spec[2]}"


def auto_report(spec, table: np.ndarray, S: int) -> list:
    """The lines the command lines print once per shape under an ('auto', ...) spec: every candidate's tile density, and a warning where the densities
    differ by more than a factor 1.25 - recall, the selection criterion, favours the denser candidate."""
    dens = tile_density(table, S)
    lines = [f"[gen3c_amd] self-attention pattern auto, S = {S}: " + ", ".join(f"{i} = {spec_text(c)} tile density {d:.3f}" for i, (c, d) in
                                                                             enumerate(zip(spec[1:], dens)))]
    if max(dens) > 1.25 * min(dens):
        lines.append(f"[gen3c_amd] warning: the candidates' tile densities differ by a factor {max(dens) / min(dens):.2f} (> 1.25): heads are chosen by the "
                     "softmax mass a candidate keeps, which favours the denser one")
    return lines
