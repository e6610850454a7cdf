"""CPU: the host side of the per-head pattern selection (g3_attn_pattern_profile_bf16, include/gen3c_hip.h): the band pattern against its row-level
definition, stacked tables, the membership bitmask against ops.ranges_attn_mask, every refusal's text through the dry run, the "auto=" spec, the
DiT's refusals under it, and the fp64 reference's teeth."""
import argparse
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import attn_profile_ref as ref

BAR = 2e-4  # the GPU tests' recall bar (tests/test_attn_profile_gpu.py derives it)


@pytest.mark.parametrize("T,frame_len,width,sink", [(6, 1024, 0.0625, 0), (5, 320, 0.1, 1)])
def test_band_ranges_against_row_level_definition(T, frame_len, width, sink):
    from gen3c_amd import ops, sparse_attn
    S = T * frame_len
    tab = sparse_attn.band_ranges(T, frame_len, width, sink)
    hw = max(64, math.ceil(frame_len * width))
    rows = np.arange(S)
    f, p = rows // frame_len, rows % frame_len
    row_level = (f[None, :] < sink) | (np.abs(p[:, None] - p[None, :]) < hw)  # [query, key]
    want = np.zeros((S, S), dtype=bool)  # per block: the union over its rows, outward to whole 64-key tiles
    for b in range(-(-S // 256)):
        tiles = row_level[256 * b:256 * b + 256].any(axis=0).reshape(S // 64, 64).any(axis=1)
        want[256 * b:256 * b + 256] = np.repeat(tiles, 64)[None, :]
    table = _host_table(tab, S)
    assert np.array_equal(ops.ranges_attn_mask(table, S).numpy(), want)
    assert (want | ~row_level).all()  # a superset of every row's own definition
    lists = tab[0]
    assert all((lists[b, 1:, 0][lists[b, 1:, 1] > 0] > (lists[b, :-1, 0] + lists[b, :-1, 1])[lists[b, 1:, 1] > 0]).all() for b in range(len(lists))), "touching ranges merged"


def _host_table(tab, S, head_pattern=None):
    """ops.attn_range_table without the upload (no GPU here): validated by g3_attn_ranges_check."""
    from gen3c_amd import _lib, ops
    host = torch.from_numpy(np.ascontiguousarray(tab))
    att, dense = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().g3_attn_ranges_check(host.data_ptr(), host.shape[0], S, host.shape[2], None, 1, ctypes.byref(att), ctypes.byref(dense)))
    t = ops.AttnRangeTable()
    t.ranges, t.S, t.n_patterns, t.max_ranges = host, S, host.shape[0], host.shape[2]
    return t


def test_band_density_at_the_product_shape():
    from gen3c_amd import sparse_attn
    tab = sparse_attn.band_ranges(16, 3520, 0.125, 1)
    assert tab.shape[2] <= 16 and abs(sparse_attn.tile_density(tab, 56320)[0] - 0.352) < 5e-4
    assert abs(sparse_attn.tile_density(sparse_attn.frame_ranges(16, 3520, 2, 1), 56320)[0] - 0.343) < 5e-4


def test_stack_tables_is_a_valid_table():
    from gen3c_amd import ops, sparse_attn
    S = 6 * 1024
    a, b, c = sparse_attn.frame_ranges(6, 1024, 0, 0), sparse_attn.band_ranges(6, 1024, 0.0625, 0), sparse_attn.radial_ranges(6, 1024, 0.25, 1)
    st = sparse_attn.stack_tables([a, b, c])
    assert st.shape == (3, 24, max(a.shape[2], b.shape[2], c.shape[2]), 2) and st.dtype == np.int32
    table = _host_table(st, S)  # g3_attn_ranges_check: zero behind every terminator included
    for p, one in enumerate((a, b, c)):
        assert torch.equal(ops.ranges_attn_mask(table, S, pattern=p), ops.ranges_attn_mask(one, S))
    assert np.array_equal(sparse_attn.build_spec(("auto", ("frame", 0, 0), ("band", 0.0625, 0)), 6, 1024), sparse_attn.stack_tables([a, b]))
    with pytest.raises(ValueError, match="one n_qblk"):
        sparse_attn.stack_tables([a, sparse_attn.frame_ranges(5, 1024, 0, 0)])


def _members(tab, S, rows):
    from gen3c_amd import _lib
    host = torch.from_numpy(np.ascontiguousarray(tab))
    r = torch.tensor(rows, dtype=torch.int32)
    out = torch.full((len(rows), S // 64), 255, dtype=torch.uint8)
    rc = _lib.load().g3_attn_profile_members(host.data_ptr(), host.shape[0], S, host.shape[2], r.data_ptr(), len(rows), out.data_ptr())
    return rc, out


@pytest.mark.parametrize("S", [832, 1920])
def test_members_against_ranges_attn_mask(S):
    from gen3c_amd import ops, sparse_attn
    if S == 832:
        tab, rows = ref.hand_table_832(), ref.SAMPLE_ROWS_832
    else:
        tab = sparse_attn.stack_tables([sparse_attn.frame_ranges(5, 384, 5, 0), sparse_attn.frame_ranges(5, 384, 0, 1), sparse_attn.band_ranges(5, 384, 0.2, 0)])
        rows = [((2 * i + 1) * S) // (2 * 33) for i in range(33)]
    rc, got = _members(tab, S, rows)
    assert rc == 0
    table = _host_table(tab, S)
    want = torch.zeros_like(got)
    for p in range(tab.shape[0]):
        mask = ops.ranges_attn_mask(table, S, pattern=p)[rows]  # [n, S]
        tiles = mask.reshape(len(rows), S // 64, 64)
        assert (tiles.all(dim=2) == tiles.any(dim=2)).all()
        want |= tiles.any(dim=2).to(torch.uint8) << p
    assert torch.equal(got, want)


def test_members_refusals():
    from gen3c_amd import _lib
    tab = ref.hand_table_832()
    for rows, text in (([0, 0], "sample_rows[1] = 0: the rows must be strictly ascending in [0, 832)"), ([5, 832], "sample_rows[1] = 832"),
                       ([-1], "sample_rows[0] = -1"), (list(range(65)), "n 65 sample rows outside [1, 64]")):
        rc, _ = _members(tab, 832, rows)
        assert rc == _lib.G3_ERR_ARG and text in _lib.last_error()
    bad = tab.copy()
    bad[1, 2, 1] = (704, 192)
    rc, _ = _members(bad, 832, [600])
    assert rc == _lib.G3_ERR_ARG and "pattern 1, block 2, range 1" in _lib.last_error()


def _plan(**over):
    from gen3c_amd import _lib
    S, B, H, nc = over.get("S", 832), over.get("B", 1), over.get("H", 2), over.get("n_chunks", 5)
    a = dict(q=0x10000, q_row=3 * H * 128 * B, q_batch=3 * H * 128, q_head=128, k=0x20000, k_row=3 * H * 128 * B, k_batch=3 * H * 128, k_head=128, S=S, B=B, H=H,
             head_dim=128, softmax_scale=0.0884, sample_rows=0x30000, n=13, tile_member=0x40001, n_patterns=3, n_chunks=nc, workspace=0x50000,
             workspace_bytes=None, recall=0x60000)
    a.update(over)
    lib = _lib.load()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.g3_attn_profile_workspace_bytes(a["B"], a["H"], a["n_chunks"])
    name = lib.g3_attn_pattern_profile_plan_bf16(*a.values())
    return (name.decode() if name else None), _lib.last_error()


def test_dry_run_names_the_kernel_and_every_refusal():
    from gen3c_amd import _lib
    lib = _lib.load()
    assert _plan()[0] == "attn_pattern_profile_kernel"
    assert _plan(n_chunks=1)[0] and _plan(n_chunks=13)[0] and _plan(n_patterns=1)[0] and _plan(n_patterns=8)[0] and _plan(n=1)[0] and _plan(n=64)[0]
    fn = "g3_attn_pattern_profile_bf16: "
    for over, text in [
            (dict(S=0), "S 0 must be a positive multiple of 64"), (dict(S=840), "S 840 must be a positive multiple of 64"),
            (dict(n_patterns=0), "n_patterns 0 outside [1, 8]"), (dict(n_patterns=9), "n_patterns 9 outside [1, 8]"),
            (dict(n=0), "n 0 sample rows outside [1, 64]"), (dict(n=65), "n 65 sample rows outside [1, 64]"),
            (dict(n_chunks=0), "n_chunks 0 outside [1, S / 64 = 13]"), (dict(n_chunks=14), "n_chunks 14 outside [1, S / 64 = 13]"),
            (dict(q=0), "null operand"), (dict(k=0), "null operand"), (dict(sample_rows=0), "null operand"), (dict(tile_member=0), "null operand"),
            (dict(workspace=0), "null operand"), (dict(recall=0), "null operand"),
            (dict(q=0x10008), "misaligned pointer (q, k: 16 bytes; sample_rows, workspace, recall: 4)"), (dict(k=0x20002), "misaligned pointer"),
            (dict(sample_rows=0x30002), "misaligned pointer"), (dict(recall=0x60001), "misaligned pointer"), (dict(workspace=0x50002), "misaligned pointer"),
            (dict(q_row=772), "q / k strides must be non-negative multiples of 8 elements"), (dict(k_head=132), "q / k strides must be"),
            (dict(k_batch=-768), "q / k strides must be"),
            (dict(head_dim=64), "head_dim 64: only 128 is supported"),
            (dict(workspace_bytes=lib.g3_attn_profile_workspace_bytes(1, 2, 5) - 1), "workspace of 25599 bytes is too small: g3_attn_profile_workspace_bytes gives 25600"),
            (dict(S=56320, n_chunks=4, q_row=40000), "operands beyond the kernel's 32-bit byte offsets over all S rows"),
            (dict(S=56320, n_chunks=4, k_row=40000), "operands beyond the kernel's 32-bit byte offsets over all S rows")]:
        name, err = _plan(**over)
        assert name is None and err.startswith(fn) and text in err, (over, err)
    # the product's fused QKV buffer (B = 2, 3 x 4096 columns) is inside the offset arithmetic
    assert _plan(S=56320, B=2, H=32, n_chunks=8, q_row=2 * 12288, q_batch=12288, k_row=2 * 12288, k_batch=12288)[0] == "attn_pattern_profile_kernel"


def test_default_chunks_and_workspace():
    from gen3c_amd import _lib
    lib = _lib.load()
    assert lib.g3_attn_profile_chunks(56320, 2, 32) == 8 and lib.g3_attn_profile_chunks(56320, 1, 32) == 16  # 512 workgroups: two per CU
    assert lib.g3_attn_profile_chunks(832, 1, 2) == 13 and lib.g3_attn_profile_chunks(64, 1, 1) == 1 and lib.g3_attn_profile_chunks(6144, 2, 512) == 1
    assert lib.g3_attn_profile_workspace_bytes(2, 3, 7) == 2 * 3 * 7 * 64 * 10 * 4 and lib.g3_attn_profile_workspace_bytes(0, 3, 7) == 0


def test_auto_spec_parsing_and_the_unchanged_error_text():
    from gen3c_amd import cli_common, sparse_attn
    assert sparse_attn.parse_pattern("auto=frame:2:1,band:0.125:1") == ("auto", ("frame", 2, 1), ("band", 0.125, 1))
    assert sparse_attn.parse_pattern("band:0.125:1") == ("band", 0.125, 1) and sparse_attn.parse_pattern("frame:2:1") == ("frame", 2, 1)
    assert sparse_attn.check_spec("auto=radial:0.25:1,frame:0:0,band:0.5:0") == ("auto", ("radial", 0.25, 1), ("frame", 0, 0), ("band", 0.5, 0))
    assert sparse_attn.check_spec(("auto", ("frame", 2, 1), ["band", 0.125, 1])) == ("auto", ("frame", 2, 1), ("band", 0.125, 1))
    assert sparse_attn.spec_text(("auto", ("frame", 2, 1), ("band", 0.125, 1))) == "auto=frame:2:1,band:0.125:1"
    nine = ",".join(["frame:1:1"] * 9)
    for bad in ("auto=frame:2:1", "auto=", f"auto={nine}", "auto=frame:2:1,zig:1:1", "auto=frame:2:1,auto=frame:1:1,frame:0:0", "band:x:1", "zig:1:1"):
        with pytest.raises(ValueError, match="expected radial:WIDTH1:SINK or frame:W:S"):
            sparse_attn.parse_pattern(bad)
        with pytest.raises(ValueError, match="expected radial:WIDTH1:SINK or frame:W:S"):
            sparse_attn.check_spec(bad)
    for bad in (("auto", ("frame", 2, 1)), ("auto", ("frame", 2, 1), ("band", -1.0, 1)), ("auto", ("frame", 2, 1), ("auto", ("frame", 1, 1), ("frame", 0, 0))),
                ("band", 0.0, 1), ("auto",) + (("frame", 1, 1),) * 9):
        with pytest.raises(ValueError, match="expected .*radial"):
            sparse_attn.check_spec(bad)
    args = argparse.Namespace(self_attn_pattern="auto=frame:2:1,band:0.125:1")
    assert cli_common.self_attn_pattern_requested(args) == ("auto", ("frame", 2, 1), ("band", 0.125, 1))
    lines = sparse_attn.auto_report(("auto", ("frame", 0, 0), ("band", 0.0625, 0)), sparse_attn.build_spec("auto=frame:0:0,band:0.0625:0", 6, 1024), 6144)
    assert "0 = frame:0:0 tile density 0.167" in lines[0] and "1 = band:0.0625:0 tile density 0.344" in lines[0]
    assert len(lines) == 2 and "differ by a factor 2.06 (> 1.25)" in lines[1]
    assert len(sparse_attn.auto_report(("auto", ("frame", 2, 1), ("band", 0.125, 1)), sparse_attn.build_spec("auto=frame:2:1,band:0.125:1", 16, 3520), 56320)) == 1


def test_env_selects_auto(monkeypatch):
    from gen3c_amd import cli_common
    monkeypatch.setenv("G3_SELF_ATTN_PATTERN", "auto=frame:2:1,band:0.125:1")
    assert cli_common.self_attn_pattern_requested(argparse.Namespace(self_attn_pattern=None)) == ("auto", ("frame", 2, 1), ("band", 0.125, 1))


def test_dit_refusals_with_auto():
    from gen3c_amd.dit import VideoExtendGeneralDIT
    kw = dict(max_img_h=48, max_img_w=48, max_frames=16, in_channels=81, model_channels=256, num_blocks=1, num_heads=2, adaln_lora_dim=32,
              crossattn_emb_channels=128, device="cpu", init_weights=False)
    spec = ("auto", ("frame", 0, 0), ("frame", 1, 1))
    net = VideoExtendGeneralDIT(self_attn_pattern="auto=frame:0:0,frame:1:1", **kw)
    assert net.self_attn_pattern == spec and net.self_attn_head_patterns() is None
    with pytest.raises(ValueError, match="not a multiple of 64, the kernel's key tile"):
        net._self_attn_table_for(3, 5, 8, "cpu")
    net.set_self_attn_window(1, 1)
    with pytest.raises(ValueError, match="self_attn_pattern and self_attn_window are both set"):
        net._self_attn_table_for(6, 8, 8, "cpu")
    net.set_self_attn_window(None)
    net._cp_attn, net.cp_size = object(), 4
    with pytest.raises(ValueError, match="with context parallelism over 4 ranks: range tables under key sharding are out of scope"):
        net._self_attn_table_for(6, 8, 8, "cpu")
    with pytest.raises(ValueError, match="expected .*radial"):
        net.set_self_attn_pattern(("auto", ("frame", 0, 0)))


def test_reference_has_teeth():
    """One tile's membership flipped moves a recall by far more than the GPU tests' bar."""
    g = torch.Generator().manual_seed(5)
    S, B, H = 832, 1, 2
    q = torch.randn(S * B, H * 128, generator=g).to(torch.bfloat16)
    k = torch.randn(S * B, H * 128, generator=g).to(torch.bfloat16)
    tab, rows = ref.hand_table_832(), ref.SAMPLE_ROWS_832
    base = ref.recall_ref(q, k, S, B, H, tab, rows)
    assert base.shape == (1, 2, 13, 3) and (base > 0).all() and (base < 1).all()
    for flip in ((0, 0, 0), (5, 1, 12), (12, 2, 6), (8, 2, 3)):
        moved = np.abs(ref.recall_ref(q, k, S, B, H, tab, rows, flip=flip) - base)[:, :, flip[0], flip[1]]
        assert moved.min() > 50 * BAR, (flip, moved)
    score, hp = ref.select_ref(np.array([[[[0.5, 0.5, 0.25]], [[0.1, 0.7, 0.7]]]]))
    assert hp.tolist() == [0, 1] and score.shape == (2, 3)
