"""CPU: what the attention host code decides, through the dry run g3_attn_plan_bf16 and the four *_kernel_name functions ONLY - no launching entry point
is called (the operand pointers are placeholders). tests/golden/attn_plan_parent.json holds, for 916 calls of the seven launching entries, what the
launcher did before the call record / plan / kernel table existed: the kernel it launched, or the status and full text of its refusal (recorded from that
library: refusals as it returned them, accepted calls from a build that reported the kernel's name where it would have asked HIP for the device), and
what the name functions answered on a grid of shapes, variants, bounds and "attn_variant" options (inputs the entry points refuse included)."""
import json
import math
import re
from pathlib import Path

from gen3c_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = json.loads((ROOT / "tests" / "golden" / "attn_plan_parent.json").read_text())
ENTRY = {"fwd": 0, "kvseg": 1, "cross": 2, "ex": 3, "bounded": 4, "carry": 5, "bounded_cp": 6}  # enum g3_attn_entry
PLAN_ARGS = ["q", "q_row", "q_batch", "q_head", "q_norm_weight", "q_norm_eps", "k", "k_row", "k_batch", "k_head", "vt", "vt_row", "vt_batch", "vt_head",
             "vt_seg_len", "vt_seg_stride", "kv_skip_begin", "kv_skip_len", "carry_o", "carry_lse", "o", "o_partial", "lse", "o_row", "o_batch", "o_head",
             "Sq", "Skv", "kv_dense", "B", "H", "head_dim", "softmax_scale", "logit_bound", "variant"]


def _canonical(Sq, Skv, B, H):
    """Contiguous [S*B, H*128] q / k / o and V^T [B, H, 128, ceil64(Skv)] at placeholder addresses; a fixture row lists what differs."""
    ld = (Skv + 63) // 64 * 64
    return dict(q=0x10000, q_row=B * H * 128, q_batch=H * 128, q_head=128, q_norm_weight=0, q_norm_eps=0.0,
                k=0x20000, k_row=B * H * 128, k_batch=H * 128, k_head=128, vt=0x30000, vt_row=ld, vt_batch=H * 128 * ld, vt_head=128 * ld,
                vt_seg_len=0, vt_seg_stride=0, kv_skip_begin=0, kv_skip_len=0, carry_o=0, carry_lse=0,
                o=0x40000, o_partial=0, lse=0, o_row=B * H * 128, o_batch=H * 128, o_head=128,
                Sq=Sq, Skv=Skv, kv_dense=0, B=B, H=H, head_dim=128, softmax_scale=1.0 / math.sqrt(128), logit_bound=0.0, variant=0)


def _num(v):
    return float(v) if isinstance(v, str) else v  # "nan" / "inf": JSON has neither


def _plan(lib, entry, args, option=0):
    """(kernel name, None) or (None, (status is G3_ERR_ARG, error text)) of the dry run under the option."""
    lib.g3_set_option(b"attn_variant", option)
    try:
        name = lib.g3_attn_plan_bf16(ENTRY[entry], *[_num(args[n]) for n in PLAN_ARGS])
        return (name.decode(), None) if name is not None else (None, lib.g3_last_error().decode())
    finally:
        lib.g3_set_option(b"attn_variant", 0)


def _calls():
    """(note, entry, option, shape, arguments that differ from the canonical ones, recorded kernel or None, recorded refusal text or None) per call."""
    for g in FIXTURE["groups"]:
        for entries, option, Sq, Skv, B, H, over, result in g["calls"]:
            for entry in entries.split("|"):  # "a|b": the same call through each entry, with the same outcome
                yield (g["note"], entry, option, (Sq, Skv, B, H), over, FIXTURE["kernels"][result] if result >= 0 else None,
                       FIXTURE["errors"][-1 - result] if result < 0 else None)


def test_plan_equals_the_recorded_launcher():
    lib = _lib.load()
    calls = list(_calls())
    assert len(calls) == 916
    bad = []
    for note, entry, option, shape, over, kernel, error in calls:  # (every recorded refusal has status G3_ERR_ARG; the dry run's is NULL + the text)
        got = _plan(lib, entry, {**_canonical(*shape), **over}, option)
        if got != (kernel, error):
            bad.append((entry, note, shape, over, (kernel, error), got))
    assert not bad, f"{len(bad)} of {len(calls)} calls differ, first: {bad[:5]}"


def test_a_refusal_leaves_its_text_and_an_accepted_call_leaves_the_last_error_alone():
    lib = _lib.load()
    a = _canonical(512, 4096, 1, 8)
    assert _plan(lib, "carry", dict(a, variant=9)) == (None, "g3_flash_attn_fwd_carry_bf16: the carry / key-skip form exists for the 8-wave (4) and "
                                                            "one-wave-per-SIMD (11) kernels only (variant 9 chosen; 11 needs S_kv % 64 == 0)")
    before = lib.g3_last_error()
    assert _plan(lib, "carry", dict(a, variant=11)) == ("flash_attn_fwd_w4b_carry_kernel<true>", None) and lib.g3_last_error() == before
    assert lib.g3_attn_plan_bf16(7, *[a[n] for n in PLAN_ARGS]) is None and lib.g3_last_error() == b"g3_attn_plan_bf16: unknown entry 7"


def test_name_functions_answer_as_before():
    lib = _lib.load()
    kernels, variants = FIXTURE["kernels"], FIXTURE["name_variants"]
    rows = FIXTURE["names (option, shape, logit_bound, per variant the kernel indices of name_columns)"]
    assert len(rows) * len(variants) == 756
    bad = []
    try:
        for option, s, bound, per_variant in rows:
            lib.g3_set_option(b"attn_variant", option)
            for v, want in zip(variants, per_variant):
                got = [lib.g3_flash_attn_kernel_name(*s), lib.g3_flash_attn_kernel_name_ex(*s, v), lib.g3_self_attn_kernel_name(*s, _num(bound), v)]
                got += [lib.g3_self_attn_cp_kernel_name(*s, _num(bound), v, seg, cp) for seg in (0, 1) for cp in (0, 1)]
                if [g.decode() for g in got] != [kernels[i] for i in want]:
                    bad.append((option, s, bound, v, got))
    finally:
        lib.g3_set_option(b"attn_variant", 0)
    assert not bad, f"{len(bad)} rows differ, first: {bad[:3]}"


def test_plan_agrees_with_the_name_functions_on_canonical_operands():
    """Over the fixture's grid of shapes: wherever a call with canonical operands is accepted, the dry run names what the shapes-only function names."""
    lib = _lib.load()
    shapes = sorted({c[3] for c in _calls()})
    unit = 128 / math.sqrt(128) * 1.03
    n = 0
    for option in (0, 11, 4):
        for s in shapes:
            a = _canonical(*s)
            opt = lambda f, *args: _with_option(lib, option, f, *args)
            for v in range(0, 12):
                checks = [("ex", dict(a, variant=v), opt(lib.g3_flash_attn_kernel_name_ex, *s, v))]
                if v == 0:
                    checks += [(e, a, opt(lib.g3_flash_attn_kernel_name, *s)) for e in ("fwd", "cross")]
                for bound in (0.0, unit, 61.0 / math.log2(math.e)):
                    ab = dict(a, variant=v, logit_bound=bound)
                    checks.append(("bounded", ab, opt(lib.g3_self_attn_kernel_name, *s, bound, v)))
                    checks.append(("bounded_cp", ab, opt(lib.g3_self_attn_cp_kernel_name, *s, bound, v, 0, 0)))
                    checks.append(("bounded_cp", dict(ab, carry_o=0x70000, carry_lse=0x80000), opt(lib.g3_self_attn_cp_kernel_name, *s, bound, v, 0, 1)))
                    checks.append(("carry", ab, opt(lib.g3_self_attn_cp_kernel_name, *s, 0.0, v, 0, 0)))
                for entry, args, want in checks:
                    name, err = _plan(lib, entry, args, option)
                    if err is None:
                        assert name == want.decode(), (option, s, v, entry, name, want)
                        n += 1
    assert n > 1000


def _with_option(lib, option, f, *args):
    lib.g3_set_option(b"attn_variant", option)
    try:
        return f(*args)
    finally:
        lib.g3_set_option(b"attn_variant", 0)


def test_kernel_table_has_one_row_per_instantiation():
    """The table is the one place on the host side that names the instantiations: 21 rows, no name twice, and the recorded calls reach every one."""
    src = (ROOT / "gen3c_amd" / "csrc" / "attention.hip").read_text()
    table = src[src.index("#define G3_ATTN_KERNELS(X)"):src.index("#define G3_ATTN_ID")]
    rows = re.findall(r"X\((\w+), \w+, \w+, (flash_attn_fwd_\w+<[^>]*>)\)", table)
    assert len(rows) == 21 and table.count("X(") == 21
    assert len({r[0] for r in rows}) == 21 and len({r[1] for r in rows}) == 21
    reached = {c[5] for c in _calls() if c[5] is not None}
    assert reached == {r[1] for r in rows}
    host = src[src.index('#include "gen3c_hip.h"'):]
    for _, name in rows:
        assert host.count(name) == 1, name


def test_operand_spans_at_the_32_bit_budget_of_the_lds_dma_kernels():
    """attn_plan: k_max = (S_kv - 1 + 128) k_row 2 + 256 and v_max = 127 vt_row 2 + (S_kv + 64) 2 + 256 (plain V^T) must not exceed 2^32 - 1 for the
    kernels that address K / V^T with 32-bit byte offsets. One step (8 elements) below the bound every variant keeps its kernel; at it the plain and
    the bounded entry run the 64-bit-addressing kernel (variant 2) and the carry entries refuse. Batch and head strides, and every stride of Q and
    O, are 64-bit in all kernels: no bound."""
    lib = _lib.load()
    Sq, Skv, B, H = 200, 320, 2, 3
    a = _canonical(Sq, Skv, B, H)
    k_row = ((1 << 32) - 1 - 256) // (2 * (Skv - 1 + 128)) // 8 * 8
    vt_row = ((1 << 32) - 1 - 256 - 2 * (Skv + 64)) // (2 * 127) // 8 * 8
    assert (Skv + 127) * k_row * 2 + 256 < 1 << 32 <= (Skv + 127) * (k_row + 8) * 2 + 256
    assert 127 * vt_row * 2 + (Skv + 64) * 2 + 256 < 1 << 32 <= 127 * (vt_row + 8) * 2 + (Skv + 64) * 2 + 256
    v2 = lib.g3_flash_attn_kernel_name_ex(Sq, Skv, B, H, 2).decode()
    assert "v2" in v2
    for variant in (0, 4, 9, 11):
        for entry, bound in (("ex", 0.0), ("bounded", 23.0)):
            base = dict(a, variant=variant, logit_bound=bound)
            same, _ = _plan(lib, entry, base)
            assert same is not None and "v2" not in same
            for stride, at in (("k_row", k_row), ("vt_row", vt_row)):
                far = dict(base, **{stride: at}, **({"vt_head": 128 * at, "vt_batch": H * 128 * at} if stride == "vt_row" else {}))
                assert _plan(lib, entry, far) == (same, None), (variant, entry, stride)
                far[stride] = at + 8
                assert _plan(lib, entry, far) == (v2, None), (variant, entry, stride)
            huge = dict(base, q_row=1 << 40, q_batch=1 << 50, k_batch=1 << 50, k_head=1 << 45, vt_batch=1 << 50, vt_head=1 << 45, o_row=1 << 40, o_head=1 << 50)
            assert _plan(lib, entry, huge) == (same, None), (variant, entry)
    for entry in ("carry", "bounded_cp"):
        base = dict(a, variant=11, logit_bound=23.0 if entry == "bounded_cp" else 0.0, carry_o=0x50000, carry_lse=0x60000)
        assert _plan(lib, entry, dict(base, k_row=k_row))[0] is not None
        name, err = _plan(lib, entry, dict(base, k_row=k_row + 8))
        assert name is None and err.startswith("g3_flash_attn_fwd_carry_bf16: K / V^T span (skipped keys included) exceeds the kernel's 32-bit byte offsets"), err


def test_spatial_attention_d512_refuses_at_its_two_span_bounds():
    """g3_spatial_attn_d512_bf16 has no dry run and no fallback: hw 512 2 >= 2^32 (a K piece's offset inside a frame) and 8 ld_vt 2 >= 2^32 (a V^T
    piece's 8 rows) are refused with G3_ERR_ARG before anything is launched. One step below either bound the operands span 4 GiB and 256 GiB, which
    no test allocates, so the refusals are called with placeholder pointers - and ONLY where the process has no GPU: there a weakened bound
    ends in a failed launch (another status, a failed assertion below), never in a kernel that follows the placeholders. With a GPU the launching
    entry is not called (the loop only restates the bounds); tests/test_far_operands_gpu.py runs it on real operands on both sides of 2^31 and 2^32 bytes of V^T span."""
    import torch
    lib = _lib.load()
    text = b"g3_spatial_attn_d512_bf16: a frame exceeds the 32-bit byte offsets of the LDS-DMA addressing"
    for hw, ld_vt in ((64, 1 << 28), (64, (1 << 28) + 8), (1 << 22, 1 << 22)):
        assert (hw * 1024 >= 1 << 32) or (16 * ld_vt >= 1 << 32)
        if torch.cuda.is_available():
            continue  # placeholder pointers go to a launching entry only where no GPU can follow them
        rc = lib.g3_spatial_attn_d512_bf16(0x10000, 0x20000, 0x30000, ld_vt, 512 * ld_vt, 0x40000, 1, hw, 0.044, None)
        assert rc == _lib.G3_ERR_ARG and lib.g3_last_error() == text, (hw, ld_vt, rc, lib.g3_last_error())
