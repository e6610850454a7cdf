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
