"""CPU: what the bf16 GEMM / convolution host code decides, through the dry run g3_gemm_plan_bf16 and g3_gemm_kernel_name ONLY - no launching entry point is
called (the operand pointers are placeholders). tests/golden/gemm_plan_parent.json holds, for every call below, what the launcher did before the call record /
plan / kernel table existed, with 256 and with 64 CUs: the instantiation it launched, its grid and the follow-up launches of the entry, or the full text of its
refusal (recorded from that library: refusals as it returned them, accepted calls from a build of it whose launch sites reported the instantiation, the grid and
the follow-ups without touching HIP, the CU count forced), and what g3_gemm_kernel_name answered on a grid of shapes, epilogues and options with no device."""
import ctypes as C
import json
import re
from pathlib import Path

from gen3c_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = json.loads((ROOT / "tests" / "golden" / "gemm_plan_parent.json").read_text())
ENTRIES = ["nt", "qk", "conv", "conv_gnstats"]  # enum g3_gemm_entry
DEFAULTS = {"gemm_pingpong": 3, "gemm_regstage": 0, "gemm_unpinned": 1, "conv_w4": 1, "gemm_deferred": 1, "gemm_persistent": 0, "gemm_tokens_first": 2,
            "gemm_wide_store": 1, "gemm_deferred_grid": 0}  # the options the choice reads, and their defaults (csrc/api.hip)
N_CU = (256, 64)  # both sides of the "two tiles per workgroup" rules


def canonical(entry, base):
    """The call record of `entry` for a shape, with dense, aligned operands at placeholder addresses; a fixture row lists what differs.
    nt: (M, N, K, epilogue) with gate / residual where the epilogue reads them; qk: (M, N, K, B), one q and one k head, RoPE, no V^T;
    conv*: (K, N, Ti, Hi, Wi, kt, kh, kw) with bias, stride 1, 'same' padding (causal in time), one statistics frame per output frame."""
    a = dict(entry=ENTRIES.index(entry), A=0x10000, W=0x20000, C=0x30000)
    if entry == "nt":
        M, N, K, epi = base
        a.update(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, epilogue=epi, gate=0x40000 if epi in (2, 3, 4) else 0, gate_rows=1, ldg=N,
                 residual=0x50000 if epi in (2, 4) else 0, ldr=N)
    elif entry == "qk":
        M, N, K, B = base
        a.update(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, n_q=128, n_k=128, norm_q=0x60000, norm_k=0x61000, cos_table=0x70000, sin_table=0x80000, B=B, eps=1e-6,
                 vt=0, vt_ld=(max(M // max(B, 1), 0) + 7) // 8 * 8)
    else:
        K, N, Ti, Hi, Wi, kt, kh, kw = base
        a.update(N=N, K=K, lda=K, ldw=K, ldc=N, gate=0x40000, residual=0, ldr=N, Ti=Ti, Hi=Hi, Wi=Wi, To=Ti, Ho=Hi, Wo=Wi, kt=kt, kh=kh, kw=kw, st=1, sh=1, sw=1,
                 ot=1 - kt, oh=-(kh // 2), ow=-(kw // 2), gn_stats=0x90000, gn_rows=Hi * Wi)
    return a


def set_options(lib, options):
    for name, value in {**DEFAULTS, **options}.items():
        assert lib.g3_set_option(name.encode(), value) == 0


def plan(lib, args, n_cu):
    """[instantiation, grid, follow-up flags], or the refusal's text."""
    grid, follow = C.c_int(-1), C.c_uint(0)
    name = lib.g3_gemm_plan_bf16(C.byref(_lib.GemmCall(**args)), n_cu, C.byref(grid), C.byref(follow))
    return [name.decode(), grid.value, follow.value] if name is not None else lib.g3_last_error().decode()


def calls():
    """(note, entry, options, arguments, {n_cu: recorded [instantiation, grid, flags] or refusal text}) per recorded call: a group's calls are the
    product of its option sets, canonical shapes and argument replacements, in that order."""
    result = lambda r: FIXTURE["errors"][-1 - r] if isinstance(r, int) else [FIXTURE["kernels"][r[0]], r[1], r[2]]
    for g in FIXTURE["groups"]:
        entry, grid = ENTRIES[g["entry"]], [(o, b, v) for o in g["options"] for b in g["bases"] for v in g["overs"]]
        assert len(grid) == len(g["results"])
        for (option, base, over), r in zip(grid, g["results"]):
            outcome = FIXTURE["outcomes"][r]  # (one result: the same with either CU count)
            yield g["note"], entry, FIXTURE["option_sets"][option], {**canonical(entry, base), **over}, {n: result(x) for n, x in zip(N_CU, outcome * 2)}


def names():
    """(options, M, N, K, epilogue, recorded family) per recorded answer of g3_gemm_kernel_name."""
    n = FIXTURE["names"]
    for option, answers in zip(n["options"], n["answers"]):
        grid = [(M, N, K, e) for M in n["M"] for N in n["N"] for K in n["K"] for e in n["epilogues"]]
        assert len(grid) == len(answers)
        for (M, N, K, e), digit in zip(grid, answers):
            yield FIXTURE["option_sets"][option], M, N, K, e, n["families"][int(digit)]


def table():
    """{instantiation: family} as csrc/gemm.hip's kernel table spells them: the family rows, expanded over their epilogue lists."""
    src = (ROOT / "gen3c_amd" / "csrc" / "gemm.hip").read_text()
    lists = {m[0]: re.findall(r"X\((\d),", m[1]) for m in re.findall(r"#define G3_EPI_(\w+)\(X, \.\.\.\) ((?:X\(\d, __VA_ARGS__\) ?)+)$", src, flags=re.M)}
    lists["ALL_QK"] = lists["ALL"] + ["5"]
    fams = src[src.index("#define G3_GEMM_FAMILIES(F)"):src.index("#define G3_STR")]
    rows = {}
    for stem, epis, family, kernel, rest in re.findall(r'F\((GK_\w+), (\w+), \w+, \w+, "([^"]+)", (\w+)((?:, \w+)*)\)', fams):
        for e in lists[epis]:
            name = f"{kernel}<{e}{rest}>"
            assert name not in rows, name
            rows[name] = family
    assert fams.count("F(GK_") == 16
    return rows, src


def test_plan_equals_the_recorded_launcher():
    lib = _lib.load()
    recorded = list(calls())
    assert len(recorded) == FIXTURE["n_calls"] and len(recorded) > 1500
    bad = []
    try:
        for note, entry, options, args, want in recorded:
            set_options(lib, options)
            got = {n_cu: plan(lib, args, n_cu) for n_cu in N_CU}
            if got != want:
                bad.append((note, entry, options, args, want, got))
    finally:
        set_options(lib, {})
    assert not bad, f"{len(bad)} of {len(recorded)} calls differ, first: {bad[:3]}"


def test_a_refusal_leaves_its_text_and_an_accepted_call_leaves_the_last_error_alone():
    lib = _lib.load()
    set_options(lib, {})
    a = canonical("nt", (256, 256, 128, 0))
    assert plan(lib, dict(a, epilogue=7), 256) == "g3_gemm_bf16_nt: unknown epilogue 7"
    before = lib.g3_last_error()
    assert plan(lib, a, 256) == ["gemm_bf16_nt_w4_kernel<0, false>", 1, 0] and lib.g3_last_error() == before
    assert lib.g3_gemm_plan_bf16(C.byref(_lib.GemmCall(**a)), 256, None, None) == b"gemm_bf16_nt_w4_kernel<0, false>"  # the out-pointers are optional
    assert plan(lib, dict(a, entry=4), 256) == "g3_gemm_plan_bf16: unknown entry 4"
    # what an entry does not take is ignored: the qk entry has no gate / residual / epilogue, the plain one no statistics buffer
    q = canonical("qk", (256, 384, 128, 1))
    assert plan(lib, dict(q, gate=0x40004, gate_rows=3, ldg=5, residual=0x50004, ldr=5, epilogue=9, gn_stats=4, gn_rows=1), 256) == plan(lib, q, 256)
    assert plan(lib, dict(a, gn_stats=4, gn_rows=1, vt=4, B=0), 256) == plan(lib, a, 256)


def test_kernel_name_answers_as_before():
    lib = _lib.load()
    recorded = list(names())
    assert len(recorded) > 8000 and {-1, 5, 9} <= {r[4] for r in recorded}
    bad = []
    try:
        for options, M, N, K, e, want in recorded:
            set_options(lib, options)
            got = lib.g3_gemm_kernel_name(M, N, K, e).decode()
            if got != want:
                bad.append((options, M, N, K, e, got, want))
    finally:
        set_options(lib, {})
    assert not bad, f"{len(bad)} answers differ, first: {bad[:3]}"


def test_plan_agrees_with_the_name_function_on_canonical_operands():
    """Wherever the plain entry accepts a call with canonical operands, the dry run's row is of the family g3_gemm_kernel_name reports (n_cu 0: the
    device's count, which is what the name function uses - none on a CPU machine)."""
    lib = _lib.load()
    rows, _ = table()
    n = 0
    try:
        for options, M, N, K, e, _ in names():
            set_options(lib, options)
            got = plan(lib, canonical("nt", (M, N, K, e)), 0)
            if not isinstance(got, str):
                assert rows[got[0]] == lib.g3_gemm_kernel_name(M, N, K, e).decode(), (options, M, N, K, e, got)
                n += 1
    finally:
        set_options(lib, {})
    assert n > 1000


def test_kernel_table_has_one_row_per_instantiation():
    """The table is the one place on the host side that names the instantiations: its rows are exactly the fixture's kernels - the 65 kernel symbols of
    the parent's code object, which is what its launch sites named when the fixture was recorded -, the recorded calls reach every one, every row's family is one the name function knew, and no kernel template is named outside the table."""
    rows, src = table()
    assert len(rows) == 65 and sorted(rows) == sorted(FIXTURE["kernels"])
    reached = {r[0] for *_, want in calls() for r in want.values() if not isinstance(r, str)}
    assert reached == set(rows)
    assert {f for f in rows.values() if ", true, PIN>" not in f and "2, true>" not in f and "w4_conv" not in f} == set(FIXTURE["names"]["families"])
    host = src[src.index("/* ---- host side"):]
    kernels = {name.split("<")[0] for name in rows}
    assert len(kernels) == 5
    for k in kernels:  # once per family row of the table, and nowhere else in gemm.hip's host part or in the headers' host parts
        assert host.count(k) == 2 * host.count(f", {k}") > 0, k
    for header in ("gemm_w4.hpp", "gemm_w4e.hpp", "gemm_w4_conv.hpp"):
        text = (ROOT / "gen3c_amd" / "csrc" / header).read_text()
        assert "hipLaunchKernelGGL" not in text and "hipFuncSetAttribute" not in text, header


# ---- the bounds on how far an operand may lie: the kernel chosen one step below each, and at it ----------------------------------------------------------
LD_TILE_MAX = ((1 << 32) - 129) // 510 // 8 * 8  # the largest leading dimension (a multiple of 8) with 255 ld 2 + 128 < 2^32


def test_one_wave_kernels_only_where_a_tile_row_offset_fits_32_bits():
    """gemm_w4.hpp / gemm_w4e.hpp keep the LDS-DMA source of tile row r as the 32-bit byte offset r ld 2 + chunk 16, r <= 255, from the tile's first
    row: gemm_choose takes GK_W4_0 / GK_W4_PERSIST_0 and w4e_applies the deferred kernels only where 255 ld 2 + 128 < 2^32 for lda and for ldw;
    beyond, the call runs on the ping-pong kernel (64-bit row pointers) - under every option set that reached a one-wave kernel before."""
    lib = _lib.load()
    assert 255 * LD_TILE_MAX * 2 + 128 < 1 << 32 <= 255 * (LD_TILE_MAX + 8) * 2 + 128
    pp2 = "gemm_bf16_nt_pp_kernel<{e}, 2, false>"
    cases = [  # (options, canonical base, n_cu, kernel up to the bound)
        ({}, (257, 264, 192, 0), 256, "gemm_bf16_nt_w4_kernel<{e}, false>"),
        ({}, (257, 264, 192, 4), 256, "gemm_bf16_nt_w4_kernel<{e}, false>"),
        ({"gemm_persistent": 1}, (2048, 4096, 128, 0), 64, "gemm_bf16_nt_w4_kernel<{e}, true>"),
        ({}, (2048, 4096, 2432, 0), 64, "gemm_bf16_nt_w4e_kernel<{e}, true>"),
        ({"gemm_tokens_first": 0}, (2048, 4096, 2432, 2), 64, "gemm_bf16_nt_w4e_kernel<{e}, false>"),
        ({"gemm_deferred_grid": 8}, (2048, 4096, 2432, 1), 64, "gemm_bf16_nt_w4e_kernel<{e}, true>"),
    ]
    try:
        for options, base, n_cu, kernel in cases:
            set_options(lib, options)
            a, e = canonical("nt", base), base[3]
            for ld in ("lda", "ldw"):
                assert plan(lib, dict(a, **{ld: LD_TILE_MAX}), n_cu)[0] == kernel.format(e=e), (options, base, ld)
                assert plan(lib, dict(a, **{ld: LD_TILE_MAX + 8}), n_cu)[0] == pp2.format(e=e), (options, base, ld)
            assert plan(lib, dict(a, lda=LD_TILE_MAX, ldw=LD_TILE_MAX), n_cu)[0] == kernel.format(e=e)
        # the fused norm / RoPE entry exists on the one-wave kernel only: beyond the bound, the ping-pong kernel and the standalone passes
        set_options(lib, {})
        q = canonical("qk", (256, 384, 128, 2))
        assert plan(lib, dict(q, lda=LD_TILE_MAX), 256) == ["gemm_bf16_nt_w4_kernel<5, false>", 2, 0]
        assert plan(lib, dict(q, lda=LD_TILE_MAX + 8), 256) == ["gemm_bf16_nt_pp_kernel<0, 2, false>", 2, 3]  # then norm q, then norm k
    finally:
        set_options(lib, {})


def test_the_bound_reroutes_no_shape_of_the_benchmark_or_the_dit():
    """The block linears of the DiT bench.py measures (D = 4096, MLP 16 384, fused QKV 12 288, 56 320 tokens; 14 080 and 7040 under context
    parallelism), with dense operands and with A a column view of the widest buffer the model keeps (the MLP's 16 384 features): every one still gets
    the one-wave or the deferred kernel, none the ping-pong kernel the bound reroutes to. The widest row is 32 KiB, the bound 16 MiB - and for the
    recorded calls test_plan_equals_the_recorded_launcher shows every plan unchanged."""
    lib = _lib.load()
    assert LD_TILE_MAX == 8421504 and all(max(args.get("lda", 0), args.get("ldw", 0)) < LD_TILE_MAX // 64 for _, entry, _, args, _ in calls() if entry in ("nt", "qk"))
    linears = [(12288, 4096, 0), (4096, 4096, 2), (16384, 4096, 1), (4096, 16384, 2), (4096, 4096, 0), (8192, 1024, 0)]  # qkv, out, mlp up / down, cross q, cross kv
    try:
        set_options(lib, {})
        for M in (56320, 14080, 7040):
            for N, K, epi in linears:
                for lda in (K, 16384):
                    for n_cu in N_CU:
                        got = plan(lib, dict(canonical("nt", (M, N, K, epi)), lda=max(lda, K)), n_cu)
                        assert got[0].startswith(("gemm_bf16_nt_w4_kernel<", "gemm_bf16_nt_w4e_kernel<")), (M, N, K, epi, lda, n_cu, got)
    finally:
        set_options(lib, {})


def test_deferred_kernel_epilogue_strides_and_conv_spans_at_their_bounds():
    """w4e_applies: 8 ldc 2, 8 ldr 2 and 4 ldg 2 below 2^31 (the epilogue's 32-bit per-lane offsets), else the one-wave kernel. conv_w4_applies:
    ld_in 2 < 2^31, input rows < 2^31, N ldw 2 < 2^32 (the tap slab), else the ping-pong convolution."""
    lib = _lib.load()
    w4e, w4, cv, pp = "gemm_bf16_nt_w4e_kernel<2, true>", "gemm_bf16_nt_w4_kernel<2, false>", "gemm_bf16_nt_w4_conv_kernel<3>", "gemm_bf16_nt_pp_kernel<3, 2, true>"
    try:
        set_options(lib, {})
        a = canonical("nt", (2048, 4096, 2432, 2))
        for ld, bound in (("ldc", 1 << 27), ("ldr", 1 << 27), ("ldg", 1 << 28)):
            assert plan(lib, dict(a, **{ld: bound - 8}), 64)[0] == w4e, ld
            assert plan(lib, dict(a, **{ld: bound}), 64)[0] == w4, ld
        c = canonical("conv", (128, 128, 2, 16, 16, 1, 3, 3))
        assert plan(lib, dict(c, lda=(1 << 30) - 8), 256)[0] == cv and plan(lib, dict(c, lda=1 << 30), 256)[0] == pp
        assert plan(lib, dict(c, Ti=2047, Hi=1024, Wi=1024), 256)[0] == cv and plan(lib, dict(c, Ti=2048, Hi=1024, Wi=1024), 256)[0] == pp
        assert plan(lib, dict(c, ldw=(1 << 24) - 8), 256)[0] == cv and plan(lib, dict(c, ldw=1 << 24), 256)[0] == pp  # N = 128: 128 ldw 2 = 2^32
    finally:
        set_options(lib, {})
