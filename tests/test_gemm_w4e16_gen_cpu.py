"""CPU checks of the 16x16x32 body of gemm_bf16_nt_w4e_kernel (tools/gen_gemm_w4e16.py -> gen3c_amd/csrc/gemm_w4e16_gen.hpp), in the manner of
test_gemm_w4e_gen_cpu.py: the committed header is the generator's; drain -> pack -> X write -> transposing read -> store is the identity of the wave's
128 x 128 quadrant; every fragment register holds what v_mfma_f32_16x16x32_bf16 documents for it, read without a bank conflict; every accumulator sees
k in ascending chunks of 32 with C = 0 on the first; no fragment is overwritten or multiplied too early over whole tile lists; the per-gap budget of the
probe arm that decided for this body (profiles/gemm_mfma16_ab.txt) holds.

The tests restate three facts of gemm_w4e.hpp, which no CPU test can read out of the kernel: the LDS-DMA image (row r of a 256-row operand tile at byte
128 r, its 16-byte chunk c at position c ^ (r >> 1 & 7)), the narrow body's fragment address (row l & 15, position (l >> 4) ^ (row >> 1 & 7), ^ 4 for
the second K half, fragment f at + 2048 f) and the order of the statements in the tile loop. tests/test_gemm_mfma16_gpu.py checks them on the device."""
import importlib.util
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _gen():
    sys.path.insert(0, str(ROOT / "tools"))
    spec = importlib.util.spec_from_file_location("gen_gemm_w4e16", ROOT / "tools" / "gen_gemm_w4e16.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()
STATEMENTS = {name[len("gw4e16_"):]: ops for name, ops, _ in GEN.all_statements()}
# ds_read_b128 is served in four groups of 16 lanes (MI355X_MICROARCH.md, LDS table): within a group the 16-byte slots (address mod 256) must differ
SERVICE_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
SERVICE_GROUPS += [[l + 32 for l in g] for g in SERVICE_GROUPS]


def test_committed_header_is_up_to_date():
    assert GEN.OUT.read_text() == GEN.generate(), "gemm_w4e16_gen.hpp is stale: run python tools/gen_gemm_w4e16.py"


def test_the_wide_header_is_untouched_by_this_generator():
    spec = importlib.util.spec_from_file_location("gen_gemm_w4e", ROOT / "tools" / "gen_gemm_w4e.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.OUT.read_text() == mod.generate()


def test_layout_model_is_the_identity_of_the_quadrant():
    m = GEN.layout_model()
    assert len(m) == 128 * 128
    for (row, col), (tok, feat) in m.items():
        assert (row, col) == (tok, feat)


# ---------------------------------------------------------------------------------------------------------------- operand model
def _frag_reads(ops):
    """(operand, fragment, address operand, offset) of a statement's fragment reads."""
    out = []
    for op in ops:
        m = re.match(r"ds_read_b128 v\[(\d+):(\d+)\], %\[(adw|adt)\] offset:(\d+)", op.text)
        if m and int(m.group(1)) >= GEN.W0:
            lo = int(m.group(1))
            assert int(m.group(2)) == lo + 3 and lo % 4 == 0
            opd = "W" if lo < GEN.T0 else "T"
            assert m.group(3) == ("adw" if opd == "W" else "adt")
            out.append((opd, (lo - (GEN.W0 if opd == "W" else GEN.T0)) // 4, int(m.group(4))))
    return out


def _lane_addr(lane, half_wave_rows, khalf):
    """gemm_w4e.hpp, narrow body: adw / adt less the LDS base and the stage: the wave's 128 rows start at row half_wave_rows of the 256-row tile."""
    l15, c4 = lane & 15, lane >> 4
    return ((half_wave_rows + l15) * 128 + ((c4 ^ ((l15 >> 1) & 7)) << 4)) ^ (khalf << 6)


def _image_at(byte):
    """LDS-DMA image of one operand tile (32 KiB): byte -> (tile row, k of the K tile) of the bf16 it holds."""
    r, pos, e = byte // 128, (byte % 128) // 16, (byte % 16) // 2
    return r, 8 * (pos ^ ((r >> 1) & 7)) + e


def test_fragment_registers_hold_the_documented_operand_and_reads_are_conflict_free():
    """v_mfma_f32_16x16x32_bf16 (cdna_hip_programming.md, section 3): lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15]
    in element j of its fragment. Weight fragment f of K half h must therefore hold rows 16 f + (l & 15) of the wave's 128 feature rows, k = 32 h + 8 (l >> 4) + j
    - the same for the token fragments - in every statement, for both wave halves (the stage is a constant on the address)."""
    seen = set()
    for name, ops in STATEMENTS.items():
        ks = int(re.search(r"(?:ks|_k)(\d+)", name).group(1)) & 3
        khalf = GEN.READ_KHALF[ks][1]
        for opd, f, off in _frag_reads(ops):
            seen.add((ks, opd, f))
            base_off = off - (GEN.T_OFF if opd == "T" else 0)
            assert 0 <= base_off < GEN.T_OFF
            for half in (0, 128):
                addrs = [_lane_addr(lane, half, khalf) + base_off for lane in range(64)]
                for lane, a in enumerate(addrs):
                    assert a % 16 == 0 and a + 16 <= GEN.T_OFF
                    for j in range(8):
                        assert _image_at(a + 2 * j) == (half + 16 * f + (lane & 15), 32 * khalf + 8 * (lane >> 4) + j), (name, opd, f, lane, j)
                for grp in SERVICE_GROUPS:
                    assert len({(addrs[lane] % 256) // 16 for lane in grp}) == 16, (name, opd, f)
    # every fragment of both operands in both K halves is read somewhere in a K tile
    assert {(opd, f, GEN.READ_KHALF[ks][1]) for ks, opd, f in seen} == {(opd, f, h) for opd in "WT" for f in range(8) for h in range(2)}


# ---------------------------------------------------------------------------------------------------------------- program order over tile lists
def _tile_statements(carry, epi, nk, has_next):
    """The statements of one output tile in the order gemm_w4e.hpp issues them (nk K tiles of four statements; epi names the carried epilogue)."""
    plain = ["ks0", "ks1", "ks2_bar", "ks3"]
    if carry:
        seq = ["ks0_init", "ks1_pre", "ks2_bar", "ks3"]
        for u in range(8):
            seq += [f"{epi}_k{k}" if not (u == 0 and k == 2) else f"{epi}_k2f" for k in range(16)]
        seq += ["ks0", "ks1", "ks2_bar_store3", "ks3"] + plain
        t = 35
    else:
        seq = ["ks0_init", "ks1_init", "ks2_bar", "ks3"]
        t = 1
    while t + 3 < nk:
        seq += plain + plain
        t += 2
    seq += ["ks0", "ks1", "ks2_bar", "ks3_gate" if epi == "gated" else "ks3"]
    seq += plain + plain if has_next else ["ks0", "ks1", "ks2_bar", "ks3_nodma", "ks0_nodma", "ks1_nodma", "ks2_nobar", "ks3_last"]
    assert len(seq) == 4 * nk
    return seq


def _walk(tiles):
    """Runs the generated streams in program order over a list of output tiles [(carry, epi, nk, has_next)]: an in-order LDS queue retired by the
    lgkmcnt waits, the contents of the 16 fragments, and per accumulator block the K chunks it has seen. Asserts, per MFMA: both fragments have landed
    (no read of them in flight), they hold the operand rows and the K chunk the MFMA is due, C = 0 exactly on an output tile's first chunk."""
    # the kernel's prologue reads W0-3 and T0-3 of K tile 0, K half 0, and the first statement opens with lgkmcnt(0)
    content = {(opd, f): (0, 0) for opd in "WT" for f in range(4)}
    queue = []  # LDS operations in flight, oldest first: (fragment or None, content)
    n_mfma = 0
    kt = 0  # K tiles since the kernel began: the stage is kt & 1, and a read "one K tile ahead" fetches K tile kt + 1 whatever output tile it belongs to
    for carry, epi, nk, has_next in tiles:
        seen = {}
        for si, name in enumerate(_tile_statements(carry, epi, nk, has_next)):
            ks = si & 3
            assert int(re.search(r"(?:ks|_k)(\d+)", name).group(1)) & 3 == ks, name
            first_chunk = si < 2  # the K = 32 step that starts an output tile spans its first two statements
            for op in STATEMENTS[name]:
                if op.kind == "lds":
                    fr = _frag_reads([op])
                    if fr:
                        ahead, h = GEN.READ_KHALF[ks]
                        queue.append(((fr[0][0], fr[0][1]), (kt + ahead, h)))
                    else:
                        queue.append((None, None))
                elif op.kind == "wait":
                    m = re.search(r"lgkmcnt\((\d+)\)", op.text)
                    n = int(m.group(1)) if m else 0  # the barrier's wait (macro GW4E_BARWAIT_n) is lgkmcnt(0)
                    assert m or "BARWAIT" in op.text
                    while len(queue) > n:
                        frag, what = queue.pop(0)
                        if frag:
                            content[frag] = what
                elif op.kind == "mfma":
                    m = re.match(r"v_mfma_f32_16x16x32_bf16 a\[(\d+):(\d+)\], v\[(\d+):\d+\], v\[(\d+):\d+\], (0|a\[(\d+):\d+\])$", op.text)
                    blk, wf, tf = int(m.group(1)) // 4, (int(m.group(3)) - GEN.W0) // 4, (int(m.group(4)) - GEN.T0) // 4
                    assert int(m.group(2)) == 4 * blk + 3 and (m.group(5) == "0" or int(m.group(6)) == 4 * blk)
                    assert (wf, tf) == (blk >> 3, blk & 7), "block (I, J) multiplies weight fragment I by token fragment J"
                    for frag in (("W", wf), ("T", tf)):
                        assert all(q[0] != frag for q in queue), f"{name}: MFMA reads {frag} with a read of it in flight"
                        assert content.get(frag) == (kt, GEN.KHALF[ks]), f"{name}: {frag} holds {content.get(frag)}, due {(kt, GEN.KHALF[ks])}"
                    chunks = seen.setdefault(blk, [])
                    assert (m.group(5) == "0") == (not chunks) == first_chunk, f"{name}: C = 0 exactly on the block's first K chunk"
                    chunks.append(2 * (si >> 2) + GEN.KHALF[ks])
                    n_mfma += 1
            if ks == 3:
                kt += 1
        assert len(seen) == 64 and all(c == list(range(2 * nk)) for c in seen.values()), "every block: K chunks 0 .. 2 nk - 1 in ascending order"
    return n_mfma


def test_k_order_c_zero_and_fragment_liveness_over_tile_lists():
    """Tile lists as the launches make them: a workgroup's first tile carries nothing, every further one carries the epilogue of the tile before;
    the minimum of 38 K tiles and a longer, even count; every epilogue class; one, two and three tiles per workgroup."""
    for epi in ("none", "gelu", "gated"):
        for nk in (38, 40, 64):
            assert _walk([(False, epi, nk, False)]) == 128 * nk
            assert _walk([(False, epi, nk, True), (True, epi, nk, False)]) == 2 * 128 * nk
        assert _walk([(False, epi, 38, True), (True, epi, 38, True), (True, epi, 38, False)]) == 3 * 128 * 38


def test_walk_catches_a_read_that_lands_too_early():
    """The walk is not vacuous: reading K half 1's T4-7 one quadrant earlier (in the quadrant that still multiplies the old T4-7) must fail it."""
    ops = STATEMENTS["ks1"]
    idx = [i for i, op in enumerate(ops) if op.kind == "lds" and _frag_reads([op]) and _frag_reads([op])[0][0] == "T"]
    first_w = min(i for i, op in enumerate(ops) if op.kind == "lds" and _frag_reads([op]) and _frag_reads([op])[0][0] == "W")
    moved = list(ops)
    for i in reversed(idx):
        moved.insert(first_w, moved.pop(i))
    STATEMENTS["ks1"] = moved
    try:
        try:
            _walk([(False, "none", 38, False)])
        except AssertionError:
            return
        raise AssertionError("the walk accepted T4-7 overwritten under the quadrant that multiplies it")
    finally:
        STATEMENTS["ks1"] = ops


def test_every_statement_keeps_its_32_mfmas_and_the_gap_budget():
    """The probe arm that went "go" (tools/mfma_shape_probe.hip, section c) had at most 2 instructions between two 16-cycle MFMAs, the s_waitcnt at a quadrant's
    head not counted: GAP_BUDGET. Checked on the generator's statements, which the committed header is (first test), and every one of which the header
    defines; the barrier statement carries its wait + barrier behind the last MFMA."""
    assert GEN.GAP_BUDGET == 2
    defined = re.findall(r"G3_DEVICE void gw4e16_(\w+)\(const GW4EOps& o\) \{\n(?:    uint32_t [^\n]*\n)?    asm volatile\(GW16_S\d+\(", GEN.OUT.read_text())
    assert sorted(defined) == sorted(STATEMENTS) and len(STATEMENTS) == 14 + 3 * 17
    assert sum(1 for n in STATEMENTS if re.search(r"^(none|gelu|gated)_k\d+$", n)) == 48
    for name, ops in STATEMENTS.items():
        idx = [i for i, op in enumerate(ops) if op.kind == "mfma"]
        assert len(idx) == 32 and all(ops[i].text.startswith("v_mfma_f32_16x16x32_bf16 ") for i in idx), name
        assert ops[0].kind == "wait" and idx[0] == 1, name
        for k in range(31):
            gap = [op for op in ops[idx[k] + 1:idx[k + 1]] if not (k == 15 and op.tag == "qhead")]  # (the second quadrant's head)
            assert len(gap) <= GEN.GAP_BUDGET, (name, k, [op.text for op in gap])


def test_skeleton_macros_hold_the_mfmas_and_reads_the_statements_are_made_of():
    """The header writes a statement as a skeleton macro + 32 gap arguments. Expanding the macros by hand here would restate the preprocessor; instead: every
    skeleton has 32 MFMA macro calls and 32 parameters used once each, in order, and each statement passes exactly 32 arguments."""
    text = GEN.OUT.read_text()
    skels = re.findall(r"#define (GW16_S\d+)\(([^)]*)\) \\\n(.*?)\n\n", text, re.S)
    assert skels
    for name, params, body in skels:
        assert params.split(", ") == [f"g{g}" for g in range(32)]
        assert len(re.findall(r"GW16_M0?\(", body)) == 32, name
        assert re.findall(r"\bg(\d+)\b", body) == [str(g) for g in range(32)], name
    for call in re.findall(r"asm volatile\(GW16_S\d+\(\n(.*?)\n        \)\n", text, re.S):
        depth, commas = 0, 0
        for ch in re.sub(r'"[^"]*"', '""', call):
            depth += (ch == "(") - (ch == ")")
            commas += ch == "," and depth == 0
        assert commas == 31
