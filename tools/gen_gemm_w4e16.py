"""Generator of gen3c_amd/csrc/gemm_w4e16_gen.hpp: the instruction streams of gemm_bf16_nt_w4e_kernel (csrc/gemm_w4e.hpp) with the K loop on
v_mfma_f32_16x16x32_bf16 (g3_set_option("gemm_mfma16", 1)). Everything that is not the core of a K step, the drain or the X write comes from
tools/gen_gemm_w4e.py unchanged: the epilogue micro-ops, the piece order, the barrier step, the flush. The statements keep their names (gw4e16_<name>
for gw4e_<name>) and their place in the tile loop, so gemm_w4e.hpp runs either body from the same call sites.

Why: the chip holds a higher clock under the narrow shape (profiles/gemm_mfma16_ab.txt: the probe arm of tools/mfma_shape_probe.hip, +7.8 % by wall at
3.3 % more cycles), and one 16x16x32 rounds like two chained 32x32x16 (profiles/mfma_shape_probe.txt, a), so the bits stay.

Registers: a[0:255]   block (I, J) = features 16 I .., tokens 16 J .. at a[4 (8 I + J) : +3]; lane l holds token l & 15, features 4 (l >> 4) + r
           v[192:223] weight fragments W0..W7 (16 feature rows each), v[224:255] token fragments T0..T7: ONE K = 32 step, no second buffer
           v[56:191]  as gen_gemm_w4e.py
A K tile of 64 is two K = 32 steps of four QUADRANTS (4 x 4 blocks), two quadrants = 32 MFMAs per statement (the time of the wide body's 16):
   statement       0            1            2 (barrier)   3
   quadrants       00  01       11  10       01  00        10  11          (feature half, token half)
   K half          0   0        0   0        1   1         1   1
   reads (4 each)  T4-7 W4-7    W0-3' T4-7'  T0-3' W4-7'   W0-3" T0-3"     ' = K half 1 of this K tile, " = K half 0 of the next one (other stage)
Every read lands in the four fragments whose last reader was the quadrant before it, and is first used one quadrant (T4-7, T0-3') or two later. Per output
element k ascends: K half 0 then 1 of every K tile, 32 k per MFMA; the first two statements of an output tile multiply into C = 0.
A fragment: lane l reads row l & 15, 16-byte chunk (l >> 4) + 4 half of the operand image (128-byte rows, chunk ^ (row >> 1 & 7)): fragment f at offset 2048 f,
the K half is ^ 64 on the address (gemm_w4e.hpp: adw / adt of the narrow body).

Gaps: 32 per statement, 16 cycles each. Budget: at most GAP_BUDGET = 2 instructions in a gap (the probe arm that went "go" had 2), the s_waitcnt at a
quadrant's head not counted. Pinned ops of the wide body's gap p sit in gap 2 p (2 p + 1 for those that go behind the spread ops).

The header is written compactly: a K step's 32 MFMAs, fragment reads and operand pieces are one SKELETON macro per distinct layout (ten of them), a
statement is the skeleton plus what it adds per gap, the epilogue arithmetic is one macro per instruction. The compiled assembly is the one of the
statements written out line by line.

usage: python tools/gen_gemm_w4e16.py [--check]"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_gemm_w4e as w  # noqa: E402
from gen_gemm_w4e import EPI_GATED, EPI_GELU, EPI_NAME, EPI_NONE, G0, P0, T_OFF, Op  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "gen3c_amd" / "csrc" / "gemm_w4e16_gen.hpp"

W0, T0 = 192, 224
NGAPS = 32
GAP_BUDGET = 2
QUADS = {0: [(0, 0), (0, 1)], 1: [(1, 1), (1, 0)], 2: [(0, 1), (0, 0)], 3: [(1, 0), (1, 1)]}  # statement -> its two quadrants (feature half, token half)
READS = {0: [("T", 4), ("W", 4)], 1: [("W", 0), ("T", 4)], 2: [("T", 0), ("W", 4)], 3: [("W", 0), ("T", 0)]}  # statement -> per quadrant (operand, first fragment)
KHALF = {0: 0, 1: 0, 2: 1, 3: 1}  # K half the statement multiplies
READ_KHALF = {0: (0, 0), 1: (0, 1), 2: (0, 1), 3: (1, 0)}  # statement -> (K tile ahead, K half) its reads fetch: the fragment addresses gemm_w4e.hpp hands it
MID_WAIT = (0, 2)  # statements whose second quadrant multiplies what their first one read


def wfrag(f: int) -> str:
    return f"v[{W0 + 4 * f}:{W0 + 4 * f + 3}]"


def tfrag(f: int) -> str:
    return f"v[{T0 + 4 * f}:{T0 + 4 * f + 3}]"


def accblk(I: int, J: int) -> str:
    b = 4 * (8 * I + J)
    return f"a[{b}:{b + 3}]"


def mfma(I: int, J: int, init: bool) -> str:
    return f"v_mfma_f32_16x16x32_bf16 {accblk(I, J)}, {wfrag(I)}, {tfrag(J)}, {'0' if init else accblk(I, J)}"


def quad_order(fh: int, th: int) -> list[tuple[int, int]]:
    return [(4 * fh + i, 4 * th + j) for i in range(4) for j in range(4)]


def frag_read(opd: str, f: int, tag: str) -> Op:
    if opd == "W":
        return Op(f"ds_read_b128 {wfrag(f)}, %[adw] offset:{2048 * f}", "lds", tag=tag)
    return Op(f"ds_read_b128 {tfrag(f)}, %[adt] offset:{T_OFF + 2048 * f}", "lds", tag=tag)


def base_layout(ks: int, read: bool, np_: int) -> list[list[Op]]:
    """The fragment reads (gaps 0..3 of each quadrant) and the operand LDS-DMA pieces of the wide body's K step ks, one gap later than twice the wide gap:
    gap 0 stays free for the residual word's read."""
    gaps: list[list[Op]] = [[] for _ in range(NGAPS)]
    if read:
        for q, (opd, f0) in enumerate(READS[ks]):
            for n in range(4):
                gaps[16 * q + n].append(frag_read(opd, f0 + n, f"fr{4 * q + n}"))
    if np_ == 5:
        for q, (gm, gl) in enumerate(((0, 1), (3, 4), (6, 7), (9, 10), (12, 13))):
            gaps[2 * gm + 1].append(w.dma_m0(q))
            gaps[2 * gl + 1].append(w.dma_ld(q, ("F" if q < 2 else "S") if ks == 0 else "S"))
    elif np_ == 6:
        for q, (gm, gl) in enumerate(((0, 1), (3, 4), (5, 6), (8, 9), (11, 12), (13, 14))):
            gaps[2 * gm + 1].append(w.dma_m0(q))
            gaps[2 * gl + 1].append(w.dma_ld(q, "F"))
    elif np_ != 0:
        raise ValueError(np_)
    for gap in gaps:
        for op in gap:
            op.base = True  # part of the K step's skeleton (generate())
    return gaps


def spread(gaps: list[list[Op]], ops: list[Op]) -> None:
    """gen_gemm_w4e.spread over 32 gaps: pinned ops at twice their wide gap, the others in order, water-filled."""
    for op in ops:
        if op.pin is not None and not op.last:
            gaps[2 * op.pin].append(op)
    free = [op for op in ops if op.pin is None]
    tail = [op for op in ops if op.pin is not None and op.last]
    g = 0
    if free:
        load = [len(x) for x in gaps]
        level = 0
        while sum(max(0, level - x) for x in load) < len(free):
            level += 1
        room = max(0, level - load[0])
        for op in free:
            while room == 0:
                g += 1
                room = max(0, level - load[g])
            gaps[g].append(op)
            room -= 1
    for op in tail:
        assert 2 * op.pin + 1 >= g, "a trailing pinned op would overtake the ops it depends on"
        gaps[2 * op.pin + 1].append(op)


def assemble_ops(ks: int, init: bool, gaps: list[list[Op]], bar: bool, read: bool = True, trailing: int = 0) -> list[Op]:
    seq: list[Op] = [Op("s_waitcnt lgkmcnt(0)", "wait", tag="qhead")]
    order = quad_order(*QUADS[ks][0]) + quad_order(*QUADS[ks][1])
    for g, (I, J) in enumerate(order):
        if g == 16 and read and ks in MID_WAIT:
            seq.append(Op("s_waitcnt lgkmcnt(@fr3)", "wait", tag="qhead"))
        seq.append(Op(mfma(I, J, init), "mfma"))
        assert len(gaps[g]) <= GAP_BUDGET, f"K step {ks}: {len(gaps[g])} instructions in gap {g}"
        seq.extend(gaps[g])
    if bar:
        seq.append(Op(f"@GW4E_BARWAIT_{trailing}", "wait"))
        seq.append(Op("s_barrier", "salu"))
    w.fix_waits(seq)
    w.check_m0_pairs(seq)
    w.check_trans(seq)
    return seq


def assemble(*a, **k) -> list[str]:
    return [w.ab_text(op) for op in assemble_ops(*a, **k)]


def emit_fn(name: str, texts: list[str], comment: str = "") -> str:
    return w.emit_fn(name, texts, comment)


# (name, K step, C = 0, reads, pieces, barrier): gen_gemm_w4e.gen_plain's list + K step 1 of an output tile's first K tile (its quadrants start at C = 0 too)
PLAIN = [
    ("ks0", 0, False, True, 5, False), ("ks0_init", 0, True, True, 5, False), ("ks1", 1, False, True, 5, False), ("ks1_init", 1, True, True, 5, False),
    ("ks2_bar", 2, False, True, 0, True), ("ks3", 3, False, True, 6, False),
    ("ks3_nodma", 3, False, True, 0, False), ("ks0_nodma", 0, False, True, 0, False), ("ks1_nodma", 1, False, True, 0, False),
    ("ks2_nobar", 2, False, True, 0, False), ("ks3_last", 3, False, False, 0, False),
]


def plain_statements() -> list[tuple[str, list[Op], str]]:
    out = []
    for name, ks, init, read, np_, bar in PLAIN:
        gaps = base_layout(ks, read, np_)
        if bar:
            spread(gaps, w.prefetch_ops())
        out.append((f"gw4e16_{name}", assemble_ops(ks, init, gaps, bar, read=read), f"plain K step {ks}" + (" (first K tile of an output tile: C = 0)" if init else "") + (", barrier" if bar else "")))
    gaps = base_layout(2, True, 0)
    spread(gaps, [w.store_chunk(3, pin=14)] + w.prefetch_ops())
    out.append(("gw4e16_ks2_bar_store3", assemble_ops(2, False, gaps, True, trailing=1), "plain K step 2 + store of W[12:15] (chunk 3 of the last unit), barrier"))
    gaps = base_layout(1, True, 5)
    spread(gaps, [Op(w.x_read(ch).text, "lds", pin=8 + 2 * ch, ab="L") for ch in range(4)])
    out.append(("gw4e16_ks1_pre", assemble_ops(1, True, gaps, False), "preamble K tile (C = 0), K step 1: + transposing reads of unit 0 (chunks 0..3) into W"))
    gaps = base_layout(3, True, 6)
    spread(gaps, [Op(f"global_load_dwordx4 v[{G0}:{G0 + 3}], %[goff], %[gb0]", "vmem", pin=2), Op(f"global_load_dwordx4 v[{G0 + 4}:{G0 + 7}], %[goff], %[gb1]", "vmem", pin=7)])
    out.append(("gw4e16_ks3_gate", assemble_ops(3, False, gaps, False), "K step 3 + the two gate vector loads (certified by the next barrier's vmcnt(0))"))
    return out


def carry_statements(epi: int) -> list[tuple[str, list[Op], str]]:
    out = []
    for kappa in range(16):
        ks = kappa & 3
        gaps = base_layout(ks, True, (5, 5, 0, 6)[ks])
        ops, trailing = w.carry_ops(epi, kappa)
        spread(gaps, ops + (w.prefetch_ops() if ks == 2 else []))
        out.append((f"gw4e16_{EPI_NAME[epi]}_k{kappa}", assemble_ops(ks, False, gaps, ks == 2, trailing=trailing),
                    f"{EPI_NAME[epi]}: period K step kappa = {kappa} (K step {ks}" + (", barrier" if ks == 2 else "") + ")"))
    gaps = base_layout(2, True, 0)
    ops, trailing = w.carry_ops(epi, 2, store=False)
    spread(gaps, ops + w.prefetch_ops())
    out.append((f"gw4e16_{EPI_NAME[epi]}_k2f", assemble_ops(2, False, gaps, True, trailing=trailing), f"{EPI_NAME[epi]}: period K step kappa = 2 of unit 0 (no store), barrier"))
    return out


def all_statements() -> list[tuple[str, list[Op], str]]:
    out = plain_statements()
    for epi in (EPI_NONE, EPI_GELU, EPI_GATED):
        out += carry_statements(epi)
    return out


# ---- drain and X write. Unit u (token block u >> 1 of 32, feature half u & 1 of 64) = blocks (I = 4 (u & 1) + fi, J = 2 (u >> 1) + jt); its register
# P[16 u + 4 fi + 2 jt + h] holds features 16 I + 4 (l >> 4) + 2 h, + 1 of token 16 J + (l & 15).
def p_reg(u: int, fi: int, jt: int, h: int) -> int:
    return P0 + 16 * u + 4 * fi + 2 * jt + h


def drain_texts() -> list[str]:
    texts = ["s_nop 7", "s_nop 3"]
    tmp = [W0 + 16 + k for k in range(4)]  # W4: free behind the last K step (W0-3 and T0-3 hold the next tile's first fragments)
    n = 0
    for u in range(8):
        for fi in range(4):
            for jt in range(2):
                for h in range(2):
                    a = 4 * (8 * (4 * (u & 1) + fi) + 2 * (u >> 1) + jt) + 2 * h
                    pr, t = p_reg(u, fi, jt, h), tmp[n & 3]
                    n += 1
                    texts += [f"v_accvgpr_read_b32 v{pr}, a{a}", f"v_accvgpr_read_b32 v{t}, a{a + 1}", f"v_cvt_pk_bf16_f32 v{pr}, v{pr}, v{t}"]
    return texts


def xwrite_texts(u: int) -> list[str]:
    """Lane (l15 = l & 15, c = l >> 4) writes features 16 fi + 4 c .. + 3 of row 16 jt + l15 of X ([32 rows][128 B], 16-byte chunk ^ row & 7): %[xw] is the
    address of (fi, jt) = (0, 0); fi is ^ 32 fi on it (chunk 2 fi + (c >> 1)), jt is + 2048."""
    texts = []
    for fi in range(4):
        ad = "%[xw]"
        if fi:
            ad = "%[xt]" if fi & 1 else "%[xu]"
            texts.append(f"#L#v_xor_b32 {ad}, {32 * fi}, %[xw]")
        for jt in range(2):
            r = p_reg(u, fi, jt, 0)
            texts.append(f"#L#ds_write_b64 {ad}, v[{r}:{r + 1}]" + (f" offset:{2048 * jt}" if jt else ""))
    return texts


HEADER = """// GENERATED by tools/gen_gemm_w4e16.py - do not edit; tests/test_gemm_w4e16_gen_cpu.py checks that it is up to date.
// gemm_bf16_nt_w4e_kernel's K loop on v_mfma_f32_16x16x32_bf16 (gemm_mfma16 = 1): the statements of gemm_w4e_gen.hpp whose MFMAs, fragment reads, drain or
// X write differ, under the names gw4e16_<name>. See the generator for the schedule. Included behind gemm_w4e_gen.hpp.
//
// A statement is a SKELETON - its 32 MFMAs with what every statement of that K step carries in the same gaps: the eight fragment reads and the operand LDS-DMA
// pieces - and, as the skeleton macro's 32 arguments, what this statement adds to each gap (epilogue micro-ops, the second quadrant's lgkmcnt wait in front of
// MFMA 16, the barrier behind MFMA 31). Argument g goes behind the skeleton's own instructions of gap g.

#define GW16_M(a0, a1, w0, w1, t0, t1) "v_mfma_f32_16x16x32_bf16 a[" #a0 ":" #a1 "], v[" #w0 ":" #w1 "], v[" #t0 ":" #t1 "], a[" #a0 ":" #a1 "]\\n\\t"
#define GW16_M0(a0, a1, w0, w1, t0, t1) "v_mfma_f32_16x16x32_bf16 a[" #a0 ":" #a1 "], v[" #w0 ":" #w1 "], v[" #t0 ":" #t1 "], 0\\n\\t"
#define GW16_RW(r0, r1, off) "ds_read_b128 v[" #r0 ":" #r1 "], %[adw] offset:" #off "\\n\\t"
#define GW16_RT(r0, r1, off) "ds_read_b128 v[" #r0 ":" #r1 "], %[adt] offset:" #off "\\n\\t"
#define GW16_D(p, t, a0, a1) "v_accvgpr_read_b32 v" #p ", a" #a0 "\\n\\tv_accvgpr_read_b32 v" #t ", a" #a1 "\\n\\tv_cvt_pk_bf16_f32 v" #p ", v" #p ", v" #t "\\n\\t"
#define GW16_P(q) "s_mov_b32 m0, %[m" #q "]\\n\\t"
#define GW16_L(q, cpol) "global_load_lds_dwordx4 %[vo" #q "], %[sb" #q "]" cpol "\\n\\t"

"""

LINE = 168  # width the statements' arguments are packed to


EPI_MACROS: dict = {}  # epilogue arithmetic instruction, its literal v registers left open -> (macro name, definition)


def render(text: str) -> str:
    """One instruction as a C string-literal expression (gen_gemm_w4e.emit_fn's forms: @MACRO, #ablation class#text, text@@cache-policy role). The epilogue
    arithmetic (class M), the same instructions in every period statement but for the register they work on, goes through one macro per instruction:
    GW16_E<n>(register numbers)."""
    import re
    if text.startswith("@"):
        return text[1:]
    if text.startswith("#"):
        _, cls, txt = text.split("#", 2)
        if cls != "M":
            return f'GW4E_AB_{cls}("{txt}\\n\\t")'
        regs = re.findall(r"\bv(\d+)\b", txt)
        n = iter(range(len(regs)))
        tmpl = re.sub(r"\bv\d+\b", lambda m: f'v" #r{next(n)} "', txt)
        if tmpl not in EPI_MACROS:
            name = f"GW16_E{len(EPI_MACROS)}"
            params = "(" + ", ".join(f"r{k}" for k in range(len(regs))) + ")" if regs else ""
            EPI_MACROS[tmpl] = (name, f'#define {name}{params} GW4E_AB_M("{tmpl}\\n\\t")')
        name = EPI_MACROS[tmpl][0]
        return name + ("(" + ", ".join(regs) + ")" if regs else "")
    if "@@" in text:
        txt, role = text.split("@@")
        return f'"{txt}" GW4E_CPOL_{role} "\\n\\t"'
    return f'"{text}\\n\\t"'


def render_base(text: str) -> str:
    """An instruction of a skeleton through the short macros above (the same characters as render() gives)."""
    import re
    m = re.match(r"v_mfma_f32_16x16x32_bf16 a\[(\d+):(\d+)\], v\[(\d+):(\d+)\], v\[(\d+):(\d+)\], (0|a\[\d+:\d+\])$", text)
    if m:
        return f"GW16_M{'0' if m.group(7) == '0' else ''}({', '.join(m.group(k) for k in range(1, 7))})"
    m = re.match(r"ds_read_b128 v\[(\d+):(\d+)\], %\[ad([wt])\] offset:(\d+)$", text)
    if m:
        return f"GW16_R{m.group(3).upper()}({m.group(1)}, {m.group(2)}, {m.group(4)})"
    m = re.match(r"s_mov_b32 m0, %\[m(\d)\]$", text)
    if m:
        return f"GW16_P({m.group(1)})"
    m = re.match(r"global_load_lds_dwordx4 %\[vo(\d)\], %\[sb\1\]@@([FS])$", text)
    if m:
        return f"GW16_L({m.group(1)}, GW4E_CPOL_{m.group(2)})"
    raise ValueError(text)


def split_statement(ops: list[Op]):
    """-> (skeleton key: per gap the MFMA and the base ops behind it, per gap the other ops' rendered texts). The head wait belongs to the skeleton; the wait in
    front of MFMA 16 and the barrier's wait + barrier are the statement's (arguments 15 and 31)."""
    assert ops[0].text == "s_waitcnt lgkmcnt(0)"
    skel, extra = [], []
    for op in ops[1:]:
        if op.kind == "mfma":
            skel.append([op.text])
            extra.append([])
        elif getattr(op, "base", False):
            assert not extra[-1], "a skeleton op behind a statement's own op of the same gap"
            skel[-1].append(w.ab_text(op))
        else:
            extra[-1].append(render(w.ab_text(op)))
    assert len(skel) == NGAPS
    return tuple(tuple(g) for g in skel), extra


def drain_macro(rd0: str, rd1: str, cvt: str) -> str:
    """GW16_D(p, t, a): v_accvgpr_read_b32 vp, a<a>; v_accvgpr_read_b32 vt, a<a + 1>; v_cvt_pk_bf16_f32 vp, vp, vt"""
    import re
    p_, a0 = re.match(r"v_accvgpr_read_b32 v(\d+), a(\d+)$", rd0).groups()
    t_, a1 = re.match(r"v_accvgpr_read_b32 v(\d+), a(\d+)$", rd1).groups()
    assert cvt == f"v_cvt_pk_bf16_f32 v{p_}, v{p_}, v{t_}" and int(a1) == int(a0) + 1
    return f"GW16_D({p_}, {t_}, {a0}, {a1})"


def pack(items: list[str], indent: str, sep: str = " ") -> list[str]:
    lines, cur = [], ""
    for it in items:
        if cur and len(indent) + len(cur) + len(sep) + len(it) > LINE:
            lines.append((indent + cur).rstrip())
            cur = it
        else:
            cur = (cur + sep + it) if cur else it
    if cur:
        lines.append((indent + cur).rstrip())
    return lines


def emit_statement(name: str, ops: list[Op], comment: str, skeletons: dict) -> str:
    key, extra = split_statement(ops)
    macro = skeletons.setdefault(key, f"GW16_S{len(skeletons)}")
    outs, ins = w.operand_lists([w.ab_text(op) for op in ops])
    temps = [o.split("(")[1].rstrip(")") for o in outs]
    args = [" ".join(e) + ("," if g < NGAPS - 1 else "") for g, e in enumerate(extra)]  # an empty argument is an empty gap
    body = [f"// {comment}", f"G3_DEVICE void {name}(const GW4EOps& o) {{"]
    if temps:
        body.append("    uint32_t " + ", ".join(temps) + ";")
    body.append(f"    asm volatile({macro}(")
    body += pack(args, "        ")
    body.append("        )")
    body.append(("        : " + ", ".join(outs)).rstrip())
    body += pack([i + "," for i in ins[:-1]] + ins[-1:], "        : ")[:1] + pack([i + "," for i in ins[:-1]] + ins[-1:], "          ")[1:] if ins else ["        :"]
    if any(op.text == "@GW4E_PFA" for op in ops):
        body[-1] += " GW4E_PF_OPERANDS"
    body.append('        : GW4E_OWNED, "memory");')
    if temps:
        body.append("    " + " ".join(f"(void){t};" for t in temps))
    body.append("}")
    return "\n".join(body) + "\n"


def emit_skeleton(macro: str, key) -> str:
    params = ", ".join(f"g{g}" for g in range(NGAPS))
    lines = [f"#define {macro}({params}) \\", '    "s_waitcnt lgkmcnt(0)\\n\\t" \\']
    for g, gap in enumerate(key):
        lines.append("    " + " ".join(render_base(t) for t in gap) + f" g{g}" + (" \\" if g < NGAPS - 1 else ""))
    return "\n".join(lines) + "\n"


def generate() -> str:
    EPI_MACROS.clear()
    parts = [HEADER]
    body = ["// drain: the 256 accumulators of the finished tile -> 128 packed bf16 registers v[64:191] (feature pairs; the Linear's own rounding to bf16)",
            "G3_DEVICE void gw4e16_drain() {", "    asm volatile("]
    dt = drain_texts()
    body += pack([f'"{t}\\n\\t"' for t in dt[:2]] + [drain_macro(*dt[k:k + 3]) for k in range(2, len(dt), 3)], "        ")
    body += ['        : : : GW4E_OWNED, "memory");', "}"]
    parts.append("\n".join(body) + "\n")
    for u in range(8):
        parts.append(emit_fn(f"gw4e16_xwrite_{u}", xwrite_texts(u), f"unit {u} (token block {u >> 1}, feature half {u & 1}): registers v[{P0 + 16 * u}:{P0 + 16 * u + 15}] -> LDS slice X"))
    skeletons: dict = {}
    fns = [emit_statement(name, ops, comment, skeletons) for name, ops, comment in all_statements()]
    parts.append("// the epilogue arithmetic, one macro per instruction (r<n>: the numbers of the v registers it names)\n" + "\n".join(d for _, d in EPI_MACROS.values()) + "\n")
    parts += [emit_skeleton(macro, key) for key, macro in skeletons.items()]
    parts += fns
    return "\n".join(parts)


# ---------------------------------------------------------------------------------------------------------------- models (tests)
def layout_model():
    """gen_gemm_w4e.layout_model for this body: every accumulator element of a wave quadrant through drain -> X write -> X read -> store; {(row, col): (token, feature)}."""
    import re
    acc_of = {}  # P register -> (accumulator of the low half, of the high half)
    tmp_src = {}
    for t in drain_texts():
        m = re.match(r"v_accvgpr_read_b32 v(\d+), a(\d+)", t)
        if m:
            tmp_src[int(m.group(1))] = int(m.group(2))
        m = re.match(r"v_cvt_pk_bf16_f32 v(\d+), v(\d+), v(\d+)", t)
        if m:
            assert m.group(1) == m.group(2)
            acc_of[int(m.group(1))] = (tmp_src[int(m.group(2))], tmp_src[int(m.group(3))])
    assert sorted(a for pair in acc_of.values() for a in pair) == list(range(256))

    def elem(a, lane):  # accumulator register a of lane -> (feature, token)
        blk, r = a >> 2, a & 3
        return 16 * (blk >> 3) + 4 * (lane >> 4) + r, 16 * (blk & 7) + (lane & 15)

    out = {}
    for u in range(8):
        xmem = {}
        for lane in range(64):
            l15, c = lane & 15, lane >> 4
            xw = l15 * 128 + (((c >> 1) ^ (l15 & 7)) << 4) + 8 * (c & 1)  # gemm_w4e.hpp: E.xw of the narrow body, less the slice base
            regs = {"xw": xw}
            for t in xwrite_texts(u):
                t = t.split("#", 2)[2]
                m = re.match(r"v_xor_b32 %\[(\w+)\], (\d+), %\[xw\]", t)
                if m:
                    regs[m.group(1)] = xw ^ int(m.group(2))
                    continue
                m = re.match(r"ds_write_b64 %\[(\w+)\], v\[(\d+):(\d+)\](?: offset:(\d+))?", t)
                addr = regs[m.group(1)] + int(m.group(4) or 0)
                for k, pr in enumerate((int(m.group(2)), int(m.group(3)))):
                    for e in range(2):
                        assert addr + 4 * k + 2 * e not in xmem
                        xmem[addr + 4 * k + 2 * e] = elem(acc_of[pr][e], lane)
        for lane in range(64):
            rr, c = lane >> 3, lane & 7
            xr = rr * 128 + ((c ^ rr) << 4)
            for ch in range(4):
                for e in range(8):
                    feat, tok = xmem[xr + 1024 * ch + 2 * e]
                    out[(32 * (u >> 1) + 8 * ch + rr, 64 * (u & 1) + 8 * c + e)] = (tok, feat)
    return out


def main():
    text = generate()
    if "--check" in sys.argv:
        if not OUT.exists() or OUT.read_text() != text:
            print(f"{OUT} is stale: run python tools/gen_gemm_w4e16.py")
            sys.exit(1)
        print("up to date")
        return
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")


if __name__ == "__main__":
    main()
