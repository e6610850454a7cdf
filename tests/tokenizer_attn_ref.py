"""Exact probes, fp64 references and torch restatements for the tokenizer's three attention entries (TEST INFRASTRUCTURE - a plain helper module;
tests/test_tokenizer_attn_ref_cpu.py checks it, tests/test_tokenizer_attn_kernels_gpu.py uses it).

1. g3_spatial_attn_d512_bf16 (csrc/attention_d512.hip). The probes of tests/attn_probe_ref.py at d = 512: Hd is the 512 x 512 Sylvester Hadamard
matrix, C = min(512, hw) classes, key j of every frame is Hd[j % C], query i of frame f is 2 Hd[(5 i + shift(f)) % C] (11 i where 5 divides C, so that the queries
visit every class) - a key of the query's class
scores 2 * 512 * scale, every other key exactly 0. Tensors are [frames, hw, 512] fp64 on the CPU holding bf16 values. V of frame f carries the gain
2^-(f % 4), an exact power of two, so that a frame reading another frame's V^T shows (K and the V pattern are the same in every frame).

The launch scale is SOFTMAX_SCALE_512 = 2^-5 / log2(e): its fp32 product with fp32(log2 e) is exactly 2^-5 (asserted on the CPU), a matching key
scores exactly 32 in the log2 domain. The kernel applies the scale in fp32 AFTER the MFMA (the scores of bf16-exact probes are exact integers in
fp32), so nothing is folded into Q and the default scale 512^-0.5 is a second family with references of its own scale (a match then scores 65.3).

 * census-position   V[j, d] = (d == j % 512): the expected row is one-hot at the query's class. A P fragment paired with the wrong V^T column of a
                     tile moves the 1; so does a wrong register-to-dim map of the epilogue (wave -> 128 dims, register r -> 32 db + (r & 3) + 8 (r >> 2) + 4 g).
 * census-block      V[j, d] = (d == j // C): every key owns one output element per query class (keys_all_owned).
 * uniform           q = 0, census-block V: the output is count_d / hw.
 * threshold census  census-position with q = 0.5 Hd[..]: a match scores exactly 8.0 in the log2 domain. A row whose first tile holds no match keeps
                     its reference point at 0 (8 > 0 + 8 is false) and its matches carry P = 2^8 exactly; a row whose first tile holds its match
                     sits at 8 with P = 1 and 2^-8. Both are exact, so the bar is the census bar: this pins the strict `>` of the rescale test from
                     the side that matters (P <= 2^8 stays exact) - moving AT the threshold (`>=`) gives the same exact values and is no defect.
 * staircase         q = 2 Hd[0], k_j = s_j Hd[0], log2-domain logit step * t for tile t = j // 64 (ascending or descending), V[j, d] = (d == j // 64):
                     output column d is the mass of tile d. s_j is rounded to bf16, the reference uses the rounded value. Step 8 ascending lands on
                     the threshold at every other tile, step 12 moves every tile, step 0.5 first exceeds 8 at its 18th tile (17 tiles: never).
 * mixed rows        the staircase with a per-row factor on q (MIXED_FACTORS, including 0): inside one 32-row group some rows move their maximum
                     in a tile in which others do not, and one 32-row group of a 128-row block moves where another does not - what the kernel's
                     per-row factor array and per-block flags exist for (the CPU test asserts both from emulate()'s trace).

reference() is the fp64 softmax of the bf16 inputs; emulate() restates the kernel's arithmetic in torch (64-key tiles, fp32 scores, the reference
point moves only on a jump > 8, P rounded to bf16 into P V, l summed from the unrounded P, fp32 accumulation, bf16 output) and takes ONE defect.

2. g3_temporal_attn_cl_bf16: temporal_reference() restates the reference's dtype chain (layers3d.py:386-427: bmm -> bf16 scores, * scale, causal
softmax, bf16 weights, bmm, bf16 output) in fp64; temporal_fp32() is the same chain in torch fp32. The probes use +-1 Hadamard rows (every score an
exact integer that bf16 holds, so the rounding of the score does not depend on the summation order) with per-pixel class shifts.

3. g3_softmax_rows_bf16: softmax_reference() = softmax(bf16 x * fp32 scale) in fp64."""
import math

import torch

from tests import attn_probe_ref as R
from tests.attn_probe_ref import REL_BF16, REL_EXACT_P, SMALL_OUT, SMALL_REF, bf16_exact, first_bad, hadamard, out_errors  # noqa: F401  (re-exported)
from tests.tokenizer_kernel_ref import bf16_round, bf16_ulp

D = 512
KVB = 64
QB = 128            # query rows of a workgroup
GROUP = 32          # query rows of a wave: one per-block flag, 32 per-row factors
RESCALE_THR = 8.0
A_STEP = 5
LOG2E = math.log2(math.e)
SCALE_LOG2_512 = 2.0 ** -5
SOFTMAX_SCALE_512 = SCALE_LOG2_512 / LOG2E   # fp32(SOFTMAX_SCALE_512) * fp32(log2 e) == 2^-5 exactly (asserted on the CPU)
DEFAULT_SCALE_512 = D ** -0.5
MATCH_LOG2_512 = 2.0 * D * SCALE_LOG2_512    # 32
STAIR_STEPS = (0.5, 4.0, 8.0, 12.0)
MIXED_FACTORS = ((0.0, 0.0, 0.0, 0.0), (0.0, 0.5, 1.0, 2.0), (2.0, 2.0, 2.0, 2.0), (1.0, 1.0, 0.5, 0.5))  # [32-row group % 4][row % 4]
MIXED_STAIRS = ((4.0, False), (4.0, True), (12.0, False))
C_GAUSS = 4.0       # the Gaussian bar 0.5 ulp + C_GAUSS E: 2 x emulate()'s worst (err - 0.5 ulp) / E, rounded up to a power of two (CPU test)
GAUSS_SHAPES = ((3, 320), (8, 192), (1, 1088))
U16 = 2.0 ** -16


def frame_shift(f):
    return R.shift(f, 0, 1)


def a_step(C):
    """the query class step: 5 as in tests/attn_probe_ref.py, 11 where 5 divides C (hw = 320) - coprime to C, so the queries of a frame visit every class"""
    a = A_STEP if C % A_STEP else 11
    assert math.gcd(a, C) == 1
    return a


def v_gain(f):
    return 2.0 ** -(f % 4)


def fp32_scale_log2(softmax_scale):
    return R.fp32_scale_log2(softmax_scale)


class Probe512:
    def __init__(self, name, q, k, v, q_class=None, C=None, exact=True, rel=REL_BF16):
        self.name, self.q, self.k, self.v, self.q_class, self.C, self.rel = name, q, k, v, q_class, C, rel
        self.F, self.hw = q.shape[:2]
        assert q.shape == k.shape == v.shape == (self.F, self.hw, D)
        for t in (q, k, v):
            assert not exact or bf16_exact(t), f"{name}: a probe tensor is not bf16-exact"


def _census_qk(F, hw, q_scale=2.0):
    Hd = hadamard(D)
    C = min(D, hw)
    i = torch.arange(hw)[None, :]
    sh = torch.tensor([frame_shift(f) for f in range(F)])[:, None]
    qc = (a_step(C) * i + sh) % C  # [F, hw]
    q = q_scale * Hd[qc]
    k = Hd[torch.arange(hw) % C][None].expand(F, hw, D).contiguous()
    return q, k, qc, C


def _onehot_v(F, hw, col):
    v = torch.zeros(hw, D, dtype=torch.float64)
    v[torch.arange(hw), col] = 1.0
    gain = torch.tensor([v_gain(f) for f in range(F)], dtype=torch.float64)
    return (gain[:, None, None] * v[None]).contiguous()


def census_position(F, hw):
    q, k, qc, C = _census_qk(F, hw)
    return Probe512("census-position", q, k, _onehot_v(F, hw, torch.arange(hw) % D), qc, C, rel=REL_EXACT_P)


def census_block(F, hw):
    q, k, qc, C = _census_qk(F, hw)
    return Probe512("census-block", q, k, _onehot_v(F, hw, torch.arange(hw) // C), qc, C, rel=REL_EXACT_P)


def uniform(F, hw):
    _q, k, _qc, C = _census_qk(F, hw)
    return Probe512("uniform", torch.zeros(F, hw, D, dtype=torch.float64), k, _onehot_v(F, hw, torch.arange(hw) // C), rel=REL_EXACT_P)


def threshold_census(F, hw):
    """a match scores RESCALE_THR exactly at SOFTMAX_SCALE_512 (module docstring); no leak check: a non-matching key weighs 2^-8 of a match"""
    q, k, qc, C = _census_qk(F, hw, q_scale=RESCALE_THR / (D * SCALE_LOG2_512))
    return Probe512("threshold census", q, k, _onehot_v(F, hw, torch.arange(hw) % D), None, C, rel=REL_EXACT_P)


def row_factors(hw):
    i = torch.arange(hw)
    return torch.tensor(MIXED_FACTORS, dtype=torch.float64)[(i // GROUP) % 4, i % 4]


def staircase(F, hw, step, descending, scale_log2=SCALE_LOG2_512, mixed=False):
    assert hw <= KVB * D
    Hd = hadamard(D)
    nt = (hw + KVB - 1) // KVB
    t = torch.arange(hw) // KVB
    if descending:
        t = nt - 1 - t
    s = (step * t.double() / (2.0 * D * scale_log2)).to(torch.bfloat16).double()  # rounded: the reference uses what the kernel reads
    f = row_factors(hw) if mixed else torch.ones(hw, dtype=torch.float64)
    q = (f[:, None] * 2.0 * Hd[0][None, :])[None].expand(F, hw, D).contiguous()
    k = (s[:, None] * Hd[0][None, :])[None].expand(F, hw, D).contiguous()
    name = f"{'mixed rows' if mixed else 'staircase'} step {step:g} {'desc' if descending else 'asc'}"
    return Probe512(name, q, k, _onehot_v(F, hw, torch.arange(hw) // KVB), rel=REL_BF16)


def gaussian(F, hw, seed=None):
    """the operand recipe of tests/test_tokenizer_gpu.py's d512 test (score std ~2.5, every 97th key dominant), from a CPU generator"""
    g = torch.Generator().manual_seed(F * 1000 + hw if seed is None else seed)
    q = (torch.randn(F, hw, D, generator=g) * 0.75).to(torch.bfloat16)
    k = (torch.randn(F, hw, D, generator=g) * 0.75).to(torch.bfloat16)
    k[:, ::97] *= 3.0
    v = torch.randn(F, hw, D, generator=g).to(torch.bfloat16)
    return Probe512("gaussian", q.double(), k.double(), v.double(), exact=False)


PROBES = {"census-position": census_position, "census-block": census_block, "uniform": uniform, "threshold census": threshold_census}
STAIRS = tuple((s, d) for s in STAIR_STEPS for d in (False, True))


def make(kind, F, hw, scale_log2=SCALE_LOG2_512):
    """kind: a key of PROBES, (step, descending) or ("mixed", step, descending)"""
    if kind in PROBES:
        return PROBES[kind](F, hw)
    if kind[0] == "mixed":
        return staircase(F, hw, kind[1], kind[2], scale_log2, mixed=True)
    return staircase(F, hw, kind[0], kind[1], scale_log2)


MIXED = tuple(("mixed",) + m for m in MIXED_STAIRS)
ALL_KINDS = tuple(PROBES) + STAIRS + MIXED
CENSUS = ("census-position", "census-block")
STAIR_HW = (64, 128, 192, 320, 1088)
# (frames, hw, kinds) at SOFTMAX_SCALE_512: every probe at (3, 320) and (8, 192); the census at every hw with one frame, the staircases where listed;
# 16 frames (two per XCD) once. hw = 64: one tile, no next-K fetch; 192, 320, 448: a half-empty last query block; 1088: 17 tiles.
PLAN_512 = ((3, 320, ALL_KINDS), (8, 192, ALL_KINDS)) + tuple(
    (1, hw, CENSUS + ("threshold census",) + ((STAIRS + MIXED) if hw in STAIR_HW else ())) for hw in (64, 128, 192, 320, 448, 1088)) + ((16, 192, CENSUS + ("uniform",)),)
PLAN_512_DEFAULT_SCALE = ((3, 320, CENSUS + STAIRS), (8, 192, CENSUS + STAIRS))


def reference(p, softmax_scale=SOFTMAX_SCALE_512, check_leak=True, with_abs=False):
    """fp64 softmax attention per frame -> out [F, hw, 512] (with_abs: also sum_j p_j |v_j|). Asserts, where the probe has classes, that all but
    1e-6 of every row's weight lies on the keys of the query's class."""
    sc = torch.einsum("fid,fjd->fij", p.q, p.k) * softmax_scale
    w = torch.softmax(sc, dim=-1)
    if check_leak and p.q_class is not None:
        same = (torch.arange(p.hw) % p.C)[None, None, :] == p.q_class[..., None]
        leak = float((w * ~same).sum(-1).max())
        assert leak < 1e-6, f"{p.name}: {leak:.3e} of a row's weight lies outside the query's class"
    out = torch.einsum("fij,fjd->fid", w, p.v)
    return (out, torch.einsum("fij,fjd->fid", w, p.v.abs())) if with_abs else out


def keys_all_owned(p):
    """census-block: every key owns a nonzero reference element in some query row of some frame"""
    out = reference(p)
    j = torch.arange(p.hw)
    owned = torch.zeros(p.hw, dtype=torch.bool)
    for f in range(p.F):
        hit = p.q_class[f][:, None] == (j % p.C)[None, :]
        owned |= (hit & (out[f][:, j // p.C] > SMALL_REF)).any(dim=0)
    return bool(owned.all())


def first_bad512(out, ref, rel):
    """the first failing element, as text (frame, query row, column)"""
    out, ref = out.double(), ref.double()
    big = ref >= SMALL_REF
    bad = torch.where(big, (out - ref).abs() > rel * ref, out.abs() > SMALL_OUT) | ~torch.isfinite(out)
    idx = bad.nonzero()
    if not idx.numel():
        return "none"
    i = tuple(int(x) for x in idx[0])
    return f"{int(bad.sum())} bad elements, first at (frame, row, col) {i}: got {float(out[i]):.6g}, want {float(ref[i]):.6g}"


DEFECTS = ("drop_key", "swap_vt_cols", "skip_rescale_row", "other_block_factor", "next_frame_vt", "ragged_rows_unwritten")
NOT_A_DEFECT = "ge_threshold"  # moving AT the threshold: P <= 2^8 either way, every probe keeps its exact values (module docstring)
SKIP_ROW = 37


def emulate(p, softmax_scale=SOFTMAX_SCALE_512, defect=None, trace=None):
    """The kernel's arithmetic on probe p -> out [F, hw, 512] fp32 holding bf16 values (NaN where a defect leaves a row unwritten).
    trace: a list that receives, per tile, the bool [F, hw] "row moved its reference point in this tile".
    defect: one of DEFECTS, or NOT_A_DEFECT -
      drop_key               the last key of the frame is not attended
      swap_vt_cols           keys 3 and 5 of tile 0 read each other's V^T column
      skip_rescale_row       row SKIP_ROW's accumulators miss every rescale after tile 0 (its l does not)
      other_block_factor     the accumulators of 32-row group g take the factors of group (g + 1) % 4 of the same 128-row block
      next_frame_vt          frame f multiplies with frame (f + 1) % frames' V^T
      ragged_rows_unwritten  hw % 128 == 64: the last 64 rows stay unwritten"""
    assert defect in (None, NOT_A_DEFECT) + DEFECTS
    f32 = torch.float32
    F, hw = p.F, p.hw
    qf, kf, vf = p.q.to(f32), p.k.to(f32), p.v.to(f32)
    if defect == "next_frame_vt":
        vf = vf.roll(-1, dims=0)
    c = torch.tensor(softmax_scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    O = torch.zeros(F, hw, D, dtype=f32)
    l = torch.zeros(F, hw, dtype=f32)
    m = torch.full((F, hw), -1e30, dtype=f32)
    rows = torch.arange(hw)
    other = (rows // QB) * QB + (rows % QB + GROUP) % QB  # the same lane of the next 32-row group of the block
    for t in range(hw // KVB):
        idx = torch.arange(t * KVB, (t + 1) * KVB)
        vidx = idx.clone()
        if defect == "swap_vt_cols" and t == 0:
            vidx[3], vidx[5] = 5, 3
        S = qf @ kf[:, idx].transpose(-1, -2)  # [F, hw, 64] fp32 (exact on the probes)
        mx = S.max(dim=-1).values * c
        move = (mx >= m + RESCALE_THR) if defect == NOT_A_DEFECT else (mx > m + RESCALE_THR)
        alpha = torch.where(move, torch.exp2(m - mx), torch.ones((), dtype=f32))
        m = torch.where(move, mx, m)
        if trace is not None:
            trace.append(move.clone())
        pv = torch.exp2((S.double() * c.double() - m.double()[..., None]).to(f32))  # fma: one rounding
        if defect == "drop_key" and t == hw // KVB - 1:
            pv[..., -1] = 0.0
        l = l * alpha + pv.sum(dim=-1)
        a_o = alpha
        if defect == "other_block_factor":
            a_o = torch.where(other < hw, alpha[:, other.clamp(max=hw - 1)], torch.ones((), dtype=f32))  # (rows past hw: q = 0, factor 1 after tile 0)
            if t == 0:
                a_o = alpha
        if defect == "skip_rescale_row" and t > 0 and SKIP_ROW < hw:
            a_o = a_o.clone()
            a_o[:, SKIP_ROW] = 1.0
        O = O * a_o[..., None] + pv.to(torch.bfloat16).to(f32) @ vf[:, vidx]
    out = (O * (1.0 / l)[..., None]).to(torch.bfloat16).to(f32)
    if defect == "ragged_rows_unwritten" and hw % QB == KVB:
        out[:, hw - KVB:] = float("nan")
    return out


def gauss_excess(out, ref, absum):
    """the Gaussian bar's figure: the largest (|out - ref| - 0.5 bf16_ulp(ref)) / E over all elements, E = 2^-9 sum_j p_j |v_j|"""
    o = out.double()
    if not bool(torch.isfinite(o).all()):
        return math.inf
    return float((((o - ref).abs() - 0.5 * bf16_ulp(ref)) / (2.0 ** -9 * absum)).max())


# ---- temporal attention ---------------------------------------------------------------------------------------------------------------------------------

TEMPORAL_SHAPES = ((1, 5, 64), (2, 3, 8), (16, 7, 512), (5, 9, 520), (3, 6, 1024), (17, 5, 256), (33, 3, 64), (64, 2, 128))  # (T, HW, C)
TEMPORAL_PERIOD = 3
TEMPORAL_GAUSS = (16, 1000, 512)  # ~136 000 scores: enough for a handful to round to the other bf16 neighbour in fp32


def px_applies(T, C):
    """the launcher's choice (csrc/tokenizer.hip), operands 16-byte aligned: the one-wave-per-pixel kernel serves T <= 16 and C <= 512"""
    return T <= 16 and C <= 512


def _temporal_qk(T, HW, C):
    """q / k [T, HW, C]: frame t of pixel p is the +-1 row Hd[(t % 3 + 5 p) % n] over the first n = 2^floor(log2 C) channels and +1 on the others:
    a query matches the keys whose frame is congruent to its own mod 3 - score C - and scores C - n against every other key"""
    n = 1 << (C.bit_length() - 1)
    Hd = hadamard(n)
    cls = (torch.arange(T)[:, None] % TEMPORAL_PERIOD + 5 * torch.arange(HW)[None, :]) % n
    x = torch.ones(T, HW, C, dtype=torch.float64)
    x[..., :n] = Hd[cls]
    return x


def _temporal_values(T, HW, C):
    t, p, c = torch.arange(T)[:, None, None], torch.arange(HW)[None, :, None], torch.arange(C)[None, None, :]
    return ((7 * t + 3 * p + c) % 5).double()  # no negative values: no cancellation, an fp32 sum of <= 64 terms is within 2^-18 of the fp64 one


def temporal_probe(kind, T, HW, C):
    """kind: "causality" (V[t] = one-hot(t): output column d is the weight on frame d, bitwise +0 for d > query frame), "values" (small integers
    that depend on frame, pixel and channel), "uniform" (q = 0) -> (q, k, v) [T, HW, C] fp64 holding bf16 values"""
    qk = _temporal_qk(T, HW, C)
    q = torch.zeros_like(qk) if kind == "uniform" else qk
    if kind == "causality":
        assert C >= T
        v = torch.zeros(T, HW, C, dtype=torch.float64)
        v[torch.arange(T), :, torch.arange(T)] = 1.0
    else:
        v = _temporal_values(T, HW, C)
    for x in (q, qk, v):
        assert bf16_exact(x)
    return q, qk, v


TEMPORAL_KINDS = ("causality", "values", "uniform")


def temporal_gaussian(T, HW, C, seed=0):
    g = torch.Generator().manual_seed(1000 * T + C + seed)
    return tuple(torch.randn(T, HW, C, generator=g).to(torch.bfloat16).double() for _ in range(3))


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def temporal_reference(q, k, v, scale, detail=False):
    """The reference's dtype chain in fp64: scores rounded to bf16, * fp32(scale), causal softmax, weights rounded to bf16, sum -> [T, HW, C] fp64
    (the caller compares a bf16 output against it). detail: also (sum_j P_j |v_j| [T, HW, C], the bf16 scores [HW, T, T], the unrounded weights)."""
    T = q.shape[0]
    s = bf16_round(torch.einsum("thc,uhc->htu", q, k)).double()
    future = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    w = torch.softmax((s * _f32(scale)).masked_fill(future, -math.inf), dim=-1)
    P = bf16_round(w).double()
    out = torch.einsum("htu,uhc->thc", P, v)
    return (out, torch.einsum("htu,uhc->thc", P, v.abs()), s, w) if detail else out


def temporal_fp32(q, k, v, scale, px_block=64):
    """The same chain in fp32, in the kernels' operation order, from elementwise fp32 operations only (the same bits on every host): a lane sums
    its 8 channels of every 512-channel chunk one after the other (the products of two bf16 values are exact in fp32, so a fused multiply-add
    changes nothing), the 64 lanes combine in a xor butterfly 32 .. 1, the denominator and the output sums run over the key frames in order. What
    is left to differ from the kernels is exp and the reciprocal. -> bf16 [T, HW, C]"""
    f32 = torch.float32
    T, HW, C = q.shape
    J = (C + 511) // 512
    pad = lambda x: torch.nn.functional.pad(x.to(f32), (0, 512 * J - C)).view(T, -1, J, 64, 8)
    future = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    sc32 = torch.tensor(scale, dtype=f32)
    lanes = torch.arange(64)
    out = torch.empty(T, HW, C, dtype=torch.bfloat16)
    for p0 in range(0, HW, px_block):
        qq, kk, vv = pad(q[:, p0:p0 + px_block]), pad(k[:, p0:p0 + px_block]), v[:, p0:p0 + px_block].to(f32)
        n = qq.shape[1]
        part = torch.zeros(T, T, n, 64, dtype=f32)  # [query frame, key frame, pixel, lane]
        for j in range(J):
            for e in range(8):
                part = part + qq[:, None, :, j, :, e] * kk[None, :, :, j, :, e]
        o = 32
        while o:
            part = part + part[..., lanes ^ o]
            o //= 2
        s = (part[..., 0].to(torch.bfloat16).to(f32) * sc32).masked_fill(future[:, :, None], -math.inf)  # [T, T, n]
        ex = torch.exp(s - s.max(dim=1, keepdim=True).values)
        den = torch.zeros(T, n, dtype=f32)
        for tj in range(T):
            den = den + ex[:, tj]
        w = (ex * (1.0 / den)[:, None]).to(torch.bfloat16).to(f32)
        acc = torch.zeros(T, n, C, dtype=f32)
        for tj in range(T):
            acc = acc + w[:, tj, :, None] * vv[tj][None]
        out[:, p0:p0 + n] = acc.to(torch.bfloat16)
    return out


def temporal_scores_exact(q, k):
    """every score is a value bf16 holds: its rounding cannot depend on the summation order"""
    return bf16_exact(torch.einsum("thc,uhc->htu", q, k))


def tie_margin(w):
    """the smallest distance of a nonzero softmax weight from a bf16 rounding tie, in bf16 ulp (0.5 = as far as can be): an fp32 weight within
    2^-15 relative of the fp64 one rounds like it wherever this is above 2^-6"""
    w = w[w > 0]
    x = w / bf16_ulp(w)
    return float(((x - torch.floor(x)) - 0.5).abs().min()) if w.numel() else 0.5


def temporal_bar(ref):
    return 0.5 * bf16_ulp(ref) + U16 * ref.abs()


def temporal_flip_allowance(absum, s, scale):
    """per element [T, HW, C]: what one score rounded to the other bf16 neighbour (an fp32 dot product against the exact one) can move an output by -
    the weights of the row change by at most a factor e^+-delta, delta = scale x the largest bf16 ulp of the row's scores, twice (numerator and
    denominator), and any weight may then round to bf16 the other way (2^-8)"""
    delta = _f32(scale) * bf16_ulp(s).amax(dim=-1)  # [HW, T]
    return ((2.0 * torch.expm1(delta) + 2.0 ** -8).transpose(0, 1)[..., None]) * absum


def temporal_outliers(out, ref, absum, s, scale):
    """-> (share of elements outside temporal_bar, whether every one of them is finite and within 0.5 ulp + the flip allowance)"""
    o = out.double()
    err = (o - ref).abs()
    outside = ~(err <= temporal_bar(ref))
    ok = bool(torch.isfinite(o).all()) and bool((err[outside] <= 0.5 * bf16_ulp(ref)[outside] + temporal_flip_allowance(absum, s, scale)[outside]).all())
    return float(outside.double().mean()), ok


# ---- row softmax ------------------------------------------------------------------------------------------------------------------------------------------

SOFTMAX_SCALE_ROWS = 0.37
SOFTMAX_CONTENTS = ("gaussian", "all-equal", "dominant", "minus-inf", "large-negative")
SOFTMAX_REG_MAX = 16384


def softmax_reg_path(n, ld, ptr):
    """the launcher's choice (csrc/tokenizer.hip): rows that fit the workgroup's registers, 16-byte vectors"""
    return n <= SOFTMAX_REG_MAX and n % 8 == 0 and ld % 8 == 0 and ptr % 16 == 0


def softmax_row(content, n, g):
    """one row of bf16 scores [n]. The scale is 0.37; `dominant` is 162 (59.94 after the scale) in a row of Gaussians x 0.25, `large-negative`
    -300 - 2 k (k = 0 .. 7: exp would underflow to 0 without the row maximum, and |x scale| ~ 115 keeps the fp32 rounding of the product, 2^-24 x 115 =
    7e-6 relative in the result, under the bar's 2^-16), `minus-inf` a Gaussian row with one -inf (n >= 2; a Gaussian row otherwise)."""
    x = (torch.randn(n, generator=g) * 3).to(torch.bfloat16)
    if content == "all-equal":
        x[:] = 1.75
    elif content == "dominant":
        x = (x.float() / 12).to(torch.bfloat16)
        x[int(torch.randint(0, n, (1,), generator=g))] = 162.0
    elif content == "minus-inf" and n >= 2:
        x[int(torch.randint(0, n, (1,), generator=g))] = -math.inf
    elif content == "large-negative":
        x = (-300.0 - 2.0 * torch.randint(0, 8, (n,), generator=g)).to(torch.bfloat16)
    return x


def softmax_rows_input(rows, n, first=0, seed=0):
    """[rows, n] bf16 and the content name of every row (row r: SOFTMAX_CONTENTS[(first + r) % 5])"""
    g = torch.Generator().manual_seed(seed + 31 * rows + n)
    names = [SOFTMAX_CONTENTS[(first + r) % len(SOFTMAX_CONTENTS)] for r in range(rows)]
    return torch.stack([softmax_row(c, n, g) for c in names]), names


def softmax_reference(x, scale):
    return torch.softmax(x.double() * _f32(scale), dim=-1)


def softmax_bar(ref):
    return 0.5 * bf16_ulp(ref) + U16 * ref


def softmax_fp32(x, scale):
    return torch.softmax(x.float() * torch.tensor(scale, dtype=torch.float32), dim=-1).to(torch.bfloat16)


def _ceil8(n):
    return (n + 7) // 8 * 8


# (rows, n, ld, elements the base pointer is offset by): n in {1 .. 16384} with ld = n rounded up to 8 and a twin 8 columns wider; one row past the
# register path's 16384; an ld and an n that are no multiple of 8; a base 8 bytes off a 16-byte boundary. Row r of case i holds SOFTMAX_CONTENTS[(i + r) % 5].
SOFTMAX_CASES = tuple(c for n in (1, 7, 8, 100, 2048, 16384) for c in ((5, n, _ceil8(n), 0), (5, n, _ceil8(n) + 8, 0))) + (
    (3, 16392, 16392, 0), (2, 64, 68, 0), (2, 35, 40, 0), (5, 2048, 2056, 4), (5, 128, 136, 4))


def temporal_scales(C):
    """the network's scale and a soft one (a match 3 nats above the rest: graded weights). 3 / C keeps every probe weight at least 2^-7 bf16 ulp from
    a rounding tie (2 / C does not: 2e-4 ulp at T = 64) - the CPU test asserts the margin of both scales at every shape"""
    return (float(C) ** -0.5, 3.0 / C)
