"""Exact probes for the attention kernels, their fp64 references and a torch emulation of the kernels' arithmetic (TEST INFRASTRUCTURE - a
plain helper module; tests/test_attn_probe_ref_cpu.py checks it, tests/test_attn_probes_gpu.py uses it).

Every probe tensor is exactly representable in bf16, so the expected output is a closed form in fp64 and every output element is the trace of
specific keys. Hd is the 128 x 128 Sylvester Hadamard matrix (rows +-1, pairwise dot 0, self dot 128), C = min(128, Skv) classes, key j is Hd[j % C],
query i of pair (b, h) is 2 Hd[(A i + shift(b, h)) % C]: a key of the query's class scores 2 * 128 * scale, every other key exactly 0.

The softmax scale. The one-wave-per-SIMD kernels (w4, w4b and its no-max / carry / window forms, w4c) and the folded 8-wave kernels multiply Q by
scale * log2(e) and round the product to bf16 before the MFMA ("the softmax scale rides on Q"). At the default scale 1 / sqrt(128) that factor is
0.12752: 2 * 0.12752 = 0.25503 rounds to 0.25586, EVERY element of every probe query by the same +0.323 %, so those kernels compute the softmax at a
temperature 0.323 % off: measured on an MI355X, LSE 0.1055 above the fp64 value (32.65 * 0.00323) and staircase masses 2.8e-2 off at step 12. That
is the kernels' documented number format, not a dropped key - but it is what "bf16-exact inputs give a closed form" overlooked. The probes therefore
run at SOFTMAX_SCALE = 2^-3 / log2(e), whose fp32 product with log2(e) is exactly 2^-3: the scaled Q is again bf16-exact, in every kernel, and the
closed form holds through the fold. A matching key then scores exactly 32 in the log2 domain (22.18 nats; all but < Skv e^-22.1 of a row's weight
sits on the keys of its class) and the staircase's s_j = step t / 32 is bf16-exact. `emulate(fold_q=True)` is the kernels' rounding;
`reference(fold_q=True)` is the fp64 softmax of the inputs those kernels' MFMAs see (tests/test_attn_probes_gpu.py: the default-scale test).

 * census-position  V[j, d] = (d == j % 128): the expected row is one-hot at the query's class; a P row paired with the wrong V^T column inside a
                    128-key block moves the 1.
 * census-block     V[j, d] = (d == j // 128): element (i, d) is 1 / n_r iff key 128 d + r exists and is attended (r the query's class, n_r the
                    attended keys of that class), else 0 - every key owns one output element per query class.
 * uniform          q = 0, census-block V: the output is count_d / n, and 2^lse == n.
 * staircase        one class: q = 2 Hd[0], k_j = s_j Hd[0] with the log2-domain logit step * t, t = j // 64 ascending or descending over the tiles, and
                    V[j, d] = (d == j // 64): output column d is the softmax mass of tile d. s_j is rounded to bf16 and the reference uses the rounded value.

Range tables (g3_self_attn_fwd_ranges_bf16). With the default 128 classes a 64-key tile holds half of them, and a block that attends one tile leaves
rows without a key of their class; the range family therefore takes classes = 64 (RANGE_CLASSES): every tile holds every class, census-block's V
column of key j is j // 64, its tile, and output element (i, d) is 1 / n iff tile d is in the list of row i's block (n attended tiles) - every (head,
query block, tile) triple of a launch owns an output element. ranges_mask / head_masks write the function down from gen3c_hip.h, range_walks the
kernel's walk (and nine defects of it), range_shape the shapes and tables that the CPU and the GPU test share.

Tensors are [S, B, H, 128] fp64 on the CPU; `flat` gives the kernels' [S*B, H*128] layout (rows (s, b), b fastest)."""
import functools
import math

import numpy as np
import torch

HD = 128
KVB = 64
Q_ROWS = 256
A_STEP = 5
LOG2E = math.log2(math.e)
SCALE_LOG2 = 2.0 ** -3              # softmax scale in the exp2 domain: a power of two, so that Q * scale is bf16-exact (module docstring)
SOFTMAX_SCALE = SCALE_LOG2 / LOG2E  # what the launches pass; fp32(SOFTMAX_SCALE) * fp32(log2 e) == 2^-3 exactly (asserted on the CPU)
DEFAULT_SCALE = 1.0 / math.sqrt(HD)
BOUND_NATS = 23.0  # >= 22.18 (22.63 at the default scale), the largest census logit; 33.2 in the log2 domain, inside the no-max kernels' limit of 60
MATCH_LOG2 = 2.0 * HD * SCALE_LOG2

# bars (derivations: tests/test_attn_probes_gpu.py)
REL_BF16 = 2.0 ** -7      # bf16 output of any kernel: 2 x (2^-9 bf16 P + 2^-9 bf16 output)
REL_EXACT_P = 2.0 ** -8   # running-max kernels on the census / uniform probes (P == 1), and every fp32 partial output
SMALL_REF, SMALL_OUT = 2.0 ** -20, 2.0 ** -18
LSE_ABS = 1e-4
UNIFORM_L_ABS = 0.25


def hadamard(n=HD):
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n
    return h


def shift(b, h, H):
    """per-(batch, head) class shift: all different, and neighbouring pairs 64 apart so that pairs of 64-row query sets cover all 128 classes"""
    idx = b * H + h
    return 64 * (idx % 2) + 6 * (idx // 2) + (idx % 2)


def bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).to(t.dtype), t)


def flat(x):
    """[S, B, H, 128] -> [S*B, H*128]"""
    return x.reshape(x.shape[0] * x.shape[1], x.shape[2] * x.shape[3])


def unflat(x, B, H):
    return x.reshape(-1, B, H, HD)


class Probe:
    def __init__(self, name, q, k, v, q_class=None, C=None, exact=True):
        """exact=False: inputs that are bf16 values but no probe (the Gaussian report) - the same container, no classes"""
        self.name, self.q, self.k, self.v, self.q_class, self.C = name, q, k, v, q_class, C  # q_class [Sq, B, H] long (None: no classes)
        self.Sq, self.B, self.H = q.shape[:3]
        self.Skv = k.shape[0]
        for t in (q, k, v):
            assert not exact or bf16_exact(t), f"{name}: a probe tensor is not bf16-exact"


def _classes(Sq, Skv, B, H, classes=None):
    C = min(HD, Skv) if classes is None else classes
    assert 0 < C <= HD
    i = torch.arange(Sq)[:, None, None]
    sh = torch.tensor([[shift(b, h, H) for h in range(H)] for b in range(B)])[None]
    return (A_STEP * i + sh) % C, C


def _census_qk(Sq, Skv, B, H, q_scale=2.0, classes=None):
    Hd = hadamard()
    qc, C = _classes(Sq, Skv, B, H, classes)
    q = q_scale * Hd[qc]  # [Sq, B, H, 128]
    k = Hd[torch.arange(Skv) % C][:, None, None, :].expand(Skv, B, H, HD).contiguous()
    return q, k, qc, C


def _onehot_v(Skv, B, H, col):
    v = torch.zeros(Skv, HD, dtype=torch.float64)
    v[torch.arange(Skv), col] = 1.0
    return v[:, None, None, :].expand(Skv, B, H, HD).contiguous()


def census_position(Sq, Skv, B, H, q_scale=2.0, classes=None):
    q, k, qc, C = _census_qk(Sq, Skv, B, H, q_scale, classes)
    return Probe("census-position", q, k, _onehot_v(Skv, B, H, torch.arange(Skv) % HD), qc, C)


def census_block(Sq, Skv, B, H, q_scale=2.0, classes=None):
    """classes (default min(128, Skv)): the class count C - a launch chain over key blocks of L < 128 keys takes C = L, so that every block holds
    every class; the V column of key j is j // C (j // 128 at the default wherever it matters)."""
    q, k, qc, C = _census_qk(Sq, Skv, B, H, q_scale, classes)
    assert Skv <= C * HD
    return Probe("census-block", q, k, _onehot_v(Skv, B, H, torch.arange(Skv) // C), qc, C)


def uniform(Sq, Skv, B, H, classes=None):
    _q, k, _qc, C = _census_qk(Sq, Skv, B, H, classes=classes)
    return Probe("uniform", torch.zeros(Sq, B, H, HD, dtype=torch.float64), k, _onehot_v(Skv, B, H, torch.arange(Skv) // C))


def staircase(Sq, Skv, B, H, step, descending, scale_log2=SCALE_LOG2):
    assert Skv <= KVB * HD
    Hd = hadamard()
    nt = (Skv + KVB - 1) // KVB
    t = torch.arange(Skv) // KVB
    if descending:
        t = nt - 1 - t
    s = (step * t.double() / (2.0 * HD * scale_log2)).to(torch.bfloat16).double()  # rounded: the reference uses what the kernel reads
    q = (2.0 * Hd[0])[None, None, None, :].expand(Sq, B, H, HD).contiguous()
    k = (s[:, None] * Hd[0][None, :])[:, None, None, :].expand(Skv, B, H, HD).contiguous()
    return Probe(f"staircase step {step} {'desc' if descending else 'asc'}", q, k, _onehot_v(Skv, B, H, torch.arange(Skv) // KVB))


def staircase_bound_nats(step, Skv):
    """the smallest comfortable logit bound of a staircase, natural units"""
    return max(1.0, step * ((Skv + KVB - 1) // KVB - 1) / LOG2E * 1.01 + 0.1)


def fp32_scale_log2(softmax_scale):
    """the kernels' exp2-domain scale: fp32(softmax_scale) * fp32(log2 e), rounded to fp32 - as a double"""
    return float(torch.tensor(softmax_scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def reference(p, mask=None, check_leak=True, softmax_scale=SOFTMAX_SCALE, fold_q=False):
    """fp64 softmax attention of probe p under the bool mask [Sq, Skv] or, one per head, [H, Sq, Skv] (None: every key) -> (out [Sq, B, H, 128],
    lse [B, H, Sq] in the log2 domain).
    Asserts that all but 1e-6 of every row's weight lies on the keys of the query's class.
    fold_q: of the inputs the folding kernels' MFMAs see - q * fp32 scale_log2 rounded to bf16 (identical at SOFTMAX_SCALE, where that is exact)."""
    if fold_q:
        qs = (p.q.float() * torch.tensor(fp32_scale_log2(softmax_scale), dtype=torch.float32)).to(torch.bfloat16).double()
        sc = torch.einsum("sbhd,kbhd->bhsk", qs, p.k) / LOG2E
    else:
        sc = torch.einsum("sbhd,kbhd->bhsk", p.q, p.k) * softmax_scale
    if mask is not None:
        assert mask.shape in ((p.Sq, p.Skv), (p.H, p.Sq, p.Skv)) and bool(mask.any(dim=-1).all()), "every query row needs an attended key"
        sc = sc.masked_fill(~(mask[None, None] if mask.dim() == 2 else mask[None]), -math.inf)
    lse = torch.logsumexp(sc, dim=-1)
    w = torch.exp(sc - lse[..., None])
    if check_leak and p.q_class is not None:
        C = p.C
        same = (torch.arange(p.Skv) % C)[None, None, None, :] == p.q_class.permute(1, 2, 0)[..., None]
        leak = float((w * ~same).sum(-1).max())
        assert leak < 1e-6, f"{p.name}: {leak:.3e} of a row's weight lies outside the query's class"
    out = torch.einsum("bhsk,kbhd->sbhd", w, p.v)
    return out, lse * LOG2E


def keys_all_owned(p, mask=None):
    """census-block: every (attended) key owns a nonzero reference element in some query row of some (batch, head); under a per-head mask
    [H, Sq, Skv]: every key a head attends owns one in some query row of some batch OF THAT HEAD"""
    out, _ = reference(p, mask)
    C = p.C
    if mask is not None and mask.dim() == 3:
        j = torch.arange(p.Skv)
        for h in range(p.H):
            owned = torch.zeros(p.Skv, dtype=torch.bool)
            for b in range(p.B):
                hit = mask[h] & (p.q_class[:, b, h][:, None] == (j % C)[None, :])
                owned |= (hit & (out[:, b, h, :][:, j // C] > SMALL_REF)).any(dim=0)
            if not bool(owned[mask[h].any(dim=0)].all()):
                return False
        return True
    owned = torch.zeros(p.Skv, dtype=torch.bool)
    att = torch.ones(p.Sq, p.Skv, dtype=torch.bool) if mask is None else mask
    j = torch.arange(p.Skv)
    for b in range(p.B):
        for h in range(p.H):
            hit = att & (p.q_class[:, b, h][:, None] == (j % C)[None, :])  # [Sq, Skv]: row i traces key j
            val = out[:, b, h, :][:, j // C]  # [Sq, Skv]: the element key j owns in row i
            owned |= (hit & (val > SMALL_REF)).any(dim=0)
    return bool(owned[att.any(dim=0)].all())


# ---- bars --------------------------------------------------------------------------------------------------------------------------------------------

def out_errors(out, ref, rel):
    """(ok, max relative error over the elements with ref >= 2^-20, max |out| over the others); EVERY element is checked"""
    out, ref = out.double(), ref.double()
    big = ref >= SMALL_REF
    err = (out - ref).abs()
    ok = bool(torch.isfinite(out).all()) and bool((err[big] <= rel * ref[big]).all()) and bool((out[~big].abs() <= SMALL_OUT).all())
    relmax = float((err[big] / ref[big]).max()) if bool(big.any()) else 0.0
    small = float(out[~big].abs().max()) if bool((~big).any()) else 0.0
    return ok, relmax, small


def first_bad(out, ref, rel):
    """the first failing element, as text (query row, batch, head, column)"""
    out, ref = out.double(), ref.double()
    big = ref >= SMALL_REF
    bad = torch.where(big, (out - ref).abs() > rel * ref, out.abs() > SMALL_OUT) | ~torch.isfinite(out)
    idx = bad.nonzero()
    if not idx.numel():
        return "none"
    i = tuple(int(x) for x in idx[0])
    return f"{int(bad.sum())} bad elements, first at (row, batch, head, col) {i}: got {float(out[i]):.6g}, want {float(ref[i]):.6g}"


# ---- NaN-guarded fp32 buffer (the fp32 sibling of tests/guarded.py's Guarded) ------------------------------------------------------------------------

class Guarded32:
    """[guard + rows + guard][ld] fp32 on the device, NaN everywhere; the payload is rows x C at row `guard`."""

    def __init__(self, rows, C, ld=None, guard=64):
        self.rows, self.C, self.ld, self.guard = rows, C, ld or C, guard
        assert self.ld >= C
        self.buf = torch.full((rows + 2 * guard, self.ld), float("nan"), dtype=torch.float32, device=torch.device("cuda:0"))
        self.fill = self.buf.view(torch.int32)[0, 0].clone()

    @property
    def payload(self):
        return self.buf[self.guard:self.guard + self.rows, :self.C]

    def assert_only_payload_written(self, what):
        outside = torch.ones_like(self.buf, dtype=torch.bool)
        outside[self.guard:self.guard + self.rows, :self.C] = False
        touched = int((self.buf.view(torch.int32)[outside] != self.fill).sum())
        assert touched == 0, f"{what}: {touched} elements of the guard rows / padding columns were written"
        assert bool(torch.isfinite(self.payload).all()), f"{what}: non-finite values in the payload"


# ---- masks -------------------------------------------------------------------------------------------------------------------------------------------

def skip_mask(Sq, Skv_all, begin, length):
    m = torch.ones(Sq, Skv_all, dtype=torch.bool)
    m[:, begin:begin + length] = False
    return m


def window_ranges(S, frame_len, W, s, q_row0=0, T_total=None, q_rows=Q_ROWS):
    """per query block: (row0, row1, sink_end, lo, hi) in global keys - gen3c_hip.h's definition, as ops.window_attn_mask writes it down"""
    T = S // frame_len if T_total is None else T_total
    out = []
    for r0 in range(0, S, q_rows):
        r1 = min(r0 + q_rows, S)
        f0, f1 = (r0 + q_row0) // frame_len, (r1 - 1 + q_row0) // frame_len
        out.append((r0, r1, min(s, T) * frame_len, max(0, f0 - W) * frame_len, min(T, f1 + W + 1) * frame_len))
    return out


def window_mask(S, frame_len, W, s, q_row0=0, T_total=None, hi_shift=0):
    """the mask of window_ranges; hi_shift moves every block's window end by that many keys (the emulation's range defects)"""
    T = S // frame_len if T_total is None else T_total
    m = torch.zeros(S, T * frame_len, dtype=torch.bool)
    for r0, r1, sink_end, lo, hi in window_ranges(S, frame_len, W, s, q_row0, T_total):
        m[r0:r1, :sink_end] = True
        m[r0:r1, lo:max(lo + KVB, min(T * frame_len, hi + hi_shift))] = True
    return m


# ---- range tables (g3_self_attn_fwd_ranges_bf16) ---------------------------------------------------------------------------------------------------------
# Lists are in TILES: lists[pattern][block] = [(first_tile, n_tiles), ...], ascending and disjoint, without the terminator.

def random_list(rng, n_tiles, max_n):
    """1..max_n ascending disjoint (first_tile, n_tiles) ranges of random lengths; about a third of the neighbours touch"""
    n = int(rng.randint(1, max_n + 1))
    pos, out = int(rng.randint(0, max(1, n_tiles // 3))), []
    for _ in range(n):
        ln = int(rng.randint(1, 5))
        if pos + ln > n_tiles:
            break
        out.append((pos, ln))
        pos += ln + int(rng.choice([0, 1, 2, int(rng.randint(1, max(2, n_tiles // 4)))]))
    return out or [(n_tiles - 1, 1)]


def pack(lists, max_ranges):
    """lists[pattern][block] = [(first_tile, n_tiles), ...] -> int32 [n_patterns, n_qblk, max_ranges, 2] in keys"""
    t = np.zeros((len(lists), len(lists[0]), max_ranges, 2), dtype=np.int32)
    for p, blocks in enumerate(lists):
        for b, rl in enumerate(blocks):
            assert 1 <= len(rl) <= max_ranges
            t[p, b, :len(rl)] = np.asarray(rl, dtype=np.int32) * KVB
    return t


def ranges_mask(lists, S, q_rows=Q_ROWS):
    """bool [S, S] of ONE pattern's lists - gen3c_hip.h's definition: every row of query block b, rows [q_rows b, min(q_rows b + q_rows, S)), attends
    the keys [64 first_tile, 64 (first_tile + n_tiles)) of every range of the block's list, and no other key"""
    assert S % KVB == 0 and len(lists) == (S + q_rows - 1) // q_rows
    m = torch.zeros(S, S, dtype=torch.bool)
    for b, rl in enumerate(lists):
        assert len(rl) >= 1
        for first, n in rl:
            assert first >= 0 and n >= 1 and (first + n) * KVB <= S
            m[b * q_rows:min((b + 1) * q_rows, S), first * KVB:(first + n) * KVB] = True
    return m


def head_masks(lists, head_pattern, S):
    """[H, S, S]: the mask of every head's pattern"""
    by_pattern = [ranges_mask(blocks, S) for blocks in lists]
    return torch.stack([by_pattern[p] for p in head_pattern])


def ranges_counts(lists, head_pattern, S):
    """(attended, dense): the (head, query block, tile) triples of a launch, counted from the lists, and H * n_qblk * S / 64"""
    return sum(n for p in head_pattern for rl in lists[p] for _f, n in rl), len(head_pattern) * len(lists[0]) * (S // KVB)


def _list_walk(rl, n_tiles, defect):
    """the (k_tile, vt_tile) steps of one block's list as the kernel walks it: lane r holds range r, nt is the sum of the lengths, a cursor runs through
    the ranges for K, and V^T(t) is read where the K cursor stood one tile earlier. Every tile index is clamped to the operand, as the kernel's are."""
    rl = list(rl)
    if defect == "range_list_short" and len(rl) > 1:
        rl = rl[:-1]
    if defect == "range_lane_wrap":
        rl = [rl[r - 32] if r >= 32 else rl[r] for r in range(len(rl))]
    nt = sum(n for _f, n in (rl[:32] if defect == "range_sum_half" else rl))
    kt, opens = [], []
    for r, (first, n) in enumerate(rl):
        late = 1 if (defect == "range_starts_late" and r > 0) else 0
        for i in range(n):
            kt.append(min(first + i + late, n_tiles - 1))
            opens.append(r if i == 0 else 0)  # (the index of the range this step opens, 0: none or the first)
    vt = list(kt)
    if defect == "vt_follows_old_range":
        vt = [rl[r - 1][0] + rl[r - 1][1] if r else t for t, r in zip(kt, opens)]
    if defect == "vt_same_step":  # V^T(0) is the prologue's; behind the last tile the cursor stays
        vt = [kt[0]] + [kt[min(t + 1, len(kt) - 1)] for t in range(1, len(kt))]
    return list(zip(kt, vt))[:nt]


def range_walks(lists, head_pattern, B, S, defect=None):
    """walks[batch][head][block] for emulate_walks: the clean kernel (defect None: every listed tile once, in list order, K and V^T alike) or one of
    RANGE_DEFECTS. pattern_by_grid_index: head_pattern read at the (batch, head) pair index, clamped to the array."""
    H, walks = len(head_pattern), []
    for b in range(B):
        per_head = []
        for h in range(H):
            pat = head_pattern[h]
            if defect == "pattern_zero":
                pat = 0
            if defect == "pattern_by_grid_index":
                pat = head_pattern[min(b * H + h, H - 1)]
            blocks = list(lists[pat])
            if defect == "last_block_uses_first":
                blocks[-1] = blocks[0]
            per_head.append([_list_walk(rl, S // KVB, defect) for rl in blocks])
        walks.append(per_head)
    return walks


def emulate_walks(q, k, v, walks, **kw):
    """emulate(walk=...) with walks[batch][head][block]: one call where every batch walks alike, else one per batch"""
    if all(w == walks[0] for w in walks):
        return emulate(q, k, v, walk=walks[0], **kw)
    parts = [emulate(q[:, b:b + 1], k[:, b:b + 1], v[:, b:b + 1], walk=w, **kw) for b, w in enumerate(walks)]
    return torch.cat([o for o, _l in parts], dim=1), torch.cat([l for _o, l in parts], dim=0)


# Family 7 of tests/test_attn_probes_gpu.py, and what tests/test_attn_probe_ref_cpu.py proves about it: the shapes, tables and probes, in one place.
RANGE_CLASSES = KVB  # every 64-key tile holds every class, and the census-block V column of key j is its tile: element (i, d) is 1 / n iff tile d is in row i's list
RANGE_HEAD_PATTERNS = {(1, 8): (0, 1, 2, 1, 1, 0, 2, 0), (2, 3): (2, 0, 1), (1, 2): (1, 0)}  # not monotone, the last pattern used, one pattern on two heads
RANGE_STAIRS_AT = (2, 3)
RANGE_SHAPES = ("a", "b", "c")


@functools.lru_cache(maxsize=None)
def range_shape(name):
    """-> dict(S, max_ranges, lists, bhs, probes, stairs): the smallest shapes at which each mechanism of the range kernels exists"""
    if name == "a":  # three full blocks and a 64-row block, 13 tiles: nt = 1, 2, 3; the prologue's K(1) out of a second range; the operand's last tile
        rng = np.random.RandomState(832)
        lists = [[[(0, 1)], [(0, 1), (2, 1)], [(1, 1), (5, 1), (12, 1)], [(0, 2), (3, 1), (6, 7)]],
                 [[(12, 1)], [(0, 13)], [(3, 2), (5, 2)], [(11, 2)]],
                 [random_list(rng, 13, 8) for _b in range(4)]]
        return dict(S=832, max_ranges=8, lists=lists, bhs=((1, 8), (2, 3)), probes=("census-position", "census-block", "uniform"), stairs=True)
    if name == "b":  # random lists of 1 to 6 ranges over 30 tiles, 7 full blocks and one of 128 rows
        rng = np.random.RandomState(1920)
        lists = [[random_list(rng, 30, 6) for _b in range(8)] for _p in range(3)]
        flat_ = [rl for p in lists for rl in p]
        assert any(a[0] + a[1] == b[0] for rl in flat_ for a, b in zip(rl, rl[1:])), "some ranges touch"
        assert any(a[0] + a[1] < b[0] for rl in flat_ for a, b in zip(rl, rl[1:])), "some ranges jump"
        assert {len(rl) for rl in flat_} >= {1, 2} and max(len(rl) for rl in flat_) >= 5
        return dict(S=1920, max_ranges=6, lists=lists, bhs=((1, 8), (2, 3)), probes=("census-position", "census-block"), stairs=False)
    assert name == "c"  # 65 tiles, 16 full blocks and a 64-row one, 64 ranges: table lanes >= 32 in the load, the butterfly and the lane read
    rng = np.random.RandomState(4160)
    p0 = [[(t, 1) for t in range(65) if t != (7 * b + 3) % 65] for b in range(17)]  # a cursor step on every tile and one jump
    p0[5] = [(t, 1) for t in range(63)]
    p0[9] = [(0, 65)]
    p0[13] = [(2 * t, 1) for t in range(33)]
    assert all(len(rl) == 64 for b, rl in enumerate(p0) if b not in (5, 9, 13)) and len(p0[16]) == 64
    lists = [p0, [random_list(rng, 65, 10) for _b in range(17)]]
    return dict(S=4160, max_ranges=64, lists=lists, bhs=((1, 2),), probes=("census-block", "census-position"), stairs=False)


def range_cases():
    """(shape name, B, H) of every launch group of family 7"""
    return [(name, B, H) for name in RANGE_SHAPES for B, H in range_shape(name)["bhs"]]


def range_probe(kind, S, B, H):
    """a probe of family 7: a name of the census / uniform probes at RANGE_CLASSES classes, or a (step, descending) staircase"""
    if isinstance(kind, tuple):
        return staircase(S, S, B, H, *kind)
    return {"census-position": census_position, "census-block": census_block, "uniform": uniform}[kind](S, S, B, H, classes=RANGE_CLASSES)


# ---- emulation of the kernels' arithmetic -------------------------------------------------------------------------------------------------------------

RANGE_DEFECTS = ("range_starts_late", "range_list_short", "range_lane_wrap", "range_sum_half", "vt_follows_old_range", "vt_same_step", "pattern_zero",
                 "pattern_by_grid_index", "last_block_uses_first")  # made by the caller through another walk: range_walks(defect=...)
DEFECTS = ("drop_last_key", "dup_seam_key", "pad_scored_zero", "swap_vt_cols", "skip_o_rescale", "skip_l_rescale", "window_short", "window_long",
           "skip_shifted", "lse_without_log2_l", "bh_strides_swapped") + RANGE_DEFECTS


def emulate(q, k, v, mask=None, bound_log2=None, defect=None, partial=False, carry=None, softmax_scale=SOFTMAX_SCALE, fold_q=False, walk=None,
            q_rows=Q_ROWS):
    """A tile loop with the kernels' number formats: 64-key tiles, fp32 scores in the log2 domain, a running row maximum (bound_log2 None) or the
    constant bound as the reference point, P rounded to bf16 into P V, l summed in fp32 from the unrounded P, then out = O / l as bf16 (or fp32 with
    partial=True) and lse = m + log2 l. q [Sq, B, H, 128], k / v [Skv, B, H, 128] hold bf16-exact values; mask [Sq, Skv] or [H, Sq, Skv] bool or None.
    walk (in place of a mask): walk[h][block] = the ordered (k_tile, vt_tile) pairs that the block of q_rows query rows of head h visits - K and V^T
    of one step may come from different tiles and a tile may be visited twice, neither of which a mask can say. Each (head, block) is the same
    tile loop over its tiles gathered in that order.
    carry = (o fp32 [Sq, B, H, 128], lse [B, H, Sq]): the carry-in fold of g3_flash_attn_fwd_carry_bf16.
    fold_q: the scale rides on Q - q * scale_log2 rounded to bf16 before the products, as the w4 / w4b / w4c and folded v3 kernels do.
    defect: one of DEFECTS that this function implements itself (the mask defects are made by the caller through another mask).
    -> (out [Sq, B, H, 128] fp32 holding bf16 or fp32 values, lse [B, H, Sq] fp32)."""
    Sq, B, H, _ = q.shape
    Skv = k.shape[0]
    f32 = torch.float32
    if walk is not None:
        assert mask is None and carry is None and defect is None and len(walk) == H
        out, lse = torch.empty(Sq, B, H, HD, dtype=f32), torch.empty(B, H, Sq, dtype=f32)
        tile = torch.arange(KVB)
        for h in range(H):
            assert len(walk[h]) == (Sq + q_rows - 1) // q_rows
            for blk, steps in enumerate(walk[h]):
                rows = slice(blk * q_rows, min((blk + 1) * q_rows, Sq))
                kt, vt = (torch.cat([t[i] * KVB + tile for t in steps]) for i in (0, 1))
                o, l = emulate(q[rows, :, h:h + 1], k[kt][:, :, h:h + 1], v[vt][:, :, h:h + 1], bound_log2=bound_log2, partial=partial,
                               softmax_scale=softmax_scale, fold_q=fold_q)
                out[rows, :, h:h + 1], lse[:, h:h + 1, rows] = o, l
        return out, lse
    if defect == "bh_strides_swapped":  # element (b, h) read at batch stride H' = 1, head stride B: pair index h * B + b in place of b * H + h
        perm = torch.tensor([(idx % H) * B + idx // H for idx in range(B * H)])
        swap = lambda x: x.reshape(x.shape[0], B * H, HD)[:, perm].reshape(x.shape[0], B, H, HD)
        q, k, v = swap(q), swap(k), swap(v)
    qf = q.to(f32).permute(1, 2, 0, 3)  # [B, H, Sq, 128]
    kf = k.to(f32).permute(1, 2, 0, 3)
    vf = v.to(f32).permute(1, 2, 0, 3)
    c = torch.tensor(softmax_scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    if fold_q:
        qf, c = (qf * c).to(torch.bfloat16).to(f32), torch.ones((), dtype=f32)
    nt = (Skv + KVB - 1) // KVB
    O = torch.zeros(B, H, Sq, HD, dtype=f32)
    l = torch.zeros(B, H, Sq, dtype=f32)
    m = torch.full((B, H, Sq), -1e30 if bound_log2 is None else float(bound_log2), dtype=f32)
    for t in range(nt):
        idx = torch.arange(t * KVB, (t + 1) * KVB)
        valid = idx < Skv
        if defect == "drop_last_key":
            valid = valid & (idx != Skv - 1)
        idx = idx.clamp(max=Skv - 1)  # (the kernels re-read the last key row past the end)
        vidx = idx.clone()
        if defect == "dup_seam_key" and t == 1:  # the first key of tile 1 is read at the last key of tile 0, in K and in V^T
            idx[0] = vidx[0] = KVB - 1
        if defect == "swap_vt_cols" and t == 0:
            vidx[3], vidx[5] = 5, 3
        s = (qf @ kf[:, :, idx].transpose(-1, -2)) * c  # [B, H, Sq, 64] fp32
        att = valid[None, :].expand(Sq, KVB)
        if mask is not None:
            att = att & mask[..., idx]  # ([H, Sq, 64] under a per-head mask)
        if defect == "pad_scored_zero":
            s = torch.where(valid[None, None, None, :], s, torch.zeros((), dtype=f32))
            att = att | ~valid[None, :]
        s = s.masked_fill(~(att[None, None] if att.dim() == 2 else att[None]), -math.inf)
        vt = vf[:, :, vidx] * valid[None, None, :, None].to(f32)  # V^T's zero tail
        if bound_log2 is None:
            m_new = torch.maximum(m, s.max(dim=-1).values)
            alpha = torch.exp2(m - m_new)
            O = O * (1.0 if (defect == "skip_o_rescale" and t == 1) else alpha[..., None])
            l = l * (1.0 if (defect == "skip_l_rescale" and t == 1) else alpha)
            m = m_new
        p = torch.exp2(s - m[..., None])
        l = l + p.sum(dim=-1)
        O = O + p.to(torch.bfloat16).to(f32) @ vt
    out = O / l[..., None]
    lse = m if defect == "lse_without_log2_l" else m + torch.log2(l)
    if carry is not None:
        o_c, l_c = carry[0].to(f32).permute(1, 2, 0, 3), carry[1].to(f32)
        M = torch.maximum(l_c, lse)
        wc, wk = torch.exp2(l_c - M), torch.exp2(lse - M)
        out = (wc[..., None] * torch.nan_to_num(o_c) * (wc[..., None] > 0) + wk[..., None] * out) / (wc + wk)[..., None]
        lse = M + torch.log2(wc + wk)
    out = out.permute(2, 0, 1, 3)
    if not partial:
        out = out.to(torch.bfloat16).to(f32)
    return out.contiguous(), lse
