"""References, inputs and the workspace layout for the stage-by-stage tests of gen3c_amd/csrc/align.hip (TEST INFRASTRUCTURE - a plain helper
module; tests/test_align_kernel_ref_cpu.py pins it, tests/test_align_kernels_gpu.py uses it, tools/gen_golden_align_edges.py writes its fixture).

What is restated here, each independent of the library and of oracle/align_oracle.py:
  * exact order statistics by sorting (order_stats), and torch.quantile's fp32 rank / weight / lerp (quantile_parts);
  * the inlier set and the affine fit in fp64 with its condition number n sum(x^2) / det (fit64);
  * the gradient of the reference's loss in fp64 (grad64) and the closed form of Adam steps 1 and 2 (adam_step1, adam_step2).

ROUNDING MARGIN of the data term (grad64): the kernel takes sign(Ps_c - Pt_c) of two fp32 evaluations of
    P_c = ((T_c0 cam_0 + T_c1 cam_1) + T_c2 cam_2) + T_c3,  cam_k = d * ((Kinv_k0 x + Kinv_k1 y) + Kinv_k2),
each a chain of at most eight roundings per operand path. Both carry an absolute error of at most 8 * 2^-24 * A, A = the sum of the absolute
values of every term of that P_c (plus one rounding of d_s * sc). A pixel is left out of the Adam comparisons only when, for some c,
|Ps_c - Pt_c| in fp64 is below MARGIN_ROUNDINGS * 2^-24 * (A_s + A_t): there the fp32 sign is not determined by the mathematics."""
from pathlib import Path

import numpy as np

F32 = np.float32
GOLD = Path(__file__).parent / "golden" / "align_edges.npz"
H, W = 23, 37
MARGIN_ROUNDINGS = 9
LR = 1e-3
LAMBDA = 0.1
NO_KEY = 0xFFFFFFFF

# ---- workspace layout (mirrors struct AlignState and g3_align_depth_f32 in gen3c_amd/csrc/align.hip, pinned there by static_asserts) ----------------
STATE_FIELDS = {  # name: (byte offset, dtype, count)
    "count": (0, np.uint32, 2), "rank": (8, np.uint32, 8), "prefix": (40, np.uint32, 8), "weight": (72, np.float32, 4),
    "qlo": (88, np.float32, 2), "qhi": (96, np.float32, 2), "scale": (104, np.float32, 1), "bias": (108, np.float32, 1),
    "mask_count": (112, np.uint32, 1), "hist": (116, np.uint32, 8 * 256), "partial": (8312, np.float64, 256 * 5),
}
STATE_BYTES = 18552
PLANES = ("src_inv", "tgt_inv", "key_s", "key_t", "sc", "m1", "v2", "e")


def _up(x):
    return (x + 255) & ~255


def workspace_layout(h, w):
    """-> (total bytes, {plane name: byte offset}) - what g3_align_depth_workspace_bytes / the launcher compute"""
    plane = _up(h * w * 4)
    base = _up(STATE_BYTES)
    return base + 8 * plane, {name: base + i * plane for i, name in enumerate(PLANES)}


def parse_workspace(raw: np.ndarray, h, w):
    """raw: the workspace bytes (uint8) -> dict of the state fields and the eight planes"""
    total, off = workspace_layout(h, w)
    assert raw.dtype == np.uint8 and raw.size >= total
    out = {}
    for name, (o, dt, cnt) in STATE_FIELDS.items():
        out[name] = raw[o:o + cnt * np.dtype(dt).itemsize].view(dt).copy()
    for name, o in off.items():
        dt = np.uint32 if name.startswith("key") else np.float32
        out[name] = raw[o:o + h * w * 4].view(dt).reshape(h, w).copy()
    return out


# ---- the rigid stage ------------------------------------------------------------------------------------------------------------------------------------
def inverses(src, tgt, mask):
    """-> (src_inv, tgt_inv, source valid, target valid, mask as bool) as the prep kernel defines them"""
    with np.errstate(all="ignore"):
        si = (F32(1) / src.astype(F32)).astype(F32)
        ti = (F32(1) / tgt.astype(F32)).astype(F32)
    m = np.ones(src.shape, bool) if mask is None else mask.astype(bool)
    with np.errstate(invalid="ignore"):
        return si, ti, si > 0, m & (tgt > 0), m


def order_stats(valid_values: np.ndarray):
    """sorted valid values; the k-th order statistic is [k]"""
    return np.sort(valid_values.astype(F32), kind="stable")


def quantile_parts(sorted_vals: np.ndarray, q: float, rank_n_minus=1, floor_both=False):
    """torch.quantile(x, q, interpolation='linear') restated in its fp32 arithmetic (ATen Sorting.cpp quantile_compute):
    rank = q * (n - 1), floor, ceil, weight = rank - floor, at::lerp. -> dict(lo, hi, weight, a, b, value).
    rank_n_minus / floor_both are the mutants the CPU test shows caught."""
    n = sorted_vals.size
    rank = F32(q) * F32(n - rank_n_minus) if n else F32(0)
    lo = int(np.floor(rank))
    hi = lo if floor_both else int(np.ceil(rank))
    hi = min(hi, max(n - 1, 0))
    w = F32(rank - F32(lo))
    if n == 0:
        return dict(lo=0, hi=0, weight=w, a=F32(0), b=F32(0), value=F32(0))
    a, b = sorted_vals[lo], sorted_vals[hi]
    with np.errstate(all="ignore"):
        v = F32(a + w * F32(b - a)) if w < F32(0.5) else F32(b - F32(b - a) * F32(F32(1) - w))
    return dict(lo=lo, hi=hi, weight=w, a=a, b=b, value=v)


def rigid_reference(src, tgt, mask, *, rank_n_minus=1, floor_both=False, inclusive=False, drop_last_digit=False, mask_count_with_depth=False):
    """Every observable stage of the rigid part for one input. Keyword arguments switch on the mutants."""
    si, ti, sv, tv, m = inverses(src, tgt, mask)
    out = dict(count=np.array([sv.sum(), tv.sum()], np.uint32), mask_count=int((m & (tgt > 0)).sum() if mask_count_with_depth else m.sum()))
    sorted_ = [order_stats(si[sv]), order_stats(ti[tv])]
    out["sorted"] = sorted_
    parts = [[quantile_parts(sorted_[a], q, rank_n_minus, floor_both) for q in (0.1, 0.9)] for a in range(2)]
    if drop_last_digit:  # a select that stops after three digits returns the bucket's lower edge
        for a in range(2):
            for p in parts[a]:
                for k in ("a", "b"):
                    p[k] = (np.array([p[k]], F32).view(np.uint32) & np.uint32(0xFFFFFF00)).view(F32)[0]
                w, x, y = p["weight"], p["a"], p["b"]
                p["value"] = F32(x + w * F32(y - x)) if w < F32(0.5) else F32(y - F32(y - x) * F32(F32(1) - w))
    out["parts"] = parts
    out["qlo"] = np.array([parts[0][0]["value"], parts[1][0]["value"]], F32)
    out["qhi"] = np.array([parts[0][1]["value"], parts[1][1]["value"]], F32)
    out["weight"] = np.array([parts[0][0]["weight"], parts[0][1]["weight"], parts[1][0]["weight"], parts[1][1]["weight"]], F32)
    out["stat"] = np.array([parts[a][qi][k] for a in range(2) for qi in range(2) for k in ("a", "b")], F32)  # order of AlignState.prefix
    out["stat_rank"] = [parts[a][qi][k] for a in range(2) for qi in range(2) for k in ("lo", "hi")]
    with np.errstate(invalid="ignore"):
        if inclusive:
            inl = (si >= out["qlo"][0]) & (si <= out["qhi"][0]) & (ti >= out["qlo"][1]) & (ti <= out["qhi"][1])
        else:
            inl = (si > out["qlo"][0]) & (si < out["qhi"][0]) & (ti > out["qlo"][1]) & (ti < out["qhi"][1])
    out["inliers"] = inl
    out.update(fit64(si, ti, inl))
    out["src_inv"], out["tgt_inv"] = si, ti
    return out


def fit64(si, ti, inl):
    """closed-form least squares tgt_inv ~ scale * src_inv + bias over the inliers, in fp64; cond = n sum(x^2) / det"""
    x, y = si[inl].astype(np.float64), ti[inl].astype(np.float64)
    n = float(x.size)
    sx, sy, sxx, sxy = x.sum(), y.sum(), (x * x).sum(), (x * y).sum()
    det = n * sxx - sx * sx
    with np.errstate(all="ignore"):
        return dict(scale64=(n * sxy - sx * sy) / det, bias64=(sxx * sy - sx * sxy) / det, cond=n * sxx / det if det else np.inf, n_inliers=int(n))


def ulp32(x):
    return float(np.spacing(np.abs(F32(x))))


def multiplicity(sorted_vals, v):
    return int(np.searchsorted(sorted_vals, v, "right") - np.searchsorted(sorted_vals, v, "left"))


# ---- the non-rigid stage --------------------------------------------------------------------------------------------------------------------------------
def box3_f32(a):
    """3 x 3 box sum with zero padding in the kernel's accumulation order (row-major over the window), fp32"""
    p = np.pad(a.astype(F32), 1)
    h, w = a.shape
    acc = np.zeros((h, w), F32)
    for dy in range(3):
        for dx in range(3):
            acc = (acc + p[dy:dy + h, dx:dx + w]).astype(F32)
    return acc


def arap_sign_f32(sc):
    """e = sign(box3(sc) / 9 - sc) in the kernel's fp32 operations (IEEE adds and one multiply: bitwise reproducible)"""
    with np.errstate(invalid="ignore"):
        r = (box3_f32(sc) * F32(1.0 / 9.0)).astype(F32) - sc.astype(F32)
        return (r > 0).astype(F32) - (r < 0).astype(F32)  # 0 for NaN, as torch.sign and the kernel


def grad64(d_s, d_t, mask, Kinv, T, sc, lambda_arap=LAMBDA):
    """fp64 gradient of  mean_{mask, c} |P(d_s sc)_c - P(d_t)_c| + lambda mean |box3(sc)/9 - sc|  with respect to sc, written out as in
    oracle/align_oracle.py, from fp32 operands. -> (g, scale of g's terms, undecided): `undecided` marks masked pixels where some
    |Ps_c - Pt_c| is below the fp32 rounding margin stated in the module docstring. e is taken from arap_sign_f32."""
    h, w = d_s.shape
    m = np.ones((h, w), bool) if mask is None else mask.astype(bool)
    K64, T64 = Kinv.astype(np.float64), T.astype(np.float64)
    xs = np.arange(w, dtype=np.float64)[None, :]
    ys = np.arange(h, dtype=np.float64)[:, None]
    un = [K64[r, 0] * xs + K64[r, 1] * ys + K64[r, 2] for r in range(3)]
    un_abs = [abs(K64[r, 0]) * xs + abs(K64[r, 1]) * ys + abs(K64[r, 2]) for r in range(3)]
    ds64 = d_s.astype(np.float64)
    dsc = (d_s.astype(F32) * sc.astype(F32)).astype(F32).astype(np.float64)  # the kernel rounds d_s * sc once
    dt64 = d_t.astype(np.float64)
    sg, undecided = [], np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        for c in range(3):
            ps = sum(T64[c, k] * dsc * un[k] for k in range(3)) + T64[c, 3]
            pt = sum(T64[c, k] * dt64 * un[k] for k in range(3)) + T64[c, 3]
            A = sum(abs(T64[c, k]) * (np.abs(dsc) + np.abs(dt64)) * un_abs[k] for k in range(3)) + 2 * abs(T64[c, 3])
            res = ps - pt
            undecided |= m & (np.abs(res) < MARGIN_ROUNDINGS * 2.0 ** -24 * A)
            sg.append(np.sign(res))
        gc = [sum(T64[c, k] * sg[c] for c in range(3)) for k in range(3)]
        gdv = sum(gc[k] * un[k] for k in range(3))
        gdv_abs = sum(sum(abs(T64[c, k]) for c in range(3)) * un_abs[k] for k in range(3))
        nm = int(m.sum())
        inv_data = 1.0 / (3.0 * nm) if nm else 0.0
        g_data = np.where(m, gdv * ds64 * inv_data, 0.0)
        a_data = np.where(m, gdv_abs * np.abs(ds64) * inv_data, 0.0)
    e = arap_sign_f32(sc).astype(np.float64)
    p = np.pad(e, 1)
    box = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    g_arap = lambda_arap * ((box / 9.0 - e) / (h * w))
    a_arap = lambda_arap * ((np.abs(box) / 9.0 + np.abs(e)) / (h * w))
    return g_data + g_arap, a_data + a_arap, undecided


def adam_step1(g, lr=LR):
    """sc after the first torch.optim.Adam step from sc = 1, m = v = 0: 1 - lr g / (|g| + 1e-8) (bias corrections cancel)"""
    with np.errstate(all="ignore"):
        return 1.0 - lr * g / (np.abs(g) + 1e-8)


def adam_step2(g1, g2):
    """first and second moment after two steps (betas 0.9 / 0.999)"""
    return 0.1 * g2 + 0.9 * (0.1 * g1), 0.001 * g2 * g2 + 0.999 * (0.001 * g1 * g1)


def camera(h, w):
    """(K, c2w, Kinv, T = inv(c2w)[:3]) of the non-rigid cases: principal point at the centre, a yaw and a translation; inverses in fp32 on the host"""
    K = np.array([[41.0, 0, w / 2], [0, 41.0, h / 2], [0, 0, 1]], F32)  # focal chosen so that no pixel column sits on the zero of T_00 un_0 + T_02
    ang = 0.1
    c2w = np.eye(4, dtype=F32)
    c2w[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], F32)
    c2w[:3, 3] = [0.2, -0.1, 0.05]
    Kinv = np.linalg.inv(K).astype(F32)
    T = np.ascontiguousarray(np.linalg.inv(c2w).astype(F32)[:3])
    return K, c2w, Kinv, T


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------
def _planes(h, w, seed):
    """a slanted target plane, and a source that is affine in inverse depth with a smooth 3 % error and 0.2 % noise"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(F32)
    base = (2 + 0.6 * xs / w + 0.35 * ys / h).astype(F32)
    smooth = 1 + 0.12 * (xs / w - 0.5) * (ys / h - 0.4)
    src = (1 / (0.6 / base + 0.05) * smooth * (1 + 0.002 * rng.randn(h, w))).astype(F32)
    mask = rng.rand(h, w) < 0.8
    tgt = base.copy()
    tgt[~mask] = 0
    return src, tgt, mask, rng


def _ulp_steps(base_bits, rng, shape):
    """depths whose fp32 inverses are base + k ulps, k < 256: only the lowest key byte differs"""
    want = (np.uint32(base_bits) + (4 + np.floor(rng.rand(*shape) * 248)).astype(np.uint32)).view(F32)
    return (F32(1) / want).astype(F32)


FIXTURE_CASES = ("ragged", "plateaus", "plateau_at_rank", "last_digit", "top_digit", "nonfinite")
FIT_CASES = ("ragged", "plateaus", "plateau_at_rank", "nonfinite")  # well-conditioned fits (the CPU test asserts cond < 1e4)
TINY_COUNTS = (1, 2, 3, 11, 21)


def build_case(name):
    """-> (source depth, target depth, mask) of one named case, deterministic"""
    src, tgt, mask, rng = _planes(H, W, 15)
    if name == "ragged":
        pass
    elif name == "plateaus":  # 8 depth levels: both ranks of every quantile land on one value
        lv = (F32(1.0) + F32(0.25) * np.floor(rng.rand(H, W) * 8).astype(F32)).astype(F32)
        src, tgt, mask = (lv * F32(1.3) + F32(0.1) * lv * lv).astype(F32), lv.copy(), np.ones((H, W), bool)  # not affine in inverse depth: residuals stay
    elif name == "plateau_at_rank":
        src[:5] = 6.0  # the smallest inverse depth on 185 of 851 pixels: ranks 0 .. 184 cover the 10 % rank (85)
        tgt[:, :8] = np.where(mask[:, :8], F32(1.0), F32(0))  # the largest target inverse on ~ 21 % of the valid pixels: covers the 90 % rank
    elif name == "last_digit":
        src = _ulp_steps(0x3F000100, rng, (H, W))
        tgt = _ulp_steps(0x3E800300, rng, (H, W))
        tgt[~mask] = 0
    elif name == "top_digit":
        src = (2.0 ** rng.uniform(-60, 60, (H, W))).astype(F32)
        tgt = (2.0 ** rng.uniform(-60, 60, (H, W))).astype(F32)
        mask = np.ones((H, W), bool)
    elif name == "nonfinite":
        src[0, :5] = 0          # inverse +inf: valid, the largest key
        src[1, :5] = -1         # invalid
        src[2, :3] = 1e-38      # inverse 1e38
        src[3, :3] = 3e38       # inverse subnormal, still > 0
        src[4, :3] = np.nan     # invalid
        mask[5, :4] = True
        tgt[5, :4] = 0          # inside the mask, no depth: counts for mask_count, not for the quantiles
    elif name.startswith("tiny_counts_"):
        n = int(name.rsplit("_", 1)[1])
        order = np.random.RandomState(100 + n).permutation(H * W)[:n]
        mask = np.zeros(H * W, bool)
        mask[order] = True
        mask = mask.reshape(H, W)
        tgt = (2 + 0.6 * np.mgrid[0:H, 0:W][1].astype(F32) / W + 0.35 * np.mgrid[0:H, 0:W][0].astype(F32) / H).astype(F32)
        tgt[~mask] = 0
    else:
        raise KeyError(name)
    return src, tgt, mask


def build_grid_stride():
    """257 x 1031 = 264 967 pixels > 1024 x 256: a second trip of the prep / histogram loops, per = 5 with a ragged last chunk"""
    return _planes(257, 1031, 12)[:3]


def build_small_frame(h, w):
    """1 x 7, 7 x 1, 2 x 2: all pixels masked, distinct depths"""
    n = h * w
    rng = np.random.RandomState(1000 + 10 * h + w)
    tgt = (2 + 0.2 * np.arange(n, dtype=F32) + 0.05 * rng.rand(n)).astype(F32).reshape(h, w)
    src = (1 / (0.6 / tgt + 0.05) * (1 + 0.02 * (rng.rand(h, w) - 0.5))).astype(F32)
    return src, tgt, np.ones((h, w), bool)


_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        _FIX = dict(np.load(GOLD))
    return _FIX


def load_case(name):
    """inputs of a fixture case as committed (the CPU test pins build_case against them)"""
    z = fixture()
    return z[f"{name}_source"], z[f"{name}_target"], z[f"{name}_mask"]
