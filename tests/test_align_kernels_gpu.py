"""gen3c_amd/csrc/align.hip stage by stage: g3_align_depth_f32 through ctypes on a workspace the test owns, every stage read back from it
(AlignState and the planes behind it, at the offsets tests/align_kernel_ref.py mirrors and align.hip pins with static_asserts) and held to the
references of tests/align_kernel_ref.py, which tests/test_align_kernel_ref_cpu.py pins against torch.quantile and the reference's own results
(tests/golden/align_edges.npz) and whose mutants it shows caught on these very inputs.

Rules (those of tests/test_norm_rope_kernels_gpu.py): operands are built on the CPU from seeded generators / read from the fixture and feed kernel
and reference alike; the output lives in a NaN-guarded fp32 buffer, the workspace has 4 KB of a byte pattern behind it, both must come back
untouched outside the payload; inputs must come back as they were.

Bars. count[2], mask_count: exact. prefix[8]: bitwise the sorted value at the floor / ceil rank; rank[s] below that value's multiplicity; hist
zero again. weight[4], qlo, qhi: bitwise torch.quantile's fp32 arithmetic restated. src_inv / tgt_inv / keys: bitwise 1 / x. scale, bias: within
1 fp32 ulp of the fp64 fit over the reference's inlier set (fit condition < 1e4 asserted). Rigid output: |out / oracle - 1| <= 2e-6, zero and
non-finite positions coincide. Repeated calls: bitwise. One Adam step: sc within 2e-6 of 1 - lr g / (|g| + 1e-8) from the fp64 gradient, pixels
inside the stated rounding margin left out (at most 2 % of the masked ones); m1, v2 after two steps within 2e-6 of their closed form's terms;
2 and 3 steps: 2e-3 max / 1e-5 mean against the reference (fixture) / the oracle.

Measured on an MI355X (profiles/cache_update_parity_measured.txt): every state field, the quantiles included, bitwise on all 12 cases - no
rounding separates the hardware from torch.quantile's fp32 arithmetic; scale / bias off by at most 0.354 / 0.295 ulp; the rigid output bitwise
the oracle's on 100 % of the pixels; step 1 max |sc - closed form| 5.97e-08, m1 / v2 at <= 0.062 / 0.046 of their bars, at most 6 of 669 masked
pixels left out (cap 2 % = 13); 2 steps against the reference 7.44e-04 max / 2.57e-06 mean, 3 steps against the oracle 2.38e-07 max."""
import numpy as np
import pytest
import torch

from tests import align_kernel_ref as kr
from tests import attn_probe_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
TAIL = 4096
TINY = [f"tiny_counts_{n}" for n in kr.TINY_COUNTS]


def _lib():
    from gen3c_amd import _lib as L
    return L, L.load()


def _dev():
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same_bits(a, b):
    """bitwise equal, any NaN equal to any NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


class Workspace:
    """a 256-aligned workspace of exactly g3_align_depth_workspace_bytes(h, w) with TAIL pattern bytes behind it; starts as garbage (0xA5)"""

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.n = int(_lib()[1].g3_align_depth_workspace_bytes(h, w))
        assert self.n == kr.workspace_layout(h, w)[0], "tests/align_kernel_ref.workspace_layout no longer mirrors the launcher"
        self.buf = torch.full((self.n + TAIL + 512,), 0xA5, dtype=torch.uint8, device=_dev())
        self.off = (-self.buf.data_ptr()) % 256
        self.pattern = (torch.arange(TAIL, dtype=torch.int32) % 251 + 1).to(torch.uint8).to(_dev())
        self.buf[self.off + self.n:self.off + self.n + TAIL] = self.pattern

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def raw(self):
        return self.buf[self.off:self.off + self.n].cpu().numpy()

    def read(self):
        return kr.parse_workspace(self.raw(), self.h, self.w)

    def assert_tail_untouched(self, what):
        assert torch.equal(self.buf[self.off + self.n:self.off + self.n + TAIL], self.pattern), f"{what}: bytes behind the workspace were written"
        assert bool((self.buf[:self.off] == 0xA5).all()) and bool((self.buf[self.off + self.n + TAIL:] == 0xA5).all()), f"{what}: bytes around the workspace written"


def _outside_untouched(g, what):
    outside = torch.ones_like(g.buf, dtype=torch.bool)
    outside[g.guard:g.guard + g.rows, :g.C] = False
    touched = int((g.buf.view(torch.int32)[outside] != g.fill).sum())
    assert touched == 0, f"{what}: {touched} elements around the output were written"


def _call(ws, src, tgt, mask, *, non_rigid=0, iters=0, Kinv=None, T=None, lam=kr.LAMBDA, lr=kr.LR, what=""):
    """-> (output (h, w) numpy, parsed workspace). Checks the return code, the guards, the tail pattern and that the inputs came back as they were."""
    L, lib = _lib()
    h, w = src.shape
    s_d = torch.from_numpy(np.ascontiguousarray(src, F32)).to(_dev())
    t_d = torch.from_numpy(np.ascontiguousarray(tgt, F32)).to(_dev())
    m_d = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(_dev())
    out = R.Guarded32(h, w)
    kp = None if Kinv is None else np.ascontiguousarray(Kinv, F32)
    tp = None if T is None else np.ascontiguousarray(T, F32)
    rc = lib.g3_align_depth_f32(s_d.data_ptr(), t_d.data_ptr(), None if m_d is None else m_d.data_ptr(), None if kp is None else kp.ctypes.data,
                                None if tp is None else tp.ctypes.data, non_rigid, iters, lam, lr, out.payload.data_ptr(), ws.ptr, ws.n, h, w,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}: {L.last_error()}"
    _outside_untouched(out, what)
    ws.assert_tail_untouched(what)
    assert _same_bits(s_d.cpu().numpy(), src) and _same_bits(t_d.cpu().numpy(), tgt), f"{what}: an input was written"
    assert m_d is None or np.array_equal(m_d.cpu().numpy() != 0, mask)
    return out.payload.cpu().numpy(), ws.read()


def _inputs(name):
    if name == "grid_stride":
        return kr.build_grid_stride()
    if name in kr.FIXTURE_CASES:
        return kr.load_case(name)
    return kr.build_case(name)


_REF = {}


def _rigid_ref(name):
    """computed once per case and shared"""
    if name not in _REF:
        _REF[name] = kr.rigid_reference(*_inputs(name))
    return _REF[name]


def _check_state(name, st, ref):
    assert st["count"].tolist() == ref["count"].tolist(), f"{name}: count {st['count']} != {ref['count']}"
    assert int(st["mask_count"][0]) == ref["mask_count"], f"{name}: mask_count {st['mask_count'][0]} != {ref['mask_count']}"
    got_stat = st["prefix"].view(F32)
    assert np.array_equal(st["prefix"], _bits(ref["stat"])), f"{name}: order statistics {got_stat} != {ref['stat']} (ranks {ref['stat_rank']})"
    mult = [kr.multiplicity(ref["sorted"][s // 4], ref["stat"][s]) for s in range(8)]
    assert all(int(st["rank"][s]) < mult[s] for s in range(8)), f"{name}: remaining ranks {st['rank']} against multiplicities {mult}"
    assert np.array_equal(_bits(st["weight"]), _bits(ref["weight"])), f"{name}: weights {st['weight']} != {ref['weight']}"
    assert np.array_equal(_bits(st["qlo"]), _bits(ref["qlo"])) and np.array_equal(_bits(st["qhi"]), _bits(ref["qhi"])), \
        f"{name}: quantiles {st['qlo']} {st['qhi']} != {ref['qlo']} {ref['qhi']}"
    assert not st["hist"].any(), f"{name}: the histogram was not left clean"
    si, ti = ref["src_inv"], ref["tgt_inv"]
    assert _same_bits(st["src_inv"], si) and _same_bits(st["tgt_inv"], ti), f"{name}: inverse depths differ from IEEE 1 / x"
    src, tgt, mask = _inputs(name)
    _, _, sv, tv, _ = kr.inverses(src, tgt, mask)
    assert np.array_equal(st["key_s"], np.where(sv, _bits(si), np.uint32(kr.NO_KEY))) and np.array_equal(st["key_t"], np.where(tv, _bits(ti), np.uint32(kr.NO_KEY)))
    return max(mult)


@pytest.mark.parametrize("name", list(kr.FIXTURE_CASES) + TINY + ["grid_stride"])
def test_rigid_stages_against_exact_references(name):
    """prep -> radix select -> quantiles -> fp64 fit -> apply, read back stage by stage. Cases (tests/align_kernel_ref.build_case): a ragged frame
    of 851 pixels (per = 1: most threads of the fit reduction idle), 8 plateaus, a plateau across the 10 % rank of the source and one across the
    90 % rank of the target, keys that differ in the last radix digit only, keys that use every digit, 0 / negative / NaN / 1e-38 / 3e38 source
    depths with target 0 inside the mask, 1 / 2 / 3 / 11 / 21 valid target pixels, and 257 x 1031 (a second trip of the grid-stride loops, per = 5).
    The fit is held to its bar where it is well conditioned (asserted); last_digit (x spans 256 ulps: condition 1e10), top_digit and the tiny
    counts are checked up to the quantiles."""
    from oracle import align_oracle as ao
    src, tgt, mask = _inputs(name)
    ref = _rigid_ref(name)
    ws = Workspace(*src.shape)
    out, st = _call(ws, src, tgt, None if name == "plateaus" else mask, what=name)  # plateaus: every pixel valid, through the no-mask form
    top = _check_state(name, st, ref)
    line = f"[align stages {name}] n {src.size} counts {st['count'].tolist()} mask_count {int(st['mask_count'][0])}; order statistics, weights, quantiles bitwise; largest tie {top}"
    if name in kr.FIT_CASES or name == "grid_stride":
        assert ref["cond"] < 1e4 and ref["n_inliers"] >= 2
        es = abs(float(st["scale"][0]) - ref["scale64"]) / kr.ulp32(ref["scale64"])
        eb = abs(float(st["bias"][0]) - ref["bias64"]) / kr.ulp32(ref["bias64"])
        with np.errstate(all="ignore"):
            o = ao.align_depth(src, tgt, mask)
        special = ~np.isfinite(o) | (o == 0)
        got_special = ~np.isfinite(out) | (out == 0)
        with np.errstate(all="ignore"):
            rel = np.abs(out / o - 1)[~special].max()
        exact = float((_bits(out) == _bits(o))[~special].mean())
        print(line + f"; inliers {ref['n_inliers']} cond {ref['cond']:.0f}; scale off {es:.3f} ulp, bias off {eb:.3f} ulp; rigid max rel {rel:.2e}, bitwise share {exact:.4f}, "
              f"zero / non-finite px {int(special.sum())}")
        assert es <= 1.0 and eb <= 1.0, f"{name}: scale {st['scale'][0]!r} vs {ref['scale64']!r}, bias {st['bias'][0]!r} vs {ref['bias64']!r}"
        assert np.array_equal(special, got_special) and _same_bits(np.where(special, out, 0), np.where(special, o, 0)), f"{name}: zero / non-finite positions differ"
        assert rel <= 2e-6
    else:
        print(line)


def test_repeated_calls_on_one_workspace_are_bitwise_equal():
    """fixed-order reduction and self-cleaning state: ragged, then another input, then ragged again on the same workspace"""
    a, b = _inputs("ragged"), _inputs("plateau_at_rank")
    ws = Workspace(kr.H, kr.W)
    o1, s1 = _call(ws, *a, what="first")
    _call(ws, *b, what="other data")
    o2, s2 = _call(ws, *a, what="again")
    assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(_bits(s1["scale"]), _bits(s2["scale"])) and np.array_equal(_bits(s1["bias"]), _bits(s2["bias"]))
    assert np.array_equal(s1["partial"].view(np.uint64), s2["partial"].view(np.uint64)), "the partial sums of the fit differ between two calls"
    fresh, sf = _call(Workspace(kr.H, kr.W), *a, what="fresh workspace")
    assert np.array_equal(_bits(o1), _bits(fresh)) and np.array_equal(_bits(s1["scale"]), _bits(sf["scale"]))
    print("[align repeat] scale, bias, partial sums and output bitwise equal over three calls and a fresh workspace")


def _nonrigid_inputs(case):
    if case in ("1x7", "7x1", "2x2"):
        h, w = map(int, case.split("x"))
        src, tgt, mask = kr.build_small_frame(h, w)
        if case == "2x2":  # four pixels leave two inliers: the fit passes through both, their residuals are pure rounding - ARAP term alone
            mask = np.zeros_like(mask)
    elif case == "all_false":
        src, tgt, mask = _inputs("ragged")
        mask = np.zeros_like(mask)
    else:
        src, tgt, mask = _inputs(case)
    h, w = src.shape
    K, c2w, Kinv, T = kr.camera(h, w)
    return src, tgt, mask, K, c2w, Kinv, T


def test_zero_iterations_is_the_rigid_output():
    src, tgt, mask, K, c2w, Kinv, T = _nonrigid_inputs("ragged")
    ws = Workspace(kr.H, kr.W)
    rigid, _ = _call(ws, src, tgt, mask, what="rigid")
    out, st = _call(ws, src, tgt, mask, non_rigid=1, iters=0, Kinv=Kinv, T=T, what="0 iterations")
    assert np.array_equal(_bits(out), _bits(rigid))
    assert np.all(st["sc"] == 1) and not st["m1"].any() and not st["v2"].any()


def _moment_check(what, got, ref, scale, keep, tol=2e-6):
    """|got - ref| <= tol * scale on the kept pixels; -> worst error over the bar"""
    err = np.abs(got.astype(np.float64) - ref)[keep]
    bar = tol * scale[keep] + 1e-45
    worst = float((err / bar).max()) if err.size else 0.0
    assert worst <= 1.0, f"{what}: worst error {worst:.3f} of the bar"
    return worst


@pytest.mark.parametrize("case", ["ragged", "plateaus", "plateau_at_rank", "all_false", "1x7", "7x1", "2x2"])
def test_one_adam_step_against_the_closed_form(case):
    """num_iters = 1: e = sign(box3(1) / 9 - 1) bitwise (-1 on the border ring, 0 inside: the box filter's zero padding), sc against
    1 - lr g / (|g| + 1e-8) with g the fp64 gradient at the kernel's own rigid depth, m1 = 0.1 g, v2 = 0.001 g^2, output = rigid * sc bitwise.
    all_false: mask_count = 0, the ARAP term alone, non-zero within two pixels of the border. 1 x 7, 7 x 1, 2 x 2: every pixel is border; 2 x 2
    runs with an empty mask too (its fit has two inliers and passes through both, so the data residuals there are rounding alone)."""
    src, tgt, mask, K, c2w, Kinv, T = _nonrigid_inputs(case)
    h, w = src.shape
    ws = Workspace(h, w)
    d_s, _ = _call(ws, src, tgt, mask, what=f"{case} rigid")
    out, st = _call(ws, src, tgt, mask, non_rigid=1, iters=1, Kinv=Kinv, T=T, what=f"{case} 1 step")
    assert int(st["mask_count"][0]) == int(mask.sum())
    ones = np.ones((h, w), F32)
    assert np.array_equal(_bits(st["e"]), _bits(kr.arap_sign_f32(ones)))
    if not mask.any():
        assert int(st["mask_count"][0]) == 0 and np.all(st["sc"][2:-2, 2:-2] == 1) and np.all(st["sc"][0] != 1) and np.all(st["sc"][:, -1] != 1)
        d_s = np.ones((h, w), F32)  # no valid target pixel: the rigid fit is undefined (NaN) and, with the mask empty, unused
    else:
        assert np.isfinite(d_s).all() and _same_bits(out, (d_s * st["sc"]).astype(F32))
    g, a, und = kr.grad64(d_s, tgt, mask, Kinv, T, ones)
    keep = ~und
    nm = max(int(mask.sum()), 1)
    assert und.sum() <= 0.02 * nm, f"{case}: {int(und.sum())} of {nm} masked pixels inside the rounding margin"
    err = np.abs(st["sc"].astype(np.float64) - kr.adam_step1(g))[keep].max()
    wm = _moment_check(f"{case} m1", st["m1"], 0.1 * g, 0.1 * a, keep)
    wv = _moment_check(f"{case} v2", st["v2"], 0.001 * g * g, 0.001 * a * a * 2, keep)
    print(f"[align 1 step {case}] max |sc - closed form| {err:.2e} (bar 2e-6); m1 at {wm:.3f}, v2 at {wv:.3f} of their bars; left out {int(und.sum())}/{nm} (cap 2 %)")
    assert err <= 2e-6


@pytest.mark.parametrize("case", ["ragged", "plateaus", "plateau_at_rank", "nonfinite"])
def test_two_and_three_adam_steps(case):
    """2 steps against the reference's autograd + torch.optim.Adam (fixture) and m1 / v2 against 0.1 g2 + 0.09 g1 and 0.001 g2^2 + 0.000999 g1^2
    (g2: the fp64 gradient at the kernel's own sc after one step); 3 steps against the oracle. Bars 2e-3 max / 1e-5 mean relative."""
    from oracle import align_oracle as ao
    src, tgt, mask, K, c2w, Kinv, T = _nonrigid_inputs(case)
    z = kr.fixture()
    ws = Workspace(kr.H, kr.W)
    d_s, _ = _call(ws, src, tgt, mask, what=f"{case} rigid")
    _, st1 = _call(ws, src, tgt, mask, non_rigid=1, iters=1, Kinv=Kinv, T=T, what=f"{case} 1 step")
    out2, st2 = _call(ws, src, tgt, mask, non_rigid=1, iters=2, Kinv=Kinv, T=T, what=f"{case} 2 steps")
    out3, _ = _call(ws, src, tgt, mask, non_rigid=1, iters=3, Kinv=Kinv, T=T, what=f"{case} 3 steps")
    with np.errstate(all="ignore"):
        o3 = ao.align_depth(src, tgt, mask, k=K, c2w=c2w, alignment_method="non_rigid", num_iters=3)
    figs = []
    for it, got, ref in ((2, out2, z[f"{case}_non_rigid_2"]), (3, out3, o3)):
        ok = np.isfinite(ref) & (ref != 0)
        assert np.array_equal(ok, np.isfinite(got) & (got != 0)), f"{case} {it} steps: zero / non-finite positions differ"
        rel = np.abs(got[ok] / ref[ok] - 1)
        figs.append(f"{it} steps max rel {rel.max():.2e} mean {rel.mean():.2e}")
        assert rel.max() <= 2e-3 and rel.mean() <= 1e-5, figs[-1]
    if case != "nonfinite":
        ones = np.ones_like(d_s)
        g1, a1, u1 = kr.grad64(d_s, tgt, mask, Kinv, T, ones)
        g2, a2, u2 = kr.grad64(d_s, tgt, mask, Kinv, T, st1["sc"])
        assert np.array_equal(_bits(st2["e"]), _bits(kr.arap_sign_f32(st1["sc"]))), "e of the second step is not sign(box3(sc) / 9 - sc) of the first step's sc"
        und = u1 | u2
        assert und.sum() <= 0.02 * mask.sum()
        m_ref, v_ref = kr.adam_step2(g1, g2)
        wm = _moment_check(f"{case} m1", st2["m1"], m_ref, 0.1 * a2 + 0.09 * a1, ~und)
        wv = _moment_check(f"{case} v2", st2["v2"], v_ref, 2 * (0.001 * a2 * a2 + 0.000999 * a1 * a1), ~und)
        figs.append(f"m1 at {wm:.3f}, v2 at {wv:.3f} of their 2e-6 bars; left out {int(und.sum())}/{int(mask.sum())} (cap 2 %)")
    print(f"[align steps {case}] " + "; ".join(figs))


def test_refusals_leave_output_and_workspace_untouched():
    L, lib = _lib()
    src, tgt, mask, K, c2w, Kinv, T = _nonrigid_inputs("ragged")
    h, w = src.shape
    ws = Workspace(h, w)
    before = ws.buf.clone()
    s_d, t_d = (torch.from_numpy(x).to(_dev()) for x in (src, tgt))
    m_d = torch.from_numpy(mask.astype(np.uint8)).to(_dev())
    out = R.Guarded32(h, w)
    fill = out.buf.view(torch.int32).clone()
    kp, tp = Kinv.ctypes.data, T.ctypes.data
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(s=s_d.data_ptr(), t=t_d.data_ptr(), m=m_d.data_ptr(), k=kp, T=tp, nr=1, it=1, o=out.payload.data_ptr(), ws=ws.ptr, n=ws.n, h=h, w=w)
    cases = {"null source": dict(s=None), "null target": dict(t=None), "null output": dict(o=None), "null workspace": dict(ws=None), "H = 0": dict(h=0),
             "H < 0": dict(h=-1), "W = 0": dict(w=0), "workspace one byte short": dict(n=ws.n - 1), "workspace misaligned by 128": dict(ws=ws.ptr + 128, n=ws.n),
             "non-rigid without Kinv": dict(k=None), "non-rigid without T": dict(T=None), "num_iters < 0": dict(it=-1)}
    for what, edit in cases.items():
        a = dict(good, **edit)
        rc = lib.g3_align_depth_f32(a["s"], a["t"], a["m"], a["k"], a["T"], a["nr"], a["it"], kr.LAMBDA, kr.LR, a["o"], a["ws"], a["n"], a["h"], a["w"], stream)
        torch.cuda.synchronize()
        assert rc == L.G3_ERR_ARG, f"{what}: rc {rc}"
        assert "g3_align_depth_f32" in L.last_error()
        assert torch.equal(out.buf.view(torch.int32), fill), f"{what}: the output was written"
        assert torch.equal(ws.buf, before), f"{what}: the workspace was written"
    print(f"[align refusals] {len(cases)} refused with G3_ERR_ARG, nothing written")
