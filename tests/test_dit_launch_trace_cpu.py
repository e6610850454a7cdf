"""CPU: the C calls the Python front end makes - gen3c_amd/dit.py's forward of the tiny two-block net and every public attention, GEMM and layer-norm
wrapper of gen3c_amd/ops.py - row for row against tests/golden/dit_launch_trace_parent.json, which tools/gen_dit_launch_trace.py recorded from the
commit BEFORE the front end was folded (one self-attention stage in the DiT, one marshaller per op family in ops): same symbols in the same
order, same scalars, same null-ness and aliasing of pointers, and the same (kind, meta) of every kernel timer. Nothing is launched
(tests/dit_launch_trace.py); contexts have no zero tail and no traced path reads back what a kernel would have written.

CASES is also what the generator runs: name -> fn(patch, tmp_dir) with patch(obj, name, value) a setattr that is undone after the case."""
import json
import math
from pathlib import Path

import pytest
import torch

from gen3c_amd import dit, ops, parallel, sparse_attn
from tests._mxfp8_tiny_dit import _inputs, _net
from tests.dit_launch_trace import traced

GOLDEN = Path(__file__).resolve().parent / "golden" / "dit_launch_trace_parent.json"
BOUND = 128 / math.sqrt(128) * 1.03


def _shape(B=1, T=6, H=16, W=16):
    return _inputs(B=B, T=T, H=H, W=W)  # [B, 16, 6, 16, 16]: 6 latent frames of 8 x 8 = 64 tokens, S = 384


def _forward(net, inp, n=1, timers=False):
    """n forwards of one net inside one trace -> dict(rows=..., timers=[(kind, meta)] where timers are on)."""
    ops.enable_kernel_timers(timers)
    try:
        with traced() as rows:
            for _ in range(n):
                net(crossattn_mask=None, **inp)
            got = dict(rows=rows)
            if timers:
                got["timers"] = [[kind, meta] for kind, meta, _ in ops.collected_kernel_timers()]
        return got
    finally:
        ops.enable_kernel_timers(False)


def _configured(inp=None, n=1, timers=False, switch=None, net_kw=None, **setup):
    """A forward of a net: `switch` = (name, value) of a module switch of gen3c_amd.dit, net_kw the constructor's keywords, then
    net.<setter>(*args) / net.<attribute> = value for every other keyword."""
    def case(patch, tmp):
        if switch is not None:
            patch(dit, *switch)
        net = _net("cpu", **(net_kw or {}))
        for name, value in setup.items():
            if callable(getattr(net, name, None)):
                getattr(net, name)(*value)
            else:
                setattr(net, name, value)
        return _forward(net, _shape() if inp is None else inp(), n=n, timers=timers)
    return case


def _option(value):
    def case(patch, tmp):
        ops.set_option("attn_variant", value)
        try:
            return _forward(_net("cpu"), _shape())
        finally:
            ops.set_option("attn_variant", 0)
    return case


def _gloo(tmp):
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group("gloo", store=dist.FileStore(str(Path(tmp) / "gloo_store"), 1), rank=0, world_size=1)
    return dist.group.WORLD


def _cp(schedule=None, window=None, bounded=False, timers=False):
    def case(patch, tmp):
        net = _net("cpu")
        net.enable_context_parallel(_gloo(tmp))
        if schedule is not None:
            net._cp_attn.configure(schedule=schedule)
        if window is not None:
            net.set_self_attn_window(*window, context_parallel=True)
        if bounded:
            net._cp_attn.configure(bounded=True)
        got = _forward(net, _shape(), timers=timers)
        # (at world 1 nothing is remote: local_first and local_carry run gather_first's one launch per head group, and `effective` says so)
        assert net._cp_attn.schedule == (schedule or ("window_halo" if window else "local_first")) and net._cp_attn.effective_bounded == bounded
        return got
    return case


def _direct(timers):
    """Every public attention, GEMM and layer-norm wrapper of ops once, at its smallest legal shape."""
    def case(patch, tmp):
        z = lambda *s, dtype=torch.bfloat16: torch.zeros(*s, dtype=dtype)
        f32, u8, f8, i32 = torch.float32, torch.uint8, torch.float8_e4m3fn, torch.int32
        S, B, H = 256, 1, 1
        q, k, vt = z(S, 128), z(S, 128), z(B, H, 128, S)
        k2, vt2, vt5 = z(2 * S, 128), z(B, H, 128, 2 * S), z(2, B, H, 128, S // 2)
        state = lambda: (z(S, 128, dtype=f32), z(B, H, S, dtype=f32))
        ops.enable_kernel_timers(timers)
        try:
            with traced() as rows:
                ops.flash_attn(q, k, vt, S, S, B, H)
                ops.flash_attn(q, k, vt, S, S, B, H, partial=True)
                ops.flash_attn(q, k, vt5, S, S, B, H)
                ops.flash_attn(q, k, vt, S, S, B, H, kv_dense=64, q_norm_weight=z(128))
                ops.flash_attn(q, k2, vt2, S, S, B, H, carry=state(), kv_skip=(64, S))
                o32 = z(S, 256, dtype=f32)
                ops.flash_attn(q, k, vt, S, S, B, H, partial=True, out=o32[:, 128:])
                ops.self_attn_bounded(q, k, vt, S, S, B, H, BOUND)
                ops.self_attn_bounded(q, k, vt, S, S, B, H, BOUND, mfma16=True)
                ops.self_attn_bounded(q, k, vt5, S, S, B, H, BOUND)
                ops.self_attn_bounded(q, k2, vt2, S, S, B, H, BOUND, carry=state(), kv_skip=(S, S), variant=11)
                ops.self_attn_window(q, k, vt, S, B, H, BOUND, 64, 1, 1)
                # rank 2 of 4 over 8 frames of 64 tokens, W = s = 1: frames 4, 5 attend the compact buffer [0, 1) ++ [3, 7)
                a, b, c = parallel.window_halo_plan(8, 4, 1, 1)["buffers"][2]
                ops.self_attn_window_cp(q[:128], z((a + c - b) * 64, 128), z(B, H, 128, (a + c - b) * 64), 128, (a + c - b) * 64, B, H, BOUND, 64, 8, 4, a, b, 1, 1)
                S2 = 512
                q2, kk2, vtt2 = z(S2, 128), z(S2, 128), z(B, H, 128, S2)
                table = ops.attn_range_table(sparse_attn.build_spec(("auto", ("frame", 1, 1), ("band", 0.125, 1)), 8, 64), S2, device="cpu")
                ops.self_attn_ranges(q2, kk2, vtt2, S2, B, H, BOUND, table)
                ops.self_attn_ranges(q2, kk2, vtt2, S2, B, H, BOUND, table, head_pattern_dev=z(H, dtype=i32))
                ops.attn_pattern_profile(q2, kk2, S2, B, H, ops.attn_profile_plan(table))
                ops.attn_merge([state(), state()], S, B, H)
                # the GEMM family: M = 4096 is where the kernel timers begin
                for M in (128, 4096):
                    x, w = z(M, 64), z(64, 64)
                    ops.gemm_nt(x, w)
                    ops.gemm_nt(x, w, out=x, epilogue=ops.EPI_GATED_RESIDUAL, gate=z(1, 64), residual=x)
                    xq, xs, wq, ws = z(M, 64, dtype=f8), z(M, 2, dtype=u8), z(64, 64, dtype=f8), z(64, 2, dtype=u8)
                    ops.gemm_mxfp8_nt(xq, xs, wq, ws, out=x, epilogue=ops.EPI_GATED_RESIDUAL, gate=z(1, 64), residual=x)
                    ops.gemm_mxfp8_nt(xq, xs, wq, ws, epilogue=ops.EPI_GELU, out_mx=True)
                    ops.gemm_mxfp6_nt(z(M, 48, dtype=u8), xs, z(64, 48, dtype=u8), ws, epilogue=ops.EPI_GATED_RESIDUAL, gate=z(1, 64), residual=x)
                    cos, sin = z(M, 128, dtype=f32), z(M, 128, dtype=f32)
                    ops.gemm_qk_norm_rope(x, z(384, 64), 128, 128, z(128), z(128), cos, sin, M, 1, vt=z(1, 1, 128, M))
                    ops.quant_mxfp8(x)
                    ops.quant_mxfp6(x)
                qk = z(S, 256)
                ops.qk_rmsnorm_rope(qk[:, :128], z(128), cos[:S], sin[:S], S, B, H)
                ops.qk_rmsnorm_rope(qk[:, :128], z(128), None, None, S, B, H, out=qk[:, :128])
                ops.qk_rmsnorm_rope_pair(qk, z(128), 1, z(128), 1, cos[:S], sin[:S], S, B)
                ops.transpose_v(qk[:, 128:], S, B, H)
                # the four layer-norm wrappers; rows (t, h, w, b) = 2 x 2 x 2 x 2, D = 64
                x, shift, scale = z(16, 64), z(2, 192)[:, :64], z(2, 192)[:, 64:128]
                ops.layernorm_modulate(x, shift, scale)
                ops.layernorm_modulate_mxfp8(x, shift, scale)
                for pe in ((z(8, 64), None, None, None), (z(2, 64), z(2, 64), z(2, 64), z(8))):
                    ops.posemb_layernorm_modulate(x, *pe, 2, 2, 2, 2, shift, scale)
                    ops.posemb_layernorm_modulate_mxfp8(x, *pe, 2, 2, 2, 2, shift, scale)
                got = dict(rows=rows)
                if timers:
                    got["timers"] = [[kind, meta] for kind, meta, _ in ops.collected_kernel_timers()]
            return got
        finally:
            ops.enable_kernel_timers(False)
    return case


CASES = {
    "default B=1, two forwards": _configured(n=2),
    "default B=2": _configured(inp=lambda: _shape(B=2)),
    "T=1 H=W=10 (S = 25, S % 4 != 0)": _configured(inp=lambda: _shape(T=1, H=10, W=10)),
    "_SELF_ATTN_LOGIT_BOUND=False": _configured(switch=("_SELF_ATTN_LOGIT_BOUND", False)),
    "_SELF_ATTN_MFMA16=False": _configured(switch=("_SELF_ATTN_MFMA16", False)),
    "_SELF_ATTN_MFMA16=True": _configured(switch=("_SELF_ATTN_MFMA16", True)),
    "_V_OPERAND_SWAP=False": _configured(switch=("_V_OPERAND_SWAP", False)),
    "_FUSE_QKV_EPILOGUE=True": _configured(switch=("_FUSE_QKV_EPILOGUE", True)),
    "_CROSS_Q_NORM_IN_ATTENTION=False": _configured(switch=("_CROSS_Q_NORM_IN_ATTENTION", False)),
    "attn_variant=11": _option(11),
    "attn_variant=4": _option(4),
    "mxfp8 separate B=2": _configured(inp=lambda: _shape(B=2), net_kw=dict(precision="mxfp8", producers="separate")),
    "mxfp8 fused B=2": _configured(inp=lambda: _shape(B=2), net_kw=dict(precision="mxfp8", producers="fused")),
    "mxfp8 fused B=2, _CROSS_Q_NORM_IN_ATTENTION=False": _configured(inp=lambda: _shape(B=2), switch=("_CROSS_Q_NORM_IN_ATTENTION", False), net_kw=dict(precision="mxfp8", producers="fused")),
    "mxfp6 B=2": _configured(inp=lambda: _shape(B=2), net_kw=dict(precision="mxfp6")),
    "self_attn_window (1, 1)": _configured(set_self_attn_window=(1, 1)),
    "self_attn_window (5, 0): dense": _configured(set_self_attn_window=(5, 0)),
    "self_attn_pattern frame:1:1": _configured(set_self_attn_pattern=(("frame", 1, 1),)),
    "self_attn_pattern radial:0.25:1 at 24 x 24 tokens per frame": _configured(inp=lambda: _shape(T=2, H=48, W=48), set_self_attn_pattern=("radial:0.25:1",)),
    "self_attn_pattern auto=frame:1:1,band:0.125:1": _configured(set_self_attn_pattern=("auto=frame:1:1,band:0.125:1",)),
    "self_attn_pattern frame:5:0: every tile": _configured(set_self_attn_pattern=("frame:5:0",)),
    "cross_attention_skip_zero_context=False": _configured(cross_attention_skip_zero_context=False),
    "kernel timers": _configured(timers=True),
    "kernel timers, self_attn_window (1, 1)": _configured(timers=True, set_self_attn_window=(1, 1)),
    "kernel timers, mxfp8 fused B=2": _configured(timers=True, inp=lambda: _shape(B=2), net_kw=dict(precision="mxfp8", producers="fused")),
    "kernel timers, self_attn_pattern auto=frame:1:1,band:0.125:1": _configured(timers=True, set_self_attn_pattern=("auto=frame:1:1,band:0.125:1",)),
    "cp local_first (the DiT's default)": _cp(),
    "cp gather_first": _cp("gather_first"),
    "cp local_carry": _cp("local_carry"),
    "cp head_parallel": _cp("head_parallel"),
    "cp window_halo": _cp(window=(1, 1)),
    "cp local_first bounded": _cp("local_first", bounded=True),
    "kernel timers, cp head_parallel": _cp("head_parallel", timers=True),
    "kernel timers, cp window_halo": _cp(window=(1, 1), timers=True),
    "ops wrappers": _direct(False),
    "ops wrappers, kernel timers": _direct(True),
}


def run_case(name, patch, tmp):
    """The case's rows and timers as JSON holds them (tuples as lists)."""
    return json.loads(json.dumps(CASES[name](patch, tmp)))


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module", autouse=True)
def _gloo_group_teardown():
    import torch.distributed as dist
    before = dist.is_initialized()
    yield
    if dist.is_initialized() and not before:
        dist.destroy_process_group()


def test_the_golden_holds_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_front_end_makes_the_recorded_calls(name, golden, monkeypatch, tmp_path_factory):
    got = run_case(name, monkeypatch.setattr, tmp_path_factory.getbasetemp())
    want = golden["cases"][name]
    rows = [golden["rows"][i] for i in want["rows"]]
    assert len(got["rows"]) == len(rows), f"{len(got['rows'])} calls, recorded {len(rows)}"
    for i, (g, w) in enumerate(zip(got["rows"], rows)):
        assert g == w, f"call {i}: {g} != recorded {w}"
    assert got.get("timers") == want.get("timers")


def test_recorded_call_counts(golden):
    """The counts the dry run gave when the front end was first traced: 54 calls per default forward (the second forward of the same net
    saves the 2 x 3 cross-attention K / V calls), 78 / 70 / 78 under mxfp8 with separate and fused producers and under mxfp6 at B = 2."""
    n = {name: len(c["rows"]) for name, c in golden["cases"].items()}
    assert n["default B=1, two forwards"] == 54 + 48
    assert (n["mxfp8 separate B=2"], n["mxfp8 fused B=2"], n["mxfp6 B=2"]) == (78, 70, 78)
