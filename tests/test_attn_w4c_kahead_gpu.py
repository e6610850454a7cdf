"""GPU: flash_attn_fwd_w4c_nm_kernel with K fetched one tile ahead (the K(t+3) pieces behind tile t's barrier, K(2) from the prologue), through
ops.self_attn_bounded(mfma16=True). B = 2, H = 2, S_q = 320 (the second query block is ragged), q / k column views of NaN-guarded fused buffers.

S_kv = 64 .. 384 and 1024, 1 to 6 key tiles and 16: the smallest shapes at which each path of the new schedule first runs - no K(2) (1, 2 tiles); K(2) from
the prologue and no K(3) (3 tiles); the first K(3) fetched in the loop (4); both loop exits after a steady pair (5, 6); every tail re-fetches the last tile
(the last three tiles' pieces), which must stay in bounds: the rows behind K are NaN guard rows.

Checks: the kernel's name; nothing outside the output payload written and the payload finite (no guard row reached it); two calls bitwise equal; worst
(batch, head) rel-L2 against the fp32 softmax < 4e-3 (the project's bar at unit norm weights); and the output BITWISE what the kernel wrote before the
schedule changed: tests/golden/attn_w4c_parent_bits.json (tools/gen_attn_w4c_bits.py, run once at the parent commit) holds, per shape, the SHA-256 of the
output bytes and the first 64 values. The inputs are recomputed from the tool's host_inputs(): numpy.random.RandomState on the host, uniform in [-1, 1]
rounded to bf16, so |q|, |k| <= sqrt(128) and the unit-weight bound holds."""
import json

import pytest
import torch

from tests.guarded import Guarded
from tests.test_attn_bounded_gpu import _fp32, _rel_l2, _worst_pair
from tools.gen_attn_w4c_bits import B, BOUND, D, H, SKVS, SQ, host_inputs, output_record

pytestmark = pytest.mark.gpu

W4C = "flash_attn_fwd_w4c_nm_kernel"


@pytest.fixture(scope="module")
def parent_bits(golden_dir):
    rec = json.loads((golden_dir / "attn_w4c_parent_bits.json").read_text())
    assert rec["kernel"] == W4C and rec["B"] == B and rec["H"] == H and rec["bound"] == BOUND
    return rec["shapes"]


def _call(q, k, vt, Skv, out):
    from gen3c_amd import ops
    ops.enable_kernel_timers(True)
    try:
        ops.self_attn_bounded(q, k, vt, SQ, Skv, B, H, BOUND, out=out, variant=11, mfma16=True)
        launched = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    finally:
        ops.enable_kernel_timers(False)
    torch.cuda.synchronize()
    return launched[-1]["kernel"]


@pytest.mark.parametrize("Skv", SKVS)
def test_w4c_k_ahead_bitwise_the_parents(Skv, parent_bits):
    from gen3c_amd import ops
    qf, kf, v = host_inputs(SQ, Skv)
    qbuf, kbuf = Guarded(SQ * B, 3 * D, data=qf), Guarded(Skv * B, 3 * D, data=kf)
    q, k, v = qbuf.payload[:, :D], kbuf.payload[:, D:2 * D], v.to(qbuf.buf.device)
    assert q.stride(0) == 3 * D and k.stride(0) == 3 * D and not q.is_contiguous() and not k.is_contiguous()
    vt = ops.transpose_v(v, Skv, B, H)
    o1, o2 = Guarded(SQ * B, D, ld=D + 64), Guarded(SQ * B, D, ld=D + 64)
    assert _call(q, k, vt, Skv, o1.payload) == W4C
    o1.assert_only_payload_written(f"w4c K-ahead Skv={Skv}")  # also: the payload is finite - no NaN guard row behind K reached it
    assert _call(q, k, vt, Skv, o2.payload) == W4C
    o2.assert_only_payload_written(f"w4c K-ahead Skv={Skv}, second call")
    out = o1.payload.clone()
    assert torch.equal(out, o2.payload), "two calls differ"
    err = _worst_pair(out, _fp32(q, k, v, B, H), B, H)
    print(f"[w4c K-ahead Sq={SQ} Skv={Skv}] worst (batch, head) rel-L2 vs fp32 softmax {err:.4e}")
    assert err < 4e-3, f"rel-L2 {err:.3e} vs fp32 softmax"
    want, got = parent_bits[f"{SQ}x{Skv}"], output_record(out)
    if got["sha256"] != want["sha256"]:
        first = next((i for i, (a, b) in enumerate(zip(got["first64"], want["first64"])) if a != b), None)
        print(f"[w4c K-ahead Sq={SQ} Skv={Skv}] output bits differ from the parent's; rel-L2 vs fp32 {_rel_l2(out, _fp32(q, k, v, B, H)):.4e}; first differing "
              f"index among the 64 recorded values: {first}" + ("" if first is None else f" ({got['first64'][first]!r} vs {want['first64'][first]!r})"))
    assert got["sha256"] == want["sha256"], f"Skv={Skv}: the output is not bit for bit the parent's"
