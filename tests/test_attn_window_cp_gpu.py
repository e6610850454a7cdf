"""GPU: the frame-window self-attention under key sharding (g3_self_attn_fwd_window_cp_bf16: the window kernels over one rank's query rows and a
compact K / V^T buffer of the frames [0, a) ++ [b, c)). One GPU, no process group: one process plays each rank in turn - it slices the rank's compact
buffer (parallel.window_halo_plan) out of the global K / V, transposes it with ops.transpose_v and launches.

Inputs and references are tests/test_attn_window_gpu.py's (built once per shape, shared, never written): q, k behind a unit-weight RMSNorm as column
views of fused buffers, the fp64 logits per (batch, head).

 * aligned shards (frame_len 256, T 8, world 4: every rank's first row is a multiple of 256): every rank's output EQUALS its rows of ops.self_attn_window
   on the whole sequence - same key order, same tile boundaries - for the no-max form and the running-maximum form. (W, s) = (1, 1) meets all of
   the prologue's cases: a sink that reaches the window (one range), a block whose gap is the buffer's gap (nothing left to skip), a block whose gap
   is larger than the buffer's, and a buffer without a gap whose block still skips.
 * misaligned shards (frame_len 320, T 6, world 6 and 3): blocks count from the rank's first row, so the function is ops.window_attn_mask's rank
   form; worst (batch, head) rel-L2 against the fp64 softmax under that mask < 4e-3, the bar of the existing window tests.
 * a buffer one frame wider on each side gives the tight buffer's bits; the whole sequence as the buffer at world 1 is ops.self_attn_window.
 * frame_len 64, T 13, world 13, W 0, s 1: one-tile workgroups, and two-tile ones that skip from logical tile 1."""
import pytest
import torch

from tests.test_attn_window_gpu import BOUND, HD, MAX_WIN, NM_WIN, _problem, _timed

pytestmark = pytest.mark.gpu
FORMS = ((BOUND, NM_WIN), (0.0, MAX_WIN))


def _rank_operands(S, B, H, fl, r, world, buf):
    """(q rows of rank r, compact k, plain V^T of the compact v, Sq, Skv_buf) for the buffer (a, b, c) in frames."""
    from gen3c_amd import ops
    q, k, v, _vt, _ = _problem(S, B, H)
    Sl = S // world
    a, b, c = buf
    rows = lambda f0, f1: slice(f0 * fl * B, f1 * fl * B)  # rows are (s, b) pairs: a frame's rows are contiguous
    kc = torch.cat([k[rows(0, a)], k[rows(b, c)]])
    vc = torch.cat([v[rows(0, a)], v[rows(b, c)]])
    n = (a + c - b) * fl
    return q[r * Sl * B:(r + 1) * Sl * B], kc, ops.transpose_v(vc, n, B, H), Sl, n


def _launch(S, B, H, fl, T, r, world, buf, W, s, bound):
    from gen3c_amd import ops
    qr, kc, vtc, Sl, n = _rank_operands(S, B, H, fl, r, world, buf)
    return ops.self_attn_window_cp(qr, kc, vtc, Sl, n, B, H, bound, fl, T, r * (T // world), buf[0], buf[1], W, s)


def _block_cases(mask, buf, fl):
    """Which prologue case every 256-row block of a rank is, from the written-down mask and the buffer."""
    a, b, _c = buf
    out = set()
    for r0 in range(0, mask.shape[0], 256):
        keys = mask[r0].nonzero().flatten()
        gap = (keys[1:] - keys[:-1] > 1).nonzero().flatten()
        if not gap.numel():
            out.add("one range")
            continue
        sink_end, lo = int(keys[gap[0]]) + 1, int(keys[gap[0] + 1])
        lo_buf = lo - (b - a) * fl if lo >= b * fl else lo
        out.add("the buffer's gap" if lo_buf == sink_end else "a larger gap" if b > a else "a gap inside one range")
    return out


def _fp64_rows(S, B, H, r0, mask):
    """fp64 softmax of the query rows [r0, r0 + mask.shape[0]) under mask [rows, S] -> [rows*B, H*128]."""
    logits = _problem(S, B, H)[4]
    n = mask.shape[0]
    out = torch.empty(n * B, H * HD, device="cuda:0", dtype=torch.float64)
    for (b, h), (sc, v) in logits.items():
        out[b::B, h * HD:(h + 1) * HD] = torch.softmax(sc[r0:r0 + n].masked_fill(~mask, float("-inf")), dim=-1) @ v
    return out


def _worst_pair(out, ref, B, H):
    rel = lambda x, y: float((x.double() - y).norm() / y.norm())
    return max(rel(out[b::B, h * HD:(h + 1) * HD], ref[b::B, h * HD:(h + 1) * HD]) for b in range(B) for h in range(H))


@pytest.mark.parametrize("W,s", [(1, 1), (0, 2), (2, 0)])
def test_aligned_shards_equal_the_single_gpu_window_bit_for_bit(W, s):
    from gen3c_amd import ops, parallel
    fl, T, world, B, H = 256, 8, 4, 2, 2
    S = fl * T
    q, k, _v, vt, _ = _problem(S, B, H)
    plan = parallel.window_halo_plan(T, world, W, s)
    Sl = S // world
    cases = set()
    for r in range(world):
        cases |= _block_cases(ops.window_attn_mask(Sl, fl, W, s, q_row0=r * Sl, T_total=T), plan["buffers"][r], fl)
    if (W, s) == (1, 1):
        assert cases == {"one range", "the buffer's gap", "a larger gap", "a gap inside one range"}, cases
    for bound, kernel in FORMS:
        whole = ops.self_attn_window(q, k, vt, S, B, H, bound, fl, W, s)
        for r in range(world):
            out, metas = _timed(lambda: _launch(S, B, H, fl, T, r, world, plan["buffers"][r], W, s, bound))
            assert len(metas) == 1 and metas[0]["kernel"] == kernel, metas
            assert torch.equal(out, whole[r * Sl * B:(r + 1) * Sl * B]), f"rank {r} buffer {plan['buffers'][r]} {kernel}"


@pytest.mark.parametrize("world", [6, 3])
@pytest.mark.parametrize("W,s", [(1, 1), (0, 2)])
def test_misaligned_shards_vs_fp64_under_the_ranks_mask(world, W, s):
    from gen3c_amd import ops, parallel
    fl, T, B, H = 320, 6, 2, 2
    S = fl * T
    plan = parallel.window_halo_plan(T, world, W, s)
    Sl = S // world
    worst = {kernel: 0.0 for _b, kernel in FORMS}
    for r in range(world):
        mask = ops.window_attn_mask(Sl, fl, W, s, q_row0=r * Sl, T_total=T)
        ref = _fp64_rows(S, B, H, r * Sl, mask.to("cuda:0"))
        for bound, kernel in FORMS:
            out = _launch(S, B, H, fl, T, r, world, plan["buffers"][r], W, s, bound)
            assert torch.isfinite(out.float()).all()
            worst[kernel] = max(worst[kernel], _worst_pair(out, ref, B, H))
    print(f"[window cp fl={fl} T={T} world={world} W={W} s={s}] worst (rank, batch, head) rel-L2 vs masked fp64: {worst}")
    for kernel, err in worst.items():
        assert err < 4e-3, f"{kernel}: rel-L2 {err:.3e} vs the fp64 softmax under the rank's mask"


@pytest.mark.parametrize("fl,T,world", [(256, 8, 4), (320, 6, 6)])
def test_a_wider_buffer_gives_the_tight_buffers_bits(fl, T, world):
    from gen3c_amd import parallel
    B, H, W, s = 2, 2, 1, 1
    S = fl * T
    plan = parallel.window_halo_plan(T, world, W, s)
    widened = 0
    for r in range(world):
        a, b, c = plan["buffers"][r]
        # one frame more at the end of the head piece, at the start of the tail piece and at its end; a gap of one or two frames closes
        wide = (a + 1, b - 1, min(c + 1, T)) if a + 1 < b - 1 else (0, 0, min(c + 1, T))
        if wide == (a, b, c):
            continue
        widened += 1
        for bound, _kernel in FORMS:
            tight = _launch(S, B, H, fl, T, r, world, (a, b, c), W, s, bound)
            assert torch.equal(_launch(S, B, H, fl, T, r, world, wide, W, s, bound), tight), f"rank {r}: {wide} against {(a, b, c)}"
    assert widened >= world - 1


@pytest.mark.parametrize("fl,S,W,s", [(320, 1920, 1, 1), (256, 2048, 0, 2), (64, 832, 0, 1)])
def test_the_whole_sequence_as_the_buffer_is_the_single_gpu_window(fl, S, W, s):
    from gen3c_amd import ops
    B, H = (1, 1) if fl == 64 else (2, 2)
    q, k, _v, vt, _ = _problem(S, B, H)
    T = S // fl
    for bound, kernel in FORMS:
        out, metas = _timed(lambda: _launch(S, B, H, fl, T, 0, 1, (0, 0, T), W, s, bound))
        assert metas[0]["kernel"] == kernel
        assert torch.equal(out, ops.self_attn_window(q, k, vt, S, B, H, bound, fl, W, s))


def test_single_tile_workgroups_and_a_skip_from_tile_one():
    from gen3c_amd import ops, parallel
    fl, T, world, W, s, B, H = 64, 13, 13, 0, 1, 1, 1
    S = fl * T
    plan = parallel.window_halo_plan(T, world, W, s)
    assert plan["buffers"][0] == (0, 0, 1) and plan["buffers"][1] == (0, 0, 2) and plan["buffers"][5] == (1, 5, 6)
    worst = {kernel: 0.0 for _b, kernel in FORMS}
    for r in range(world):
        mask = ops.window_attn_mask(fl, fl, W, s, q_row0=r * fl, T_total=T)
        assert int(mask[0].sum()) == (64 if r == 0 else 128)  # one tile; afterwards the sink tile and the own frame: skip_t0 == 1
        ref = _fp64_rows(S, B, H, r * fl, mask.to("cuda:0"))
        for bound, kernel in FORMS:
            out = _launch(S, B, H, fl, T, r, world, plan["buffers"][r], W, s, bound)
            assert torch.isfinite(out.float()).all()
            worst[kernel] = max(worst[kernel], _worst_pair(out, ref, B, H))
    print(f"[window cp fl=64 T=13 world=13 W=0 s=1] worst (rank, batch, head) rel-L2 vs masked fp64: {worst}")
    for kernel, err in worst.items():
        assert err < 4e-3, f"{kernel}: rel-L2 {err:.3e}"
