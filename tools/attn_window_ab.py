"""What does the opt-in frame-window self-attention (g3_self_attn_fwd_window_bf16) buy at the product shape?
One process, one box, interleaved arms.

Launch level - S = 56 320 tokens (16 latent frames of 44 x 80 = 3 520), H = 32, B = 2, q / k behind a unit-weight RMSNorm:
  dense16  the self-attention launch as the product runs it today: ops.self_attn_bounded(mfma16=True) -> flash_attn_fwd_w4c_nm_kernel
  dense    the same on the 32x32x16 tile loop the window kernels share:  ops.self_attn_bounded(variant=11) -> flash_attn_fwd_w4b_nm_kernel<true>
  W, s     ops.self_attn_window for W in {1, 2, 4} x s in {0, 1}          -> flash_attn_fwd_w4b_nm_win_kernel<true>
Per arm: median ms of ROUNDS rounds (each: 1 warm + REPS timed launches between hipEvents), the ratio to dense16, the tile density
(g3_self_attn_window_tiles: visited / all (query block, 64-key tile) pairs) and ratio / density - 1.0 would be a launch whose time is its tiles.
"in-order bound": workgroups of unequal length, one per CU, taken in index order by the first free CU of their XCD - the finish time of that schedule
in tile units over the dense launch's: what the launch could reach if a workgroup cost nothing but its tiles.

Step level - the full denoise step of bench.py's workload (28 blocks, 2 forwards) with the option off and with W = 2, s = 1, alternating.

usage (GPU box): python tools/attn_window_ab.py [--no-step] [--out profiles/attn_window_ab.txt]"""
import argparse
import heapq
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gen3c_amd import _lib, ops  # noqa: E402

S, H, B, FL, HD = 56320, 32, 2, 3520, 128
BOUND = HD / math.sqrt(HD) * 1.03
ROUNDS, REPS = 5, 3
WINDOWS = [(W, s) for W in (1, 2, 4) for s in (0, 1)]
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def block_tiles(W, s):
    """64-key tiles per query block of the launch (W None: dense), from the written-down function at one row per block."""
    n_blk = (S + ops.window_q_rows() - 1) // ops.window_q_rows()
    if W is None:
        return [S // 64] * n_blk
    T, QR = S // FL, ops.window_q_rows()
    out = []
    for b in range(n_blk):
        f0, f1 = b * QR // FL, (min(b * QR + QR, S) - 1) // FL
        frames = {f for f in range(T) if max(0, f0 - W) <= f < min(T, f1 + W + 1) or f < min(s, T)}
        out.append(len(frames) * FL // 64)
    return out


def in_order_makespan(tiles):
    """The launch's 1-D grid (attention_w4b.hpp: XCD x works through the (batch, head) pairs x, x + 8, ... block by block, one workgroup per CU, 32 CUs per
    XCD) with every workgroup handed, in index order, to the first free CU of its XCD: finish time in tile units. The eight XCDs run the same sequence."""
    free = [0] * 32
    heapq.heapify(free)
    end = 0
    for _pair in range(H * B // 8):
        for t in tiles:
            t0 = heapq.heappop(free)
            heapq.heappush(free, t0 + t)
            end = max(end, t0 + t)
    return end


def launches(dev):
    g = torch.Generator(device=dev).manual_seed(3)
    D = H * HD

    def rms(x):
        x = x.float().view(x.shape[0], -1, HD)
        return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True))).reshape(x.shape[0], -1).to(torch.bfloat16)
    q = rms(torch.randn(S * B, D, device=dev, generator=g, dtype=torch.bfloat16))
    k = rms(torch.randn(S * B, D, device=dev, generator=g, dtype=torch.bfloat16))
    v = torch.randn(S * B, D, device=dev, generator=g, dtype=torch.bfloat16)
    vt = ops.transpose_v(v, S, B, H)
    del v
    out = torch.empty_like(q)
    arms = {"dense16": lambda: ops.self_attn_bounded(q, k, vt, S, S, B, H, BOUND, out=out, mfma16=True),
            "dense": lambda: ops.self_attn_bounded(q, k, vt, S, S, B, H, BOUND, out=out, variant=11)}
    for W, s in WINDOWS:
        arms[f"W={W} s={s}"] = (lambda W=W, s=s: ops.self_attn_window(q, k, vt, S, B, H, BOUND, FL, W, s, out=out))
    ops.enable_kernel_timers(True)
    for f in arms.values():
        f()
    names = [m["kernel"] for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    ops.enable_kernel_timers(False)
    torch.cuda.synchronize()
    times = {n: [] for n in arms}
    for _ in range(ROUNDS):
        for n, f in arms.items():
            f()
            tm = ops.HipTimer()
            tm.start()
            for _i in range(REPS):
                f()
            tm.stop()
            times[n].append(tm.elapsed_ms() / REPS)
    med = {n: float(np.median(t)) for n, t in times.items()}
    dense_span = in_order_makespan(block_tiles(None, None))
    say(f"self-attention launch, S = {S} ({S // FL} frames of {FL}), H = {H}, B = {B}; median of {ROUNDS} rounds x {REPS} launches, arms interleaved")
    say(f"{'arm':10s} {'kernel':42s} {'ms':>8s} {'/dense16':>9s} {'density':>8s} {'ratio/density':>14s} {'in-order bound':>15s}   runs")
    for (n, f), kern in zip(arms.items(), names):
        if n.startswith("W="):
            W, s = (int(x.split("=")[1]) for x in n.split())
            att, dense = ops.window_attn_tiles(S, FL, W, s)
            assert sum(block_tiles(W, s)) == att
            dens, bound = att / dense, in_order_makespan(block_tiles(W, s)) / dense_span
        else:
            dens, bound = 1.0, 1.0
        ratio = med[n] / med["dense16"]
        say(f"{n:10s} {kern:42s} {med[n]:8.3f} {ratio:9.3f} {dens:8.3f} {ratio / dens:14.3f} {bound:15.3f}   " + " ".join(f"{t:.2f}" for t in times[n]))
    return med


def step(dev):
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
    T, Hl, Wl = 16, 88, 160
    net = VideoExtendGeneralDIT(in_channels=16 + 16 * 4 + 1, rope_t_extrapolation_ratio=2.0, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=1234)
    rs = np.random.RandomState(1)
    normal = lambda shape, std: torch.from_numpy((rs.standard_normal(shape) * std).astype(np.float32)).to(torch.bfloat16).to(dev)
    den = Gen3CDenoiser(net, state_shape=(16, T, Hl, Wl))
    den.scheduler.set_timesteps(35)
    xt = normal((1, 16, T, Hl, Wl), den.scheduler.init_noise_sigma)
    gt, pose, ctx = normal((1, 16, T, Hl, Wl), 0.5), normal((1, 64, T, Hl, Wl), 0.5), normal((1, 512, 1024), 0.2)
    ctx[:, 64:] = 0
    pad = torch.zeros(1, 1, 8 * Hl, 8 * Wl, device=dev, dtype=torch.bfloat16)

    def make_cond(p):
        c = VideoExtendCondition(crossattn_emb=ctx, crossattn_mask=None, padding_mask=pad, fps=torch.tensor([24.0], device=dev), video_cond_bool=True,
                                 condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)
    cond, uncond = make_cond(pose), make_cond(torch.zeros_like(pose))
    arms = {"dense": None, "W=2 s=1": (2, 1)}
    times = {n: [] for n in arms}
    for rnd in range(4):  # round 0 warms both arms
        for n, win in arms.items():
            net.set_self_attn_window(*win) if win else net.set_self_attn_window(None)
            torch.cuda.synchronize()
            tm = ops.HipTimer()
            tm.start()
            for i in range(2):
                den.denoise_step(xt, i, cond, uncond, 1.0, 0.001, 1)
            tm.stop()
            if rnd:
                times[n].append(tm.elapsed_ms() / 2)
    med = {n: float(np.median(t)) for n, t in times.items()}
    say()
    say("full denoise step (bench.py's workload with the product defaults: 28 blocks, cond + uncond forwards), median of 3 rounds x 2 steps, arms alternating")
    for n in arms:
        say(f"{n:10s} {med[n]:9.1f} ms/step  {med[n] / med['dense']:6.3f} of dense   runs " + " ".join(f"{t:.1f}" for t in times[n]))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-step", action="store_true", help="launch level only")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda:0")
    launches(dev)
    torch.cuda.empty_cache()
    if not args.no_step:
        step(dev)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
