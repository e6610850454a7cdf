"""What does the range-table self-attention (g3_self_attn_fwd_ranges_bf16) cost and buy at the product shape?
One process, one box, arms interleaved after warm-up.

Launch level - S = 56 320 tokens (16 latent frames of 44 x 80 = 3 520), H = 32, B = 2, q / k behind a unit-weight RMSNorm:
  dense        the product launch: ops.self_attn_bounded(mfma16=True)                  -> flash_attn_fwd_w4c_nm_kernel
  window a, b  ops.self_attn_window(W = 2, s = 1), twice (their difference is the spread) -> flash_attn_fwd_w4b_nm_win_kernel<true>
  frame 2:1    ops.self_attn_ranges on sparse_attn.frame_ranges(16, 3520, 2, 1): the window's tiles in the window's order, so
               frame / window is the price of the table walk                             -> flash_attn_fwd_w4b_nm_rng_kernel<true>
  radial w     ops.self_attn_ranges on sparse_attn.radial_ranges(16, 3520, w, 1), w = 0.5, 0.25, 0.125
Per arm: median ms of ROUNDS rounds (each: 1 warm + REPS timed launches between hipEvents), the share of the dense launch, the tile density
(attended / dense (query block, 64-key tile) pairs) and share / density - 1.0 would be a launch whose time is its tiles.

Step level - the full denoise step of bench.py's workload (28 blocks, 2 forwards) with the option off and with radial:0.25:1, alternating.

usage (GPU box): python tools/attn_ranges_ab.py [--no-step] [--out profiles/attn_ranges_ab.txt]"""
import argparse
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gen3c_amd import _lib, ops, sparse_attn  # noqa: E402

S, H, B, FL, T, HD = 56320, 32, 2, 3520, 16, 128
BOUND = HD / math.sqrt(HD) * 1.03
ROUNDS, REPS = 5, 3
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


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
    window = lambda: ops.self_attn_window(q, k, vt, S, B, H, BOUND, FL, 2, 1, out=out)
    tables = {"frame 2:1": ops.attn_range_table(sparse_attn.frame_ranges(T, FL, 2, 1), S, H=H)}
    for w in (0.5, 0.25, 0.125):
        tables[f"radial {w}"] = ops.attn_range_table(sparse_attn.radial_ranges(T, FL, w, 1), S, H=H)
    arms = {"dense": lambda: ops.self_attn_bounded(q, k, vt, S, S, B, H, BOUND, out=out, mfma16=True), "window a": window, "window b": window}
    for n, t in tables.items():
        arms[n] = (lambda t=t: ops.self_attn_ranges(q, k, vt, S, B, H, BOUND, t, out=out))
    ops.enable_kernel_timers(True)
    outs = {}
    for n, f in arms.items():
        outs[n] = f().clone() if n in ("window a", "frame 2:1") else f()
    metas = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    ops.enable_kernel_timers(False)
    torch.cuda.synchronize()
    same = torch.equal(outs["window a"], outs["frame 2:1"])
    del outs
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
    say(f"self-attention launch, S = {S} ({T} frames of {FL}), H = {H}, B = {B}; median of {ROUNDS} rounds x {REPS} launches, arms interleaved")
    say(f"{'arm':13s} {'kernel':42s} {'ms':>8s} {'/dense':>7s} {'density':>8s} {'share/density':>14s} {'max ranges':>10s}   runs")
    for (n, f), m in zip(arms.items(), metas):
        dens = m.get("tile_density", 1.0)
        share = med[n] / med["dense"]
        say(f"{n:13s} {m['kernel']:42s} {med[n]:8.3f} {share:7.3f} {dens:8.3f} {share / dens:14.3f} {str(m.get('max_ranges', '-')):>10s}   "
            + " ".join(f"{t:.2f}" for t in times[n]))
    spread = abs(med["window a"] - med["window b"]) / min(med["window a"], med["window b"])
    walk = med["frame 2:1"] / min(med["window a"], med["window b"])
    say()
    say(f"frame 2:1 output equals the window launch bit for bit: {same}")
    say(f"price of the table walk: frame 2:1 / window = {walk:.4f}; spread between the two window arms {spread:.4f}; "
        f"the bar 1 + max(0.02, 3 x spread) = {1 + max(0.02, 3 * spread):.4f}: {'within' if walk <= 1 + max(0.02, 3 * spread) else 'EXCEEDED'}")
    return med


def step(dev):
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
    Hl, Wl = 88, 160
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
    arms = {"dense": None, "radial:0.25:1": ("radial", 0.25, 1)}
    times = {n: [] for n in arms}
    for rnd in range(4):  # round 0 warms both arms (and builds the table)
        for n, spec in arms.items():
            net.set_self_attn_pattern(spec)
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
        say(f"{n:14s} {med[n]:9.1f} ms/step  {med[n] / med['dense']:6.3f} of dense   runs " + " ".join(f"{t:.1f}" for t in times[n]))
    say("picture quality under the pattern: unmeasured (no trained checkpoint exists in this project)")
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
