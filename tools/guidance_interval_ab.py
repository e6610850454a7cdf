"""GPU: what a denoise step outside the guidance interval costs next to a guided one, at bench.py's workload (latent [1,16,16,88,160], 28 blocks,
random weights, the dense 512-token context), on one MI355X in one process:
  (a) a guided step: the fused conditional + unconditional forward at B = 2 and the CFG step kernel (Gen3CDenoiser.denoise_step as bench.py calls it);
  (b) a cond-only step: ONE forward at B = 1 and the cond step kernel (denoise_step(..., guided=False)).
Method: both shapes are warmed up, then the arms alternate in windows of --window steps for --rounds rounds; every step is timed on the host
around a device synchronisation (a step is seconds long). The FIRST step of a window is the first step after a switch of B (the DiT's single-entry
V^T buffer is rebuilt, the allocator sees the other shape) and is reported separately; the arm's time is the median over the other steps of all
windows, with min and max. Prints the ratio b / a and, from the two medians, the MODELLED denoise time of a 35-step video with no interval and
with the intervals (0.19, 1.61] and (0.5, 20] - a model built from two measured step times, not a measured video. Writes
profiles/guidance_interval_ab.txt.

  python tools/guidance_interval_ab.py [--rounds 5] [--window 3] [--blocks 28] [--out profiles/guidance_interval_ab.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from gen3c_amd.dit import VideoExtendGeneralDIT  # noqa: E402
from gen3c_amd.sampler import (EDMEulerScheduler, Gen3CDenoiser, VideoExtendCondition,  # noqa: E402
                               add_condition_video_indicator_and_video_input_mask, guided_steps)

T, HL, WL, STEP, VIDEO_STEPS = 16, 88, 160, 17, 35
INTERVALS = (None, (0.19, 1.61), (0.5, 20.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "guidance_interval_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=3, help="steps per arm and round; the first of them follows a switch of B")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps per arm before the rounds")
    ap.add_argument("--blocks", type=int, default=28)
    args = ap.parse_args()
    assert args.window >= 2 and args.rounds >= 1
    dev = torch.device("cuda:0")
    net = VideoExtendGeneralDIT(in_channels=16 + 16 * 4 + 1, rope_t_extrapolation_ratio=2.0, num_blocks=args.blocks, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=1234)
    net.cross_attention_skip_zero_context = False  # bench.py's timed region: every context token through the tile loop
    rs = np.random.RandomState(1)
    normal = lambda shape, std: torch.from_numpy((rs.standard_normal(shape) * std).astype(np.float32)).to(torch.bfloat16).to(dev)
    den = Gen3CDenoiser(net, state_shape=(16, T, HL, WL))
    den.scheduler.set_timesteps(VIDEO_STEPS)
    xt = normal((1, 16, T, HL, WL), den.scheduler.init_noise_sigma)
    gt, pose, ctx = normal((1, 16, T, HL, WL), 0.5), normal((1, 64, T, HL, WL), 0.5), normal((1, 512, 1024), 0.2)
    ctx[:, 64:] = 0
    pad = torch.zeros(1, 1, 8 * HL, 8 * WL, device=dev, dtype=torch.bfloat16)
    fps = torch.tensor([24.0], device=dev)

    def make_cond(p):
        c = VideoExtendCondition(crossattn_emb=ctx, crossattn_mask=None, padding_mask=pad, fps=fps, video_cond_bool=True, condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

    cond, uncond = make_cond(pose), make_cond(torch.zeros_like(pose))

    def step(guided: bool) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        den.denoise_step(xt, STEP, cond, uncond, 1.0, 0.001, 1, guided=guided)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    arms = {"a: guided, fused B = 2": True, "b: cond-only, B = 1": False}
    for guided in arms.values():
        for _ in range(args.warmup):
            step(guided)
    steady, first = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, guided in arms.items():
            ms = [step(guided) for _ in range(args.window)]
            first[name].append(ms[0])
            steady[name].extend(ms[1:])
            print(f"{name}: first after the switch {ms[0]:.1f} ms, then " + ", ".join(f"{v:.1f}" for v in ms[1:]), flush=True)
    med = {k: statistics.median(v) for k, v in steady.items()}
    a, b = (med[k] for k in arms)
    lines = [f"guided step against cond-only step at latent [1,16,{T},{HL},{WL}], {args.blocks} blocks, random weights, schedule step {STEP} of {VIDEO_STEPS}; one GPU, one process",
             f"ms per Gen3CDenoiser.denoise_step (host clock around a device synchronisation); arms alternating in windows of {args.window} steps, "
             f"{args.rounds} rounds after {args.warmup} warm-up steps per arm",
             f"steady: every step of a window but the first ({args.rounds * (args.window - 1)} per arm); first after a switch of B: the first step of a window ({args.rounds} per arm)", "",
             "| arm | steady median ms | min | max | spread % | first after a switch: median ms | min | max | switch cost ms | % of a guided step |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name in arms:
        v, f = steady[name], first[name]
        cost = statistics.median(f) - med[name]
        lines.append(f"| {name} | {med[name]:.1f} | {min(v):.1f} | {max(v):.1f} | {100 * (max(v) - min(v)) / med[name]:.2f} | {statistics.median(f):.1f} | {min(f):.1f} | "
                     f"{max(f):.1f} | {cost:+.1f} | {100 * cost / a:+.2f} |")
    lines += ["", f"ratio b / a = {b / a:.3f}", "",
              f"MODEL (not a measurement of a video): denoise time of a {VIDEO_STEPS}-step video = guided steps x a + other steps x b, from the two steady medians above",
              "(switch costs not included: at most two switches per sampling call)", "",
              "| interval | guided steps | modelled denoise s | of the always-guided time |", "|---|---|---|---|"]
    sch = EDMEulerScheduler()
    sch.set_timesteps(VIDEO_STEPS)
    for interval in INTERVALS:
        n = sum(guided_steps(sch.sigmas, interval))
        total = n * a + (VIDEO_STEPS - n) * b
        name = "None (every step guided)" if interval is None else f"({interval[0]:g}, {interval[1]:g}]"
        lines.append(f"| {name} | {n} of {VIDEO_STEPS} | {total / 1e3:.1f} | {total / (VIDEO_STEPS * a):.3f} |")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
