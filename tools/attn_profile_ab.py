"""What does the on-GPU per-head pattern selection (g3_attn_pattern_profile_bf16 + g3_attn_pattern_select) cost at the product
shape? One process, one box, arms interleaved after warm-up (tools/attn_ranges_ab.py's method).

Launch level - S = 56 320 tokens (16 latent frames of 44 x 80 = 3 520), H = 32, B = 2, q / k behind a unit-weight RMSNorm, the stacked table
auto=frame:2:1,band:0.125:1:
  fixed a, b   ops.self_attn_ranges with a fixed half / half head_pattern on the device, twice (their difference is the run-to-run spread)
  auto         ops.attn_pattern_profile (64 sample rows, default chunks) + the same launch reading the choice
  profile      ops.attn_pattern_profile alone, per n_chunks
Reported: profile + select in ms and as a share of the sparse launch; its multiple of the floor, ONE read of K (S * B * H * 128 * 2 bytes = 923 MB)
at the HBM peak; the spread.

Step level - the full denoise step of bench.py's workload under frame:2:1 and under auto=frame:2:1,band:0.125:1, alternating.

usage (GPU box): python tools/attn_profile_ab.py [--no-step] [--out profiles/attn_profile_ab.txt]"""
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
HBM_PEAK = 8.0e12  # bytes / s (MI355X)
ROUNDS, REPS = 5, 3
SPEC = ("auto", ("frame", 2, 1), ("band", 0.125, 1))
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def timed(f):
    f()
    tm = ops.HipTimer()
    tm.start()
    for _i in range(REPS):
        f()
    tm.stop()
    return tm.elapsed_ms() / REPS


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
    host = sparse_attn.build_spec(SPEC, T, FL)
    table = ops.attn_range_table(host, S, device=dev)
    plan = ops.attn_profile_plan(table)
    half = torch.tensor([h % 2 for h in range(H)], dtype=torch.int32, device=dev)
    fixed = lambda: ops.self_attn_ranges(q, k, vt, S, B, H, BOUND, table, out=out, head_pattern_dev=half)
    auto = lambda: ops.self_attn_ranges(q, k, vt, S, B, H, BOUND, table, out=out, head_pattern_dev=ops.attn_pattern_profile(q, k, S, B, H, plan))
    nc0 = ops.attn_profile_chunks(S, B, H)
    arms = {"fixed a": fixed, "auto": auto, "fixed b": fixed}
    for nc in sorted({1, 4, nc0, 2 * nc0, 4 * nc0}):
        arms[f"profile nc={nc}"] = (lambda nc=nc: ops.attn_pattern_profile(q, k, S, B, H, plan, n_chunks=nc))
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    times = {n: [] for n in arms}
    for _ in range(ROUNDS):
        for n, f in arms.items():
            times[n].append(timed(f))
    med = {n: float(np.median(t)) for n, t in times.items()}
    dens = sparse_attn.tile_density(host, S)
    say(f"per-head pattern selection, S = {S} ({T} frames of {FL}), H = {H}, B = {B}, candidates {sparse_attn.spec_text(SPEC)} (tile densities "
        f"{dens[0]:.3f}, {dens[1]:.3f}); median of {ROUNDS} rounds x {REPS} launches, arms interleaved; default n_chunks {nc0}")
    for n in arms:
        say(f"{n:16s} {med[n]:9.3f} ms   runs " + " ".join(f"{t:.3f}" for t in times[n]))
    sparse = min(med["fixed a"], med["fixed b"])
    spread = abs(med["fixed a"] - med["fixed b"]) / sparse
    prof = med[f"profile nc={nc0}"]
    floor_ms = S * B * H * HD * 2 / HBM_PEAK * 1e3
    say()
    say(f"profile + select (default chunks): {prof:.3f} ms = {100 * prof / sparse:.2f} % of the sparse launch ({sparse:.3f} ms); auto - fixed = "
        f"{med['auto'] - sparse:.3f} ms; spread between the two fixed arms {100 * spread:.2f} %")
    say(f"floor: one read of K, {S * B * H * HD * 2 / 1e6:.0f} MB at {HBM_PEAK / 1e12:.1f} TB/s = {floor_ms:.3f} ms; profile + select is {prof / floor_ms:.2f} x the floor")
    say(f"the choice on these (random, structureless) operands: {ops.attn_pattern_profile(q, k, S, B, H, plan).cpu().tolist()}")


def step(dev):
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
    Hl, Wl = 88, 160
    net = VideoExtendGeneralDIT(in_channels=16 + 16 * 4 + 1, rope_t_extrapolation_ratio=2.0, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=1234)
    net.self_attn_pattern_log = say
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
    arms = {"frame:2:1": ("frame", 2, 1), sparse_attn.spec_text(SPEC): SPEC}
    times = {n: [] for n in arms}
    say()
    for rnd in range(4):  # round 0 warms both arms (and builds the tables)
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
    say("full denoise step (bench.py's workload with the product defaults: 28 blocks, cond + uncond forwards), median of 3 rounds x 2 steps, arms alternating")
    for n in arms:
        say(f"{n:30s} {med[n]:9.1f} ms/step  {med[n] / med['frame:2:1']:6.3f} of frame:2:1   runs " + " ".join(f"{t:.1f}" for t in times[n]))
    hp = np.asarray(net.self_attn_head_patterns())
    say(f"heads that chose the band (pattern 1) in the last forward, per block (random weights: no claim about trained ones): {hp.sum(axis=1).tolist()}")
    say("picture quality under the patterns: unmeasured (no trained checkpoint exists in this project)")


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
