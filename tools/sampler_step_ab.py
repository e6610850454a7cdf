"""GPU: time of the sampler's step kernels at the product shape ([1,16,16,88,160] latent, 3 604 480 elements) - the Euler entry
(g3_edm_cfg_euler_step_bf16, 10 B per element) next to the opt-in "2ab" entry (g3_edm_cfg_2ab_step_bf16, 18 B per element with a history, 14 B
without) - through gen3c_amd.ops as the sampler calls them. A record, not a gate: both are microseconds in a 3 s denoise step.

Method: device events around windows of 4 000 back-to-back calls on one stream (the output allocation of the front end included, as in the loop),
the calls rotating over 8 operand sets (about 400 MB together, more than the 256 MB Infinity Cache: in the loop the operands come from HBM, the
DiT has run in between), the three arms alternating window by window for 15 rounds after 3 warm-up rounds; per arm the median window and the
spread over the rounds. That is the time per call of the front end (a host that enqueues slower than the kernel runs would show here); the kernels'
own durations are read from a kernel trace of a short run (--calls 100 under rocprofv3 --kernel-trace --stats), kept next to this table.
Writes profiles/sampler_step_ab.txt.

  python tools/sampler_step_ab.py [--out profiles/sampler_step_ab.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from gen3c_amd import ops  # noqa: E402
from gen3c_amd.sampler import Gen3CDenoiser, res_2ab_coefficients  # noqa: E402

SHAPE, CALLS, SETS, ROUNDS, WARMUP, STEP = (1, 16, 16, 88, 160), 4000, 8, 15, 3, 17


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sampler_step_ab.txt"))
    ap.add_argument("--calls", type=int, default=CALLS, help="calls per timed window (a short run under a kernel tracer)")
    args = ap.parse_args()
    calls = args.calls
    dev = torch.device("cuda:0")
    from types import SimpleNamespace
    den = Gen3CDenoiser(SimpleNamespace(is_context_parallel_enabled=False))
    den.scheduler.set_timesteps(35)
    sig = den.scheduler.sigmas
    co = den._coefficients(sig[STEP], sig[STEP + 1], 0.001)
    coef = res_2ab_coefficients(float(sig[STEP]), float(sig[STEP + 1]), float(sig[STEP - 1]))
    g = torch.Generator().manual_seed(0)
    B, C, T, H, W = SHAPE
    bf = lambda std: (std * torch.randn(SHAPE, generator=g)).to(torch.bfloat16).to(dev)
    ind = torch.tensor([1.0] + [0.0] * (T - 1), device=dev)
    scalars = (T, H * W, 1.0, co["c_skip_bf16"], co["c_out_bf16"], co["c_skip"], co["c_out"], co["sigma"], co["inv_sigma"], co["sigma_next"])
    sets = [((bf(1.0), bf(1.0), bf(float(sig[STEP])), bf(0.5), ind) + scalars, (0.5 * torch.randn(SHAPE, generator=g)).to(dev)) for _ in range(SETS)]
    arms = {"euler": lambda c, hist: ops.edm_cfg_euler_step(*c),
            "2ab, no history": lambda c, hist: ops.edm_cfg_2ab_step(*c, hist, False, 0.0, 0.0, 0.0),
            "2ab, history": lambda c, hist: ops.edm_cfg_2ab_step(*c, hist, True, *coef)}
    times = {k: [] for k in arms}
    for rnd in range(WARMUP + ROUNDS):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(calls):
                fn(*sets[i % SETS])
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if rnd >= WARMUP:
                times[name].append(1e3 * ms / calls)
    n = B * C * T * H * W
    bytes_per = {"euler": 10, "2ab, no history": 14, "2ab, history": 18}
    lines = [f"sampler step kernels at {SHAPE} ({n} elements), step {STEP} of 35; us per call, device events around {calls} back-to-back calls",
             f"rotating over {SETS} operand sets, arms alternating, {ROUNDS} rounds after {WARMUP} warm-up rounds", "",
             "| arm | median us | min | max | B / element | GB/s at the median |", "|---|---|---|---|---|---|"]
    for name, v in times.items():
        med = statistics.median(v)
        lines.append(f"| {name} | {med:.1f} | {min(v):.1f} | {max(v):.1f} | {bytes_per[name]} | {bytes_per[name] * n / med / 1e3:.0f} |")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
