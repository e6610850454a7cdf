"""CPU only: what the opt-in sampler solver "2ab" buys in solver (ODE discretisation) error on GEN3C's own sigma schedule, against the default
EDM-Euler solver, with two analytic denoisers standing in for the network. Writes profiles/sampler_solver_proxy.txt (the table of DESIGN.md
section 12). A proxy for the ODE error only: picture quality with trained weights is not measured by this.

Setup (fixed; tests/test_sampler_2ab_cpu.py asserts on the same functions):
  * schedule: gen3c_amd.sampler.EDMEulerScheduler.set_timesteps(N) - sigma_max 80, sigma_min 0.0002, rho 7, final sigma 0 - as fp64 values of
    its fp32 sigmas;
  * x_init = 80 z, z = 4 096 standard normals from numpy's default_rng(0);
  * denoiser (a), Gaussian data of standard deviation sd = 0.5:            x0 = x sd^2 / (sd^2 + sigma^2);
  * denoiser (b), two-point mixture +-1 of width w = 0.25, v = w^2 + sigma^2: x0 = (w^2 / v) x + (sigma^2 / v) tanh(x / v);
  * error: RMS over the elements against the 20 000-step solution of the same solver family's limit (the 20 000-step 2ab solution; the 20 000-step
    Euler solution agrees with it to a few 1e-4, which the tool prints).
The loops are pure fp64 around gen3c_amd.sampler.res_2ab_coefficients: step 0 and the step to sigma 0 are Euler steps, as in the sampling loop.

  python tools/sampler_solver_proxy.py [--out profiles/sampler_solver_proxy.txt]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from gen3c_amd.sampler import EDMEulerScheduler, res_2ab_coefficients  # noqa: E402

STEPS = (12, 18, 24, 35, 70)
REFERENCE_STEPS = 20000


def schedule(num_steps: int) -> list:
    sch = EDMEulerScheduler()
    sch.set_timesteps(num_steps)
    return [float(v) for v in sch.sigmas]  # num_steps sigmas and the trailing 0


def x_init() -> np.ndarray:
    return 80.0 * np.random.default_rng(0).standard_normal(4096)


def denoiser_gaussian(x: np.ndarray, sigma: float, sd: float = 0.5) -> np.ndarray:
    return x * (sd * sd / (sd * sd + sigma * sigma))


def denoiser_mixture(x: np.ndarray, sigma: float, w: float = 0.25) -> np.ndarray:
    v = w * w + sigma * sigma
    return (w * w / v) * x + (sigma * sigma / v) * np.tanh(x / v)


DENOISERS = {"a": denoiser_gaussian, "b": denoiser_mixture}


def solve(denoiser, num_steps: int, solver: str) -> np.ndarray:
    """x after the whole loop. Euler step: x_t = (t / s) x + (1 - t / s) x0. 2ab: a x + cb1 x0 + cb2 x0_prev where there is a previous x0 and t > 0."""
    sig = schedule(num_steps)
    x, x0_prev = x_init(), None
    for i in range(num_steps):
        s, t = sig[i], sig[i + 1]
        x0 = denoiser(x, s)
        if solver == "2ab" and x0_prev is not None and t > 0.0:
            a, cb1, cb2 = res_2ab_coefficients(s, t, sig[i - 1])
            x = a * x + (cb1 * x0 + cb2 * x0_prev)
        else:
            x = (t / s) * x + (1.0 - t / s) * x0
        x0_prev = x0
    return x


def rms(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.sqrt(np.mean((a - b) ** 2)))


def table(steps=STEPS) -> dict:
    """{denoiser: {"reference_gap": rms(Euler 20 000, 2ab 20 000), "euler": {N: error}, "2ab": {N: error}}}"""
    out = {}
    for name, den in DENOISERS.items():
        ref_2ab, ref_euler = solve(den, REFERENCE_STEPS, "2ab"), solve(den, REFERENCE_STEPS, "euler")
        out[name] = {"reference_gap": rms(ref_2ab, ref_euler),
                     "euler": {n: rms(solve(den, n, "euler"), ref_2ab) for n in steps},
                     "2ab": {n: rms(solve(den, n, "2ab"), ref_2ab) for n in steps}}
    return out


def render(tab: dict) -> str:
    lines = ["sampler solver proxy: RMS error against the 20 000-step solution, EDMEulerScheduler (sigma_max 80, sigma_min 0.0002, rho 7, final 0)",
             "x_init = 80 z, 4 096 normals from default_rng(0); (a) Gaussian data sd 0.5, (b) two-point mixture +-1 of width 0.25",
             f"20 000-step Euler vs 2ab solutions: (a) {tab['a']['reference_gap']:.1e}, (b) {tab['b']['reference_gap']:.1e}", "",
             "| steps | Euler (a) | 2ab (a) | Euler (b) | 2ab (b) |", "|---|---|---|---|---|"]
    for n in tab["a"]["euler"]:
        lines.append(f"| {n} | {tab['a']['euler'][n]:.2e} | {tab['a']['2ab'][n]:.2e} | {tab['b']['euler'][n]:.2e} | {tab['b']['2ab'][n]:.2e} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sampler_solver_proxy.txt"))
    args = ap.parse_args()
    text = render(table())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
