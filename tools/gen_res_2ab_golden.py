"""Regenerates tests/golden/res_2ab/order2_fn_12_steps.npz: what the reference's second-order multistep solver computes, step by step, recorded as
data. CPU only. The single argument is the path of a checkout of the reference project (https://github.com/nv-tlabs/GEN3C); only its
cosmos_predict1/diffusion/functional/multi_step.py is imported (with the two modules it pulls in, which need nothing beyond torch).

Recorded: a 12-step GEN3C sigma schedule (gen3c_amd.sampler.EDMEulerScheduler) without the trailing 0 - 11 steps from sigmas[i] to sigmas[i + 1] -
driven through `order2_fn` in fp64 with the analytic two-point-mixture denoiser of tools/sampler_solver_proxy.py on 64 values
(x_init = 80 z, z from numpy's default_rng(1)). Per step: x_s, s, t, x0_s, x0_prev, s1, x_t; step 0 has no history (have_prev 0, x0_prev and s1 NaN).

  python tools/gen_res_2ab_golden.py /path/to/GEN3C
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "res_2ab" / "order2_fn_12_steps.npz"


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    sys.path.insert(0, str(ROOT))
    from gen3c_amd.sampler import EDMEulerScheduler
    from tools.sampler_solver_proxy import denoiser_mixture
    sys.path.insert(0, str(ref))  # in front of this repository's own cosmos_predict1 entry-point package
    from cosmos_predict1.diffusion.functional import multi_step
    assert Path(multi_step.__file__).resolve().is_relative_to(ref), f"imported {multi_step.__file__}, not the checkout at {ref}"

    sch = EDMEulerScheduler()
    sch.set_timesteps(12)
    sig = [float(v) for v in sch.sigmas[:-1]]
    f64 = lambda v: torch.tensor([v], dtype=torch.float64)
    x = torch.from_numpy(80.0 * np.random.default_rng(1).standard_normal(64)).reshape(1, 64)
    history = []
    rec = {k: [] for k in ("x_s", "s", "t", "x0_s", "x0_prev", "s1", "x_t", "have_prev")}
    for i in range(len(sig) - 1):
        s, t = sig[i], sig[i + 1]
        x0 = torch.from_numpy(denoiser_mixture(x.numpy(), s))
        x_t, new_history = multi_step.order2_fn(x, f64(s), f64(t), x0, history)
        rec["x_s"].append(x.numpy()[0].copy())
        rec["s"].append(s)
        rec["t"].append(t)
        rec["x0_s"].append(x0.numpy()[0].copy())
        rec["have_prev"].append(1 if history else 0)
        rec["x0_prev"].append(history[0][0].numpy()[0].copy() if history else np.full(64, np.nan))
        rec["s1"].append(float(history[0][1]) if history else np.nan)
        rec["x_t"].append(x_t.numpy()[0].copy())
        x, history = x_t, new_history
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez(OUT, **{k: np.asarray(v, dtype=np.int64 if k == "have_prev" else np.float64) for k, v in rec.items()})
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(rec['s'])} steps)")


if __name__ == "__main__":
    main()
