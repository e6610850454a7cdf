"""The denoise step under the opt-in solver "2ab" restated in plain torch with its dtypes (test infrastructure next to tests/sampler_ref.py, whose
pieces it uses; runs on any device, imports nothing from gen3c_amd). Everything up to the fp32 x0 prediction is sampler_ref.step's text; the update
is xt_next = bf16(a * x + (cb1 * x0 + cb2 * x0_prev)) with fp32 scalars, every operation a torch kernel of its own (one IEEE operation each)."""
import numpy as np
import torch

from tests import sampler_ref as sr


def x0_prediction(out_cond, out_uncond, new_xt, gt, indicator_effective, sigma32_cpu, guidance, dtype=torch.bfloat16):
    """sampler_ref.step up to and including pred_original_sample -> (sample fp32, x0 fp32)."""
    sigma = sr.model_sigma(sigma32_cpu, new_xt.device, dtype)
    latent = gt.to(dtype)
    indicator = indicator_effective.to(dtype)
    net_output = out_cond + guidance * (out_cond - out_uncond)
    latent_unscaled = (latent - sr.c_skip_of(sigma) * new_xt) / sr.c_out_of(sigma)
    new_output = indicator * latent_unscaled + (1 - indicator) * net_output
    sample = new_xt.to(torch.float32)
    sigma_hat = sr.sigma_hat_of(sigma32_cpu)
    return sample, sr.c_skip_of(sigma_hat) * sample + sr.c_out_of(sigma_hat) * new_output


def f32(v: float) -> float:
    """the fp32 value a C float argument takes"""
    return float(np.float32(v))


def step_2ab(out_cond, out_uncond, new_xt, gt, indicator_effective, sigma32_cpu, sigma_next32_cpu, guidance, x0_prev, coefficients):
    """-> (xt_next bf16, x0 fp32). x0_prev None: no history, the Euler step of sampler_ref. coefficients = (a, cb1, cb2) as Python floats."""
    sample, x0 = x0_prediction(out_cond, out_uncond, new_xt, gt, indicator_effective, sigma32_cpu, guidance)
    if x0_prev is None:
        return sr.step(out_cond, out_uncond, new_xt, gt, indicator_effective, sigma32_cpu, sigma_next32_cpu, guidance), x0
    a, cb1, cb2 = (f32(c) for c in coefficients)
    history = cb1 * x0 + cb2 * x0_prev
    return (a * sample + history).to(torch.bfloat16), x0


def step_2ab_fp64(sample, x0, x0_prev, coefficients):
    """The same update from the same fp32 inputs in fp64, rounded once to bf16."""
    a, cb1, cb2 = (f32(c) for c in coefficients)
    return (a * sample.double() + (cb1 * x0.double() + cb2 * x0_prev.double())).to(torch.bfloat16)
