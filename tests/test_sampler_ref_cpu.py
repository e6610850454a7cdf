"""CPU: tests/sampler_ref.py (the denoise step restated with the reference's dtypes and devices) is anchored on diffusers' own known answer and
on oracle/sampler_oracle.py in its all-fp32 mode, and the host scalars of gen3c_amd/sampler.py:_coefficients are pinned to its literal
expressions - the seven coefficients exactly, and the `augment_sigma >= sigma` switch at the edges of the bf16 comparison."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import sampler_ref as sr
from tests.test_scheduler_kat_cpu import DIFFUSERS_FULL_LOOP_MEAN, DIFFUSERS_FULL_LOOP_SUM, DIFFUSERS_TOL, _diffusers_dummy_sample

f32, bf16 = torch.float32, torch.bfloat16
COEFFS = ("c_in_bf16", "c_skip_bf16", "c_out_bf16", "c_in_step", "c_skip", "c_out", "c_in_aug")


def _denoiser(num_steps):
    from gen3c_amd.sampler import Gen3CDenoiser
    den = Gen3CDenoiser(SimpleNamespace(is_context_parallel_enabled=False))
    den.scheduler.set_timesteps(num_steps)
    return den


def test_fp32_mode_reproduces_diffusers_full_loop_known_answer():
    """scale_model_input and step of sampler_ref, all-fp32, driven as diffusers' EDMEulerSchedulerTest.test_full_loop_no_noise (see
    tests/test_scheduler_kat_cpu.py for the configuration and the quoted constants): no condition region, guidance 0."""
    from gen3c_amd.sampler import EDMEulerScheduler
    sch = EDMEulerScheduler(sigma_max=80.0, sigma_min=0.002, sigma_data=0.5)
    sch.set_timesteps(10)
    x = _diffusers_dummy_sample().reshape(1, 4, 3, 8, 8) * sch.init_noise_sigma
    zeros, ind = torch.zeros_like(x), torch.zeros(1, 1, 3, 1, 1)
    for i, t in enumerate(sch.timesteps):
        out = sr.scale_model_input(x, sch.sigmas[i]) * t / (t + 1)  # the dummy model
        x = sr.step(out, out, x, zeros, ind, sch.sigmas[i], sch.sigmas[i + 1], guidance=0.0, dtype=f32)
    assert x.dtype == f32
    assert abs(float(x.abs().sum()) - DIFFUSERS_FULL_LOOP_SUM) < DIFFUSERS_TOL, float(x.abs().sum())
    assert abs(float(x.abs().mean()) - DIFFUSERS_FULL_LOOP_MEAN) < DIFFUSERS_TOL


@pytest.mark.parametrize("augment_sigma", [0.001, 0.5])
def test_fp32_mode_agrees_with_the_oracle_on_every_step(augment_sigma):
    """One loop iteration of sampler_ref in all-fp32 mode against oracle.sampler_oracle.denoise_step, at each of the 35 steps, on the oracle's own
    trajectory, with a stub network (elementwise in x, the timestep and 16 pose channels). The oracle hands its network the bf16-rounded
    timestep whatever its own dtype; the stub rounds it itself so that both see the same number. rtol 1e-5 is fp32 rounding of the handful
    of operations that the two write in a different order; atol covers cancellation in x + derivative * dt at the scale of the operands."""
    from oracle import sampler_oracle as so
    n_steps, seed, guidance = 35, 3, 1.7
    B, C, T, H, W = 1, 16, 3, 4, 5
    g = torch.Generator().manual_seed(11)
    gt = 0.5 * torch.randn(B, C, T, H, W, generator=g)
    pose = 0.5 * torch.randn(B, 64, T, H, W, generator=g)
    ind = torch.zeros(1, 1, T, 1, 1)
    ind[:, :, :1] = 1
    sig = so.karras_sigmas(n_steps)
    tim = 0.25 * torch.log(sig[:-1])
    noise = torch.from_numpy(np.random.RandomState(seed).standard_normal((B, C, T, H, W)).astype(np.float32))
    x = torch.randn(B, C, T, H, W, generator=g) * (so.SIGMA_MAX ** 2 + 1) ** 0.5

    def stub(inp, t, p):
        return torch.tanh(inp) * (1 + 0.1 * t.to(bf16).float()) + 0.05 * p[:, :16]

    for i in range(n_steps):
        ref = so.denoise_step(stub, x, i, gt, ind, pose, n_steps, guidance, augment_sigma, seed)
        got = sr.loop_iteration(lambda a, t: stub(a, t, pose), lambda a, t: stub(a, t, torch.zeros_like(pose)), x, gt, noise, ind, sig[i], sig[i + 1],
                                tim[i], guidance, augment_sigma, dtype=f32)
        assert got.dtype == f32
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6 * float(x.abs().max()), msg=lambda m: f"step {i}: {m}")
        x = ref


@pytest.mark.parametrize("num_steps", [10, 35, 50])
def test_host_coefficients_equal_the_literal_expressions(num_steps):
    den = _denoiser(num_steps)
    sig = den.scheduler.sigmas
    for i in range(num_steps):
        for aug in (0.001, 0.5):
            got = den._coefficients(sig[i], sig[i + 1], aug)
            want = sr.coefficients(sig[i], sig[i + 1], aug, device="cpu")
            assert set(got) == set(want)
            for k in COEFFS + ("sigma", "inv_sigma", "sigma_next"):
                assert got[k] == want[k], (num_steps, i, aug, k, got[k], want[k])
            assert got["indicator_off"] is want["indicator_off"], (num_steps, i, aug)


def test_indicator_off_is_the_bf16_tensor_comparison():
    """`if augment_sigma >= sigma` (model_v2w.py:229) with sigma a bf16 0-dim tensor: torch rounds the Python float to bf16 before it compares,
    so v * (1 - 1e-4) - which rounds back to v - counts as reached, while the bf16 value below v does not."""
    den = _denoiser(35)
    sig = den.scheduler.sigmas
    seen = set()
    for i in range(35):
        s_bf = sig[i].to(bf16)
        v = float(s_bf)
        below = float((s_bf.view(torch.int16) - 1).view(bf16))
        assert 0 < below < v
        for aug in (v, v * (1 - 1e-4), v * (1 + 1e-4), below):
            want = bool(aug >= s_bf)
            seen.add(want)
            assert den._coefficients(sig[i], sig[i + 1], aug)["indicator_off"] is want, (i, v, aug, want)
        assert bool(v * (1 - 1e-4) >= s_bf) and not bool(below >= s_bf)  # the property of torch that the edge rests on
    assert seen == {True, False}
