"""The EDM-Euler denoise step of the GEN3C sampler restated expression by expression WITH its dtypes and devices (test infrastructure:
plain torch, runs on any device, imports nothing from gen3c_amd). It is the statement of the dtype chain that csrc/sampler.hip and
gen3c_amd/sampler.py:_coefficients follow; oracle/sampler_oracle.py is the same arithmetic with no rounding points.

What is restated: one iteration of the sampling loop (cosmos_predict1/diffusion/model/model_v2w.py:130-149 with its helpers :201-259) and
the arithmetic of diffusers 0.32.2 EDMEulerScheduler.scale_model_input / precondition_inputs / precondition_outputs / step (cited below as
`edm_euler:<method>`; diffusers is a third-party dependency, the restatement is anchored on diffusers' own full-loop known answer in
tests/test_sampler_ref_cpu.py).

Where every value lives in the reference (and therefore here), because torch's type promotion and its device kernels depend on it:
  * `sigma` of the model's own expressions is `scheduler.sigmas[i].to(**tensor_kwargs)`: a bf16 0-dim tensor ON THE COMPUTE DEVICE (:132);
  * the scheduler's `sigmas` and everything derived inside the scheduler (c_in, c_skip, c_out, sigma_hat, dt) are fp32 0-dim tensors ON THE
    CPU (`set_timesteps(num_steps)` is called without a device, :121). A CPU 0-dim operand does not take part in type promotion against a
    tensor with dimensions and reaches a device kernel as an fp32 scalar argument;
  * `guidance` and `condition_augment_sigma` are Python floats;
  * `condition_video_indicator` is a bf16 [1,1,T,1,1] tensor; the augmentation noise is an fp32 tensor (:232-237).
`dtype=torch.float32` runs the same expressions with every bf16 replaced by fp32 (the reference's tensor_kwargs dtype)."""
import torch

SIGMA_DATA = 0.5


# ---- scalar coefficient expressions (the argument decides dtype and device) -----------------------------------------------------------
def c_in_of(sigma):
    """:250 `_reverse_precondition_input` and edm_euler:precondition_inputs - the same text in both."""
    return 1 / ((sigma ** 2 + SIGMA_DATA ** 2) ** 0.5)


def c_skip_of(sigma):
    """:256 `_reverse_precondition_output` and edm_euler:precondition_outputs."""
    return SIGMA_DATA ** 2 / (sigma ** 2 + SIGMA_DATA ** 2)


def c_out_of(sigma):
    """:257 and edm_euler:precondition_outputs (prediction_type 'epsilon')."""
    return sigma * SIGMA_DATA / (sigma ** 2 + SIGMA_DATA ** 2) ** 0.5


def model_sigma(sigma32_cpu, device, dtype=torch.bfloat16):
    """:132 `sigma = self.scheduler.sigmas[step_index].to(**self.tensor_kwargs)`."""
    return sigma32_cpu.to(device=device, dtype=dtype)


def sigma_hat_of(sigma32_cpu):
    """edm_euler:step with s_churn = 0: gamma is the Python float 0.0 and sigma_hat = sigma * (gamma + 1), fp32 on the CPU."""
    gamma = 0.0
    return sigma32_cpu * (gamma + 1)


def indicator_off(sigma32_cpu, augment_sigma, device, dtype=torch.bfloat16) -> bool:
    """:229 `if augment_sigma >= sigma` - a Python float against the 0-dim `sigma` tensor: torch casts the float to the tensor's dtype."""
    return bool(augment_sigma >= model_sigma(sigma32_cpu, device, dtype))


def coefficients(sigma32_cpu, sigma_next32_cpu, augment_sigma, device="cpu", dtype=torch.bfloat16) -> dict:
    """Every scalar of one step as a Python float, each evaluated by the literal expression on the device / in the dtype the reference has.
    `inv_sigma` is no expression of the reference: it is what torch's device kernel makes of `/ sigma_hat` in edm_euler:step, where the divisor is a
    CPU 0-dim tensor (aten's true-division kernel takes 1 / b on the host in fp32 and multiplies; step() below leaves that to torch)."""
    s_model = model_sigma(sigma32_cpu, device, dtype)
    s_hat = sigma_hat_of(sigma32_cpu)
    return dict(c_in_bf16=float(c_in_of(s_model)), c_skip_bf16=float(c_skip_of(s_model)), c_out_bf16=float(c_out_of(s_model)),
                c_in_step=float(c_in_of(sigma32_cpu)), c_skip=float(c_skip_of(s_hat)), c_out=float(c_out_of(s_hat)),
                c_in_aug=float(c_in_of(augment_sigma)), sigma=float(s_hat), inv_sigma=float(1 / s_hat), sigma_next=float(sigma_next32_cpu),
                indicator_off=indicator_off(sigma32_cpu, augment_sigma, device, dtype))


# ---- the two elementwise halves of a step -----------------------------------------------------------------------------------------------
def effective_indicator(indicator, sigma32_cpu, augment_sigma, dtype=torch.bfloat16):
    """:228-230: the condition region is switched off once the step's sigma has come down to the augmentation sigma."""
    indicator = indicator.to(dtype)
    if indicator_off(sigma32_cpu, augment_sigma, indicator.device, dtype):
        indicator = torch.zeros_like(indicator)
    return indicator


def scale_model_input(sample, sigma32_cpu):
    """edm_euler:scale_model_input -> precondition_inputs(sample, self.sigmas[step_index]): tensor * fp32 CPU 0-dim, result in sample's dtype."""
    return sample * c_in_of(sigma32_cpu)


def prepare(xt, gt, noise, indicator, sigma32_cpu, augment_sigma, dtype=torch.bfloat16):
    """model_v2w.py:132-139: the network input of one step. xt, gt [B,C,T,H,W]; noise fp32, same shape; indicator [1,1,T,1,1];
    sigma32_cpu the scheduler's fp32 CPU sigma of the step. -> (new_xt, new_xt_scaled)."""
    sigma = model_sigma(sigma32_cpu, xt.device, dtype)                       # :132
    xt = xt.to(dtype)                                                        # :134
    latent = gt.to(dtype)                                                    # :227 condition.gt_latent (tensor_kwargs dtype)
    indicator = effective_indicator(indicator, sigma32_cpu, augment_sigma, dtype)  # :228-230
    augment_latent = latent + noise * augment_sigma                          # :238  bf16 + fp32 * float -> fp32
    augment_latent = augment_latent * c_in_of(augment_sigma)                 # :239  edm_euler:precondition_inputs with a Python float sigma
    augment_latent_unscaled = augment_latent / c_in_of(sigma)                # :250-251  fp32 tensor / bf16 0-dim device tensor -> fp32
    new_xt = indicator * augment_latent_unscaled + (1 - indicator) * xt      # :246  bf16*fp32 -> fp32; bf16*bf16 -> bf16; sum fp32
    new_xt = new_xt.to(dtype)                                                # :138
    return new_xt, scale_model_input(new_xt, sigma32_cpu)                    # :139


def step(out_cond, out_uncond, new_xt, gt, indicator_effective, sigma32_cpu, sigma_next32_cpu, guidance, dtype=torch.bfloat16):
    """model_v2w.py:144-149: classifier-free guidance, replacement of the condition frames, and EDMEulerScheduler.step. `indicator_effective` is
    what effective_indicator() returned for this step. -> xt_next."""
    sigma = model_sigma(sigma32_cpu, new_xt.device, dtype)                   # :132
    latent = gt.to(dtype)
    indicator = indicator_effective.to(dtype)
    net_output = out_cond + guidance * (out_cond - out_uncond)               # :144  three ops in the network's dtype
    latent_unscaled = (latent - c_skip_of(sigma) * new_xt) / c_out_of(sigma)  # :256-258  0-dim device tensors: all in `dtype`
    new_output = indicator * latent_unscaled + (1 - indicator) * net_output  # :147
    # edm_euler:step(new_output, t, new_xt)
    sample = new_xt.to(torch.float32)                                        # "upcast to avoid precision issues"
    sigma_hat = sigma_hat_of(sigma32_cpu)                                    # fp32 CPU 0-dim
    pred_original_sample = c_skip_of(sigma_hat) * sample + c_out_of(sigma_hat) * new_output  # precondition_outputs: fp32 + (fp32 CPU 0-dim * bf16 -> bf16)
    derivative = (sample - pred_original_sample) / sigma_hat                 # fp32 tensor / fp32 CPU 0-dim
    dt = sigma_next32_cpu - sigma_hat                                        # fp32 CPU 0-dim
    prev_sample = sample + derivative * dt
    return prev_sample.to(new_output.dtype)                                  # "cast sample back to model compatible dtype"


def loop_iteration(net_cond, net_uncond, xt, gt, noise, indicator, sigma32_cpu, sigma_next32_cpu, timestep32_cpu, guidance, augment_sigma,
                   dtype=torch.bfloat16):
    """model_v2w.py:130-149 around two network callables `net(x, timesteps) -> output`; timestep32_cpu is scheduler.timesteps[i]."""
    new_xt, new_xt_scaled = prepare(xt, gt, noise, indicator, sigma32_cpu, augment_sigma, dtype)
    t = timestep32_cpu.to(device=xt.device, dtype=dtype)                     # :141
    out_cond = net_cond(new_xt_scaled, t)                                    # :142
    out_uncond = net_uncond(new_xt_scaled, t)                                # :143
    ind = effective_indicator(indicator.to(xt.device), sigma32_cpu, augment_sigma, dtype)
    return step(out_cond, out_uncond, new_xt, gt, ind, sigma32_cpu, sigma_next32_cpu, guidance, dtype)
