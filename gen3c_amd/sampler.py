"""EDM-Euler sampling loop of GEN3C on the HIP path.

Mirrors (same names, argument meaning, CP behaviour):
  * diffusers 0.32.2 `EDMEulerScheduler(sigma_max=80, sigma_min=0.0002, sigma_data=0.5)` as used at
    cosmos_predict1/diffusion/model/model_t2w.py:65 (restated - diffusers is a third-party dependency that is not
    vendored in the reference; anchored on diffusers' own full-loop known answer, tests/test_scheduler_kat_cpu.py);
  * `DiffusionV2WModel.generate_samples_from_batch / _augment_noise_with_latent / _reverse_precondition_*`
    (model_v2w.py:84-155, 201-259) and `add_condition_video_indicator_and_video_input_mask` (model_v2w.py:32-82);
  * `VideoExtendCondition` (conditioner.py:107-134).

Per step the only device work outside the two network calls is two fused HIP kernels (csrc/sampler.hip). Scalar
coefficients are evaluated here on the host with 0-dim torch tensors in the SAME dtypes the reference's expressions
produce (several of them are bf16 because the loop's `sigma` is cast with `.to(**tensor_kwargs)`). The reference evaluates the
bf16 ones on the device; tests/test_sampler_kernels_gpu.py checks that the host gives the same numbers at every step.
tests/sampler_ref.py states the whole dtype chain - which operand is bf16 or fp32, on the device or a CPU 0-dim scalar - and
the kernels plus these scalars are held to it bit for bit.

Opt-in and outside that statement: solver "2ab" (Gen3CDenoiser.solver) - the second-order multistep update of the reference's
res_sampler.py in place of the Euler update, from the previous step's x0 prediction, in a third kernel (g3_edm_cfg_2ab_step_bf16).
Opt-in and outside it too: a guidance interval (Gen3CDenoiser.guidance_interval) - classifier-free guidance only while
sigma_lo < sigma <= sigma_hi (arXiv 2404.07724); a step outside it makes ONE network call at B, the conditional one, and its update runs in a
kernel that has no unconditional operand (g3_edm_cond_euler_step_bf16 / g3_edm_cond_2ab_step_bf16).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .dit import DataType, cacheable, tensor_version
from .parallel import cat_outputs_cp, cfg_exchange, split_inputs_cp


class EDMEulerScheduler:
    """Karras-rho EDM schedule + Euler step (diffusers 0.32.2 semantics, prediction_type='epsilon', final sigma 0)."""

    def __init__(self, sigma_max: float = 80.0, sigma_min: float = 0.0002, sigma_data: float = 0.5, rho: float = 7.0):
        self.sigma_max, self.sigma_min, self.sigma_data, self.rho = sigma_max, sigma_min, sigma_data, rho
        self.sigmas: Optional[torch.Tensor] = None
        self.timesteps: Optional[torch.Tensor] = None
        self.num_inference_steps: Optional[int] = None

    @property
    def init_noise_sigma(self) -> float:
        return (self.sigma_max ** 2 + 1) ** 0.5

    def set_timesteps(self, num_inference_steps: int):
        self.num_inference_steps = num_inference_steps
        ramp = torch.linspace(0, 1, num_inference_steps)
        min_inv_rho = self.sigma_min ** (1 / self.rho)
        max_inv_rho = self.sigma_max ** (1 / self.rho)
        sigmas = ((max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** self.rho).to(torch.float32)
        self.timesteps = 0.25 * torch.log(sigmas)  # precondition_noise
        self.sigmas = torch.cat([sigmas, torch.zeros(1, dtype=torch.float32)])

    def index_for_timestep(self, timestep: torch.Tensor) -> int:
        idx = (self.timesteps == timestep).nonzero()
        pos = 1 if len(idx) > 1 else 0
        return int(idx[pos].item())


SOLVERS = ("euler", "2ab")


def check_solver(name: str) -> str:
    if name not in SOLVERS:
        raise ValueError(f"sampler solver {name!r}: expected one of {SOLVERS}")
    return name


def check_guidance_interval(v) -> Optional[Tuple[float, float]]:
    """None (guide every step, the reference's loop), or (lo, hi) in sigma units with 0 <= lo < hi; hi may be inf. -> None / (float, float)."""
    if v is None:
        return None
    try:
        lo, hi = v
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"guidance interval {v!r}: expected None or (lo, hi) with 0 <= lo < hi (sigma units, hi may be inf)") from None
    if not (0.0 <= lo < hi) or math.isinf(lo):  # (a NaN fails the comparison)
        raise ValueError(f"guidance interval {v!r}: expected None or (lo, hi) with 0 <= lo < hi (sigma units, hi may be inf)")
    return lo, hi


def guided_steps(sigmas, interval) -> List[bool]:
    """Per step of the schedule `sigmas` (the scheduler's fp32 sigmas, the final 0 included or not: a sigma of 0 is no step): does the step apply
    classifier-free guidance? Step i does iff interval is None or lo < float(sigmas[i]) <= hi."""
    interval = check_guidance_interval(interval)
    sig = [float(v) for v in sigmas]
    if sig and sig[-1] == 0.0:
        sig = sig[:-1]
    return [interval is None or interval[0] < v <= interval[1] for v in sig]


def res_2ab_coefficients(s: float, t: float, s1: float) -> Tuple[float, float, float]:
    """(a, cb1, cb2) of one second-order multistep step from sigma s to sigma t with the previous step's sigma s1 (s1 > s > t > 0):
    x_t = a * x_s + cb1 * x0_s + cb2 * x0_s1. The Adams-Bashforth exponential integrator of arXiv 2308.02157 in the reference's form
    (functional/multi_step.py::order2_fn -> functional/runge_kutta.py::res_x0_rk2_step: time is -log sigma), in fp64 on the host."""
    ls, lt, lm = -math.log(s), -math.log(t), -math.log(s1)
    dt = lt - ls
    c2 = (lm - ls) / dt

    def phi1(u):
        return math.expm1(u) / u

    def phi2(u):
        return (phi1(u) - 1.0) / u

    return math.exp(-dt), dt * (phi1(-dt) - phi2(-dt) / c2), dt * phi2(-dt) / c2


@dataclass
class Res2abState:
    """What solver "2ab" carries from step to step of ONE sampling loop: the previous step's fp32 x0 prediction (this rank's shard, allocated by the
    first step, overwritten in place) and whether it holds one yet."""
    x0: Optional[torch.Tensor] = None
    have_prev: bool = False
    prev_guided: Optional[bool] = None  # under a guidance interval: whether the step that wrote x0 was guided


@dataclass
class VideoExtendCondition:
    """Field-for-field mirror of conditioner.py:107-134 (BaseVideoCondition + VideoExtendCondition)."""
    crossattn_emb: torch.Tensor
    crossattn_mask: Optional[torch.Tensor] = None
    data_type: DataType = DataType.VIDEO
    padding_mask: Optional[torch.Tensor] = None
    fps: Optional[torch.Tensor] = None
    num_frames: Optional[torch.Tensor] = None
    image_size: Optional[torch.Tensor] = None
    scalar_feature: Optional[torch.Tensor] = None
    frame_repeat: Optional[torch.Tensor] = None
    video_cond_bool: Optional[bool] = None
    gt_latent: Optional[torch.Tensor] = None
    condition_video_indicator: Optional[torch.Tensor] = None
    condition_video_input_mask: Optional[torch.Tensor] = None
    condition_video_augment_sigma: Optional[torch.Tensor] = None
    condition_video_pose: Optional[torch.Tensor] = None

    def to_dict(self) -> Dict[str, Optional[torch.Tensor]]:
        return {f.name: getattr(self, f.name) for f in fields(self)}


def arch_invariant_rand(shape, dtype, device, seed=None) -> torch.Tensor:
    """utils/misc.py:133-154: numpy RandomState normals (GPU-architecture independent)."""
    arr = np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
    return torch.from_numpy(arr).to(dtype=dtype, device=device)


def add_condition_video_indicator_and_video_input_mask(latent_state: torch.Tensor, condition: VideoExtendCondition,
                                                       num_condition_t: int) -> VideoExtendCondition:
    """model_v2w.py:32-82 (inference branch: first `num_condition_t` latent frames are the condition region)."""
    B, C, T, H, W = latent_state.shape
    assert num_condition_t is not None and num_condition_t <= T
    ind = torch.zeros(1, 1, T, 1, 1, device=latent_state.device, dtype=latent_state.dtype)
    ind[:, :, :num_condition_t] += 1.0
    condition.gt_latent = latent_state
    condition.condition_video_indicator = ind
    assert condition.video_cond_bool is not None, "video_cond_bool should be set"
    if condition.video_cond_bool:
        condition.condition_video_input_mask = ind.expand(B, 1, T, H, W).contiguous()
    else:
        condition.condition_video_input_mask = torch.zeros((B, 1, T, H, W), dtype=latent_state.dtype, device=latent_state.device)
    return condition


class Gen3CDenoiser:
    """The sampling half of `DiffusionGen3CModel` (model_gen3c.py:26-139 on top of model_v2w.py / model_t2w.py).

    `net` is a gen3c_amd.dit.VideoExtendGeneralDIT. Conditions are VideoExtendCondition objects that already carry
    `condition_video_pose` (the tokenizer-encoded warp buffers; zeros for the unconditional branch)."""

    def __init__(self, net, sigma_data: float = 0.5, state_shape=(16, 16, 88, 160)):
        self.net = net
        self.sigma_data = sigma_data
        self.state_shape = list(state_shape)
        self.scheduler = EDMEulerScheduler(sigma_max=80, sigma_min=0.0002, sigma_data=sigma_data)
        self._noise_cache: Dict[tuple, torch.Tensor] = {}
        self._fused_cache = None
        self.fuse_cond_uncond = os.environ.get("G3_FUSE_COND_UNCOND", "1") != "0"  # one batched forward for the conditional and the unconditional branch of a step (False: two calls)
        self.cfg_group = None  # CFG-parallel (opt-in): the pair of ranks that run the two guidance branches of a step, see enable_cfg_parallel
        self.solver = "euler"  # "2ab" (opt-in): second-order multistep update from the previous step's x0 prediction, outside the parity statement
        self.guidance_interval = None  # (lo, hi) (opt-in): guidance only while lo < sigma <= hi, one network call per step outside; outside the parity statement

    @property
    def solver(self) -> str:
        return self._solver

    @solver.setter
    def solver(self, name: str) -> None:
        self._solver = check_solver(name)

    @property
    def guidance_interval(self) -> Optional[Tuple[float, float]]:
        return self._guidance_interval

    @guidance_interval.setter
    def guidance_interval(self, v) -> None:
        self._guidance_interval = check_guidance_interval(v)

    def enable_cfg_parallel(self, group) -> None:
        """CFG-parallel: `group` is a 2-rank torch.distributed group (parallel_state.get_cfg_parallel_group()). Its rank 0 runs the conditional
        branch of every step, its rank 1 the unconditional one, each as ONE network call at B; the outputs are exchanged (parallel.cfg_exchange)
        and both ranks run the same CFG / Euler kernel on the same bytes, so both end the step with bit-identical xt. The network call of a
        branch is the call the two-call form makes, hence the step is bit-identical to fuse_cond_uncond=False (and to the fused form, which is
        pinned to it). Context parallelism, if enabled on the net, shards the frames of each branch over the net's own CP group as before."""
        assert dist.get_world_size(group) == 2, "classifier-free guidance has two branches"
        self.cfg_group = group

    def disable_cfg_parallel(self) -> None:
        self.cfg_group = None

    # ---- host-side scalar algebra, in the reference's dtypes ------------------------------------------------------
    def _coefficients(self, sigma32: torch.Tensor, sigma_next32: torch.Tensor, augment_sigma: float) -> dict:
        sd = self.sigma_data
        s_bf = sigma32.to(torch.bfloat16)  # `sigma = ....to(**self.tensor_kwargs)` (model_v2w.py:132)
        c_in_bf16 = 1 / ((s_bf ** 2 + sd ** 2) ** 0.5)                    # model_v2w.py:250 (bf16 0-dim tensor)
        c_skip_bf16 = sd ** 2 / (s_bf ** 2 + sd ** 2)                      # model_v2w.py:256
        c_out_bf16 = s_bf * sd / (s_bf ** 2 + sd ** 2) ** 0.5              # model_v2w.py:257
        c_in_step = 1 / ((sigma32 ** 2 + sd ** 2) ** 0.5)                  # scheduler.precondition_inputs (fp32)
        c_skip = sd ** 2 / (sigma32 ** 2 + sd ** 2)                        # scheduler.precondition_outputs
        c_out = sigma32 * sd / (sigma32 ** 2 + sd ** 2) ** 0.5
        c_in_aug = 1 / ((augment_sigma ** 2 + sd ** 2) ** 0.5)             # python floats
        # scheduler.step divides an fp32 device tensor by its fp32 CPU 0-dim sigma: torch's device kernel takes the reciprocal of a CPU
        # scalar divisor on the host, in fp32, and multiplies (measured: bitwise that, and not the true quotient)
        inv_sigma = torch.ones((), dtype=torch.float32) / sigma32
        # `if augment_sigma >= sigma` (model_v2w.py:229) compares a Python float with the bf16 0-dim tensor: torch rounds the float to
        # bf16 first, so an augment sigma just under the step's bf16 sigma compares equal and switches the condition region off
        indicator_off = bool(augment_sigma >= s_bf)
        return dict(c_in_bf16=float(c_in_bf16), c_skip_bf16=float(c_skip_bf16), c_out_bf16=float(c_out_bf16),
                    c_in_step=float(c_in_step), c_skip=float(c_skip), c_out=float(c_out), c_in_aug=float(c_in_aug),
                    sigma=float(sigma32), inv_sigma=float(inv_sigma), sigma_next=float(sigma_next32), indicator_off=indicator_off)

    @staticmethod
    def _fused_cond_uncond_kwargs(condition: "VideoExtendCondition", uncondition: "VideoExtendCondition", B: int) -> Optional[dict]:
        """Keyword arguments of one net call over [cond batch | uncond batch], or None when the two conditions cannot share a call
        (different shapes / flags). Per-sample tensors (leading dim B) are concatenated; broadcast tensors (leading dim 1) and non-tensors
        must agree and are passed once."""
        dc, du = condition.to_dict(), uncondition.to_dict()
        out = {}
        for k, vc in dc.items():
            vu = du.get(k)
            if isinstance(vc, torch.Tensor) and isinstance(vu, torch.Tensor):
                if vc.shape != vu.shape or vc.dtype != vu.dtype:
                    return None
                if k == "gt_latent":  # not an input of the net
                    out[k] = vc
                elif vc.dim() >= 1 and vc.shape[0] == B:
                    out[k] = torch.cat([vc, vu], dim=0)
                elif vc.dim() >= 1 and vc.shape[0] == 1 and B != 1:
                    if not torch.equal(vc, vu):
                        return None
                    out[k] = vc
                else:
                    out[k] = torch.cat([vc, vu], dim=0) if vc.dim() >= 1 else vc
            elif vc is None and vu is None:
                out[k] = None
            elif isinstance(vc, torch.Tensor) or isinstance(vu, torch.Tensor):
                return None
            else:
                if vc != vu:
                    return None
                out[k] = vc
        return out

    def _augment_noise(self, shape, device, seed: int) -> torch.Tensor:
        key = (tuple(shape), str(device), seed)
        if key not in self._noise_cache:  # the reference regenerates the SAME numpy normals every step (seeded)
            self._noise_cache = {key: arch_invariant_rand(shape, torch.float32, device, seed)}
        return self._noise_cache[key]

    # ---- one denoise step (the unit bench.py times) ----------------------------------------------------------------
    @torch.no_grad()
    def denoise_step(self, xt: torch.Tensor, step_index: int, condition: VideoExtendCondition,
                     uncondition: VideoExtendCondition, guidance: float, condition_augment_sigma: float,
                     seed: int, *, solver_state: Optional[Res2abState] = None, guided: bool = True) -> torch.Tensor:
        """model_v2w.py:130-149 for scheduler step `step_index`; xt is this rank's [B,C,T_local,H,W] bf16 shard. `solver_state` (None: the
        reference's Euler update) is the loop's state under solver "2ab": the step's x0 prediction is kept in it, and a step that has a previous one
        and does not end at sigma 0 takes the second-order update instead (the step to sigma 0 returns x0 either way: -log 0 has no 2ab form).
        `guided` (True: the reference's step) is False for a step outside the guidance interval: ONE network call at B, the conditional one - the
        first call of the two-call form, on every rank of a CFG-parallel pair, no exchange - and the cond entry of the solver in force; `uncondition`,
        `guidance` and the fused-call cache are not looked at. Under "2ab" a step whose guidedness differs from the previous step's ignores the
        history (the extrapolation assumes one smooth denoiser; the two predictions differ by g (c - u)), takes the Euler update and stores its x0."""
        sch = self.scheduler
        sigma32, sigma_next32 = sch.sigmas[step_index], sch.sigmas[step_index + 1]
        co = self._coefficients(sigma32, sigma_next32, condition_augment_sigma)
        to_cp = self.net.is_context_parallel_enabled
        gt = condition.gt_latent
        ind = condition.condition_video_indicator.float()
        if co["indicator_off"]:
            ind = torch.zeros_like(ind)  # `if augment_sigma >= sigma: indicator = zeros` (model_v2w.py:229-230)
        noise = self._augment_noise(gt.shape, gt.device, seed)
        if to_cp:
            gt = split_inputs_cp(gt, 2, self.net.cp_group)
            ind = split_inputs_cp(ind, 2, self.net.cp_group)
            noise = split_inputs_cp(noise, 2, self.net.cp_group)
        B, C, T, H, W = xt.shape
        ind_t = ind.reshape(-1).contiguous()
        xt = xt.to(torch.bfloat16).contiguous()
        gt = gt.to(torch.bfloat16).contiguous()
        new_xt, new_xt_scaled = ops.edm_prepare_input(xt, gt, noise.contiguous(), ind_t, T, H * W, condition_augment_sigma,
                                                      co["c_in_aug"], co["c_in_bf16"], co["c_in_step"])
        t = sch.timesteps[step_index].to(device=xt.device, dtype=torch.bfloat16)
        st = solver_state
        # the history of a step on the other side of an interval boundary is another denoiser's: not used (never so without an interval)
        have_prev = st is not None and st.have_prev and st.prev_guided in (None, guided)
        if not guided:
            out_c = self.net(x=new_xt_scaled, timesteps=t, **condition.to_dict())
            if st is None or co["sigma_next"] == 0.0:
                return ops.edm_cond_euler_step(out_c, new_xt, gt, ind_t, T, H * W, co["c_skip_bf16"], co["c_out_bf16"], co["c_skip"], co["c_out"],
                                               co["sigma"], co["inv_sigma"], co["sigma_next"])
            if st.x0 is None:
                st.x0 = torch.empty(new_xt.shape, dtype=torch.float32, device=new_xt.device)
            a, cb1, cb2 = res_2ab_coefficients(co["sigma"], co["sigma_next"], float(sch.sigmas[step_index - 1])) if have_prev else (0.0, 0.0, 0.0)
            out = ops.edm_cond_2ab_step(out_c, new_xt, gt, ind_t, T, H * W, co["c_skip_bf16"], co["c_out_bf16"], co["c_skip"], co["c_out"],
                                        co["sigma"], co["inv_sigma"], co["sigma_next"], st.x0, have_prev, a, cb1, cb2)
            st.have_prev, st.prev_guided = True, False
            return out
        fused = None
        if self.fuse_cond_uncond and self.cfg_group is None:
            # the conditions are the same objects for all steps of a chunk: build the batched arguments once (this also keeps the DiT's
            # per-context cross-attention K / V cache valid, which is keyed on the context tensor)
            # identity AND content version of every value: an in-place edit of a condition tensor between steps / chunks (crossattn_emb.copy_,
            # a refilled pose buffer) must rebuild the concatenated copies, exactly as the DiT's own K / V cache does
            def _ident(v):
                return (id(v), v.data_ptr(), tensor_version(v)) if isinstance(v, torch.Tensor) else (id(v),)
            key = (B,) + tuple(_ident(v) for v in condition.to_dict().values()) + tuple(_ident(v) for v in uncondition.to_dict().values())
            fc = self._fused_cache
            if not cacheable(*condition.to_dict().values(), *uncondition.to_dict().values()):
                # inference tensors carry no version counter: an in-place edit would go unnoticed -> rebuild the batched arguments every step
                fc = (key, self._fused_cond_uncond_kwargs(condition, uncondition, B))
            elif fc is None or fc[0] != key:
                # (the cache entry keeps the condition objects alive, so the ids in the key cannot be recycled while it is valid)
                fc = self._fused_cache = (key, self._fused_cond_uncond_kwargs(condition, uncondition, B), condition.to_dict(), uncondition.to_dict())
            fused = fc[1]
        if self.cfg_group is not None:
            # CFG-parallel: this rank's branch only, at B (the fused-call cache is not consulted); the exchange is the step's one collective
            # besides the net's own context-parallel ones
            branch = condition if dist.get_rank(self.cfg_group) == 0 else uncondition
            out_c, out_u = cfg_exchange(self.net(x=new_xt_scaled, timesteps=t, **branch.to_dict()), self.cfg_group)
        elif fused is not None:
            # the conditional and the unconditional forward (model_v2w.py:137-141: two net calls) as ONE forward over a batch of 2 B: every
            # row is computed exactly as in its own call (GEMM / attention / norm kernels work row-, head- and batch-wise), but the chip sees
            # launches twice as long - 55 instead of 27.5 rounds of attention workgroups, no half-empty last round - and half as many of them
            out = self.net(x=torch.cat([new_xt_scaled, new_xt_scaled], dim=0), timesteps=t, **fused)
            out_c, out_u = out[:B], out[B:]
        else:
            out_c = self.net(x=new_xt_scaled, timesteps=t, **condition.to_dict())
            out_u = self.net(x=new_xt_scaled, timesteps=t, **uncondition.to_dict())
        if solver_state is None or co["sigma_next"] == 0.0:
            return ops.edm_cfg_euler_step(out_c, out_u, new_xt, gt, ind_t, T, H * W, guidance, co["c_skip_bf16"], co["c_out_bf16"],
                                          co["c_skip"], co["c_out"], co["sigma"], co["inv_sigma"], co["sigma_next"])
        if st.x0 is None:
            st.x0 = torch.empty(new_xt.shape, dtype=torch.float32, device=new_xt.device)
        a, cb1, cb2 = res_2ab_coefficients(co["sigma"], co["sigma_next"], float(sch.sigmas[step_index - 1])) if have_prev else (0.0, 0.0, 0.0)
        out = ops.edm_cfg_2ab_step(out_c, out_u, new_xt, gt, ind_t, T, H * W, guidance, co["c_skip_bf16"], co["c_out_bf16"], co["c_skip"],
                                   co["c_out"], co["sigma"], co["inv_sigma"], co["sigma_next"], st.x0, have_prev, a, cb1, cb2)
        st.have_prev, st.prev_guided = True, True
        return out

    @torch.no_grad()
    def generate_samples_from_batch(self, condition: VideoExtendCondition, uncondition: VideoExtendCondition,
                                    guidance: float = 1.0, seed: int = 1, state_shape=None, n_sample: int = 1,
                                    num_steps: int = 35, condition_augment_sigma: float = 0.001,
                                    xt: Optional[torch.Tensor] = None, solver: Optional[str] = None, guidance_interval=None) -> torch.Tensor:
        """Sampling loop of model_v2w.py:84-155 given ready conditions. `xt` (optional) injects the initial noise
        (already multiplied by init_noise_sigma) - torch.randn on the device is not reproducible across vendors, parity
        runs inject it (SURVEY.md 7 'RNG parity'). `solver` (None: self.solver): "euler" is the reference's loop; "2ab" (opt-in, DESIGN.md
        section 12) keeps the x0 prediction of the previous step for the length of this call and takes second-order steps from it.
        `guidance_interval` (None: self.guidance_interval; that None too: every step guided, the reference's loop): (lo, hi) in sigma units - the steps
        with lo < sigma <= hi are guided, the others run the conditional branch alone (opt-in)."""
        solver = self.solver if solver is None else check_solver(solver)
        interval = self.guidance_interval if guidance_interval is None else check_guidance_interval(guidance_interval)
        state_shape = list(state_shape or self.state_shape)
        self.scheduler.set_timesteps(num_steps)
        dev = condition.gt_latent.device
        if xt is None:
            g = torch.Generator(device=dev).manual_seed(seed)
            xt = torch.randn((n_sample, *state_shape), device=dev, dtype=torch.bfloat16, generator=g) * self.scheduler.init_noise_sigma
        to_cp = self.net.is_context_parallel_enabled
        if to_cp:
            xt = split_inputs_cp(xt, 2, self.net.cp_group)
        if interval is not None:
            state = Res2abState() if solver == "2ab" else None
            for i, guided in enumerate(guided_steps(self.scheduler.sigmas, interval)):
                xt = self.denoise_step(xt, i, condition, uncondition, guidance, condition_augment_sigma, seed, solver_state=state, guided=guided)
        elif solver == "euler":
            for i in range(num_steps):
                xt = self.denoise_step(xt, i, condition, uncondition, guidance, condition_augment_sigma, seed)
        else:
            state = Res2abState()  # lives for this call only: a new chunk never sees the previous chunk's history
            for i in range(num_steps):
                xt = self.denoise_step(xt, i, condition, uncondition, guidance, condition_augment_sigma, seed, solver_state=state)
        if to_cp:
            xt = cat_outputs_cp(xt, 2, self.net.cp_group)
        return xt
