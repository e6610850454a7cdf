"""csrc/sampler.hip through gen3c_amd.ops, and the host scalars of Gen3CDenoiser._coefficients that ship with it, against tests/sampler_ref.py
run ON THE DEVICE: the denoise step restated with the reference's dtypes and tensor placements (bf16 0-dim sigma on the device, the
scheduler's fp32 0-dim scalars on the CPU, Python-float guidance and augment sigma). Every comparison is torch.equal: the kernels claim the
reference's rounding points, not a tolerance. torch.equal is value equality, so +0 and -0 compare equal - deliberately: where the indicator is 0
the kernels pass x through and keep a -0, while torch's 0 * a + 1 * (-0) gives +0; sign bits of zero are not pinned.

Inputs are built on the CPU from seeded generators and cached; the reference is computed per case on the device (a few small torch kernels)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import sampler_ref as sr

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
NUM_STEPS = 35
# (B, C, T, H, W) -> per-frame condition indicator
SHAPES = {
    (1, 1, 1, 1, 1): [1],                 # n = 1: the single-thread tail
    (2, 3, 4, 3, 5): [1, 1, 0, 0],        # n = 360: a partial block; odd hw, frame boundaries fall mid-wave
    (1, 16, 5, 7, 9): [1, 0, 1, 0, 0],    # non-prefix frame pattern: a wrong (i / hw) % T, or C and T swapped, shows at once
    (2, 16, 3, 61, 91): [1, 0, 1],        # n = 532 896 > 2048 * 256: the grid-stride loop runs, with a ragged last pass
}
STEPS = [0, 10, 25, 33, 34]               # 34: sigma_next = 0
AUGMENT_SIGMAS = [0.001, 0.5]             # 0.5 switches the condition region off from mid-schedule on
GUIDANCES = [0.0, 1.0, 1.7, 7.5]          # 1.7 is not representable in bf16


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _denoiser():
    from gen3c_amd.sampler import Gen3CDenoiser
    den = Gen3CDenoiser(SimpleNamespace(is_context_parallel_enabled=False))
    den.scheduler.set_timesteps(NUM_STEPS)
    return den


@functools.lru_cache(maxsize=None)
def _inputs(shape, step):
    """xt ~ N(0, sigma^2 + 1) with exact +-0 and +-3 sigma_max planted; gt ~ N(0, 0.25) with a zero frame (frame 0, a condition frame, where
    there is more than one); out_uncond equal to out_cond on the last frame (cond - uncond = 0 there); fp32 noise. All on the device."""
    B, C, T, H, W = shape
    n = B * C * T * H * W
    g = torch.Generator().manual_seed(1000 * n + step)
    sigma = float(_denoiser().scheduler.sigmas[step])
    xt = (torch.randn(shape, generator=g) * (sigma ** 2 + 1) ** 0.5).to(bf16)
    if n >= 16:
        flat = xt.view(-1)
        flat[[1, n // 3]] = 0.0
        flat[[2, n // 3 + 1]] = -0.0
        flat[[3, n // 2]] = 240.0    # 3 * sigma_max
        flat[[4, n - 1]] = -240.0
    gt = (0.5 * torch.randn(shape, generator=g)).to(bf16)
    if T > 1:
        gt[:, :, 0] = 0
    oc = torch.randn(shape, generator=g).to(bf16)
    ou = torch.randn(shape, generator=g).to(bf16)
    ou[:, :, T - 1] = oc[:, :, T - 1]
    noise = torch.randn(shape, generator=g)
    ind = torch.tensor(SHAPES[shape], dtype=bf16).reshape(1, 1, T, 1, 1)
    return tuple(t.to(_dev()) for t in (xt, gt, oc, ou, noise, ind))


def _kernel_indicator(ind, co):
    """what denoise_step hands the kernels: the fp32 indicator, zeroed by the host when augment_sigma >= sigma"""
    ind = ind.float()
    if co["indicator_off"]:
        ind = torch.zeros_like(ind)
    return ind.reshape(-1).contiguous()


def _prepare(xt, gt, noise, ind, co, aug):
    from gen3c_amd import ops
    T, hw = xt.shape[2], xt.shape[3] * xt.shape[4]
    return ops.edm_prepare_input(xt, gt, noise, _kernel_indicator(ind, co), T, hw, aug, co["c_in_aug"], co["c_in_bf16"], co["c_in_step"])


def _step(oc, ou, new_xt, gt, ind, co, guidance):
    from gen3c_amd import ops
    T, hw = new_xt.shape[2], new_xt.shape[3] * new_xt.shape[4]
    return ops.edm_cfg_euler_step(oc, ou, new_xt, gt, _kernel_indicator(ind, co), T, hw, guidance, co["c_skip_bf16"], co["c_out_bf16"],
                                  co["c_skip"], co["c_out"], co["sigma"], co["inv_sigma"], co["sigma_next"])


def _ulps(a, b):
    """distance in bf16 steps between two finite bf16 tensors (ordered-integer view)"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def _assert_equal(got, ref, what):
    assert got.dtype == ref.dtype == bf16 and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref).reshape(-1).nonzero().reshape(-1)
        d = _ulps(got.reshape(-1)[bad], ref.reshape(-1)[bad])
        first = [(int(i), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i])) for i in bad[:5]]
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ, up to {int(d.max())} bf16 ulp; (index, got, ref): {first}")


def _sigmas(step):
    sig = _denoiser().scheduler.sigmas
    assert sig.device.type == "cpu" and sig.dtype == f32  # the placement the reference has (set_timesteps without a device)
    return sig[step], sig[step + 1]


@pytest.mark.parametrize("aug", AUGMENT_SIGMAS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_prepare_input_equals_the_reference_dtype_chain(shape, step, aug):
    xt, gt, oc, ou, noise, ind = _inputs(shape, step)
    s, s_next = _sigmas(step)
    co = _denoiser()._coefficients(s, s_next, aug)
    new_xt, new_xt_scaled = _prepare(xt, gt, noise, ind, co, aug)
    ref_xt, ref_scaled = sr.prepare(xt, gt, noise, ind, s, aug)
    _assert_equal(new_xt, ref_xt, "new_xt")
    _assert_equal(new_xt_scaled, ref_scaled, "new_xt_scaled")


@pytest.mark.parametrize("guidance", GUIDANCES)
@pytest.mark.parametrize("aug", AUGMENT_SIGMAS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_cfg_euler_step_equals_the_reference_dtype_chain(shape, step, aug, guidance):
    xt, gt, oc, ou, noise, ind = _inputs(shape, step)
    s, s_next = _sigmas(step)
    co = _denoiser()._coefficients(s, s_next, aug)
    new_xt, _ = sr.prepare(xt, gt, noise, ind, s, aug)  # the reference's own network input: this test judges the step kernel alone
    got = _step(oc, ou, new_xt, gt, ind, co, guidance)
    ref = sr.step(oc, ou, new_xt, gt, sr.effective_indicator(ind, s, aug), s, s_next, guidance)
    _assert_equal(got, ref, "xt_next")


def test_host_coefficients_equal_their_evaluation_on_the_device():
    """The model's own coefficients come from a bf16 0-dim sigma ON THE DEVICE in the reference; _coefficients evaluates them on the host. Both must
    give the same numbers at every step (bf16 pow / sqrt / reciprocal / multiply of single values), and the same `augment_sigma >= sigma`."""
    den = _denoiser()
    sig = den.scheduler.sigmas
    for i in range(NUM_STEPS):
        s_bf = sig[i].to(bf16)
        edges = [float(s_bf), float(s_bf) * (1 - 1e-4), float(s_bf) * (1 + 1e-4), float((s_bf.view(torch.int16) - 1).view(bf16))]
        for aug in AUGMENT_SIGMAS + edges:
            got = den._coefficients(sig[i], sig[i + 1], aug)
            want = sr.coefficients(sig[i], sig[i + 1], aug, device=_dev())
            assert got == want, (i, aug, {k: (got[k], want[k]) for k in got if got[k] != want[k]})


@pytest.mark.parametrize("aug", AUGMENT_SIGMAS)
@pytest.mark.parametrize("step", [10, 25, 34])
def test_rank_local_frame_slices_equal_the_whole_tensor(step, aug):
    """What a context-parallel rank computes after split_inputs_cp: both kernels on the frame slices [0:2] and [2:5] of the T = 5 case, the
    indicator sliced to match, must give the matching slices of the whole-tensor result bit for bit (and the whole equals the reference)."""
    shape, guidance = (1, 16, 5, 7, 9), 1.7
    xt, gt, oc, ou, noise, ind = _inputs(shape, step)
    s, s_next = _sigmas(step)
    co = _denoiser()._coefficients(s, s_next, aug)
    whole_xt, whole_scaled = _prepare(xt, gt, noise, ind, co, aug)
    whole_next = _step(oc, ou, whole_xt, gt, ind, co, guidance)
    for lo, hi in ((0, 2), (2, 5)):
        cut = lambda t: t[:, :, lo:hi].contiguous()
        part_xt, part_scaled = _prepare(cut(xt), cut(gt), cut(noise), cut(ind), co, aug)
        part_next = _step(cut(oc), cut(ou), part_xt, cut(gt), cut(ind), co, guidance)
        for got, whole, what in ((part_xt, whole_xt, "new_xt"), (part_scaled, whole_scaled, "new_xt_scaled"), (part_next, whole_next, "xt_next")):
            assert torch.equal(got.view(torch.int16), cut(whole).view(torch.int16)), (what, lo, hi)


class _StubNet:
    """Stands in for the DiT: an elementwise bf16 function of x, the timestep and 16 pose channels, so every batch row is computed alike
    whether the conditional and the unconditional branch share a call or not."""
    is_context_parallel_enabled = False

    def __init__(self):
        self.calls = 0

    @staticmethod
    def fn(x, timesteps, pose):
        return (torch.tanh(x.float()) * (1 + 0.1 * timesteps.float()) + 0.05 * pose[:, :16].float()).to(bf16)

    def __call__(self, x, timesteps, condition_video_pose=None, **kw):
        self.calls += 1
        assert x.dtype == bf16 and timesteps.dtype == bf16 and timesteps.is_cuda
        return self.fn(x, timesteps, condition_video_pose)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "two_calls"])
@pytest.mark.parametrize("aug", AUGMENT_SIGMAS)
def test_denoise_step_loop_equals_the_reference_loop(aug, fuse):
    """All 35 steps through Gen3CDenoiser.denoise_step with a stub network: after every step xt equals the same loop through sampler_ref on the
    device. Pins the wiring around the kernels: the indicator zeroing, the noise cache, the cast of t, the out[:B] / out[B:] split."""
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
    dev = _dev()
    B, C, T, H, W, guidance, seed = 1, 16, 4, 6, 10, 1.7, 5
    g = torch.Generator().manual_seed(77)
    gt = (0.5 * torch.randn(B, C, T, H, W, generator=g)).to(bf16).to(dev)
    pose = (0.5 * torch.randn(B, 64, T, H, W, generator=g)).to(bf16).to(dev)
    ctx = torch.zeros(B, 4, 8, dtype=bf16, device=dev)
    net = _StubNet()
    den = Gen3CDenoiser(net, state_shape=(C, T, H, W))
    den.fuse_cond_uncond = fuse
    den.scheduler.set_timesteps(NUM_STEPS)
    sch = den.scheduler

    def cond(p):
        c = VideoExtendCondition(crossattn_emb=ctx, fps=torch.tensor([24.0], device=dev), video_cond_bool=True, condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 2)

    c, u = cond(pose), cond(torch.zeros_like(pose))
    ind = torch.tensor([1, 1, 0, 0], dtype=bf16, device=dev).reshape(1, 1, T, 1, 1)
    noise = torch.from_numpy(np.random.RandomState(seed).standard_normal((B, C, T, H, W)).astype(np.float32)).to(dev)  # utils/misc.py:133-154
    xt = (torch.randn(B, C, T, H, W, generator=g) * sch.init_noise_sigma).to(bf16).to(dev)
    ref = xt.clone()
    for i in range(NUM_STEPS):
        xt = den.denoise_step(xt, i, c, u, guidance, aug, seed)
        ref = sr.loop_iteration(lambda x, t: net.fn(x, t, pose), lambda x, t: net.fn(x, t, torch.zeros_like(pose)), ref, gt, noise, ind,
                                sch.sigmas[i], sch.sigmas[i + 1], sch.timesteps[i], guidance, aug)
        _assert_equal(xt, ref, f"xt after step {i}")
    assert net.calls == (NUM_STEPS if fuse else 2 * NUM_STEPS)  # the path asked for is the path that ran


def test_refusals_name_their_entry_and_launch_nothing():
    """sigma = 0, n = 0 and a null operand: a non-zero status whose message names the entry point, Gen3cHipError from the binding, and outputs that
    stay as they were."""
    from gen3c_amd import _lib as L, ops
    lib = L.load()
    dev, n = _dev(), 64
    s = torch.cuda.current_stream().cuda_stream
    a = torch.zeros(n, dtype=bf16, device=dev)
    nz = torch.zeros(n, dtype=f32, device=dev)
    ind = torch.ones(1, dtype=f32, device=dev)
    o1, o2 = (torch.full((n,), float("nan"), dtype=bf16, device=dev) for _ in range(2))
    p = lambda t: t.data_ptr()
    prep, step = "g3_edm_prepare_input_bf16", "g3_edm_cfg_euler_step_bf16"
    calls = [
        (step, lambda: lib.g3_edm_cfg_euler_step_bf16(p(a), p(a), p(a), p(a), p(ind), p(o1), n, 1, n, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, s)),   # sigma = 0
        (step, lambda: lib.g3_edm_cfg_euler_step_bf16(p(a), p(a), p(a), p(a), p(ind), p(o1), 0, 1, n, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, s)),   # n = 0
        (step, lambda: lib.g3_edm_cfg_euler_step_bf16(p(a), None, p(a), p(a), p(ind), p(o1), n, 1, n, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, s)),   # null out_uncond
        (step, lambda: lib.g3_edm_cfg_euler_step_bf16(p(a), p(a), p(a), p(a), p(ind), None, n, 1, n, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, s)),    # null output
        (prep, lambda: lib.g3_edm_prepare_input_bf16(p(a), p(a), p(nz), p(ind), p(o1), p(o2), 0, 1, n, 0.001, 1.0, 1.0, 1.0, s)),               # n = 0
        (prep, lambda: lib.g3_edm_prepare_input_bf16(p(a), p(a), None, p(ind), p(o1), p(o2), n, 1, n, 0.001, 1.0, 1.0, 1.0, s)),                # null noise
        (prep, lambda: lib.g3_edm_prepare_input_bf16(p(a), p(a), p(nz), p(ind), p(o1), None, n, 1, n, 0.001, 1.0, 1.0, 1.0, s)),                # null output
    ]
    for entry, call in calls:
        rc = call()
        assert rc != 0, entry
        assert entry in L.last_error(), (entry, L.last_error())
        with pytest.raises(L.Gen3cHipError, match=entry):
            L.check(rc, entry)
    with pytest.raises(L.Gen3cHipError, match=step):  # the same refusal through the front end the sampler uses
        ops.edm_cfg_euler_step(a, a, a, a, ind, 1, n, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o1.float()).all()) and bool(torch.isnan(o2.float()).all()), "a refused call wrote output"
