"""GPU: the opt-in second-order multistep sampler solver "2ab" - edm_step_2ab_kernel through gen3c_amd.ops.edm_cfg_2ab_step, and the loop of
Gen3CDenoiser.generate_samples_from_batch(solver="2ab") - against tests/sampler_2ab_ref.py run on the device (tests/sampler_ref.py's dtype chain plus
the 2ab update). The update is three fp32 multiplies and two fp32 adds, each one IEEE operation with no contraction, in the kernel and in torch
alike, so every comparison with the restatement is equality, not a tolerance. Inputs are built as tests/test_sampler_kernels_gpu.py builds them."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import sampler_2ab_ref as r2
from tests import sampler_ref as sr
from tests.test_sampler_kernels_gpu import _StubNet, _assert_equal, _kernel_indicator, _ulps

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

bf16, f32 = torch.bfloat16, torch.float32
NUM_STEPS, AUG = 35, 0.001
SHAPES = [(1, 16, 3, 4, 6),      # n = 1 152
          (2, 16, 4, 5, 7),      # n = 4 480: batch 2, odd hw, a ragged tail for any vector width
          (1, 16, 5, 88, 80)]    # n = 563 200 > 2048 * 256: the grid-stride loop turns over
CONDITION_FRAMES = [0, 1, 2]     # indicator: all zero, the first frame set, the first two frames set
GUIDANCES = [1.0, 1.5]
STEPS = [0, 1, 17, NUM_STEPS - 2]
shape_ids = lambda s: "x".join(map(str, s))


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _denoiser():
    from types import SimpleNamespace
    from gen3c_amd.sampler import Gen3CDenoiser
    den = Gen3CDenoiser(SimpleNamespace(is_context_parallel_enabled=False))
    den.scheduler.set_timesteps(NUM_STEPS)
    return den


@functools.lru_cache(maxsize=None)
def _inputs(shape, step):
    """tests/test_sampler_kernels_gpu.py::_inputs (xt ~ N(0, sigma^2 + 1) with +-0 and +-3 sigma_max planted, gt ~ N(0, 0.25) with a zero first frame,
    out_uncond equal to out_cond on the last frame, fp32 noise) plus a previous x0 prediction at the data's scale, N(0, 0.25) in fp32, with +-0 planted."""
    B, C, T, H, W = shape
    n = B * C * T * H * W
    g = torch.Generator().manual_seed(2000 * n + step)
    sigma = float(_denoiser().scheduler.sigmas[step])
    xt = (torch.randn(shape, generator=g) * (sigma ** 2 + 1) ** 0.5).to(bf16)
    flat = xt.view(-1)
    flat[[1, n // 3]] = 0.0
    flat[[2, n // 3 + 1]] = -0.0
    flat[[3, n // 2]] = 240.0
    flat[[4, n - 1]] = -240.0
    gt = (0.5 * torch.randn(shape, generator=g)).to(bf16)
    gt[:, :, 0] = 0
    oc = torch.randn(shape, generator=g).to(bf16)
    ou = torch.randn(shape, generator=g).to(bf16)
    ou[:, :, T - 1] = oc[:, :, T - 1]
    noise = torch.randn(shape, generator=g)
    x0_prev = 0.5 * torch.randn(shape, generator=g)
    x0_prev.view(-1)[[5, n - 2]] = 0.0
    x0_prev.view(-1)[[6, n - 3]] = -0.0
    return tuple(t.to(_dev()) for t in (xt, gt, oc, ou, noise, x0_prev))


def _indicator(T, frames):
    return torch.tensor([1.0] * frames + [0.0] * (T - frames), dtype=bf16, device=_dev()).reshape(1, 1, T, 1, 1)


def _coefficients_2ab(step):
    """(a, cb1, cb2) of the step. Step 0 has no previous sigma in the loop (it never runs with a history); the kernel takes any coefficients, so for
    the kernel-level cases it gets those of a made-up previous sigma of twice its own."""
    from gen3c_amd.sampler import res_2ab_coefficients
    sig = _denoiser().scheduler.sigmas
    return res_2ab_coefficients(float(sig[step]), float(sig[step + 1]), float(sig[step - 1]) if step else 2 * float(sig[0]))


class _Case:
    def __init__(self, shape, step, frames, guidance, cut=None):
        cut = cut or (lambda t: t)
        den = _denoiser()
        self.s, self.s_next = den.scheduler.sigmas[step], den.scheduler.sigmas[step + 1]
        self.co = den._coefficients(self.s, self.s_next, AUG)
        xt, gt, oc, ou, noise, x0_prev = _inputs(shape, step)
        ind = _indicator(shape[2], frames)
        new_xt, _ = sr.prepare(xt, gt, noise, ind, self.s, AUG)  # the reference's own network input: these tests judge the step kernel alone
        self.gt, self.oc, self.ou, self.new_xt, self.x0_prev, self.ind = (cut(t).contiguous() for t in (gt, oc, ou, new_xt, x0_prev, ind))
        self.ind_eff = sr.effective_indicator(self.ind, self.s, AUG)
        self.guidance, self.coef = guidance, _coefficients_2ab(step)

    def kernel(self, have_prev, in_place=False):
        """-> (xt_next, x0_out) of ops.edm_cfg_2ab_step; in_place: the history buffer is also the output (the form the loop uses)."""
        from gen3c_amd import ops
        co, x = self.co, self.new_xt
        hist = self.x0_prev.clone()
        out = hist if in_place else torch.full_like(hist, float("nan"))
        a, cb1, cb2 = self.coef if have_prev else (0.0, 0.0, 0.0)
        nxt = ops.edm_cfg_2ab_step(self.oc, self.ou, x, self.gt, _kernel_indicator(self.ind, co), x.shape[2], x.shape[3] * x.shape[4], self.guidance,
                                   co["c_skip_bf16"], co["c_out_bf16"], co["c_skip"], co["c_out"], co["sigma"], co["inv_sigma"], co["sigma_next"],
                                   hist, have_prev, a, cb1, cb2, x0_out=None if in_place else out)
        if not in_place:
            assert torch.equal(hist.view(torch.int32), self.x0_prev.view(torch.int32)), "x0_prev was written although x0_out is another buffer"
        return nxt, out

    def euler(self):
        from gen3c_amd import ops
        co, x = self.co, self.new_xt
        return ops.edm_cfg_euler_step(self.oc, self.ou, x, self.gt, _kernel_indicator(self.ind, co), x.shape[2], x.shape[3] * x.shape[4], self.guidance,
                                      co["c_skip_bf16"], co["c_out_bf16"], co["c_skip"], co["c_out"], co["sigma"], co["inv_sigma"], co["sigma_next"])

    def reference(self, have_prev):
        return r2.step_2ab(self.oc, self.ou, self.new_xt, self.gt, self.ind_eff, self.s, self.s_next, self.guidance,
                           self.x0_prev if have_prev else None, self.coef)


def _cases(shape, step):
    for frames in CONDITION_FRAMES:
        for guidance in GUIDANCES:
            yield f"condition frames {frames}, guidance {guidance}", _Case(shape, step, frames, guidance)


def _same_bits(a, b):
    view = torch.int16 if a.dtype == bf16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _assert_x0_equal(got, ref, what):
    assert got.dtype == ref.dtype == f32 and got.shape == ref.shape
    if not torch.equal(got, ref):  # value equality, as for xt: the sign of a zero is not pinned
        bad = (got != ref).reshape(-1).nonzero().reshape(-1)
        first = [(int(i), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i])) for i in bad[:5]]
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ; (index, got, ref): {first}")


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_without_history_xt_is_the_euler_kernels_and_x0_is_stored(shape, step):
    for what, c in _cases(shape, step):
        nxt, x0 = c.kernel(have_prev=False)
        assert _same_bits(nxt, c.euler()), f"{what}: xt_next is not the Euler entry's"
        _assert_x0_equal(x0, r2.x0_prediction(c.oc, c.ou, c.new_xt, c.gt, c.ind_eff, c.s, c.guidance)[1], f"{what}: x0_out")


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_with_history_equals_the_fp32_restatement_and_is_within_one_ulp_of_fp64(shape, step):
    differ = total = 0
    for what, c in _cases(shape, step):
        nxt, x0 = c.kernel(have_prev=True)
        ref_next, ref_x0 = c.reference(have_prev=True)
        _assert_equal(nxt, ref_next, f"{what}: xt_next")
        _assert_x0_equal(x0, ref_x0, f"{what}: x0_out")
        exact = r2.step_2ab_fp64(c.new_xt.float(), ref_x0, c.x0_prev, c.coef)
        d = _ulps(nxt, exact)
        differ, total = differ + int((d != 0).sum()), total + d.numel()
        print(f"{shape_ids(shape)} step {step}, {what}: {int((d != 0).sum())} of {d.numel()} elements differ from the fp64 evaluation, max {int(d.max())} bf16 ulp")
        assert int(d.max()) <= 1, f"{what}: {int((d > 1).sum())} elements more than 1 bf16 ulp from the fp64 evaluation (max {int(d.max())})"
    print(f"{shape_ids(shape)} step {step}: share of elements that differ from the fp64 evaluation {differ / total:.2e}")


@pytest.mark.parametrize("have_prev", [False, True], ids=["no_history", "history"])
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_history_updated_in_place_gives_the_same_bits(shape, step, have_prev):
    for what, c in _cases(shape, step):
        nxt, x0 = c.kernel(have_prev)
        nxt_ip, x0_ip = c.kernel(have_prev, in_place=True)
        assert _same_bits(nxt, nxt_ip) and _same_bits(x0, x0_ip), what


@pytest.mark.parametrize("have_prev", [False, True], ids=["no_history", "history"])
@pytest.mark.parametrize("step", [1, 17, NUM_STEPS - 2])
def test_rank_local_frame_slices_equal_the_whole_tensor(step, have_prev):
    """What a context-parallel rank computes: the kernel on the frame slices [0:1] and [1:4] of every operand (the history is the rank's own shard)
    gives the matching slices of the whole-tensor result bit for bit."""
    shape, frames, guidance = (2, 16, 4, 5, 7), 2, 1.5
    whole_next, whole_x0 = _Case(shape, step, frames, guidance).kernel(have_prev)
    for lo, hi in ((0, 1), (1, 4)):
        cut = lambda t: t[:, :, lo:hi]
        part_next, part_x0 = _Case(shape, step, frames, guidance, cut=cut).kernel(have_prev)
        assert _same_bits(part_next, cut(whole_next)) and _same_bits(part_x0, cut(whole_x0)), (lo, hi)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
class _Loop:
    """Gen3CDenoiser around the stub network of the existing loop test, and the same loop through the restatements."""
    B, C, T, H, W, guidance, seed = 1, 16, 4, 6, 10, 1.5, 5

    def __init__(self, fuse):
        from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
        dev, shape = _dev(), (self.B, self.C, self.T, self.H, self.W)
        g = torch.Generator().manual_seed(78)
        self.gt = (0.5 * torch.randn(shape, generator=g)).to(bf16).to(dev)
        self.pose = (0.5 * torch.randn(self.B, 64, self.T, self.H, self.W, generator=g)).to(bf16).to(dev)
        ctx = torch.zeros(self.B, 4, 8, dtype=bf16, device=dev)
        self.net = _StubNet()
        self.den = Gen3CDenoiser(self.net, state_shape=shape[1:])
        self.den.fuse_cond_uncond = fuse

        def cond(p):
            c = VideoExtendCondition(crossattn_emb=ctx, fps=torch.tensor([24.0], device=dev), video_cond_bool=True, condition_video_pose=p)
            return add_condition_video_indicator_and_video_input_mask(self.gt, c, 2)

        self.c, self.u = cond(self.pose), cond(torch.zeros_like(self.pose))
        self.ind = torch.tensor([1, 1, 0, 0], dtype=bf16, device=dev).reshape(1, 1, self.T, 1, 1)
        self.noise = torch.from_numpy(np.random.RandomState(self.seed).standard_normal(shape).astype(np.float32)).to(dev)
        self.xt = (torch.randn(shape, generator=g) * self.den.scheduler.init_noise_sigma).to(bf16).to(dev)

    def run(self, num_steps, **kw):
        return self.den.generate_samples_from_batch(self.c, self.u, guidance=self.guidance, seed=self.seed, num_steps=num_steps,
                                                    condition_augment_sigma=AUG, xt=self.xt.clone(), **kw)

    def reference(self, num_steps, solver):
        """model_v2w.py:130-149 per step (sampler_ref.loop_iteration's pieces); under "2ab" the update of every step that has a previous x0 and does
        not end at sigma 0 is sampler_2ab_ref.step_2ab, and every step but the last keeps its x0."""
        from gen3c_amd.sampler import EDMEulerScheduler, res_2ab_coefficients
        sch = EDMEulerScheduler()
        sch.set_timesteps(num_steps)
        zero_pose = torch.zeros_like(self.pose)
        xt, x0_prev = self.xt.clone(), None
        for i in range(num_steps):
            s, s_next = sch.sigmas[i], sch.sigmas[i + 1]
            new_xt, scaled = sr.prepare(xt, self.gt, self.noise, self.ind, s, AUG)
            t = sch.timesteps[i].to(device=xt.device, dtype=bf16)
            oc, ou = self.net.fn(scaled, t, self.pose), self.net.fn(scaled, t, zero_pose)
            eff = sr.effective_indicator(self.ind, s, AUG)
            if solver == "euler" or float(s_next) == 0.0:
                xt = sr.step(oc, ou, new_xt, self.gt, eff, s, s_next, self.guidance)
            else:
                coef = res_2ab_coefficients(float(s), float(s_next), float(sch.sigmas[i - 1])) if x0_prev is not None else None
                xt, x0_prev = r2.step_2ab(oc, ou, new_xt, self.gt, eff, s, s_next, self.guidance, x0_prev, coef)
        return xt


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "two_calls"])
def test_2ab_loop_equals_the_restated_loop(fuse):
    loop = _Loop(fuse)
    got = loop.run(6, solver="2ab")
    assert loop.net.calls == (6 if fuse else 12)
    _assert_equal(got, loop.reference(6, "2ab"), "xt after the 6-step 2ab loop")
    assert not torch.equal(got, loop.reference(6, "euler")), "the 2ab loop gave the Euler loop's result: the second-order steps did not run"
    _assert_equal(loop.run(6, solver="2ab"), got, "a second call (a history left over from the first would change it)")
    loop.den.solver = "2ab"  # the denoiser's setting instead of the argument
    _assert_equal(loop.run(6), got, "xt with Gen3CDenoiser.solver = '2ab'")


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "two_calls"])
def test_2ab_loop_of_two_steps_is_the_euler_loop(fuse):
    loop = _Loop(fuse)
    euler = loop.run(2)
    _assert_equal(euler, loop.reference(2, "euler"), "xt after the 2-step Euler loop")
    for n in (1, 2):
        assert _same_bits(loop.run(n, solver="2ab"), loop.run(n)), n


def test_euler_by_name_is_the_default_loop_and_never_reaches_the_2ab_entry(monkeypatch):
    from gen3c_amd import ops
    loop = _Loop(True)

    def refuse(*a, **k):
        raise AssertionError("ops.edm_cfg_2ab_step was called under solver 'euler'")

    monkeypatch.setattr(ops, "edm_cfg_2ab_step", refuse)
    default = loop.run(6)
    assert _same_bits(loop.run(6, solver="euler"), default)
    _assert_equal(default, loop.reference(6, "euler"), "xt after the 6-step Euler loop")
    with pytest.raises(AssertionError, match="edm_cfg_2ab_step was called"):
        loop.run(6, solver="2ab")  # the patch is in the loop's way: the 2ab loop does go through this front end


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_and_launch_nothing():
    from gen3c_amd import _lib as L, ops
    lib = L.load()
    dev, n = _dev(), 64
    s = torch.cuda.current_stream().cuda_stream
    a = torch.zeros(n, dtype=bf16, device=dev)
    ind = torch.ones(1, dtype=f32, device=dev)
    prev = torch.zeros(n, dtype=f32, device=dev)
    o = torch.full((n,), float("nan"), dtype=bf16, device=dev)
    h = torch.full((n,), float("nan"), dtype=f32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    entry = "g3_edm_cfg_2ab_step_bf16"

    def call(oc=a, ou=a, out=o, n_=n, sigma=1.0, x0_prev=prev, x0_out=h, have_prev=1, coef_a=0.5):
        return lib.g3_edm_cfg_2ab_step_bf16(p(oc), p(ou), p(a), p(a), p(ind), p(out), n_, 1, n, 1.0, 1.0, 1.0, 1.0, 1.0, sigma, 1.0, 0.5,
                                            p(x0_prev), p(x0_out), have_prev, coef_a, 0.3, 0.2, s)

    refused = dict(sigma_zero=dict(sigma=0.0), sigma_negative=dict(sigma=-1.0), n_zero=dict(n_=0), null_out_uncond=dict(ou=None),
                   null_xt_next=dict(out=None), null_x0_out=dict(x0_out=None), null_x0_out_without_history=dict(x0_out=None, have_prev=0),
                   history_without_x0_prev=dict(x0_prev=None), a_zero=dict(coef_a=0.0), a_negative=dict(coef_a=-0.5),
                   a_nan=dict(coef_a=float("nan")), a_inf=dict(coef_a=float("inf")))
    for what, kw in refused.items():
        rc = call(**kw)
        assert rc != 0, what
        assert entry in L.last_error(), (what, L.last_error())
        with pytest.raises(L.Gen3cHipError, match=entry):
            L.check(rc, entry)
    with pytest.raises(L.Gen3cHipError, match=entry):  # the same refusal through the front end the sampler uses
        ops.edm_cfg_2ab_step(a, a, a, a, ind, 1, n, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, h, True, 0.5, 0.3, 0.2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o.float()).all()) and bool(torch.isnan(h).all()), "a refused call wrote output"
    assert call(x0_prev=None, have_prev=0, coef_a=0.0) == 0  # without history neither x0_prev nor `a` is looked at
    torch.cuda.synchronize()
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(h).any())


# ---- the command line --------------------------------------------------------------------------------------------------------------------------
def test_single_image_cli_runs_the_2ab_loop(tmp_path, capsys, monkeypatch):
    """--sampler_solver 2ab end to end through the single-image entry point (tiny random-weight models, 9-frame chunk, 4 steps): the flag reaches the
    denoiser's loop - the 2ab front end is called for steps 0..2 and not for the step to sigma 0 - and the session says that the mode is outside parity."""
    from PIL import Image
    from gen3c_amd import gen3c_single_image as cli, ops
    H, W = 64, 96
    ys, xs = np.mgrid[0:H, 0:W]
    Image.fromarray(np.stack([(xs * 2) % 256, (ys * 3) % 256, ((xs + ys) * 2) % 256], -1).astype(np.uint8)).save(tmp_path / "in.png")
    np.savez(tmp_path / "depth.npz", depth=(2.0 + 0.01 * xs).astype(np.float32), intrinsics=np.array([[80, 0, W / 2], [0, 80, H / 2], [0, 0, 1]], np.float32))
    have_prev = []
    real = ops.edm_cfg_2ab_step
    monkeypatch.setattr(ops, "edm_cfg_2ab_step", lambda *a, **k: have_prev.append(bool(a[16])) or real(*a, **k))
    args = cli.create_parser().parse_args([
        "--input_image_path", str(tmp_path / "in.png"), "--depth_path", str(tmp_path / "depth.npz"), "--height", str(H), "--width", str(W),
        "--num_steps", "4", "--random_init", "--tiny", "--video_save_folder", str(tmp_path / "out"), "--video_save_name", "v",
        "--trajectory", "clockwise", "--sampler_solver", "2ab"])
    video = cli.demo(args)
    assert video.shape == (9, H, W, 3) and video.dtype == np.uint8
    assert have_prev == [False, True, True]
    assert "--sampler_solver 2ab" in capsys.readouterr().out


# ---- CFG-parallel ------------------------------------------------------------------------------------------------------------------------------
def test_cfg_parallel_pair_equals_the_single_process_2ab_loop(tmp_path):
    """2 processes on cuda:0 over gloo (tests/_sampler_2ab_cfg_worker.py): each rank's CFG-parallel 2ab loop ends bit-identical to its own
    single-process 2ab loop, and the two ranks agree."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    worker = str(ROOT / "tests" / "_sampler_2ab_cfg_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(rank), port, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              cwd=str(ROOT), env=dict(os.environ)) for rank in (0, 1)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=150)[0])  # each process under its own limit; the collectives inside give up after 60 s
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    for rank, pr in enumerate(procs):
        assert pr.returncode == 0, f"rank {rank}:\n{outs[rank][-3000:]}"
        assert (tmp_path / f"ok{rank}").exists()
