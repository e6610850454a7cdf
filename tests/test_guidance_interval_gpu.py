"""GPU: the opt-in guidance interval - classifier-free guidance only while lo < sigma <= hi, one network call per step outside it.
  * the two step kernels without an unconditional operand (gen3c_amd.ops.edm_cond_euler_step / edm_cond_2ab_step) against tests/sampler_ref.py and
    tests/sampler_2ab_ref.py run on the device with out_uncond := out_cond and guidance 0.0 (net_output = out_cond + 0.0 * 0 = out_cond), and
    against the existing CFG kernels at guidance 0;
  * the loop of Gen3CDenoiser.generate_samples_from_batch(guidance_interval=...) against a loop restated here from the same pieces, with the "2ab"
    reset rule (a step whose guidedness differs from the previous step's takes the Euler update), and the default against today's loop;
  * a real (tiny) DiT, the refusals, the command line and a CFG-parallel pair.
Every comparison is equality - by value against the restatements (the sign of a zero is not pinned, as in tests/test_sampler_kernels_gpu.py), by bits
where two kernel paths are compared. Inputs are built as tests/test_sampler_2ab_gpu.py builds them (its builders are imported)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import sampler_2ab_ref as r2
from tests import sampler_ref as sr
from tests.test_sampler_2ab_gpu import _Loop, _assert_x0_equal, _coefficients_2ab, _denoiser, _indicator, _inputs, _same_bits
from tests.test_sampler_kernels_gpu import _assert_equal, _kernel_indicator

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

bf16, f32 = torch.bfloat16, torch.float32
NUM_STEPS, AUG = 35, 0.001
SHAPES = [(1, 16, 3, 4, 6), (2, 16, 4, 5, 7), (1, 16, 5, 88, 80)]  # the last: 563 200 elements > 2048 * 256, the grid-stride loop turns over
CONDITION_FRAMES = [0, 1, 2]
STEPS = [0, 1, 17, NUM_STEPS - 2]
shape_ids = lambda s: "x".join(map(str, s))


def _dev():
    return torch.device("cuda:0")


class _Case:
    def __init__(self, shape, step, frames, cut=None):
        cut = cut or (lambda t: t)
        den = _denoiser()
        self.s, self.s_next = den.scheduler.sigmas[step], den.scheduler.sigmas[step + 1]
        self.co = den._coefficients(self.s, self.s_next, AUG)
        xt, gt, oc, ou, noise, x0_prev = _inputs(shape, step)
        ind = _indicator(shape[2], frames)
        new_xt, _ = sr.prepare(xt, gt, noise, ind, self.s, AUG)
        self.gt, self.oc, self.ou, self.new_xt, self.x0_prev, self.ind = (cut(t).contiguous() for t in (gt, oc, ou, new_xt, x0_prev, ind))
        self.ind_eff = sr.effective_indicator(self.ind, self.s, AUG)
        self.coef = _coefficients_2ab(step)

    def _common(self):
        co, x = self.co, self.new_xt
        return (x, self.gt, _kernel_indicator(self.ind, co), x.shape[2], x.shape[3] * x.shape[4]), \
               (co["c_skip_bf16"], co["c_out_bf16"], co["c_skip"], co["c_out"], co["sigma"], co["inv_sigma"], co["sigma_next"])

    def cond_euler(self):
        from gen3c_amd import ops
        head, scalars = self._common()
        return ops.edm_cond_euler_step(self.oc, *head, *scalars)

    def cfg_euler_guidance_0(self):
        """the existing CFG entry at guidance 0.0 with an unrelated finite out_uncond"""
        from gen3c_amd import ops
        head, scalars = self._common()
        return ops.edm_cfg_euler_step(self.oc, self.ou, *head, 0.0, *scalars)

    def cond_2ab(self, have_prev, in_place=False):
        """-> (xt_next, x0_out) of ops.edm_cond_2ab_step; in_place: the history buffer is also the output (the form the loop uses)."""
        from gen3c_amd import ops
        head, scalars = self._common()
        hist = self.x0_prev.clone()
        out = hist if in_place else torch.full_like(hist, float("nan"))
        a, cb1, cb2 = self.coef if have_prev else (0.0, 0.0, 0.0)
        nxt = ops.edm_cond_2ab_step(self.oc, *head, *scalars, hist, have_prev, a, cb1, cb2, x0_out=None if in_place else out)
        if not in_place:
            assert torch.equal(hist.view(torch.int32), self.x0_prev.view(torch.int32)), "x0_prev was written although x0_out is another buffer"
        return nxt, out


def _cases(shape, step):
    for frames in CONDITION_FRAMES:
        yield f"condition frames {frames}", _Case(shape, step, frames)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_cond_euler_entry_equals_the_restatement_and_the_cfg_entry_at_guidance_0(shape, step):
    for what, c in _cases(shape, step):
        got = c.cond_euler()
        _assert_equal(got, sr.step(c.oc, c.oc, c.new_xt, c.gt, c.ind_eff, c.s, c.s_next, 0.0), f"{what}: xt_next")
        cfg = c.cfg_euler_guidance_0()
        _assert_equal(got, cfg, f"{what}: xt_next against the CFG entry at guidance 0")
        both = (got != 0) & (cfg != 0)
        assert bool(both.any()) and torch.equal(got.view(torch.int16)[both], cfg.view(torch.int16)[both]), f"{what}: bits differ from the CFG entry's"


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_cond_2ab_entry_without_history_is_the_cond_euler_entry_and_stores_x0(shape, step):
    for what, c in _cases(shape, step):
        nxt, x0 = c.cond_2ab(have_prev=False)
        assert _same_bits(nxt, c.cond_euler()), f"{what}: xt_next is not the cond Euler entry's"
        _assert_x0_equal(x0, r2.x0_prediction(c.oc, c.oc, c.new_xt, c.gt, c.ind_eff, c.s, 0.0)[1], f"{what}: x0_out")


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_cond_2ab_entry_with_history_equals_the_restatement_also_in_place(shape, step):
    for what, c in _cases(shape, step):
        nxt, x0 = c.cond_2ab(have_prev=True)
        ref_next, ref_x0 = r2.step_2ab(c.oc, c.oc, c.new_xt, c.gt, c.ind_eff, c.s, c.s_next, 0.0, c.x0_prev, c.coef)
        _assert_equal(nxt, ref_next, f"{what}: xt_next")
        _assert_x0_equal(x0, ref_x0, f"{what}: x0_out")
        for have_prev, (n_, x_) in ((True, (nxt, x0)), (False, c.cond_2ab(False))):
            nxt_ip, x0_ip = c.cond_2ab(have_prev, in_place=True)
            assert _same_bits(n_, nxt_ip) and _same_bits(x_, x0_ip), f"{what}: in-place history, have_prev {have_prev}"


@pytest.mark.parametrize("step", [1, 17, NUM_STEPS - 2])
def test_rank_local_frame_slices_equal_the_whole_tensor(step):
    """What a context-parallel rank computes: both cond entries on the frame slices [0:1] and [1:4] of every operand give the matching slices of
    the whole-tensor result bit for bit."""
    shape, frames = (2, 16, 4, 5, 7), 2
    whole = _Case(shape, step, frames)
    whole_euler, whole_2ab = whole.cond_euler(), {hp: whole.cond_2ab(hp) for hp in (False, True)}
    for lo, hi in ((0, 1), (1, 4)):
        cut = lambda t: t[:, :, lo:hi]
        part = _Case(shape, step, frames, cut=cut)
        assert _same_bits(part.cond_euler(), cut(whole_euler)), (lo, hi)
        for hp in (False, True):
            nxt, x0 = part.cond_2ab(hp)
            assert _same_bits(nxt, cut(whole_2ab[hp][0])) and _same_bits(x0, cut(whole_2ab[hp][1])), (lo, hi, hp)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
INTERVAL = (0.1, 10.0)  # of the 6-step schedule (sigmas 80, 22.02, 4.52, 0.583, 0.0318, 2e-4) steps 2 and 3 are guided


class _IntervalLoop(_Loop):
    def reference(self, num_steps, solver, interval):
        """The loop restated from sampler_ref / sampler_2ab_ref pieces. A guided step is model_v2w.py:130-149; an unguided one makes the conditional
        call alone and its net_output is that call's output (out_uncond := out_cond, guidance 0.0 in the restatements). Under "2ab" every step but
        the last stores its x0, and a step uses the stored one only if it came from a step of the same guidedness."""
        from gen3c_amd.sampler import EDMEulerScheduler, res_2ab_coefficients
        sch = EDMEulerScheduler()
        sch.set_timesteps(num_steps)
        zero_pose = torch.zeros_like(self.pose)
        xt, x0_prev, prev_guided = self.xt.clone(), None, None
        for i in range(num_steps):
            s, s_next = sch.sigmas[i], sch.sigmas[i + 1]
            guided = interval is None or interval[0] < float(s) <= interval[1]
            new_xt, scaled = sr.prepare(xt, self.gt, self.noise, self.ind, s, AUG)
            t = sch.timesteps[i].to(device=xt.device, dtype=bf16)
            oc = self.net.fn(scaled, t, self.pose)
            ou, g = (self.net.fn(scaled, t, zero_pose), self.guidance) if guided else (oc, 0.0)
            eff = sr.effective_indicator(self.ind, s, AUG)
            if solver == "euler" or float(s_next) == 0.0:
                xt = sr.step(oc, ou, new_xt, self.gt, eff, s, s_next, g)
            else:
                use = x0_prev is not None and prev_guided == guided
                coef = res_2ab_coefficients(float(s), float(s_next), float(sch.sigmas[i - 1])) if use else None
                xt, x0_prev = r2.step_2ab(oc, ou, new_xt, self.gt, eff, s, s_next, g, x0_prev if use else None, coef)
                prev_guided = guided
        return xt


def _record_front_ends(monkeypatch):
    """-> the list every sampler step front end appends (name, have_prev or None) to, the real front ends still running."""
    from gen3c_amd import ops
    seen = []
    for name, hp in (("edm_cfg_euler_step", None), ("edm_cond_euler_step", None), ("edm_cfg_2ab_step", 16), ("edm_cond_2ab_step", 14)):
        def wrap(*a, _real=getattr(ops, name), _name=name, _hp=hp, **k):
            seen.append((_name, None if _hp is None else bool(a[_hp])))
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, wrap)
    return seen


def test_schedule_of_the_loop_tests():
    from gen3c_amd.sampler import EDMEulerScheduler, guided_steps
    sch = EDMEulerScheduler()
    sch.set_timesteps(6)
    assert guided_steps(sch.sigmas, INTERVAL) == [False, False, True, True, False, False]
    assert guided_steps(sch.sigmas, None) == [True] * 6


@pytest.mark.parametrize("solver", ["euler", "2ab"])
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "two_calls"])
def test_interval_loop_equals_the_restated_loop(fuse, solver):
    loop = _IntervalLoop(fuse)
    got = loop.run(6, solver=solver, guidance_interval=INTERVAL)
    assert loop.net.calls == (6 if fuse else 8)  # 4 unguided steps of one call, 2 guided steps of one fused call or two
    _assert_equal(got, loop.reference(6, solver, INTERVAL), f"xt after the 6-step {solver} loop with guidance in {INTERVAL}")
    assert not torch.equal(got, loop.reference(6, solver, None)), "the interval loop gave the always-guided loop's result"
    _assert_equal(loop.run(6, solver=solver, guidance_interval=INTERVAL), got, "a second call")
    loop.den.guidance_interval = INTERVAL  # the denoiser's setting instead of the argument
    _assert_equal(loop.run(6, solver=solver), got, "xt with Gen3CDenoiser.guidance_interval set")


def test_2ab_takes_the_euler_update_where_guidedness_changes(monkeypatch):
    loop = _IntervalLoop(True)
    seen = _record_front_ends(monkeypatch)
    loop.run(6, solver="2ab", guidance_interval=INTERVAL)
    # steps 0, 2, 4 (no history / the history is the other denoiser's) and 5 (to sigma 0) take the Euler update, steps 1 and 3 the second-order one
    assert seen == [("edm_cond_2ab_step", False), ("edm_cond_2ab_step", True), ("edm_cfg_2ab_step", False), ("edm_cfg_2ab_step", True),
                    ("edm_cond_2ab_step", False), ("edm_cond_euler_step", None)]
    seen.clear()
    loop.run(6, solver="euler", guidance_interval=INTERVAL)
    assert [n for n, _ in seen] == ["edm_cond_euler_step"] * 2 + ["edm_cfg_euler_step"] * 2 + ["edm_cond_euler_step"] * 2


def test_interval_is_open_below_and_closed_above(monkeypatch):
    loop = _IntervalLoop(True)
    loop.den.scheduler.set_timesteps(6)
    sig = loop.den.scheduler.sigmas
    seen = _record_front_ends(monkeypatch)
    loop.run(6, guidance_interval=(float(sig[3]), float(sig[2])))  # hi = sigma of step 2: guided; lo = sigma of step 3: not guided
    assert [n for n, _ in seen] == ["edm_cond_euler_step"] * 2 + ["edm_cfg_euler_step"] + ["edm_cond_euler_step"] * 3


@pytest.mark.parametrize("solver", ["euler", "2ab"])
def test_without_an_interval_the_loop_is_todays_and_never_reaches_the_cond_front_ends(monkeypatch, solver):
    from gen3c_amd import ops
    from gen3c_amd.sampler import Res2abState
    loop = _IntervalLoop(True)

    def refuse(*a, **k):
        raise AssertionError("a cond front end was called without a guidance interval")

    monkeypatch.setattr(ops, "edm_cond_euler_step", refuse)
    monkeypatch.setattr(ops, "edm_cond_2ab_step", refuse)
    assert loop.den.guidance_interval is None
    by_attribute = loop.run(6, solver=solver)
    assert _same_bits(loop.run(6, solver=solver, guidance_interval=None), by_attribute)
    # today's loop: denoise_step called as before this mode existed (positionally, `solver_state` only under "2ab")
    den = loop.den
    den.scheduler.set_timesteps(6)
    xt, state = loop.xt.clone(), Res2abState()
    for i in range(6):
        kw = dict(solver_state=state) if solver == "2ab" else {}
        xt = den.denoise_step(xt, i, loop.c, loop.u, loop.guidance, AUG, loop.seed, **kw)
    assert _same_bits(by_attribute, xt)
    _assert_equal(by_attribute, _Loop.reference(loop, 6, solver), "xt after the 6-step loop")
    with pytest.raises(AssertionError, match="cond front end was called"):
        loop.run(6, solver=solver, guidance_interval=INTERVAL)  # the patch is in the interval loop's way


# ---- a real network --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["euler", "2ab"])
def test_never_guided_loop_through_a_real_dit_equals_the_cfg_loop_with_the_condition_as_uncondition(solver):
    """A tiny 2-block DiT, two-call form, 4 steps: the loop that is never guided (interval (1e9, inf)) against the existing loop called with
    uncondition := condition, where cond - uncond = 0 and net_output = out_cond by value. Pins the cond-only call and kernels against the
    existing CFG path through a real network."""
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
    from tests._mxfp8_tiny_dit import _inputs as dit_inputs, _net
    dev = _dev()
    net = _net(dev)
    inp = {k: v.to(dev) for k, v in dit_inputs().items()}
    gt = (0.5 * inp["x"]).contiguous()
    den = Gen3CDenoiser(net, state_shape=tuple(gt.shape[1:]))
    den.fuse_cond_uncond = False
    cond = VideoExtendCondition(crossattn_emb=inp["crossattn_emb"], fps=inp["fps"], padding_mask=inp["padding_mask"], video_cond_bool=True,
                                condition_video_pose=inp["condition_video_pose"])
    cond = add_condition_video_indicator_and_video_input_mask(gt, cond, 1)
    g = torch.Generator().manual_seed(11)
    xt = (torch.randn(gt.shape, generator=g) * den.scheduler.init_noise_sigma).to(bf16).to(dev)
    run = lambda **kw: den.generate_samples_from_batch(cond, cond, guidance=1.5, seed=3, num_steps=4, condition_augment_sigma=AUG, xt=xt.clone(),
                                                       solver=solver, **kw)
    want = run()
    got = run(guidance_interval=(1e9, float("inf")))
    assert bool(torch.isfinite(got.float()).all()) and float(got.float().abs().max()) > 0
    _assert_equal(got, want, f"xt after the never-guided 4-step {solver} loop")


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
    euler, two = "g3_edm_cond_euler_step_bf16", "g3_edm_cond_2ab_step_bf16"

    def call_euler(oc=a, x=a, gt=a, ind_=ind, out=o, n_=n, T=1, hw=n, sigma=1.0, inv_sigma=1.0):
        return lib.g3_edm_cond_euler_step_bf16(p(oc), p(x), p(gt), p(ind_), p(out), n_, T, hw, 1.0, 1.0, 1.0, 1.0, sigma, inv_sigma, 0.5, s)

    def call_2ab(oc=a, x=a, gt=a, ind_=ind, out=o, n_=n, T=1, hw=n, sigma=1.0, inv_sigma=1.0, x0_prev=prev, x0_out=h, have_prev=1, coef_a=0.5):
        return lib.g3_edm_cond_2ab_step_bf16(p(oc), p(x), p(gt), p(ind_), p(out), n_, T, hw, 1.0, 1.0, 1.0, 1.0, sigma, inv_sigma, 0.5,
                                             p(x0_prev), p(x0_out), have_prev, coef_a, 0.3, 0.2, s)

    shared = dict(null_out_cond=dict(oc=None), null_new_xt=dict(x=None), null_gt_latent=dict(gt=None), null_indicator=dict(ind_=None),
                  null_xt_next=dict(out=None), n_zero=dict(n_=0), n_negative=dict(n_=-1), T_zero=dict(T=0), hw_zero=dict(hw=0),
                  sigma_zero=dict(sigma=0.0), sigma_negative=dict(sigma=-1.0), inv_sigma_zero=dict(inv_sigma=0.0),
                  inv_sigma_nan=dict(inv_sigma=float("nan")))
    only_2ab = dict(null_x0_out=dict(x0_out=None), null_x0_out_without_history=dict(x0_out=None, have_prev=0),
                    history_without_x0_prev=dict(x0_prev=None), a_zero=dict(coef_a=0.0), a_negative=dict(coef_a=-0.5),
                    a_nan=dict(coef_a=float("nan")), a_inf=dict(coef_a=float("inf")))
    for entry, call, cases in ((euler, call_euler, shared), (two, call_2ab, {**shared, **only_2ab})):
        for what, kw in cases.items():
            rc = call(**kw)
            assert rc != 0, (entry, what)
            assert entry in L.last_error(), (entry, what, L.last_error())
            with pytest.raises(L.Gen3cHipError, match=entry):
                L.check(rc, entry)
    with pytest.raises(L.Gen3cHipError, match=euler):  # the same refusals through the front ends the sampler uses
        ops.edm_cond_euler_step(a, a, a, ind, 1, n, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
    with pytest.raises(L.Gen3cHipError, match=two):
        ops.edm_cond_2ab_step(a, a, a, ind, 1, n, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, h, True, 0.5, 0.3, 0.2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o.float()).all()) and bool(torch.isnan(h).all()), "a refused call wrote output"
    assert call_euler() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(o.float()).any())
    o.fill_(float("nan"))
    assert call_2ab(x0_prev=None, have_prev=0, coef_a=0.0) == 0  # without history neither x0_prev nor `a` is looked at
    torch.cuda.synchronize()
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(h).any())


# ---- the command line --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["euler", "2ab"])
def test_single_image_cli_runs_the_interval_loop(tmp_path, capsys, monkeypatch, solver):
    """--guidance_interval 0.1,10 end to end through the single-image entry point (tiny random-weight models, 9-frame chunk, 4 steps with sigmas
    80, 7.99, 0.251, 2e-4): the steps call the cond, cfg, cfg, cond front ends, and the session says what the mode does."""
    from PIL import Image
    from gen3c_amd import gen3c_single_image as cli
    H, W = 64, 96
    ys, xs = np.mgrid[0:H, 0:W]
    Image.fromarray(np.stack([(xs * 2) % 256, (ys * 3) % 256, ((xs + ys) * 2) % 256], -1).astype(np.uint8)).save(tmp_path / "in.png")
    np.savez(tmp_path / "depth.npz", depth=(2.0 + 0.01 * xs).astype(np.float32), intrinsics=np.array([[80, 0, W / 2], [0, 80, H / 2], [0, 0, 1]], np.float32))
    monkeypatch.delenv("G3_GUIDANCE_INTERVAL", raising=False)
    seen = _record_front_ends(monkeypatch)
    args = cli.create_parser().parse_args([
        "--input_image_path", str(tmp_path / "in.png"), "--depth_path", str(tmp_path / "depth.npz"), "--height", str(H), "--width", str(W),
        "--num_steps", "4", "--random_init", "--tiny", "--video_save_folder", str(tmp_path / "out"), "--video_save_name", "v",
        "--trajectory", "clockwise", "--guidance_interval", "0.1,10", "--sampler_solver", solver])
    video = cli.demo(args)
    assert video.shape == (9, H, W, 3) and video.dtype == np.uint8
    if solver == "euler":
        assert seen == [("edm_cond_euler_step", None), ("edm_cfg_euler_step", None), ("edm_cfg_euler_step", None), ("edm_cond_euler_step", None)]
    else:  # step 1 is the first guided one (Euler update), step 2 has its history, the step to sigma 0 goes through the Euler entry
        assert seen == [("edm_cond_2ab_step", False), ("edm_cfg_2ab_step", False), ("edm_cfg_2ab_step", True), ("edm_cond_euler_step", None)]
    out = capsys.readouterr().out
    assert "--guidance_interval 0.1,10" in out and "outside the parity statement" in out


# ---- CFG-parallel ------------------------------------------------------------------------------------------------------------------------------
def test_cfg_parallel_pair_equals_the_single_process_interval_loop(tmp_path):
    """2 processes on cuda:0 over gloo (tests/_guidance_interval_cfg_worker.py): each rank's CFG-parallel interval loop, both solvers, ends
    bit-identical to its own single-process interval loop, the two ranks agree, and the pair exchanges on the guided steps only."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    worker = str(ROOT / "tests" / "_guidance_interval_cfg_worker.py")
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
