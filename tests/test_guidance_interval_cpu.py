"""CPU: the opt-in guidance interval (gen3c_amd.sampler.check_guidance_interval / guided_steps, Gen3CDenoiser.guidance_interval, --guidance_interval):
which values are accepted, which steps of GEN3C's schedule are guided, and the plumbing - names, defaults, flag and environment down to the denoiser,
the pipeline's pass-through, and which network calls and kernel front ends each step of the loop makes - with the kernels replaced by recorders
and a stand-in network, no GPU."""
import argparse
import math
from types import SimpleNamespace

import pytest
import torch


def _denoiser():
    from gen3c_amd.sampler import Gen3CDenoiser
    return Gen3CDenoiser(SimpleNamespace(is_context_parallel_enabled=False), state_shape=(16, 2, 3, 4))


def test_check_guidance_interval_accepts_and_refuses():
    from gen3c_amd.sampler import check_guidance_interval
    assert check_guidance_interval(None) is None
    assert check_guidance_interval((0.19, 1.61)) == (0.19, 1.61)
    assert check_guidance_interval([0, 5]) == (0.0, 5.0) and all(isinstance(v, float) for v in check_guidance_interval([0, 5]))
    assert check_guidance_interval((0.5, float("inf"))) == (0.5, math.inf)
    for bad in ((1.0, 1.0), (2.0, 1.0), (-0.1, 1.0), (float("nan"), 1.0), (0.0, float("nan")), (float("inf"), float("inf")), (1.0,), (1.0, 2.0, 3.0),
                1.0, "0.1,10", ("a", "b")):
        with pytest.raises(ValueError, match="guidance interval"):
            check_guidance_interval(bad)


def test_denoiser_property_validates():
    den = _denoiser()
    assert den.guidance_interval is None
    den.guidance_interval = (0.5, 20)
    assert den.guidance_interval == (0.5, 20.0)
    with pytest.raises(ValueError, match="guidance interval"):
        den.guidance_interval = (20, 0.5)
    assert den.guidance_interval == (0.5, 20.0)
    den.guidance_interval = None
    assert den.guidance_interval is None
    with pytest.raises(ValueError, match="guidance interval"):
        den.generate_samples_from_batch(None, None, guidance_interval=(3.0, 2.0))  # refused before anything else is touched


def test_guided_steps_on_the_35_step_schedule():
    from gen3c_amd.sampler import EDMEulerScheduler, guided_steps
    sch = EDMEulerScheduler()
    sch.set_timesteps(35)
    g = guided_steps(sch.sigmas, (0.19, 1.61))
    assert len(g) == 35 and [i for i, v in enumerate(g) if v] == [18, 19, 20, 21, 22, 23]
    assert guided_steps(sch.sigmas[:-1], (0.19, 1.61)) == g  # the final sigma 0 is no step, given or not
    assert sum(guided_steps(sch.sigmas, (0.5, 20))) == 13
    assert guided_steps(sch.sigmas, None) == [True] * 35
    assert guided_steps(sch.sigmas, (0.0, float("inf"))) == [True] * 35
    sch.set_timesteps(24)
    assert sum(guided_steps(sch.sigmas, (0.19, 1.61))) == 4
    # open below, closed above, on the scheduler's fp32 sigma
    sch.set_timesteps(35)
    s18, s23 = float(sch.sigmas[18]), float(sch.sigmas[23])
    assert [i for i, v in enumerate(guided_steps(sch.sigmas, (s23, s18))) if v] == [18, 19, 20, 21, 22]


def test_parser_flag_and_environment(monkeypatch):
    from gen3c_amd.cli_common import add_common_args, apply_guidance_interval, guidance_interval_requested
    p = add_common_args(argparse.ArgumentParser())
    monkeypatch.delenv("G3_GUIDANCE_INTERVAL", raising=False)
    assert p.parse_args([]).guidance_interval is None
    said = []
    den = _denoiser()
    assert apply_guidance_interval(p.parse_args([]), den, log=said.append) is None and den.guidance_interval is None and not said
    got = apply_guidance_interval(p.parse_args(["--guidance_interval", "0.19,1.61"]), den, log=said.append)
    assert got == (0.19, 1.61) and den.guidance_interval == (0.19, 1.61)
    assert len(said) == 1 and "--guidance_interval" in said[0] and "outside the parity statement" in said[0]
    assert guidance_interval_requested(p.parse_args(["--guidance_interval", " 0.5 , inf "])) == (0.5, math.inf)
    monkeypatch.setenv("G3_GUIDANCE_INTERVAL", "0.5,20")
    den = _denoiser()
    assert apply_guidance_interval(p.parse_args([]), den, log=said.append) == (0.5, 20.0) and den.guidance_interval == (0.5, 20.0) and len(said) == 2
    assert "--guidance_interval" in said[1]
    assert guidance_interval_requested(p.parse_args(["--guidance_interval", "1,2"])) == (1.0, 2.0)  # the flag wins over the environment
    monkeypatch.setenv("G3_GUIDANCE_INTERVAL", "")
    assert guidance_interval_requested(p.parse_args([])) is None


@pytest.mark.parametrize("text", ["1", "1,2,3", "a,b", "2,1", "1,1", "-1,2", "nan,2", ",", "1;2"])
def test_malformed_values_are_refused(monkeypatch, text):
    from gen3c_amd.cli_common import add_common_args, guidance_interval_requested
    p = add_common_args(argparse.ArgumentParser())
    monkeypatch.delenv("G3_GUIDANCE_INTERVAL", raising=False)
    with pytest.raises(ValueError):
        guidance_interval_requested(p.parse_args([f"--guidance_interval={text}"]))
    monkeypatch.setenv("G3_GUIDANCE_INTERVAL", text)
    with pytest.raises(ValueError):
        guidance_interval_requested(p.parse_args([]))


def test_pipeline_hands_its_interval_down_to_the_denoiser():
    """Gen3cPipeline(guidance_interval=...) -> generate_world_from_video -> DiffusionGen3CModel.generate_samples_from_batch -> the denoiser's loop, on
    an unbuilt network: the tokenizer, the conditions and the loop itself are stand-ins (as tests/test_sampler_2ab_cpu.py does for the solver)."""
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from gen3c_amd.pipeline import DiffusionGen3CModel, Gen3cPipeline, generate_world_from_video
    net = VideoExtendGeneralDIT.__new__(VideoExtendGeneralDIT)
    tk = SimpleNamespace(pixel_chunk_duration=9, latent_chunk_duration=2)
    model = DiffusionGen3CModel(net, tk, latent_shape=(16, 2, 3, 4))
    assert model.denoiser.guidance_interval is None
    seen = []
    model._get_conditions = lambda *a, **k: ("cond", "uncond")
    model.denoiser.generate_samples_from_batch = lambda c, u, **kw: seen.append(kw["guidance_interval"]) or "sample"
    lat = torch.zeros(1, 16, 2, 3, 4)
    for interval in (None, (0.19, 1.61), (0.5, float("inf"))):
        pipe = Gen3cPipeline(model, guidance_interval=interval)
        assert pipe.guidance_interval == interval
        assert generate_world_from_video(model, model.state_shape, True, {}, 1.0, 4, 1, lat, 1, guidance_interval=pipe.guidance_interval) == "sample"
    assert generate_world_from_video(model, model.state_shape, True, {}, 1.0, 4, 1, lat, 1) == "sample"  # the keyword left out
    assert seen == [None, (0.19, 1.61), (0.5, math.inf), None]
    with pytest.raises(ValueError, match="guidance interval"):
        Gen3cPipeline(model, guidance_interval=(2.0, 1.0))


def test_loop_calls_per_step(monkeypatch):
    """Recorders in place of the kernels and the network. 6 steps, guidance in (0.1, 10]: steps 2 and 3 are guided. An unguided step makes ONE network
    call, with the condition's arguments and the un-concatenated input, leaves the fused-call cache alone and goes to the cond front end of the solver
    in force; a guided step makes the calls it makes today. Under "2ab" one history buffer serves both kinds of step, and a step whose guidedness
    differs from the previous step's runs without history. Without an interval the cond front ends are never reached."""
    from gen3c_amd import ops
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask, res_2ab_coefficients
    calls, net_calls = [], []

    def fake_cfg_2ab(oc, ou, new_xt, gt, ind, T, hw, g, csb, cob, cs, cout, sigma, inv_sigma, sigma_next, x0, have_prev, a, cb1, cb2):
        calls.append(("cfg_2ab", sigma, x0, bool(have_prev), (a, cb1, cb2)))
        return new_xt

    def fake_cond_2ab(oc, new_xt, gt, ind, T, hw, csb, cob, cs, cout, sigma, inv_sigma, sigma_next, x0, have_prev, a, cb1, cb2):
        calls.append(("cond_2ab", sigma, x0, bool(have_prev), (a, cb1, cb2)))
        return new_xt

    monkeypatch.setattr(ops, "edm_prepare_input", lambda xt, *a: (xt, xt))
    monkeypatch.setattr(ops, "edm_cfg_euler_step", lambda oc, ou, new_xt, *a: calls.append(("cfg_euler", a[-3])) or new_xt)
    monkeypatch.setattr(ops, "edm_cond_euler_step", lambda oc, new_xt, *a: calls.append(("cond_euler", a[-3])) or new_xt)
    monkeypatch.setattr(ops, "edm_cfg_2ab_step", fake_cfg_2ab)
    monkeypatch.setattr(ops, "edm_cond_2ab_step", fake_cond_2ab)

    def net(x, timesteps, **kw):
        net_calls.append((x.shape[0], kw["condition_video_pose"]))
        return x
    net.is_context_parallel_enabled = False
    den = Gen3CDenoiser(net, state_shape=(16, 2, 3, 4))
    gt = torch.zeros(1, 16, 2, 3, 4, dtype=torch.bfloat16)
    pose_c, pose_u = torch.ones(1, 64, 2, 3, 4), torch.zeros(1, 64, 2, 3, 4)
    mk = lambda pose: add_condition_video_indicator_and_video_input_mask(
        gt, VideoExtendCondition(crossattn_emb=torch.zeros(1, 2, 4), video_cond_bool=True, condition_video_pose=pose), 1)
    cond, uncond = mk(pose_c), mk(pose_u)
    run = lambda **kw: den.generate_samples_from_batch(cond, uncond, num_steps=6, xt=torch.zeros_like(gt), **kw)
    interval = (0.1, 10.0)

    den.fuse_cond_uncond = False
    run(guidance_interval=interval)
    assert [c[0] for c in calls] == ["cond_euler"] * 2 + ["cfg_euler"] * 2 + ["cond_euler"] * 2
    assert [b for b, _ in net_calls] == [1] * 8
    assert [p is pose_c for _, p in net_calls] == [True, True, True, False, True, False, True, True]
    calls.clear(), net_calls.clear()

    den.fuse_cond_uncond = True
    run(guidance_interval=interval)
    assert [b for b, _ in net_calls] == [1, 1, 2, 2, 1, 1] and all(p is pose_c for b, p in net_calls if b == 1)
    assert den._fused_cache is not None
    calls.clear(), net_calls.clear()
    den._fused_cache = None
    run(guidance_interval=(1e9, float("inf")))  # never guided: the fused-call cache is not touched
    assert den._fused_cache is None and [c[0] for c in calls] == ["cond_euler"] * 6 and [b for b, _ in net_calls] == [1] * 6
    calls.clear(), net_calls.clear()

    den.guidance_interval = interval  # the setting; "2ab"
    run(solver="2ab")
    den.guidance_interval = None
    sig = [float(v) for v in den.scheduler.sigmas]
    assert [c[0] for c in calls] == ["cond_2ab", "cond_2ab", "cfg_2ab", "cfg_2ab", "cond_2ab", "cond_euler"]
    assert [c[3] for c in calls[:5]] == [False, True, False, True, False]
    assert all(c[2] is calls[0][2] for c in calls[:5]) and calls[0][2].dtype == torch.float32 and calls[0][2].shape == gt.shape
    for i in (1, 3):
        assert calls[i][1] == sig[i] and calls[i][4] == res_2ab_coefficients(sig[i], sig[i + 1], sig[i - 1])
    for i in (0, 2, 4):
        assert calls[i][4] == (0.0, 0.0, 0.0)
    calls.clear(), net_calls.clear()

    for kw in ({}, dict(guidance_interval=None), dict(solver="2ab")):  # no interval: today's calls
        run(**kw)
    assert [c[0] for c in calls] == ["cfg_euler"] * 12 + ["cfg_2ab"] * 5 + ["cfg_euler"]
    assert [c[3] for c in calls[12:17]] == [False, True, True, True, True]
    assert [b for b, _ in net_calls] == [2] * 18


def test_denoise_step_keeps_its_positional_signature():
    import inspect
    from gen3c_amd.sampler import Gen3CDenoiser
    params = inspect.signature(Gen3CDenoiser.denoise_step).parameters
    assert list(params)[:8] == ["self", "xt", "step_index", "condition", "uncondition", "guidance", "condition_augment_sigma", "seed"]
    assert params["guided"].kind is inspect.Parameter.KEYWORD_ONLY and params["guided"].default is True
    assert params["solver_state"].kind is inspect.Parameter.KEYWORD_ONLY
