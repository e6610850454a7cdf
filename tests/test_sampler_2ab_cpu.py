"""CPU: the opt-in second-order multistep sampler solver "2ab" (gen3c_amd.sampler.res_2ab_coefficients, Gen3CDenoiser.solver, --sampler_solver).
  * coefficients against what the reference's functional/multi_step.py::order2_fn computed, recorded step by step in
    tests/golden/res_2ab/order2_fn_12_steps.npz (tools/gen_res_2ab_golden.py);
  * the convergence proxy of DESIGN.md section 12 (tools/sampler_solver_proxy.py: pure fp64 loops around res_2ab_coefficients);
  * plumbing: names, defaults, flag and environment down to the denoiser, and which kernel front end the loop calls at which step - with the
    kernels replaced by recorders and an unbuilt network, no GPU."""
import argparse
import functools
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


# ---- coefficients ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(ROOT / "tests" / "golden" / "res_2ab" / "order2_fn_12_steps.npz"))


def test_coefficients_reproduce_the_recorded_reference_steps():
    from gen3c_amd.sampler import res_2ab_coefficients
    g = _golden()
    assert g["x_t"].shape == (11, 64) and list(g["have_prev"]) == [0] + [1] * 10
    worst = 0.0
    for i in range(1, 11):
        a, cb1, cb2 = res_2ab_coefficients(float(g["s"][i]), float(g["t"][i]), float(g["s1"][i]))
        got = a * g["x_s"][i] + cb1 * g["x0_s"][i] + cb2 * g["x0_prev"][i]
        rel = float(np.abs(got - g["x_t"][i]).max() / np.abs(g["x_t"][i]).max())
        worst = max(worst, rel)
        assert rel <= 1e-12, (i, rel)
        assert g["s1"][i] == g["s"][i - 1] and np.array_equal(g["x0_prev"][i], g["x0_s"][i - 1])  # the history is the previous step's
    print(f"max relative difference to the recorded order2_fn steps: {worst:.1e}")


def test_first_recorded_step_has_no_history_and_is_the_euler_step():
    g = _golden()
    s, t, x, x0 = float(g["s"][0]), float(g["t"][0]), g["x_s"][0], g["x0_s"][0]
    assert g["have_prev"][0] == 0 and np.isnan(g["s1"][0])
    want = (t / s) * x + (1 - t / s) * x0
    assert float(np.abs(want - g["x_t"][0]).max() / np.abs(g["x_t"][0]).max()) <= 1e-12


def test_coefficients_sum_to_one_on_the_35_step_schedule():
    """a + cb1 + cb2 = 1: a constant denoiser output equal to x is a fixed point, as for the Euler step's t/s + (1 - t/s)."""
    from gen3c_amd.sampler import EDMEulerScheduler, res_2ab_coefficients
    sch = EDMEulerScheduler()
    sch.set_timesteps(35)
    sig = [float(v) for v in sch.sigmas]
    assert sig[35] == 0.0
    for i in range(1, 34):  # every step that has a previous one and does not end at sigma 0
        a, cb1, cb2 = res_2ab_coefficients(sig[i], sig[i + 1], sig[i - 1])
        assert abs(a + cb1 + cb2 - 1.0) <= 1e-14, (i, a + cb1 + cb2 - 1.0)
        assert 0.0 < a < 1.0 and np.isfinite(np.float32(a)) and np.float32(a) > 0  # what the entry's refusal of a non-positive `a` expects


# ---- convergence proxy -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _proxy():
    from tools import sampler_solver_proxy as proxy
    tab = proxy.table(steps=(24, 35))
    print(proxy.render(tab))
    return tab


@pytest.mark.parametrize("denoiser", ["a", "b"])
def test_the_two_solvers_converge_to_the_same_solution(denoiser):
    assert _proxy()[denoiser]["reference_gap"] <= 1e-3


@pytest.mark.parametrize("denoiser", ["a", "b"])
def test_2ab_halves_the_euler_error_at_35_steps(denoiser):
    t = _proxy()[denoiser]
    assert t["2ab"][35] <= 0.5 * t["euler"][35], (t["2ab"][35], t["euler"][35])


@pytest.mark.parametrize("denoiser", ["a", "b"])
def test_2ab_at_24_steps_is_below_euler_at_35(denoiser):
    t = _proxy()[denoiser]
    assert t["2ab"][24] < t["euler"][35], (t["2ab"][24], t["euler"][35])


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------------
def _denoiser():
    from gen3c_amd.sampler import Gen3CDenoiser
    return Gen3CDenoiser(SimpleNamespace(is_context_parallel_enabled=False), state_shape=(16, 2, 3, 4))


def test_default_is_euler_and_unknown_names_raise():
    from gen3c_amd.cli_common import add_common_args
    den = _denoiser()
    assert den.solver == "euler"
    den.solver = "2ab"
    assert den.solver == "2ab"
    with pytest.raises(ValueError, match=r"euler.*2ab"):
        den.solver = "heun"
    assert den.solver == "2ab"
    with pytest.raises(ValueError, match=r"euler.*2ab"):
        den.generate_samples_from_batch(None, None, solver="rk4")  # refused before anything else is touched
    p = add_common_args(argparse.ArgumentParser())
    assert p.parse_args([]).sampler_solver == "euler" and p.parse_args(["--sampler_solver", "2ab"]).sampler_solver == "2ab"
    with pytest.raises(SystemExit):
        p.parse_args(["--sampler_solver", "heun"])


def test_flag_and_environment_reach_the_denoiser(monkeypatch):
    from gen3c_amd.cli_common import add_common_args, apply_sampler_solver, sampler_solver_requested
    p = add_common_args(argparse.ArgumentParser())
    monkeypatch.delenv("G3_SAMPLER_SOLVER", raising=False)
    said = []
    den = _denoiser()
    assert apply_sampler_solver(p.parse_args([]), den, log=said.append) == "euler" and den.solver == "euler" and not said
    assert apply_sampler_solver(p.parse_args(["--sampler_solver", "2ab"]), den, log=said.append) == "2ab" and den.solver == "2ab"
    assert len(said) == 1 and "outside the parity statement" in said[0]
    monkeypatch.setenv("G3_SAMPLER_SOLVER", "2ab")
    den = _denoiser()
    assert apply_sampler_solver(p.parse_args([]), den, log=said.append) == "2ab" and den.solver == "2ab" and len(said) == 2
    monkeypatch.setenv("G3_SAMPLER_SOLVER", "euler")
    assert sampler_solver_requested(p.parse_args([])) == "euler"
    monkeypatch.setenv("G3_SAMPLER_SOLVER", "heun")
    with pytest.raises(ValueError, match=r"euler.*2ab"):
        sampler_solver_requested(p.parse_args([]))


def test_pipeline_hands_its_solver_down_to_the_denoiser():
    """Gen3cPipeline(sampler_solver=...) -> generate_world_from_video -> DiffusionGen3CModel.generate_samples_from_batch -> the denoiser's loop, on an
    unbuilt network: the tokenizer, the conditions and the loop itself are stand-ins."""
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from gen3c_amd.pipeline import DiffusionGen3CModel, Gen3cPipeline, generate_world_from_video
    net = VideoExtendGeneralDIT.__new__(VideoExtendGeneralDIT)
    tk = SimpleNamespace(pixel_chunk_duration=9, latent_chunk_duration=2)
    model = DiffusionGen3CModel(net, tk, latent_shape=(16, 2, 3, 4))
    assert model.denoiser.solver == "euler"
    seen = []
    model._get_conditions = lambda *a, **k: ("cond", "uncond")
    model.denoiser.generate_samples_from_batch = lambda c, u, **kw: seen.append(kw["solver"]) or "sample"
    lat = torch.zeros(1, 16, 2, 3, 4)
    for name in (None, "euler", "2ab"):
        pipe = Gen3cPipeline(model, sampler_solver=name)
        assert pipe.sampler_solver == name
        assert generate_world_from_video(model, model.state_shape, True, {}, 1.0, 4, 1, lat, 1, solver=pipe.sampler_solver) == "sample"
    assert generate_world_from_video(model, model.state_shape, True, {}, 1.0, 4, 1, lat, 1) == "sample"  # the keyword left out
    assert seen == [None, "euler", "2ab", None]
    with pytest.raises(ValueError, match=r"euler.*2ab"):
        Gen3cPipeline(model, sampler_solver="heun")


def test_loop_calls_the_euler_front_end_unless_2ab_is_asked_for(monkeypatch):
    """Which front end each step of the loop calls, with recorders in place of the kernels: "euler" (by default, by name, by the denoiser's setting)
    never reaches ops.edm_cfg_2ab_step; "2ab" takes it for every step but the one to sigma 0, without history at step 0 and then with the
    coefficients of res_2ab_coefficients and ONE history buffer updated in place; a second call starts without history again."""
    from gen3c_amd import ops
    from gen3c_amd.sampler import VideoExtendCondition, add_condition_video_indicator_and_video_input_mask, res_2ab_coefficients
    calls = []

    def fake_2ab(oc, ou, new_xt, gt, ind, T, hw, g, csb, cob, cs, cout, sigma, inv_sigma, sigma_next, x0, have_prev, a, cb1, cb2):
        calls.append(("2ab", sigma, sigma_next, x0, bool(have_prev), (a, cb1, cb2)))
        return new_xt

    monkeypatch.setattr(ops, "edm_prepare_input", lambda xt, *a: (xt, xt))
    monkeypatch.setattr(ops, "edm_cfg_euler_step", lambda oc, ou, new_xt, *a: calls.append(("euler", a[-3], a[-1])) or new_xt)
    monkeypatch.setattr(ops, "edm_cfg_2ab_step", fake_2ab)
    net = lambda x, timesteps, **kw: x
    net.is_context_parallel_enabled = False
    from gen3c_amd.sampler import Gen3CDenoiser
    den = Gen3CDenoiser(net, state_shape=(16, 2, 3, 4))
    gt = torch.zeros(1, 16, 2, 3, 4, dtype=torch.bfloat16)
    cond = add_condition_video_indicator_and_video_input_mask(gt, VideoExtendCondition(crossattn_emb=torch.zeros(1, 2, 4), video_cond_bool=True), 1)
    run = lambda **kw: den.generate_samples_from_batch(cond, cond, num_steps=5, xt=torch.zeros_like(gt), **kw)
    run()
    run(solver="euler")
    assert [c[0] for c in calls] == ["euler"] * 10
    calls.clear()
    den.solver = "2ab"
    run(solver="euler")  # the argument wins over the setting
    assert [c[0] for c in calls] == ["euler"] * 5
    calls.clear()
    run()                # the setting
    den.solver = "euler"
    run(solver="2ab")    # the argument
    sig = [float(v) for v in den.scheduler.sigmas]
    for first in (0, 5):
        loop = calls[first:first + 5]
        assert [c[0] for c in loop] == ["2ab"] * 4 + ["euler"] and loop[4][1:] == (sig[4], 0.0)
        assert [c[4] for c in loop[:4]] == [False, True, True, True]
        assert all(c[3] is loop[0][3] for c in loop[:4]) and loop[0][3].dtype == torch.float32 and loop[0][3].shape == gt.shape
        for i in (1, 2, 3):
            assert loop[i][1:3] == (sig[i], sig[i + 1]) and loop[i][5] == res_2ab_coefficients(sig[i], sig[i + 1], sig[i - 1])
    assert calls[0][3] is not calls[5][3]  # a history buffer per call
    calls.clear()
    den.generate_samples_from_batch(cond, cond, num_steps=2, xt=torch.zeros_like(gt), solver="2ab")
    assert [(c[0], c[4] if c[0] == "2ab" else None) for c in calls] == [("2ab", False), ("euler", None)]
    calls.clear()
    den.generate_samples_from_batch(cond, cond, num_steps=1, xt=torch.zeros_like(gt), solver="2ab")
    assert [c[0] for c in calls] == ["euler"]
