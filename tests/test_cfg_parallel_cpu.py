"""CPU (gloo, worlds of 2 and 4): CFG-parallel - the two classifier-free-guidance branches of a denoise step on separate rank groups (opt-in).
Groups and accessors of parallel_state with cfg_parallel_size = 2 (and unchanged with 1), cfg_exchange, Gen3CDenoiser.denoise_step with the sampler
kernels replaced by tests/sampler_ref.py and a stand-in net (bit-equal to the single-process two-call step; one net call per rank on its own branch),
broadcast / run_jobs_round_robin over the model-parallel group (tests/_cfg_parallel_gloo_worker.py), and the command line's layout helper."""
import socket

import pytest
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 4], ids=["cfg2_x_cp1", "cfg2_x_cp2"])
def test_cfg_parallel_groups_exchange_step_and_sharding(tmp_path, world):
    from tests._cfg_parallel_gloo_worker import worker
    mp.spawn(worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


def test_resolve_parallel_layout():
    from gen3c_amd.cli_common import resolve_parallel_layout
    for n, want in ((2, (2, 1)), (4, (2, 2)), (8, (2, 4)), (16, (2, 8))):
        assert resolve_parallel_layout(n, True, 16) == want
    for n in (1, 3, 6, 12):
        with pytest.raises(ValueError) as e:
            resolve_parallel_layout(n, True, 16)
        assert "[2, 4, 8, 16, 32]" in str(e.value) and str(n) in str(e.value)  # the message names the valid rank counts
    assert resolve_parallel_layout(4, True, 2) == (2, 2)  # the 9-frame --tiny chunk: 2 latent frames
    with pytest.raises(ValueError):
        resolve_parallel_layout(8, True, 2)
    for n in (1, 2, 3, 8):  # the option off: --num_gpus stays the context-parallel size, as before
        assert resolve_parallel_layout(n, False, 16) == (1, n)


def test_flag_and_env_switch_are_opt_in(monkeypatch):
    import argparse
    from gen3c_amd.cli_common import add_common_args, cfg_parallel_requested
    monkeypatch.delenv("G3_CFG_PARALLEL", raising=False)
    p = add_common_args(argparse.ArgumentParser())
    off, on = p.parse_args([]), p.parse_args(["--cfg_parallel", "--num_gpus", "4"])
    assert off.cfg_parallel is False and not cfg_parallel_requested(off)
    assert on.cfg_parallel is True and on.num_gpus == 4 and cfg_parallel_requested(on)
    monkeypatch.setenv("G3_CFG_PARALLEL", "0")
    assert not cfg_parallel_requested(off)
    monkeypatch.setenv("G3_CFG_PARALLEL", "1")
    assert cfg_parallel_requested(off)


def test_denoiser_and_model_defaults_are_off():
    from types import SimpleNamespace
    from gen3c_amd.parallel import parallel_state
    from gen3c_amd.sampler import Gen3CDenoiser
    assert Gen3CDenoiser(SimpleNamespace(is_context_parallel_enabled=False)).cfg_group is None
    assert parallel_state.get_cfg_parallel_group() is None and parallel_state.get_cfg_parallel_world_size() == 1 and parallel_state.get_cfg_parallel_rank() == 0
