"""gloo worker of tests/test_cfg_parallel_cpu.py (a module of its own so that torch.multiprocessing's spawned children can import it): one process per
rank of a world of 2 (cfg 2 x cp 1) or 4 (cfg 2 x cp 2). No kernel runs here: the two sampler kernels are replaced by tests/sampler_ref.py's
statements of them and the network by an elementwise stand-in, so what is checked is the second parallel axis itself - groups, exchange, branch
selection, broadcast source, job sharding."""
import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tests import sampler_ref as sr  # noqa: E402

bf16 = torch.bfloat16
GUIDANCE, STEP, AUG, SEED = 1.5, 5, 0.001, 3


class StubNet:
    """Deterministic, frame-wise function of (x, crossattn_emb, condition_video_pose) with the DiT's context-parallel surface: like the DiT it is
    handed the full-length pose buffer and cuts this rank's frames out itself."""

    def __init__(self):
        self.cp_group = None
        self.calls = []

    @property
    def is_context_parallel_enabled(self):
        return self.cp_group is not None

    def __call__(self, x, timesteps, crossattn_emb=None, condition_video_pose=None, **kw):
        from gen3c_amd.parallel import split_inputs_cp
        self.calls.append(dict(rows=x.shape[0], ctx=crossattn_emb, pose=condition_video_pose))
        pose = condition_video_pose if self.cp_group is None else split_inputs_cp(condition_video_pose, 2, self.cp_group)
        return (torch.tanh(x.float()) * (1 + 0.1 * timesteps.float()) + 0.05 * pose[:, :16].float() + crossattn_emb.float().mean()).to(bf16)


def _denoiser_inputs(T):
    from gen3c_amd.sampler import VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
    B, C, H, W = 1, 16, 3, 5
    g = torch.Generator().manual_seed(5)
    gt = (0.5 * torch.randn(B, C, T, H, W, generator=g)).to(bf16)
    pose = (0.5 * torch.randn(B, 64, T, H, W, generator=g)).to(bf16)
    ctx_c, ctx_u = (torch.randn(B, 4, 8, generator=g).to(bf16) for _ in range(2))
    xt = (80.0 * torch.randn(B, C, T, H, W, generator=g)).to(bf16)

    def cond(ctx, p):
        c = VideoExtendCondition(crossattn_emb=ctx, fps=torch.tensor([24.0]), video_cond_bool=True, condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

    return xt, cond(ctx_c, pose), cond(ctx_u, torch.zeros_like(pose)), (C, T, H, W)


def _patch_sampler_kernels(sigma32, sigma_next32):
    """gen3c_amd.ops.edm_prepare_input / edm_cfg_euler_step -> sampler_ref.prepare / step (same arguments; the host coefficients are recomputed there)."""
    from gen3c_amd import ops
    ops.edm_prepare_input = lambda xt, gt, noise, ind_t, T, HW, aug, *coef: sr.prepare(xt, gt, noise, ind_t.reshape(1, 1, T, 1, 1), sigma32, aug)
    ops.edm_cfg_euler_step = lambda oc, ou, new_xt, gt, ind_t, T, HW, guidance, *coef: sr.step(oc, ou, new_xt, gt, ind_t.reshape(1, 1, T, 1, 1), sigma32,
                                                                                               sigma_next32, guidance)


def worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from gen3c_amd import parallel
    from gen3c_amd.parallel import parallel_state as ps
    from gen3c_amd.sampler import Gen3CDenoiser
    parallel.init_distributed("gloo")
    cp = world // 2
    try:
        # ---- 1. groups. cfg_parallel_size = 1 first: what the function builds today, and nothing else
        ps.initialize_model_parallel(context_parallel_size=cp)
        plain = ps.get_context_parallel_group()
        assert dist.get_process_group_ranks(plain) == list(range(rank // cp * cp, rank // cp * cp + cp))
        assert ps.get_context_parallel_rank() == rank % cp and ps.get_context_parallel_world_size() == cp
        assert ps.get_cfg_parallel_group() is None and ps.get_cfg_parallel_rank() == 0 and ps.get_cfg_parallel_world_size() == 1
        assert ps.get_model_parallel_group() is plain
        ps.destroy_model_parallel()
        assert not ps.is_initialized() and ps.get_cfg_parallel_group() is None
        ps.initialize_model_parallel(context_parallel_size=cp, cfg_parallel_size=2)
        cp_group, pair, everyone = ps.get_context_parallel_group(), ps.get_cfg_parallel_group(), ps.get_model_parallel_group()
        assert dist.get_process_group_ranks(cp_group) == list(range(rank // cp * cp, rank // cp * cp + cp))
        assert dist.get_process_group_ranks(pair) == [rank % cp, rank % cp + cp]
        assert dist.get_process_group_ranks(everyone) == list(range(world))
        assert ps.get_cfg_parallel_rank() == rank // cp and ps.get_cfg_parallel_world_size() == 2
        assert ps.get_context_parallel_rank() == rank % cp and ps.get_context_parallel_world_size() == cp
        try:
            ps.initialize_model_parallel(context_parallel_size=world, cfg_parallel_size=2)  # world != 2 x cp: refused before any group is created
            raise RuntimeError("world != 2 x cp was accepted")
        except AssertionError:
            pass

        # ---- 2. cfg_exchange: slot 0 is the conditional rank's tensor on both ranks of every pair
        mine = torch.full((2, 3), float(rank + 1)).to(bf16)
        oc, ou = parallel.cfg_exchange(mine, pair)
        assert torch.equal(oc, torch.full((2, 3), float(rank % cp + 1)).to(bf16)) and torch.equal(ou, torch.full((2, 3), float(rank % cp + cp + 1)).to(bf16))
        oc, ou = parallel.cfg_exchange(torch.arange(12.0).reshape(3, 4).t() + rank, pair)  # a strided input
        assert torch.equal(oc, torch.arange(12.0).reshape(3, 4).t() + rank % cp) and torch.equal(ou, oc + cp)

        # ---- 3. denoise_step: one net call per rank, this rank's branch, B rows; bit-equal to the single-process two-call step
        T = 2 * cp
        xt, c, u, state = _denoiser_inputs(T)
        net = StubNet()
        den = Gen3CDenoiser(net, state_shape=state)
        den.scheduler.set_timesteps(35)
        _patch_sampler_kernels(den.scheduler.sigmas[STEP], den.scheduler.sigmas[STEP + 1])
        den.fuse_cond_uncond = False
        single = den.denoise_step(xt, STEP, c, u, GUIDANCE, AUG, SEED)
        assert len(net.calls) == 2 and not torch.equal(single, den.denoise_step(xt, STEP, u, c, GUIDANCE, AUG, SEED))  # the branches matter
        den.fuse_cond_uncond = True  # not consulted under CFG-parallel
        if cp > 1:
            net.cp_group = cp_group
        den.enable_cfg_parallel(pair)
        shard = (lambda t: parallel.split_inputs_cp(t, 2, cp_group)) if cp > 1 else (lambda t: t)
        net.calls.clear()
        out = den.denoise_step(shard(xt), STEP, c, u, GUIDANCE, AUG, SEED)
        assert len(net.calls) == 1 and net.calls[0]["rows"] == xt.shape[0] and den._fused_cache is None
        own = c if rank // cp == 0 else u
        assert net.calls[0]["ctx"] is own.crossattn_emb and net.calls[0]["pose"] is own.condition_video_pose
        assert out.dtype == bf16 and torch.equal(out, shard(single)), f"rank {rank}: CFG-parallel step differs from the two-call step"
        swapped = den.denoise_step(shard(xt), STEP, u, c, GUIDANCE, AUG, SEED)
        assert not torch.equal(swapped, out)
        den.disable_cfg_parallel()
        net.cp_group = None
        assert den.cfg_group is None

        # ---- 4. broadcast from the lowest rank of the model-parallel group (also with to_cp=False: cfg 2 x cp 1 has no context parallelism), jobs over all ranks
        for to_cp in (True, False):
            t = torch.arange(10.0).reshape(2, 5) + rank if rank == 0 else torch.zeros(1, 1)
            assert torch.equal(parallel.broadcast(t, to_cp=to_cp), torch.arange(10.0).reshape(2, 5))
            assert parallel.broadcast(f"from {rank}", to_cp=to_cp) == "from 0"
        ran = []
        jobs = [(lambda j=j: (ran.append(j), torch.full((1, 2), float(j + 1)))[1]) for j in range(5)]
        outs = parallel.run_jobs_round_robin(jobs, everyone, (1, 2), torch.float32, torch.device("cpu"))
        assert ran == list(range(rank, 5, world)) and [float(o.mean()) for o in outs] == [1.0, 2.0, 3.0, 4.0, 5.0]
        ps.destroy_model_parallel()
        assert ps.get_cfg_parallel_group() is None and not ps.is_initialized()
        with open(os.path.join(tmp, f"ok{rank}"), "w") as f:
            f.write("ok")
    finally:
        dist.destroy_process_group()
