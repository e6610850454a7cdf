"""Worker of tests/test_guidance_interval_gpu.py::test_cfg_parallel_pair_equals_the_single_process_interval_loop: one of 2 processes that share cuda:0
and talk over gloo (built like tests/_sampler_2ab_cfg_worker.py). Each runs the 6-step loop with guidance in (0.1, 10] (steps 2 and 3 of 6) with the
real sampler kernels and an elementwise stand-in network, for both solvers: first on its own (two-call form), then as one rank of a CFG-parallel
pair, and holds the second to the first bit for bit; the pair then compares its two results. On an unguided step both ranks run the conditional
branch and nothing is exchanged: the exchange is counted.

  python tests/_guidance_interval_cfg_worker.py RANK PORT OUT_DIR      (started twice by the test, RANK 0 and 1, each under its own time limit)
"""
import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

bf16 = torch.bfloat16
GUIDANCE, AUG, SEED, STEPS, INTERVAL, GUIDED = 1.5, 0.001, 3, 6, (0.1, 10.0), 2


class StubNet:
    """Elementwise, non-linear in x, depends on the timestep and on the branch (the pose buffer is zero for the unconditional one)."""
    is_context_parallel_enabled = False

    def __init__(self):
        self.calls = 0

    def __call__(self, x, timesteps, condition_video_pose=None, **kw):
        self.calls += 1
        return (torch.tanh(x.float()) * (1 + 0.1 * timesteps.float()) + 0.05 * condition_video_pose[:, :16].float()).to(bf16)


def main():
    rank, port, out_dir = int(sys.argv[1]), sys.argv[2], sys.argv[3]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    from gen3c_amd import sampler
    from gen3c_amd.parallel import cfg_exchange, init_distributed, parallel_state
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask, guided_steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    init_distributed("gloo", timeout_s=60)
    try:
        parallel_state.initialize_model_parallel(context_parallel_size=1, cfg_parallel_size=2)
        pair = parallel_state.get_cfg_parallel_group()
        B, C, T, H, W = 1, 16, 3, 5, 7
        g = torch.Generator().manual_seed(5)
        gt = (0.5 * torch.randn(B, C, T, H, W, generator=g)).to(bf16).to(dev)
        pose = (0.5 * torch.randn(B, 64, T, H, W, generator=g)).to(bf16).to(dev)
        ctx = torch.zeros(B, 4, 8, dtype=bf16, device=dev)
        xt = (80.0 * torch.randn(B, C, T, H, W, generator=g)).to(bf16).to(dev)

        def cond(p):
            c = VideoExtendCondition(crossattn_emb=ctx, fps=torch.tensor([24.0], device=dev), video_cond_bool=True, condition_video_pose=p)
            return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

        c, u = cond(pose), cond(torch.zeros_like(pose))
        net = StubNet()
        den = Gen3CDenoiser(net, state_shape=(C, T, H, W))
        den.fuse_cond_uncond = False
        exchanges = []
        sampler.cfg_exchange = lambda out, group: exchanges.append(1) or cfg_exchange(out, group)  # the name denoise_step looks up
        run = lambda solver, interval: den.generate_samples_from_batch(c, u, guidance=GUIDANCE, seed=SEED, num_steps=STEPS, condition_augment_sigma=AUG,
                                                                       xt=xt.clone(), solver=solver, guidance_interval=interval)
        for solver in ("euler", "2ab"):
            net.calls = 0
            single, always = run(solver, INTERVAL), run(solver, None)
            assert sum(guided_steps(den.scheduler.sigmas, INTERVAL)) == GUIDED
            assert net.calls == (STEPS + GUIDED) + 2 * STEPS and not exchanges and not torch.equal(single, always), "the interval loop is the always-guided loop"
            den.enable_cfg_parallel(pair)
            net.calls = 0
            par = run(solver, INTERVAL)
            den.disable_cfg_parallel()
            torch.cuda.synchronize()
            assert net.calls == STEPS, f"rank {rank}, {solver}: {net.calls} network calls under CFG-parallel"
            assert len(exchanges) == GUIDED, f"rank {rank}, {solver}: {len(exchanges)} exchanges for {GUIDED} guided steps"
            exchanges.clear()
            assert par.dtype == bf16 and torch.equal(par.view(torch.int16), single.view(torch.int16)), \
                f"rank {rank}, {solver}: the CFG-parallel interval loop differs from the single-process one"
            mine, other = cfg_exchange(par.cpu(), pair)
            assert torch.equal(mine.view(torch.int16), other.view(torch.int16)), f"{solver}: the two ranks of the pair end with different xt"
        parallel_state.destroy_model_parallel()
        with open(os.path.join(out_dir, f"ok{rank}"), "w") as f:
            f.write("ok")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
