"""Worker of tests/test_sampler_2ab_gpu.py::test_cfg_parallel_pair_equals_the_single_process_2ab_loop: one of 2 processes that share cuda:0 and talk
over gloo (as tools/cfg_check.py's ranks do). Each runs the 6-step "2ab" loop with the real sampler kernels and an elementwise stand-in network,
first on its own (two-call form), then as one rank of a CFG-parallel pair, and holds the second to the first bit for bit; the pair then compares
its two results. Both ranks keep their own x0 history: nothing but the network output is exchanged.

  python tests/_sampler_2ab_cfg_worker.py RANK PORT OUT_DIR      (started twice by the test, RANK 0 and 1, each under its own time limit)
"""
import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

bf16 = torch.bfloat16
GUIDANCE, AUG, SEED, STEPS = 1.5, 0.001, 3, 6


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
    from gen3c_amd.parallel import cfg_exchange, init_distributed, parallel_state
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
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
        run = lambda solver: den.generate_samples_from_batch(c, u, guidance=GUIDANCE, seed=SEED, num_steps=STEPS, condition_augment_sigma=AUG,
                                                             xt=xt.clone(), solver=solver)
        single, euler = run("2ab"), run("euler")
        assert net.calls == 4 * STEPS and not torch.equal(single, euler), "the 2ab loop is the Euler loop"
        den.enable_cfg_parallel(pair)
        net.calls = 0
        par = run("2ab")
        den.disable_cfg_parallel()
        torch.cuda.synchronize()
        assert net.calls == STEPS, f"rank {rank}: {net.calls} network calls under CFG-parallel"
        assert par.dtype == bf16 and torch.equal(par, single), f"rank {rank}: the CFG-parallel 2ab loop differs from the single-process one"
        assert torch.equal(*cfg_exchange(par.cpu(), pair)), "the two ranks of the pair end with different xt"
        parallel_state.destroy_model_parallel()
        with open(os.path.join(out_dir, f"ok{rank}"), "w") as f:
            f.write("ok")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
