"""The frame-window self-attention under context parallelism, end to end with the REAL HIP kernels on ONE GPU: N ranks (torchrun) share cuda:0 and talk
over gloo, as in tools/cp_check.py. The tiny DiT runs with self_attn_window=(1, 1) and the context-parallel switch on a latent of 8 frames x 16 x 16
= 256 tokens per frame, so every rank's first row is a multiple of the kernel's 256-row query block and the function is the single-GPU one. Each
rank compares the CP denoise step on its frame shard (ContextParallelAttention's "window_halo" schedule: split-size all-to-alls of the halo frames,
one g3_self_attn_fwd_window_cp_bf16 launch per head group) against the same windowed step computed without CP on the full latent, and checks the
schedule that ran and the bytes it received against parallel.window_halo_plan.

  torchrun --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 tools/cp_window_check.py
  G3_CP_CHECK_BACKEND=nccl with ONE rank: the same calls through the real RCCL group (a self-exchange).
"""
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gen3c_amd.dit import VideoExtendGeneralDIT  # noqa: E402
from gen3c_amd.parallel import init_distributed, parallel_state, split_inputs_cp, window_halo_plan  # noqa: E402
from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask  # noqa: E402

WINDOW = (1, 1)


def main():
    torch.cuda.set_device(0)
    backend = os.environ.get("G3_CP_CHECK_BACKEND", "gloo")
    init_distributed(backend)
    world, rank = dist.get_world_size(), dist.get_rank()
    parallel_state.initialize_model_parallel(context_parallel_size=world)
    dev = torch.device("cuda:0")
    D, n_blocks = 512, 2
    net = VideoExtendGeneralDIT(max_img_h=64, max_img_w=64, max_frames=32, in_channels=81, model_channels=D, num_blocks=n_blocks, num_heads=4,
                                adaln_lora_dim=64, crossattn_emb_channels=256, rope_t_extrapolation_ratio=2.0, device=dev, init_weights=False,
                                self_attn_window=WINDOW, self_attn_window_cp=True)
    net.initialize_weights(randomize_adaln=True, seed=11)
    B, T, H, W, M = 1, 8, 32, 32, 64  # 16 x 16 = 256 tokens per latent frame
    assert T % world == 0
    frame_len = (H // net.patch_spatial) * (W // net.patch_spatial)
    assert frame_len == 256 and net.patch_temporal == 1
    rs = np.random.RandomState(3)
    nrm = lambda shape, std: torch.from_numpy((rs.standard_normal(shape) * std).astype(np.float32)).to(torch.bfloat16).to(dev)
    den = Gen3CDenoiser(net, state_shape=(16, T, H, W))
    den.scheduler.set_timesteps(35)
    xt = nrm((B, 16, T, H, W), den.scheduler.init_noise_sigma)
    gt, pose, ctx = nrm((B, 16, T, H, W), 0.5), nrm((B, 64, T, H, W), 0.5), nrm((B, M, 256), 0.2)
    pad = torch.zeros(B, 1, 8 * H, 8 * W, device=dev, dtype=torch.bfloat16)

    def cond(p):
        c = VideoExtendCondition(crossattn_emb=ctx, padding_mask=pad, fps=torch.tensor([24.0], device=dev), video_cond_bool=True,
                                 condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

    c, u = cond(pose), cond(torch.zeros_like(pose))
    full = den.denoise_step(xt, 5, c, u, 1.0, 0.001, 1)  # no CP: every rank computes the whole windowed step (ops.self_attn_window)
    net.enable_context_parallel(parallel_state.get_context_parallel_group())
    net._cp_attn.configure(head_groups=2)  # two groups: alternating streams
    ref = split_inputs_cp(full, 2, net.cp_group).float()
    batches = []  # the batch size of every network forward of the step: what the exchange's byte count scales with
    hook = net.register_forward_pre_hook(lambda mod, args, kwargs: batches.append((args[0] if args else kwargs["x"]).shape[0]), with_kwargs=True)
    net._cp_attn.bytes_gathered = 0
    part = den.denoise_step(split_inputs_cp(xt, 2, net.cp_group), 5, c, u, 1.0, 0.001, 1)
    torch.cuda.synchronize()
    hook.remove()
    rel = float((part.float() - ref).norm() / ref.norm())
    eff = net._cp_attn.effective
    plan = window_halo_plan(T, world, *WINDOW)
    want = sum(n_blocks * 2 * plan["remote_frames"][rank] * frame_len * b * D * 2 for b in batches)  # K and V rows, bf16
    got = net._cp_attn.bytes_gathered
    print(f"[cp_window_check] rank {rank}/{world}: CP window_halo vs single-rank windowed denoise step rel_l2={rel:.3e} effective={eff['schedule']} "
          f"buffer={plan['buffers'][rank]} received {got} bytes (plan: {want}; forwards with batch {batches})", flush=True)
    good = bool(np.isfinite(rel)) and rel < 5e-3 and eff["schedule"] == "window_halo" and got == want and len(batches) > 0
    ok = torch.tensor([1.0 if good else 0.0], device=dev if backend == "nccl" else "cpu")
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    dist.destroy_process_group()
    if ok.item() != 1.0:
        sys.exit(1)
    if rank == 0:
        print("[cp_window_check] OK", flush=True)


if __name__ == "__main__":
    main()
