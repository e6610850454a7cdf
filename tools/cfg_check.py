"""CFG-parallel end-to-end check with the REAL HIP kernels on ONE GPU (sibling of tools/cp_check.py, same tiny net): 2 or 4 ranks (torchrun) share
cuda:0 and talk over gloo. The world is 2 guidance branches x cp = world / 2 context-parallel ranks (parallel_state.initialize_model_parallel(
cfg_parallel_size=2)): global rank r runs the conditional branch when r < cp, the unconditional one otherwise, and the pair {r, r + cp} exchanges the
network output of the step (parallel.cfg_exchange). Conditional and unconditional branch get different text contexts and guidance is 1.5, so a swapped
or duplicated branch changes the result.

  world 2 (cfg 2 x cp 1, context parallelism off on the net): the CFG-parallel step is torch.equal to this process's own single-rank step, two-call
    form and fused form, and the two ranks' outputs are equal.
  world 4 (cfg 2 x cp 2), for gather_first and local_first with 2 head groups: the reference is the plain cp = 2 step in the two-call form, computed
    twice by each CP group - the two runs must equal each other (a schedule that is not deterministic is reported as that) - and the CFG-parallel step
    is torch.equal to it on every rank; against the non-parallel full step it is held to cp_check's bar (rel-L2 < 5e-3) and the schedule that ran must
    be the requested one. Then the chunk's other stages sharded over all 4 ranks (the model-parallel group): render item pairs and the four tokenizer
    encodes, the same statements cp_check makes over its CP group.

  torchrun --nnodes=1 --nproc-per-node 4 --master-addr 127.0.0.1 --master-port 29512 tools/cfg_check.py
"""
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gen3c_amd.dit import VideoExtendGeneralDIT  # noqa: E402
from gen3c_amd.parallel import cfg_exchange, init_distributed, parallel_state, split_inputs_cp  # noqa: E402
from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask  # noqa: E402

GUIDANCE, STEP = 1.5, 5


def main():
    torch.cuda.set_device(0)
    init_distributed("gloo")
    world, rank = dist.get_world_size(), dist.get_rank()
    assert world in (2, 4), "cfg_check runs cfg 2 x cp 1 (2 ranks) or cfg 2 x cp 2 (4 ranks)"
    cp = world // 2
    parallel_state.initialize_model_parallel(context_parallel_size=cp, cfg_parallel_size=2)
    pair, cp_group, everyone = parallel_state.get_cfg_parallel_group(), parallel_state.get_context_parallel_group(), parallel_state.get_model_parallel_group()
    branch = parallel_state.get_cfg_parallel_rank()
    dev = torch.device("cuda:0")
    net = VideoExtendGeneralDIT(max_img_h=64, max_img_w=64, max_frames=32, in_channels=81, model_channels=512, num_blocks=2, num_heads=4,
                                adaln_lora_dim=64, crossattn_emb_channels=256, rope_t_extrapolation_ratio=2.0, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=11)
    B, T, H, W, M = 1, 4 * cp, 16, 24, 64
    rs = np.random.RandomState(3)
    nrm = lambda shape, std: torch.from_numpy((rs.standard_normal(shape) * std).astype(np.float32)).to(torch.bfloat16).to(dev)
    den = Gen3CDenoiser(net, state_shape=(16, T, H, W))
    den.scheduler.set_timesteps(35)
    xt = nrm((B, 16, T, H, W), den.scheduler.init_noise_sigma)
    gt, pose, ctx_c, ctx_u = nrm((B, 16, T, H, W), 0.5), nrm((B, 64, T, H, W), 0.5), nrm((B, M, 256), 0.2), nrm((B, M, 256), 0.2)
    pad = torch.zeros(B, 1, 8 * H, 8 * W, device=dev, dtype=torch.bfloat16)

    def cond(ctx, p):
        c = VideoExtendCondition(crossattn_emb=ctx, padding_mask=pad, fps=torch.tensor([24.0], device=dev), video_cond_bool=True,
                                 condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

    c, u = cond(ctx_c, pose), cond(ctx_u, torch.zeros_like(pose))
    good = True

    def check(what, ok, extra=""):
        nonlocal good
        sys.stdout.write(f"[cfg_check] rank {rank}/{world} (branch {branch}, cp rank {parallel_state.get_context_parallel_rank()}/{cp}): {what}: {bool(ok)}{extra}\n")
        sys.stdout.flush()  # one write per line: the ranks share a pipe
        good = good and bool(ok)

    def step(x, fuse):
        den.fuse_cond_uncond = fuse
        out = den.denoise_step(x, STEP, c, u, GUIDANCE, 0.001, 1)
        torch.cuda.synchronize()
        return out

    def pair_agrees(x):
        return torch.equal(*cfg_exchange(x.cpu(), pair))  # a gathered host copy of both ranks' results

    # no parallelism at all: every rank computes the whole step, both forms
    full_two, full_fused = step(xt, False), step(xt, True)
    check("non-parallel fused step == two-call step", torch.equal(full_two, full_fused))
    check("swapping the branches changes the non-parallel step", not torch.equal(full_two, den.denoise_step(xt, STEP, u, c, GUIDANCE, 0.001, 1)))
    if cp == 1:
        den.enable_cfg_parallel(pair)
        par = step(xt, True)  # fuse_cond_uncond is not consulted under CFG-parallel
        den.disable_cfg_parallel()
        check("CFG-parallel step == single-rank two-call step", torch.equal(par, full_two))
        check("CFG-parallel step == single-rank fused step", torch.equal(par, full_fused))
        check("both ranks of the pair hold the same xt", pair_agrees(par))
    else:
        net.enable_context_parallel(cp_group)
        ref_full = split_inputs_cp(full_two, 2, cp_group).float()
        xs = split_inputs_cp(xt, 2, cp_group)
        for sched in ("gather_first", "local_first"):
            net._cp_attn.configure(head_groups=2, schedule=sched, kernel="auto", bounded=False)
            plain_a, plain_b = step(xs, False), step(xs, False)
            check(f"plain cp = {cp} ({sched}) two-call step is deterministic", torch.equal(plain_a, plain_b))
            den.enable_cfg_parallel(pair)
            par = step(xs, True)
            den.disable_cfg_parallel()
            eff = net._cp_attn.effective["schedule"]
            check(f"CFG-parallel ({sched}) step == plain cp = {cp} two-call step", torch.equal(par, plain_a), f" effective={eff}")
            check(f"CFG-parallel ({sched}) ran the requested schedule", eff == sched)
            rel = float((par.float() - ref_full).norm() / ref_full.norm())
            check(f"CFG-parallel ({sched}) vs non-parallel full step rel_l2 < 5e-3", rel < 5e-3 and np.isfinite(rel), f" rel_l2={rel:.3e}")
            check(f"both ranks of the pair hold the same xt ({sched})", pair_agrees(par))
        net._cp_attn.configure(head_groups=4, schedule="gather_first", kernel="auto", bounded=False)

        # ---- the chunk's other stages over ALL ranks (both branch groups need the same renders and latents, so the model-parallel group shares the work)
        from gen3c_amd import renderer
        from gen3c_amd.pipeline import DiffusionGen3CModel
        from gen3c_amd.tokenizer import VideoTokenizer
        hh, ww, n_frames = 64, 96, 9
        ys, xs_ = np.mgrid[0:hh, 0:ww].astype(np.float32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        K = t(np.array([[80.0, 0, ww / 2], [0, 80.0, hh / 2], [0, 0, 1]], np.float32))
        for n_buf, fg in ((1, False), (2, True)):
            depth = (3.0 + 0.01 * xs_ + 0.004 * ys).astype(np.float32)
            depth = np.where((ys - 30) ** 2 + (xs_ - 40) ** 2 < 15 ** 2, 1.5 + 0.002 * xs_, depth).astype(np.float32)
            img = np.stack([np.sin(xs_ * 0.2 + ch) * np.cos(ys * 0.15 - ch) for ch in range(3)], 0).astype(np.float32)
            cache = renderer.Cache3D_Buffer(frame_buffer_max=2, input_image=t(img)[None], input_depth=t(depth)[None, None], input_w2c=torch.eye(4, device=dev)[None],
                                            input_intrinsics=K[None], filter_points_threshold=0.05, foreground_masking=fg, input_format=["B", "C", "H", "W"])
            if n_buf == 2:
                w2 = torch.eye(4, device=dev)
                w2[0, 3] = -0.2
                cache.update_cache(t(img[::-1].copy())[None], t(depth * 1.1)[None, None], w2[None], new_intrinsics=K[None], depth_alignment=False)
            w2cs = torch.eye(4, device=dev).repeat(1, n_frames, 1, 1)
            w2cs[0, :, 0, 3] = torch.linspace(0.0, 0.3, n_frames, device=dev)
            Ks = K.repeat(1, n_frames, 1, 1)
            full_r = cache.render_cache(w2cs, Ks)
            cache.shard_group = everyone
            shard_r = cache.render_cache(w2cs, Ks)
            # masks bit-identical; colours are sums of fp32 atomics whose order is not reproducible between two launches (cp_check's statement)
            same = torch.equal(full_r[1], shard_r[1]) and torch.allclose(full_r[0], shard_r[0], rtol=1e-4, atol=1e-5)
            check(f"render sharded over {world} ranks (N={n_buf}, foreground_masking={fg}) == replicated", same,
                  f" (max colour diff {float((full_r[0] - shard_r[0]).abs().max()):.2e})")
        tk = VideoTokenizer(pixel_chunk_duration=n_frames, channels=16, device=dev)
        tk.net.init_random(seed=2)
        tk.register_mean_std(torch.zeros(16, 32), torch.ones(16, 32))
        renders, masks = shard_r
        net.disable_context_parallel()
        lat_full = DiffusionGen3CModel(net, tk, latent_shape=(16, 2, hh // 8, ww // 8)).encode_warped_frames(renders, masks, torch.bfloat16)
        lat_shard = DiffusionGen3CModel(net, tk, latent_shape=(16, 2, hh // 8, ww // 8), shard_group=everyone).encode_warped_frames(renders, masks, torch.bfloat16)
        check(f"tokenizer encodes sharded (4 clips over {world} ranks) == replicated", torch.equal(lat_full, lat_shard) and lat_full.shape == (1, 64, 2, hh // 8, ww // 8))
    torch.cuda.synchronize()
    ok = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    parallel_state.destroy_model_parallel()
    dist.destroy_process_group()
    if ok.item() != 1.0:
        sys.exit(1)
    if rank == 0:
        print("[cfg_check] OK", flush=True)


if __name__ == "__main__":
    main()
