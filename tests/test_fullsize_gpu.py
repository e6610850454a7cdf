"""GPU: the two MFMA kernels at BASELINE.json's full size (56 320 tokens, 32 x 128 heads, D = 4096), checked through properties
that do not need the (far too slow) CPU oracle at this size:
  * sampled rows against an fp32 torch reference of the same op on the same device (the op is floating point; tolerances below);
  * permutation invariance of attention over the key/value tokens;
  * linearity of the GEMM in its token rows (row subsets give the same rows)."""
import math
import os
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
S, D, HD = 56320, 4096, 128


def _rel_l2(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def test_attention_full_sequence_sampled_rows_and_kv_permutation():
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    H = 4  # four of the 32 heads keep the test at ~2 s; every head runs the same code path
    g = torch.Generator(device=dev).manual_seed(7)
    q = torch.randn(S, H * HD, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(S, H * HD, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(S, H * HD, device=dev, generator=g).to(torch.bfloat16)
    out = ops.flash_attn(q, k, ops.transpose_v(v, S, 1, H), S, S, 1, H)
    rows = torch.cat([torch.arange(0, 64, device=dev), torch.randint(0, S, (128,), device=dev, generator=g), torch.arange(S - 64, S, device=dev)])
    for h in range(H):
        sl = slice(h * HD, (h + 1) * HD)
        sc = (q[rows, sl].float() @ k[:, sl].float().t()) / math.sqrt(HD)
        ref = torch.softmax(sc, dim=-1) @ v[:, sl].float()
        r = _rel_l2(out[rows, sl], ref)
        # bf16 Q*scale, P and output roundings give 2.9e-3 here; a staging race in the first tiles (K read before its LDS-DMA landed,
        # or overwritten while a late wave still reads it) showed up as 6.6e-3 on this very check
        assert r < 4e-3, f"head {h}: rel-L2 {r:.3e} vs fp32 reference on sampled rows"
    # softmax(QK^T)V does not depend on the order of the key/value tokens
    perm = torch.randperm(S, device=dev, generator=g)
    out_p = ops.flash_attn(q, k[perm].contiguous(), ops.transpose_v(v[perm].contiguous(), S, 1, H), S, S, 1, H)
    r = _rel_l2(out_p, out)
    print(f"[attn 56320] kv-permutation rel-L2 {r:.3e}")
    # P is rounded to bf16 relative to the running maximum of ITS tile order, so the two runs carry independent 2^-9 roundings; with
    # zero-mean random V the output is itself a random-walk sum and that rounding noise does not average out: expect ~3e-3
    assert r < 6e-3


@pytest.mark.parametrize("N,K,epi", [(12288, 4096, 0), (16384, 4096, 1), (4096, 16384, 2)])
def test_gemm_full_size_sampled_rows_and_row_subsets(N, K, epi):
    from gen3c_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N + K)
    a = torch.randn(S, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    gate = torch.randn(1, N, device=dev, generator=g).to(torch.bfloat16)
    res = torch.randn(S, N, device=dev, generator=g).to(torch.bfloat16)
    kw = dict(gate=gate, residual=res) if epi == 2 else {}
    out = ops.gemm_nt(a, w, epilogue=epi, **kw)
    rows = torch.cat([torch.arange(0, 32, device=dev), torch.randint(0, S, (192,), device=dev, generator=g), torch.arange(S - 32, S, device=dev)])
    ref = a[rows].float() @ w.float().t()
    if epi == 1:
        ref = torch.nn.functional.gelu(ref)
    elif epi == 2:
        ref = res[rows].float() + gate.float() * ref
    r = _rel_l2(out[rows], ref)
    assert r < 4e-3, f"rel-L2 {r:.3e} vs fp32 reference on sampled rows"
    # the same rows computed as their own (ragged, 1 000-row) problem are bit-identical: every output element accumulates over K in
    # the same order whatever tile it lands in
    sub = slice(12345, 13345)
    kw2 = dict(gate=gate, residual=res[sub].contiguous()) if epi == 2 else {}
    out_sub = ops.gemm_nt(a[sub].contiguous(), w, epilogue=epi, **kw2)
    assert torch.equal(out_sub, out[sub])


def _bench_launch_operands(dev, H=32, B=2, seed=11, chain="default"):
    """The operands of the benchmark's self-attention launch, produced the way the DiT forward produces them (gen3c_amd/dit.py, the arms of the
    self-attention block; chain="default" resolves through the predicates forward() itself uses, so it follows the product's default, whatever it is):
      * "swap" (the default since round 6, dit._v_by_operand_swap): the q | k projection on the first 2 D rows of the fused weight, q and k normalised +
        rotated IN PLACE by ONE pass (g3_qk_rmsnorm_rope_pair_bf16), and V projected with the operands swapped, one GEMM per batch item (N = S,
        ldw = B D) straight into vt[b][:, :S];
      * "separate" (G3_V_OPERAND_SWAP=0, and every S % 4 != 0): ONE plain QKV projection into a [S*B, 3*H*128] buffer, then q and k normalised + rotated
        IN PLACE on strided column views of it and the v columns transposed into V^T by g3_transpose_v_bf16;
      * "fused" (G3_FUSE_QKV_EPILOGUE=1): g3_gemm_qk_norm_rope_bf16 does all three in the projection's epilogue.
    In every chain q / k handed to the attention kernel are strided column views of the buffer `qkv` ([S*B, 2 D] in "swap", [S*B, 3 D] otherwise; k offsets
    reach 2.77 GB of the kernel's 32-bit byte-offset budget at H = 32, B = 2 in the 3 D form; the in-place norm passes address the same range)."""
    from gen3c_amd import dit, ops
    if chain == "default":
        chain = "fused" if dit._FUSE_QKV_EPILOGUE else ("swap" if dit._v_by_operand_swap(S) else "separate")
    g = torch.Generator(device=dev).manual_seed(seed)
    Dm = H * HD
    h = torch.randn(S * B, Dm, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(3 * Dm, Dm, device=dev, generator=g) / math.sqrt(Dm)).to(torch.bfloat16)
    nq = (1.0 + 0.1 * torch.randn(HD, device=dev, generator=g)).to(torch.bfloat16)
    nk = (1.0 + 0.1 * torch.randn(HD, device=dev, generator=g)).to(torch.bfloat16)
    ang = torch.rand(S, HD // 2, device=dev, generator=g) * 6.2831853
    ang = torch.cat([ang, ang], dim=-1)
    cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    vt = torch.zeros(B, H, HD, ops.ceil_to(S, 64), device=dev, dtype=torch.bfloat16)
    if chain == "fused":
        qkv = ops.gemm_qk_norm_rope(h, w, Dm, Dm, nq, nk, cos, sin, S, B, vt=vt)
    elif chain == "swap":
        qkv = ops.gemm_nt(h, w[:2 * Dm])
        ops.qk_rmsnorm_rope_pair(qkv, nq, H, nk, H, cos, sin, S, B)
        hv = h.view(S, B, Dm)
        for b_ in range(B):
            ops.gemm_nt(w[2 * Dm:], hv[:, b_], out=vt[b_].view(Dm, -1)[:, :S])
    else:
        assert chain == "separate"
        qkv = ops.gemm_nt(h, w)
        ops.qk_rmsnorm_rope_pair(qkv[:, :2 * Dm], nq, H, nk, H, cos, sin, S, B)
        ops.transpose_v(qkv[:, 2 * Dm:], S, B, H, out=vt)
    return dict(h=h, w=w, nq=nq, nk=nk, ang=ang, qkv=qkv, vt=vt, Dm=Dm, chain=chain)


def test_bench_attention_launch_w4b_xcd_grid_vs_fp32():
    """the launch bench.py times - flash_attn_fwd_w4b_kernel<true>, 1-D XCD-local grid, S = 56 320, H = 32, B = 2,
    q / k as column views of the fused QKV buffer, V^T as the product's default QKV chain writes it - against an fp32 softmax on sampled rows.
    (batch, head) pair hb = b*H + h is worked on by XCD hb % 8 (attention_w4b.hpp): the 8 checked pairs cover all 8 XCDs, both batch
    items, the first and the last head. 256 sampled rows per pair: the first / last row block (prologue and ragged tail paths) + random ones."""
    from gen3c_amd import _lib, ops
    dev = torch.device("cuda:0")
    H, B = 32, 2
    name = _lib.load().g3_flash_attn_kernel_name(S, S, B, H).decode()
    assert name == "flash_attn_fwd_w4b_kernel<true>", f"the automatic choice for the benchmark shape is {name}"
    op = _bench_launch_operands(dev, H, B)
    Dm, qkv, vt = op["Dm"], op["qkv"], op["vt"]
    q, k = qkv[:, :Dm], qkv[:, Dm:2 * Dm]
    assert q.stride(0) == qkv.shape[1] and qkv.shape[1] in (2 * Dm, 3 * Dm) and k.data_ptr() - qkv.data_ptr() == 2 * Dm  # strided views, nothing repacked
    ops.enable_kernel_timers(True)
    out = ops.flash_attn(q, k, vt, S, S, B, H)
    launched = [m for (n, m, _t) in ops.collected_kernel_timers() if n == "flash_attn_fwd"]
    ops.enable_kernel_timers(False)
    assert launched and launched[-1]["kernel"] == "flash_attn_fwd_w4b_kernel<true>", launched
    assert torch.isfinite(out.float()).all()
    g = torch.Generator(device=dev).manual_seed(3)
    rows = torch.cat([torch.arange(0, 64, device=dev), torch.randint(64, S - 64, (128,), device=dev, generator=g), torch.arange(S - 64, S, device=dev)])
    worst = 0.0
    for (b, hh) in [(0, 0), (0, 9), (0, 18), (0, 27), (1, 4), (1, 13), (1, 22), (1, 31)]:
        assert (b * H + hh) % 8 == [(0, 0), (0, 9), (0, 18), (0, 27), (1, 4), (1, 13), (1, 22), (1, 31)].index((b, hh))
        sl = slice(hh * HD, (hh + 1) * HD)
        qs = q[rows * B + b][:, sl].float()
        ks = k[b::B][:, sl].float()
        vs = vt[b, hh, :, :S].float().t()
        ref = torch.softmax((qs @ ks.t()) / math.sqrt(HD), dim=-1) @ vs
        r = _rel_l2(out[rows * B + b][:, sl], ref)
        worst = max(worst, r)
        assert r < 4e-3, f"(b={b}, h={hh}): rel-L2 {r:.3e} vs fp32 softmax on 256 sampled rows"
    print(f"[bench attention launch w4b<true> S=56320 H=32 B=2] worst rel-L2 over 8 (batch, head) pairs = {worst:.3e}")


@pytest.mark.parametrize("chain", ["separate", "fused", "swap"])
def test_bench_qkv_epilogue_vs_fp32_norm_rope(chain):
    """The three forms of the QKV chain at the benchmark size (S = 56 320, B = 2, D = 4096) - "swap" = what the DiT forward runs by default (q | k
    projection + one in-place norm + RoPE pass, V by two operand-swapped GEMMs at N = 56 320, ldw = B D), "separate" = plain projection, in-place norm +
    RoPE passes over 2.77 GB of strided views, V transpose, "fused" = the opt-in epilogue - against an fp32 evaluation of Attention.cal_qkv
    (attention.py:247-280: Linear, per-head RMSNorm with weight, non-interleaved RoPE; v plain) on sampled rows, and against each other ("swap" is
    bitwise "separate"; "fused" has the same rounding points with the sum of squares accumulated in another order)."""
    from oracle import dit_oracle
    dev = torch.device("cuda:0")
    H, B = 32, 2
    op = _bench_launch_operands(dev, H, B, seed=12, chain=chain)
    Dm, qkv, vt = op["Dm"], op["qkv"], op["vt"]
    g = torch.Generator(device=dev).manual_seed(5)
    srow = torch.cat([torch.arange(0, 16, device=dev), torch.randint(16, S - 16, (96,), device=dev, generator=g), torch.arange(S - 16, S, device=dev)])  # tokens
    for b in range(B):
        rows = srow * B + b
        y = op["h"][rows].float() @ op["w"].float().t()  # [n, 3 Dm] fp32
        fr = op["ang"][srow].reshape(-1, 1, 1, HD)
        for name, c0, nw in (("q", 0, op["nq"]), ("k", Dm, op["nk"])):
            t = y[:, c0:c0 + Dm].reshape(-1, 1, H, HD)
            ref = dit_oracle.te_rope_fused(dit_oracle.te_rmsnorm(t, nw.float()), fr).reshape(-1, Dm)
            r = _rel_l2(qkv[rows][:, c0:c0 + Dm], ref)
            # three bf16 roundings on the kernel's path (projection, norm, rope - TE's rounding points) vs none in the reference
            assert r < 6e-3, f"{name} (b={b}): rel-L2 {r:.3e} vs fp32 RMSNorm + RoPE"
        vref = y[:, 2 * Dm:].reshape(-1, H, HD)
        vgot = vt[b][:, :, srow].permute(2, 0, 1)
        r = _rel_l2(vgot, vref)
        assert r < 4e-3, f"v^T (b={b}): rel-L2 {r:.3e}"
    if vt.shape[-1] > S:
        assert float(vt[:, :, :, S:].float().abs().max()) == 0.0  # the zero tail the attention kernel relies on
    if chain == "fused":
        # the two chains share every rounding point; what differs is the fp32 summation order of a head's 128 squares (tests/test_kernels_gpu.py), so
        # V^T is bitwise equal and q | k agree up to an occasional 1-ulp bf16 flip
        other = _bench_launch_operands(dev, H, B, seed=12, chain="separate")
        assert torch.equal(other["vt"], vt)
        r = _rel_l2(other["qkv"][:, :2 * Dm], qkv[:, :2 * Dm])
        assert r < 1e-3, f"fused vs separate chain: rel-L2 {r:.3e}"
    if chain == "swap":
        # same products in the same K order per element, the same norm + RoPE kernel on the same q | k values: V^T (its zero tail included) and q | k are
        # the transpose chain's bits ("bitwise")
        other = _bench_launch_operands(dev, H, B, seed=12, chain="separate")
        assert torch.equal(vt, other["vt"]), "V^T of the operand-swap chain differs from the GEMM + transpose chain's"
        assert qkv.shape == (S * B, 2 * Dm) and torch.equal(qkv, other["qkv"][:, :2 * Dm])


def test_dit_full_size_single_block_vs_fp32_oracle():
    """The WHOLE forward composition at BASELINE.json's size - latent [1,16,16,88,160] = 56 320 tokens, D = 4096, 32 heads, context 512 x 1024,
    patch embedding -> one of the 28 blocks (self-attention on the one-wave kernel over all 56 320 keys, cross-attention, 16 384-wide MLP, AdaLN-LoRA,
    absolute + rotary position embeddings for the full 16 x 44 x 80 grid) -> final layer -> unpatchify - against oracle/dit_oracle.py evaluated in
    fp32 on the same device (the oracle is plain torch; on the host this size would take ~10 minutes per block). Every other test at this size
    checks single kernels on sampled rows; this one checks that what they add up to is the reference's network. Measured rel-L2 5.87e-3 (the 4 096-token
    full-width block: 6.0e-3)."""
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from oracle import dit_oracle
    dev = torch.device("cuda:0")
    net = VideoExtendGeneralDIT(in_channels=81, rope_t_extrapolation_ratio=2.0, num_blocks=1, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=17)
    B, T, H, W, M = 1, 16, 88, 160, 512
    g = torch.Generator(device=dev).manual_seed(23)
    rnd = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    x = rnd(B, 16, T, H, W).to(torch.bfloat16)
    mask = torch.zeros(B, 1, T, H, W, dtype=torch.bfloat16, device=dev)
    mask[:, :, :1] = 1
    pose = (0.5 * rnd(B, 64, T, H, W)).to(torch.bfloat16)
    ctx = (0.2 * rnd(B, M, 1024)).to(torch.bfloat16)
    ctx[:, 64:] = 0
    ts = torch.tensor([0.3], dtype=torch.bfloat16, device=dev)
    pad = torch.zeros(B, 1, 8 * H, 8 * W, dtype=torch.bfloat16, device=dev)
    fps = torch.tensor([24.0], device=dev)
    y = net(x=x, timesteps=ts, crossattn_emb=ctx, crossattn_mask=None, fps=fps, padding_mask=pad, condition_video_indicator=mask[:, :, :, :1, :1],
            condition_video_input_mask=mask, condition_video_pose=pose)
    torch.cuda.synchronize()
    assert y.shape == (B, 16, T, H, W) and torch.isfinite(y.float()).all()
    sd = {k: v.detach().float() for k, v in net.state_dict().items()}
    with torch.no_grad():
        y_ref = dit_oracle.dit_forward(sd, x.float(), ts.float(), ctx.float(), mask.float(), pose.float(), pad.float(), fps, num_blocks=1, num_heads=32)
    rel = _rel_l2(y, y_ref)
    mx = float((y.float() - y_ref).abs().max())
    print(f"[dit D=4096 H=32, 1 block, 56320 tokens (full size)] rel_l2={rel:.3e} max_abs={mx:.3e} ref_absmax={float(y_ref.abs().max()):.3e}")
    assert rel <= 9e-3 and mx <= 1.5e-2 * float(y_ref.abs().max())  # measured 5.87e-3 / 6.7e-3 of max|y|


def _oracle_conv_impl(dev):
    """The vendor's fp32 conv3d may fall back to a naive kernel at these sizes: probe one 256 -> 256 (1,3,3) convolution on a
    31 x 176 x 320 tensor and switch the oracle to its per-tap matmul form (equal to F.conv3d: tests/test_tokenizer_oracle_golden.py) if slow."""
    import time
    x = torch.randn(1, 256, 31, 176, 320, device=dev)
    w = torch.randn(256, 256, 1, 3, 3, device=dev) * 0.02
    try:
        torch.nn.functional.conv3d(x[:, :, :2], w)  # (first call: kernel selection / compilation)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.nn.functional.conv3d(x, w)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    except RuntimeError:
        dt = float("inf")
    return ("torch" if dt < 2.0 else "taps"), dt


def test_tokenizer_full_clip_vs_fp32_oracle():
    """the ONE tokenizer configuration bench.py times - channels = 128 (256 / 512-wide levels), one 121 x 704 x 1280 clip, encode and
    decode (tokenizer/modules/layers3d.py:669-949, diffusion/module/pretrained_vae.py:342-359) - against oracle/tokenizer_oracle.py evaluated in
    fp32 on the same device (the oracle is plain torch). At this size the 512-channel activations are 1.79 GB (byte offsets within 17 % of 2^31), the
    spatial attention's 16 frames alternate over two streams with per-stream 14 080 x 14 080 score buffers, GroupNorm statistics arrive from the
    producing convolutions' epilogues through fp64 atomics and the causal temporal attention sees all 16 latent frames. The error is reported PER
    LATENT FRAME (and, for the reconstruction, per group of 8 pixel frames) so that a fault in the temporal chain cannot hide in the mean."""
    from gen3c_amd.tokenizer import CausalVideoTokenizerNet
    from oracle import tokenizer_oracle as tok
    dev = torch.device("cuda:0")
    net = CausalVideoTokenizerNet(channels=128, device=dev)
    sd = net.init_random(seed=3)
    sd32 = {k: v.to(torch.bfloat16).float().to(dev) for k, v in sd.items()}
    import bench
    x = bench.tokenizer_bench_clip(dev)
    z = net.encoder(x)
    torch.cuda.synchronize()
    assert z.shape == (1, 16, 16, 88, 160) and torch.isfinite(z.float()).all()
    z2 = net.encoder(x)  # a second pass through the cached streams / buffers: same input, same latent (up to the order of the fp64 statistics atomics)
    torch.cuda.synchronize()
    rr = _rel_l2(z2, z)
    assert rr < 1e-3, f"two encodes of the same clip differ by rel-L2 {rr:.3e}"
    impl, probe_s = _oracle_conv_impl(dev)
    tok.CONV_IMPL = impl
    try:
        with torch.no_grad():
            z_ref = tok.encoder(sd32, x.float())
            zin = z_ref.to(torch.bfloat16)
            y_ref = tok.decoder(sd32, zin.float())
    finally:
        tok.CONV_IMPL = "torch"
    y = net.decoder(zin)
    torch.cuda.synchronize()
    assert y.shape == (1, 3, 121, 704, 1280) and torch.isfinite(y.float()).all()
    rz, ry = _rel_l2(z, z_ref), _rel_l2(y, y_ref)
    per_z = [_rel_l2(z[:, :, t], z_ref[:, :, t]) for t in range(16)]
    groups = [slice(0, 1)] + [slice(1 + 8 * i, 9 + 8 * i) for i in range(15)]
    per_y = [_rel_l2(y[:, :, s_], y_ref[:, :, s_]) for s_ in groups]
    print(f"[tokenizer ch128 121x704x1280 (bench size), oracle conv = {impl} ({probe_s:.2f}s probe)] encoder rel_l2={rz:.3e} decoder rel_l2={ry:.3e} re-encode={rr:.1e}")
    print("  per latent frame, encoder: " + " ".join(f"{v:.2e}" for v in per_z))
    print("  per latent frame, decoder: " + " ".join(f"{v:.2e}" for v in per_y))
    if os.environ.get("G3_WRITE_FULLSIZE_FIXTURE"):  # samples of the oracle's outputs for bench.py's parity entry (copied to tests/golden/ by hand)
        import numpy as np
        with torch.no_grad():  # bench.py decodes ITS OWN latent: commit the oracle's reconstruction of the oracle's latent (what the product should approach)
            out = Path(os.environ["G3_WRITE_FULLSIZE_FIXTURE"])
            out.parent.mkdir(parents=True, exist_ok=True)
            np.savez(out, z_ref=z_ref.reshape(-1)[bench.tokenizer_sample_index(z_ref.numel()).to(dev)].cpu().numpy(),
                     y_ref=y_ref.reshape(-1)[bench.tokenizer_sample_index(y_ref.numel()).to(dev)].cpu().numpy())
    assert rz <= 1.5e-2 and ry <= 1.8e-2  # 17x352x640 / 9x704x1280 clips measure 7.0e-3 / 9.2e-3
    assert max(per_z) <= 2.5e-2 and max(per_y) <= 3.0e-2, "one latent frame is off: temporal chain / stream hand-off"
