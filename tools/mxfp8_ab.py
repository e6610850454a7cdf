"""A/B of the opt-in MXFP8 and MXFP6 DiT linears against the bf16 product path, in one process (measuring rules: all arms warmed up, then alternated).

    python tools/mxfp8_ab.py --classes [--out FILE]   the six per-block linears at M = 112 640 (bench, B = 2) and 14 080 (cp = 8 rank), launch
                                                     by launch: bf16 product GEMM (g3_gemm_bf16_nt) vs g3_gemm_mxfp8_nt vs g3_gemm_mxfp6_nt, and the
                                                     quantisation pass of each class's activations (time and counted bytes: 2 B read + 1 B + 1/32 B
                                                     written for MXFP8, 2 B read + 0.75 B + 1/32 B written for MXFP6)
    python tools/mxfp8_ab.py --quant-only             only the quantisation passes (for a `rocprofv3 --kernel-trace --stats` run of its own)
    python tools/mxfp8_ab.py --step [--steps N]       the full 28-block denoise step at the bench workload (net built as bench.py builds it: latent
                                                     16 x 88 x 160, dense 512-token context), linear_precision bf16 vs mxfp8 vs mxfp6, all warmed up,
                                                     then alternating; steps/s of each arm
    python tools/mxfp8_ab.py --accum                  the scaled MFMA's accumulation error: the fa_qkv GEMM at M = 14 080 against the exact fp64
                                                     sum of the dequantised operands on sampled outputs, next to the bf16 GEMM on the same values
                                                     (an MXFP8 arm and an MXFP6 arm)
    python tools/mxfp8_ab.py --producers [--steps N]  mxfp8_producers "separate" vs "fused" (default FILE profiles/r8_mxfp8_producers_ab.txt): launch by launch at
                                                     M = 112 640 and 14 080 - LayerNorm + quantiser vs the LayerNorm that emits MXFP8, plain and with the position
                                                     embedding, and the w1 GELU GEMM + quantiser vs w1 with MXFP8 output - then the full mxfp8 step with either
                                                     setting (torch.equal of the two arms' x_t asserted after 2 steps; the kernel timers confirm which launches ran)
Results are appended to FILE (default profiles/r9_mxfp6_ab.txt; profiles/r7_mxfp8_ab.txt is the record of the two-arm form of this tool)."""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from gen3c_amd import ops  # noqa: E402
from tools.microbench import timeit  # noqa: E402

D = 4096
CLASSES = [("fa_qkv", 3 * D, D, 0), ("fa_out", D, D, 2), ("ca_q", D, D, 0), ("ca_out", D, D, 2), ("w1", 4 * D, D, 1), ("w2", D, 4 * D, 2)]


def _log(out, line):
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def classes(out, quant_only=False, rounds=3, iters=5):
    dev = torch.device("cuda:0")
    if not quant_only:
        _log(out, f"== per-class GEMM A/B ({torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M')}): bf16 product kernel vs MXFP8 vs MXFP6, "
                  f"{rounds} alternating rounds x {iters} launches, TF = 2MNK / time")
    for M in (112640, 14080):
        for name, N, K, epi in CLASSES:
            torch.manual_seed(M + N + K)
            a = torch.randn(M, K, device=dev).to(torch.bfloat16)
            w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
            aq, as_ = ops.quant_mxfp8(a)
            wq, ws = ops.quant_mxfp8(w)
            a6, as6 = ops.quant_mxfp6(a)
            w6, ws6 = ops.quant_mxfp6(w)
            qbytes = M * K * (2 + 1 + 1 / 32)
            qbytes6 = M * K * (2 + 0.75 + 1 / 32)
            q8 = lambda: ops.quant_mxfp8(a, out=(aq, as_))  # noqa: E731
            q6 = lambda: ops.quant_mxfp6(a, out=(a6, as6))  # noqa: E731
            tq8, tq6 = [], []
            for _ in range(rounds):
                tq8.append(timeit(q8, iters))
                tq6.append(timeit(q6, iters))
            qms, qms6 = min(tq8), min(tq6)
            if quant_only:
                _log(out, f"quant {name:7s} M={M:6d} K={K:5d}: {qms:.3f} ms {qbytes / qms / 1e9:5.2f} TB/s (event-timed inside a rocprofv3 --kernel-trace --stats run)")
                _log(out, f"quant6 {name:6s} M={M:6d} K={K:5d}: {qms6:.3f} ms {qbytes6 / qms6 / 1e9:5.2f} TB/s")
                continue
            gate = (torch.rand(2, N, device=dev) + 0.1).to(torch.bfloat16)
            res = torch.randn(M, N, device=dev).to(torch.bfloat16)
            c = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            kw = dict(gate=gate, residual=res) if epi == 2 else {}
            bf = lambda: ops.gemm_nt(a, w, out=c, epilogue=epi, **kw)  # noqa: E731
            mx = lambda: ops.gemm_mxfp8_nt(aq, as_, wq, ws, out=c, epilogue=epi, **kw)  # noqa: E731
            m6 = lambda: ops.gemm_mxfp6_nt(a6, as6, w6, ws6, out=c, epilogue=epi, **kw)  # noqa: E731
            bf(), mx(), m6()
            t_bf, t_mx, t_m6 = [], [], []
            for _ in range(rounds):
                t_bf.append(timeit(bf, iters))
                t_mx.append(timeit(mx, iters))
                t_m6.append(timeit(m6, iters))
            fl = 2.0 * M * N * K
            b, m = min(t_bf), min(t_mx)
            _log(out, f"{name:7s} M={M:6d} N={N:5d} K={K:5d} epi={epi}: bf16 {b:7.3f} ms {fl / b / 1e9:6.0f} TF | mxfp8 {m:7.3f} ms "
                      f"{fl / m / 1e9:6.0f} TF | speed-up {b / m:5.3f}x (rounds bf16 {' '.join(f'{t:.3f}' for t in t_bf)}, "
                      f"mxfp8 {' '.join(f'{t:.3f}' for t in t_mx)}) | quant A {qms:6.3f} ms {qbytes / qms / 1e9:5.2f} TB/s")
            s6 = min(t_m6)
            wins = sum(t6 < t8 for t6, t8 in zip(t_m6, t_mx))
            _log(out, f"{'':7s} {'':43s} mxfp6 {s6:7.3f} ms {fl / s6 / 1e9:6.0f} TF | vs bf16 {b / s6:5.3f}x, vs mxfp8 {m / s6:5.3f}x, faster than mxfp8 in "
                      f"{wins} of {rounds} rounds (rounds mxfp6 {' '.join(f'{t:.3f}' for t in t_m6)}) | quant A {qms6:6.3f} ms "
                      f"{qbytes6 / qms6 / 1e9:5.2f} TB/s | GEMM + quant: mxfp8 {m + qms:7.3f} ms, mxfp6 {s6 + qms6:7.3f} ms")
            del a, w, aq, as_, wq, ws, a6, as6, w6, ws6, gate, res, c
            torch.cuda.empty_cache()


def step(out, steps=3, rounds=3):
    import numpy as np
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
    dev = torch.device("cuda:0")
    net = VideoExtendGeneralDIT(in_channels=16 + 16 * 4 + 1, rope_t_extrapolation_ratio=2.0, num_blocks=28, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=1234)
    net.cross_attention_skip_zero_context = False
    T, Hl, Wl, B = 16, 88, 160, 1
    rs = np.random.RandomState(1)
    normal = lambda shape, std: torch.from_numpy((rs.standard_normal(shape) * std).astype(np.float32)).to(torch.bfloat16).to(dev)  # noqa: E731
    den = Gen3CDenoiser(net, state_shape=(16, T, Hl, Wl))
    den.scheduler.set_timesteps(35)
    xt = normal((B, 16, T, Hl, Wl), den.scheduler.init_noise_sigma)
    gt, pose = normal((B, 16, T, Hl, Wl), 0.5), normal((B, 64, T, Hl, Wl), 0.5)
    ctx = normal((B, 512, 1024), 0.2)
    ctx[:, 64:] = 0
    pad = torch.zeros(B, 1, 8 * Hl, 8 * Wl, device=dev, dtype=torch.bfloat16)
    fps = torch.tensor([24.0], device=dev)

    def make_cond(p):
        c = VideoExtendCondition(crossattn_emb=ctx, crossattn_mask=None, padding_mask=pad, fps=fps, video_cond_bool=True, condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

    cond, uncond = make_cond(pose), make_cond(torch.zeros_like(pose))

    def run(prec):
        net.set_linear_precision(prec)
        tm = ops.HipTimer()
        x = xt
        tm.start()
        for i in range(steps):
            x = den.denoise_step(x, i, cond, uncond, 1.0, 0.001, 1)
        tm.stop()
        torch.cuda.synchronize()
        return tm.elapsed_ms() / steps, x

    arms = ("bf16", "mxfp8", "mxfp6")
    for prec in arms:  # warm-up of every arm (weight quantisation, tables, context K / V)
        run(prec)
    res = {prec: [] for prec in arms}
    outs = {}
    for _ in range(rounds):
        for prec in arms:
            ms, outs[prec] = run(prec)
            res[prec].append(ms)
    b, m = min(res["bf16"]), min(res["mxfp8"])
    rel = float((outs["mxfp8"].float() - outs["bf16"].float()).norm() / outs["bf16"].float().norm())
    _log(out, f"== full denoise step A/B ({torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M')}): 28 blocks, latent {T}x{Hl}x{Wl}, "
              f"B = 1 (CFG branches batched: M = 112 640), dense context, {rounds} alternating rounds x {steps} steps after warm-up of all arms")
    _log(out, f"bf16  {b:8.1f} ms/step  {1000 / b:.4f} steps/s  (rounds {' '.join(f'{t:.1f}' for t in res['bf16'])})")
    _log(out, f"mxfp8 {m:8.1f} ms/step  {1000 / m:.4f} steps/s  (rounds {' '.join(f'{t:.1f}' for t in res['mxfp8'])})  "
              f"steps/s {100 * (b / m - 1):+.1f} %, quantisation passes included; rel-L2 of the mxfp8 x_t after {steps} steps vs bf16 {rel:.3e}")
    s6 = min(res["mxfp6"])
    rel6 = float((outs["mxfp6"].float() - outs["bf16"].float()).norm() / outs["bf16"].float().norm())
    wins = sum(t6 < t8 for t6, t8 in zip(res["mxfp6"], res["mxfp8"]))
    _log(out, f"mxfp6 {s6:8.1f} ms/step  {1000 / s6:.4f} steps/s  (rounds {' '.join(f'{t:.1f}' for t in res['mxfp6'])})  "
              f"steps/s {100 * (b / s6 - 1):+.1f} % vs bf16, {100 * (m / s6 - 1):+.1f} % vs mxfp8 (faster than mxfp8 in {wins} of {rounds} rounds), quantisation "
              f"passes included; rel-L2 of the mxfp6 x_t after {steps} steps vs bf16 {rel6:.3e}")


def _bench_step_setup(dev):
    """The bench workload of step(): the 28-block net as bench.py builds it and one denoise step's inputs."""
    import numpy as np
    from gen3c_amd.dit import VideoExtendGeneralDIT
    from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask
    net = VideoExtendGeneralDIT(in_channels=16 + 16 * 4 + 1, rope_t_extrapolation_ratio=2.0, num_blocks=28, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=1234)
    net.cross_attention_skip_zero_context = False
    T, Hl, Wl, B = 16, 88, 160, 1
    rs = np.random.RandomState(1)
    normal = lambda shape, std: torch.from_numpy((rs.standard_normal(shape) * std).astype(np.float32)).to(torch.bfloat16).to(dev)  # noqa: E731
    den = Gen3CDenoiser(net, state_shape=(16, T, Hl, Wl))
    den.scheduler.set_timesteps(35)
    xt = normal((B, 16, T, Hl, Wl), den.scheduler.init_noise_sigma)
    gt, pose = normal((B, 16, T, Hl, Wl), 0.5), normal((B, 64, T, Hl, Wl), 0.5)
    ctx = normal((B, 512, 1024), 0.2)
    ctx[:, 64:] = 0
    pad = torch.zeros(B, 1, 8 * Hl, 8 * Wl, device=dev, dtype=torch.bfloat16)
    fps = torch.tensor([24.0], device=dev)

    def make_cond(p):
        c = VideoExtendCondition(crossattn_emb=ctx, crossattn_mask=None, padding_mask=pad, fps=fps, video_cond_bool=True, condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

    return net, den, xt, make_cond(pose), make_cond(torch.zeros_like(pose))


def producers(out, steps=3, rounds=3, iters=5):
    """mxfp8_producers "separate" vs "fused": the four fused hand-overs launch by launch, then the step."""
    dev = torch.device("cuda:0")
    _log(out, f"== MXFP8 producers A/B ({torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M')}): separate = bf16 producer + g3_quant_mxfp8_bf16, "
              f"fused = the producer emits MXFP8; both warmed, {rounds} alternating rounds x {iters} launches, min of rounds (all rounds listed)")
    fmt = lambda ts: " ".join(f"{t:.3f}" for t in ts)  # noqa: E731

    def ab(label, sep, fused):
        sep(), fused()
        t_s, t_f = [], []
        for _ in range(rounds):
            t_s.append(timeit(sep, iters))
            t_f.append(timeit(fused, iters))
        s_, f_ = min(t_s), min(t_f)
        _log(out, f"{label}: separate {s_:7.3f} ms | fused {f_:7.3f} ms | saved {s_ - f_:6.3f} ms ({s_ / f_:5.3f}x) (rounds separate {fmt(t_s)}, fused {fmt(t_f)})")

    for M in (112640, 14080):
        B = 2
        Tp, Hp, Wp = (16, 44, 80) if M == 112640 else (2, 44, 80)
        assert Tp * Hp * Wp * B == M
        torch.manual_seed(M)
        x = torch.randn(M, D, device=dev).to(torch.bfloat16)
        shift = (0.5 * torch.randn(B, D, device=dev)).to(torch.bfloat16)
        scale = (0.5 * torch.randn(B, D, device=dev)).to(torch.bfloat16)
        pe = (0.3 * torch.randn(M // B, D, device=dev)).to(torch.bfloat16)
        h = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
        pair = (torch.empty(M, D, device=dev, dtype=torch.float8_e4m3fn), torch.empty(M, D // 32, device=dev, dtype=torch.uint8))
        ab(f"LayerNorm + modulate        M={M:6d} D={D}",
           lambda: ops.quant_mxfp8(ops.layernorm_modulate(x, shift, scale, out=h), out=pair),
           lambda: ops.layernorm_modulate_mxfp8(x, shift, scale, out=pair))
        # the position-embedding form updates x in place: a zero table keeps x (and the work per launch) the same over the repetitions
        pe.zero_()
        ab(f"posemb LayerNorm + modulate M={M:6d} D={D}",
           lambda: ops.quant_mxfp8(ops.posemb_layernorm_modulate(x, pe, None, None, None, Tp, Hp, Wp, B, shift, scale, out=h), out=pair),
           lambda: ops.posemb_layernorm_modulate_mxfp8(x, pe, None, None, None, Tp, Hp, Wp, B, shift, scale, out=pair))
        del h, pe
        aq, as_ = ops.quant_mxfp8(x)
        wq, ws = ops.quant_mxfp8((torch.randn(4 * D, D, device=dev) * 0.02).to(torch.bfloat16))
        u = torch.empty(M, 4 * D, device=dev, dtype=torch.bfloat16)
        upair = (torch.empty(M, 4 * D, device=dev, dtype=torch.float8_e4m3fn), torch.empty(M, 4 * D // 32, device=dev, dtype=torch.uint8))
        ab(f"w1 (GELU) -> MXFP8          M={M:6d} N={4 * D} K={D}",
           lambda: ops.quant_mxfp8(ops.gemm_mxfp8_nt(aq, as_, wq, ws, out=u, epilogue=ops.EPI_GELU), out=upair),
           lambda: ops.gemm_mxfp8_nt(aq, as_, wq, ws, epilogue=ops.EPI_GELU, out_mx=upair))
        t_plain = min(timeit(lambda: ops.gemm_mxfp8_nt(aq, as_, wq, ws, out=u, epilogue=ops.EPI_GELU), iters) for _ in range(rounds))
        t_mxo = min(timeit(lambda: ops.gemm_mxfp8_nt(aq, as_, wq, ws, epilogue=ops.EPI_GELU, out_mx=upair), iters) for _ in range(rounds))
        fl = 2.0 * M * 4 * D * D
        _log(out, f"   the w1 GEMM alone            M={M:6d}: bf16 output {t_plain:7.3f} ms {fl / t_plain / 1e9:6.0f} TF | MXFP8 output {t_mxo:7.3f} ms "
                  f"{fl / t_mxo / 1e9:6.0f} TF (the in-epilogue quantisation costs {t_mxo - t_plain:+.3f} ms against the bf16 store)")
        del x, u, upair, aq, as_, wq, ws, pair
        torch.cuda.empty_cache()

    net, den, xt, cond, uncond = _bench_step_setup(dev)
    net.set_linear_precision("mxfp8")

    def run(arm, n):
        net.set_mxfp8_producers(arm)
        tm = ops.HipTimer()
        x = xt
        tm.start()
        for i in range(n):
            x = den.denoise_step(x, i, cond, uncond, 1.0, 0.001, 1)
        tm.stop()
        torch.cuda.synchronize()
        return tm.elapsed_ms() / n, x

    arms = ("separate", "fused")
    two = {arm: run(arm, 2)[1] for arm in arms}  # warm-up of both arms, and the equality check
    same = torch.equal(two["separate"], two["fused"])
    _log(out, f"== full mxfp8 denoise step, mxfp8_producers separate vs fused: 28 blocks, latent 16x88x160, B = 1 (CFG branches batched: M = 112 640), dense "
              f"context; x_t after 2 steps torch.equal between the arms: {same}")
    assert same, "mxfp8_producers='fused' changed x_t"
    del two
    # which launches each arm runs, from the kernel timers of one step (the separate arm must be the parent commit's launch list: no *_mxout entry)
    for arm in arms:
        ops.enable_kernel_timers(True)
        run(arm, 1)
        names = [n for n, _, _ in ops.collected_kernel_timers()]
        ops.enable_kernel_timers(False)
        _log(out, f"kernel timers, one step, {arm:8s}: " + ", ".join(f"{names.count(n)} x {n}" for n in sorted(set(names))))
    res = {arm: [] for arm in arms}
    for _ in range(rounds):
        for arm in arms:
            res[arm].append(run(arm, steps)[0])
    s_, f_ = min(res["separate"]), min(res["fused"])
    spread = lambda ts: 100 * (max(ts) - min(ts)) / min(ts)  # noqa: E731
    _log(out, f"separate {s_:8.1f} ms/step  {1000 / s_:.4f} steps/s  (rounds {' '.join(f'{t:.1f}' for t in res['separate'])}; spread {spread(res['separate']):.2f} %)")
    _log(out, f"fused    {f_:8.1f} ms/step  {1000 / f_:.4f} steps/s  (rounds {' '.join(f'{t:.1f}' for t in res['fused'])}; spread {spread(res['fused']):.2f} %)  "
              f"fused / separate steps/s {s_ / f_:.4f} ({100 * (s_ / f_ - 1):+.2f} %; derived expectation +2 to +2.5 %), {rounds} alternating rounds x {steps} steps")


def accum(out):
    dev = torch.device("cuda:0")
    M, N, K = 14080, 3 * D, D
    torch.manual_seed(0)
    a = torch.randn(M, K, device=dev).to(torch.bfloat16)
    a[:, 5::613] *= 30
    w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
    aq, as_ = ops.quant_mxfp8(a)
    wq, ws = ops.quant_mxfp8(w)
    deq = lambda q, s_: (q.float().view(q.shape[0], -1, 32) * torch.exp2(s_.float() - 127).unsqueeze(-1)).view(q.shape)  # noqa: E731
    ad, wd = deq(aq, as_), deq(wq, ws)
    rows = torch.randint(0, M, (512,), device=dev)
    # both GEMMs round to bf16: each is measured against the exact fp64 sum, in ulps of it and relative to sum |a w|
    ex = ad[rows].double() @ wd.double().T
    s_abs = ad[rows].abs().double() @ wd.abs().double().T
    mx = ops.gemm_mxfp8_nt(aq[rows].contiguous(), as_[rows].contiguous(), wq, ws).double()
    bf = ops.gemm_nt(ad[rows].to(torch.bfloat16).contiguous(), wd.to(torch.bfloat16)).double()
    ulp = torch.exp2(torch.floor(torch.log2(ex.abs().clamp_min(2.0 ** -126))) - 7)
    rnd = ex.float().to(torch.bfloat16).double()  # the correctly rounded result
    _log(out, f"== scaled-MFMA accumulation probe ({torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M')}): fa_qkv operands "
              f"(N(0,1) activations with 30x outlier channels, N(0, 0.02) weights), {rows.numel()} sampled rows x {N} columns, K = {K}")
    for name, y in (("mxfp8 GEMM", mx), ("bf16 GEMM on dequantised operands", bf)):
        err = (y - ex).abs()
        _log(out, f"{name:34s}: correctly rounded {float((y == rnd).double().mean()):.5f}, |err| / ulp(exact) max {float((err / ulp).max()):.3f}, "
                  f"|err| / sum|a w| max {float((err / s_abs).max()):.3e} (2^{float(torch.log2((err / s_abs).max())):.1f})")
    del aq, as_, wq, ws, ad, wd, ex, s_abs, mx, bf
    accum6(out, a, w, rows)


def _dequant6(q, s_):
    """Exact fp32 values of a packed MXFP6 matrix (gen3c_amd.ops.quant_mxfp6's layout: element i of a 24-byte block at bits [6 i, 6 i + 6))."""
    M, B = q.shape
    b = q.view(M, B // 3, 3).to(torch.int32)
    v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    c = torch.stack([(v >> (6 * i)) & 63 for i in range(4)], dim=-1).view(M, -1, 32)
    e, m = (c >> 3) & 3, (c & 7).float()
    mag = torch.where(e == 0, m / 8, torch.exp2((e - 1).float()) * (1 + m / 8))
    val = torch.where((c & 32) != 0, -mag, mag)
    return (val * torch.exp2(s_.float() - 127).unsqueeze(-1)).view(M, -1)


def accum6(out, a, w, rows):
    """The MXFP6 arm of accum(): the same bf16 tensors and sampled rows, quantised to MXFP6."""
    N, K = w.shape
    aq, as_ = ops.quant_mxfp6(a)
    wq, ws = ops.quant_mxfp6(w)
    ad, wd = _dequant6(aq[rows].contiguous(), as_[rows].contiguous()), _dequant6(wq, ws)
    ex = ad.double() @ wd.double().T
    s_abs = ad.abs().double() @ wd.abs().double().T
    mx = ops.gemm_mxfp6_nt(aq[rows].contiguous(), as_[rows].contiguous(), wq, ws).double()
    bf = ops.gemm_nt(ad.to(torch.bfloat16).contiguous(), wd.to(torch.bfloat16)).double()
    ulp = torch.exp2(torch.floor(torch.log2(ex.abs().clamp_min(2.0 ** -126))) - 7)
    rnd = ex.float().to(torch.bfloat16).double()
    _log(out, f"== scaled-MFMA accumulation probe, MXFP6 e2m3 operands ({torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M')}): fa_qkv operands, "
              f"{rows.numel()} sampled rows x {N} columns, K = {K}")
    for name, y in (("mxfp6 GEMM", mx), ("bf16 GEMM on dequantised operands", bf)):
        err = (y - ex).abs()
        _log(out, f"{name:34s}: correctly rounded {float((y == rnd).double().mean()):.5f}, |err| / ulp(exact) max {float((err / ulp).max()):.3f}, "
                  f"|err| / sum|a w| max {float((err / s_abs).max()):.3e} (2^{float(torch.log2((err / s_abs).max())):.1f})")
    _log(out, f"share of outputs bitwise equal between the mxfp6 GEMM and the bf16 GEMM on the same values: {float((mx == bf).double().mean()):.5f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", action="store_true")
    ap.add_argument("--quant-only", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--accum", action="store_true")
    ap.add_argument("--producers", action="store_true")
    ap.add_argument("--out", default=None, help="default: profiles/r9_mxfp6_ab.txt; --producers writes to profiles/r8_mxfp8_producers_ab.txt")
    args = ap.parse_args()
    out_ab = args.out or str(ROOT / "profiles" / "r9_mxfp6_ab.txt")  # the default is resolved per mode: each section keeps its own record
    out_r8 = args.out or str(ROOT / "profiles" / "r8_mxfp8_producers_ab.txt")
    if args.classes or args.quant_only:
        classes(out_ab, quant_only=args.quant_only)
    if args.accum:
        accum(out_ab)
    if args.step:
        step(out_ab, steps=args.steps)
    if args.producers:
        producers(out_r8, steps=args.steps)
