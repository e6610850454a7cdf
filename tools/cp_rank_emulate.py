"""One GPU plays ONE RANK of a context-parallel run of the full-size denoise step: the PRODUCT code path - Gen3CDenoiser.denoise_step ->
VideoExtendGeneralDIT.forward with context parallelism enabled -> parallel.ContextParallelAttention, every kernel at the per-rank shapes of cp = 1 / 2 / 4 / 8
(M = 2 x S_local rows, attention Sq = S_local against all 56 320 keys in head groups on two streams) - with the torch.distributed calls the path makes
(get_world_size / get_rank / get_backend / all_gather_into_tensor / all_to_all_single) replaced by an in-process stand-in that plays rank `--rank` of `cp` ranks: the "exchange" is a
device copy of this rank's shard into every slot of the gathered buffer on a separate stream (the bytes a real exchange would deliver into HBM; the values of the
other ranks' keys are this rank's own - irrelevant for timing). What this measures: the COMPUTE side of a rank's step with today's kernels, launch gaps included.
What it cannot: the xGMI exchange itself - the model printed at the end adds it under stated assumptions.

  python tools/cp_rank_emulate.py [--cps 1,2,4,8] [--steps 3] [--blocks 28] [--configs 4,auto,gather_first;4,w4b,gather_first;...] [--out gpurun_out/r6_cp_rank_shapes.json]

Schedules (the third field of a config): gather_first, local_first, local_carry (own-shard partial, then ONE carry launch per head group over every remote
key - no merge pass), head_parallel (heads sharded by two all-to-alls around the ordinary full-length attention; the stand-in's all-to-all is a device
copy of the same size). The exchange model below replays each of them.

  python tools/cp_rank_emulate.py --cfg 2 [--worlds 8,4,2] [--rounds 2] [--steps 2] [--configs "4,auto,local_first;4,auto,local_carry"] [--out ...]
CFG-parallel (opt-in: the two guidance branches on separate rank groups, 2 x cp ranks, each rank at B = 1) against plain context parallelism at the same
total rank count, ALTERNATING in one process: a middle rank of cp = 8 against one of cfg 2 x cp 4, cp = 4 against cfg 2 x cp 2, cp = 2 against
cfg 2 x cp 1 (no context parallelism at all). The stand-in is group-aware (the pair group has world 2, the CP group world cp); the pair's all-gather of
the network output is a device copy of the real size on the stand-in's stream. The K / V bytes received per step are asserted against
L * 2 * (S_local * B * 4096 * 2) * (cp - 1); the exchange model counts cp - 1 peers and B = 1 for the CFG-parallel arms.

  python tools/cp_rank_emulate.py --ab_bounded 3 [--cps 1,2,4,8] [--steps 2] [--configs "4,auto,local_first;4,auto,gather_first;4,auto,local_carry"] [--out ...]
  python tools/cp_rank_emulate.py --window 2,1 [--cps 8,4] [--rounds 2] [--steps 2] [--configs "4,auto,local_first"] [--out FILE]
The frame window under context parallelism (the DiT's opt-in switch; ContextParallelAttention's "window_halo") against the dense schedule, ALTERNATING in
one process: rank 0, a middle rank and the last rank of each cp through the product path. Prints per rank the step ms of both arms, the self-attention
ms per layer, the visited and dense (query block, tile) pairs and the received bytes (asserted against parallel.window_halo_plan); the step is paced by
the slowest rank, so the maximum over the ranks is the line to read. The stand-in's split-size all-to-all is a device copy of the received size.

The logit-bound switch of the key-sharding schedules (ContextParallelAttention's `bounded`) off and on, ALTERNATING in one process after both arms are warm:
per configuration `--ab_bounded` rounds of (off, on), each `--steps` untimed-by-events steps; then one step per arm with the kernel timers on for the per-class
table. The off arm is the behaviour without the switch. Then, launch by launch on one stream, the partial / carry / kvseg launches at each cp's rank shapes
(Sq = S_local, 8 heads, B = 2), max form and bounded form alternating.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gen3c_amd import _lib, ops  # noqa: E402
from gen3c_amd.dit import VideoExtendGeneralDIT  # noqa: E402
from gen3c_amd.sampler import Gen3CDenoiser, VideoExtendCondition, add_condition_video_indicator_and_video_input_mask  # noqa: E402

PEAK = 2500.0


class _Work:
    def __init__(self, ev):
        self.ev = ev

    def wait(self):
        torch.cuda.current_stream().wait_event(self.ev)
        return True


CP_GROUP, CFG_GROUP = "fake-cp-group", "fake-cfg-group"


class FakeRank:
    """Stand-in for the torch.distributed calls on the CP path: plays rank `rank` of `world`. Group-aware for CFG-parallel (`cfg_rank` 0 / 1: the
    guidance branch this rank runs): CFG_GROUP is the pair, world 2; every other group is the CP group of `world` ranks. The pair's all-gather of the
    network output is counted apart (`pair_bytes`), so `bytes` stays the K / V exchange."""

    def __init__(self, world, rank, dev, cfg_rank=None):
        self.world, self.rank, self.cfg_rank = world, rank, cfg_rank
        self.comm = torch.cuda.Stream(device=dev)
        self.bytes = 0
        self.pair_bytes = 0
        self._orig = {}

    def _size(self, group):
        return 2 if group == CFG_GROUP else self.world

    def __enter__(self):
        for name in ("get_world_size", "get_rank", "get_backend", "all_gather_into_tensor", "all_to_all_single"):
            self._orig[name] = getattr(dist, name)
        dist.get_world_size = lambda group=None: self._size(group)
        dist.get_rank = lambda group=None: self.cfg_rank if group == CFG_GROUP else self.rank
        dist.get_backend = lambda group=None: "nccl"
        dist.all_gather_into_tensor = self._all_gather
        dist.all_to_all_single = self._all_to_all
        return self

    def __exit__(self, *exc):
        for name, fn in self._orig.items():
            setattr(dist, name, fn)
        return False

    def _all_gather(self, out, inp, group=None, async_op=False):
        cur = torch.cuda.current_stream()
        self.comm.wait_stream(cur)  # the send buffer is produced on the launch stream
        world = self._size(group)
        with torch.cuda.stream(self.comm):
            out.view(world, -1).copy_(inp.reshape(1, -1).expand(world, -1))
            ev = self.comm.record_event()
        if group == CFG_GROUP:
            self.pair_bytes += (world - 1) * inp.numel() * inp.element_size()
        else:
            self.bytes += (world - 1) * inp.numel() * inp.element_size()
        w = _Work(ev)
        if not async_op:
            w.wait()
        return w


    def _all_to_all(self, out, inp, output_split_sizes=None, input_split_sizes=None, group=None, async_op=False):
        """A device copy of the same size on the stand-in's stream: 1 / world of it stays on the rank, the rest is what a real exchange would deliver.
        With split sizes (the window_halo exchange: rows along dim 0) the receive buffer is filled from the send buffer piece by piece, and what the
        other ranks' splits hold is counted."""
        cur = torch.cuda.current_stream()
        self.comm.wait_stream(cur)
        with torch.cuda.stream(self.comm):
            if output_split_sizes is None:
                out.copy_(inp)
            else:
                assert sum(output_split_sizes) == out.shape[0] and sum(input_split_sizes) == inp.shape[0] and output_split_sizes[self.rank] == input_split_sizes[self.rank]
                for off in range(0, out.shape[0], inp.shape[0]):
                    n = min(inp.shape[0], out.shape[0] - off)
                    out[off:off + n].copy_(inp[:n])
            ev = self.comm.record_event()
        if output_split_sizes is None:
            self.bytes += (self.world - 1) * (inp.numel() // self.world) * inp.element_size()
        else:
            self.bytes += (out.shape[0] - output_split_sizes[self.rank]) * (out.numel() // out.shape[0]) * out.element_size()
        w = _Work(ev)
        if not async_op:
            w.wait()
        return w


def _class_table(timers, steps, lib):
    """Kernel timers of `steps` steps -> per-class rows (GEMMs by shape and epilogue, attention launches by shape and kernel), slowest first."""
    cls = {}
    for name, meta, tm in timers:
        if name == "gemm_nt":
            key = ("gemm", meta["epilogue"], meta["M"], meta["N"], meta["K"])
            fl = 2.0 * meta["M"] * meta["N"] * meta["K"]
        elif name == "flash_attn_fwd":
            key = ("attn", meta["Sq"], meta["Skv"], meta["B"], meta["H"], meta.get("kernel", "?"))
            fl = 4.0 * meta["Sq"] * meta["Skv"] * meta["H"] * 128 * meta["B"]
        else:
            continue
        c = cls.setdefault(key, [0, 0.0, 0.0])
        c[0] += 1
        c[1] += tm.elapsed_ms()
        c[2] += fl
    table = []
    for key, (n, tms, fl) in sorted(cls.items(), key=lambda kv: -kv[1][1]):
        if tms <= 0:
            continue
        d = dict(kind=key[0], launches_per_step=n / steps, ms_per_step=round(tms / steps, 3), tflops=round(fl / tms / 1e9, 1))
        if key[0] == "gemm":
            d.update(epilogue=key[1], M=key[2], N=key[3], K=key[4], kernel=lib.g3_gemm_kernel_name(key[2], key[3], key[4], key[1]).decode(),
                     tile_rounds=round(((key[2] + 255) // 256) * ((key[3] + 255) // 256) / 256.0, 3))
        else:
            d.update(Sq=key[1], Skv=key[2], B=key[3], H=key[4], kernel=key[5])
        table.append(d)
    return table


def _step_inputs(net, dev):
    """The full-size step's denoiser and inputs (the same numbers run_cp draws) -> (den, xt_full, cond, uncond)."""
    T, Hl, Wl = 16, 88, 160
    rs = np.random.RandomState(1)
    normal = lambda shape, std: torch.from_numpy((rs.standard_normal(shape) * std).astype(np.float32)).to(torch.bfloat16).to(dev)
    den = Gen3CDenoiser(net, state_shape=(16, T, Hl, Wl))
    den.scheduler.set_timesteps(35)
    xt_full = normal((1, 16, T, Hl, Wl), den.scheduler.init_noise_sigma)
    gt, pose, ctx = normal((1, 16, T, Hl, Wl), 0.5), normal((1, 64, T, Hl, Wl), 0.5), normal((1, 512, 1024), 0.2)
    ctx[:, 64:] = 0
    pad = torch.zeros(1, 1, 8 * Hl, 8 * Wl, device=dev, dtype=torch.bfloat16)
    fps = torch.tensor([24.0], device=dev)

    def make_cond(p):
        c = VideoExtendCondition(crossattn_emb=ctx, crossattn_mask=None, padding_mask=pad, fps=fps, video_cond_bool=True, condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

    return den, xt_full, make_cond(pose), make_cond(torch.zeros_like(pose))


def run_cp(cp, rank, configs, steps, blocks, dev, net):
    den, xt_full, cond, uncond = _step_inputs(net, dev)
    results = []
    lib = _lib.load()
    with FakeRank(cp, rank, dev) as fr:
        if cp > 1:
            net.enable_context_parallel(CP_GROUP)
            from gen3c_amd.parallel import split_inputs_cp
            xt0 = split_inputs_cp(xt_full, 2, net.cp_group)
        else:
            net.disable_context_parallel()
            xt0 = xt_full
        for cfg in (configs if cp > 1 else [None]):
            if cfg is not None:
                G, kern, sched = cfg
                net._cp_attn.configure(head_groups=G, kernel=kern, schedule=sched)
                net._cp_attn.stats = None
            xt = xt0
            xt = den.denoise_step(xt, 0, cond, uncond, 1.0, 0.001, 1)  # warm-up (tables, workspaces, cross-attention K / V)
            torch.cuda.synchronize()
            ops.enable_kernel_timers(True)
            if cp > 1:
                net._cp_attn.stats = []
            fr.bytes = 0
            t0 = time.perf_counter()
            for i in range(steps):
                xt = den.denoise_step(xt, 1 + i, cond, uncond, 1.0, 0.001, 1)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            timers = ops.collected_kernel_timers()
            ops.enable_kernel_timers(False)
            assert bool(torch.isfinite(xt.float()).all())
            table = _class_table(timers, steps, lib)
            wait_ms = None
            if cp > 1 and net._cp_attn.stats:
                wait_ms = round(sum(tm.elapsed_ms() for (_k, _g, tm) in net._cp_attn.stats) / steps, 3)
                net._cp_attn.stats = None
            eff = dict(net._cp_attn.effective) if cp > 1 and net._cp_attn.effective else None
            res = dict(cp=cp, rank=rank, config=None if cfg is None else dict(head_groups=cfg[0], kernel=cfg[1], schedule=cfg[2]), effective=eff,
                       ms_per_step=round(ms, 2), gathered_bytes_per_step=fr.bytes // steps, emulated_exchange_wait_ms_per_step=wait_ms, classes=table)
            results.append(res)
            a = sum(c["ms_per_step"] for c in table if c["kind"] == "attn" and c["Skv"] > 2048)
            n_sa = sum(c["launches_per_step"] for c in table if c["kind"] == "attn" and c["Skv"] > 2048)
            n_layers = sum(c["launches_per_step"] for c in table if c["kind"] == "attn" and c["Skv"] <= 2048)  # one cross-attention launch per layer
            res["self_attention_launches_per_layer"] = round(n_sa / n_layers, 2) if n_layers else None
            g = sum(c["ms_per_step"] for c in table if c["kind"] == "gemm")
            print(f"cp={cp} rank={rank} cfg={cfg} eff={eff}: {ms:.1f} ms/step  (self-attn launches {a:.1f} ms [overlapping streams are summed], block GEMMs {g:.1f} ms, "
                  f"emulated exchange wait {wait_ms}; self-attention launches per layer {res['self_attention_launches_per_layer']})", flush=True)
    if cp > 1:
        net.disable_context_parallel()
    return results


def _exchange_model(r, base, base_rest, layers):
    """The exchange model of main() (described there) for one run record `r` with cp > 1: fills r["self_attention_and_cp_ms_per_layer"] and
    r["predicted"][bandwidth] and returns one (GB/s, predicted ms/step, exposed ms/layer, exchange ms/layer, attention ms/layer, Q ms/layer) per assumed
    rate. A CFG-parallel record (r["cfg"] == 2) is one of 2 x cp ranks at B = 1: its K / V exchange has cp - 1 peers (the bytes the run counted), the
    HBM-bound rest of the cp = 1, B = 2 step is scaled by 1 / (2 cp), and the pair's exchange of the network output is added to every step unhidden."""
    cp = r["cp"]
    eff = r["effective"] or {}
    G, sched = eff.get("head_groups", 4), eff.get("schedule", "gather_first")
    gemm = sum(c["ms_per_step"] for c in r["classes"] if c["kind"] == "gemm")
    cross = sum(c["ms_per_step"] for c in r["classes"] if c["kind"] == "attn" and c["Skv"] <= 2048)
    attn_layer = max(0.0, r["ms_per_step"] - gemm - cross - base_rest / (cp * r.get("cfg", 1))) / layers
    r["self_attention_and_cp_ms_per_layer"] = round(attn_layer, 3)
    q_ms = 0.0
    if sched == "gather_first":  # the self-attention Q projection: one of the two plain N = 4096 launches per block (the other is the cross-attention Q)
        q_ms = sum(c["ms_per_step"] for c in r["classes"] if c["kind"] == "gemm" and c["N"] == 4096 and c["K"] == 4096 and c["epilogue"] == 0) / 2 / layers
    rows = []
    for bw in (250.0, 375.0, 500.0):
        ex_g = r["gathered_bytes_per_step"] / layers / G / (bw * 1e9) * 1e3
        if sched == "gather_first":
            t = q_ms
            for g_ in range(G):
                t = max(t, (g_ + 1) * ex_g) + attn_layer / G
            exposed = t - (q_ms + attn_layer)
        elif sched in ("local_first", "local_carry"):
            t = attn_layer / cp
            for g_ in range(G):
                t = max(t, (g_ + 1) * ex_g) + attn_layer * (cp - 1) / cp / G
            exposed = t - attn_layer
        elif sched == "head_parallel":
            exposed = ex_g  # 3 of the first group's 4 tensors + 1 of the last group's 4 = one group's exchange
        else:
            raise ValueError(f"exchange model: unknown schedule {sched}")
        pred = r["ms_per_step"] + layers * exposed + r.get("cfg_exchange_bytes_per_step", 0) / (bw * 1e9) * 1e3
        r.setdefault("predicted", {})[str(int(bw))] = dict(exchange_ms_per_layer=round(ex_g * G, 3), exposed_ms_per_layer=round(exposed, 3), ms_per_step=round(pred, 1),
                                                           speedup=round(base["ms_per_step"] / pred, 3))
        rows.append((bw, pred, exposed, ex_g * G, attn_layer, q_ms))
    return rows


def _steps_ms(den, xt, cond, uncond, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        xt = den.denoise_step(xt, 1 + i, cond, uncond, 1.0, 0.001, 1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xt.float()).all())
    return (time.perf_counter() - t0) / steps * 1e3


def run_ab_bounded(cp, rank, configs, steps, rounds, blocks, dev, net, base_rest):
    """Switch off / on alternating (see the module docstring) -> one dict per configuration."""
    T, Hl, Wl = 16, 88, 160
    rs = np.random.RandomState(1)
    normal = lambda shape, std: torch.from_numpy((rs.standard_normal(shape) * std).astype(np.float32)).to(torch.bfloat16).to(dev)
    den = Gen3CDenoiser(net, state_shape=(16, T, Hl, Wl))
    den.scheduler.set_timesteps(35)
    xt_full = normal((1, 16, T, Hl, Wl), den.scheduler.init_noise_sigma)
    gt, pose, ctx = normal((1, 16, T, Hl, Wl), 0.5), normal((1, 64, T, Hl, Wl), 0.5), normal((1, 512, 1024), 0.2)
    ctx[:, 64:] = 0
    pad = torch.zeros(1, 1, 8 * Hl, 8 * Wl, device=dev, dtype=torch.bfloat16)
    fps = torch.tensor([24.0], device=dev)

    def make_cond(p):
        c = VideoExtendCondition(crossattn_emb=ctx, crossattn_mask=None, padding_mask=pad, fps=fps, video_cond_bool=True, condition_video_pose=p)
        return add_condition_video_indicator_and_video_input_mask(gt, c, 1)

    cond, uncond = make_cond(pose), make_cond(torch.zeros_like(pose))
    results = []
    with FakeRank(cp, rank, dev):
        net.enable_context_parallel("fake-cp-group")
        from gen3c_amd.parallel import split_inputs_cp
        xt0 = split_inputs_cp(xt_full, 2, net.cp_group)
        for (G, kern, sched) in configs:
            arms = {False: [], True: []}
            eff = {}
            for on in (False, True):  # warm-up of both arms
                net._cp_attn.configure(head_groups=G, kernel=kern, schedule=sched, bounded=on)
                den.denoise_step(xt0, 0, cond, uncond, 1.0, 0.001, 1)
                eff[on] = (dict(net._cp_attn.effective), net._cp_attn.effective_bounded)
            for _ in range(rounds):
                for on in (False, True):
                    net._cp_attn.configure(bounded=on)
                    arms[on].append(_steps_ms(den, xt0, cond, uncond, steps))
            tables = {}
            for on in (False, True):  # one step per arm with the kernel timers on: the per-class table (event pairs around every launch: not part of the timing above)
                net._cp_attn.configure(bounded=on)
                ops.enable_kernel_timers(True)
                den.denoise_step(xt0, 1, cond, uncond, 1.0, 0.001, 1)
                torch.cuda.synchronize()
                cls = {}
                for name, meta, tm in ops.collected_kernel_timers():
                    if name == "gemm_nt":
                        key = ("gemm", meta["M"], meta["N"], meta["K"], "")
                    elif name == "flash_attn_fwd":
                        key = ("attn", meta["Sq"], meta["Skv"], meta["H"], meta.get("kernel", "?") + (" partial" if meta.get("partial") else "") + (" carry" if meta.get("carry") else ""))
                    else:
                        continue
                    c = cls.setdefault(key, [0, 0.0])
                    c[0] += 1
                    c[1] += tm.elapsed_ms()
                ops.enable_kernel_timers(False)
                tables[on] = cls
            net._cp_attn.configure(bounded=False)
            res = dict(cp=cp, rank=rank, config=dict(head_groups=G, kernel=kern, schedule=sched), steps=steps, rounds=rounds)
            for on in (False, True):
                a = arms[on]
                gemm = sum(v[1] for k_, v in tables[on].items() if k_[0] == "gemm")
                cross = sum(v[1] for k_, v in tables[on].items() if k_[0] == "attn" and k_[2] <= 2048)
                mean = sum(a) / len(a)
                res["on" if on else "off"] = dict(
                    effective=eff[on][0], effective_bounded=eff[on][1], ms_per_step_rounds=[round(x, 2) for x in a], ms_per_step=round(mean, 2),
                    spread_pct=round((max(a) - min(a)) / mean * 100, 2),
                    self_attention_and_cp_ms_per_layer=None if base_rest is None else round((mean - gemm - cross - base_rest / cp) / blocks, 3),
                    self_attention_launches=[dict(Sq=k_[1], Skv=k_[2], H=k_[3], kernel=k_[4], launches=v[0], ms_sum=round(v[1], 3))
                                             for k_, v in sorted(tables[on].items()) if k_[0] == "attn" and k_[2] > 2048])
            res["on_over_off"] = round(res["on"]["ms_per_step"] / res["off"]["ms_per_step"], 4)
            results.append(res)
            print(f"cp={cp} rank={rank} {G},{kern},{sched}: off {res['off']['ms_per_step_rounds']} on {res['on']['ms_per_step_rounds']} ms/step -> on / off {res['on_over_off']}"
                  f" (bounded ran: {eff[True][1]})", flush=True)
    net.disable_context_parallel()
    return results


def run_launches(cp, rank, dev, rounds, iters):
    """The self-attention launches of one head group at cp's rank shapes (Sq = S_local, 8 heads, B = 2), alone on one stream: max form and bounded form
    alternating, `rounds` x `iters` launches each. q, k RMS-normalised per head (unit weights), as behind the DiT's QK-norm."""
    import math
    S_all, B, H = 56320, 2, 8
    Sl = S_all // cp
    g = torch.Generator(device=dev).manual_seed(cp)
    rms = lambda x: (x.view(x.shape[0], H, 128) * torch.rsqrt(x.view(x.shape[0], H, 128).pow(2).mean(-1, keepdim=True))).reshape(x.shape[0], H * 128)
    q = rms(torch.randn(Sl * B, H * 128, device=dev, generator=g)).to(torch.bfloat16)
    k = rms(torch.randn(S_all * B, H * 128, device=dev, generator=g)).to(torch.bfloat16)
    vseg = torch.randn(cp, B, H, 128, Sl, device=dev, generator=g).to(torch.bfloat16)
    bound = 128 / math.sqrt(128) * 1.03
    own_k, own_v = k[rank * Sl * B:(rank + 1) * Sl * B], vseg[rank:rank + 1]
    own = ops.flash_attn(q, own_k, own_v, Sl, Sl, B, H, partial=True, variant=11)
    skip = (rank * Sl, Sl) if 0 < rank < cp - 1 else None
    out = torch.empty_like(q)
    forms = {
        "partial (own shard, Skv = S_local)": lambda at: at(q, own_k, own_v, Sl, Sl, B, H, partial=True),
        "carry (remote keys, own block skipped)": lambda at: at(q, k, vseg, Sl, S_all - Sl, B, H, out=out, carry=own, kv_skip=skip),
        "kvseg (gather_first, all keys)": lambda at: at(q, k, vseg, Sl, S_all, B, H, out=out),
    }
    arms = {"max": lambda *a, **kw: ops.flash_attn(*a, variant=11, **kw), "bounded": lambda *a, **kw: ops.self_attn_bounded(*a, bound, variant=11, **kw)}
    rows = []
    for what, call in forms.items():
        ms = {"max": [], "bounded": []}
        for arm in arms:
            call(arms[arm])  # warm-up
        for _ in range(rounds):
            for arm in arms:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _i in range(iters):
                    call(arms[arm])
                e1.record()
                torch.cuda.synchronize()
                ms[arm].append(e0.elapsed_time(e1) / iters)
        mean = {a: sum(v) / len(v) for a, v in ms.items()}
        rows.append(dict(cp=cp, rank=rank, launch=what, Sq=Sl, max_ms=[round(x, 4) for x in ms["max"]], bounded_ms=[round(x, 4) for x in ms["bounded"]],
                         bounded_over_max=round(mean["bounded"] / mean["max"], 4),
                         spread_pct={a: round((max(v) - min(v)) / mean[a] * 100, 2) for a, v in ms.items()}))
        print(f"cp={cp} launch {what}: max {rows[-1]['max_ms']} bounded {rows[-1]['bounded_ms']} ms -> bounded / max {rows[-1]['bounded_over_max']}", flush=True)
    return rows


def main_ab(args, dev, configs, net):
    configs = [c for c in configs if c[2] in ("gather_first", "local_first", "local_carry")]
    cps = [int(c) for c in args.cps.split(",")]
    base_rest = None
    if 1 in cps:
        base = run_cp(1, 0, configs, args.steps, args.blocks, dev, net)[0]
        base_rest = base["ms_per_step"] - sum(c["ms_per_step"] for c in base["classes"] if c["kind"] in ("attn", "gemm"))
    runs, launches = [], []
    for cp in cps:
        if cp > 1:
            runs += run_ab_bounded(cp, cp // 2 if args.rank < 0 else args.rank, configs, args.steps, args.ab_bounded, args.blocks, dev, net, base_rest)
    for cp in cps:
        if cp > 1 and args.launch_iters > 0:
            launches += run_launches(cp, cp // 2 if args.rank < 0 else args.rank, dev, args.ab_bounded, args.launch_iters)
    lines = [f"{'cp':>3} {'config':<22} {'off ms/step (rounds)':<34} {'on ms/step (rounds)':<34} {'on/off':>7} {'spread off/on %':>16} {'self-attn + CP ms/layer off -> on':>34}"]
    for r in runs:
        c = r["config"]
        lines.append(f"{r['cp']:>3} {'%d,%s,%s' % (c['head_groups'], c['kernel'], c['schedule']):<22} {str(r['off']['ms_per_step_rounds']):<34} {str(r['on']['ms_per_step_rounds']):<34} "
                     f"{r['on_over_off']:>7.4f} {'%.2f / %.2f' % (r['off']['spread_pct'], r['on']['spread_pct']):>16} "
                     f"{'%s -> %s' % (r['off']['self_attention_and_cp_ms_per_layer'], r['on']['self_attention_and_cp_ms_per_layer']):>34}"
                     + ("" if r["on"]["effective_bounded"] else "   (the bound was NOT used)"))
    lines.append("")
    lines.append(f"{'cp':>3} {'launch (8 heads, B = 2, one stream)':<42} {'Sq':>6} {'max form ms (rounds)':<30} {'bounded ms (rounds)':<30} {'bounded/max':>11} {'spread max/bounded %':>21}")
    for r in launches:
        lines.append(f"{r['cp']:>3} {r['launch']:<42} {r['Sq']:>6} {str(r['max_ms']):<30} {str(r['bounded_ms']):<30} {r['bounded_over_max']:>11.4f} "
                     f"{'%.2f / %.2f' % (r['spread_pct']['max'], r['spread_pct']['bounded']):>21}")
    text = "\n".join(lines)
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(runs=runs, launches=launches, summary_text=text), indent=1))
    out.with_suffix(".txt").write_text(text + "\n")


def run_cfg_ab(world, configs, steps, rounds, blocks, dev, net):
    """`world` ranks two ways, alternating in one process: plain context parallelism (cp = world, both guidance branches batched as B = 2) against
    CFG-parallel (2 branches x cp = world / 2, the emulated rank runs the conditional branch at B = 1 and exchanges the network output with its pair),
    a middle rank of each. Per configuration `rounds` rounds of (plain, CFG-parallel), each one untimed step after the switch (the switch rebuilds the
    position tables) and `steps` timed ones; then one step per arm with the kernel timers on for the per-class table. The K / V bytes a rank receives
    per step must be L * 2 * (S_local * B * 4096 * 2) * (cp - 1) exactly, the pair's exchange the size of the rank's latent shard."""
    from gen3c_amd.parallel import split_inputs_cp
    den, xt_full, cond, uncond = _step_inputs(net, dev)
    lib = _lib.load()
    S_all, T = 56320, 16
    records = []
    for (G, kern, sched) in (configs if world > 2 else configs[:1]):  # world 2: the CFG-parallel arm has no context parallelism to configure
        arms = [dict(world=world, cfg=1, cp=world, rank=world // 2, B=2), dict(world=world, cfg=2, cp=world // 2, rank=world // 4, B=1)]
        for rnd in range(rounds + 1):
            for a in arms:
                cp = a["cp"]
                with FakeRank(cp, a["rank"], dev, cfg_rank=0 if a["cfg"] == 2 else None) as fr:
                    try:
                        if a["cfg"] == 2:
                            den.enable_cfg_parallel(CFG_GROUP)
                        if cp > 1:
                            net.enable_context_parallel(CP_GROUP)
                            net._cp_attn.configure(head_groups=G, kernel=kern, schedule=sched)
                            xt0 = split_inputs_cp(xt_full, 2, net.cp_group)
                        else:
                            net.disable_context_parallel()
                            xt0 = xt_full
                        den.denoise_step(xt0, 0, cond, uncond, 1.0, 0.001, 1)  # warm-up after the switch
                        torch.cuda.synchronize()
                        fr.bytes = fr.pair_bytes = 0
                        if rnd < rounds:
                            a.setdefault("ms_per_step_rounds", []).append(round(_steps_ms(den, xt0, cond, uncond, steps), 2))
                            n = steps
                        else:  # event pairs around every launch: not part of the timing above
                            ops.enable_kernel_timers(True)
                            den.denoise_step(xt0, 1, cond, uncond, 1.0, 0.001, 1)
                            torch.cuda.synchronize()
                            a["classes"] = _class_table(ops.collected_kernel_timers(), 1, lib)
                            ops.enable_kernel_timers(False)
                            n = 1
                        a["effective"] = dict(net._cp_attn.effective) if cp > 1 and net._cp_attn.effective else None
                        a["gathered_bytes_per_step"], pair_bytes = fr.bytes // n, fr.pair_bytes // n
                        if a["effective"] is None or a["effective"]["schedule"] != "head_parallel":
                            want = blocks * 2 * (S_all // cp * a["B"] * 4096 * 2) * (cp - 1)
                            assert a["gathered_bytes_per_step"] == want, f"{a}: received {a['gathered_bytes_per_step']} B per step, the formula gives {want}"
                        assert pair_bytes == (16 * (T // cp) * 88 * 160 * 2 if a["cfg"] == 2 else 0), pair_bytes
                        if a["cfg"] == 2:
                            a["cfg_exchange_bytes_per_step"] = pair_bytes
                    finally:
                        den.disable_cfg_parallel()
                        net.disable_context_parallel()
        for a in arms:
            r = a["ms_per_step_rounds"]
            a.update(config=dict(head_groups=G, kernel=kern, schedule=sched) if a["cp"] > 1 else None, steps=steps, ms_per_step=round(sum(r) / len(r), 2),
                     spread_pct=round((max(r) - min(r)) / (sum(r) / len(r)) * 100, 2))
            records.append(a)
        print(f"world={world} {G},{kern},{sched}: cp={world} (B=2) {arms[0]['ms_per_step_rounds']}  cfg 2 x cp={world // 2} (B=1) {arms[1]['ms_per_step_rounds']} ms/step -> "
              f"CFG-parallel / plain {arms[1]['ms_per_step'] / arms[0]['ms_per_step']:.4f}", flush=True)
    return records


def main_cfg(args, dev, configs, net):
    """--cfg 2: per total rank count of --worlds, plain CP against CFG-parallel (run_cfg_ab), then the exchange model of main() on every arm."""
    base = run_cp(1, 0, configs, args.steps, args.blocks, dev, net)[0]
    base_rest = base["ms_per_step"] - sum(c["ms_per_step"] for c in base["classes"] if c["kind"] in ("attn", "gemm"))
    runs = []
    for world in [int(w) for w in args.worlds.split(",")]:
        assert world >= 2 and world % 2 == 0, "--worlds: total rank counts, even (2 guidance branches x cp)"
        runs += run_cfg_ab(world, configs, args.steps, args.rounds, args.blocks, dev, net)
    for r in runs:
        _exchange_model(r, base, base_rest, args.blocks)
    ms_of = lambda r, pred: sum(c["ms_per_step"] for c in r["classes"] if pred(c))
    lines = [f"one MI355X as one rank, {args.blocks} blocks, {args.rounds} alternating rounds x {args.steps} steps; cp = 1 (B = 2) base: {base['ms_per_step']:.1f} ms/step. "
             f"compute = measured, no exchange; predicted = compute + exposed K / V exchange (+ the pair's output exchange) at 250 / 375 / 500 GB/s into the rank: a MODEL,",
             "no multi-GPU run exists. Kernel sums are durations of launches that overlap on two streams.", "",
             f"{'ranks':>5} {'layout':<16} {'B':>2} {'config':<22} {'compute ms/step (rounds)':<28} {'mean':>8} {'spread %':>8} {'x cp=1':>7} {'K/V GB/step':>12} {'pair MB/step':>13} "
             f"{'self-attn ms':>13} {'cross-attn ms':>14} {'GEMM ms':>9}  predicted ms/step (speed-up)"]
    for r in runs:
        c, pr = r["config"], r["predicted"]
        lines.append(f"{r['world']:>5} {('cfg 2 x cp %d' % r['cp']) if r['cfg'] == 2 else ('cp %d' % r['cp']):<16} {r['B']:>2} "
                     f"{('%d,%s,%s' % (c['head_groups'], c['kernel'], c['schedule'])) if c else '-':<22} {str(r['ms_per_step_rounds']):<28} {r['ms_per_step']:>8.1f} {r['spread_pct']:>8.2f} "
                     f"{base['ms_per_step'] / r['ms_per_step']:>7.2f} {r['gathered_bytes_per_step'] / 1e9:>12.2f} {r.get('cfg_exchange_bytes_per_step', 0) / 1e6:>13.2f} "
                     f"{ms_of(r, lambda k: k['kind'] == 'attn' and k['Skv'] > 2048):>13.1f} {ms_of(r, lambda k: k['kind'] == 'attn' and k['Skv'] <= 2048):>14.1f} "
                     f"{ms_of(r, lambda k: k['kind'] == 'gemm'):>9.1f}  "
                     + " / ".join(f"{pr[b]['ms_per_step']:.1f} ({pr[b]['speedup']:.2f} x)" for b in ("250", "375", "500")))
    text = "\n".join(lines)
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(base=base, runs=runs, summary_text=text), indent=1))
    out.with_suffix(".txt").write_text(text + "\n")


def run_window(cp, rank, window, config, steps, rounds, blocks, dev, net):
    """Rank `rank` of `cp` two ways, alternating in one process after both arms are warm: the dense context-parallel schedule `config`, and the frame
    window (W, s) under context parallelism - the "window_halo" schedule through the product path (the DiT's switch). Per arm `rounds` rounds of one
    untimed step after the switch and `steps` timed ones; then one step per arm with the kernel timers on for the self-attention launches. The bytes the
    halo arm receives per step are asserted against parallel.window_halo_plan."""
    from gen3c_amd.parallel import split_inputs_cp, window_halo_plan
    den, xt_full, cond, uncond = _step_inputs(net, dev)
    lib = _lib.load()
    W, s = window
    G, kern, sched = config
    T, fl, S_all = 16, 3520, 56320
    plan = window_halo_plan(T, cp, W, s)
    a, b, c = plan["buffers"][rank]
    tiles = ops.window_attn_tiles_cp(S_all // cp, (a + c - b) * fl, fl, T, rank * (T // cp), a, b, W, s)
    arms = {"dense": dict(ms=[]), "halo": dict(ms=[])}
    with FakeRank(cp, rank, dev) as fr:
        try:
            net.enable_context_parallel(CP_GROUP)
            net._cp_attn.configure(head_groups=G, kernel=kern, schedule=sched)
            xt0 = split_inputs_cp(xt_full, 2, net.cp_group)
            for rnd in range(rounds + 1):
                for name, arm in arms.items():
                    net.set_self_attn_window(*((W, s) if name == "halo" else (None,)), context_parallel=name == "halo")
                    den.denoise_step(xt0, 0, cond, uncond, 1.0, 0.001, 1)  # warm-up after the switch
                    torch.cuda.synchronize()
                    fr.bytes = 0
                    if rnd < rounds:
                        arm["ms"].append(round(_steps_ms(den, xt0, cond, uncond, steps), 2))
                        n = steps
                    else:  # event pairs around every launch: not part of the timing above
                        ops.enable_kernel_timers(True)
                        den.denoise_step(xt0, 1, cond, uncond, 1.0, 0.001, 1)
                        torch.cuda.synchronize()
                        table = _class_table(ops.collected_kernel_timers(), 1, lib)
                        ops.enable_kernel_timers(False)
                        sa = [k for k in table if k["kind"] == "attn" and k["Skv"] > 2048]
                        arm["self_attention_ms_per_layer"] = round(sum(k["ms_per_step"] for k in sa) / blocks, 3)  # (launches on two streams overlap: summed)
                        arm["self_attention_kernels"] = sorted({k["kernel"] for k in sa})
                        n = 1
                    arm["effective"] = dict(net._cp_attn.effective)
                    arm["received_bytes_per_step"] = fr.bytes // n
            want = blocks * 2 * plan["remote_frames"][rank] * fl * 2 * 4096 * 2  # K and V rows of the remote frames, B = 2, bf16
            assert arms["halo"]["effective"]["schedule"] == "window_halo" and arms["halo"]["received_bytes_per_step"] == want, (arms["halo"], want)
        finally:
            net.set_self_attn_window(None)
            net.disable_context_parallel()
    for arm in arms.values():
        arm["ms_per_step"] = round(sum(arm["ms"]) / len(arm["ms"]), 2)
        arm["spread_pct"] = round((max(arm["ms"]) - min(arm["ms"])) / arm["ms_per_step"] * 100, 2)
    rec = dict(cp=cp, rank=rank, window=[W, s], buffer=[a, b, c], dense_config=dict(head_groups=G, kernel=kern, schedule=sched), steps=steps, rounds=rounds,
               visited_tiles=tiles[0], dense_tiles=tiles[1], dense=arms["dense"], halo=arms["halo"],
               halo_over_dense=round(arms["halo"]["ms_per_step"] / arms["dense"]["ms_per_step"], 4))
    print(f"cp={cp} rank={rank} window={window} buffer={(a, b, c)}: dense {arms['dense']['ms']} halo {arms['halo']['ms']} ms/step -> halo / dense {rec['halo_over_dense']}; "
          f"tiles {tiles[0]}/{tiles[1]}; received {arms['halo']['received_bytes_per_step'] / 1e9:.2f} against {arms['dense']['received_bytes_per_step'] / 1e9:.2f} GB/step", flush=True)
    return rec


def main_window(args, dev, configs, net):
    """--window W,S: rank 0, a middle rank and the last rank of cp = 8 and cp = 4 (or --cps), dense context parallelism against the window_halo arm
    (run_window). A step is paced by its slowest rank - interior ranks visit more tiles than rank 0 - so the maximum over the ranks is reported."""
    W, s = (int(x) for x in args.window.split(","))
    runs = []
    for cp in [int(c) for c in args.cps.split(",")]:
        if cp > 1:
            for rank in sorted({0, cp // 2, cp - 1}):
                runs.append(run_window(cp, rank, (W, s), configs[0], args.steps, args.rounds, args.blocks, dev, net))
    lines = [f"one MI355X as one rank, {args.blocks} blocks, B = 2, {args.rounds} alternating rounds x {args.steps} steps; window W = {W}, sink s = {s}; compute only - the "
             "exchange is a device copy of the received size. Self-attention ms are summed durations of launches that overlap on two streams.", "",
             f"{'cp':>3} {'rank':>4} {'buffer (a, b, c)':<17} {'dense arm':<22} {'dense ms/step (rounds)':<26} {'halo ms/step (rounds)':<26} {'halo/dense':>10} "
             f"{'spread d / h %':>15} {'self-attn ms/layer d -> h':>26} {'tiles visited / dense':>22} {'received GB/step d -> h':>24}"]
    for r in runs:
        c = r["dense_config"]
        lines.append(f"{r['cp']:>3} {r['rank']:>4} {str(tuple(r['buffer'])):<17} {'%d,%s,%s' % (c['head_groups'], c['kernel'], c['schedule']):<22} {str(r['dense']['ms']):<26} "
                     f"{str(r['halo']['ms']):<26} {r['halo_over_dense']:>10.4f} {'%.2f / %.2f' % (r['dense']['spread_pct'], r['halo']['spread_pct']):>15} "
                     f"{'%.3f -> %.3f' % (r['dense']['self_attention_ms_per_layer'], r['halo']['self_attention_ms_per_layer']):>26} "
                     f"{'%d / %d' % (r['visited_tiles'], r['dense_tiles']):>22} "
                     f"{'%.2f -> %.2f' % (r['dense']['received_bytes_per_step'] / 1e9, r['halo']['received_bytes_per_step'] / 1e9):>24}")
    lines.append("")
    for cp in sorted({r["cp"] for r in runs}):
        rs = [r for r in runs if r["cp"] == cp]
        d, h = max(r["dense"]["ms_per_step"] for r in rs), max(r["halo"]["ms_per_step"] for r in rs)
        lines.append(f"cp={cp}: slowest emulated rank, dense {d:.1f} ms/step, halo {h:.1f} ms/step -> {h / d:.4f} (compute only)")
    text = "\n".join(lines)
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(runs=runs, summary_text=text), indent=1))
    out.with_suffix(".txt").write_text(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", default=None, metavar="W,S", help="the frame window under context parallelism (window_halo) against the dense schedule of the first "
                    "--configs entry, arms alternating: rank 0, a middle rank and the last rank of every --cps entry (default 8,4); --rounds, --steps as for --cfg 2")
    ap.add_argument("--cfg", type=int, choices=(1, 2), default=1, help="2: CFG-parallel (2 guidance branches x cp) against plain context parallelism at the same total "
                    "rank count, arms alternating (run_cfg_ab); 1: the arms below, unchanged")
    ap.add_argument("--worlds", default="8,4,2", help="with --cfg 2: total rank counts")
    ap.add_argument("--rounds", type=int, default=2, help="with --cfg 2: alternating rounds")
    ap.add_argument("--ab_bounded", type=int, default=0, help="> 0: the logit-bound switch off / on alternating, this many rounds (see the module docstring)")
    ap.add_argument("--launch_iters", type=int, default=5, help="with --ab_bounded: launches per round of the launch-by-launch table (0: skip it)")
    ap.add_argument("--cps", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=28)
    ap.add_argument("--rank", type=int, default=-1, help="-1: a middle rank (cp // 2)")
    ap.add_argument("--configs", default="4,auto,gather_first;4,w4b,gather_first;2,auto,gather_first;8,auto,gather_first;4,auto,local_first;4,auto,local_carry;"
                                          "1,auto,gather_first")
    ap.add_argument("--out", default="gpurun_out/r6_cp_rank_shapes.json")
    args = ap.parse_args()
    if args.cfg == 2:  # its own defaults: the shipped schedule plus local_carry, and a record of its own beside the default one
        if args.configs == ap.get_default("configs"):
            args.configs = "4,auto,local_first;4,auto,local_carry"
        if args.out == ap.get_default("out"):
            args.out = str(Path(args.out).with_name("cfg_parallel_rank_shapes.json"))
    if args.window is not None:  # its own defaults: the DiT's shipped schedule as the dense arm, cp = 8 and 4, and a record of its own
        if args.configs == ap.get_default("configs"):
            args.configs = "4,auto,local_first"
        if args.cps == ap.get_default("cps"):
            args.cps = "8,4"
        if args.out == ap.get_default("out"):
            args.out = str(Path(args.out).with_name("attn_window_cp_emulated.json"))
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    configs = [(int(c.split(",")[0]), c.split(",")[1], c.split(",")[2]) for c in args.configs.split(";")]
    net = VideoExtendGeneralDIT(in_channels=16 + 16 * 4 + 1, rope_t_extrapolation_ratio=2.0, num_blocks=args.blocks, device=dev, init_weights=False)
    net.initialize_weights(randomize_adaln=True, seed=1234)
    net.cross_attention_skip_zero_context = False  # the dense workload bench.py times (the record profiles/r6_cp_rank_shapes.* was taken with the product default, ~17 / cp ms less per step)
    if args.window is not None:
        return main_window(args, dev, configs, net)
    if args.ab_bounded > 0:
        return main_ab(args, dev, configs, net)
    if args.cfg == 2:
        return main_cfg(args, dev, configs, net)
    allres = []
    for cp in [int(c) for c in args.cps.split(",")]:
        rank = (cp // 2 if args.rank < 0 else args.rank) if cp > 1 else 0
        allres += run_cp(cp, rank, configs, args.steps, args.blocks, dev, net)
    # ---- summary: best configuration per cp, per-class ratios to cp = 1, and the speed-up model
    base = next(r for r in allres if r["cp"] == 1) if any(r["cp"] == 1 for r in allres) else None
    summary = {}
    for cp in sorted({r["cp"] for r in allres}):
        # per-class rates are read from the run with ONE head group where there is one: with G > 1 the groups' launches overlap on two streams and their
        # summed durations would understate the attention rate
        runs = [r for r in allres if r["cp"] == cp]
        one = [r for r in runs if (r["effective"] or {}).get("head_groups") == 1]
        summary[cp] = one[0] if one else min(runs, key=lambda r: r["ms_per_step"])
    lines = []
    if base is not None:
        def rate(r, pred):
            sel = [c for c in r["classes"] if pred(c)]
            fl = sum(c["tflops"] * c["ms_per_step"] for c in sel)
            ms = sum(c["ms_per_step"] for c in sel)
            return fl / ms if ms else None
        names = [("self-attention", lambda c: c["kind"] == "attn" and c["Skv"] > 2048), ("cross-attention", lambda c: c["kind"] == "attn" and c["Skv"] <= 2048),
                 ("GEMM N>=8192 K=4096 (QKV / KV, MLP-up)", lambda c: c["kind"] == "gemm" and c["N"] >= 8192 and c["K"] == 4096 and c["M"] > 4096),
                 ("GEMM N=4096 K=4096 (Q, out-projections)", lambda c: c["kind"] == "gemm" and c["N"] == 4096 and c["K"] == 4096 and c["M"] > 4096),
                 ("GEMM N=4096 K=16384 (MLP-down)", lambda c: c["kind"] == "gemm" and c["N"] == 4096 and c["K"] == 16384)]
        for nm, pred in names:
            b = rate(base, pred)
            row = [f"{nm}: cp=1 {b:.0f} TF/s" if b else f"{nm}: -"]
            for cp, r in summary.items():
                if cp == 1:
                    continue
                v = rate(r, pred)
                if v and b:
                    row.append(f"cp={cp} {v:.0f} ({v / b * 100:.0f} %)")
            lines.append("  ".join(row))
        lines.append("")
        # ---- exchange model. A rank RECEIVES gathered_bytes_per_step per step; assumed sustained all-gather rate INTO one GPU over its 7 xGMI links: 250 / 375 / 500 GB/s
        # (the guide: ~153 GB/s per link peak; 375 = 35 % of 7 links' bidirectional peak - unmeasured here, hence three values). Per layer the schedule of parallel.py is
        # replayed: the G head groups' collectives go out back to back on RCCL's stream when K | V exist; gather_first: Q projection + its norm pass (q_ms), then group g's
        # attention as soon as group g's exchange has landed; local_first: every group's partial over this rank's own shard first (1 / cp of the attention, no wait), then
        # group g's remote part once its exchange has landed; local_carry: the same timeline (own-shard partials first, then ONE launch per group over every remote key
        # once its exchange has landed, the merge pass folded into that launch's epilogue - its saving is inside the measured attention time). Attention wall time per layer = this run's step time minus its GEMM time minus the HBM-bound rest (the
        # cp = 1 rest scaled by 1 / cp) - launches on two streams overlap, so their summed durations overstate it. RCCL's own CU use while a collective is in flight is
        # NOT modelled (no second GPU here); the driver's --gpus 8 run measures all of it (bench.py `cp` object).
        # head_parallel: per layer and head group four all-to-alls of one size (k, v, q out, o back). Nothing runs before the first group's k, v and q have landed
        # and nothing hides the last group's o: those four are counted as exposed, every other exchange as hidden under the groups' attention.
        base_attn = sum(c["ms_per_step"] for c in base["classes"] if c["kind"] == "attn")
        base_gemm = sum(c["ms_per_step"] for c in base["classes"] if c["kind"] == "gemm")
        base_rest = base["ms_per_step"] - base_attn - base_gemm
        layers = args.blocks
        best_pred = {}
        for r in allres:
            cp = r["cp"]
            if cp == 1:
                continue
            for bw, pred, exposed, ex_layer, attn_layer, q_ms in _exchange_model(r, base, base_rest, layers):
                key = (cp, bw)
                if key not in best_pred or pred < best_pred[key][0]:
                    best_pred[key] = (pred, r, exposed, ex_layer, attn_layer, q_ms)
        for (cp, bw), (pred, r, exposed, ex_layer, attn_layer, q_ms) in sorted(best_pred.items()):
            lines.append(f"cp={cp} @ {bw:.0f} GB/s: best {r['effective']}: compute {r['ms_per_step']:.1f} ms/step (measured, one GPU as rank {r['rank']}); exchange "
                         f"{r['gathered_bytes_per_step'] / 1e9:.1f} GB/step = {ex_layer:.2f} ms/layer vs attention {attn_layer:.2f} ms/layer (+ Q {q_ms:.2f}) -> exposed {exposed:.2f} ms/layer; "
                         f"predicted {pred:.1f} ms/step = {base['ms_per_step'] / pred:.2f} x (compute only: {base['ms_per_step'] / r['ms_per_step']:.2f} x)")
        lines.append("")
        lines.append("per run (compute measured on one GPU as one rank; predicted = compute + exposed exchange at 250 / 375 / 500 GB/s into the rank):")
        lines.append(f"{'cp':>3} {'requested':<24} {'effective':<24} {'self-attn + CP ms/layer':>24} {'compute ms/step':>16} {'received GB/step':>17}  predicted ms/step")
        for r in allres:
            if r["cp"] == 1 or "predicted" not in r:
                continue
            c, e = r["config"], r["effective"] or {}
            pr = r["predicted"]
            lines.append(f"{r['cp']:>3} {'%d,%s,%s' % (c['head_groups'], c['kernel'], c['schedule']):<24} "
                         f"{'%s,%s,%s' % (e.get('head_groups'), e.get('kernel'), e.get('schedule')):<24} {r['self_attention_and_cp_ms_per_layer']:>24.2f} {r['ms_per_step']:>16.1f} "
                         f"{r['gathered_bytes_per_step'] / 1e9:>17.2f}  {pr['250']['ms_per_step']:.1f} / {pr['375']['ms_per_step']:.1f} / {pr['500']['ms_per_step']:.1f}")
    text = "\n".join(lines)
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(runs=allres, summary_text=text), indent=1))
    out.with_suffix(".txt").write_text(text + "\n")


if __name__ == "__main__":
    main()
