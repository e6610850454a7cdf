"""Context parallelism for the DiT over RCCL / xGMI (one process per GPU, torch.distributed backend "nccl" = RCCL).

Mirrors the reference surface
  * split_inputs_cp / cat_outputs_cp / broadcast   (cosmos_predict1/diffusion/module/parallel.py:25-163)
  * distributed.init()                             (cosmos_predict1/utils/distributed.py:49-79)
  * the slice of megatron-core `parallel_state` the GEN3C CLIs touch (gen3c_single_image.py:248-255, 480-484)
but NOT its communication pattern. The reference lets TransformerEngine run a P2P *ring* over the CP ranks
(general_dit.py:540-541), which on xGMI's point-to-point mesh is bound by a single ~153 GB/s link. Here every rank's
K / V shard is exchanged with a direct all-gather (all 7 links busy at once), split into head groups so that the
attention kernel of group g runs on the compute stream while RCCL is still gathering group g+1. An opt-in schedule, "head_parallel",
exchanges heads for tokens with two all-to-alls instead (ContextParallelAttention below).
A second, opt-in axis (CFG-parallel) puts the two classifier-free-guidance branches of a step on separate groups of cp ranks each: the extra groups of
_ParallelState, and cfg_exchange for the one tensor the pairs exchange per step.

Token layout: rows are (s, b) pairs with b fastest and the latent frames sharded contiguously over ranks, so a
rank-major all-gather of row blocks IS the global (s, b) order - no re-sort after the collective.
"""
from __future__ import annotations

import os
from datetime import timedelta
from typing import Callable, List, Optional

import torch
import torch.distributed as dist


# ------------------------------------------------------------------------------------------------------------------
# reference-compatible helpers
# ------------------------------------------------------------------------------------------------------------------
def split_inputs_cp(x: torch.Tensor, seq_dim: int, cp_group) -> torch.Tensor:
    """This rank's contiguous slice of `x` along `seq_dim` (parallel.py:25-53)."""
    cp_size = dist.get_world_size(cp_group)
    rank = dist.get_rank(cp_group)
    n = x.shape[seq_dim]
    assert n % cp_size == 0, f"{n} cannot divide cp_size {cp_size}"
    step = n // cp_size
    return x.narrow(seq_dim, rank * step, step).contiguous()


def cat_outputs_cp(x: torch.Tensor, seq_dim: int, cp_group) -> torch.Tensor:
    """All-gather the per-rank slices and concatenate them along `seq_dim` (parallel.py:56-87)."""
    world = dist.get_world_size(cp_group)
    parts = [torch.empty_like(x) for _ in range(world)]
    dist.all_gather(parts, x.contiguous(), group=cp_group)
    return torch.cat(parts, dim=seq_dim)


def broadcast(item, to_tp: bool = True, to_cp: bool = True):
    """Broadcast a tensor / picklable object from the lowest rank of the CP group (parallel.py:90-163).
    There is no tensor parallelism on this path (Attention.tp_size = 1, attention.py:205): `to_tp` is accepted
    and ignored.
    Under CFG-parallel (initialize_model_parallel(cfg_parallel_size=2)) the source is the lowest rank of the model-parallel group - all 2 cp ranks -
    with or without `to_cp`: the two branch groups feed the same gt_latent and pose buffers to the Euler kernel, and gt_latent derives from renders
    whose fp32 atomic sums are not order-reproducible, so "every rank computes it" does not give both groups the same bytes."""
    if not parallel_state.is_initialized():
        return item
    if parallel_state.get_cfg_parallel_world_size() > 1:
        group = parallel_state.get_model_parallel_group()
    else:
        group = parallel_state.get_context_parallel_group()
        if not (to_cp and dist.get_world_size(group) > 1):
            return item
    src = min(dist.get_process_group_ranks(group))
    if isinstance(item, torch.Tensor):
        dev = item.device
        if dist.get_rank() == src:
            shape = torch.tensor(item.shape, dtype=torch.long, device=dev)
        else:
            shape = torch.empty(item.dim(), dtype=torch.long, device=dev)
        dist.broadcast(shape, src, group=group)
        if dist.get_rank() != src:
            item = item.new_empty(shape.tolist())
        item = item.contiguous()
        dist.broadcast(item, src, group=group)
        return item
    if item is not None:
        box = [item]
        dist.broadcast_object_list(box, src, group=group)
        return box[0]
    return item


class _ParallelState:
    """The part of megatron.core.parallel_state that gen3c_*.py use, for a context-parallel job, optionally with the two classifier-free-guidance
    branches on separate rank groups (CFG-parallel, opt-in).

    cfg_parallel_size = 2 needs world == 2 * cp. Global rank r: cfg_rank = r // cp (0 runs the conditional branch, 1 the unconditional one),
    cp_rank = r % cp. The CP groups are the contiguous blocks [0, cp) and [cp, 2 cp); the pair groups {r, r + cp} exchange the network output of a
    step (cfg_exchange); the model-parallel group is all 2 cp ranks (broadcast, the sharded render / encode stages of a chunk)."""

    def __init__(self):
        self._cp_group = None
        self._cfg_group = None
        self._mp_group = None

    def initialize_model_parallel(self, context_parallel_size: int = 1, cfg_parallel_size: int = 1, **_unused):
        world = dist.get_world_size()
        assert world % context_parallel_size == 0, f"world size {world} not divisible by cp {context_parallel_size}"
        assert cfg_parallel_size in (1, 2), f"cfg_parallel_size {cfg_parallel_size}: classifier-free guidance has two branches (1 = off, 2 = one rank group each)"
        if cfg_parallel_size == 2:
            assert world == 2 * context_parallel_size, f"CFG-parallel needs world == 2 x cp: world {world}, cp {context_parallel_size}"
        # every rank creates every group, in the same order (torch.distributed.new_group is collective over the whole world)
        my_group = None
        for start in range(0, world, context_parallel_size):
            ranks = list(range(start, start + context_parallel_size))
            g = dist.new_group(ranks)
            if dist.get_rank() in ranks:
                my_group = g
        self._cp_group = my_group
        self._cfg_group = self._mp_group = None
        if cfg_parallel_size == 2:
            for r in range(context_parallel_size):
                ranks = [r, r + context_parallel_size]
                g = dist.new_group(ranks)
                if dist.get_rank() in ranks:
                    self._cfg_group = g
            self._mp_group = dist.new_group(list(range(world)))

    def get_cfg_parallel_group(self):
        """The pair {r, r + cp} of this rank, or None without CFG-parallel."""
        return self._cfg_group

    def get_cfg_parallel_world_size(self) -> int:
        return dist.get_world_size(self._cfg_group) if self._cfg_group is not None else 1

    def get_cfg_parallel_rank(self) -> int:
        """0: this rank runs the conditional branch (also without CFG-parallel), 1: the unconditional one."""
        return dist.get_rank(self._cfg_group) if self._cfg_group is not None else 0

    def get_model_parallel_group(self):
        """Every rank that works on the same sample: all 2 cp ranks under CFG-parallel, otherwise the CP group itself."""
        return self._mp_group if self._mp_group is not None else self.get_context_parallel_group()

    def is_initialized(self) -> bool:
        return self._cp_group is not None

    def get_context_parallel_group(self):
        assert self._cp_group is not None, "context parallel group is not initialized"
        return self._cp_group

    def get_context_parallel_world_size(self) -> int:
        return dist.get_world_size(self._cp_group) if self._cp_group is not None else 1

    def get_context_parallel_rank(self) -> int:
        return dist.get_rank(self._cp_group) if self._cp_group is not None else 0

    def get_tensor_model_parallel_group(self):
        return None

    def get_tensor_model_parallel_world_size(self) -> int:
        return 1

    def destroy_model_parallel(self):
        self._cp_group = None
        self._cfg_group = None
        self._mp_group = None


parallel_state = _ParallelState()


def init_distributed(backend: Optional[str] = None, timeout_s: Optional[int] = None) -> int:
    """Counterpart of cosmos_predict1.utils.distributed.init (utils/distributed.py:49-79) without the NVIDIA-only
    parts (pynvml affinity, libcudart cudaDeviceSetLimit). One process per GPU; rendezvous via env:// as set by
    torchrun. Returns the local device index."""
    local_rank = int(os.getenv("LOCAL_RANK", 0))
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (required by RCCL on this driver)
    if backend == "nccl":
        torch.cuda.set_device(local_rank)
    if not dist.is_initialized():
        # timeout_s: bench.py passes a short collective timeout - a hung exchange must end the run inside the driver's budget, not after 30 min
        timeout = timedelta(seconds=int(timeout_s if timeout_s is not None else os.getenv("TORCH_NCCL_HEARTBEAT_TIMEOUT_SEC", 1800)))
        dist.init_process_group(backend=backend, init_method="env://", timeout=timeout)
    return local_rank


# ------------------------------------------------------------------------------------------------------------------
# sharding the replicated stages of a chunk: render items and tokenizer encodes are independent units
# ------------------------------------------------------------------------------------------------------------------
def shard_range(n_units: int, rank: int, world: int):
    """Contiguous, balanced split of `n_units` over `world` ranks -> [lo, hi) of `rank` (the first n % world ranks get one more)."""
    q, r = divmod(n_units, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def gather_rows(local: torch.Tensor, counts: List[int], group) -> torch.Tensor:
    """All-gather of per-rank row blocks of different lengths (`counts[r]` rows on rank r, identical trailing shape): every rank pads
    its block to max(counts), one all_gather_into_tensor, the padding is cut out. Rank-major = the original unit order."""
    world = dist.get_world_size(group)
    assert len(counts) == world and local.shape[0] == counts[dist.get_rank(group)]
    m = max(counts)
    pad = local if local.shape[0] == m else torch.cat([local, local.new_zeros((m - local.shape[0],) + tuple(local.shape[1:]))], 0)
    full = torch.empty((world * m,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(full, pad.contiguous(), group=group)
    if all(c == m for c in counts):
        return full
    return torch.cat([full[r * m:r * m + c] for r, c in enumerate(counts)], 0)


def run_jobs_round_robin(jobs: List[Callable[[], torch.Tensor]], group, shape, dtype, device) -> List[torch.Tensor]:
    """Independent jobs whose results all have `shape` / `dtype` (the 2N+1 tokenizer encodes of a chunk): job j runs on rank
    j % world only, the results are all-gathered and returned in job order on every rank. group=None (or one rank): plain sequential
    execution. A rank without a job (more ranks than jobs) contributes zeros that nobody reads."""
    world = 1 if group is None else dist.get_world_size(group)
    if world == 1:
        return [j() for j in jobs]
    rank = dist.get_rank(group)
    slots = (len(jobs) + world - 1) // world
    local = torch.zeros((slots, *shape), dtype=dtype, device=device)
    for i, j in enumerate(range(rank, len(jobs), world)):
        out = jobs[j]()
        assert tuple(out.shape) == tuple(shape) and out.dtype == dtype, f"job {j}: {tuple(out.shape)} {out.dtype} vs declared {tuple(shape)} {dtype}"
        local[i] = out
    full = torch.empty((world * slots, *shape), dtype=dtype, device=device)
    dist.all_gather_into_tensor(full, local, group=group)
    return [full[(j % world) * slots + j // world] for j in range(len(jobs))]


def cfg_exchange(out_local: torch.Tensor, cfg_group):
    """CFG-parallel: the one exchange of a denoise step. Each rank of the pair `cfg_group` has run the network on its own guidance branch;
    one all_gather_into_tensor hands both outputs to both ranks -> (out_cond, out_uncond), slot 0 = the pair's rank 0 = the conditional branch.
    7.2 MB / cp per step at full size, against the per-layer K / V exchange of context parallelism. CPU tensors over gloo and device tensors over
    RCCL go straight through; device tensors on a gloo group (tests and tools/cfg_check.py with several ranks on one GPU) are staged through the host."""
    assert dist.get_world_size(cfg_group) == 2, "classifier-free guidance has two branches"
    flat = out_local.contiguous().view(-1)
    both = torch.empty(2 * flat.numel(), dtype=flat.dtype, device=flat.device)  # rank-major concatenation along dim 0: the form every backend takes
    if flat.is_cuda and dist.get_backend(cfg_group) == "gloo":
        host = torch.empty(both.shape, dtype=both.dtype)
        _HostStagedWork(dist.all_gather_into_tensor(host, flat.cpu(), group=cfg_group, async_op=True), host, both).wait()
    else:
        dist.all_gather_into_tensor(both, flat, group=cfg_group)
    both = both.view((2,) + tuple(out_local.shape))
    return both[0], both[1]


# ------------------------------------------------------------------------------------------------------------------
# context-parallel self-attention
# ------------------------------------------------------------------------------------------------------------------
ATTN_KERNELS = {"auto": None, "w4b": 11, "wave8": 4}  # per-call kernel choice of g3_flash_attn_fwd_ex_bf16 ("auto": the even-fill rule below)
CP_SCHEDULES = ("gather_first", "local_first", "local_carry", "head_parallel", "window_halo")


def window_halo_plan(T: int, world: int, W: int, s: int) -> dict:
    """The exchange of the frame-window self-attention under key sharding (schedule "window_halo"): T latent frames sharded contiguously, fpr = T / world
    per rank, window W frames either side, the first s frames attended by everyone. Rank r owns frames [r fpr, (r + 1) fpr); its query blocks lie
    inside them, so together they attend the frames [max(0, r fpr - W), min(T, (r + 1) fpr + W)) and [0, min(s, T)) - whatever the frame length.
    Returns dict(fpr=..., buffers=[(a, b, c) per rank], sends={(p, r): [(f0, f1), ...]}, remote_frames=[per rank]):
      buffers[r]     the rank's compact K / V buffer holds the global frames [0, a) ++ [b, c) in ascending order, and no others (a sink that reaches
                     the window: a == b == 0, the one range [0, c))
      sends[(p, r)]  the whole-frame pieces [f0, f1) of rank p's shard that rank r's buffer holds, ascending (at most one per buffer piece; p == r: the
                     rank's own frames). Sender-major they are rank r's buffer: ranks own ascending frames.
      remote_frames  frames rank r receives from others = what the exchange moves
    Every number is derived from the four arguments."""
    T, world, W, s = int(T), int(world), int(W), int(s)
    if T <= 0 or world <= 0 or T % world or W < 0 or s < 0:
        raise ValueError(f"window_halo_plan: T {T} must be a positive multiple of world {world}, W {W} and s {s} >= 0")
    fpr = T // world
    sink = min(s, T)
    buffers, sends, remote = [], {}, []
    for r in range(world):
        lo, hi = max(0, r * fpr - W), min(T, (r + 1) * fpr + W)
        buffers.append((0, 0, max(hi, sink)) if sink >= lo else (sink, lo, hi))
        a, b, c = buffers[r]
        n = 0
        for p in range(world):
            p0, p1 = p * fpr, (p + 1) * fpr
            pieces = [(max(x0, p0), min(x1, p1)) for x0, x1 in ((0, a), (b, c)) if max(x0, p0) < min(x1, p1)]
            if len(pieces) == 2 and pieces[0][1] == pieces[1][0]:  # (a == b inside p's shard)
                pieces = [(pieces[0][0], pieces[1][1])]
            sends[(p, r)] = pieces
            if p != r:
                n += sum(f1 - f0 for f0, f1 in pieces)
        remote.append(n)
    return dict(fpr=fpr, buffers=buffers, sends=sends, remote_frames=remote)


def _default_backend():
    from . import ops
    return dict(
        pack=lambda t: t.contiguous(),
        transpose_v=lambda v, S, B, H: ops.transpose_v(v, S, B, H),
        attention=lambda q, k, vt, Sq, Skv, B, H, out, variant=0: ops.flash_attn(q, k, vt, Sq, Skv, B, H, out=out, variant=variant),
        attention_partial=lambda q, k, vt, Sq, Skv, B, H, variant=0: ops.flash_attn(q, k, vt, Sq, Skv, B, H, variant=variant, partial=True),
        merge=lambda parts, Sq, B, H, out: ops.attn_merge(parts, Sq, B, H, out=out),
        attention_carry=lambda q, k, vt, Sq, Skv, B, H, out=None, carry=None, kv_skip=None, partial=False, variant=0: ops.flash_attn(
            q, k, vt, Sq, Skv, B, H, out=out, variant=variant, partial=partial, carry=carry, kv_skip=kv_skip),
        scatter_heads=lambda q, k, v, H, n_dest, head0, Hg: ops.cp_scatter_heads(q, k, v, H, n_dest, head0, Hg),
        gather_heads=lambda x, out, H, head0: ops.cp_gather_heads(x, out, H, head0),
        attention_bounded=lambda q, k, vt, Sq, Skv, B, H, logit_bound, out, variant=0, mfma16=False: ops.self_attn_bounded(
            q, k, vt, Sq, Skv, B, H, logit_bound, out=out, variant=variant, mfma16=mfma16),
        # the key-sharded forms with a logit bound (g3_self_attn_fwd_bounded_cp_bf16): what "attention", "attention_partial" and "attention_carry" take
        attention_bounded_cp=lambda q, k, vt, Sq, Skv, B, H, logit_bound, out=None, carry=None, kv_skip=None, partial=False, variant=0: ops.self_attn_bounded(
            q, k, vt, Sq, Skv, B, H, logit_bound, out=out, variant=variant, partial=partial, carry=carry, kv_skip=kv_skip),
        # the frame window over a compact halo buffer (g3_self_attn_fwd_window_cp_bf16): schedule "window_halo". `window`: frame_len, total_frames,
        # q_frame0, buf_head_frames, buf_tail_frame0, window_frames, sink_frames
        attention_window_cp=lambda q, k, vt, Sq, Skv_buf, B, H, logit_bound, out, *window: ops.self_attn_window_cp(
            q, k, vt, Sq, Skv_buf, B, H, logit_bound, *window, out=out),
        timer=ops.HipTimer,
    )


class _HostStagedWork:
    """Work of a collective that ran on host copies of device tensors: wait() also enqueues the copy of the result back to the device."""

    def __init__(self, work, host: torch.Tensor, dev: torch.Tensor):
        self.work, self.host, self.dev = work, host, dev

    def wait(self):
        self.work.wait()
        self.dev.copy_(self.host)
        return True


class ContextParallelAttention:
    """softmax(Q_local K_all^T) V_all for a token-sharded sequence.

    q, k, v: [S_local*B, H*128] (v may be a strided column view). K and V shards are all-gathered head-group by
    head-group (async, RCCL stream) and consumed by the attention kernel in the same order.

    schedule "gather_first": one attention launch per head group over the gathered keys; only the first group's exchange is exposed (behind
    the Q projection), the rest hides under the attention of earlier groups.
    schedule "local_first" (what TransformerEngine's ring does behind attn_op.set_context_parallel_group, general_dit.py:540-541: start on the
    local shard at once): every head group first runs over THIS rank's K / V shard - no collective is waited for - and returns a normalised
    fp32 partial + log-sum-exp; the remote keys (ranks before / after this one in the gathered buffers) follow as the groups' exchanges land,
    and g3_attn_merge_partials_bf16 combines the parts. Costs one fp32 round trip of the group's output per part; hides the first exchange.
    schedule "local_carry": the same phase 1 (an fp32 partial + log-sum-exp over the own shard, no wait), then ONE launch per group over every
    remote key - an interior rank skips its own block inside the gathered buffers (g3_flash_attn_fwd_carry_bf16's kv_skip) - that carries the
    phase-1 state in and writes bf16 straight into the group's columns of the output: two launches per group, no merge pass. Needs a backend with
    "attention_carry", segmented V^T and world > 1; otherwise it runs as "local_first" (and `effective` says so).
    schedule "head_parallel" (DeepSpeed-Ulysses): HEADS are sharded instead of keys. Per head group one g3_cp_scatter_heads_bf16 launch packs q, k and
    v by destination rank, three all-to-alls hand this rank ALL tokens of its H / world heads of the group, the ordinary full-length self-attention
    runs on them (Sq = Skv = S_all, plain V^T: with `logit_bound` the no-running-max kernel applies), a fourth all-to-all returns the output and
    g3_cp_gather_heads_bf16 writes it into the group's columns. No partials, no merge, a quarter of the exchanged bytes at cp = 8; the first group's
    exchange and the last group's return hide behind nothing. Needs H % world == 0 and a backend with "scatter_heads", "gather_heads" and
    "attention_bounded"; otherwise it runs as "local_first" (and `effective` says so). Runs at world 1 too (a self-exchange).
    schedule "window_halo" (opt-in, with configure(window=(frame_len, W, s)); the frame-window self-attention, a different FUNCTION: DESIGN.md section
    11): a rank needs only the frames within W of its own and the first s. Per head group the K rows and the V rows of exactly those frames travel by
    one all-to-all with split sizes each (window_halo_plan; a rank's own frames are its split to itself), so the receive buffer IS the compact buffer
    in global ascending order. finish(): wait, transpose the compact V, one g3_self_attn_fwd_window_cp_bf16 launch per group straight into its output
    columns. No partials, no merge, no carry; only the first group's exchange is exposed. Needs S_local a multiple of frame_len and a backend with
    "attention_window_cp"; anything else raises (no other schedule computes this function). Runs at world 1 too.

    bounded (opt-in, default off): with a caller's `logit_bound` > 0 the three key-sharding schedules run every attention launch through the backend's
    "attention_bounded_cp" - the no-running-max forms of the one-wave-per-SIMD kernel, g3_self_attn_fwd_bounded_cp_bf16 - where the layer's kernel is
    that kernel (variant 11). The bound is the same constant reference point in every launch of a row, so parts merge and carry exactly as the
    max form's do. `effective_bounded` says whether the last finish() did; off, or where it does not apply, the launches are exactly the ones above.

    kernel: "auto" (the one-wave-per-SIMD kernel when the groups' workgroups together fill the 256 CUs evenly, else the 8-wave kernel), "w4b",
    "wave8" - passed PER CALL through the C ABI; no process-wide option is touched (launches go out on two streams).

    `backend` (dict of callables) exists so the sharding + collective schedule can be exercised on CPU with gloo in tests; the product path
    always uses the HIP kernels. `stats` (set to a list to enable): one (kind, head group, HipTimer) per collective wait - the time the launch
    stream stalled for that exchange - read by bench.py.
    """

    def __init__(self, cp_group, head_groups: int = 4, backend: Optional[dict] = None, schedule: str = "gather_first", kernel: str = "auto",
                 bounded: bool = False):
        assert schedule in CP_SCHEDULES and kernel in ATTN_KERNELS
        self.group = cp_group
        self.world = dist.get_world_size(cp_group)
        self.rank = dist.get_rank(cp_group)
        self.head_groups = head_groups
        self.backend = backend
        self.schedule = schedule
        self.kernel = kernel
        self.bounded = bool(bounded)
        self.window = None  # (frame_len, W, s) of schedule "window_halo"
        self._schedule_without_window = "gather_first" if schedule == "window_halo" else schedule
        # head_parallel only (its launches see all keys of their heads at once, as the single-GPU call): ask "attention_bounded" for the 16x16x32 tile
        # loop (ops.self_attn_bounded(mfma16=True)). The DiT sets it from dit._SELF_ATTN_MFMA16; the backend is passed the keyword only when it is on.
        self.mfma16 = False
        self.stats = None
        self.effective = None  # set by finish(): dict(schedule, kernel, head_groups) of the configuration that actually ran
        self.effective_bounded = False  # set by finish(): the key-sharding schedules' launches went through "attention_bounded_cp" (see `bounded`)
        self.bytes_gathered = 0  # received from the other ranks since construction / the last reset (bench.py's "cp" object)

    def configure(self, head_groups: Optional[int] = None, schedule: Optional[str] = None, kernel: Optional[str] = None, bounded: Optional[bool] = None,
                  window=False):
        """window=(frame_len, W, s): select schedule "window_halo" with these numbers; window=None: back to the schedule configured before it."""
        if head_groups is not None:
            self.head_groups = int(head_groups)
        if schedule is not None:
            assert schedule in CP_SCHEDULES
            self.schedule = schedule
            if schedule != "window_halo":
                self._schedule_without_window = schedule
        if window is None:
            self.window = None
            if self.schedule == "window_halo":
                self.schedule = self._schedule_without_window
        elif window is not False:
            fl, W, s = (int(x) for x in window)
            if fl <= 0 or W < 0 or s < 0:
                raise ValueError(f"window_halo: frame_len {fl} must be positive, window frames {W} and sink frames {s} >= 0")
            self.window = (fl, W, s)
            self.schedule = "window_halo"
        if kernel is not None:
            assert kernel in ATTN_KERNELS
            self.kernel = kernel
        if bounded is not None:
            self.bounded = bool(bounded)
        return self

    def start(self, k: torch.Tensor, v: torch.Tensor, S_local: int, B: int, H: int):
        """Issue the K / V all-gathers of every head group (async). Call as soon as K and V exist: whatever the caller
        launches before finish() - the Q projection and its norm/RoPE in the DiT - hides part of the first group's exchange.

        V is transposed LOCALLY (this rank's S_local keys) and the V^T shards are gathered rank-major; the attention kernel reads
        them as key segments, so no rank re-transposes the full-length V (needs S_local % 64 == 0, true for the 3 520-token
        latent frames; otherwise V is gathered row-major and transposed after the exchange).
        "head_parallel" sends q together with k and v, so nothing goes out here: k and v are kept for finish()."""
        be = self.backend or _default_backend()
        if self.schedule == "window_halo":
            return self._start_window_halo(be, k, v, S_local, B, H)
        if self.schedule == "head_parallel" and H % self.world == 0 and all(n in be for n in ("scatter_heads", "gather_heads", "attention_bounded")):
            # nothing can go out before q exists: one scatter launch fills the q, k and v send buffers of a head group (finish())
            return dict(head_parallel=True, k=k, v=v, S_local=S_local, B=B, H=H, rows=S_local * B, be=be)
        G = self.head_groups
        while H % G != 0:
            G -= 1
        Hg = H // G
        W = Hg * 128
        rows = S_local * B
        segmented = S_local % 64 == 0
        works = []
        for g in range(G):
            ks = be["pack"](k[:, g * W:(g + 1) * W])
            kf = torch.empty((self.world * rows, W), dtype=k.dtype, device=k.device)
            wk = dist.all_gather_into_tensor(kf, ks, group=self.group, async_op=True)
            if segmented:
                vs = be["transpose_v"](v[:, g * W:(g + 1) * W], S_local, B, Hg)  # [B, Hg, 128, S_local]
                vf = torch.empty((self.world * vs.shape[0],) + tuple(vs.shape[1:]), dtype=v.dtype, device=v.device)  # dim-0 concat
            else:
                vs = be["pack"](v[:, g * W:(g + 1) * W])
                vf = torch.empty((self.world * rows, W), dtype=v.dtype, device=v.device)
            wv = dist.all_gather_into_tensor(vf, vs, group=self.group, async_op=True)
            self.bytes_gathered += (self.world - 1) * (ks.numel() * ks.element_size() + vs.numel() * vs.element_size())
            works.append((wk, wv, kf, vf, ks, vs))
        return dict(works=works, S_local=S_local, B=B, H=H, Hg=Hg, W=W, rows=rows, be=be, segmented=segmented)

    def _variant(self, S_local: int, S_all: int, B: int, H: int) -> int:
        """Kernel for every launch of this layer. One launch per head group covers only H / G heads - 0.9 to 3.4 rounds of the 256 CUs at
        cp = 8..2 - but the groups run back to back on two streams, so the chip sees their SUM: the one-wave-per-SIMD kernel's even-fill rule
        (attention.hip: attn_resolve_variant) is applied to all H heads."""
        forced = ATTN_KERNELS[self.kernel]
        if forced is not None:
            return forced if S_all % 64 == 0 else 4
        total_wg = ((S_local + 255) // 256) * H * B
        rounds = (total_wg + 255) // 256
        return 11 if (S_all > 2048 and S_all % 64 == 0 and total_wg * 100 >= rounds * 256 * 93) else 4

    def _wait(self, be, g: int, *works):
        """Work.wait() makes the CURRENT stream wait for the collective (torch.distributed semantics on the NCCL / RCCL backend). With stats
        enabled an event pair brackets it: elapsed = how long this stream had nothing to run because the exchange had not landed yet."""
        tm = None
        if self.stats is not None and "timer" in be:
            tm = be["timer"]()
            tm.start()
        for w in works:
            w.wait()
        if tm is not None:
            tm.stop()
            self.stats.append(("wait", g, tm))

    def _all_to_all(self, recv: torch.Tensor, send: torch.Tensor, recv_splits=None, send_splits=None):
        """Async single-tensor all-to-all of equal chunks (send / recv: contiguous [world, ...]) or, with split sizes, of per-rank row counts along
        dim 0 -> a Work. Device tensors on a gloo group (tests and tools/cp_check.py with several ranks on one GPU; the product path is RCCL) are
        staged through host memory: only the single-tensor all-to-all on CPU tensors is relied on with gloo."""
        splits = {} if recv_splits is None else dict(output_split_sizes=recv_splits, input_split_sizes=send_splits)
        if send.is_cuda and dist.get_backend(self.group) == "gloo":
            host = torch.empty(recv.shape, dtype=recv.dtype)
            return _HostStagedWork(dist.all_to_all_single(host, send.cpu(), group=self.group, async_op=True, **splits), host, recv)
        return dist.all_to_all_single(recv, send, group=self.group, async_op=True, **splits)

    def _start_window_halo(self, be, k: torch.Tensor, v: torch.Tensor, S_local: int, B: int, H: int):
        if self.window is None:
            raise ValueError('schedule "window_halo" needs configure(window=(frame_len, W, s))')
        if "attention_window_cp" not in be:
            raise ValueError('schedule "window_halo": the backend has no "attention_window_cp", and no other schedule computes the window function')
        fl, Wf, sf = self.window
        if S_local % fl:
            raise ValueError(f"window_halo: S_local {S_local} is not a multiple of frame_len {fl} (a rank owns whole latent frames)")
        P, r = self.world, self.rank
        fpr = S_local // fl
        plan = window_halo_plan(fpr * P, P, Wf, sf)
        a, b, c = plan["buffers"][r]
        rpf = fl * B  # rows of a frame: contiguous in the (s, b) row order
        frames = lambda pieces: sum(f1 - f0 for f0, f1 in pieces)
        send_splits = [frames(plan["sends"][(r, d)]) * rpf for d in range(P)]
        recv_splits = [frames(plan["sends"][(p, r)]) * rpf for p in range(P)]
        assert sum(recv_splits) == (a + c - b) * rpf
        # destination-major row slices of this rank's shard (frame f = local rows [(f - r fpr) rpf, (f + 1 - r fpr) rpf))
        slices = [slice((f0 - r * fpr) * rpf, (f1 - r * fpr) * rpf) for d in range(P) for f0, f1 in plan["sends"][(r, d)]]
        G = self.head_groups
        while H % G != 0:
            G -= 1
        Hg = H // G
        W = Hg * 128
        works = []
        for g in range(G):
            bufs = []
            for t in (k, v):
                send = torch.cat([t[sl, g * W:(g + 1) * W] for sl in slices], 0)  # the one pack pass: K / V rows by destination
                recv = torch.empty((sum(recv_splits), W), dtype=t.dtype, device=t.device)
                bufs.append((self._all_to_all(recv, send, recv_splits, send_splits), recv, send))
            self.bytes_gathered += 2 * plan["remote_frames"][r] * rpf * W * k.element_size()
            works.append(bufs)
        return dict(window_halo=True, works=works, S_local=S_local, B=B, H=H, Hg=Hg, W=W, rows=S_local * B, be=be, frame_len=fl, window=(Wf, sf),
                    total_frames=fpr * P, q_frame0=r * fpr, buffer=(a, b, c), Skv_buf=(a + c - b) * fl)

    def _finish_window_halo(self, q: torch.Tensor, pending: dict, logit_bound: float) -> torch.Tensor:
        be, W, Hg, B, S_local, works = (pending[n] for n in ("be", "W", "Hg", "B", "S_local", "works"))
        (a, b, _c), Skv_buf, (Wf, sf) = pending["buffer"], pending["Skv_buf"], pending["window"]
        self.effective = dict(schedule="window_halo", kernel="w4b", head_groups=len(works))
        out = torch.empty((pending["rows"], pending["H"] * 128), dtype=q.dtype, device=q.device)
        two_streams = q.is_cuda and len(works) >= 2
        main = side = q_ready = None
        if two_streams:
            main = torch.cuda.current_stream(q.device)
            side = self._side_stream(q.device)
            q_ready = main.record_event()  # q (and `out`) were produced / allocated on the main stream
        # Lifetime contract (as in finish()): the send and receive buffers stay referenced by `pending` until every launch below is enqueued; `keep`
        # does the same for the transposed V^T buffers, which only kernels launched through ctypes read.
        keep = []
        try:
            for g, ((wk, kr, _ks), (wv, vr, _vs)) in enumerate(works):
                st = main if (not two_streams or g % 2 == 0) else side
                with (torch.cuda.stream(st) if two_streams else _NullCtx()):
                    if two_streams and st is side:
                        st.wait_event(q_ready)
                    self._wait(be, g, wv)
                    vt = be["transpose_v"](vr, Skv_buf, B, Hg)  # plain V^T of the compact buffer
                    keep.append(vt)
                    self._wait(be, g, wk)
                    be["attention_window_cp"](q[:, g * W:(g + 1) * W], kr, vt, S_local, Skv_buf, B, Hg, logit_bound, out[:, g * W:(g + 1) * W],
                                              pending["frame_len"], pending["total_frames"], pending["q_frame0"], a, b, Wf, sf)
        finally:
            if two_streams:
                main.wait_stream(side)
        del keep
        return out

    def _finish_head_parallel(self, q: torch.Tensor, pending: dict, logit_bound: float) -> torch.Tensor:
        be, B, S_local, H, rows, k, v = (pending[n] for n in ("be", "B", "S_local", "H", "rows", "k", "v"))
        P = self.world
        Hl = H // P
        G = max(1, min(self.head_groups, Hl))
        while Hl % G != 0:
            G -= 1
        Hg = Hl // G
        S_all = S_local * P
        # the launches' own shape - all tokens as queries - with the heads of ALL groups: as for the other schedules the groups run back to back on two
        # streams and the chip sees their sum. (Per group the even-fill rule picks the 8-wave kernel at cp = 8 with G >= 2, and loses the
        # no-running-max kernel with it: 478.8 against 425.7 ms per emulated step, profiles/cp_head_parallel_emulated.txt.)
        variant = self._variant(S_all, S_all, B, Hl) if q.is_cuda else 0
        self.effective = dict(schedule="head_parallel", kernel={11: "w4b", 4: "wave8"}.get(variant, str(variant)), head_groups=G)
        out = torch.empty((rows, H * 128), dtype=q.dtype, device=q.device)
        two_streams = q.is_cuda and G >= 2
        main = side = q_ready = None
        if two_streams:
            main = torch.cuda.current_stream(q.device)
            side = self._side_stream(q.device)
            q_ready = main.record_event()  # q, k, v (and `out`) were produced / allocated on the main stream

        def on_stream(g):
            return torch.cuda.stream(main if g % 2 == 0 else side) if two_streams else _NullCtx()

        # Lifetime contract (as in finish()): every send / receive buffer is read or written by the collective's own stream and by HIP kernels launched
        # through ctypes; `keep` references all of them until the last consumer - the gather of the last group - is enqueued.
        keep = []
        try:
            for g in range(G):
                with on_stream(g):
                    if two_streams and g % 2 == 1:
                        side.wait_event(q_ready)
                    qs, ks, vs = be["scatter_heads"](q, k, v, H, P, g * Hg, Hg)  # [P, rows, Hg*128] each: chunk p goes to rank p
                    kr, vr, qr = torch.empty_like(ks), torch.empty_like(vs), torch.empty_like(qs)  # rank-major = the global (s, b) row order
                    works = [self._all_to_all(kr, ks), self._all_to_all(vr, vs), self._all_to_all(qr, qs)]
                    self.bytes_gathered += 3 * (P - 1) * ks[0].numel() * ks.element_size()
                    keep.append([works, (qs, ks, vs), (qr, kr, vr)])
            for g in range(G):
                with on_stream(g):
                    (wk, wv, wq), _sent, (qr, kr, vr) = keep[g]
                    self._wait(be, g, wv)
                    vt = be["transpose_v"](vr.view(S_all * B, Hg * 128), S_all, B, Hg)  # plain V^T over all keys
                    self._wait(be, g, wk)
                    self._wait(be, g, wq)
                    ob = torch.empty_like(qr)  # [S_all*B, Hg*128] in row blocks of `rows`: already one chunk per destination rank
                    qa, ka, oa = (t.view(S_all * B, Hg * 128) for t in (qr, kr, ob))
                    if logit_bound > 0:
                        be["attention_bounded"](qa, ka, vt, S_all, S_all, B, Hg, logit_bound, oa, variant=variant, **(dict(mfma16=True) if self.mfma16 else {}))
                    else:
                        be["attention"](qa, ka, vt, S_all, S_all, B, Hg, oa, variant=variant)
                    orecv = torch.empty_like(ob)
                    wo = self._all_to_all(orecv, ob)
                    self.bytes_gathered += (P - 1) * ob[0].numel() * ob.element_size()
                    keep[g] += [vt, ob, orecv, wo]
            for g in range(G):
                with on_stream(g):
                    orecv, wo = keep[g][-2:]
                    self._wait(be, g, wo)
                    be["gather_heads"](orecv, out, H, g * Hg)  # chunk p: heads p * Hl + g * Hg .. of this rank's rows
        finally:
            if two_streams:
                main.wait_stream(side)
        del keep
        return out

    def finish(self, q: torch.Tensor, pending: dict, logit_bound: float = 0.0) -> torch.Tensor:
        """logit_bound > 0 (a caller's bound on |q . k| * softmax_scale, see ops.self_attn_bounded) is always used by "head_parallel". The other
        schedules shard a row's keys over launches; they use it when `bounded` is set, the layer's kernel is the one-wave-per-SIMD kernel (variant 11;
        a stub backend on CPU has no kernel choice) and the backend offers "attention_bounded_cp": then EVERY attention launch - gather_first's one,
        local_first's own-shard partial and both remote partials ahead of the unchanged merge, local_carry's own-shard partial and its carry launch
        with the skip - goes through that callable, and `effective_bounded` is True. Otherwise the launches are the unbounded ones, unchanged."""
        self.effective_bounded = False
        if pending.get("head_parallel"):
            return self._finish_head_parallel(q, pending, logit_bound)
        if pending.get("window_halo"):
            return self._finish_window_halo(q, pending, logit_bound)
        be, W, Hg, B, S_local = pending["be"], pending["W"], pending["Hg"], pending["B"], pending["S_local"]
        S_all = S_local * self.world
        out = torch.empty((pending["rows"], pending["H"] * 128), dtype=q.dtype, device=q.device)
        # Lifetime contract: the gathered buffers (kf, vf) and the packed send buffers (_ks, _vs) are consumed by RCCL on its own stream
        # and by HIP kernels launched through ctypes, which the caching allocator knows nothing about. They stay referenced by `pending`
        # (held by the caller's frame) until every attention launch below is enqueued on the compute stream; after that, stream order on
        # the compute stream protects them (a later allocation that reuses the memory is also enqueued there). Do not drop `pending`
        # entries inside this loop.
        assert all(len(w) == 6 and w[2] is not None and w[3] is not None for w in pending["works"]), "gathered K / V buffers must stay referenced"
        works = pending["works"]
        variant = self._variant(S_local, S_all, B, pending["H"]) if q.is_cuda else 0
        split = pending["segmented"] and self.world > 1
        use_bound = self.bounded and logit_bound > 0 and "attention_bounded_cp" in be and (variant == 11 or not q.is_cuda)
        self.effective_bounded = bool(use_bound)
        if use_bound:  # the same launches with the bound: one callable stands in for the three unbounded ones
            bcp = be["attention_bounded_cp"]
            attention = lambda q_, k_, vt_, Sq, Skv, B_, H_, out_, variant=0: bcp(q_, k_, vt_, Sq, Skv, B_, H_, logit_bound, out=out_, variant=variant)
            attention_partial = lambda q_, k_, vt_, Sq, Skv, B_, H_, variant=0: bcp(q_, k_, vt_, Sq, Skv, B_, H_, logit_bound, partial=True, variant=variant)
            attention_carry = lambda q_, k_, vt_, Sq, Skv, B_, H_, out=None, carry=None, kv_skip=None, partial=False, variant=0: bcp(
                q_, k_, vt_, Sq, Skv, B_, H_, logit_bound, out=out, carry=carry, kv_skip=kv_skip, partial=partial, variant=variant)
        else:
            attention, attention_partial, attention_carry = be["attention"], be.get("attention_partial"), be.get("attention_carry")
        local_carry = self.schedule == "local_carry" and split and "attention_carry" in be
        # (a "head_parallel" request that start() could not honour - H % world != 0, a backend without the exchange callables - runs as local_first)
        local_first = not local_carry and self.schedule in ("local_first", "local_carry", "head_parallel") and split and "attention_partial" in be
        # what this layer actually runs (a requested "local_first" needs segmented V^T and a split-KV backend; a forced one-wave kernel needs
        # S_all % 64 == 0): read by bench.py so that its autotune table and `cp.chosen` never label a fallback with the requested name
        self.effective = dict(schedule="local_carry" if local_carry else "local_first" if local_first else "gather_first",
                              kernel={11: "w4b", 4: "wave8"}.get(variant, str(variant)), head_groups=len(pending["works"]))
        # local_carry: the phase-1 partials of all groups in ONE fp32 buffer shaped like `out`, so that a group's partial has the strides of its
        # bf16 output columns (the carry-in form reads carry_o with the output's strides). Allocated here, before q_ready, like `out`.
        o32 = torch.empty((pending["rows"], pending["H"] * 128), dtype=torch.float32, device=q.device) if local_carry else None
        two_streams = q.is_cuda and len(works) >= 2
        main = side = q_ready = None
        if two_streams:
            # The groups are independent, so odd groups go to a second stream: the next group's workgroups fill the CUs the previous launch has drained.
            main = torch.cuda.current_stream(q.device)
            side = self._side_stream(q.device)
            q_ready = main.record_event()

        def on_stream(g):
            st = main if (not two_streams or g % 2 == 0) else side
            ctx = torch.cuda.stream(st) if two_streams else _NullCtx()
            return st, ctx

        try:
            local_parts = {}
            if local_carry:
                # phase 1: as local_first, into this group's columns of o32 (the partial stays referenced by local_parts until phase 2 is enqueued)
                for g, (wk, wv, kf, vf, ks, vs) in enumerate(works):
                    st, ctx = on_stream(g)
                    with ctx:
                        if two_streams and st is side:
                            st.wait_event(q_ready)
                        local_parts[g] = attention_carry(q[:, g * W:(g + 1) * W], ks, vs.reshape(1, B, Hg, 128, -1), S_local, S_local, B, Hg,
                                                               out=o32[:, g * W:(g + 1) * W], partial=True, variant=variant)
            elif local_first:
                # phase 1: every group over this rank's own shard - the packed K columns and the local V^T that were SENT (w[4], w[5]); no wait
                for g, (wk, wv, kf, vf, ks, vs) in enumerate(works):
                    st, ctx = on_stream(g)
                    with ctx:
                        if two_streams and st is side:
                            st.wait_event(q_ready)  # q (and `out`) were produced / allocated on the main stream
                        local_parts[g] = attention_partial(q[:, g * W:(g + 1) * W], ks, vs.reshape(1, B, Hg, 128, -1), S_local, S_local, B, Hg, variant=variant)
            for g, (wk, wv, kf, vf, _ks, _vs) in enumerate(works):
                st, ctx = on_stream(g)
                with ctx:
                    if two_streams and st is side and not (local_first or local_carry):
                        st.wait_event(q_ready)
                    self._wait(be, g, wk, wv)
                    qg, og = q[:, g * W:(g + 1) * W], out[:, g * W:(g + 1) * W]
                    if local_carry:
                        # phase 2: every remote key in one launch that resumes from the phase-1 state. Rank 0 / the last rank: the remote blocks
                        # are contiguous (a sub-range of the gathered buffers); an interior rank skips its own block (whole V^T segments).
                        vseg = vf.view(self.world, B, Hg, 128, -1)
                        rows, r = pending["rows"], self.rank
                        S_rem = (self.world - 1) * S_local
                        if r == 0:
                            kk, vv, skip = kf[rows:], vseg[1:], None
                        elif r == self.world - 1:
                            kk, vv, skip = kf[:r * rows], vseg[:r], None
                        else:
                            kk, vv, skip = kf, vseg, (r * S_local, S_local)
                        attention_carry(qg, kk, vv, S_local, S_rem, B, Hg, out=og, carry=local_parts[g], kv_skip=skip, variant=variant)
                    elif local_first:
                        # phase 2: the other ranks' keys = the row blocks / V^T segments before and after this rank's in the gathered buffers
                        parts = [local_parts[g]]
                        vseg = vf.view(self.world, B, Hg, 128, -1)
                        rows = pending["rows"]
                        for (r0, r1) in ((0, self.rank), (self.rank + 1, self.world)):
                            if r1 > r0:
                                parts.append(attention_partial(qg, kf[r0 * rows:r1 * rows], vseg[r0:r1], S_local, (r1 - r0) * S_local, B, Hg, variant=variant))
                        be["merge"](parts, S_local, B, Hg, og)
                    else:
                        vt = vf.view(self.world, B, Hg, 128, -1) if pending["segmented"] else be["transpose_v"](vf, S_all, B, Hg)
                        attention(qg, kf, vt, S_local, S_all, B, Hg, og, variant=variant)
        finally:
            if two_streams:
                main.wait_stream(side)  # everything enqueued on the main stream from here on (out-projection, buffer reuse) follows both streams
        return out

    def _side_stream(self, device):
        st = getattr(self, "_side", None)
        if st is None or st.device != device:
            st = self._side = torch.cuda.Stream(device=device)
        return st

    def __call__(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, S_local: int, B: int, H: int, logit_bound: float = 0.0) -> torch.Tensor:
        return self.finish(q, self.start(k, v, S_local, B, H), logit_bound)


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False
