"""csrc/embed.hip at kernel level. Patchify and unpatchify are pure data movement and must equal the torch view / permute expressions they replace
(general_dit_video_conditioned.py:77-101 torch.cat + blocks.py:154-159 Rearrange "b c (t r) (h m) (w n) -> b t h w (c r m n)" in (t h w b) row
order; general_dit.py:348-357 "(B T) (H W) (p1 p2 t C) -> B C (T t) (H p1) (W p2)") at both temporal patch sizes, with every kind of source list,
past the grid cap of 8192 blocks x 256 threads, and from a row-padded matrix. The timestep embedding (blocks.py:38-57, general_dit.py:173-177)
is judged against fp64, stage by stage, and may disagree with the rounded fp64 value no more often than torch's own fp32 evaluation does."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
GRID_CAP = 8192 * 256
PATCHES = [(1, 2), (2, 2), (2, 1), (1, 1)]                     # (patch_t, patch_s)
SHAPES = [(1, 2, 2, 2), (3, 4, 6, 10), (2, 2, 66, 98)]         # (B, T, H, W); the last one passes the grid cap with the network's 82 channels
# source lists as (channels, has_t): 1, 2 and 4 entries, a 4-D source (broadcast over T) first and last
SOURCE_LISTS = {
    "one": [(16, True)],
    "two_broadcast_first": [(2, False), (3, True)],
    "two_broadcast_last": [(3, True), (2, False)],
    "four_network": [(16, True), (1, True), (64, True), (1, False)],   # x, input mask, pose, padding mask
    "four_broadcast_first": [(2, False), (5, True), (1, True), (3, True)],
}


def _dev():
    return torch.device("cuda:0")


def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(bf16).to(_dev())


def _patchify_case(shape, patch, sources, seed):
    from gen3c_amd import ops
    (B, T, H, W), (pt, ps) = shape, patch
    g = torch.Generator().manual_seed(seed)
    src = [(_rand(g, B, c, T, H, W) if ht else _rand(g, B, c, H, W), ht) for c, ht in sources]
    got = ops.dit_patchify(src, B, T, H, W, pt, ps)
    cat = torch.cat([t if ht else t[:, :, None].expand(B, t.shape[1], T, H, W) for t, ht in src], dim=1)
    Tp, Hp, Wp = T // pt, H // ps, W // ps
    ref = cat.view(B, -1, Tp, pt, Hp, ps, Wp, ps).permute(2, 4, 6, 0, 1, 3, 5, 7).reshape(Tp * Hp * Wp * B, -1)
    assert got.shape == ref.shape and got.dtype == bf16
    assert torch.equal(got.view(torch.int16), ref.contiguous().view(torch.int16)), (shape, patch, sources)
    return got.numel()


@pytest.mark.parametrize("patch", PATCHES, ids=lambda p: f"pt{p[0]}ps{p[1]}")
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_patchify_equals_cat_and_rearrange(shape, patch):
    for k, (name, sources) in enumerate(SOURCE_LISTS.items()):
        _patchify_case(shape, patch, sources, seed=10 + k)


@pytest.mark.parametrize("patch", PATCHES, ids=lambda p: f"pt{p[0]}ps{p[1]}")
def test_patchify_past_the_grid_cap(patch):
    """2 * 2 * 66 * 98 * 82 = 2 121 504 elements > 2 097 152: every thread takes a second pass of the grid-stride loop or (the ragged tail) does not."""
    n = _patchify_case(SHAPES[2], patch, SOURCE_LISTS["four_network"], seed=3)
    assert GRID_CAP < n < 2 * GRID_CAP and n % 256 != 0


def _unpatchify_case(shape, patch, Co, pad, seed):
    """pad > 0: y is a column slice of a wider matrix (ldy = row width + 2 * pad), as when the final layer's output sits inside a larger buffer"""
    from gen3c_amd import ops
    (B, T, H, W), (pt, ps) = shape, patch
    Tp, Hp, Wp = T // pt, H // ps, W // ps
    rows, cols = Tp * Hp * Wp * B, ps * ps * pt * Co
    g = torch.Generator().manual_seed(seed)
    wide = _rand(g, rows, cols + 2 * pad)
    y = wide[:, pad:pad + cols]
    assert y.stride(0) == cols + 2 * pad
    got = ops.dit_unpatchify(y, B, Co, T, H, W, pt, ps)
    ref = y.reshape(Tp, Hp, Wp, B, ps, ps, pt, Co).permute(3, 7, 0, 6, 1, 4, 2, 5).reshape(B, Co, T, H, W)
    assert got.shape == ref.shape and got.dtype == bf16
    assert torch.equal(got.view(torch.int16), ref.contiguous().view(torch.int16)), (shape, patch, Co, pad)
    return got.numel()


@pytest.mark.parametrize("pad", [0, 5], ids=["dense", "ldy_wider_than_row"])
@pytest.mark.parametrize("patch", PATCHES, ids=lambda p: f"pt{p[0]}ps{p[1]}")
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_unpatchify_equals_rearrange(shape, patch, pad):
    for Co in (1, 3, 16):
        _unpatchify_case(shape, patch, Co, pad, seed=20 + Co)


@pytest.mark.parametrize("pad", [0, 5], ids=["dense", "ldy_wider_than_row"])
@pytest.mark.parametrize("patch", PATCHES, ids=lambda p: f"pt{p[0]}ps{p[1]}")
def test_unpatchify_past_the_grid_cap(patch, pad):
    n = _unpatchify_case(SHAPES[2], patch, 82, pad, seed=4)  # C_out = 82: 2 121 504 output elements, one ragged second pass
    assert GRID_CAP < n < 2 * GRID_CAP and n % 256 != 0


def test_patchify_and_unpatchify_refusals_name_their_entry_and_launch_nothing():
    import ctypes as C
    from gen3c_amd import _lib as L
    lib = L.load()
    dev = _dev()
    s = torch.cuda.current_stream().cuda_stream
    src = torch.zeros(4096, dtype=bf16, device=dev)   # large enough for every shape named below
    out = torch.full((4096,), float("nan"), dtype=bf16, device=dev)
    ptrs = lambda n: (C.c_void_p * n)(*([src.data_ptr()] * n))
    ints = lambda n, v: (C.c_int * n)(*([v] * n))
    pat, unp = "g3_dit_patchify_bf16", "g3_dit_unpatchify_bf16"
    calls = [
        (pat, lambda: lib.g3_dit_patchify_bf16(ptrs(1), ints(1, 2), ints(1, 1), 1, out.data_ptr(), 1, 3, 4, 4, 2, 2, s)),    # T % patch_t
        (pat, lambda: lib.g3_dit_patchify_bf16(ptrs(1), ints(1, 2), ints(1, 1), 1, out.data_ptr(), 1, 2, 3, 4, 1, 2, s)),    # H % patch_s
        (pat, lambda: lib.g3_dit_patchify_bf16(ptrs(5), ints(5, 1), ints(5, 1), 5, out.data_ptr(), 1, 2, 4, 4, 1, 2, s)),    # 5 sources
        (unp, lambda: lib.g3_dit_unpatchify_bf16(src.data_ptr(), 16, out.data_ptr(), 1, 2, 3, 4, 4, 2, 2, s)),               # T % patch_t
        (unp, lambda: lib.g3_dit_unpatchify_bf16(src.data_ptr(), 8, out.data_ptr(), 1, 2, 2, 3, 4, 1, 2, s)),                # H % patch_s
        (unp, lambda: lib.g3_dit_unpatchify_bf16(src.data_ptr(), 7, out.data_ptr(), 1, 2, 2, 4, 4, 1, 2, s)),                # ldy = 7 < 2 * 2 * 1 * 2
    ]
    for entry, call in calls:
        rc = call()
        assert rc != 0, entry
        assert entry in L.last_error(), (entry, L.last_error())
        with pytest.raises(L.Gen3cHipError, match=entry):
            L.check(rc, entry)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()), "a refused call wrote output"


# ---- timestep embedding -----------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """distance in bf16 steps between two finite bf16 tensors (ordered-integer view; +0 and -0 coincide)"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


@functools.lru_cache(maxsize=None)
def _timesteps():
    """every 0.25 ln sigma_i of the 35-step schedule as the sampler hands it to the network (rounded to bf16), plus 0.0: 36 values, fp32, CPU"""
    from gen3c_amd.sampler import EDMEulerScheduler
    sch = EDMEulerScheduler(sigma_max=80, sigma_min=0.0002, sigma_data=0.5)
    sch.set_timesteps(35)
    return torch.cat([sch.timesteps.to(bf16).float(), torch.zeros(1)])


def _to_bf16(x64):
    return x64.float().to(bf16)  # fp64 -> fp32 -> bf16: the first rounding moves the value by 2^-24 relative, far inside the ties of the second


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [2, 6, 256, 770, 4096])
def test_timestep_embedding_against_fp64(D, B):
    """Both outputs of g3_timestep_embedding_bf16 over the 36 timesteps, B at a time.
    t_sin: [cos | sin](t * exp(-ln(10000) * j / half)) in fp64, rounded to bf16. Every element within one bf16 ulp; the share of elements that differ
    at all at most twice the share at which torch's fp32 evaluation of blocks.py:38-57 on the device differs from the same fp64 values (at least 2
    elements allowed) - fp32 exp / cos / sin put a value on the other side of a bf16 tie now and then, for torch as for the kernel.
    emb: the affine RMSNorm of general_dit.py:173-177 in fp64 applied to the KERNEL'S OWN t_sin, so that this stage is judged alone; same two
    rules, against torch's fp32 evaluation on the same t_sin.
    Measured on an MI355X (differing elements of 36 * D; the same for B = 1 and 3): D = 2, 6, 256, 770: kernel 0, torch 0, for both outputs.
    D = 4096 (147 456 elements): t_sin kernel 3 (2.0e-5), torch 3 (2.0e-5); emb kernel 1 (6.8e-6), torch 0 - inside the floor of 2 elements.
    No element further than one ulp. Both counts are printed before each assertion."""
    from gen3c_amd import ops
    dev = _dev()
    ts = _timesteps().to(dev)
    g = torch.Generator().manual_seed(D)
    w = (1.0 + 0.1 * torch.randn(D, generator=g)).to(bf16).to(dev)
    got_sin, got_emb = [], []
    for k in range(0, ts.numel(), B):
        a, b = ops.timestep_embedding(ts[k:k + B].contiguous(), w, D)
        got_sin.append(a)
        got_emb.append(b)
    t_sin, emb = torch.cat(got_sin), torch.cat(got_emb)
    assert t_sin.shape == emb.shape == (ts.numel(), D) and t_sin.dtype == emb.dtype == bf16
    half = D // 2
    n = t_sin.numel()

    ang64 = ts.double()[:, None] * torch.exp(-math.log(10000) * torch.arange(half, dtype=f64, device=dev) / half)[None]
    ref_sin = _to_bf16(torch.cat([torch.cos(ang64), torch.sin(ang64)], dim=-1))
    expo = -math.log(10000) * torch.arange(half, dtype=f32, device=dev)       # blocks.py:41-51 in fp32 on the device
    expo = expo / (half - 0.0)
    ang32 = ts[:, None].float() * torch.exp(expo)[None, :]
    torch_sin = torch.cat([torch.cos(ang32), torch.sin(ang32)], dim=-1).to(bf16)
    d = _ulps(t_sin, ref_sin)
    n_kernel, n_torch = int((d != 0).sum()), int((_ulps(torch_sin, ref_sin) != 0).sum())
    print(f"t_sin D={D} B={B}: kernel differs from bf16(fp64) at {n_kernel} of {n} ({n_kernel / n:.2e}), torch fp32 at {n_torch} ({n_torch / n:.2e}), "
          f"max {int(d.max())} ulp")
    assert int(d.max()) <= 1
    assert n_kernel <= max(2, 2 * n_torch), (n_kernel, n_torch, n)  # measured at D = 4096: 3 <= max(2, 2 * 3)

    v64, w64 = t_sin.double(), w.double()
    ref_emb = _to_bf16(v64 * torch.rsqrt(v64.pow(2).mean(-1, keepdim=True) + 1e-6) * w64)
    v32 = t_sin.float()
    torch_emb = (v32 * torch.rsqrt(v32.pow(2).mean(-1, keepdim=True) + 1e-6) * w.float()).to(bf16)
    d = _ulps(emb, ref_emb)
    n_kernel, n_torch = int((d != 0).sum()), int((_ulps(torch_emb, ref_emb) != 0).sum())
    print(f"emb   D={D} B={B}: kernel differs from bf16(fp64) at {n_kernel} of {n} ({n_kernel / n:.2e}), torch fp32 at {n_torch} ({n_torch / n:.2e}), "
          f"max {int(d.max())} ulp")
    assert int(d.max()) <= 1
    assert n_kernel <= max(2, 2 * n_torch), (n_kernel, n_torch, n)  # measured at D = 4096: 1 <= max(2, 2 * 0)
