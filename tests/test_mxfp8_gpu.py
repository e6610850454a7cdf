"""GPU: the opt-in MXFP8 DiT linears (g3_quant_mxfp8_bf16, g3_gemm_mxfp8_nt).

The quantiser must match the CPU reference (tests/mxfp8_ref.py) bit for bit. The GEMM is pinned two ways: on exact small-integer data, where
every partial sum is exact in fp32 and the bf16 output must be bitwise the RNE of the exact result (this fixes the scaled MFMA's lane and
scale maps), and at the DiT shapes against the bf16 product GEMM on the dequantised operands - every dequantised value is exactly a bf16
value, so the two differ only in summation order and in the scaled MFMA's accumulation, which is measured to be coarser than an fp32 fmaf
chain (up to ~2^-15 of the partial sums): about 2 % of the bf16 outputs differ by one ulp from the bf16 kernel's, not the < 1 % an fp32-exact
accumulation would give. The bars below are set on that measurement (97 % bitwise equal, rel-L2 <= 1e-3, no difference beyond
ulp + 2^-12 sum |a w|).
"""
import ctypes
import math

import pytest
import torch

from tests.mxfp8_ref import dequant_mxfp8, quant_mxfp8_ref

pytestmark = pytest.mark.gpu

D = 4096
# the six per-block linears: (name, N, K, epilogue)
CLASSES = [("fa_qkv", 3 * D, D, 0), ("fa_out", D, D, 2), ("ca_q", D, D, 0), ("ca_out", D, D, 2), ("w1", 4 * D, D, 1), ("w2", D, 4 * D, 2)]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _codes(q):
    return q.view(torch.uint8)


def _dequant_gpu(q, s):
    """Exact dequantisation on the GPU, as bf16 (exact for |X| <= 110)."""
    M, K = q.shape
    return (q.float().view(M, K // 32, 32) * torch.exp2(s.float() - 127.0).unsqueeze(-1)).view(M, K).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. quantiser
# ---------------------------------------------------------------------------------------------------------------------------------------

def _adversarial(M, K, g, dev):
    x = torch.randn(M, K, generator=g, device=dev)
    x[:, 3::97] *= 30.0  # outlier channels
    x[: M // 3] *= torch.exp2(torch.randint(-20, 20, (M // 3, 1), generator=g, device=dev).float())
    x[M // 3: M // 3 + 1, :64] = 0.0  # all-zero blocks
    x[M // 3 + 1, :32] = 1.875 * torch.exp2(torch.arange(32, device=dev).float() % 5)  # amax in (448, 512) * 2^X
    x[M // 3 + 2, :32] = 2.0 ** -133  # bf16 subnormal block
    x[M // 3 + 3, 32:64] = -(2.0 ** 120)
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("M,K,width", [(37, 256, 256), (300, 512, 640), (64, 4096, 4096), (129, 96, 104)])
def test_quant_bitwise_vs_reference(M, K, width):
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(M * 7 + K)
    full = _adversarial(M, width, g, dev)
    x = full[:, :K]  # ldx = width >= K
    q, s = ops.quant_mxfp8(x)
    torch.cuda.synchronize()
    rq, rs = quant_mxfp8_ref(x.cpu())
    assert torch.equal(s.cpu(), rs), "scale bytes differ"
    assert torch.equal(_codes(q).cpu(), _codes(rq)), "e4m3 codes differ"


@pytest.mark.parametrize("M", [14080, 112640])
def test_quant_bitwise_large_sampled(M):
    from gen3c_amd import ops
    dev = _dev()
    K = 4 * D
    g = torch.Generator(device=dev).manual_seed(M)
    x = (torch.randn(M, K, generator=g, device=dev) * 0.5).to(torch.bfloat16)
    x[:, 11::512] *= 30
    q, s = ops.quant_mxfp8(x)
    torch.cuda.synchronize()
    rows = torch.cat([torch.arange(4), torch.randint(0, M, (60,), generator=torch.Generator().manual_seed(M)), torch.tensor([M - 1])])
    rq, rs = quant_mxfp8_ref(x[rows.to(dev)].cpu())
    assert torch.equal(s[rows.to(dev)].cpu(), rs)
    assert torch.equal(_codes(q)[rows.to(dev)].cpu(), _codes(rq))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. lane and scale layout, exact
# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (64, 512, 128), (513, 256, 512)])
def test_gemm_exact_small_integers(M, N, K):
    """e4m3 small integers in [-4, 4] with scale bytes 127 + [-2, 2] that differ per (row, block) on both operands (an asymmetric W):
    every product is a multiple of 2^-4 below 2^4 * 2^4, every partial sum below 2^20 * 2^-4 - exact in fp32 in any order."""
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-4, 5, (M, K), generator=g).float()
    w = torch.randint(-4, 5, (N, K), generator=g).float()
    w[:, 0] += torch.arange(N).float() % 3  # no symmetry between rows / columns
    w = w.clamp(-4, 4)
    sa = (127 + torch.randint(-2, 3, (M, K // 32), generator=g)).to(torch.uint8)
    sw = (127 + torch.randint(-2, 3, (N, K // 32), generator=g)).to(torch.uint8)
    aq, wq = a.to(torch.float8_e4m3fn), w.to(torch.float8_e4m3fn)
    exact = dequant_mxfp8(aq, sa).double() @ dequant_mxfp8(wq, sw).double().T
    ref = exact.float().to(torch.bfloat16)
    got = ops.gemm_mxfp8_nt(aq.to(dev), sa.to(dev), wq.to(dev), sw.to(dev))
    torch.cuda.synchronize()
    got = got.cpu()
    bad = (got.view(torch.int16) != ref.view(torch.int16)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {M * N} outputs differ, first at {bad[:4].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. against the bf16 product GEMM on dequantised operands
# ---------------------------------------------------------------------------------------------------------------------------------------

def _ulp(x):
    """bf16 ulp at |x| (fp32 tensor)."""
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def _compare(got, ref, tol_ulps, name):
    g32, r32 = got.float(), ref.float()
    diff = (g32 - r32).abs()
    equal = float((got.view(torch.int16) == ref.view(torch.int16)).float().mean())
    rel = float((g32 - r32).norm() / r32.norm())
    worst = float((diff / tol_ulps).max())
    print(f"[{name}] bitwise-equal {equal:.5f} rel_l2 {rel:.2e} worst diff / allowed {worst:.3f}")
    assert worst <= 1.0, f"{name}: a difference beyond the allowed bound"
    assert equal >= 0.97, f"{name}: only {equal:.4f} of the outputs bitwise equal"
    assert rel <= 1e-3, f"{name}: rel-L2 {rel:.2e}"


def _operands(M, N, K, seed, dev):
    from gen3c_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
    a[:, 5::613] *= 30
    w = (torch.randn(N, K, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    aq, as_ = ops.quant_mxfp8(a)
    del a
    wq, ws = ops.quant_mxfp8(w)
    gate = (torch.rand(2, N, generator=g, device=dev) + 0.1).to(torch.bfloat16)
    res = torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16)
    return aq, as_, wq, ws, gate, res


def _check_class(M, N, K, epis, seed, inplace=False):
    from gen3c_amd import ops
    dev = _dev()
    aq, as_, wq, ws, gate, res = _operands(M, N, K, seed, dev)
    ad, wd = _dequant_gpu(aq, as_), _dequant_gpu(wq, ws)
    lin_ref = ops.gemm_nt(ad, wd)  # the Linear's own bf16 output: the scale of its 1-ulp freedom
    # the scaled MFMA's own accumulation error: measured at up to ~2^-15 of the partial sums (not the 2^-24 of an fp32 fmaf chain), so an
    # output near zero or near a bf16 rounding midpoint may differ by more than its ulp; bound it by 2^-12 sum_k |a_k w_k|
    acc_err = ops.gemm_nt(ad.abs(), wd.abs()).float() * 2.0 ** -12
    for epi in epis:
        kw = dict(gate=gate, residual=res) if epi == 2 else {}
        ref = ops.gemm_nt(ad, wd, epilogue=epi, **kw)
        if epi == 2 and inplace:
            out = res.clone()
            got = ops.gemm_mxfp8_nt(aq, as_, wq, ws, out=out, epilogue=2, gate=gate, residual=out)
        else:
            got = ops.gemm_mxfp8_nt(aq, as_, wq, ws, epilogue=epi, **kw)
        torch.cuda.synchronize()
        # 1 bf16 ulp of the result, plus what 1 ulp of the Linear's output becomes through the epilogue (GELU' <= 1.13; gate * ulp)
        tol = _ulp(ref.float()) + acc_err
        if epi == 1:
            tol = tol + 1.13 * _ulp(lin_ref.float())
        elif epi == 2:
            rows = torch.arange(M, device=dev) % gate.shape[0]
            tol = tol + gate.float()[rows] * (_ulp(lin_ref.float()) + acc_err)
        _compare(got, ref, tol, f"M={M} N={N} K={K} epi={epi}{' in place' if inplace else ''}")
        del got, ref


@pytest.mark.parametrize("M", [14080, 112640])
@pytest.mark.parametrize("name,N,K,epi", CLASSES)
def test_gemm_vs_bf16_product_kernel(M, name, N, K, epi):
    _check_class(M, N, K, [epi], seed=M + N + K + epi, inplace=(epi == 2 and name == "fa_out"))


def test_gemm_every_epilogue_with_row_tail():
    _check_class(14080 + 77, D, D, [0, 1, 2], seed=5)
    _check_class(14080 + 77, D, D, [2], seed=6, inplace=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from gen3c_amd import _lib
    lib = _lib.load()
    dev = _dev()
    M, N, K = 256, 512, 512
    aq = torch.zeros(M, K + 64, dtype=torch.uint8, device=dev)
    wq = torch.zeros(N + 256, K + 64, dtype=torch.uint8, device=dev)
    sa = torch.full((M, 64), 127, dtype=torch.uint8, device=dev)
    sw = torch.full((N + 256, 64), 127, dtype=torch.uint8, device=dev)
    c = torch.full((M, N + 256), 7.0, dtype=torch.bfloat16, device=dev)
    gate = torch.ones(1, N + 256, dtype=torch.bfloat16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(aq_p=None, lda=K + 64, as_p=None, ldas=64, wq_p=None, ldw=K + 64, ldws=64, n=N, k=K, epi=0, ldc=N + 256, c_p=None, gate_p=None, res_p=None):
        return lib.g3_gemm_mxfp8_nt(aq_p or aq.data_ptr(), lda, as_p or sa.data_ptr(), ldas, wq_p or wq.data_ptr(), ldw, sw.data_ptr(), ldws,
                                    c_p or c.data_ptr(), ldc, M, n, k, epi, gate_p or 0, 1, N + 256, res_p or 0, N + 256, stream)

    cases = {
        "K not a multiple of 128": dict(k=K + 32),
        "N not a multiple of 256": dict(n=N + 128),
        "misaligned activations": dict(aq_p=aq.data_ptr() + 8),
        "misaligned weights": dict(wq_p=wq.data_ptr() + 4),
        "misaligned scales": dict(as_p=sa.data_ptr() + 2),
        "short activation scale stride": dict(ldas=K // 32 - 4),
        "short weight scale stride": dict(ldws=K // 32 - 4),
        "odd scale stride": dict(ldas=17),
        "short lda": dict(lda=K - 16),
        "misaligned C": dict(c_p=c.data_ptr() + 8),
        "unknown epilogue": dict(epi=3),
        "gated residual without operands": dict(epi=2),
        "gated residual, misaligned gate": dict(epi=2, gate_p=gate.data_ptr() + 2, res_p=c.data_ptr()),
    }
    # a short gate stride with more than one gate row
    rc = lib.g3_gemm_mxfp8_nt(aq.data_ptr(), K + 64, sa.data_ptr(), 64, wq.data_ptr(), K + 64, sw.data_ptr(), 64, c.data_ptr(), N + 256, M, N, K, 2,
                              gate.data_ptr(), 2, N - 8, c.data_ptr(), N + 256, stream)
    assert rc == _lib.G3_ERR_ARG and "gated-residual" in _lib.last_error(), "short gate stride"
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == _lib.G3_ERR_ARG, f"{what}: rc {rc}"
        assert _lib.last_error().startswith("g3_gemm_mxfp8_nt"), what
    torch.cuda.synchronize()
    assert bool((c == 7.0).all()), "a refused call wrote C"
    assert call() == _lib.G3_OK  # the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert bool((c[:, :N] == 0).all()) and bool((c[:, N:] == 7.0).all())
    assert lib.g3_gemm_mxfp8_kernel_name(M, N + 128, K, 0) is None
    assert [lib.g3_gemm_mxfp8_kernel_name(M, N, K, e) for e in (0, 1, 2)] == [b"gemm_mxfp8_nt_kernel<%d>" % e for e in (0, 1, 2)]
    assert lib.g3_gemm_mxfp8_kernel_name(M, N, K, 3) is None

    x = torch.zeros(M, 96, dtype=torch.bfloat16, device=dev)
    q = torch.zeros(M, 128, dtype=torch.uint8, device=dev)
    s = torch.zeros(M, 4, dtype=torch.uint8, device=dev)
    assert lib.g3_quant_mxfp8_bf16(x.data_ptr(), 96, q.data_ptr(), 128, s.data_ptr(), 4, M, 80, stream) == _lib.G3_ERR_ARG  # K % 32
    assert lib.g3_quant_mxfp8_bf16(x.data_ptr() + 2, 96, q.data_ptr(), 128, s.data_ptr(), 4, M, 64, stream) == _lib.G3_ERR_ARG
    assert lib.g3_quant_mxfp8_bf16(x.data_ptr(), 96, q.data_ptr(), 128, s.data_ptr(), 1, M, 64, stream) == _lib.G3_ERR_ARG  # lds < K/32
    torch.cuda.synchronize()
    assert bool((q == 0).all()) and bool((s == 0).all())
