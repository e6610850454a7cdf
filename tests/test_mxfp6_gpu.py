"""GPU: the opt-in MXFP6 DiT linears (g3_quant_mxfp6_bf16, g3_gemm_mxfp6_nt).

The quantiser must match the CPU reference (tests/mxfp6_ref.py) bit for bit, codes and scale bytes. The GEMM is pinned two ways: on e2m3-exact
data, where every product and partial sum is exact in fp32 and the bf16 output must be bitwise the RNE of the fp64 result (this fixes the scaled
MFMA's lane, bit and scale maps for 6-bit operands), and at the DiT classes against the bf16 product GEMM on the dequantised operands - every
dequantised value is exactly a bf16 value, so the two differ only in summation order and in the scaled MFMA's accumulation. The bars are the
MXFP8 test's three (share of bitwise-equal outputs >= 0.97, rel-L2 <= 1e-3, no difference beyond ulp + 2^-12 sum |a w|). Measured on e2m3
operands (tools/mxfp8_ab.py --accum, profiles/r9_mxfp6_ab.txt): against exact fp64 sums 100.000 % of the MXFP6 GEMM's bf16 outputs are the
correctly rounded value (MXFP8: 97.8 %), and every class below came out bitwise equal to the bf16 product GEMM - the 8-bit products of two
4-bit significands leave the accumulation no visible error at these K. The measured share is not lower than 0.97, so the bar stays there.
"""
import pytest
import torch

from tests.mxfp6_ref import dequant_mxfp6, e2m3_encode, e2m3_values, pack_e2m3, quant_mxfp6_ref
from tests.test_mxfp8_gpu import CLASSES, D, _ulp

pytestmark = pytest.mark.gpu

# Share of outputs bitwise equal to the bf16 product kernel's: the MXFP8 test's 0.97; the measured share on 6-bit operands is 1.00000
# (profiles/r9_mxfp6_ab.txt), which does not lower it.
EQUAL_SHARE = 0.97


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _dequant_gpu(q, s):
    """Exact dequantisation of a packed MXFP6 matrix on the GPU, as bf16 (exact for |X| <= 120), in row chunks."""
    M, B = q.shape
    K = B // 3 * 4
    out = torch.empty(M, K, dtype=torch.bfloat16, device=q.device)
    table = e2m3_values().float().to(q.device)
    for r0 in range(0, M, 8192):
        b = q[r0:r0 + 8192].reshape(-1, B // 3, 3).to(torch.int32)
        v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
        codes = torch.stack([(v >> (6 * i)) & 63 for i in range(4)], dim=-1).reshape(-1, K // 32, 32)
        out[r0:r0 + 8192] = (table[codes.long()] * torch.exp2(s[r0:r0 + 8192].float() - 127.0).unsqueeze(-1)).reshape(-1, K).to(torch.bfloat16)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. quantiser
# ---------------------------------------------------------------------------------------------------------------------------------------

def _adversarial(M, K, g, dev):
    """The generator pattern of tests/test_mxfp8_gpu.py, with the saturating block moved to e2m3's range: amax 31 = 7.75 * 2^2."""
    x = torch.randn(M, K, generator=g, device=dev)
    x[:, 3::97] *= 30.0  # outlier channels
    x[: M // 3] *= torch.exp2(torch.randint(-20, 20, (M // 3, 1), generator=g, device=dev).float())
    x[M // 3: M // 3 + 1, :64] = 0.0  # all-zero blocks
    x[M // 3 + 1, :32] = 1.9375 * torch.exp2(torch.arange(32, device=dev).float() % 5)  # scaled amax 7.75 in (7.5, 8): saturates, a tie that must not become 8
    x[M // 3 + 2, :32] = 2.0 ** -133  # bf16 subnormal block
    x[M // 3 + 3, 32:64] = -(2.0 ** 120)
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("M,K,width", [(37, 256, 256), (300, 512, 640), (129, 96, 104)])
def test_quant_bitwise_vs_reference(M, K, width):
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(M * 7 + K)
    full = _adversarial(M, width, g, dev)
    x = full[:, :K]  # ldx = width >= K
    q, s = ops.quant_mxfp6(x)
    torch.cuda.synchronize()
    assert q.shape == (M, K // 4 * 3) and q.dtype == torch.uint8 and s.shape == (M, K // 32)
    rq, rs = quant_mxfp6_ref(x.cpu())
    sat = x[M // 3 + 1, :32].float().cpu()
    assert 7.5 < float(sat.abs().max()) / 4.0 < 8.0  # the block this pattern adds for e2m3
    assert torch.equal(s.cpu(), rs), "scale bytes differ"
    assert torch.equal(q.cpu(), rq), "e2m3 codes differ"
    # into a wider buffer: ldq > 3K/4, and nothing outside [M, 3K/4] is written
    qb = torch.full((M, K // 4 * 3 + 16), 0xAB, dtype=torch.uint8, device=dev)
    sb = torch.full((M, K // 32 + 3), 0xCD, dtype=torch.uint8, device=dev)
    ops.quant_mxfp6(x, out=(qb[:, : K // 4 * 3], sb[:, : K // 32]))
    torch.cuda.synchronize()
    assert torch.equal(qb[:, : K // 4 * 3].cpu(), rq) and bool((qb[:, K // 4 * 3:] == 0xAB).all())
    assert torch.equal(sb[:, : K // 32].cpu(), rs) and bool((sb[:, K // 32:] == 0xCD).all())


def test_quant_bitwise_large_sampled():
    """M = 112 640, K = 16 384: the one shape whose byte offsets pass 2^31 (x: 3.7e9 bytes; q, at 1.38e9 bytes, stays below it)."""
    from gen3c_amd import ops
    dev = _dev()
    M, K = 112640, 4 * D
    g = torch.Generator(device=dev).manual_seed(M)
    x = (torch.randn(M, K, generator=g, device=dev) * 0.5).to(torch.bfloat16)
    x[:, 11::512] *= 30
    q, s = ops.quant_mxfp6(x)
    torch.cuda.synchronize()
    rows = torch.cat([torch.arange(4), torch.randint(0, M, (60,), generator=torch.Generator().manual_seed(M)), torch.tensor([M - 1])])
    rq, rs = quant_mxfp6_ref(x[rows.to(dev)].cpu())
    assert torch.equal(s[rows.to(dev)].cpu(), rs)
    assert torch.equal(q[rows.to(dev)].cpu(), rq)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. lane, bit and scale maps, exact
# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (64, 512, 128), (1100, 768, 512)])
def test_gemm_exact_e2m3_values(M, N, K):
    """e2m3-exact operands: integers in [-7, 7]; in the columns k = 1 mod 5 of A and k = 3 mod 5 of W multiples of 1/8 below 1 instead (all
    three mantissa bits and the subnormals carry information; no fraction meets a fraction). Scale bytes 127 + [-2, 2] differ per (row, block)
    on both operands; W is made asymmetric. Every product is a multiple of 2^-3 2^-4 = 2^-7, and sum_k |a w| is checked below to stay under
    2^24 2^-7 = 2^17, so every partial sum is exact in fp32 in any order and the bf16 output must be bitwise the RNE of the fp64 result."""
    from gen3c_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-7, 8, (M, K), generator=g).double()
    w = torch.randint(-7, 8, (N, K), generator=g).double()
    a[:, 1::5] = torch.randint(-7, 8, (M, len(range(1, K, 5))), generator=g).double() / 8
    w[:, 3::5] = torch.randint(-7, 8, (N, len(range(3, K, 5))), generator=g).double() / 8
    w[:, 0] += (torch.arange(N) % 3).double()  # no symmetry between rows / columns
    w = w.clamp(-7, 7)
    sa = (127 + torch.randint(-2, 3, (M, K // 32), generator=g)).to(torch.uint8)
    sw = (127 + torch.randint(-2, 3, (N, K // 32), generator=g)).to(torch.uint8)
    aq, wq = pack_e2m3(e2m3_encode(a)), pack_e2m3(e2m3_encode(w))
    ad, wd = dequant_mxfp6(aq, sa).double(), dequant_mxfp6(wq, sw).double()
    assert torch.equal(ad.reshape(M, K // 32, 32), a.reshape(M, K // 32, 32) * torch.exp2(sa.double() - 127).unsqueeze(-1))  # the codes are exact
    assert float((ad.abs() @ wd.abs().T).max()) < 2.0 ** 17  # the premise: exact in fp32 in any order
    ref = (ad @ wd.T).float().to(torch.bfloat16)
    got = ops.gemm_mxfp6_nt(aq.to(dev), sa.to(dev), wq.to(dev), sw.to(dev))
    torch.cuda.synchronize()
    got = got.cpu()
    bad = (got.view(torch.int16) != ref.view(torch.int16)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {M * N} outputs differ, first at {bad[:4].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. against the bf16 product GEMM on dequantised operands
# ---------------------------------------------------------------------------------------------------------------------------------------

def _compare(got, ref, tol_ulps, name):
    g32, r32 = got.float(), ref.float()
    diff = (g32 - r32).abs()
    equal = float((got.view(torch.int16) == ref.view(torch.int16)).float().mean())
    rel = float((g32 - r32).norm() / r32.norm())
    worst = float((diff / tol_ulps).max())
    print(f"[{name}] bitwise-equal {equal:.5f} rel_l2 {rel:.2e} worst diff / allowed {worst:.3f}")
    assert worst <= 1.0, f"{name}: a difference beyond the allowed bound"
    assert equal >= EQUAL_SHARE, f"{name}: only {equal:.4f} of the outputs bitwise equal"
    assert rel <= 1e-3, f"{name}: rel-L2 {rel:.2e}"


def _operands(M, N, K, seed, dev):
    from gen3c_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
    a[:, 5::613] *= 30
    w = (torch.randn(N, K, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    aq, as_ = ops.quant_mxfp6(a)
    del a
    wq, ws = ops.quant_mxfp6(w)
    gate = (torch.rand(2, N, generator=g, device=dev) + 0.1).to(torch.bfloat16)
    res = torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16)
    return aq, as_, wq, ws, gate, res


def _check_class(M, N, K, epis, seed, inplace=False):
    from gen3c_amd import ops
    dev = _dev()
    aq, as_, wq, ws, gate, res = _operands(M, N, K, seed, dev)
    ad, wd = _dequant_gpu(aq, as_), _dequant_gpu(wq, ws)
    lin_ref = ops.gemm_nt(ad, wd)  # the Linear's own bf16 output: the scale of its 1-ulp freedom
    acc_err = ops.gemm_nt(ad.abs(), wd.abs()).float() * 2.0 ** -12  # the scaled MFMA's own accumulation error, bounded as in the MXFP8 test
    for epi in epis:
        kw = dict(gate=gate, residual=res) if epi == 2 else {}
        ref = ops.gemm_nt(ad, wd, epilogue=epi, **kw)
        if epi == 2 and inplace:
            out = res.clone()
            got = ops.gemm_mxfp6_nt(aq, as_, wq, ws, out=out, epilogue=2, gate=gate, residual=out)
        else:
            got = ops.gemm_mxfp6_nt(aq, as_, wq, ws, epilogue=epi, **kw)
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


@pytest.mark.parametrize("name,N,K,epi", CLASSES)
def test_gemm_vs_bf16_product_kernel(name, N, K, epi):
    """M = 577: two token tiles and a 65-row tail."""
    _check_class(577, N, K, [epi], seed=577 + N + K + epi, inplace=(epi == 2 and name == "fa_out"))


def test_gemm_every_epilogue_with_row_tail():
    _check_class(577, D, D, [0, 1, 2], seed=5)
    _check_class(577, D, D, [2], seed=6, inplace=True)


def test_gemm_w2_class_full_size():
    """The longest K loop and the largest operand: w2 at M = 112 640."""
    _check_class(112640, D, 4 * D, [2], seed=112640)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from gen3c_amd import _lib
    lib = _lib.load()
    dev = _dev()
    M, N, K = 256, 512, 512
    KB = K // 4 * 3  # packed row bytes
    aq = torch.zeros(M, KB + 64, dtype=torch.uint8, device=dev)
    wq = torch.zeros(N + 256, KB + 64, dtype=torch.uint8, device=dev)
    sa = torch.full((M, 64), 127, dtype=torch.uint8, device=dev)
    sw = torch.full((N + 256, 64), 127, dtype=torch.uint8, device=dev)
    c = torch.full((M, N + 256), 7.0, dtype=torch.bfloat16, device=dev)
    gate = torch.ones(1, N + 256, dtype=torch.bfloat16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(aq_p=None, lda=KB + 64, as_p=None, ldas=64, wq_p=None, ldw=KB + 64, ldws=64, n=N, k=K, epi=0, ldc=N + 256, c_p=None, gate_p=None,
             res_p=None, null_a=False):
        return lib.g3_gemm_mxfp6_nt(0 if null_a else (aq_p or aq.data_ptr()), lda, as_p or sa.data_ptr(), ldas, wq_p or wq.data_ptr(), ldw,
                                    sw.data_ptr(), ldws, c_p or c.data_ptr(), ldc, M, n, k, epi, gate_p or 0, 1, N + 256, res_p or 0, N + 256, stream)

    cases = {
        "K not a multiple of 128": dict(k=640 - 96),
        "N not a multiple of 256": dict(n=N + 128),
        "activations off by 8 bytes": dict(aq_p=aq.data_ptr() + 8),
        "weights off by 4 bytes": dict(wq_p=wq.data_ptr() + 4),
        "scales off by 2 bytes": dict(as_p=sa.data_ptr() + 2),
        "lda < 3K/4": dict(lda=KB - 16),
        "null operand": dict(null_a=True),
        "unknown epilogue": dict(epi=3),
        "gated residual without a gate": dict(epi=2, res_p=c.data_ptr()),
        "short activation scale stride": dict(ldas=K // 32 - 4),
        "misaligned C": dict(c_p=c.data_ptr() + 8),
        "gated residual, misaligned gate": dict(epi=2, gate_p=gate.data_ptr() + 2, res_p=c.data_ptr()),
    }
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == _lib.G3_ERR_ARG, f"{what}: rc {rc}"
        assert _lib.last_error().startswith("g3_gemm_mxfp6_nt"), what
    torch.cuda.synchronize()
    assert bool((c == 7.0).all()), "a refused call wrote C"
    assert call() == _lib.G3_OK  # the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert bool((c[:, :N] == 0).all()) and bool((c[:, N:] == 7.0).all())
    assert lib.g3_gemm_mxfp6_kernel_name(M, N + 128, K, 0) is None
    assert [lib.g3_gemm_mxfp6_kernel_name(M, N, K, e) for e in (0, 1, 2)] == [b"gemm_mxfp6_nt_kernel<%d>" % e for e in (0, 1, 2)]
    assert lib.g3_gemm_mxfp6_kernel_name(M, N, K, 3) is None

    x = torch.zeros(M, 96, dtype=torch.bfloat16, device=dev)
    q = torch.zeros(M, 128, dtype=torch.uint8, device=dev)
    s = torch.zeros(M, 4, dtype=torch.uint8, device=dev)
    assert lib.g3_quant_mxfp6_bf16(x.data_ptr(), 96, q.data_ptr(), 128, s.data_ptr(), 4, M, 80, stream) == _lib.G3_ERR_ARG  # K % 32
    assert lib.g3_quant_mxfp6_bf16(x.data_ptr() + 2, 96, q.data_ptr(), 128, s.data_ptr(), 4, M, 64, stream) == _lib.G3_ERR_ARG
    assert lib.g3_quant_mxfp6_bf16(x.data_ptr(), 96, q.data_ptr(), 40, s.data_ptr(), 4, M, 64, stream) == _lib.G3_ERR_ARG  # ldq < 3K/4
    assert lib.g3_quant_mxfp6_bf16(x.data_ptr(), 96, q.data_ptr(), 128, s.data_ptr(), 1, M, 64, stream) == _lib.G3_ERR_ARG  # lds < K/32
    torch.cuda.synchronize()
    assert bool((q == 0).all()) and bool((s == 0).all())
