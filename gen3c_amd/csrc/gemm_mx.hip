// MXFP8 (OCP Microscaling Formats v1.0, e4m3 elements) quantisation and block GEMM for the opt-in low-precision DiT linears.
//
// Format (MXFP8 linears): a block is 32 consecutive elements along K of one row. Its shared exponent is
//   X = floor(log2(amax_block)) - 8, stored as the E8M0 byte X + 127 clamped to 0..254 (all-zero block: byte 127, elements 0),
// and every element is RNE(clamp(x / 2^X, -448, 448)) as OCP e4m3fn (not the MI300 fnuz variant). amax / 2^X lies in [256, 512), so the clamp
// matters and no element is ever flushed to more than the format's own subnormal step. A block that holds a NaN or an infinity leaves as the
// E8M0 NaN - byte 0xFF, zero elements -, which the scaled matrix core turns into NaN in every output that consumes the block (mx_quant.hpp).
//
// GEMM: C[M,N] = epi( sum_k (a 2^Xa)(w 2^Xw) ) on v_mfma_scale_f32_32x32x64_f8f6f4, which runs e4m3 operands at twice the bf16 rate and applies
// the block scales inside the matrix core. The structure is the bf16 kernels' direct-to-LDS form (gemm.hip, gemm_bf16_nt_kernel) at the same
// BYTES per K tile: 8 wave64 per 256 (token) x 256 (feature) tile, a K tile of 128 fp8 is a [256 rows][128 B] image per operand - byte for byte
// the [rows][64] bf16 image of those kernels, with the same 16-byte chunk XOR swizzle - staged by global_load_lds_dwordx4 into two LDS stages,
// plus one dword of 4 scale bytes per row and K tile (global_load_lds_dword). Weights are the MFMA's A operand, tokens its B operand, so the
// accumulators come out in the layout gemm_epilogue.hpp's store_tile_lds takes: the epilogues (and their bf16 rounding points) are the bf16 GEMM's.
//
// Scaled-MFMA lane maps (32x32x64, 8-bit formats; measured with single-k probes and pinned by tests/test_mxfp8_gpu.py on exact small-integer
// data): lane l = (r = l & 31, h = l >> 5) holds row r; operand bytes 0..15 are k = 16 h .. 16 h + 15 of the 64-deep step and bytes 16..31 are
// k = 32 + 16 h .. 32 + 16 h + 15, so scale block 0 of the step is the low half of BOTH lane halves and block 1 the high half. The block-b scale
// is the byte op_sel names of the scale VGPR of the lanes with h = b (row r). Each lane keeps the scale dword of its row (k blocks 4t .. 4t + 3
// of K tile t) shifted right by 8 h, so k-step s uses op_sel byte 2 s in both lane halves.
#include "common.hpp"
#include "gen3c_hip.h"
#include "mx_quant.hpp"  // e4m3_rne, mx_block_exponent, mx_quant_quad: shared with norm_rope.hip

namespace {

constexpr int BM = 256;
constexpr int BN = 256;
constexpr int NTHREADS = 512;
constexpr int MX_BK = 128;   // fp8 elements (= bytes) per K tile
constexpr int MX_BLOCK = 32;  // elements per scale block

#include "gemm_epilogue.hpp"

typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------------
// Quantisation
// ---------------------------------------------------------------------------------------------------------------

// 4 lanes per 32-element block, 8 elements (16 bytes) each: every load and store is a contiguous run across the wave.
__global__ __launch_bounds__(256) void quant_mxfp8_kernel(const bf16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ q, int64_t ldq,
                                                          uint8_t* __restrict__ scales, int64_t lds, int M, int K) {
    const int per_row = K >> 3;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < (int64_t)M * per_row;  // dead lanes still join the shuffles (their amax is 0)
    const int row = live ? (int)(idx / per_row) : 0;
    const int c8 = live ? (int)(idx - (int64_t)row * per_row) : 0;
    bf16x8 v = zero_bf16x8();
    if (live) v = load_bf16x8(x + (int64_t)row * ldx + 8 * c8);
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
    const uint32_t abits = mx_quad_amax_bits(f);
    if (!live) return;
    const float amax = __uint_as_float(abits);
    const bool finite = abits < MX_INF_BITS;  // a NaN or an infinity in the block: the E8M0 NaN and zero codes (mx_quant.hpp)
    const int X = finite ? mx_block_exponent(amax) : MX_X_NAN;
    u32x2 o = {0u, 0u};
    if (finite && amax != 0.0f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float y = fminf(fmaxf(ldexpf(f[e], -X), -448.0f), 448.0f);
            o[e >> 2] |= e4m3_rne(y) << (8 * (e & 3));
        }
    }
    *reinterpret_cast<u32x2*>(q + (int64_t)row * ldq + 8 * c8) = o;
    if ((c8 & 3) == 0) scales[(int64_t)row * lds + (c8 >> 2)] = (uint8_t)(X + 127);
}

// ---------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------

struct MxParams {
    GemmParams ep;  // C / gate / residual, M, N, K and the tile grid: what the shared epilogue reads
    const uint8_t* A; int64_t lda; const uint8_t* As; int64_t ldas;  // activations [M][lda] e4m3, scales [M][ldas] E8M0
    const uint8_t* W; int64_t ldw; const uint8_t* Ws; int64_t ldws;  // weights [N][ldw] e4m3, scales [N][ldws] E8M0
    uint8_t* Q; int64_t ldq; uint8_t* S; int64_t lds;                // MX_OUT instantiations: the output as e4m3 [M][ldq] + E8M0 [M][lds] (ep.C unused)
};

// Template flag on top of the epilogue code: the output leaves as MXFP8 (g3_gemm_mxfp8_nt_mxout). gemm_mxfp8_nt_kernel<MX_OUT | EPI_NONE / EPI_GELU>.
constexpr int MX_OUT = 0x100;

constexpr int MX_TILE_BYTES = BM * MX_BK;                          // one operand, one stage: 32 KiB
constexpr int MX_SCALE_OFF = 2 * (BM + BN) * MX_BK;                // 128 KiB of operand stages, then [2 stages][256 A rows + 256 W rows] dwords
constexpr int MX_SMEM = MX_SCALE_OFF + 2 * (BM + BN) * 4;          // 132 KiB

G3_DEVICE i32x8 mx_frag(const char* tile, int row, int chunk) {  // 32 bytes = logical chunks `chunk`, `chunk` + 2 of a swizzled 128-B row
    const u32x4 lo = *reinterpret_cast<const u32x4*>(tile + row * MX_BK + ((chunk ^ ((row >> 1) & 7)) << 4));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(tile + row * MX_BK + (((chunk + 2) ^ ((row >> 1) & 7)) << 4));
    i32x8 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = (int)lo[e];
        r[4 + e] = (int)hi[e];
    }
    return r;
}

// store_tile_lds (gemm_epilogue.hpp) with another store: the same LDS transpose and the same rounding points up to and including the final
// f32_to_bf16, then the lane's 8 bf16 values are quantised where they sit. After the transpose a lane owns 8 consecutive features of one token row
// and the 4 lanes c2 = 4 b .. 4 b + 3 own the 32-element block b of the wave's 128 features: the block amax is two cross-lane steps (mx_quant_quad),
// the lane stores 8 bytes of q and the quad's first lane the scale byte. What quant_mxfp8_kernel would compute from the bf16 tile, without the
// tile ever reaching memory. The shuffles run BEFORE the row predicate (a quad is one token row: live or dead as a whole, but every lane takes part).
template <int EPI>
G3_DEVICE void store_tile_lds_mx(const MxParams& p, f32x16 (&acc)[4][2], int mw, int nw, int lane, char* stage) {
    static_assert(EPI == EPI_NONE || EPI == EPI_GELU, "MXFP8 output: plain or GELU epilogue only");
    const int l31 = lane & 31, g = lane >> 5;
    const int rsub = lane >> 4, c2 = lane & 15;
    const int n = nw + 8 * c2;  // < N: N is a multiple of the tile (host)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q4 + e];
                *reinterpret_cast<f32x4*>(stage + l31 * 512 + (((8 * i + 2 * q4 + g) ^ l31) << 4)) = v;
            }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int row = 4 * s + rsub;
            const int m = mw + 32 * j + row;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(stage + row * 512 + (((2 * c2) ^ row) << 4));
            const f32x4 hi = *reinterpret_cast<const f32x4*>(stage + row * 512 + (((2 * c2 + 1) ^ row) << 4));
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = lo[e];
                v[4 + e] = hi[e];
            }
            if (EPI == EPI_GELU) {  // the Linear's own rounding to bf16 (see store_tile), then GELU
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = gelu_erf_fast((float)f32_to_bf16(v[e]));
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (float)f32_to_bf16(v[e]);  // the bf16 the plain epilogue stores
            int X;
            const u32x2 o = mx_quant_quad(v, X);  // rows m >= M run the arithmetic too, on the accumulators of the clamped (last) token row: finite, discarded
            if (m >= p.ep.M) continue;
            *reinterpret_cast<u32x2*>(p.Q + (int64_t)m * p.ldq + n) = o;
            if ((c2 & 3) == 0) p.S[(int64_t)m * p.lds + (n >> 5)] = (uint8_t)(X + 127);
        }
    }
}

template <int EPI>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_mxfp8_nt_kernel(MxParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* sA = smem_raw;                       // [2][BM][128]
    char* sW = smem_raw + 2 * MX_TILE_BYTES;   // [2][BN][128]
    const uint32_t* sS = reinterpret_cast<const uint32_t*>(smem_raw + MX_SCALE_OFF);  // [2][A rows 256 | W rows 256]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int g = lane >> 5;

    // tile order of the bf16 kernels: a contiguous run of the global order per XCD, token tiles in super-rows of 4
    const int nblk = p.ep.tiles_m * p.ep.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7;
        const int xcd = bid & 7, slot = bid >> 3;
        bid = ((xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    }
    constexpr int GM = 4;
    const int per_group = GM * p.ep.tiles_n;
    const int grp = bid / per_group;
    const int within = bid - grp * per_group;
    const int gm = min(GM, p.ep.tiles_m - grp * GM);
    const int tile_n = within / gm;
    const int tile_m = grp * GM + (within - tile_n * gm);
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;
    const int M = p.ep.M;

    // ---- LDS-DMA sources: this lane fills physical chunk tid & 7 of rows (tid >> 3) + 64 i, i.e. logical chunk (tid & 7) ^ ((tid >> 4) & 7).
    // Token rows past M read the last row (never stored); N is a multiple of 256 (host).
    const int src_chunk = (tid & 7) ^ ((tid >> 4) & 7);
    const uint8_t* ga[4];
    const uint8_t* gw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (tid >> 3) + 64 * i;
        ga[i] = p.A + (int64_t)min(m0 + row, M - 1) * p.lda + src_chunk * 16;
        gw[i] = p.W + (int64_t)(n0 + row) * p.ldw + src_chunk * 16;
    }
    // scale dwords: threads 0..255 fetch token row tid's, 256..511 weight row (tid - 256)'s
    const uint8_t* gs = tid < 256 ? p.As + (int64_t)min(m0 + tid, M - 1) * p.ldas : p.Ws + (int64_t)(n0 + tid - 256) * p.ldws;

    auto stage = [&](int t, int buf) {
        const int k0 = t * MX_BK;
        char* dA = sA + buf * MX_TILE_BYTES + wave * 1024;  // wave-uniform base; the hardware adds lane * 16 bytes
        char* dW = sW + buf * MX_TILE_BYTES + wave * 1024;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ga[i] + k0),
                                             (__attribute__((address_space(3))) void*)(dA + i * 8192), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gw[i] + k0),
                                             (__attribute__((address_space(3))) void*)(dW + i * 8192), 16, 0, 0);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gs + 4 * t),
                                         (__attribute__((address_space(3))) void*)(smem_raw + MX_SCALE_OFF + buf * 2048 + wave * 256), 4, 0, 0);
    };

    // ---- wave tile: 128 features x 64 tokens (the layout store_tile_lds takes)
    const int n_w0 = (wave & 1) * 128;
    const int m_w0 = (wave >> 1) * 64;

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = p.ep.K / MX_BK;
    stage(0, 0);
    lds_dma_publish_barrier();

    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        G3_JITTER(wave + blockIdx.x, t);
        if (t + 1 < nk) stage(t + 1, buf ^ 1);  // buf ^ 1 was last read in iteration t - 1 (barrier passed)

        const char* cA = sA + buf * MX_TILE_BYTES;
        const char* cW = sW + buf * MX_TILE_BYTES;
        const uint32_t* cS = sS + buf * 512;
        uint32_t ws[4], as[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) ws[i] = cS[256 + n_w0 + 32 * i + l31] >> (8 * g);
#pragma unroll
        for (int j = 0; j < 2; ++j) as[j] = cS[m_w0 + 32 * j + l31] >> (8 * g);

        i32x8 wf[2][4], af[2][2];
        auto load_frags = [&](int ks, int slot) {
            const int chunk = 4 * ks + g;
#pragma unroll
            for (int i = 0; i < 4; ++i) wf[slot][i] = mx_frag(cW, n_w0 + 32 * i + l31, chunk);
#pragma unroll
            for (int j = 0; j < 2; ++j) af[slot][j] = mx_frag(cA, m_w0 + 32 * j + l31, chunk);
        };
        load_frags(0, 0);
        load_frags(1, 1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[0][i], af[0][j], acc[i][j], 0, 0, 0, (int)ws[i], 0, (int)as[j]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[1][i], af[1][j], acc[i][j], 0, 0, 2, (int)ws[i], 2, (int)as[j]);

        lds_dma_publish_barrier();  // tile t + 1 has landed for every wave; every wave is done with stage buf
    }

    if constexpr ((EPI & MX_OUT) != 0)
        store_tile_lds_mx<EPI & ~MX_OUT>(p, acc, m0 + m_w0, n0 + n_w0, lane, smem_raw + wave * 16384);
    else
        store_tile_lds<EPI>(p.ep, acc, m0 + m_w0, n0 + n_w0, lane, smem_raw + wave * 16384);
}

// The one launch of the MX GEMMs. KERNEL: the instantiation; P: its parameter block (MxParams / Mx6Params).
template <auto KERNEL, class P>
int mx_launch(const P& p, void* stream, const char* f) {
    static bool granted[G3_MAX_DEVICES] = {};
    if (int rc = g3_grant_dynamic_lds(reinterpret_cast<const void*>(KERNEL), MX_SMEM, granted, f)) return rc;
    hipLaunchKernelGGL(KERNEL, dim3(p.ep.tiles_m * p.ep.tiles_n), dim3(NTHREADS), MX_SMEM, (hipStream_t)stream, p);
    return g3_check_launch(f);
}

bool mx_shape_ok(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && (N % BN) == 0 && (K % MX_BK) == 0; }

// What every GEMM entry point requires of its MX operands; row_bytes: the packed bytes of a row's K elements (K as e4m3, 3K/4 as e2m3). G3_OK or the error already set.
int mx_check_operands(const char* f, const void* aq, int64_t lda, const void* as, int64_t ldas, const void* wq, int64_t ldw, const void* ws, int64_t ldws,
                      int M, int N, int K, int64_t row_bytes) {
    if (!aq || !as || !wq || !ws) return g3_set_error(G3_ERR_ARG, "%s: null operand", f);
    if (!mx_shape_ok(M, N, K)) return g3_set_error(G3_ERR_ARG, "%s: need M > 0, N a multiple of 256 and K a multiple of 128 (M=%d N=%d K=%d)", f, M, N, K);
    if (lda < row_bytes || ldw < row_bytes || (lda & 15) || (ldw & 15))
        return row_bytes == K ? g3_set_error(G3_ERR_ARG, "%s: need lda, ldw >= K and multiples of 16 (lda=%lld ldw=%lld)", f, (long long)lda, (long long)ldw)
                              : g3_set_error(G3_ERR_ARG, "%s: need lda, ldw >= 3K/4 and multiples of 16 (lda=%lld ldw=%lld K=%d)", f, (long long)lda, (long long)ldw, K);
    if (ldas < K / MX_BLOCK || ldws < K / MX_BLOCK || (ldas & 3) || (ldws & 3))
        return g3_set_error(G3_ERR_ARG, "%s: need scale strides >= K/32 and multiples of 4 (ldas=%lld ldws=%lld K=%d)", f, (long long)ldas, (long long)ldws, K);
    if (((uintptr_t)aq | (uintptr_t)wq) & 15) return g3_set_error(G3_ERR_ARG, "%s: operands must be 16-byte aligned", f);
    if (((uintptr_t)as | (uintptr_t)ws) & 3) return g3_set_error(G3_ERR_ARG, "%s: scales must be 4-byte aligned", f);
    return G3_OK;
}

// What the entries with a bf16 output (MXFP8 and MXFP6 operands) require of C and of the epilogue's operands.
int mx_check_bf16_output(const char* f, const void* c, int64_t ldc, int N, int epilogue, const void* gate, int gate_rows, int64_t ldg, const void* residual, int64_t ldr) {
    if (ldc < N || (ldc & 7) || ((uintptr_t)c & 15)) return g3_set_error(G3_ERR_ARG, "%s: C needs ldc >= N, ldc %% 8 == 0 and 16-byte alignment", f);
    if (epilogue != EPI_NONE && epilogue != EPI_GELU && epilogue != EPI_GATED_RESIDUAL) return g3_set_error(G3_ERR_ARG, "%s: unsupported epilogue %d", f, epilogue);
    if (epilogue == EPI_GATED_RESIDUAL &&
        (!gate || !residual || gate_rows <= 0 || (ldg & 7) || (ldr & 7) || ldr < N || (gate_rows > 1 && ldg < N) ||
         (((uintptr_t)gate | (uintptr_t)residual) & 15)))
        return g3_set_error(G3_ERR_ARG, "%s: gated-residual epilogue needs gate [gate_rows][ldg >= N] and residual [M][ldr >= N], 16-byte aligned rows", f);
    return G3_OK;
}

// The one fill of a parameter block (P: MxParams / Mx6Params): the operands, and the part the shared epilogue reads (the MXFP8-output entry has no C, gate or residual).
template <class P>
P mx_params(const void* aq, int64_t lda, const void* as, int64_t ldas, const void* wq, int64_t ldw, const void* ws, int64_t ldws, int M, int N, int K,
            void* c = nullptr, int64_t ldc = 0, const void* gate = nullptr, int gate_rows = 1, int64_t ldg = 0, const void* residual = nullptr, int64_t ldr = 0) {
    P p{};
    p.ep.tile_order_rowmajor = 0;
    p.ep.wide_store = 1;
    p.ep.C = (bf16_t*)c; p.ep.ldc = ldc;
    p.ep.M = M; p.ep.N = N; p.ep.K = K;
    p.ep.gate = (const bf16_t*)gate; p.ep.gate_rows = gate_rows > 0 ? gate_rows : 1; p.ep.ldg = ldg;
    p.ep.R = (const bf16_t*)residual; p.ep.ldr = ldr;
    p.ep.tiles_m = (M + BM - 1) / BM; p.ep.tiles_n = N / BN;
    p.A = (const uint8_t*)aq; p.lda = lda; p.As = (const uint8_t*)as; p.ldas = ldas;
    p.W = (const uint8_t*)wq; p.ldw = ldw; p.Ws = (const uint8_t*)ws; p.ldws = ldws;
    return p;
}

}  // namespace

extern "C" int g3_quant_mxfp8_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int M, int K, void* stream) {
    if (!x || !q || !scales) return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp8_bf16: null operand");
    if (M <= 0 || K <= 0 || (K % MX_BLOCK)) return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp8_bf16: need M > 0 and K a positive multiple of 32 (M=%d K=%d)", M, K);
    if (ldx < K || (ldx & 7) || ldq < K || (ldq & 7) || lds < K / MX_BLOCK)
        return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp8_bf16: need ldx >= K, ldq >= K (multiples of 8), lds >= K/32 (ldx=%lld ldq=%lld lds=%lld K=%d)",
                            (long long)ldx, (long long)ldq, (long long)lds, K);
    if (((uintptr_t)x & 15) || ((uintptr_t)q & 7)) return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp8_bf16: x must be 16-byte and q 8-byte aligned");
    const int64_t threads = (int64_t)M * (K / 8);
    const int64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp8_bf16: tensor too large");
    hipLaunchKernelGGL(quant_mxfp8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (uint8_t*)q, ldq,
                       (uint8_t*)scales, lds, M, K);
    return g3_check_launch("g3_quant_mxfp8_bf16");
}

extern "C" int g3_gemm_mxfp8_nt(const void* aq, int64_t lda, const void* as, int64_t ldas, const void* wq, int64_t ldw, const void* ws,
                                int64_t ldws, void* c, int64_t ldc, int M, int N, int K, int epilogue, const void* gate, int gate_rows,
                                int64_t ldg, const void* residual, int64_t ldr, void* stream) {
    const char* f = "g3_gemm_mxfp8_nt";
    if (!c) return g3_set_error(G3_ERR_ARG, "%s: null operand", f);
    if (int rc = mx_check_operands(f, aq, lda, as, ldas, wq, ldw, ws, ldws, M, N, K, K)) return rc;
    if (int rc = mx_check_bf16_output(f, c, ldc, N, epilogue, gate, gate_rows, ldg, residual, ldr)) return rc;
    const MxParams p = mx_params<MxParams>(aq, lda, as, ldas, wq, ldw, ws, ldws, M, N, K, c, ldc, gate, gate_rows, ldg, residual, ldr);
    switch (epilogue) {
        case EPI_NONE: return mx_launch<gemm_mxfp8_nt_kernel<EPI_NONE>>(p, stream, f);
        case EPI_GELU: return mx_launch<gemm_mxfp8_nt_kernel<EPI_GELU>>(p, stream, f);
        default: return mx_launch<gemm_mxfp8_nt_kernel<EPI_GATED_RESIDUAL>>(p, stream, f);
    }
}

extern "C" const char* g3_gemm_mxfp8_kernel_name(int M, int N, int K, int epilogue) {
    if (!mx_shape_ok(M, N, K) || (epilogue != EPI_NONE && epilogue != EPI_GELU && epilogue != EPI_GATED_RESIDUAL)) return nullptr;
    static const char* const names[3] = {"gemm_mxfp8_nt_kernel<0>", "gemm_mxfp8_nt_kernel<1>", "gemm_mxfp8_nt_kernel<2>"};  // EPI_NONE, GELU, GATED_RESIDUAL
    return names[epilogue];
}

extern "C" int g3_gemm_mxfp8_nt_mxout(const void* aq, int64_t lda, const void* as, int64_t ldas, const void* wq, int64_t ldw, const void* ws,
                                      int64_t ldws, void* q_out, int64_t ldq, void* s_out, int64_t lds, int M, int N, int K, int epilogue,
                                      void* stream) {
    const char* f = "g3_gemm_mxfp8_nt_mxout";
    if (!q_out || !s_out) return g3_set_error(G3_ERR_ARG, "%s: null output", f);
    if (int rc = mx_check_operands(f, aq, lda, as, ldas, wq, ldw, ws, ldws, M, N, K, K)) return rc;
    if (ldq < N || (ldq & 7) || lds < N / MX_BLOCK)
        return g3_set_error(G3_ERR_ARG, "%s: need ldq >= N (a multiple of 8) and lds >= N/32 (ldq=%lld lds=%lld N=%d)", f, (long long)ldq, (long long)lds, N);
    if ((uintptr_t)q_out & 7) return g3_set_error(G3_ERR_ARG, "%s: q_out must be 8-byte aligned", f);
    if (epilogue != EPI_NONE && epilogue != EPI_GELU)
        return g3_set_error(G3_ERR_ARG, "%s: epilogue %d has no MXFP8 output (NONE and GELU only: the gated residual's output is the bf16 residual stream)", f, epilogue);
    MxParams p = mx_params<MxParams>(aq, lda, as, ldas, wq, ldw, ws, ldws, M, N, K);
    p.Q = (uint8_t*)q_out; p.ldq = ldq; p.S = (uint8_t*)s_out; p.lds = lds;
    return epilogue == EPI_GELU ? mx_launch<gemm_mxfp8_nt_kernel<MX_OUT | EPI_GELU>>(p, stream, f) : mx_launch<gemm_mxfp8_nt_kernel<MX_OUT | EPI_NONE>>(p, stream, f);
}

extern "C" const char* g3_gemm_mxfp8_mxout_kernel_name(int M, int N, int K, int epilogue) {
    if (!mx_shape_ok(M, N, K) || (epilogue != EPI_NONE && epilogue != EPI_GELU)) return nullptr;
    return epilogue == EPI_GELU ? "gemm_mxfp8_nt_kernel<257>" : "gemm_mxfp8_nt_kernel<256>";  // MX_OUT | epilogue
}

// ===============================================================================================================
// MXFP6 (OCP MX v1.0, e2m3 elements): the same instruction at the MXFP4 rate (cbsz / blgp = 2), three quarters of the operand bytes in memory.
// ===============================================================================================================
//
// Format: e2m3 = 1 sign, 2 exponent, 3 mantissa bits, bias 1: subnormals m/8, normals 2^(e-1)(1 + m/8), maximum 7.5, no Inf / NaN.
// A block is 32 consecutive k of one row; X = floor(log2(amax)) - 2, byte X + 127 clamped to 0..254 (all-zero block: byte 127, zero codes);
// elements are RNE(clamp(x / 2^X, -7.5, 7.5)): amax / 2^X lies in [4, 8), so (7.5, 8) saturates and the tie 7.75 does not become 8.
// Storage: q [M][3K/4] bytes, block b of a row = bytes [24 b, 24 b + 24), element i = the 6-bit code at bits [6 i, 6 i + 6) of that 192-bit
// little-endian string; scales [M][K/32] as for MXFP8.
//
// Scaled-MFMA lane maps (32x32x64, both operands e2m3). The kernel was written to the map below; it is probed k by k, code by code and scale
// byte by scale byte by tests/test_mx_kernels_gpu.py (weight row n one-hot at k = n under scale bytes 127 +- 40 on both operands, up to
// K = 16384; bf16 output bitwise the closed form) and by the exact test of tests/test_mxfp6_gpu.py, which any other k order, bit order or
// scale assignment fails:
// the operand is 6 VGPRs = 192 bits. Lane l = (r = l & 31, h = l >> 5) holds row r, k = 32 h + i of the 64-deep step in bits [6 i, 6 i + 6) of
// its 192-bit little-endian operand - unlike the 8-bit map a lane half holds ONE contiguous scale block, which is exactly one stored 24-byte block,
// so no repacking is needed. The scale of that block is the byte op_sel names in the lane's OWN scale VGPR. Each lane keeps the scale dword of
// its row (blocks 4 t .. 4 t + 3 of K tile t) shifted right by 8 h, so k-step s uses op_sel byte 2 s in both lane halves, as in the MXFP8 kernel.
//
// LDS image: a lane's operand is 24 bytes, 8- but not 16-byte aligned in the packed 96-byte row, and a 96-byte row stride puts the 32 rows of
// a lane group on 8 bank offsets (a 4-way conflict on ds_read_b64); the 16-byte-chunk XOR of the 128-byte image has no 6-chunk form. Instead
// each 24-byte block is staged as TWO 16-byte chunks that overlap by 8 bytes: bytes [24 b, 24 b + 16) and [24 b + 8, 24 b + 24) of the packed row
// (global_load_lds_dwordx4 from 8-byte aligned global addresses; no chunk reads outside its own block, so nothing is read past a row's end).
// A K tile is then again a [256 rows][8 chunks = 128 B] image per operand with the MXFP8 kernel's chunk XOR ((row >> 1) & 7), read with
// two ds_read_b128 per operand (registers 0..3 from the first chunk, 4..5 from the upper half of the second): conflict-free for the reason the
// MXFP8 image is - the 16 lanes of a ds_read_b128 group hold 16 rows distinct mod 16, bank = 32 (row & 1) + 4 (chunk ^ ((row >> 1) & 7)) + 0..3,
// distinct for distinct (row & 1, (row >> 1) & 7). (A ds_read_b64 of just the upper half would serve 32 rows from the same 8 bytes of every
// chunk - half the banks, 2-way, the same 4 LDS cycles - and the compiler pairs such reads into ds_read2st64_b64 at half the rate again.)
// The price of the image: LDS bytes and L2 -> LDS bytes per K tile are the MXFP8 kernel's (132 KiB dynamic LDS, two stages); what MXFP6 saves
// is MFMA cycles (half) and bytes from HBM (three quarters).
namespace {

constexpr int MX6_ROW_BYTES = 96;  // packed bytes of one K tile (128 elements) of a row in memory

// 24 bytes of block `blk` (0..3) of a swizzled row: chunks 2 blk and 2 blk + 1 of the 128-byte LDS row; the builtin's operand type is 8 ints,
// of which the e2m3 form reads the first six.
G3_DEVICE i32x8 mx6_frag(const char* tile, int row, int blk) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(tile + row * MX_BK + (((2 * blk) ^ ((row >> 1) & 7)) << 4));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(tile + row * MX_BK + (((2 * blk + 1) ^ ((row >> 1) & 7)) << 4));
    i32x8 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (int)lo[e];
    r[4] = (int)hi[2];
    r[5] = (int)hi[3];
    r[6] = 0;
    r[7] = 0;
    return r;
}

// 4 lanes per 32-element block, 8 elements each, as quant_mxfp8_kernel; a lane's 8 codes are 6 bytes, and the quad's 24 bytes leave as three
// 8-byte stores (lanes 0..2 of the quad), gathered through two shuffles: a wave writes 16 blocks = one contiguous 384-byte run.
__global__ __launch_bounds__(256) void quant_mxfp6_kernel(const bf16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ q, int64_t ldq,
                                                          uint8_t* __restrict__ scales, int64_t lds, int M, int K) {
    const int per_row = K >> 3;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < (int64_t)M * per_row;  // dead lanes still join the shuffles (their amax is 0); a quad is live or dead as a whole
    const int row = live ? (int)(idx / per_row) : 0;
    const int c8 = live ? (int)(idx - (int64_t)row * per_row) : 0;
    bf16x8 v = zero_bf16x8();
    if (live) v = load_bf16x8(x + (int64_t)row * ldx + 8 * c8);
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
    const uint32_t abits = mx_quad_amax_bits(f);
    const float amax = __uint_as_float(abits);
    const bool finite = abits < MX_INF_BITS;  // a NaN or an infinity in the block: the E8M0 NaN and zero codes (mx_quant.hpp)
    const int X = finite ? mx6_block_exponent(amax) : MX_X_NAN;
    uint32_t lo = 0u, hi = 0u;
    if (finite && amax != 0.0f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = ldexpf(f[e], -X);
        mx6_pack8(f, lo, hi);
    }
    const int j = threadIdx.x & 3;  // = c8 & 3: K/8 is a multiple of 4
    const u32x2 o = mx6_gather_quad(lo, hi, j);
    if (!live) return;
    if (j < 3) *reinterpret_cast<u32x2*>(q + (int64_t)row * ldq + 24 * (c8 >> 2) + 8 * j) = o;
    if (j == 0) scales[(int64_t)row * lds + (c8 >> 2)] = (uint8_t)(X + 127);
}

struct Mx6Params {
    GemmParams ep;  // C / gate / residual, M, N, K and the tile grid: what the shared epilogue reads
    const uint8_t* A; int64_t lda; const uint8_t* As; int64_t ldas;  // activations [M][lda >= 3K/4] packed e2m3, scales [M][ldas] E8M0
    const uint8_t* W; int64_t ldw; const uint8_t* Ws; int64_t ldws;  // weights [N][ldw >= 3K/4] packed e2m3, scales [N][ldws] E8M0
};

// gemm_mxfp8_nt_kernel with e2m3 operands: the same tile, waves, tile order, stages, scale handling and epilogue; the staging sources and the
// fragment reads follow the LDS image described above.
template <int EPI>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_mxfp6_nt_kernel(Mx6Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* sA = smem_raw;                       // [2][BM][128]
    char* sW = smem_raw + 2 * MX_TILE_BYTES;   // [2][BN][128]
    const uint32_t* sS = reinterpret_cast<const uint32_t*>(smem_raw + MX_SCALE_OFF);  // [2][A rows 256 | W rows 256]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int g = lane >> 5;

    // tile order of the bf16 kernels: a contiguous run of the global order per XCD, token tiles in super-rows of 4
    const int nblk = p.ep.tiles_m * p.ep.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7;
        const int xcd = bid & 7, slot = bid >> 3;
        bid = ((xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    }
    constexpr int GM = 4;
    const int per_group = GM * p.ep.tiles_n;
    const int grp = bid / per_group;
    const int within = bid - grp * per_group;
    const int gm = min(GM, p.ep.tiles_m - grp * GM);
    const int tile_n = within / gm;
    const int tile_m = grp * GM + (within - tile_n * gm);
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;
    const int M = p.ep.M;

    // ---- LDS-DMA sources: this lane fills physical chunk tid & 7 of rows (tid >> 3) + 64 i, i.e. logical chunk c = (tid & 7) ^ ((tid >> 4) & 7):
    // the first (c & 1 = 0) or second 16 bytes of block c >> 1 of the row's packed 96-byte K tile, at byte 24 (c >> 1) + 8 (c & 1).
    // Token rows past M read the last row (never stored); N is a multiple of 256 (host).
    const int src_chunk = (tid & 7) ^ ((tid >> 4) & 7);
    const int src_off = 24 * (src_chunk >> 1) + 8 * (src_chunk & 1);  // <= 80: the 16 bytes end at or before byte 96
    const uint8_t* ga[4];
    const uint8_t* gw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (tid >> 3) + 64 * i;
        ga[i] = p.A + (int64_t)min(m0 + row, M - 1) * p.lda + src_off;
        gw[i] = p.W + (int64_t)(n0 + row) * p.ldw + src_off;
    }
    // scale dwords: threads 0..255 fetch token row tid's, 256..511 weight row (tid - 256)'s
    const uint8_t* gs = tid < 256 ? p.As + (int64_t)min(m0 + tid, M - 1) * p.ldas : p.Ws + (int64_t)(n0 + tid - 256) * p.ldws;

    auto stage = [&](int t, int buf) {
        const int k0 = t * MX6_ROW_BYTES;
        char* dA = sA + buf * MX_TILE_BYTES + wave * 1024;  // wave-uniform base; the hardware adds lane * 16 bytes
        char* dW = sW + buf * MX_TILE_BYTES + wave * 1024;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ga[i] + k0),
                                             (__attribute__((address_space(3))) void*)(dA + i * 8192), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gw[i] + k0),
                                             (__attribute__((address_space(3))) void*)(dW + i * 8192), 16, 0, 0);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gs + 4 * t),
                                         (__attribute__((address_space(3))) void*)(smem_raw + MX_SCALE_OFF + buf * 2048 + wave * 256), 4, 0, 0);
    };

    // ---- wave tile: 128 features x 64 tokens (the layout store_tile_lds takes)
    const int n_w0 = (wave & 1) * 128;
    const int m_w0 = (wave >> 1) * 64;

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = p.ep.K / MX_BK;
    stage(0, 0);
    lds_dma_publish_barrier();

    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        G3_JITTER(wave + blockIdx.x, t);
        if (t + 1 < nk) stage(t + 1, buf ^ 1);  // buf ^ 1 was last read in iteration t - 1 (barrier passed)

        const char* cA = sA + buf * MX_TILE_BYTES;
        const char* cW = sW + buf * MX_TILE_BYTES;
        const uint32_t* cS = sS + buf * 512;
        uint32_t ws[4], as[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) ws[i] = cS[256 + n_w0 + 32 * i + l31] >> (8 * g);
#pragma unroll
        for (int j = 0; j < 2; ++j) as[j] = cS[m_w0 + 32 * j + l31] >> (8 * g);

        i32x8 wf[2][4], af[2][2];
        auto load_frags = [&](int ks, int slot) {
            const int blk = 2 * ks + g;  // the lane half's own scale block of the 64-deep step
#pragma unroll
            for (int i = 0; i < 4; ++i) wf[slot][i] = mx6_frag(cW, n_w0 + 32 * i + l31, blk);
#pragma unroll
            for (int j = 0; j < 2; ++j) af[slot][j] = mx6_frag(cA, m_w0 + 32 * j + l31, blk);
        };
        load_frags(0, 0);
        load_frags(1, 1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[0][i], af[0][j], acc[i][j], 2, 2, 0, (int)ws[i], 0, (int)as[j]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[1][i], af[1][j], acc[i][j], 2, 2, 2, (int)ws[i], 2, (int)as[j]);

        lds_dma_publish_barrier();  // tile t + 1 has landed for every wave; every wave is done with stage buf
    }

    store_tile_lds<EPI>(p.ep, acc, m0 + m_w0, n0 + n_w0, lane, smem_raw + wave * 16384);
}

}  // namespace

extern "C" int g3_quant_mxfp6_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int M, int K, void* stream) {
    if (!x || !q || !scales) return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp6_bf16: null operand");
    if (M <= 0 || K <= 0 || (K % MX_BLOCK)) return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp6_bf16: need M > 0 and K a positive multiple of 32 (M=%d K=%d)", M, K);
    if (ldx < K || (ldx & 7) || ldq < (int64_t)K / 4 * 3 || (ldq & 7) || lds < K / MX_BLOCK)
        return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp6_bf16: need ldx >= K, ldq >= 3K/4 (multiples of 8), lds >= K/32 (ldx=%lld ldq=%lld lds=%lld K=%d)",
                            (long long)ldx, (long long)ldq, (long long)lds, K);
    if (((uintptr_t)x & 15) || ((uintptr_t)q & 7)) return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp6_bf16: x must be 16-byte and q 8-byte aligned");
    const int64_t threads = (int64_t)M * (K / 8);
    const int64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return g3_set_error(G3_ERR_ARG, "g3_quant_mxfp6_bf16: tensor too large");
    hipLaunchKernelGGL(quant_mxfp6_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (uint8_t*)q, ldq,
                       (uint8_t*)scales, lds, M, K);
    return g3_check_launch("g3_quant_mxfp6_bf16");
}

extern "C" int g3_gemm_mxfp6_nt(const void* aq, int64_t lda, const void* as, int64_t ldas, const void* wq, int64_t ldw, const void* ws,
                                int64_t ldws, void* c, int64_t ldc, int M, int N, int K, int epilogue, const void* gate, int gate_rows,
                                int64_t ldg, const void* residual, int64_t ldr, void* stream) {
    const char* f = "g3_gemm_mxfp6_nt";
    if (!c) return g3_set_error(G3_ERR_ARG, "%s: null operand", f);
    if (int rc = mx_check_operands(f, aq, lda, as, ldas, wq, ldw, ws, ldws, M, N, K, (int64_t)K / 4 * 3)) return rc;
    if (int rc = mx_check_bf16_output(f, c, ldc, N, epilogue, gate, gate_rows, ldg, residual, ldr)) return rc;
    const Mx6Params p = mx_params<Mx6Params>(aq, lda, as, ldas, wq, ldw, ws, ldws, M, N, K, c, ldc, gate, gate_rows, ldg, residual, ldr);
    switch (epilogue) {
        case EPI_NONE: return mx_launch<gemm_mxfp6_nt_kernel<EPI_NONE>>(p, stream, f);
        case EPI_GELU: return mx_launch<gemm_mxfp6_nt_kernel<EPI_GELU>>(p, stream, f);
        default: return mx_launch<gemm_mxfp6_nt_kernel<EPI_GATED_RESIDUAL>>(p, stream, f);
    }
}

extern "C" const char* g3_gemm_mxfp6_kernel_name(int M, int N, int K, int epilogue) {
    if (!mx_shape_ok(M, N, K) || (epilogue != EPI_NONE && epilogue != EPI_GELU && epilogue != EPI_GATED_RESIDUAL)) return nullptr;
    static const char* const names[3] = {"gemm_mxfp6_nt_kernel<0>", "gemm_mxfp6_nt_kernel<1>", "gemm_mxfp6_nt_kernel<2>"};  // EPI_NONE, GELU, GATED_RESIDUAL
    return names[epilogue];
}
