// Included inside the anonymous namespace of the GEMM translation units (gemm.hip, gemm_mx.hip): the epilogue codes, the parameter
// block and the two epilogues that turn a finished 256 x 256 tile of fp32 accumulators (v_mfma_*_32x32x* layout, 8 waves of 128 features x
// 64 tokens) into bf16 rows. One copy, so the bf16 and the MXFP8 GEMMs round at the same points.

enum { EPI_NONE = 0, EPI_GELU = 1, EPI_GATED_RESIDUAL = 2, EPI_BIAS = 3, EPI_BIAS_RESIDUAL = 4,
       EPI_QK_NORM_ROPE = 5 };  // 5: per-head RMSNorm (+ RoPE) on the q / k feature ranges (gemm_w4.hpp only; g3_gemm_qk_norm_rope_bf16)

// Implicit-GEMM convolution geometry (channels-last activations [T][H][W][C], one batch item):
// output row m = (to, yo, xo); tap (dt, dy, dx) reads input position
//   ti = max(to*st + ot + dt, 0)   (causal: the first frame is replicated in front - CausalConv3d._replication_pad)
//   yi = yo*sh + oh + dy, xi = xo*sw + ow + dx   (outside [0,Hi) x [0,Wi) -> zero padding)
// and multiplies with the tap's [N][K] weight slab.
struct ConvGeom {
    int To, Ho, Wo, Ti, Hi, Wi;
    int kt, kh, kw, st, sh, sw, ot, oh, ow;
    int ntaps;
    int64_t w_tap_stride;  // elements between consecutive tap slabs of W
    int tap_gaps;          // gemm_w4_conv.hpp: compute a new tap's token addresses in the MFMA gaps of the barrier K step (option conv_w4 = 2: off, for A/B runs)
};

struct GemmParams {
    int tile_order_rowmajor;
    int wide_store;  // C / residual / gate rows are 16-byte addressable: epilogue goes through the LDS transpose (full-line stores)
    const bf16_t* A; int64_t lda;
    const bf16_t* W; int64_t ldw;
    bf16_t* C; int64_t ldc;
    int M, N, K;
    const bf16_t* gate; int gate_rows; int64_t ldg;  // gate[(m % gate_rows)][n]  (EPI_GATED_RESIDUAL) / bias (EPI_BIAS)
    const bf16_t* R; int64_t ldr;                     // residual rows
    int tiles_m, tiles_n;
    ConvGeom cv;
    // EPI_QK_NORM_ROPE: features [0, n_q) are q heads (weight nw_q), [n_q, n_q + n_k) k heads (nw_k), the rest is stored as is
    const bf16_t* nw_q; const bf16_t* nw_k; const float* rope_cos; const float* rope_sin; int n_q, n_k, rope_B; float rms_eps;
    bf16_t* vt; int64_t vt_ld, vt_batch; int vt_S;  // optional V^T destination of the remaining (v) heads: [B][H_v][128][vt_ld], S valid positions
    // gemm_w4_conv.hpp: optional GroupNorm statistics of the output ([frames][2] doubles: sum, sum of squares; frame = gn_rows consecutive rows)
    double* gn_stats = nullptr; int gn_rows = 0;
    int mfma16 = 0;  // gemm_w4e.hpp: the K loop on v_mfma_f32_16x16x32_bf16 (option gemm_mfma16; same bits, same kernel names)
};

// ---- epilogue shared by the kernels below. acc[i][j][r]: feature = nw + 32 i + (r & 3) + 8 (r >> 2) + 4 g ; token = mw + 32 j + l31
template <int EPI>
G3_DEVICE void store_tile(const GemmParams& p, f32x16 (&acc)[4][2], int mw, int nw, int l31, int g) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = mw + 32 * j + l31;
        if (m >= p.M) continue;
        bf16_t* crow = p.C + (int64_t)m * p.ldc;
        const bf16_t* rrow = (EPI == EPI_GATED_RESIDUAL || EPI == EPI_BIAS_RESIDUAL) ? (p.R + (int64_t)m * p.ldr) : nullptr;
        const bf16_t* grow = (EPI == EPI_GATED_RESIDUAL || EPI == EPI_BIAS || EPI == EPI_BIAS_RESIDUAL)
                                 ? (p.gate + (int64_t)(m % p.gate_rows) * p.ldg)
                                 : nullptr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int n = nw + 32 * i + 8 * q4 + 4 * g;
                if (n >= p.N) continue;  // N % 4 == 0 is required by the host wrapper
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q4 + e];
                // GELU / gated residual act on the Linear's OUTPUT, which nn.Linear rounds to bf16 (attention.py:94-99, blocks.py:455-471); every GEMM
                // kernel rounds here since round 5 (gemm_w4e.hpp keeps a finished tile as packed bf16): bitwise equal outputs across the kernels
                if (EPI == EPI_GELU || EPI == EPI_GATED_RESIDUAL) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (float)f32_to_bf16(v[e]);
                }
                if (EPI == EPI_GELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_erf_fast(v[e]);
                } else if (EPI == EPI_GATED_RESIDUAL) {
                    const bf16x4 gv = *reinterpret_cast<const bf16x4*>(grow + n);
                    const bf16x4 rv = *reinterpret_cast<const bf16x4*>(rrow + n);
                    // reference order (blocks.py:456): block output is rounded to bf16 by its Linear, then
                    // gate*out and x+.. ; we keep fp32 until the single final rounding.
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (float)rv[e] + (float)gv[e] * v[e];
                } else if (EPI == EPI_BIAS) {
                    const bf16x4 gv = *reinterpret_cast<const bf16x4*>(grow + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += (float)gv[e];
                } else if (EPI == EPI_BIAS_RESIDUAL) {
                    const bf16x4 gv = *reinterpret_cast<const bf16x4*>(grow + n);
                    const bf16x4 rv = *reinterpret_cast<const bf16x4*>(rrow + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (v[e] + (float)gv[e]) + (float)rv[e];
                }
                bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = f32_to_bf16(v[e]);
                *reinterpret_cast<bf16x4*>(crow + n) = o;
            }
        }
    }
}

// Full-line epilogue: the MFMA layout gives a lane 4 features of 32 different token rows, so direct stores touch 32 cache
// lines with 16 bytes each per instruction (measured ~2.5 TB/s of C traffic). Instead each wave transposes its tile through
// a PRIVATE 16 KiB slice of the (now idle) operand LDS, one 32-token half at a time, as fp32 [32 tokens][128 features]
// with the 16-byte chunk index XOR-ed by the row, and reads it back row-major: a lane then owns 8 consecutive features
// (one 16-byte bf16 store), 16 lanes cover a token row's 256 bytes, and residual/gate loads coalesce the same way.
// No barrier: LDS operations of one wave execute in order and the slice is not shared. Same arithmetic as store_tile.
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
template <int EPI>
G3_DEVICE void store_tile_lds(const GemmParams& p, f32x16 (&acc)[4][2], int mw, int nw, int lane, char* stage) {
    const int l31 = lane & 31, g = lane >> 5;
    const int rsub = lane >> 4, c2 = lane & 15;
    const int n = nw + 8 * c2;
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
            if (m >= p.M || n >= p.N) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = lo[e];
                v[4 + e] = hi[e];
            }
            if (EPI == EPI_GELU || EPI == EPI_GATED_RESIDUAL) {  // the Linear's own rounding to bf16 (see store_tile)
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (float)f32_to_bf16(v[e]);
            }
            if (EPI == EPI_GELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = gelu_erf_fast(v[e]);
            } else if (EPI != EPI_NONE) {
                const bf16x8 gv = load_bf16x8(p.gate + (int64_t)(p.gate_rows == 1 ? 0 : m % p.gate_rows) * p.ldg + n);
                if (EPI == EPI_GATED_RESIDUAL) {
                    const bf16x8 rv = load_bf16x8(p.R + (int64_t)m * p.ldr + n);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = (float)rv[e] + (float)gv[e] * v[e];
                } else if (EPI == EPI_BIAS) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += (float)gv[e];
                } else if (EPI == EPI_BIAS_RESIDUAL) {
                    const bf16x8 rv = load_bf16x8(p.R + (int64_t)m * p.ldr + n);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = (v[e] + (float)gv[e]) + (float)rv[e];
                }
            }
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f32_to_bf16(v[e]);
            store_bf16x8(p.C + (int64_t)m * p.ldc + n, o);
        }
    }
}
