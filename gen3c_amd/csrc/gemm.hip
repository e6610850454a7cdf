// bf16 "NT" GEMM for the DiT linears:  C[M,N] = epi( A[M,K] . W[N,K]^T )
//
// Replaces the nn.Linear(bias=False) calls of the reference's DiT blocks
// (cosmos_predict1/diffusion/module/attention.py:61-62,207-223; blocks.py:160-162,205-206) together with
// the elementwise tail each of them feeds (GELU: attention.py:94-99; gated residual: blocks.py:455-471).
//
// MI355X design (not a port of any CUDA tiling):
//   * one workgroup = 8 wave64 = 512 threads computes a 256(token) x 256(feature) tile, K-step 64;
//   * v_mfma_f32_32x32x16_bf16, operands swapped (A-operand = weight rows, B-operand = token rows) so that a
//     lane ends up owning 4 CONSECUTIVE output features of one token row -> 8-byte stores, and per-feature
//     epilogue vectors (gate) are lane-local;
//   * both operands have K contiguous, so every fragment is one 16-byte LDS read; both MFMA inputs use the
//     same lane->k mapping, so the contraction is independent of the hardware's k order inside a fragment;
//   * LDS tiles are [rows][64] bf16 (128-B rows) with the 16-B chunk index XOR-ed by (row>>1)&7, which makes
//     every 16-lane ds_read_b128 group hit 16 distinct 16-B slots of the 256-B bank row (conflict-free);
//   * global->register->LDS staging is split (issue the loads for tile t+1 before the MFMAs of tile t, write
//     them to the other LDS buffer afterwards) so HBM/L2 latency hides under 32 MFMAs per wave; one barrier/tile;
//   * blockIdx is remapped so that the 8 XCDs each own a contiguous band of token tiles (private L2 reuse of
//     the weight panel).
#include "common.hpp"
#include "gen3c_hip.h"
#include <stdlib.h>
#include <mutex>
#include <type_traits>

namespace {

constexpr int BM = 256;  // tokens per block tile
constexpr int BN = 256;  // features per block tile
constexpr int BK = 64;
constexpr int NTHREADS = 512;

#include "gemm_epilogue.hpp"

__device__ __attribute__((aligned(16))) unsigned g3_zero_page[2048];  // 8 KiB of zeros: source of padded taps on the LDS-DMA path (the one-wave kernel walks up to K * 2 bytes into it)

G3_DEVICE int lds_off(int row, int chunk) {  // element offset in a [rows][64] bf16 tile
    return row * BK + ((chunk ^ ((row >> 1) & 7)) << 3);
}

// STAGE_GLDS = true : tiles go HBM/L2 -> LDS directly with global_load_lds_dwordx4 (no staging VGPRs, no ds_write
//                     pass); the LDS image is lane-linear per wave, so the XOR swizzle is applied to the per-lane
//                     SOURCE address (same involution as the read side). Needs K % 64 == 0 (no zero-fill on this path;
//                     M/N tails read a clamped valid row whose results are never stored).
// STAGE_GLDS = false: global -> VGPR -> ds_write_b128 with zero-fill guards (any K % 8 == 0).
// CONV = true: A rows are gathered per tap according to p.cv (implicit GEMM); K is the per-tap channel count.
template <int EPI, bool STAGE_GLDS, bool CONV, bool PIN>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_bf16_nt_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    bf16_t* sA = reinterpret_cast<bf16_t*>(smem_raw);  // [2][BM][BK]
    bf16_t* sW = sA + 2 * BM * BK;                      // [2][BN][BK]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int g = lane >> 5;

    // XCD-aware tile order: dispatch puts block b on XCD b%8; give each XCD a contiguous run of a global tile order
    // (bijective for any tile count). The order itself is built for the private 4 MiB L2s: token tiles are taken in
    // super-rows of GM=4 and swept feature-tile by feature-tile (token tile fastest), so the ~32 workgroups an XCD
    // runs concurrently form an ~(4 token x 8 feature) block: 12 operand panels feed 32 tiles instead of 33.
    const int nblk = p.tiles_m * p.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7;
        const int xcd = bid & 7, slot = bid >> 3;
        const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        bid = base + slot;
    }
    int tile_m, tile_n;
    if (p.tile_order_rowmajor) {
        tile_m = bid / p.tiles_n;
        tile_n = bid - tile_m * p.tiles_n;
    } else {
        constexpr int GM = 4;
        const int per_group = GM * p.tiles_n;
        const int grp = bid / per_group;
        const int within = bid - grp * per_group;
        const int gm = min(GM, p.tiles_m - grp * GM);  // last super-row may be shorter
        tile_n = within / gm;
        tile_m = grp * GM + (within - tile_n * gm);
    }
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;

    // ---- staging assignment: 4 chunks of A and 4 of W per thread per K tile
    const int ld_chunk = tid & 7;
    const int ld_row = tid >> 3;  // + 64*i
    const bf16_t* a_ptr[4];
    const bf16_t* w_ptr[4];
    bool a_ok[4], w_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = ld_row + 64 * i;
        a_ok[i] = (m0 + row) < p.M;
        w_ok[i] = (n0 + row) < p.N;
        a_ptr[i] = p.A + (int64_t)(a_ok[i] ? (m0 + row) : 0) * p.lda + ld_chunk * 8;
        w_ptr[i] = p.W + (int64_t)(w_ok[i] ? (n0 + row) : 0) * p.ldw + ld_chunk * 8;
    }

    // conv: per-row base input coordinates (before adding the tap offset)
    int cbt[4], cby[4], cbx[4];
    if (CONV) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + ld_row + 64 * i;
            const int mm = m < p.M ? m : 0;
            const int to = mm / (p.cv.Ho * p.cv.Wo);
            const int rem = mm - to * (p.cv.Ho * p.cv.Wo);
            const int yo = rem / p.cv.Wo;
            const int xo = rem - yo * p.cv.Wo;
            cbt[i] = to * p.cv.st + p.cv.ot;
            cby[i] = yo * p.cv.sh + p.cv.oh;
            cbx[i] = xo * p.cv.sw + p.cv.ow;
        }
    }
    // source row of slot i for tap `tap`, or -1 for a zero (padded / out-of-range) row
    auto conv_src_row = [&](int i, int tap) -> int64_t {
        const int khw = p.cv.kh * p.cv.kw;
        const int dt = tap / khw;
        const int r2 = tap - dt * khw;
        const int dy = r2 / p.cv.kw;
        const int dx = r2 - dy * p.cv.kw;
        int ti = cbt[i] + dt;
        ti = ti < 0 ? 0 : ti;
        const int yi = cby[i] + dy, xi = cbx[i] + dx;
        const bool ok = a_ok[i] && ti < p.cv.Ti && yi >= 0 && yi < p.cv.Hi && xi >= 0 && xi < p.cv.Wi;
        return ok ? ((int64_t)ti * p.cv.Hi + yi) * p.cv.Wi + xi : (int64_t)-1;
    };
    const int nkc = (p.K + BK - 1) / BK;  // K tiles per tap

    bf16x8 ra[4], rw[4];
    auto stage_load = [&](int it) {
        const int tap = CONV ? it / nkc : 0;
        const int k0 = (CONV ? it - tap * nkc : it) * BK;
        const bool k_ok = (k0 + ld_chunk * 8) < p.K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (CONV) {
                const int64_t src = conv_src_row(i, tap);
                ra[i] = (src >= 0 && k_ok) ? load_bf16x8(p.A + src * p.lda + ld_chunk * 8 + k0) : zero_bf16x8();
                rw[i] = (w_ok[i] && k_ok) ? load_bf16x8(w_ptr[i] + tap * p.cv.w_tap_stride + k0) : zero_bf16x8();
            } else {
                ra[i] = (a_ok[i] && k_ok) ? load_bf16x8(a_ptr[i] + k0) : zero_bf16x8();
                rw[i] = (w_ok[i] && k_ok) ? load_bf16x8(w_ptr[i] + k0) : zero_bf16x8();
            }
        }
    };
    auto stage_write = [&](int buf) {
        bf16_t* dA = sA + buf * BM * BK;
        bf16_t* dW = sW + buf * BN * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = ld_row + 64 * i;
            store_bf16x8(dA + lds_off(row, ld_chunk), ra[i]);
            store_bf16x8(dW + lds_off(row, ld_chunk), rw[i]);
        }
    };
    // direct-to-LDS staging: this lane fills physical slot (row = ld_row + 64 i, chunk = ld_chunk) of the tile, i.e. it
    // must fetch LOGICAL chunk ld_chunk ^ ((row >> 1) & 7) = ld_chunk ^ ((tid >> 4) & 7)  (64 i does not touch bits 1..3).
    const int src_chunk = ld_chunk ^ ((tid >> 4) & 7);
    const bf16_t* ga[4];
    const bf16_t* gw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = ld_row + 64 * i;
        const int ra_row = (m0 + row) < p.M ? (m0 + row) : (p.M - 1);
        const int rw_row = (n0 + row) < p.N ? (n0 + row) : (p.N - 1);
        ga[i] = p.A + (int64_t)ra_row * p.lda + src_chunk * 8;
        gw[i] = p.W + (int64_t)rw_row * p.ldw + src_chunk * 8;
    }
    auto stage_glds = [&](int it, int buf) {
        const int tap = CONV ? it / nkc : 0;
        const int k0 = (CONV ? it - tap * nkc : it) * BK;
        bf16_t* dA = sA + buf * BM * BK + wave * 64 * 8;  // wave-uniform base; the hardware adds lane*16 bytes
        bf16_t* dW = sW + buf * BN * BK + wave * 64 * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bf16_t* asrc;
            const bf16_t* wsrc;
            if (CONV) {
                const int64_t src = conv_src_row(i, tap);
                asrc = src >= 0 ? p.A + src * p.lda + src_chunk * 8 + k0 : reinterpret_cast<const bf16_t*>(g3_zero_page) + src_chunk * 8;
                wsrc = gw[i] + tap * p.cv.w_tap_stride + k0;
            } else {
                asrc = ga[i] + k0;
                wsrc = gw[i] + k0;
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)asrc,
                                             (__attribute__((address_space(3))) void*)(dA + i * 512 * 8), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)wsrc,
                                             (__attribute__((address_space(3))) void*)(dW + i * 512 * 8), 16, 0, 0);
        }
    };

    // ---- wave tile: 128 features x 64 tokens
    const int wn = wave & 1;
    const int wm = wave >> 1;
    const int n_w0 = wn * 128;
    const int m_w0 = wm * 64;

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = CONV ? nkc * p.cv.ntaps : nkc;
    if (STAGE_GLDS) {
        stage_glds(0, 0);
    } else {
        stage_load(0);
        stage_write(0);
    }
    lds_dma_publish_barrier();

    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        G3_JITTER(wave + blockIdx.x, t);
        if (t + 1 < nk) {
            if (STAGE_GLDS) stage_glds(t + 1, buf ^ 1);  // buf^1 was last read in iteration t-1 (barrier passed)
            else stage_load(t + 1);
        }

        const bf16_t* cA = sA + buf * BM * BK;
        const bf16_t* cW = sW + buf * BN * BK;
        // register double-buffered fragments: the ds_reads of k-step ks+1 are issued before the MFMAs of k-step ks
        bf16x8 wf[2][4], af[2][2];
        auto load_frags = [&](int ks, int slot) {
            const int chunk = 2 * ks + g;
#pragma unroll
            for (int i = 0; i < 4; ++i) wf[slot][i] = load_bf16x8(cW + lds_off(n_w0 + 32 * i + l31, chunk));
#pragma unroll
            for (int j = 0; j < 2; ++j) af[slot][j] = load_bf16x8(cA + lds_off(m_w0 + 32 * j + l31, chunk));
        };
        load_frags(0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks + 1 < 4) load_frags(ks + 1, (ks + 1) & 1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks & 1][i], af[ks & 1][j], acc[i][j], 0, 0, 0);
        }
        // pin the stream: the 6 fragment reads of k-step ks+1 ride behind the first 6 of the 8 MFMAs of k-step ks, so
        // only the first k-step after the barrier waits on LDS latency (0x8 = MFMA, 0x100 = DS read)
        if (PIN) {
            __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                    if (ks + 1 < 4 && m < 6) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
            }
        }

        if (!STAGE_GLDS && t + 1 < nk) stage_write(buf ^ 1);
        lds_dma_publish_barrier();  // tile t+1 has landed for every wave
    }

    if (p.wide_store) store_tile_lds<EPI>(p, acc, m0 + m_w0, n0 + n_w0, lane, smem_raw + wave * 16384);
    else store_tile<EPI>(p, acc, m0 + m_w0, n0 + n_w0, l31, g);
}


// ---------------------------------------------------------------------------------------------------------------
// Ping-pong variant of the plain GEMM (no conv, K % 64 == 0) - the default for the DiT linears.
//
// Same 256 x 256 x 64 block tile, same 128(feature) x 64(token) wave tile and accumulator layout as the kernel above, but
// the K loop is cut into 4 PHASES per K tile, one accumulator quadrant (64 features x 32 tokens, 8 MFMAs = 256 MFMA
// cycles) each, and the two waves that share a SIMD run half a phase apart:
//
//     load section : fragment ds_reads of this phase (W half: 8, token half: 4) + ONE half-tile of LDS-DMA (2 per lane)
//     s_waitcnt vmcnt(8) ; s_barrier
//     MFMA section : s_setprio 1 ; 8 MFMAs ; s_setprio 0
//     s_barrier
//
// Waves 4..7 execute one extra s_barrier up front, so while waves 0..3 (one per SIMD) are in their MFMA section waves
// 4..7 are in their load section and vice versa: the 60-180 cycle issue cost of each LDS-DMA instruction and the LDS
// latency hide behind the other wave's MFMAs instead of stalling the matrix pipe.
//
// Operand tiles are staged as HALF-TILES of 128 rows x 64 k (16 KiB: W rows with bit 6 = h, token rows with bit 5 = h),
// so that they can be retired and restaged one at a time. Half-tiles are numbered q = 4 t + {0: W0, 1: T0, 2: T1, 3: W1}
// in the order they are needed; phase f = 4 t + P issues q = f + 6 and reads (P0: q = 4t, 4t+1; P1: 4t+2; P2: 4t+3),
// LDS holds two K tiles (2 x 4 x 16 KiB = 128 KiB), and the vmcnt before a phase's first barrier leaves the 4 newest
// half-tiles in flight - everything the NEXT phase reads has landed for every wave once that barrier (plus the stagger
// barrier) is passed; a buffer is restaged no earlier than two phases after its last ds_read.
// ---------------------------------------------------------------------------------------------------------------
#ifdef G3_AB_NO_GEMM_SETPRIO
#define G3_PP_SETPRIO(x) ((void)0)
#else
#define G3_PP_SETPRIO(x) __builtin_amdgcn_s_setprio(x)
#endif
template <int N> G3_DEVICE void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
G3_DEVICE void wait_vmcnt_rt(int halftiles) {  // tail phases: the number of half-tiles that may stay in flight
    switch (halftiles) {
        case 0: wait_vmcnt<0>(); break;
        case 1: wait_vmcnt<2>(); break;
        case 2: wait_vmcnt<4>(); break;
        case 3: wait_vmcnt<6>(); break;
        default: wait_vmcnt<8>(); break;
    }
}
G3_DEVICE void phase_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

template <int EPI, int PH, bool CONV>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_bf16_nt_pp_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];  // [slot 2][region 4][128 rows][64] bf16
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int g = lane >> 5;

    const int nblk = p.tiles_m * p.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7;
        const int xcd = bid & 7, slot = bid >> 3;
        const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        bid = base + slot;
    }
    int tile_m, tile_n;
    if (p.tile_order_rowmajor) {
        tile_m = bid / p.tiles_n;
        tile_n = bid - tile_m * p.tiles_n;
    } else {
        constexpr int GM = 4;
        const int per_group = GM * p.tiles_n;
        const int grp = bid / per_group;
        const int within = bid - grp * per_group;
        const int gm = min(GM, p.tiles_m - grp * GM);
        tile_n = within / gm;
        tile_m = grp * GM + (within - tile_n * gm);
    }
    const int m0 = tile_m * BM;
    const int n0 = tile_n * BN;
    const int wn = wave & 1;   // feature half of the block tile
    const int wm = wave >> 1;  // token quarter of the block tile
    const int n_w0 = wn * 128, m_w0 = wm * 64;

    // ---- LDS-DMA sources. A half-tile is 1024 16-B slots, 2 per lane: slot = j*512 + tid -> local row j*64 + (tid >> 3),
    // physical chunk tid & 7, which holds logical chunk (tid & 7) ^ ((row >> 1) & 7).
    //   W half h : local row r <-> feature n0 + (r >> 6)*128 + h*64 + (r & 63)
    //   T half h : local row r <-> token   m0 + (r >> 5)*64  + h*32 + (r & 31)
    const int src_chunk = (tid & 7) ^ ((tid >> 4) & 7);
    const bf16_t* src[4][2];  // [region: W0, T0, T1, W1][j]   (CONV: only the W regions; token rows are gathered per tap)
    int crd_t[2][2], crd_yx[2][2];  // CONV: per (token half, j) base input coordinates: t, and (y << 16) | (x & 0xffff)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = j * 64 + (tid >> 3);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int nrow = min(n0 + (r >> 6) * 128 + h * 64 + (r & 63), p.N - 1);
            const int mrow = min(m0 + (r >> 5) * 64 + h * 32 + (r & 31), p.M - 1);
            src[h ? 3 : 0][j] = p.W + (int64_t)nrow * p.ldw + src_chunk * 8;
            if (CONV) {
                const int to = mrow / (p.cv.Ho * p.cv.Wo);
                const int rem = mrow - to * (p.cv.Ho * p.cv.Wo);
                const int yo = rem / p.cv.Wo;
                const int xo = rem - yo * p.cv.Wo;
                crd_t[h][j] = to * p.cv.st + p.cv.ot;
                crd_yx[h][j] = ((yo * p.cv.sh + p.cv.oh) << 16) | ((xo * p.cv.sw + p.cv.ow) & 0xffff);
                src[h ? 2 : 1][j] = nullptr;
            } else {
                src[h ? 2 : 1][j] = p.A + (int64_t)mrow * p.lda + src_chunk * 8;
            }
        }
    }
    // CONV: K tile `tile` = (tap, channel tile kc); every region is issued once per K tile in increasing order, so each keeps
    // its own (kc, dt, dy, dx) odometer in scalars instead of dividing. Weights of tap (dt,dy,dx) start at W + tap*w_tap_stride.
    const int nkc = CONV ? p.K / BK : 1;
    int od_kc[4] = {0, 0, 0, 0}, od_tap[4] = {0, 0, 0, 0}, od_dt[4] = {0, 0, 0, 0}, od_dy[4] = {0, 0, 0, 0}, od_dx[4] = {0, 0, 0, 0};
    auto issue = [&](int region, int tile) __attribute__((always_inline)) {  // region compile-time after inlining
        char* dst = smem_raw + ((tile & 1) << 16) + region * 16384 + wave * 1024;
        if (!CONV) {
            const int k0 = tile * BK;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[region][j] + k0),
                                                 (__attribute__((address_space(3))) void*)(dst + j * 8192), 16, 0, 0);
            return;
        }
        const int k0 = od_kc[region] * BK;
        const bool is_w = region == 0 || region == 3;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bf16_t* a;
            if (is_w) {
                a = src[region][j] + (int64_t)od_tap[region] * p.cv.w_tap_stride + k0;
            } else {
                const int h = region - 1;
                int ti = crd_t[h][j] + od_dt[region];
                ti = ti < 0 ? 0 : ti;  // causal: the first frame is replicated in front
                const int yi = (crd_yx[h][j] >> 16) + od_dy[region];
                const int xi = (int)(short)(crd_yx[h][j] & 0xffff) + od_dx[region];
                const bool ok = ti < p.cv.Ti && yi >= 0 && yi < p.cv.Hi && xi >= 0 && xi < p.cv.Wi;
                a = ok ? p.A + (((int64_t)ti * p.cv.Hi + yi) * p.cv.Wi + xi) * p.lda + src_chunk * 8 + k0
                       : reinterpret_cast<const bf16_t*>(g3_zero_page) + src_chunk * 8;
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)a,
                                             (__attribute__((address_space(3))) void*)(dst + j * 8192), 16, 0, 0);
        }
        if (++od_kc[region] == nkc) {
            od_kc[region] = 0;
            ++od_tap[region];
            if (++od_dx[region] == p.cv.kw) {
                od_dx[region] = 0;
                if (++od_dy[region] == p.cv.kh) {
                    od_dy[region] = 0;
                    ++od_dt[region];
                }
            }
        }
    };

    // ---- fragment read addresses (bytes inside a slot): row*128 + ((2 ks + g) ^ ((row >> 1) & 7))*16
    unsigned koff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) koff[ks] = (unsigned)(l31 * 128 + (((2 * ks + g) ^ ((l31 >> 1) & 7)) << 4));
    const unsigned w_base = (unsigned)(wn * 64 * 128);  // + region*16384 + i*32*128
    const unsigned t_base = (unsigned)(wm * 32 * 128);

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    bf16x8 wf[2][4];  // current W half: [row block][k-step]
    bf16x8 tf[2][4];  // both token halves: [half][k-step]

    const int nk = CONV ? nkc * p.cv.ntaps : p.K / BK;
    const int nq = 4 * nk;

    auto read_w = [&](const char* sl, int region) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                wf[i][ks] = *reinterpret_cast<const bf16x8*>(sl + region * 16384 + w_base + i * 4096 + koff[ks]);
    };
    auto read_t = [&](const char* sl, int h) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) tf[h][ks] = *reinterpret_cast<const bf16x8*>(sl + (1 + h) * 16384 + t_base + koff[ks]);
    };

    // PH == 4: one accumulator quadrant (8 MFMAs) per phase, one half-tile issued per phase.
    auto phase4 = [&](auto PC, auto FULL, int t) __attribute__((always_inline)) {
        constexpr int P = decltype(PC)::value;
        G3_JITTER(wave + blockIdx.x, 4 * t + P);
        constexpr bool full = decltype(FULL)::value;
        const char* sl = smem_raw + ((t & 1) << 16);
        if (P == 0) {
            read_w(sl, 0);
            read_t(sl, 0);
        } else if (P == 1) {
            read_t(sl, 1);
        } else if (P == 2) {
            read_w(sl, 3);
        }
        const int f = 4 * t + P;
        if (full) {
            issue((P + 2) & 3, t + (P < 2 ? 1 : 2));
            wait_vmcnt<8>();
        } else {
            if (f + 6 < nq) issue((P + 2) & 3, t + (P < 2 ? 1 : 2));
            const int newest = min(f + 6, nq - 1);
            wait_vmcnt_rt(max(newest - (f + 2), 0));
        }
        phase_barrier();
        constexpr int ih = (P >= 2) ? 2 : 0;
        constexpr int jh = (P == 1 || P == 2) ? 1 : 0;
        G3_PP_SETPRIO(1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                acc[ih + i][jh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][ks], tf[jh][ks], acc[ih + i][jh], 0, 0, 0);
        G3_PP_SETPRIO(0);
        phase_barrier();
    };
    // PH == 2: one W half x both token halves (16 MFMAs) per phase, two half-tiles issued per phase. A buffer is restaged
    // one phase after its last read here, which is safe because the reads are retired (lgkmcnt(0)) BEFORE the reading
    // phase's first barrier - also for the wave group that runs a barrier behind.
    auto phase2 = [&](auto PC, auto FULL, int t) __attribute__((always_inline)) {
        constexpr int P = decltype(PC)::value;
        G3_JITTER(wave + blockIdx.x, 2 * t + P);
        constexpr bool full = decltype(FULL)::value;
        const char* sl = smem_raw + ((t & 1) << 16);
        if (P == 0) {
            read_w(sl, 0);
            read_t(sl, 0);
            read_t(sl, 1);
        } else {
            read_w(sl, 3);
        }
        const int q0 = 4 * t + (P == 0 ? 6 : 8);     // first of the two half-tiles this phase issues
        const int need = 4 * t + (P == 0 ? 3 : 6);   // newest half-tile the NEXT phase reads
        if (full) {
            issue(P == 0 ? 2 : 0, t + (P == 0 ? 1 : 2));
            issue(P == 0 ? 3 : 1, t + (P == 0 ? 1 : 2));
            wait_vmcnt<(P == 0 ? 8 : 6)>();
        } else {
            if (q0 < nq) {
                issue(P == 0 ? 2 : 0, t + (P == 0 ? 1 : 2));
                issue(P == 0 ? 3 : 1, t + (P == 0 ? 1 : 2));
            }
            const int newest = min(q0 + 1, nq - 1);
            wait_vmcnt_rt(max(newest - need, 0));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        phase_barrier();
        constexpr int ih = P * 2;
        G3_PP_SETPRIO(1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[ih + i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][ks], tf[j][ks], acc[ih + i][j], 0, 0, 0);
        G3_PP_SETPRIO(0);
        phase_barrier();
    };

    // ---- prologue: half-tiles 0..5; what the first phase reads has landed before anyone starts
    {
        const int n0q = min(6, nq);
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if (q < n0q) issue(q & 3, q >> 2);
        wait_vmcnt_rt(n0q - (PH == 4 ? 2 : 3));
        phase_barrier();
        if (wave >= 4) phase_barrier();  // stagger: waves 4..7 run half a phase behind waves 0..3
    }
    using std::integral_constant;
    using T_ = integral_constant<bool, true>;
    using F_ = integral_constant<bool, false>;
    int t = 0;
    if (PH == 4) {
        for (; t + 2 < nk; ++t) {
            phase4(integral_constant<int, 0>{}, T_{}, t);
            phase4(integral_constant<int, 1>{}, T_{}, t);
            phase4(integral_constant<int, 2>{}, T_{}, t);
            phase4(integral_constant<int, 3>{}, T_{}, t);
        }
        for (; t < nk; ++t) {
            phase4(integral_constant<int, 0>{}, F_{}, t);
            phase4(integral_constant<int, 1>{}, F_{}, t);
            phase4(integral_constant<int, 2>{}, F_{}, t);
            phase4(integral_constant<int, 3>{}, F_{}, t);
        }
    } else {
        for (; t + 2 < nk; ++t) {
            phase2(integral_constant<int, 0>{}, T_{}, t);
            phase2(integral_constant<int, 1>{}, T_{}, t);
        }
        for (; t < nk; ++t) {
            phase2(integral_constant<int, 0>{}, F_{}, t);
            phase2(integral_constant<int, 1>{}, F_{}, t);
        }
    }
    if (wave < 4) phase_barrier();

    if (p.wide_store) store_tile_lds<EPI>(p, acc, m0 + m_w0, n0 + n_w0, lane, smem_raw + wave * 16384);
    else store_tile<EPI>(p, acc, m0 + m_w0, n0 + n_w0, l31, g);
}
// The one-wave-per-SIMD kernels (gemm_w4.hpp, gemm_w4e.hpp) keep the LDS-DMA source of a tile row as a 32-bit byte offset from the tile's first row:
// row 255 and its last 16-byte chunk must lie below 4 GiB - 255 ld 2 + 128 < 2^32 for lda and ldw. Beyond that (host: gemm_choose, w4e_applies) the
// call runs on the ping-pong / classic kernels, which form 64-bit pointers per row - and so does one with a negative lda or ldw, which an unsigned
// 32-bit offset cannot express either.
static bool w4_tile_rows_addressable(const GemmParams& p) {
    const int64_t ld_max = ((1ll << 32) - 129) / 510;
    return p.lda >= 0 && p.lda <= ld_max && p.ldw >= 0 && p.ldw <= ld_max;
}
#include "gemm_w4.hpp"
#include "gemm_w4_conv.hpp"
#include "gemm_w4e.hpp"

/* ---- host side: every public entry point fills ONE call record (g3_gemm_call, gen3c_hip.h); gemm_plan turns it into a refusal or into the kernel's
 * parameters, its row of the ONE kernel table, the grid and the entry's follow-up launches; gemm_launch launches that. g3_gemm_plan_bf16 and
 * g3_gemm_kernel_name ask the same code. ------------------------------------------------------------------------------------------------------ */

// The kernel table: one row per instantiation = family x epilogue. The reported names, the dynamic-LDS grant and the launch all come from here.
struct GemmKernel { const char* name; void (*fn)(GemmParams); int threads, lds; const char* family; };
constexpr int GEMM_LDS_BYTES = 2 * (BM + BN) * BK * (int)sizeof(bf16_t);  // 128 KiB: two stages of both operand tiles (= 2 * GW4_STAGE_BYTES)
// epilogue lists, as the numerals of the EPI_* codes so that a row's name is the instantiation's own; a family's rows follow its list
#define G3_EPI_ALL(X, ...) X(0, __VA_ARGS__) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__)
#define G3_EPI_ALL_QK(X, ...) G3_EPI_ALL(X, __VA_ARGS__) X(5, __VA_ARGS__)
#define G3_EPI_DEFERRED(X, ...) X(0, __VA_ARGS__) X(1, __VA_ARGS__) X(2, __VA_ARGS__)
#define G3_EPI_CONV(X, ...) X(0, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__)
// F(row id stem, epilogue list, threads, LDS bytes, family as g3_gemm_kernel_name reports it, kernel template, its arguments behind EPI)
#define G3_GEMM_FAMILIES(F) \
    F(GK_W4E, DEFERRED, GW4_THREADS, GW4E_LDS_BYTES, "gemm_bf16_nt_w4e_kernel<EPI>", gemm_bf16_nt_w4e_kernel, false) \
    F(GK_W4E_TF, DEFERRED, GW4_THREADS, GW4E_LDS_BYTES, "gemm_bf16_nt_w4e_kernel<EPI>", gemm_bf16_nt_w4e_kernel, true) \
    F(GK_W4, ALL_QK, GW4_THREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_w4_kernel<EPI>", gemm_bf16_nt_w4_kernel, false) \
    F(GK_W4_PERSIST, ALL, GW4_THREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_w4_kernel<EPI>", gemm_bf16_nt_w4_kernel, true) \
    F(GK_W4_CONV, CONV, GW4_THREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_w4_conv_kernel<EPI>", gemm_bf16_nt_w4_conv_kernel) \
    F(GK_PP2, ALL, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_pp_kernel<EPI, 2, false>", gemm_bf16_nt_pp_kernel, 2, false) \
    F(GK_PP2_CONV, CONV, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_pp_kernel<EPI, 2, true>", gemm_bf16_nt_pp_kernel, 2, true) \
    F(GK_PP4, ALL, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_pp_kernel<EPI, 4, false>", gemm_bf16_nt_pp_kernel, 4, false) \
    F(GK_REG, ALL, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_kernel<EPI, false, false, PIN>", gemm_bf16_nt_kernel, false, false, false) \
    F(GK_REG_PIN, ALL, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_kernel<EPI, false, false, PIN>", gemm_bf16_nt_kernel, false, false, true) \
    F(GK_GLDS, ALL, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_kernel<EPI, true, false, PIN>", gemm_bf16_nt_kernel, true, false, false) \
    F(GK_GLDS_PIN, ALL, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_kernel<EPI, true, false, PIN>", gemm_bf16_nt_kernel, true, false, true) \
    F(GK_REG_CONV, CONV, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_kernel<EPI, false, true, PIN>", gemm_bf16_nt_kernel, false, true, false) \
    F(GK_REG_CONV_PIN, CONV, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_kernel<EPI, false, true, PIN>", gemm_bf16_nt_kernel, false, true, true) \
    F(GK_GLDS_CONV, CONV, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_kernel<EPI, true, true, PIN>", gemm_bf16_nt_kernel, true, true, false) \
    F(GK_GLDS_CONV_PIN, CONV, NTHREADS, GEMM_LDS_BYTES, "gemm_bf16_nt_kernel<EPI, true, true, PIN>", gemm_bf16_nt_kernel, true, true, true)
#define G3_STR(...) #__VA_ARGS__
#define G3_GEMM_IDS(ID, EPIS, ...) G3_EPI_##EPIS(G3_GEMM_ID, ID)
#define G3_GEMM_ID(E, ID) ID##_##E,
#define G3_GEMM_ROWS(ID, EPIS, ...) G3_EPI_##EPIS(G3_GEMM_ROW, __VA_ARGS__)
#define G3_GEMM_ROW(E, THREADS, LDS, FAMILY, KERNEL, ...) {G3_STR(KERNEL<E, ##__VA_ARGS__>), &KERNEL<E, ##__VA_ARGS__>, THREADS, LDS, FAMILY},
enum GemmKernelId { G3_GEMM_FAMILIES(G3_GEMM_IDS) GK_COUNT };  // GK_<family>_<epilogue>; a family's first row is GK_<family>_0
const GemmKernel gemm_kernels[GK_COUNT] = {G3_GEMM_FAMILIES(G3_GEMM_ROWS)};
// The twins of the GK_W4E / GK_W4E_TF rows with the K loop on v_mfma_f32_16x16x32_bf16 (gemm_w4e.hpp), [tokens first][epilogue]: gemm_launch starts them from
// those rows where p.mfma16 is set. No rows of their own: the plan, the names and the grid do not depend on the option, and the bits are the same.
void (*const gemm_w4e16_twins[2][3])(GemmParams) = {
    {&gemm_bf16_nt_w4e16_kernel<0, false>, &gemm_bf16_nt_w4e16_kernel<1, false>, &gemm_bf16_nt_w4e16_kernel<2, false>},
    {&gemm_bf16_nt_w4e16_kernel<0, true>, &gemm_bf16_nt_w4e16_kernel<1, true>, &gemm_bf16_nt_w4e16_kernel<2, true>}};
#undef G3_GEMM_IDS
#undef G3_GEMM_ID
#undef G3_GEMM_ROWS
#undef G3_GEMM_ROW

int device_cu_count() {  // cached per device (sizes the persistent grids); 0 without a device
    static int n_cu[G3_MAX_DEVICES] = {};
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= G3_MAX_DEVICES) return 0;
    std::lock_guard<std::mutex> lock(mu);
    if (!n_cu[dev]) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        n_cu[dev] = cus;
    }
    return n_cu[dev];
}

// CONV on the one-wave-per-SIMD kernel (gemm_w4_conv.hpp): whole 64-channel tiles, >= 2 K tiles, K * 2 bytes inside the zero page,
// <= 32 spatial taps (bit masks), full-line epilogue, activation span addressable with 32-bit row * lda products
bool conv_w4_applies(const GemmParams& p) {
    const int64_t in_rows = (int64_t)p.cv.Ti * p.cv.Hi * p.cv.Wi;
    return g3_opt_conv_w4 && (p.K % BK) == 0 && !g3_opt_gemm_regstage && p.wide_store && (p.K / BK) * p.cv.ntaps >= 2 && p.K * 2 <= G3_ZERO_PAGE_BYTES &&
           p.cv.kh * p.cv.kw <= 32 && in_rows < (1ll << 31) && p.lda * 2 < (1ll << 31) && p.cv.w_tap_stride * 2 < (1ll << 32);
}

// The whole kernel choice: the FIRST row of the family that runs p with epilogue epi (the row itself is that plus the epilogue's place in the family's
// list) and the grid. Reads the shapes, strides and wide_store of p and the options only.
int gemm_choose(const GemmParams& p, int epi, bool conv, int n_cu, int& grid) {
    const bool glds = (p.K % BK) == 0 && !g3_opt_gemm_regstage;
    const int nblk = p.tiles_m * p.tiles_n;
    grid = nblk;
    if (conv) {
        if (conv_w4_applies(p)) return GK_W4_CONV_0;
    } else if (glds && g3_opt_gemm_pingpong == 3) {
        // persistent forms: one workgroup per CU (a multiple of 8 keeps a workgroup's tiles on its XCD's band of the XCD-aware order)
        const int grid_cu = (n_cu / 8) * 8;
        if ((epi == EPI_NONE || epi == EPI_GELU || epi == EPI_GATED_RESIDUAL) && w4e_applies(p, epi, n_cu)) {  // deferred epilogue (gemm_w4e.hpp)
            // (tests: g3_set_option("gemm_deferred_grid", g) runs the tile loop on g workgroups - any multiple of 8 that leaves every workgroup a tile -
            // to walk long and uneven tile lists; 0 = one workgroup per CU)
            const int g = g3_opt_gemm_deferred_grid;
            grid = (g >= 8 && (g % 8) == 0 && g <= nblk) ? g : grid_cu;
            // piece order, g3_set_option("gemm_tokens_first", 0 / 1 / 2): never / always / (default) where few feature tiles share a token panel (N <= 4096: its
            // rows are fetched from HBM by the first of at most 16 workgroups and everybody waits for them) - measured (profiles/r5_gemm_tokens_first_ab.txt):
            // out-projection +1 %, MLP-down +1.5 %; QKV (N = 12 288) -3.5 %, MLP-up (N = 16 384) -1 % -> those keep the weights-first order
            const bool tf = g3_opt_gemm_tokens_first == 1 || (g3_opt_gemm_tokens_first == 2 && p.N <= 4096);
            return tf ? GK_W4E_TF_0 : GK_W4E_0;
        }
        // one wave per SIMD (gemm_w4.hpp): whole 64-wide K tiles, at least two, full-line epilogue, tile rows inside the 32-bit source offsets
        if (p.wide_store && p.K >= 2 * BK && w4_tile_rows_addressable(p)) {
            // persistent only where a workgroup gets at least two tiles (the norm / RoPE epilogue's tables do not fit beside the tile state: no such form)
            if (epi != EPI_QK_NORM_ROPE && g3_opt_gemm_persistent && grid_cu >= 8 && nblk >= 2 * grid_cu) {
                grid = grid_cu;
                return GK_W4_PERSIST_0;
            }
            return GK_W4_0;
        }
    }
    if (glds && g3_opt_gemm_pingpong >= 2) return conv ? GK_PP2_CONV_0 : GK_PP2_0;
    if (!conv && glds && g3_opt_gemm_pingpong) return GK_PP4_0;
    static const GemmKernelId classic[2][2][2] = {{{GK_REG_PIN_0, GK_REG_0}, {GK_GLDS_PIN_0, GK_GLDS_0}},  // [conv][glds][unpinned]
                                                  {{GK_REG_CONV_PIN_0, GK_REG_CONV_0}, {GK_GLDS_CONV_PIN_0, GK_GLDS_CONV_0}}};
    return classic[conv][glds][g3_opt_gemm_unpinned != 0];
}

struct GemmPlan { GemmParams p; int row, grid; unsigned follow_up; const char* what; };  // what: the name g3_check_launch reports

// Every check of a call, the one fill of GemmParams and the kernel choice; G3_OK and a filled plan, or the refusal (g3_set_error). No HIP call, and no
// operand is dereferenced: n_cu comes from the caller.
int gemm_plan(const g3_gemm_call& call, int n_cu, GemmPlan& plan) {
    g3_gemm_call c = call;  // (normalised below: what the entry does not take, and what it derives)
    const bool conv = c.entry == G3_GEMM_ENTRY_CONV || c.entry == G3_GEMM_ENTRY_CONV_GNSTATS, qk = c.entry == G3_GEMM_ENTRY_QK_NORM_ROPE;
    auto at = [](const void* ptr) { return (uintptr_t)ptr; };
    if (qk) {
        if (!c.A || !c.W || !c.C) return g3_set_error(G3_ERR_ARG, "g3_gemm_qk_norm_rope_bf16: null operand");
        if (c.M <= 0 || c.N <= 0 || c.K <= 0 || c.B <= 0 || (c.M % c.B))
            return g3_set_error(G3_ERR_ARG, "g3_gemm_qk_norm_rope_bf16: bad shape M=%d N=%d K=%d B=%d", c.M, c.N, c.K, c.B);
        if (c.n_q < 0 || c.n_k < 0 || (c.n_q % 128) || (c.n_k % 128) || c.n_q + c.n_k > c.N || (c.N % 128))
            return g3_set_error(G3_ERR_ARG, "g3_gemm_qk_norm_rope_bf16: q / k feature ranges must be whole 128-wide heads inside N (n_q=%d n_k=%d N=%d)", c.n_q, c.n_k, c.N);
        if ((c.n_q && !c.norm_q) || (c.n_k && !c.norm_k)) return g3_set_error(G3_ERR_ARG, "g3_gemm_qk_norm_rope_bf16: missing norm weight");
        if ((c.cos_table == nullptr) != (c.sin_table == nullptr)) return g3_set_error(G3_ERR_ARG, "g3_gemm_qk_norm_rope_bf16: need both cos and sin tables or neither");
        if ((c.K & 7) || (c.lda & 7) || (c.ldw & 7) || (c.ldc & 7)) return g3_set_error(G3_ERR_ARG, "g3_gemm_qk_norm_rope_bf16: K, lda, ldw, ldc must be multiples of 8");
        if (((at(c.A) | at(c.W) | at(c.C)) & 15) || ((at(c.norm_q) | at(c.norm_k)) & 15) || ((at(c.cos_table) | at(c.sin_table)) & 15))
            return g3_set_error(G3_ERR_ARG, "g3_gemm_qk_norm_rope_bf16: operands must be 16-byte aligned");
        if (c.vt && (c.N - c.n_q - c.n_k <= 0 || (c.vt_ld & 7) || c.vt_ld < c.M / c.B || (at(c.vt) & 15)))
            return g3_set_error(G3_ERR_ARG, "g3_gemm_qk_norm_rope_bf16: V^T destination needs v heads, vt_ld %% 8 == 0, vt_ld >= S and 16-byte alignment");
        c.epilogue = EPI_QK_NORM_ROPE; c.gate = c.residual = nullptr; c.ldg = c.ldr = 0;
    } else if (conv) {
        if (c.entry == G3_GEMM_ENTRY_CONV_GNSTATS) {
            if (!c.gn_stats || c.gn_rows <= 0 || (at(c.gn_stats) & 7)) return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_gnstats_bf16: bad statistics buffer");
            if (((int64_t)c.To * c.Ho * c.Wo) % c.gn_rows) return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_gnstats_bf16: gn_rows_per_frame must divide the output rows");
        } else {
            c.gn_stats = nullptr;
        }
        if (!c.A || !c.W || !c.C) return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_bf16: null operand");
        if (c.K <= 0 || c.N <= 0 || (c.K & 7) || (c.lda & 7) || (c.ldw & 7) || (c.N & 3) || (c.ldc & 3))
            return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_bf16: need K, ld_in, ldw %% 8 == 0 and N, ld_out %% 4 == 0 (K=%d N=%d)", c.K, c.N);
        if (c.Ti <= 0 || c.Hi <= 0 || c.Wi <= 0 || c.To <= 0 || c.Ho <= 0 || c.Wo <= 0 || c.kt <= 0 || c.kh <= 0 || c.kw <= 0 || c.st <= 0 || c.sh <= 0 || c.sw <= 0)
            return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_bf16: bad geometry");
        if ((int64_t)c.To * c.Ho * c.Wo > 0x7fffffffLL) return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_bf16: too many output positions");
        if (((at(c.A) | at(c.W)) & 15) || (at(c.C) & 7)) return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_bf16: misaligned pointer");
        if (c.residual && ((c.ldr & 3) || (at(c.residual) & 7))) return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_bf16: misaligned residual");
        if (c.residual && !c.gate) return g3_set_error(G3_ERR_ARG, "g3_conv3d_cl_bf16: residual without bias is not instantiated");
        c.M = c.To * c.Ho * c.Wo; c.epilogue = c.residual ? EPI_BIAS_RESIDUAL : c.gate ? EPI_BIAS : EPI_NONE; c.ldg = 0;
    } else {
        const bool gate_ok = c.gate && !(c.ldg & 3) && !(at(c.gate) & 7), gate_residual_ok = gate_ok && c.residual && !(c.ldr & 3) && !(at(c.residual) & 7);
        if (!c.A || !c.W || !c.C) return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: null operand");
        if (c.M <= 0 || c.N <= 0 || c.K <= 0) return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: bad shape M=%d N=%d K=%d", c.M, c.N, c.K);
        if ((c.K & 7) || (c.lda & 7) || (c.ldw & 7) || (c.N & 3) || (c.ldc & 3))
            return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: need K,lda,ldw %% 8 == 0 and N,ldc %% 4 == 0 (K=%d lda=%lld ldw=%lld N=%d ldc=%lld)",
                                c.K, (long long)c.lda, (long long)c.ldw, c.N, (long long)c.ldc);
        if ((at(c.A) | at(c.W)) & 15) return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: A/W must be 16-byte aligned");
        if (at(c.C) & 7) return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: C must be 8-byte aligned");
        if (c.epilogue == EPI_GATED_RESIDUAL && !gate_residual_ok)
            return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: gated-residual epilogue needs 8-byte aligned gate+residual");
        if (c.epilogue == EPI_BIAS && !gate_ok) return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: bias epilogue needs bias");
        if (c.epilogue == EPI_BIAS_RESIDUAL && !gate_residual_ok)
            return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: bias-residual epilogue needs 8-byte aligned bias+residual");
        if (c.epilogue < EPI_NONE || c.epilogue > EPI_BIAS_RESIDUAL) return g3_set_error(G3_ERR_ARG, "g3_gemm_bf16_nt: unknown epilogue %d", c.epilogue);
    }
    if (c.entry != G3_GEMM_ENTRY_NT) c.gate_rows = 1;

    GemmParams& p = plan.p;
    p = GemmParams{};
    p.A = (const bf16_t*)c.A; p.lda = c.lda; p.W = (const bf16_t*)c.W; p.ldw = c.ldw; p.C = (bf16_t*)c.C; p.ldc = c.ldc;
    p.M = c.M; p.N = c.N; p.K = c.K;
    p.gate = (const bf16_t*)c.gate; p.gate_rows = c.gate_rows > 0 ? c.gate_rows : 1; p.ldg = c.ldg;
    p.R = (const bf16_t*)c.residual; p.ldr = c.ldr;
    p.tiles_m = (c.M + BM - 1) / BM; p.tiles_n = (c.N + BN - 1) / BN;
    p.tile_order_rowmajor = g3_opt_gemm_rowmajor_tiles;
    p.mfma16 = g3_opt_gemm_mfma16 != 0;
    p.wide_store = g3_opt_gemm_wide_store && !(c.N & 7) && !(c.ldc & 7) && !(at(c.C) & 15) && (!c.gate || (!(c.ldg & 7) && !(at(c.gate) & 15))) &&
                   (!c.residual || (!(c.ldr & 7) && !(at(c.residual) & 15)));
    if (conv) p.cv = ConvGeom{c.To, c.Ho, c.Wo, c.Ti, c.Hi, c.Wi, c.kt, c.kh, c.kw, c.st, c.sh, c.sw, c.ot, c.oh, c.ow, c.kt * c.kh * c.kw, (int64_t)c.N * c.ldw, g3_opt_conv_w4 != 2};

    const int first = gemm_choose(p, c.epilogue, conv, n_cu, plan.grid);
    plan.follow_up = 0;
    plan.what = qk ? "g3_gemm_qk_norm_rope_bf16" : conv ? "g3_conv3d_cl_bf16" : "g3_gemm_bf16_nt";
    if (qk) {
        // The norm / RoPE epilogue exists on the one-wave-per-SIMD kernel only. Where the choice is another family it is the plain entry's for these operands (the
        // deferred form applies to nothing the one-wave kernel does not): that kernel without epilogue, then the standalone passes over C in place.
        const bool fused = first == GK_W4_0, vt_fused = fused && c.vt && (c.B == 1 || c.B == 2 || c.B == 4);
        const int S = c.M / c.B, n_v = c.N - c.n_q - c.n_k;
        if (fused) {
            p.nw_q = (const bf16_t*)c.norm_q; p.nw_k = (const bf16_t*)c.norm_k; p.rope_cos = c.cos_table; p.rope_sin = c.sin_table;
            p.n_q = c.n_q; p.n_k = c.n_k; p.rope_B = c.B; p.rms_eps = c.eps;
            p.vt = vt_fused ? (bf16_t*)c.vt : nullptr; p.vt_ld = c.vt_ld; p.vt_batch = (int64_t)(n_v / 128) * 128 * c.vt_ld; p.vt_S = S;
        } else {
            c.epilogue = EPI_NONE;
            plan.what = "g3_gemm_bf16_nt";
            plan.follow_up = (c.n_q ? G3_GEMM_THEN_NORM_Q : 0) | (c.n_k ? G3_GEMM_THEN_NORM_K : 0);
        }
        if (c.vt && !vt_fused) plan.follow_up |= G3_GEMM_THEN_VT;  // (the fused form leaves C's v columns unwritten only where it writes V^T)
    }
    if (c.gn_stats && conv) {
        // GroupNorm statistics of the output: in the one-wave kernel's epilogue when it runs (and a frame is at least one wave quadrant of rows), else by the
        // statistics pass over the finished output
        if (c.gn_rows >= 128 && first == GK_W4_CONV_0) { p.gn_stats = (double*)c.gn_stats; p.gn_rows = c.gn_rows; }
        else plan.follow_up = G3_GEMM_THEN_GN_STATS;
    }
    plan.row = first + (conv && c.epilogue ? c.epilogue - 2 : c.epilogue);  // the epilogue's place in the family's list (G3_EPI_CONV: 0, 3, 4)
    return G3_OK;
}

int gemm_launch(const g3_gemm_call& c) {
    GemmPlan plan;
    if (int rc = gemm_plan(c, device_cu_count(), plan)) return rc;
    const GemmKernel& k = gemm_kernels[plan.row];
    const GemmParams& p = plan.p;
    static bool granted[GK_COUNT][G3_MAX_DEVICES] = {}, granted16[6][G3_MAX_DEVICES] = {};
    void (*fn)(GemmParams) = k.fn;
    bool (*grant)[G3_MAX_DEVICES] = &granted[plan.row];
    if (p.mfma16 && plan.row >= GK_W4E_0 && plan.row <= GK_W4E_TF_2) {  // the deferred kernel's 16x16x32 twin (gemm_w4e16_twins)
        const int t = plan.row - GK_W4E_0;
        fn = gemm_w4e16_twins[t / 3][t % 3];
        grant = &granted16[t];
    }
    if (int rc = g3_grant_dynamic_lds(reinterpret_cast<const void*>(fn), k.lds, *grant, "gemm")) return rc;
    hipLaunchKernelGGL(fn, dim3(plan.grid), dim3(k.threads), k.lds, (hipStream_t)c.stream, p);
    int rc = g3_check_launch(plan.what);
    const int S = c.B > 0 ? p.M / c.B : 0;
    if (rc == G3_OK && (plan.follow_up & G3_GEMM_THEN_NORM_Q))
        rc = g3_qk_rmsnorm_rope_bf16(p.C, p.ldc, c.norm_q, c.cos_table, c.sin_table, p.C, p.ldc, S, c.B, c.n_q / 128, 128, c.eps, c.stream);
    if (rc == G3_OK && (plan.follow_up & G3_GEMM_THEN_NORM_K))
        rc = g3_qk_rmsnorm_rope_bf16(p.C + c.n_q, p.ldc, c.norm_k, c.cos_table, c.sin_table, p.C + c.n_q, p.ldc, S, c.B, c.n_k / 128, 128, c.eps, c.stream);
    if (rc == G3_OK && (plan.follow_up & G3_GEMM_THEN_VT))
        rc = g3_transpose_v_bf16(p.C + c.n_q + c.n_k, p.ldc, c.vt, c.vt_ld, S, c.B, (p.N - c.n_q - c.n_k) / 128, 128, c.stream);
    if (rc == G3_OK && (plan.follow_up & G3_GEMM_THEN_GN_STATS))
        rc = g3_groupnorm_stats_cl_bf16(p.C, p.ldc, c.gn_stats, p.M / c.gn_rows, c.gn_rows, p.N, c.stream);
    return rc;
}

}  // namespace

extern "C" int g3_gemm_bf16_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M,
                               int N, int K, int epilogue, const void* gate, int gate_rows, int64_t ldg,
                               const void* residual, int64_t ldr, void* stream) {
    g3_gemm_call c{};
    c.entry = G3_GEMM_ENTRY_NT;
    c.A = A; c.lda = lda; c.W = W; c.ldw = ldw; c.C = C; c.ldc = ldc; c.M = M; c.N = N; c.K = K;
    c.epilogue = epilogue; c.gate = gate; c.gate_rows = gate_rows; c.ldg = ldg; c.residual = residual; c.ldr = ldr; c.stream = stream;
    return gemm_launch(c);
}

// Name of the kernel family g3_gemm_bf16_nt / g3_gemm_qk_norm_rope_bf16 launch for this shape under the options in force (16-byte aligned,
// 8-element-strided operands assumed - what the DiT passes): for profilers and bench.py's roofline_gemm line, never needed to run the op.
// The plan's own choice code on those canonical operands; g3_gemm_plan_bf16 is the exact answer for a given call.
extern "C" const char* g3_gemm_kernel_name(int M, int N, int K, int epilogue) {
    GemmParams p{};
    p.M = M; p.N = N; p.K = K; p.gate_rows = 1; p.ldc = p.ldr = p.ldg = N;
    p.wide_store = g3_opt_gemm_wide_store && !(N & 7);
    p.tiles_m = (M + BM - 1) / BM; p.tiles_n = (N + BN - 1) / BN;
    int grid;
    return gemm_kernels[gemm_choose(p, epilogue, false, device_cu_count(), grid)].family;
}

extern "C" const char* g3_gemm_plan_bf16(const g3_gemm_call* call, int n_cu, int* grid, unsigned* follow_up) {
    if (!call || call->entry < G3_GEMM_ENTRY_NT || call->entry > G3_GEMM_ENTRY_CONV_GNSTATS) {
        g3_set_error(G3_ERR_ARG, "g3_gemm_plan_bf16: unknown entry %d", call ? call->entry : -1);
        return nullptr;
    }
    GemmPlan plan;
    if (gemm_plan(*call, n_cu > 0 ? n_cu : device_cu_count(), plan)) return nullptr;
    if (grid) *grid = plan.grid;
    if (follow_up) *follow_up = plan.follow_up;
    return gemm_kernels[plan.row].name;
}

// Q / K projection with the per-head RMSNorm (+ RoPE) of the reference's Attention.cal_qkv (attention.py:247-280) in the epilogue:
//   C[:, 0:n_q]         = rope(rmsnorm(A W^T, norm_q))     C[:, n_q:n_q+n_k] = rope(rmsnorm(A W^T, norm_k))     C[:, n_q+n_k:] = A W^T
// With vt != NULL the remaining (v) heads are written TRANSPOSED into vt [B][H_v][128][vt_ld] (g3_transpose_v_bf16's layout, zero beyond S)
// and their columns of C are left untouched.
// Row m is token (s = m / B, b = m % B); cos / sin are fp32 [S][128] (NULL: no RoPE - cross-attention). Same rounding points as
// g3_gemm_bf16_nt followed by g3_qk_rmsnorm_rope_bf16 in place, which is also what runs when the one-wave-per-SIMD kernel does not apply.
extern "C" int g3_gemm_qk_norm_rope_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                                         int n_q, int n_k, const void* norm_q, const void* norm_k, const float* cos_table,
                                         const float* sin_table, int B, float eps, void* vt, int64_t vt_ld, void* stream) {
    g3_gemm_call c{};
    c.entry = G3_GEMM_ENTRY_QK_NORM_ROPE;
    c.A = A; c.lda = lda; c.W = W; c.ldw = ldw; c.C = C; c.ldc = ldc; c.M = M; c.N = N; c.K = K;
    c.n_q = n_q; c.n_k = n_k; c.norm_q = norm_q; c.norm_k = norm_k; c.cos_table = cos_table; c.sin_table = sin_table; c.B = B; c.eps = eps;
    c.vt = vt; c.vt_ld = vt_ld; c.stream = stream;
    return gemm_launch(c);
}

// Causal 3-D convolution as an implicit GEMM over channels-last activations.
//   in  [Ti*Hi*Wi][ld_in]  (C_in = K valid channels per position), w [kt*kh*kw][N][ldw] (tap-major, K contiguous),
//   out [To*Ho*Wo][ld_out]; bias [N] (may be NULL), residual [To*Ho*Wo][ldr] (may be NULL) added after the bias.
// g3_conv3d_cl_gnstats_bf16 additionally ADDS, per output frame (gn_rows_per_frame consecutive output rows = Ho * Wo), the sum and the sum of squares of
// the stored bf16 outputs to gn_stats[frame][0 / 1] (doubles; the caller zeroes them): the statistics CausalNormalize needs of this tensor
// (tokenizer/modules/utils.py:58-83), so that the following g3_groupnorm_apply_cl_bf16 does not have to read the tensor twice.
static int conv3d_cl(int entry, const void* in, int64_t ld_in, const void* w, int64_t ldw, const void* bias, const void* residual, int64_t ldr, void* out,
                     int64_t ld_out, int K, int N, int Ti, int Hi, int Wi, int To, int Ho, int Wo, int kt, int kh, int kw, int st, int sh, int sw, int ot,
                     int oh, int ow, void* gn_stats_f64, int gn_rows_per_frame, void* stream) {
    g3_gemm_call c{};
    c.entry = entry;
    c.A = in; c.lda = ld_in; c.W = w; c.ldw = ldw; c.C = out; c.ldc = ld_out; c.N = N; c.K = K; c.gate = bias; c.residual = residual; c.ldr = ldr;
    c.Ti = Ti; c.Hi = Hi; c.Wi = Wi; c.To = To; c.Ho = Ho; c.Wo = Wo; c.kt = kt; c.kh = kh; c.kw = kw; c.st = st; c.sh = sh; c.sw = sw; c.ot = ot; c.oh = oh; c.ow = ow;
    c.gn_stats = gn_stats_f64; c.gn_rows = gn_rows_per_frame; c.stream = stream;
    return gemm_launch(c);
}

extern "C" int g3_conv3d_cl_bf16(const void* in, int64_t ld_in, const void* w, int64_t ldw, const void* bias, const void* residual,
                                 int64_t ldr, void* out, int64_t ld_out, int K, int N, int Ti, int Hi, int Wi, int To, int Ho,
                                 int Wo, int kt, int kh, int kw, int st, int sh, int sw, int ot, int oh, int ow, void* stream) {
    return conv3d_cl(G3_GEMM_ENTRY_CONV, in, ld_in, w, ldw, bias, residual, ldr, out, ld_out, K, N, Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw, st, sh, sw, ot, oh, ow,
                     nullptr, 0, stream);
}

extern "C" int g3_conv3d_cl_gnstats_bf16(const void* in, int64_t ld_in, const void* w, int64_t ldw, const void* bias, const void* residual,
                                         int64_t ldr, void* out, int64_t ld_out, int K, int N, int Ti, int Hi, int Wi, int To, int Ho,
                                         int Wo, int kt, int kh, int kw, int st, int sh, int sw, int ot, int oh, int ow, void* gn_stats_f64,
                                         int gn_rows_per_frame, void* stream) {
    return conv3d_cl(G3_GEMM_ENTRY_CONV_GNSTATS, in, ld_in, w, ldw, bias, residual, ldr, out, ld_out, K, N, Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw, st, sh, sw, ot, oh, ow,
                     gn_stats_f64, gn_rows_per_frame, stream);
}
