// Per-head choice among the patterns of a range table (g3_self_attn_fwd_ranges_bf16), made on the device from the activations of the running forward:
// the function, the criterion and the refusals are written down in include/gen3c_hip.h (g3_attn_pattern_profile_bf16, g3_attn_pattern_select).
//
//   attn_pattern_profile_kernel   grid (key chunk, head, batch), 4 waves. Every wave keeps the up-to-64 sampled Q rows of its (b, h) as the B operand of
//                                 mfma_f32_32x32x16_bf16 for its whole life (64 VGPRs) and walks the 64-key tiles wave, wave + 4, ... of its chunk: the K rows
//                                 come straight from global memory in the A operand's lane map (lane (c, hf) owns key c's elements 8 hf .. 8 hf + 7 of every
//                                 16-element k step: one 16-byte load each), in units of 32 keys with the next unit's loads issued before this unit's MFMAs. S^T = K Qs^T
//                                 puts a sample row on the lane pair (c, c + 32) and a unit's 32 logits in 16 registers of each: row maximum and row sum
//                                 are in-lane plus ONE cross-lane exchange. The unit's row sum goes - the same value, the same operation - into the dense
//                                 accumulator and into the accumulator of every pattern whose bit the host-built tile_member byte carries, so a pattern that
//                                 holds every tile keeps accumulators that equal the dense one bit for bit, through every merge. The 4 waves merge in LDS in
//                                 wave order; one partial (m, dense, sum_0 .. sum_7) per (b, h, chunk, row) goes to the workspace.
//   attn_pattern_merge_kernel     merges the chunks of a (b, h, row) in ascending order and writes recall = sum_p / dense.
//   attn_pattern_select_kernel    score[h][p] = mean of recall over (b, i) in that order; head_pattern[h] = the first maximum.
// No atomics, no dependence on the launch's timing: two launches over the same operands give the same bits.
//
// Plain C++ with builtins, not hand-scheduled: at the product shape the work is 64 of 56 320 query rows, 1/880 of the dense launch, and the kernel is bound
// by its one read of K.
#include "common.hpp"
#include "gen3c_hip.h"

#define PRF_THREADS 256
#define PRF_WAVES 4
#define PRF_ROWS 64        // sampled rows a workgroup holds (padded)
#define PRF_KT 64          // keys per tile (the attention kernel's)
#define PRF_QBLK 256       // query rows per block of the range table (g3_self_attn_window_q_rows())
#define PRF_MAXP 8         // patterns: the bits of a tile_member byte
#define PRF_REC (2 + PRF_MAXP)  // floats of a partial: m, dense, sum_p
// "no key yet": finite, so that the merge of two empty partials is exp2(0) * 0 and never inf - inf
#define PRF_M_EMPTY (-3.0e38f)

// a <- a (+) b, the partials of two disjoint key sets of one row. The dense accumulator and every pattern's go through the same two factors.
G3_DEVICE void prf_merge(float& m, float& dn, float (&sp)[PRF_MAXP], float mb, float db, const float (&sb)[PRF_MAXP]) {
    const float mn = fmaxf(m, mb);
    const float fa = __builtin_amdgcn_exp2f(m - mn), fb = __builtin_amdgcn_exp2f(mb - mn);
    dn = dn * fa + db * fb;
#pragma unroll
    for (int p = 0; p < PRF_MAXP; ++p) sp[p] = sp[p] * fa + sb[p] * fb;
    m = mn;
}

// the A-operand fragments of the 32 keys from key0: [k step]
G3_DEVICE void prf_load_k(bf16x8 (&kf)[8], const char* kb, uint32_t k_row_bytes, int key0, int c, int hf) {
    const char* p = kb + (uint32_t)(key0 + c) * k_row_bytes + 16 * hf;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(p + 32 * ks);
}

__global__ __launch_bounds__(PRF_THREADS, 2) void attn_pattern_profile_kernel(const bf16_t* __restrict__ q, uint32_t q_row_bytes, int64_t q_batch, int64_t q_head,
                                                                            const bf16_t* __restrict__ k, uint32_t k_row_bytes, int64_t k_batch, int64_t k_head,
                                                                            int S, int H, float scale_log2, const int32_t* __restrict__ sample_rows, int n,
                                                                            const uint8_t* __restrict__ tile_member, int n_chunks, float* __restrict__ ws) {
    __shared__ float part[PRF_WAVES][PRF_REC][PRF_ROWS];
    const int chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, hf = lane >> 5;
    const char* qb = reinterpret_cast<const char*>(q + (int64_t)b * q_batch + (int64_t)h * q_head);
    const char* kb = reinterpret_cast<const char*>(k + (int64_t)b * k_batch + (int64_t)h * k_head);
    const int n_tiles = S / PRF_KT;

    // the sampled rows: B operand, lane (c, hf) holds row st * 32 + c, elements 16 ks + 8 hf .. + 7. Rows past n are zero (their results are never read).
    bf16x8 qf[2][8];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        const int i = st * 32 + c;
        if (i < n) {
            int r = sample_rows[i];
            r = r < 0 ? 0 : (r > S - 1 ? S - 1 : r);
            const char* p = qb + (uint32_t)r * q_row_bytes + 16 * hf;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) qf[st][ks] = *reinterpret_cast<const bf16x8*>(p + 32 * ks);
        } else {
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) qf[st][ks] = zero_bf16x8();
        }
    }
    const uint8_t* mem[2] = {tile_member + (int64_t)(c < n ? c : 0) * n_tiles, tile_member + (int64_t)(32 + c < n ? 32 + c : 0) * n_tiles};
    const bool live[2] = {c < n, 32 + c < n};

    // (one set per 32-row half of the samples, as separate objects: the hand-over below selects between them by lane)
    float m0 = PRF_M_EMPTY, m1 = PRF_M_EMPTY, dn0 = 0.0f, dn1 = 0.0f, sp0[PRF_MAXP], sp1[PRF_MAXP];
#pragma unroll
    for (int p = 0; p < PRF_MAXP; ++p) sp0[p] = sp1[p] = 0.0f;
    // one unit's 32 logits of a sample row (log2 units after the scale) into the row's running state
    auto advance = [&](f32x16& a, uint32_t bits, float& m, float& dn, float (&sp)[PRF_MAXP]) {
        float tm = PRF_M_EMPTY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            a[e] *= scale_log2;
            tm = fmaxf(tm, a[e]);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mn = fmaxf(m, tm);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        float ts = 0.0f;
#pragma unroll
        for (int e = 0; e < 16; ++e) ts += __builtin_amdgcn_exp2f(a[e] - mn);
        ts = ts + __shfl_xor(ts, 32, 64);  // (a + b == b + a: both lanes of the pair hold the same bits)
        dn = dn * alpha + ts;
#pragma unroll
        for (int p = 0; p < PRF_MAXP; ++p) sp[p] = sp[p] * alpha + (((bits >> p) & 1u) ? ts : 0.0f);
        m = mn;
    };

    // this chunk's tiles [t0, t1): n_chunks <= n_tiles, so every chunk has at least one. This wave's are t0 + wave, t0 + wave + 4, ...; it walks them in
    // units of 32 keys (one MFMA row block: 32 accumulator registers for the two 32-row halves of the samples), the next unit's K in flight under
    // this unit's MFMAs. Running maximum and row sums advance per unit; membership is the unit's tile's.
    const int t0 = (int)((int64_t)chunk * n_tiles / n_chunks), t1 = (int)((int64_t)(chunk + 1) * n_tiles / n_chunks);
    const int n_units = t0 + wave < t1 ? 2 * ((t1 - t0 - wave + PRF_WAVES - 1) / PRF_WAVES) : 0;
    bf16x8 kf[8];
    if (n_units) prf_load_k(kf, kb, k_row_bytes, (t0 + wave) * PRF_KT, c, hf);
    for (int u = 0; u < n_units; ++u) {
        const int t = t0 + wave + PRF_WAVES * (u >> 1);
        bf16x8 kn[8];
        if (u + 1 < n_units) prf_load_k(kn, kb, k_row_bytes, (t0 + wave + PRF_WAVES * ((u + 1) >> 1)) * PRF_KT + ((u + 1) & 1) * 32, c, hf);
        uint32_t bits[2];
#pragma unroll
        for (int st = 0; st < 2; ++st) bits[st] = live[st] ? mem[st][t] : 0u;
        f32x16 acc[2];
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[st][e] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int st = 0; st < 2; ++st) acc[st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[st][ks], acc[st], 0, 0, 0);
        // acc[st][e]: key (e & 3) + 8 (e >> 2) + 4 hf of the unit, sample row st * 32 + c. In log2 units from here.
        advance(acc[0], bits[0], m0, dn0, sp0);
        advance(acc[1], bits[1], m1, dn1, sp1);
        if (u + 1 < n_units) {
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) kf[ks] = kn[ks];
        }
    }

    // lane l hands over row l (both lanes of a pair hold rows c and 32 + c)
    part[wave][0][lane] = hf ? m1 : m0;
    part[wave][1][lane] = hf ? dn1 : dn0;
#pragma unroll
    for (int p = 0; p < PRF_MAXP; ++p) part[wave][2 + p][lane] = hf ? sp1[p] : sp0[p];
    __syncthreads();
    if (wave == 0) {
        float M = part[0][0][lane], D = part[0][1][lane], P[PRF_MAXP];
#pragma unroll
        for (int p = 0; p < PRF_MAXP; ++p) P[p] = part[0][2 + p][lane];
        for (int w = 1; w < PRF_WAVES; ++w) {
            float pw[PRF_MAXP];
#pragma unroll
            for (int p = 0; p < PRF_MAXP; ++p) pw[p] = part[w][2 + p][lane];
            prf_merge(M, D, P, part[w][0][lane], part[w][1][lane], pw);
        }
        float* o = ws + (((int64_t)b * H + h) * n_chunks + chunk) * (PRF_REC * PRF_ROWS) + lane;
        o[0] = M;
        o[PRF_ROWS] = D;
#pragma unroll
        for (int p = 0; p < PRF_MAXP; ++p) o[(2 + p) * PRF_ROWS] = P[p];
    }
}

// grid (head, batch), one lane per sampled row
__global__ __launch_bounds__(PRF_ROWS) void attn_pattern_merge_kernel(const float* __restrict__ ws, int H, int n, int n_patterns, int n_chunks,
                                                                       float* __restrict__ recall) {
    const int h = blockIdx.x, b = blockIdx.y, i = threadIdx.x;
    if (i >= n) return;
    const float* in = ws + ((int64_t)b * H + h) * n_chunks * (PRF_REC * PRF_ROWS) + i;
    float M = in[0], D = in[PRF_ROWS], P[PRF_MAXP];
#pragma unroll
    for (int p = 0; p < PRF_MAXP; ++p) P[p] = in[(2 + p) * PRF_ROWS];
    for (int ch = 1; ch < n_chunks; ++ch) {
        const float* x = in + (int64_t)ch * (PRF_REC * PRF_ROWS);
        float px[PRF_MAXP];
#pragma unroll
        for (int p = 0; p < PRF_MAXP; ++p) px[p] = x[(2 + p) * PRF_ROWS];
        prf_merge(M, D, P, x[0], x[PRF_ROWS], px);
    }
    float* o = recall + (((int64_t)b * H + h) * n + i) * n_patterns;
#pragma unroll
    for (int p = 0; p < PRF_MAXP; ++p)
        if (p < n_patterns) o[p] = P[p] / D;
}

// one lane per head
__global__ __launch_bounds__(64) void attn_pattern_select_kernel(const float* __restrict__ recall, int B, int H, int n, int n_patterns, float* __restrict__ score,
                                                                  int32_t* __restrict__ head_pattern) {
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= H) return;
    const float inv = 1.0f / (float)(B * n);
    int best = 0;
    float best_s = 0.0f;
    for (int p = 0; p < n_patterns; ++p) {
        float s = 0.0f;
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < n; ++i) s += recall[(((int64_t)b * H + h) * n + i) * n_patterns + p];
        s *= inv;
        if (score) score[(int64_t)h * n_patterns + p] = s;
        if (p == 0 || s > best_s) { best = p; best_s = s; }  // (the lowest index on ties)
    }
    head_pattern[h] = best;
}

/* ------------------------------------------------------------------------------------------------------------------------------ host */
extern "C" size_t g3_attn_profile_workspace_bytes(int B, int H, int n_chunks) {
    if (B < 1 || H < 1 || n_chunks < 1) return 0;
    return (size_t)B * H * n_chunks * PRF_REC * PRF_ROWS * sizeof(float);
}

extern "C" int g3_attn_profile_chunks(int S, int B, int H) {
    if (S < PRF_KT || B < 1 || H < 1) return 1;
    const int64_t bh = (int64_t)B * H;
    int64_t nc = (512 + bh - 1) / bh;  // two workgroups (the kernel's occupancy: 210 VGPRs) on each of the 256 CUs
    if (nc > S / PRF_KT) nc = S / PRF_KT;
    return (int)(nc < 1 ? 1 : nc);
}

#define G3_ATTN_PROFILE_PARAMS                                                                                                                        \
    const void *q, int64_t q_row, int64_t q_batch, int64_t q_head, const void *k, int64_t k_row, int64_t k_batch, int64_t k_head, int S, int B, int H, \
        int head_dim, float softmax_scale, const int32_t *sample_rows, int n, const uint8_t *tile_member, int n_patterns, int n_chunks,               \
        void *workspace, size_t workspace_bytes, float *recall
#define G3_ATTN_PROFILE_ARGS                                                                                                                           \
    q, q_row, q_batch, q_head, k, k_row, k_batch, k_head, S, B, H, head_dim, softmax_scale, sample_rows, n, tile_member, n_patterns, n_chunks, workspace, \
        workspace_bytes, recall

// every refusal of the launch; no HIP call, no pointer dereferenced
static int attn_profile_check(const char* fn, G3_ATTN_PROFILE_PARAMS) {
    if (!q || !k || !sample_rows || !tile_member || !workspace || !recall) return g3_set_error(G3_ERR_ARG, "%s: null operand", fn);
    if (head_dim != 128) return g3_set_error(G3_ERR_ARG, "%s: head_dim %d: only 128 is supported", fn, head_dim);
    if (S <= 0 || (S % PRF_KT)) return g3_set_error(G3_ERR_ARG, "%s: S %d must be a positive multiple of 64", fn, S);
    if (B < 1 || B > 65535 || H < 1 || H > 65535) return g3_set_error(G3_ERR_ARG, "%s: B %d and H %d must lie in [1, 65535]", fn, B, H);
    if (n_patterns < 1 || n_patterns > PRF_MAXP) return g3_set_error(G3_ERR_ARG, "%s: n_patterns %d outside [1, 8]", fn, n_patterns);
    if (n < 1 || n > PRF_ROWS) return g3_set_error(G3_ERR_ARG, "%s: n %d sample rows outside [1, 64]", fn, n);
    if (n_chunks < 1 || n_chunks > S / PRF_KT) return g3_set_error(G3_ERR_ARG, "%s: n_chunks %d outside [1, S / 64 = %d]", fn, n_chunks, S / PRF_KT);
    if ((((uintptr_t)q | (uintptr_t)k) & 15) || (((uintptr_t)sample_rows | (uintptr_t)workspace | (uintptr_t)recall) & 3))
        return g3_set_error(G3_ERR_ARG, "%s: misaligned pointer (q, k: 16 bytes; sample_rows, workspace, recall: 4)", fn);
    if (((q_row | q_batch | q_head | k_row | k_batch | k_head) & 7) || q_row < 0 || k_row < 0 || q_batch < 0 || q_head < 0 || k_batch < 0 || k_head < 0)
        return g3_set_error(G3_ERR_ARG, "%s: q / k strides must be non-negative multiples of 8 elements", fn);
    if (workspace_bytes < g3_attn_profile_workspace_bytes(B, H, n_chunks))
        return g3_set_error(G3_ERR_ARG, "%s: workspace of %zu bytes is too small: g3_attn_profile_workspace_bytes gives %zu", fn, workspace_bytes,
                            g3_attn_profile_workspace_bytes(B, H, n_chunks));
    // (a row's bytes are addressed as a 32-bit offset from the (batch, head) base)
    const int64_t lim = (int64_t)1 << 32;
    if ((int64_t)(S - 1) * q_row * 2 + 256 > lim || (int64_t)(S - 1) * k_row * 2 + 256 > lim)
        return g3_set_error(G3_ERR_ARG, "%s: operands beyond the kernel's 32-bit byte offsets over all S rows (row strides %lld, %lld elements, S %d)", fn,
                            (long long)q_row, (long long)k_row, S);
    return G3_OK;
}

extern "C" const char* g3_attn_pattern_profile_plan_bf16(G3_ATTN_PROFILE_PARAMS) {
    return attn_profile_check("g3_attn_pattern_profile_bf16", G3_ATTN_PROFILE_ARGS) == G3_OK ? "attn_pattern_profile_kernel" : nullptr;
}

extern "C" int g3_attn_pattern_profile_bf16(G3_ATTN_PROFILE_PARAMS, void* stream) {
    const char* fn = "g3_attn_pattern_profile_bf16";
    if (int rc = attn_profile_check(fn, G3_ATTN_PROFILE_ARGS)) return rc;
    const float scale_log2 = softmax_scale * 1.44269504088896340736f;
    hipLaunchKernelGGL(attn_pattern_profile_kernel, dim3((unsigned)n_chunks, (unsigned)H, (unsigned)B), dim3(PRF_THREADS), 0, (hipStream_t)stream,
                       (const bf16_t*)q, (uint32_t)(q_row * 2), q_batch, q_head, (const bf16_t*)k, (uint32_t)(k_row * 2), k_batch, k_head, S, H, scale_log2,
                       sample_rows, n, tile_member, n_chunks, (float*)workspace);
    if (int rc = g3_check_launch(fn)) return rc;
    hipLaunchKernelGGL(attn_pattern_merge_kernel, dim3((unsigned)H, (unsigned)B), dim3(PRF_ROWS), 0, (hipStream_t)stream, (const float*)workspace, H, n,
                       n_patterns, n_chunks, recall);
    return g3_check_launch(fn);
}
#undef G3_ATTN_PROFILE_PARAMS
#undef G3_ATTN_PROFILE_ARGS

extern "C" int g3_attn_pattern_select(const float* recall, int B, int H, int n, int n_patterns, float* score, int32_t* head_pattern, void* stream) {
    const char* fn = "g3_attn_pattern_select";
    if (!recall || !head_pattern) return g3_set_error(G3_ERR_ARG, "%s: null operand", fn);
    if (B < 1 || H < 1) return g3_set_error(G3_ERR_ARG, "%s: B %d and H %d must be >= 1", fn, B, H);
    if (n_patterns < 1 || n_patterns > PRF_MAXP) return g3_set_error(G3_ERR_ARG, "%s: n_patterns %d outside [1, 8]", fn, n_patterns);
    if (n < 1 || n > PRF_ROWS) return g3_set_error(G3_ERR_ARG, "%s: n %d sample rows outside [1, 64]", fn, n);
    if (((uintptr_t)recall | (uintptr_t)score | (uintptr_t)head_pattern) & 3) return g3_set_error(G3_ERR_ARG, "%s: misaligned pointer (4 bytes)", fn);
    hipLaunchKernelGGL(attn_pattern_select_kernel, dim3((unsigned)((H + 63) / 64)), dim3(64), 0, (hipStream_t)stream, recall, B, H, n, n_patterns, score,
                       head_pattern);
    return g3_check_launch(fn);
}

/* Pure host code over HOST copies: member_out[i][t] bit p = tile t lies in the list (pattern p, block sample_rows[i] / 256). */
extern "C" int g3_attn_profile_members(const int32_t* ranges_host, int n_patterns, int S, int max_ranges, const int32_t* sample_rows_host, int n,
                                       uint8_t* member_out) {
    const char* fn = "g3_attn_profile_members";
    if (!ranges_host || !sample_rows_host || !member_out) return g3_set_error(G3_ERR_ARG, "%s: null table, sample rows or result pointer", fn);
    if (S <= 0 || (S % PRF_KT)) return g3_set_error(G3_ERR_ARG, "%s: S %d must be a positive multiple of 64", fn, S);
    if (n_patterns < 1 || n_patterns > PRF_MAXP) return g3_set_error(G3_ERR_ARG, "%s: n_patterns %d outside [1, 8]", fn, n_patterns);
    if (max_ranges < 1 || max_ranges > 64) return g3_set_error(G3_ERR_ARG, "%s: max_ranges %d outside [1, 64]", fn, max_ranges);
    if (n < 1 || n > PRF_ROWS) return g3_set_error(G3_ERR_ARG, "%s: n %d sample rows outside [1, 64]", fn, n);
    for (int i = 0; i < n; ++i)
        if (sample_rows_host[i] < 0 || sample_rows_host[i] >= S || (i && sample_rows_host[i] <= sample_rows_host[i - 1]))
            return g3_set_error(G3_ERR_ARG, "%s: sample_rows[%d] = %d: the rows must be strictly ascending in [0, %d)", fn, i, sample_rows_host[i], S);
    const int n_blk = (S + PRF_QBLK - 1) / PRF_QBLK, n_tiles = S / PRF_KT;
    for (int i = 0; i < n; ++i) {
        uint8_t* out = member_out + (int64_t)i * n_tiles;
        for (int t = 0; t < n_tiles; ++t) out[t] = 0;
        const int blk = sample_rows_host[i] / PRF_QBLK;
        for (int p = 0; p < n_patterns; ++p) {
            const int32_t* row = ranges_host + ((int64_t)p * n_blk + blk) * max_ranges * 2;
            for (int r = 0; r < max_ranges && row[2 * r + 1] != 0; ++r) {
                const int64_t first = row[2 * r], len = row[2 * r + 1];
                if (first < 0 || len < 0 || (first % PRF_KT) || (len % PRF_KT) || first + len > S)
                    return g3_set_error(G3_ERR_ARG, "%s: pattern %d, block %d, range %d: (%d, %d) is no range of whole tiles inside S %d (validate the table "
                                        "with g3_attn_ranges_check)", fn, p, blk, r, (int)first, (int)len, S);
                for (int64_t t = first / PRF_KT; t < (first + len) / PRF_KT; ++t) out[t] |= (uint8_t)(1u << p);
            }
        }
    }
    return G3_OK;
}
