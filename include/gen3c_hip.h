/*
 * gen3c_hip.h - C ABI of libgen3c_hip.so: the MI355X (gfx950) kernels of the GEN3C-Cosmos-7B denoising path.
 *
 * The reference (nv-tlabs/GEN3C, a Cosmos-Predict1 fork) has no FFI boundary for this path: the hot operators sit
 * behind Python module seams and third-party CUDA libraries (TransformerEngine, cuBLAS via nn.Linear, ATen
 * index_put_, NVIDIA Warp).  Each entry point below names the reference call site(s) it replaces; INTEGRATION.md
 * shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless marked "host"; nothing is allocated or freed inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on that stream;
 *   - tensors are bf16 (uint16 storage) unless the name says f32; leading dims / strides are in ELEMENTS;
 *   - return value: 0 = G3_OK, non-zero = error (g3_last_error() returns a thread-local message);
 *   - thread-compatible: no mutable global state besides lazily-set kernel attributes and the g3_set_option A/B switches (process-wide,
 *     meant for tools; per-call choices go through the *_ex entry points).
 */
#ifndef GEN3C_HIP_H
#define GEN3C_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G3_OK 0
#define G3_ERR_ARG 1
#define G3_ERR_LAUNCH 2
#define G3_ERR_RESOURCE 3 /* the device refused a static resource request (dynamic LDS size): the caller may take another path */

/* epilogues of g3_gemm_bf16_nt */
#define G3_EPI_NONE 0           /* C = A.W^T                                   */
#define G3_EPI_GELU 1           /* C = gelu_erf(A.W^T)      attention.py:86,94-99 (GPT2FeedForward)            */
#define G3_EPI_GATED_RESIDUAL 2 /* C = R + gate[m%rows] * (A.W^T)   blocks.py:455-471 (x + gate * block(...))   */
#define G3_EPI_BIAS 3           /* C = A.W^T + bias[m%rows]                                                     */
#define G3_EPI_BIAS_RESIDUAL 4  /* C = A.W^T + bias[m%rows] + R                                                 */

const char* g3_last_error(void);
int g3_abi_version(void);
/* runtime switches for A/B measurements: "gemm_regstage", "gemm_rowmajor_tiles", "gemm_unpinned" (0/1), "gemm_pingpong" (3 = one wave per SIMD, the
 * default), "gemm_deferred" (1 = the persistent block GEMM with the deferred epilogue where it applies, the default; 0 = epilogue behind every K loop),
 * "gemm_mfma16" (1, the default: that kernel's K loop on v_mfma_f32_16x16x32_bf16; 0: on v_mfma_f32_32x32x16_bf16 - the same bits and the same reported kernel name),
 * "gemm_persistent", "conv_w4" (2 = without the in-gap tap change), "attn_variant" (0 = automatic), "attn_xcd_heads", "splat_tiled", "render_overlap", "render_fused", "render_full_extent"
 * (1, default: the renderer's tiles publish unclamped destination rectangles and the gather pass reads the dense accumulator per texel),
 * "render_exclusive" (1: extent pre-pass + single-writer texels resolved inside the splat - a quarter less memory traffic, 18 % slower; default 0),
 * "tok_tattn_px". Outputs do not depend on them. */
int g3_set_option(const char* name /*host*/, int value);
/* The value of a switch in force in this process (its default, its environment variable or the last g3_set_option). */
int g3_get_option(const char* name /*host*/, int* value /*host*/);
int g3_device_info(int device, int* cu_count, int* is_gfx950, char* arch_name /*host*/, int arch_name_len);

/* hipEvent helpers (opaque handles) so a host can time a stream without linking HIP itself. */
int g3_event_create(void** ev);
int g3_event_record(void* ev, void* stream);
int g3_event_elapsed_ms(void* start, void* stop, float* ms /*host*/);
int g3_event_destroy(void* ev);

/* ---- DiT linears ---------------------------------------------------------------------------------------------
 * C[M,N] = epi(A[M,K] . W[N,K]^T): replaces nn.Linear(bias=False) in Attention.to_q/to_k/to_v/to_out
 * (cosmos_predict1/diffusion/module/attention.py:207-223), GPT2FeedForward.layer1/layer2 (attention.py:61-62),
 * PatchEmbed.proj (blocks.py:160-162) and FinalLayer.linear (blocks.py:205-206).
 * Needs K, lda, ldw multiples of 8; N, ldc (ldg, ldr) multiples of 4. gate/bias is [gate_rows][ldg]. */
int g3_gemm_bf16_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                    int epilogue, const void* gate, int gate_rows, int64_t ldg, const void* residual, int64_t ldr,
                    void* stream);

/* Name of the kernel the call above launches for this shape under the options in force (aligned operands assumed): profilers / bench.py only. */
const char* g3_gemm_kernel_name(int M, int N, int K, int epilogue);

/* ---- opt-in MXFP8 DiT linears (OCP MX v1.0, e4m3fn elements; outside the bf16 parity statement, DESIGN.md "MXFP8 linears") -------------
 * x [M][ldx] bf16 -> q [M][ldq] e4m3fn bytes + scales [M][lds] E8M0 bytes, one per 32 consecutive k of a row:
 *   X = floor(log2(amax of the block)) - 8, byte X + 127 clamped to 0..254; q = RNE(clamp(x / 2^X, -448, 448)); an all-zero block gets byte 127
 *   and zero elements; a block that holds a NaN or an infinity gets byte 0xFF (the E8M0 NaN) and zero elements, and every output of a GEMM
 *   below that consumes it is NaN. Needs K % 32 == 0, ldx and ldq multiples of 8 (>= K), lds >= K/32; x 16-byte, q 8-byte aligned. */
int g3_quant_mxfp8_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int M, int K, void* stream);

/* C[M,N] = epi( sum_k (aq[m][k] 2^as[m][k/32]) (wq[n][k] 2^ws[n][k/32]) ) with fp32 accumulation on the block-scaled matrix cores; operands as
 * g3_quant_mxfp8_bf16 writes them. Epilogues G3_EPI_NONE, G3_EPI_GELU, G3_EPI_GATED_RESIDUAL with the rounding points of g3_gemm_bf16_nt
 * (C may alias the residual). Needs N % 256 == 0, K % 128 == 0, lda / ldw >= K multiples of 16 with 16-byte aligned operands, scale strides
 * >= K/32 multiples of 4 with 4-byte aligned scales, ldc (ldg, ldr) multiples of 8 with 16-byte aligned rows, ldr >= N and ldg >= N when
 * gate_rows > 1; anything else is refused with
 * G3_ERR_ARG before any launch. */
int g3_gemm_mxfp8_nt(const void* aq, int64_t lda, const void* as, int64_t ldas, const void* wq, int64_t ldw, const void* ws, int64_t ldws,
                     void* c, int64_t ldc, int M, int N, int K, int epilogue, const void* gate, int gate_rows, int64_t ldg,
                     const void* residual, int64_t ldr, void* stream);

/* Name of the kernel instantiation g3_gemm_mxfp8_nt launches for this shape and epilogue ("gemm_mxfp8_nt_kernel<epilogue>"), or NULL where it
 * refuses the shape or epilogue: profilers / tools only. */
const char* g3_gemm_mxfp8_kernel_name(int M, int N, int K, int epilogue);

/* g3_gemm_mxfp8_nt whose OUTPUT is MXFP8 as well: q_out [M][ldq] e4m3fn + s_out [M][lds] E8M0 are bitwise what g3_quant_mxfp8_bf16 makes of the
 * bf16 C of g3_gemm_mxfp8_nt with the same epilogue (rounded to bf16 at the same points, then the same quantiser arithmetic, in the epilogue's
 * registers: C itself is never written). For a producer whose only consumer is the next MXFP8 linear (the MLP: layer1 + GELU into layer2).
 * Epilogues G3_EPI_NONE and G3_EPI_GELU only. Operands as g3_gemm_mxfp8_nt; ldq >= N a multiple of 8, lds >= N/32, q_out 8-byte aligned;
 * anything else is refused with G3_ERR_ARG before any launch. Rows >= M of the outputs are not written. */
int g3_gemm_mxfp8_nt_mxout(const void* aq, int64_t lda, const void* as, int64_t ldas, const void* wq, int64_t ldw, const void* ws, int64_t ldws,
                           void* q_out, int64_t ldq, void* s_out, int64_t lds, int M, int N, int K, int epilogue, void* stream);

/* Name of the instantiation g3_gemm_mxfp8_nt_mxout launches ("gemm_mxfp8_nt_kernel<256 + epilogue>"), or NULL where it refuses: tools only. */
const char* g3_gemm_mxfp8_mxout_kernel_name(int M, int N, int K, int epilogue);

/* MXFP6 (OCP MX v1.0, e2m3 elements: 1 sign, 2 exponent, 3 mantissa bits, bias 1, maximum 7.5, no Inf / NaN) of a bf16 matrix:
 * x [M][ldx] bf16 -> q [M][ldq] packed 6-bit codes + scales [M][lds] E8M0 bytes, one per 32 consecutive k of a row:
 *   X = floor(log2(amax of the block)) - 2, byte X + 127 clamped to 0..254; code = RNE(clamp(x / 2^X, -7.5, 7.5)) with the sign bit of x;
 *   an all-zero block gets byte 127 and zero codes, a block that holds a NaN or an infinity byte 0xFF (the E8M0 NaN) and zero codes. Block b of a row is the 24 bytes [24 b, 24 b + 24) of q's row, element i of the block
 *   the 6 bits [6 i, 6 i + 6) of that 192-bit little-endian string. Needs K % 32 == 0, ldx >= K and ldq >= 3K/4 multiples of 8,
 *   lds >= K/32; x 16-byte, q 8-byte aligned. */
int g3_quant_mxfp6_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int M, int K, void* stream);

/* g3_gemm_mxfp8_nt on MXFP6 operands as g3_quant_mxfp6_bf16 writes them (the same matrix-core instruction at twice the MXFP8 rate):
 * C[M,N] = epi( sum_k (aq[m][k] 2^as[m][k/32]) (wq[n][k] 2^ws[n][k/32]) ), the same epilogues and rounding points (C may alias the
 * residual). Needs N % 256 == 0, K % 128 == 0, lda / ldw >= 3K/4 multiples of 16 with 16-byte aligned operands, scale strides >= K/32
 * multiples of 4 with 4-byte aligned scales, ldc (ldg, ldr) multiples of 8 with 16-byte aligned rows, ldr >= N and ldg >= N when
 * gate_rows > 1; anything else is refused with G3_ERR_ARG before any launch. */
int g3_gemm_mxfp6_nt(const void* aq, int64_t lda, const void* as, int64_t ldas, const void* wq, int64_t ldw, const void* ws, int64_t ldws,
                     void* c, int64_t ldc, int M, int N, int K, int epilogue, const void* gate, int gate_rows, int64_t ldg,
                     const void* residual, int64_t ldr, void* stream);

/* Name of the kernel instantiation g3_gemm_mxfp6_nt launches for this shape and epilogue ("gemm_mxfp6_nt_kernel<epilogue>"), or NULL where it
 * refuses the shape or epilogue: profilers / tools only. */
const char* g3_gemm_mxfp6_kernel_name(int M, int N, int K, int epilogue);

/* out[M<=8][N] = (act_in(a) . w^T) (+ add): TimestepEmbedding (blocks.py:60-80) and adaLN_modulation
 * (blocks.py:411-415, 442-447; FinalLayer blocks.py:212-216, 230). act_in: 0 none, 1 SiLU. */
int g3_gemv_bf16(const void* a, int64_t lda, const void* w, int64_t ldw, const void* add, int64_t ldadd, void* out,
                 int64_t ldo, int M, int N, int K, int act_in, void* stream);

/* ---- attention -------------------------------------------------------------------------------------------------
 * O = softmax(Q K^T * softmax_scale) V, no mask, head_dim 128: replaces TransformerEngine DotProductAttention
 * (attention.py:228-238, 288). Element (s, b, h, d) of Q is at q + s*q_row + b*q_batch + h*q_head + d (same for K, O);
 * V is passed TRANSPOSED: element (b, h, d, kv) at vt + b*vt_batch + h*vt_head + d*vt_row + kv, with
 * vt_row >= S_kv rounded up to 8 and the tail [S_kv, vt_row) zero (g3_transpose_v_bf16 writes exactly this). */
int g3_flash_attn_fwd_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row,
                           int64_t k_batch, int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch,
                           int64_t vt_head, void* o, int64_t o_row, int64_t o_batch, int64_t o_head, int Sq, int Skv,
                           int B, int H, int head_dim, float softmax_scale, void* stream);

/* Name of the kernel g3_flash_attn_fwd_bf16 launches for this problem under the current "attn_variant" option (0 = automatic choice
 * between the 8-wave and the one-wave-per-SIMD kernels): for profilers and bench.py's roofline line, never needed to run the op. From shapes only,
 * i.e. for plain V^T and operands the 32-bit-offset kernels can address; g3_attn_plan_bf16 is the exact answer for a given call. */
const char* g3_flash_attn_kernel_name(int Sq, int Skv, int B, int H);

/* The CROSS-attention form of the same call (Attention.forward with a context: cal_qkv's to_q[1] norm + DotProductAttention, attention.py:247-297), two options:
 *  - q_norm_weight != NULL: q holds the RAW to_q[0] projection; the per-head te.pytorch.RMSNorm(128, eps) with this weight (attention.py:130-131, 262-273) is
 *    applied inside the kernel's Q load, so the cross-attention's Q never makes the separate read + write pass of g3_qk_rmsnorm_rope_bf16 (no RoPE here:
 *    cross-attention applies none). NULL: q is used as it is.
 *  - kv_dense > 0: keys with an ALL-ZERO TAIL - the caller guarantees that the K rows AND the V^T columns of keys [kv_dense, S_kv) are exactly zero: a T5
 *    context that text_encoder zero-pads to 512 tokens (to_k / to_v carry no bias and RMSNorm(0) = 0, so the padding stays zero through cal_qkv). Those keys
 *    score exactly 0 and add nothing to the output but they DO stay in the softmax denominator (the reference attends over all 512 context tokens unmasked,
 *    general_dit.py:407-410): only the first ceil64(kv_dense) keys go through the kernel's tile loop, the tail enters in closed form (m' = max(m, 0),
 *    l' = l 2^(m-m') + n_tail 2^(-m')). Same function of the same inputs. 0: every key goes through the loop. */
int g3_cross_attn_fwd_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* q_norm_weight, float q_norm_eps,
                           const void* k, int64_t k_row, int64_t k_batch, int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch,
                           int64_t vt_head, void* o, int64_t o_row, int64_t o_batch, int64_t o_head, int Sq, int Skv, int kv_dense, int B, int H,
                           int head_dim, float softmax_scale, void* stream);

/* Same, with V^T stored in KEY SEGMENTS: keys [s*vt_seg_len, (s+1)*vt_seg_len) live in the block at vt + s*vt_seg_stride (each block
 * laid out as above with its own vt_row >= vt_seg_len). vt_seg_len must be a multiple of 64 and divide S_kv. This is what a rank-major
 * all-gather of per-rank V^T shards produces under context parallelism (module/parallel.py:110-163 gathers; TE's CP attention is the
 * reference counterpart), so no rank has to re-transpose the gathered V. */
int g3_flash_attn_fwd_kvseg_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row,
                                 int64_t k_batch, int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head,
                                 int vt_seg_len, int64_t vt_seg_stride, void* o, int64_t o_row, int64_t o_batch, int64_t o_head, int Sq,
                                 int Skv, int B, int H, int head_dim, float softmax_scale, void* stream);

/* Extended form of the two calls above (one entry point: vt_seg_len == 0 = plain V^T) for hosts that shard the KEYS of a row over several
 * launches - the context-parallel schedule that starts on the local K / V shard before any remote shard has arrived, which is what
 * TransformerEngine's ring does behind attn_op.set_context_parallel_group (general_dit.py:536-541, module/attention.py:228-238):
 *   variant   per-call kernel choice, 0 = the process-wide "attn_variant" option (whose 0 = automatic). Nothing global is touched, so
 *             concurrent launches on several streams can use different kernels (4 = 8-wave kernel, 11 = one-wave-per-SIMD kernel).
 *   o         bf16 result as above, or NULL when o_partial / lse are given:
 *   o_partial fp32 [Sq][B][H][128] addressed with the SAME element strides o_row / o_batch / o_head: the softmax-NORMALISED result over
 *             this launch's keys only;  lse fp32 [B][H][Sq] contiguous: log2(sum_k exp2(s_qk * scale * log2 e)) of those keys.
 * g3_attn_merge_partials_bf16 combines n_parts (1..8) such parts of the same rows into the bf16 result over the union of their keys:
 *   out = sum_i w_i * o_part_i,  w_i = 2^(lse_i - max lse) / sum_j 2^(lse_j - max lse).  o_parts / lse_parts are HOST arrays of device pointers. */
int g3_flash_attn_fwd_ex_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                              int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, int vt_seg_len,
                              int64_t vt_seg_stride, void* o, float* o_partial, float* lse, int64_t o_row, int64_t o_batch, int64_t o_head,
                              int Sq, int Skv, int B, int H, int head_dim, float softmax_scale, int variant, void* stream);
/* g3_flash_attn_kernel_name with the per-call variant, from shapes only: g3_attn_plan_bf16 is the exact answer for a given call. */
const char* g3_flash_attn_kernel_name_ex(int Sq, int Skv, int B, int H, int variant);

/* g3_flash_attn_fwd_ex_bf16 for callers that can BOUND the logits: logit_bound >= |q . k| * softmax_scale (natural units) for every query / key
 * pair of the call - e.g. per-head RMSNorm of q and k (RoPE keeps the norm): |q . k| / sqrt(128) <= sqrt(128) * max|w_q| * max|w_k|. Where the
 * resolved variant is 11, V^T is not segmented (with segments: g3_self_attn_fwd_bounded_cp_bf16) and 0 < logit_bound * log2(e) <= 60, the one-wave-per-SIMD kernel then runs without its running
 * row maximum (the bound is the softmax's constant reference point; the same function, fewer instructions per tile). In every other case - bound 0,
 * bound above the limit, another kernel - the call IS g3_flash_attn_fwd_ex_bf16. An understated bound is a caller error (rows may overflow).
 * g3_self_attn_kernel_name reports the kernel such a call launches with PLAIN V^T (vt_seg_len == 0) and operands the 32-bit-offset kernels can
 * address; like g3_flash_attn_kernel_name_ex it sees shapes only: a call with segments runs what g3_flash_attn_fwd_ex_bf16 runs, and a V^T leading
 * dimension below ceil64(S_kv) or operands spanning more than 4 GiB demote either entry to the 64-bit-addressing kernel, whatever the name says:
 * g3_attn_plan_bf16 is the exact answer for a given call. */
int g3_self_attn_fwd_bounded_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                  int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, int vt_seg_len,
                                  int64_t vt_seg_stride, void* o, float* o_partial, float* lse, int64_t o_row, int64_t o_batch, int64_t o_head,
                                  int Sq, int Skv, int B, int H, int head_dim, float softmax_scale, float logit_bound, int variant, void* stream);
const char* g3_self_attn_kernel_name(int Sq, int Skv, int B, int H, float logit_bound, int variant);
/* g3_self_attn_fwd_bounded_bf16 with the tile loop on 16x16x32 MFMAs (flash_attn_fwd_w4c_nm_kernel; the chip holds a higher clock on that shape,
 * profiles/mfma_shape_probe.txt) where that call would launch flash_attn_fwd_w4b_nm_kernel<true> with a bf16 output (o, not o_partial): the same
 * function, P rounded to bf16, row sums and O accumulated in fp32, so the result agrees to rounding, not bit for bit. In every other case - a
 * partial output, segments, a bound out of range, another variant, S_kv % 64 != 0 - the call IS g3_self_attn_fwd_bounded_bf16: the same kernel,
 * bit for bit, the same refusals. g3_self_attn16_kernel_name is g3_self_attn_kernel_name for this entry (a bf16-output call);
 * g3_attn_plan16_bf16 is g3_attn_plan_bf16 with G3_ATTN_ENTRY_BOUNDED standing for this entry. */
int g3_self_attn_fwd_bounded16_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                    int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, int vt_seg_len,
                                    int64_t vt_seg_stride, void* o, float* o_partial, float* lse, int64_t o_row, int64_t o_batch, int64_t o_head,
                                    int Sq, int Skv, int B, int H, int head_dim, float softmax_scale, float logit_bound, int variant, void* stream);
const char* g3_self_attn16_kernel_name(int Sq, int Skv, int B, int H, float logit_bound, int variant);

/* Carry-in form of g3_flash_attn_fwd_ex_bf16: a row's keys in a CHAIN of launches with no merge pass - the context-parallel schedule that
 * TransformerEngine's CP attention runs behind attn_op.set_context_parallel_group (general_dit.py:536-541, module/attention.py:282-297) keeps
 * a running softmax state per row; here each launch can resume from one.
 *   carry_o / carry_lse  an earlier state of the same rows, or both NULL: carry_o fp32 normalised, addressed with the o strides (as o_partial),
 *             carry_lse fp32 [B][H][Sq] in the log2 domain (what o_partial / lse hold). carry_lse = -inf: no earlier keys for that row. The
 *             launch's own part (lse_k = m + log2 l) is folded in after the tile loop: M = max(lse_c, lse_k), w_x = 2^(lse_x - M),
 *             out = (w_c o_c + w_k acc / l) / (w_c + w_k) in fp32, written as the bf16 o or as a new o_partial + lse (lse = M + log2(w_c + w_k)),
 *             so chains of any length work. carry_o may alias o_partial (and carry_lse lse).
 *   kv_skip_begin / kv_skip_len  multiples of 64: S_kv counts the ATTENDED keys only; logical key j is read at physical key
 *             j + (j >= kv_skip_begin ? kv_skip_len : 0) in K and in V^T (plain or segmented: then whole segments). kv_skip_len = 0: none.
 *             Context parallelism: an interior rank attends every remote key of the gathered buffers in one launch, skipping its own block.
 * Kernels: variant 0 (automatic), 4 (8-wave) or 11 (one-wave-per-SIMD). G3_ERR_ARG, with nothing launched, for any other, for a problem that needs
 * the 64-bit-addressing kernel (operands spanning more than 4 GiB, skipped keys included; V^T leading dim below ceil64 of the keys it spans), for a
 * misaligned or out-of-range skip or one that splits a V^T segment, and for misaligned carry buffers (carry_o 16 B, carry_lse 4 B) or o strides. */
int g3_flash_attn_fwd_carry_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                 int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, int vt_seg_len,
                                 int64_t vt_seg_stride, int kv_skip_begin, int kv_skip_len, const float* carry_o, const float* carry_lse,
                                 void* o, float* o_partial, float* lse, int64_t o_row, int64_t o_batch, int64_t o_head, int Sq, int Skv, int B,
                                 int H, int head_dim, float softmax_scale, int variant, void* stream);
/* g3_flash_attn_fwd_carry_bf16 for callers that can BOUND the logits (logit_bound as for g3_self_attn_fwd_bounded_bf16): the no-running-max kernels
 * under key sharding. A constant reference point suits a row whose keys are spread over launches: every launch uses the same one, so a key's
 * P = exp2(s - bound) does not depend on the split, and a launch's (normalised o, lse = bound + log2 l) is what the merge kernel and the carry-in
 * epilogue consume - bounded and max-form parts of the same rows mix freely. Where the resolved variant is 11, 0 < logit_bound * log2(e) <= 60
 * and the 32-bit-offset kernels can address the operands:
 *   no carry-in state and no skipped range inside the keys -> flash_attn_fwd_w4b_nm_kernel<true>, with plain or segmented V^T;
 *   a carry-in state or a skipped range                    -> flash_attn_fwd_w4b_nm_carry_kernel<true>.
 * In every other case - bound 0, negative or above the limit, variant 4 - the call IS g3_flash_attn_fwd_carry_bf16: the same output bit for bit,
 * the same refusals (G3_ERR_ARG, nothing launched). g3_self_attn_fwd_bounded_bf16 keeps its own contract: a segmented call through it runs the max form.
 * g3_self_attn_cp_kernel_name: the kernel such a call launches, from shapes only (Skv = attended keys; cp_form != 0: a carry-in state, or a skip
 * with 0 < kv_skip_begin < S_kv and kv_skip_len > 0; segmented is informational - both V^T forms run the same kernels); g3_attn_plan_bf16 is the
 * exact answer for a given call. */
int g3_self_attn_fwd_bounded_cp_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                     int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, int vt_seg_len,
                                     int64_t vt_seg_stride, int kv_skip_begin, int kv_skip_len, const float* carry_o, const float* carry_lse,
                                     void* o, float* o_partial, float* lse, int64_t o_row, int64_t o_batch, int64_t o_head, int Sq, int Skv, int B,
                                     int H, int head_dim, float softmax_scale, float logit_bound, int variant, void* stream);
const char* g3_self_attn_cp_kernel_name(int Sq, int Skv, int B, int H, float logit_bound, int variant, int segmented, int cp_form);

/* Dry run of the launching entry points above: the name of the kernel instantiation the call `entry` would launch with exactly these arguments -
 * every check, normalisation and fallback of the real call (per-call variant and "attn_variant" option, split-KV partials, the cross-attention
 * form, a short V^T leading dimension, operands beyond 4 GiB, carry / skip, the logit bound) - or NULL where the call would be refused, with
 * g3_last_error() set exactly as the call sets it. Nothing is launched, no HIP call is made and no pointer is dereferenced (pointers are tested for
 * NULL and alignment only). The arguments are the union of the entries' arguments (no stream); those `entry` does not take are ignored. */
enum g3_attn_entry {
    G3_ATTN_ENTRY_FWD = 0,        /* g3_flash_attn_fwd_bf16 */
    G3_ATTN_ENTRY_KVSEG = 1,      /* g3_flash_attn_fwd_kvseg_bf16 */
    G3_ATTN_ENTRY_CROSS = 2,      /* g3_cross_attn_fwd_bf16 */
    G3_ATTN_ENTRY_EX = 3,         /* g3_flash_attn_fwd_ex_bf16 */
    G3_ATTN_ENTRY_BOUNDED = 4,    /* g3_self_attn_fwd_bounded_bf16 */
    G3_ATTN_ENTRY_CARRY = 5,      /* g3_flash_attn_fwd_carry_bf16 */
    G3_ATTN_ENTRY_BOUNDED_CP = 6  /* g3_self_attn_fwd_bounded_cp_bf16 */
};
const char* g3_attn_plan_bf16(int entry, const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* q_norm_weight, float q_norm_eps,
                              const void* k, int64_t k_row, int64_t k_batch, int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch,
                              int64_t vt_head, int vt_seg_len, int64_t vt_seg_stride, int kv_skip_begin, int kv_skip_len, const float* carry_o,
                              const float* carry_lse, void* o, float* o_partial, float* lse, int64_t o_row, int64_t o_batch, int64_t o_head, int Sq,
                              int Skv, int kv_dense, int B, int H, int head_dim, float softmax_scale, float logit_bound, int variant);
/* The same dry run with G3_ATTN_ENTRY_BOUNDED standing for g3_self_attn_fwd_bounded16_bf16 (every other entry: g3_attn_plan_bf16's answer). */
const char* g3_attn_plan16_bf16(int entry, const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* q_norm_weight, float q_norm_eps,
                                const void* k, int64_t k_row, int64_t k_batch, int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch,
                                int64_t vt_head, int vt_seg_len, int64_t vt_seg_stride, int kv_skip_begin, int kv_skip_len, const float* carry_o,
                                const float* carry_lse, void* o, float* o_partial, float* lse, int64_t o_row, int64_t o_batch, int64_t o_head, int Sq,
                                int Skv, int kv_dense, int B, int H, int head_dim, float softmax_scale, float logit_bound, int variant);

/* Self-attention (Sq == Skv == S) over a temporal FRAME WINDOW, for tokens ordered (t, h, w): opt-in, training-free local attention. Parameters:
 *   frame_len      tokens per latent frame (Hp * Wp); T = S / frame_len frames
 *   window_frames  W >= 0: a query attends the frames within W of its own
 *   sink_frames    s >= 0: the first s frames are attended by every query (in GEN3C the first latent frames are the conditioning frames)
 *   the query block: g3_self_attn_window_q_rows() = 256 rows, the kernel's workgroup
 * Query block b holds rows [256 b, min(256 b + 256, S)), which lie in frames f0..f1. It attends
 *   the keys of frames [max(0, f0 - W), min(T, f1 + W + 1))  and  the keys of frames [0, min(s, T)),
 * and the output is the exact softmax over that key set. The key set is BLOCK-granular: a block that straddles a frame boundary attends the union
 * of its rows' windows, a superset of each row's own window (no mask inside the kernel's tile loop; at 3 520 tokens per frame = 13.75 blocks about
 * one block in 14 straddles). Every workgroup of flash_attn_fwd_w4b_nm_win_kernel<true> (0 < logit_bound * log2(e) <= 60, as for
 * g3_self_attn_fwd_bounded_bf16) or flash_attn_fwd_w4b_win_kernel<true> (any other bound: the running-maximum form) derives its key range from
 * its block index and these numbers; the operand rules are variant 11's. When the window covers every key of every block (W >= T - 1 or s >= T)
 * the call IS g3_self_attn_fwd_bounded_bf16 with variant 11, bit for bit.
 * G3_ERR_ARG, with nothing launched: S, frame_len not positive multiples of 64 or S no multiple of frame_len; negative W or s; a V^T leading
 * dimension below ceil64(S); operands beyond the kernel's 32-bit byte offsets (the carry entry's arithmetic over all S keys); misaligned
 * pointers or strides; head_dim != 128.
 * g3_attn_window_plan_bf16: the dry run - the kernel's name, or NULL with g3_last_error() set exactly as the call sets it; no HIP call, no pointer
 * dereferenced. g3_self_attn_window_tiles: the (query block, 64-key tile) pairs such a launch visits and the dense launch's count. */
int g3_self_attn_fwd_window_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                 int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, void* o, int64_t o_row,
                                 int64_t o_batch, int64_t o_head, int S, int B, int H, int head_dim, float softmax_scale, float logit_bound,
                                 int frame_len, int window_frames, int sink_frames, void* stream);
const char* g3_attn_window_plan_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                     int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, void* o, int64_t o_row,
                                     int64_t o_batch, int64_t o_head, int S, int B, int H, int head_dim, float softmax_scale, float logit_bound,
                                     int frame_len, int window_frames, int sink_frames);
int g3_self_attn_window_q_rows(void);
int g3_self_attn_window_tiles(int S, int frame_len, int window_frames, int sink_frames, int64_t* attended, int64_t* dense);

/* The frame window under KEY SHARDING (context parallelism; opt-in inside the opt-in): the same two kernels, one launch per rank. Parameters beyond
 * g3_self_attn_fwd_window_bf16's:
 *   Sq               this rank's query rows, whole frames: frames [q_frame0, q_frame0 + Sq / frame_len) of the sequence's total_frames
 *   Skv_buf          keys in the COMPACT K / V^T operand, which holds the global frames [0, a) ++ [b, c) in ascending order,
 *                    a = buf_head_frames <= b = buf_tail_frame0, c = Skv_buf / frame_len - a + b (a == b: the one range [0, c)); V^T is plain
 * Query block blk holds the rank's rows [256 blk, min(256 blk + 256, Sq)), global frames f0..f1, and attends the frames [max(0, f0 - W),
 * min(total_frames, f1 + W + 1)) and [0, min(s, total_frames)) exactly as above; the prologue computes that key set in global coordinates and maps
 * it into the buffer (a key at or past frame b moves down by b - a frames). Where the rank's first row is a multiple of 256 in the whole sequence,
 * the blocks are the single-GPU blocks and the output is g3_self_attn_fwd_window_bf16's, bit for bit. Otherwise the blocks that straddle a frame
 * boundary are different blocks, so for those rows (about one block in 14 at 3 520 tokens per frame) the function depends on the number of ranks.
 * Always the window kernels, also when the window covers everything. Keys in the buffer that no block attends are allowed; the kernel skips them.
 * G3_ERR_ARG, with nothing launched and one message each: everything g3_self_attn_fwd_window_bf16 refuses (with Skv_buf in the place of S for the V^T
 * leading dimension and the 32-bit offsets); Sq no multiple of frame_len; total_frames <= 0 or q_frame0 < 0; not 0 <= a <= b;
 * q_frame0 + Sq / frame_len > total_frames; Skv_buf not (a + c - b) * frame_len for a c in [b, total_frames]; a buffer that does not hold the key
 * set of some query block (the host walks the blocks: this is what keeps a wrong exchange plan from becoming a read outside the operand).
 * g3_attn_window_cp_plan_bf16: the dry run, as g3_attn_window_plan_bf16. g3_self_attn_window_cp_tiles: the (query block, 64-key tile) pairs this
 * rank's launch visits, and its query blocks times the tiles of the whole sequence; the same refusals. */
int g3_self_attn_fwd_window_cp_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                    int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, void* o, int64_t o_row,
                                    int64_t o_batch, int64_t o_head, int Sq, int Skv_buf, int B, int H, int head_dim, float softmax_scale,
                                    float logit_bound, int frame_len, int total_frames, int q_frame0, int buf_head_frames, int buf_tail_frame0,
                                    int window_frames, int sink_frames, void* stream);
const char* g3_attn_window_cp_plan_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                        int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, void* o, int64_t o_row,
                                        int64_t o_batch, int64_t o_head, int Sq, int Skv_buf, int B, int H, int head_dim, float softmax_scale,
                                        float logit_bound, int frame_len, int total_frames, int q_frame0, int buf_head_frames, int buf_tail_frame0,
                                        int window_frames, int sink_frames);
int g3_self_attn_window_cp_tiles(int Sq, int Skv_buf, int frame_len, int total_frames, int q_frame0, int buf_head_frames, int buf_tail_frame0,
                                 int window_frames, int sink_frames, int64_t* attended, int64_t* dense);

/* Self-attention (Sq == Skv == S, S % 64 == 0) over a RANGE TABLE, for tokens ordered (t, h, w): opt-in, training-free sparse attention whose key set
 * is, per block of query rows, a short list of contiguous key ranges - the shape of the published sparse patterns for video DiTs in this token order
 * (a spatial band that narrows with frame distance, per-head spatial / temporal patterns, sliding tiles). Definitions:
 *   query block b   rows [256 b, min(256 b + 256, S)); 256 = g3_self_attn_window_q_rows(); n_qblk = ceil(S / 256)
 *   range table     int32 ranges[n_patterns][n_qblk][max_ranges][2] of (first_key, n_keys) pairs, 1 <= max_ranges <= 64 = g3_self_attn_ranges_max();
 *                   n_keys == 0 ends a block's list
 *   a valid list    has at least one range; first_key and n_keys are positive multiples of 64, except that first_key may be 0; it is ascending
 *                   and disjoint, first_key[r + 1] >= first_key[r] + n_keys[r] (touching ranges are allowed and stay two ranges);
 *                   first_key + n_keys <= S; the entries behind the terminator are zero
 *   head_pattern    optional int32 [H], values in [0, n_patterns): the pattern of a head. NULL: pattern 0 for every head
 * Every row of query block b of head h attends the keys of the list (head_pattern[h], b), and the output is the exact softmax over those keys, visited
 * in list order. The function is block-granular and tile-granular by construction: nothing is masked in the kernel's tile loop.
 * ranges and head_pattern are DEVICE pointers. flash_attn_fwd_w4b_nm_rng_kernel<true> (0 < logit_bound * log2(e) <= 60) or
 * flash_attn_fwd_w4b_rng_kernel<true> (any other bound: the running-maximum form); always variant 11's family, never another kernel. The launch does not
 * read the table on the host: validate it once with g3_attn_ranges_check before the upload. The kernel clamps every range (and the pattern index) to
 * the operand, so a table that breaks the rules gives unspecified values in o and never an access outside K / V^T.
 * G3_ERR_ARG, with nothing launched and one message each: S no positive multiple of 64; n_patterns < 1; max_ranges outside [1, 64]; a NULL or
 * misaligned table (8 bytes; head_pattern 4); a V^T leading dimension below ceil64(S); operands beyond the kernel's 32-bit byte offsets over all S keys
 * (g3_self_attn_fwd_window_bf16's arithmetic); misaligned pointers or strides; head_dim != 128.
 * g3_attn_ranges_plan_bf16: the dry run - the kernel's name, or NULL with g3_last_error() set exactly as the call sets it; no HIP call, no pointer
 * dereferenced. g3_attn_ranges_check: pure host code over HOST copies - every rule above, refused with a message that names the pattern, the block
 * and the range; attended = the (head, query block, 64-key tile) triples a launch with H heads visits, dense = H * n_qblk * S / 64. */
int g3_self_attn_fwd_ranges_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                 int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, void* o, int64_t o_row,
                                 int64_t o_batch, int64_t o_head, int S, int B, int H, int head_dim, float softmax_scale, float logit_bound,
                                 const int32_t* ranges, int n_patterns, int max_ranges, const int32_t* head_pattern, void* stream);
const char* g3_attn_ranges_plan_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                     int64_t k_head, const void* vt, int64_t vt_row, int64_t vt_batch, int64_t vt_head, void* o, int64_t o_row,
                                     int64_t o_batch, int64_t o_head, int S, int B, int H, int head_dim, float softmax_scale, float logit_bound,
                                     const int32_t* ranges, int n_patterns, int max_ranges, const int32_t* head_pattern);
int g3_attn_ranges_check(const int32_t* ranges_host, int n_patterns, int S, int max_ranges, const int32_t* head_pattern_host, int H, int64_t* attended,
                         int64_t* dense);
int g3_self_attn_ranges_max(void);

/* Per-head choice among the patterns of a range table, made on the device, in stream order, from the q and k of the forward that is running (opt-in; the
 * online head classification of the published training-free sparse schemes for video DiTs). A few query rows per head are profiled against every
 * candidate pattern and each head gets the pattern that loses least of its softmax mass. Definitions, for sample row r = sample_rows[i] (int32,
 * strictly ascending, in [0, S), 1 <= n <= 64), batch b, head h:
 *   l_j            = softmax_scale * (q_r . k_j) over ALL S keys, m = max_j l_j (always a running maximum: no logit bound, no dependence on QK-norm)
 *   recall[b][h][i][p] = sum over the keys j of the list (pattern p, block r / 256) of exp(l_j - m)  /  sum over all j of exp(l_j - m):
 *                    the share of the row's softmax mass pattern p keeps. 2 (1 - recall) is the L1 distance between the row's dense and masked
 *                    softmax weights; no V is needed. Membership is tile-granular, as in the attention kernel.
 *   score[h][p]    = mean of recall over b and i, summed in that order;  head_pattern[h] = argmax_p score[h][p], the lowest index on ties.
 * A pattern whose list holds every tile has recall == 1.0f exactly: every tile's row sum enters the dense accumulator and each member pattern's
 * accumulator as the same value by the same operations. Deterministic: no atomics, fixed merge orders.
 * g3_attn_pattern_profile_bf16: q, k [S*B, H*128] bf16 strided as for g3_self_attn_fwd_ranges_bf16 (element strides; row s*B + b); sample_rows and
 *   tile_member are DEVICE pointers; tile_member is uint8 [n][S / 64], bit p = "tile in pattern p's list for that sample row's block"
 *   (g3_attn_profile_members builds it on the host from HOST copies of a table g3_attn_ranges_check accepted); n_chunks in [1, S / 64] key chunks
 *   (g3_attn_profile_chunks: the default, two workgroups per CU); workspace of g3_attn_profile_workspace_bytes(B, H, n_chunks) bytes; recall is
 *   float [B][H][n][n_patterns]. The kernel clamps the sample rows to [0, S - 1].
 * G3_ERR_ARG, with nothing launched and one message each: a NULL operand; head_dim != 128; S no positive multiple of 64; n_patterns outside [1, 8];
 *   n outside [1, 64]; n_chunks outside [1, S / 64]; misaligned pointers (q, k 16 bytes) or strides (8 elements); a workspace too small; operands
 *   beyond the kernel's 32-bit byte offsets over all S rows.
 * g3_attn_pattern_profile_plan_bf16: the dry run - the kernel's name, or NULL with g3_last_error() set exactly as the call sets it; no HIP call.
 * g3_attn_pattern_select: recall -> score [H][n_patterns] (optional, may be NULL) and int32 head_pattern [H], all on the device. */
int g3_attn_pattern_profile_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row, int64_t k_batch,
                                 int64_t k_head, int S, int B, int H, int head_dim, float softmax_scale, const int32_t* sample_rows, int n,
                                 const uint8_t* tile_member, int n_patterns, int n_chunks, void* workspace, size_t workspace_bytes, float* recall,
                                 void* stream);
const char* g3_attn_pattern_profile_plan_bf16(const void* q, int64_t q_row, int64_t q_batch, int64_t q_head, const void* k, int64_t k_row,
                                              int64_t k_batch, int64_t k_head, int S, int B, int H, int head_dim, float softmax_scale,
                                              const int32_t* sample_rows, int n, const uint8_t* tile_member, int n_patterns, int n_chunks,
                                              void* workspace, size_t workspace_bytes, float* recall);
int g3_attn_pattern_select(const float* recall, int B, int H, int n, int n_patterns, float* score, int32_t* head_pattern, void* stream);
size_t g3_attn_profile_workspace_bytes(int B, int H, int n_chunks);
int g3_attn_profile_chunks(int S, int B, int H);
int g3_attn_profile_members(const int32_t* ranges_host, int n_patterns, int S, int max_ranges, const int32_t* sample_rows_host, int n,
                            uint8_t* member_out);

int g3_attn_merge_partials_bf16(const float* const* o_parts /*host*/, const float* const* lse_parts /*host*/, int n_parts, int64_t p_row,
                                int64_t p_batch, int64_t p_head, void* out, int64_t o_row, int64_t o_batch, int64_t o_head, int Sq, int B,
                                int H, int head_dim, void* stream);

/* V [S][B][H][128] (row stride ld_in) -> V^T [B][H][128][ldvt], zero-filling kv in [S, ldvt). */
int g3_transpose_v_bf16(const void* v, int64_t ld_in, void* vt, int64_t ldvt, int S, int B, int H, int head_dim,
                        void* stream);

/* Head-parallel context parallelism: the layout passes around an all-to-all that trades a rank's tokens of ALL heads for all tokens of H / n
 * heads, in place of the K / V ring TransformerEngine runs behind attn_op.set_context_parallel_group (general_dit.py:536-541) and next to
 * split_inputs_cp / cat_outputs_cp (module/parallel.py:25-87), which shard the same rows.
 * scatter: for each non-NULL x of q, k, v (column views [rows][H * 128] of one buffer with row stride ld_in; any of them may be NULL, not all):
 *   x_out[d][r][j] = x[r][(d * (H / n_dest) + head0) * 128 + j],  d < n_dest, r < rows, j < Hg * 128;
 *   x_out is contiguous [n_dest][rows][Hg * 128]: one contiguous chunk per destination rank, what a single-tensor all-to-all sends.
 * gather (the inverse, after the returning all-to-all): in [n_src][rows][Hg * 128] contiguous ->
 *   out[r][(s * (H / n_src) + head0) * 128 + j] = in[s][r][j],  out rows of stride ld_out; the other columns of out are not touched.
 * 16-byte loads and stores, 64-bit offsets. G3_ERR_ARG before any launch: H % n != 0, head0 + Hg > H / n (or head0 < 0, Hg <= 0), rows <= 0,
 * a leading dimension below H * 128 or not a multiple of 8, a pointer that is not 16-byte aligned, an input without its output. */
int g3_cp_scatter_heads_bf16(const void* q, const void* k, const void* v, int64_t ld_in, void* q_out, void* k_out, void* v_out, int64_t rows,
                             int H, int n_dest, int head0, int Hg, void* stream);
int g3_cp_gather_heads_bf16(const void* in, void* out, int64_t ld_out, int64_t rows, int H, int n_src, int head0, int Hg, void* stream);

/* ---- norms -----------------------------------------------------------------------------------------------------
 * out = LayerNorm(x; no affine, eps) * (1 + scale[row % mod_rows]) + shift[row % mod_rows]
 * replaces DITBuildingBlock.norm_state + adaln_norm_state (blocks.py:339-341, 408) and FinalLayer (blocks.py:204, 239). */
int g3_layernorm_modulate_bf16(const void* x, int64_t ldx, const void* shift, const void* scale, int64_t ldmod,
                               int mod_rows, void* out, int64_t ldo, int rows, int D, float eps, void* stream);

/* The same with the result as MXFP8 (opt-in MXFP8 linears): q [rows][ldq] e4m3fn + scales [rows][lds] E8M0, bitwise what g3_quant_mxfp8_bf16
 * makes of g3_layernorm_modulate_bf16's `out` under the same "ln_wave_rows" option - each value is rounded to bf16 first, then quantised in the
 * kernel's registers; no bf16 output is written. Refuses what the bf16 call refuses and D % 32 != 0, ldq < D, ldq % 8 != 0, lds < D/32,
 * q not 8-byte aligned, NULL q / scales (G3_ERR_ARG before any launch). */
int g3_layernorm_modulate_mxfp8(const void* x, int64_t ldx, const void* shift, const void* scale, int64_t ldmod, int mod_rows, void* q,
                                int64_t ldq, void* scales, int64_t lds, int rows, int D, float eps, void* stream);

/* per-head RMSNorm(weight[128], eps) then (optional) non-interleaved RoPE with f32 cos/sin tables [S][128]:
 * replaces te.pytorch.RMSNorm + apply_rotary_pos_emb(fused=True) in Attention.cal_qkv (attention.py:262-280).
 * in/out rows are (s, b) pairs, b fastest; cos_table == sin_table == NULL skips RoPE (cross-attention, k of context). */
int g3_qk_rmsnorm_rope_bf16(const void* in, int64_t ld_in, const void* weight, const float* cos_table,
                            const float* sin_table, void* out, int64_t ld_out, int S, int B, int H, int head_dim,
                            float eps, void* stream);

/* The same pass over TWO adjacent head ranges with their own norm weights in one launch: heads [0, H_q) of a row with weight_q, heads
 * [H_q, H_q + H_k) with weight_k - q and k of the fused QKV buffer as Attention.cal_qkv normalises and rotates them (attention.py:262-280:
 * to_q[1] / to_k[1] then apply_rotary_pos_emb on both). in / out: [S*B][(H_q + H_k) * 128] views (out may alias in). */
int g3_qk_rmsnorm_rope_pair_bf16(const void* in, int64_t ld_in, const void* weight_q, int H_q, const void* weight_k, int H_k,
                                 const float* cos_table, const float* sin_table, void* out, int64_t ld_out, int S, int B, int head_dim,
                                 float eps, void* stream);

/* Q / K(/V) projection with that per-head RMSNorm (+ RoPE) in the GEMM's epilogue (Attention.cal_qkv, attention.py:247-280, as one call):
 *   C[:, 0:n_q] = rope(rmsnorm(A W^T, norm_q)),  C[:, n_q:n_q+n_k] = rope(rmsnorm(A W^T, norm_k)),  C[:, n_q+n_k:N] = A W^T (e.g. v).
 * Row m is token (s = m / B, b = m % B); n_q, n_k, N multiples of 128 (whole heads); cos / sin fp32 [M/B][128] or both NULL. Same
 * rounding points as g3_gemm_bf16_nt followed by g3_qk_rmsnorm_rope_bf16 in place (which is what runs where the fused kernel does not apply).
 * vt != NULL: the remaining (v) heads are written TRANSPOSED, vt[b][h][d][s] with row length vt_ld >= M/B (g3_transpose_v_bf16's layout:
 * what g3_flash_attn_fwd_bf16 takes; positions >= M/B written as zeros up to the end of the last 32-row block, the rest of the tail is the
 * caller's: allocate it zeroed once), and their columns of C are NOT written. */
int g3_gemm_qk_norm_rope_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                              int n_q, int n_k, const void* norm_q, const void* norm_k, const float* cos_table,
                              const float* sin_table, int B, float eps, void* vt, int64_t vt_ld, void* stream);

/* Top of a DiT block in ONE pass over x:  x += extra_per_block_pos_emb  (in place; blocks.py:547-548), then
 * out = LayerNorm(x) * (1 + scale) + shift  as g3_layernorm_modulate_bf16. The [S*B, D] embedding is not read from memory: it is
 * rebuilt per row from LearnablePosEmbAxis' three tables pe_t [T,D], pe_h [Hp,D], pe_w [Wp,D] with the reference's bf16 rounding
 * points (position_embedding.py:218-233; normalize, attention.py:108-124):  bf16(bf16(bf16(pe_t+pe_h)+pe_w) / pos_norm[s]),
 * pos_norm [T*Hp*Wp] bf16 = 1e-6 + ||.||_2 / sqrt(D) per token. x: [T*Hp*Wp*B, D] rows (s, b), b fastest. With context
 * parallelism pe_t / pos_norm point at this rank's frames.  * pe_h == pe_w == pos_norm == NULL: pe_t is the finished (summed, normalised, rounded) embedding [T*Hp*Wp][D] and every row
 * reads one table row instead of three (what gen3c_amd/dit.py passes: the table is input-independent and built once per shape). */
int g3_posemb_layernorm_modulate_bf16(void* x, int64_t ldx, const void* pe_t, const void* pe_h, const void* pe_w,
                                      const void* pos_norm, int T, int Hp, int Wp, int B, const void* shift, const void* scale,
                                      int64_t ldmod, int mod_rows, void* out, int64_t ldo, int D, float eps, void* stream);

/* g3_posemb_layernorm_modulate_bf16 with the result as MXFP8 (see g3_layernorm_modulate_mxfp8: same output rules and refusals); x is updated
 * in place exactly as by the bf16 call. */
int g3_posemb_layernorm_modulate_mxfp8(void* x, int64_t ldx, const void* pe_t, const void* pe_h, const void* pe_w, const void* pos_norm, int T,
                                       int Hp, int Wp, int B, const void* shift, const void* scale, int64_t ldmod, int mod_rows, void* q,
                                       int64_t ldq, void* scales, int64_t lds, int D, float eps, void* stream);

/* x += y (n % 8 == 0): "x = x + extra_per_block_pos_emb" (blocks.py:547-548). */
int g3_add_inplace_bf16(void* x, const void* y, int64_t n, void* stream);

/* DiT input/output plumbing. patchify: channel-concatenates up to 4 bf16 sources ([B,C_i,T,H,W] contiguous, or [B,C_i,H,W]
 * broadcast over T when has_t[i] == 0 - the padding mask) and gathers patch_t x patch_s x patch_s patches into the token-major
 * matrix out[(t h w) b][(c r m n)] the embedding GEMM reads (general_dit_video_conditioned.py:77-101, blocks.py:154-159).
 * srcs / chans / has_t are HOST arrays of n_src entries. unpatchify: final-layer rows y[(t h w) b][(p1 p2 t C)] (ld = ldy) ->
 * out [B,C_out,T,H,W] (general_dit.py:348-357). timestep_embedding: timesteps f32 [B] (device) -> t_sin bf16 [B,D] = [cos | sin]
 * sinusoid (blocks.py:38-57) and emb bf16 [B,D] = its affine RMSNorm with norm_weight [D], eps 1e-6 (general_dit.py:173-177). */
int g3_dit_patchify_bf16(const void* const* srcs, const int* chans, const int* has_t, int n_src, void* out, int B, int T, int H,
                         int W, int patch_t, int patch_s, void* stream);
int g3_dit_unpatchify_bf16(const void* y, int64_t ldy, void* out, int B, int C_out, int T, int H, int W, int patch_t, int patch_s,
                           void* stream);
int g3_timestep_embedding_bf16(const float* timesteps, const void* norm_weight, void* t_sin, void* emb, int B, int D, void* stream);

/* ---- EDM-Euler sampler step (model_v2w.py:130-149, 201-259; diffusers 0.32.2 EDMEulerScheduler) ------------------
 * Two fused elementwise passes around the two network calls of one denoise step, over a [B,C,T,H,W] latent of n
 * elements (hw = H*W, indicator = f32 [T], 1 on conditioning frames). Scalar coefficients are evaluated by the host
 * in the dtypes the reference uses (see gen3c_amd/sampler.py) and passed as floats.
 *   prepare: new_xt = bf16(ind*((gt+noise*aug)*c_in_aug/c_in_bf16) + (1-ind)*xt); new_xt_scaled = bf16(new_xt*c_in_step)
 *   step   : net = cond + g*(cond-uncond); replace conditioning frames by the (un-preconditioned) latent; Euler update
 *            x + (x - x0) * inv_sigma * (sigma_next - sigma), inv_sigma = fp32 1 / sigma from the host (what torch's device
 *            division by a CPU 0-dim tensor computes). */
int g3_edm_prepare_input_bf16(const void* xt, const void* gt_latent, const float* noise, const float* indicator,
                              void* new_xt, void* new_xt_scaled, int64_t n, int T, int hw, float augment_sigma,
                              float c_in_aug, float c_in_bf16, float c_in_step, void* stream);
int g3_edm_cfg_euler_step_bf16(const void* out_cond, const void* out_uncond, const void* new_xt, const void* gt_latent,
                               const float* indicator, void* xt_next, int64_t n, int T, int hw, float guidance,
                               float c_skip_bf16, float c_out_bf16, float c_skip, float c_out, float sigma,
                               float inv_sigma, float sigma_next, void* stream);
/* Opt-in second-order multistep solver "2ab" (Adams-Bashforth exponential integrator, arXiv 2308.02157; the reference's
 * functional/multi_step.py::order2_fn). The step entry's chain up to the fp32 x0 prediction, unchanged, then
 *   have_prev == 0: the Euler update above, the same bits as g3_edm_cfg_euler_step_bf16;
 *   have_prev != 0: xt_next = bf16(a*x + (cb1*x0 + cb2*x0_prev)), fp32, evaluated in that order without contraction. With
 *     s = sigma, t = sigma_next, s1 = the previous step's sigma: dt = log(s/t), c2 = log(s/s1)/dt, phi1(u) = expm1(u)/u,
 *     phi2(u) = (phi1(u)-1)/u, a = exp(-dt), cb1 = dt*(phi1(-dt) - phi2(-dt)/c2), cb2 = dt*phi2(-dt)/c2 (host, fp64, passed as fp32).
 * Both write x0_out (f32 [n]), the next step's x0_prev. x0_out may alias x0_prev: every element is read before it is written,
 * by the same thread. No other aliasing is allowed. Refused: null operands (x0_prev only when have_prev), bad shapes, sigma <= 0,
 * and with have_prev a non-finite or non-positive a. */
int g3_edm_cfg_2ab_step_bf16(const void* out_cond, const void* out_uncond, const void* new_xt, const void* gt_latent,
                             const float* indicator, void* xt_next, int64_t n, int T, int hw, float guidance, float c_skip_bf16,
                             float c_out_bf16, float c_skip, float c_out, float sigma, float inv_sigma, float sigma_next,
                             const float* x0_prev, float* x0_out, int have_prev, float a, float cb1, float cb2, void* stream);
/* Opt-in guidance interval (classifier-free guidance only while sigma_lo < sigma <= sigma_hi: Kynkaanniemi et al., "Applying Guidance in a
 * Limited Interval Improves Sample and Distribution Quality in Diffusion Models", arXiv 2404.07724; the reference's loop, model_v2w.py:130-149,
 * guides every step). The step of a sigma outside the interval: the two entries above without out_uncond and guidance - net_output = out_cond,
 * no arithmetic on it - and from the conditioning-frame replacement on the same chain, operation for operation and rounding for rounding
 * (g3_edm_cfg_*_step_bf16 with guidance 0 computes the same values; it still reads an out_uncond, these do not). x0_prev / x0_out / have_prev /
 * a / cb1 / cb2 as in g3_edm_cfg_2ab_step_bf16, x0_out may alias x0_prev. Refused like their counterparts: null operands (x0_prev only when
 * have_prev), bad shapes, sigma <= 0, a bad inv_sigma, and with have_prev a non-finite or non-positive a. */
int g3_edm_cond_euler_step_bf16(const void* out_cond, const void* new_xt, const void* gt_latent, const float* indicator, void* xt_next,
                                int64_t n, int T, int hw, float c_skip_bf16, float c_out_bf16, float c_skip, float c_out, float sigma,
                                float inv_sigma, float sigma_next, void* stream);
int g3_edm_cond_2ab_step_bf16(const void* out_cond, const void* new_xt, const void* gt_latent, const float* indicator, void* xt_next,
                              int64_t n, int T, int hw, float c_skip_bf16, float c_out_bf16, float c_skip, float c_out, float sigma,
                              float inv_sigma, float sigma_next, const float* x0_prev, float* x0_out, int have_prev, float a, float cb1,
                              float cb2, void* stream);

/* ---- 3D-cache renderer (all f32; n "items" = (target frame, cache buffer) pairs, each h x w) -----------------------
 * Replaces forward_warp(depth1=None, world_points1=...) + bilinear_splatting + the mesh-occlusion branch
 * (cosmos_predict1/diffusion/inference/forward_warp_utils_pytorch.py:171-336, 462-486, 576-695, 49-132) and the NVIDIA
 * Warp ray/triangle kernel (ray_triangle_intersection_warp.py:23-105).
 * The reference takes max(log1p(z)) over every item of one forward_warp call (warp_chunk_size = 2 items,
 * cache_3d.py:183); `group_size` reproduces that grouping: item i belongs to group i / group_size.
 *   project : points [n][h][w][3], w2c [n][16], K [n][9], mask1 [n][h][w] or NULL ->
 *             z [n][h][w], flow [n][2][h][w] (= forward_warp's flow12), cam_points [n][h][w][3] or NULL,
 *             maskz = mask1*(z>0) [n][h][w], group_max [ceil(n/group_size)] u32 (float bits; ZERO it before the call)
 *   splat   : accumulates (r,g,b,z,weight) into accum [n][h+2][w+2][5] (ZERO it before the call)
 *   resolve : frame [n][3][h][w] (fill -1, clamp [-1,1]), mask [n][h][w], depth [n][h][w] or NULL (fill 0)
 *   mesh_occlusion: boundary_mask [n][h][w] u8, Kinv [n][9]; scratch pts_ds [n][h/f][w/f][3], mask_ds [n][h/f][w/f] u8,
 *             tmin [n][h][w] u32; zeroes mask/depth and sets frame to -1 where the boundary mesh is closer by > 0.02. */
int g3_warp_project_f32(const float* points, const float* w2c, const float* K, const float* mask1, float* z, float* flow,
                        float* cam_points, float* maskz, void* group_max, int n, int h, int w, int group_size, void* stream);
int g3_warp_splat_f32(const float* image, const float* z, const float* flow, const float* maskz, const void* group_max,
                      float* accum, int n, int h, int w, int group_size, void* stream);
int g3_warp_resolve_f32(const float* accum, float* frame, float* mask, float* depth, int n, int h, int w, void* stream);

/* g3_warp_splat_f32 + g3_warp_resolve_f32 in one call without global atomics on the common path: every 32x32 source tile stores its 40x40
 * destination window (32 KiB; size the workspace with g3_warp_windows_workspace_bytes, never from this text) into `workspace` and a destination-owning pass sums the overlapping windows in a fixed order and resolves the pixel
 * (bilinear_splatting + the normalisation / clamp of forward_warp, forward_warp_utils_pytorch.py:576-695,300-334). Same contributions as
 * the two-call form (whose accumulator still receives the rare out-of-window corners here: zero it first). workspace: g3_warp_windows_workspace_bytes(n, h, w) bytes, 16-byte aligned. depth may be NULL. */
size_t g3_warp_windows_workspace_bytes(int n, int h, int w);
int g3_warp_splat_resolve_f32(const float* image, const float* z, const float* flow, const float* maskz, const void* group_max,
                              float* accum, void* workspace, float* frame, float* mask, float* depth, int n, int h, int w,
                              int group_size, void* stream);
/* One call per batch of render items (Cache3D_Base.render_cache, cache_3d.py:151-236): n items = (target camera, cached source view) pairs rendered
 * from n_src source views WITHOUT replicating the sources - item i reads source src_index[i] (device int32 [n]): points_src [n_src][h][w][3],
 * image_src [n_src][3][h][w], mask_src [n_src][h][w] or NULL, boundary_src u8 [n_src][h][w] or NULL (NULL = no foreground masking; else Kinv
 * [n][9] and depth are required). w2c [n][16], K [n][9] are the TARGET cameras. Runs project -> window splat -> gather / resolve -> (mesh
 * occlusion) as g3_warp_project_f32 + g3_warp_splat_resolve_f32 + g3_mesh_occlusion_f32 would on expanded inputs (same arithmetic, same
 * group_size pairing). Outputs frame [n][3][h][w], mask [n][h][w], depth [n][h][w] or NULL, flow_out [n][2][h][w] or NULL.
 * workspace: g3_render_workspace_bytes(n, h, w, group_size) bytes, 256-byte aligned, prepared ONCE by g3_render_workspace_init for exactly this
 * (n, h, w, group_size) and then reused call after call: the dense out-of-window accumulator inside it is kept all-zero by the kernels
 * themselves (items whose accumulator a launch touched are stamped, and only those are read back and cleared), so no per-call clearing pass;
 * likewise the nearest-hit buffer of the occlusion pass is left at +inf by the resolve pass (per-tile stamps). With foreground masking the
 * occlusion is applied inside the resolve pass (the arithmetic of g3_mesh_occlusion_f32's apply step on the values being written), and the
 * marking / rasterising pass runs on a stream the library owns, forked from and joined back into `stream` with events inside this call (all
 * inputs must be ready on `stream` at call time, as for every entry point; option render_overlap = 0 keeps everything on `stream`). Limits:
 * h < 32766, w < 65534 (packed texel ids); calls that share a workspace must be ordered (same stream). */
size_t g3_render_workspace_bytes(int n, int h, int w, int group_size);
int g3_render_workspace_init(void* workspace, int n, int h, int w, int group_size, void* stream);
int g3_render_items_f32(const float* points_src, const float* image_src, const float* mask_src, const uint8_t* boundary_src,
                        const int* src_index, const float* w2c, const float* K, const float* Kinv, void* workspace, float* frame, float* mask,
                        float* depth, float* flow_out, int n, int n_src, int h, int w, int group_size, void* stream);
int g3_mesh_occlusion_f32(const float* cam_points, const uint8_t* boundary_mask, const float* K, const float* Kinv,
                          float* pts_ds, uint8_t* mask_ds, void* tmin, float* frame, float* mask, float* depth, int n, int h,
                          int w, int factor, void* stream);
/* cache construction: unproject_points(is_depth=True) (forward_warp_utils_pytorch.py:410-460; c2w = inverse(w2c), Kinv =
 * inverse(K), both [n][..] f32 computed by the host) and reliable_depth_mask_range_batch (:338-353) -> u8 mask. */
int g3_unproject_points_f32(const float* depth, const float* c2w, const float* Kinv, float* points, int n, int h, int w,
                            void* stream);
int g3_reliable_depth_mask_f32(const float* depth, uint8_t* out, int n, int h, int w, int window, float ratio_thresh,
                               float eps, void* stream);
/* autoregressive cache update: camera_utils.align_depth (camera_utils.py:225-345) for one [H][W] fp32 depth map, enqueued on
 * `stream` without host synchronisation. Rigid part: 10 %/90 % quantile outlier rejection (torch.quantile 'linear' rank
 * arithmetic) + affine fit in inverse depth. non_rigid != 0 adds `num_iters` Adam steps (lr, betas 0.9/0.999, eps 1e-8) on a
 * per-pixel scale map with the reference's data + lambda_arap * 3x3-ARAP loss; T_host = first three rows of inv(c2w) (12
 * floats - unproject_points inverts what align_depth passes in its w2c slot) and Kinv_host = inverse(K) (9 floats) are HOST
 * pointers, read at call time. target_mask: u8 [H][W] or NULL (= all pixels). out_depth may not alias the inputs.
 * workspace: device memory, 256-byte aligned, at least g3_align_depth_workspace_bytes(H, W) bytes. */
size_t g3_align_depth_workspace_bytes(int H, int W);
int g3_align_depth_f32(const float* source_depth, const float* target_depth, const uint8_t* target_mask, const float* Kinv_host,
                       const float* T_host, int non_rigid, int num_iters, float lambda_arap, float lr, float* out_depth,
                       void* workspace, size_t workspace_bytes, int H, int W, void* stream);

/* ---- causal video tokenizer (Cosmos-Tokenize1-CV8x8x8; tokenizer/modules/{layers3d,patching,utils}.py) ---------------
 * Activations are channels-last bf16 [T][H][W][C] for one batch item.
 * conv3d_cl: CausalConv3d (layers3d.py:50-97) as an implicit GEMM on the MFMA kernel. Output position (to,yo,xo), tap
 *   (dt,dy,dx) reads ti = max(to*st+ot+dt, 0) (first frame replicated in front), yi = yo*sh+oh+dy, xi = xo*sw+ow+dx
 *   (outside the frame = zero padding). w is tap-major [kt*kh*kw][N][ldw]; bias [N] or NULL; residual (needs bias) is
 *   added after the bias: out = conv(in) + bias + residual  (res-block skip, hybrid up/down-sample "+ x").
 * groupnorm_swish_cl: CausalNormalize = GroupNorm(1 group, eps) per frame (+ optional x*sigmoid(x)); stats_f64 is a
 *   [frames][2] double scratch. haar3d_(un)patch: Patcher3D/UnPatcher3D, patch_size 4; video is planar [3][T][H][W].
 * resample_cl modes: 0 avg-pool(1,2,2) on right/bottom zero pad, 1 avg-pool(2,1,1) on front-replicated input,
 *   2 repeat_interleave(2) in time minus the first frame, 3 repeat_interleave(2) in H and W (layers3d.py:135-234).
 * softmax_rows / transpose2d / temporal_attn_cl: CausalAttnBlock and CausalTemporalAttnBlock (layers3d.py:345-427). */
int g3_conv3d_cl_bf16(const void* in, int64_t ld_in, const void* w, int64_t ldw, const void* bias, const void* residual,
                      int64_t ldr, void* out, int64_t ld_out, int K, int N, int Ti, int Hi, int Wi, int To, int Ho, int Wo,
                      int kt, int kh, int kw, int st, int sh, int sw, int ot, int oh, int ow, void* stream);
/* g3_conv3d_cl_gnstats_bf16: the same convolution, which additionally ADDS per output frame (gn_rows_per_frame = Ho*Wo consecutive output rows)
 * the sum and sum of squares of its stored bf16 outputs to gn_stats_f64[frame][0 / 1] (doubles, zeroed by the caller) - in the kernel's epilogue
 * where the one-wave-per-SIMD convolution kernel runs, by a statistics pass otherwise. g3_groupnorm_stats_cl_bf16 / g3_groupnorm_apply_cl_bf16
 * are the two halves of g3_groupnorm_swish_cl_bf16: statistics (added to a zeroed buffer), and the normalisation given finished statistics
 * - CausalNormalize of a tensor whose producing convolution already delivered them reads the tensor once instead of twice. */
int g3_conv3d_cl_gnstats_bf16(const void* in, int64_t ld_in, const void* w, int64_t ldw, const void* bias, const void* residual,
                              int64_t ldr, void* out, int64_t ld_out, int K, int N, int Ti, int Hi, int Wi, int To, int Ho, int Wo,
                              int kt, int kh, int kw, int st, int sh, int sw, int ot, int oh, int ow, void* gn_stats_f64,
                              int gn_rows_per_frame, void* stream);

/* Dry run of the bf16 GEMM entries (g3_gemm_bf16_nt, g3_gemm_qk_norm_rope_bf16, g3_conv3d_cl_bf16, g3_conv3d_cl_gnstats_bf16): the call record those
 * entries fill, and the name of the kernel instantiation the call would launch with exactly these arguments under the options in force - every check
 * and the whole kernel choice of the real call - or NULL where the call would be refused, with g3_last_error() set exactly as the call sets it.
 * n_cu: the device's CU count the choice assumes (0 = the current device's). *grid (if not NULL): workgroups of that launch; *follow_up (if not
 * NULL): the G3_GEMM_THEN_* launches the entry makes after it. Nothing is launched, the plan itself makes no HIP call and no pointer is dereferenced
 * (pointers are tested for NULL and alignment only). Fields `entry` does not take are ignored. */
enum g3_gemm_entry { G3_GEMM_ENTRY_NT = 0, G3_GEMM_ENTRY_QK_NORM_ROPE = 1, G3_GEMM_ENTRY_CONV = 2, G3_GEMM_ENTRY_CONV_GNSTATS = 3 };
typedef struct g3_gemm_call {
    int entry;                                                                         /* enum g3_gemm_entry */
    const void* A; int64_t lda; const void* W; int64_t ldw; void* C; int64_t ldc;      /* conv: in / ld_in, w / ldw, out / ld_out */
    int M, N, K;                                                                       /* conv: M = To*Ho*Wo is derived */
    int epilogue; const void* gate; int gate_rows; int64_t ldg;                        /* NT only, but gate: also the conv's bias */
    const void* residual; int64_t ldr;                                                 /* NT and conv */
    int n_q, n_k; const void* norm_q; const void* norm_k; const float* cos_table; const float* sin_table; int B; float eps; void* vt; int64_t vt_ld;
    int Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw, st, sh, sw, ot, oh, ow;                    /* conv geometry */
    void* gn_stats; int gn_rows;                                                       /* CONV_GNSTATS: gn_stats_f64, gn_rows_per_frame */
    void* stream;                                                                      /* (not read by the dry run) */
} g3_gemm_call;
#define G3_GEMM_THEN_NORM_Q 1u   /* g3_qk_rmsnorm_rope_bf16 over the q heads (the norm / RoPE epilogue does not apply) */
#define G3_GEMM_THEN_NORM_K 2u   /* ... over the k heads */
#define G3_GEMM_THEN_VT 4u       /* g3_transpose_v_bf16 of C's v columns (the epilogue does not write V^T for this call) */
#define G3_GEMM_THEN_GN_STATS 8u /* g3_groupnorm_stats_cl_bf16 over the finished output (the statistics are not taken in the epilogue) */
const char* g3_gemm_plan_bf16(const g3_gemm_call* call /*host*/, int n_cu, int* grid /*host*/, unsigned* follow_up /*host*/);

int g3_groupnorm_stats_cl_bf16(const void* x, int64_t ld, void* stats_f64, int frames, int rows_per_frame, int C, void* stream);
int g3_groupnorm_apply_cl_bf16(const void* x, int64_t ld, const void* gamma, const void* beta, const void* stats_f64, void* out,
                               int64_t ldo, int frames, int rows_per_frame, int C, float eps, int swish, void* stream);
int g3_groupnorm_swish_cl_bf16(const void* x, int64_t ld, const void* gamma, const void* beta, void* stats_f64, void* out,
                               int64_t ldo, int frames, int rows_per_frame, int C, float eps, int swish, void* stream);
int g3_haar3d_patch_bf16(const void* video, void* out, int T, int H, int W, void* stream);
int g3_haar3d_unpatch_bf16(const void* coef, int64_t ld, void* video, int Tp, int Hp, int Wp, void* stream);
int g3_resample_cl_bf16(const void* in, void* out, int Ti, int Hi, int Wi, int C, int mode, void* stream);
int g3_softmax_rows_bf16(void* x, int64_t ld, int rows, int n, float scale, void* stream);
int g3_transpose2d_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int R, int C, void* stream);
int g3_temporal_attn_cl_bf16(const void* q, const void* k, const void* v, void* o, int T, int HW, int C, float scale,
                             void* stream);
/* CausalAttnBlock's attention core (tokenizer/modules/layers3d.py:362-377: per frame w = softmax(q^T k * C^-0.5), h = v w^T) for C = 512 in ONE
 * flash-style pass: q, k, o [frames][hw][512] bf16 (channels-last pixels), vt = V^T [frames][512][ld_vt] (g3_transpose2d_bf16 per frame;
 * vt_frame_stride in elements), hw % 64 == 0. fp32 softmax statistics and accumulation, P rounded to bf16 before P.V like the bf16 reference.
 * Replaces the scores-GEMM + g3_softmax_rows_bf16 + P.V-GEMM sequence of earlier rounds (csrc/attention_d512.hip). */
int g3_spatial_attn_d512_bf16(const void* q, const void* k, const void* vt, int64_t ld_vt, int64_t vt_frame_stride, void* o, int frames,
                              int hw, float softmax_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEN3C_HIP_H */
