// Head-parallel context parallelism (parallel.py, schedule "head_parallel"): the layout passes around the two all-to-all exchanges.
//
//   scatter: x [rows][ld_in] (q, k, v column views of the fused QKV buffer; heads of 128 bf16) -> x_out [n_dest][rows][Hg*128] contiguous, the
//            send layout of a single-tensor all-to-all: destination d gets heads d * (H / n_dest) + head0 .. + Hg of every row.
//   gather:  in [n_src][rows][Hg*128] contiguous (the receive layout of the returning all-to-all) -> columns (s * (H / n_src) + head0) * 128 .. of
//            out [rows][ld_out].
//
// Both are pure bandwidth passes: one 16-byte load and one 16-byte store per lane and tensor, the contiguous side addressed by the loop index
// itself. Offsets are 64-bit throughout (rows * ld of the full-size QKV buffer stays below 2^31 elements, a gathered buffer need not).
#include "common.hpp"

#define CPX_THREADS 256
#define CPX_MAX_BLOCKS (256 * 16)  // grid-stride beyond 16 workgroups per CU

// grid (x: chunk blocks of one destination's [rows][W16] plane, y: destination). W16 = 16-byte chunks per packed row = Hg * 16.
__global__ __launch_bounds__(CPX_THREADS) void cp_scatter_heads_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                                        const bf16_t* __restrict__ v, int64_t ld_in, bf16_t* __restrict__ q_out,
                                                                        bf16_t* __restrict__ k_out, bf16_t* __restrict__ v_out, int64_t rows, int W16,
                                                                        int64_t dest_col_stride, int64_t col0) {
    const int64_t d = blockIdx.y;
    const int64_t plane = rows * W16;  // chunks per destination
    const int64_t src_col = col0 + d * dest_col_stride;
    for (int64_t i = (int64_t)blockIdx.x * CPX_THREADS + threadIdx.x; i < plane; i += (int64_t)gridDim.x * CPX_THREADS) {
        const int64_t r = i / W16;
        const int64_t c = i - r * W16;
        const int64_t src = r * ld_in + src_col + c * 8;
        const int64_t dst = (d * plane + i) * 8;
        if (k) store_bf16x8(k_out + dst, load_bf16x8(k + src));
        if (v) store_bf16x8(v_out + dst, load_bf16x8(v + src));
        if (q) store_bf16x8(q_out + dst, load_bf16x8(q + src));
    }
}

__global__ __launch_bounds__(CPX_THREADS) void cp_gather_heads_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int64_t ld_out, int64_t rows,
                                                                       int W16, int64_t src_col_stride, int64_t col0) {
    const int64_t s = blockIdx.y;
    const int64_t plane = rows * W16;
    const int64_t dst_col = col0 + s * src_col_stride;
    for (int64_t i = (int64_t)blockIdx.x * CPX_THREADS + threadIdx.x; i < plane; i += (int64_t)gridDim.x * CPX_THREADS) {
        const int64_t r = i / W16;
        const int64_t c = i - r * W16;
        store_bf16x8(out + r * ld_out + dst_col + c * 8, load_bf16x8(in + (s * plane + i) * 8));
    }
}

// shared refusals: the head split, the row count, the strided side's leading dimension
static int cp_exchange_check(const char* f, int64_t ld, int64_t rows, int H, int n, int head0, int Hg) {
    if (H <= 0 || n <= 0 || n > 65535 || H % n != 0) return g3_set_error(G3_ERR_ARG, "%s: H = %d must be a positive multiple of the rank count %d", f, H, n);
    if (head0 < 0 || Hg <= 0 || head0 + Hg > H / n)
        return g3_set_error(G3_ERR_ARG, "%s: heads [%d, %d) are not inside a rank's %d heads", f, head0, head0 + Hg, H / n);
    if (rows <= 0) return g3_set_error(G3_ERR_ARG, "%s: rows must be positive", f);
    if (ld < (int64_t)H * 128 || (ld & 7)) return g3_set_error(G3_ERR_ARG, "%s: leading dim %lld must be a multiple of 8 and at least H * 128 = %d", f, (long long)ld, H * 128);
    return G3_OK;
}

static unsigned cp_exchange_blocks(int64_t plane) {
    const int64_t nblk = (plane + CPX_THREADS - 1) / CPX_THREADS;
    return (unsigned)(nblk < CPX_MAX_BLOCKS ? nblk : CPX_MAX_BLOCKS);
}

extern "C" int g3_cp_scatter_heads_bf16(const void* q, const void* k, const void* v, int64_t ld_in, void* q_out, void* k_out, void* v_out, int64_t rows,
                                        int H, int n_dest, int head0, int Hg, void* stream) {
    const char* f = "g3_cp_scatter_heads_bf16";
    if (int rc = cp_exchange_check(f, ld_in, rows, H, n_dest, head0, Hg)) return rc;
    if (!q && !k && !v) return g3_set_error(G3_ERR_ARG, "%s: q, k and v are all NULL", f);
    if ((q && !q_out) || (k && !k_out) || (v && !v_out)) return g3_set_error(G3_ERR_ARG, "%s: an input without its output", f);
    if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) || ((q ? (uintptr_t)q_out : 0) | (k ? (uintptr_t)k_out : 0) | (v ? (uintptr_t)v_out : 0)) & 15)
        return g3_set_error(G3_ERR_ARG, "%s: pointers must be 16-byte aligned", f);
    const int W16 = Hg * 16;
    dim3 grid(cp_exchange_blocks(rows * W16), (unsigned)n_dest);
    hipLaunchKernelGGL(cp_scatter_heads_kernel, grid, dim3(CPX_THREADS), 0, (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld_in,
                       (bf16_t*)q_out, (bf16_t*)k_out, (bf16_t*)v_out, rows, W16, (int64_t)(H / n_dest) * 128, (int64_t)head0 * 128);
    return g3_check_launch(f);
}

extern "C" int g3_cp_gather_heads_bf16(const void* in, void* out, int64_t ld_out, int64_t rows, int H, int n_src, int head0, int Hg, void* stream) {
    const char* f = "g3_cp_gather_heads_bf16";
    if (int rc = cp_exchange_check(f, ld_out, rows, H, n_src, head0, Hg)) return rc;
    if (!in || !out) return g3_set_error(G3_ERR_ARG, "%s: null operand", f);
    if (((uintptr_t)in | (uintptr_t)out) & 15) return g3_set_error(G3_ERR_ARG, "%s: pointers must be 16-byte aligned", f);
    const int W16 = Hg * 16;
    dim3 grid(cp_exchange_blocks(rows * W16), (unsigned)n_src);
    hipLaunchKernelGGL(cp_gather_heads_kernel, grid, dim3(CPX_THREADS), 0, (hipStream_t)stream, (const bf16_t*)in, (bf16_t*)out, ld_out, rows, W16,
                       (int64_t)(H / n_src) * 128, (int64_t)head0 * 128);
    return g3_check_launch(f);
}
