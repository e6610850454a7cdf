// The MXFP8 quantiser arithmetic (OCP MX v1.0, e4m3fn elements + one E8M0 scale per 32 elements; format notes at the top of gemm_mx.hip).
// ONE copy for the stand-alone pass (gemm_mx.hip, quant_mxfp8_kernel) and for the producers that quantise their own output in registers
// (norm_rope.hip: LayerNorm + modulate; gemm_mx.hip: the MXFP8 GEMM with MXFP8 output), so that all of them are bitwise equal by construction.
#pragma once
#include "common.hpp"

// OCP e4m3fn bits of RNE(y), |y| <= 448 (sign kept, so a negative value that rounds to zero gives 0x80). With e = max(floor(log2|y|), -6)
// the step is 2^(e-3) and q = |y| / 2^(e-3) in [0, 16]; bits = 8 (e + 6) + q covers normals (q >= 8), subnormals (e = -6, q < 8) and the carry
// of q = 16 into the next exponent in one expression.
G3_DEVICE uint32_t e4m3_rne(float y) {
    const uint32_t b = __float_as_uint(y);
    int e = (int)((b >> 23) & 0xff) - 127;
    e = e < -6 ? -6 : e;
    const float q = rintf(ldexpf(fabsf(y), 3 - e));
    return ((b >> 24) & 0x80) | (uint32_t)((e + 6) * 8 + (int)q);
}

// Non-finite rule ("Non-finite inputs"; both formats): a block that holds a NaN or an infinity leaves as the E8M0 NaN - scale byte 0xFF, X = MX_X_NAN -
// with zero codes, which the scaled matrix core turns into NaN in every output that consumes the block, as a bf16 linear would carry it.
constexpr int MX_X_NAN = 128;
constexpr uint32_t MX_INF_BITS = 0x7f800000u;

// The block amax of a lane quad as the BIT PATTERN of |x|, through the quad's two shuffles. For non-negative floats the unsigned order of the
// bits is the order of the values, so on finite data this is fmaxf's amax bit for bit; an infinity or a NaN (which fmaxf would drop) is the
// largest pattern of all and comes out >= MX_INF_BITS. A dead lane passes zeros and leaves its quad's amax alone.
G3_DEVICE uint32_t mx_quad_amax_bits(const float (&f)[8]) {
    uint32_t m = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) m = max(m, __float_as_uint(f[e]) & 0x7fffffffu);
    m = max(m, (uint32_t)__shfl_xor((int)m, 1, 64));
    m = max(m, (uint32_t)__shfl_xor((int)m, 2, 64));
    return m;
}

// Shared exponent X of a block (E8M0 byte = X + 127). amax is a finite non-negative bf16 value widened to fp32.
G3_DEVICE int mx_block_exponent(float amax) {
    if (amax == 0.0f) return 0;
    int X = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - 8;  // subnormal amax: exponent field 0 -> X far below -127, clamped
    return X < -127 ? -127 : (X > 127 ? 127 : X);
}

// A producer's lane holds 8 consecutive elements f[0..7] (bf16 values widened to fp32) of a 32-element block whose other 24 sit in the lanes
// lane ^ 1, lane ^ 2, lane ^ 3: the block amax over the lane quad, then this lane's 8 e4m3 bytes (returned) and the block's exponent X (the quad's
// first lane stores the byte X + 127; a block with a NaN or an infinity: X = MX_X_NAN, zero codes). The arithmetic of quant_mxfp8_kernel,
// statement for statement. EVERY lane of the wave has to call this (the shuffles); a lane without data passes zeros, which leaves its quad's amax alone.
G3_DEVICE u32x2 mx_quant_quad(const float (&f)[8], int& X) {
    const uint32_t abits = mx_quad_amax_bits(f);
    const float amax = __uint_as_float(abits);
    const bool finite = abits < MX_INF_BITS;
    X = finite ? mx_block_exponent(amax) : MX_X_NAN;
    u32x2 o = {0u, 0u};
    if (finite && amax != 0.0f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float y = fminf(fmaxf(ldexpf(f[e], -X), -448.0f), 448.0f);
            o[e >> 2] |= e4m3_rne(y) << (8 * (e & 3));
        }
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------------
// MXFP6 (OCP MX v1.0, e2m3 elements: 1 sign, 2 exponent, 3 mantissa bits, bias 1; subnormals m/8, normals 2^(e-1)(1 + m/8), maximum 7.5, no Inf or
// NaN codes; format notes in the MXFP6 part of gemm_mx.hip). The e4m3 routines above are left as they are.
// ---------------------------------------------------------------------------------------------------------------

// e2m3 code of RNE(y), |y| <= 7.5 (the caller clamps, so 7.75 never reaches the tie to 8). With e = max(floor(log2|y|), 0) the step is 2^(e-3) and
// q = |y| / 2^(e-3) in [0, 16]; code = 8 e + q covers subnormals (e = 0, q < 8), normals and the carry of q = 16 into the next exponent. The
// sign bit (0x20) is the input's, so a negative value that rounds to zero gives 0x20 (-0), as e4m3_rne gives 0x80.
G3_DEVICE uint32_t e2m3_rne(float y) {
    const uint32_t b = __float_as_uint(y);
    int e = (int)((b >> 23) & 0xff) - 127;
    e = e < 0 ? 0 : e;
    const float q = rintf(ldexpf(fabsf(y), 3 - e));
    return ((b >> 26) & 0x20) | (uint32_t)(e * 8 + (int)q);
}

// Shared exponent X of an MXFP6 block: floor(log2(amax)) - 2, so amax / 2^X lies in [4, 8) (E8M0 byte = X + 127).
G3_DEVICE int mx6_block_exponent(float amax) {
    if (amax == 0.0f) return 0;
    int X = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - 2;  // subnormal amax: exponent field 0 -> X = -129, clamped
    return X < -127 ? -127 : (X > 127 ? 127 : X);
}

// 8 consecutive elements of a block (already divided by 2^X) as 48 bits: element i at bits [6 i, 6 i + 6). lo = bits 0..31, hi = bits 32..47.
G3_DEVICE void mx6_pack8(const float (&y)[8], uint32_t& lo, uint32_t& hi) {
    uint64_t v = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) v |= (uint64_t)e2m3_rne(fminf(fmaxf(y[e], -7.5f), 7.5f)) << (6 * e);
    lo = (uint32_t)v;
    hi = (uint32_t)(v >> 32);
}

// The lane quad j = lane & 3 holds the four 48-bit pieces of one 24-byte block. Returns the 8 bytes [8 j, 8 j + 8) of the block for j < 3
// (lane 3 of the quad stores nothing), gathered from this lane and its right neighbour. EVERY lane of the wave has to call this (the shuffles).
G3_DEVICE u32x2 mx6_gather_quad(uint32_t lo, uint32_t hi, int j) {
    const uint32_t nlo = (uint32_t)__shfl_down((int)lo, 1, 64);
    const uint32_t nhi = (uint32_t)__shfl_down((int)hi, 1, 64);
    u32x2 o;
    if (j == 0) {         // bytes 0..7: own 48 bits, then the neighbour's low 16
        o[0] = lo;
        o[1] = hi | (nlo << 16);
    } else if (j == 1) {  // bytes 8..15: own bits 16..47, then the neighbour's low 32
        o[0] = (lo >> 16) | (hi << 16);
        o[1] = nlo;
    } else {              // j == 2, bytes 16..23: own bits 32..47, then the neighbour's 48
        o[0] = hi | (nlo << 16);
        o[1] = (nlo >> 16) | (nhi << 16);
    }
    return o;
}
