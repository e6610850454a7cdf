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

// Shared exponent X of a block (E8M0 byte = X + 127). amax is a finite non-negative bf16 value widened to fp32.
G3_DEVICE int mx_block_exponent(float amax) {
    if (amax == 0.0f) return 0;
    int X = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - 8;  // subnormal amax: exponent field 0 -> X far below -127, clamped
    return X < -127 ? -127 : (X > 127 ? 127 : X);
}

// A producer's lane holds 8 consecutive elements f[0..7] (bf16 values widened to fp32) of a 32-element block whose other 24 sit in the lanes
// lane ^ 1, lane ^ 2, lane ^ 3: the block amax over the lane quad, then this lane's 8 e4m3 bytes (returned) and the block's exponent X (the quad's
// first lane stores the byte X + 127). The arithmetic of quant_mxfp8_kernel, statement for statement. EVERY lane of the wave has to call this
// (the shuffles); a lane without data passes zeros, which leaves its quad's amax alone.
G3_DEVICE u32x2 mx_quant_quad(const float (&f)[8], int& X) {
    float amax = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
    amax = fmaxf(amax, wave_xor_f32(amax, 1));
    amax = fmaxf(amax, wave_xor_f32(amax, 2));
    X = mx_block_exponent(amax);
    u32x2 o = {0u, 0u};
    if (amax != 0.0f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float y = fminf(fmaxf(ldexpf(f[e], -X), -448.0f), 448.0f);
            o[e >> 2] |= e4m3_rne(y) << (8 * (e & 3));
        }
    }
    return o;
}
