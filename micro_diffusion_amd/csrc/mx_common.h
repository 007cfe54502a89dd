// OCP MX (MXFP8) quantisation of one block of 32 values, shared by mx_quant.hip and the MX-writing SwiGLU.
//
//   amax = largest magnitude of the block;  X = clamp(floor(log2 amax) - 8, -127, 127);  scale byte = X + 127 (e8m0)
//   element = e4m3fn_rne(clamp(v * 2^-X, -448, 448))
//
// Everything that decides a bit is integer arithmetic on the bf16 / fp32 encodings plus two exact fp32 operations (a multiplication by a
// power of two, one addition that rounds to nearest even), so the functions give the same bits on the host and on the device and do
// not depend on how a hardware conversion instruction treats overflow.  Inputs are finite.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MX_FN __host__ __device__ __forceinline__
#else
#define MX_FN inline
#endif

MX_FN uint32_t mx_f32_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
MX_FN float mx_bits_f32(uint32_t u) {
    float v;
    memcpy(&v, &u, 4);
    return v;
}

// Scale byte of a block from the largest |bf16 encoding| (sign bit cleared) of its elements.  floor(log2 amax) is the exponent field
// minus 127 (a bf16 subnormal or zero has field 0: X clamps to -127 either way), so X + 127 = max(field - 8, 0).
MX_FN uint32_t mx_scale_byte(uint32_t amax_bf16_bits) {
    const int field = (int)(amax_bf16_bits >> 7);
    return field > 8 ? (uint32_t)(field - 8) : 0u;
}

// 2^-X as fp32 for scale byte b = X + 127: exponent field 254 - b, always a normal number (b <= 246).
MX_FN float mx_inv_scale(uint32_t scale_byte) { return mx_bits_f32((254u - scale_byte) << 23); }

// e4m3fn (OCP: bias 7, no infinity, 0x7f = NaN, largest finite 448 = 0x7e), round to nearest even, of a finite fp32 value; magnitudes above
// 448 saturate.
MX_FN uint32_t mx_e4m3_rne(float v) {
    const uint32_t u = mx_f32_bits(v);
    const uint32_t sign = (u >> 24) & 0x80u;
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x43e00000u) a = 0x43e00000u;                      // clamp to 448
    if (a < 0x3c800000u) {                                     // below 2^-6: subnormal of quantum 2^-9 (8 rounds up into 0x08 = 2^-6)
        const float r = mx_bits_f32(a) * 512.f + 8388608.f;    // the sum has quantum 1: the addition rounds to nearest even
        return sign | (mx_f32_bits(r) & 0xfu);
    }
    a += 0x7ffffu + ((a >> 20) & 1u);                           // round the 23-bit mantissa to 3 bits, ties to even
    return sign | ((a >> 20) - (120u << 3));                   // rebias 127 -> 7
}
