// MXFP8 quantisers: bf16 -> e4m3fn elements + one e8m0 scale per 32 consecutive elements along K (mx_common.h).
//
//   md_mx_quant_rows   a bf16 matrix [rows, K], K-contiguous (activations, nn.Linear weights [N, K]) or K-strided (the MoE expert
//                      tensors [E, d, f] / [E, f, d], whose contraction dimension is the strided one), to K-contiguous fp8 [rows, K]
//                      and scales uint8 [rows, K / 32]; batched with strides
//   md_swiglu_fwd_mx   md_swiglu_fwd writing a = silu(h1) * h2 in that form: the bits of md_swiglu_fwd followed by md_mx_quant_rows
//
// Bandwidth-bound; 16-byte pieces on the contiguous side of both the source and the elements; no atomics, one writer per output byte.
#include "md_common.h"
#include "mx_common.h"
#include "../../include/microdit_hip.h"

namespace {

// bf16 pairs are handled on their encodings: a 32-bit word holds elements 2 j (low half) and 2 j + 1 (high half).
__device__ __forceinline__ uint32_t amax_word(uint32_t amax, uint32_t w) {
    const uint32_t lo = w & 0x7fffu, hi = (w >> 16) & 0x7fffu;
    amax = lo > amax ? lo : amax;
    return hi > amax ? hi : amax;
}
__device__ __forceinline__ float bf16_lo(uint32_t w) { return mx_bits_f32(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return mx_bits_f32(w & 0xffff0000u); }
// four elements (two words) -> four fp8 bytes
__device__ __forceinline__ uint32_t quant4(uint32_t w0, uint32_t w1, float inv) {
    return mx_e4m3_rne(bf16_lo(w0) * inv) | (mx_e4m3_rne(bf16_hi(w0) * inv) << 8) | (mx_e4m3_rne(bf16_lo(w1) * inv) << 16) |
           (mx_e4m3_rne(bf16_hi(w1) * inv) << 24);
}

// One block of 32 bf16 values (four 16-byte pieces) -> 32 fp8 bytes (two 16-byte pieces) and the scale byte.
__device__ __forceinline__ uint32_t mx_quant_block(const uint4 (&v)[4], uint4& lo, uint4& hi) {
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) amax = amax_word(amax_word(amax_word(amax_word(amax, v[i].x), v[i].y), v[i].z), v[i].w);
    const uint32_t sb = mx_scale_byte(amax);
    const float inv = mx_inv_scale(sb);
    lo = make_uint4(quant4(v[0].x, v[0].y, inv), quant4(v[0].z, v[0].w, inv), quant4(v[1].x, v[1].y, inv), quant4(v[1].z, v[1].w, inv));
    hi = make_uint4(quant4(v[2].x, v[2].y, inv), quant4(v[2].z, v[2].w, inv), quant4(v[3].x, v[3].y, inv), quant4(v[3].z, v[3].w, inv));
    return sb;
}

// K-contiguous source: one thread per block of 32 (64 contiguous source bytes, neighbouring lanes neighbouring blocks).
__global__ __launch_bounds__(256) void mx_quant_kc_kernel(const bf16* __restrict__ src, int64_t ld, unsigned char* __restrict__ dst, int64_t ldd,
                                                          unsigned char* __restrict__ scales, int64_t lds, int64_t rows, int64_t nkb,
                                                          int64_t sSrc, int64_t sDst, int64_t sScale, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t kb = i % nkb, rr = i / nkb, r = rr % rows, b = rr / rows;
        const bf16* p = src + b * sSrc + r * ld + kb * 32;
        uint4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const uint4*>(p + j * 8);
        uint4 lo, hi;
        const uint32_t sb = mx_quant_block(v, lo, hi);
        unsigned char* q = dst + b * sDst + r * ldd + kb * 32;
        *reinterpret_cast<uint4*>(q) = lo;
        *reinterpret_cast<uint4*>(q + 16) = hi;
        scales[b * sScale + r * lds + kb] = (unsigned char)sb;
    }
}

// K-strided source src[k * ld + r]: one thread per (8 consecutive rows, block of 32 k).  The 32 source rows are read as 16-byte pieces
// (neighbouring lanes neighbouring row groups) twice -- once for the eight maxima, once for the elements, the second time from cache --
// and every row's 32 output bytes leave as two 16-byte pieces.  A ragged last group (rows % 8 != 0) reads its nv < 8 rows one by one.
__device__ __forceinline__ void ld_rows8(uint32_t (&w)[4], const bf16* p, int nv) {
    if (nv == 8) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
        return;
    }
    const unsigned short* q = reinterpret_cast<const unsigned short*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (2 * j < nv ? (uint32_t)q[2 * j] : 0u) | (2 * j + 1 < nv ? (uint32_t)q[2 * j + 1] << 16 : 0u);
}
__global__ __launch_bounds__(256) void mx_quant_ks_kernel(const bf16* __restrict__ src, int64_t ld, unsigned char* __restrict__ dst, int64_t ldd,
                                                          unsigned char* __restrict__ scales, int64_t lds, int64_t rows, int64_t nkb,
                                                          int64_t sSrc, int64_t sDst, int64_t sScale, int64_t total) {
    const int64_t ng = (rows + 7) / 8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t g = i % ng, rr = i / ng, kb = rr % nkb, b = rr / nkb;
        const bf16* p = src + b * sSrc + kb * 32 * ld + g * 8;
        const int nv = rows - g * 8 < 8 ? (int)(rows - g * 8) : 8;
        uint32_t amax[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) amax[e] = 0;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            uint32_t w[4];
            ld_rows8(w, p + k * ld, nv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t lo = w[j] & 0x7fffu, hi = (w[j] >> 16) & 0x7fffu;
                amax[2 * j] = lo > amax[2 * j] ? lo : amax[2 * j];
                amax[2 * j + 1] = hi > amax[2 * j + 1] ? hi : amax[2 * j + 1];
            }
        }
        uint32_t sb[8];
        float inv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sb[e] = mx_scale_byte(amax[e]);
            inv[e] = mx_inv_scale(sb[e]);
            if (e < nv) scales[b * sScale + (g * 8 + e) * lds + kb] = (unsigned char)sb[e];
        }
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {        // 16 k at a time: eight 16-byte output pieces in registers
            uint32_t w[8][4];
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j) w[e][j] = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                uint32_t u[4];
                ld_rows8(u, p + (h * 16 + k) * ld, nv);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    w[2 * j][k >> 2] |= mx_e4m3_rne(bf16_lo(u[j]) * inv[2 * j]) << (8 * (k & 3));
                    w[2 * j + 1][k >> 2] |= mx_e4m3_rne(bf16_hi(u[j]) * inv[2 * j + 1]) << (8 * (k & 3));
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < nv) *reinterpret_cast<uint4*>(dst + b * sDst + (g * 8 + e) * ldd + kb * 32 + h * 16) = make_uint4(w[e][0], w[e][1], w[e][2], w[e][3]);
        }
    }
}

__device__ __forceinline__ void swiglu_fwd8(const bf16x8& h1, const bf16x8& h2, bf16x8& o) {   // the arithmetic of md_swiglu_fwd
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(bf2f(f2bf(silu_f(bf2f(h1[e])))) * bf2f(h2[e]));
}

__global__ __launch_bounds__(256) void swiglu_fwd_mx_kernel(const bf16* __restrict__ h12, int64_t ldh, unsigned char* __restrict__ dst,
                                                            int64_t ldd, unsigned char* __restrict__ scales, int64_t lds, int64_t f,
                                                            int64_t nkb, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t kb = i % nkb, r = i / nkb;
        const bf16* p = h12 + r * ldh + kb * 32;
        bf16x8 h1[4], h2[4];
        uint4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h1[j] = ld_bf16x8(p + j * 8);
            h2[j] = ld_bf16x8(p + f + j * 8);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            U128 t;
            swiglu_fwd8(h1[j], h2[j], t.h);
            v[j] = t.u;
        }
        uint4 lo, hi;
        const uint32_t sb = mx_quant_block(v, lo, hi);
        unsigned char* q = dst + r * ldd + kb * 32;
        *reinterpret_cast<uint4*>(q) = lo;
        *reinterpret_cast<uint4*>(q + 16) = hi;
        scales[r * lds + kb] = (unsigned char)sb;
    }
}

inline unsigned mx_grid(int64_t items) {
    int64_t g = (items + 255) / 256;
    if (g > 16384) g = 16384;
    return (unsigned)(g < 1 ? 1 : g);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int md_mx_quant_rows(const void* src, int64_t ld, int32_t src_kcontig, void* dst, int64_t ldd, void* scales, int64_t lds,
                                int64_t rows, int64_t K, int32_t batch, int64_t sSrc, int64_t sDst, int64_t sScale, hipStream_t stream) {
    if (!src || !dst || !scales || rows <= 0 || K <= 0 || K % 32 || batch <= 0 || (src_kcontig != 0 && src_kcontig != 1)) return MD_BAD_ARG;
    if (ld % 8 || ldd % 16 || ldd < K || lds < K / 32 || sSrc % 8 || sDst % 16 || !aligned16(src) || !aligned16(dst)) return MD_BAD_ARG;
    if (ld < (src_kcontig ? K : rows)) return MD_BAD_ARG;
    const int64_t nkb = K / 32;
    if (src_kcontig) {
        const int64_t total = (int64_t)batch * rows * nkb;
        hipLaunchKernelGGL(mx_quant_kc_kernel, dim3(mx_grid(total)), dim3(256), 0, stream, (const bf16*)src, ld, (unsigned char*)dst, ldd,
                           (unsigned char*)scales, lds, rows, nkb, sSrc, sDst, sScale, total);
    } else {
        const int64_t total = (int64_t)batch * ((rows + 7) / 8) * nkb;
        hipLaunchKernelGGL(mx_quant_ks_kernel, dim3(mx_grid(total)), dim3(256), 0, stream, (const bf16*)src, ld, (unsigned char*)dst, ldd,
                           (unsigned char*)scales, lds, rows, nkb, sSrc, sDst, sScale, total);
    }
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_swiglu_fwd_mx(const void* h12, int64_t ldh, void* a, int64_t lda, void* scales, int64_t lds, int64_t M, int64_t f,
                                hipStream_t stream) {
    if (!h12 || !a || !scales || M <= 0 || f <= 0 || f % 32 || ldh % 8 || ldh < 2 * f || lda % 16 || lda < f || lds < f / 32 ||
        !aligned16(h12) || !aligned16(a))
        return MD_BAD_ARG;
    const int64_t nkb = f / 32, total = M * nkb;
    hipLaunchKernelGGL(swiglu_fwd_mx_kernel, dim3(mx_grid(total)), dim3(256), 0, stream, (const bf16*)h12, ldh, (unsigned char*)a, lda,
                       (unsigned char*)scales, lds, f, nkb, total);
    MD_LAUNCH_CHECK();
    return 0;
}
