// Image-conditioned sampling (SDEdit image-to-image, inpainting, RePaint resampling; no reference counterpart: the reference's
// sampler starts from pure noise).  One kernel on the fp64 sampler state [B, C, HW], between network evaluations:
//   k = noise ? fma(sigma, noise, x0) : x0        the known latents x0, brought to the noise level sigma of the state
//   x = fma(m, x, (1 - m) * k)                    m = mask[b or 0, i] in [0, 1], broadcast over the channels: 1 = generated, 0 = known
// It is the SDEdit initialisation (mask == NULL: x = k everywhere), the blend at the start of every inpainting step and the final
// paste (noise == NULL, sigma = 0).  The multiply-adds are explicit fmas, as in edm.hip (see the comment at its sampler helpers): the
// bits must not depend on how the compiler contracts.  With this form m = 1 returns x and m = 0 returns k, exactly.
// The state is small (2 MiB at B = 64, 4 x 32 x 32): the launch is the cost, so nothing here goes beyond coalesced 16-byte accesses.
#include "md_common.h"
#include "../../include/microdit_hip.h"

#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(2))) double f64x2;

// The grid helper of edm.hip (its egrid), for V elements per lane.
inline int blend_grid(int64_t work) {
    int64_t g = (work + 255) / 256;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (int)g;
}

__device__ __forceinline__ double blend_element(double x, double x0, double noise, double m, double sigma, bool has_noise) {
    const double k = has_noise ? fma(sigma, noise, x0) : x0;
    return fma(m, x, (1.0 - m) * k);
}

// V = 2: HW is even, so the two elements of a lane share (b, c) and are neighbours in the mask row; every fp64 base is 16-byte aligned.
// mask and noise are workgroup-uniform pointers: the branches on them do not diverge.  Every element is loaded before it is stored, so
// x may alias noise (the SDEdit initialisation runs in place on an fp64 copy of the caller's unit noise).  Without a mask x is not
// read at all: an uninitialised state (NaN, Inf) cannot reach the result through 0 * x.
template <int V>
__global__ __launch_bounds__(256) void blend_known_kernel(double* x, const double* x0, const double* noise, const float* mask, int64_t total,
                                                          int32_t C, int64_t HW, int32_t mask_B, double sigma) {
    const int64_t items = total / V;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
        const int64_t e = it * V;
        const float* mrow = nullptr;
        if (mask) {
            const int64_t bc = e / HW;
            mrow = mask + (mask_B == 1 ? 0 : bc / C) * HW + (e - bc * HW);
        }
        if (V == 2) {
            const f64x2 k0 = *reinterpret_cast<const f64x2*>(x0 + e);
            const f64x2 nz = noise ? *reinterpret_cast<const f64x2*>(noise + e) : f64x2{0.0, 0.0};
            f64x2 out;
            if (mask) {
                const f64x2 xs = *reinterpret_cast<const f64x2*>(x + e);
                out.x = blend_element(xs.x, k0.x, nz.x, (double)mrow[0], sigma, noise != nullptr);
                out.y = blend_element(xs.y, k0.y, nz.y, (double)mrow[1], sigma, noise != nullptr);
            } else {
                out.x = noise ? fma(sigma, nz.x, k0.x) : k0.x;
                out.y = noise ? fma(sigma, nz.y, k0.y) : k0.y;
            }
            *reinterpret_cast<f64x2*>(x + e) = out;
        } else {
            const double k0 = x0[e], nz = noise ? noise[e] : 0.0;
            x[e] = mask ? blend_element(x[e], k0, nz, (double)mrow[0], sigma, noise != nullptr) : (noise ? fma(sigma, nz, k0) : k0);
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int md_edm_blend_known(double* x, const double* x0, const double* noise, const float* mask, int64_t B, int32_t C, int64_t HW,
                                  int32_t mask_B, double sigma, hipStream_t st) {
    if (!x || !x0 || B <= 0 || C <= 0 || HW <= 0) return MD_BAD_ARG;
    if (mask && mask_B != 1 && (int64_t)mask_B != B) return MD_BAD_ARG;
    if (!(sigma >= 0.0) || !isfinite(sigma)) return MD_BAD_ARG;          // negative, NaN or infinite
    if (!noise && sigma != 0.0) return MD_BAD_ARG;
    const int64_t total = B * C * HW;
    if (HW % 2 == 0 && aligned16(x) && aligned16(x0) && (!noise || aligned16(noise))) {
        hipLaunchKernelGGL(blend_known_kernel<2>, dim3(blend_grid(total / 2)), dim3(256), 0, st, x, x0, noise, mask, total, C, HW, mask_B, sigma);
    } else {
        hipLaunchKernelGGL(blend_known_kernel<1>, dim3(blend_grid(total)), dim3(256), 0, st, x, x0, noise, mask, total, C, HW, mask_B, sigma);
    }
    MD_LAUNCH_CHECK();
    return 0;
}
