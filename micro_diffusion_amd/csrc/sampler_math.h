// The per-element fp32 arithmetic of the EDM sampler (model.py:144-179, dit.py:542-550), shared by the update kernels of edm.hip and the
// measurement-guidance kernels of guide.hip: both form the denoised prediction from these functions, so they give the same bits.
#pragma once
#include "md_common.h"

// Every multiply-add is written as an explicit fma: left to the compiler, the same expression was contracted in one kernel and
// evaluated as multiply, multiply, add in another (it vectorises the two products first), and the two forms of a step must give
// the same bits.
__device__ __forceinline__ float sampler_c_in(float sigma, float sigma_data) {
    return 1.f / sqrtf(fmaf(sigma, sigma, sigma_data * sigma_data));
}
__device__ __forceinline__ float sampler_net_in(float c_in, double x) { return c_in * (float)x; }
__device__ __forceinline__ void heun_coef(double t_in, float sigma_data, float& c_skip, float& c_out) {
    const float sg = (float)t_in;
    const float den = fmaf(sg, sg, sigma_data * sigma_data);
    c_skip = sigma_data * sigma_data / den;
    c_out = sg * sigma_data / sqrtf(den);
}
__device__ __forceinline__ float cfg_combine(float fc, float fu, float cfg) { return fmaf(cfg, fc - fu, fu); }
// D = c_skip * float(x_in) + c_out * F in fp32 (model.py:177), widened to the fp64 of the state.
__device__ __forceinline__ float sampler_denoised_f32(double xi, float f, float c_skip, float c_out) {
    return fmaf(c_skip, (float)xi, c_out * f);
}
__device__ __forceinline__ double sampler_denoised(double xi, float f, float c_skip, float c_out) {
    return (double)sampler_denoised_f32(xi, f, c_skip, c_out);
}
