// Step cache: the backbone's contribution to the residual stream, kept from one sampler evaluation and added back in
// the next, and the distance probe of the adaptive policy.
//
//   md_residual_delta      delta = bf16(f32(x_out) - f32(x_in)); the apply step is md_add_bf16(x_in', delta, x)
//   md_step_probe          per workgroup, fp64 partial sums of |x - ref| and |ref| over its slice of one sample; ref <- x in the same pass
//   md_step_probe_finish   rel[b] = f32(sum |x - ref| / sum |ref|) (+inf for a zero reference), rel_max = max_b rel[b]
//
// The probe's sums are fp64 in an order that is a function of (B, per_sample) alone: a thread adds its 16-byte chunks in ascending
// order, the 64 lanes of a wave through a fixed shuffle tree, the four waves in ascending order through LDS, and one thread per sample
// adds that sample's workgroup partials in ascending order.  No atomics, nothing returns to the host, no workgroup straddles two samples.
#include "md_common.h"
#include "../../include/microdit_hip.h"
#include <math.h>

namespace {

constexpr int SC_THREADS = 256;
constexpr int64_t SC_DELTA_MAX_BLOCKS = MD_STEP_DELTA_MAX_BLOCKS;   // 2048 x 256 threads: eight waves on every SIMD of 256 CUs, once
constexpr int64_t SC_PROBE_CHUNKS = MD_STEP_PROBE_CHUNKS;           // 16-byte chunks of one workgroup: four per thread
constexpr int64_t SC_WS_HEADER = 2;                                 // ws[0] = workgroups per sample (ws[1] unused), then [B][groups][2]

__global__ __launch_bounds__(SC_THREADS) void residual_delta_kernel(const bf16* __restrict__ x_out, const bf16* __restrict__ x_in,
                                                                    bf16* __restrict__ delta, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; i < n8; i += (int64_t)gridDim.x * SC_THREADS) {
        const bf16x8 u = ld_bf16x8(x_out + i * 8), v = ld_bf16x8(x_in + i * 8);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f2bf(bf2f(u[e]) - bf2f(v[e]));
        st_bf16x8(delta + i * 8, o);
    }
}

// Sum of one double per lane over the 64 lanes of a wave, fixed tree; lane 0 holds the total.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// grid = (workgroups per sample, B).  Workgroup (c, b) takes the chunks [c * SC_PROBE_CHUNKS, (c + 1) * SC_PROBE_CHUNKS) of sample b,
// thread t the chunks t, t + 256, ... of them (every load of an iteration is one contiguous 4 KB wave access).
__global__ __launch_bounds__(SC_THREADS) void step_probe_kernel(const bf16* __restrict__ x, bf16* __restrict__ ref, int64_t per8,
                                                                double* __restrict__ ws) {
    __shared__ double part[2][SC_THREADS / MD_WAVE];
    const int64_t base = (int64_t)blockIdx.y * per8;
    const int64_t c0 = (int64_t)blockIdx.x * SC_PROBE_CHUNKS;
    const int64_t c1 = c0 + SC_PROBE_CHUNKS < per8 ? c0 + SC_PROBE_CHUNKS : per8;
    double sd = 0.0, sr = 0.0;
    for (int64_t c = c0 + threadIdx.x; c < c1; c += SC_THREADS) {
        const int64_t off = (base + c) * 8;
        const bf16x8 u = ld_bf16x8(x + off), r = ld_bf16x8(ref + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float rf = bf2f(r[e]);
            sd += (double)fabsf(bf2f(u[e]) - rf);
            sr += (double)fabsf(rf);
        }
        st_bf16x8(ref + off, u);
    }
    sd = wave_sum_f64(sd);
    sr = wave_sum_f64(sr);
    const int lane = threadIdx.x & (MD_WAVE - 1), wave = threadIdx.x / MD_WAVE;
    if (lane == 0) {
        part[0][wave] = sd;
        part[1][wave] = sr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0 && blockIdx.y == 0) ws[0] = (double)gridDim.x;    // header: workgroups per sample, read by the finish
        double* out = ws + SC_WS_HEADER + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
        out[0] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
        out[1] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    }
}

// Larger of two ratios; a NaN wins over every number, so the result does not depend on the order.
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

// One workgroup: thread b, b + 256, ... adds the partials of its samples in ascending order; the maximum goes through a fixed LDS tree.
__global__ __launch_bounds__(SC_THREADS) void step_probe_finish_kernel(const double* __restrict__ ws, int64_t B, float* __restrict__ rel,
                                                                       float* __restrict__ rel_max) {
    __shared__ float sh[SC_THREADS];
    const int64_t groups = (int64_t)ws[0];
    float m = 0.f;                                   // every ratio is >= 0 (or NaN)
    for (int64_t b = threadIdx.x; b < B; b += SC_THREADS) {
        const double* p = ws + SC_WS_HEADER + 2 * b * groups;
        double sd = 0.0, sr = 0.0;
        for (int64_t g = 0; g < groups; ++g) {
            sd += p[2 * g];
            sr += p[2 * g + 1];
        }
        const float r = sr > 0.0 ? (float)(sd / sr) : (sr == 0.0 ? INFINITY : (float)sr);   // (sr is NaN: the ratio is NaN)
        rel[b] = r;
        m = max_nan(r, m);
    }
    sh[threadIdx.x] = m;
    __syncthreads();
#pragma unroll
    for (int o = SC_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = max_nan(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) rel_max[0] = sh[0];
}

inline int64_t probe_groups(int64_t per_sample) { return (per_sample / 8 + SC_PROBE_CHUNKS - 1) / SC_PROBE_CHUNKS; }

inline bool probe_shape_ok(int64_t B, int64_t per_sample) {
    // grid.y carries the sample: the hardware limit of that dimension
    return B >= 1 && B <= 65535 && per_sample >= 8 && per_sample % 8 == 0 && probe_groups(per_sample) <= 0x7fffffff;
}

inline bool overlap(const void* a, const void* b, int64_t bytes) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p < q + (uintptr_t)bytes && q < p + (uintptr_t)bytes;
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int md_residual_delta(const void* x_out, const void* x_in, void* delta, int64_t n, hipStream_t stream) {
    if (!x_out || !x_in || !delta || n <= 0 || n % 8) return MD_BAD_ARG;
    if (!aligned16(x_out) || !aligned16(x_in) || !aligned16(delta)) return MD_BAD_ARG;
    if (overlap(delta, x_out, 2 * n) || overlap(delta, x_in, 2 * n)) return MD_BAD_ARG;
    const int64_t n8 = n / 8;
    int64_t grid = (n8 + SC_THREADS - 1) / SC_THREADS;
    if (grid > SC_DELTA_MAX_BLOCKS) grid = SC_DELTA_MAX_BLOCKS;
    hipLaunchKernelGGL(residual_delta_kernel, dim3((unsigned)grid), dim3(SC_THREADS), 0, stream, reinterpret_cast<const bf16*>(x_out),
                       reinterpret_cast<const bf16*>(x_in), reinterpret_cast<bf16*>(delta), n8);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_step_probe_ws_doubles(int64_t B, int64_t per_sample, int64_t* out) {
    if (!out || !probe_shape_ok(B, per_sample)) return MD_BAD_ARG;
    *out = SC_WS_HEADER + 2 * B * probe_groups(per_sample);
    return 0;
}

extern "C" int md_step_probe(const void* x, void* ref, int64_t B, int64_t per_sample, double* ws, hipStream_t stream) {
    if (!x || !ref || !ws || !probe_shape_ok(B, per_sample)) return MD_BAD_ARG;
    if (!aligned16(x) || !aligned16(ref) || overlap(x, ref, 2 * B * per_sample)) return MD_BAD_ARG;
    hipLaunchKernelGGL(step_probe_kernel, dim3((unsigned)probe_groups(per_sample), (unsigned)B), dim3(SC_THREADS), 0, stream,
                       reinterpret_cast<const bf16*>(x), reinterpret_cast<bf16*>(ref), per_sample / 8, ws);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_step_probe_finish(const double* ws, int64_t B, float* rel, float* rel_max, hipStream_t stream) {
    if (!ws || !rel || !rel_max || B < 1 || B > 65535) return MD_BAD_ARG;
    hipLaunchKernelGGL(step_probe_finish_kernel, dim3(1), dim3(SC_THREADS), 0, stream, ws, B, rel, rel_max);
    MD_LAUNCH_CHECK();
    return 0;
}
