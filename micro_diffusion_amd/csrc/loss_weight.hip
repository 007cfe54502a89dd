// Learned per-noise-level loss weighting (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models",
// section 2.2, uncertainty-based loss weighting; no reference counterpart: the reference trains with the fixed EDM weight alone).
//   feat[b, c] = sqrt(2) * cosf(cnoise[b] * freq[c] + phase[c])     random Fourier features of c_noise = ln(sigma) / 4
//   u[b]       = sum_c w[c] * feat[b, c]                            the learned log-variance of the loss at that noise level
//   inv[b]     = expf(-u[b])                                        the per-sample factor md_edm_loss_train_weighted puts on dL/dF
//   objective  = (1 / B) sum_b (L[b] * inv[b] + u[b])
//   dw[c]     += sum_b gscale / B * (1 - inv[b] * L[b]) * feat[b, c]
// All fp32, no float atomic, every sum in an order that is a function of the shape alone (the policy of md_tensor_stats_* and
// md_loss_sigma_hist): two calls on the same inputs give the same bits.  The features are recomputed in the backward (C cosf per
// sample) rather than stored: B * C floats per microbatch would outlive the whole DiT backward for nothing.
#include "md_common.h"
#include "../../include/microdit_hip.h"

namespace {

constexpr float LV_SQRT2 = 1.41421356237309504880f;

__device__ __forceinline__ float logvar_feat(float cn, float freq, float phase) { return LV_SQRT2 * cosf(fmaf(cn, freq, phase)); }

// One wave per sample (four samples per workgroup): lane l adds channels l, l + 64, ... in ascending order, then the wave reduction.
__global__ __launch_bounds__(256) void logvar_fwd_kernel(const float* cnoise, const float* freq, const float* phase, const float* w,
                                                         float* u, float* inv, int64_t B, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                      // wave-uniform: a whole wave leaves, no barrier follows
    const float cn = cnoise[b];
    float acc = 0.f;
    for (int c = lane; c < C; c += 64) acc = fmaf(w[c], logvar_feat(cn, freq[c], phase[c]), acc);
    acc = wave_sum(acc);
    if (lane == 0) {
        u[b] = acc;
        inv[b] = expf(-acc);
    }
}

// One workgroup.  Samples go through LDS in chunks of 256: thread t forms du and the objective term of sample base + t, then thread
// c < C walks the chunk in index order, dw[c] <- fma(du[b], feat[b, c], dw[c]) -- one chain per channel that starts from the value
// already in dw, so for every c the samples are added in index order whatever B is.  The objective terms are added lane-strided by
// wave 0 (lane j: samples j, j + 64, ... in ascending order) and closed by the wave reduction, like edm_loss_finish_kernel.
// A non-finite L[b] makes du[b] non-finite and reaches dw: not masked, the step guard sees it in the gradient norm of the step.
__global__ __launch_bounds__(256) void logvar_bwd_kernel(const float* cnoise, const float* freq, const float* phase, const float* u,
                                                         const float* loss, float gscale, float* dw, float* obj_mean, float* obj_accum,
                                                         float accum_weight, int64_t B, int C) {
    __shared__ float s_du[256], s_cn[256], s_obj[256];
    const int tid = threadIdx.x;
    const float gfac = gscale / (float)B;
    const bool own = tid < C;
    const float fr = own ? freq[tid] : 0.f, ph = own ? phase[tid] : 0.f;
    float acc = own ? dw[tid] : 0.f;
    float obj = 0.f;
    for (int64_t base = 0; base < B; base += 256) {
        const int n = (int)(B - base < 256 ? B - base : 256);
        if (tid < n) {
            const float ub = u[base + tid], l = loss[base + tid];
            const float iv = expf(-ub);
            s_du[tid] = gfac * fmaf(-iv, l, 1.f);
            s_cn[tid] = cnoise[base + tid];
            s_obj[tid] = fmaf(l, iv, ub);
        }
        __syncthreads();
        if (own)
            for (int i = 0; i < n; ++i) acc = fmaf(s_du[i], logvar_feat(s_cn[i], fr, ph), acc);
        if (tid < 64)
            for (int i = tid; i < n; i += 64) obj += s_obj[i];
        __syncthreads();                                     // the next chunk rewrites the three arrays
    }
    if (own) dw[tid] = acc;
    if (tid < 64) {                                          // wave 0, all 64 lanes
        obj = wave_sum(obj);
        if (tid == 0) {
            const float m = obj / (float)B;
            *obj_mean = m;
            if (obj_accum) *obj_accum += accum_weight * m;
        }
    }
}

inline bool logvar_channels_ok(int32_t C) { return C >= 64 && C <= 256 && C % 64 == 0; }

}  // namespace

extern "C" int md_logvar_fwd(const float* cnoise, const float* freq, const float* phase, const float* w, float* u, float* inv,
                             int64_t B, int32_t C, hipStream_t st) {
    if (!cnoise || !freq || !phase || !w || !u || !inv || B < 1 || !logvar_channels_ok(C)) return MD_BAD_ARG;
    hipLaunchKernelGGL(logvar_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, cnoise, freq, phase, w, u, inv, B, (int)C);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_logvar_bwd(const float* cnoise, const float* freq, const float* phase, const float* u, const float* loss_per_sample,
                             float gscale, float* dw, float* obj_mean, float* obj_accum, float accum_weight, int64_t B, int32_t C,
                             hipStream_t st) {
    if (!cnoise || !freq || !phase || !u || !loss_per_sample || !dw || !obj_mean || B < 1 || !logvar_channels_ok(C)) return MD_BAD_ARG;
    hipLaunchKernelGGL(logvar_bwd_kernel, dim3(1), dim3(256), 0, st, cnoise, freq, phase, u, loss_per_sample, gscale, dw, obj_mean,
                       obj_accum, accum_weight, B, (int)C);
    MD_LAUNCH_CHECK();
    return 0;
}
