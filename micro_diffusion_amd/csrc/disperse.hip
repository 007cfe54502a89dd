// Dispersive loss: the pairwise stage between the two skinny GEMMs, and the bounds-checked Gram for batch sizes the
// GEMM family's split-K slices do not take.
//
//   G = Z Z^T (fp32)      D_ij = max(0, G_ii + G_jj - 2 G_ij) / K  (i != j), D_ii = 0      E_ij = exp(-D_ij / tau)
//   S = sum_ij E_ij       L = log(S / B^2)      p_ij = E_ij / S
//   W_aj = p_aj (j != a), W_aa = -sum_{j != a} p_aj          dL/dz_a = 4 / (tau K) * sum_j W_aj z_j
//
// D_ii = 0 makes 0 the largest exponent and S >= B: no max-subtraction pass, S can neither overflow nor vanish.  The squared distance is
// formed in fp64 from the fp32 Gram entries (exact: three fp32 numbers), the exponential is fp32 expf, every sum is fp64 in an order that
// is a function of B alone (per-thread strided partials in ascending order, a fixed LDS tree, rows added in ascending order by one
// workgroup): no atomics, nothing returns to the host, two launches on the same Gram give identical bits.
#include "md_common.h"
#include "../../include/microdit_hip.h"
#include <math.h>

namespace {

constexpr int DP_THREADS = 256;

// Sum of one double per thread of a 256-thread workgroup, fixed tree; every thread returns the total.
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int o = DP_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] = sh[t] + sh[t + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// E_aj and D_aj of one off-diagonal pair: the same instructions in the row-sum pass and in the W' pass, so both see the same bits.
__device__ __forceinline__ float pair_exp(const float* __restrict__ G, int64_t ldg, int64_t a, int64_t j, double na, double inv_k,
                                          float inv_tau, double& d_out) {
    const double nj = (double)G[j * ldg + j];
    double d = na + nj - 2.0 * (double)G[a * ldg + j];
    d = d > 0.0 ? d * inv_k : 0.0;
    d_out = d;
    return expf(-(float)d * inv_tau);
}

// Stage 1: one workgroup per row a -> ws[a] = sum_{j != a} E_aj, ws[B + a] = sum_{j != a} D_aj.
__global__ __launch_bounds__(DP_THREADS) void disperse_rows_kernel(const float* __restrict__ G, int64_t ldg, int64_t B, double inv_k,
                                                                   float inv_tau, double* __restrict__ ws) {
    __shared__ double sh[DP_THREADS];
    const int64_t a = blockIdx.x;
    const double na = (double)G[a * ldg + a];
    double se = 0.0, sd = 0.0;
    for (int64_t j = threadIdx.x; j < B; j += DP_THREADS) {
        if (j == a) continue;
        double d;
        se += (double)pair_exp(G, ldg, a, j, na, inv_k, inv_tau, d);
        sd += d;
    }
    se = block_sum_f64(se, sh);
    sd = block_sum_f64(sd, sh);
    if (threadIdx.x == 0) {
        ws[a] = se;
        ws[B + a] = sd;
    }
}

// Stage 2: one workgroup adds the row sums in a fixed order -> result block {L, mean off-diagonal D, mean off-diagonal p B^2, S}.
__global__ __launch_bounds__(DP_THREADS) void disperse_total_kernel(const double* __restrict__ ws, int64_t B, double* __restrict__ result,
                                                                    float* loss_accum, float* dist_accum, float accum_weight) {
    __shared__ double sh[DP_THREADS];
    double se = 0.0, sd = 0.0;
    for (int64_t a = threadIdx.x; a < B; a += DP_THREADS) {
        se += ws[a];
        sd += ws[B + a];
    }
    se = block_sum_f64(se, sh);
    sd = block_sum_f64(sd, sh);
    if (threadIdx.x == 0) {
        const double b = (double)B, S = b + se;               // the B diagonal entries are exp(0) = 1 exactly
        const double pairs = b * (b - 1.0);
        const double L = B > 1 ? log(S / (b * b)) : 0.0;
        const double md = B > 1 ? sd / pairs : 0.0;
        result[0] = L;
        result[1] = md;
        result[2] = B > 1 ? (se / S) * (b * b) / pairs : 0.0;
        result[3] = S;
        if (loss_accum) *loss_accum += accum_weight * (float)L;
        if (dist_accum) *dist_accum += accum_weight * (float)md;
    }
}

// Stage 3: one workgroup per row a -> W'[a, j] = coef * p_aj (j != a), W'[a, a] = -coef * (row sum) / S, pad columns [B, ldw) = 0.
__global__ __launch_bounds__(DP_THREADS) void disperse_weights_kernel(const float* __restrict__ G, int64_t ldg, int64_t B, double inv_k,
                                                                      float inv_tau, double coef, const double* __restrict__ ws,
                                                                      const double* __restrict__ result, bf16* __restrict__ W, int64_t ldw) {
    const int64_t a = blockIdx.x;
    const double na = (double)G[a * ldg + a];
    const double c = coef / result[3];
    for (int64_t j = threadIdx.x; j < ldw; j += DP_THREADS) {
        float w = 0.f;
        if (j == a) {
            w = (float)(-c * ws[a]);
        } else if (j < B) {
            double d;
            w = (float)(c * (double)pair_exp(G, ldg, a, j, na, inv_k, inv_tau, d));
        }
        W[a * ldw + j] = f2bf(w);
    }
}

// G[i, j] = sum_k Z[i, k] Z[j, k]: one workgroup per output row i, wave w takes the columns j = w, w + 4, ...; a lane walks its 16-byte
// chunks of the contraction in ascending order (fp32 FMA), the 64 lane sums are added by the fixed DPP tree.  Reads rows < B only.
__global__ __launch_bounds__(256) void disperse_gram_small_kernel(const bf16* __restrict__ Z, int64_t ldz, int64_t B, int64_t K,
                                                                  float* __restrict__ G, int64_t ldg) {
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bf16* zi = Z + i * ldz;
    for (int64_t j = wave; j < B; j += 4) {
        const bf16* zj = Z + j * ldz;
        float acc = 0.f;
        for (int64_t k = (int64_t)lane * 8; k < K; k += 64 * 8) {
            const bf16x8 x = ld_bf16x8(zi + k), y = ld_bf16x8(zj + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(bf2f(x[e]), bf2f(y[e]), acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) G[i * ldg + j] = acc;
    }
}

}  // namespace

extern "C" int md_disperse_ws_doubles(int64_t B, int64_t* out) {
    if (!out || B < 1 || B > MD_DISPERSE_MAX_B) return MD_BAD_ARG;
    *out = 2 * B;
    return 0;
}

extern "C" int md_disperse_pairs(const float* G, int64_t ldg, int64_t B, int64_t K, float tau, double coef, void* W, int64_t ldw,
                                 double* result, double* ws, int64_t ws_doubles, float* loss_accum, float* dist_accum,
                                 float accum_weight, hipStream_t stream) {
    if (!G || !W || !result || !ws || B < 1 || B > MD_DISPERSE_MAX_B || K < 1 || ldg < B || ldw < B || ldw % 8 || ws_doubles < 2 * B)
        return MD_BAD_ARG;
    if (!(tau > 0.f) || !isfinite(tau) || !isfinite(coef)) return MD_BAD_ARG;
    const double inv_k = 1.0 / (double)K;
    const float inv_tau = 1.f / tau;
    hipLaunchKernelGGL(disperse_rows_kernel, dim3((unsigned)B), dim3(DP_THREADS), 0, stream, G, ldg, B, inv_k, inv_tau, ws);
    hipLaunchKernelGGL(disperse_total_kernel, dim3(1), dim3(DP_THREADS), 0, stream, ws, B, result, loss_accum, dist_accum, accum_weight);
    hipLaunchKernelGGL(disperse_weights_kernel, dim3((unsigned)B), dim3(DP_THREADS), 0, stream, G, ldg, B, inv_k, inv_tau, coef, ws, result,
                       reinterpret_cast<bf16*>(W), ldw);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_disperse_gram_small(const void* Z, int64_t ldz, int64_t B, int64_t K, float* G, int64_t ldg, hipStream_t stream) {
    if (!Z || !G || B < 1 || B > MD_DISPERSE_MAX_B || K < 8 || K % 8 || ldz < K || ldz % 8 || ldg < B) return MD_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(Z) % 16) return MD_BAD_ARG;
    hipLaunchKernelGGL(disperse_gram_small_kernel, dim3((unsigned)B), dim3(256), 0, stream, reinterpret_cast<const bf16*>(Z), ldz, B, K, G, ldg);
    MD_LAUNCH_CHECK();
    return 0;
}
