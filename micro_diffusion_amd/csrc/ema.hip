// Post-hoc EMA (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 3 / App. C):
//   md_ema_power_update[_ranges]   up to MD_EMA_MAX_PROFILES power-function averages of the fp32 masters in ONE pass behind the AdamW
//                                  pass: every float4 of p is read once, every profile k is read and written once,
//                                  e_k = beta_k * e_k + (1 - beta_k) * p in fp32: 4 + 8 K bytes per parameter.  beta_k is computed by
//                                  the host (fp64, (1 - 1/t)^(gamma_k + 1)); beta_k == 0 (t = 1) stores p without reading e_k.
// A pass of its own, NOT one more template form of adamw_kernel (optim.hip): folding it in would save the 4 B / parameter re-read of
// p, but it would change the code of the default step, which stays bit-identical, and that kernel already carries 6 forms.
// No reference counterpart: the reference trains with one fixed EMA length at most (configs/res_512_*.yaml:4-9).
#include "md_common.h"
#include "../../include/microdit_hip.h"

namespace {

// 16-byte non-temporal accesses (as optim.hip: the builtins take clang vector types, not HIP's float4 struct)
__device__ __forceinline__ float4 nt_load4(const float* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void nt_store4(float* p, const float4& v) {
    f32x4 t;
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p));
}

constexpr int EMA_MAX = MD_EMA_MAX_PROFILES;
constexpr int EMA_MAX_RANGES = MD_ADAMW_MAX_RANGES;

// Kernel arguments by value (like AdamWRanges): the profile pointers and their betas; no device-side pointer table.
struct EmaProfiles {
    float* e[EMA_MAX];
    float beta[EMA_MAX];
};

// The rank's chunks of the flat buffers, packed back to back in the index space the kernel walks (the convention of
// md_adamw_step_ranges; here every buffer is flat, the packed index only enumerates the work).
struct EmaRanges {
    int n;
    int64_t start[EMA_MAX_RANGES + 1];     // start[n] = total packed elements
    int64_t flat[EMA_MAX_RANGES];
};

__device__ __forceinline__ int64_t range_flat4(const EmaRanges& rg, int64_t ip) {
    int lo = 0, hi = rg.n - 1;
    const int64_t e = ip * 4;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rg.start[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return (rg.flat[lo] + (e - rg.start[lo])) >> 2;
}

// `guard` (NULL = no guard): the go flag of md_step_guard.  At 0 (a skipped step) every profile stays as it is, bit for bit: the
// contract of md_adamw_step_guarded for a live EMA.
template <int K, bool RANGES>
__global__ __launch_bounds__(256) void ema_power_kernel(const float* __restrict__ P, EmaProfiles pr, EmaRanges rg, int64_t n4,
                                                        const int32_t* guard) {
    if (guard && *guard == 0) return;
    for (int64_t ip = (int64_t)blockIdx.x * 256 + threadIdx.x; ip < n4; ip += (int64_t)gridDim.x * 256) {
        const int64_t i = RANGES ? range_flat4(rg, ip) : ip;
        const float4 p = nt_load4(P + i * 4);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float b = pr.beta[k];
            float4 e = p;
            if (b != 0.f) {                 // uniform: beta == 0 (t = 1) never reads the buffer -- NaN in it must not survive
                const float4 o = nt_load4(pr.e[k] + i * 4);
                e.x = b * o.x + (1.f - b) * p.x;
                e.y = b * o.y + (1.f - b) * p.y;
                e.z = b * o.z + (1.f - b) * p.z;
                e.w = b * o.w + (1.f - b) * p.w;
            }
            nt_store4(pr.e[k] + i * 4, e);
        }
    }
}

int check_profiles(const float* p, float* const* ema, const float* beta, int32_t n_profiles, EmaProfiles* pr) {
    if (!p || !ema || !beta || n_profiles < 1 || n_profiles > EMA_MAX || ((uintptr_t)p & 15)) return MD_BAD_ARG;
    for (int k = 0; k < EMA_MAX; ++k) {
        pr->e[k] = nullptr;
        pr->beta[k] = 0.f;
    }
    for (int k = 0; k < n_profiles; ++k) {
        if (!ema[k] || ((uintptr_t)ema[k] & 15) || !(beta[k] >= 0.f) || !(beta[k] < 1.f)) return MD_BAD_ARG;     // (NaN fails both)
        pr->e[k] = ema[k];
        pr->beta[k] = beta[k];
    }
    return 0;
}

template <bool RANGES>
void launch(const float* p, const EmaProfiles& pr, const EmaRanges& rg, int32_t n_profiles, int64_t n, const int32_t* guard,
            hipStream_t st) {
    // the grid of adamw_kernel: one 256-thread workgroup per 4 KiB of every stream and iteration, capped at 8192 workgroups
    int64_t grid = (n / 4 + 255) / 256;
    if (grid > 8192) grid = 8192;
    const dim3 gd((unsigned)grid), bd(256);
#define EMAK(K) hipLaunchKernelGGL((ema_power_kernel<K, RANGES>), gd, bd, 0, st, p, pr, rg, n / 4, guard)
    if (n_profiles == 1) EMAK(1); else if (n_profiles == 2) EMAK(2); else if (n_profiles == 3) EMAK(3); else EMAK(4);
#undef EMAK
}

}  // namespace

extern "C" int md_ema_power_update(const float* p, float* const* ema, const float* beta, int32_t n_profiles, int64_t n,
                                   const int32_t* guard, hipStream_t st) {
    EmaProfiles pr;
    if (check_profiles(p, ema, beta, n_profiles, &pr)) return MD_BAD_ARG;
    if (n <= 0 || n % 4) return MD_BAD_ARG;
    EmaRanges none;
    none.n = 0;
    launch<false>(p, pr, none, n_profiles, n, guard, st);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_ema_power_update_ranges(const float* p, float* const* ema, const float* beta, int32_t n_profiles,
                                          const int64_t* flat_off, const int64_t* count, int32_t n_ranges, const int32_t* guard,
                                          hipStream_t st) {
    EmaProfiles pr;
    if (check_profiles(p, ema, beta, n_profiles, &pr)) return MD_BAD_ARG;
    if (!flat_off || !count || n_ranges < 1 || n_ranges > EMA_MAX_RANGES) return MD_BAD_ARG;
    EmaRanges rg;
    rg.n = n_ranges;
    int64_t tot = 0;
    for (int j = 0; j < n_ranges; ++j) {
        if (count[j] <= 0 || count[j] % 4 || flat_off[j] < 0 || flat_off[j] % 4) return MD_BAD_ARG;
        rg.start[j] = tot;
        rg.flat[j] = flat_off[j];
        tot += count[j];
    }
    rg.start[n_ranges] = tot;
    launch<true>(p, pr, rg, n_profiles, tot, guard, st);
    MD_LAUNCH_CHECK();
    return 0;
}
