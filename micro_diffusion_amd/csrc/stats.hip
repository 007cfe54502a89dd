// Per-tensor statistics of a flat buffer (the optimizer monitor: composer.callbacks.OptimizerMonitor named by configs/*.yaml):
//   md_tensor_stats_partial   one workgroup per WORK ITEM (a piece of at most MD_STATS_ITEM_MAX elements of one tensor, grid-strided):
//                             sum of squares, max |x| and the number of non-finite elements of the piece -> part_*[item]
//   md_tensor_stats_finish    one wave per tensor: adds / maxes the partials of the tensor's run of items -> sumsq / absmax / nonfinite [t]
// A segmented form of md_sumsq / md_sumsq_finish (optim.hip): the same bytes are read once, with non-temporal 16-byte loads, plus one
// 16-byte table entry per item.  DETERMINISTIC: no atomics, one writer per address, every sum in an order that is a function of the
// item table alone (thread t of the workgroup owns vectors t, t + 256, ... of the item; fixed wave and workgroup reduction trees; the
// finish adds items begin + lane, begin + lane + 64, ... and then reduces the 64 lanes by the same fixed tree).
// A non-finite element (NaN, +-Inf) is counted and EXCLUDED from the sum and the maximum: the table still describes the rest of the
// tensor.  The last, partial vector of an item is read element by element: nothing beyond `count` is touched, padding may hold anything.
#include "md_common.h"
#include "../../include/microdit_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

struct Acc {
    float s, mx;
    int nf;
};

__device__ __forceinline__ void take_bits(Acc& a, uint32_t bits) {
    const bool fin = (bits & 0x7f800000u) != 0x7f800000u;
    const float x = fin ? __builtin_bit_cast(float, bits) : 0.f;
    a.s += x * x;
    a.mx = fmaxf(a.mx, fabsf(x));
    a.nf += fin ? 0 : 1;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool BF16>
__global__ __launch_bounds__(256) void stats_partial_kernel(const void* xv, const md_stats_item* items, int64_t n_items, float* part_sumsq,
                                                            float* part_absmax, int32_t* part_nonfinite) {
    __shared__ float red_s[4], red_m[4];
    __shared__ int red_n[4];
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const md_stats_item item = items[it];                    // uniform: scalar loads
        const int count = item.count;
        Acc a = {0.f, 0.f, 0};
        // 8 elements per thread and iteration (two 16-byte loads of fp32, one of bf16): at most 65536 / 2048 = 32 iterations, so one
        // thread chains at most 256 terms
        for (int e0 = threadIdx.x * 8; e0 < count; e0 += 256 * 8) {
            if (BF16) {
                const uint16_t* p = reinterpret_cast<const uint16_t*>(xv) + item.src_off + e0;
                if (e0 + 8 <= count) {
                    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        take_bits(a, v[e] << 16);
                        take_bits(a, v[e] & 0xffff0000u);
                    }
                } else {
                    for (int e = 0; e < count - e0; ++e) take_bits(a, (uint32_t)p[e] << 16);
                }
            } else {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(xv) + item.src_off + e0;
                if (e0 + 8 <= count) {
                    const u32x4 v0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
                    const u32x4 v1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 4));
#pragma unroll
                    for (int e = 0; e < 4; ++e) take_bits(a, v0[e]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) take_bits(a, v1[e]);
                } else {
                    for (int e = 0; e < count - e0; ++e) take_bits(a, p[e]);
                }
            }
        }
        const float s = wave_sum(a.s);
        const float m = wave_max(a.mx);
        const int n = wave_sum_i(a.nf);
        if ((threadIdx.x & 63) == 0) {
            red_s[threadIdx.x >> 6] = s;
            red_m[threadIdx.x >> 6] = m;
            red_n[threadIdx.x >> 6] = n;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            part_sumsq[it] = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
            part_absmax[it] = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
            part_nonfinite[it] = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
        }
        __syncthreads();                                         // red_* are rewritten by the next item
    }
}

// One wave per tensor.  An empty run (a tensor of which this rank holds nothing: sharded mode) gives 0 / 0 / 0.
__global__ __launch_bounds__(64) void stats_finish_kernel(const float* part_sumsq, const float* part_absmax, const int32_t* part_nonfinite,
                                                          const int32_t* item_begin, float* sumsq, float* absmax, int32_t* nonfinite) {
    const int t = blockIdx.x;
    const int lo = item_begin[t], hi = item_begin[t + 1];
    float s = 0.f, m = 0.f;
    int n = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 64) {
        s += part_sumsq[i];
        m = fmaxf(m, part_absmax[i]);
        n += part_nonfinite[i];
    }
    s = wave_sum(s);
    m = wave_max(m);
    n = wave_sum_i(n);
    if (threadIdx.x == 0) {
        sumsq[t] = s;
        absmax[t] = m;
        nonfinite[t] = n;
    }
}

}  // namespace

extern "C" int md_tensor_stats_partial(const void* x, int32_t x_is_bf16, const md_stats_item* items, int64_t n_items, float* part_sumsq,
                                       float* part_absmax, int32_t* part_nonfinite, hipStream_t st) {
    if (!x || !items || !part_sumsq || !part_absmax || !part_nonfinite || n_items <= 0 || ((uintptr_t)x & 15)) return MD_BAD_ARG;
    // 8 workgroups of 256 threads resident per CU x 256 CUs; longer tables are grid-strided
    const dim3 gd((unsigned)(n_items < 2048 ? n_items : 2048)), bd(256);
    if (x_is_bf16)
        hipLaunchKernelGGL((stats_partial_kernel<true>), gd, bd, 0, st, x, items, n_items, part_sumsq, part_absmax, part_nonfinite);
    else
        hipLaunchKernelGGL((stats_partial_kernel<false>), gd, bd, 0, st, x, items, n_items, part_sumsq, part_absmax, part_nonfinite);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_tensor_stats_finish(const float* part_sumsq, const float* part_absmax, const int32_t* part_nonfinite,
                                      const int32_t* item_begin, int32_t n_tensors, float* sumsq, float* absmax, int32_t* nonfinite,
                                      hipStream_t st) {
    if (!part_sumsq || !part_absmax || !part_nonfinite || !item_begin || !sumsq || !absmax || !nonfinite || n_tensors <= 0)
        return MD_BAD_ARG;
    hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)n_tensors), dim3(64), 0, st, part_sumsq, part_absmax, part_nonfinite, item_begin,
                       sumsq, absmax, nonfinite);
    MD_LAUNCH_CHECK();
    return 0;
}
