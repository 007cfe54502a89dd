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


// ---------------------------------------------------------------------------------------------------------------------
// Model diagnostics: the EDM loss by noise level and the state of the expert-choice router.  Same rules as above:
// no float atomic, every floating sum in an order that is a function of the shape alone, fp64 accumulators; the counts are integers
// (LDS / global integer atomics: exact in any order).  All outputs are ADDED TO.
// ---------------------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) int32_t i32x4;

constexpr int HIST_CHUNK = 1024;   // samples staged in LDS at a time
constexpr int HIST_MAX_BINS = 64;  // one lane of a wave per bin

// ONE workgroup.  Per chunk of 1024 samples: all threads compute the bin (-1: loss not finite) of their samples into LDS, then wave q
// scans quarter q of the chunk in ascending sample order with lane j keeping bin j (every lane reads the same LDS word: a broadcast);
// wave 0 adds the four quarter sums in ascending order onto the bin's running total.
__global__ __launch_bounds__(256) void loss_sigma_hist_kernel(const float* sigma, const float* loss, int64_t B, float log_lo, float log_hi,
                                                              int nbins, double* sum, long long* count, long long* nonfinite) {
    __shared__ float s_loss[HIST_CHUNK];
    __shared__ int s_bin[HIST_CHUNK];
    __shared__ double part[4][HIST_MAX_BINS];
    __shared__ int pcnt[4][HIST_MAX_BINS];
    __shared__ int s_nf;
    const int tid = threadIdx.x, j = tid & 63, q = tid >> 6;
    double acc = 0.0;
    long long cnt = 0;
    if (tid == 0) s_nf = 0;
    __syncthreads();
    for (int64_t base = 0; base < B; base += HIST_CHUNK) {
        const int n = (int)(B - base < HIST_CHUNK ? B - base : HIST_CHUNK);
        for (int i = tid; i < n; i += 256) {
            const float l = loss[base + i];
            const bool fin = (__builtin_bit_cast(uint32_t, l) & 0x7f800000u) != 0x7f800000u;
            const float t = floorf((logf(sigma[base + i]) - log_lo) * (float)nbins / (log_hi - log_lo));
            const int bin = t >= (float)(nbins - 1) ? nbins - 1 : (t > 0.f ? (int)t : 0);      // a NaN lands in bin 0
            s_loss[i] = l;
            s_bin[i] = fin ? bin : -1;
            if (!fin) atomicAdd(&s_nf, 1);
        }
        __syncthreads();
        double s = 0.0;
        int c = 0;
        const int i1 = n < (q + 1) * 256 ? n : (q + 1) * 256;
        for (int i = q * 256; i < i1; ++i) {
            const bool hit = s_bin[i] == j;
            s += hit ? (double)s_loss[i] : 0.0;
            c += hit ? 1 : 0;
        }
        part[q][j] = s;
        pcnt[q][j] = c;
        __syncthreads();                                         // (also: s_loss / s_bin are rewritten by the next chunk)
        if (q == 0) {
            acc += ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
            cnt += (pcnt[0][j] + pcnt[1][j]) + (pcnt[2][j] + pcnt[3][j]);
        }
    }
    if (q == 0 && j < nbins) {
        sum[j] += acc;
        count[j] += cnt;
    }
    if (tid == 0) nonfinite[0] += s_nf;
}

// Launch shape of md_moe_route_stats, a function of (B, S, E, k) alone: RS_TOK_WGS workgroups take the 256-token blocks w, w + G, ...;
// every expert's run of B*k gate values is cut over GG workgroups in chunks of 2048.  The workspace holds DOUBLES (two floats each):
// [G][1 + E] token partials, then [E][GG] gate partials.
constexpr int RS_TOK_WGS = 128, RS_GATE_WGS = 32, RS_GATE_CHUNK = 2048;
inline int64_t rs_tok_wgs(int64_t M) { return (M + 255) / 256 < RS_TOK_WGS ? (M + 255) / 256 : RS_TOK_WGS; }
inline int64_t rs_gate_wgs(int64_t Bk) {
    const int64_t c = (Bk + RS_GATE_CHUNK - 1) / RS_GATE_CHUNK;
    return c < RS_GATE_WGS ? c : RS_GATE_WGS;
}
// B*k <= B*S: the size asked for (B, S, E) covers every k
inline int64_t rs_ws_doubles(int64_t M, int64_t E) { return rs_tok_wgs(M) * (1 + E) + E * rs_gate_wgs(M); }

// Workgroups [0, G): tokens.  Thread t of a block holds one token: its slot row (coverage = entries >= 0 -> LDS histogram) and its
// E probabilities (16-byte loads when vec_tok: E % 4 == 0, ldp % 4 == 0, aligned bases; columns >= E are never read), entropy in
// fp32; entropy and probabilities go to an LDS tile [256][1 + EMAX] (odd leading dimension: conflict-free both ways), whose columns
// are then summed in fp64: lane c of the 32-lane group g adds tokens 32 g .. 32 g + 31 of column c in ascending order, thread c adds
// the 8 group sums in ascending order onto the column's running total.  Rows past M hold zeros.
// Workgroups [G, G + E * GG): gate values.  Thread t adds elements 8 t .. 8 t + 7 of each of its chunks in fp64, then a fixed tree.
template <int EMAX>
__global__ __launch_bounds__(256) void route_stats_partial_kernel(const int32_t* slot, const float* probs, int64_t ldp, const float* gval,
                                                                  int64_t M, int E, int64_t Bk, int G, int GG, int vec_tok, int vec_gate,
                                                                  double* ws, unsigned long long* cover_hist) {
    constexpr int LD = EMAX + 1;
    __shared__ double sh[(256 * LD + 1) / 2 + 8 * 32];           // tile (floats), then the 8 x 32 group sums; the gate part: red[256]
    __shared__ int lh[EMAX + 1];
    const int tid = threadIdx.x;
    const int NC = E + 1;
    if ((int)blockIdx.x < G) {
        float* tile = reinterpret_cast<float*>(sh);
        double* seg = sh + (256 * LD + 1) / 2;
        if (tid <= EMAX) lh[tid] = 0;
        __syncthreads();
        double run = 0.0;
        for (int64_t blk = blockIdx.x; blk * 256 < M; blk += G) {
            const int64_t row = blk * 256 + tid;
            float* my = tile + tid * LD;
            if (row < M) {
                const int32_t* sr = slot + row * E;
                const float* pr = probs + row * ldp;
                int cover = 0;
                float ent = 0.f;
#pragma unroll
                for (int e0 = 0; e0 < EMAX; e0 += 4) {
                    if (e0 < E) {
                        i32x4 s4 = {-1, -1, -1, -1};
                        f32x4 p4 = {0.f, 0.f, 0.f, 0.f};
                        if (vec_tok && e0 + 4 <= E) {
                            s4 = *reinterpret_cast<const i32x4*>(sr + e0);
                            p4 = *reinterpret_cast<const f32x4*>(pr + e0);
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (e0 + i < E) {
                                    s4[i] = sr[e0 + i];
                                    p4[i] = pr[e0 + i];
                                }
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            cover += s4[i] >= 0 ? 1 : 0;
                            ent -= p4[i] > 0.f ? p4[i] * logf(p4[i]) : 0.f;
                            if (e0 + i < E) my[1 + e0 + i] = p4[i];
                        }
                    }
                }
                my[0] = ent;
                atomicAdd(&lh[cover], 1);
            } else {
                for (int c = 0; c < NC; ++c) my[c] = 0.f;
            }
            __syncthreads();
            const int c = tid & 31, g = tid >> 5;
            if (c < NC) {
                double s = 0.0;
                for (int i = 0; i < 32; ++i) s += (double)tile[(g * 32 + i) * LD + c];
                seg[g * 32 + c] = s;
            }
            __syncthreads();                                     // (also: the tile is rewritten by the next block)
            if (tid < NC) {
                double s = seg[tid];
                for (int g2 = 1; g2 < 8; ++g2) s += seg[g2 * 32 + tid];
                run += s;
            }
        }
        if (tid < NC) ws[(int64_t)blockIdx.x * NC + tid] = run;
        if (tid <= E && lh[tid] != 0) atomicAdd(&cover_hist[tid], (unsigned long long)lh[tid]);
    } else {
        double* red = sh;
        const int w = (int)blockIdx.x - G;
        const int e = w / GG, g = w % GG;
        const float* src = gval + (int64_t)e * Bk;
        double s = 0.0;
        for (int64_t c0 = (int64_t)g * RS_GATE_CHUNK; c0 < Bk; c0 += (int64_t)GG * RS_GATE_CHUNK) {
            const int64_t i0 = c0 + tid * 8;
            if (vec_gate && i0 + 8 <= Bk) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + i0);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + i0 + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) s += (double)v0[i];
#pragma unroll
                for (int i = 0; i < 4; ++i) s += (double)v1[i];
            } else {
                for (int i = 0; i < 8; ++i)
                    if (i0 + i < Bk) s += (double)src[i0 + i];
            }
        }
        red[tid] = s;
        __syncthreads();
        if (tid < 64) red[tid] = ((red[tid] + red[tid + 64]) + red[tid + 128]) + red[tid + 192];
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int i = 0; i < 64; ++i) t += red[i];
            ws[(int64_t)G * NC + (int64_t)e * GG + g] = t;
        }
    }
}

// One wave: thread c < 1 + E adds the G token partials of column c, thread 1 + E + e the GG gate partials of expert e, both in
// ascending workgroup order, onto fstats.
__global__ __launch_bounds__(64) void route_stats_finish_kernel(const double* ws, int E, int G, int GG, double* fstats) {
    const int c = threadIdx.x, NC = E + 1;
    if (c < NC) {
        double s = 0.0;
        for (int w = 0; w < G; ++w) s += ws[(int64_t)w * NC + c];
        fstats[c] += s;
    } else if (c < NC + E) {
        const double* p = ws + (int64_t)G * NC + (int64_t)(c - NC) * GG;
        double s = 0.0;
        for (int g = 0; g < GG; ++g) s += p[g];
        fstats[c] += s;
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

extern "C" int md_loss_sigma_hist(const float* sigma, const float* loss_per_sample, int64_t B, float log_lo, float log_hi, int32_t nbins,
                                  double* sum, int64_t* count, int64_t* nonfinite, hipStream_t st) {
    if (!sigma || !loss_per_sample || !sum || !count || !nonfinite || B <= 0 || nbins < 1 || nbins > HIST_MAX_BINS || !(log_hi > log_lo))
        return MD_BAD_ARG;
    hipLaunchKernelGGL(loss_sigma_hist_kernel, dim3(1), dim3(256), 0, st, sigma, loss_per_sample, B, log_lo, log_hi, (int)nbins, sum,
                       (long long*)count, (long long*)nonfinite);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_moe_route_stats_ws_floats(int64_t B, int64_t S, int32_t E, int64_t* out) {
    if (!out || B <= 0 || S <= 0 || E <= 0 || E > 16) return MD_BAD_ARG;
    *out = 2 * rs_ws_doubles(B * S, E);
    return 0;
}

extern "C" int md_moe_route_stats(const int32_t* slot, const float* probs, int64_t ldp, const float* gval, int64_t B, int64_t S, int32_t E,
                                  int32_t k, float* ws, int64_t ws_floats, int64_t* cover_hist, double* fstats, hipStream_t st) {
    if (!slot || !probs || !gval || !ws || !cover_hist || !fstats || B <= 0 || S <= 0 || E <= 0 || E > 16 || ldp < E || k <= 0 || k > S ||
        ((uintptr_t)ws & 7))
        return MD_BAD_ARG;
    const int64_t M = B * S, Bk = B * k;
    if (ws_floats < 2 * rs_ws_doubles(M, E)) return MD_BAD_ARG;
    const int G = (int)rs_tok_wgs(M), GG = (int)rs_gate_wgs(Bk);
    const int vec_tok = E % 4 == 0 && ldp % 4 == 0 && !((uintptr_t)slot & 15) && !((uintptr_t)probs & 15);
    const int vec_gate = Bk % 4 == 0 && !((uintptr_t)gval & 15);
    const dim3 gd((unsigned)(G + E * GG)), bd(256);
    double* wsd = reinterpret_cast<double*>(ws);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(cover_hist);
    if (E <= 4)
        hipLaunchKernelGGL((route_stats_partial_kernel<4>), gd, bd, 0, st, slot, probs, ldp, gval, M, (int)E, Bk, G, GG, vec_tok, vec_gate, wsd, hist);
    else if (E <= 8)
        hipLaunchKernelGGL((route_stats_partial_kernel<8>), gd, bd, 0, st, slot, probs, ldp, gval, M, (int)E, Bk, G, GG, vec_tok, vec_gate, wsd, hist);
    else
        hipLaunchKernelGGL((route_stats_partial_kernel<16>), gd, bd, 0, st, slot, probs, ldp, gval, M, (int)E, Bk, G, GG, vec_tok, vec_gate, wsd, hist);
    hipLaunchKernelGGL(route_stats_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)wsd, (int)E, G, GG, fstats);
    MD_LAUNCH_CHECK();
    return 0;
}
