// Muon (opt-in): orthogonalised momentum for the hidden matrices of the DiT blocks (Jordan et al. 2024; Liu et al. 2025,
// "Muon is Scalable for LLM Training").  No reference counterpart: the reference trains every tensor with AdamW.
//   md_muon_ws_bytes        lays the workspace out: per matrix bf16 [X | A | B] (the iterate, two Gram-sized matrices), then one shared
//                           fp32 scratch the size of the largest matrix
//   md_muon_momentum        m' = mu m + coef g, u = coef g + mu m' (Nesterov), ||u||_F^2 per matrix in fp64 (fixed order, two stages),
//                           X0 = bf16(u / ||u||_F); the fp32 gradient accumulators of the matrices are zeroed.  Two launches over a
//                           work table: the norm pass reads g and m, the store pass recomputes u from the same values with the same
//                           instructions (parking u would cost the same 26 B / element and a buffer)
//   md_muon_newton_schulz   the quintic iteration on every matrix, driven from C: three md_gemm_bf16 launches per iteration and matrix
//                           (the Gram products of consecutive same-shape matrices -- the experts of one tensor -- as one batched launch)
//                           and two launches of the small a x + b y kernel that round the fp32 products to bf16 (md_muon_axpby)
//   md_muon_apply           p' = decay p - lr scale O, bf16 shadow, EMA of the weights, one launch over the table
// Table-driven like md_lora_* / md_tensor_stats_partial: a device copy the kernels read, a host copy the entry points validate and size
// their grids from.  16-byte accesses, no float atomics, one writer per address.
#include "md_common.h"
#include "../../include/microdit_hip.h"

#include <cmath>

namespace {

// The two scalars adamw_kernel forms before its loop, in its own words and under the same compiler settings (this block sits in front of
// the contraction pragma below): the clip coefficient and the weight-decay factor of a tensor under Muon are the bits AdamW would use.
__device__ __forceinline__ float clip_coef(float grad_scale, const float* sumsq, float max_norm) {
    float coef = grad_scale;
    if (sumsq && max_norm > 0.f) {
        const float nrm = sqrtf(*sumsq) * grad_scale;
        coef *= fminf(1.f, max_norm / (nrm + 1e-6f));
    }
    return coef;
}
__device__ __forceinline__ float decay_factor(float lr, float weight_decay) { return 1.f - lr * weight_decay; }

// Everything below states its fused multiply-adds itself (fmaf): the header promises one bit pattern per element.
#pragma clang fp contract(off)

constexpr int PARTS = MD_MUON_NORM_PARTS;     // workgroups (= fp64 partial sums) per matrix in the norm pass
constexpr int MAX_BATCH = 16;                 // same-shape matrices whose Gram products go out as one batched launch

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }

template <bool GBF16>
__device__ __forceinline__ float4 load_grad(const float* G, const bf16* Gb, int64_t e) {
    if (GBF16) {
        const bf16x4 gb = ld_bf16x4(Gb + e);
        return make_float4(bf2f(gb[0]), bf2f(gb[1]), bf2f(gb[2]), bf2f(gb[3]));
    }
    return ld4(G + e);
}

// m' and u of one element (the contract of md_muon_momentum)
__device__ __forceinline__ void momentum_1(float g, float m, float coef, float mu, bool nesterov, float& m_new, float& u) {
    const float gc = coef * g;
    m_new = fmaf(mu, m, gc);
    u = nesterov ? fmaf(mu, m_new, gc) : m_new;
}

// Stage one of ||u||^2: workgroup (x, item) adds the squares of float4 x * 256 + t, + PARTS * 256, ... of the item in fp64 (every
// square of an fp32 number is exact in fp64), thread by thread in ascending order, then the 256 thread sums by a fixed tree.
template <bool GBF16>
__global__ __launch_bounds__(256) void muon_norm_kernel(const float* G, const bf16* Gb, const float* M, const md_muon_item* items, float mu,
                                                         int nesterov, float grad_scale, const float* sumsq, float max_norm,
                                                         const int32_t* guard, double* partial) {
    if (guard && *guard == 0) return;          // skipped step: the store pass does not read the partials either
    __shared__ double red[256];
    const md_muon_item it = items[blockIdx.y];
    const int64_t n4 = (int64_t)it.rows * it.cols / 4;
    const float coef = clip_coef(grad_scale, sumsq, max_norm);
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)PARTS * 256) {
        const int64_t e = it.flat_off + i * 4;
        const float4 g = load_grad<GBF16>(G, Gb, e);
        const float4 m = ld4(M + e);
        const float* gp = &g.x;
        const float* mp = &m.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float mn, u;
            momentum_1(gp[k], mp[k], coef, mu, nesterov != 0, mn, u);
            s += (double)u * (double)u;
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * PARTS + blockIdx.x] = red[0];
}

// Stage two and the stores: every workgroup of an item adds the item's PARTS partials in ascending order (the same bits in all of
// them), workgroup 0 publishes the sum.
template <bool GBF16>
__global__ __launch_bounds__(256) void muon_momentum_kernel(float* G, const bf16* Gb, float* M, const md_muon_item* items, float mu, int nesterov,
                                                             float grad_scale, const float* sumsq, float max_norm, int zero_grad,
                                                             const int32_t* guard, bf16* ws, const double* partial, double* norms) {
    const bool go = !(guard && *guard == 0);
    const md_muon_item it = items[blockIdx.y];
    const int64_t n4 = (int64_t)it.rows * it.cols / 4;
    float inv = 0.f, coef = 0.f;
    if (go) {
        double nrm = 0.0;
        for (int k = 0; k < PARTS; ++k) nrm += partial[(int64_t)blockIdx.y * PARTS + k];
        inv = (float)(1.0 / (sqrt(nrm) + 1e-7));
        coef = clip_coef(grad_scale, sumsq, max_norm);
        if (blockIdx.x == 0 && threadIdx.x == 0) norms[blockIdx.y] = nrm;
    }
    bf16* X = ws + it.ws_off;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t e = it.flat_off + i * 4;
        if (go) {
            const float4 g = load_grad<GBF16>(G, Gb, e);
            float4 m = ld4(M + e);
            const float* gp = &g.x;
            float* mp = &m.x;
            bf16x4 x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float mn, u;
                momentum_1(gp[k], mp[k], coef, mu, nesterov != 0, mn, u);
                mp[k] = mn;
                x[k] = f2bf(u * inv);
            }
            st4(M + e, m);
            st_bf16x4(X + i * 4, x);
        }
        if (zero_grad) st4(G + e, make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

template <int EMA>
__global__ __launch_bounds__(256) void muon_apply_kernel(float* P, bf16* S, float* Em, const md_muon_item* items, float lr, float weight_decay,
                                                          float es, const int32_t* guard, const bf16* ws) {
    const bool go = !(guard && *guard == 0);
    const md_muon_item it = items[blockIdx.y];
    const int64_t n4 = (int64_t)it.rows * it.cols / 4;
    const float decay = decay_factor(lr, weight_decay);
    const float nls = -(lr * it.scale);
    const float omes = 1.f - es;
    const bf16* O = ws + it.ws_off;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t e = it.flat_off + i * 4;
        float4 p = ld4(P + e);
        float* pp = &p.x;
        if (go) {
            const bf16x4 o = ld_bf16x4(O + i * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) pp[k] = fmaf(nls, bf2f(o[k]), pp[k] * decay);
            st4(P + e, p);
            if (EMA == 2) {
                float4 em = ld4(Em + e);
                float* ep = &em.x;
#pragma unroll
                for (int k = 0; k < 4; ++k) ep[k] = fmaf(es, ep[k], omes * pp[k]);
                st4(Em + e, em);
            }
        }
        if (EMA == 1) st4(Em + e, p);           // ema_start: ema = weights (also on a skipped step, as in adamw_kernel)
        bf16x4 s;
        s[0] = f2bf(p.x); s[1] = f2bf(p.y); s[2] = f2bf(p.z); s[3] = f2bf(p.w);
        st_bf16x4(S + e, s);
    }
}

// out = bf16(a * x + b * y): x bf16, y the fp32 accumulators a GEMM left in the scratch; product, product, sum, each rounded once (no
// fused multiply-add), then one rounding to bf16 -- the iteration rounds where its emulation rounds.  out == x is allowed.
__global__ __launch_bounds__(256) void muon_axpby_kernel(const bf16* x, const float* y, bf16* out, float a, float b, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const bf16x8 xv = ld_bf16x8(x + i * 8);
        const float4 y0 = ld4(y + i * 8), y1 = ld4(y + i * 8 + 4);
        const float yv[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float ax = a * bf2f(xv[k]);
            const float by = b * yv[k];
            o[k] = f2bf(ax + by);
        }
        st_bf16x8(out + i * 8, o);
    }
}

void launch_axpby(const bf16* x, const float* y, bf16* out, float a, float b, int64_t n, hipStream_t st) {
    int64_t grid = (n / 8 + 255) / 256;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(muon_axpby_kernel, dim3((unsigned)grid), dim3(256), 0, st, x, y, out, a, b, n / 8);
}

inline int64_t gram_side(const md_muon_item& it) { return it.rows < it.cols ? it.rows : it.cols; }
inline int64_t ws_elems(const md_muon_item& it) {
    const int64_t g = gram_side(it);
    return (int64_t)it.rows * it.cols + 2 * g * g;
}

// Shapes, alignment and (check_ws) the workspace offsets of the host table; the size of the bf16 part of the workspace in elements (or
// -1) and, in *scratch, the floats of the shared fp32 scratch behind it: the largest matrix.
int64_t check_items(const md_muon_item* h, int32_t n, bool check_ws, int64_t* scratch = nullptr) {
    if (!h || n < 1 || n > 65535) return -1;
    int64_t at = 0, mx = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (h[i].rows < 64 || h[i].cols < 64 || h[i].rows % 64 || h[i].cols % 64 || h[i].flat_off < 0 || h[i].flat_off % 8) return -1;
        if (check_ws && h[i].ws_off != at) return -1;
        at += ws_elems(h[i]);
        const int64_t rc = (int64_t)h[i].rows * h[i].cols;
        if (rc > mx) mx = rc;
    }
    if (scratch) *scratch = mx;
    return at;
}

unsigned grid_x(const md_muon_item* h, int32_t n) {
    int64_t mx = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t c = ((int64_t)h[i].rows * h[i].cols / 4 + 255) / 256;
        if (c > mx) mx = c;
    }
    return (unsigned)(mx < 64 ? mx : 64);
}

}  // namespace

extern "C" int md_muon_ws_bytes(md_muon_item* items_host, int32_t n_items, int64_t* out) {
    int64_t scratch = 0;
    if (!out || check_items(items_host, n_items, false, &scratch) < 0) return MD_BAD_ARG;
    int64_t at = 0;
    for (int32_t i = 0; i < n_items; ++i) {
        items_host[i].ws_off = at;
        at += ws_elems(items_host[i]);
    }
    *out = at * 2 + scratch * 4;
    return 0;
}

extern "C" int md_muon_momentum(float* g, const void* g_bf16, float* m, const md_muon_item* items, const md_muon_item* items_host,
                                int32_t n_items, float mu, int32_t nesterov, float grad_scale, const float* sumsq, float max_norm,
                                int32_t zero_grad, const int32_t* guard, void* ws, double* partials, double* norms, hipStream_t st) {
    if (!g || !m || !items || !ws || !partials || !norms || check_items(items_host, n_items, true) < 0) return MD_BAD_ARG;
    if ((((uintptr_t)g | (uintptr_t)m | (uintptr_t)ws) & 15) || ((uintptr_t)g_bf16 & 15) || (((uintptr_t)partials | (uintptr_t)norms) & 7))
        return MD_BAD_ARG;
    if (!(mu >= 0.f && mu < 1.f)) return MD_BAD_ARG;
    const dim3 g1(PARTS, (unsigned)n_items), g2(grid_x(items_host, n_items), (unsigned)n_items), bd(256);
    const bf16* gb = static_cast<const bf16*>(g_bf16);
    if (gb) {
        hipLaunchKernelGGL((muon_norm_kernel<true>), g1, bd, 0, st, g, gb, m, items, mu, nesterov, grad_scale, sumsq, max_norm, guard, partials);
        hipLaunchKernelGGL((muon_momentum_kernel<true>), g2, bd, 0, st, g, gb, m, items, mu, nesterov, grad_scale, sumsq, max_norm, zero_grad,
                           guard, static_cast<bf16*>(ws), partials, norms);
    } else {
        hipLaunchKernelGGL((muon_norm_kernel<false>), g1, bd, 0, st, g, gb, m, items, mu, nesterov, grad_scale, sumsq, max_norm, guard, partials);
        hipLaunchKernelGGL((muon_momentum_kernel<false>), g2, bd, 0, st, g, gb, m, items, mu, nesterov, grad_scale, sumsq, max_norm, zero_grad,
                           guard, static_cast<bf16*>(ws), partials, norms);
    }
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_muon_apply(float* p, void* shadow, float* ema, const md_muon_item* items, const md_muon_item* items_host, int32_t n_items,
                             float lr, float weight_decay, int32_t ema_mode, float ema_smoothing, const int32_t* guard, const void* ws,
                             hipStream_t st) {
    if (!p || !shadow || !items || !ws || check_items(items_host, n_items, true) < 0) return MD_BAD_ARG;
    if (ema_mode < 0 || ema_mode > 2 || (ema_mode && !ema)) return MD_BAD_ARG;
    if ((((uintptr_t)p | (uintptr_t)shadow | (uintptr_t)ws) & 15) || (ema_mode && ((uintptr_t)ema & 15))) return MD_BAD_ARG;
    const dim3 gd(grid_x(items_host, n_items), (unsigned)n_items), bd(256);
    bf16* S = static_cast<bf16*>(shadow);
    const bf16* W = static_cast<const bf16*>(ws);
    if (ema_mode == 0) hipLaunchKernelGGL((muon_apply_kernel<0>), gd, bd, 0, st, p, S, ema, items, lr, weight_decay, ema_smoothing, guard, W);
    else if (ema_mode == 1) hipLaunchKernelGGL((muon_apply_kernel<1>), gd, bd, 0, st, p, S, ema, items, lr, weight_decay, ema_smoothing, guard, W);
    else hipLaunchKernelGGL((muon_apply_kernel<2>), gd, bd, 0, st, p, S, ema, items, lr, weight_decay, ema_smoothing, guard, W);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_muon_axpby(const void* x, const float* y, void* out, float a, float b, int64_t n, hipStream_t st) {
    if (!x || !y || !out || n <= 0 || n % 8 || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)out) & 15)) return MD_BAD_ARG;
    launch_axpby(static_cast<const bf16*>(x), y, static_cast<bf16*>(out), a, b, n, st);
    MD_LAUNCH_CHECK();
    return 0;
}

// One iteration of one matrix: A = bf16(X X^T) (bf16 store; the Gram products of a run of same-shape items as ONE batched launch),
// T = A A and U = B X as fp32 stores into the shared scratch, B = bf16(b A + c T) and X = bf16(a X + U) by the axpby kernel, in place.
// The fp32 sums round to bf16 exactly where the emulation of tests/muon_ref.py rounds: after A, after B, after the new X.
extern "C" int md_muon_newton_schulz(const md_muon_item* items_host, int32_t n_items, int32_t steps, float a, float b, float c, void* ws,
                                     int32_t* gemm_launches, hipStream_t st) {
    int64_t scratch_floats = 0;
    const int64_t bf_elems = check_items(items_host, n_items, true, &scratch_floats);
    if (!ws || ((uintptr_t)ws & 15) || bf_elems < 0) return MD_BAD_ARG;
    if (steps < 1 || steps > 8 || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c)) return MD_BAD_ARG;
    bf16* W = static_cast<bf16*>(ws);
    float* T = reinterpret_cast<float*>(W + bf_elems);      // bf_elems is a multiple of 4096: 16-byte aligned
    int32_t launches = 0;
    for (int32_t i0 = 0; i0 < n_items;) {
        const md_muon_item& h = items_host[i0];
        int32_t nb = 1;                       // consecutive items of one shape sit one ws_elems apart: a batch stride
        while (i0 + nb < n_items && nb < MAX_BATCH && items_host[i0 + nb].rows == h.rows && items_host[i0 + nb].cols == h.cols) ++nb;
        const int64_t r = h.rows, cc = h.cols, rc = r * cc, gs = gram_side(h), stride = ws_elems(h);
        const bool wide = r <= cc;
        const int64_t offX = h.ws_off, offA = offX + rc, offB = offA + gs * gs;
        for (int32_t k = 0; k < steps; ++k) {
            md_gemm_args ga = {};
            ga.A = ga.B = W + offX;
            ga.C = W + offA;
            ga.M = ga.N = gs;
            ga.K = wide ? cc : r;
            ga.lda = ga.ldb = cc;
            ga.ldc = gs;
            ga.a_kcontig = ga.b_kcontig = wide ? 1 : 0;
            ga.batch = nb;
            ga.sA = ga.sB = ga.sC = stride;
            ga.ksplit = 1;
            ga.mode = MD_EPI_STORE_BF16;
            ga.alpha = 1.f;
            int rcode = md_gemm_bf16(&ga, st);
            if (rcode) return rcode;
            ++launches;
            for (int32_t j = 0; j < nb; ++j) {
                bf16* base = W + (int64_t)j * stride;
                md_gemm_args gt = {};                           // T = A A, as stored: sum_k A[m, k] A[k, n]
                gt.A = gt.B = base + offA;
                gt.C = T;
                gt.M = gt.N = gt.K = gs;
                gt.lda = gt.ldb = gt.ldc = gs;
                gt.a_kcontig = 1;
                gt.b_kcontig = 0;
                gt.batch = gt.ksplit = 1;
                gt.mode = MD_EPI_STORE_F32;
                gt.alpha = 1.f;
                if ((rcode = md_gemm_bf16(&gt, st))) return rcode;
                launch_axpby(base + offA, T, base + offB, b, c, gs * gs, st);
                md_gemm_args gx = {};                           // U = B X (wide) or X B (tall)
                gx.A = wide ? base + offB : base + offX;
                gx.B = wide ? base + offX : base + offB;
                gx.C = T;
                gx.M = r;
                gx.N = cc;
                gx.K = gs;
                gx.lda = wide ? gs : cc;
                gx.ldb = cc;
                gx.ldc = cc;
                gx.a_kcontig = 1;
                gx.b_kcontig = 0;
                gx.batch = gx.ksplit = 1;
                gx.mode = MD_EPI_STORE_F32;
                gx.alpha = 1.f;
                if ((rcode = md_gemm_bf16(&gx, st))) return rcode;
                launch_axpby(base + offX, T, base + offX, a, 1.f, rc, st);
                launches += 2;
            }
        }
        i0 += nb;
    }
    MD_LAUNCH_CHECK();
    if (gemm_launches) *gemm_launches = launches;
    return 0;
}
