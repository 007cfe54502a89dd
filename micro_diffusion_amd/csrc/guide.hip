// Measurement-guided sampling (Chung et al. 2023, "Diffusion Posterior Sampling", on the EDM loop): everything around
// the two network passes of a guided step.  No reference source: the reference has no guided sampler.
//   md_edm_denoised(_tok)    D = c_skip * float(x_hat) + c_out * F as an fp32 image, F from the fp32 image output or the bf16 token rows
//   md_measure_residual      r = m * (meas - pool_s(D));  L_b = sum r^2 (fp64);  q = dL/dD = -2 m r / s^2 over each pooling window
//   md_guide_cotangent_tok   dtok = w c_out q (conditional rows), (1 - w) c_out q (unconditional rows): bf16, the output-token layout
//   md_edm_guide_apply       x_next -= zeta / max(sqrt(L_b), MD_GUIDE_TINY) * (c_skip q + c_in (dx_c + dx_u)) in fp64, in place
// All four are bandwidth-bound passes over B * C * H * W elements (262,144 at XL/2 and B = 64: about a megabyte each way), without
// atomics; two calls give the same bits.
#include "md_common.h"
#include "sampler_math.h"
#include "sampler_tok.h"
#include "../../include/microdit_hip.h"
#include <cmath>

namespace {

// the grid helper of edm.hip
inline int egrid(int64_t work) {
    int64_t g = (work + 255) / 256;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (int)g;
}

// ---------------------------------------------------------------------------------------------------------------------
// md_edm_denoised: item = 4 consecutive elements (two 16-byte loads of the state, one of each F, one 16-byte store), or one element.
// ---------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void denoised_kernel(const double* x_in, const float* F, const float* Fu, float* D, int64_t n, float cfg,
                                                       double t_in, float sigma_data) {
    float c_skip, c_out;
    heun_coef(t_in, sigma_data, c_skip, c_out);
    const int64_t items = VEC ? n / 4 : n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        if (VEC) {
            const double2 xa = reinterpret_cast<const double2*>(x_in)[2 * i], xb = reinterpret_cast<const double2*>(x_in)[2 * i + 1];
            float4 f = reinterpret_cast<const float4*>(F)[i];
            if (Fu) {
                const float4 u = reinterpret_cast<const float4*>(Fu)[i];
                f.x = cfg_combine(f.x, u.x, cfg), f.y = cfg_combine(f.y, u.y, cfg);
                f.z = cfg_combine(f.z, u.z, cfg), f.w = cfg_combine(f.w, u.w, cfg);
            }
            float4 d;
            d.x = sampler_denoised_f32(xa.x, f.x, c_skip, c_out), d.y = sampler_denoised_f32(xa.y, f.y, c_skip, c_out);
            d.z = sampler_denoised_f32(xb.x, f.z, c_skip, c_out), d.w = sampler_denoised_f32(xb.y, f.w, c_skip, c_out);
            reinterpret_cast<float4*>(D)[i] = d;
        } else {
            float f = F[i];
            if (Fu) f = cfg_combine(f, Fu[i], cfg);
            D[i] = sampler_denoised_f32(x_in[i], f, c_skip, c_out);
        }
    }
}

// Token-space items: sampler_tok.h.
// D[b, c, ti*p+ph, tj*p+pw] from tok[row, (ph*p + pw)*C + c] (the second operand: the same row of tok_u): md_unpatchify followed by
// denoised_kernel, without the fp32 image of F in between
template <bool VEC>
__global__ __launch_bounds__(256) void denoised_tok_kernel(const double* x_in, const bf16* tok, const bf16* tok_u, float* D, int64_t B, int C,
                                                           int H, int W, int p, float cfg, double t_in, float sigma_data) {
    float c_skip, c_out;
    heun_coef(t_in, sigma_data, c_skip, c_out);
    const int gh = H / p, gw = W / p, pv = C * p * p, nseg = (pv + 7) / 8;
    const int64_t total = B * gh * gw * nseg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const tok_item t = tok_item_of(i, gh, gw, nseg);
        const int64_t off = t.row * pv + t.e0;
        U128 vc, vu;
        if (VEC) {
            vc.h = ld_bf16x8(tok + off);
            if (tok_u) vu.h = ld_bf16x8(tok_u + off);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = t.e0 + j;
            if (!VEC && e >= pv) break;
            float f = bf2f(VEC ? vc.e[j] : tok[off + j]);
            if (tok_u) f = cfg_combine(f, bf2f(VEC ? vu.e[j] : tok_u[off + j]), cfg);
            const int64_t pix = tok_pixel(t, e, C, H, W, p);
            D[pix] = sampler_denoised_f32(x_in[pix], f, c_skip, c_out);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// md_measure_residual.  One workgroup per sample (as md_guidance_prepare: 4,096 ... 16,384 elements per sample; a grid-wide reduction
// would need a second launch or atomics).  Per pooled cell, in fp32: a = (sum of its s x s window of D, row by row) / s^2;
// r = m * (meas - a);  q = (-2 * (m * r)) / s^2, written to every pixel of the window;  L_b += double(r * r).  Thread t adds the cells
// of its items in ascending order into one fp64 partial, then a fixed tree over the 256 partials in LDS.
//   plain kernel: item = one cell, any s
//   vector kernel <S> (S = 1, 2, 4; W % 4 == 0, 16-byte aligned D and q): item = S rows of 4 pixels = 4 / S cells, every row of D read
//   and of q written as one 16-byte piece.  Each cell's arithmetic is the plain kernel's; the order in which a thread meets the cells
//   differs, so L_b may differ from the plain kernel's in the last bits of its fp64 sum.
// ---------------------------------------------------------------------------------------------------------------------
struct residual_args {
    const float* D;
    const float* meas;
    const float* mask;      // [mask_B, Hs * Ws] or NULL
    float* q;
    double* L;
    int mask_B, C, H, W, s;
};

__device__ __forceinline__ float residual_cell(float sum, float area, float meas, float m, double& acc) {
    const float r = m * (meas - sum / area);
    acc += (double)(r * r);
    return (-2.f * (m * r)) / area;
}

__device__ __forceinline__ void residual_finish(double acc, double* out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    red[t] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) *out = red[0];
}

__global__ __launch_bounds__(256) void measure_residual_kernel(residual_args a) {
    const int64_t b = blockIdx.x;
    const int s = a.s, Hs = a.H / s, Ws = a.W / s;
    const int64_t cells = (int64_t)a.C * Hs * Ws;
    const float area = (float)(s * s);
    const float* mk = a.mask ? a.mask + (a.mask_B > 1 ? b : 0) * (int64_t)Hs * Ws : nullptr;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < cells; i += 256) {
        const int wp = (int)(i % Ws), hp = (int)((i / Ws) % Hs), c = (int)(i / ((int64_t)Ws * Hs));
        const int64_t base = ((b * a.C + c) * a.H + (int64_t)hp * s) * a.W + (int64_t)wp * s;
        float sum = 0.f;
        for (int r = 0; r < s; ++r)
            for (int k = 0; k < s; ++k) sum += a.D[base + (int64_t)r * a.W + k];
        const float qv = residual_cell(sum, area, a.meas[b * cells + i], mk ? mk[hp * Ws + wp] : 1.f, acc);
        for (int r = 0; r < s; ++r)
            for (int k = 0; k < s; ++k) a.q[base + (int64_t)r * a.W + k] = qv;
    }
    residual_finish(acc, a.L + b);
}

template <int S>
__global__ __launch_bounds__(256) void measure_residual_vec_kernel(residual_args a) {
    constexpr int CPI = 4 / S;                          // pooled cells per item
    const int64_t b = blockIdx.x;
    const int Hs = a.H / S, Ws = a.W / S, ipr = a.W / 4;  // items per pooled row
    const int64_t items = (int64_t)a.C * Hs * ipr, cells = (int64_t)a.C * Hs * Ws;
    const float area = (float)(S * S);
    const float* mk = a.mask ? a.mask + (a.mask_B > 1 ? b : 0) * (int64_t)Hs * Ws : nullptr;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < items; i += 256) {
        const int wi = (int)(i % ipr), hp = (int)((i / ipr) % Hs), c = (int)(i / ((int64_t)ipr * Hs));
        const int64_t base = ((b * a.C + c) * a.H + (int64_t)hp * S) * a.W + (int64_t)wi * 4;
        float sum[CPI];
#pragma unroll
        for (int j = 0; j < CPI; ++j) sum[j] = 0.f;
#pragma unroll
        for (int r = 0; r < S; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(a.D + base + (int64_t)r * a.W);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) sum[k / S] += e[k];
        }
        float qv[CPI];
#pragma unroll
        for (int j = 0; j < CPI; ++j) {
            const int wp = wi * CPI + j;
            const int64_t cell = ((int64_t)c * Hs + hp) * Ws + wp;
            qv[j] = residual_cell(sum[j], area, a.meas[b * cells + cell], mk ? mk[hp * Ws + wp] : 1.f, acc);
        }
        const float4 o = {qv[0], qv[1 / S], qv[2 / S], qv[3 / S]};
#pragma unroll
        for (int r = 0; r < S; ++r) *reinterpret_cast<float4*>(a.q + base + (int64_t)r * a.W) = o;
    }
    residual_finish(acc, a.L + b);
}

// ---------------------------------------------------------------------------------------------------------------------
// md_guide_cotangent_tok: the transpose of md_unpatchify on q, times the weight of each half of the guidance combine and c_out (the
// denoised prediction is c_skip x + c_out (F_u + w (F_c - F_u)), so dL/dF_c = w c_out q and dL/dF_u = (1 - w) c_out q), rounded once to bf16.
// ---------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void guide_cotangent_tok_kernel(const float* q, bf16* dtok, int64_t B, int C, int H, int W, int p, float cfg,
                                                                  int has_uncond, double t_in, float sigma_data) {
    float c_skip, c_out;
    heun_coef(t_in, sigma_data, c_skip, c_out);
    const float wc = has_uncond ? cfg * c_out : c_out, wu = (1.f - cfg) * c_out;
    const int gh = H / p, gw = W / p, pv = C * p * p, nseg = (pv + 7) / 8;
    const int64_t rows = B * gh * gw, total = rows * nseg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const tok_item t = tok_item_of(i, gh, gw, nseg);
        const int64_t off = t.row * pv + t.e0;
        U128 vc, vu;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = t.e0 + j;
            if (!VEC && e >= pv) break;
            const float qv = q[tok_pixel(t, e, C, H, W, p)];
            const bf16 rc = f2bf(wc * qv), ru = f2bf(wu * qv);
            if (VEC) {
                vc.e[j] = rc, vu.e[j] = ru;
            } else {
                dtok[off + j] = rc;
                if (has_uncond) dtok[rows * pv + off + j] = ru;
            }
        }
        if (VEC) {
            st_bf16x8(dtok + off, vc.h);
            if (has_uncond) st_bf16x8(dtok + rows * pv + off, vu.h);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// md_edm_guide_apply: g = c_skip q + c_in (dx_c + dx_u) and the step along it, in the fp64 of the state; c_skip and c_in are the fp32
// values the evaluation ran with (heun_coef, sampler_c_in), widened.  Item = 4 consecutive elements of one sample, or one element.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double guide_step(double x, float q, float dxc, float dxu, double c_skip, double c_in, double coef) {
    return fma(-coef, fma(c_skip, (double)q, c_in * ((double)dxc + (double)dxu)), x);
}

template <bool VEC>
__global__ __launch_bounds__(256) void guide_apply_kernel(double* x_next, const float* q, const float* dx, const float* dxu, const double* L,
                                                          int64_t B, int64_t per, double zeta, double t_in, float sigma_data) {
    float cs, co;
    heun_coef(t_in, sigma_data, cs, co);
    const double c_skip = (double)cs, c_in = (double)sampler_c_in((float)t_in, sigma_data);
    const int64_t n = B * per, items = VEC ? n / 4 : n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int64_t b = (VEC ? 4 * i : i) / per;
        const double coef = zeta / fmax(sqrt(L[b]), MD_GUIDE_TINY);
        if (VEC) {
            double2* xp = reinterpret_cast<double2*>(x_next) + 2 * i;
            double2 xa = xp[0], xb = xp[1];
            const float4 qv = reinterpret_cast<const float4*>(q)[i], dc = reinterpret_cast<const float4*>(dx)[i];
            float4 du = {0.f, 0.f, 0.f, 0.f};
            if (dxu) du = reinterpret_cast<const float4*>(dxu)[i];
            xa.x = guide_step(xa.x, qv.x, dc.x, du.x, c_skip, c_in, coef), xa.y = guide_step(xa.y, qv.y, dc.y, du.y, c_skip, c_in, coef);
            xb.x = guide_step(xb.x, qv.z, dc.z, du.z, c_skip, c_in, coef), xb.y = guide_step(xb.y, qv.w, dc.w, du.w, c_skip, c_in, coef);
            xp[0] = xa, xp[1] = xb;
        } else {
            x_next[i] = guide_step(x_next[i], q[i], dx[i], dxu ? dxu[i] : 0.f, c_skip, c_in, coef);
        }
    }
}

inline bool image_ok(int64_t B, int C, int H, int W) { return B > 0 && C > 0 && H > 0 && W > 0; }
inline bool level_ok(double t_in, float sigma_data) { return std::isfinite(t_in) && t_in > 0 && std::isfinite(sigma_data) && sigma_data > 0; }

}  // namespace

extern "C" int md_edm_denoised(const double* x_in, const float* F, float* D, int64_t B, int64_t per_sample, float cfg, int32_t has_uncond,
                               double t_in, float sigma_data, hipStream_t st) {
    if (!x_in || !F || !D || B <= 0 || per_sample <= 0 || !level_ok(t_in, sigma_data) || !std::isfinite(cfg)) return MD_BAD_ARG;
    const int64_t n = B * per_sample;
    const float* Fu = has_uncond ? F + n : nullptr;
    if (n % 4 == 0 && aligned16(x_in) && aligned16(F) && aligned16(D))      // (n % 4 == 0 and an aligned F: F + n is aligned too)
        hipLaunchKernelGGL(denoised_kernel<true>, dim3(egrid(n / 4)), dim3(256), 0, st, x_in, F, Fu, D, n, cfg, t_in, sigma_data);
    else
        hipLaunchKernelGGL(denoised_kernel<false>, dim3(egrid(n)), dim3(256), 0, st, x_in, F, Fu, D, n, cfg, t_in, sigma_data);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_denoised_tok(const double* x_in, const void* tok_bf16, float* D, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p,
                                   float cfg, int32_t has_uncond, double t_in, float sigma_data, hipStream_t st) {
    if (!x_in || !tok_bf16 || !D || !tok_geometry_ok(B, C, H, W, p) || !level_ok(t_in, sigma_data) || !std::isfinite(cfg))
        return MD_BAD_ARG;
    const int pv = C * p * p;
    const int64_t rows = B * (H / p) * (W / p), items = rows * ((pv + 7) / 8);
    const bf16* tok = (const bf16*)tok_bf16;
    const bf16* tok_u = has_uncond ? tok + rows * pv : nullptr;
    if (pv % 8 == 0 && aligned16(tok) && aligned16(tok_u))
        hipLaunchKernelGGL(denoised_tok_kernel<true>, dim3(egrid(items)), dim3(256), 0, st, x_in, tok, tok_u, D, B, C, H, W, p, cfg, t_in,
                           sigma_data);
    else
        hipLaunchKernelGGL(denoised_tok_kernel<false>, dim3(egrid(items)), dim3(256), 0, st, x_in, tok, tok_u, D, B, C, H, W, p, cfg, t_in,
                           sigma_data);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_measure_residual(const float* D, const float* meas, const float* mask, int32_t mask_B, float* q, double* L, int64_t B,
                                   int32_t C, int32_t H, int32_t W, int32_t s, hipStream_t st) {
    if (!D || !meas || !q || !L || !image_ok(B, C, H, W) || s <= 0 || H % s || W % s || (mask && mask_B != 1 && mask_B != B)) return MD_BAD_ARG;
    const residual_args a = {D, meas, mask, q, L, mask_B, C, H, W, s};
    const bool vec = W % 4 == 0 && aligned16(D) && aligned16(q);
    if (vec && s == 1)
        hipLaunchKernelGGL(measure_residual_vec_kernel<1>, dim3((unsigned)B), dim3(256), 0, st, a);
    else if (vec && s == 2)
        hipLaunchKernelGGL(measure_residual_vec_kernel<2>, dim3((unsigned)B), dim3(256), 0, st, a);
    else if (vec && s == 4)
        hipLaunchKernelGGL(measure_residual_vec_kernel<4>, dim3((unsigned)B), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(measure_residual_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_guide_cotangent_tok(const float* q, void* dtok_bf16, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float cfg,
                                      int32_t has_uncond, double t_in, float sigma_data, hipStream_t st) {
    if (!q || !dtok_bf16 || !tok_geometry_ok(B, C, H, W, p) || !level_ok(t_in, sigma_data) || !std::isfinite(cfg))
        return MD_BAD_ARG;
    const int pv = C * p * p;
    const int64_t rows = B * (H / p) * (W / p), items = rows * ((pv + 7) / 8);
    bf16* dtok = (bf16*)dtok_bf16;
    if (pv % 8 == 0 && aligned16(dtok) && aligned16(dtok + rows * pv))
        hipLaunchKernelGGL(guide_cotangent_tok_kernel<true>, dim3(egrid(items)), dim3(256), 0, st, q, dtok, B, C, H, W, p, cfg, has_uncond,
                           t_in, sigma_data);
    else
        hipLaunchKernelGGL(guide_cotangent_tok_kernel<false>, dim3(egrid(items)), dim3(256), 0, st, q, dtok, B, C, H, W, p, cfg, has_uncond,
                           t_in, sigma_data);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_guide_apply(double* x_next, const float* q, const float* dx, const double* L, int64_t B, int64_t per_sample,
                                  int32_t has_uncond, double zeta, double t_in, float sigma_data, hipStream_t st) {
    if (!x_next || !q || !dx || !L || B <= 0 || per_sample <= 0 || !level_ok(t_in, sigma_data) || !std::isfinite(zeta)) return MD_BAD_ARG;
    const int64_t n = B * per_sample;
    const float* dxu = has_uncond ? dx + n : nullptr;
    if (per_sample % 4 == 0 && aligned16(x_next) && aligned16(q) && aligned16(dx))
        hipLaunchKernelGGL(guide_apply_kernel<true>, dim3(egrid(n / 4)), dim3(256), 0, st, x_next, q, dx, dxu, L, B, per_sample, zeta, t_in,
                           sigma_data);
    else
        hipLaunchKernelGGL(guide_apply_kernel<false>, dim3(egrid(n)), dim3(256), 0, st, x_next, q, dx, dxu, L, B, per_sample, zeta, t_in,
                           sigma_data);
    MD_LAUNCH_CHECK();
    return 0;
}
