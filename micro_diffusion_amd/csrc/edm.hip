// Front / back end of the MicroDiT training step (all fp32 math, HBM-bound, tiny next to the transformer):
//   md_edm_prepare      sigma sampling + noise add + c_in/c_noise (model.py:154-164,182-188)
//   md_patchify         [B,C,H,W] f32 (* per-sample scale) -> bf16 patch rows ordered (c, ph, pw) = the im2col of
//                       timm PatchEmbed's stride-p conv (dit.py:312-314,479); the conv itself is a GEMM.
//   md_timestep_embed   sinusoidal features [cos | sin] (utils.py:266-281)
//   md_unpatchify       (+ unmask_tokens) token rows ordered (ph, pw, c) -> [B,C,H,W] f32 (utils.py:417-426,
//                       dit.py:566-575)
//   md_edm_loss         D = c_skip*xn + c_out*F, weighted SE, mean over the UN-MASKED patches per sample, batch
//                       mean (model.py:177,199-210) and its gradient w.r.t. the kept-token network output.
#include "md_common.h"
#include "sampler_math.h"
#include "sampler_tok.h"
#include "../../include/microdit_hip.h"
#include <cmath>

namespace {

template <typename XT>
__global__ __launch_bounds__(256) void edm_prepare_kernel(const XT* x0, const float* eps, const float* rnd, float* xn,
                                                          float* x0_f32, float* sigma, float* cin, float* cnoise, int64_t B,
                                                          int64_t per, float p_mean, float p_std, float sd) {
    const int64_t total = B * per;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / per;
        const float s = expf(rnd[b] * p_std + p_mean);
        const float x = (float)x0[i];
        xn[i] = x + eps[i] * s;
        if (x0_f32) x0_f32[i] = x;      // the loss reads the clean latents as fp32 (model.py:104-110 casts the fp16 batch once)
        if (i % per == 0) {
            sigma[b] = s;
            cin[b] = 1.f / sqrtf(sd * sd + s * s);
            cnoise[b] = logf(s) * 0.25f;
        }
    }
}

// out[(b*T + ti*gw + tj), c*p*p + ph*p + pw] = x[b, c, ti*p + ph, tj*p + pw] * scale[b]
__global__ __launch_bounds__(256) void patchify_kernel(const float* x, const float* scale, bf16* out, int64_t B, int C,
                                                       int H, int W, int p) {
    const int gh = H / p, gw = W / p, pv = C * p * p;
    const int64_t total = B * gh * gw * pv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int e = (int)(i % pv);
        const int64_t tok = i / pv;
        const int tj = (int)(tok % gw), ti = (int)((tok / gw) % gh);
        const int64_t b = tok / ((int64_t)gw * gh);
        const int c = e / (p * p), ph = (e / p) % p, pw = e % p;
        const float v = x[((b * C + c) * H + ti * p + ph) * W + tj * p + pw];
        out[i] = f2bf(scale ? v * scale[b] : v);
    }
}

__global__ __launch_bounds__(256) void timestep_embed_kernel(const float* t, bf16* out, int64_t B, int dim) {
    const int half = dim / 2;
    const int64_t total = B * half;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / half;
        const int k = (int)(i % half);
        const float f = timestep_freq(k, half);
        const float a = t[b] * f;
        out[b * dim + k] = f2bf(cosf(a));
        out[b * dim + half + k] = f2bf(sinf(a));
    }
}

// image[b, c, ti*p+ph, tj*p+pw] = tok[row(b, ti*gw+tj), (ph*p + pw)*C + c];  masked tokens -> mask_token
__global__ __launch_bounds__(256) void unpatchify_kernel(const bf16* tok, const int32_t* ids_restore, int64_t Tk,
                                                         const float* mask_token, float* img, int64_t B, int C, int H,
                                                         int W, int p) {
    const int gh = H / p, gw = W / p, pv = C * p * p;
    const int64_t T = (int64_t)gh * gw, total = B * C * H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int w = (int)(i % W), hrow = (int)((i / W) % H), c = (int)((i / ((int64_t)W * H)) % C);
        const int64_t b = i / ((int64_t)W * H * C);
        const int ti = hrow / p, ph = hrow % p, tj = w / p, pw = w % p;
        const int64_t t = (int64_t)ti * gw + tj;
        const int e = (ph * p + pw) * C + c;
        float v;
        if (ids_restore) {
            const int rank = ids_restore[b * T + t];
            v = rank < Tk ? bf2f(tok[(b * Tk + rank) * pv + e]) : (mask_token ? mask_token[e] : 0.f);
        } else {
            v = bf2f(tok[(b * T + t) * pv + e]);
        }
        img[i] = v;
    }
}

// One workgroup per sample.  Kept token j of sample b sits at grid position keep_rows[b*Tk + j] - b*T (or j when
// keep_rows is NULL = no masking).  loss_b = mean over kept patches of mean_{c,ph,pw} w * (D - x0)^2;
// dtok = gscale * d(mean_b loss_b)/dF for the kept tokens ([B*Tk, C*p*p], (ph, pw, c) order; f32, or bf16 for the
// training step, whose backward starts from bf16 anyway).  The batch mean is taken by edm_loss_finish_kernel in sample
// order (the first version added the per-sample terms with float atomics: the loss depended on the arrival order).
// WEIGHTED (md_edm_loss_train_weighted): the gradient factor of sample b is (gfac * sample_scale[b]), formed once; the loss outputs
// stay the raw loss.  The unweighted instantiations never read sample_scale (NULL).
template <typename DT, bool WEIGHTED = false>
__global__ __launch_bounds__(256) void edm_loss_kernel(const bf16* tok, const int32_t* keep_rows, const float* xn,
                                                       const float* x0, const float* sigma, float* loss_per_sample,
                                                       DT* dtok, float gscale, int64_t B, int64_t Tk, int C, int H,
                                                       int W, int p, float sd, const float* sample_scale) {
    __shared__ float red[4];
    const int gh = H / p, gw = W / p, pv = C * p * p;
    const int64_t T = (int64_t)gh * gw;
    const int64_t b = blockIdx.x;
    const float s = sigma[b];
    const float wgt = (s * s + sd * sd) / ((s * sd) * (s * sd));
    const float cskip = sd * sd / (s * s + sd * sd);
    const float cout = s * sd / sqrtf(s * s + sd * sd);
    const float norm = 1.f / ((float)pv * (float)Tk);
    float gfac = 2.f * wgt * cout * norm / (float)B * gscale;
    if constexpr (WEIGHTED) gfac = gfac * sample_scale[b];
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < Tk * pv; i += 256) {
        const int64_t j = i / pv;
        const int e = (int)(i % pv);
        const int64_t t = keep_rows ? (int64_t)keep_rows[b * Tk + j] - b * T : j;
        const int ti = (int)(t / gw), tj = (int)(t % gw);
        const int c = e % C, pw = (e / C) % p, ph = e / (C * p);
        const int64_t pix = ((b * C + c) * H + ti * p + ph) * W + tj * p + pw;
        const float F = bf2f(tok[(b * Tk + j) * pv + e]);
        const float D = cskip * xn[pix] + cout * F;
        const float diff = D - x0[pix];
        acc += wgt * diff * diff;
        if (dtok) {
            if constexpr (sizeof(DT) == 4) dtok[(b * Tk + j) * pv + e] = gfac * diff;
            else dtok[(b * Tk + j) * pv + e] = f2bf(gfac * diff);
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss_per_sample[b] = (red[0] + red[1] + red[2] + red[3]) * norm;
}

// loss_mean = (1 / B) sum_b loss_per_sample[b] in a fixed order (one wave: lane-strided partial sums, then the wave
// reduction); optionally loss_accum += accum_weight * loss_mean (the rank-mean loss of a microbatched step).
__global__ __launch_bounds__(64) void edm_loss_finish_kernel(const float* loss_per_sample, float* loss_mean, float* loss_accum,
                                                             float accum_weight, int64_t B) {
    float acc = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 64) acc += loss_per_sample[b];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) {
        const float m = acc / (float)B;
        *loss_mean = m;
        if (loss_accum) *loss_accum += accum_weight * m;
    }
}

// Grid of a 256-thread grid-stride launch over `work` items (tests/test_kernel_geometry_cpu.py reads the cap here; guide.hip keeps the
// same helper).
inline int egrid(int64_t work) {
    int64_t g = (work + 255) / 256;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (int)g;
}

// ---------------------------------------------------------------------------------------------------------------------
// Sampler (model.py:231-297): the arithmetic around each network evaluation of the sampling loop as two fused kernels, with the
// reference's precisions: fp64 sampler state, fp32 preconditioning (model.py:144-179) and fp32 classifier-free-guidance
// combine (dit.py:542-550).
//   sampler_input : net_in = float(c_in(sigma) * float(x)), written once, or twice when the batch is doubled for guidance
//   update        : x_next = Step(x_in, D), D = Source(x_in, network output): one kernel template per layout (update_kernel: fp32 images,
//                   one element per item; update_tok_kernel: bf16 token rows, one 8-element segment per item) behind all twelve
//                   md_edm_{heun,solver}_update[_guide|_coef][_tok] entry points.
//       Source cfg_source : F = Fu + cfg * (Fc - Fu) (Fu NULL: F = Fc);  D = c_skip * float(x_in) + c_out * F
//              coef_source: D = alpha_b * (c_skip * float(x_in) + c_out * Fc) + gamma_b * M                     (guidance modes)
//       Step   heun_step  : d = (x_in - D) / sigma;  first half-step : d_cur = d, x_next = x_hat + (t_next - t_hat) * d
//                                                    second half-step: x_next = x_hat + (t_next - t_hat) * (0.5 d_cur + 0.5 d)
//              solver_step: x_next = a * x_in + b * (c1 * D - c2 * hist);  hist = D                      (Euler, DPM-Solver++(2M))
//   sampler_patchify: sampler_input writing bf16 patch rows
// ---------------------------------------------------------------------------------------------------------------------
// The per-element arithmetic, shared by the image-space and the token-space kernels below (and by guide.hip): sampler_math.h.
// The combine of the guidance modes, in the space of the denoised value: D = alpha_b * D_c + gamma_b * M with D_c the
// conditional prediction, M the running difference md_guidance_prepare left in the layout of the state and (alpha_b, gamma_b) the
// per-sample coefficients it formed.  fp32 like the preconditioning, widened to the fp64 of the state.
__device__ __forceinline__ double sampler_guided(double xi, float fc, float m, float c_skip, float c_out, float alpha, float gamma) {
    return (double)fmaf(alpha, sampler_denoised_f32(xi, fc, c_skip, c_out), gamma * m);
}
// Returns x_next of one element from its denoised value D; d receives the slope of this evaluation (the first half-step stores it as
// d_cur), d_prev is the d_cur the second half-step reads.  Values in, values out: the callers load before they store, so x_next may
// alias x_in or x_hat.
__device__ __forceinline__ double heun_from_denoised(double xi, double xh, double D, double t_in, double t_hat, double t_next, int second,
                                                     double d_prev, double& d) {
    d = (xi - D) / t_in;
    if (!second) return fma(t_next - t_hat, d, xh);
    return fma(t_next - t_hat, fma(0.5, d, 0.5 * d_prev), xh);
}

// One step of a linear multistep solver on the denoised value (Euler, DPM-Solver++(2M)): x_next = a * x_in + b * (c1 * den - c2 * hist);
// den goes back to the caller, which stores it as the next step's hist.  hist is 0.0 when c2 == 0 (the callers do not load it then),
// so c1 * den - c2 * hist is c1 * den exactly and a stale or non-finite history buffer never reaches x_next.
__device__ __forceinline__ double solver_from_denoised(double xi, double den, double a, double b, double c1, double c2, double hist) {
    return fma(a, xi, b * fma(c1, den, -(c2 * hist)));
}

__global__ __launch_bounds__(256) void sampler_input_kernel(const double* x, float* out, int64_t n, float sigma, float sigma_data, int dup) {
    const float c_in = sampler_c_in(sigma, sigma_data);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = sampler_net_in(c_in, x[i]);
        out[i] = v;
        if (dup) out[n + i] = v;
    }
}

// x_hat = x + coef * noise: the stochastic churn of model.py:258, coef = sqrt(t_hat^2 - t_cur^2) * S_noise from the host.
__global__ __launch_bounds__(256) void churn_kernel(const double* x, const double* noise, double* x_hat, int64_t n, double coef) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x_hat[i] = fma(coef, noise[i], x[i]);
}

// patches[row, c*p*p + ph*p + pw] = bf16(c_in * float(x[b, c, ti*p+ph, tj*p+pw]));  rows [B*T, 2*B*T) repeat them when dup
template <bool VEC>
__global__ __launch_bounds__(256) void sampler_patchify_kernel(const double* x, bf16* out, int64_t B, int C, int H, int W, int p,
                                                               float sigma, float sigma_data, int dup) {
    const float c_in = sampler_c_in(sigma, sigma_data);
    const int gh = H / p, gw = W / p, pp = p * p, pv = C * pp, nseg = (pv + 7) / 8;
    const int64_t rows = B * gh * gw, total = rows * nseg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const tok_item t = tok_item_of(i, gh, gw, nseg);
        U128 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = t.e0 + j;
            if (!VEC && e >= pv) break;
            const int c = e / pp, ph = (e / p) % p, pw = e % p;
            const bf16 r = f2bf(sampler_net_in(c_in, x[((t.b * C + c) * H + t.ti * p + ph) * W + t.tj * p + pw]));
            if (VEC) {
                v.e[j] = r;
            } else {
                out[t.row * pv + e] = r;
                if (dup) out[(rows + t.row) * pv + e] = r;
            }
        }
        if (VEC) {
            st_bf16x8(out + t.row * pv + t.e0, v.h);
            if (dup) st_bf16x8(out + (rows + t.row) * pv + t.e0, v.h);
        }
    }
}

// The update kernels: x_next = Step(x_in, D) with D = Source(x_in, network output).  Source and Step are small structs passed by value;
// all arithmetic goes through sampler_math.h and the functions above, so every form of a step gives the same bits by construction.
// FT is the type of the network output: float (image layout) or bf16 (token rows; a token row holds the elements of its patch in
// (ph, pw, c) order, tok_pixel).  In the token layout a Source keeps what it loads for one item in its `segment`.
__device__ __forceinline__ float f32_of(float v) { return v; }
__device__ __forceinline__ float f32_of(bf16 v) { return bf2f(v); }

// The guidance combine of two network outputs.  The second operand is a pointer of its own (NULL: no combine): the unconditional half
// of a doubled batch (fc + n, the has_uncond entry points) or the output of a second, weaker network (the _guide entry points).
template <typename FT>
struct cfg_source {
    const FT *fc, *fu;
    float cfg;
    struct segment {
        const FT *pc, *pu;
        U128 vc, vu;
    };
    bool aligned() const { return aligned16(fc) && aligned16(fu); }
    __device__ __forceinline__ double flat(int64_t i, double xi, float c_skip, float c_out) const {
        float f = f32_of(fc[i]);
        if (fu) f = cfg_combine(f, f32_of(fu[i]), cfg);
        return sampler_denoised(xi, f, c_skip, c_out);
    }
    template <bool VEC>
    __device__ __forceinline__ void load_segment(segment& s, const tok_item& t, int pv) const {
        const int64_t off = t.row * pv + t.e0;
        s.pc = fc + off;
        s.pu = fu ? fu + off : s.pc;
        if (VEC) {
            s.vc.h = ld_bf16x8(s.pc);
            if (fu) s.vu.h = ld_bf16x8(s.pu);
        }
    }
    __device__ __forceinline__ void load_pixel(segment&, int, int64_t) const {}
    template <bool VEC>
    __device__ __forceinline__ double denoised(const segment& s, int j, double xi, float c_skip, float c_out) const {
        float f = bf2f(VEC ? s.vc.e[j] : s.pc[j]);
        if (fu) f = cfg_combine(f, bf2f(VEC ? s.vu.e[j] : s.pu[j]), cfg);
        return sampler_denoised(xi, f, c_skip, c_out);
    }
};

// The coefficient form of the guidance modes: M and the per-sample (alpha_b, gamma_b) of md_guidance_prepare, both in the layout of the
// state whatever the layout of fc.  per: elements of one sample (the image layout finds its sample with it).
template <typename FT>
struct coef_source {
    const FT* fc;
    const float *M, *coef;
    int64_t per;
    struct segment {
        const FT* pc;
        U128 vc;
        float alpha, gamma, m[8];
    };
    bool aligned() const { return aligned16(fc); }
    __device__ __forceinline__ double flat(int64_t i, double xi, float c_skip, float c_out) const {
        const int64_t b = i / per;
        return sampler_guided(xi, f32_of(fc[i]), M[i], c_skip, c_out, coef[b * 2], coef[b * 2 + 1]);
    }
    template <bool VEC>
    __device__ __forceinline__ void load_segment(segment& s, const tok_item& t, int pv) const {
        s.pc = fc + t.row * pv + t.e0;
        s.alpha = coef[t.b * 2], s.gamma = coef[t.b * 2 + 1];
        if (VEC) s.vc.h = ld_bf16x8(s.pc);
    }
    __device__ __forceinline__ void load_pixel(segment& s, int j, int64_t pix) const { s.m[j] = M[pix]; }
    template <bool VEC>
    __device__ __forceinline__ double denoised(const segment& s, int j, double xi, float c_skip, float c_out) const {
        return sampler_guided(xi, bf2f(VEC ? s.vc.e[j] : s.pc[j]), s.m[j], c_skip, c_out, s.alpha, s.gamma);
    }
};

// A Step loads its per-pixel state (load) and stores x_next and its own output (apply).  d_cur is read only by the second half-step
// and hist only when c2 != 0, so a stale or non-finite buffer never reaches x_next.
struct heun_step {
    const double* x_hat;
    double* d_cur;
    double t_hat, t_next;
    int second;
    struct state {
        double xh, dp;
    };
    __device__ __forceinline__ state load(int64_t i) const { return {x_hat[i], second ? d_cur[i] : 0.0}; }
    __device__ __forceinline__ void apply(int64_t i, double xi, double D, const state& s, double t_in, double* x_next) const {
        double d;
        x_next[i] = heun_from_denoised(xi, s.xh, D, t_in, t_hat, t_next, second, s.dp, d);
        if (!second) d_cur[i] = d;
    }
};

struct solver_step {
    double* hist;
    double a, b, c1, c2;
    struct state {
        double hp;
    };
    __device__ __forceinline__ state load(int64_t i) const { return {c2 != 0.0 ? hist[i] : 0.0}; }
    __device__ __forceinline__ void apply(int64_t i, double xi, double D, const state& s, double, double* x_next) const {
        x_next[i] = solver_from_denoised(xi, D, a, b, c1, c2, s.hp);
        hist[i] = D;
    }
};

// Per item, every load comes before the first store, so x_next may alias x_in or x_hat.
template <typename Source, typename Step>
__global__ __launch_bounds__(256) void update_kernel(Source src, Step step, const double* x_in, double* x_next, int64_t n, double t_in,
                                                     float sigma_data) {
    float c_skip, c_out;
    heun_coef(t_in, sigma_data, c_skip, c_out);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double xi = x_in[i];
        const double D = src.flat(i, xi, c_skip, c_out);
        const typename Step::state s = step.load(i);
        step.apply(i, xi, D, s, t_in, x_next);
    }
}

// (The geometry is formed here from the five sizes, in scalar registers: handed over as a tok_geometry argument, the solver
// instantiations took 2-3 more VGPRs, one occupancy step.)
template <bool VEC, typename Source, typename Step>
__global__ __launch_bounds__(256) void update_tok_kernel(Source src, Step step, const double* x_in, double* x_next, int64_t B, int C, int H,
                                                         int W, int p, double t_in, float sigma_data) {
    const tok_geometry g = tok_geometry_of(B, C, H, W, p);
    float c_skip, c_out;
    heun_coef(t_in, sigma_data, c_skip, c_out);
    const int64_t total = g.items();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const tok_item t = tok_item_of(i, g.gh, g.gw, g.nseg);
        typename Source::segment seg;
        src.template load_segment<VEC>(seg, t, g.pv);
        int64_t pix[8];
        double xi[8];
        typename Step::state s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {          // every load of the item before its first store
            const int e = t.e0 + j;
            if (!VEC && e >= g.pv) break;
            pix[j] = tok_pixel(t, e, g.C, g.H, g.W, g.p);
            xi[j] = x_in[pix[j]];
            s[j] = step.load(pix[j]);
            src.load_pixel(seg, j, pix[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!VEC && t.e0 + j >= g.pv) break;
            step.apply(pix[j], xi[j], src.template denoised<VEC>(seg, j, xi[j], c_skip, c_out), s[j], t_in, x_next);
        }
    }
}

// One launcher per layout (arguments checked by the callers).  The token form takes the 16-byte path only when the row width is a
// multiple of 8 and EVERY token pointer of the source is 16-byte aligned: one misaligned pointer sends the whole launch element by
// element, so it is never read as a vector.
template <typename Source, typename Step>
int launch_update(Source src, Step step, const double* x_in, double* x_next, int64_t n, double t_in, float sigma_data, hipStream_t st) {
    hipLaunchKernelGGL((update_kernel<Source, Step>), dim3(egrid(n)), dim3(256), 0, st, src, step, x_in, x_next, n, t_in, sigma_data);
    MD_LAUNCH_CHECK();
    return 0;
}

template <typename Source, typename Step>
int launch_update_tok(Source src, Step step, const double* x_in, double* x_next, const tok_geometry& g, double t_in, float sigma_data,
                      hipStream_t st) {
    if (g.pv % 8 == 0 && src.aligned())
        hipLaunchKernelGGL((update_tok_kernel<true, Source, Step>), dim3(egrid(g.items())), dim3(256), 0, st, src, step, x_in, x_next, g.B,
                           g.C, g.H, g.W, g.p, t_in, sigma_data);
    else
        hipLaunchKernelGGL((update_tok_kernel<false, Source, Step>), dim3(egrid(g.items())), dim3(256), 0, st, src, step, x_in, x_next, g.B,
                           g.C, g.H, g.W, g.p, t_in, sigma_data);
    MD_LAUNCH_CHECK();
    return 0;
}

// The second operand of the has_uncond entry points: the unconditional half of the doubled batch, or none.
template <typename FT>
cfg_source<FT> cfg_pair(const void* F, int64_t n, float cfg, int has_uncond) {
    return {(const FT*)F, has_uncond ? (const FT*)F + n : nullptr, cfg};
}

// ---------------------------------------------------------------------------------------------------------------------
// Guidance modes: CFG rescale and adaptive projected guidance need per-sample reductions over the denoised prediction,
// so a guided evaluation is two launches: guidance_prepare_kernel (M, the five moments, alpha_b and gamma_b) and one of the _coef update
// entry points, which are the update kernels above with coef_source (D = alpha_b * D_c + gamma_b * M) in place of the cfg combine.
// ---------------------------------------------------------------------------------------------------------------------
struct guidance_args {
    int mode, first, has_r;             // MD_GUIDANCE_*; first: M holds nothing yet (not read); has_r: the norm threshold r is set
    double w, phi, eta, r;
    float beta;
};

// One workgroup per sample.  Thread t takes the image-layout elements t, t + 256, ... of its sample in that order, five fp64 partial
// sums each, then a fixed tree over the 256 partials in LDS; thread 0 forms the coefficients.  The order of every addition depends
// on the image-layout element index alone: the token form (TOK) differs only in where it finds F of that element, so the two forms
// give the same bits, and so do two calls.  The fp64 products of two fp32 values are exact.  M_prev is read and M written by the
// same work item.  D_c - D_u is formed as c_out * (F_c - F_u): c_skip * x is the same in both and cancels, and the difference of the two
// fp32 D would carry the rounding of that term, which is of the size of D, not of M, and comes back (w - 1) times in the result.  n per sample is 4,096 ... 16,384 here (16 ... 64 rounds): a grid-wide reduction would need a second launch or
// atomics for less than a microsecond of arithmetic.
template <bool TOK>
__global__ __launch_bounds__(256) void guidance_prepare_kernel(const double* x_in, const void* Fc, const void* Fu, float* M, float* coef,
                                                               double* moments, int64_t per, int C, int H, int W, int p, double t_in,
                                                               float sigma_data, guidance_args g) {
    __shared__ double red[5][256];
    float c_skip, c_out;
    heun_coef(t_in, sigma_data, c_skip, c_out);
    const int64_t b = blockIdx.x;
    const bool read_m = g.mode == MD_GUIDANCE_APG && !g.first && g.beta != 0.f;
    double sc = 0.0, sm = 0.0, qcc = 0.0, qmm = 0.0, qcm = 0.0;
    for (int64_t i = threadIdx.x; i < per; i += 256) {
        const int64_t pix = b * per + i;
        float fc, fu;
        if (TOK) {
            const int gw = W / p, w = (int)(i % W), hrow = (int)((i / W) % H), c = (int)(i / ((int64_t)W * H));
            const int64_t row = (b * (H / p) + hrow / p) * gw + w / p;
            const int64_t off = row * ((int64_t)C * p * p) + ((hrow % p) * p + w % p) * C + c;
            fc = bf2f(((const bf16*)Fc)[off]);
            fu = bf2f(((const bf16*)Fu)[off]);
        } else {
            fc = ((const float*)Fc)[pix];
            fu = ((const float*)Fu)[pix];
        }
        const double xi = x_in[pix];
        const float dc = sampler_denoised_f32(xi, fc, c_skip, c_out);
        float m = c_out * (fc - fu);            // D_c - D_u without its cancelling c_skip * x (see above)
        if (read_m) m = fmaf(g.beta, M[pix], m);
        M[pix] = m;
        const double dcd = (double)dc, md = (double)m;
        sc += dcd;
        sm += md;
        qcc = fma(dcd, dcd, qcc);
        qmm = fma(md, md, qmm);
        qcm = fma(dcd, md, qcm);
    }
    const int t = threadIdx.x;
    red[0][t] = sc, red[1][t] = sm, red[2][t] = qcc, red[3][t] = qmm, red[4][t] = qcm;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < 5; ++k) red[k][t] += red[k][t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double S_c = red[0][0], S_m = red[1][0], Q_cc = red[2][0], Q_mm = red[3][0], Q_cm = red[4][0];
    double* mo = moments + b * 5;
    mo[0] = S_c, mo[1] = S_m, mo[2] = Q_cc, mo[3] = Q_mm, mo[4] = Q_cm;
    const double w1 = g.w - 1.0;
    double alpha, gamma;
    if (g.mode == MD_GUIDANCE_APG) {
        const double s = g.has_r && Q_mm > 0.0 ? fmin(1.0, g.r / sqrt(Q_mm)) : 1.0;
        const double pr = Q_cc > 0.0 ? s * Q_cm / Q_cc : 0.0;
        alpha = 1.0 - w1 * (1.0 - g.eta) * pr;
        gamma = w1 * s;
    } else {
        const double n = (double)per;
        const double var_c = fmax(Q_cc / n - (S_c / n) * (S_c / n), 0.0);     // a constant D_c can round below zero
        const double S_g = S_c + w1 * S_m;
        const double var_g = (Q_cc + 2.0 * w1 * Q_cm + w1 * w1 * Q_mm) / n - (S_g / n) * (S_g / n);
        const double k = var_g > 0.0 ? g.phi * sqrt(var_c / var_g) + 1.0 - g.phi : 1.0;
        alpha = k;
        gamma = k * w1;
    }
    coef[b * 2] = (float)alpha;
    coef[b * 2 + 1] = (float)gamma;
}

// Everything md_guidance_prepare(_tok) refuses about the mode and its parameters; the comparisons are written so that a NaN fails them.
inline bool guidance_args_ok(int mode, double w, double phi, double eta, int has_r, double r, double beta) {
    if (mode != MD_GUIDANCE_RESCALE && mode != MD_GUIDANCE_APG) return false;
    if (!std::isfinite(w) || !std::isfinite(phi) || !std::isfinite(eta) || !std::isfinite(r) || !std::isfinite(beta)) return false;
    if (!(phi >= 0.0 && phi <= 1.0)) return false;
    if (has_r && !(r > 0.0)) return false;
    return std::fabs(beta) < 1.0;
}

inline guidance_args make_guidance_args(int mode, double w, double phi, double eta, int has_r, double r, double beta, int first) {
    guidance_args g;
    g.mode = mode, g.first = first, g.has_r = has_r;
    g.w = w, g.phi = phi, g.eta = eta, g.r = r;
    g.beta = mode == MD_GUIDANCE_APG ? (float)beta : 0.f;      // rescale keeps no momentum
    return g;
}

}  // namespace

extern "C" int md_edm_prepare(const float* x0, const float* eps, const float* rnd, float* xn, float* sigma, float* cin,
                              float* cnoise, int64_t B, int64_t per_sample, float p_mean, float p_std, float sigma_data,
                              hipStream_t st) {
    if (!x0 || !eps || !rnd || !xn || !sigma || !cin || !cnoise || B <= 0 || per_sample <= 0) return MD_BAD_ARG;
    hipLaunchKernelGGL(edm_prepare_kernel<float>, dim3(egrid(B * per_sample)), dim3(256), 0, st, x0, eps, rnd, xn, (float*)nullptr,
                       sigma, cin, cnoise, B, per_sample, p_mean, p_std, sigma_data);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_prepare_f16(const void* x0_f16, const float* eps, const float* rnd, float* xn, float* x0_f32, float* sigma,
                                  float* cin, float* cnoise, int64_t B, int64_t per_sample, float p_mean, float p_std,
                                  float sigma_data, hipStream_t st) {
    if (!x0_f16 || !eps || !rnd || !xn || !x0_f32 || !sigma || !cin || !cnoise || B <= 0 || per_sample <= 0) return MD_BAD_ARG;
    hipLaunchKernelGGL(edm_prepare_kernel<_Float16>, dim3(egrid(B * per_sample)), dim3(256), 0, st, (const _Float16*)x0_f16, eps,
                       rnd, xn, x0_f32, sigma, cin, cnoise, B, per_sample, p_mean, p_std, sigma_data);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_patchify(const float* x, const float* scale, void* out, int64_t B, int32_t C, int32_t H, int32_t W,
                           int32_t p, hipStream_t st) {
    if (!x || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || p <= 0 || H % p || W % p) return MD_BAD_ARG;
    hipLaunchKernelGGL(patchify_kernel, dim3(egrid(B * C * H * W)), dim3(256), 0, st, x, scale, (bf16*)out, B, C, H, W, p);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_timestep_embed(const float* t, void* out, int64_t B, int32_t dim, hipStream_t st) {
    if (!t || !out || B <= 0 || dim <= 0 || dim % 2) return MD_BAD_ARG;
    hipLaunchKernelGGL(timestep_embed_kernel, dim3(egrid(B * dim / 2)), dim3(256), 0, st, t, (bf16*)out, B, dim);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_unpatchify(const void* tok, const int32_t* ids_restore, int64_t Tk, const float* mask_token, float* img,
                             int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, hipStream_t st) {
    if (!tok || !img || B <= 0 || C <= 0 || H % p || W % p || (ids_restore && Tk <= 0)) return MD_BAD_ARG;
    hipLaunchKernelGGL(unpatchify_kernel, dim3(egrid(B * C * H * W)), dim3(256), 0, st, (const bf16*)tok, ids_restore, Tk,
                       mask_token, img, B, C, H, W, p);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_loss(const void* tok, const int32_t* keep_rows, const float* xn, const float* x0, const float* sigma,
                           float* loss_per_sample, float* loss_mean, float* dtok, int64_t B, int64_t Tk, int32_t C,
                           int32_t H, int32_t W, int32_t p, float sigma_data, hipStream_t st) {
    if (!tok || !xn || !x0 || !sigma || !loss_per_sample || !loss_mean || B <= 0 || Tk <= 0 || H % p || W % p)
        return MD_BAD_ARG;
    hipLaunchKernelGGL(edm_loss_kernel<float>, dim3((unsigned)B), dim3(256), 0, st, (const bf16*)tok, keep_rows, xn, x0, sigma,
                       loss_per_sample, dtok, 1.f, B, Tk, C, H, W, p, sigma_data, (const float*)nullptr);
    hipLaunchKernelGGL(edm_loss_finish_kernel, dim3(1), dim3(64), 0, st, loss_per_sample, loss_mean, (float*)nullptr, 0.f, B);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_loss_train(const void* tok, const int32_t* keep_rows, const float* xn, const float* x0, const float* sigma,
                                 float* loss_per_sample, float* loss_mean, void* dtok_bf16, float grad_scale, float* loss_accum,
                                 float accum_weight, int64_t B, int64_t Tk, int32_t C, int32_t H, int32_t W, int32_t p,
                                 float sigma_data, hipStream_t st) {
    if (!tok || !xn || !x0 || !sigma || !loss_per_sample || !loss_mean || !dtok_bf16 || B <= 0 || Tk <= 0 || H % p || W % p)
        return MD_BAD_ARG;
    hipLaunchKernelGGL(edm_loss_kernel<bf16>, dim3((unsigned)B), dim3(256), 0, st, (const bf16*)tok, keep_rows, xn, x0, sigma,
                       loss_per_sample, (bf16*)dtok_bf16, grad_scale, B, Tk, C, H, W, p, sigma_data, (const float*)nullptr);
    hipLaunchKernelGGL(edm_loss_finish_kernel, dim3(1), dim3(64), 0, st, loss_per_sample, loss_mean, loss_accum, accum_weight, B);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_loss_train_weighted(const void* tok, const int32_t* keep_rows, const float* xn, const float* x0,
                                          const float* sigma, float* loss_per_sample, float* loss_mean, void* dtok_bf16,
                                          float grad_scale, float* loss_accum, float accum_weight, int64_t B, int64_t Tk, int32_t C,
                                          int32_t H, int32_t W, int32_t p, float sigma_data, const float* sample_scale, hipStream_t st) {
    if (!tok || !xn || !x0 || !sigma || !loss_per_sample || !loss_mean || !dtok_bf16 || !sample_scale || B <= 0 || Tk <= 0 || H % p ||
        W % p)
        return MD_BAD_ARG;
    hipLaunchKernelGGL((edm_loss_kernel<bf16, true>), dim3((unsigned)B), dim3(256), 0, st, (const bf16*)tok, keep_rows, xn, x0, sigma,
                       loss_per_sample, (bf16*)dtok_bf16, grad_scale, B, Tk, C, H, W, p, sigma_data, sample_scale);
    hipLaunchKernelGGL(edm_loss_finish_kernel, dim3(1), dim3(64), 0, st, loss_per_sample, loss_mean, loss_accum, accum_weight, B);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_sampler_input(const double* x, float* out, int64_t n, float sigma, float sigma_data, int32_t duplicate,
                                    hipStream_t st) {
    if (!x || !out || n <= 0) return MD_BAD_ARG;
    hipLaunchKernelGGL(sampler_input_kernel, dim3(egrid(n)), dim3(256), 0, st, x, out, n, sigma, sigma_data, duplicate);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_sampler_patchify(const double* x, void* patches_bf16, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p,
                                       float sigma, float sigma_data, int32_t duplicate, hipStream_t st) {
    if (!x || !patches_bf16 || !tok_geometry_ok(B, C, H, W, p)) return MD_BAD_ARG;
    const tok_geometry g = tok_geometry_of(B, C, H, W, p);
    const int64_t items = g.items();
    if (g.pv % 8 == 0 && aligned16(patches_bf16))
        hipLaunchKernelGGL(sampler_patchify_kernel<true>, dim3(egrid(items)), dim3(256), 0, st, x, (bf16*)patches_bf16, B, C, H, W, p,
                           sigma, sigma_data, duplicate);
    else
        hipLaunchKernelGGL(sampler_patchify_kernel<false>, dim3(egrid(items)), dim3(256), 0, st, x, (bf16*)patches_bf16, B, C, H, W, p,
                           sigma, sigma_data, duplicate);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_edm_churn(const double* x, const double* noise, double* x_hat, int64_t n, double coef, hipStream_t st) {
    if (!x || !noise || !x_hat || n <= 0) return MD_BAD_ARG;
    hipLaunchKernelGGL(churn_kernel, dim3(egrid(n)), dim3(256), 0, st, x, noise, x_hat, n, coef);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_guidance_prepare(const double* x_in, const float* F_c, const float* F_u, float* M, float* coef, double* moments, int64_t B,
                                   int64_t per_sample, double t_in, float sigma_data, int32_t mode, double w, double rescale_phi,
                                   double apg_eta, int32_t has_norm_threshold, double apg_norm_threshold, double apg_momentum, int32_t first,
                                   hipStream_t st) {
    if (!x_in || !F_c || !F_u || !M || !coef || !moments || B <= 0 || per_sample <= 0 || !(t_in > 0) ||
        !guidance_args_ok(mode, w, rescale_phi, apg_eta, has_norm_threshold, apg_norm_threshold, apg_momentum))
        return MD_BAD_ARG;
    hipLaunchKernelGGL(guidance_prepare_kernel<false>, dim3((unsigned)B), dim3(256), 0, st, x_in, (const void*)F_c, (const void*)F_u, M, coef,
                       moments, per_sample, 0, 0, 0, 0, t_in, sigma_data,
                       make_guidance_args(mode, w, rescale_phi, apg_eta, has_norm_threshold, apg_norm_threshold, apg_momentum, first));
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_guidance_prepare_tok(const double* x_in, const void* tok_bf16, const void* tok_u_bf16, float* M, float* coef,
                                       double* moments, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, double t_in, float sigma_data,
                                       int32_t mode, double w, double rescale_phi, double apg_eta, int32_t has_norm_threshold,
                                       double apg_norm_threshold, double apg_momentum, int32_t first, hipStream_t st) {
    if (!x_in || !tok_bf16 || !tok_u_bf16 || !M || !coef || !moments || !tok_geometry_ok(B, C, H, W, p) || !(t_in > 0) ||
        !guidance_args_ok(mode, w, rescale_phi, apg_eta, has_norm_threshold, apg_norm_threshold, apg_momentum))
        return MD_BAD_ARG;
    hipLaunchKernelGGL(guidance_prepare_kernel<true>, dim3((unsigned)B), dim3(256), 0, st, x_in, tok_bf16, tok_u_bf16, M, coef, moments,
                       (int64_t)C * H * W, C, H, W, p, t_in, sigma_data,
                       make_guidance_args(mode, w, rescale_phi, apg_eta, has_norm_threshold, apg_norm_threshold, apg_momentum, first));
    MD_LAUNCH_CHECK();
    return 0;
}

// The twelve update entry points: {heun, solver} x {cfg pair in one buffer, cfg pair in two (_guide), coefficient form (_coef)} x {image,
// _tok}.  Each checks its arguments and makes one launch_update(_tok) call; a time that is not positive (NaN included) is refused.
extern "C" int md_edm_heun_update(const double* x_hat, const double* x_in, const float* F, double* d_cur, double* x_next, int64_t n,
                                  float cfg, int32_t has_uncond, double t_in, double t_hat, double t_next, float sigma_data,
                                  int32_t second, hipStream_t st) {
    if (!x_hat || !x_in || !F || !d_cur || !x_next || n <= 0 || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update(cfg_pair<float>(F, n, cfg, has_uncond), heun_step{x_hat, d_cur, t_hat, t_next, second}, x_in, x_next, n, t_in,
                         sigma_data, st);
}

extern "C" int md_edm_heun_update_guide(const double* x_hat, const double* x_in, const float* F, const float* F_guide, double* d_cur,
                                        double* x_next, int64_t n, float cfg, double t_in, double t_hat, double t_next, float sigma_data,
                                        int32_t second, hipStream_t st) {
    if (!x_hat || !x_in || !F || !F_guide || !d_cur || !x_next || n <= 0 || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update(cfg_source<float>{F, F_guide, cfg}, heun_step{x_hat, d_cur, t_hat, t_next, second}, x_in, x_next, n, t_in, sigma_data,
                         st);
}

extern "C" int md_edm_heun_update_coef(const double* x_hat, const double* x_in, const float* F_c, const float* M, const float* coef,
                                       double* d_cur, double* x_next, int64_t B, int64_t per_sample, double t_in, double t_hat, double t_next,
                                       float sigma_data, int32_t second, hipStream_t st) {
    if (!x_hat || !x_in || !F_c || !M || !coef || !d_cur || !x_next || B <= 0 || per_sample <= 0 || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update(coef_source<float>{F_c, M, coef, per_sample}, heun_step{x_hat, d_cur, t_hat, t_next, second}, x_in, x_next,
                         B * per_sample, t_in, sigma_data, st);
}

extern "C" int md_edm_heun_update_tok(const double* x_hat, const double* x_in, const void* tok_bf16, double* d_cur, double* x_next,
                                      int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float cfg, int32_t has_uncond, double t_in,
                                      double t_hat, double t_next, float sigma_data, int32_t second, hipStream_t st) {
    if (!x_hat || !x_in || !tok_bf16 || !d_cur || !x_next || !tok_geometry_ok(B, C, H, W, p) || !(t_in > 0)) return MD_BAD_ARG;
    const tok_geometry g = tok_geometry_of(B, C, H, W, p);
    return launch_update_tok(cfg_pair<bf16>(tok_bf16, g.rows() * g.pv, cfg, has_uncond), heun_step{x_hat, d_cur, t_hat, t_next, second}, x_in,
                             x_next, g, t_in, sigma_data, st);
}

extern "C" int md_edm_heun_update_guide_tok(const double* x_hat, const double* x_in, const void* tok_bf16, const void* tok_guide_bf16,
                                            double* d_cur, double* x_next, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float cfg,
                                            double t_in, double t_hat, double t_next, float sigma_data, int32_t second, hipStream_t st) {
    if (!x_hat || !x_in || !tok_bf16 || !tok_guide_bf16 || !d_cur || !x_next || !tok_geometry_ok(B, C, H, W, p) || !(t_in > 0))
        return MD_BAD_ARG;
    return launch_update_tok(cfg_source<bf16>{(const bf16*)tok_bf16, (const bf16*)tok_guide_bf16, cfg},
                             heun_step{x_hat, d_cur, t_hat, t_next, second}, x_in, x_next, tok_geometry_of(B, C, H, W, p), t_in, sigma_data, st);
}

extern "C" int md_edm_heun_update_coef_tok(const double* x_hat, const double* x_in, const void* tok_bf16, const float* M, const float* coef,
                                           double* d_cur, double* x_next, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, double t_in,
                                           double t_hat, double t_next, float sigma_data, int32_t second, hipStream_t st) {
    if (!x_hat || !x_in || !tok_bf16 || !M || !coef || !d_cur || !x_next || !tok_geometry_ok(B, C, H, W, p) || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update_tok(coef_source<bf16>{(const bf16*)tok_bf16, M, coef, (int64_t)C * H * W}, heun_step{x_hat, d_cur, t_hat, t_next, second},
                             x_in, x_next, tok_geometry_of(B, C, H, W, p), t_in, sigma_data, st);
}

extern "C" int md_edm_solver_update(const double* x_in, const float* F, double* hist, double* x_next, int64_t n, float cfg,
                                    int32_t has_uncond, double t_in, float sigma_data, double a, double b, double c1, double c2,
                                    hipStream_t st) {
    if (!x_in || !F || !hist || !x_next || n <= 0 || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update(cfg_pair<float>(F, n, cfg, has_uncond), solver_step{hist, a, b, c1, c2}, x_in, x_next, n, t_in, sigma_data, st);
}

extern "C" int md_edm_solver_update_guide(const double* x_in, const float* F, const float* F_guide, double* hist, double* x_next, int64_t n,
                                          float cfg, double t_in, float sigma_data, double a, double b, double c1, double c2,
                                          hipStream_t st) {
    if (!x_in || !F || !F_guide || !hist || !x_next || n <= 0 || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update(cfg_source<float>{F, F_guide, cfg}, solver_step{hist, a, b, c1, c2}, x_in, x_next, n, t_in, sigma_data, st);
}

extern "C" int md_edm_solver_update_coef(const double* x_in, const float* F_c, const float* M, const float* coef, double* hist, double* x_next,
                                         int64_t B, int64_t per_sample, double t_in, float sigma_data, double a, double b, double c1, double c2,
                                         hipStream_t st) {
    if (!x_in || !F_c || !M || !coef || !hist || !x_next || B <= 0 || per_sample <= 0 || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update(coef_source<float>{F_c, M, coef, per_sample}, solver_step{hist, a, b, c1, c2}, x_in, x_next, B * per_sample, t_in,
                         sigma_data, st);
}

extern "C" int md_edm_solver_update_tok(const double* x_in, const void* tok_bf16, double* hist, double* x_next, int64_t B, int32_t C,
                                        int32_t H, int32_t W, int32_t p, float cfg, int32_t has_uncond, double t_in, float sigma_data,
                                        double a, double b, double c1, double c2, hipStream_t st) {
    if (!x_in || !tok_bf16 || !hist || !x_next || !tok_geometry_ok(B, C, H, W, p) || !(t_in > 0)) return MD_BAD_ARG;
    const tok_geometry g = tok_geometry_of(B, C, H, W, p);
    return launch_update_tok(cfg_pair<bf16>(tok_bf16, g.rows() * g.pv, cfg, has_uncond), solver_step{hist, a, b, c1, c2}, x_in, x_next, g, t_in,
                             sigma_data, st);
}

extern "C" int md_edm_solver_update_guide_tok(const double* x_in, const void* tok_bf16, const void* tok_guide_bf16, double* hist,
                                              double* x_next, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float cfg, double t_in,
                                              float sigma_data, double a, double b, double c1, double c2, hipStream_t st) {
    if (!x_in || !tok_bf16 || !tok_guide_bf16 || !hist || !x_next || !tok_geometry_ok(B, C, H, W, p) || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update_tok(cfg_source<bf16>{(const bf16*)tok_bf16, (const bf16*)tok_guide_bf16, cfg}, solver_step{hist, a, b, c1, c2}, x_in,
                             x_next, tok_geometry_of(B, C, H, W, p), t_in, sigma_data, st);
}

extern "C" int md_edm_solver_update_coef_tok(const double* x_in, const void* tok_bf16, const float* M, const float* coef, double* hist,
                                             double* x_next, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, double t_in,
                                             float sigma_data, double a, double b, double c1, double c2, hipStream_t st) {
    if (!x_in || !tok_bf16 || !M || !coef || !hist || !x_next || !tok_geometry_ok(B, C, H, W, p) || !(t_in > 0)) return MD_BAD_ARG;
    return launch_update_tok(coef_source<bf16>{(const bf16*)tok_bf16, M, coef, (int64_t)C * H * W}, solver_step{hist, a, b, c1, c2}, x_in, x_next,
                             tok_geometry_of(B, C, H, W, p), t_in, sigma_data, st);
}

