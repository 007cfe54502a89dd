// Input gradients: the last step of the hand-written backward to each of the three network inputs.
//   md_patch_embed_dgrad     dL/d(embedded tokens) [B*T, D] bf16 -> dL/d(image) [B,C,H,W] f32 in one launch: the transpose of
//                            md_patchify(scale) + the x_embedder.proj GEMM (dit.py:479).  A [rows, D] x [D, patch_vec] product
//                            with patch_vec = 16 or 64: bound by the one read of dtok, so the kernel is built around that read.
//   md_timestep_embed_bwd    dL/d(sinusoidal features) [B, dim] bf16 -> dL/dt [B] f32 (utils.py:266-281)
//   md_cast_rows_from_bf16   dL/d(bf16 caption rows) -> f32 | f16 rows times the per-sample factor: the transpose of md_cast_rows_bf16
// No atomics anywhere: every output element has one writer and a fixed summation order, so a second call gives the same bits.
#include "md_common.h"
#include "../../include/microdit_hip.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 frag8;

constexpr int PED_KC = 256;            // contraction elements of W staged in LDS per pass
constexpr int PED_LDW = PED_KC + 8;    // bf16 pitch of a column of the transposed LDS image (16-byte aligned, odd in 16-byte units)
constexpr int PED_STEPS = PED_KC / 32; // MFMA k-steps per pass

// MFMA path, patch_vec = 16 NT.  A workgroup owns 64 token rows, wave w the 16 rows from 16 w: its A operand of
// v_mfma_f32_16x16x32_bf16 (lane l: row l & 15, k = 8 (l >> 4) + j, j < 8) is one 16-byte global load per lane and k-step, straight
// from dtok -- every byte of dtok is read exactly once by the whole grid.  The B operand (lane l: column l & 15, the same eight k)
// needs W [D, patch_vec] transposed: per pass of PED_KC rows of W, a thread loads an 8 x 8 block as eight 16-byte rows, transposes
// it in registers and writes eight 16-byte LDS rows of sW [patch_vec][PED_LDW].  The A fragments of the NEXT pass are requested
// before the MFMAs of this one, so the global read never waits for the staging barriers.  (Measured and dropped: two or one wave per
// workgroup -- no faster at patch_vec 16, 1.6x / 2.4x slower at 64; the next pass's block of W prefetched in registers too -- 32 more
// VGPRs, a workgroup less per CU, 3-28 % slower except on inputs far larger than the Infinity Cache.)
// C / D layout: column l & 15, row 4 (l >> 4) + reg.  Rows >= M: loads are clamped to row M - 1 (valid memory), nothing is stored.
template <int NT>
__global__ __launch_bounds__(256) void patch_embed_dgrad_mfma_kernel(const bf16* __restrict__ dtok, int64_t ldd,
                                                                     const bf16* __restrict__ Wt, const float* __restrict__ scale,
                                                                     float* __restrict__ dx, int64_t M, int D, int C, int H, int Wd,
                                                                     int p) {
    constexpr int PV = NT * 16;
    __shared__ __attribute__((aligned(16))) bf16 sW[PV * PED_LDW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * 64 + wave * 16;
    int64_t arow = row0 + r;
    if (arow >= M) arow = M - 1;
    const bf16* ap = dtok + arow * ldd + 8 * g;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    frag8 a[PED_STEPS];
    auto load_a = [&](frag8 (&dst)[PED_STEPS], int k0) {
#pragma unroll
        for (int kk = 0; kk < PED_STEPS; ++kk) {
            const int k = k0 + kk * 32 + 8 * g;           // D % 8 == 0: a group of eight lies inside the row or behind it
            U128 t;
            t.u = k < D ? *reinterpret_cast<const uint4*>(ap + k0 + kk * 32) : make_uint4(0, 0, 0, 0);
            dst[kk] = t.h;
        }
    };
    load_a(a, 0);
    for (int k0 = 0; k0 < D; k0 += PED_KC) {
        __syncthreads();                                  // the previous pass has read sW
        for (int blk = tid; blk < (PED_KC / 8) * (PV / 8); blk += 256) {
            const int nb = blk % (PV / 8), kb = blk / (PV / 8);
            U128 in[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = k0 + kb * 8 + i;
                in[i].u = k < D ? *reinterpret_cast<const uint4*>(Wt + (int64_t)k * PV + nb * 8) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                U128 o;
#pragma unroll
                for (int i = 0; i < 8; ++i) o.e[i] = in[i].e[n];
                *reinterpret_cast<uint4*>(sW + (nb * 8 + n) * PED_LDW + kb * 8) = o.u;
            }
        }
        __syncthreads();
        frag8 an[PED_STEPS];
        const bool more = k0 + PED_KC < D;                // uniform
        if (more) load_a(an, k0 + PED_KC);
#pragma unroll
        for (int kk = 0; kk < PED_STEPS; ++kk) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                U128 b;
                b.u = *reinterpret_cast<const uint4*>(sW + (nt * 16 + r) * PED_LDW + kk * 32 + 8 * g);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk], b.h, acc[nt], 0, 0, 0);
            }
        }
        if (more) {
#pragma unroll
            for (int kk = 0; kk < PED_STEPS; ++kk) a[kk] = an[kk];
        }
    }
    // dx[b, c, ti p + ph, tj p + pw] = scale[b] * dpatch[row, c p p + ph p + pw]
    const int gw = Wd / p, pp = p * p;
    const int64_t T = (int64_t)(H / p) * gw;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t row = row0 + 4 * g + reg;
        if (row >= M) continue;
        const int64_t b = row / T;
        const int t = (int)(row - b * T);
        const int ti = t / gw, tj = t - ti * gw;
        const float sc = scale ? scale[b] : 1.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int j = nt * 16 + r;
            const int c = j / pp, ph = (j - c * pp) / p, pw = j % p;
            const float v = acc[nt][reg];
            dx[((b * C + c) * H + ti * p + ph) * Wd + tj * p + pw] = scale ? v * sc : v;
        }
    }
}

// Plain path (every patch_vec <= MD_PATCH_EMBED_DGRAD_MAX_PV, no alignment asked of dtok or W): thread (row, j) of a workgroup of
// floor(256 / patch_vec) rows adds dtok[row, d] * W[d, j] in ascending d with fp32 FMAs; W goes through LDS a pass of PED_KC rows at a
// time in its own layout (threads j, j + 1 read adjacent elements).
__global__ __launch_bounds__(256) void patch_embed_dgrad_fma_kernel(const bf16* __restrict__ dtok, int64_t ldd, const bf16* __restrict__ Wt,
                                                                    const float* __restrict__ scale, float* __restrict__ dx, int64_t M,
                                                                    int D, int pv, int C, int H, int Wd, int p) {
    __shared__ bf16 sW[PED_KC * MD_PATCH_EMBED_DGRAD_MAX_PV];
    const int tid = threadIdx.x;
    const int rpb = 256 / pv;
    const int rl = tid / pv, j = tid - rl * pv;
    const int64_t row = (int64_t)blockIdx.x * rpb + rl;
    const bool live = rl < rpb && row < M;
    const bf16* ap = dtok + (live ? row : 0) * ldd;
    float acc = 0.f;
    for (int k0 = 0; k0 < D; k0 += PED_KC) {
        const int kn = D - k0 < PED_KC ? D - k0 : PED_KC;
        __syncthreads();
        for (int i = tid; i < kn * pv; i += 256) sW[i] = Wt[(int64_t)k0 * pv + i];
        __syncthreads();
        if (live)
            for (int k = 0; k < kn; ++k) acc = fmaf(bf2f(ap[k0 + k]), bf2f(sW[k * pv + j]), acc);
    }
    if (!live) return;
    const int gw = Wd / p, pp = p * p;
    const int64_t T = (int64_t)(H / p) * gw;
    const int64_t b = row / T;
    const int t = (int)(row - b * T);
    const int ti = t / gw, tj = t - ti * gw;
    const int c = j / pp, ph = (j - c * pp) / p, pw = j % p;
    dx[((b * C + c) * H + ti * p + ph) * Wd + tj * p + pw] = scale ? acc * scale[b] : acc;
}

// One wave per sample: lane l adds its frequencies l, l + 64, ... in ascending order, wave_sum adds the 64 lane sums in its fixed order.
__global__ __launch_bounds__(256) void timestep_embed_bwd_kernel(const float* __restrict__ t, const bf16* __restrict__ dout,
                                                                 float* __restrict__ dt, int64_t B, int dim) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                   // a whole wave
    const int half = dim / 2;
    const float tb = t[b];
    const bf16* d = dout + b * dim;
    float s = 0.f;
    for (int k = lane; k < half; k += 64) {
        const float f = timestep_freq(k, half);
        const float a = tb * f;
        s += f * (cosf(a) * bf2f(d[half + k]) - sinf(a) * bf2f(d[k]));     // [cos | sin]: d cos = -sin, d sin = cos
    }
    s = wave_sum(s);
    if (lane == 0) dt[b] = s;
}

template <typename OUT>
__global__ __launch_bounds__(256) void cast_rows_from_bf16_kernel(const bf16* __restrict__ x, OUT* __restrict__ y, int64_t rows, int64_t C,
                                                                  const float* __restrict__ rowscale, int64_t rps) {
    const int64_t total = rows * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const float v = bf2f(x[i]);
        y[i] = (OUT)(rowscale ? v * rowscale[(i / C) / rps] : v);
    }
}

}  // namespace

extern "C" int md_patch_embed_dgrad(const void* dtok, int64_t ld_dtok, const void* w, const float* scale, float* dx, int64_t B, int32_t C,
                                    int32_t H, int32_t W, int32_t p, int32_t D, int32_t* path, hipStream_t st) {
    if (!dtok || !w || !dx || B <= 0 || C <= 0 || H <= 0 || W <= 0 || p <= 0 || D <= 0 || H % p || W % p || D % 8 || ld_dtok < D)
        return MD_BAD_ARG;
    const int64_t pv64 = (int64_t)C * p * p;
    if (pv64 > MD_PATCH_EMBED_DGRAD_MAX_PV) return MD_BAD_ARG;
    const int pv = (int)pv64;
    const int64_t M = B * (H / p) * (W / p);
    const bf16* a = reinterpret_cast<const bf16*>(dtok);
    const bf16* wt = reinterpret_cast<const bf16*>(w);
    const bool mfma = pv % 16 == 0 && ld_dtok % 8 == 0 && !((uintptr_t)dtok & 15) && !((uintptr_t)w & 15);
    if (path) *path = mfma ? 1 : 0;
    if (mfma) {
        const dim3 grid((unsigned)((M + 63) / 64)), block(256);
        switch (pv / 16) {
            case 1: hipLaunchKernelGGL(patch_embed_dgrad_mfma_kernel<1>, grid, block, 0, st, a, ld_dtok, wt, scale, dx, M, D, C, H, W, p); break;
            case 2: hipLaunchKernelGGL(patch_embed_dgrad_mfma_kernel<2>, grid, block, 0, st, a, ld_dtok, wt, scale, dx, M, D, C, H, W, p); break;
            case 3: hipLaunchKernelGGL(patch_embed_dgrad_mfma_kernel<3>, grid, block, 0, st, a, ld_dtok, wt, scale, dx, M, D, C, H, W, p); break;
            default: hipLaunchKernelGGL(patch_embed_dgrad_mfma_kernel<4>, grid, block, 0, st, a, ld_dtok, wt, scale, dx, M, D, C, H, W, p); break;
        }
    } else {
        const int rpb = 256 / pv;
        hipLaunchKernelGGL(patch_embed_dgrad_fma_kernel, dim3((unsigned)((M + rpb - 1) / rpb)), dim3(256), 0, st, a, ld_dtok, wt, scale, dx,
                           M, D, pv, C, H, W, p);
    }
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_timestep_embed_bwd(const float* t, const void* dout, float* dt, int64_t B, int32_t dim, hipStream_t st) {
    if (!t || !dout || !dt || B <= 0 || dim <= 0 || dim % 2) return MD_BAD_ARG;
    hipLaunchKernelGGL(timestep_embed_bwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, t, reinterpret_cast<const bf16*>(dout),
                       dt, B, dim);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_cast_rows_from_bf16(const void* x, void* y, int32_t y_dtype /*0 = f16, 1 = f32*/, int64_t rows, int64_t C,
                                      const float* rowscale, int64_t rows_per_sample, hipStream_t st) {
    if (!x || !y || rows <= 0 || C <= 0 || (y_dtype != 0 && y_dtype != 1) || (rowscale && rows_per_sample <= 0)) return MD_BAD_ARG;
    const int64_t blocks64 = (rows * C + 255) / 256;
    const dim3 grid((unsigned)(blocks64 < 65536 ? blocks64 : 65536));
    if (y_dtype == 0)
        hipLaunchKernelGGL(cast_rows_from_bf16_kernel<_Float16>, grid, dim3(256), 0, st, reinterpret_cast<const bf16*>(x),
                           reinterpret_cast<_Float16*>(y), rows, C, rowscale, rows_per_sample);
    else
        hipLaunchKernelGGL(cast_rows_from_bf16_kernel<float>, grid, dim3(256), 0, st, reinterpret_cast<const bf16*>(x),
                           reinterpret_cast<float*>(y), rows, C, rowscale, rows_per_sample);
    MD_LAUNCH_CHECK();
    return 0;
}
