// LoRA factored weight-gradient backward ("Factored backward"): the adapter's gradient straight from the backward's
// dy [M, N] and the saved input x [M, K] (bf16, row-major with leading dimensions), without ever forming G = dy^T x:
//   P = x A^T [M, r],  Q = dy B [M, r],  dB += c * dy^T P [N, r],  dA += c * Q^T x [r, K]
// Four launches per call, all on v_mfma_f32_16x16x32_bf16 with fp32 accumulators except the two element-wise ends:
//   prep     A -> Wa [R16][Kp] bf16, B^T -> Wb [R16][Np] bf16 (R16 = max(r, 16): ranks below 16 padded with zero rows; Kp / Np = K / N
//            rounded up to 64, zero-filled): the MFMA operand of the projections, 16 bytes per lane and k-step.
//   proj     grid (Mpad / 32, 2): a workgroup owns 32 rows of x (y = 0) or dy (y = 1); its four waves take the 64-column steps
//            w, w + 4, ... (adjacent 128-byte pieces of the same rows), wave 0 adds the four partial tiles in wave order and stores
//            P^T / Q^T as bf16 [R16][Mpad] (Mpad = M rounded up to 128; rows >= M hold zeros).
//   reduce   grid (column blocks of 128 over dy then x, groups): workgroup (cb, g) owns 128 columns and the row strips g, g + G, ...
//            of 128 rows; wave w takes rows 32 w .. 32 w + 31 of every strip.  A lane loads an 8 row x 8 column block (eight 16-byte
//            loads; a row of the wave's block is 256 contiguous bytes) and picks column c of it as the operand of MFMA c: the
//            transpose dy^T / x^T needs no LDS.  The [R16][128] share stays in registers across the strips; the four waves' shares are
//            added in wave order through LDS and stored to ws [g][R16][Ccat].
//   finish   d_adapter += c * (share 0 + share 1 + ...), ascending.
// DETERMINISTIC: no atomics, one writer per address, every order a function of (M, N, K, rank) alone.  Rows >= M, columns >= N of dy
// and columns >= K of x are never read (their operand elements are zeros); ws needs no initialisation.
#include "md_common.h"
#include "../../include/microdit_hip.h"

namespace {

constexpr int W_STRIP = 128;          // rows of one strip of the reduction (4 waves x 32 rows)
constexpr int W_COLS = 128;           // columns of dy / x one workgroup of the reduction owns
constexpr int W_MAX_GROUPS = 64;      // row groups (shares per output element) at the most
constexpr int W_TARGET_WGS = 1024;    // workgroups of the reduction aimed at: 4 per CU
constexpr int P_ROWS = 32, P_STEP = 64;

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct wgrad_plan {
    int R16, RJ;
    int64_t Mpad, Kp, Np, nbdy, nbx, Ccat, strips, groups;
    int64_t off_w, off_pq, total;     // floats from ws: [shares | Wa, Wb (bf16) | P^T, Q^T (bf16)]
};

bool rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32 || r == 64; }

bool make_plan(int32_t M, int32_t N, int32_t K, int32_t rank, wgrad_plan& p) {
    if (!rank_ok(rank) || M < 1 || N < 1 || K < 8 || K % 8) return false;
    p.R16 = rank < 16 ? 16 : rank;
    p.RJ = p.R16 / 16;
    p.Mpad = ((int64_t)M + W_STRIP - 1) / W_STRIP * W_STRIP;
    p.Kp = ((int64_t)K + P_STEP - 1) / P_STEP * P_STEP;
    p.Np = ((int64_t)N + P_STEP - 1) / P_STEP * P_STEP;
    p.nbdy = ((int64_t)N + W_COLS - 1) / W_COLS;
    p.nbx = ((int64_t)K + W_COLS - 1) / W_COLS;
    p.Ccat = (p.nbdy + p.nbx) * W_COLS;
    p.strips = p.Mpad / W_STRIP;
    int64_t g = W_TARGET_WGS / (p.nbdy + p.nbx);
    g = g < 1 ? 1 : g;
    g = g > W_MAX_GROUPS ? W_MAX_GROUPS : g;
    p.groups = g > p.strips ? p.strips : g;
    p.off_w = p.groups * p.R16 * p.Ccat;
    p.off_pq = p.off_w + p.R16 * (p.Kp + p.Np) / 2;
    p.total = p.off_pq + p.R16 * p.Mpad;
    return true;
}

// Eight bf16 of row `row` from column c on: zeros outside [0, M) x [0, C); a group that straddles C (N need not be a multiple of 8)
// is read element by element, so that nothing past the logical row end is touched.
__device__ __forceinline__ bf16x8 ld_guard(const bf16* src, int64_t ld, int64_t row, int64_t M, int64_t c, int64_t C) {
    U128 t;
    t.u = uint4{0u, 0u, 0u, 0u};
    if (row < M && c < C) {
        const bf16* p = src + row * ld + c;
        if (c + 8 <= C) {
            t.u = *reinterpret_cast<const uint4*>(p);
        } else {
            for (int e = 0; e < 8; ++e)
                if (c + e < C) t.e[e] = p[e];
        }
    }
    return t.h;
}

__global__ __launch_bounds__(256) void wgrad_prep_kernel(const float* A, const float* B, int r, int K, int N, int R16, int64_t Kp, int64_t Np,
                                                         bf16* Wa, bf16* Wb) {
    const int64_t na = (int64_t)R16 * Kp, total = na + (int64_t)R16 * Np;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        if (i < na) {
            const int64_t j = i / Kp, k = i - j * Kp;
            Wa[i] = f2bf(j < r && k < K ? A[j * K + k] : 0.f);
        } else {
            const int64_t i2 = i - na, j = i2 / Np, n = i2 - j * Np;
            Wb[i2] = f2bf(j < r && n < N ? B[n * r + j] : 0.f);
        }
    }
}

// out^T[j, m] = sum_c src[m, c] W[j, c]: the x rows are the MFMA's A operand, the adapter rows its B operand.  Both take k slot
// (q, i) of the two MFMAs of a step from columns 64 s + 16 q + i and 64 s + 16 q + 8 + i: a lane reads 32 contiguous bytes.
template <int RJ>
__global__ __launch_bounds__(256) void wgrad_proj_kernel(const bf16* x, int64_t ldx, int K, const bf16* dy, int64_t lddy, int N, int M,
                                                         int64_t Mpad, const bf16* Wa, int64_t Kp, const bf16* Wb, int64_t Np, bf16* pq) {
    constexpr int E = 2 * RJ * 4;
    __shared__ float red[4 * E * 64];
    const bool is_dy = blockIdx.y == 1;                            // uniform
    const bf16* src = is_dy ? dy : x;
    const int64_t ld = is_dy ? lddy : ldx, C = is_dy ? N : K, Cp = is_dy ? Np : Kp;
    const bf16* W = is_dy ? Wb : Wa;
    bf16* out = pq + (is_dy ? (int64_t)(16 * RJ) * Mpad : 0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, q = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * P_ROWS;
    f32x4 acc[2][RJ];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int jj = 0; jj < RJ; ++jj) acc[rt][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps = (int)(Cp / P_STEP);
    for (int s = w; s < steps; s += 4) {
        const int64_t c = (int64_t)s * P_STEP + 16 * q;
        bf16x8 xa[2], xb[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            xa[rt] = ld_guard(src, ld, m0 + 16 * rt + t, M, c, C);
            xb[rt] = ld_guard(src, ld, m0 + 16 * rt + t, M, c + 8, C);
        }
#pragma unroll
        for (int jj = 0; jj < RJ; ++jj) {
            const bf16* wp = W + (int64_t)(16 * jj + t) * Cp + c;
            const bf16x8 wa = ld_bf16x8(wp), wb = ld_bf16x8(wp + 8);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                acc[rt][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[rt], wa, acc[rt][jj], 0, 0, 0);
                acc[rt][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xb[rt], wb, acc[rt][jj], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int jj = 0; jj < RJ; ++jj)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[((w * E) + (rt * RJ + jj) * 4 + e) * 64 + lane] = acc[rt][jj][e];
    __syncthreads();
    if (w != 0) return;
    // lane (t, q) holds column j = 16 jj + t, rows m0 + 16 rt + 4 q + e of the tile
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int jj = 0; jj < RJ; ++jj) {
            bf16x4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = (rt * RJ + jj) * 4 + e;
                const float v = ((red[i * 64 + lane] + red[(E + i) * 64 + lane]) + red[(2 * E + i) * 64 + lane]) + red[(3 * E + i) * 64 + lane];
                h[e] = f2bf(v);
            }
            st_bf16x4(out + (int64_t)(16 * jj + t) * Mpad + m0 + 16 * rt + 4 * q, h);
        }
}

// share[j, col] = sum over the group's rows m of src[m, col] * other^T[j, m]
template <int RJ>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const bf16* x, int64_t ldx, int K, const bf16* dy, int64_t lddy, int N, int M,
                                                           int64_t Mpad, const bf16* pq, int nbdy, int strips, int64_t Ccat, float* shares) {
    constexpr int E = 8 * RJ * 4;
    __shared__ float red[E * 64];
    const int cb = blockIdx.x, g = blockIdx.y, G = gridDim.y;
    const bool is_dy = cb < nbdy;                                  // uniform
    const bf16* src = is_dy ? dy : x;
    const int64_t ld = is_dy ? lddy : ldx, C = is_dy ? N : K;
    const int64_t c0 = (int64_t)(is_dy ? cb : cb - nbdy) * W_COLS;
    const bf16* other = pq + (is_dy ? 0 : (int64_t)(16 * RJ) * Mpad);   // dB takes P^T, dA takes Q^T
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, q = lane >> 4;
    f32x4 acc[8][RJ];
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int jj = 0; jj < RJ; ++jj) acc[c][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = g; s < strips; s += G) {
        const int64_t mb = (int64_t)s * W_STRIP + 32 * w + 8 * q;  // k slot (q, i) <-> row mb + i, for both operands
        bf16x8 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ld_guard(src, ld, mb + i, M, c0 + 8 * t, C);
        bf16x8 pf[RJ];
#pragma unroll
        for (int jj = 0; jj < RJ; ++jj) pf[jj] = ld_bf16x8(other + (int64_t)(16 * jj + t) * Mpad + mb);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            // column c0 + 8 t + c of the lane's 8 x 8 block: half (c & 1) of dword c / 2 of every row
            U128 f;
            const unsigned sel = (c & 1) ? 0x07060302u : 0x05040100u;
            unsigned d0[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) d0[i] = __builtin_bit_cast(u32x4, v[i])[c >> 1];
            f.u.x = __builtin_amdgcn_perm(d0[1], d0[0], sel);
            f.u.y = __builtin_amdgcn_perm(d0[3], d0[2], sel);
            f.u.z = __builtin_amdgcn_perm(d0[5], d0[4], sel);
            f.u.w = __builtin_amdgcn_perm(d0[7], d0[6], sel);
#pragma unroll
            for (int jj = 0; jj < RJ; ++jj) acc[c][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.h, pf[jj], acc[c][jj], 0, 0, 0);
        }
    }
    // ((wave 0 + wave 1) + wave 2) + wave 3, through one LDS image
#pragma unroll 1
    for (int o = 1; o < 4; ++o) {
        if (w == o) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
#pragma unroll
                for (int jj = 0; jj < RJ; ++jj)
#pragma unroll
                    for (int e = 0; e < 4; ++e) red[((c * RJ + jj) * 4 + e) * 64 + lane] = acc[c][jj][e];
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
#pragma unroll
                for (int jj = 0; jj < RJ; ++jj)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[c][jj][e] += red[((c * RJ + jj) * 4 + e) * 64 + lane];
        }
        __syncthreads();
    }
    if (w != 0) return;
    // lane (t, q): rank row j = 16 jj + t; register e of MFMA c is column 8 (4 q + e) + c of the block: 32 contiguous columns per lane
    float* dst = shares + ((int64_t)g * (16 * RJ)) * Ccat + (int64_t)cb * W_COLS + 32 * q;
#pragma unroll
    for (int jj = 0; jj < RJ; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float* p = dst + (int64_t)(16 * jj + t) * Ccat + 8 * e;
            *reinterpret_cast<f32x4*>(p) = f32x4{acc[0][jj][e], acc[1][jj][e], acc[2][jj][e], acc[3][jj][e]};
            *reinterpret_cast<f32x4*>(p + 4) = f32x4{acc[4][jj][e], acc[5][jj][e], acc[6][jj][e], acc[7][jj][e]};
        }
}

__global__ __launch_bounds__(256) void wgrad_finish_kernel(const float* shares, int G, int R16, int64_t Ccat, int64_t xcol0, int r, int N,
                                                           int K, float coef, float* dA, float* dB) {
    const int64_t nb = (int64_t)r * N, total = nb + (int64_t)r * K, slice = (int64_t)R16 * Ccat;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t j, col;
        float* dst;
        if (i < nb) {
            j = i / N;
            col = i - j * N;
            dst = dB + col * r + j;
        } else {
            const int64_t i2 = i - nb;
            j = i2 / K;
            const int64_t k = i2 - j * K;
            col = xcol0 + k;
            dst = dA + j * K + k;
        }
        const float* src = shares + j * Ccat + col;
        float s = src[0];
        for (int g = 1; g < G; ++g) s += src[g * slice];
        *dst += coef * s;
    }
}

}  // namespace

extern "C" int md_lora_wgrad_ws_floats(int32_t M, int32_t N, int32_t K, int32_t rank, int64_t* out) {
    wgrad_plan p;
    if (!out || !make_plan(M, N, K, rank, p)) return MD_BAD_ARG;
    *out = p.total;
    return 0;
}

extern "C" int md_lora_wgrad_geometry(int32_t M, int32_t N, int32_t K, int32_t rank, int32_t* strip_rows, int32_t* groups) {
    wgrad_plan p;
    if (!strip_rows || !groups || !make_plan(M, N, K, rank, p)) return MD_BAD_ARG;
    *strip_rows = W_STRIP;
    *groups = (int32_t)p.groups;
    return 0;
}

extern "C" int md_lora_wgrad(const void* dy, int32_t lddy, const void* x, int32_t ldx, int32_t M, int32_t N, int32_t K, const float* A,
                             const float* B, int32_t rank, float c, float* dA, float* dB, float* ws, int64_t ws_floats, hipStream_t st) {
    wgrad_plan p;
    if (!dy || !x || !A || !B || !dA || !dB || !ws || !make_plan(M, N, K, rank, p)) return MD_BAD_ARG;
    if (lddy < N || lddy % 8 || ldx < K || ldx % 8 || ws_floats < p.total) return MD_BAD_ARG;
    if (((uintptr_t)dy & 15) || ((uintptr_t)x & 15) || ((uintptr_t)A & 15) || ((uintptr_t)B & 15) || ((uintptr_t)dA & 15) ||
        ((uintptr_t)dB & 15) || ((uintptr_t)ws & 15))
        return MD_BAD_ARG;
    const bf16* dyp = static_cast<const bf16*>(dy);
    const bf16* xp = static_cast<const bf16*>(x);
    bf16* Wa = reinterpret_cast<bf16*>(ws + p.off_w);
    bf16* Wb = Wa + (int64_t)p.R16 * p.Kp;
    bf16* pq = reinterpret_cast<bf16*>(ws + p.off_pq);
    const dim3 bd(256);
    const int64_t nprep = ((int64_t)p.R16 * (p.Kp + p.Np) + 255) / 256;
    hipLaunchKernelGGL(wgrad_prep_kernel, dim3((unsigned)(nprep < 1024 ? nprep : 1024)), bd, 0, st, A, B, (int)rank, (int)K, (int)N, p.R16,
                       p.Kp, p.Np, Wa, Wb);
    MD_LAUNCH_CHECK();
    const dim3 gp((unsigned)(p.Mpad / P_ROWS), 2), gr((unsigned)(p.nbdy + p.nbx), (unsigned)p.groups);
#define MD_WGRAD_LAUNCH(RJ)                                                                                                          \
    hipLaunchKernelGGL(wgrad_proj_kernel<RJ>, gp, bd, 0, st, xp, (int64_t)ldx, (int)K, dyp, (int64_t)lddy, (int)N, (int)M, p.Mpad,   \
                       (const bf16*)Wa, p.Kp, (const bf16*)Wb, p.Np, pq);                                                            \
    MD_LAUNCH_CHECK();                                                                                                               \
    hipLaunchKernelGGL(wgrad_reduce_kernel<RJ>, gr, bd, 0, st, xp, (int64_t)ldx, (int)K, dyp, (int64_t)lddy, (int)N, (int)M, p.Mpad, \
                       (const bf16*)pq, (int)p.nbdy, (int)p.strips, p.Ccat, ws);                                                     \
    MD_LAUNCH_CHECK();
    switch (p.RJ) {
    case 1: MD_WGRAD_LAUNCH(1) break;
    case 2: MD_WGRAD_LAUNCH(2) break;
    default: MD_WGRAD_LAUNCH(4) break;
    }
#undef MD_WGRAD_LAUNCH
    const int64_t nfin = ((int64_t)rank * ((int64_t)N + K) + 255) / 256;
    hipLaunchKernelGGL(wgrad_finish_kernel, dim3((unsigned)(nfin < 1024 ? nfin : 1024)), bd, 0, st, (const float*)ws, (int)p.groups, p.R16,
                       p.Ccat, p.nbdy * W_COLS, (int)rank, (int)N, (int)K, c, dA, dB);
    MD_LAUNCH_CHECK();
    return 0;
}
