// MXFP8 GEMM for the sampler's block linears:
//
//   C[m, n] = epilogue(sum_k A(m, k) * B(n, k)),   A(m, k) = e4m3(a[m, k]) * 2^(sa[m, k / 32] - 127),  B likewise
//
// Both operands are K-contiguous fp8 (OCP e4m3fn) with one e8m0 scale per 32 consecutive k (md_mx_quant_rows / md_swiglu_fwd_mx write
// them), accumulated in fp32 on v_mfma_scale_f32_16x16x128_f8f6f4: one instruction contracts 128 k of a 16 x 16 output block and
// applies the two block scales in hardware.  Operand map of that instruction (measured with one-hot operands, and held in place by
// tests/test_mxfp8_kernels_gpu.py, whose exact cases give every (row, k-block) its own scale and every operand asymmetric data): lane l
// holds row (l & 15); with g = l >> 4 its VGPRs 0-3 hold k = 16 g ... 16 g + 15 and its VGPRs 4-7 hold k = 64 + 16 g ... 64 + 16 g + 15
// -- NOT 32 consecutive k -- while the scale byte it supplies (byte 0 of its scale operand, op_sel 0) is the one of MX block g,
// k = 32 g ... 32 g + 31.  C/D: col = l & 15, row = 4 * (l >> 4) + reg, as for the bf16 16x16 forms.
//
// Tile: 128 x 128 x 128 per 256-thread workgroup (4 waves, 64 x 64 per wave = 4 x 4 MFMA blocks), register-staged global -> LDS
// prefetch (the loads of k-tile t + 1 -- elements and scale bytes -- are in flight while k-tile t is multiplied), the XCD-aware tile
// order of the bf16 family, its LDS-staged epilogue (16-byte row-contiguous global accesses) and its rounding steps.  All LDS is one
// array.  Rows and columns past M / N are zero-filled on the way in and never written.
#include "md_common.h"
#include "gemm_common.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int TM = 128, TN = 128, TK = 128;
constexpr int PITCH = TK + 16;              // bytes per LDS row: 16 lanes reading 16 bytes of 16 consecutive rows touch 64 distinct banks
constexpr int TILE_BYTES = TM * PITCH;      // 18432
constexpr int SLAB_PITCH = 68;              // floats per row of the epilogue slab [32][64 + 4]
constexpr int SLAB_FLOATS = 32 * SLAB_PITCH;
static_assert(4 * SLAB_FLOATS * 4 <= 2 * TILE_BYTES, "epilogue slabs must fit in the staging LDS");

// The tile order of gemm.hip: workgroup b runs on XCD b % 8; every XCD gets a contiguous range of tiles, walked in groups of
// `group_n` column tiles x all row tiles so that a group's weight sub-panel stays in that XCD's L2.
__device__ __forceinline__ void tile_coords(int bid, int nwg, int ntn, int group_n, int& tm, int& tn) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, j = bid >> 3;
    const int logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    const int ntm = nwg / ntn;
    const int per_group = group_n * ntm;
    const int g = logical / per_group, rem = logical % per_group;
    const int first_n = g * group_n;
    const int gn = (ntn - first_n) < group_n ? (ntn - first_n) : group_n;
    tm = rem / gn;
    tn = first_n + rem % gn;
}

// 128 rows x 128 bytes of a K-contiguous fp8 operand: thread t takes the 16-byte chunk (t & 7) of rows (t >> 3) + 32 i.
__device__ __forceinline__ void load_tile(uint4 (&r)[4], const unsigned char* __restrict__ base, int64_t ld, int64_t r0, int64_t rmax,
                                          int64_t k0, int tid) {
    const int c = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t gr = r0 + (tid >> 3) + 32 * i;
        r[i] = gr < rmax ? *reinterpret_cast<const uint4*>(base + gr * ld + k0 + c * 16) : make_uint4(0, 0, 0, 0);
    }
}
__device__ __forceinline__ void store_tile(const uint4 (&r)[4], unsigned char* s, int tid) {
    const int c = tid & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(s + ((tid >> 3) + 32 * i) * PITCH + c * 16) = r[i];
}
// The scale bytes this lane supplies for k-tile kt: rows row0 + 16 i + (lane & 15), k-block 4 kt + (lane >> 4).  A row past the
// operand gets 127 (2^0; its elements are zero).
__device__ __forceinline__ void load_scales(int (&s)[4], const unsigned char* __restrict__ base, int64_t ld, int64_t row0, int64_t rmax,
                                            int64_t kt, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t gr = row0 + 16 * i + (lane & 15);
        s[i] = gr < rmax ? (int)base[gr * ld + kt * 4 + (lane >> 4)] : 127;
    }
}
__device__ __forceinline__ i32x8 load_frag(const unsigned char* s, int row0, int lane) {
    const unsigned char* p = s + (row0 + (lane & 15)) * PITCH + (lane >> 4) * 16;
    const uint4 lo = *reinterpret_cast<const uint4*>(p), hi = *reinterpret_cast<const uint4*>(p + 64);
    i32x8 f;
    f[0] = (int)lo.x; f[1] = (int)lo.y; f[2] = (int)lo.z; f[3] = (int)lo.w;
    f[4] = (int)hi.x; f[5] = (int)hi.y; f[6] = (int)hi.z; f[7] = (int)hi.w;
    return f;
}

__global__ __launch_bounds__(256) void gemm_mxfp8_kernel(md_gemm_mx_args p, int raster_group_n) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TILE_BYTES];
    unsigned char* sA = smem;
    unsigned char* sB = smem + TILE_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = (int)((p.N + TN - 1) / TN);
    int tile_m, tile_n;
    tile_coords(blockIdx.x, gridDim.x, ntn, raster_group_n, tile_m, tile_n);
    const int64_t m0 = (int64_t)tile_m * TM, n0 = (int64_t)tile_n * TN;
    const int batch = blockIdx.y;
    const unsigned char* A = reinterpret_cast<const unsigned char*>(p.A) + (int64_t)batch * p.sA;
    const unsigned char* B = reinterpret_cast<const unsigned char*>(p.B) + (int64_t)batch * p.sB;
    const unsigned char* SA = reinterpret_cast<const unsigned char*>(p.scaleA) + (int64_t)batch * p.sScaleA;
    const unsigned char* SB = reinterpret_cast<const unsigned char*>(p.scaleB) + (int64_t)batch * p.sScaleB;
    const int nt = (int)(p.K / TK);

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    uint4 ra[4], rb[4];
    int nsa[4], nsb[4], sa[4], sb[4];
    load_tile(ra, A, p.lda, m0, p.M, 0, tid);
    load_tile(rb, B, p.ldb, n0, p.N, 0, tid);
    load_scales(nsa, SA, p.ldsa, m0 + wm * 64, p.M, 0, lane);
    load_scales(nsb, SB, p.ldsb, n0 + wn * 64, p.N, 0, lane);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();   // everyone finished reading the previous tile
        store_tile(ra, sA, tid);
        store_tile(rb, sB, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sa[i] = nsa[i];
            sb[i] = nsb[i];
        }
        __syncthreads();
        if (t + 1 < nt) {
            load_tile(ra, A, p.lda, m0, p.M, (int64_t)(t + 1) * TK, tid);
            load_tile(rb, B, p.ldb, n0, p.N, (int64_t)(t + 1) * TK, tid);
            load_scales(nsa, SA, p.ldsa, m0 + wm * 64, p.M, t + 1, lane);
            load_scales(nsb, SB, p.ldsb, n0 + wn * 64, p.N, t + 1, lane);
        }
        i32x8 fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = load_frag(sA, wm * 64 + i * 16, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = load_frag(sB, wn * 64 + j * 16, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)   // cbsz = blgp = 0: both operands e4m3; op_sel 0: scale in byte 0 of the lane's scale operand
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
    }

    // ---- epilogue: accumulators -> per-wave fp32 slab -> 16-byte row-contiguous global accesses (the steps of gemm.hip's epilogue) ----
    float* slab = reinterpret_cast<float*>(smem) + wave * SLAB_FLOATS;
    const int mode = p.mode;
    const int erow = lane >> 3, ecol = (lane & 7) * 8;
    const int64_t mw0 = m0 + wm * 64, gc = n0 + wn * 64 + ecol;
    const bool col_ok = gc < p.N;
    const bool has_gate = mode == MD_EPI_RESIDUAL && p.gate != nullptr;
    const unsigned rps = has_gate ? (unsigned)p.rows_per_sample : 1u;
    float bv[8];
    if (p.bias && col_ok) {
        const float* bp = reinterpret_cast<const float*>(p.bias) + (int64_t)batch * p.sBias + gc;
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = bp[e];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = 0.f;
    }
    __syncthreads();   // every wave is done reading the staging buffers the slabs alias
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    slab[(ii * 16 + (lane >> 4) * 4 + r) * SLAB_PITCH + j * 16 + (lane & 15)] = acc[mi * 2 + ii][j][r];
        // the slab is private to this wave, whose LDS operations execute in issue order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int lr = it * 8 + erow;
            const int64_t gr = mw0 + mi * 32 + lr;
            if (gr >= p.M || !col_ok) continue;
            float v[8];
            {
                const float4 v0 = *reinterpret_cast<const float4*>(slab + lr * SLAB_PITCH + ecol);
                const float4 v1 = *reinterpret_cast<const float4*>(slab + lr * SLAB_PITCH + ecol + 4);
                v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w;
                v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] + bv[e];
            if (p.C2) {   // the pre-activation / pre-gate value
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
                st_bf16x8(reinterpret_cast<bf16*>(p.C2) + (int64_t)batch * p.sC2 + gr * p.ldc2 + gc, o);
            }
            if (mode == MD_EPI_STORE_BF16) {
                if (p.act != MD_ACT_NONE) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = apply_act(v[e], p.act);
                }
            } else {
                const bf16x8 rs = ld_bf16x8(reinterpret_cast<const bf16*>(p.res) + gr * p.ldr + gc);
                if (has_gate) {
                    const bf16x8 g = ld_bf16x8(reinterpret_cast<const bf16*>(p.gate) + (int64_t)((unsigned)gr / rps) * p.ldg + gc);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = bf2f(rs[e]) + bf2f(g[e]) * bf2f(f2bf(v[e]));
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = bf2f(rs[e]) + bf2f(f2bf(v[e]));
                }
            }
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
            st_bf16x8(reinterpret_cast<bf16*>(p.C) + (int64_t)batch * p.sC + gr * p.ldc + gc, o);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int md_gemm_mxfp8(const md_gemm_mx_args* a, hipStream_t stream) {
    if (!a || !a->A || !a->B || !a->scaleA || !a->scaleB || !a->C) return MD_BAD_ARG;
    if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch <= 0) return MD_BAD_ARG;
    if (a->mode != MD_EPI_STORE_BF16 && a->mode != MD_EPI_RESIDUAL) return MD_BAD_ARG;
    if (a->act != MD_ACT_NONE && a->act != MD_ACT_GELU_ERF) return MD_BAD_ARG;
    if (a->mode == MD_EPI_RESIDUAL && (!a->res || a->act != MD_ACT_NONE || a->batch != 1 || a->ldr % 8 || (a->gate && (a->rows_per_sample <= 0 || a->ldg % 8))))
        return MD_BAD_ARG;
    if (a->mode == MD_EPI_STORE_BF16 && (a->res || a->gate)) return MD_BAD_ARG;
    if (a->N % 16 || a->K % 128) return MD_NOT_ELIGIBLE;          // nothing is launched: the caller runs the bf16 family
    if (a->lda % 16 || a->ldb % 16 || a->lda < a->K || a->ldb < a->K || a->ldsa < a->K / 32 || a->ldsb < a->K / 32) return MD_BAD_ARG;
    if (a->sA % 16 || a->sB % 16 || !aligned16(a->A) || !aligned16(a->B)) return MD_BAD_ARG;
    if (a->ldc % 8 || a->ldc < a->N || (a->C2 && (a->ldc2 % 8 || a->ldc2 < a->N))) return MD_BAD_ARG;
    // every bf16 access of the epilogue is a 16-byte piece: C, C2, res and gate on 16-byte addresses, row and batch pitches of whole pieces
    if (!aligned16(a->C) || a->sC % 8 || (a->C2 && (!aligned16(a->C2) || a->sC2 % 8))) return MD_BAD_ARG;
    if (a->mode == MD_EPI_RESIDUAL && (!aligned16(a->res) || a->ldr < a->N || (a->gate && (!aligned16(a->gate) || a->ldg < a->N)))) return MD_BAD_ARG;
    const int64_t ntm = (a->M + TM - 1) / TM, ntn = (a->N + TN - 1) / TN;
    if (ntm * ntn > 0x7fffffff || a->batch > 65535) return MD_BAD_ARG;
    int64_t g = (2 << 20) / ((int64_t)TN * a->K);   // column tiles per raster group: the group's fp8 weight sub-panel within ~2 MiB of L2
    if (g < 1) g = 1;
    if (g > ntn) g = ntn;
    hipLaunchKernelGGL(gemm_mxfp8_kernel, dim3((unsigned)(ntm * ntn), (unsigned)a->batch), dim3(256), 0, stream, *a, (int)g);
    MD_LAUNCH_CHECK();
    return 0;
}
