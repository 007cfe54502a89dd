// LoRA on the flat buffers: low-rank adapters trained on a frozen base, two table-driven launches per step.
//   md_lora_merge   out_W = p_W + scale * (B A) for every targeted matrix W [N, K] (A [r, K], B [N, r]): the bf16 shadow the engine reads,
//                   or fp32 (out == p: the adapter fused into the masters).  4 B read + 2 B written per weight; A and B are tiny.
//   md_lora_grad    dB = c * G A^T, dA = c * B^T G (c = scale * grad_scale) from the accumulated full gradient G = g_W, added into the
//                   adapter's gradient buffer.  G is read once.
// One work table (md_lora_item, one entry per target) drives both, in the manner of md_tensor_stats_partial: grid.y walks the table,
// grid.x the tiles / row strips of an item (grid-strided: no tile size is assumed to divide rows or cols).
// DETERMINISTIC: no atomics, one writer per address, every sum in an order that is a function of the table alone.
//   merge: thread (tx, ty) of a 64 x 128 tile owns columns 8 tx .. 8 tx + 7 of rows ty + 16 i: acc = fma(B[n,j], A[j,k], acc) for j
//          ascending, v = fma(scale, acc, p).  The bf16 form rounds exactly that v (round to nearest even): the same template, the same
//          instructions, only the store differs.
//   grad:  a workgroup owns a strip of 64 rows over ALL columns, in chunks of 64 columns staged in LDS.  dB[n, j] is a chain of fmas
//          over k ascending held in a register from the first chunk to the last: complete inside the workgroup.  dA[j, k] of the strip is
//          a chain over the strip's rows ascending, stored to the workspace slice [strip][r][cols]; the finish launch adds the slices
//          in ascending strip order, multiplies by c and adds to d_adapter.
// Rows past `rows` and columns past `cols` are never read or written (LDS holds zeros there).
#include "md_common.h"
#include "../../include/microdit_hip.h"

namespace {

constexpr int M_ROWS = 64, M_COLS = 128, M_LDA = M_COLS + 4;       // merge tile; LDS leading dimensions keep 16-byte rows and
constexpr int G_ROWS = 64, G_COLS = 64, G_LD = G_COLS + 4;         // spread the rows one wave reads over distinct bank groups
constexpr int MERGE_GRID_X = 64, GRAD_GRID_X = 256, FINISH_GRID_X = 64;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4_stream(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

template <int R, bool F32OUT>
__global__ __launch_bounds__(256) void lora_merge_kernel(const float* p, const float* adapter, const md_lora_item* items, float scale,
                                                         void* out) {
    constexpr int LDB = R + 4;
    __shared__ __attribute__((aligned(16))) float As[R * M_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[M_ROWS * LDB];
    const md_lora_item it = items[blockIdx.y];                     // uniform
    const int rows = it.rows, cols = it.cols;
    const int nrs = (rows + M_ROWS - 1) / M_ROWS, ncc = (cols + M_COLS - 1) / M_COLS;
    const int ntiles = nrs * ncc;
    const int per = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t0 = (int)blockIdx.x * per;
    const int t1 = t0 + per < ntiles ? t0 + per : ntiles;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const float* A = adapter + it.a_off;
    const float* B = adapter + it.b_off;
    int cur_cc = -1;
    // tiles in column-chunk-major order: the consecutive tiles of a workgroup share their A tile
    for (int t = t0; t < t1; ++t) {
        const int cc = t / nrs, rs = t - cc * nrs;
        const int k0 = cc * M_COLS, n0 = rs * M_ROWS;
        __syncthreads();                                           // the previous tile's LDS reads are done
        if (cc != cur_cc) {
            cur_cc = cc;
            for (int i = tid; i < R * (M_COLS / 4); i += 256) {
                const int j = i / (M_COLS / 4), c = (i % (M_COLS / 4)) * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (k0 + c < cols) v = ld4(A + (int64_t)j * cols + k0 + c);
                st4(As + j * M_LDA + c, v);
            }
        }
        for (int i = tid; i < M_ROWS * (R / 4); i += 256) {
            const int n = i / (R / 4), j = (i % (R / 4)) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (n0 + n < rows) v = ld4(B + (int64_t)(n0 + n) * R + j);
            st4(Bs + n * LDB + j, v);
        }
        __syncthreads();
        const int k = k0 + tx * 8;
        if (k >= cols) continue;                                   // (cols % 8 == 0: a thread's 8 columns are all in or all out)
        f32x4 pv[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + ty + 16 * i;
            if (n < rows) {
                const float* src = p + it.w_off + (int64_t)n * cols + k;
                pv[i][0] = ld4_stream(src);
                pv[i][1] = ld4_stream(src + 4);
            } else {
                pv[i][0] = pv[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        f32x4 acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int j = 0; j < R; j += 4) {
            f32x4 b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = ld4(Bs + (ty + 16 * i) * LDB + j);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const f32x4 a0 = ld4(As + (j + jj) * M_LDA + tx * 8);
                const f32x4 a1 = ld4(As + (j + jj) * M_LDA + tx * 8 + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[i][0][e] = __builtin_fmaf(b[i][jj], a0[e], acc[i][0][e]);
                        acc[i][1][e] = __builtin_fmaf(b[i][jj], a1[e], acc[i][1][e]);
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + ty + 16 * i;
            if (n >= rows) continue;
            f32x4 v0, v1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v0[e] = __builtin_fmaf(scale, acc[i][0][e], pv[i][0][e]);
                v1[e] = __builtin_fmaf(scale, acc[i][1][e], pv[i][1][e]);
            }
            const int64_t o = it.w_off + (int64_t)n * cols + k;
            if (F32OUT) {
                st4(static_cast<float*>(out) + o, v0);
                st4(static_cast<float*>(out) + o + 4, v1);
            } else {
                bf16x8 h;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    h[e] = f2bf(v0[e]);
                    h[4 + e] = f2bf(v1[e]);
                }
                st_bf16x8(static_cast<bf16*>(out) + o, h);
            }
        }
    }
}

template <int R>
__global__ __launch_bounds__(256) void lora_grad_kernel(const float* g, const float* adapter, const md_lora_item* items, float coef,
                                                        float* d_adapter, float* ws) {
    // dB: thread -> row tid / 4 of the strip, ranks (tid % 4) + 4 m;  dA: thread -> columns 4 (tid % 16) .. + 3 of the chunk, ranks
    // (tid / 16) + 16 m.  Below 16 ranks the dA threads of the missing ranks idle.
    constexpr int NB = R / 4, NA = R >= 16 ? R / 16 : 1;
    __shared__ __attribute__((aligned(16))) float Gs[G_ROWS * G_LD];
    __shared__ __attribute__((aligned(16))) float As[R * G_LD];
    __shared__ __attribute__((aligned(16))) float Bs[G_ROWS * R];
    const md_lora_item it = items[blockIdx.y];                     // uniform
    const int rows = it.rows, cols = it.cols;
    const int nstrips = (rows + G_ROWS - 1) / G_ROWS;
    const int tid = threadIdx.x;
    const float* A = adapter + it.a_off;
    const float* B = adapter + it.b_off;
    const int brow = tid >> 2, bj = tid & 3;
    const int ac = (tid & 15) * 4, aj = tid >> 4;
    for (int s = blockIdx.x; s < nstrips; s += gridDim.x) {
        const int n0 = s * G_ROWS;
        __syncthreads();                                           // the previous strip's LDS reads are done
        for (int i = tid; i < G_ROWS * (R / 4); i += 256) {
            const int n = i / (R / 4), j = (i % (R / 4)) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (n0 + n < rows) v = ld4(B + (int64_t)(n0 + n) * R + j);
            st4(Bs + n * R + j, v);
        }
        float db[NB];
#pragma unroll
        for (int m = 0; m < NB; ++m) db[m] = 0.f;
        for (int k0 = 0; k0 < cols; k0 += G_COLS) {
            if (k0) __syncthreads();                               // the previous chunk's LDS reads are done
#pragma unroll
            for (int i = 0; i < G_ROWS * (G_COLS / 4) / 256; ++i) {
                const int q = tid + 256 * i;
                const int n = q / (G_COLS / 4), c = (q % (G_COLS / 4)) * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (n0 + n < rows && k0 + c < cols) v = ld4_stream(g + it.w_off + (int64_t)(n0 + n) * cols + k0 + c);
                st4(Gs + n * G_LD + c, v);
            }
            for (int i = tid; i < R * (G_COLS / 4); i += 256) {
                const int j = i / (G_COLS / 4), c = (i % (G_COLS / 4)) * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (k0 + c < cols) v = ld4(A + (int64_t)j * cols + k0 + c);
                st4(As + j * G_LD + c, v);
            }
            __syncthreads();
            // dB[n, j] += sum_k G[n, k] A[j, k], k ascending
#pragma unroll 4
            for (int k = 0; k < G_COLS; k += 4) {
                const f32x4 gv = ld4(Gs + brow * G_LD + k);
#pragma unroll
                for (int m = 0; m < NB; ++m) {
                    const f32x4 av = ld4(As + (bj + 4 * m) * G_LD + k);
#pragma unroll
                    for (int e = 0; e < 4; ++e) db[m] = __builtin_fmaf(gv[e], av[e], db[m]);
                }
            }
            // dA[j, k] of this strip = sum_n B[n, j] G[n, k], n ascending
            if (aj < R && k0 + ac < cols) {
                f32x4 da[NA];
#pragma unroll
                for (int m = 0; m < NA; ++m) da[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                for (int n = 0; n < G_ROWS; ++n) {
                    const f32x4 gv = ld4(Gs + n * G_LD + ac);
#pragma unroll
                    for (int m = 0; m < NA; ++m) {
                        const float b = Bs[n * R + aj + 16 * m];
#pragma unroll
                        for (int e = 0; e < 4; ++e) da[m][e] = __builtin_fmaf(b, gv[e], da[m][e]);
                    }
                }
#pragma unroll
                for (int m = 0; m < NA; ++m)
                    st4(ws + it.ws_off + ((int64_t)s * R + aj + 16 * m) * cols + k0 + ac, da[m]);
            }
        }
        if (n0 + brow < rows) {
#pragma unroll
            for (int m = 0; m < NB; ++m) {
                float* dst = d_adapter + it.b_off + (int64_t)(n0 + brow) * R + bj + 4 * m;
                *dst += coef * db[m];
            }
        }
    }
}

// d_adapter[A] += coef * (slice 0 + slice 1 + ...), one thread per four columns
__global__ __launch_bounds__(256) void lora_grad_finish_kernel(const md_lora_item* items, int R, float coef, float* d_adapter,
                                                               const float* ws) {
    const md_lora_item it = items[blockIdx.y];
    const int nstrips = (it.rows + G_ROWS - 1) / G_ROWS;
    const int64_t n4 = (int64_t)R * it.cols / 4, slice = (int64_t)R * it.cols;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
        const float* src = ws + it.ws_off + q * 4;
        f32x4 s = ld4(src);
        for (int k = 1; k < nstrips; ++k) s += ld4(src + k * slice);
        float* dst = d_adapter + it.a_off + q * 4;
        f32x4 d = ld4(dst);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] += coef * s[e];
        st4(dst, d);
    }
}

bool rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32 || r == 64; }

// The host mirror of the table: shapes the kernels take, offsets that keep every 16-byte access aligned.
bool items_ok(const md_lora_item* h, int32_t n, int32_t rank) {
    if (!h || n <= 0 || !rank_ok(rank)) return false;
    for (int32_t i = 0; i < n; ++i) {
        if (h[i].rows < 1 || h[i].cols < 8 || h[i].cols % 8) return false;
        if (h[i].w_off < 0 || h[i].w_off % 8 || h[i].a_off < 0 || h[i].a_off % 4 || h[i].b_off < 0 || h[i].b_off % 4) return false;
    }
    return true;
}

int64_t strips_of(const md_lora_item& it) { return ((int64_t)it.rows + G_ROWS - 1) / G_ROWS; }

template <bool F32OUT>
void launch_merge(int rank, dim3 gd, hipStream_t st, const float* p, const float* adapter, const md_lora_item* items, float scale,
                  void* out) {
    const dim3 bd(256);
    switch (rank) {
    case 4: hipLaunchKernelGGL((lora_merge_kernel<4, F32OUT>), gd, bd, 0, st, p, adapter, items, scale, out); break;
    case 8: hipLaunchKernelGGL((lora_merge_kernel<8, F32OUT>), gd, bd, 0, st, p, adapter, items, scale, out); break;
    case 16: hipLaunchKernelGGL((lora_merge_kernel<16, F32OUT>), gd, bd, 0, st, p, adapter, items, scale, out); break;
    case 32: hipLaunchKernelGGL((lora_merge_kernel<32, F32OUT>), gd, bd, 0, st, p, adapter, items, scale, out); break;
    default: hipLaunchKernelGGL((lora_merge_kernel<64, F32OUT>), gd, bd, 0, st, p, adapter, items, scale, out); break;
    }
}

}  // namespace

extern "C" int md_lora_merge(const float* p, const float* adapter, const md_lora_item* items, const md_lora_item* items_host,
                             int32_t n_items, int32_t rank, float scale, void* out, int32_t out_is_f32, hipStream_t st) {
    if (!p || !adapter || !items || !out || !items_ok(items_host, n_items, rank)) return MD_BAD_ARG;
    if (((uintptr_t)p & 15) || ((uintptr_t)adapter & 15) || ((uintptr_t)out & 15)) return MD_BAD_ARG;
    int64_t tiles = 1;
    for (int32_t i = 0; i < n_items; ++i) {
        const int64_t t = (((int64_t)items_host[i].rows + M_ROWS - 1) / M_ROWS) * (((int64_t)items_host[i].cols + M_COLS - 1) / M_COLS);
        if (t > 0x7fffffff) return MD_BAD_ARG;
        tiles = t > tiles ? t : tiles;
    }
    const dim3 gd((unsigned)(tiles < MERGE_GRID_X ? tiles : MERGE_GRID_X), (unsigned)n_items);
    if (out_is_f32) launch_merge<true>(rank, gd, st, p, adapter, items, scale, out);
    else launch_merge<false>(rank, gd, st, p, adapter, items, scale, out);
    MD_LAUNCH_CHECK();
    return 0;
}

extern "C" int md_lora_grad_ws_floats(md_lora_item* items_host, int32_t n_items, int32_t rank, int64_t* out) {
    if (!out || !items_ok(items_host, n_items, rank)) return MD_BAD_ARG;
    int64_t tot = 0;
    for (int32_t i = 0; i < n_items; ++i) {
        items_host[i].ws_off = tot;
        tot += strips_of(items_host[i]) * rank * items_host[i].cols;
    }
    *out = tot;
    return 0;
}

extern "C" int md_lora_grad(const float* g, const float* adapter, const md_lora_item* items, const md_lora_item* items_host,
                            int32_t n_items, int32_t rank, float scale, float grad_scale, float* d_adapter, float* ws, int64_t ws_floats,
                            hipStream_t st) {
    if (!g || !adapter || !items || !d_adapter || !ws || !items_ok(items_host, n_items, rank)) return MD_BAD_ARG;
    if (((uintptr_t)g & 15) || ((uintptr_t)adapter & 15) || ((uintptr_t)d_adapter & 15) || ((uintptr_t)ws & 15)) return MD_BAD_ARG;
    int64_t tot = 0, strips = 1, quads = 1;
    for (int32_t i = 0; i < n_items; ++i) {
        if (items_host[i].ws_off != tot) return MD_BAD_ARG;        // the layout md_lora_grad_ws_floats wrote into the table
        tot += strips_of(items_host[i]) * rank * items_host[i].cols;
        strips = strips_of(items_host[i]) > strips ? strips_of(items_host[i]) : strips;
        const int64_t q = ((int64_t)rank * items_host[i].cols / 4 + 255) / 256;
        quads = q > quads ? q : quads;
    }
    if (ws_floats < tot) return MD_BAD_ARG;
    const float coef = scale * grad_scale;
    const dim3 gd((unsigned)(strips < GRAD_GRID_X ? strips : GRAD_GRID_X), (unsigned)n_items), bd(256);
    switch (rank) {
    case 4: hipLaunchKernelGGL((lora_grad_kernel<4>), gd, bd, 0, st, g, adapter, items, coef, d_adapter, ws); break;
    case 8: hipLaunchKernelGGL((lora_grad_kernel<8>), gd, bd, 0, st, g, adapter, items, coef, d_adapter, ws); break;
    case 16: hipLaunchKernelGGL((lora_grad_kernel<16>), gd, bd, 0, st, g, adapter, items, coef, d_adapter, ws); break;
    case 32: hipLaunchKernelGGL((lora_grad_kernel<32>), gd, bd, 0, st, g, adapter, items, coef, d_adapter, ws); break;
    default: hipLaunchKernelGGL((lora_grad_kernel<64>), gd, bd, 0, st, g, adapter, items, coef, d_adapter, ws); break;
    }
    MD_LAUNCH_CHECK();
    const dim3 gf((unsigned)(quads < FINISH_GRID_X ? quads : FINISH_GRID_X), (unsigned)n_items);
    hipLaunchKernelGGL(lora_grad_finish_kernel, gf, bd, 0, st, items, (int)rank, coef, d_adapter, (const float*)ws);
    MD_LAUNCH_CHECK();
    return 0;
}
