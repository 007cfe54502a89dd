/* microdit_hip.h — C ABI of libmicrodit_hip.so: the MI355X (gfx950) kernels of the MicroDiT training path.
 *
 * The reference (SonyResearch/micro_diffusion) has no FFI layer: every kernel it runs is reached implicitly
 * through PyTorch ATen / cuBLAS / SDPA from micro_diffusion/models/{dit,utils,model}.py.  This header is the
 * boundary a maintainer binds instead (ctypes stub in INTEGRATION.md).  Each entry cites the reference code
 * whose implicit kernels it replaces.
 *
 * Conventions
 *  - every function returns int: 0 = ok, -1 = bad argument, otherwise the hipError_t of the failed launch;
 *    nothing throws across the ABI.
 *  - all memory is owned by the caller (PyTorch): arguments are raw device pointers, explicit sizes / strides
 *    in ELEMENTS as int64_t, and an explicit hipStream_t.  No allocation, no synchronisation inside.
 *  - re-entrant, no global or thread-local state on host or device (no environment reads, no device globals):
 *    safe to call from the autograd worker thread.
 *  - "bf16" pointers are device uint16 storage of bfloat16; "f32" are float.
 */
#ifndef MICRODIT_HIP_H
#define MICRODIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#define MD_ABI_VERSION 6
int md_abi_version(void);

/* ------------------------------------------------------------------------------------------------ GEMM */
enum md_act { MD_ACT_NONE = 0, MD_ACT_GELU_TANH = 1, MD_ACT_GELU_ERF = 2, MD_ACT_SILU = 3 };

enum md_epilogue {
    MD_EPI_STORE_BF16 = 0, /* C = bf16(act(alpha*acc + bias)); optional C2 = bf16(alpha*acc + bias)            */
    MD_EPI_RESIDUAL = 1,   /* C = bf16(res + gate[row / rows_per_sample, col] * (alpha*acc + bias)); opt. C2   */
    MD_EPI_STORE_F32 = 2,  /* C(f32)  = alpha*acc + bias                                                       */
    MD_EPI_ACCUM_F32 = 3,  /* C(f32) += alpha*acc + bias   (single writer per element)                         */
    MD_EPI_ATOMIC_F32 = 4, /* atomicAdd(C(f32), alpha*acc) (split-K weight gradients)                          */
    MD_EPI_DACT = 5,       /* C = bf16(alpha*acc * act'(aux))  (dgrad through an activation)                   */
    MD_EPI_SWIGLU_BWD = 6  /* ABI 6: the SwiGLU backward (dit.py:88-89) fused into the w3 data gradient da = dy W3: aux = h12
                              [M, 2N] (ldaux), C = dh12 [M, 2N] (ldc); with g = bf16(acc): C[:, n] = g * h2 * silu'(h1),
                              C[:, N + n] = g * silu(h1).  Built into the 4-wave kernel only (A K-contiguous, M % 256 == N % 256
                              == 0, no cu_limit): any other problem returns MD_NOT_ELIGIBLE and launches nothing -- the caller
                              then runs the plain data gradient + md_swiglu_bwd.                                  */
};

/* C[m,n] (+)= alpha * sum_k A(m,k) * B(n,k).  a_kcontig: A(m,k) = A[m*lda + k], else A[k*lda + m]; same for B
 * with n.  Replaces nn.Linear / einsum GEMMs: dit.py:84-89 (SwiGLU), dit.py:131-142 (MoE experts, batch = 8
 * experts), dit.py:222-225 (adaLN), utils.py:58-61, 109-111, 172-173, 225-233, and their autograd backward. */
/* One problem of a grouped launch (md_gemm_args.problems): C_p[M, N] = A_p B_p^T with the launch's K, ksplit and operand layouts.
 * The fp32 result of split s goes to C + s * sSplit + c_off (dense rows of N): the slices of a group mirror the layout of the
 * gradient tensors they are reduced into, so ONE md_splitk_reduce_flat call per contiguous run finishes the whole group. */
typedef struct md_gemm_problem {
    const void* A;
    const void* B;
    int64_t lda, ldb;
    int64_t M, N;
    int64_t c_off;   /* elements, multiple of 4 */
} md_gemm_problem;
#define MD_GEMM_MAX_PROBLEMS 8

typedef struct md_gemm_args {
    const void* A;      /* bf16 */
    const void* B;      /* bf16 */
    void* C;            /* bf16 or f32 depending on mode */
    void* C2;           /* optional bf16 second output (STORE_BF16 / RESIDUAL) */
    const void* bias;   /* optional f32 [N] */
    const void* res;    /* RESIDUAL: bf16 [M, ldr] */
    const void* gate;   /* RESIDUAL: optional bf16 [M / rows_per_sample, ldg] */
    const void* aux;    /* DACT: bf16 [M, ldaux] pre-activation */
    int64_t M, N, K;
    int64_t lda, ldb, ldc, ldc2, ldr, ldg, ldaux;
    int64_t sA, sB, sC, sC2, sBias, sAux; /* batch strides (elements) */
    int64_t sSplit;                       /* STORE_F32 with ksplit > 1: split s writes its partial at C + s * sSplit; ignored by every
                                             other mode (ATOMIC_F32 splits all add into C).  K is cut in whole 64-wide k-tiles,
                                             ceil(tiles / ksplit) per split: the last split may be shorter, and a split left without
                                             work (K = 64, ksplit = 3) still WRITES its slice (alpha * 0 + bias: zeros) */
    int64_t rows_per_sample;
    int32_t batch;
    int32_t ksplit;
    int32_t a_kcontig, b_kcontig;
    int32_t mode; /* md_epilogue */
    int32_t act;  /* md_act */
    float alpha;
    int32_t variant;        /* md_gemm_variant; 0 = the library picks per shape (tests force each kernel) */
    int32_t raster_group_n; /* column-tiles per L2 raster group; 0 = the library picks */
    void* timeline;         /* profiling aid, normally NULL: every workgroup of the 2-stage kernels writes 8 int64
                               {t_entry, t_prologue_done, t_loop_done, t_stores_drained (shader clock), wall clock
                               (100 MHz), XCC_ID << 32 | HW_ID, 0, 0} at timeline[linear_workgroup_id * 8] */
    int32_t* chosen_variant; /* optional HOST pointer: receives the md_gemm_variant that was actually launched */
    /* Operand lists (PP256 fp32-slice kernels only; NULL = the strided form above).  DEVICE arrays of
     * batch * ksplit * list_segments device pointers.  Item (batch b, split s) contracts, in order, the list_segments operand
     * pairs A_list[i] / B_list[i], i = (b * ksplit + s) * list_segments + j, each over K / (ksplit * list_segments) elements
     * starting at its element 0, accumulating all of them in registers before its one fp32 slice is written:
     *   list_segments = 1, ksplit = G : G separate operand pairs whose products md_splitk_reduce sums (the adaLN
     *                                   condition-vector gradient: sum over the layers of dmod_l W_l in ONE launch);
     *   list_segments = G, ksplit = 1 : ONE contraction over the concatenation of G operand pairs (the caption-token gradient
     *                                   sum_l dkv_l Wkv_l of all 28 blocks: no slices, no reduction pass). */
    const void* const* A_list;
    const void* const* B_list;
    int32_t list_segments;   /* 0 or 1 = one pair per item */
    /* Grouped launch (PP256, both operands K-strided, MD_EPI_STORE_F32 slices: the weight gradients of one DiT block that
     * contract over the same tokens -- qkv, proj, q_linear, ... -- as ONE launch instead of one launch + one reduction each,
     * every one of them too small to fill the chip without a deep split).  HOST array of n_problems <= MD_GEMM_MAX_PROBLEMS
     * entries; A / B / M / N / lda / ldb / sC of the struct are ignored, K / ksplit / sSplit are shared. */
    const md_gemm_problem* problems;
    int32_t n_problems;
    /* PP256 only: upper bound on the workgroups (= CUs) the persistent kernel occupies; 0 = all 256.  The data-parallel step
     * sets 256 - (RCCL channels) while a collective is in flight: an RCCL kernel holds one CU per channel for its whole duration
     * and a PP256 workgroup fills a CU (128 KiB LDS, every VGPR), so with 256 workgroups the ones that find their CU taken start
     * only when another workgroup has finished its whole tile list -- the launch takes up to twice as long; with the smaller grid
     * the same tiles are dealt to the CUs that are free (ceil(tiles / (256 - k)) rounds). */
    int32_t cu_limit;
    /* PP256 only, bf16-output epilogues (STORE_BF16 +- GELU, RESIDUAL, DACT): "whole rounds + split-K tail".  When the work items
     * of a launch do not make whole rounds of its G workgroups (256 tiles on the 248 CUs RCCL leaves: one round + 8 tiles, i.e.
     * TWO rounds), the r left-over tiles are cut along K into s units each (r * s <= G); workgroup u runs unit u after its own
     * whole tiles, in the same k-tile stream, and writes its 256 x 256 fp32 partial to tail_ws + u * 256 KiB; a second, small
     * launch sums the s partials of every left-over tile and applies the launch's epilogue.  The caller provides the workspace
     * (tail_ws_bytes >= 256 KiB * 256 covers every case; NULL = the form is never used).  tail_mode: 0 = the library decides
     * (only when its cost model predicts a gain), 1 = never, 2 = whenever it is structurally possible (tests, A/B runs). */
    void* tail_ws;
    int64_t tail_ws_bytes;
    int32_t tail_mode;
    int32_t* tail_used; /* optional HOST pointer: receives units per left-over tile (s) when the tail form was launched, else 0 */
    /* Activation derivative cached by the forward (MD_ACT_GELU_ERF only; the expert-choice MoE of dit.py:124,131-142, whose
     * pre-activation is needed by NOTHING but gelu' in the backward).  MD_EPI_STORE_BF16 with C2: C2 receives
     * bf16(gelu'(bf16(alpha*acc + bias))) instead of the pre-activation (the forward epilogue has Phi and the density in registers
     * anyway: +2 operations per pair).  MD_EPI_DACT: aux already holds the derivative, C = bf16(bf16(alpha*acc) * aux) -- the
     * backward epilogue loses its transcendental and its polynomial.  0 = the plain forms above. */
    int32_t dact_cached;
} md_gemm_args;

/* Kernels behind md_gemm_bf16.  AUTO applies the measured per-shape rules; a kernel that cannot
 * run the requested problem (PP256 needs K / ksplit to be a multiple of 128, N a multiple of 8, no atomics) is
 * rejected with MD_NOT_ELIGIBLE (-2; nothing was launched) rather than silently replaced; a malformed problem is -1. */
#define MD_NOT_ELIGIBLE (-2)
enum md_gemm_variant {
    MD_GEMM_AUTO = 0,
    MD_GEMM_REG128 = 1,   /* 128 x 128 tile, register-staged global -> LDS, 3 workgroups / CU                        */
    MD_GEMM_DMA128 = 2,   /* 128 x 128 tile, LDS-DMA double buffer                                                   */
    MD_GEMM_PACED256 = 3, /* 256 x 256 tile, LDS-DMA double buffer, DMA issue paced over the k-steps                 */
    MD_GEMM_PP256 = 4,    /* 256 x 256 tile, persistent, two wave groups half a phase apart, 8-slot half-tile ring   */
    MD_GEMM_W4 = 5        /* 256 x 256 tile, persistent, 4 waves x 128 x 128 (accumulators in the AGPR half of the file),
                             register-staged operands; K-contiguous x K-contiguous (nn.Linear forward) only          */
};

int md_gemm_bf16(const md_gemm_args* args, hipStream_t stream);
/* out[b] (+)= sum over the ksplit dense fp32 [M, N] slices a split-K md_gemm_bf16 left in ws (deterministic).
 * accumulate: 0 = store fp32, 1 = add to the fp32 out, 2 (ABI 6) = round the sum to bf16 and STORE it: out is then a bf16 matrix
 * (ldo / sOut in bf16 elements) -- the gradient-exchange buffer of a step that has one microbatch (configs/res_256_pretrain.yaml:24,111:
 * a rank of the 8-GPU run), which needs no fp32 accumulator pass.  Same for the flat form. */
int md_splitk_reduce(const float* ws, float* out, int64_t M, int64_t N, int64_t ldo, int64_t sOut, int32_t ksplit,
                     int32_t batch, int32_t accumulate, hipStream_t stream);

/* out[i] (+)= sum_s ws[s * slice_stride + i], i < n: the flat form for grouped launches (n % 4 == 0). */
int md_splitk_reduce_flat(const float* ws, float* out, int64_t n, int64_t slice_stride, int32_t ksplit, int32_t accumulate,
                          hipStream_t stream);

/* ------------------------------------------------------------------------------------------- LayerNorm */
/* y = LN(act(x + pos[row % pos_rows])) * w;  out = y * (1 + scale[row / rows_per_sample]) + shift[...].
 * w (f32 [C]), pos (f32 [pos_rows, C]), act, scale/shift (bf16 [samples, ldmod]) are all optional.
 * Replaces nn.LayerNorm(bias=False) under low-precision LayerNorm (utils.py:71-78, train.py:81-84), modulate
 * (utils.py:28-30), the `+ pos_embed` of dit.py:479 and the act->norm order of Mlp (utils.py:63-68). */
typedef struct md_ln_args {
    const void* x;     /* bf16 [rows, ldx] */
    const void* w;     /* f32 [C] or NULL */
    const void* shift; /* bf16 or NULL */
    const void* scale; /* bf16 or NULL */
    const void* pos;   /* f32 or NULL */
    void* out;         /* bf16 [rows, ldo] (forward only) */
    void* mean;        /* f32 [rows]: written by fwd (optional), read by bwd */
    void* rstd;        /* f32 [rows] */
    int64_t rows, C, ldx, ldo, ldmod, rows_per_sample, pos_rows;
    float eps;
    int32_t act; /* md_act applied to x before the norm */
} md_ln_args;

typedef struct md_ln_bwd_args {
    const void* dz;  /* bf16 [rows, lddz]: grad of the (modulated) output */
    void* dx;        /* bf16 [rows, lddx] or NULL */
    void* dscale;    /* f32 [samples, ldg], ZERO on entry: receives the per-sample sums dS = sum_t dz * xhat; if
                        dscale_is_output it is turned into the modulation-scale gradient w * dS.  Required when dw is set
                        (plain LayerNorms pass a zeroed scratch [samples, C]). */
    void* dshift;    /* f32 [samples, ldg] (+=) or NULL */
    void* dw;        /* f32 [C] (+= sum_b (1 + scale_b) * dS_b) or NULL */
    int64_t lddz, lddx, ldg;
    int64_t rows_per_block; /* rows of one sample handled by one workgroup (column-sum granularity) */
    int32_t accumulate;     /* dx += instead of dx = */
    int32_t dscale_is_output;
} md_ln_bwd_args;

int md_ln_fwd(const md_ln_args* a, hipStream_t stream);
int md_ln_bwd(const md_ln_args* a, const md_ln_bwd_args* b, hipStream_t stream);

/* Non-parametric LayerNorm over nseg column segments of every row of buf, in place: segment s covers columns
 * [col0 + s * seg_stride, ... + width); rstd_out is [nseg][rows].  nseg = 2, seg_stride = hidden normalises the q and the k
 * half of a packed qkv row in one launch.
 * (ln_q / ln_k over ALL heads concatenated: utils.py:113-114,122-125,175-176,183-186.) */
int md_qkln_fwd(void* buf, int64_t rows, int64_t ld, int64_t col0, int64_t width, int32_t nseg, int64_t seg_stride,
                float* rstd_out, float eps, hipStream_t stream);
/* d: grad buffer (in place, dy -> dx); y: the normalised forward output; same segment addressing in both. */
int md_qkln_bwd(void* d, int64_t ldd, int64_t dcol0, const void* y, int64_t ldy, int64_t ycol0, int64_t rows,
                int64_t width, int32_t nseg, int64_t dseg_stride, int64_t yseg_stride, const float* rstd, hipStream_t stream);

/* Head-major forms (ABI 6).  The forward reads the row-major segments like md_qkln_fwd and writes the normalised values
 * HEAD-MAJOR into a separate buffer: element (row = b * S + s, segment g, column c = h * hd + e) goes to
 * out[g * out_seg_stride + ((b * H + h) * S + s) * hd + e], H = width / hd -- one contiguous [S, hd] block per (sample, head), which is
 * what the attention kernels read (md_attn_args.hsq / hsk); buf is left untouched.  The backward reads dL/dy (written head-major by
 * md_attn_bwd) and y in that layout and writes dL/dx row-major into d (the operand of the qkv / q / kv weight- and data-gradient
 * GEMMs).  rows % S == 0.  The [B, N, 3, H, hd] reshape + permute of utils.py:177-182 (116-121) is the layout freedom used. */
int md_qkln_fwd_hm(const void* buf, int64_t rows, int64_t ld, int64_t col0, int64_t width, int32_t nseg, int64_t seg_stride,
                   void* out, int64_t out_seg_stride, int64_t S, int32_t hd, float* rstd_out, float eps, hipStream_t stream);
int md_qkln_bwd_hm(const void* dy, int64_t dy_seg_stride, const void* y, int64_t y_seg_stride, void* d, int64_t ldd, int64_t dcol0,
                   int64_t dseg_stride, int64_t rows, int64_t width, int32_t nseg, int64_t S, int32_t hd, const float* rstd,
                   hipStream_t stream);

/* Deterministic forms (added under ABI 6: the change only ADDS symbols, every existing entry point and struct is untouched, so
 * MD_ABI_VERSION stays 6 and callers built against the earlier header keep working).
 *
 * md_ln_bwd, md_gate_bwd and md_colsum publish their per-column sums with fp32 atomics: the order of the adds, and with it the
 * last bits of the result, changes from run to run.  The _det entry points compute the same sums with NO float atomic and one
 * writer per address: every workgroup of the row kernel stores its partial sums into its own slice of a caller-supplied fp32
 * workspace, and a finish kernel adds the slices of one output element in ascending slice order and adds the total to the
 * output (+=, as the atomic forms do).  Same binary + same GPU model + same arguments => bit-identical results; another
 * rows_per_block is another summation order.  Row outputs (dx, dbr) are bit-identical to the atomic forms.
 *
 * The workspace needs NO initialisation (every slice element the finish reads is written by the row kernel of the same call) and
 * may be reused by the next call on the same stream.  md_det_ws_floats answers its size in floats (0 = none needed, ws may be
 * NULL); a launcher given ws == NULL where one is needed, or ws_floats below that size, returns -1 and launches nothing.
 *   MD_DET_GATE_BWD  chunks = ceil(rows_per_sample / rows_per_block), samples = rows / rows_per_sample:
 *                    samples * chunks * C  ([samples][chunks][C]); 0 when chunks == 1 (the workgroup is the only writer of its row)
 *   MD_DET_LN_BWD    2 * samples * chunks * C  ([2][samples][chunks][C]: dS, dshift; 0 when chunks == 1)
 *                    + groups * C, groups = ceil(samples / 16)  (weight-gradient partials of 16 samples each, added in ascending
 *                    order by a third kernel; 0 when groups == 1).  rows_per_sample <= 0 means one sample, as in md_ln_args.
 *   MD_DET_COLSUM    blocks * C, blocks = ceil(rows / r) with the library's own rows-per-workgroup rule r(rows, C) -- the one md_colsum
 *                    uses; 0 when blocks == 1.  rows_per_sample and rows_per_block are ignored.
 * md_ln_bwd_det: dw[c] += sum_b (1 + scale[b, c]) * dS[b, c] in ascending b within a group of 16, groups in ascending order. */
enum md_det_kind { MD_DET_GATE_BWD = 0, MD_DET_LN_BWD = 1, MD_DET_COLSUM = 2 };
int md_det_ws_floats(int32_t kind, int64_t rows, int64_t rows_per_sample, int64_t rows_per_block, int64_t C, int64_t* out_floats);
int md_ln_bwd_det(const md_ln_args* a, const md_ln_bwd_args* b, float* ws, int64_t ws_floats, hipStream_t stream);
int md_gate_bwd_det(const void* dx, const void* br, const void* gate, int64_t ldgate, void* dbr, float* dgate, int64_t lddg,
                    int64_t rows, int64_t C, int64_t rows_per_sample, int64_t rows_per_block, float* ws, int64_t ws_floats,
                    hipStream_t stream);
int md_colsum_det(const void* x, int32_t x_is_f32, int64_t ld, float* out, int64_t rows, int64_t C, float* ws, int64_t ws_floats,
                  hipStream_t stream);

/* ------------------------------------------------------------------------------------------- attention */
/* softmax(scale * Q K^T) V per (batch, head), non-causal, no mask (md_attn_fwd_kbias below: a per-key bias).  Row r of head h of
 * batch b of X lives at X + b*sX + r*ldX + h*hsX (bf16; hsX = hd unless set), so packed qkv / kv projection buffers are addressed in
 * place.
 * lse / delta: f32 [B, H, Sq].  Replaces F.scaled_dot_product_attention (utils.py:127-132,188-193) + backward. */
typedef struct md_attn_args {
    const void *q, *k, *v;
    void* o;          /* fwd: output; bwd: the forward output (input) */
    void* lse;        /* fwd: written; bwd: read */
    const void* d_o;  /* bwd: grad of o */
    void *dq, *dk, *dv;
    void* delta;      /* bwd workspace f32 [B, H, Sq] */
    int64_t B, H, Sq, Skv;
    int64_t ldq, ldk, ldv, ldo, sq, sk, sv, so;
    int64_t lddq, lddk, lddv, lddo, sdq, sdk, sdv, sdo;
    float scale;
    int32_t hd;        /* 32 or 64 */
    int32_t bwd_split; /* backward kernel: 0 = the library picks (one fused launch per (batch, head) for Sq, Skv <= 256; the streaming
                          pair (5) for longer sequences);
                          forced (tests, A/B runs): 2 = fused with Q, dO, K, V in LDS together, 3 = fused in two phases on half the
                          LDS, 4 = the same with dK / dV as two passes for every size (3 does that for the 256-row buckets only)
                          -- all three for Sq, Skv <= 256 only; 5 = the streaming pair (two launches, 128-row chunks, register
                          prefetch, 8-wave workgroups; any size).  A forced variant that does not cover the problem returns -1 and
                          launches nothing.  (1, the round-4 dQ + dK/dV pair, and the block-pair form of 3 / 4 for long sequences
                          were removed in ABI 6.) */
    /* ABI 6: element offset of head h inside its row, per tensor (0 = hd: heads packed side by side in the row).  A head-major
     * tensor [B, H, S, hd] (what md_qkln_fwd_hm writes) is ldX = hd, sX = H * S * hd, hsX = S * hd. */
    int64_t hsq, hsk, hsv, hso, hsdq, hsdk, hsdv, hsdo;
} md_attn_args;

int md_attn_fwd(const md_attn_args* a, hipStream_t stream);
int md_attn_bwd(const md_attn_args* a, hipStream_t stream);
/* (symbol added, MD_ABI_VERSION stays 6.)  o = softmax_j(scale * q . k_j + kbias[b * ldb + j]) V per (sample, head): one
 * fp32 bias per (sample, key), shared by all heads and all queries of the sample; lse includes the bias; -inf removes a key.
 * Everything md_attn_fwd accepts in `a` (packed and head-major layouts) with 1 <= Skv <= 256: the kernel follows the phased forward
 * that md_attn_fwd runs for these key counts -- same grid, workgroups, stores and arithmetic, the score in the log2 domain being
 * acc * (scale * log2 e) + kbias * log2 e, the bias added in fp32.  A zero bias gives the bits of md_attn_fwd; -inf on the trailing
 * keys [n, Skv) gives the bits of md_attn_fwd with Skv = n.  kbias non-NULL and 16-byte aligned, ldb >= Skv, ldb % 4 == 0; anything
 * else returns MD_BAD_ARG and launches nothing.  Only rows [0, B) and columns [0, Skv) of kbias are read.  The caller's contract: no
 * + inf or NaN in the bias, at least one finite bias per sample, K and V finite at removed keys (0 * NaN would poison the row).
 * There is no backward for this form and no bias form of the streaming forward (Skv > 256). */
int md_attn_fwd_kbias(const md_attn_args* a, const float* kbias, int64_t ldb, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- elementwise */
/* a = silu(h12[:, :f]) * h12[:, f:]  (FeedForward, dit.py:88-89) and its backward (dh12 from da). */
int md_swiglu_fwd(const void* h12, int64_t ldh, void* a, int64_t lda, int64_t M, int64_t f, hipStream_t stream);
int md_swiglu_bwd(const void* da, int64_t ldda, const void* h12, int64_t ldh, void* dh12, int64_t lddh, int64_t M, int64_t f,
                  hipStream_t stream);
/* adaLN-Zero gate backward (dit.py:236,238): dbr = gate[b] * dx; dgate[b, :] += sum_t dx * br.  All [rows, C] dense. */
int md_gate_bwd(const void* dx, const void* br, const void* gate, int64_t ldgate, void* dbr, float* dgate, int64_t lddg,
                int64_t rows, int64_t C, int64_t rows_per_sample, int64_t rows_per_block, hipStream_t stream);
int md_act_fwd(const void* x, void* y, int64_t n, int32_t act, hipStream_t stream);               /* bf16 -> bf16 */
int md_act_bwd(const float* dy, const void* x, void* dx, int64_t n, int32_t act, hipStream_t stream); /* dx = dy*act'(x) */
int md_colsum(const void* x, int32_t x_is_f32, int64_t ld, float* out, int64_t rows, int64_t C, hipStream_t stream); /* out += */
int md_cast_f32_bf16(const float* x, void* y, int64_t n, const float* scale_ptr, hipStream_t stream);
/* y = bf16(x), x = 0: stages one bucket of the fp32 gradient accumulators for the data-parallel exchange and clears it in the
 * same pass (the reduce-scatter form of FSDP's gradient reduction, configs/res_256_pretrain.yaml:117-118 SHARD_GRAD_OP). */
int md_cast_f32_bf16_clear(float* x, void* y, int64_t n, hipStream_t stream);
/* y(bf16)[r, :] = x[r, :] * rowscale[r / rows_per_sample]; x_dtype 0 = f16, 1 = f32 (caption cast + drop, model.py:132-139) */
int md_cast_rows_bf16(const void* x, int32_t x_dtype, void* y, int64_t rows, int64_t C, const float* rowscale,
                      int64_t rows_per_sample, hipStream_t stream);
int md_mean_tokens(const void* y, void* out, int64_t B, int64_t L, int64_t C, hipStream_t stream);     /* dit.py:484 */
int md_mean_tokens_bwd(const void* dpool, float* dy, int64_t B, int64_t L, int64_t C, hipStream_t stream); /* dy += */
int md_add_bf16(const void* a, const void* b, void* y, int64_t n, hipStream_t stream);
/* zero-fill (fp32 gradient accumulators, scatter targets): hipMemsetAsync on the caller's stream */
int md_fill_zero(void* p, int64_t bytes, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- masking / MoE routing */
/* utils.py:382-403 given the uniform noise: stable ascending rank.  keep_rows[b*len_keep + r] = b*T + token with rank r
 * (absolute row for md_gather_rows), ids_restore[b, t] = rank, mask[b, t] = rank >= len_keep. */
int md_get_mask(const float* noise, int64_t B, int64_t T, int64_t len_keep, int32_t* keep_rows, int32_t* ids_restore,
                float* mask, hipStream_t stream);
int md_gather_rows(const void* src, int64_t ld_src, const int32_t* idx, void* dst, int64_t ld_dst, int64_t n, int64_t C,
                   hipStream_t stream);  /* dst[i] = src[idx[i]]   (mask_out_token utils.py:406-414; MoE dispatch) */
int md_scatter_rows(const void* src, int64_t ld_src, const int32_t* idx, void* dst, int64_t ld_dst, int64_t n, int64_t C,
                    hipStream_t stream); /* dst[idx[i]] = src[i]   (their backward; dst pre-zeroed) */
/* Expert-choice routing (dit.py:131-133): probs = softmax(logits) (f32, rows padded to ld); expert e of sample n takes
 * its k best tokens: rowidx/gval [E, B*k], slot [B*S, E] (position in the expert's list, or -1). */
int md_moe_route(const float* logits, float* probs, int64_t ld, int64_t B, int64_t S, int32_t E, int32_t k, int32_t* rowidx,
                 float* gval, int32_t* slot, hipStream_t stream);
/* dit.py:141-142 + the gated residual of dit.py:238: br = sum_e g*h2, out = res + gate*br. */
int md_moe_combine(const void* h2, const float* gval, const int32_t* slot, const void* res, const void* gate, int64_t ldgate,
                   void* br, void* out, int64_t B, int64_t S, int32_t E, int32_t k, int64_t C, hipStream_t stream);
int md_moe_combine_bwd(const void* dbr, const void* h2, const int32_t* rowidx, const float* gval, void* dh2, float* dgval,
                       int64_t R, int64_t C, hipStream_t stream);
int md_moe_dispatch_bwd(const void* dxin, const int32_t* slot, void* dx, const float* probs, int64_t ldp, const float* dgval,
                        void* dlogits, int64_t ldo, int64_t B, int64_t S, int32_t E, int32_t k, int64_t C, hipStream_t stream);

/* Masked-expert pruning (added under ABI 6: new symbols only).  A MoE block whose output is masked right behind it (the last
 * patch-mixer block: dit.py:495-504 keeps len_keep of the S tokens of a sample) needs its expert MLPs only on routed rows whose
 * token survives.  md_moe_compact_kept reads what md_moe_route left (after any override) and ids_restore of md_get_mask (a token
 * is kept iff ids_restore < len_keep) and writes, per expert e, with stride = B*k:
 *   rowidx_c[e*stride + p], gval_c[e*stride + p]   the kept routed rows in list order (sample-major, then rank), p < count[e];
 *                                                  p in [count[e], stride): pad rows -- the expert's first routed row, gate value 0
 *   count[e]                                       int32
 *   slot_c[token*E + e]                            p, or -1 (every dropped token: -1 for every expert)
 * The order comes from prefix sums (per-chunk counts in ws, then a scan inside each workgroup): no atomics.  ws: int32 workspace of
 * ws_ints >= E * ceil(B*k / 1024) elements, dead when the call's kernels have run.  B*S < 2^31, B*k <= 65535 * 1024.
 * md_moe_gather_compact / md_moe_combine_bwd_compact are md_gather_rows / md_moe_combine_bwd over rows e*stride + j, j < cap, of
 * every expert (dst / h2 / dh2 are [E, stride, C], dgval [E, stride]).  md_moe_combine_abs / md_moe_dispatch_bwd_abs are
 * md_moe_combine / md_moe_dispatch_bwd with slot_c holding the absolute position in the expert's list: they index (e, slot_c)
 * where the originals index (e, n*k + slot), same kernels, same arithmetic in expert order, and still write every token row (a
 * token without an expert: br = 0, out = res, dx = 0, dlogits = 0). */
int md_moe_compact_kept(const int32_t* rowidx, const float* gval, const int32_t* ids_restore, int64_t len_keep, int64_t B, int64_t S,
                        int32_t E, int32_t k, int32_t* rowidx_c, float* gval_c, int32_t* count, int32_t* slot_c, int32_t* ws,
                        int64_t ws_ints, hipStream_t stream);
int md_moe_gather_compact(const void* src, int64_t ld_src, const int32_t* rowidx_c, void* dst, int32_t E, int64_t cap, int64_t stride,
                          int64_t C, hipStream_t stream);
int md_moe_combine_abs(const void* h2, const float* gval_c, const int32_t* slot_c, const void* res, const void* gate, int64_t ldgate,
                       void* br, void* out, int64_t B, int64_t S, int32_t E, int64_t stride, int64_t C, hipStream_t stream);
int md_moe_combine_bwd_compact(const void* dbr, const void* h2, const int32_t* rowidx_c, const float* gval_c, void* dh2, float* dgval,
                               int32_t E, int64_t cap, int64_t stride, int64_t C, hipStream_t stream);
int md_moe_dispatch_bwd_abs(const void* dxin, const int32_t* slot_c, void* dx, const float* probs, int64_t ldp, const float* dgval,
                            void* dlogits, int64_t ldo, int64_t B, int64_t S, int32_t E, int64_t stride, int64_t C,
                            hipStream_t stream);

/* ------------------------------------------------------------------------------------------- EDM front / back end */
int md_edm_prepare(const float* x0, const float* eps, const float* rnd, float* xn, float* sigma, float* cin, float* cnoise,
                   int64_t B, int64_t per_sample, float p_mean, float p_std, float sigma_data, hipStream_t stream);
/* The same for the fp16 latents the precomputed-latent datasets hold (datasets/latents_loader.py:55-66): also writes the
 * fp32 copy of the clean latents the loss reads, so no torch cast runs on the step path. */
int md_edm_prepare_f16(const void* x0_f16, const float* eps, const float* rnd, float* xn, float* x0_f32, float* sigma, float* cin,
                       float* cnoise, int64_t B, int64_t per_sample, float p_mean, float p_std, float sigma_data,
                       hipStream_t stream);
int md_patchify(const float* x, const float* scale, void* out, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p,
                hipStream_t stream);
int md_timestep_embed(const float* t, void* out, int64_t B, int32_t dim, hipStream_t stream);
int md_unpatchify(const void* tok, const int32_t* ids_restore, int64_t Tk, const float* mask_token, float* img, int64_t B,
                  int32_t C, int32_t H, int32_t W, int32_t p, hipStream_t stream);
/* model.py:177,199-210 on the kept tokens; dtok (optional) = d(batch-mean loss)/d(network output), f32 [B*Tk, C*p*p]. */
int md_edm_loss(const void* tok, const int32_t* keep_rows, const float* xn, const float* x0, const float* sigma,
                float* loss_per_sample, float* loss_mean, float* dtok, int64_t B, int64_t Tk, int32_t C, int32_t H, int32_t W,
                int32_t p, float sigma_data, hipStream_t stream);
/* The form one microbatch of a training step uses (replaces `(loss * n_micro / n_rank).backward()` of Composer's microbatch
 * loop around model.py:104-142 and the scalar torch ops that come with it): dtok is written as bf16 (what the hand-written
 * backward starts from) and pre-multiplied by grad_scale (the microbatch weight); loss_accum (optional) += accum_weight *
 * batch-mean loss, so the rank-mean loss of the step accumulates on the device. */
int md_edm_loss_train(const void* tok, const int32_t* keep_rows, const float* xn, const float* x0, const float* sigma,
                      float* loss_per_sample, float* loss_mean, void* dtok_bf16, float grad_scale, float* loss_accum,
                      float accum_weight, int64_t B, int64_t Tk, int32_t C, int32_t H, int32_t W, int32_t p, float sigma_data,
                      hipStream_t stream);

/* Learned per-noise-level loss weighting (added under ABI 6: new symbols only).  Karras et al. 2024, "Analyzing and Improving the
 * Training Dynamics of Diffusion Models", section 2.2 (uncertainty-based loss weighting); no reference counterpart: models/model.py:199-210
 * trains with the fixed EDM weight alone.  With C channels (C a multiple of 64, 64 <= C <= 256), cnoise[b] = ln(sigma[b]) / 4 as
 * md_edm_prepare(_f16) writes it and L[b] the loss_per_sample of md_edm_loss_train(_weighted), all fp32:
 *   feat[b, c] = sqrt(2) * cosf(cnoise[b] * freq[c] + phase[c])        freq, phase: fixed buffers [C]
 *   u[b]       = sum_c w[c] * feat[b, c]                               w: the C trainable weights (w = 0: u = 0, inv = 1 exactly)
 *   inv[b]     = expf(-u[b])
 *   objective  = (1 / B) sum_b (L[b] * inv[b] + u[b])
 *   dw[c]     += sum_b gscale / B * (1 - inv[b] * L[b]) * feat[b, c]
 * md_logvar_fwd writes u [B] and inv [B]: one wave per sample, lane l adds channels l, l + 64, ... in ascending order.
 * md_edm_loss_train_weighted is md_edm_loss_train with sample_scale [B] (the inv above): the gradient factor of sample b is
 * (gfac * sample_scale[b]), formed once, then * diff; loss_per_sample, loss_mean and loss_accum stay the RAW loss (sample_scale = 1
 * gives the bits of md_edm_loss_train).
 * md_logvar_bwd: one workgroup, no float atomic; for every c the samples are added to dw[c] in index order (two calls from the same
 * buffers give the same bits); obj_mean = the objective, obj_accum (optional) += accum_weight * obj_mean.  inv is recomputed from u.
 * A non-finite L[b] propagates into dw (not masked: the step guard handles it).
 * All three return -1 on a null pointer (obj_accum excepted), B < 1 or a C outside the set above; no allocation, no synchronisation. */
int md_logvar_fwd(const float* cnoise, const float* freq, const float* phase, const float* w, float* u, float* inv, int64_t B,
                  int32_t C, hipStream_t stream);
int md_edm_loss_train_weighted(const void* tok, const int32_t* keep_rows, const float* xn, const float* x0, const float* sigma,
                               float* loss_per_sample, float* loss_mean, void* dtok_bf16, float grad_scale, float* loss_accum,
                               float accum_weight, int64_t B, int64_t Tk, int32_t C, int32_t H, int32_t W, int32_t p,
                               float sigma_data, const float* sample_scale, hipStream_t stream);
int md_logvar_bwd(const float* cnoise, const float* freq, const float* phase, const float* u, const float* loss_per_sample,
                  float gscale, float* dw, float* obj_mean, float* obj_accum, float accum_weight, int64_t B, int32_t C,
                  hipStream_t stream);

/* Sampler (model.py:231-297): the arithmetic around each network evaluation of the Heun loop, fused; fp64 state, fp32
 * preconditioning (model.py:144-179) and classifier-free-guidance combine (dit.py:542-550: F = [cond; uncond] halves). */
int md_edm_sampler_input(const double* x, float* out, int64_t n, float sigma, float sigma_data, int32_t duplicate, hipStream_t stream);
int md_edm_heun_update(const double* x_hat, const double* x_in, const float* F, double* d_cur, double* x_next, int64_t n, float cfg,
                       int32_t has_uncond, double t_in, double t_hat, double t_next, float sigma_data, int32_t second,
                       hipStream_t stream);
/* The same two steps in token space (the cached sampling path: the fp64 state is the only image-shaped tensor).
 * md_edm_sampler_patchify: patches[row(b,ti,tj), c*p*p + ph*p + pw] = bf16(c_in(sigma) * (float)x[b,c,ti*p+ph,tj*p+pw]), bf16
 * [B*T, C*p*p] (T = H/p * W/p); with `duplicate`, rows [B*T, 2*B*T) repeat rows [0, B*T).  The bits of md_edm_sampler_input followed
 * by md_patchify(scale = NULL).
 * md_edm_heun_update_tok: F of image element (b,c,h,w) is read from the network's token output, element (ph*p+pw)*C + c of row
 * b*T + t (the unconditional half starts at row B*T), then exactly md_edm_heun_update.  The bits of md_unpatchify(ids_restore =
 * NULL) followed by md_edm_heun_update. */
int md_edm_sampler_patchify(const double* x, void* patches_bf16, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float sigma,
                            float sigma_data, int32_t duplicate, hipStream_t stream);
int md_edm_heun_update_tok(const double* x_hat, const double* x_in, const void* tok_bf16, double* d_cur, double* x_next, int64_t B,
                           int32_t C, int32_t H, int32_t W, int32_t p, float cfg, int32_t has_uncond, double t_in, double t_hat,
                           double t_next, float sigma_data, int32_t second, hipStream_t stream);
/* One step of a linear multistep solver on the denoised value (Euler, DPM-Solver++(2M); opt-in, the Heun loop above is the default):
 *   F = Fu + cfg * (Fc - Fu) (has_uncond; else F = Fc);  den = c_skip(t_in) * (float)x_in + c_out(t_in) * F  (fp32, as md_edm_heun_update);
 *   x_next = a * x_in + b * (c1 * den - c2 * hist);  hist = den.
 * hist is one f64 buffer of the state's shape: read only when c2 != 0, always written.  x_next may alias x_in.  The host computes a, b,
 * c1, c2 in fp64 (Euler: a = t_next / t_in, b = 1 - a, c1 = 1, c2 = 0; 2M: a = t_next / t_in, b = -expm1(-h), c1 = 1 + 1/(2r), c2 = 1/(2r)).
 * md_edm_solver_update_tok reads F from the network's bf16 token output as md_edm_heun_update_tok does: the bits of
 * md_unpatchify(ids_restore = NULL) followed by md_edm_solver_update. */
int md_edm_solver_update(const double* x_in, const float* F, double* hist, double* x_next, int64_t n, float cfg, int32_t has_uncond,
                         double t_in, float sigma_data, double a, double b, double c1, double c2, hipStream_t stream);
int md_edm_solver_update_tok(const double* x_in, const void* tok_bf16, double* hist, double* x_next, int64_t B, int32_t C, int32_t H,
                             int32_t W, int32_t p, float cfg, int32_t has_uncond, double t_in, float sigma_data, double a, double b,
                             double c1, double c2, hipStream_t stream);
/* Autoguidance (Karras et al. 2024, "Guiding a diffusion model with a bad version of itself"): the two-pointer forms of the four
 * update entry points above.  The second operand of the guidance combine F = Fg + cfg * (Fm - Fg) is the output of a second, weaker
 * network in a buffer of its own -- F_guide: n floats; tok_guide_bf16: [B*T, C*p*p] bf16 rows -- in place of the unconditional half
 * behind the conditional one (`has_uncond`), so two batch-B outputs need no concatenation.
 *   - Each gives the bits of its counterpart called with has_uncond = 1 on the concatenation [F; F_guide] ([tok; tok_guide]): the same
 *     kernels run, with the same fp32 combine (one fma), fp32 preconditioning and fp64 state.
 *   - The token forms take the 16-byte vector path only when C*p*p is a multiple of 8 and BOTH token pointers are 16-byte aligned;
 *     otherwise the whole launch goes element by element.  A misaligned pointer is never read with a vector load.
 *   - A null pointer (the guide's included), a non-positive size, H % p or W % p non-zero, or a t_in that is not positive (NaN
 *     included) returns MD_BAD_ARG and launches nothing.
 *   - Aliasing as above: x_next may alias x_in / x_hat; the two network outputs are only read and may alias each other. */
int md_edm_heun_update_guide(const double* x_hat, const double* x_in, const float* F, const float* F_guide, double* d_cur, double* x_next,
                             int64_t n, float cfg, double t_in, double t_hat, double t_next, float sigma_data, int32_t second,
                             hipStream_t stream);
int md_edm_solver_update_guide(const double* x_in, const float* F, const float* F_guide, double* hist, double* x_next, int64_t n, float cfg,
                               double t_in, float sigma_data, double a, double b, double c1, double c2, hipStream_t stream);
int md_edm_heun_update_guide_tok(const double* x_hat, const double* x_in, const void* tok_bf16, const void* tok_guide_bf16, double* d_cur,
                                 double* x_next, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float cfg, double t_in, double t_hat,
                                 double t_next, float sigma_data, int32_t second, hipStream_t stream);
int md_edm_solver_update_guide_tok(const double* x_in, const void* tok_bf16, const void* tok_guide_bf16, double* hist, double* x_next,
                                   int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float cfg, double t_in, float sigma_data, double a,
                                   double b, double c1, double c2, hipStream_t stream);
/* Stochastic churn (model.py:254-258): x_hat = x + coef * noise in fp64, one fma per element; coef = sqrt(t_hat^2 - t_cur^2) * S_noise
 * from the host.  x_hat may alias x. */
int md_edm_churn(const double* x, const double* noise, double* x_hat, int64_t n, double coef, hipStream_t stream);
/* Image-conditioned sampling (SDEdit image-to-image, inpainting, RePaint resampling; opt-in): blend the known latents x0, brought to
 * the noise level sigma of the state, into the fp64 sampler state x [B, C, HW], in place:
 *   x[b,c,i] = fma(m, x[b,c,i], (1 - m) * k),  k = noise ? fma(sigma, noise[b,c,i], x0[b,c,i]) : x0[b,c,i],
 *   m = (double)mask[(mask_B == 1 ? 0 : b), i]   (mask == NULL: m = 0, the whole state is replaced)
 * mask: f32 [mask_B, HW] with values in [0, 1] (the caller's check), broadcast over the channels; 1 = generated, 0 = known.
 *   - Explicit fmas, so m = 1 returns x and m = 0 returns k bit for bit.  Without a mask x is written and never read.
 *   - One entry point for the SDEdit initialisation (mask = NULL, noise = the unit noise, sigma = the first executed level), the blend
 *     at the start of an inpainting step (noise = a fresh draw, sigma = t_i) and the final paste (noise = NULL, sigma = 0).
 *   - x may alias noise; x0 and mask are only read.  Two elements per lane (16-byte accesses) when HW is even and x, x0 and noise are
 *     16-byte aligned, element by element otherwise.
 *   - MD_BAD_ARG, nothing launched: x or x0 NULL; B, C or HW <= 0; a mask with mask_B not in {1, B}; noise == NULL with sigma != 0;
 *     sigma negative or not finite.
 * The RePaint jump back to level t_i is md_edm_churn(x, noise, x, n, sqrt(t_i^2 - t_next^2)). */
int md_edm_blend_known(double* x, const double* x0, const double* noise, const float* mask, int64_t B, int32_t C, int64_t HW,
                       int32_t mask_B, double sigma, hipStream_t stream);

/* Guidance modes (opt-in; the default stays the cfg combine of the entry points above): CFG rescale (Lin et al. 2024, "Common Diffusion
 * Noise Schedules and Sample Steps are Flawed", 3.4) and adaptive projected guidance, APG (Sadat et al. 2024, "Eliminating Oversaturation
 * and Artifacts of High Guidance Scales").  Both act on the denoised prediction D = c_skip * (float)x_in + c_out * F (fp32, as
 * md_edm_heun_update forms it) and need reductions per sample over its n = per_sample = C*H*W elements, so a guided evaluation is
 * md_guidance_prepare(_tok) followed by one of the four _coef update entry points.
 *   D_c, D_u: D of the conditional output and of the second operand (the unconditional half of a doubled batch, or a guide network's
 *             output; two pointers, as in the _guide entry points).
 *   M = (D_c - D_u) + beta * M_prev   fp32, [B, n] in the layout of the state, in place; beta = apg_momentum (APG only, |beta| < 1;
 *             0 in rescale mode).  M_prev is not read when `first` is set, in rescale mode or when beta == 0.  D_c - D_u is evaluated
 *             as c_out * (F_c - F_u) in fp32: the c_skip * x term is common to both and cancels, so its rounding stays out of M.
 *   moments[b] = (S_c, S_m, Q_cc, Q_mm, Q_cm) = (sum D_c, sum M, sum D_c^2, sum M^2, sum D_c * M) over sample b, accumulated in fp64.
 *   coef[b] = (alpha, gamma), formed in fp64 with w1 = w - 1 and stored as fp32:
 *     MD_GUIDANCE_APG      s = has_norm_threshold && Q_mm > 0 ? min(1, r / sqrt(Q_mm)) : 1;   p = Q_cc > 0 ? s * Q_cm / Q_cc : 0;
 *                          alpha = 1 - w1 * (1 - eta) * p;   gamma = w1 * s
 *                          (= D_c + w1 * (orth + eta * par) for s * M split into its projection on D_c and the rest)
 *     MD_GUIDANCE_RESCALE  var_c = max(Q_cc / n - (S_c / n)^2, 0);   S_g = S_c + w1 * S_m;
 *                          var_g = (Q_cc + 2 w1 Q_cm + w1^2 Q_mm) / n - (S_g / n)^2;
 *                          k = var_g > 0 ? phi * sqrt(var_c / var_g) + 1 - phi : 1;   alpha = k;   gamma = k * w1
 *   The guided prediction is D = alpha_b * D_c + gamma_b * M: the _coef entry points are md_edm_heun_update(_tok) and
 *   md_edm_solver_update(_tok) with D = fmaf(alpha_b, D_c, gamma_b * M) (fp32, widened to fp64) in place of the cfg combine, followed
 *   by the same fp64 update.  F_c / tok_bf16 there is the conditional output alone ([B, n] floats / [B*T, C*p*p] bf16 rows).
 *   - One workgroup per sample, fixed-order reduction, no atomics: two calls give the same bits, and the token form gives the bits of
 *     md_unpatchify followed by the image form (the order of the sums depends on the image-layout element index alone).
 *   - Nothing is copied to the host and nothing synchronises.  M must not alias another operand; in the _coef entry points x_next may
 *     alias x_in / x_hat as above, and F_c, M and coef are only read.
 *   - MD_BAD_ARG, nothing launched: a null pointer, a non-positive size, H % p or W % p non-zero, t_in <= 0, a mode other than the two
 *     below, phi outside [0, 1], has_norm_threshold with r <= 0, |beta| >= 1, or a parameter that is not finite. */
#define MD_GUIDANCE_RESCALE 1
#define MD_GUIDANCE_APG 2
int md_guidance_prepare(const double* x_in, const float* F_c, const float* F_u, float* M, float* coef, double* moments, int64_t B,
                        int64_t per_sample, double t_in, float sigma_data, int32_t mode, double w, double rescale_phi, double apg_eta,
                        int32_t has_norm_threshold, double apg_norm_threshold, double apg_momentum, int32_t first, hipStream_t stream);
int md_guidance_prepare_tok(const double* x_in, const void* tok_bf16, const void* tok_u_bf16, float* M, float* coef, double* moments,
                            int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, double t_in, float sigma_data, int32_t mode, double w,
                            double rescale_phi, double apg_eta, int32_t has_norm_threshold, double apg_norm_threshold, double apg_momentum,
                            int32_t first, hipStream_t stream);
int md_edm_heun_update_coef(const double* x_hat, const double* x_in, const float* F_c, const float* M, const float* coef, double* d_cur,
                            double* x_next, int64_t B, int64_t per_sample, double t_in, double t_hat, double t_next, float sigma_data,
                            int32_t second, hipStream_t stream);
int md_edm_solver_update_coef(const double* x_in, const float* F_c, const float* M, const float* coef, double* hist, double* x_next,
                              int64_t B, int64_t per_sample, double t_in, float sigma_data, double a, double b, double c1, double c2,
                              hipStream_t stream);
int md_edm_heun_update_coef_tok(const double* x_hat, const double* x_in, const void* tok_bf16, const float* M, const float* coef,
                                double* d_cur, double* x_next, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, double t_in,
                                double t_hat, double t_next, float sigma_data, int32_t second, hipStream_t stream);
int md_edm_solver_update_coef_tok(const double* x_in, const void* tok_bf16, const float* M, const float* coef, double* hist, double* x_next,
                                  int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, double t_in, float sigma_data, double a, double b,
                                  double c1, double c2, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- optimiser */
/* Sum of squares of a gradient buffer (fp32, or bf16 when g_is_bf16), deterministic: workgroup b of a fixed grid writes
 * partials[b] (MD_SUMSQ_PARTIALS floats per call); md_sumsq_finish adds `count` partials (several calls' worth, e.g. one per
 * data-parallel bucket) in a fixed order into out[0].  n must be a multiple of 8 and g 16-byte aligned (16-byte loads for both
 * types); anything else is MD_BAD_ARG with nothing launched.  md_sumsq writes ALL MD_SUMSQ_PARTIALS partials whatever n is (a
 * workgroup without work writes 0), so partials needs no initialisation, and nothing outside them.
 * Non-finite input is not filtered: a NaN or +-Inf element makes the sum NaN or +Inf, and so does a FINITE gradient whose sum of
 * squares exceeds FLT_MAX (the sum is then +Inf): md_step_guard reads all three as "skip the step". */
#define MD_SUMSQ_PARTIALS 1024
int md_sumsq(const void* g, int32_t g_is_bf16, int64_t n, float* partials, hipStream_t stream);
int md_sumsq_finish(const float* partials, int64_t count, float* out, hipStream_t stream);
/* Exact integer checksum of n 16-bit words (n % 8 == 0, x 16-byte aligned): out2[0] += sum of the words, out2[1] += sum of
 * word_i * h(i) with h an odd 32-bit hash of the index; out2 (two uint64 on the device) must be zero on entry.  Order-independent
 * and exact, so bit-identical on identical data: the replica-consistency check of the data-parallel step compares it across ranks
 * (a single bf16 ulp, a sign flip or a permutation changes it; no reference counterpart: FSDP keeps one sharded copy). */
int md_checksum_u16(const void* x, int64_t n, uint64_t* out2, hipStream_t stream);
/* clip_grad_norm_ (train.py:85-86) + torch.optim.AdamW (train.py:39-43) + bf16 shadow emit (+ EMA of the weights,
 * configs/res_512_*.yaml:4-9), one pass. */
typedef struct md_adamw_args {
    void *p, *g, *m, *v; /* f32 [n]; g is zeroed when zero_grad */
    void* shadow;        /* bf16 [n] or NULL */
    const void* sumsq;   /* f32 [1] device: sum of squared (unscaled) grads, or NULL for no clipping */
    const void* g_bf16;  /* optional bf16 [n]: take the gradient from here (the data-parallel exchange buffer) instead of g */
    void* ema;           /* optional f32 [n] */
    int64_t n;
    float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, max_norm, grad_scale;
    float ema_smoothing;
    int32_t zero_grad;
    int32_t ema_mode;    /* 0 = none, 1 = ema <- updated weights (ema_start), 2 = ema <- s * ema + (1 - s) * weights */
} md_adamw_args;
int md_adamw_step(const md_adamw_args* a, hipStream_t stream);
/* The sharded form of the same pass (FSDP SHARD_GRAD_OP, configs/res_256_pretrain.yaml:117-118: every rank updates its slice of
 * the optimiser state): ONE launch over n_ranges <= MD_ADAMW_MAX_RANGES chunks of the flat buffers.  Range j covers flat
 * elements [flat_off[j], flat_off[j] + count[j]) of p / m / v / ema (a->p ... are the flat bases); a->g_bf16 (the
 * reduce-scattered gradient) and a->shadow (the bf16 weights to all-gather) are PACKED: range j starts at sum(count[0..j)).
 * a->n is ignored; zero_grad must be 0 (the staging cast cleared the accumulators).  flat_off / count are HOST arrays, every entry
 * a multiple of 4 (count > 0, flat_off >= 0); the ranges may come in any flat order and must not overlap.
 * Both forms, MD_BAD_ARG with nothing launched otherwise: p, g, m, v non-NULL (g also in the range form, which never touches it);
 * ema_mode in 0..2 and ema non-NULL unless it is 0; p, g, m, v (and ema unless ema_mode is 0) 16-byte aligned, g_bf16 and shadow
 * 8-byte aligned (the widths of the kernel's vector accesses; with offsets that are multiples of 4 the bases' alignment carries to
 * every range).  md_adamw_step: n > 0 and n % 4 == 0.  The range form: g_bf16 non-NULL and 1 <= n_ranges <= MD_ADAMW_MAX_RANGES. */
#define MD_ADAMW_MAX_RANGES 64
int md_adamw_step_ranges(const md_adamw_args* a, const int64_t* flat_off, const int64_t* count, int32_t n_ranges, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- training health */
/* (Added under ABI 6: new symbols only, no existing entry point or struct changes.)
 *
 * Per-tensor statistics of a flat buffer -- the gradient norms composer.callbacks.OptimizerMonitor logs (the stage configs'
 * optimizer_monitor), plus max |x| and a non-finite count -- as a segmented two-stage reduction shaped like md_sumsq /
 * md_sumsq_finish.  The caller cuts every tensor into WORK ITEMS of 1 <= count <= MD_STATS_ITEM_MAX elements at src_off (in
 * elements of x, src_off % 8 == 0 so that 16-byte loads are legal for fp32 and bf16; count is arbitrary, the last partial vector
 * is read element by element and nothing past it is touched), sorted by tensor; item_begin[n_tensors + 1] gives each tensor's run
 * of items (empty runs allowed: 0 / 0 / 0).  items and item_begin are DEVICE arrays.
 *   md_tensor_stats_partial  one workgroup per item: part_sumsq / part_absmax / part_nonfinite [item].  Several calls may fill
 *                            disjoint slices of one partial array (pass offset pointers): e.g. the packed chunk buffer and the
 *                            small region of the sharded exchange.  x must be 16-byte aligned.
 *   md_tensor_stats_finish   one wave per tensor adds its items' partials in a fixed order: sumsq / absmax / nonfinite [tensor].
 * A non-finite element (NaN, +-Inf) is counted in nonfinite and EXCLUDED from sumsq and absmax.  fp32 accumulation, no atomics:
 * two calls on the same data and table give bit-identical results. */
#define MD_STATS_ITEM_MAX 65536
typedef struct md_stats_item {
    int64_t src_off; /* first element of the piece inside x */
    int32_t count;   /* 1 .. MD_STATS_ITEM_MAX */
    int32_t tensor;  /* row of the result table */
} md_stats_item;
int md_tensor_stats_partial(const void* x, int32_t x_is_bf16, const md_stats_item* items, int64_t n_items, float* part_sumsq,
                            float* part_absmax, int32_t* part_nonfinite, hipStream_t stream);
int md_tensor_stats_finish(const float* part_sumsq, const float* part_absmax, const int32_t* part_nonfinite,
                           const int32_t* item_begin, int32_t n_tensors, float* sumsq, float* absmax, int32_t* nonfinite,
                           hipStream_t stream);
/* Device-side non-finite step guard (micro_diffusion.models.callbacks.NaNCatcher without a host sync, and BEFORE the update
 * reaches the weights).  md_step_guard (one thread, plain stores): state[0] = isfinite(*sumsq) ? 1 : 0 -- the step's go flag --
 * and state[1] += 1 when it is not -- the running count of skipped steps; state is int32 [4] on the device, [2] and [3] reserved.
 * The _guarded forms are md_adamw_step / md_adamw_step_ranges with that flag as one more kernel argument (guard == NULL: exactly
 * the unguarded pass).  With *guard == 0 the pass leaves p, m, v (and ema in ema_mode 2) untouched bit for bit, and still zeroes
 * g when zero_grad, still writes shadow = bf16(p) (the sharded all-gather sends that buffer) and in ema_mode 1 still copies p
 * into ema (the host flips to mode 2 after that step regardless). */
int md_step_guard(const float* sumsq, int32_t* state, hipStream_t stream);
int md_adamw_step_guarded(const md_adamw_args* a, const int32_t* guard, hipStream_t stream);
int md_adamw_step_ranges_guarded(const md_adamw_args* a, const int64_t* flat_off, const int64_t* count, int32_t n_ranges,
                                 const int32_t* guard, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- model diagnostics */
/* (Added under ABI 6: new symbols only.)  Two reductions over what a training step already leaves on the device, in the style of
 * md_tensor_stats_*: no float atomic, fp64 sums in an order that is a function of the shape alone (two calls on the same inputs
 * give identical bits), no allocation, no synchronisation.  Every output is ADDED TO: the caller zeroes the tables when a
 * reporting interval starts.
 *
 * md_loss_sigma_hist: the EDM loss (models/model.py:181-210: one sigma per sample, log-normal with P_mean / P_std, and the
 * per-sample loss md_edm_loss(_train) writes) split by noise level.  Sample i goes to bin
 *   floor((logf(sigma[i]) - log_lo) * nbins / (log_hi - log_lo)),  fp32, clamped to [0, nbins - 1]
 * (a sigma outside [exp(log_lo), exp(log_hi)) lands in an end bin): sum[bin] += loss_per_sample[i], count[bin] += 1.  A sample
 * whose loss is not finite is counted in nonfinite[0] and left out of sum and count (the policy of md_tensor_stats_*).  One
 * workgroup; per bin the samples are added in a fixed order.  1 <= nbins <= 64, log_hi > log_lo, B >= 1. */
int md_loss_sigma_hist(const float* sigma, const float* loss_per_sample, int64_t B, float log_lo, float log_hi, int32_t nbins,
                       double* sum, int64_t* count, int64_t* nonfinite, hipStream_t stream);
/* md_moe_route_stats: the state of one expert-choice routing layer (models/dit.py:131-133) from what md_moe_route leaves: slot
 * [B*S, E] (position in the expert's list, or -1), probs [B*S, ldp] (ldp >= E; columns >= E are padding and are NOT read), gval
 * [E, B*k].  E <= 16, k <= S.
 *   cover_hist[c], c = 0 .. E    += number of tokens that exactly c experts took (c entries >= 0 in the token's slot row);
 *                                   the sum over c of c * cover_hist[c] grows by E * B * k
 *   fstats[0]                    += sum over tokens of the router entropy -sum_e p ln p (per token in fp32; p == 0 adds 0)
 *   fstats[1 + e]                += sum over tokens of probs[t, e]        (router marginal)
 *   fstats[1 + E + e]            += sum of gval[e, 0 .. B*k)              (gate values of the chosen entries)
 * Two stages in one call: per-workgroup fp64 partials stored into ws (written before it is read: needs no initialisation; 8-byte
 * aligned; at least md_moe_route_stats_ws_floats(B, S, E) floats, which covers every k), then one wave adds them in ascending
 * workgroup order.  Integer atomics for cover_hist only.  16-byte loads when E % 4 == 0, ldp % 4 == 0 (B*k % 4 == 0 for gval) and
 * the bases are 16-byte aligned, element by element otherwise. */
int md_moe_route_stats_ws_floats(int64_t B, int64_t S, int32_t E, int64_t* out);
int md_moe_route_stats(const int32_t* slot, const float* probs, int64_t ldp, const float* gval, int64_t B, int64_t S, int32_t E,
                       int32_t k, float* ws, int64_t ws_floats, int64_t* cover_hist, double* fstats, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- post-hoc EMA */
/* (Added under ABI 6: new symbols only.)  Power-function averages of the fp32 masters (Karras et al. 2024, "Analyzing and Improving
 * the Training Dynamics of Diffusion Models", section 3 / App. C; no reference counterpart: the reference knows one fixed EMA length,
 * configs/res_512_*.yaml:4-9).  One pass behind the AdamW pass: every float4 of p is read once and for every profile k < n_profiles
 *   ema[k][i] = beta[k] * ema[k][i] + (1.f - beta[k]) * p[i]      (fp32; 4 + 8 * n_profiles bytes per parameter)
 * with beta[k] = (1 - 1/t)^(gamma_k + 1) computed by the caller (t = optimiser steps taken, counted from 1).  beta[k] == 0 (t = 1)
 * stores p WITHOUT reading ema[k]: whatever the buffer held (NaN included), it comes out as an exact copy of p.
 * ema and beta are HOST arrays of n_profiles <= MD_EMA_MAX_PROFILES entries, copied into the kernel arguments by value (no device
 * pointer table); p and every ema[k] are device f32, 16-byte aligned; n % 4 == 0; 0 <= beta[k] < 1.
 * guard (NULL = none): the go flag of md_step_guard; at *guard == 0 every profile stays untouched bit for bit (the contract of
 * md_adamw_step_guarded for a live EMA).
 * The _ranges form walks n_ranges <= MD_ADAMW_MAX_RANGES chunks [flat_off[j], flat_off[j] + count[j]) of the flat buffers (the
 * convention of md_adamw_step_ranges: host arrays, offsets and counts multiples of 4; p and the profiles are all flat, so only the
 * flat indices matter) and touches nothing outside them. */
#define MD_EMA_MAX_PROFILES 4
int md_ema_power_update(const float* p, float* const* ema, const float* beta, int32_t n_profiles, int64_t n, const int32_t* guard,
                        hipStream_t stream);
int md_ema_power_update_ranges(const float* p, float* const* ema, const float* beta, int32_t n_profiles, const int64_t* flat_off,
                               const int64_t* count, int32_t n_ranges, const int32_t* guard, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- LoRA */
/* (Added under ABI 6: new symbols only.)  Low-rank adapters on a frozen base (Hu et al. 2021, "LoRA: Low-Rank Adaptation of Large
 * Language Models"; no reference counterpart: the reference fine-tunes every weight).  For a targeted matrix W [rows, cols] of the
 * flat buffers with adapter A [rank, cols], B [rows, rank] (row-major, inside the adapter's own flat fp32 buffer) and scale = alpha / rank:
 *   md_lora_merge   v = p_W + scale * (B A) in fp32 for every item: acc = fma(B[n,j], A[j,k], acc) for j ascending from 0, then
 *                   v = fma(scale, acc, p).  out_is_f32 = 0 stores bf16(v) (round to nearest even) at the tensor's offset of a bf16
 *                   buffer -- the shadow the engine reads --, out_is_f32 = 1 stores v itself (out == p allowed: the adapter fused into
 *                   the masters).  Both forms run the same instructions up to the store, so the bf16 form holds exactly the rounding of
 *                   what the fp32 form stores.  Nothing outside the items' [w_off, w_off + rows * cols) is written.
 *   md_lora_grad    from the accumulated fp32 gradient G = g_W, with c = scale * grad_scale:
 *                     d_adapter[B][n, j] += c * sum_k G[n, k] A[j, k]        d_adapter[A][j, k] += c * sum_n B[n, j] G[n, k]
 *                   (d_adapter has the adapter's layout).  fp32, no atomics, one writer per address, every sum in an order that is a
 *                   function of the table alone: two calls on the same data give identical bits.  A workgroup owns a strip of 64 rows
 *                   over all columns: dB rows are complete inside it (k ascending); the strip's share of dA (n ascending) goes to the
 *                   workspace slice [strip][rank][cols] of the item, and a finish launch issued by the same call adds the slices in
 *                   ascending strip order.  G is read once.  ws needs no initialisation (written before it is read).
 * ONE launch over all items (two for md_lora_grad), driven by a work table in the manner of md_tensor_stats_partial.  `items` is the
 * DEVICE copy the kernels read; `items_host` is the caller's HOST copy of the same n_items entries: shapes, alignment and the
 * workspace size are checked on it and the grids are sized from it (an error code has to come from the host, and a launch path does
 * not synchronise to read a device table).  md_lora_grad_ws_floats checks the host table, writes every item's ws_off into it (upload
 * the table afterwards) and returns the workspace size in floats.
 * Supported: rank in {4, 8, 16, 32, 64}; rows >= 1 (no tile size is assumed to divide it); cols a multiple of 8; w_off a multiple of
 * 8, a_off / b_off multiples of 4 (16-byte accesses); p, g, out, adapter, d_adapter, ws 16-byte aligned.  Anything else, a NULL
 * pointer, a ws_off that is not what md_lora_grad_ws_floats wrote, or ws_floats below its result: MD_BAD_ARG, nothing launched. */
typedef struct md_lora_item {
    int64_t w_off;  /* first element of W inside p / g / out */
    int64_t a_off;  /* first element of A [rank, cols] inside adapter / d_adapter */
    int64_t b_off;  /* first element of B [rows, rank] inside adapter / d_adapter */
    int64_t ws_off; /* first float of the item's dA slices inside ws: written by md_lora_grad_ws_floats, not read by md_lora_merge */
    int32_t rows, cols;
} md_lora_item;
int md_lora_merge(const float* p, const float* adapter, const md_lora_item* items, const md_lora_item* items_host, int32_t n_items,
                  int32_t rank, float scale, void* out, int32_t out_is_f32, hipStream_t stream);
int md_lora_grad_ws_floats(md_lora_item* items_host, int32_t n_items, int32_t rank, int64_t* out);
int md_lora_grad(const float* g, const float* adapter, const md_lora_item* items, const md_lora_item* items_host, int32_t n_items,
                 int32_t rank, float scale, float grad_scale, float* d_adapter, float* ws, int64_t ws_floats, hipStream_t stream);

/* (Added under ABI 6: new symbols only.)  The factored weight-gradient backward of one targeted linear y = x W_eff^T: the adapter's
 * gradient from the backward's dy [M, N] and the saved input x [M, K] (bf16, row-major, leading dimensions lddy >= N, ldx >= K; the
 * pointers already include any column offset), without forming G = dy^T x:
 *     P = x A^T [M, r]    Q = dy B [M, r]    dB[n, j] += c * sum_m dy[m, n] P[m, j]    dA[j, k] += c * sum_m Q[m, j] x[m, k]
 * A [rank, K], B [N, rank], dA, dB fp32 in the adapter's layout.  A, B, P and Q are rounded to bf16 (round to nearest even) as
 * operands of v_mfma_f32_16x16x32_bf16 (ranks below 16 padded with zero rows); every sum is accumulated in fp32.  No buffer of N * K
 * elements exists: the workspace holds the bf16 adapter operands [r, N + K], P^T and Q^T [2 r, M] as bf16 and `groups` fp32 shares
 * [r, N + K] of row groups, which a finish launch of the same call adds in ascending order, multiplies by c and adds into dA / dB.
 * Four launches (prep, projections, reductions, finish); no atomics, one writer per address, every order a function of (M, N, K,
 * rank) alone: two calls on the same data give identical bits.  Rows >= M, columns >= N of dy and columns >= K of x are not read.
 * ws needs no initialisation.  md_lora_wgrad_geometry reports the rows of one strip of the reduction and the number of row groups
 * (workgroup g of a column block takes the strips g, g + groups, ...).
 * Supported: rank in {4, 8, 16, 32, 64}; M >= 1, N >= 1 (nothing is assumed to divide them); K, lddy, ldx multiples of 8; every
 * pointer 16-byte aligned.  Anything else, a NULL pointer, or ws_floats below md_lora_wgrad_ws_floats: MD_BAD_ARG, nothing launched. */
int md_lora_wgrad_ws_floats(int32_t M, int32_t N, int32_t K, int32_t rank, int64_t* out);
int md_lora_wgrad_geometry(int32_t M, int32_t N, int32_t K, int32_t rank, int32_t* strip_rows, int32_t* groups);
int md_lora_wgrad(const void* dy, int32_t lddy, const void* x, int32_t ldx, int32_t M, int32_t N, int32_t K, const float* A,
                  const float* B, int32_t rank, float c, float* dA, float* dB, float* ws, int64_t ws_floats, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- dispersive loss */
/* (Added under ABI 6: new symbols only.)  Batch-repulsion regulariser on one block's output (Wang & He 2025, "Diffuse and Disperse",
 * the InfoNCE-l2 form; no reference counterpart).  Z [B, K] bf16 is the block output of a microbatch, one row per sample:
 *   G = Z Z^T (fp32)     D_ij = max(0, G_ii + G_jj - 2 G_ij) / K (i != j), D_ii = 0     E_ij = exp(-D_ij / tau)     S = sum_ij E_ij
 *   L = log(S / B^2)     p_ij = E_ij / S     W_aj = p_aj (j != a), W_aa = -sum_{j != a} p_aj     dL/dz_a = 4 / (tau K) sum_j W_aj z_j
 * md_disperse_pairs reads the fp32 Gram G [B, ldg] (columns >= B are not read) and writes
 *   W [B, ldw] bf16 = coef * W, ldw a multiple of 8, the pad columns [B, ldw) zero (the injection GEMM reads whole 16-byte chunks);
 *   result[0 .. 3] fp64 = L, the mean off-diagonal D, the mean off-diagonal p * B^2 (1 = uniform, -> 0 = saturated: every pair so
 *   far apart that only the diagonal is left in S), S;     *loss_accum += accum_weight * L, *dist_accum += accum_weight * mean D
 *   (either may be NULL).
 * W_aa is the negative off-diagonal row sum (never p_aa - rho_a, which cancels).  The squared distance is formed in fp64 from the fp32
 * Gram, exp is fp32, S and the row sums are fp64 in two stages (per row, then over the rows by one workgroup) in an order that is a
 * function of B alone: no atomics, nothing returns to the host, two calls on the same G give identical bits.  ws: fp64 workspace of at
 * least md_disperse_ws_doubles(B) = 2 B entries, written before it is read.  1 <= B <= MD_DISPERSE_MAX_B (B = 1: L = 0, W = 0);
 * tau > 0.  Three launches.
 * md_disperse_gram_small: G [B, ldg] fp32 = Z Z^T for the batch sizes whose fp32 split-K slices md_gemm_bf16 / md_splitk_reduce do
 * not take (B not a multiple of 8).  Plain and bounds-checked: one workgroup per output row, fp32 FMA over the contraction in a fixed
 * order, rows >= B of Z are never read; columns >= B of G are not written.  K and ldz multiples of 8, Z 16-byte aligned. */
#define MD_DISPERSE_MAX_B 4096
int md_disperse_ws_doubles(int64_t B, int64_t* out);
int md_disperse_pairs(const float* G, int64_t ldg, int64_t B, int64_t K, float tau, double coef, void* W, int64_t ldw, double* result,
                      double* ws, int64_t ws_doubles, float* loss_accum, float* dist_accum, float accum_weight, hipStream_t stream);
int md_disperse_gram_small(const void* Z, int64_t ldz, int64_t B, int64_t K, float* G, int64_t ldg, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- input gradients */
/* (Added under ABI 6: new symbols only.)  The last step of the backward to the three network inputs (no reference source: the
 * reference gets them from autograd).
 * md_patch_embed_dgrad: the transpose of md_patchify(scale) followed by the x_embedder.proj GEMM (dit.py:312-314,479), in one launch:
 *   dpatch[row, j] = sum_d dtok[row, d] * w[d, j]                                     (fp32 accumulation, never rounded to bf16)
 *   dx[b, c, ti*p + ph, tj*p + pw] = scale[b] * dpatch[b*T + ti*(W/p) + tj, c*p*p + ph*p + pw]
 * dtok bf16 [B*T, D] with row pitch ld_dtok >= D, w the bf16 weight [D, patch_vec = C*p*p], scale f32 [B] or NULL (= 1), dx f32
 * [B, C, H, W], written, not accumulated.  patch_vec a multiple of 16 with 16-byte aligned dtok / w and ld_dtok % 8 == 0 runs on
 * v_mfma_f32_16x16x32_bf16 (w staged in LDS, transposed, 256 rows of it at a time); everything else on a plain fp32 FMA kernel.
 * *path (host pointer, may be NULL) receives 1 for the MFMA kernel, 0 for the plain one.  No atomics; two calls give the same bits.
 * MD_BAD_ARG, nothing launched: a null dtok / w / dx, a non-positive size, H % p or W % p non-zero, D % 8 != 0, ld_dtok < D, or
 * patch_vec > MD_PATCH_EMBED_DGRAD_MAX_PV.
 * md_timestep_embed_bwd: dt[b] = sum_k f_k * (cos(t_b f_k) * dsin[b, k] - sin(t_b f_k) * dcos[b, k]) from dout bf16 [B, dim] in
 * md_timestep_embed's [cos | sin] layout (utils.py:266-281), f_k from the device function the forward uses.  One wave per sample,
 * fixed-order fp32 sum.
 * md_cast_rows_from_bf16: y[r, :] = float(x_bf16[r, :]) * rowscale[r / rows_per_sample] (rowscale NULL = 1), y f16 (y_dtype 0) or
 * f32 (1): the transpose of md_cast_rows_bf16 (the caption cast + drop, model.py:132-139); any C. */
#define MD_PATCH_EMBED_DGRAD_MAX_PV 64
int md_patch_embed_dgrad(const void* dtok, int64_t ld_dtok, const void* w, const float* scale, float* dx, int64_t B, int32_t C, int32_t H,
                         int32_t W, int32_t p, int32_t D, int32_t* path, hipStream_t stream);
int md_timestep_embed_bwd(const float* t, const void* dout, float* dt, int64_t B, int32_t dim, hipStream_t stream);
int md_cast_rows_from_bf16(const void* x, void* y, int32_t y_dtype, int64_t rows, int64_t C, const float* rowscale,
                           int64_t rows_per_sample, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- measurement-guided sampling */
/* (Added under ABI 6: new symbols only.)  Everything around the two network passes of a guided sampler step (Chung et
 * al. 2023 on the EDM loop; no reference source).  x_hat is the fp64 state the step's first evaluation read at level t_in, F the
 * network output of that evaluation (has_uncond: the unconditional half behind the conditional one, combined as in the update
 * kernels).  Bandwidth-bound, no atomics, nothing returns to the host; two calls give the same bits.
 * md_edm_denoised(_tok): D f32 [B, C, H, W] = c_skip * float(x_hat) + c_out * F with F = F_u + cfg * (F_c - F_u) under has_uncond -- the
 *   same fp32 expressions (sampler_math.h) as `den` inside md_edm_heun_update / md_edm_solver_update, so D has the bits of the value the
 *   step's own update forms.  F is the fp32 image [B or 2B, per_sample], or (_tok) the bf16 token rows in md_edm_heun_update_tok's
 *   layout; the token form gives the bits of md_unpatchify followed by the image form.
 * md_measure_residual: for the measurement operator A = s x s average pooling (s = 1: the identity), per pooled cell in fp32
 *   r = m * (meas - A(D)),  q = -2 * m * r / s^2 written to every pixel of the cell's window (q = dL/dD, f32 [B, C, H, W]),
 *   L[b] = sum over the sample of r^2: the fp32 squares summed in fp64, one workgroup per sample, fixed order (per-thread partials,
 *   then a tree over the 256 partials in LDS).  meas f32 [B, C, H/s, W/s]; mask f32 [mask_B, H/s * W/s] with mask_B 1 or B,
 *   broadcast over the channels, or NULL (= 1).  For a 0 / 1 mask q is -2 * A^T(m * (meas - A(D))).
 * md_guide_cotangent_tok: dtok bf16 [B*T or 2B*T, C*p*p] in the network's output-token layout (element (ph*p + pw)*C + c): the
 *   cotangent of the network output under q.  Rows of the conditional half are (cfg * c_out) * q, with has_uncond rows from B*T on
 *   are ((1 - cfg) * c_out) * q; without has_uncond the one half is c_out * q (cfg is not read).  One bf16 rounding.
 * md_edm_guide_apply: x_next[b] -= zeta / max(sqrt(L[b]), MD_GUIDE_TINY) * (c_skip * q[b] + c_in * (dx[b] + dx[B + b])), in fp64, in
 *   place on the state the solver wrote.  dx f32 [B or 2B, per_sample]: the gradient of the network input from the engine, the
 *   unconditional half (has_uncond) behind the conditional; c_skip and c_in are the fp32 values of level t_in, widened.
 * 16-byte accesses where the sizes and the pointers allow (4 elements per item, patch_vec % 8 == 0 for token rows, W % 4 == 0 and s in
 * {1, 2, 4} for the residual), element by element otherwise.
 * MD_BAD_ARG, nothing launched: a null pointer (mask excepted), a non-positive size, H % p or W % p non-zero, H % s or W % s non-zero,
 * mask_B other than 1 or B, t_in <= 0, or a non-finite cfg, zeta, t_in or sigma_data. */
#define MD_GUIDE_TINY 1e-30 /* floor of sqrt(L[b]) in md_edm_guide_apply: a sample whose residual is exactly zero gets a finite step (its q, dx are zero too) */
int md_edm_denoised(const double* x_hat, const float* F, float* D, int64_t B, int64_t per_sample, float cfg, int32_t has_uncond, double t_in,
                    float sigma_data, hipStream_t stream);
int md_edm_denoised_tok(const double* x_hat, const void* tok_bf16, float* D, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float cfg,
                        int32_t has_uncond, double t_in, float sigma_data, hipStream_t stream);
int md_measure_residual(const float* D, const float* meas, const float* mask, int32_t mask_B, float* q, double* L, int64_t B, int32_t C,
                        int32_t H, int32_t W, int32_t s, hipStream_t stream);
int md_guide_cotangent_tok(const float* q, void* dtok_bf16, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, float cfg,
                           int32_t has_uncond, double t_in, float sigma_data, hipStream_t stream);
int md_edm_guide_apply(double* x_next, const float* q, const float* dx, const double* L, int64_t B, int64_t per_sample, int32_t has_uncond,
                       double zeta, double t_in, float sigma_data, hipStream_t stream);

/* ---- step cache (symbols added, MD_ABI_VERSION stays 6): the contribution of a run of blocks to the residual stream,
 * kept from one sampler evaluation and added back in the next (Delta-DiT / FORA / TeaCache), and the distance probe of the adaptive policy.
 * md_residual_delta: delta = bf16(f32(x_out) - f32(x_in)) over n bf16 elements, one rounding.  16-byte work items in a grid-stride loop
 *   of min(ceil(n / 8 / 256), MD_STEP_DELTA_MAX_BLOCKS) workgroups.  The apply step is md_add_bf16(x_in', delta, x).
 *   MD_BAD_ARG, nothing launched: a null pointer, n <= 0, n % 8 != 0, a pointer that is not 16-byte aligned, delta overlapping an input.
 * md_step_probe: x, ref bf16 [B, per_sample].  One pass: workgroup (g, b) forms sum |f32(x) - f32(ref)| and sum |f32(ref)| over the 16-byte
 *   chunks [g * MD_STEP_PROBE_CHUNKS, (g + 1) * MD_STEP_PROBE_CHUNKS) of sample b in fp64 (per thread in ascending order, a fixed shuffle
 *   tree, the waves in ascending order) and stores the pair into ws; every chunk of ref is overwritten with x's by the thread that
 *   read it.  No workgroup straddles two samples.  ws: at least md_step_probe_ws_doubles(B, per_sample) doubles: a header of two (the
 *   workgroups per sample, which the finish reads), then [B][workgroups per sample][2]; written before it is read.
 *   MD_BAD_ARG, nothing launched: a null pointer, B < 1 or > 65535, per_sample < 8 or % 8 != 0, x or ref not 16-byte aligned, x and ref
 *   overlapping.
 * md_step_probe_finish: one workgroup; one thread per sample adds its partials in ascending order: rel[b] = f32(sum |x - ref| / sum |ref|),
 *   +inf when sum |ref| is 0 (a zero reference is never close), NaN when a sum is NaN; rel_max[0] = max_b rel[b] (NaN if any is).
 *   No atomics; two calls on the same operands give identical bits.  B as in the md_step_probe launch that wrote ws.
 * Nothing here synchronises, allocates or returns to the host. */
#define MD_STEP_DELTA_MAX_BLOCKS 2048 /* 256-thread workgroups of md_residual_delta: eight waves on every SIMD of the chip, once */
#define MD_STEP_PROBE_CHUNKS 1024     /* 16-byte chunks one md_step_probe workgroup reads of each operand (16 KB) */
int md_residual_delta(const void* x_out, const void* x_in, void* delta, int64_t n, hipStream_t stream);
int md_step_probe_ws_doubles(int64_t B, int64_t per_sample, int64_t* out);
int md_step_probe(const void* x, void* ref, int64_t B, int64_t per_sample, double* ws, hipStream_t stream);
int md_step_probe_finish(const double* ws, int64_t B, float* rel, float* rel_max, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- Muon */
/* (symbols added, MD_ABI_VERSION stays 6.)  Orthogonalised momentum for the hidden matrices of the DiT blocks (Jordan et
 * al. 2024, "Muon"; Liu et al. 2025, "Muon is Scalable for LLM Training"; no reference counterpart: the reference knows AdamW only).  For a
 * targeted matrix W [rows, cols] of the flat buffers, with the accumulated gradient g and the momentum m (the `m` buffer of the optimiser):
 *
 * md_muon_momentum   per element, fp32, every operation rounded once, in this order:
 *     coef   as md_adamw_step forms it: grad_scale, times min(1, max_norm / (sqrtf(*sumsq) * grad_scale + 1e-6f)) with sumsq non-NULL and
 *            max_norm > 0
 *     gc = coef * g        m' = fmaf(mu, m, gc)        u = nesterov ? fmaf(mu, m', gc) : m'        m' is stored
 *   per item:  norms[item] = sum u^2 in fp64 (squares exact), in an order that is a function of the table alone: MD_MUON_NORM_PARTS
 *     workgroups per item, each thread its float4s in ascending order, a fixed tree over the 256 threads, the partials in ascending
 *     order;  inv = (float)(1.0 / (sqrt(norms[item]) + 1e-7));  X = bf16(u * inv), row-major [rows, cols], at ws + ws_off.
 *   g: the fp32 accumulators: read (g_bf16 == NULL) and, with zero_grad, zeroed on the items and nowhere else.  g_bf16 (optional): a
 *     flat bf16 gradient buffer (the data-parallel exchange buffer) read INSTEAD at the same flat index; it is only read.
 *   guard (NULL = none) with *guard == 0: m, ws and norms stay untouched bit for bit, the accumulators are still zeroed.
 *   partials: MD_MUON_NORM_PARTS * n_items doubles of scratch, written before they are read.
 * md_muon_newton_schulz   on every item, in place, `steps` (1 .. 8) iterations of  A = X X^T,  B = b A + c A A,  X <- a X + B X  for
 *   rows <= cols, and of  A = X^T X,  X <- a X + X B  for rows > cols (X keeps the parameter's orientation; the operand-layout flags of
 *   md_gemm_bf16 pick the side).  bf16 operands, fp32 accumulation, ksplit = 1, and a rounding to bf16 at three points per iteration:
 *   A = bf16(X X^T) (MD_EPI_STORE_BF16);  T = A A as an fp32 store into the shared scratch, B = bf16(b A + c T);  U = B X as an fp32
 *   store, X = bf16(a X + U) -- the two sums by md_muon_axpby.  Two calls on the same data give identical bits.  Five launches per
 *   iteration and item; the Gram products of up to 16 consecutive items of one shape (the experts of one tensor) go out as one batched
 *   launch.  Host loop, no synchronisation; gemm_launches (optional HOST pointer) receives the number of md_gemm_bf16 launches.
 * md_muon_axpby   out[i] = bf16(a * (float)x[i] + b * y[i]), x / out bf16, y fp32, n elements: the two products and the sum are rounded
 *   once each (no fused multiply-add), then once to bf16.  out == x is allowed.  n > 0, n % 8 == 0, 16-byte aligned pointers; anything
 *   else MD_BAD_ARG, nothing launched.
 * md_muon_apply   per element:  q = p * decay, decay = 1.f - lr * weight_decay as md_adamw_step forms it;
 *     p' = fmaf(-(lr * scale_item), (float)O, q), O read at ws + ws_off (where md_muon_newton_schulz leaves it);  shadow = bf16(p') at the flat index;
 *     ema_mode 0: ema not touched; 1: ema = p'; 2: ema = fmaf(ema_smoothing, ema, (1.f - ema_smoothing) * p').
 *   *guard == 0: p and a live EMA stay untouched bit for bit, shadow = bf16(p), mode 1 still copies p.  Nothing outside the items is
 *   written.
 * Work table (the convention of md_lora_*): `items` is the DEVICE copy the kernels read, `items_host` the caller's HOST copy of the same
 * entries, on which shapes, alignment and workspace offsets are checked and from which the grids are sized.  md_muon_ws_bytes checks
 * the host table, writes every ws_off into it (upload the table afterwards) and returns the workspace size in BYTES.  Workspace of an
 * item, in bf16 elements from ws_off: [X: rows * cols | A: s * s | B: s * s], s = min(rows, cols); items follow each other without a
 * gap; behind the last one, max(rows * cols) floats of fp32 scratch shared by all items (the launches of one stream run in order).
 * Supported: 1 <= n_items <= 65535; rows and cols multiples of 64; flat_off >= 0 and a multiple of 8; every pointer 16-byte aligned
 * (partials / norms 8); 0 <= mu < 1; a, b, c finite.  Anything else, a NULL pointer (g_bf16, sumsq, guard, gemm_launches and, in mode
 * 0, ema excepted) or a ws_off that is not what md_muon_ws_bytes wrote: MD_BAD_ARG, nothing launched. */
#define MD_MUON_NORM_PARTS 16
typedef struct md_muon_item {
    int64_t flat_off; /* first element of W inside p / g / m / shadow / ema */
    int32_t rows, cols;
    int64_t ws_off;   /* first bf16 element of the item's workspace: written by md_muon_ws_bytes */
    float scale;      /* md_muon_apply: the update is lr * scale * O (the shape factor) */
    int32_t reserved;
} md_muon_item;
int md_muon_ws_bytes(md_muon_item* items_host, int32_t n_items, int64_t* out);
int md_muon_momentum(float* g, const void* g_bf16, float* m, const md_muon_item* items, const md_muon_item* items_host, int32_t n_items,
                     float mu, int32_t nesterov, float grad_scale, const float* sumsq, float max_norm, int32_t zero_grad,
                     const int32_t* guard, void* ws, double* partials, double* norms, hipStream_t stream);
int md_muon_newton_schulz(const md_muon_item* items_host, int32_t n_items, int32_t steps, float a, float b, float c, void* ws,
                          int32_t* gemm_launches, hipStream_t stream);
int md_muon_apply(float* p, void* shadow, float* ema, const md_muon_item* items, const md_muon_item* items_host, int32_t n_items, float lr,
                  float weight_decay, int32_t ema_mode, float ema_smoothing, const int32_t* guard, const void* ws, hipStream_t stream);
int md_muon_axpby(const void* x, const float* y, void* out, float a, float b, int64_t n, hipStream_t stream);

/* ------------------------------------------------------------------------------------------- cross-attention probe */
/* (symbol added, MD_ABI_VERSION stays 6.)  Observes the cross-attention of a DiT block (utils.py:122-132), whose fused
 * form md_attn_fwd, like the reference's F.scaled_dot_product_attention, never materialises its probabilities.
 *
 * out[row, j] += (1/H) * sum_h softmax_j(scale * q_h(b,q) . k_h(b,j)),  j < Skv;  row = out_rows ? out_rows[b*Sq+q] : b*Sq+q
 * Reads a->q, a->k, B, H, Sq, Skv, ldq, ldk, sq, sk, hsq, hsk, scale, hd (both packed and head-major addressing, as md_attn_fwd);
 * ignores every other field.  out f32, row pitch ldo >= Skv floats, ldo % 4 == 0, 16-byte aligned.
 *
 * hd in {32, 64}, 1 <= Skv <= 128 (the 77 caption tokens; self-attention maps are out of scope), any Sq, B, H >= 1; q and k 16-byte
 * aligned with ldq, ldk, sq, sk, hsq, hsk multiples of 8 elements.  Anything else, a NULL q / k / out or a bad ldo: MD_BAD_ARG, nothing
 * launched.  The softmax takes its own row maximum and sum in fp32 (lse is not read): s = acc * scale, p = exp2((s - max) * log2 e),
 * P = p * rcp(sum).  Heads are added in ascending order in fp32, the sum is multiplied once by 1.0f / H and added to out; every output
 * element has one writer and there are no atomics: same binary and same arguments give the same bits.  Columns [Skv, ldo) of a row and
 * rows the launch does not name are not written; nothing is read past row Sq - 1 of q or row Skv - 1 of k of any sample.  out_rows holds
 * global row indices (md_get_mask's keep_rows, what md_gather_rows consumes). */
int md_attn_probs(const md_attn_args* a, float* out, int64_t ldo, const int32_t* out_rows, hipStream_t stream);
/* (symbol added.)  md_attn_probs of the attention md_attn_fwd_kbias ran: s = acc * scale + kbias[b * ldb + j] (natural
 * units, the sum rounded on its own in fp32), everything else and every limit as above; a key with bias -inf adds exactly + 0 to its
 * column.  kbias as for md_attn_fwd_kbias (non-NULL, 16-byte aligned, ldb >= Skv, ldb % 4 == 0, rows [0, B) x columns [0, Skv) read,
 * no + inf / NaN, a finite bias in every row); else MD_BAD_ARG, nothing launched.  md_attn_probs itself keeps its bits. */
int md_attn_probs_kbias(const md_attn_args* a, const float* kbias, int64_t ldb, float* out, int64_t ldo, const int32_t* out_rows,
                        hipStream_t stream);

/* ------------------------------------------------------------------------------------------- MXFP8 (block-scaled fp8) */
/* (symbols added, MD_ABI_VERSION stays 6.)  OCP MX with e4m3fn elements ("MXFP8"): a matrix [rows, K] is stored as fp8
 * elements, K-contiguous, plus one e8m0 scale byte per 32 consecutive elements along K, row-major uint8 [rows, K / 32].  For a block with
 * largest magnitude amax:  X = clamp(floor(log2 amax) - 8, -127, 127), scale byte = X + 127 (0 with zero elements when amax = 0),
 * element = e4m3fn_rne(clamp(v * 2^-X, -448, 448)); the scaling is exact, the clamp keeps amax in (448 * 2^X, 512 * 2^X) from
 * overflowing.  Inputs are finite.  Inference only (the sampler's opt-in mxfp8=): nothing here has a backward.
 *
 * md_mx_quant_rows: src bf16, element (r, k) at src[r * ld + k] (src_kcontig = 1: activations, nn.Linear weights [N, K]) or at
 * src[k * ld + r] (src_kcontig = 0: the MoE expert tensors, whose contraction dimension is the strided one) ->
 * dst[r * ldd + k] fp8 and scales[r * lds + k / 32]; `batch` matrices sSrc elements / sDst bytes / sScale bytes apart.  K % 32 == 0,
 * ld % 8 == 0, ldd % 16 == 0, ldd >= K, lds >= K / 32, src and dst 16-byte aligned; else MD_BAD_ARG, nothing launched.  No atomics,
 * one writer per output byte; bytes [K, ldd) of a dst row, [K / 32, lds) of a scale row and rows the call does not name are not
 * written.  Bit-exact against the rule above (tests/mx_ref.py). */
int md_mx_quant_rows(const void* src, int64_t ld, int32_t src_kcontig, void* dst, int64_t ldd, void* scales, int64_t lds, int64_t rows,
                     int64_t K, int32_t batch, int64_t sSrc, int64_t sDst, int64_t sScale, hipStream_t stream);
/* md_swiglu_fwd writing a[m, c] = silu(h12[m, c]) * h12[m, f + c] as MXFP8 (a: fp8 [M, f] with pitch lda bytes, scales uint8 [M, f / 32]
 * with pitch lds): the bits of md_swiglu_fwd followed by md_mx_quant_rows.  f % 32 == 0, ldh % 8 == 0, lda % 16 == 0. */
int md_swiglu_fwd_mx(const void* h12, int64_t ldh, void* a, int64_t lda, void* scales, int64_t lds, int64_t M, int64_t f,
                     hipStream_t stream);

/* C[m, n] = epilogue(sum_k A(m, k) * B(n, k)): A [M, K] and B [N, K] MXFP8 (above), fp32 accumulation on
 * v_mfma_scale_f32_16x16x128_f8f6f4, the hardware applying both block scales.  Epilogues, with the rounding steps of md_gemm_bf16:
 *   MD_EPI_STORE_BF16  C = bf16(act(acc + bias)), act in {MD_ACT_NONE, MD_ACT_GELU_ERF}; optional C2 = bf16(acc + bias)
 *   MD_EPI_RESIDUAL    C = bf16(res + gate[row / rows_per_sample, col] * bf16(acc + bias)) (gate optional); optional C2; batch == 1
 * bias fp32 [N] (optional).  `batch` problems sA / sB / sScaleA / sScaleB bytes and sC / sC2 / sBias elements apart (the experts).
 * Any M >= 1; N % 16 == 0 and K % 128 == 0, else MD_NOT_ELIGIBLE (-2) and nothing is launched.  lda, ldb (bytes) % 16 == 0, ldc, ldc2,
 * ldr, ldg,
 * sC, sC2 % 8 == 0, A, B, C, C2, res and gate 16-byte aligned, ldr and ldg >= N; a malformed problem is MD_BAD_ARG.  Nothing is read or written outside the named rows
 * and columns; no atomics, one writer per output element. */
typedef struct md_gemm_mx_args {
    const void* A;       /* fp8 [M, K], element (m, k) at A[m * lda + k] */
    const void* B;       /* fp8 [N, K] */
    const void* scaleA;  /* uint8 [M, K / 32], pitch ldsa */
    const void* scaleB;  /* uint8 [N, K / 32], pitch ldsb */
    void* C;             /* bf16 [M, N] */
    void* C2;            /* bf16 [M, N] or NULL */
    const void* bias;    /* fp32 [N] or NULL */
    const void* res;     /* bf16 [M, N] (MD_EPI_RESIDUAL) */
    const void* gate;    /* bf16 [M / rows_per_sample, N] or NULL */
    int64_t M, N, K;
    int64_t lda, ldb, ldsa, ldsb, ldc, ldc2, ldr, ldg;
    int64_t sA, sB, sScaleA, sScaleB, sC, sC2, sBias;
    int64_t rows_per_sample;
    int32_t batch, mode, act, reserved;
} md_gemm_mx_args;
int md_gemm_mxfp8(const md_gemm_mx_args* a, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MICRODIT_HIP_H */
