// Cross-attention probe: head-averaged attention probabilities of a short key set, recomputed from the normalised q and
// k the fused attention ran on (md_attn_fwd never materialises them; the reference's F.scaled_dot_product_attention, utils.py:122-132,
// does not either).
//
//   md_attn_probs         out[row, j] += (1 / H) * sum_h softmax_j(scale * q_h(b, q) . k_h(b, j)),  j < Skv <= 128
//   md_attn_probs_kbias   the same with kbias[b, j] added to the logit of key j (what md_attn_fwd_kbias ran on); -inf
//                         removes a key, whose column then gets exactly + 0
//
// One workgroup of four waves takes 64 query rows of one sample and walks the heads in ascending order.  K of one head, padded with zero
// rows to a multiple of 16 keys, lives in LDS (two buffers of 128 rows x (hd + 8) bf16: 36,864 bytes at hd = 64, 20,480 at hd = 32; the 8
// elements of row padding keep the 16-byte fragment reads of 16 consecutive rows off one bank group); the K tile and the Q fragments of
// head h + 1 are fetched into registers while head h is computed, so there is one barrier per head.  Each wave forms S^T = K Q^T with
// v_mfma_f32_16x16x32_bf16: the Q fragment (B operand: lane l holds query l & 15, k = 8 (l >> 4) + j) is one 16-byte global load per
// lane and k-step, and a lane ends with one query column and 4 consecutive keys per 16-key block (col = l & 15, row = 4 (l >> 4) + reg).
// The kernel is bound by the latency of the per-head fetches, not by bandwidth: a 64-row tile and a serial walk over the heads leave
// B * Sq / 16 waves for the whole chip (one per SIMD at B = 64, Sq = 256), each with one head's operands in flight.
// Row maximum and row sum are then 4 * blocks values in the lane plus two cross-lane steps (lanes l, l ^ 16, l ^ 32, l ^ 48 share a query).
//
// Arithmetic per score, all fp32: s = acc * scale;  p = exp2((s - max) * log2 e) (v_exp_f32);  sum: the lane's values in ascending key
// order, then the two cross-lane adds (both symmetric: the four lanes of a query hold the same bits);  P = p * rcp(sum);  the head sum
// in ascending head order in registers;  out += headsum * (1.0f / H) as the only writer of the element.  No atomics: same binary and
// same arguments give the same bits.
// The bias form is the same kernel with a.kbias set (one kernel per head_dim, a wave-uniform branch per score block): s = acc * scale + bias,
// the sum rounded on its own.  The sample's biases are fetched once per workgroup into LDS that is already there and idle -- the first four
// of the 16 padding bytes of key row j of buffer 0, which no K store and no fragment read touches -- so LDS and registers stay as they were.
#include "md_common.h"
#include "../../include/microdit_hip.h"
#include <math.h>

// Every product and sum below is rounded on its own, as written: a fused multiply-add in `out += headsum * (1 / H)` would make two
// launches into one buffer differ from the fp32 sum of two single launches.
#pragma clang fp contract(off)

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_ROWS = 64;          // query rows of one workgroup: 16 per wave
constexpr int AP_MAX_KEYS = 128;
constexpr int AP_MAX_KB = AP_MAX_KEYS / 16;

struct ap_args {
    const bf16 *q, *k;
    const float* kbias;                  // [B, ldb] or nullptr
    float* out;
    const int32_t* out_rows;
    int64_t H, Sq, Skv, ldq, ldk, sq, sk, hsq, hsk, ldo, tiles, ldb;
    float scale, inv_h;
};

template <int HD>
__global__ __launch_bounds__(AP_THREADS) void attn_probs_kernel(const ap_args a) {
    constexpr int KS = HD / 32;          // k-steps of the 16x16x32 MFMA
    constexpr int LDK = HD + 8;          // LDS row pitch in elements (144 / 80 bytes: a multiple of 16)
    constexpr int CPR = HD / 8;          // 16-byte chunks of one K row
    constexpr int KCH = HD / 16;         // chunks of the K tile per thread: 128 * CPR / 256
    __shared__ __attribute__((aligned(16))) bf16 sK[2][AP_MAX_KEYS * LDK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int64_t b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int64_t qrow = tile * AP_ROWS + wave * 16 + col;
    const bool qok = qrow < a.Sq;
    const int Skv = (int)a.Skv;
    const int nkb = (Skv + 15) >> 4;
    const int nchunks = Skv * CPR;

    // rows [Skv, 16 nkb) of both buffers: zero once, no head writes them
    for (int c = nchunks + tid; c < nkb * 16 * CPR; c += AP_THREADS) {
        const int off = (c / CPR) * LDK + (c % CPR) * 8;
        *reinterpret_cast<uint4*>(&sK[0][off]) = make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4*>(&sK[1][off]) = make_uint4(0, 0, 0, 0);
    }

    const bool biased = a.kbias != nullptr;
    if (biased)     // key j's bias -> the padding of row j of buffer 0 (rows [Skv, 16 nkb): 0, those keys are masked below)
        for (int j = tid; j < nkb * 16; j += AP_THREADS)
            *reinterpret_cast<float*>(&sK[0][j * LDK + HD]) = j < Skv ? a.kbias[b * a.ldb + j] : 0.f;

    const bf16* qp = a.q + b * a.sq + (qok ? qrow : 0) * a.ldq + 8 * quad;
    const bf16* kp = a.k + b * a.sk;

    uint4 kr[KCH];
    bf16x8 qf[KS], qn[KS];
// the K tile of head h_: global -> registers, registers -> LDS buffer buf_; the Q fragments of head h_ (rows past Sq - 1 are never read)
#define AP_LOAD_K(h_)                                                                                                             \
    _Pragma("unroll") for (int i = 0; i < KCH; ++i) {                                                                            \
        const int c = tid + i * AP_THREADS;                                                                                      \
        kr[i] = c < nchunks ? *reinterpret_cast<const uint4*>(kp + (h_) * a.hsk + (int64_t)(c / CPR) * a.ldk + (c % CPR) * 8)    \
                            : make_uint4(0, 0, 0, 0);                                                                            \
    }
#define AP_STORE_K(buf_)                                                                                                          \
    _Pragma("unroll") for (int i = 0; i < KCH; ++i) {                                                                            \
        const int c = tid + i * AP_THREADS;                                                                                      \
        if (c < nchunks) *reinterpret_cast<uint4*>(&sK[buf_][(c / CPR) * LDK + (c % CPR) * 8]) = kr[i];                          \
    }
#define AP_LOAD_Q(h_, f_)                                                                                                         \
    _Pragma("unroll") for (int kk = 0; kk < KS; ++kk) {                                                                          \
        U128 t;                                                                                                                   \
        t.u = qok ? *reinterpret_cast<const uint4*>(qp + (h_) * a.hsq + kk * 32) : make_uint4(0, 0, 0, 0);                        \
        f_[kk] = t.h;                                                                                                             \
    }

    AP_LOAD_K(0)
    AP_LOAD_Q(0, qf)
    AP_STORE_K(0)
    __syncthreads();

    f32x4 hs[AP_MAX_KB];
#pragma unroll
    for (int kb = 0; kb < AP_MAX_KB; ++kb) hs[kb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int64_t h = 0; h < a.H; ++h) {
        const int buf = (int)(h & 1);
        const bool more = h + 1 < a.H;
        if (more) {
            AP_LOAD_K(h + 1)
            AP_LOAD_Q(h + 1, qn)
        }
        // S^T block kb: keys 16 kb .. 16 kb + 15 x the wave's 16 queries
        f32x4 s[AP_MAX_KB];
        float m = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < AP_MAX_KB; ++kb) {
            if (kb < nkb) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    const bf16x8 kf = ld_bf16x8(&sK[buf][(16 * kb + col) * LDK + kk * 32 + 8 * quad]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[r] * a.scale;
                    if (biased) v = v + *reinterpret_cast<const float*>(&sK[0][(16 * kb + 4 * quad + r) * LDK + HD]);
                    v = (16 * kb + 4 * quad + r < Skv) ? v : -INFINITY;
                    s[kb][r] = v;
                    m = fmaxf(m, v);
                }
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));      // a real key with a finite bias exists (the caller's contract): the maximum is finite
        float sum = 0.f;
#pragma unroll
        for (int kb = 0; kb < AP_MAX_KB; ++kb) {
            if (kb < nkb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f((s[kb][r] - m) * 1.4426950408889634f);   // exp2(-inf) = 0: the padded keys
                    s[kb][r] = p;
                    sum += p;
                }
            }
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = fast_rcp(sum);           // sum >= 1: the maximum's own term
#pragma unroll
        for (int kb = 0; kb < AP_MAX_KB; ++kb) {
            if (kb < nkb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) hs[kb][r] += s[kb][r] * inv;
            }
        }
        if (more) {
            AP_STORE_K(buf ^ 1)                    // last read while head h - 1 was computed: every wave is past that barrier
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) qf[kk] = qn[kk];
        }
        __syncthreads();
    }

#undef AP_LOAD_K
#undef AP_STORE_K
#undef AP_LOAD_Q
    if (!qok) return;
    const int64_t gr = b * a.Sq + qrow;
    const int64_t orow = a.out_rows ? (int64_t)a.out_rows[gr] : gr;
    float* o = a.out + orow * a.ldo + 4 * quad;
#pragma unroll
    for (int kb = 0; kb < AP_MAX_KB; ++kb) {
        if (kb < nkb) {
            const int key0 = 16 * kb + 4 * quad;
            if (key0 + 4 <= Skv) {
                float4* p4 = reinterpret_cast<float4*>(o + 16 * kb);
                float4 v = *p4;
                v.x += hs[kb][0] * a.inv_h;
                v.y += hs[kb][1] * a.inv_h;
                v.z += hs[kb][2] * a.inv_h;
                v.w += hs[kb][3] * a.inv_h;
                *p4 = v;
            } else {                               // the ragged group: columns [Skv, ldo) are not touched
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (key0 + r < Skv) o[16 * kb + r] += hs[kb][r] * a.inv_h;
            }
        }
    }
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int launch_probs(const md_attn_args* a, const float* kbias, int64_t ldb, float* out, int64_t ldo, const int32_t* out_rows, hipStream_t stream) {
    if (!a || !a->q || !a->k || !out) return MD_BAD_ARG;
    if (a->B < 1 || a->H < 1 || a->Sq < 1 || a->Skv < 1 || a->Skv > AP_MAX_KEYS || (a->hd != 32 && a->hd != 64)) return MD_BAD_ARG;
    if (ldo < a->Skv || ldo % 4 != 0 || !aligned16(out)) return MD_BAD_ARG;
    if (a->ldq % 8 || a->ldk % 8 || a->sq % 8 || a->sk % 8 || a->hsq % 8 || a->hsk % 8 || !aligned16(a->q) || !aligned16(a->k)) return MD_BAD_ARG;
    ap_args p;
    p.q = reinterpret_cast<const bf16*>(a->q);
    p.k = reinterpret_cast<const bf16*>(a->k);
    p.kbias = kbias;
    p.ldb = ldb;
    p.out = out;
    p.out_rows = out_rows;
    p.H = a->H, p.Sq = a->Sq, p.Skv = a->Skv, p.ldq = a->ldq, p.ldk = a->ldk, p.sq = a->sq, p.sk = a->sk;
    p.hsq = a->hsq ? a->hsq : a->hd;             // 0 = heads packed side by side in the row, as md_attn_fwd reads it
    p.hsk = a->hsk ? a->hsk : a->hd;
    p.ldo = ldo;
    p.tiles = (a->Sq + AP_ROWS - 1) / AP_ROWS;
    p.scale = a->scale;
    p.inv_h = 1.0f / (float)a->H;
    if (p.tiles > 0x7fffffff / a->B) return MD_BAD_ARG;     // the grid's x dimension carries (sample, tile)
    const dim3 grid((unsigned)(p.tiles * a->B));
    if (a->hd == 64) hipLaunchKernelGGL((attn_probs_kernel<64>), grid, dim3(AP_THREADS), 0, stream, p);
    else hipLaunchKernelGGL((attn_probs_kernel<32>), grid, dim3(AP_THREADS), 0, stream, p);
    MD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int md_attn_probs(const md_attn_args* a, float* out, int64_t ldo, const int32_t* out_rows, hipStream_t stream) {
    return launch_probs(a, nullptr, 0, out, ldo, out_rows, stream);
}

extern "C" int md_attn_probs_kbias(const md_attn_args* a, const float* kbias, int64_t ldb, float* out, int64_t ldo, const int32_t* out_rows,
                                   hipStream_t stream) {
    if (!kbias || !aligned16(kbias) || !a || ldb < a->Skv || ldb % 4 != 0) return MD_BAD_ARG;
    return launch_probs(a, kbias, ldb, out, ldo, out_rows, stream);
}
