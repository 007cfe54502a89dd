// The token-space geometry of the sampler's elementwise kernels (edm.hip, guide.hip), once.
// The network reads bf16 patch rows and writes bf16 token rows; the fp64 sampler state is the only image-shaped tensor.  A work item is
// one 8-element (16-byte) segment of one token row; items are ordered (b, ti, segment, tj) with tj fastest, so the lanes of a wave walk
// along w: the image-shaped operands are read / written along w and every lane moves its bf16 segment as one 16-byte piece (VEC; rows
// that are no multiple of 8 wide, or a misaligned base, go element by element).
#pragma once
#include "md_common.h"

struct tok_item {
    int64_t b, row;     // sample, token row b * T + ti * gw + tj
    int ti, tj, e0;     // grid position, first element of the segment
};
__device__ __forceinline__ tok_item tok_item_of(int64_t i, int gh, int gw, int nseg) {
    tok_item t;
    t.tj = (int)(i % gw);
    const int64_t r = i / gw;
    t.e0 = (int)(r % nseg) * 8;
    const int64_t bt = r / nseg;
    t.ti = (int)(bt % gh);
    t.b = bt / gh;
    t.row = (t.b * gh + t.ti) * gw + t.tj;
    return t;
}
// image offset of element e = (ph * p + pw) * C + c (the order of the network's output rows) of the token at (b, ti, tj)
__device__ __forceinline__ int64_t tok_pixel(const tok_item& t, int e, int C, int H, int W, int p) {
    const int c = e % C, pw = (e / C) % p, ph = e / (C * p);
    return ((t.b * C + c) * H + t.ti * p + ph) * W + t.tj * p + pw;
}

// Everything a token-space entry point refuses about its sizes (p is tested before it divides).
inline bool tok_geometry_ok(int64_t B, int C, int H, int W, int p) { return B > 0 && C > 0 && H > 0 && W > 0 && p > 0 && H % p == 0 && W % p == 0; }

struct tok_geometry {
    int64_t B;
    int C, H, W, p;
    int gh, gw, pv, nseg;       // token grid, row width C * p * p, 8-element segments per row (the last may be ragged)
    __host__ __device__ int64_t rows() const { return B * gh * gw; }
    __host__ __device__ int64_t items() const { return rows() * nseg; }
};
__host__ __device__ inline tok_geometry tok_geometry_of(int64_t B, int C, int H, int W, int p) {
    const int pv = C * p * p;
    return {B, C, H, W, p, H / p, W / p, pv, (pv + 7) / 8};
}

inline bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }
