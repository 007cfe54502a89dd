"""md_lora_wgrad (csrc/lora_wgrad.hip, DESIGN.md 4.13 "Factored backward") through ctypes: the adapter's gradient of one linear
straight from dy [M, N] and x [M, K], dB += c dy^T (x A^T), dA += c (dy B)^T x.

Exact cases in the manner of tests/gemm_exact.py: x, dy, A, B in {-1, 0, 1} with at most 256 non-zeros per row of A and per column of
B, so P = x A^T and Q = dy B are integers of magnitude <= 256 (exact in bf16), every sum stays below 2^24 and the result must equal the
integer reference bit for bit whatever the kernel keeps internally.  The guard-band form surrounds the logical extents of dy and x
(64 rows past M, the pad columns of a leading dimension) and the whole workspace with NaN.

Random data against lora.ref_wgrad_factored (fp64 on the same bf16 x, dy and fp32 A, B), every element, u = 2^-9, U = 2^-24:
    |dB^ - dB|[n, j] <= c (2 u + (M + K + 8) U) sum_m |dy[m, n]| sum_k |x[m, k]| |A[j, k]|
    |dA^ - dA|[j, k] <= c (2 u + (M + N + 8) U) sum_m (sum_n |dy[m, n]| |B[n, j]|) |x[m, k]|
(one rounding of A resp. B and one of P resp. Q to bf16, then fp32 accumulation over K resp. N and over M)."""
import ctypes

import pytest
import torch

from micro_diffusion_amd import lora

pytestmark = pytest.mark.gpu

u, U = 2.0 ** -9, 2.0 ** -24
BAD = -1

# (M, N, K, rank, lddy, ldx, column offset of the dy pointer)
EXACT = [(1, 8, 64, 4, 8, 64, 0), (154, 128, 64, 16, 128, 64, 0), (200, 96, 128, 8, 192, 128, 96), (1000, 24, 256, 64, 24, 264, 0),
         (300, 3072, 1024, 16, 3072, 1024, 0), (4096, 128, 64, 32, 128, 64, 0), ("three strips", 128, 64, 32, 128, 64, 0)]


def _geometry(hip, M, N, K, r):
    strip, groups = ctypes.c_int32(0), ctypes.c_int32(0)
    assert hip.lib().md_lora_wgrad_geometry(M, N, K, r, ctypes.byref(strip), ctypes.byref(groups)) == 0
    return strip.value, groups.value


def _three_strip_m(hip, M, N, K, r):
    """The smallest multiple of 8 above M at which some workgroup of the reduction takes at least three strips (workgroup g takes the
    strips g, g + groups, ...: the first one takes ceil(strips / groups))."""
    while True:
        strip, groups = _geometry(hip, M, N, K, r)
        strips = -(-M // strip)
        if -(-strips // groups) >= 3:
            return M
        M += 8


def _ws(hip, M, N, K, r, fill=None):
    need = ctypes.c_int64(-1)
    assert hip.lib().md_lora_wgrad_ws_floats(M, N, K, r, ctypes.byref(need)) == 0 and need.value > 0
    ws = torch.empty(need.value, device="cuda", dtype=torch.float32)
    if fill is not None:
        ws.fill_(fill)
    return ws


def _embed(t, ld, off, pad_rows, fill):
    """t [M, C] inside a [(M + pad_rows), ld] bf16 allocation filled with `fill`, at column `off`; returns (allocation, pointer)."""
    M, C = t.shape
    buf = torch.full((M + pad_rows, ld), fill, dtype=torch.bfloat16, device="cuda")
    buf[:M, off:off + C] = t.to(torch.bfloat16).cuda()
    return buf, buf.data_ptr() + 2 * off


def _call(hip, dy_ptr, lddy, x_ptr, ldx, M, N, K, A, B, r, c, dA, dB, ws, ws_floats=None):
    return hip.lib().md_lora_wgrad(dy_ptr, lddy, x_ptr, ldx, M, N, K, A.data_ptr(), B.data_ptr(), r, c, dA.data_ptr(), dB.data_ptr(),
                                   ws.data_ptr(), ws.numel() if ws_floats is None else ws_floats, hip.stream_ptr())


def _ternary(shape, gen):
    return torch.randint(-1, 2, shape, generator=gen).float()


def _sparse_ternary(rows, cols, gen, nnz=256):
    """{-1, 0, 1} with at most `nnz` non-zeros per row."""
    t = _ternary((rows, cols), gen)
    if cols > nnz:
        keep = torch.zeros(rows, cols)
        idx = torch.stack([torch.randperm(cols, generator=gen)[:nnz] for _ in range(rows)])
        keep.scatter_(1, idx, 1.0)
        t = t * keep
    return t


def _exact_case(hip, case, guard, c):
    M, N, K, r, lddy, ldx, off = case
    if M == "three strips":
        M = _three_strip_m(hip, 4096, N, K, r)
        strip, groups = _geometry(hip, M, N, K, r)
        print(f"three strips: M = {M} (strips of {strip} rows, {groups} row groups)")
        assert M % 8 == 0 and M * max(N, K) < 2 ** 24
    gen = torch.Generator().manual_seed(M + 3 * N + 7 * K + r)
    x, dy = _ternary((M, K), gen), _ternary((M, N), gen)
    A = _sparse_ternary(r, K, gen)
    B = _sparse_ternary(r, N, gen).t().contiguous()              # at most 256 non-zeros per COLUMN of B [N, r]
    dA0 = torch.randint(-3, 4, (r, K), generator=gen).float()
    dB0 = torch.randint(-3, 4, (N, r), generator=gen).float()
    P, Q = x.double() @ A.double().t(), dy.double() @ B.double()
    assert float(P.abs().max()) <= 256 and float(Q.abs().max()) <= 256
    wantA = dA0.double() + c * (Q.t() @ x.double())
    wantB = dB0.double() + c * (dy.double().t() @ P)
    assert float(wantA.abs().max()) < 2 ** 24 and float(wantB.abs().max()) < 2 ** 24
    fill = float("nan") if guard else 0.0
    pad = 64 if guard else 0
    dyb, dyp = _embed(dy, lddy, off, pad, fill)
    xb, xp = _embed(x, ldx, 0, pad, fill)
    ws = _ws(hip, M, N, K, r, fill=float("nan") if guard else None)
    Ad, Bd, dA, dB = A.cuda(), B.cuda(), dA0.cuda(), dB0.cuda()
    assert _call(hip, dyp, lddy, xp, ldx, M, N, K, Ad, Bd, r, c, dA, dB, ws) == 0
    torch.cuda.synchronize()
    for name, got, want in (("dA", dA, wantA), ("dB", dB, wantB)):
        bad = int((got.cpu().double() != want).sum())
        print(f"{name} M={M} N={N} K={K} r={r} guard={guard}: {bad} of {want.numel()} elements differ from the integer reference")
        assert bad == 0 and bool(want.any())


@pytest.mark.parametrize("c", [1.0, 0.5])
@pytest.mark.parametrize("case", EXACT, ids=lambda s: "-".join(str(v) for v in s))
def test_exact(hip, case, c):
    _exact_case(hip, case, False, c)


@pytest.mark.parametrize("case", EXACT, ids=lambda s: "-".join(str(v) for v in s))
def test_exact_inside_nan_guard_bands(hip, case):
    _exact_case(hip, case, True, 1.0)


@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("M,N,K", [(154, 128, 64), (1000, 192, 256), (300, 3072, 1024)])
def test_random_against_fp64(hip, M, N, K, r):
    gen = torch.Generator().manual_seed(M + N + K + r)
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    dy = torch.randn(M, N, generator=gen).to(torch.bfloat16)
    A = torch.randn(r, K, generator=gen) / K ** 0.5
    B = torch.randn(N, r, generator=gen) * 0.05
    c = 0.75
    rA, rB = lora.ref_wgrad_factored(dy, x, A, B, c)
    xa, dya = x.double().abs(), dy.double().abs()
    bB = c * (2 * u + (M + K + 8) * U) * (dya.t() @ (xa @ A.double().abs().t()))
    bA = c * (2 * u + (M + N + 8) * U) * ((dya @ B.double().abs()).t() @ xa)
    xd, dyd = x.cuda(), dy.cuda()
    dA, dB = torch.zeros(r, K, device="cuda"), torch.zeros(N, r, device="cuda")
    ws = _ws(hip, M, N, K, r)
    assert _call(hip, dyd.data_ptr(), N, xd.data_ptr(), K, M, N, K, A.cuda(), B.cuda(), r, c, dA, dB, ws) == 0
    torch.cuda.synchronize()
    wA = float(((dA.cpu().double() - rA).abs() / bA).max())
    wB = float(((dB.cpu().double() - rB).abs() / bB).max())
    print(f"M={M} N={N} K={K} r={r}: max |dA - ref| / bound = {wA:.4f}, max |dB - ref| / bound = {wB:.4f}")
    assert wA <= 1.0 and wB <= 1.0 and bool(rA.any()) and bool(rB.any())


def test_zero_b_repeat_and_nan(hip):
    M, N, K, r = 300, 136, 72, 8
    gen = torch.Generator().manual_seed(5)
    x, dy = torch.randn(M, K, generator=gen).to(torch.bfloat16).cuda(), torch.randn(M, N, generator=gen).to(torch.bfloat16).cuda()
    A = (torch.randn(r, K, generator=gen) / K ** 0.5).cuda()
    B = (torch.randn(N, r, generator=gen) * 0.05).cuda()
    ws = _ws(hip, M, N, K, r)
    # B = 0: a fresh adapter has a zero dA -- what is there stays bit for bit
    dA0 = torch.randn(r, K, generator=gen).cuda()
    dA, dB = dA0.clone(), torch.zeros(N, r, device="cuda")
    assert _call(hip, dy.data_ptr(), N, x.data_ptr(), K, M, N, K, A, torch.zeros_like(B), r, 1.0, dA, dB, ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(dA.view(torch.int32), dA0.view(torch.int32)) and bool(dB.any())
    # two calls on the same data: identical bits (the second one on a workspace the first one left behind)
    outs = []
    for _ in range(2):
        dA, dB = torch.zeros(r, K, device="cuda"), torch.zeros(N, r, device="cuda")
        assert _call(hip, dy.data_ptr(), N, x.data_ptr(), K, M, N, K, A, B, r, 0.5, dA, dB, ws) == 0
        torch.cuda.synchronize()
        outs.append((dA.clone(), dB.clone()))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)) and bool(outs[0][0].any())
    # one NaN in dy inside the extents: the step guard relies on its reaching the gradient
    dyn = dy.clone()
    dyn[M - 3, 77] = float("nan")
    dA, dB = torch.zeros(r, K, device="cuda"), torch.zeros(N, r, device="cuda")
    assert _call(hip, dyn.data_ptr(), N, x.data_ptr(), K, M, N, K, A, B, r, 1.0, dA, dB, ws) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(dB[77]).any()), "row 77 of dB"
    rest = torch.cat([dB[:77], dB[78:]])
    assert bool(torch.isfinite(rest).all()) and torch.equal(rest, torch.cat([outs[0][1][:77], outs[0][1][78:]]) * 2.0)


def test_refusals_launch_nothing(hip):
    M, N, K, r = 64, 32, 64, 8
    x = torch.ones(M, 72, dtype=torch.bfloat16, device="cuda")
    dy = torch.ones(M, 40, dtype=torch.bfloat16, device="cuda")
    A, B = torch.ones(16, 64, device="cuda"), torch.ones(N, 16, device="cuda")
    dA, dB = torch.full((16, 64), 3.0, device="cuda"), torch.full((N, 16), 5.0, device="cuda")
    ws = _ws(hip, M, N, K, 16)
    need = ctypes.c_int64(-1)
    L = hip.lib()
    for args in ((M, N, K, 12), (M, N, 60, r), (0, N, K, r), (M, 0, K, r)):
        assert L.md_lora_wgrad_ws_floats(*args, ctypes.byref(need)) == BAD, args
    assert L.md_lora_wgrad_ws_floats(M, N, K, r, None) == BAD

    def call(lddy=40, ldx=72, K=K, r=r, dyp=None, xp=None, a=A, dA_=dA, ws_floats=None):
        return L.md_lora_wgrad(dy.data_ptr() if dyp is None else dyp, lddy, x.data_ptr() if xp is None else xp, ldx, M, N, K,
                               a if a is None else a.data_ptr(), B.data_ptr(), r, 1.0, dA_ if dA_ is None else dA_.data_ptr(), dB.data_ptr(),
                               ws.data_ptr(), ws.numel() if ws_floats is None else ws_floats, hip.stream_ptr())

    need_ok = ctypes.c_int64(-1)
    assert L.md_lora_wgrad_ws_floats(M, N, K, r, ctypes.byref(need_ok)) == 0
    bad = {"rank 12": dict(r=12), "K = 60": dict(K=60), "lddy < N": dict(lddy=24), "ldx % 8": dict(ldx=68), "NULL A": dict(a=None),
           "NULL dA": dict(dA_=None), "NULL dy": dict(dyp=0), "short ws": dict(ws_floats=need_ok.value - 1),
           "misaligned x": dict(xp=x.data_ptr() + 2)}
    for why, kw in bad.items():
        assert call(**kw) == BAD, why
    torch.cuda.synchronize()
    assert bool((dA == 3.0).all()) and bool((dB == 5.0).all()), "a refused call must leave the outputs alone"
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((dA[:r] == 3.0).any()) and not bool((dB[:, :r] == 5.0).all())
