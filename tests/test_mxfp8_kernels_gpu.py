"""md_mx_quant_rows, md_gemm_mxfp8 and md_swiglu_fwd_mx against tests/mx_ref.py.

Quantiser: bit-exact, elements and scale bytes, on random bf16 with planted blocks (zero, the saturation case amax = 460 * 2^j, results
that are e4m3 subnormals, one huge element, bf16-subnormal inputs), rows in {1, 7, 129} x K in {32, 128, 416}, both source layouts,
ld > K, batch 3 with strides, guard bands untouched.

GEMM, exact: small-integer operands (|v| <= 8) with a different power-of-two scale per (row, k-block) -- 2^-2 ... 2^2 on A, 2^-1 ... 2^1
on B -- so that every product is a multiple of 2^-3 below 2^9 and every partial sum of K <= 640 of them stays below 2^24 in units of
2^-3: the fp32 accumulation is exact in any order, and the result must EQUAL bf16(exact).  Because rows, columns and k-blocks all carry
their own data and their own scale, a wrong operand lane map, a swapped operand or a scale taken from the wrong block changes the
result; these cases are what establishes the lane map of v_mfma_scale_f32_16x16x128_f8f6f4 that gemm_mxfp8.hip states.  T = 128 is the
kernel's tile edge: M in {1, T-1, T+1, 2T+17} x N in {16, T, T+16} x K in {128, 256, 640} x batch in {1, 3}, leading dimensions wider
than the matrices, guard bands checked.  Bias + GELU(erf) is compared with apply_act's formula in fp64 within one bf16 ulp; the gated
residual (rows_per_sample = 50, not a divisor of T) is exact.  K = 96 and N = 8 return MD_NOT_ELIGIBLE and write nothing.

GEMM, random data: against the fp64 product of the dequantised operands, every element within
(K - 1) * 2^-23 * sum_k |a_k b_k| (fp32 summation in any order, with truncation) + 2^-8 * |exact| (the bf16 store).
"""

import pytest
import torch

from micro_diffusion_amd import hip
from tests import mx_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 128
GUARD = 2            # guard rows before and after every matrix
FP8 = torch.float8_e4m3fn


class Banded:
    """A [planes, rows, cols] matrix inside a raw buffer with leading dimension ld > cols, GUARD rows of sentinel before and after every
    plane; `untouched()` is True when nothing but the interior changed."""

    def __init__(self, planes, rows, cols, ld, dtype, sentinel):
        self.planes, self.rows, self.cols, self.ld = planes, rows, cols, ld
        self.prows = rows + 2 * GUARD
        self.raw = torch.full((planes, self.prows, ld), sentinel, dtype=dtype, device=DEV)
        self.before = self.raw.clone()

    @property
    def view(self):
        return self.raw[:, GUARD:GUARD + self.rows, :self.cols]

    def set(self, vals):
        self.view.copy_(vals.to(self.raw.dtype).reshape(self.planes, self.rows, self.cols))
        self.before = self.raw.clone()

    def ptr(self):
        return self.raw.data_ptr() + GUARD * self.ld * self.raw.element_size()

    @property
    def stride(self):          # elements between planes
        return self.prows * self.ld

    def untouched(self):
        a, b = self.raw.clone(), self.before.clone()
        a[:, GUARD:GUARD + self.rows, :self.cols] = 0
        b[:, GUARD:GUARD + self.rows, :self.cols] = 0
        return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ quantiser
def quant_input(batch, rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(batch, rows, K, generator=g) * torch.exp2(torch.randint(-12, 12, (batch, rows, K // 32, 1), generator=g).float())
         .expand(-1, -1, -1, 32).reshape(batch, rows, K)).to(torch.bfloat16)
    xb = x.view(batch, rows, K // 32, 32)
    nb = K // 32
    for b in range(batch):
        for r in range(rows):
            kind = (r + b) % 6
            kb = (r * 7 + b) % nb
            if kind == 0:
                xb[b, r, kb] = 0                                             # a zero block
            elif kind == 1:
                xb[b, r, kb, 5] = 460.0 * 2.0 ** ((r % 9) - 4)               # saturation: amax in (448, 512) * 2^X
                xb[b, r, kb, 6] = -460.0 * 2.0 ** ((r % 9) - 4)
            elif kind == 2:
                xb[b, r, kb] = (torch.arange(32) - 16).float() * 2.0 ** -9    # e4m3 subnormal results next to amax = 256
                xb[b, r, kb, 0] = 256.0
            elif kind == 3:
                xb[b, r, kb, 31] = 2.0 ** 100                                # one huge element: the others flush to zero
            elif kind == 4:
                xb[b, r, kb] = (torch.arange(32).float() * 2.0 ** -133).to(torch.bfloat16)   # bf16 subnormals: X clamps to -127
    return x


QUANT_CASES = [(rows, K, kc, batch) for rows in (1, 7, 129) for K in (32, 128, 416) for kc in (1, 0) for batch in (1,)]
QUANT_CASES += [(7, 128, 1, 3), (129, 416, 0, 3), (16, 32, 0, 3)]


@pytest.mark.parametrize("rows,K,kc,batch", QUANT_CASES)
def test_quant_rows_bit_exact(rows, K, kc, batch):
    x = quant_input(batch, rows, K, 1000 + rows + K + kc)
    q_ref, s_ref = mx_ref.mx_quantize(x)
    if kc:
        src = Banded(batch, rows, K, K + 24, torch.bfloat16, 7.0)
        src.set(x)
    else:
        src = Banded(batch, K, rows, (rows + 7) // 8 * 8 + 16, torch.bfloat16, 7.0)
        src.set(x.transpose(1, 2))
    dst = Banded(batch, rows, K, K + 48, torch.uint8, 0xAB)
    sc = Banded(batch, rows, K // 32, K // 32 + 3, torch.uint8, 0xCD)
    hip.mx_quant_rows(src.ptr(), dst.ptr(), sc.ptr(), rows, K, ld=src.ld, ldd=dst.ld, lds=sc.ld, src_kcontig=bool(kc), batch=batch,
                      sSrc=src.stride, sDst=dst.stride, sScale=sc.stride)
    torch.cuda.synchronize()
    assert torch.equal(sc.view.cpu(), s_ref), "scale bytes differ"
    assert torch.equal(dst.view.cpu(), q_ref.view(torch.uint8)), "elements differ"
    assert dst.untouched() and sc.untouched() and src.untouched()
    assert torch.equal(src.view.cpu().view(torch.int16), (x if kc else x.transpose(1, 2)).contiguous().view(torch.int16))


def test_quant_rows_refuses_bad_arguments():
    x = torch.zeros(8, 64, dtype=torch.bfloat16, device=DEV)
    q = torch.full((8, 64), 0xAB, dtype=torch.uint8, device=DEV)
    s = torch.full((8, 2), 0xCD, dtype=torch.uint8, device=DEV)
    assert hip.mx_quant_rows(x, q, s, 8, 48, ld=64, ldd=64, lds=2, expect=None) == -1          # K % 32
    assert hip.mx_quant_rows(x, q, s, 8, 64, ld=64, ldd=56, lds=2, expect=None) == -1          # ldd < K
    torch.cuda.synchronize()
    assert bool((q == 0xAB).all()) and bool((s == 0xCD).all())


# ------------------------------------------------------------------------------------------------------------------ GEMM
def int_operand(batch, rows, K, max_shift, seed):
    """Integer elements |v| <= 8 as fp8 and scale bytes 127 + s, s in [-max_shift, max_shift], one per (row, k-block)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-8, 9, (batch, rows, K), generator=g).float()
    s = (torch.randint(-max_shift, max_shift + 1, (batch, rows, K // 32), generator=g) + 127).to(torch.uint8)
    return v.to(FP8), s


def upload(q, s, K):
    batch, rows = q.shape[0], q.shape[1]
    qb = Banded(batch, rows, K, K + 32, torch.uint8, 0x7F)          # sentinel 0x7f: the e4m3fn NaN
    qb.set(q.view(torch.uint8))
    sb = Banded(batch, rows, K // 32, K // 32 + 5, torch.uint8, 0xFF)   # sentinel 0xff: the e8m0 NaN
    sb.set(s)
    return qb, sb


def launch(A, SA, Bm, SB, C, M, N, K, batch, **kw):
    return hip.gemm_mxfp8(A.ptr(), SA.ptr(), Bm.ptr(), SB.ptr(), C.ptr(), M, N, K, lda=A.ld, ldb=Bm.ld, ldsa=SA.ld, ldsb=SB.ld, ldc=C.ld,
                          batch=batch, sA=A.stride, sB=Bm.stride, sScaleA=SA.stride, sScaleB=SB.stride, sC=C.stride, **kw)


def exact_problem(M, N, K, batch, seed):
    qa, sa = int_operand(batch, M, K, 2, seed)
    qb, sb = int_operand(batch, N, K, 1, seed + 1)
    da, db = mx_ref.mx_dequantize(qa, sa), mx_ref.mx_dequantize(qb, sb)
    ref = da @ db.transpose(1, 2)                                                           # fp64: exact
    assert float((da.abs() @ db.abs().transpose(1, 2)).max()) * 8 < 2 ** 24                 # every partial sum, in units of 2^-3
    return qa, sa, qb, sb, ref


@pytest.mark.parametrize("K", (128, 256, 640))
@pytest.mark.parametrize("batch", (1, 3))
def test_gemm_exact_integers(K, batch):
    for M in (1, T - 1, T + 1, 2 * T + 17):
        for N in (16, T, T + 16):
            qa, sa, qb, sb, ref = exact_problem(M, N, K, batch, 17 * M + N + K + batch)
            A, SA = upload(qa, sa, K)
            Bm, SB = upload(qb, sb, K)
            C = Banded(batch, M, N, N + 24, torch.bfloat16, -777.0)
            launch(A, SA, Bm, SB, C, M, N, K, batch)
            torch.cuda.synchronize()
            want = ref.to(torch.bfloat16)
            got = C.view.cpu()
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
                f"M={M} N={N} K={K} batch={batch}: {int((got != want).sum())} of {got.numel()} elements differ"
            assert C.untouched() and A.untouched() and Bm.untouched() and SA.untouched() and SB.untouched()


def gelu_erf_formula(x):
    """apply_act(MD_ACT_GELU_ERF) of csrc/md_common.h (normal CDF through Abramowitz-Stegun 7.1.26) in fp64."""
    z = x.abs() * 0.7071067811865476
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    q = 0.5 * poly * torch.exp(-z * z)
    return x * torch.where(x < 0, q, 1.0 - q)


def bf16_ulp(x):
    """One bf16 unit in the last place at |x| (fp64), never below the smallest normal's."""
    _, e = torch.frexp(x.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 1 - 7)


def test_gemm_bias_gelu_epilogue():
    """Integer pre-activations of GELU's own range: elements |v| <= 2, A sparse (one element in 32), unit scales, integer bias, so acc +
    bias is an integer of a few units (exact, checked through C2).  On integers the formula never lands in the fp32-subnormal window
    [2^-149, 2^-126), where the hardware exponential behind apply_act returns 0: gelu(-13) = -7.9e-38 is a normal number and |gelu(x)| <
    2^-134, half the smallest bf16 step, for every integer x <= -14.  (Pre-activations between about -13.4 and -13.0 do land there and
    come out as 0, up to 50 bf16 steps of 2^-133 from the formula: measured with operands scaled by 2^-7; the bf16 family's epilogue
    shares this, it is a property of apply_act.)"""
    M, N, K = T + 1, T + 16, 256
    g = torch.Generator().manual_seed(5)
    va = torch.randint(-2, 3, (1, M, K), generator=g).float() * (torch.rand(1, M, K, generator=g) < 1 / 32)
    vb = torch.randint(-2, 3, (1, N, K), generator=g).float()
    qa, qb = va.to(FP8), vb.to(FP8)
    sa = torch.full((1, M, K // 32), 127, dtype=torch.uint8)
    sb = torch.full((1, N, K // 32), 127, dtype=torch.uint8)
    pre = mx_ref.mx_dequantize(qa, sa) @ mx_ref.mx_dequantize(qb, sb).transpose(1, 2)
    bias = torch.randint(-3, 4, (N,), generator=g).float()
    pre = pre + bias.double()
    assert float(pre.min()) < -6 and float(pre.max()) > 6 and bool((pre == pre.round()).all())
    A, SA = upload(qa, sa, K)
    Bm, SB = upload(qb, sb, K)
    C = Banded(1, M, N, N + 8, torch.bfloat16, -777.0)
    C2 = Banded(1, M, N, N + 16, torch.bfloat16, -555.0)
    launch(A, SA, Bm, SB, C, M, N, K, 1, bias=bias.to(DEV), act=hip.ACT_GELU_ERF, C2=C2.ptr(), ldc2=C2.ld)
    torch.cuda.synchronize()
    assert torch.equal(C2.view.cpu().view(torch.int16), pre.to(torch.bfloat16).view(torch.int16)), "C2 = bf16(acc + bias) must be exact"
    want = gelu_erf_formula(pre)
    err = (C.view.cpu().double() - want).abs()
    worst = float((err / bf16_ulp(want)).max())
    print(f"bias + GELU: worst error {worst:.3f} bf16 ulp")
    assert bool((err <= bf16_ulp(want)).all()), worst
    assert C.untouched() and C2.untouched()


def test_gemm_gated_residual_epilogue():
    M, N, K, rps = 150, T + 16, 256, 50
    g = torch.Generator().manual_seed(6)
    qa, sa, qb, sb, ref = exact_problem(M, N, K, 1, 60)
    res = torch.randint(-256, 257, (1, M, N), generator=g).to(torch.bfloat16)
    gate = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (1, M // rps, N), generator=g)].to(torch.bfloat16)
    A, SA = upload(qa, sa, K)
    Bm, SB = upload(qb, sb, K)
    R = Banded(1, M, N, N + 8, torch.bfloat16, 3.0)
    R.set(res)
    G = Banded(1, M // rps, N, N + 40, torch.bfloat16, 5.0)
    G.set(gate)
    for with_gate in (True, False):
        C = Banded(1, M, N, N + 24, torch.bfloat16, -777.0)
        C2 = Banded(1, M, N, N, torch.bfloat16, -555.0)
        launch(A, SA, Bm, SB, C, M, N, K, 1, mode=hip.EPI_RESIDUAL, res=R.ptr(), ldr=R.ld, gate=G.ptr() if with_gate else None, ldg=G.ld,
               rows_per_sample=rps if with_gate else 0, C2=C2.ptr(), ldc2=C2.ld)
        torch.cuda.synchronize()
        br = ref.to(torch.bfloat16)                                     # one rounding of the accumulator
        gg = gate.double().repeat_interleave(rps, dim=1) if with_gate else 1.0
        want = (res.double() + gg * br.double()).to(torch.bfloat16)     # exact in fp32, one rounding to bf16
        assert torch.equal(C2.view.cpu().view(torch.int16), br.view(torch.int16))
        assert torch.equal(C.view.cpu().view(torch.int16), want.view(torch.int16)), f"gate={with_gate}"
        assert C.untouched() and C2.untouched() and R.untouched() and G.untouched()


@pytest.mark.parametrize("M,N,K", [(64, 128, 96), (64, 8, 128)])
def test_gemm_ineligible_launches_nothing(M, N, K):
    Kp = (K + 127) // 128 * 128
    A = torch.zeros(M, Kp, dtype=torch.uint8, device=DEV)
    Bm = torch.zeros(max(N, 16), Kp, dtype=torch.uint8, device=DEV)
    SA = torch.full((M, Kp // 32), 127, dtype=torch.uint8, device=DEV)
    SB = torch.full((max(N, 16), Kp // 32), 127, dtype=torch.uint8, device=DEV)
    C = torch.full((M, 128), -777.0, dtype=torch.bfloat16, device=DEV)
    rc = hip.gemm_mxfp8(A, SA, Bm, SB, C, M, N, K, lda=Kp, ldb=Kp, ldsa=Kp // 32, ldsb=Kp // 32, ldc=128, expect=None)
    torch.cuda.synchronize()
    assert rc == hip.NOT_ELIGIBLE
    assert bool((C == -777.0).all())


def test_gemm_refuses_misaligned_epilogue_operands():
    M, N, K = 16, 32, 128
    A = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
    Bm = torch.zeros(N, K, dtype=torch.uint8, device=DEV)
    SA = torch.full((M, 4), 127, dtype=torch.uint8, device=DEV)
    SB = torch.full((N, 4), 127, dtype=torch.uint8, device=DEV)
    buf = torch.full((M + 1, N), -777.0, dtype=torch.bfloat16, device=DEV)
    res = torch.zeros(M + 1, N, dtype=torch.bfloat16, device=DEV)
    kw = dict(lda=K, ldb=K, ldsa=4, ldsb=4, ldc=N, expect=None)
    assert hip.gemm_mxfp8(A, SA, Bm, SB, buf.data_ptr() + 2, M, N, K, **kw) == -1                       # C off a 16-byte address
    assert hip.gemm_mxfp8(A, SA, Bm, SB, buf, M, N, K, C2=buf.data_ptr() + 6, ldc2=N, **kw) == -1       # C2
    assert hip.gemm_mxfp8(A, SA, Bm, SB, buf, M, N, K, mode=hip.EPI_RESIDUAL, res=res.data_ptr() + 2, ldr=N, **kw) == -1
    assert hip.gemm_mxfp8(A, SA, Bm, SB, buf, M, N, K, mode=hip.EPI_RESIDUAL, res=res, ldr=N - 8, **kw) == -1   # ldr < N
    assert hip.gemm_mxfp8(A, SA, Bm, SB, buf, M, N, K, batch=1, sC=4, **kw) == -1                      # sC % 8
    torch.cuda.synchronize()
    assert bool((buf == -777.0).all())
    assert hip.gemm_mxfp8(A, SA, Bm, SB, buf, M, N, K, **kw) == 0


@pytest.mark.parametrize("M,N,K,batch", [(2 * T + 17, T + 16, 640, 1), (T + 1, T, 256, 3)])
def test_gemm_random_data_within_fp32_bound(M, N, K, batch):
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(batch, M, K, generator=g) * torch.exp2(torch.randint(-6, 6, (batch, M, 1), generator=g).float())).to(torch.bfloat16)
    b = (torch.randn(batch, N, K, generator=g) * 0.05).to(torch.bfloat16)
    qa, sa = mx_ref.mx_quantize(a)
    qb, sb = mx_ref.mx_quantize(b)
    da, db = mx_ref.mx_dequantize(qa, sa), mx_ref.mx_dequantize(qb, sb)
    exact = da @ db.transpose(1, 2)
    mag = da.abs() @ db.abs().transpose(1, 2)
    A, SA = upload(qa, sa, K)
    Bm, SB = upload(qb, sb, K)
    C = Banded(batch, M, N, N + 8, torch.bfloat16, -777.0)
    launch(A, SA, Bm, SB, C, M, N, K, batch)
    torch.cuda.synchronize()
    err = (C.view.cpu().double() - exact).abs()
    bound = (K - 1) * 2.0 ** -23 * mag + 2.0 ** -8 * exact.abs()
    print(f"random data M={M} N={N} K={K}: worst error / bound = {float((err / bound.clamp(min=1e-300)).max()):.4f}")
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    assert C.untouched()


# ------------------------------------------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("M", (1, 130))
@pytest.mark.parametrize("f", (32, 384))
def test_swiglu_fwd_mx_equals_swiglu_then_quantise(M, f):
    g = torch.Generator().manual_seed(M + f)
    h12 = Banded(1, M, 2 * f, 2 * f + 8, torch.bfloat16, 9.0)
    h12.set((torch.randn(1, M, 2 * f, generator=g) * 3).to(torch.bfloat16))
    L, st = hip.lib(), hip.stream_ptr()
    a = torch.empty(M, f, dtype=torch.bfloat16, device=DEV)
    hip.check(L.md_swiglu_fwd(h12.ptr(), h12.ld, a.data_ptr(), f, M, f, st), "md_swiglu_fwd")
    q2 = torch.empty(M, f, dtype=torch.uint8, device=DEV)
    s2 = torch.empty(M, f // 32, dtype=torch.uint8, device=DEV)
    hip.mx_quant_rows(a, q2, s2, M, f, ld=f, ldd=f, lds=f // 32)
    q1 = Banded(1, M, f, f + 16, torch.uint8, 0xAB)
    s1 = Banded(1, M, f // 32, f // 32 + 3, torch.uint8, 0xCD)
    hip.check(L.md_swiglu_fwd_mx(h12.ptr(), h12.ld, q1.ptr(), q1.ld, s1.ptr(), s1.ld, M, f, st), "md_swiglu_fwd_mx")
    torch.cuda.synchronize()
    assert torch.equal(q1.view[0], q2) and torch.equal(s1.view[0], s2)
    assert q1.untouched() and s1.untouched() and h12.untouched()
    qr, sr = mx_ref.mx_quantize(a.cpu())                                # and both agree with the reference rule
    assert torch.equal(q2.cpu(), qr.view(torch.uint8)) and torch.equal(s2.cpu(), sr)
