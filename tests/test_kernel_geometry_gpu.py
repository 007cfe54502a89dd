"""The norm, elementwise, EDM and row gather / scatter kernels at the shapes where their launch heuristics take the production
branch (tests/kernel_geometry.py names the branch of every case), each element against an fp64 reference built from the same bf16 /
fp16 / fp32 inputs.  The MoE routing kernels (mask ranking, softmax / top-k, combine, the backward kernels, compaction) have their own
file with the same helpers: tests/test_moe_geometry_gpu.py.

How outputs are compared (helpers below; U = 2^-24 is the fp32 unit roundoff, ulp(r) the bf16 spacing at |r|):
  * exact      -- the kernel does one correctly rounded fp32 operation (or a copy) and nothing else: the bits must equal torch's
                  fp32 op followed by its round-to-nearest-even bf16 conversion.
  * one ulp    -- a bf16 output of an fp32 computation: |got - ref| <= ulp(ref) + e, e the fp32 evaluation error of that
                  computation, stated next to each use (a few U relative, far below ulp; for the hardware transcendentals an
                  absolute term that only matters in their far tails).
  * sums       -- |got - ref| <= rtol * sum|terms| + atol, sum|terms| in fp64 and rtol = (h + c) U with h the longest chain of
                  fp32 additions the launch geometry gives (serial rows per wave, LDS adds, atomics into one address, ...): the
                  worst-case bound of summation in any order, so the outcome does not depend on atomic arrival order.  Every sum
                  also asserts its own sensitivity: the reference with one term (a row, a sample) left out must fail the bound.
"""
from ctypes import byref

import math
import pytest
import torch

from tests import kernel_geometry as kg

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------- comparison
def ulp(r):
    """bf16 spacing at |r| (fp64): 2^(e - 8) for |r| = m 2^e, m in [0.5, 1); floored at the smallest normal."""
    _, e = torch.frexp(r.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(r), e - 8)


def rne_bf16(x):
    """fp64 -> the nearest bf16 value, ties to even (one rounding: torch's fp64 -> bf16 cast goes through fp32)."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256), e - 8)


def _report(ok, got, ref, bound, what):
    if bool(ok.all()):
        return
    bad = (~ok).nonzero()
    i = tuple(bad[0].tolist())
    ref = torch.broadcast_to(ref, got.shape)
    bound = torch.broadcast_to(bound, got.shape) if torch.is_tensor(bound) else bound
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if torch.is_tensor(bound) else float(err.max() / bound)
    b = bound[i] if torch.is_tensor(bound) else bound
    raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements out of bound; first at {i}: got {float(got[i])!r} "
                         f"ref {float(ref[i])!r} bound {float(b):.3g}; worst err / bound {worst:.3g}")


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound elementwise (got any float dtype, ref / bound fp64); non-finite output fails."""
    g = got.double()
    ok = torch.isfinite(g) & ((g - ref).abs() <= bound)
    _report(ok, got, ref, bound, what)


def assert_exact(got, want, what):
    """Bit equality (bf16 / fp32 / int tensors of the same dtype)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype in (torch.bfloat16, torch.float16):
        a, b = got.view(torch.int16), want.view(torch.int16)
    elif got.dtype == torch.float32:
        a, b = got.view(torch.int32), want.view(torch.int32)
    else:
        a, b = got, want
    ok = a == b
    if not bool(ok.all()):
        i = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements differ; first at {i}: got {got[i].item()!r} "
                             f"want {want[i].item()!r}")


def assert_sum(got, ref, abs_sum, rtol, what, dropped=None, atol=0.0):
    """A reduction: |got - ref| <= rtol * abs_sum + atol.  dropped: the reference with one term left out, which must NOT pass."""
    bound = rtol * abs_sum + atol
    assert_within(got, ref, bound, what)
    if dropped is not None:
        assert bool(((got.double() - dropped).abs() > bound).any()), f"{what}: the bound (rtol {rtol:.3g}) misses one left-out term"


# fp32 evaluation error of the hardware-transcendental activations of md_common.h (v_exp_f32 / v_rcp_f32 forms), absolute,
# as a function of the fp32 input x: an fp32 emulation of the same formulas over every bf16 |x| <= 12 stays below 1/9 of these
# envelopes.  They matter only in the far negative tails, where 1 + tanh and sigmoid are a few ulps of 1 and the result is tiny.
def eps_gelu(x):
    return 2.0 ** -20 * (1 + x.abs()) ** 2


def eps_silu(x, s):          # s = silu(x) in fp64: relative error <= 16 U measured, 64 U allowed
    return 64 * U * s.abs()


def eps_dsilu(x, sg):        # sg = sigmoid(x) in fp64
    return 2.0 ** -18 * sg * (1 + x.abs())


def gelu_tanh64(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def dgelu_tanh64(x):
    t = torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)


def bf(t):
    return t.to(torch.bfloat16)


def sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def _stat_bounds(v, C):
    """fp64 mean / rstd of rows v and the kernel's fp32 error bounds on them.  The kernel sums a lane's 8 * NCH values serially,
    then over the wave in 6 DPP steps: h = 8 NCH + 6 additions on the longest chain (+1 for the 1 / C product, +1 margin)."""
    h = 8 * kg.nch(C) + 6
    mean = v.mean(1)
    var = (v - mean[:, None]).pow(2).mean(1)
    return mean, var, h, (h + 2) * U * v.abs().mean(1)


@pytest.mark.parametrize("case", kg.LN_FWD, ids=[c.id for c in kg.LN_FWD])
def test_ln_fwd(hip, case):
    """md_ln_fwd at the rows-per-wave the engine's microbatches give (4, 5, 8; 5 with waves that straddle two samples) and the
    generic (act / pos) path past 16,384 rows.  mean / rstd against fp64 statistics; the output against fp64 LN evaluated with the
    kernel's own statistics, modulated outputs with the kernel's bf16 rounding of the normalised value reproduced (norm.hip:161)."""
    rows, rps, C = case.rows, case.rps, case.C
    B = rows // rps
    torch.manual_seed(rows + C + case.act)
    L, st = hip.lib(), hip.stream_ptr()
    x = bf(torch.randn(rows, C, device=DEV) * 1.5 + 0.3)
    w = (1 + 0.2 * torch.randn(C, device=DEV)).float()
    mod = bf(torch.randn(B, 6 * C, device=DEV) * 0.4)        # engine layout: shift at 0, scale at C, in a 6 C row
    pos = torch.randn(rps, C, device=DEV) * 0.5 if case.pos else None
    out = torch.full((rows, C), 7.0, device=DEV, dtype=torch.bfloat16)
    mean = torch.full((rows,), float("nan"), device=DEV)
    rstd = torch.full((rows,), float("nan"), device=DEV)
    a = hip.LnArgs(x.data_ptr(), w.data_ptr(), mod.data_ptr() if case.mod else None, mod[:, C:].data_ptr() if case.mod else None,
                   pos.data_ptr() if case.pos else None, out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, C, C, C, 6 * C,
                   rps, rps if case.pos else 0, 1e-6, case.act)
    hip.check(L.md_ln_fwd(byref(a), st), "md_ln_fwd")
    sync()
    w64 = w.double()
    step = 8192
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        xr = x[r0:r1].double()
        # the LN input the kernel forms in fp32: act(fl(x + pos)); dv bounds its fp32 evaluation error
        dv = torch.zeros_like(xr)
        if case.pos:
            xr = xr + pos.double()[torch.arange(r0, r1, device=DEV) % rps]
            dv = U * xr.abs()
        if case.act:
            dv = dv * 1.2 + eps_gelu(xr)               # |gelu'| <= 1.13 carries the rounding of x + pos through
            xr = gelu_tanh64(xr)
        m64, var64, h, dm = _stat_bounds(xr, C)
        dm = dm + dv.mean(1)
        r64 = (var64 + 1e-6).rsqrt()
        mk, rk = mean[r0:r1].double(), rstd[r0:r1].double()
        assert_within(mk, m64, dm, f"{case.id}: mean rows {r0}..{r1}")
        # rstd: the squared deviations summed on the same chain (h), relative; halved by the square root, + rsqrt and 1 / C
        assert_within(rk, r64, ((h + 8) * U + 2 * dv.mean(1) / var64.sqrt()) * r64, f"{case.id}: rstd rows {r0}..{r1}")
        # y = (v - mean) rstd w with the kernel's statistics: 3 fp32 roundings (3 U relative) + the propagated input error
        y64 = (xr - mk[:, None]) * rk[:, None] * w64
        dy = 3 * U * y64.abs() + dv * rk[:, None] * w64.abs()
        got = out[r0:r1]
        if not case.mod:
            assert_within(got, y64, ulp(y64) + dy, f"{case.id}: out rows {r0}..{r1}")
            continue
        smp = torch.arange(r0, r1, device=DEV) // rps
        sh = mod[smp, :C].double()
        sc1 = 1 + mod[smp, C:2 * C].double()
        # the kernel rounds y to bf16 before modulating; y in fp32 is within dy of y64, so its bf16 is one of the roundings of
        # y64 -/+ dy (the same value except next to a rounding midpoint).  z = yb (1 + scale) + shift: 3 fp32 roundings.
        ok = None
        for yb in (rne_bf16(y64 - dy), rne_bf16(y64 + dy)):
            z = yb * sc1 + sh
            bound = ulp(z) + 4 * U * ((yb * sc1).abs() + sh.abs())
            hit = (got.double() - z).abs() <= bound
            ok = hit if ok is None else ok | hit
        z = rne_bf16(y64) * sc1 + sh
        _report(ok & torch.isfinite(got.double()), got, z, ulp(z), f"{case.id}: modulated out rows {r0}..{r1}")


def _row_stats32(x, eps=1e-6, step=8192):
    """fp32 roundings of the fp64 per-row mean and rstd of x (the statistics md_ln_bwd is handed), in row chunks."""
    m, r = torch.empty(x.shape[0], device=DEV), torch.empty(x.shape[0], device=DEV)
    for r0 in range(0, x.shape[0], step):
        v = x[r0:r0 + step].double()
        mu = v.mean(1, keepdim=True)
        m[r0:r0 + step] = mu[:, 0].float()
        r[r0:r0 + step] = ((v - mu).pow(2).mean(1) + eps).rsqrt().float()
    return m, r


@pytest.mark.parametrize("case", kg.LN_BWD, ids=[c.id for c in kg.LN_BWD])
def test_ln_bwd(hip, case):
    """md_ln_bwd (+ ln_bwd_finish_kernel) at DiTEngine's own rows_per_block, with enough samples for several (and a partial)
    finish chunk, in the engine's three forms.  dx elementwise; dS / dscale, dshift and dw as sums with their sensitivity."""
    from micro_diffusion_amd.engine import DiTEngine
    rows, C = case.rows, case.C
    rps = case.rps if case.rps > 0 else rows
    B = rows // rps
    rpb = DiTEngine._rows_per_block(rows, rps, 1024)
    torch.manual_seed(rows + C)
    L, st = hip.lib(), hip.stream_ptr()
    x = bf(torch.randn(rows, C, device=DEV) * 1.5 + 0.3)
    w = (1 + 0.2 * torch.randn(C, device=DEV)).float()
    mod = bf(torch.randn(B, 6 * C, device=DEV) * 0.4)
    m32, r32 = _row_stats32(x)
    dz = bf(torch.randn(rows, C, device=DEV))
    dx0 = bf(torch.randn(rows, C, device=DEV)) if case.accumulate else torch.full((rows, C), 7.0, device=DEV, dtype=torch.bfloat16)
    dx = dx0.clone()
    dw0 = torch.randn(C, device=DEV)
    dw = dw0.clone()
    modded = case.form == "mod"
    a = hip.LnArgs(x.data_ptr(), w.data_ptr(), mod.data_ptr() if modded else None, mod[:, C:].data_ptr() if modded else None, None,
                   None, m32.data_ptr(), r32.data_ptr(), rows, C, C, C, 6 * C, case.rps, 0, 1e-6, 0)
    if modded:
        dmod = torch.zeros(B, 6 * C, device=DEV)
        dS = dmod[:, C:2 * C]
        b = hip.LnBwdArgs(dz.data_ptr(), dx.data_ptr(), dmod[:, C:].data_ptr(), dmod.data_ptr(), dw.data_ptr(), C, C, 6 * C, rpb,
                          case.accumulate, 1)
    else:
        scratch = torch.zeros(B, C, device=DEV)
        dS = scratch
        b = hip.LnBwdArgs(dz.data_ptr(), dx.data_ptr(), scratch.data_ptr(), None, dw.data_ptr(), C, C, C, rpb, case.accumulate, 0)
    hip.check(L.md_ln_bwd(byref(a), byref(b), st), "md_ln_bwd")
    sync()
    w64, h = w.double(), 8 * kg.nch(C) + 6
    S = torch.zeros(B, C, device=DEV, dtype=F64)         # sum_t dz xhat per sample
    Sa = torch.zeros_like(S)                             # sum_t |dz xhat|
    D = torch.zeros_like(S)                              # sum_t dz
    Da = torch.zeros_like(S)
    one_row = None                                       # dz xhat of sample 0's row 5 (the sensitivity probe)
    step = max(1, 8192 // rps) * rps if rps <= 8192 else 8192
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        smp = torch.arange(r0, r1, device=DEV) // rps
        xh = (x[r0:r1].double() - m32[r0:r1].double()[:, None]) * r32[r0:r1].double()[:, None]
        g = dz[r0:r1].double()
        wm = w64 * (1 + mod[smp, C:2 * C].double()) if modded else w64.expand(r1 - r0, C)
        gg = g * wm
        s1, s2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
        a1, a2 = gg.abs().mean(1, keepdim=True), (gg * xh).abs().mean(1, keepdim=True)
        r = r32[r0:r1].double()[:, None]
        ref = r * (gg - s1 - xh * s2)
        # fp32 error of rstd (dz wm - s1 - xhat s2): xhat 2 U, wm 2 U, the products and two subtractions ~6 U of the terms,
        # s1 / s2 summed on the h-chain of the wave reduction; then the accumulate add (U of the result)
        err = r * (6 * U * (gg.abs() + s1.abs() + (xh * s2).abs()) + (h + 5) * U * a1 + xh.abs() * (h + 8) * U * a2)
        if case.accumulate:
            ref = ref + dx0[r0:r1].double()
        err = err + 2 * U * ref.abs()
        assert_within(dx[r0:r1], ref, ulp(ref) + err, f"{case.id}: dx rows {r0}..{r1}")
        t = g * xh
        S.index_add_(0, smp, t)
        Sa.index_add_(0, smp, t.abs())
        D.index_add_(0, smp, g)
        Da.index_add_(0, smp, g.abs())
        if one_row is None:
            one_row = (t[5].clone(), g[5].clone())
    # dS: per lane serial over a wave's rows, 3 LDS adds, one atomic per workgroup of the sample; products 3 U
    per_wave = -(-min(rpb, rps) // 4)
    blocks = -(-rps // rpb)
    rtol_s = (per_wave + 3 + blocks + 5) * U
    drop = torch.zeros_like(S)
    drop[0] = one_row[0]
    if modded:
        assert_sum(dS, S * w64, Sa * w64.abs(), rtol_s + U, f"{case.id}: dscale = w dS", dropped=(S - drop) * w64)
        drop[0] = one_row[1]
        assert_sum(dmod[:, :C], D, Da, rtol_s, f"{case.id}: dshift", dropped=D - drop)
        assert float(dmod[:, 2 * C:].abs().max()) == 0.0, "columns past dscale must not be written"
    else:
        assert_sum(dS, S, Sa, rtol_s, f"{case.id}: per-sample dS (scratch)", dropped=S - drop)
    # dw = dw0 + sum_b (1 + scale_b) dS_b: dS's error, then (1 + s) dS (2 U), 16 serial adds per finish chunk, one atomic per chunk
    chunks, _ = kg.finish_chunks(B, {"finish_chunk": 16})
    m = (1 + mod[:, C:2 * C].double()) if modded else torch.ones_like(S)
    ref_w = dw0.double() + (m * S).sum(0)
    abs_w = dw0.double().abs() + (m.abs() * Sa).sum(0)
    rtol_w = rtol_s + (16 + chunks + 4) * U
    # sensitivity: the last sample left out (one row of the only sample when rows_per_sample = 0)
    assert_sum(dw, ref_w, abs_w, rtol_w, f"{case.id}: dw", dropped=ref_w - (m[B - 1] * S[B - 1] if B > 1 else one_row[0]))


@pytest.mark.parametrize("case", kg.QKLN, ids=[c.id for c in kg.QKLN])
def test_qkln_grid_stride(hip, case):
    """md_qkln_fwd / md_qkln_bwd (q and k in one launch) past ln_grid's 16,384 waves: every wave takes several grid-stride passes
    and the last pass is partial.  Forward against fp64 LN, backward against fp64 of its formula on the kernel's stored y and rstd;
    the head-major forms must give the same bits."""
    rows, width, hd, S = case.rows, case.width, case.hd, case.S
    B, H, ld = rows // S, width // hd, 3 * width
    torch.manual_seed(rows + width)
    L, st = hip.lib(), hip.stream_ptr()
    buf = bf(torch.randn(rows, ld, device=DEV) * 2 + 0.5)
    work, rstd = buf.clone(), torch.full((2, rows), float("nan"), device=DEV)
    hip.check(L.md_qkln_fwd(work.data_ptr(), rows, ld, 0, width, 2, width, rstd.data_ptr(), 1e-6, st), "md_qkln_fwd")
    out = torch.zeros(2, B, H, S, hd, device=DEV, dtype=torch.bfloat16)
    rstd_hm = torch.empty(2, rows, device=DEV)
    hip.check(L.md_qkln_fwd_hm(buf.data_ptr(), rows, ld, 0, width, 2, width, out.data_ptr(), rows * width, S, hd, rstd_hm.data_ptr(),
                               1e-6, st), "md_qkln_fwd_hm")
    d = bf(torch.randn(rows, ld, device=DEV))
    dwork = d.clone()
    hip.check(L.md_qkln_bwd(dwork.data_ptr(), ld, 0, work.data_ptr(), ld, 0, rows, width, 2, width, width, rstd.data_ptr(), st),
              "md_qkln_bwd")

    def to_hm(t):
        return t.reshape(B, S, H, hd).permute(0, 2, 1, 3).contiguous()

    dy = torch.stack([to_hm(d[:, :width]), to_hm(d[:, width:2 * width])])
    dhm = torch.full_like(d, 7.0)
    hip.check(L.md_qkln_bwd_hm(dy.data_ptr(), rows * width, out.data_ptr(), rows * width, dhm.data_ptr(), ld, 0, width, rows, width, 2,
                               S, hd, rstd.data_ptr(), st), "md_qkln_bwd_hm")
    sync()
    assert_exact(work[:, 2 * width:], buf[:, 2 * width:], "v columns untouched")
    assert_exact(rstd_hm, rstd, "head-major rstd")
    for seg in range(2):
        cols = slice(seg * width, (seg + 1) * width)
        assert_exact(out[seg], to_hm(work[:, cols]), f"head-major y, segment {seg}")
        assert_exact(dhm[:, cols], dwork[:, cols], f"head-major dx, segment {seg}")
        v = buf[:, cols].double()
        m64, var64, h, dm = _stat_bounds(v, width)
        r64 = (var64 + 1e-6).rsqrt()
        rk = rstd[seg].double()
        rrel = (h + 8) * U
        assert_within(rk, r64, rrel * r64, f"rstd segment {seg}")
        y64 = (v - m64[:, None]) * r64[:, None]
        # the kernel's own mean (not stored) is within dm of m64, its rstd within rrel; + 2 fp32 roundings
        assert_within(work[:, cols], y64, ulp(y64) + r64[:, None] * dm[:, None] + (rrel + 3 * U) * y64.abs(), f"y segment {seg}")
        del v, y64
        # backward: dx = rstd (g - mean(g) - y mean(g y)) on the stored bf16 y and fp32 rstd
        g, y = d[:, cols].double(), work[:, cols].double()
        s1, s2 = g.mean(1, keepdim=True), (g * y).mean(1, keepdim=True)
        a1, a2 = g.abs().mean(1, keepdim=True), (g * y).abs().mean(1, keepdim=True)
        ref = rk[:, None] * (g - s1 - y * s2)
        err = rk[:, None] * (4 * U * (g.abs() + s1.abs() + (y * s2).abs()) + (h + 2) * U * a1 + y.abs() * (h + 3) * U * a2) + U * ref.abs()
        assert_within(dwork[:, cols], ref, ulp(ref) + err, f"dx segment {seg}")
        del g, y, ref, err


# ---------------------------------------------------------------------------------------------------------------- elementwise
@pytest.mark.parametrize("case", kg.EW, ids=[c.id for c in kg.EW])
def test_elementwise_exact(hip, case):
    """The single-rounding ew_grid kernels bit-exact at n = 8 and past the first grid-stride pass (ragged second pass):
    md_cast_f32_bf16 with and without the device scale, md_cast_f32_bf16_clear (source cleared), md_add_bf16, md_fill_zero
    (a byte count that is not a multiple of 16; the bytes past it untouched)."""
    n = case.n
    torch.manual_seed(n)
    L, st = hip.lib(), hip.stream_ptr()
    x = torch.randn(n, device=DEV) * 3
    x[::97] *= 1e-30                                     # tiny (still normal) values round too
    sc = torch.tensor([0.3712], device=DEV)
    for sptr, want in ((None, x.bfloat16()), (sc.data_ptr(), (x * sc).bfloat16())):
        y = torch.full((n,), 7.0, device=DEV, dtype=torch.bfloat16)
        hip.check(L.md_cast_f32_bf16(x.data_ptr(), y.data_ptr(), n, sptr, st), "md_cast_f32_bf16")
        sync()
        assert_exact(y, want, f"cast_f32_bf16 scale={'ptr' if sptr else 'none'}")
    xc = x.clone()
    y = torch.full((n,), 7.0, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_cast_f32_bf16_clear(xc.data_ptr(), y.data_ptr(), n, st), "md_cast_f32_bf16_clear")
    a, b = bf(torch.randn(n, device=DEV)), bf(torch.randn(n, device=DEV) * 0.01)
    s = torch.full((n,), 7.0, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_add_bf16(a.data_ptr(), b.data_ptr(), s.data_ptr(), n, st), "md_add_bf16")
    sync()
    assert_exact(y, x.bfloat16(), "cast_f32_bf16_clear")
    assert float(xc.abs().max()) == 0.0, "cast_f32_bf16_clear must clear its source"
    assert_exact(s, (a.float() + b.float()).bfloat16(), "add_bf16")
    nbytes = 4 * n - 4                                   # not a multiple of 16
    z = torch.full((4 * n + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    hip.check(L.md_fill_zero(z.data_ptr(), nbytes, st), "md_fill_zero")
    sync()
    assert int(z[:nbytes].max()) == 0, "fill_zero left bytes"
    assert bool((z[nbytes:] == 0xA5).all()), "fill_zero wrote past its byte count"


@pytest.mark.parametrize("act", [1, 3], ids=["gelu-tanh", "silu"])
@pytest.mark.parametrize("case", kg.EW, ids=[c.id for c in kg.EW])
def test_act_fwd_bwd(hip, case, act):
    """md_act_fwd / md_act_bwd: one bf16 ulp of the fp64 activation + the hardware-transcendental envelope (eps_*)."""
    n = case.n
    torch.manual_seed(n + act)
    L, st = hip.lib(), hip.stream_ptr()
    x = bf(torch.randn(n, device=DEV) * 2)
    dyv = torch.randn(n, device=DEV)
    y = torch.full((n,), 7.0, device=DEV, dtype=torch.bfloat16)
    dx = torch.full((n,), 7.0, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_act_fwd(x.data_ptr(), y.data_ptr(), n, act, st), "md_act_fwd")
    hip.check(L.md_act_bwd(dyv.data_ptr(), x.data_ptr(), dx.data_ptr(), n, act, st), "md_act_bwd")
    sync()
    xd, g = x.double(), dyv.double()
    if act == 1:
        ref, e = gelu_tanh64(xd), eps_gelu(xd)
        dref, de = g * dgelu_tanh64(xd), g.abs() * eps_gelu(xd)
    else:
        sg = torch.sigmoid(xd)
        ref = xd * sg
        e = eps_silu(xd, ref)
        dref, de = g * sg * (1 + xd * (1 - sg)), g.abs() * eps_dsilu(xd, sg)
    assert_within(y, ref, ulp(ref) + e, "act fwd")
    assert_within(dx, dref, ulp(dref) + de + U * dref.abs(), "act bwd")


def test_cast_rows_mean_tokens(hip):
    """md_cast_rows_bf16 bit-exact for fp32 and fp16 input, with and without the per-sample row scale; md_mean_tokens /
    md_mean_tokens_bwd past the first grid-stride pass."""
    rows, C = kg.CAST_ROWS
    Lc = 77
    torch.manual_seed(rows)
    L, st = hip.lib(), hip.stream_ptr()
    x32 = torch.randn(rows, C, device=DEV) * 2
    x16 = x32.half()
    scale = torch.rand(rows // Lc, device=DEV) + 0.25
    scale[::3] = 0.0                                     # dropped captions
    rs = scale.repeat_interleave(Lc)[:, None]
    for name, x, dt, sptr, want in (("f32 scaled", x32, 1, scale.data_ptr(), (x32 * rs).bfloat16()),
                                    ("f32 no scale", x32, 1, None, x32.bfloat16()),
                                    ("f16 no scale", x16, 0, None, x16.float().bfloat16()),
                                    ("f16 scaled", x16, 0, scale.data_ptr(), (x16.float() * rs).bfloat16())):
        y = torch.full((rows, C), 7.0, device=DEV, dtype=torch.bfloat16)
        hip.check(L.md_cast_rows_bf16(x.data_ptr(), dt, y.data_ptr(), rows, C, sptr, Lc, st), "md_cast_rows_bf16")
        sync()
        assert_exact(y, want, f"cast_rows {name}")
    B, Lt, Cm = kg.MEAN_TOKENS
    yt = bf(torch.randn(B, Lt, Cm, device=DEV))
    pooled = torch.full((B, Cm), 7.0, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_mean_tokens(yt.data_ptr(), pooled.data_ptr(), B, Lt, Cm, st), "md_mean_tokens")
    dy = torch.randn(B * Lt, Cm, device=DEV)
    dy0 = dy.clone()
    hip.check(L.md_mean_tokens_bwd(pooled.data_ptr(), dy.data_ptr(), B, Lt, Cm, st), "md_mean_tokens_bwd")
    sync()
    ref = yt.double().mean(1)
    # L serial fp32 adds and the 1 / L division, then one bf16 rounding
    absum = yt.double().abs().mean(1)
    assert_sum(pooled, ref, absum, (Lt + 2) * U, "mean_tokens", dropped=ref - yt[:, 0].double() / Lt, atol=ulp(ref))
    want = dy0.double().view(B, Lt, Cm) + pooled.double()[:, None] / Lt
    assert_within(dy.view(B, Lt, Cm), want, 2 * U * want.abs() + U * pooled.double().abs()[:, None], "mean_tokens_bwd")


def test_gather_scatter_rows(hip):
    """md_gather_rows / md_scatter_rows (rgrid) bit-exact past the first grid-stride pass, on padded leading dimensions."""
    n, C = kg.GATHER
    src_rows = n + 3001
    torch.manual_seed(n)
    L, st = hip.lib(), hip.stream_ptr()
    src = bf(torch.randn(src_rows, C + 8, device=DEV))
    idx = torch.randperm(src_rows, device=DEV)[:n].int()
    g = torch.full((n, C + 16), 7.0, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_gather_rows(src.data_ptr(), C + 8, idx.data_ptr(), g.data_ptr(), C + 16, n, C, st), "md_gather_rows")
    back = torch.zeros(src_rows, C + 8, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_scatter_rows(g.data_ptr(), C + 16, idx.data_ptr(), back.data_ptr(), C + 8, n, C, st), "md_scatter_rows")
    sync()
    assert_exact(g[:, :C], src[idx.long(), :C], "gather")
    assert bool((g[:, C:] == 7.0).all()), "gather wrote into the padding"
    want = torch.zeros_like(back)
    want[idx.long(), :C] = src[idx.long(), :C]
    assert_exact(back, want, "scatter")


@pytest.mark.parametrize("case", kg.GATE_BWD, ids=[c.id for c in kg.GATE_BWD])
def test_gate_bwd(hip, case):
    """md_gate_bwd for each NCH instance with 64 rows per workgroup: dbr bit-exact, dgate as a per-sample sum."""
    B, rps, C, rpb = case.B, case.rps, case.C, case.rpb
    rows = B * rps
    torch.manual_seed(rows + C)
    L, st = hip.lib(), hip.stream_ptr()
    dx, br = bf(torch.randn(rows, C, device=DEV)), bf(torch.randn(rows, C, device=DEV))
    mod = bf(torch.randn(B, 6 * C, device=DEV))
    dbr = torch.full((rows, C), 7.0, device=DEV, dtype=torch.bfloat16)
    dmod = torch.zeros(B, 6 * C, device=DEV)
    hip.check(L.md_gate_bwd(dx.data_ptr(), br.data_ptr(), mod[:, 2 * C:].data_ptr(), 6 * C, dbr.data_ptr(), dmod[:, 2 * C:].data_ptr(),
                            6 * C, rows, C, rps, rpb, st), "md_gate_bwd")
    sync()
    gate = mod[:, 2 * C:3 * C].repeat_interleave(rps, 0)
    assert_exact(dbr, (dx.float() * gate.float()).bfloat16(), "dbr")
    t = (dx.double() * br.double()).view(B, rps, C)     # bf16 x bf16 products are exact in fp32
    ref = t.sum(1)
    # per lane serial over rpb / 4 rows, 3 LDS adds, one atomic per workgroup of the sample
    rtol = (rpb // 4 + 3 + -(-rps // rpb) + 1) * U
    assert_sum(dmod[:, 2 * C:3 * C], ref, t.abs().sum(1), rtol, "dgate", dropped=ref - t[:, rps - 1])
    assert float(dmod[:, :2 * C].abs().max()) == 0.0 and float(dmod[:, 3 * C:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- EDM
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_edm_res512(hip, masked):
    """The EDM front and back end at res-512 latents (64 x 64, T = 1024) for B = 130 samples: 130 * 16,384 > 2^21 items, so
    prepare / patchify / unpatchify take a second grid-stride pass (the per-sample sigma of samples 128, 129 is written there),
    and the batch-mean loss sums three lane-strided steps.  masked: fp16 latents (the training step's prepare), 75 % masking."""
    B, C, HW, p = kg.EDM_B, kg.EDM_C, kg.EDM_HW, kg.EDM_P
    H = W = HW
    T, pv, per = (H // p) * (W // p), C * p * p, C * H * W
    sd, pm, ps = 0.5, -0.6, 1.2
    torch.manual_seed(B + masked)
    L, st = hip.lib(), hip.stream_ptr()
    x0 = torch.randn(B, C, H, W, device=DEV) * 0.8
    eps = torch.randn(B, C, H, W, device=DEV)
    rnd = torch.randn(B, device=DEV)
    xn = torch.full_like(x0, float("nan"))
    sigma, cin, cnoise = (torch.full((B,), float("nan"), device=DEV) for _ in range(3))
    if masked:
        x0h = x0.half()
        x0f = torch.full_like(x0, float("nan"))
        hip.check(L.md_edm_prepare_f16(x0h.data_ptr(), eps.data_ptr(), rnd.data_ptr(), xn.data_ptr(), x0f.data_ptr(), sigma.data_ptr(),
                                       cin.data_ptr(), cnoise.data_ptr(), B, per, pm, ps, sd, st), "md_edm_prepare_f16")
        x0 = x0h.float()
    else:
        hip.check(L.md_edm_prepare(x0.data_ptr(), eps.data_ptr(), rnd.data_ptr(), xn.data_ptr(), sigma.data_ptr(), cin.data_ptr(),
                                   cnoise.data_ptr(), B, per, pm, ps, sd, st), "md_edm_prepare")
    patches = torch.full((B * T, pv), 7.0, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_patchify(xn.data_ptr(), cin.data_ptr(), patches.data_ptr(), B, C, H, W, p, st), "md_patchify")
    temb = torch.full((B, 256), 7.0, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_timestep_embed(cnoise.data_ptr(), temb.data_ptr(), B, 256, st), "md_timestep_embed")
    sync()
    if masked:
        assert_exact(x0f, x0, "fp32 copy of the fp16 latents")
    arg = rnd.double() * ps + pm
    s64 = arg.exp()
    srel = 8 * U * (1 + arg.abs())                       # fl(rnd p_std + p_mean) carries U |arg|; expf ~2 ulp
    assert_within(sigma, s64, srel * s64, "sigma")
    assert_within(cin, (sd * sd + s64 ** 2).rsqrt(), (srel + 6 * U) * (sd * sd + s64 ** 2).rsqrt(), "c_in")
    assert_within(cnoise, s64.log() / 4, (srel + 4 * U * (1 + arg.abs())) / 4, "c_noise")
    sk = sigma.double().view(B, 1, 1, 1)                 # the sigma the kernel used (checked above)
    xn64 = x0.double() + eps.double() * sk
    assert_within(xn, xn64, 2 * U * (xn64.abs() + (eps.double() * sk).abs()), "x_noisy")
    ref_p = torch.nn.functional.unfold(xn * cin.view(-1, 1, 1, 1), p, stride=p).transpose(1, 2).reshape(B * T, pv)
    assert_exact(patches, ref_p.bfloat16(), "patchify")
    # timestep embedding: f = exp(-ln(1e4) k / half) and a = t f in fp32 (relative (|ln f| + 4) U), then cos / sin (~2 U)
    half = 128
    k = torch.arange(half, device=DEV, dtype=F64)
    lnf = -math.log(10000) * k / half
    a64 = cnoise.double()[:, None] * lnf.exp()[None]
    da = a64.abs() * (lnf.abs() + 4) * U
    for part, ref in ((temb[:, :half], a64.cos()), (temb[:, half:], a64.sin())):
        assert_within(part, ref, ulp(ref) + da + 2 * U, "timestep embedding")
    # ---- unpatchify + loss
    Tk = T // 4 if masked else T
    keep = restore = None
    if masked:
        noise = torch.rand(B, T, device=DEV)
        keep = torch.empty(B * Tk, dtype=torch.int32, device=DEV)
        restore = torch.empty(B, T, dtype=torch.int32, device=DEV)
        mask = torch.empty(B, T, device=DEV)
        hip.check(L.md_get_mask(noise.data_ptr(), B, T, Tk, keep.data_ptr(), restore.data_ptr(), mask.data_ptr(), st), "md_get_mask")
    tok = bf(torch.randn(B * Tk, pv, device=DEV))
    mtok = torch.randn(pv, device=DEV)
    img = torch.full((B, C, H, W), float("nan"), device=DEV)
    hip.check(L.md_unpatchify(tok.data_ptr(), restore.data_ptr() if masked else None, Tk, mtok.data_ptr() if masked else None,
                              img.data_ptr(), B, C, H, W, p, st), "md_unpatchify")
    lps, lmean = torch.full((B,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    dtok = torch.full((B * Tk, pv), float("nan"), device=DEV)
    hip.check(L.md_edm_loss(tok.data_ptr(), keep.data_ptr() if masked else None, xn.data_ptr(), x0.data_ptr(), sigma.data_ptr(),
                            lps.data_ptr(), lmean.data_ptr(), dtok.data_ptr(), B, Tk, C, H, W, p, sd, st), "md_edm_loss")
    gw = 0.375
    lps2, lmean2, acc = torch.empty(B, device=DEV), torch.empty(1, device=DEV), torch.full((1,), 2.0, device=DEV)
    dtb = torch.full((B * Tk, pv), 7.0, device=DEV, dtype=torch.bfloat16)
    hip.check(L.md_edm_loss_train(tok.data_ptr(), keep.data_ptr() if masked else None, xn.data_ptr(), x0.data_ptr(), sigma.data_ptr(),
                                  lps2.data_ptr(), lmean2.data_ptr(), dtb.data_ptr(), gw, acc.data_ptr(), gw, B, Tk, C, H, W, p, sd, st),
              "md_edm_loss_train")
    sync()
    # token j of sample b in (ph, pw, c) order -> its grid position: kept-token order (masked) or identity
    tv = tok.view(B, Tk, p, p, C)
    if masked:
        r = restore.long()
        kept = tv.float()[torch.arange(B, device=DEV)[:, None], r.clamp_max(Tk - 1)]
        full = torch.where((r < Tk).view(B, T, 1, 1, 1), kept, mtok.view(1, 1, p, p, C))
    else:
        full = tv.float()
    g = H // p
    Fimg = full.view(B, g, g, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)
    assert_exact(img, Fimg.contiguous(), "unpatchify")
    # loss terms of the kept patches in the kernel's per-sample order: tokens [b, j] at grid rows pos[b, j]
    pos = (keep.view(B, Tk).long() - torch.arange(B, device=DEV)[:, None] * T) if masked else torch.arange(T, device=DEV).expand(B, T)
    ti, tj = pos // g, pos % g

    def gather(im):                                       # [B, C, H, W] -> [B, Tk, p, p, C] at the kept positions
        v = im.double().view(B, C, g, p, g, p).permute(0, 2, 4, 3, 5, 1)   # [B, gi, gj, ph, pw, C]
        return v[torch.arange(B, device=DEV)[:, None], ti, tj]

    xk, x0k = gather(xn), gather(x0)
    Fk = tv.double()
    s = sigma.double().view(B, 1, 1, 1, 1)
    wgt = (s * s + sd * sd) / (s * sd) ** 2
    cskip, cout = sd * sd / (s * s + sd * sd), s * sd / (s * s + sd * sd).sqrt()
    diff = cskip * xk + cout * Fk - x0k
    terms = (wgt * diff * diff).reshape(B, -1)
    # fp32 evaluation: c_skip / c_out / weight ~4 U; D - x0 within 4 U of (|c_skip xn| + |c_out F| + |x0|)
    ddiff = (4 * U * ((cskip * xk).abs() + (cout * Fk).abs() + x0k.abs())).reshape(B, -1)
    tdev = (wgt.reshape(B, 1) * 2 * diff.reshape(B, -1).abs() * ddiff)
    norm = 1.0 / (pv * Tk)
    ref_l = terms.sum(1) * norm
    # per thread serial over Tk pv / 256 terms, 6 DPP steps, 4 wave partials, the norm product; terms 6 U
    h = Tk * pv // 256 + 6 + 3 + 1
    drop_tok = terms[:, :pv].sum(1) * norm                # one token (its pv terms) of every sample left out
    assert_sum(lps, ref_l, terms.sum(1) * norm, (h + 6) * U, "loss per sample", dropped=ref_l - drop_tok, atol=tdev.sum(1) * norm)
    # batch mean of the kernel's own per-sample losses: lane-strided steps, 6 DPP steps, the 1 / B division
    steps = kg.loss_finish_strides(B, {"loss_finish_stride": 64})
    lk = lps.double()
    assert_sum(lmean, lk.mean().view(1), lk.abs().mean().view(1), (steps + 8) * U, "batch mean",
               dropped=(lk.sum() - lk[B - 1]).view(1) / B)
    # dL/dF = gscale 2 w c_out norm / B * diff (fp32: ~8 U on the factor), kept-token layout [B * Tk, pv]
    fac = (2 * wgt * cout * norm / B).reshape(B, 1)
    dref = fac * diff.reshape(B, -1)
    derr = fac.abs() * ddiff + 8 * U * dref.abs()
    assert_within(dtok.view(B, -1), dref, derr, "dtok")
    assert_within(dtb.view(B, -1), gw * dref, ulp(gw * dref) + gw * derr, "dtok bf16 (training step)")
    assert_exact(lps2, lps, "loss per sample (training step)")
    assert_exact(lmean2, lmean, "batch mean (training step)")
    want = 2.0 + gw * lmean.double()
    assert_within(acc, want, 2 * U * want.abs(), "accumulated loss")
