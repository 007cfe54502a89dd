"""Reference models for the Muon tests (pure torch on the CPU, no GPU needed), as tests/optim_ref.py is for AdamW: the momentum,
normalise and apply arithmetic of include/microdit_hip.h in fp32 with its exact operation order, the Newton-Schulz iteration in fp64 and
with the kernel's rounding points emulated, and the item set / storage the kernel tests share.

Bit-exactness.  Every fp32 operation the header names is one correctly rounded IEEE operation: products, quotients and square roots of
fp32 tensors on the CPU are; a fused multiply-add is formed here as the exact product (48 bits, held in fp64), an fp64 sum ROUNDED TO
ODD (the TwoSum error term decides the sticky bit) and one rounding to fp32 -- 53 >= 2 * 24 + 2 bits, so the double rounding is
innocuous and fma32 returns the bits of the hardware's v_fma_f32.  Two scalars may be contracted by the compiler or not (decay = 1 - lr *
wd and nrm + 1e-6 in the clip chain): the test hyper-parameters are chosen so that both readings give the same bits (grad_scale a power
of two; decay_is_unambiguous asserted), as in tests/optim_ref.py."""
import math

import numpy as np
import torch

from tests.gemm_exact import SENT_BF16, SENT_F32

BAD_ARG = -1
NS_COEFFS = (3.4445, -4.7750, 2.0315)
NORM_PARTS = 16                       # MD_MUON_NORM_PARTS


def r32(x):
    return float(np.float32(x))


def fma32(a, x, y):
    """fl32(a * x + y) with ONE rounding, elementwise; a may be a Python float holding an fp32 number."""
    a = torch.as_tensor(a, dtype=torch.float32)
    p = a.double() * x.double()                       # exact
    y = y.double()
    s = p + y
    bb = s - p
    err = (p - (s - bb)) + (y - bb)                   # TwoSum: s + err == p + y exactly
    bits = s.clone().view(torch.int64)
    up = (err > 0) == (s > 0)                         # the exact sum lies further from zero than s
    odd = torch.where(up, bits + 1, bits - 1)
    fix = (err != 0) & ((bits & 1) == 0)
    s = torch.where(fix, odd, bits).view(torch.float64)
    return s.float()


def decay_is_unambiguous(lr, wd):
    lr, wd = r32(lr), r32(wd)
    return r32(1.0 - r32(lr * wd)) == r32(1.0 - lr * wd)


def decay_of(lr, wd):
    assert decay_is_unambiguous(lr, wd), (lr, wd)
    return r32(1.0 - r32(r32(lr) * r32(wd)))


def clip_coef(grad_scale, sumsq=None, max_norm=0.0):
    """coef of md_adamw_step / md_muon_momentum; grad_scale must be a power of two (the fused and the unfused nrm + 1e-6 then agree)."""
    gs = r32(grad_scale)
    assert math.frexp(gs)[0] == 0.5, "grad_scale must be a power of two"
    if sumsq is None or not max_norm > 0:
        return gs
    nrm = r32(r32(math.sqrt(r32(sumsq))) * gs)
    return r32(gs * min(1.0, r32(r32(max_norm) / r32(nrm + r32(1e-6)))))


def momentum_ref(g, m, coef, mu, nesterov):
    """(m', u) of md_muon_momentum: gc = coef * g, m' = fma(mu, m, gc), u = nesterov ? fma(mu, m', gc) : m'.  g: fp32 or bf16 values."""
    gc = torch.tensor(coef, dtype=torch.float32) * g.float()
    m_new = fma32(r32(mu), m.float(), gc)
    return m_new, (fma32(r32(mu), m_new, gc) if nesterov else m_new)


def normalise_ref(u):
    """(sum u^2 in fp64, inv, X = bf16(u * inv))."""
    nrm = float((u.double() ** 2).sum())
    inv = r32(1.0 / (math.sqrt(nrm) + 1e-7))
    return nrm, inv, (u * torch.tensor(inv, dtype=torch.float32)).to(torch.bfloat16)


def apply_ref(p, o, lr, wd, scale, ema_mode=0, es=0.0, ema=None):
    """(p', shadow, ema') of md_muon_apply: q = p * decay, p' = fma(-(lr * scale), float(O), q), shadow = bf16(p'),
    ema' = p' (mode 1) or fma(es, ema, (1 - es) * p') (mode 2)."""
    decay = torch.tensor(decay_of(lr, wd), dtype=torch.float32)
    nls = -r32(r32(lr) * r32(scale))
    pn = fma32(nls, o.float(), p * decay)
    e = ema
    if ema_mode == 1:
        e = pn.clone()
    elif ema_mode == 2:
        e = fma32(r32(es), ema, torch.tensor(r32(1.0 - r32(es)), dtype=torch.float32) * pn)
    return pn, pn.to(torch.bfloat16), e


# ------------------------------------------------------------------------------------------------ Newton-Schulz
def ns_fp64(x, steps=5, coeffs=NS_COEFFS):
    """The quintic iteration in fp64 on the values of x (any float dtype), in x's orientation."""
    a, b, c = coeffs
    X = x.double()
    tall = X.shape[0] > X.shape[1]
    if tall:
        X = X.t()
    for _ in range(steps):
        A = X @ X.t()
        X = a * X + (b * A + c * (A @ A)) @ X
    return X.t() if tall else X


def _bf(x):
    return x.to(torch.bfloat16).float()


def ns_bf16_emulated(x, steps=5, coeffs=NS_COEFFS):
    """The same iteration with the kernel's rounding points: fp32 products, rounded to bf16 after A, after B and after the new X."""
    a, b, c = coeffs
    X = _bf(x.float())
    tall = X.shape[0] > X.shape[1]
    for _ in range(steps):
        if tall:
            A = _bf(X.t() @ X)
            B = _bf(b * A + c * (A @ A))
            X = _bf(a * X + X @ B)
        else:
            A = _bf(X @ X.t())
            B = _bf(b * A + c * (A @ A))
            X = _bf(a * X + B @ X)
    return X.to(torch.bfloat16)


def rel_err(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def ulp_bf16(x):
    """Spacing of bf16 at |x| (fp64 tensor); the smallest normal's spacing below it."""
    e = torch.floor(torch.log2(x.double().abs().clamp(min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


# ------------------------------------------------------------------------------------------------ the item set of the kernel tests
# (rows, cols) in table order: square, wide, tall, a wide one of several tiles, and a 3-D tensor [2, 64, 128] as two adjacent items
# (one shape, consecutive: the batched Gram launch).  GAPS: elements between an item and the next (0 = adjacent); multiples of 8.
SHAPES = ((64, 64), (64, 192), (192, 64), (128, 320), (64, 128), (64, 128))
LEAD = 72
GAPS = (8, 64, 24, 136, 0, 40)


def layout():
    """([(flat_off, rows, cols)], total): the items at non-adjacent offsets inside one flat buffer."""
    at, out = LEAD, []
    for (r, c), gap in zip(SHAPES, GAPS):
        out.append((at, r, c))
        at += r * c + gap
    return out, at


def ws_layout(items):
    """([ws_off], bf16 elements, bytes): what md_muon_ws_bytes writes -- per item bf16 [X | A | B], back to back, then the shared fp32
    scratch of the largest matrix."""
    at, offs = 0, []
    for _, r, c in items:
        offs.append(at)
        s = min(r, c)
        at += r * c + 2 * s * s
    return offs, at, 2 * at + 4 * max(r * c for _, r, c in items)


def item_mask(items, total):
    m = torch.zeros(total, dtype=torch.bool)
    for o, r, c in items:
        m[o:o + r * c] = True
    return m


def poisoned(total, dtype, device="cpu"):
    """A buffer of sentinel NaNs (the bit patterns of tests/gemm_exact.py)."""
    if dtype == torch.float32:
        return torch.full((total,), SENT_F32, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full((total,), SENT_BF16, dtype=torch.int16, device=device).view(torch.bfloat16)


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def ns_input(rows, cols, seed):
    """A Newton-Schulz test input in the converged regime (tests/test_muon_cpu.py asserts it): Gaussian scaled to unit Frobenius norm
    for the non-square shapes (what md_muon_momentum hands over); for a square one, whose Gaussian has singular values down to 0.06 of
    the mean, prescribed singular values spread over [0.2, 1] between random orthogonal factors."""
    g = torch.Generator().manual_seed(seed)
    if rows == cols:
        q1, _ = torch.linalg.qr(torch.randn(rows, rows, generator=g, dtype=torch.float64))
        q2, _ = torch.linalg.qr(torch.randn(rows, rows, generator=g, dtype=torch.float64))
        s = torch.linspace(0.2, 1.0, rows, dtype=torch.float64)
        x = (q1 * s) @ q2.t()
    else:
        wide = torch.randn(min(rows, cols), max(rows, cols), generator=g, dtype=torch.float64)
        wide = wide / wide.norm()
        x = wide.t() if rows > cols else wide          # the tall input IS the transpose of the wide one of the same seed
    return x.float().to(torch.bfloat16)


def ns_inputs():
    """One input per item of SHAPES (the tall 192 x 64 is the transpose of the wide 64 x 192), and the larger Gaussian shape."""
    seeds = (11, 12, 12, 13, 14, 15)
    return [ns_input(r, c, s) for (r, c), s in zip(SHAPES, seeds)]
