"""Ground truth and error bound of md_attn_probs, shared by tests/test_attn_probs_kernel_gpu.py and
tests/test_attn_maps_gpu.py.  The reference cannot emit attention probabilities (F.scaled_dot_product_attention never materialises
them), so the truth is an fp64 softmax of the same bf16 operands.

The bound is derived from the kernel's arithmetic, not measured.  Per score the kernel forms, all in fp32,
    acc = sum_i q_i k_ji  (hd exact bf16 x bf16 products, fp32 accumulation),   s = acc * scale,
    p = exp2((s - max) * log2 e),   P = p * rcp(sum_j p),   out += (sum_h P_h) * (1 / H).
 * With u = 2^-24, the accumulation of hd exact products and the scale multiply leave |s - s_exact| <= (hd + 1) u scale sum_i |q_i k_ji|;
   E is the largest such value of a row over its heads and keys.  A score error of at most E moves p by a factor within e^{+-E} and the
   denominator by a factor within e^{+-E}: 2 E relative in P (first order; E <= 4e-4 at the hardest operands used).
 * The subtraction s - max and the multiply by log2 e each round a value whose magnitude, in units of the natural exponent, is <= 17:
   2 * 17 u relative in p; the fp32 constant log2 e is off by <= 2^-25 relative: 8.5 u more; v_exp_f32 adds 1 ulp (2 u): 44.5 u = 2^-18.5
   together.  Arguments below -17 belong to p < 4.2e-8 <= the absolute floor.
 * The denominator adds at most 128 + 2 terms in fp32: <= 2^-17 relative, and inherits the relative error of the p's (<= 2^-18.5).
 * rcp (1 ulp) and the product: 2^-23 + 2^-24.  The head sum of H <= 16 non-negative terms: <= 2^-20; 1 / H and the product with it:
   2^-23.  The add into a zeroed out is exact.
   Sum: 2 * 2^-18.5 + 2^-17 + 2^-20 + 4 * 2^-23 < 1.45e-5 < 2^-16 = 1.53e-5.
 * A row of one head sums to 1 up to the denominator's summation error and the rcp (2^-17 + 2^-23 + 2^-24: the p's of numerator and
   denominator are the same bits), the head mean adds 2^-20: every output row sums to 1 within 2^-16.
 * Probabilities below fp32 resolution of the row (which sums to 1) are covered by the absolute floor 2^-24.
Hence  |got - ref| <= (2 E + 2^-16) * ref + 2^-24  per element and launch.  n launches into one buffer add their values with n - 1 fp32
additions of non-negative terms: the bounds add, plus (n - 1) * 2^-24 * (the sum of the references)."""
import math

import torch

U = 2.0 ** -24


def reference(q: torch.Tensor, k: torch.Tensor, scale: float):
    """q [B, H, Sq, hd], k [B, H, Skv, hd] (bf16 values in any dtype) -> (ref fp64 [B, Sq, Skv], the head mean of the softmax over the
    keys; E fp64 [B, Sq], the row's score-error bound).  scale: the fp32 value the kernel is given."""
    q, k = q.double(), k.double()
    hd = q.shape[-1]
    s = scale * (q @ k.transpose(-1, -2))
    ref = torch.softmax(s, dim=-1).mean(1)
    E = (hd + 1) * U * scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=(1, 3))
    return ref, E


def f32_scale(hd: int) -> float:
    """1 / sqrt(hd) as the fp32 value md_attn_args carries."""
    return float(torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float32))


def assert_within_bound(got: torch.Tensor, ref, E=None, what: str = "") -> None:
    """got fp32 [B, Sq, Skv] against reference(): prints the largest error relative to its bound, then asserts.  ref may be a list of
    (ref, E) pairs: got is then the sum of that many launches into one buffer."""
    parts = [(ref, E)] if E is not None else list(ref)
    assert torch.isfinite(got).all(), f"{what}: non-finite probabilities"
    ref = sum(r for r, _ in parts)
    E = torch.stack([e for _, e in parts]).amax(0)
    err = (got.double() - ref).abs()
    bound = sum((2 * e[..., None] + 2.0 ** -16) * r + U for r, e in parts) + (len(parts) - 1) * U * ref
    worst = float((err / bound).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}, max E {float(E.max()):.3e}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the derived bound"
