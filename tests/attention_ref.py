"""Yardsticks for the attention kernel tests (tests/test_attention_ref_cpu.py, tests/test_attention_edges_gpu.py): torch only, any device.

reference   softmax(scale Q K^T) V and its backward in fp64 from the bf16 inputs -- what the kernels approximate.
emulation   the same operation with the kernels' ROUNDING POINTS and nothing else of them (no tiles, no online rescale, no log2
            domain): every product is formed in fp64 and rounded where the kernels round.  Its distance from `reference` is what the
            number formats cost on a given case; a kernel is judged by a multiple of that distance, not by a constant, because the
            hard input families below are ill-conditioned on purpose.
row_err     the worst row, so that one wrong row or tile among a thousand is not averaged away.
make_inputs the input families.

All tensors are [B, H, S, hd]."""
import math
from collections import namedtuple

import torch

Ref = namedtuple("Ref", "o lse dq dk dv logits delta p")
Emu = namedtuple("Emu", "o lse dq dk dv delta")

FAMILIES = ("randn", "peaked", "offset", "late_max", "first_max", "const_keys")


def _rb(x, dtype):
    """Round to `dtype` and come back to fp64."""
    return x.to(dtype).double()


def reference(q, k, v, do, scale):
    """fp64 from the bf16 inputs: o, lse, dq, dk, dv, the logits (scale * q k^T), delta = rowsum(dO * o) and P."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = q @ k.transpose(-1, -2) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    dv = p.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1)
    ds = p * (dp - delta[..., None]) * scale
    return Ref(o, lse, ds @ k, ds.transpose(-1, -2) @ q, dv, s, delta, p)


def emulation(q, k, v, do, scale, o=None, lse=None):
    """The kernels' rounding points: fp32 logits; the unnormalised p = exp(s - rowmax) rounded to bf16 before P.V, its row sum l
    taken from the unrounded p; o rounded to bf16; lse = rowmax + log l in fp32; delta from the bf16 o; P = exp(s - lse) and
    dS / scale = P (dP - delta) rounded to bf16 before the three gradient products; gradients rounded to bf16.
    o / lse given (bf16 / fp32): the backward alone, from that forward state."""
    bf, f32 = torch.bfloat16, torch.float32
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = _rb(q @ k.transpose(-1, -2) * scale, f32)
    if o is None:
        m = s.max(-1, keepdim=True).values
        pu = _rb(torch.exp(s - m), f32)
        l = _rb(pu.sum(-1, keepdim=True), f32)
        o = _rb((_rb(pu, bf) @ v) / l, bf)
        lse = _rb(m + torch.log(l), f32)[..., 0]
    else:
        o, lse = o.double(), lse.double()
    p = _rb(torch.exp(s - lse[..., None]), f32)
    dp = _rb(do @ v.transpose(-1, -2), f32)
    delta = _rb((do * o).sum(-1), f32)
    dsn = _rb(p * (dp - delta[..., None]), bf)
    dq = _rb((dsn @ k) * scale, bf)
    dk = _rb((dsn.transpose(-1, -2) @ q) * scale, bf)
    dv = _rb(_rb(p, bf).transpose(-1, -2) @ do, bf)
    return Emu(o, lse, dq, dk, dv, delta)


def row_err(got, ref):
    """(worst row of |got_r - ref_r|_2 / max(|ref_r|_2, typ), max |got - ref|), typ = sqrt(mean_r |ref_r|^2): rows are the last
    axis.  The floor keeps a row whose reference happens to be tiny from setting the scale; the absolute error is for tensors whose
    reference is zero."""
    got, ref = got.double(), ref.double()
    rn = ref.pow(2).sum(-1).sqrt()
    typ = ref.pow(2).sum(-1).mean().sqrt()
    den = torch.clamp(rn, min=max(typ.item(), 1e-300))
    d = got - ref
    return (d.pow(2).sum(-1).sqrt() / den).max().item(), d.abs().max().item()


def lse_limit(ref):
    """|lse - lse_ref| allowed per row: 1e-5 * max(1, |lse_ref|, max |logit| of the row) -- about 40 fp32 epsilons, for the hardware
    exp2 / log2 and up to 1,024 summed terms."""
    return 1e-5 * torch.clamp(torch.maximum(ref.lse.abs(), ref.logits.abs().amax(-1)), min=1.0)


def _unit(g, B, H, hd):
    u = torch.randn(B, H, 1, hd, generator=g)
    return u / u.norm(dim=-1, keepdim=True)


def make_inputs(family, B, H, Sq, Skv, hd, seed, device="cpu"):
    """bf16 q, k, v, dO of one family; every sample is drawn from its own seed (so no two (batch, head) slices are alike).
      randn       unit normal: logits within about +-5, a nearly flat softmax
      peaked      q and k scaled by 3: logits to about +-45, the top key holds most of the mass
      offset      12 added to q and k along one axis: every logit carries a shared offset of 144 * scale that the softmax must cancel
      late_max    the LAST key dominates every query (it sits in the ragged tail tile when Skv % 32 != 0)
      first_max   key 0 dominates: every later tile rescales by alpha ~ 1 and adds almost nothing
      const_keys  all keys of a head identical: P is exactly uniform, lse = s + ln Skv, dq is exactly 0"""
    assert family in FAMILIES, family
    outs = []
    for b in range(B):
        g = torch.Generator().manual_seed(seed * 1000003 + b)
        q = torch.randn(1, H, Sq, hd, generator=g)
        k = torch.randn(1, H, Skv, hd, generator=g)
        v = torch.randn(1, H, Skv, hd, generator=g)
        do = torch.randn(1, H, Sq, hd, generator=g)
        if family == "peaked":
            q, k = q * 3, k * 3
        elif family == "offset":
            q[..., 0] += 12
            k[..., 0] += 12
        elif family in ("late_max", "first_max"):
            # k_dom = a u, q += c u (u a unit vector per head, c = 0.8 sqrt(hd), a c = D sqrt(hd)): the dominant logit is D + (a / sqrt(hd))
            # N(0, 1); the others are N(0, 1 + c^2 / hd) = N(0, 1.28^2), whose exponentials sum to about 2.3 Skv.  D = ln(2.3 Skv) + 3
            # puts the dominant key e^3 above ALL the others together on a typical row (top probability about 0.95) and 4 - 5 above the
            # largest of them.  (More dominance makes dq and dk vanish: with top probability 0.999 their bf16 error exceeds their size.)
            u = _unit(g, 1, H, hd)
            c = 0.8 * math.sqrt(hd)
            a = (math.log(2.3 * Skv) + 3) * math.sqrt(hd) / c
            k[..., -1 if family == "late_max" else 0, :] = a * u[..., 0, :]
            q = q + c * u
        elif family == "const_keys":
            k = k[..., :1, :].expand(-1, -1, Skv, -1).contiguous()
        outs.append((q, k, v, do))
    return tuple(torch.cat([o[i] for o in outs]).to(torch.bfloat16).to(device) for i in range(4))


def leak_one_key(k, v):
    """The inputs a kernel would effectively see if its key mask let ONE padded key through: a zero key and a zero value appended."""
    zk = torch.zeros_like(k[..., :1, :])
    return torch.cat([k, zk], -2), torch.cat([v, torch.zeros_like(zk)], -2)


def scale_of(hd):
    return 1.0 / math.sqrt(hd)
