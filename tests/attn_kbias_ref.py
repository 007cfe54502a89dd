"""Yardsticks of the biased attention (md_attn_fwd_kbias, md_attn_probs_kbias), shared by
tests/test_attn_kbias_kernel_gpu.py and tests/test_prompt_control_gpu.py.  Torch only, any device; built on tests/attention_ref.py and
tests/attn_probs_ref.py, which stay as they are.

    o = softmax_j(scale q . k_j + bias[b, j]) V        bias fp32 [B, Skv], one value per (sample, key); -inf removes a key

reference   fp64 from the bf16 operands and the fp32 bias -- what the kernel approximates.
emulation   the same with the kernel's rounding points and nothing else of it: the logit scale * q . k rounded to fp32, the bias added to
            it and the sum rounded to fp32 (the one rounding the bias form adds), then attention_ref.emulation's forward: the
            unnormalised p = exp(s - rowmax) rounded to bf16 before P.V, its row sum from the unrounded p, o rounded to bf16,
            lse = rowmax + log l in fp32.
Both return attention_ref's tuples (forward fields only), so attention_ref.row_err / lse_limit and the FACTOR rule of
tests/test_attention_edges_gpu.py apply unchanged.  Ref.logits holds the biased logits with the removed entries (-inf) set to 0:
lse_limit takes the row's largest |logit|, and a removed key has none.

The probe's bound.  tests/attn_probs_ref.py derives |got - ref| <= (2 E + 2^-16) ref + 2^-24 for md_attn_probs, E being the bound of
the row's score error |s - s_exact| (accumulation and the scale multiply).  md_attn_probs_kbias forms s' = s + b with ONE more fp32
rounding, |s' - (s + b)| <= u |s + b| (u = 2^-24; b itself is exact, an input), and nothing else changes: the removed keys are
exp2(-inf) = 0 exactly, in the numerator and in the sum.  So the same derivation holds with
    E' = E + u max_j |s_j + b_j|        (the maximum over the heads and the live keys of the row; s in fp64)
and the same 2^-16 and 2^-24 terms: every magnitude bound used there (arguments of the exponent within 17 of the maximum, at most
128 + 2 summed terms) is a property of the softmax, not of where the logits come from."""
import torch

from tests import attention_ref as ar
from tests import attn_probs_ref as pr


def _biased_logits(q, k, bias, scale, round_f32):
    s = q.double() @ k.double().transpose(-1, -2) * scale
    b = bias.double()[:, None, None, :]
    if round_f32:
        return ar._rb(ar._rb(s, torch.float32) + b, torch.float32)
    return s + b


def reference(q, k, v, bias, scale):
    """q [B, H, Sq, hd], k, v [B, H, Skv, hd] (bf16), bias fp32 [B, Skv] -> attention_ref.Ref with o, lse, logits, p (fp64)."""
    s = _biased_logits(q, k, bias, scale, False)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    return ar.Ref(p @ v.double(), lse, None, None, None, s.masked_fill(torch.isinf(s), 0.0), None, p)


def emulation(q, k, v, bias, scale):
    """attention_ref.Emu with o (bf16 values) and lse (fp32 values), in fp64."""
    bf, f32 = torch.bfloat16, torch.float32
    s = _biased_logits(q, k, bias, scale, True)
    m = s.max(-1, keepdim=True).values
    pu = ar._rb(torch.exp(s - m), f32)
    l = ar._rb(pu.sum(-1, keepdim=True), f32)
    o = ar._rb((ar._rb(pu, bf) @ v.double()) / l, bf)
    return ar.Emu(o, ar._rb(m + torch.log(l), f32)[..., 0], None, None, None, None)


def probs_reference(q, k, bias, scale):
    """(ref fp64 [B, Sq, Skv], the head mean of the biased softmax; E' fp64 [B, Sq], the row's score-error bound derived above)."""
    _, E = pr.reference(q, k, scale)
    s = _biased_logits(q, k, bias, scale, False)
    ref = torch.softmax(s, dim=-1).mean(1)
    live = s.masked_fill(torch.isinf(s), 0.0).abs().amax(dim=(1, 3))
    return ref, E + pr.U * live


def log_weights(w):
    """The bias of caption weights: ln w in fp32 (0 -> -inf)."""
    return torch.log(w.to(torch.float32))
