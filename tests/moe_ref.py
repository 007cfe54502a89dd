"""Plain torch restatements of the MoE routing kernels of csrc/routing.hip (CPU or GPU tensors, no HIP), one function per kernel,
each in the arithmetic the kernel promises, so that tests/test_moe_geometry_gpu.py can demand bits wherever bits are determined.

Layouts (those of the kernels): token rows m = n * S + t; an expert's routed list rowidx / gval [E, B * k] with entry n * k + j the
rank-j pick of sample n; slot [B * S, E] the inverse map (rank, or -1).  The "absolute" forms (`stride` given) address position
slot of a list of `stride` entries per expert instead of n * k + slot (md_moe_*_abs / *_compact).

torch's fp32 -> bf16 conversion rounds to nearest even, as the kernels' f2bf does; its fp32 products and sums are IEEE.
tests/test_moe_ref_cpu.py holds these functions to the oracle (oracle/microdit_ref.py) and to closed forms."""
import torch

I32, F32, F64, BF16 = torch.int32, torch.float32, torch.float64, torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------- routing
def bf16_logits(logits, E):
    """The logits the softmax kernel sees: the first E columns rounded to bf16 (round to nearest even), as fp64."""
    return logits[:, :E].float().to(BF16).double()


def softmax64(logits, E):
    """moe_softmax_kernel: logits rounded to bf16, then an fp64 softmax over the first E columns.  [M, E] fp64."""
    return torch.softmax(bf16_logits(logits, E), dim=-1)


def topk_tables(probs, B, S, E, k):
    """moe_topk_kernel from GIVEN probabilities (any float dtype; the first E columns of [B * S, >= E]): per (sample, expert) the k
    highest, descending, ties to the lower token (a stable descending sort).  rowidx [E, B * k] int32 (absolute token rows), gval
    [E, B * k] (dtype of probs), slot [B * S, E] int32 in {-1, 0 .. k-1}."""
    p = probs[:, :E].reshape(B, S, E).permute(0, 2, 1)                                   # [B, E, S]
    order = torch.sort(p, dim=-1, descending=True, stable=True).indices[..., :k]          # [B, E, k]
    g = torch.gather(p, -1, order)
    base = (torch.arange(B, device=probs.device) * S).view(B, 1, 1)
    rowidx = (order + base).permute(1, 0, 2).reshape(E, B * k).to(I32)
    gval = g.permute(1, 0, 2).reshape(E, B * k).contiguous()
    slot = torch.full((B, E, S), -1, dtype=torch.int64, device=probs.device)
    slot.scatter_(-1, order, torch.arange(k, device=probs.device).expand(B, E, k).contiguous())
    return rowidx.contiguous(), gval, slot.permute(0, 2, 1).reshape(B * S, E).to(I32).contiguous()


def _positions(slot, B, S, k, stride):
    """(list position [M, E] int64 (0 where unselected), selected [M, E] bool, list length) for the dense (n * k + slot, B * k) or
    the absolute (slot, stride) addressing."""
    M = B * S
    sel = slot >= 0
    s = slot.long().clamp_min(0)
    if stride is None:
        n = (torch.arange(M, device=slot.device) // S).view(M, 1)
        return n * k + s, sel, B * k
    return s, sel, stride


def table_index_range(slot, B, S, k, stride=None):
    """(min, max, list length) of the list positions a slot table addresses: the host-side bounds check before a launch."""
    pos, sel, n = _positions(slot, B, S, k, stride)
    if not bool(sel.any()):
        return 0, 0, n
    return int(slot.min()), int(pos[sel].max()), n


# ------------------------------------------------------------------------------------------------------------------- combine
def combine(h2, gval, slot, res, gate, B, S, E, k, stride=None, order=None, skip=None):
    """moe_combine_kernel to the bit:  br = bf16( sum over experts in ascending order, fp32, of bf16(fp32(g * h)) ),
    out = bf16( fp32(res + gate * br) )  (gate * br is a product of two bf16 values, exact in fp32: contraction cannot change it).
    h2 [E, list, C] bf16, gval [E, list] fp32, res [M, C] bf16, gate [B, C] bf16.  order: the expert order of the sum (default
    ascending); skip = (row, expert): that one contribution left out -- both only for sensitivity checks."""
    M, C = res.shape
    pos, sel, n = _positions(slot, B, S, k, stride)
    h2, gval = h2.reshape(E, n, C), gval.reshape(E, n)
    if skip is not None:
        sel = sel.clone()
        sel[skip[0], skip[1]] = False
    acc = torch.zeros(M, C, dtype=F32, device=res.device)
    zero = torch.zeros((), dtype=F32, device=res.device)
    for e in (range(E) if order is None else order):
        term = (gval[e, pos[:, e]].view(M, 1) * h2[e, pos[:, e]].float()).to(BF16).float()
        acc = acc + torch.where(sel[:, e].view(M, 1), term, zero)
    br = acc.to(BF16)
    smp = torch.arange(M, device=res.device) // S
    out = (res.float() + gate[smp].float() * br.float()).to(BF16)
    return br, out


def combine64(h2, gval, slot, B, S, E, k, stride=None):
    """The same sum without any rounding: br [M, C] fp64."""
    M = B * S
    pos, sel, n = _positions(slot, B, S, k, stride)
    C = h2.shape[-1]
    h2, gval = h2.reshape(E, n, C).double(), gval.reshape(E, n).double()
    acc = torch.zeros(M, C, dtype=F64, device=slot.device)
    zero = torch.zeros((), dtype=F64, device=slot.device)
    for e in range(E):
        acc = acc + torch.where(sel[:, e].view(M, 1), gval[e, pos[:, e]].view(M, 1) * h2[e, pos[:, e]], zero)
    return acc


def combine_bwd(dbr, h2, rowidx, gval, rows=None):
    """moe_combine_bwd_kernel over the flat routed rows `rows` (default: all):  dh2 = bf16(fp32(g * dbr[token])) to the bit; dg the
    dot product <dbr[token], h2[row]> in fp64, with sum|terms| next to it and the per-column terms (for a left-out-term check)."""
    C = dbr.shape[-1]
    h2, rowidx, gval = h2.reshape(-1, C), rowidx.reshape(-1), gval.reshape(-1)
    if rows is None:
        rows = torch.arange(rowidx.numel(), device=rowidx.device)
    d = dbr[rowidx[rows].long()]
    dh2 = (gval[rows].view(-1, 1) * d.float()).to(BF16)
    terms = d.double() * h2[rows].double()
    return dh2, terms.sum(-1), terms.abs().sum(-1), terms


def scatter_sum(dxin, slot, B, S, E, k, stride=None):
    """moe_scatter_sum_kernel to the bit: dx = bf16( fp32 sum over the selecting experts, ascending ) of dxin [E, list, C] bf16."""
    M = B * S
    pos, sel, n = _positions(slot, B, S, k, stride)
    C = dxin.shape[-1]
    dxin = dxin.reshape(E, n, C)
    acc = torch.zeros(M, C, dtype=F32, device=slot.device)
    zero = torch.zeros((), dtype=F32, device=slot.device)
    for e in range(E):
        acc = acc + torch.where(sel[:, e].view(M, 1), dxin[e, pos[:, e]].float(), zero)
    return acc.to(BF16)


def softmax_bwd64(probs, dgval, slot, B, S, E, k, ldo, stride=None):
    """moe_softmax_bwd_kernel in fp64: dlogits_e = p_e (dp_e - sum_e' dp_e' p_e'), dp_e = the selected entry of dgval or 0; columns
    [E, ldo) zero.  Returns (dlogits [M, ldo], mag [M, ldo]) with mag_e = p_e (|dp_e| + sum |dp p|), the scale of its fp32 error."""
    M = B * S
    pos, sel, n = _positions(slot, B, S, k, stride)
    p = probs[:, :E].double()
    dg = dgval.reshape(E, n).double()
    dp = torch.where(sel, torch.gather(dg.t(), 0, pos), torch.zeros((), dtype=F64, device=slot.device))    # [M, E]
    dot, adot = (dp * p).sum(-1, keepdim=True), (dp * p).abs().sum(-1, keepdim=True)
    ref = torch.zeros(M, ldo, dtype=F64, device=slot.device)
    mag = torch.zeros_like(ref)
    ref[:, :E] = p * (dp - dot)
    mag[:, :E] = p * (dp.abs() + adot)
    return ref, mag


# ------------------------------------------------------------------------------------------------------------------- masking
def mask_tables(noise, len_keep):
    """get_mask_kernel: a stable ascending sort of the noise [B, T] per sample.  keep_rows [B * len_keep] int32 (absolute rows of
    the len_keep lowest, in rank order), ids_restore [B, T] int32 (the rank of every token), mask [B, T] fp32 (1 = dropped)."""
    B, T = noise.shape
    shuffle = torch.sort(noise, dim=1, stable=True).indices
    restore = torch.empty_like(shuffle)
    restore.scatter_(1, shuffle, torch.arange(T, device=noise.device).expand(B, T).contiguous())
    keep_rows = (shuffle[:, :len_keep] + torch.arange(B, device=noise.device).view(B, 1) * T).reshape(-1).to(I32)
    return keep_rows.contiguous(), restore.to(I32), (restore >= len_keep).to(F32)


def compact(rowidx, gval, ids_restore, Tk, B, S, E, k):
    """md_moe_compact_kept.  List order = the order of the expert's routed list (sample-major, then rank); pads: the expert's first
    routed row, gate 0."""
    dev = rowidx.device
    keep = ids_restore.view(-1) < Tk
    rowidx_c = torch.empty_like(rowidx)
    gval_c = torch.zeros_like(gval)
    count = torch.empty(E, device=dev, dtype=I32)
    slot_c = torch.full((B * S, E), -1, device=dev, dtype=I32)
    for e in range(E):
        toks = rowidx[e].long()
        kp = keep[toks]
        c = int(kp.sum())
        rowidx_c[e, :c] = rowidx[e][kp]
        rowidx_c[e, c:] = rowidx[e, 0]
        gval_c[e, :c] = gval[e][kp]
        slot_c[toks[kp], e] = torch.arange(c, device=dev, dtype=I32)
        count[e] = c
    return rowidx_c, gval_c, count, slot_c


# ------------------------------------------------------------------------------------------------------------------- tie cases
# Logits whose top-k lists have a closed form that does not depend on any computed probability, only on "equal logit rows give equal
# probabilities" and "a larger logit in a column (the others equal) gives a larger probability there".  Each returns
# (logits [B * S, E] fp32, lists [B, E, k] int64 of token numbers inside the sample).
def tie_all_equal(B, S, E, k):
    """(i) every logit equal: every expert's list is tokens 0 .. k-1 in order."""
    return torch.full((B * S, E), 0.375), torch.arange(k).expand(B, E, k).contiguous()


def tie_saturated(S, E, k):
    """(ii) one sample, logits +-60: token t has +60 in column (t * 7) % E and -60 elsewhere, so in fp32 its probabilities are exactly
    1.0 there and 0.0 elsewhere (exp(-120) underflows to 0).  With fewer ones than k: the ones in token order, then the
    lowest-numbered zeros."""
    col = (torch.arange(S) * 7) % E
    logits = torch.full((S, E), -60.0)
    lists = torch.empty(1, E, k, dtype=torch.int64)
    t = torch.arange(S)
    for e in range(E):
        logits[col == e, e] = 60.0
        ones, zeros = t[col == e], t[col != e]
        assert 0 < ones.numel() < k <= S, "fewer ones than k"
        lists[0, e] = torch.cat([ones, zeros])[:k]
    return logits, lists


def tie_pairs(npairs, k, seed=0):
    """(iii) one sample, E = 2, S = 2 npairs: tokens (2 j, 2 j + 1) share the row (a_j, 0) with the a_j distinct multiples of 1 / 4 in
    [-8, 8) in shuffled order.  Expert 0 ranks the pairs by descending a_j, expert 1 by ascending; k odd, so a pair straddles rank
    k - 1: its token 2 j is in, 2 j + 1 is out."""
    assert k % 2 == 1 and k < 2 * npairs and npairs <= 64
    g = torch.Generator().manual_seed(seed)
    a = (torch.randperm(64, generator=g)[:npairs].double() - 32) / 4
    logits = torch.zeros(2 * npairs, 2)
    logits[:, 0] = a.repeat_interleave(2).float()
    lists = torch.empty(1, 2, k, dtype=torch.int64)
    for e, desc in ((0, True), (1, False)):
        pairs = torch.sort(a, descending=desc).indices
        lists[0, e] = torch.stack([2 * pairs, 2 * pairs + 1], 1).reshape(-1)[:k]
    return logits, lists
