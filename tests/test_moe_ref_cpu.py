"""Keeps tests/moe_ref.py honest without a GPU: its routing and combine against the oracle's expert-choice MoE, its bit-level
combine against fp64 where every sum is exact, its tie order against closed forms, its mask tables against the two-argsort form."""
import pytest
import torch
import torch.nn.functional as F

from oracle import microdit_ref as orc
from tests import moe_ref as mr

F64 = torch.float64


@pytest.mark.parametrize("n,t,E,cap,d,f", [(2, 24, 4, 2.0, 8, 12), (3, 40, 16, 2.0, 16, 8)], ids=["E4", "E16"])
def test_routing_and_combine_reproduce_the_oracle(n, t, E, cap, d, f):
    """Tie-free inputs: softmax64 + topk_tables + an fp64 combine are oracle.ec_moe.  The gate weight is [I | 0], so the logits are
    the first E features of x, which are bf16 values: softmax64's rounding changes nothing and both sides see the same logits."""
    g = torch.Generator().manual_seed(100 + E)
    x = torch.randn(n, t, d, generator=g, dtype=F64)
    x[..., :E] = x[..., :E].to(torch.bfloat16).double()
    gate = torch.zeros(E, d, dtype=F64)
    gate[:, :E] = torch.eye(E, dtype=F64)
    sd = {"m.gate.weight": gate, "m.w1": torch.randn(E, d, f, generator=g, dtype=F64), "m.w2": torch.randn(E, f, d, generator=g, dtype=F64)}
    out, m, gv = orc.ec_moe(sd, "m", x, E, cap, return_routing=True)
    k = m.shape[-1]
    assert k == int(cap * t / E)
    logits = x.reshape(n * t, d)[:, :E]
    probs = mr.softmax64(logits, E)
    for e in range(E):                                    # tie-free: the premise under which torch.topk's order is determined
        for s in range(n):
            assert probs[s * t:(s + 1) * t, e].unique().numel() == t
    rowidx, gval, slot = mr.topk_tables(probs, n, t, E, k)
    got_idx = rowidx.view(E, n, k).permute(1, 0, 2).long() - (torch.arange(n) * t).view(n, 1, 1)
    assert torch.equal(got_idx, m)
    assert torch.allclose(gval.view(E, n, k).permute(1, 0, 2), gv, rtol=1e-14, atol=0)
    assert int(slot.min()) == -1 and int(slot.max()) == k - 1
    for e in range(E):                                    # slot is the inverse of rowidx
        assert torch.equal(slot[rowidx[e].long(), e].long(), torch.arange(k).repeat(n))
    xin = x.reshape(n * t, d)[rowidx.long()]                                         # [E, n k, d]
    h2 = torch.einsum("erf,efd->erd", F.gelu(torch.einsum("erd,edf->erf", xin, sd["m.w1"])), sd["m.w2"])
    br = mr.combine64(h2, gval, slot, n, t, E, k)
    assert torch.allclose(br.view(n, t, d), out, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("stride", [None, 29], ids=["dense", "abs"])
def test_bit_level_combine_is_exact_where_sums_are_exact(stride):
    """Small integers and powers of two: every product, partial sum and the gated residual is a bf16 value, so the bit-level
    restatement (with all its intermediate roundings) must equal the unrounded fp64 result exactly, in both addressings."""
    B, S, E, k, C = 2, 12, 5, 4, 8
    g = torch.Generator().manual_seed(7)
    scores = torch.rand(B * S, E, generator=g)
    rowidx, _, slot = mr.topk_tables(scores, B, S, E, k)
    n = B * k if stride is None else stride
    if stride is not None:                                # absolute positions: the dense ones mirrored into a longer list
        smp = (torch.arange(B * S) // S).view(-1, 1)
        slot = torch.where(slot >= 0, (stride - 1 - (smp * k + slot)).to(torch.int32), slot)
    gval = 2.0 ** torch.randint(-2, 2, (E, n), generator=g).float()
    h2 = torch.randint(-3, 4, (E, n, C), generator=g).to(torch.bfloat16)
    res = torch.randint(-4, 5, (B * S, C), generator=g).to(torch.bfloat16)
    gate = (2.0 ** torch.randint(-1, 2, (B, C), generator=g).float()).to(torch.bfloat16)
    br, out = mr.combine(h2, gval, slot, res, gate, B, S, E, k, stride=stride)
    br64 = mr.combine64(h2, gval, slot, B, S, E, k, stride=stride)
    assert torch.equal(br.double(), br64)
    smp = torch.arange(B * S) // S
    assert torch.equal(out.double(), res.double() + gate[smp].double() * br64)
    none = (slot < 0).all(1)
    assert bool(none.any()) and not bool(br[none].float().abs().any()) and torch.equal(out[none], res[none])
    # the sensitivity knobs do something
    tok = int((slot[:, 0] >= 0).nonzero()[0])
    br2, _ = mr.combine(h2, gval, slot, res, gate, B, S, E, k, stride=stride, skip=(tok, 0))
    assert torch.equal(br2.double()[tok], br64[tok] - gval[0, _pos(slot, tok, 0, S, k, stride)].double() * h2[0, _pos(slot, tok, 0, S, k, stride)].double())
    dxin = torch.randint(-3, 4, (E, n, C), generator=g).to(torch.bfloat16)
    ones = torch.ones(E, n)
    assert torch.equal(mr.scatter_sum(dxin, slot, B, S, E, k, stride=stride).double(), mr.combine64(dxin, ones, slot, B, S, E, k, stride=stride))


def _pos(slot, tok, e, S, k, stride):
    return int(slot[tok, e]) if stride is not None else (tok // S) * k + int(slot[tok, e])


def test_backward_restatements_against_autograd():
    """combine_bwd's dg / dh2 and softmax_bwd64 are the gradients autograd gives for the fp64 forward."""
    B, S, E, k, C, ldo = 2, 10, 3, 4, 8, 8
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(B * S, E, generator=g).to(torch.bfloat16).double().requires_grad_(True)
    probs = torch.softmax(logits, -1)
    rowidx, gval, slot = mr.topk_tables(probs.detach(), B, S, E, k)
    h2 = torch.randn(E, B * k, C, generator=g).to(torch.bfloat16)
    dbr = torch.randn(B * S, C, generator=g).to(torch.bfloat16)
    h2d = h2.double().requires_grad_(True)
    gv = torch.gather(probs.view(B, S, E).permute(0, 2, 1), -1,
                      (rowidx.view(E, B, k).permute(1, 0, 2).long() - (torch.arange(B) * S).view(B, 1, 1))).permute(1, 0, 2).reshape(E, B * k)
    assert torch.equal(gv.detach(), gval)
    (mr.combine64(h2d, gv, slot, B, S, E, k) * dbr.double()).sum().backward()
    dh2, dg, dga, terms = mr.combine_bwd(dbr, h2, rowidx, gval.float())
    assert torch.allclose(dh2.double().view(E, B * k, C), h2d.grad, rtol=2.0 ** -7, atol=0)      # two roundings, fp32 then bf16
    assert torch.equal(terms.sum(-1), dg) and bool((dga >= dg.abs()).all())
    ref, mag = mr.softmax_bwd64(probs.detach(), dg.view(E, B * k), slot, B, S, E, k, ldo)
    assert torch.allclose(ref[:, :E], logits.grad, rtol=1e-11, atol=1e-14)
    assert not bool(ref[:, E:].abs().any()) and bool((mag[:, :E] >= ref[:, :E].abs() - 1e-15).all())


def test_crafted_ties_come_out_in_closed_form():
    """Ties go to the lower token: the three constructions of the GPU test, through an fp32 softmax (in which exp(-120) is 0)."""
    for logits, lists, B, S, E, k in ((*mr.tie_all_equal(2, 70, 3, 19), 2, 70, 3, 19), (*mr.tie_saturated(100, 4, 40), 1, 100, 4, 40),
                                      (*mr.tie_pairs(40, 33), 1, 80, 2, 33)):
        probs = torch.softmax(logits.to(torch.bfloat16).float(), -1)
        rowidx, gval, slot = mr.topk_tables(probs, B, S, E, k)
        got = rowidx.view(E, B, k).permute(1, 0, 2).long() - (torch.arange(B) * S).view(B, 1, 1)
        assert torch.equal(got, lists)
    logits, lists = mr.tie_saturated(100, 4, 40)
    p = torch.softmax(logits, -1)
    assert set(p.unique().tolist()) == {0.0, 1.0}
    logits, lists = mr.tie_pairs(40, 33)
    assert int(lists[0, 0, -1]) % 2 == 0 and int(lists[0, 0, -1]) + 1 not in lists[0, 0].tolist(), "a pair straddles rank k - 1"


def test_mask_tables_equal_the_two_argsort_form():
    g = torch.Generator().manual_seed(3)
    noise = torch.randint(0, 9, (4, 50), generator=g).float() / 8          # duplicated values throughout
    for len_keep in (1, 13, 50):
        keep_rows, restore, mask = mr.mask_tables(noise, len_keep)
        shuffle = torch.argsort(noise, dim=1, stable=True)
        want_restore = torch.argsort(shuffle, dim=1, stable=True)
        assert torch.equal(restore.long(), want_restore)
        assert torch.equal(keep_rows.view(4, len_keep).long(), shuffle[:, :len_keep] + torch.arange(4).view(4, 1) * 50)
        assert torch.equal(mask, (want_restore >= len_keep).float())
        want = orc.get_mask(noise, 1 - len_keep / 50)
        if int(50 * (1 - (1 - len_keep / 50))) == len_keep:               # the oracle derives len_keep from a ratio
            assert torch.equal(mask, want["mask"]) and torch.equal(restore.long(), want["ids_restore"])


def test_compact_restatement_on_a_hand_case():
    """One expert, two samples: list order kept, pads = the first routed row with gate 0, dropped tokens -1."""
    B, S, E, k, Tk = 2, 4, 1, 2, 2
    rowidx = torch.tensor([[3, 0, 5, 6]], dtype=torch.int32)
    gval = torch.tensor([[0.875, 0.75, 0.625, 0.5]])
    ids_restore = torch.tensor([[0, 1, 2, 3], [3, 2, 1, 0]], dtype=torch.int32)    # kept: tokens 0, 1 and 6, 7
    rc, gc, count, sc = mr.compact(rowidx, gval, ids_restore, Tk, B, S, E, k)
    assert rc.tolist() == [[0, 6, 3, 3]] and gc.tolist() == [[0.75, 0.5, 0.0, 0.0]] and count.tolist() == [2]
    assert sc.view(-1).tolist() == [0, -1, -1, -1, -1, -1, 1, -1]
