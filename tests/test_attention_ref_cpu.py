"""The yardsticks of tests/test_attention_edges_gpu.py, checked where no GPU is needed: that the input families are as hard as they
claim, that the rounding emulation is close to (and not the same as) the fp64 reference, and -- by mutation -- that the limits the GPU
test asserts are tight enough to fail for the errors they are there to find (a leaked padded key, a single wrong row)."""
import functools

import pytest
import torch

from tests import attention_ref as ar

SHAPES = [(33, 77, 64), (64, 257, 32), (300, 150, 64)]
B, H = 2, 2


@functools.lru_cache(maxsize=None)
def _case(family, Sq, Skv, hd):
    """inputs, reference and emulation of one case: computed once, shared by the tests below, never modified."""
    x = ar.make_inputs(family, B, H, Sq, Skv, hd, seed=Sq + Skv + hd)
    sc = ar.scale_of(hd)
    return x, ar.reference(*x, sc), ar.emulation(*x, sc)


@pytest.mark.parametrize("Sq,Skv,hd", SHAPES)
def test_family_conditions(Sq, Skv, hd):
    for fam in ar.FAMILIES:
        (q, k, v, do), R, _ = _case(fam, Sq, Skv, hd)
        assert all(t.dtype == torch.bfloat16 for t in (q, k, v, do))
        assert q.shape == (B, H, Sq, hd) and k.shape == v.shape == (B, H, Skv, hd) and do.shape == q.shape
        for b in range(1, B):
            assert not torch.equal(q[b], q[0]) and not torch.equal(v[b], v[0]), "samples must differ"
    _, R, _ = _case("peaked", Sq, Skv, hd)
    top, smax = R.p.amax(-1).mean().item(), R.logits.abs().max().item()
    assert top >= 0.5 and 20 <= smax <= 60, (top, smax)
    _, R, _ = _case("offset", Sq, Skv, hd)
    assert R.logits.median().item() >= 15, R.logits.median().item()
    for fam, want in (("late_max", Skv - 1), ("first_max", 0)):
        _, R, _ = _case(fam, Sq, Skv, hd)
        frac = (R.logits.argmax(-1) == want).double().mean().item()
        assert frac >= 0.9, (fam, frac)
    (q, k, v, do), R, _ = _case("const_keys", Sq, Skv, hd)
    assert (R.p - 1.0 / Skv).abs().max().item() <= 1e-12
    assert (R.lse - (R.logits[..., 0] + torch.log(torch.tensor(float(Skv), dtype=torch.float64)))).abs().max().item() <= 1e-12
    assert R.dq.abs().max().item() <= 1e-12 * R.dk.abs().max().item()


@pytest.mark.parametrize("Sq,Skv,hd", SHAPES)
@pytest.mark.parametrize("family", ar.FAMILIES)
def test_emulation_is_close_but_not_exact(family, Sq, Skv, hd):
    """o: bf16 output rounding, 2^-9 .. 2^-8 per element (measured 1.8e-3 .. 3.2e-3 per row).  Gradients: a fixed number for randn only
    (measured 3.6e-3 .. 4.4e-3); the hard families are ill-conditioned by design (dq of late_max: 1.2e-1), which is why the GPU limit is
    relative to the emulation."""
    _, R, E = _case(family, Sq, Skv, hd)
    e_o = ar.row_err(E.o, R.o)[0]
    assert 0 < e_o <= 5e-3, e_o
    assert (E.lse - R.lse).abs().le(ar.lse_limit(R)).all()
    for name in ("dq", "dk", "dv"):
        rel, ab = ar.row_err(getattr(E, name), getattr(R, name))
        assert ab > 0, name
        if family == "randn":
            assert rel <= 8e-3, (name, rel)


def test_row_err_definition():
    ref = torch.zeros(4, 8, dtype=torch.float64)
    ref[0], ref[1], ref[2], ref[3] = 1.0, 2.0, 1e-3, 0.0
    got = ref.clone()
    got[2, 0] += 0.5                   # a tiny row is measured against the typical row norm, not its own
    typ = ref.pow(2).sum(-1).mean().sqrt().item()
    rel, ab = ar.row_err(got, ref)
    assert rel == pytest.approx(0.5 / typ) and ab == pytest.approx(0.5)
    got = ref.clone()
    got[1] *= 1.01                     # a large row against its own norm
    assert ar.row_err(got, ref)[0] == pytest.approx(0.01)
    assert ar.row_err(torch.full((3, 4), 0.25), torch.zeros(3, 4))[1] == 0.25      # a zero reference: the absolute error is the measure


@pytest.mark.parametrize("hd", [64, 32])
def test_mutation_leaked_key_exceeds_lse_limit(hd):
    """const_keys at Skv = 257 (one key in the ragged tile of the phased forward, the streaming forward's first size): a padded key that
    reaches the softmax with logit 0 and value 0 shifts lse by ln(1 + exp(-s) / 257).  The lse limit of the GPU test must be 10 times or
    more below that shift at the worst row, and below it for most rows."""
    Sq, Skv = 64, 257
    q, k, v, do = ar.make_inputs("const_keys", B, H, Sq, Skv, hd, seed=5)
    sc = ar.scale_of(hd)
    R = ar.reference(q, k, v, do, sc)
    kl, vl = ar.leak_one_key(k, v)
    M = ar.reference(q, kl, vl, do, sc)
    ratio = (M.lse - R.lse).abs() / ar.lse_limit(R)
    assert ratio.max().item() >= 10, ratio.max().item()
    assert (ratio > 1).double().mean().item() > 0.5
    # and with v = 1 the output is no longer exactly 1: the leaked mass is visible in bf16 for the rows where it exceeds half an ulp
    ones = torch.ones_like(v)
    _, vl1 = ar.leak_one_key(k, ones)
    o1 = ar.emulation(q, kl, vl1, do, sc).o
    assert (o1 != 1.0).any()
    assert (ar.emulation(q, k, ones, do, sc).o == 1.0).all()


@pytest.mark.parametrize("Sq,Skv,hd", SHAPES)
@pytest.mark.parametrize("family", [f for f in ar.FAMILIES if f != "const_keys"])      # (const_keys: every row of o is the same row)
def test_mutation_single_wrong_row_exceeds_limit(family, Sq, Skv, hd):
    """An output that is the emulation's except for two swapped rows (the smallest mistake an index error makes) must exceed the GPU
    test's limit, 2 x the emulation's own row_err -- a whole-tensor relative RMS would let it pass.  o in every family listed; the gradients
    where their rows are of one size (randn, peaked, offset).  With a dominant key (late_max, first_max) the gradient rows of the
    queries it saturates are far below the typical row, and row_err measures those against the typical row by design: swapping two of
    them is a small error there."""
    _, R, E = _case(family, Sq, Skv, hd)
    for name in ("o", "dq", "dk", "dv") if family in ("randn", "peaked", "offset") else ("o",):
        got, ref = getattr(E, name), getattr(R, name)
        lim = 2 * ar.row_err(got, ref)[0]
        bad = got.clone()
        r = got.shape[-2] - 1              # the last (tail) row and its neighbour, in one (batch, head) only
        bad[1, 0, r], bad[1, 0, r - 1] = got[1, 0, r - 1], got[1, 0, r]
        assert ar.row_err(bad, ref)[0] > lim, (name, ar.row_err(bad, ref)[0], lim)
