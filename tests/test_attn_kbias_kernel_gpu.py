"""md_attn_fwd_kbias and md_attn_probs_kbias at their edges, against tests/attn_kbias_ref.py.

Accuracy follows the rule of tests/test_attention_edges_gpu.py unchanged: the worst-row error of o against the fp64 reference stays
within FACTOR = 2 x the emulation's against the same reference, lse within attention_ref.lse_limit on the biased logits.  Three
properties are exact (torch.equal on the bits of o and lse): a zero bias reproduces md_attn_fwd, -inf on the trailing keys [n, Skv)
reproduces md_attn_fwd with Skv = n on the same buffers, and NaN in everything of the bias buffer the kernel must not read changes
nothing.  The buffers are the guarded ones of that file (its Problem / GBuf / FBuf); the bias sits in a buffer whose pad columns
[Skv, ldb) and whose row behind the last sample hold NaN, in every test.

Shapes (B = 3, H = 2), layouts alternating over the sorted list, plus both layouts at 256 x 77 x 64 and 33 x 77 x 32:
    Sq in {1, 31, 33, 64, 65, 129, 256} x Skv 77 x hd 64     one to four waves; LINES (<= 2 waves), WIDE and PLAIN (hd 64, four waves) stores
    Sq in {33, 129, 256} x Skv 77 x hd 32                    the hd 32 instantiations of 2, 4 and 4 waves
    Sq 65 x Skv in {1, 31, 32, 33, 64, 77, 255, 256} x hd 64  the 32-key stage edges
    Sq 33 x the same Skv x hd 32
    256 x 256 x 64, 129 x 255 x 32
Bias families, each where the key count has room for it: random finite biases in [-8, 4]; scattered -inf (a third of the keys, never
all; Skv >= 3); a whole 32-key tile of -inf in the middle (Skv > 64); the first tile all -inf (Skv > 32); one live key.  The input
family (randn, peaked, late_max) rotates over the list, and all three run with every bias family at 65 x 77 x 64 and 256 x 77 x 64."""
import ctypes
from ctypes import byref

import pytest
import torch

from tests import attention_ref as ar
from tests import attn_kbias_ref as kr
from tests import attn_probs_ref as pr
from tests import test_attention_edges_gpu as edges
from tests import test_attn_probs_kernel_gpu as probe

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 3, 2
NEG = float("-inf")

SQ = (1, 31, 33, 64, 65, 129, 256)
SKV = (1, 31, 32, 33, 64, 77, 255, 256)
_SHAPES = sorted({(sq, 77, 64) for sq in SQ} | {(sq, 77, 32) for sq in (33, 129, 256)} | {(65, skv, 64) for skv in SKV}
                 | {(33, skv, 32) for skv in SKV} | {(256, 256, 64), (129, 255, 32)})
CASES = [(sq, skv, hd, "hm" if i % 2 else "packed") for i, (sq, skv, hd) in enumerate(_SHAPES)]
CASES += [c for c in ((256, 77, 64, "packed"), (256, 77, 64, "hm"), (33, 77, 32, "packed"), (33, 77, 32, "hm")) if c not in CASES]
BIASES = ("random", "scattered", "mid_tile", "first_tile", "one_live")
INPUTS = ("randn", "peaked", "late_max")


def applies(bias, Skv):
    return {"random": True, "scattered": Skv >= 3, "mid_tile": Skv > 64, "first_tile": Skv > 32, "one_live": True}[bias]


ACC_CASES = [(*c, bias, INPUTS[(i + j) % 3]) for i, c in enumerate(CASES) for j, bias in enumerate(BIASES) if applies(bias, c[1])]
ACC_CASES += [(sq, 77, 64, "packed", bias, fam) for sq in (65, 256) for bias in BIASES for fam in INPUTS
              if (sq, 77, 64, "packed", bias, fam) not in ACC_CASES]


def make_bias(kind, Skv, seed):
    """fp32 [B, Skv] on the GPU; every sample its own draw."""
    g = torch.Generator().manual_seed(seed)
    b = torch.rand(B, Skv, generator=g) * 12 - 8                       # finite, in [-8, 4]
    if kind == "scattered":
        for i in range(B):
            drop = torch.randperm(Skv, generator=g)[:max(1, Skv // 3)]
            b[i, drop] = NEG
    elif kind == "mid_tile":
        t = (Skv // 32) // 2                                           # a whole tile with live tiles on both sides
        b[:, 32 * t:32 * t + 32] = NEG
    elif kind == "first_tile":
        b[:, :32] = NEG
    elif kind == "one_live":
        live = torch.randint(0, Skv, (B,), generator=g)
        keep = b[torch.arange(B), live].clone()
        b[:] = NEG
        b[torch.arange(B), live] = keep
    assert bool(torch.isfinite(b).any(-1).all())
    return b.to(DEV)


class KBias:
    """The bias [B, Skv] inside fp32 [B + 1, ldb]: ldb = Skv rounded up to 4, plus 4, so pad columns always exist; the pad columns and
    the row behind the last sample hold NaN."""

    def __init__(self, bias):
        nb, Skv = bias.shape
        self.ldb = (Skv + 3) // 4 * 4 + 4
        self.buf = torch.full((nb + 1, self.ldb), float("nan"), device=DEV, dtype=torch.float32)
        self.buf[:nb, :Skv] = bias
        self.before = self.buf.clone().view(torch.int32)

    def ptr(self):
        return self.buf.data_ptr()

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before)


def run_kbias(hip, p, f, kb, expect=0):
    rc = p.L.md_attn_fwd_kbias(byref(p.args(f)), kb.ptr(), kb.ldb, p.st)
    assert rc == expect, rc
    torch.cuda.synchronize()


def problem(hip, family, Sq, Skv, hd, layout, seed):
    x = edges.inputs(family, B, H, Sq, Skv, hd, seed)
    return edges.Problem(hip, *x, layout), x


# ------------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("Sq,Skv,hd,layout,bias,family", ACC_CASES)
def test_biased_attention_meets_the_factor_rule(hip, Sq, Skv, hd, layout, bias, family):
    p, (q, k, v, _) = problem(hip, family, Sq, Skv, hd, layout, Sq * 1000 + Skv + hd)
    b = make_bias(bias, Skv, Sq + 7 * Skv + hd)
    kb, f = KBias(b), p.fwd_out()
    run_kbias(hip, p, f, kb)
    tag = f"kbias {Sq}x{Skv}x{hd} {layout} {bias}"
    p.check_memory(tag, written=list(f.items()))
    assert kb.untouched()
    R, E = kr.reference(q, k, v, b, p.scale), kr.emulation(q, k, v, b, p.scale)
    edges.judge(tag, family, {"o": f["o"].inner}, R, E, ["o"])
    edges.judge_lse(f"{tag} {family}", f["lse"].inner, R)
    if bias == "scattered":
        # the same keys deleted from the inputs: a removed key is a key that is not there
        for i in range(B):
            keep = torch.isfinite(b[i])
            qi, ki, vi, bi = q[i:i + 1], k[i:i + 1, :, keep], v[i:i + 1, :, keep], b[i:i + 1, keep]
            Rd, Ed = kr.reference(qi, ki, vi, bi, p.scale), kr.emulation(qi, ki, vi, bi, p.scale)
            edges.judge(f"{tag} deleted b={i}", family, {"o": f["o"].inner[i:i + 1]}, Rd, Ed, ["o"])
            edges.judge_lse(f"{tag} deleted b={i} {family}", f["lse"].inner[i:i + 1], Rd)


def test_cases_cover_the_issue():
    assert {c[0] for c in CASES} == set(SQ) and {c[1] for c in CASES} == set(SKV) and {c[2] for c in CASES} == {32, 64}
    assert {c[3] for c in CASES} == {"packed", "hm"}
    for bias in BIASES:
        assert {c[5] for c in ACC_CASES if c[4] == bias} == set(INPUTS), bias
        assert {c[3] for c in ACC_CASES if c[4] == bias} == {"packed", "hm"}, bias


# ------------------------------------------------------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("Sq,Skv,hd,layout", CASES)
def test_zero_bias_gives_the_bits_of_the_plain_forward(hip, Sq, Skv, hd, layout):
    p, _ = problem(hip, "randn", Sq, Skv, hd, layout, Sq * 1000 + Skv + hd + 1)
    f0, f1 = p.fwd_out(), p.fwd_out()
    hip.check(p.fwd(p.args(f0)), "md_attn_fwd")
    run_kbias(hip, p, f1, KBias(torch.zeros(B, Skv, device=DEV)))
    assert torch.equal(f0["o"].bits, f1["o"].bits) and torch.equal(f0["lse"].bits, f1["lse"].bits)


@pytest.mark.parametrize("layout", ["packed", "hm"])
@pytest.mark.parametrize("Sq,hd", [(65, 64), (256, 64), (33, 32)])
@pytest.mark.parametrize("n,Skv", [(20, 77), (32, 77), (33, 64), (1, 256)])
def test_trailing_removed_keys_give_the_bits_of_a_shorter_key_set(hip, n, Skv, Sq, hd, layout):
    """A padding mask: the caption behaves as if it were n keys long.  The plain forward runs with Skv = n on the SAME buffers (the
    strides of the Skv-key problem), so both read the same bytes for the live keys."""
    p, _ = problem(hip, "randn", Sq, Skv, hd, layout, n * 1000 + Skv + Sq)
    f0, f1 = p.fwd_out(), p.fwd_out()
    a = p.args(f0)
    a.Skv = n
    hip.check(p.fwd(a), "md_attn_fwd")
    b = torch.zeros(B, Skv, device=DEV)
    b[:, n:] = NEG
    run_kbias(hip, p, f1, KBias(b))
    assert torch.equal(f0["o"].bits, f1["o"].bits) and torch.equal(f0["lse"].bits, f1["lse"].bits)


@pytest.mark.parametrize("Sq,Skv,hd,layout", [(65, 77, 64, "packed"), (256, 77, 64, "hm"), (33, 255, 32, "packed")])
def test_constant_keys_give_the_weights_themselves(hip, Sq, Skv, hd, layout):
    """All keys of a head identical: P_j = w_j / sum w for every query, o = sum_j w_j v_j / sum w, lse = s + ln sum w."""
    p, (q, k, v, _) = problem(hip, "const_keys", Sq, Skv, hd, layout, Sq + Skv + hd)
    g = torch.Generator().manual_seed(Skv)
    w = torch.rand(B, Skv, generator=g) * 3
    w[:, ::5] = 0.0
    w[:, 1] = 1.0
    w = w.to(DEV)
    b = kr.log_weights(w)
    f = p.fwd_out()
    run_kbias(hip, p, f, KBias(b))
    wd = w.double()
    pw = (wd / wd.sum(-1, keepdim=True))[:, None, None, :]                       # [B, 1, 1, Skv]
    o_ref = (pw @ v.double()).expand(B, H, Sq, hd)
    s = (q.double() @ k.double().transpose(-1, -2) * p.scale)[..., 0]            # every key gives the same logit
    R = ar.Ref(o_ref, s + wd.sum(-1).log()[:, None, None], None, None, None, s[..., None], None, None)
    E = kr.emulation(q, k, v, b, p.scale)
    tag = f"const_keys weights {Sq}x{Skv}x{hd} {layout}"
    edges.judge(tag, "const_keys", {"o": f["o"].inner}, R, E, ["o"])
    edges.judge_lse(tag, f["lse"].inner, R)


# ------------------------------------------------------------------------------------------------------------------ guards
class OBuf(edges.GBuf):
    """The o of Problem.fwd_out() with every row piece 8 bytes off a 16-byte boundary (what md_attn_args allows: ldo, so, hso % 4)."""

    def __init__(self, nb, nh, S, hd, hid):
        G = edges.G
        self.ld, self.hs, self.hm = hid + 8, hd, False
        self.sb, self.off0, n = (S + G) * self.ld, G * self.ld + 4, (2 * G + nb * (S + G)) * self.ld
        self.flat = torch.empty(n, device=DEV, dtype=torch.bfloat16)
        self.bits = self.flat.view(torch.int16)
        self.bits.fill_(edges.NAN16)
        geom = ((nb, nh, S, hd), (self.sb, self.hs, self.ld, 1), self.off0)
        self.inner = self.flat.as_strided(*geom)
        self.outside = torch.ones(n, device=DEV, dtype=torch.bool)
        self.outside.as_strided(*geom).fill_(False)
        self.before = None


@pytest.mark.parametrize("Sq,hd", [(33, 64), (129, 32), (256, 64)])
def test_output_off_the_16_byte_grid_takes_the_plain_stores(hip, Sq, hd):
    Skv = 77
    p, (q, k, v, _) = problem(hip, "randn", Sq, Skv, hd, "packed", Sq + hd)
    b = make_bias("scattered", Skv, Sq)
    f, f8 = p.fwd_out(), p.fwd_out()
    f8["o"] = OBuf(B, H, Sq, hd, p.hid)
    f8["o"].snap()
    assert f8["o"].ptr() % 16 == 8
    run_kbias(hip, p, f, KBias(b))
    run_kbias(hip, p, f8, KBias(b))
    p.check_memory("o off the 16-byte grid", written=list(f8.items()))
    assert torch.equal(f["o"].inner, f8["o"].inner) and torch.equal(f["lse"].bits, f8["lse"].bits)


@pytest.mark.parametrize("Sq,Skv,hd,layout", [(65, 77, 64, "packed"), (256, 33, 64, "hm"), (33, 255, 32, "hm"), (1, 1, 32, "packed")])
def test_nothing_outside_the_bias_is_read(hip, Sq, Skv, hd, layout):
    """The NaN pad columns and the NaN row behind the last sample against a tight, clean buffer [B, ldb = Skv rounded up to 4] of zeros
    beyond Skv: the same bits.  (Every other test of this file runs on the NaN-padded buffer too.)"""
    p, _ = problem(hip, "randn", Sq, Skv, hd, layout, Sq + Skv)
    b = make_bias("random", Skv, Skv)
    ldb = (Skv + 3) // 4 * 4
    tight = torch.zeros(B, ldb, device=DEV)
    tight[:, :Skv] = b
    f0, f1 = p.fwd_out(), p.fwd_out()
    assert p.L.md_attn_fwd_kbias(byref(p.args(f0)), tight.data_ptr(), ldb, p.st) == 0
    run_kbias(hip, p, f1, KBias(b))
    p.check_memory("NaN pads", written=list(f1.items()))
    assert torch.equal(f0["o"].bits, f1["o"].bits) and torch.equal(f0["lse"].bits, f1["lse"].bits)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(hip):
    Sq, Skv, hd = 33, 77, 64
    p, _ = problem(hip, "randn", Sq, Skv, hd, "packed", 5)
    kb = KBias(torch.zeros(B, Skv, device=DEV))
    f = p.fwd_out()
    L, st = p.L, p.st
    a = p.args(f)
    assert L.md_attn_fwd_kbias(byref(a), None, kb.ldb, st) == -1, "NULL kbias"
    assert L.md_attn_fwd_kbias(byref(a), kb.ptr() + 4, kb.ldb, st) == -1, "kbias off the 16-byte grid"
    assert L.md_attn_fwd_kbias(byref(a), kb.ptr(), Skv - 1, st) == -1, "ldb < Skv"
    assert L.md_attn_fwd_kbias(byref(a), kb.ptr(), kb.ldb + 2, st) == -1, "ldb % 4 != 0"
    assert L.md_attn_fwd_kbias(None, kb.ptr(), kb.ldb, st) == -1, "NULL arguments"
    p.check_memory("refusals", idle=list(f.items()))
    for name, (skv, hd_) in {"Skv = 257": (257, 64), "hd = 48": (77, 48)}.items():
        p2, _ = problem(hip, "randn", Sq, skv, hd_, "packed", 6)
        kb2, f2 = KBias(torch.zeros(B, skv, device=DEV)), p2.fwd_out()
        assert L.md_attn_fwd_kbias(byref(p2.args(f2)), kb2.ptr(), kb2.ldb, st) == -1, name
        p2.check_memory(name, idle=list(f2.items()))


# ------------------------------------------------------------------------------------------------------------------ the probe
def _probs(hip, q, k, kb=None, expect=0):
    """md_attn_probs (kb None) or md_attn_probs_kbias on the packed form of test_attn_probs_kernel_gpu: out [B, Sq, ldo]."""
    nb, nh, Sq, hd = q.shape
    Skv = k.shape[2]
    qb, ldq, sq = probe._packed(q)
    kbuf, ldk, sk = probe._packed(k, width_mult=2)
    a = probe._args(hip, qb, 0, ldq, sq, 0, kbuf, 0, ldk, sk, 0, nb, nh, Sq, Skv, hd)
    ldo = (Skv + 3) // 4 * 4
    out = torch.zeros(nb * Sq, ldo, device=DEV)
    if kb is None:
        rc = hip.lib().md_attn_probs(byref(a), out.data_ptr(), ldo, None, probe._st())
    else:
        rc = hip.lib().md_attn_probs_kbias(byref(a), kb.ptr(), kb.ldb, out.data_ptr(), ldo, None, probe._st())
    assert rc == expect, rc
    torch.cuda.synchronize()
    return out.view(nb, Sq, ldo)


@pytest.mark.parametrize("bias", ["random", "scattered", "one_live"])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("Skv", [1, 17, 77, 128])
def test_probe_meets_the_derived_bound(hip, Skv, hd, bias):
    if not applies(bias, Skv):
        bias = "random"
    Sq = 65
    q, k = probe._qk(B, 3, Sq, Skv, hd, 77 + Skv + hd)
    b = make_bias(bias, Skv, Skv + hd)
    out = _probs(hip, q, k, KBias(b))
    got = out[:, :, :Skv]
    ref, E = kr.probs_reference(q, k, b, pr.f32_scale(hd))
    pr.assert_within_bound(got, ref, E, f"probe kbias Skv={Skv} hd={hd} {bias}")
    removed = torch.isinf(b)[:, None, :].expand(B, Sq, Skv)
    assert bool((got[removed] == 0).all()), "a removed position must record exactly 0"
    torch.testing.assert_close(got.sum(-1), torch.ones(B, Sq, device=DEV), rtol=2e-5, atol=0)
    assert bool((out[:, :, Skv:] == 0).all())


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("Skv", [1, 17, 77, 128])
def test_probe_with_a_zero_bias_is_the_plain_probe(hip, Skv, hd):
    q, k = probe._qk(B, 3, 65, Skv, hd, 5 + Skv + hd)
    assert torch.equal(_probs(hip, q, k), _probs(hip, q, k, KBias(torch.zeros(B, Skv, device=DEV))))


def test_probe_refusals(hip):
    q, k = probe._qk(B, 3, 17, 77, 64, 3)
    kb = KBias(torch.zeros(B, 77, device=DEV))

    class Bad:
        def __init__(self, ptr, ldb):
            self._p, self.ldb = ptr, ldb

        def ptr(self):
            return self._p
    for bad in (Bad(None, kb.ldb), Bad(kb.ptr() + 4, kb.ldb), Bad(kb.ptr(), 76), Bad(kb.ptr(), kb.ldb + 2)):
        out = _probs(hip, q, k, bad, expect=-1)
        assert bool((out == 0).all())
    q, k = probe._qk(B, 3, 17, 129, 64, 4)
    _probs(hip, q, k, KBias(torch.zeros(B, 129, device=DEV)), expect=-1)
