"""Where md_attn_fwd / md_attn_bwd put O, dQ, dK, dV (csrc/attention.hip: store_rows, store_lines), for every store path.

The kernels write their results in one of three forms -- 8 bytes per lane (plain), 16 bytes per lane after a half-wave exchange (WIDE),
whole 128-byte head slices read back from a dead LDS image (LINES) -- which must be three routes for the same bf16 values to the same
addresses.  A 16-byte or whole-slice store that lands 8 bytes or one head off would pass a value tolerance on most elements, so:

placement  every output lives in a buffer filled with one NaN bit pattern: q / k / v as thirds of one [B (S + G), 3 H hd + PAD] row (dq, dk,
           dv likewise, o and dO in [B (S + G), H hd + PAD] rows), or q, k, dq, dk head-major.  After a launch everything outside the addressed
           region must hold the pattern bit for bit: the G guard rows behind every sample (rows >= S), the PAD padding columns of every
           row, the v third when dq / dk are written (and so on), and -- when only heads 1 .. H - 1 are launched, through offset pointers --
           the slices of head 0.  Inside, everything is finite (written) and, for the sub-range launch, bit-identical to the full launch.
values     against tests/attention_ref.py with the rule of tests/test_attention_edges_gpu.py: worst-row error against the fp64 reference
           within FACTOR = 2 x that of the emulation (the kernels' rounding points) against the same reference.
agreement  the 16-byte forms need 16-byte aligned row pieces and the kernels fall back to the plain form per tensor when an output is
           not (the interface asks for 8): the same problem with o, dq, dk, dv moved 8 bytes is the forced plain form, and must give
           the same bits in every output.

Every backward selector the library accepts for the shape runs (0: its rule, 2 / 3 / 4: the fused forms, 5: the streaming pair): each
reaches another store path.  B = 9: one window of 8 samples of the XCD remap plus a sample in plain order."""
from ctypes import byref
from functools import lru_cache

import pytest
import torch

from tests import attention_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
G, PAD = 8, 8                  # guard rows behind every sample; padding columns of every row
POISON = 0x7FA5                # a bf16 NaN
FACTOR = 2.0                   # tests/test_attention_edges_gpu.py
H = 3
SHAPES = [(64, 64), (64, 77), (77, 77), (40, 77), (96, 40), (256, 77), (200, 33), (256, 256)]
CASES = [(9, Sq, Skv, hd, layout) for Sq, Skv in SHAPES for hd in (64, 32) for layout in ("packed", "hm")]
CASES += [(2, 320, 320, hd, layout) for hd in (64, 32) for layout in ("packed", "hm")]      # the streaming kernels


@lru_cache(maxsize=None)
def problem(B, Sq, Skv, hd):
    """Inputs, fp64 reference and emulation of one shape: computed once, shared by the layouts, never modified."""
    x = ar.make_inputs("randn", B, H, Sq, Skv, hd, seed=B + 7 * Sq + 11 * Skv + hd, device=DEV)
    return x, ar.reference(*x, ar.scale_of(hd)), ar.emulation(*x, ar.scale_of(hd))


class Buf:
    """A poisoned bf16 allocation and one [B, H, S, hd] tensor addressed inside it; `shift` elements (0 or 4) move the whole tensor."""

    def __init__(self, n, shift):
        self.bits = torch.full((n + 8,), POISON, device=DEV, dtype=torch.int16)
        self.flat = self.bits.view(BF)
        self.shift = shift

    def tensor(self, B, S, hd, sb, hs, ld, off):
        t = Tensor()
        t.buf, t.sb, t.hs, t.ld, t.off = self, sb, hs, ld, off + self.shift
        t.shape = (B, H, S, hd)
        return t


class Tensor:
    def view(self, h0=0):
        B, _, S, hd = self.shape
        return self.buf.flat.as_strided((B, H - h0, S, hd), (self.sb, self.hs, self.ld, 1), self.off + h0 * self.hs)

    def ptr(self, h0=0):
        return self.buf.flat.data_ptr() + 2 * (self.off + h0 * self.hs)


def outside(buf, tensors, h0):
    """Elements of buf that no launch of heads h0 .. H - 1 of `tensors` may write."""
    m = torch.ones_like(buf.bits, dtype=torch.bool)
    for t in tensors:
        B, _, S, hd = t.shape
        m.as_strided((B, H - h0, S, hd), (t.sb, t.hs, t.ld, 1), t.off + h0 * t.hs).fill_(False)
    return m


class Layout:
    """The buffers of one problem.  packed: q, k, v thirds of one row; hm: q and k head-major [B, H, S + G, hd], v in its third."""

    def __init__(self, B, Sq, Skv, hd, hm, shift):
        hid, Sm = H * hd, max(Sq, Skv)
        ld3, ld1 = 3 * hid + PAD, hid + PAD
        rows = B * (Sm + G)

        def group(shift):
            pk = Buf(rows * ld3, shift)
            t = {"v": pk.tensor(B, Skv, hd, (Sm + G) * ld3, hd, ld3, 2 * hid)}
            bufs = [pk]
            for i, (n, S) in enumerate((("q", Sq), ("k", Skv))):
                if hm:
                    b = Buf(B * H * (S + G) * hd, shift)
                    t[n] = b.tensor(B, S, hd, H * (S + G) * hd, (S + G) * hd, hd, 0)
                    bufs.append(b)
                else:
                    t[n] = pk.tensor(B, S, hd, (Sm + G) * ld3, hd, ld3, i * hid)
            return t, bufs

        self.B, self.Sq, self.Skv, self.hd, self.hm = B, Sq, Skv, hd, hm
        self.inp, _ = group(0)
        self.inp["do"] = Buf(rows * ld1, 0).tensor(B, Sq, hd, (Sm + G) * ld1, hd, ld1, 0)
        self.new_grads = lambda: group(shift)
        self.new_o = lambda s=shift: Buf(rows * ld1, s).tensor(B, Sq, hd, (Sm + G) * ld1, hd, ld1, 0)

    def args(self, hip, o, lse, g, delta, split, h0):
        i, hs = self.inp, (lambda t: t.hs if self.hm else 0)
        P = lambda t: t.ptr(h0) if t is not None else None
        dq, dk, dv = (g[n] for n in "qkv") if g else (None, None, None)
        a = hip.AttnArgs(P(i["q"]), P(i["k"]), P(i["v"]), P(o), lse.data_ptr(), P(i["do"]), P(dq), P(dk), P(dv),
                         delta.data_ptr() if delta is not None else None, self.B, H - h0, self.Sq, self.Skv,
                         i["q"].ld, i["k"].ld, i["v"].ld, o.ld, i["q"].sb, i["k"].sb, i["v"].sb, o.sb,
                         dq.ld if g else 0, dk.ld if g else 0, dv.ld if g else 0, i["do"].ld,
                         dq.sb if g else 0, dk.sb if g else 0, dv.sb if g else 0, i["do"].sb, ar.scale_of(self.hd), self.hd, split)
        a.hsq, a.hsk = hs(i["q"]), hs(i["k"])
        if g:
            a.hsdq, a.hsdk = hs(dq), hs(dk)
        return a


def placed(what, bufs, tensors, h0):
    """Nothing outside the addressed region was written; everything inside was."""
    for buf in bufs:
        mine = [t for t in tensors if t.buf is buf]
        assert bool((buf.bits[outside(buf, mine, h0)] == POISON).all()), f"{what}: a store landed outside the addressed region"
    for t in tensors:
        assert bool(torch.isfinite(t.view(h0)).all()), f"{what}: unwritten or non-finite elements inside"


def judge(what, got, ref, emu):
    kern, yard = ar.row_err(got, ref)[0], ar.row_err(emu, ref)[0]
    print(f"ATTN_STORES | {what} | kernel {kern:.3e} | emulation {yard:.3e} | ratio {kern / yard:.3f}")
    assert kern <= FACTOR * yard, f"{what}: kernel {kern:.3e} > {FACTOR} x emulation {yard:.3e}"


def run(hip, L, splits, shift, h0, o_in=None):
    """Forward, then every backward form of `splits`, heads h0 .. H - 1, outputs moved by `shift` elements; placement checked after
    every launch.  o_in: the forward output the backward reads (an aligned, bit-identical one for the shifted run: the backward LOADS
    o 16 bytes at a time).  Returns (o, lse, {split: {q, k, v: gradient tensors}})."""
    lib, st = hip.lib(), hip.stream_ptr()
    tag = f"{L.Sq}x{L.Skv}x{L.hd} {'hm' if L.hm else 'packed'} shift={shift} heads {h0}..{H - 1}"
    mk = lambda: torch.full((L.B, H - h0, L.Sq), float("nan"), device=DEV)
    o, lse = L.new_o(), mk()
    hip.check(lib.md_attn_fwd(byref(L.args(hip, o, lse, None, None, 0, h0)), st), "md_attn_fwd")
    torch.cuda.synchronize()
    placed(f"{tag} fwd", [o.buf], [o], h0)
    assert bool(torch.isfinite(lse).all())
    grads = {}
    for split in splits:
        (g, bufs), delta = L.new_grads(), mk()
        rc = lib.md_attn_bwd(byref(L.args(hip, o_in or o, lse, g, delta, split, h0)), st)
        torch.cuda.synchronize()
        if split in (2, 3, 4) and max(L.Sq, L.Skv) > 256:
            assert rc == -1, f"{tag}: forced fused form {split} must refuse this shape"
            continue
        hip.check(rc, "md_attn_bwd")
        placed(f"{tag} bwd_split={split}", bufs, list(g.values()), h0)
        grads[split] = g
    return o, lse, grads


@pytest.mark.parametrize("B,Sq,Skv,hd,layout", CASES)
def test_row_stores(hip, B, Sq, Skv, hd, layout):
    x, R, E = problem(B, Sq, Skv, hd)
    splits = (0, 2, 3, 4, 5)
    mk = lambda shift: Layout(B, Sq, Skv, hd, layout == "hm", shift)
    L = mk(0)
    for n, t in zip(("q", "k", "v", "do"), x):
        L.inp[n].view().copy_(t)
    tag = f"{Sq}x{Skv}x{hd} {layout}"

    o, lse, grads = run(hip, L, splits, 0, 0)
    assert sorted(grads) == ([0, 2, 3, 4, 5] if max(Sq, Skv) <= 256 else [0, 5])
    judge(f"{tag} o", o.view(), R.o, E.o)
    for s, g in grads.items():
        for n in "qkv":
            judge(f"{tag} bwd_split={s} d{n}", g[n].view(), getattr(R, "d" + n), getattr(E, "d" + n))

    # the plain 8-byte form (outputs 8 bytes off a 16-byte boundary) against the forms the library picked
    Ls = mk(4)
    Ls.inp = L.inp
    o8, lse8, grads8 = run(hip, Ls, splits, 4, 0, o_in=o)
    assert torch.equal(o8.view(), o.view()) and torch.equal(lse8, lse), f"{tag}: o differs between the store forms"
    for s, g in grads.items():
        for n in "qkv":
            assert torch.equal(grads8[s][n].view().view(torch.int16), g[n].view().view(torch.int16)), \
                f"{tag} bwd_split={s}: d{n} differs between the store forms"

    # heads 1 .. H - 1 alone, through offset pointers: head 0's slices stay poisoned, the others repeat the full launch
    o1, lse1, grads1 = run(hip, L, splits, 0, 1)
    assert torch.equal(o1.view(1), o.view(1)) and torch.equal(lse1, lse[:, 1:])
    for s, g in grads.items():
        for n in "qkv":
            assert torch.equal(grads1[s][n].view(1).view(torch.int16), g[n].view(1).view(torch.int16)), \
                f"{tag} bwd_split={s}: d{n} of the head sub-range differs from the full launch"
