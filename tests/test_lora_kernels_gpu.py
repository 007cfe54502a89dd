"""md_lora_merge / md_lora_grad (csrc/lora.hip) against fp64 torch on the same fp32 values, at the kernels' edge shapes: rows below,
equal to and not a multiple of the 64-row strip (8, 16, 200, 384, 1088, 1), one strip and many, one column chunk and several, cols not
a multiple of the 128-column merge tile (192, 64), every rank class.  Each shape alone, and all of them as one table at every rank.

Bounds (U = 2^-24, the fp32 unit roundoff):
  merge  |v - ref| <= (rank + 3) U (|p| + scale sum_j |B_nj| |A_jk|)           rank fmas, then one fma with p
  dB     |dB - ref| <= (cols + 4) U c sum_k |G_nk| |A_jk|                      c = scale * grad_scale (one fp32 product)
  dA     |dA - ref| <= (rows + 4) U c sum_n |B_nj| |G_nk|
The gradients are ADDED to d_adapter: with a non-zero d_adapter the stored sum carries one more rounding, U |d0 + ref|, which the bound
of that case adds (the issue's bounds are checked as they stand on a zero d_adapter).  Everything else is compared bit for bit.
Guard words (a NaN-free sentinel) fill every element the kernels must not touch: before, between and after the tensors of p / the
outputs, the adapter gradient's padding, and both ends of the workspace."""
import ctypes

import numpy as np
import pytest
import torch

from micro_diffusion_amd import lora

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -768.0                               # exactly representable in bf16 and fp32
SHAPES = [(8, 128, 4), (16, 256, 16), (200, 192, 8), (384, 128, 64), (1088, 512, 16), (1, 64, 32)]
SCALE = float(np.float32(0.6))
GSCALE = float(np.float32(0.37))


class Case:
    """Tensors of the given (rows, cols) placed in flat buffers with gaps; everything random normal fp32 from one seeded CPU generator."""

    def __init__(self, hip, shapes, rank, seed, zero_b=False):
        self.hip, self.rank, self.shapes = hip, rank, shapes
        gen = torch.Generator().manual_seed(seed)
        w_off, a_off, b_off, wtot, atot = [], [], [], 40, 12            # non-zero first offsets: multiples of 8 / 4
        for n, k in shapes:
            w_off.append(wtot)
            wtot += n * k + 8 * (1 + (n + k) % 5)                       # gaps of 8 .. 40 guard words
            a_off.append(atot)
            atot += rank * k + 4
            b_off.append(atot)
            atot += n * rank + 4 * (1 + n % 3)
        self.w_off, self.a_off, self.b_off, self.wtot, self.atot = w_off, a_off, b_off, wtot, atot
        self.p = torch.full((wtot,), SENT)
        self.g = torch.full((wtot,), SENT)
        self.ad = torch.full((atot,), SENT)
        self.wmask = torch.zeros(wtot, dtype=torch.bool)
        self.amask = torch.zeros(atot, dtype=torch.bool)
        self.P, self.G, self.A, self.B = [], [], [], []
        for (n, k), w, a, b in zip(shapes, w_off, a_off, b_off):
            for buf, lst in ((self.p, self.P), (self.g, self.G)):
                buf[w:w + n * k] = torch.randn(n * k, generator=gen)
                lst.append(buf[w:w + n * k].view(n, k))
            self.ad[a:a + rank * k] = torch.randn(rank * k, generator=gen)
            self.ad[b:b + n * rank] = 0.0 if zero_b else torch.randn(n * rank, generator=gen)
            self.A.append(self.ad[a:a + rank * k].view(rank, k))
            self.B.append(self.ad[b:b + n * rank].view(n, rank))
            self.wmask[w:w + n * k] = True
            self.amask[a:a + rank * k] = True
            self.amask[b:b + n * rank] = True
        self.d0 = torch.randn(atot, generator=gen)
        self.items = (hip.LoraItem * len(shapes))(*[hip.LoraItem(w, a, b, 0, n, k) for (n, k), w, a, b in zip(shapes, w_off, a_off, b_off)])
        need = ctypes.c_int64(-1)
        assert hip.lib().md_lora_grad_ws_floats(self.items, len(shapes), rank, ctypes.byref(need)) == 0
        self.ws_floats = need.value
        self.items_dev = torch.from_numpy(np.frombuffer(self.items, dtype=np.uint8).copy()).cuda()
        self.p_d, self.g_d, self.ad_d = self.p.cuda(), self.g.cuda(), self.ad.cuda()

    def merge(self, out, f32, p=None, scale=SCALE, rank=None, items=None, expect=0):
        rc = self.hip.lib().md_lora_merge((self.p_d if p is None else p).data_ptr(), self.ad_d.data_ptr(), self.items_dev.data_ptr(),
                                          self.items if items is None else items, len(self.shapes), self.rank if rank is None else rank,
                                          scale, out.data_ptr(), 1 if f32 else 0, self.hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == expect, rc

    def grad(self, d, ws, ws_floats=None, gscale=GSCALE, rank=None, items=None, expect=0):
        rc = self.hip.lib().md_lora_grad(self.g_d.data_ptr(), self.ad_d.data_ptr(), self.items_dev.data_ptr(),
                                         self.items if items is None else items, len(self.shapes), self.rank if rank is None else rank,
                                         SCALE, gscale, d.data_ptr(), ws.data_ptr(), ws.numel() if ws_floats is None else ws_floats,
                                         self.hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == expect, rc


def _cases():
    out = [pytest.param([(n, k)], r, id=f"{n}x{k}-r{r}") for n, k, r in SHAPES]
    out += [pytest.param([(n, k) for n, k, _ in SHAPES], r, id=f"table-r{r}") for r in lora.RANKS]
    return out


@pytest.mark.parametrize("shapes,rank", _cases())
def test_merge(hip, shapes, rank):
    c = Case(hip, shapes, rank, seed=11 + rank + len(shapes))
    out32 = torch.full((c.wtot,), SENT, device="cuda")
    out16 = torch.full((c.wtot,), SENT, device="cuda", dtype=torch.bfloat16)
    c.merge(out32, True)
    c.merge(out16, False)
    o32, o16 = out32.cpu(), out16.cpu()
    assert bool((o32[~c.wmask] == SENT).all()) and bool((o16[~c.wmask].float() == SENT).all()), "a guard word was written"
    assert torch.equal(c.p_d.cpu(), c.p) and torch.equal(c.ad_d.cpu(), c.ad), "an input was written"
    for (n, k), w, P, A, B in zip(shapes, c.w_off, c.P, c.A, c.B):
        v = o32[w:w + n * k].view(n, k).double()
        ref = lora.ref_merge(P, A, B, SCALE)
        bound = (rank + 3) * U * (P.double().abs() + SCALE * (B.double().abs() @ A.double().abs()))
        worst = float(((v - ref).abs() / bound).max())
        print(f"merge {n}x{k} r{rank}: max |v - ref| / bound = {worst:.3f}")
        assert worst <= 1.0
    # the bf16 form is the rounding of exactly what the fp32 form stores
    assert torch.equal(o16[c.wmask].view(torch.int16), o32[c.wmask].to(torch.bfloat16).view(torch.int16))
    # fused onto the masters (out == p): the same bits as out of place, nothing else moves
    p2 = c.p_d.clone()
    c.merge(p2, True, p=p2)
    p2 = p2.cpu()
    assert torch.equal(p2[c.wmask], o32[c.wmask]) and bool((p2[~c.wmask] == SENT).all())


@pytest.mark.parametrize("shapes,rank", _cases()[:6] + _cases()[8:9])
def test_merge_with_zero_b_is_the_plain_cast(hip, shapes, rank):
    c = Case(hip, shapes, rank, seed=5, zero_b=True)
    out16 = torch.full((c.wtot,), SENT, device="cuda", dtype=torch.bfloat16)
    c.merge(out16, False)
    plain = torch.empty(c.wtot, device="cuda", dtype=torch.bfloat16)
    hip.check(hip.lib().md_cast_f32_bf16(c.p_d.data_ptr(), plain.data_ptr(), c.wtot, None, hip.stream_ptr()), "md_cast_f32_bf16")
    torch.cuda.synchronize()
    assert bool((out16.cpu()[c.wmask] == plain.cpu()[c.wmask]).all())
    # scale = 0 with a non-zero B: the same
    c2 = Case(hip, shapes, rank, seed=5)
    out = torch.full((c2.wtot,), SENT, device="cuda", dtype=torch.bfloat16)
    c2.merge(out, False, scale=0.0)
    hip.check(hip.lib().md_cast_f32_bf16(c2.p_d.data_ptr(), plain.data_ptr(), c2.wtot, None, hip.stream_ptr()), "md_cast_f32_bf16")
    torch.cuda.synchronize()
    assert bool(c2.ad[c2.b_off[0]:c2.b_off[0] + 4].any()) and bool((out.cpu()[c2.wmask] == plain.cpu()[c2.wmask]).all())


def _ws(c, pad=64):
    buf = torch.full((c.ws_floats + 2 * pad,), SENT, device="cuda")
    return buf, buf[pad:pad + c.ws_floats]


@pytest.mark.parametrize("shapes,rank", _cases())
def test_grad(hip, shapes, rank):
    c = Case(hip, shapes, rank, seed=23 + rank + len(shapes))
    coef = float(np.float32(SCALE) * np.float32(GSCALE))
    refs = [lora.ref_grad(G, A, B, SCALE, GSCALE) for G, A, B in zip(c.G, c.A, c.B)]
    sums = [(coef * (B.double().abs().t() @ G.double().abs()), coef * (G.double().abs() @ A.double().abs().t()))
            for G, A, B in zip(c.G, c.A, c.B)]
    for start in ("zero", "nonzero"):
        d0 = torch.zeros(c.atot) if start == "zero" else c.d0.clone()
        d0[~c.amask] = SENT
        d = d0.cuda()
        frame, ws = _ws(c)
        c.grad(d, ws)
        got = d.cpu()
        assert bool((got[~c.amask] == SENT).all()), "padding of the adapter gradient was written"
        f = frame.cpu()
        assert bool((f[:64] == SENT).all()) and bool((f[64 + c.ws_floats:] == SENT).all()), "a workspace guard word was written"
        assert torch.equal(c.g_d.cpu(), c.g) and torch.equal(c.ad_d.cpu(), c.ad), "an input was written"
        for (n, k), a, b, (rA, rB), (sA, sB) in zip(shapes, c.a_off, c.b_off, refs, sums):
            dA, dB = got[a:a + rank * k].view(rank, k).double(), got[b:b + n * rank].view(n, rank).double()
            tA, tB = d0[a:a + rank * k].view(rank, k).double() + rA, d0[b:b + n * rank].view(n, rank).double() + rB
            bA, bB = (n + 4) * U * sA, (k + 4) * U * sB
            if start == "nonzero":
                bA, bB = bA + U * tA.abs(), bB + U * tB.abs()
            wA, wB = float(((dA - tA).abs() / bA).max()), float(((dB - tB).abs() / bB).max())
            print(f"grad {n}x{k} r{rank} from a {start} d_adapter: max |dA - ref| / bound = {wA:.3f}, max |dB - ref| / bound = {wB:.3f}")
            assert wA <= 1.0 and wB <= 1.0
        # deterministic: a second call on the same data, into a workspace that holds other bits, gives the same bits
        d2 = d0.cuda()
        frame2 = torch.full_like(frame, 3.5)
        c.grad(d2, frame2[64:64 + c.ws_floats])
        assert torch.equal(d2.cpu().view(torch.int32), got.view(torch.int32))
    # grad_scale is applied: 2 x grad_scale gives 2 x the result, exactly (a power of two)
    d1, d2 = torch.zeros(c.atot, device="cuda"), torch.zeros(c.atot, device="cuda")
    c.grad(d1, _ws(c)[1])
    c.grad(d2, _ws(c)[1], gscale=2 * GSCALE)
    assert torch.equal(d2.cpu(), 2 * d1.cpu()) and bool(d1.cpu()[c.amask].any())


def test_bad_arguments_launch_nothing(hip):
    shapes = [(200, 192), (16, 256)]
    c = Case(hip, shapes, 8, seed=3)
    out = torch.full((c.wtot,), SENT, device="cuda")
    d = torch.full((c.atot,), SENT, device="cuda")
    frame, ws = _ws(c)
    need = ctypes.c_int64(-1)

    def items(edit):
        arr = (hip.LoraItem * 2)(*[hip.LoraItem(it.w_off, it.a_off, it.b_off, it.ws_off, it.rows, it.cols) for it in c.items])
        edit(arr)
        return arr

    def set_cols(a):
        a[0].cols = 188

    def set_rows(a):
        a[1].rows = 0

    def set_off(a):
        a[0].w_off += 4

    def set_ws(a):
        a[1].ws_off += 4

    for rank in (0, 2, 12, 24, 128):                                  # unsupported rank
        c.merge(out, True, rank=rank, expect=-1)
        c.grad(d, ws, rank=rank, expect=-1)
        assert hip.lib().md_lora_grad_ws_floats(c.items, 2, rank, ctypes.byref(need)) == -1
    for edit in (set_cols, set_rows, set_off):                        # cols % 8 != 0, no rows, a misaligned tensor
        c.merge(out, True, items=items(edit), expect=-1)
        c.grad(d, ws, items=items(edit), expect=-1)
        assert hip.lib().md_lora_grad_ws_floats(items(edit), 2, 8, ctypes.byref(need)) == -1
    c.grad(d, ws, items=items(set_ws), expect=-1)                     # not the layout md_lora_grad_ws_floats wrote
    assert c.ws_floats == (4 * 8 * 192 + 1 * 8 * 256)
    c.grad(d, ws, ws_floats=c.ws_floats - 1, expect=-1)               # too small a workspace
    c.grad(d, ws, ws_floats=0, expect=-1)
    for null in ("p", "adapter", "items", "host", "out"):
        args = [c.p_d.data_ptr(), c.ad_d.data_ptr(), c.items_dev.data_ptr(), c.items, 2, 8, SCALE, out.data_ptr(), 1, hip.stream_ptr()]
        args[{"p": 0, "adapter": 1, "items": 2, "host": 3, "out": 7}[null]] = None
        assert hip.lib().md_lora_merge(*args) == -1, null
    assert hip.lib().md_lora_merge(c.p_d.data_ptr() + 4, c.ad_d.data_ptr(), c.items_dev.data_ptr(), c.items, 2, 8, SCALE, out.data_ptr(), 1,
                                   hip.stream_ptr()) == -1, "a base that is not 16-byte aligned"
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENT).all()) and bool((d.cpu() == SENT).all()) and bool((frame.cpu() == SENT).all()), "something was launched"
    c.grad(d, ws, ws_floats=c.ws_floats)                              # exactly enough: runs
    assert bool((d.cpu()[c.amask] != SENT).any()) and bool((d.cpu()[~c.amask] == SENT).all())
