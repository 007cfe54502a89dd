"""md_attn_fwd / md_attn_bwd where test_attention (tests/test_kernels_gpu.py) does not look: the XCD batch remap (B >= 8), every
dispatch boundary of the sequence lengths, inputs with a hard softmax, lse and delta as outputs, and guard rows around every buffer.

Yardsticks (tests/attention_ref.py, checked on the CPU by tests/test_attention_ref_cpu.py): `reference` is fp64 from the bf16 inputs;
`emulation` is the same operation with the kernels' rounding points.  Per case and tensor the kernel's worst-row error against the
reference (row_err) must stay within FACTOR x the emulation's against the same reference -- FACTOR = 2 covers accumulation order and
the hardware exp2 / log2.  lse is held to 1e-5 * max(1, |lse|, max |logit| of the row); delta (written by the streaming pair only) to
1e-5 * sum_d |dO * O| of the row, against fp64 over the bf16 o that the backward was given.

Guard rows: every tensor is one allocation whose batch stride is 32 rows larger than needed (head-major tensors: 32 rows after every
head), with 32 more rows in front and behind; lse and delta have 32 floats on each side.  Everything outside the addressed region
holds one NaN bit pattern.  After every call the inputs and every guard element must be bit-identical and the region inside finite, so
an access that strays by up to a tile reads a NaN or breaks the pattern inside the test's own allocation.

Measured on an MI355X (134 tests, 1,722 figures; every test prints its figures before it asserts them -- pytest -s).  Wall time of the
file: about 6 s, of which 1.4 s is the first test loading the library; every other test takes 0.01 - 0.05 s.
Worst kernel / emulation ratio of row_err per family (limit 2; no family needs more, FACTOR is 2 throughout):
                 o      dq     dk     dv
    randn        1.08   1.26   1.11   1.00      (dq: remap B=17 33x77x32, dk: remap B=9 129x128x64, o: boundary 257x257x64)
    peaked       1.00   1.00   1.03   1.00
    offset       1.04   1.00   1.34   1.00      (dk: 200x200x64)
    late_max     1.00   1.00   1.00   1.00
    first_max    1.00   1.00   1.01   1.00
    const_keys   1.00   1.00*  1.00   1.00      (* maximum absolute error: the reference is zero)
  (1.00: the worst row of the kernel is the worst row of the emulation with the same bf16 values in it.)
lse: worst 0.026 of its limit (const_keys 64x257x32).  delta: worst 0.007 of its limit (late_max 300x150x32, randn 257x257x64).
One key (Skv = 1): dq and dk, zero in the reference and in the emulation, came out at up to 8.8e-7 -- the two summation orders of
zero_grad_floor(), whose worst-case allowance for those cases is 4.6e-5 .. 6.4e-3.
Sensitivity, checked once against two deliberately wrong, memory-safe builds: a remap that is not a bijection inside a window failed
all 49 cases of test_batch_remap_isolation (unwritten rows), and a phased forward whose key mask lets one padded key through
(`<=` for `<`) failed every case with a ragged Skv that takes that kernel, by o (3 - 10 x the emulation) or, with several hundred keys,
by lse alone (28 - 160 x its limit)."""
import math
from ctypes import byref

import pytest
import torch

from tests import attention_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 32                       # guard rows (floats for lse / delta)
NAN16, NAN32 = 0x7FA5, 0x7FC5A5A5      # the guard pattern: a NaN in bf16 and in fp32
BF = torch.bfloat16

# kernel row_err <= FACTOR x emulation row_err, per input family.  Anything above 2 is justified in the module docstring; 4 is the ceiling.
FACTOR = {"randn": 2.0, "peaked": 2.0, "offset": 2.0, "late_max": 2.0, "first_max": 2.0, "const_keys": 2.0}


# ------------------------------------------------------------------------------------------------------------------ guarded buffers
class GBuf:
    """One bf16 allocation holding a [B, H, S, hd] tensor with guard rows.  row-major: row r of head h of sample b at
    (G + b (S + G) + r) ld + col0 + h hd;  head-major ("hm"): at (G + (b H + h) (S + G) + r) hd."""

    def __init__(self, B, H, S, hd, hm, ld=0, col0=0):
        if hm:
            self.ld, self.hs = hd, (S + G) * hd
            self.sb, self.off0, n = H * self.hs, G * hd, (2 * G + B * H * (S + G)) * hd
        else:
            self.ld, self.hs = ld, hd
            self.sb, self.off0, n = (S + G) * ld, G * ld + col0, (2 * G + B * (S + G)) * ld
        assert self.ld % 8 == 0 and self.hs % 8 == 0 and self.sb % 8 == 0 and self.off0 % 8 == 0
        self.hm = hm
        self.flat = torch.empty(n, device=DEV, dtype=BF)
        self.bits = self.flat.view(torch.int16)
        self.bits.fill_(NAN16)
        geom = ((B, H, S, hd), (self.sb, self.hs, self.ld, 1), self.off0)
        self.inner = self.flat.as_strided(*geom)
        self.outside = torch.ones(n, device=DEV, dtype=torch.bool)
        self.outside.as_strided(*geom).fill_(False)
        self.before = None

    def ptr(self, b=0, h=0):
        return self.flat.data_ptr() + 2 * (self.off0 + b * self.sb + h * self.hs)

    def head_stride(self):
        return self.hs if self.hm else 0         # 0 = the packed default (head h starts h * hd into the row)

    def snap(self):
        self.before = self.bits.clone()

    def untouched(self):
        return torch.equal(self.bits, self.before)

    def guards_intact(self):
        return torch.equal(self.bits[self.outside], self.before[self.outside])


class FBuf:
    """f32 [B, H, Sq] (lse, delta: compact, as the kernels index them) with G guard floats on each side."""

    def __init__(self, B, H, Sq):
        self.Sq, self.H = Sq, H
        self.flat = torch.empty(2 * G + B * H * Sq, device=DEV)
        self.bits = self.flat.view(torch.int32)
        self.bits.fill_(NAN32)
        self.inner = self.flat[G:G + B * H * Sq].view(B, H, Sq)
        self.outside = torch.ones_like(self.flat, dtype=torch.bool)
        self.outside[G:G + B * H * Sq] = False
        self.before = None

    def ptr(self, b=0, h=0):
        return self.flat.data_ptr() + 4 * (G + (b * self.H + h) * self.Sq)

    snap, untouched, guards_intact = GBuf.snap, GBuf.untouched, GBuf.guards_intact


class Problem:
    """q, k, v, dO ([B, H, S, hd] bf16 on the GPU) laid into guarded buffers, and guarded outputs on request.
    layout "packed": the row strides of the projection buffers -- self-attention (Sq == Skv) 3 hid for q, k, v and their gradients,
    cross-attention hid for q / dq and 2 hid for k, v / dk, dv; o and dO hid.  "hm": q, k, dq, dk head-major, the rest as before."""

    def __init__(self, hip, q, k, v, do, layout):
        self.hip, self.L, self.st = hip, hip.lib(), hip.stream_ptr()
        self.B, self.H, self.Sq, self.hd = q.shape
        self.Skv = k.shape[2]
        self.hm = layout == "hm"
        B, H, Sq, Skv, hd = self.B, self.H, self.Sq, self.Skv, self.hd
        self.hid = hid = H * hd
        if Sq == Skv:
            self.row = {"q": (3 * hid, 0), "k": (3 * hid, hid), "v": (3 * hid, 2 * hid)}
        else:
            self.row = {"q": (hid, 0), "k": (2 * hid, 0), "v": (2 * hid, hid)}
        self.q, self.k, self.v, self.do = self._buf("q"), self._buf("k"), self._buf("v"), GBuf(B, H, Sq, hd, False, hid, 0)
        for buf, x in ((self.q, q), (self.k, k), (self.v, v), (self.do, do)):
            buf.inner.copy_(x)
            buf.snap()
        self.scale = ar.scale_of(hd)

    def _buf(self, which):
        S = self.Sq if which == "q" else self.Skv
        if self.hm and which in "qk":
            return GBuf(self.B, self.H, S, self.hd, True)
        return GBuf(self.B, self.H, S, self.hd, False, *self.row[which])

    def inputs(self):
        return self.q, self.k, self.v, self.do

    def fwd_out(self):
        o, lse = GBuf(self.B, self.H, self.Sq, self.hd, False, self.hid, 0), FBuf(self.B, self.H, self.Sq)
        o.snap(), lse.snap()
        return {"o": o, "lse": lse}

    def bwd_out(self):
        out = {"dq": self._buf("q"), "dk": self._buf("k"), "dv": self._buf("v"), "delta": FBuf(self.B, self.H, self.Sq)}
        for b in out.values():
            b.snap()
        return out

    def args(self, f, g=None, bwd_split=0, bh=None):
        """md_attn_args for the whole batch, or (bh = (b, h)) for that one slice as a B = 1, H = 1 problem on the same strides."""
        b, h = bh if bh else (0, 0)
        B, H = (1, 1) if bh else (self.B, self.H)
        P = lambda buf: buf.ptr(b, h) if buf is not None else None
        g = g or {}
        dq, dk, dv, delta = g.get("dq"), g.get("dk"), g.get("dv"), g.get("delta")
        a = self.hip.AttnArgs(P(self.q), P(self.k), P(self.v), P(f["o"]), P(f.get("lse")), P(self.do),
                              P(dq), P(dk), P(dv), P(delta), B, H, self.Sq, self.Skv,
                              self.q.ld, self.k.ld, self.v.ld, f["o"].ld, self.q.sb, self.k.sb, self.v.sb, f["o"].sb,
                              dq.ld if dq else 0, dk.ld if dk else 0, dv.ld if dv else 0, self.do.ld,
                              dq.sb if dq else 0, dk.sb if dk else 0, dv.sb if dv else 0, self.do.sb,
                              self.scale, self.hd, bwd_split)
        a.hsq, a.hsk, a.hsv, a.hso = self.q.head_stride(), self.k.head_stride(), self.v.head_stride(), 0
        if dq:
            a.hsdq, a.hsdk, a.hsdv = dq.head_stride(), dk.head_stride(), dv.head_stride()
        return a

    def fwd(self, a):
        return self.L.md_attn_fwd(byref(a), self.st)

    def bwd(self, a):
        return self.L.md_attn_bwd(byref(a), self.st)

    def check_memory(self, what, written=(), idle=()):
        """The inputs and every buffer in `idle` bit-identical to their snapshot; the buffers in `written` finite inside, their guards
        bit-identical."""
        torch.cuda.synchronize()
        for name, buf in zip(("q", "k", "v", "dO"), self.inputs()):
            assert buf.untouched(), f"{what}: input {name} was written"
        for name, buf in idle:
            assert buf.untouched(), f"{what}: {name} was written"
        for name, buf in written:
            assert buf.guards_intact(), f"{what}: guard elements of {name} were written"
            assert bool(torch.isfinite(buf.inner).all()), f"{what}: {name} has non-finite or unwritten elements inside"


def streamed(Sq, Skv, bwd_split):
    """Did the streaming pair run (the only form that writes delta to memory)?"""
    return bwd_split == 5 or (bwd_split == 0 and max(Sq, Skv) > 256)


def fused_ok(Sq, Skv):
    return max(Sq, Skv) <= 256


def report(tag, name, kern, emu):
    """One line per figure, printed before it is asserted (pytest -s shows them)."""
    print(f"ATTN_EDGES | {tag} | {name} | kernel {kern:.3e} | yardstick {emu:.3e} | ratio {kern / emu if emu else float('nan'):.3f}")


def judge(tag, family, got, R, E, names, absolute=(), fp32_floor=0.0):
    """row_err of the kernel against the reference <= FACTOR x row_err of the emulation against the same reference.  Tensors named in
    `absolute` have a reference that is zero: the maximum absolute errors are compared instead."""
    bad = []
    for n in names:
        k_rel, k_abs = ar.row_err(got[n], getattr(R, n))
        e_rel, e_abs = ar.row_err(getattr(E, n), getattr(R, n))
        kern, emu = (k_abs, e_abs) if n in absolute else (k_rel, e_rel)
        report(f"{tag} {family}", n + ("(abs)" if n in absolute else ""), kern, emu)
        lim = FACTOR[family] * emu + (fp32_floor if n in absolute else 0.0)
        if not kern <= lim:
            bad.append(f"{n}: kernel {kern:.3e} > {FACTOR[family]} x emulation {emu:.3e}")
    assert not bad, f"{tag} {family}: " + "; ".join(bad)


def judge_lse(tag, lse, R):
    err, lim = (lse.double() - R.lse).abs(), ar.lse_limit(R)
    worst = (err / lim).max().item()
    report(tag, "lse(/limit)", worst, 1.0)
    assert worst <= 1.0, f"{tag}: lse off by {err.max().item():.3e}, {worst:.2f} x the limit"


def judge_delta(tag, delta, do, o_bf16):
    prod = do.double() * o_bf16.double()
    err, lim = (delta.double() - prod.sum(-1)).abs(), 1e-5 * prod.abs().sum(-1)
    worst = (err / lim.clamp(min=1e-300)).max().item()
    report(tag, "delta(/limit)", worst, 1.0)
    assert bool((err <= lim).all()), f"{tag}: delta off by {err.max().item():.3e}, {worst:.2f} x the limit"


def zero_grad_floor(x, o_bf16):
    """Allowance for gradients whose reference AND emulation are exactly zero (one key: P = 1, dP = delta exactly).  The kernels form
    dP and delta as two fp32 sums of the same hd products in different orders, so dS / scale = dP - delta is off by up to
    2 hd 2^-24 sum_d |dO O| per element; dq = scale dS k, dk = scale dS^T q (summed over the Sq queries)."""
    q, k, v, do = x
    eps = 2 * q.shape[-1] * 2.0 ** -24 * (do.double() * o_bf16.double()).abs().sum(-1).max().item()
    return eps * ar.scale_of(q.shape[-1]) * max(k.abs().max().item(), q.shape[-2] * q.abs().max().item())


def full_case(hip, tag, family, x, layout, splits, absolute=()):
    """Forward once, then every backward form of `splits` on fresh guarded outputs; memory, accuracy, lse and delta checks.
    Returns (problem, forward outputs, {split: backward outputs})."""
    q, k, v, do = x
    p = Problem(hip, q, k, v, do, layout)
    R, E = ar.reference(q, k, v, do, p.scale), ar.emulation(q, k, v, do, p.scale)
    f = p.fwd_out()
    hip.check(p.fwd(p.args(f)), "md_attn_fwd")
    p.check_memory(f"{tag} fwd", written=list(f.items()))
    judge(f"{tag} fwd", family, {"o": f["o"].inner}, R, E, ["o"])
    judge_lse(f"{tag} fwd {family}", f["lse"].inner, R)
    f["o"].snap(), f["lse"].snap()
    floor = zero_grad_floor(x, f["o"].inner) if p.Skv == 1 else 0.0
    outs = {}
    for split in splits:
        g = p.bwd_out()
        rc = p.bwd(p.args(f, g, split))
        what = f"{tag} bwd_split={split}"
        if split in (2, 3, 4) and not fused_ok(p.Sq, p.Skv):
            assert rc == -1, f"{what}: a forced fused form must refuse this problem (rc {rc})"
            p.check_memory(what, idle=list(f.items()) + list(g.items()))
            continue
        hip.check(rc, "md_attn_bwd")
        grads = [(n, g[n]) for n in ("dq", "dk", "dv")]
        p.check_memory(what, written=grads, idle=list(f.items()))
        assert g["delta"].guards_intact(), f"{what}: guard floats of delta were written"
        judge(what, family, {n: b.inner for n, b in grads}, R, E, ["dq", "dk", "dv"], absolute, floor)
        if streamed(p.Sq, p.Skv, split):
            judge_delta(f"{what} {family}", g["delta"].inner, do, f["o"].inner)
        outs[split] = g
    return p, f, outs


def inputs(family, B, H, Sq, Skv, hd, seed):
    return ar.make_inputs(family, B, H, Sq, Skv, hd, seed, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ 1. batch remap
REMAP_SHAPES = [(33, 77), (64, 64), (96, 40), (128, 128)]
REMAP_CASES = [(B, Sq, Skv, hd, layout) for B in (8, 9, 17) for Sq, Skv in REMAP_SHAPES for hd in (64, 32) for layout in ("packed", "hm")]
REMAP_CASES.append((9, 129, 128, 64, "packed"))     # two query blocks in the forward grid: the forward's remap is off, the backward's on


@pytest.mark.parametrize("B,Sq,Skv,hd,layout", REMAP_CASES)
def test_batch_remap_isolation(hip, B, Sq, Skv, hd, layout):
    """bh_of() re-deals (batch, head) to workgroups over whole windows of 8 samples when B >= 8 (8: no remainder; 9, 17: one sample in
    plain order behind one / two windows) -- in the forward when its grid has one query block, and in the fused backward kernels
    (bwd_split 2: single-phase, 3: two-phase, 4: two-phase with split dK / dV, 0: the library's pick among them).  Every sample has its
    own random values, so a workgroup that computes the wrong (b, h), or two that compute the same, cannot pass the accuracy check.
    Bitwise: every (b, h), launched alone as a B = 1, H = 1 problem on pointers offset to its slice, reproduces the batched o, lse, dq,
    dk, dv exactly (no atomics; the dispatch depends on Sq, Skv, hd only)."""
    H = 3
    x = inputs("randn", B, H, Sq, Skv, hd, seed=B + Sq + Skv + hd)
    tag = f"remap B={B} {Sq}x{Skv}x{hd} {layout}"
    p, f, outs = full_case(hip, tag, "randn", x, layout, (0, 2, 3, 4))
    f1 = p.fwd_out()
    g1 = {s: p.bwd_out() for s in outs}
    for b in range(B):
        for h in range(H):
            hip.check(p.fwd(p.args(f1, bh=(b, h))), "md_attn_fwd slice")
            for s in outs:
                hip.check(p.bwd(p.args(f, g1[s], s, bh=(b, h))), "md_attn_bwd slice")
    torch.cuda.synchronize()
    for n in ("o", "lse"):
        assert torch.equal(f1[n].bits, f[n].bits), f"{tag}: {n} differs from the slice-by-slice launches"
    for s in outs:
        for n in ("dq", "dk", "dv"):
            assert torch.equal(g1[s][n].bits, outs[s][n].bits), f"{tag} bwd_split={s}: {n} differs from the slice-by-slice launches"


# ------------------------------------------------------------------------------------------------------------------ 2. boundaries
# wave count 32 / 33, 128 / 129; fused buckets 64 / 65, 96 / 97; fused -> streaming 256 / 257; forward streaming (Sq >= 192 and
# Skv >= 257); stream_waves 5 -> 6 (150) and < 3 -> 3 (1, 33, 40); the 4-wave caps at Skv <= 128 (300 x 40 against 513 x 129) and
# Sq <= 128 (40 x 300 against 150 x 300); the phased forward with Skv > 256 (64 x 300, 40 x 300, 191 x 257)
BOUNDARY_SHAPES = [(1, 1), (1, 33), (33, 1), (31, 31), (32, 32), (33, 33), (64, 65), (65, 64), (96, 97), (97, 96), (128, 129), (129, 128),
                   (191, 257), (192, 256), (192, 257), (256, 257), (257, 256), (257, 257), (64, 300), (300, 40), (40, 300), (150, 300),
                   (300, 150), (220, 260), (513, 129)]
BOUNDARY_CASES = [(Sq, Skv, 64, "hm" if i % 2 else "packed") for i, (Sq, Skv) in enumerate(BOUNDARY_SHAPES)] + \
                 [(Sq, Skv, 32, "packed" if i % 2 else "hm") for i, (Sq, Skv) in enumerate(BOUNDARY_SHAPES) if i % 3 == 0]


@pytest.mark.parametrize("Sq,Skv,hd,layout", BOUNDARY_CASES)
def test_sequence_boundaries(hip, Sq, Skv, hd, layout):
    """Both sides of every size at which md_attn_fwd / md_attn_bwd pick another kernel, instantiation or workgroup size; the library's
    rule (0) and the streaming pair (5) everywhere, the forced fused forms where they cover the problem -- and where they do not, they
    must return -1 and write nothing, guard pattern included.  One key: dq and dk are exactly zero (see zero_grad_floor)."""
    x = inputs("randn", 2, 2, Sq, Skv, hd, seed=Sq * 1000 + Skv + hd)
    full_case(hip, f"boundary {Sq}x{Skv}x{hd} {layout}", "randn", x, layout, (0, 5, 2, 3, 4), absolute=("dq", "dk") if Skv == 1 else ())


# ------------------------------------------------------------------------------------------------------------------ 3. hard softmax
HARD_SHAPES = [(33, 77), (64, 257), (200, 200), (300, 150)]


@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("Sq,Skv", HARD_SHAPES)
@pytest.mark.parametrize("family", [f for f in ar.FAMILIES if f != "randn"])
def test_hard_softmax(hip, family, Sq, Skv, hd):
    """Logits far from zero: the online rescale exp2(m - m_new) with a large argument (late_max: the dominant key arrives in the last,
    ragged tile) or none (first_max), the log2-domain recomputation exp2(s c1 - l2) of the backward with |s| of 20 - 45 (peaked, offset),
    and the exact cases of const_keys: P uniform, lse = s + ln Skv, dq = 0 (judged by absolute error).  const_keys with V = 1: o must be
    exactly 1.0 -- any padded key that reaches the softmax takes mass from it -- and lse within its limit of s + ln Skv."""
    x = inputs(family, 2, 2, Sq, Skv, hd, seed=Sq + Skv + hd)
    tag = f"hard {Sq}x{Skv}x{hd}"
    splits = (0, 5, 2, 3) if fused_ok(Sq, Skv) else (0, 5)
    p, f, _ = full_case(hip, tag, family, x, "packed", splits, absolute=("dq",) if family == "const_keys" else ())
    if family == "const_keys":
        q, k, v, do = x
        p1 = Problem(hip, q, k, torch.ones_like(v), do, "hm")
        f1 = p1.fwd_out()
        hip.check(p1.fwd(p1.args(f1)), "md_attn_fwd")
        p1.check_memory(f"{tag} V=1", written=list(f1.items()))
        assert bool((f1["o"].inner == 1.0).all()), f"{tag}: o != 1.0 with V = 1 (a padded key leaked into the softmax, or l != sum p)"
        s = (q.double() * k[:, :, :1].double()).sum(-1) * p1.scale
        R = ar.reference(q, k, v, do, p1.scale)
        err = (f1["lse"].inner.double() - (s + math.log(Skv))).abs()
        assert bool((err <= ar.lse_limit(R)).all()), f"{tag}: lse - (s + ln Skv) = {err.max().item():.3e}"


# ------------------------------------------------------------------------------------------------------------------ 4. backward alone
@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("Sq,Skv", [(77, 77), (256, 77), (300, 150), (64, 300)])
def test_backward_from_reference_state(hip, Sq, Skv, family):
    """md_attn_bwd on o = bf16(reference o) and lse = fp32(reference lse) instead of the kernel's own forward output, so that a forward
    and a backward error that agree cannot cancel.  The emulation is given the same o and lse."""
    hd = 64
    x = inputs(family, 2, 2, Sq, Skv, hd, seed=Sq + 3 * Skv)
    q, k, v, do = x
    p = Problem(hip, q, k, v, do, "packed")
    R = ar.reference(q, k, v, do, p.scale)
    o_in, lse_in = R.o.to(BF), R.lse.float()
    E = ar.emulation(q, k, v, do, p.scale, o=o_in, lse=lse_in)
    f = p.fwd_out()
    f["o"].inner.copy_(o_in)
    f["lse"].inner.copy_(lse_in)
    f["o"].snap(), f["lse"].snap()
    for split in (0, 5):
        g = p.bwd_out()
        what = f"bwd-only {Sq}x{Skv}x{hd} bwd_split={split}"
        hip.check(p.bwd(p.args(f, g, split)), "md_attn_bwd")
        grads = [(n, g[n]) for n in ("dq", "dk", "dv")]
        p.check_memory(what, written=grads, idle=list(f.items()))
        assert g["delta"].guards_intact()
        judge(what, family, {n: b.inner for n, b in grads}, R, E, ["dq", "dk", "dv"])
        if streamed(Sq, Skv, split):
            judge_delta(f"{what} {family}", g["delta"].inner, do, o_in)


# ------------------------------------------------------------------------------------------------------------------ 5. lse = NULL
@pytest.mark.parametrize("Sq,Skv", [(64, 77), (300, 300)])
def test_forward_without_lse(hip, Sq, Skv):
    """lse is optional in the forward (the sampler does not keep it): the same o, bit for bit, and nothing else written."""
    x = inputs("randn", 2, 2, Sq, Skv, 64, seed=Sq + Skv)
    p = Problem(hip, *x, "packed")
    f, f0 = p.fwd_out(), p.fwd_out()
    hip.check(p.fwd(p.args(f)), "md_attn_fwd")
    hip.check(p.fwd(p.args({"o": f0["o"]})), "md_attn_fwd without lse")
    p.check_memory("lse = NULL", written=[("o", f0["o"])], idle=[("lse", f0["lse"])])
    assert torch.equal(f0["o"].bits, f["o"].bits)


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_bad_arguments_launch_nothing(hip):
    """Arguments the kernels cannot serve are refused with MD_BAD_ARG (-1) before anything is launched: every buffer stays bit-identical."""
    x = inputs("randn", 2, 2, 64, 77, 64, seed=1)
    p = Problem(hip, *x, "packed")
    f, g = p.fwd_out(), p.bwd_out()
    f["o"].inner.zero_()            # a plausible forward state for the backward calls (never read: nothing may launch)
    f["lse"].inner.zero_()
    f["o"].snap(), f["lse"].snap()

    cases = [("hd = 48", lambda a: setattr(a, "hd", 48), True), ("ldq % 8 != 0", lambda a: setattr(a, "ldq", a.ldq + 4), True),
             ("B = 0", lambda a: setattr(a, "B", 0), True), ("lse = NULL", lambda a: setattr(a, "lse", None), False),
             ("lddo % 8 != 0", lambda a: setattr(a, "lddo", a.lddo + 4), False)]
    cases += [(f"bwd_split = {s}", lambda a, s=s: setattr(a, "bwd_split", s), False) for s in (-1, 1, 6)]
    for name, mutate, fwd_too in cases:
        a = p.args(f, g)
        mutate(a)
        if fwd_too:
            assert p.fwd(a) == -1, f"md_attn_fwd accepted {name}"
        assert p.bwd(a) == -1, f"md_attn_bwd accepted {name}"
        p.check_memory(name, idle=list(f.items()) + list(g.items()))
