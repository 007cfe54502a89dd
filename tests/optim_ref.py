"""References, bounds, storage and case tables for the optimizer tail (pure torch, no GPU needed): md_sumsq / md_sumsq_finish,
md_step_guard, md_adamw_step[_ranges][_guarded], md_ema_power_update[_ranges] and md_checksum_u16.

Constants in fp32, arithmetic in fp64.  kernel_constants() forms, with torch.float32 scalar operations, every number adamw_kernel
forms in fp32 before its loop (in fp64 with a rounding to fp32 after every operation, see r32): decay = 1 - lr * wd, step_size = lr / bc1, inv_sqrt_bc2 = 1 / sqrt(bc2), 1 - b1, 1 - b2, 1 - es and
the clip chain nrm = sqrt(ss) * gs, coef = gs * min(1, max_norm / (nrm + 1e-6)).  Two of them are a product followed by a sum,
which a compiler may contract into one fused multiply-add; the hyperparameter sets are chosen so that both readings give the same
bits (grad_scale is a power of two; fused and unfused 1 - lr * wd are asserted equal), so every constant has ONE bit pattern.
The per-element arithmetic is fp64 on the fp32 / bf16 inputs.

Bounds, as counted roundings.  U = 2^-24 is the fp32 unit roundoff, g_k = k U / (1 - k U) the bound on the product of k factors
(1 + d), |d| <= U.  Every fp32 multiplication may also underflow: ETA = 2^-126 bounds that error whether the build keeps
denormals (then it is 2^-150) or flushes them; inputs are normal numbers or zero.  With gg = g * coef (one rounding, d1):
  m    fl(fl(b1 m0) + fl((1-b1) gg)): the first term carries 2 roundings (product, sum), the second 3 (d1, product, sum):
           |m - m_ref| <= g_2 |b1 m0| + g_3 |(1-b1) gg| + 4 ETA           (a fused multiply-add only removes roundings)
  v    fl(fl(b2 v0) + fl(fl((1-b2) gg) gg)): 2 roundings on the first term; on the second d1 twice, two products, the sum = 5:
           |v - v_ref| <= g_5 v_ref + av,   av = ETA (3 + 3 |gg|)         (both terms are >= 0, so g_5 covers the whole sum)
  den  sqrt(v) * isb + eps: sqrt halves the relative error of v (g_5 / 2 <= g_3), its own rounding, the product, the sum: g_6 on a
       sum of positive terms; the absolute term av enters through sqrt at worst as sqrt(av) (v_ref = 0):
           den = den_ref (1 + t),  |t| <= rel = g_6 + (isb sqrt(av) (1 + 2 U) + ETA) / den_ref
       Relative to eps: sqrt(av) <= 2^-61.7 for |gg| <= 1, times isb <= 32 is 9e-18, i.e. 9e-10 eps at eps = 1e-8, 1/70 of one U.
  p    q = fl(fl(step m) / den), p = fl(fl(p0 decay) - q).  With rho = (g_2 + rel) / (1 - rel) (two roundings over the perturbed
       denominator) and dm the bound on m:
           E = U |p0 decay| + |upd_ref| rho + step dm / den_ref (1 + rho) + ETA (2 + (1 + rho) / den_ref)
           |p - p_ref| <= E (1 + U) + U |p_ref|                            (the last subtraction rounds the perturbed value)
       i.e. U (|p0 decay| + |p_ref|) + step dm / den + 8 U |upd| to first order: g_2 + g_6 = 8 U (a count of 9 would charge the
       last subtraction to |upd| a second time; it is already in U |p_ref|).
       Where g = m0 = v0 = 0 the update is exactly 0 and p must be fl(p0 * decay) bit for bit (p0 itself when wd = 0).
  ema  mode 2: fl(fl(es e0) + fl((1-es) p)), 2 roundings per term (product, sum), p the kernel's own:
           |e - e_ref| <= g_2 (|es e0| + |(1-es) p_ref|) + (1-es) dp (1 + g_2) + 3 ETA
       mode 1: bit-equal to the kernel's p.  md_ema_power_update: the same two-term form per profile on an exact p:
           |e - e_ref| <= g_2 (|b e0| + |(1-b) p|) + 3 ETA;  beta == 0: bit-equal to p.
  shadow is compared bit for bit with the round-to-nearest-even bf16 of the kernel's own p; g after zero_grad is bit-zero; every
  element outside the ranges, every input and every fence is bit-identical to its initial value.

Reductions.  Exact cases: gradients from {0, +-0.5, +-1, +-2} (exact in bf16; the sum in units of 0.25 stays below 2^24, asserted)
and small-integer partials: fp32 summation is exact in any order, one bit pattern is right, the check is torch.equal.  General
inputs: |got - sum g^2| <= g_D sum g^2 with D the longest chain of roundings read from the kernel's geometry: one for the square,
8 additions per pass of a thread (262144 threads of 8 elements), 6 + 2 levels of the wave and block combines, and in
md_sumsq_finish ceil(count / 256) additions per thread plus the same 8 levels.

Storage (Buf): every buffer is the middle of a larger allocation filled with the sentinel NaNs of tests/gemm_exact.py; the fences
are compared bit for bit after every launch.  (gemm_exact.Fenced is not reused: it allows writes up to the next multiple of 8
columns, which would excuse exactly the 4-element overrun a float4 kernel can make at n = 4, 1020 and 1028.)

The emulators (adamw_emulate, ema_emulate, sumsq_emulate, finish_emulate, guard_emulate, checksum_ref) address the buffers as the
header says -- flat indices for p / g / m / v / ema, packed indices for g_bf16 and shadow -- in fp64, in fp32 in the kernel's
statement order, or in fp32 with the multiply-adds fused; `mut` breaks one thing at a time for the mutation tests.
contract_accepts() restates the argument rules of include/microdit_hip.h; REFUSALS is written from it.
"""
import dataclasses
import math
import zlib

import numpy as np
import torch

from tests.gemm_exact import SENT_BF16, SENT_F32

U = 2.0 ** -24
ETA = 2.0 ** -126
BAD_ARG = -1
SUMSQ_PARTIALS = 1024                      # MD_SUMSQ_PARTIALS: the fixed grid of md_sumsq, 256 threads each
SUMSQ_THREADS = SUMSQ_PARTIALS * 256
GRID_CAP = 8192                            # adamw_kernel / ema_power_kernel: workgroups of 256 float4
CHECKSUM_CAP = 2048                        # checksum_u16_kernel: workgroups of 256 8-word vectors
MAX_RANGES = 64                            # MD_ADAMW_MAX_RANGES
EMA_MAX = 4                                # MD_EMA_MAX_PROFILES
LEAD = 64                                  # fence elements on either side (a multiple of 8: the body keeps the allocation's alignment)
N_LARGE = 4 * (GRID_CAP * 256 + 37)        # a second grid-stride pass of 37 threads
SIZES = (4, 1020, 1024, 1028)


def gamma(k):
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------ storage
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64}
_SENT = {torch.float32: SENT_F32, torch.bfloat16: SENT_BF16, torch.int32: SENT_F32, torch.int64: 0x7FC0BEEF7FC0BEEF}


class Buf:
    """n elements inside a sentinel-filled allocation: LEAD fence elements before and after.  `values` None leaves the body sentinel
    (an output that must be overwritten).  The state at construction is frozen: fence_ok / untouched compare bits with it."""

    def __init__(self, n, dtype, device="cpu", values=None):
        self.n, self.dtype, self.lead = n, dtype, LEAD
        self.raw = torch.full((LEAD + n + LEAD,), _SENT[dtype], dtype=_BITS[dtype], device=device)
        if values is not None:
            self.body[:] = torch.as_tensor(values).to(device=device, dtype=dtype)
        self.frozen = self.raw.clone()

    @property
    def esize(self):
        return self.raw.element_size()

    @property
    def typed(self):
        return self.raw.view(self.dtype)

    @property
    def body(self):
        return self.typed[self.lead:self.lead + self.n]

    @property
    def bits(self):
        return self.raw[self.lead:self.lead + self.n]

    @property
    def init(self):
        return self.frozen.view(self.dtype)[self.lead:self.lead + self.n]

    @property
    def init_bits(self):
        return self.frozen[self.lead:self.lead + self.n]

    def ptr(self, extra=0):
        return self.raw.data_ptr() + (self.lead + extra) * self.esize

    def fence_ok(self):
        a, b = self.lead, self.lead + self.n
        return bool(torch.equal(self.raw[:a], self.frozen[:a]) and torch.equal(self.raw[b:], self.frozen[b:]))

    def untouched(self):
        return bool(torch.equal(self.raw, self.frozen))

    def restore(self):
        self.raw.copy_(self.frozen)

    # ---- the emulators' memory access: element index relative to the pointer a launch passes; an index outside the allocation (a
    # mutation's) is clamped for reads and dropped for writes
    def read(self, idx, dt):
        if isinstance(idx, slice):
            return self.body[idx].to(dt)
        j = (idx + self.lead).clamp(0, self.raw.numel() - 1)
        return self.typed[j].to(dt)

    def write(self, idx, vals):
        if isinstance(idx, slice):
            self.body[idx] = vals.to(self.dtype)
            return
        j = idx + self.lead
        ok = (j >= 0) & (j < self.raw.numel())
        self.typed[j[ok]] = vals.to(self.dtype)[ok]


def _fences(bufs):
    return [f"fence of {k} was written" for k, b in bufs.items() if not b.fence_ok()]


def _ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (fp64); a non-finite got counts as inf."""
    if got.numel() == 0:
        return 0.0
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, math.inf))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ hyperparameters
@dataclasses.dataclass(frozen=True)
class HP:
    lr: float
    wd: float
    b1: float
    b2: float
    eps: float
    step: int
    es: float
    gs: float
    max_norm: float
    live: bool                 # non-zero moments on entry

    @property
    def bc1(self):
        return 1 - self.b1 ** self.step

    @property
    def bc2(self):
        return 1 - self.b2 ** self.step


HPS = {
    # the production set: step 1 from zero moments, step 1000 with live moments
    "prod1": HP(2.4e-4, 0.1, 0.9, 0.999, 1e-8, 1, 0.99, 1.0, 0.25, False),
    "prod1000": HP(2.4e-4, 0.1, 0.9, 0.999, 1e-8, 1000, 0.99, 1.0, 0.25, True),
    # the loud set: every term moves the result by far more than the bound; all ten scalar fields of md_adamw_args pairwise distinct
    # (lr .0625, b1 .5, b2 .75, eps .00098, wd .25, bc1 .875, bc2 .578, max_norm 3, grad_scale .125, es .625)
    "loud": HP(2.0 ** -4, 0.25, 0.5, 0.75, 2.0 ** -10, 3, 0.625, 0.125, 3.0, True),
    # no weight decay: an element with g = m = v = 0 keeps its bits
    "nowd": HP(2.4e-4, 0.0, 0.9, 0.999, 1e-8, 1000, 0.99, 1.0, 0.25, True),
}


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def scalar_fields(hp):
    """The ten float fields of md_adamw_args as the fp32 numbers the struct holds."""
    return dict(lr=float(f32(hp.lr)), beta1=float(f32(hp.b1)), beta2=float(f32(hp.b2)), eps=float(f32(hp.eps)),
                weight_decay=float(f32(hp.wd)), bias_corr1=float(f32(hp.bc1)), bias_corr2=float(f32(hp.bc2)),
                max_norm=float(f32(hp.max_norm)), grad_scale=float(f32(hp.gs)), ema_smoothing=float(f32(hp.es)))


@dataclasses.dataclass
class Consts:
    coef: float
    decay: float
    step: float
    isb: float
    b1: float
    omb1: float
    b2: float
    omb2: float
    eps: float
    es: float
    omes: float


def r32(x):
    """Round a Python float (fp64) to fp32, returned as a Python float.  For one +, -, *, / or sqrt on fp32 operands, the fp64 result
    rounded to fp32 IS the correctly rounded fp32 result (53 >= 2 * 24 + 2 bits: the second rounding is innocuous), so the constants
    below never depend on how a machine's float32 library rounds."""
    return float(np.float32(x))


def kernel_constants(hp, ss=None, max_norm=None, mut=None):
    """Every fp32 number adamw_kernel forms before its loop, each a single correctly rounded fp32 operation on fp32 operands.
    ss: the value behind a->sumsq (None = NULL pointer)."""
    lr, wd, b1, b2, eps, es, gs = (r32(x) for x in (hp.lr, hp.wd, hp.b1, hp.b2, hp.eps, hp.es, hp.gs))
    mx = r32(hp.max_norm if max_norm is None else max_norm)
    coef = gs
    if ss is not None and mx > 0:
        root = r32(math.sqrt(r32(ss)))
        nrm = root if mut == "clip_unscaled_norm" else r32(root * gs)
        ratio = r32(mx / r32(nrm + r32(1e-6)))
        clip = ratio if mut == "min_dropped" else min(1.0, ratio)
        coef = clip if mut == "coef_missing_gs" else r32(gs * clip)
    decay = 1.0 if mut == "decay_dropped" else r32(1.0 - r32(lr * wd))
    if mut == "betas_swapped":
        b1, b2 = b2, b1
    omb2 = 0.001 if mut == "omb2_exact" else r32(1.0 - b2)
    return Consts(coef=coef, decay=decay, step=r32(lr / r32(hp.bc1)), isb=r32(1.0 / r32(math.sqrt(r32(hp.bc2)))),
                  b1=b1, omb1=r32(1.0 - b1), b2=b2, omb2=omb2, eps=eps, es=es, omes=r32(1.0 - es))


def decay_is_unambiguous(hp):
    """fl(1 - fl(lr wd)) == fl(1 - lr wd): the bits of `decay` do not depend on whether the compiler fuses the product into the sum."""
    lr, wd = r32(hp.lr), r32(hp.wd)
    return r32(1.0 - r32(lr * wd)) == r32(1.0 - lr * wd)


def clip_x(hp, ss):
    """fl(fl(fl(sqrt(ss)) * gs) + 1e-6): what the kernel compares with max_norm (grad_scale is a power of two: a fused form agrees)."""
    return r32(r32(r32(math.sqrt(r32(ss))) * r32(hp.gs)) + r32(1e-6))


def clip_edge_ss(hp, which):
    """An fp32 ss for which clip_x falls just below ('below'), exactly at ('at') or just above ('above') max_norm, found by walking
    the fp32 neighbours of ((max_norm - 1e-6) / gs)^2."""
    mx = r32(hp.max_norm)
    base = int(np.array([((hp.max_norm - 1e-6) / hp.gs) ** 2], dtype=np.float32).view(np.int32)[0])
    cand = [float(v) for v in np.arange(base - 400, base + 401, dtype=np.int32).view(np.float32)]
    x = [clip_x(hp, c) for c in cand]
    assert any(v == mx for v in x), "no fp32 ss puts nrm + 1e-6 exactly at max_norm"
    return {"below": max(c for c, v in zip(cand, x) if v < mx), "at": min(c for c, v in zip(cand, x) if v == mx),
            "above": min(c for c, v in zip(cand, x) if v > mx)}[which]


# ------------------------------------------------------------------------------------------------ range tables
def _r64():
    cyc = (4, 8, 60, 64, 68, 1028)
    off, cnt, at = [], [], 4
    for j in range(MAX_RANGES):
        off.append(at)
        cnt.append(cyc[j % len(cyc)])
        at += cnt[-1] + (4 if j % 2 else 0)            # alternately touching the next range and 4 elements apart
    order = list(range(MAX_RANGES - 2, -1, -2)) + list(range(1, MAX_RANGES, 2))      # even ranges descending, then odd ascending
    return [off[j] for j in order], [cnt[j] for j in order]


RANGE_TABLES = {                                       # name -> (flat_off, count), in the order the call passes them
    "r1": ([8], [60]),
    "r2-touch-desc": ([72, 8], [68, 64]),              # [8, 72) touches [72, 140); passed in descending flat order
    "r3-gap4-mixed": ([76, 0, 8], [68, 4, 64]),        # [0, 4) . [8, 72) . [76, 144): 4 elements apart, interleaved order
    "r64": _r64(),                                     # the full table: every count of {4, 8, 60, 64, 68, 1028}
    "rbig": ([96, 4], [4 * GRID_CAP * 256 + 64, 84]),  # packed total N_LARGE: the second pass holds 16 float4 of range 0, 21 of range 1
}
SMALL_TABLES = ("r1", "r2-touch-desc", "r3-gap4-mixed", "r64")
assert sum(RANGE_TABLES["rbig"][1]) == N_LARGE


def table_extent(off, cnt):
    return max(o + c for o, c in zip(off, cnt)) + 4    # 4 elements past the last range: inside the buffer, outside every range


def range_lookup(off, cnt, device="cpu", mut=None):
    """Flat element index of every packed element, through the search of range_flat4: the last range whose start <= the float4."""
    n = len(off)
    start = torch.tensor([0] + list(np.cumsum(cnt)[:-1]), dtype=torch.int64, device=device)
    flat = torch.tensor(off, dtype=torch.int64, device=device)
    e = torch.arange(0, sum(cnt), 4, dtype=torch.int64, device=device)
    if mut == "range_lt":
        lo = (torch.searchsorted(start, e, right=False) - 1).clamp(min=0)
    else:
        lo = torch.searchsorted(start, e, right=True) - 1
    if mut == "last_range_never" and n >= 2:
        lo = lo.clamp(max=n - 2)
    f4 = flat[lo] + (e - start[lo])
    return (f4[:, None] + torch.arange(4, dtype=torch.int64, device=device)[None]).reshape(-1)


def direct_index(off, cnt, device="cpu"):
    """The same map straight from the header: range j covers flat [off[j], off[j] + cnt[j]), packed back to back."""
    return torch.cat([torch.arange(o, o + c, dtype=torch.int64, device=device) for o, c in zip(off, cnt)])


# ------------------------------------------------------------------------------------------------ AdamW: cases
@dataclasses.dataclass(frozen=True)
class AdamCase:
    name: str
    n: int                     # flat form: elements; range form: ignored (the table decides)
    hp: str
    gbf16: bool
    ema_mode: int
    clip: str = "clipped"      # null | maxnorm0 | ss0 | below | at | above | clipped | unclipped
    zero_grad: bool = True
    shadow: bool = True
    guard: object = None       # None (the unguarded entry point), 0 or 1
    ranges: str = ""


def _form(gb, mode):
    return f"{'bf16' if gb else 'f32'}-ema{mode}"


def _adam_flat_cases():
    out = []
    for gb in (False, True):
        for mode in (0, 1, 2):
            for hp in ("prod1", "prod1000", "loud"):
                out.append(AdamCase(f"{_form(gb, mode)}-{hp}-n1028", 1028, hp, gb, mode))
    for n in SIZES[:3]:
        out.append(AdamCase(f"f32-ema2-loud-n{n}", n, "loud", False, 2))
        out.append(AdamCase(f"bf16-ema1-prod1000-n{n}", n, "prod1000", True, 1))
    for clip in ("null", "maxnorm0", "ss0", "below", "at", "above"):
        out.append(AdamCase(f"clip-{clip}-prod1000", 1028, "prod1000", False, 0, clip=clip))
    for clip in ("clipped", "unclipped", "null", "below", "at", "above"):
        out.append(AdamCase(f"clip-{clip}-loud", 1028, "loud", True, 2, clip=clip))           # grad_scale != 1
    out.append(AdamCase("nowd-keepgrad-noshadow", 1028, "nowd", False, 0, zero_grad=False, shadow=False))
    out.append(AdamCase("nowd-bf16-ema2", 1028, "nowd", True, 2))
    out.append(AdamCase("guard1-f32-ema2-loud", 1028, "loud", False, 2, guard=1))
    out.append(AdamCase("guard1-bf16-ema1-prod1000", 1020, "prod1000", True, 1, guard=1))
    return out


def _adam_range_cases():
    out = []
    for t in SMALL_TABLES:
        for mode in (0, 1, 2):
            hp = ("loud", "prod1000", "prod1")[(mode + len(t)) % 3]
            out.append(AdamCase(f"ranges-{t}-ema{mode}-{hp}", 0, hp, True, mode, zero_grad=False, ranges=t))
    out.append(AdamCase("ranges-r64-ema2-loud-guard1", 0, "loud", True, 2, zero_grad=False, ranges="r64", guard=1))
    out.append(AdamCase("ranges-r3-noshadow", 0, "loud", True, 0, zero_grad=False, shadow=False, ranges="r3-gap4-mixed"))
    return out


def _adam_guard0_cases():
    out = []
    for gb in (False, True):
        for mode in (0, 1, 2):
            out.append(AdamCase(f"guard0-{_form(gb, mode)}", 1028, "loud", gb, mode, guard=0))
    out.append(AdamCase("guard0-keepgrad-noshadow", 1020, "prod1000", False, 1, zero_grad=False, shadow=False, guard=0))
    for mode in (0, 1, 2):
        out.append(AdamCase(f"guard0-ranges-r64-ema{mode}", 0, "loud", True, mode, zero_grad=False, ranges="r64", guard=0))
    out.append(AdamCase("guard0-ranges-r3", 0, "prod1000", True, 1, zero_grad=False, ranges="r3-gap4-mixed", guard=0))
    return out


ADAM_FLAT = _adam_flat_cases()
ADAM_RANGES = _adam_range_cases()
ADAM_GUARD0 = _adam_guard0_cases()
# the three launches at the large size
ADAM_FLAT_LARGE = AdamCase("large-f32-ema2-prod1000", N_LARGE, "prod1000", False, 2)
ADAM_GUARD0_LARGE = AdamCase("large-guard0-f32-ema1", N_LARGE, "loud", False, 1, guard=0)
ADAM_RANGES_LARGE = AdamCase("large-ranges-rbig-ema0", 0, "prod1000", True, 0, zero_grad=False, ranges="rbig")
ADAM_ALL = ADAM_FLAT + ADAM_RANGES + ADAM_GUARD0 + [ADAM_FLAT_LARGE, ADAM_GUARD0_LARGE, ADAM_RANGES_LARGE]
assert len({c.name for c in ADAM_ALL}) == len(ADAM_ALL)
ADAM_BY_NAME = {c.name: c for c in ADAM_ALL}

# edge elements planted in every case: (g, m0, v0, p0); None keeps the drawn value.  "eps" stands for the case's own eps.
PLANTS = (
    (0.0, 0.0, 0.0, 1.5),          # g = m = v = 0: p' = fl(p * decay) exactly
    (0.0, 0.0, 0.0, -0.0),
    (-0.0, 0.0, 0.0, None),
    (1e-20, None, None, None),     # (1 - b2) * gg * gg underflows
    (-1e-12, None, None, None),
    (1e-6, 0.0, 0.0, None),
    (1e4, None, None, None),
    (-1e2, None, None, -0.0),
    (0.0, "half-eps", "eps^2", None),   # v about eps^2: sqrt(v) * isb and eps are of one size
)


def _seed(name):
    return zlib.crc32(name.encode())


class AdamProblem:
    """One case with its fenced storage.  call() is the launch as data; adamw_emulate / a real launch change the buffers in place;
    adamw_check compares them with the fp64 reference formed from the frozen initial state."""

    def __init__(self, case, device="cpu"):
        c = self.case = case
        self.hp = hp = HPS[c.hp]
        gen = torch.Generator().manual_seed(_seed(c.name))
        if c.ranges:
            self.off, self.cnt = RANGE_TABLES[c.ranges]
            self.tot, self.nflat = sum(self.cnt), table_extent(self.off, self.cnt)
        else:
            self.off = self.cnt = None
            self.tot = self.nflat = c.n
        nf, tot = self.nflat, self.tot

        def rn(n):
            return torch.randn(n, generator=gen, dtype=torch.float32)

        p = rn(nf) * 10.0 ** (torch.rand(nf, generator=gen) * 4 - 4)     # |p| from 1e-4 to 1: U |p| does not hide the small terms
        g = rn(nf)
        gb = rn(tot).to(torch.bfloat16)
        m = rn(nf) * 0.1 if hp.live else torch.zeros(nf)
        v = (rn(nf) * 0.1) ** 2 if hp.live else torch.zeros(nf)
        e = rn(nf)
        # plants: packed position k -> flat position
        if c.ranges and tot <= (1 << 20):
            fidx = direct_index(self.off, self.cnt)
            to_flat = lambda k: int(fidx[k])
        elif c.ranges:                                   # rbig: range 0 holds packed [0, cnt0), range 1 the rest
            to_flat = lambda k: self.off[0] + k if k < self.cnt[0] else self.off[1] + k - self.cnt[0]
        else:
            to_flat = lambda k: k
        spots = [(7 * j + 1) % tot for j in range(len(PLANTS))] if tot >= 64 else [j % tot for j in range(len(PLANTS))]
        if tot >= 64:
            spots[-1], spots[-2] = tot - 1, tot - 4      # the last element and the first of the last float4
        for k, (pg, pm, pv, pp) in zip(spots, PLANTS):
            i = to_flat(k)
            if pg is not None:
                g[i] = pg
                gb[k] = pg
            if pm is not None:
                m[i] = 0.5 * hp.eps if pm == "half-eps" else pm
            if pv is not None:
                v[i] = hp.eps ** 2 if pv == "eps^2" else pv
            if pp is not None:
                p[i] = pp
        for t in (p, g, m, v, e, gb.float()):
            a = t.abs()
            assert bool(((a == 0) | (a >= 2.0 ** -100)).all()), "inputs are normal numbers or zero"
        self.gsrc = gb.float() if c.gbf16 else None
        B = self.bufs = {}
        B["p"], B["g"], B["m"], B["v"] = (Buf(nf, torch.float32, device, x) for x in (p, g, m, v))
        B["gb"] = Buf(tot, torch.bfloat16, device, gb)
        B["ema"] = Buf(nf, torch.float32, device, None if c.ema_mode == 1 else e)      # mode 1 must overwrite a NaN-filled buffer
        B["shadow"] = Buf(tot, torch.bfloat16, device, None)
        # the clip scalar
        gsum = float(((gb.double() if c.gbf16 else (g[fidx] if c.ranges and tot <= (1 << 20) else g).double()) ** 2).sum())
        if c.clip in ("below", "at", "above"):
            ss = clip_edge_ss(hp, c.clip)
        else:
            ss = {"clipped": gsum, "unclipped": 1e-4, "ss0": 0.0, "maxnorm0": gsum, "null": gsum}[c.clip]
        self.max_norm = 0.0 if c.clip == "maxnorm0" else hp.max_norm
        B["ss"] = Buf(1, torch.float32, device, [ss])
        self.ss = None if c.clip == "null" else float(f32(ss))
        if c.clip == "clipped":
            assert math.sqrt(self.ss) * hp.gs > 2 * hp.max_norm or tot < 64, (c.name, self.ss)
        if c.clip == "unclipped":
            assert math.sqrt(self.ss) * hp.gs < 0.5 * hp.max_norm
        B["guard"] = Buf(4, torch.int32, device, [0 if c.guard is None else c.guard, 5, 6, 7])
        self.device = device

    def call(self):
        c, B = self.case, self.bufs
        d = dict(entry="adamw_ranges" if c.ranges else "adamw", p=B["p"].ptr(), g=B["g"].ptr(), m=B["m"].ptr(), v=B["v"].ptr(),
                 shadow=B["shadow"].ptr() if c.shadow else None, sumsq=None if c.clip == "null" else B["ss"].ptr(),
                 g_bf16=B["gb"].ptr() if c.gbf16 else None, ema=B["ema"].ptr(),
                 n=12 if c.ranges else self.tot,                       # the range form ignores a->n
                 zero_grad=int(c.zero_grad), ema_mode=c.ema_mode, guard=None if c.guard is None else B["guard"].ptr(),
                 guarded=c.guard is not None)
        d.update(scalar_fields(self.hp))
        d["max_norm"] = float(f32(self.max_norm))
        if c.ranges:
            d.update(flat_off=list(self.off), count=list(self.cnt), n_ranges=len(self.off))
        return d

    def restore(self):
        for b in self.bufs.values():
            b.restore()

    def snapshot(self):
        return {k: b.raw.clone() for k, b in self.bufs.items()}


# ------------------------------------------------------------------------------------------------ AdamW: the model
def _sqrt(x):
    """sqrt in the dtype of x, correctly rounded: through fp64 for fp32 (r32 says why that is exact)."""
    return torch.sqrt(x.double()).to(x.dtype)


def _div(a, b):
    return (a.double() / b.double()).to(a.dtype)


def _fma(arith):
    """a * x + y as the three arithmetics see it (a: Python float holding an fp32 constant, or a tensor)."""
    if arith == "f32fma":
        def fma(a, x, y):
            a = a.double() if torch.is_tensor(a) else a
            return (a * x.double() + y.double()).float()           # exact product, one rounding
        return fma
    return lambda a, x, y: a * x + y


def adamw_emulate(P, arith="f64", mut=None):
    """md_adamw_step[_ranges][_guarded] on the buffers of P, in place.  arith: 'f64' (the model), 'f32' (the kernel's statements,
    multiply and add separate), 'f32fma' (multiply-adds fused)."""
    c, B, hp = P.case, P.bufs, P.hp
    dt = torch.float64 if arith == "f64" else torch.float32
    fma = _fma(arith)
    dev = B["p"].raw.device
    tot = P.tot
    fl_all = range_lookup(P.off, P.cnt, dev, mut) if c.ranges else None
    first = min(tot // 4, GRID_CAP * 256) * 4               # elements of the first grid-stride pass
    segs = [(0, tot)]
    if mut == "second_pass_dropped":
        segs = [(0, first)]
    elif mut == "second_pass_twice":
        segs = [(0, tot), (first, tot)]
    k = kernel_constants(hp, P.ss, P.max_norm, mut)
    guard = None if c.guard is None else int(B["guard"].body[0])
    for (a, b) in segs:
        if a >= b:
            continue
        pk = slice(a, b)
        fl = fl_all[a:b] if c.ranges else pk
        sh_idx = fl if (mut == "shadow_flat_index" and c.ranges) else pk
        p0 = B["p"].read(fl, dt)
        if guard == 0:
            if mut == "guard0_updates_m":
                g = B["gb"].read(pk, dt) if c.gbf16 else B["g"].read(fl, dt)
                B["m"].write(fl, fma(k.b1, B["m"].read(fl, dt), k.omb1 * (g * k.coef)))
            if c.ema_mode == 1:
                B["ema"].write(fl, p0)
            if c.shadow and mut != "guard0_no_shadow":
                B["shadow"].write(sh_idx, p0.float().to(torch.bfloat16))
            if c.zero_grad and mut != "guard0_no_zero_g":
                B["g"].write(fl, torch.zeros_like(p0))
            continue
        if c.gbf16:
            g = B["gb"].read(fl if (mut == "g_flat_index" and c.ranges) else pk, dt)
        else:
            g = B["g"].read(fl, dt)
        m0, v0 = B["m"].read(fl, dt), B["v"].read(fl, dt)
        gg = g * k.coef
        m = fma(k.b1, m0, k.omb1 * gg)
        v = fma(k.b2, v0, (k.omb2 * gg) * gg)
        if mut == "eps_in_sqrt":
            den = _sqrt(v + k.eps) * k.isb
        elif mut == "bc2_on_v":
            den = fma(k.isb * k.isb, _sqrt(v), torch.full_like(v, k.eps))
        else:
            den = fma(k.isb, _sqrt(v), torch.full_like(v, k.eps))
        if mut == "decay_after":
            p = (p0 - _div(k.step * m, den)) * k.decay
        else:
            p = p0 * k.decay - _div(k.step * m, den)
        p32 = p.float()                                     # what the kernel stores, and what shadow and the EMA are formed from
        B["p"].write(fl, p32)
        B["m"].write(fl, m)
        B["v"].write(fl, v)
        src = p0 if mut == "ema_pre_update" else p32.to(dt)
        if c.ema_mode == 1 and mut != "ema1_blend":
            B["ema"].write(fl, src)
        elif c.ema_mode:
            e0 = B["ema"].read(fl, dt)
            B["ema"].write(fl, fma(k.es, e0, k.omes * src))
        if c.zero_grad:
            B["g"].write(fl, torch.zeros_like(p32))
        if c.shadow:
            B["shadow"].write(sh_idx, (p0.float() if mut == "shadow_old_p" else p32).to(torch.bfloat16))


def adamw_check(P):
    """(problems, ratios, old_rule_ok): every violated property of the buffers of P against the fp64 reference formed from their
    frozen initial state; worst error / bound per array; whether p alone passes the old rule (rtol 1e-5, atol 1e-6)."""
    c, B, hp = P.case, P.bufs, P.hp
    dev = B["p"].raw.device
    out, ratios = _fences(B), {}
    for name in ("gb", "ss", "guard"):
        if not B[name].untouched():
            out.append(f"input {name} was written")
    if c.ranges:
        fl = direct_index(P.off, P.cnt, dev)
        outside = torch.ones(P.nflat, dtype=torch.bool, device=dev)
        outside[fl] = False
    else:
        fl, outside = slice(0, P.tot), None

    def same(name, what="must stay bit-identical"):
        if not torch.equal(B[name].bits, B[name].init_bits):
            out.append(f"{name} {what}: {int((B[name].bits != B[name].init_bits).sum())} elements changed")

    if outside is not None:
        for name in ("p", "g", "m", "v", "ema"):
            if not torch.equal(B[name].bits[outside], B[name].init_bits[outside]):
                out.append(f"{name}: elements outside the ranges were written")
    pgot = B["p"].body[fl]
    # ---- what does not depend on the arithmetic
    if c.shadow:
        if not torch.equal(B["shadow"].body.view(torch.int16), pgot.to(torch.bfloat16).view(torch.int16)):
            out.append("shadow is not the round-to-nearest-even bf16 of p at the packed index")
    else:
        same("shadow")
    if c.zero_grad:
        if int((B["g"].bits[fl] != 0).sum()):
            out.append("g is not bit-zero after zero_grad")
    else:
        same("g")
    if c.ema_mode == 0:
        same("ema")
    elif c.ema_mode == 1:
        if not torch.equal(B["ema"].bits[fl], B["p"].bits[fl]):
            out.append("ema (mode 1) is not a bit copy of the updated p")
    old_ok = True
    if c.guard == 0:
        same("p", "must stay bit-identical on a skipped step")
        same("m", "must stay bit-identical on a skipped step")
        same("v", "must stay bit-identical on a skipped step")
        if c.ema_mode == 2:
            same("ema", "must stay bit-identical on a skipped step")
        return out, ratios, old_ok
    # ---- the fp64 reference and the bounds
    k = kernel_constants(hp, P.ss, P.max_norm)
    d = lambda name: B[name].init[fl].double()
    p0, m0, v0 = d("p"), d("m"), d("v")
    g = B["gb"].init.double() if c.gbf16 else d("g")
    gg = g * k.coef
    t1, t2 = k.b1 * m0, k.omb1 * gg
    m_ref, dm = t1 + t2, gamma(2) * t1.abs() + gamma(3) * t2.abs() + 4 * ETA
    v_ref = k.b2 * v0 + k.omb2 * gg * gg
    av = ETA * (3 + 3 * gg.abs())
    dv = gamma(5) * v_ref + av
    den = v_ref.sqrt() * k.isb + k.eps
    rel = gamma(6) + (k.isb * av.sqrt() * (1 + 2 * U) + ETA) / den
    rho = (gamma(2) + rel) / (1 - rel)
    upd = k.step * m_ref / den
    pd = p0 * k.decay
    p_ref = pd - upd
    E = U * pd.abs() + upd.abs() * rho + k.step * dm / den * (1 + rho) + ETA * (2 + (1 + rho) / den)
    dp = E * (1 + U) + U * p_ref.abs()
    ratios["m"] = _ratio(B["m"].body[fl], m_ref, dm)
    ratios["v"] = _ratio(B["v"].body[fl], v_ref, dv)
    ratios["p"] = _ratio(pgot, p_ref, dp)
    if c.ema_mode == 2:
        e0 = d("ema")
        e_ref = k.es * e0 + k.omes * p_ref
        de = gamma(2) * ((k.es * e0).abs() + (k.omes * p_ref).abs()) + k.omes * dp * (1 + gamma(2)) + 3 * ETA
        ratios["ema"] = _ratio(B["ema"].body[fl], e_ref, de)
    for name, r in ratios.items():
        if not r <= 1.0:
            out.append(f"{name}: worst error / bound = {r:.3g}")
    # g = m = v = 0: the update is exactly zero, p' = fl(p * decay) and the moments stay +0
    z = (g == 0) & (m0 == 0) & (v0 == 0)
    if bool(z.any()):
        want = (B["p"].init[fl][z] * torch.tensor(k.decay, dtype=torch.float32, device=dev))
        if not torch.equal(pgot[z].view(torch.int32), want.view(torch.int32)):
            out.append("an element with g = m = v = 0 is not fl(p * decay) bit for bit")
        if int((B["m"].bits[fl][z] != 0).sum()) or int((B["v"].bits[fl][z] != 0).sum()):
            out.append("an element with g = m = v = 0 has a non-zero moment")
    old_ok = bool(torch.allclose(pgot, p_ref.float(), rtol=1e-5, atol=1e-6))
    return out, ratios, old_ok


# ------------------------------------------------------------------------------------------------ EMA power
@dataclasses.dataclass(frozen=True)
class EmaCase:
    name: str
    n: int
    betas: tuple
    guard: object = None
    ranges: str = ""


_BETAS = {1: (0.9375,), 2: (0.999, 0.0), 3: (0.0, 0.5, 0.99999), 4: (0.7, 0.0, 0.9999, 0.015625)}


def _ema_cases():
    out = [EmaCase("K1-beta0-n1028", 1028, (0.0,))]
    for j, n in enumerate(SIZES):
        for K in (1, 2, 3, 4):
            out.append(EmaCase(f"K{K}-n{n}", n, _BETAS[K], guard=(None, 1)[(j + K) % 2]))
    for j, t in enumerate(SMALL_TABLES):
        for K in (1, 2, 3, 4):
            out.append(EmaCase(f"K{K}-ranges-{t}", 0, _BETAS[K], guard=(None, 1)[(j + K) % 2], ranges=t))
    for K in (1, 2, 3, 4):
        out.append(EmaCase(f"K{K}-guard0", 1028, _BETAS[K], guard=0))
    out.append(EmaCase("K3-guard0-ranges-r64", 0, _BETAS[3], guard=0, ranges="r64"))
    return out


EMA_CASES = _ema_cases()
EMA_LARGE = EmaCase("large-K3", N_LARGE, _BETAS[3])
EMA_BY_NAME = {c.name: c for c in EMA_CASES + [EMA_LARGE]}


class EmaProblem:
    def __init__(self, case, device="cpu"):
        c = self.case = case
        gen = torch.Generator().manual_seed(_seed("ema-" + c.name))
        if c.ranges:
            self.off, self.cnt = RANGE_TABLES[c.ranges]
            self.tot, self.nflat = sum(self.cnt), table_extent(self.off, self.cnt)
        else:
            self.off = self.cnt = None
            self.tot = self.nflat = c.n
        nf = self.nflat
        p = torch.randn(nf, generator=gen) * 10.0 ** (torch.rand(nf, generator=gen) * 4 - 4)
        p[0], p[nf - 1 if not c.ranges else 0] = -0.0, -0.0
        B = self.bufs = {"p": Buf(nf, torch.float32, device, p)}
        for j, b in enumerate(c.betas):
            # a profile with beta == 0 starts NaN-filled (unless the step is skipped and it must stay as it is: then random as well)
            vals = None if b == 0.0 else torch.randn(nf, generator=gen)
            B[f"e{j}"] = Buf(nf, torch.float32, device, vals)
        B["guard"] = Buf(4, torch.int32, device, [0 if c.guard is None else c.guard, 5, 6, 7])

    def call(self):
        c, B = self.case, self.bufs
        d = dict(entry="ema_ranges" if c.ranges else "ema", p=B["p"].ptr(), ema=[B[f"e{j}"].ptr() for j in range(len(c.betas))],
                 beta=[float(f32(b)) for b in c.betas], n_profiles=len(c.betas), n=self.tot,
                 guard=None if c.guard is None else B["guard"].ptr())
        if c.ranges:
            d.update(flat_off=list(self.off), count=list(self.cnt), n_ranges=len(self.off))
        return d

    def restore(self):
        for b in self.bufs.values():
            b.restore()

    def snapshot(self):
        return {k: b.raw.clone() for k, b in self.bufs.items()}


def ema_emulate(P, arith="f64", mut=None):
    c, B = P.case, P.bufs
    if c.guard == 0:
        return
    dt = torch.float64 if arith == "f64" else torch.float32
    fma = _fma(arith)
    dev = B["p"].raw.device
    fl = range_lookup(P.off, P.cnt, dev, mut) if c.ranges else slice(0, P.tot)
    if mut == "second_pass_dropped":
        first = min(P.tot // 4, GRID_CAP * 256) * 4
        fl = fl[:first] if c.ranges else slice(0, first)
    p = B["p"].read(fl, dt)
    for j, b in enumerate(c.betas):
        b = float(f32(b))
        if b == 0.0 and mut != "beta0_reads":
            B[f"e{j}"].write(fl, p)
        else:
            B[f"e{j}"].write(fl, fma(b, B[f"e{j}"].read(fl, dt), r32(1.0 - r32(b)) * p))


def ema_check(P):
    c, B = P.case, P.bufs
    dev = B["p"].raw.device
    out, ratios = _fences(B), {}
    for name in ("p", "guard"):
        if not B[name].untouched():
            out.append(f"input {name} was written")
    if c.ranges:
        fl = direct_index(P.off, P.cnt, dev)
        outside = torch.ones(P.nflat, dtype=torch.bool, device=dev)
        outside[fl] = False
    else:
        fl, outside = slice(0, P.tot), None
    p = B["p"].init[fl].double()
    for j, b in enumerate(c.betas):
        e = B[f"e{j}"]
        if c.guard == 0:
            if not e.untouched():
                out.append(f"profile {j} was written on a skipped step")
            continue
        if outside is not None and not torch.equal(e.bits[outside], e.init_bits[outside]):
            out.append(f"profile {j}: elements outside the ranges were written")
        b = float(f32(b))
        if b == 0.0:
            if not torch.equal(e.bits[fl], B["p"].init_bits[fl]):
                out.append(f"profile {j} (beta == 0) is not a bit copy of p")
            continue
        t1, t2 = b * e.init[fl].double(), r32(1.0 - r32(b)) * p
        ratios[f"e{j}"] = _ratio(e.body[fl], t1 + t2, gamma(2) * (t1.abs() + t2.abs()) + 3 * ETA)
        if not ratios[f"e{j}"] <= 1.0:
            out.append(f"profile {j}: worst error / bound = {ratios[f'e{j}']:.3g}")
    return out, ratios


# ------------------------------------------------------------------------------------------------ reductions
@dataclasses.dataclass(frozen=True)
class SumsqCase:
    name: str
    n: int
    bf16: bool
    data: str                  # exact | single:<position> | randn | wide | nan-tail | inf0 | neginf | overflow | finite


N_SUMSQ_2PASS = 8 * (SUMSQ_THREADS + 37)
SUMSQ_SIZES = (8, 8 * 255, 8 * 256, 8 * 257, 8 * SUMSQ_THREADS, N_SUMSQ_2PASS)


def single_positions(n=N_SUMSQ_2PASS):
    """One non-zero element at: the first and the last element, both sides of an 8-element (thread), a 256-thread (workgroup) and a
    262144-thread (pass) boundary, the first and the last element of the ragged second pass."""
    return sorted({0, n - 1, 7, 8, 8 * 256 - 1, 8 * 256, 8 * SUMSQ_THREADS - 1, 8 * SUMSQ_THREADS})


def _sumsq_cases():
    out = []
    for bf in (False, True):
        t = "bf16" if bf else "f32"
        for n in SUMSQ_SIZES:
            out.append(SumsqCase(f"{t}-exact-n{n}", n, bf, "exact"))
        for pos in single_positions():
            out.append(SumsqCase(f"{t}-single-{pos}", N_SUMSQ_2PASS, bf, f"single:{pos}"))
        for n in (8 * 257, N_SUMSQ_2PASS):
            out.append(SumsqCase(f"{t}-randn-n{n}", n, bf, "randn"))
            out.append(SumsqCase(f"{t}-wide-n{n}", n, bf, "wide"))
    return out


SUMSQ_CASES = _sumsq_cases()
NONFINITE_CASES = [
    SumsqCase("f32-nan-tail", N_SUMSQ_2PASS, False, "nan-tail"), SumsqCase("bf16-nan-tail", N_SUMSQ_2PASS, True, "nan-tail"),
    SumsqCase("f32-inf0", N_SUMSQ_2PASS, False, "inf0"), SumsqCase("bf16-neginf", N_SUMSQ_2PASS, True, "neginf"),
    SumsqCase("f32-overflow", N_SUMSQ_2PASS, False, "overflow"), SumsqCase("bf16-overflow", 8 * 257, True, "overflow"),
    SumsqCase("f32-finite", 8 * 257, False, "finite"), SumsqCase("bf16-finite", 8, True, "finite"),
]
SUMSQ_BY_NAME = {c.name: c for c in SUMSQ_CASES + NONFINITE_CASES}
SLOTS, SLOT = 3, 1             # the partials buffer holds three calls' worth; the call under test owns the middle one


def sumsq_depth(n, count=SUMSQ_PARTIALS):
    """The longest chain of roundings between an element and out[0]: the square, 8 additions per pass of a thread, the wave (6) and
    block (2) combines, then in md_sumsq_finish ceil(count / 256) additions and the same 8 levels."""
    passes = -(-(n // 8) // SUMSQ_THREADS)
    return 1 + 8 * passes + 8 + -(-count // 256) + 8


class SumsqProblem:
    """md_sumsq into slot SLOT of a sentinel-filled partials buffer, md_sumsq_finish over that slot, md_step_guard on the result."""

    def __init__(self, case, device="cpu"):
        c = self.case = case
        gen = torch.Generator().manual_seed(_seed("sumsq-" + c.name))
        n, kind = c.n, c.data.split(":")[0]
        if kind in ("exact", "finite"):
            ch = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
            g = ch[torch.randint(0, 7, (n,), generator=gen)]
        elif kind == "single":
            g = torch.zeros(n)
            g[int(c.data.split(":")[1])] = -2.0
        elif kind == "randn":
            g = torch.randn(n, generator=gen)
        elif kind == "wide":                           # 24 decades; every square is a normal number and the sum stays finite
            g = torch.randn(n, generator=gen).sign() * 10.0 ** (torch.rand(n, generator=gen) * 24 - 12)
        else:
            g = torch.randn(n, generator=gen)
            if kind == "nan-tail":
                g[n - 3] = math.nan
            elif kind == "inf0":
                g[0] = math.inf
            elif kind == "neginf":
                g[n // 2 + 1] = -math.inf
            elif kind == "overflow":                   # finite elements, finite squares (2.25e38 < FLT_MAX), an infinite sum
                g[5], g[n - 9], g[n // 2] = 1.5e19, -1.5e19, 1.5e19
        dtype = torch.bfloat16 if c.bf16 else torch.float32
        g = g.to(dtype)
        self.kind = kind
        self.exact = kind in ("exact", "single", "finite")
        self.sum64 = float((g.double() ** 2).sum())
        if self.exact:
            assert self.sum64 * 4 < 2 ** 24, "the sum in units of 0.25 must stay below 2^24"
        if kind in ("randn", "wide"):
            sq = g.double() ** 2
            assert self.sum64 < 1e38 and bool(((sq == 0) | (sq >= 2.0 ** -100)).all())
        if kind == "overflow":
            assert bool(torch.isfinite(g.float()).all()) and bool(torch.isfinite(g.float() * g.float()).all()) and self.sum64 > 3.5e38
        B = self.bufs = {"g": Buf(n, dtype, device, g)}
        B["partials"] = Buf(SLOTS * SUMSQ_PARTIALS, torch.float32, device, None)
        B["out"] = Buf(1, torch.float32, device, None)
        B["state"] = Buf(4, torch.int32, device, [7, 5, 6, 7])

    def restore(self):
        for b in self.bufs.values():
            b.restore()

    def snapshot(self):
        return {k: b.raw.clone() for k, b in self.bufs.items()}


def _tree256(t):
    """[.., 256] -> [..]: the fixed combine of a workgroup: adjacent pairs, 6 levels inside a wave and 2 across the four waves."""
    for _ in range(8):
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def sumsq_emulate(P, arith="f64", mut=None):
    """md_sumsq of P.bufs['g'] into slot SLOT: vector i (8 elements) belongs to thread i % 262144, i.e. workgroup (i % 262144) // 256."""
    c, B = P.case, P.bufs
    g = B["g"].body
    n8 = c.n // 8
    if mut == "skip_last_vector":
        n8 -= 1
    passes = max(-(-n8 // SUMSQ_THREADS), 1)
    dt = torch.float64 if arith == "f64" else torch.float32
    sq = torch.zeros(passes * SUMSQ_THREADS * 8, dtype=dt, device=g.device)
    x = g[:n8 * 8].to(dt)
    sq[:n8 * 8] = x * x
    sq = sq.view(passes, SUMSQ_THREADS, 8)
    if arith == "f64":
        part = sq.sum((0, 2)).view(SUMSQ_PARTIALS, 256).sum(1).float()
    else:
        s = torch.zeros(SUMSQ_THREADS, dtype=dt, device=g.device)
        for ps in range(passes):
            if c.bf16:                                 # s += v[e] * v[e], element by element
                for e in range(8):
                    s = s + sq[ps, :, e]
            else:                                      # s += a.x * a.x + ... + b.w * b.w
                t = sq[ps, :, 0]
                for e in range(1, 8):
                    t = t + sq[ps, :, e]
                s = s + t
        part = _tree256(s.view(SUMSQ_PARTIALS, 256))
    slot = B["partials"].body[SLOT * SUMSQ_PARTIALS:(SLOT + 1) * SUMSQ_PARTIALS]
    if mut == "idle_wg_no_write":
        busy = min(-(-n8 // 256), SUMSQ_PARTIALS)
        slot[:busy] = part[:busy]
    else:
        slot[:] = part


def finish_emulate(partials, count, out, arith="f64", mut=None):
    """md_sumsq_finish: thread t adds partials t, t + 256, ...; the 256 sums go through the workgroup's fixed combine."""
    x = partials[:count]
    if mut == "drop_past_256" and count > 256:
        x = x[:count // 256 * 256]
    if arith == "f64":
        out[0] = x.double().sum().float()
        return
    rows = -(-x.numel() // 256)
    pad = torch.zeros(rows * 256, dtype=torch.float32, device=x.device)
    pad[:x.numel()] = x
    s = torch.zeros(256, dtype=torch.float32, device=x.device)
    for r in pad.view(rows, 256):
        s = s + r
    out[0] = _tree256(s)


def guard_emulate(sumsq, state):
    """md_step_guard: state[0] = isfinite(*sumsq), state[1] += 1 when it is not; state[2], state[3] reserved (untouched)."""
    ok = bool(torch.isfinite(sumsq[0]))
    state[0] = 1 if ok else 0
    if not ok:
        state[1] += 1


def sumsq_pipeline_emulate(P, arith="f64", mut=None):
    B = P.bufs
    sumsq_emulate(P, arith, mut)
    finish_emulate(B["partials"].body[SLOT * SUMSQ_PARTIALS:], SUMSQ_PARTIALS, B["out"].body, arith)
    guard_emulate(B["out"].body, B["state"].body)


def sumsq_check(P):
    """(problems, ratio): md_sumsq wrote all 1024 partials of its slot and nothing else; the result is exact (exact cases), within
    g_D sum g^2 (general inputs), NaN / +Inf (non-finite cases); md_step_guard's flag and counter follow."""
    c, B = P.case, P.bufs
    out, ratio = _fences(B), None
    if not B["g"].untouched():
        out.append("the gradient was written")
    pb, pi = B["partials"].bits, B["partials"].init_bits
    a, b = SLOT * SUMSQ_PARTIALS, (SLOT + 1) * SUMSQ_PARTIALS
    if not (torch.equal(pb[:a], pi[:a]) and torch.equal(pb[b:], pi[b:])):
        out.append("md_sumsq wrote partials outside its own slot")
    slot = B["partials"].body[a:b]
    left = int((pb[a:b] == SENT_F32).sum())
    if left:
        out.append(f"{left} of {SUMSQ_PARTIALS} partials were not written")
    got = B["out"].body[0]
    finite = True
    if P.exact:
        want = torch.tensor(P.sum64, dtype=torch.float32)
        if float(slot.double().sum()) != P.sum64:
            out.append(f"partials add up to {float(slot.double().sum())!r}, want {P.sum64!r}")
        if got.cpu().view(torch.int32) != want.view(torch.int32):
            out.append(f"sum of squares {float(got)!r}, want exactly {P.sum64!r}")
    elif P.kind in ("randn", "wide"):
        ratio = abs(float(got.double()) - P.sum64) / (gamma(sumsq_depth(c.n)) * P.sum64) if math.isfinite(float(got)) else math.inf
        if not ratio <= 1.0:
            out.append(f"sum of squares: error / bound = {ratio:.3g} (D = {sumsq_depth(c.n)})")
    elif P.kind == "nan-tail":
        finite = False
        if not math.isnan(float(got)):
            out.append(f"a NaN element gave {float(got)!r}")
    else:
        finite = False
        if float(got) != math.inf:
            out.append(f"{P.kind}: sum of squares {float(got)!r}, want +inf")
    st = B["state"].body.tolist()
    if st != [1 if finite else 0, 5 if finite else 6, 6, 7]:
        out.append(f"md_step_guard left {st} from [7, 5, 6, 7] on a {'finite' if finite else 'non-finite'} sum")
    return out, ratio


FINISH_COUNTS = (1, 255, 256, 257, 1024, 1025, 64 * 1024)


class FinishProblem:
    """md_sumsq_finish on `count` small-integer partials (every one non-zero, the last one the largest: dropping it shows)."""

    def __init__(self, count, device="cpu"):
        gen = torch.Generator().manual_seed(count)
        x = torch.randint(1, 8, (count,), generator=gen).float()
        x[-1] = 64.0
        self.count, self.want = count, float(x.double().sum())
        assert self.want < 2 ** 24
        self.bufs = {"partials": Buf(count, torch.float32, device, x), "out": Buf(1, torch.float32, device, None)}

    def restore(self):
        for b in self.bufs.values():
            b.restore()

    def snapshot(self):
        return {k: b.raw.clone() for k, b in self.bufs.items()}

    def check(self):
        out = _fences(self.bufs)
        if not self.bufs["partials"].untouched():
            out.append("the partials were written")
        got = float(self.bufs["out"].body[0])
        if got != self.want:
            out.append(f"count {self.count}: got {got!r}, want exactly {self.want!r}")
        return out


CHECKSUM_SIZES = (8, 8 * (CHECKSUM_CAP * 256 + 37))


def checksum_ref(words_u16):
    """out2 of md_checksum_u16 on a numpy uint16 array: [sum of the words, sum of word_i * (((i * 0x9E3779B97F4A7C15) >> 32) | 1)] mod 2^64."""
    w = words_u16.astype(np.uint64)
    idx = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = ((idx * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)) | np.uint64(1)
        return np.array([w.sum(dtype=np.uint64), (w * h).sum(dtype=np.uint64)], dtype=np.uint64)


class ChecksumProblem:
    def __init__(self, n, device="cpu"):
        gen = torch.Generator().manual_seed(n)
        w = torch.randint(-32768, 32768, (n,), generator=gen, dtype=torch.int32).to(torch.int16)
        w[-1] = -1                                      # the last word is 0xffff: skipping it shows in both sums
        self.n = n
        self.bufs = {"x": Buf(n, torch.bfloat16, device, w.view(torch.bfloat16)), "out": Buf(2, torch.int64, device, [0, 0])}
        self.want = checksum_ref(w.numpy().view(np.uint16))

    def restore(self):
        for b in self.bufs.values():
            b.restore()

    def check(self):
        out = _fences(self.bufs)
        if not self.bufs["x"].untouched():
            out.append("the words were written")
        got = self.bufs["out"].body.cpu().numpy().view(np.uint64)
        if not (got == self.want).all():
            out.append(f"n {self.n}: checksum {got.tolist()}, want {self.want.tolist()}")
        return out


# ------------------------------------------------------------------------------------------------ the argument contract
def _aligned(ptr, a):
    return ptr is not None and ptr % a == 0


def _ranges_ok(d):
    if d.get("flat_off") is None or d.get("count") is None or not 1 <= d["n_ranges"] <= MAX_RANGES:
        return False
    return all(c > 0 and c % 4 == 0 and o >= 0 and o % 4 == 0 for o, c in zip(d["flat_off"][:d["n_ranges"]], d["count"][:d["n_ranges"]]))


def contract_accepts(d):
    """The argument rules of include/microdit_hip.h for one call (a dict as Problem.call() builds it): False = MD_BAD_ARG, nothing
    launched, nothing written."""
    e = d["entry"]
    if e == "sumsq":
        return d["g"] is not None and d["partials"] is not None and d["n"] > 0 and d["n"] % 8 == 0 and d["g"] % 16 == 0
    if e == "finish":
        return d["partials"] is not None and d["out"] is not None and d["count"] > 0
    if e == "guard":
        return d["sumsq"] is not None and d["state"] is not None
    if e == "checksum":
        return d["x"] is not None and d["out"] is not None and d["n"] > 0 and d["n"] % 8 == 0 and d["x"] % 16 == 0
    if e in ("adamw", "adamw_ranges"):
        if any(d[k] is None for k in ("p", "g", "m", "v")) or not all(_aligned(d[k], 16) for k in ("p", "g", "m", "v")):
            return False
        if d["ema_mode"] not in (0, 1, 2) or (d["ema_mode"] and not _aligned(d["ema"], 16)):
            return False
        if any(d[k] is not None and d[k] % 8 for k in ("g_bf16", "shadow")):
            return False
        if e == "adamw":
            return d["n"] > 0 and d["n"] % 4 == 0
        return d["g_bf16"] is not None and not d["zero_grad"] and _ranges_ok(d)
    if e in ("ema", "ema_ranges"):
        if d["p"] is None or d["ema"] is None or d["beta"] is None or not 1 <= d["n_profiles"] <= EMA_MAX or d["p"] % 16:
            return False
        for ptr, b in zip(d["ema"][:d["n_profiles"]], d["beta"][:d["n_profiles"]]):
            if not _aligned(ptr, 16) or not (0.0 <= b < 1.0):
                return False
        if e == "ema":
            return d["n"] > 0 and d["n"] % 4 == 0
        return _ranges_ok(d)
    raise ValueError(e)


def _set(**kw):
    return lambda d: d.update(kw)


def _shift(key, nbytes):
    def f(d):
        d[key] = d[key] + nbytes
    return f


def _item(key, j, val):
    def f(d):
        d[key] = list(d[key])
        d[key][j] = val
    return f


def _item_shift(key, j, nbytes):
    def f(d):
        d[key] = list(d[key])
        d[key][j] += nbytes
    return f


# (name, base, change): `base` names the accepted call the refusal starts from; `change` edits its dict.  Written from the header.
REFUSALS = [(f"sumsq-{n}", "sumsq", f) for n, f in (
    ("null-g", _set(g=None)), ("null-partials", _set(partials=None)), ("n0", _set(n=0)), ("n-neg", _set(n=-8)), ("n-mod4", _set(n=12)),
    ("g-misaligned-4", _shift("g", 4)), ("g-misaligned-8", _shift("g", 8)))]
REFUSALS += [(f"sumsq-bf16-{n}", "sumsq-bf16", f) for n, f in (
    ("n-mod8", _set(n=20)), ("g-misaligned-2", _shift("g", 2)), ("g-misaligned-8", _shift("g", 8)))]
REFUSALS += [(f"finish-{n}", "finish", f) for n, f in (
    ("null-partials", _set(partials=None)), ("null-out", _set(out=None)), ("count0", _set(count=0)), ("count-neg", _set(count=-1)))]
REFUSALS += [(f"guard-{n}", "guard", f) for n, f in (("null-sumsq", _set(sumsq=None)), ("null-state", _set(state=None)))]
REFUSALS += [(f"checksum-{n}", "checksum", f) for n, f in (
    ("null-x", _set(x=None)), ("null-out", _set(out=None)), ("n0", _set(n=0)), ("n-mod8", _set(n=12)), ("x-misaligned", _shift("x", 8)))]
_ADAM_COMMON = (
    ("null-p", _set(p=None)), ("null-g", _set(g=None)), ("null-m", _set(m=None)), ("null-v", _set(v=None)),
    ("ema-mode-3", _set(ema_mode=3)), ("ema-mode-neg", _set(ema_mode=-1)), ("ema-mode-1-null", _set(ema_mode=1, ema=None)),
    ("ema-mode-2-null", _set(ema_mode=2, ema=None)),
    ("p-misaligned", _shift("p", 4)), ("g-misaligned", _shift("g", 8)), ("m-misaligned", _shift("m", 12)), ("v-misaligned", _shift("v", 4)),
    ("ema-misaligned", _shift("ema", 8)), ("gbf16-misaligned-2", _shift("g_bf16", 2)), ("gbf16-misaligned-4", _shift("g_bf16", 4)),
    ("shadow-misaligned-2", _shift("shadow", 2)), ("shadow-misaligned-4", _shift("shadow", 4)))
REFUSALS += [(f"adamw-{n}", "adamw", f) for n, f in _ADAM_COMMON + (
    ("n0", _set(n=0)), ("n-neg", _set(n=-4)), ("n-mod4", _set(n=1026)))]
REFUSALS += [(f"adamw-guarded-{n}", "adamw-guarded", f) for n, f in (("null-p", _set(p=None)), ("n-mod4", _set(n=6)), ("v-misaligned", _shift("v", 8)))]
_RANGE_COMMON = (
    ("null-flat-off", _set(flat_off=None)), ("null-count", _set(count=None)), ("n-ranges-0", _set(n_ranges=0)),
    ("n-ranges-65", _set(n_ranges=65, flat_off=[8 * j for j in range(65)], count=[4] * 65)),
    ("count-0", _item("count", 1, 0)), ("count-neg", _item("count", 0, -4)), ("count-mod4", _item("count", 2, 6)),
    ("flat-off-neg", _item("flat_off", 1, -4)), ("flat-off-mod4", _item("flat_off", 2, 10)))
REFUSALS += [(f"adamw-ranges-{n}", "adamw_ranges", f) for n, f in _ADAM_COMMON + _RANGE_COMMON + (
    ("zero-grad", _set(zero_grad=1)), ("null-gbf16", _set(g_bf16=None)))]
REFUSALS += [(f"adamw-ranges-guarded-{n}", "adamw_ranges-guarded", f) for n, f in (("zero-grad", _set(zero_grad=1)), ("n-ranges-65", _RANGE_COMMON[3][1]))]
_EMA_COMMON = (
    ("null-p", _set(p=None)), ("null-ema", _set(ema=None)), ("null-beta", _set(beta=None)), ("null-profile", _item("ema", 1, None)),
    ("profiles-0", _set(n_profiles=0)), ("profiles-5", _set(n_profiles=5)),
    ("p-misaligned", _shift("p", 4)), ("profile-misaligned", _item_shift("ema", 2, 8)),
    ("beta-1", _item("beta", 0, 1.0)), ("beta-neg", _item("beta", 2, -0.25)), ("beta-nan", _item("beta", 1, math.nan)))
REFUSALS += [(f"ema-{n}", "ema", f) for n, f in _EMA_COMMON + (("n0", _set(n=0)), ("n-neg", _set(n=-4)), ("n-mod4", _set(n=1022)))]
REFUSALS += [(f"ema-ranges-{n}", "ema_ranges", f) for n, f in _EMA_COMMON + _RANGE_COMMON]
assert len({r[0] for r in REFUSALS}) == len(REFUSALS)


class RefusalBase:
    """The accepted calls the refusals start from, each with its buffers; base(name) -> (call dict, the buffers it may touch)."""

    def __init__(self, device="cpu"):
        self.adam = AdamProblem(AdamCase("refusal-flat", 1028, "loud", True, 2), device)
        self.adam_r = AdamProblem(AdamCase("refusal-ranges", 0, "loud", True, 2, zero_grad=False, ranges="r3-gap4-mixed"), device)
        self.ema = EmaProblem(EmaCase("refusal-flat", 1028, (0.5, 0.0, 0.25)), device)
        self.ema_r = EmaProblem(EmaCase("refusal-ranges", 0, (0.5, 0.0, 0.25), ranges="r3-gap4-mixed"), device)
        self.ss = SumsqProblem(SumsqCase("refusal-f32", 8 * 257, False, "exact"), device)
        self.ss_b = SumsqProblem(SumsqCase("refusal-bf16", 8 * 257, True, "exact"), device)
        self.cs = ChecksumProblem(8 * 257, device)

    def base(self, name):
        if name in ("sumsq", "sumsq-bf16"):
            P = self.ss_b if name.endswith("bf16") else self.ss
            return dict(entry="sumsq", g=P.bufs["g"].ptr(), bf16=int(P.case.bf16), n=P.case.n,
                        partials=P.bufs["partials"].ptr(SLOT * SUMSQ_PARTIALS)), P.bufs
        if name == "finish":
            return dict(entry="finish", partials=self.ss.bufs["partials"].ptr(), count=SUMSQ_PARTIALS, out=self.ss.bufs["out"].ptr()), self.ss.bufs
        if name == "guard":
            return dict(entry="guard", sumsq=self.ss.bufs["out"].ptr(), state=self.ss.bufs["state"].ptr()), self.ss.bufs
        if name == "checksum":
            return dict(entry="checksum", x=self.cs.bufs["x"].ptr(), n=self.cs.n, out=self.cs.bufs["out"].ptr()), self.cs.bufs
        if name.startswith("adamw"):
            P = self.adam_r if "ranges" in name else self.adam
            d = P.call()
            if name.endswith("guarded"):
                d.update(guard=P.bufs["guard"].ptr(), guarded=True)
            return d, P.bufs
        P = self.ema_r if "ranges" in name else self.ema
        return P.call(), P.bufs
