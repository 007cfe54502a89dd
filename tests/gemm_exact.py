"""Exact references for md_gemm_bf16 (pure torch, no GPU needed): inputs for which the right answer has no rounding error.

Operand entries come from {-1, 0, 1}: every product is an integer and every partial sum stays far below 2^24, so fp32
accumulation is exact in ANY order (any k-tile order, any split, any MFMA shape), and every |value| <= 256 is exact in bf16.
The epilogue operands are small integers or powers of two (bias in [-8, 8], alpha in {0.5, -2}, residual in [-8, 8], gate in
{-2..2}, a cached activation derivative in {-2, -1, -0.5, 0, 0.5, 1, 2}), so every non-transcendental epilogue has exactly ONE
correct bit pattern and the comparison is torch.equal against an int64 / fp64 reference.  For the transcendental epilogues B is
drawn from {-1/8, 0, 1/8}: the pre-activation is an exact multiple of 1/8, the raw copy is compared bit for bit and the activated
output per element against the fp64 function: |out - f64| <= 2^-8 |f64| + a * s  (one bf16 ulp plus the activation's own
absolute error `a`, scaled by the magnitude `s` of the exact multiplicand; tolerance_a() says where `a` comes from).

Storage (Fenced): nothing is dense and everything is fenced.  Every operand and output lies inside a larger allocation filled
with a NaN sentinel, with a leading dimension strictly larger than its extent -- a DIFFERENT excess for every field of
md_gemm_args, so that a kernel that reads one field where it should read another changes the result -- guard rows before and
after, and guard columns from round_up(N, 8) to ld (the header allows whole 16-byte chunks to be written when their first element
is in range, so the fence starts at the next multiple of 8).  After a launch the fence is compared bit for bit with its
initial contents.

The case table (CASES, expected()) states for every (variant, case) whether the kernel family must RUN the problem or must
REFUSE it; it is written from the contract in include/microdit_hip.h and the eligibility rules of the persistent kernels
(md_gemm_pp_shape_ok, pp_instantiated, w4_instantiated, md_gemm_w4_eligible), not from what a launch returns.

emulate() is a plain fp64 model of the md_gemm_bf16 contract that addresses memory exactly as the struct says (pointer + batch
stride + row * ld + column): the CPU test runs every case through it in place of the kernel, which checks the storage helper, the
references and their preconditions, and lets the mutation tests break one thing at a time.
"""
import dataclasses
import functools
import zlib

import torch

ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU = 0, 1, 2, 3
EPI_STORE_BF16, EPI_RESIDUAL, EPI_STORE_F32, EPI_ACCUM_F32, EPI_ATOMIC_F32, EPI_DACT, EPI_SWIGLU_BWD = 0, 1, 2, 3, 4, 5, 6
VARIANTS = ("reg128", "dma128", "paced256", "pp256", "w4")
TWO_STAGE = ("reg128", "dma128", "paced256")
PERSISTENT = ("pp256", "w4")
NOT_ELIGIBLE, BAD_ARG = -2, -1
BKT = 64                       # k-tile of the 2-stage kernels: split-K ranges are whole k-tiles (gemm_bf16_kernel)
ACT_NAMES = {ACT_NONE: "none", ACT_GELU_TANH: "gelu_tanh", ACT_GELU_ERF: "gelu_erf", ACT_SILU: "silu"}

SENT_BF16 = 0x7FC1             # a quiet NaN no kernel produces
SENT_F32 = 0x7FC0BEEF          # a quiet NaN with a recognisable payload
# leading-dimension excess per field: all different, so any swapped field changes the result
EXCESS = dict(lda=8, ldb=16, ldc=24, ldc2=32, ldr=40, ldg=48, ldaux=56, ldbias=64)
# extra elements between batches, per stride field: all different, none dense
STRIDE_EXTRA = dict(sA=8, sB=16, sC=24, sC2=32, sBias=40, sAux=48, sSplit=56)
GUARD_ROWS = 3


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ storage
class Fenced:
    """`planes` matrices [rows, cols] with leading dimension ld inside one sentinel-filled allocation.

    Element (p, r, c) lives at raw[off + plane_offsets[p] + r * ld + c]; off = GUARD_ROWS * ld + col0.  `ptr(p)` is what a
    launch passes.  After fill() the whole allocation is frozen; dirty() lists every element outside the may-be-written band
    (rows of the matrices, columns [0, round_up(cols, 8))) whose BITS differ from the frozen ones."""

    def __init__(self, rows, cols, ld, dtype, plane_offsets=(0,), col0=0, device="cpu"):
        assert dtype in (torch.bfloat16, torch.float32)
        assert ld % 8 == 0 and col0 % 8 == 0 and col0 + round_up(cols, 8) <= ld, (cols, col0, ld)
        assert all(o % 8 == 0 and o >= 0 for o in plane_offsets)
        self.rows, self.cols, self.ld, self.dtype, self.col0 = rows, cols, ld, dtype, col0
        self.plane_offsets = tuple(plane_offsets)
        self.off = GUARD_ROWS * ld + col0
        # the tail also holds rows * (largest excess): a launch that walks this matrix with ANOTHER field's leading dimension stays inside
        self.total = self.off + max(self.plane_offsets) + rows * ld + GUARD_ROWS * ld + rows * max(EXCESS.values())
        self.bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        sent = SENT_BF16 if dtype == torch.bfloat16 else SENT_F32
        self.raw = torch.full((self.total,), sent, dtype=self.bits, device=device)
        self.frozen = None

    @property
    def esize(self):
        return 2 if self.dtype == torch.bfloat16 else 4

    @property
    def typed(self):
        return self.raw.view(self.dtype)

    def index(self, cols=None):
        cols = self.cols if cols is None else cols
        dev = self.raw.device
        p = torch.tensor(self.plane_offsets, dtype=torch.int64, device=dev).view(-1, 1, 1)
        r = torch.arange(self.rows, dtype=torch.int64, device=dev).view(1, -1, 1) * self.ld
        c = torch.arange(cols, dtype=torch.int64, device=dev).view(1, 1, -1)
        return self.off + p + r + c

    def fill(self, values=None):
        """values [planes, rows, cols] (or None: the matrices stay sentinel); the pad columns up to the next multiple of 8
        are zeroed (the header: 'the caller pads the rows to the next multiple of 8 with finite values')."""
        if values is not None:
            pad = round_up(self.cols, 8)
            v = torch.zeros(len(self.plane_offsets), self.rows, pad, dtype=self.dtype, device=self.raw.device)
            v[:, :, :self.cols] = values.to(device=self.raw.device, dtype=self.dtype)
            self.typed[self.index(pad).reshape(-1)] = v.reshape(-1)
        self.frozen = self.raw.clone()
        return self

    def values(self):
        return self.typed[self.index().reshape(-1)].view(len(self.plane_offsets), self.rows, self.cols)

    def elem_offset(self, plane=0):
        return self.off + self.plane_offsets[plane]

    def ptr(self, plane=0, extra=0):
        return self.raw.data_ptr() + (self.elem_offset(plane) + extra) * self.esize

    def dirty(self):
        """Flat indices outside the may-be-written band whose bits changed since fill()."""
        allowed = torch.zeros(self.total, dtype=torch.bool, device=self.raw.device)
        allowed[self.index(round_up(self.cols, 8)).reshape(-1)] = True
        return torch.nonzero((self.raw != self.frozen) & ~allowed).reshape(-1)

    def untouched(self):
        return bool(torch.equal(self.raw, self.frozen))

    def refreeze(self):
        """Take the current contents as the state later checks compare with (an output that becomes the next launch's input)."""
        self.frozen = self.raw.clone()
        return self

    def describe(self, flat):
        rel = int(flat) - self.off
        return f"element {int(flat)} of the allocation = row {rel // self.ld}, column {rel % self.ld + 0} relative to plane 0 (ld {self.ld})"


class Ptr:
    """A device pointer as the emulator sees it: an allocation and an element offset into it."""

    def __init__(self, buf, offset):
        self.buf, self.offset = buf, offset

    def address(self):
        return self.buf.raw.data_ptr() + self.offset * self.buf.esize

    def advanced(self, elements):
        return Ptr(self.buf, self.offset + elements)


# ------------------------------------------------------------------------------------------------ activations
def act_fn(x, act):
    """act(x) in the dtype of x (torch fp32 = libm-grade, fp64 = the reference)."""
    if act == ACT_GELU_TANH:
        return torch.nn.functional.gelu(x, approximate="tanh")
    if act == ACT_GELU_ERF:
        return torch.nn.functional.gelu(x)
    if act == ACT_SILU:
        return torch.nn.functional.silu(x)
    return x


def dact_fn(x, act):
    """act'(x) in the dtype of x."""
    if act == ACT_GELU_TANH:
        k0, k1 = 0.7978845608028654, 0.044715
        t = torch.tanh(k0 * (x + k1 * x * x * x))
        return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k0 * (1 + 3 * k1 * x * x)
    if act == ACT_GELU_ERF:
        return 0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)
    if act == ACT_SILU:
        s = torch.sigmoid(x)
        return s * (1 + x * (1 - s))
    return torch.ones_like(x)


@functools.lru_cache(maxsize=None)
def measured_d(act, derivative):
    """d: the largest difference between torch's fp32 evaluation and the fp64 evaluation of the activation (its derivative) on the
    inputs the tests can produce: every multiple of 1/8 with |x| <= 32.  Evaluated on the CPU, never from a kernel's output."""
    x = torch.arange(-256, 257, dtype=torch.float64) / 8
    f = dact_fn if derivative else act_fn
    return float((f(x.float(), act).double() - f(x, act)).abs().max())


# `d` as measured on the CPU this file was written on (torch 2.x, glibc libm); tolerance_a() uses these FIXED values so that the bound
# does not move with the machine, and the CPU test checks that a fresh measurement does not exceed them.
D_MEASURED = {
    (ACT_GELU_TANH, False): 2.48e-7, (ACT_GELU_TANH, True): 4.81e-7,
    (ACT_SILU, False): 1.14e-6, (ACT_SILU, True): 9.67e-7,
    (ACT_GELU_ERF, False): 5.61e-7, (ACT_GELU_ERF, True): 8.82e-8,     # (reported only: the erf forms use the documented bound)
}


def tolerance_a(act, derivative):
    """The absolute term of the activation tolerance.  erf-GELU and its derivative: 4e-6 = twice the polynomial bound md_common.h
    documents (|GELU error| <= 1.6e-6), rounded up.  tanh-GELU, SiLU and their derivatives: the project states no bound, so
    a = 8 * d with d = D_MEASURED (the kernel chains about four ~1-ulp hardware operations where torch calls libm)."""
    if act == ACT_GELU_ERF:
        return 4e-6
    return 8.0 * D_MEASURED[(act, derivative)]


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    akc: int = 1
    bkc: int = 1
    mode: int = EPI_STORE_BF16
    act: int = ACT_NONE
    alpha: float = 1.0
    bias: bool = False
    c2: bool = False
    res: str = ""              # RESIDUAL: "gate" (res + gate), "plain" (res, no gate), "inplace" (C aliases res, no gate)
    rps: int = 0               # rows_per_sample of the gate
    dact_cached: int = 0
    batch: int = 1
    shared_b: bool = False     # sB = 0: one weight matrix for every batch
    ksplit: int = 1
    c_slice: bool = False      # C is a column slice of a wider matrix: pointer offset col0 = 2 N, ldc = 3 N + 8 (packed qkv)
    gate_slice: bool = False   # the gate is a column slice of a [samples, 6 N] matrix (the adaLN vector)
    cu_limit: int = 0
    tail_mode: int = 0
    variants: tuple = VARIANTS
    data: str = ""             # cases with the same `data` draw the same operands (default: the name)

    @property
    def transcendental(self):
        return self.act != ACT_NONE and not (self.mode == EPI_DACT and self.dact_cached) or self.mode == EPI_SWIGLU_BWD

    @property
    def seed(self):
        return zlib.crc32((self.data or self.name).encode())


def epi_kind(c):
    """The epilogue instantiation of the persistent kernels a case needs, or None (md_gemm_pp_epi_kind)."""
    if c.mode == EPI_STORE_BF16:
        if c.act == ACT_NONE:
            return "bf16"
        if c.act == ACT_GELU_ERF:
            return "gelu_d" if (c.dact_cached and c.c2) else "gelu"
        return None
    if c.mode == EPI_RESIDUAL:
        return "res"
    if c.mode == EPI_DACT:
        return ("dact_mul" if c.dact_cached else "dact_gelu") if c.act == ACT_GELU_ERF else None
    if c.mode == EPI_STORE_F32:
        return "f32"
    if c.mode == EPI_SWIGLU_BWD:
        return "swiglu"
    return None                # ACCUM_F32 / ATOMIC_F32 stay on the 2-stage kernels


# layout (a_kcontig, b_kcontig) -> epilogues built (pp_instantiated / w4_instantiated)
PP_BUILT = {(1, 1): {"bf16", "res", "dact_gelu", "dact_mul"}, (1, 0): {"bf16", "gelu", "gelu_d", "res", "f32"}, (0, 0): {"f32"}, (0, 1): set()}
W4_BUILT = {(1, 1): {"bf16", "res", "dact_gelu", "dact_mul"}, (1, 0): {"bf16", "gelu", "gelu_d", "res", "swiglu"}, (0, 0): {"f32"}, (0, 1): set()}
TWO_STAGE_BUILT = {"bf16", "bf16_act", "res", "f32", "accum", "atomic", "dact"}


def _pp_shape_ok(c, epi):
    if c.K % c.ksplit:
        return False
    kspan = c.K // c.ksplit
    if kspan < 128 or kspan % 128 or c.N % 8:
        return False
    if epi == "res" and c.res == "gate" and c.rps % 64:
        return False
    if epi in ("res", "dact_gelu", "dact_mul", "swiglu") and (c.bias or c.alpha != 1.0 or c.M % 256 or c.N % 256):
        return False           # only the plain, interior form of the operand-carrying epilogues is built
    return True


def expected(variant, c):
    """'run', 'refuse' (MD_NOT_ELIGIBLE, nothing launched) or 'bad' (-1) for kernel family `variant` on case c."""
    if c.ksplit > 1 and c.mode not in (EPI_ATOMIC_F32, EPI_STORE_F32):
        return "bad"
    if c.mode == EPI_SWIGLU_BWD:
        if variant != "w4":
            return "refuse"    # built into the 4-wave kernel only
        ok = W4_BUILT[(c.akc, c.bkc)].__contains__("swiglu") and _pp_shape_ok(c, "swiglu") and c.batch == 1 and not c.cu_limit
        return "run" if ok else "refuse"
    if variant in TWO_STAGE:
        return "run"           # the 2-stage kernels take every layout, shape and epilogue
    epi = epi_kind(c)
    built = PP_BUILT if variant == "pp256" else W4_BUILT
    if epi is None or epi not in built[(c.akc, c.bkc)] or not _pp_shape_ok(c, epi):
        return "refuse"
    if variant == "w4":
        if c.bias or c.alpha != 1.0:
            return "refuse"
        if epi == "f32":
            if c.M % 256 or c.N % 256:
                return "refuse"
        elif c.ksplit != 1:
            return "refuse"
    return "run"


def epilogue_name(c):
    """The epilogue a case exercises, as the coverage check counts it."""
    if c.mode == EPI_STORE_BF16:
        if c.act == ACT_NONE:
            return "bf16"
        return ("gelu_d" if (c.dact_cached and c.c2) else "gelu") if c.act == ACT_GELU_ERF else "bf16_act"
    if c.mode == EPI_DACT:
        return epi_kind(c) or "dact"
    return {EPI_RESIDUAL: "res", EPI_STORE_F32: "f32", EPI_ACCUM_F32: "accum", EPI_ATOMIC_F32: "atomic", EPI_SWIGLU_BWD: "swiglu"}[c.mode]


def split_ranges(K, ksplit, variant="reg128"):
    """[k0, k1) of every split.  The 2-stage kernels cut K in whole 64-wide k-tiles, ceil(tiles / ksplit) per split: the last
    split may be shorter, and a split past the end has NO work (K = 64, ksplit = 3) -- its slice is then written with
    alpha * 0 + bias, i.e. zeros, never left as it was.  The persistent kernels require K % (ksplit * 128) == 0, where the
    two rules agree."""
    ntk = (K + BKT - 1) // BKT
    tps = (ntk + ksplit - 1) // ksplit
    return [(min(s * tps * BKT, K), min((s + 1) * tps * BKT, K)) for s in range(ksplit)]


def _layout_cases():
    out = []
    shapes = [(136, 72, 104), (264, 136, 64), (128, 128, 24), (392, 264, 328)]
    for (M, N, K) in shapes:
        for akc in (1, 0):
            for bkc in (1, 0):
                for mode, tag in ((EPI_STORE_BF16, "bf16"), (EPI_STORE_F32, "f32")):
                    out.append(Case(f"small-{M}x{N}x{K}-a{akc}b{bkc}-{tag}", M, N, K, akc, bkc, mode, variants=TWO_STAGE))
    # the MoE gate: rows padded to 8, E = 4 / 8 experts
    for E in (4, 8):
        out.append(Case(f"moe-logits-E{E}", 192, E, 128, 1, 1, EPI_STORE_F32, variants=TWO_STAGE))
        out.append(Case(f"moe-dgrad-E{E}", 192, 128, E, 1, 0, EPI_STORE_BF16, variants=TWO_STAGE))
        out.append(Case(f"moe-wgrad-E{E}", E, 128, 192, 0, 0, EPI_STORE_F32, variants=TWO_STAGE))
    return out


def _persistent_cases():
    out = []
    shapes = [(256, 256, 128), (256, 512, 384), (520, 264, 384), (512, 512, 1024)]
    for (M, N, K) in shapes:
        for (akc, bkc) in ((1, 1), (1, 0), (0, 0)):
            for mode, tag in ((EPI_STORE_BF16, "bf16"), (EPI_STORE_F32, "f32")):
                out.append(Case(f"pers-{M}x{N}x{K}-a{akc}b{bkc}-{tag}", M, N, K, akc, bkc, mode, variants=PERSISTENT))
        # the operand-carrying epilogues: interior form only -> the ragged shape must be refused
        out.append(Case(f"pers-{M}x{N}x{K}-res", M, N, K, 1, 1, EPI_RESIDUAL, res="gate", rps=64, c2=True, variants=PERSISTENT))
        out.append(Case(f"pers-{M}x{N}x{K}-res-nn", M, N, K, 1, 0, EPI_RESIDUAL, res="inplace", variants=PERSISTENT))
        out.append(Case(f"pers-{M}x{N}x{K}-dact", M, N, K, 1, 1, EPI_DACT, act=ACT_GELU_ERF, variants=PERSISTENT))
        out.append(Case(f"pers-{M}x{N}x{K}-dactc", M, N, K, 1, 1, EPI_DACT, act=ACT_GELU_ERF, dact_cached=1, variants=PERSISTENT))
        out.append(Case(f"pers-{M}x{N}x{K}-gelu", M, N, K, 1, 0, EPI_STORE_BF16, act=ACT_GELU_ERF, c2=True, variants=PERSISTENT))
        out.append(Case(f"pers-{M}x{N}x{K}-gelud", M, N, K, 1, 0, EPI_STORE_BF16, act=ACT_GELU_ERF, c2=True, dact_cached=1, variants=PERSISTENT))
    # uneven persistent tile lists: 20 tiles dealt 3 / 2 (8 workgroups) and 2 / 1 (12 workgroups)
    for cu in (8, 12):
        out.append(Case(f"pers-cu{cu}-bf16", 1280, 1024, 256, 1, 1, cu_limit=cu, variants=PERSISTENT))
        out.append(Case(f"pers-cu{cu}-nn-res", 1280, 1024, 256, 1, 0, EPI_RESIDUAL, res="gate", rps=64, cu_limit=cu, variants=PERSISTENT))
        out.append(Case(f"pers-cu{cu}-tn-f32", 1280, 1024, 256, 0, 0, EPI_STORE_F32, cu_limit=cu, variants=PERSISTENT))
    return out


def _epilogue_cases():
    out = []
    S = (264, 136, 192)        # ragged on both tile sizes, three k-tiles
    T = (392, 264, 328)
    P = (256, 256, 256)        # whole tiles: the persistent kernels take the operand-carrying epilogues
    out.append(Case("epi-bias", *S, bias=True))
    out.append(Case("epi-alpha-half", *S, alpha=0.5, c2=True))
    out.append(Case("epi-alpha-neg2-bias", *S, 1, 0, alpha=-2.0, bias=True, c2=True))
    out.append(Case("epi-bias-c2-whole", *P, 1, 0, alpha=0.5, bias=True, c2=True))
    out.append(Case("epi-cslice", *S, c_slice=True, c2=True))
    out.append(Case("epi-cslice-f32", *S, 1, 0, EPI_STORE_F32, bias=True, alpha=-2.0, c_slice=True))
    for act in (ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU):
        nm = ACT_NAMES[act]
        out.append(Case(f"epi-{nm}-c2", *S, 1, 0, act=act, c2=True, bias=True))
        out.append(Case(f"epi-{nm}-c2-whole", *P, 1, 0, act=act, c2=True))
        out.append(Case(f"epi-{nm}-cslice", *S, 1, 1, act=act, c_slice=True))
        out.append(Case(f"epi-dact-{nm}", *S, 1, 1, EPI_DACT, act=act, alpha=0.5))
        out.append(Case(f"epi-dact-{nm}-whole", *P, 1, 1, EPI_DACT, act=act))
        out.append(Case(f"epi-dact-{nm}-cslice", *S, 1, 0, EPI_DACT, act=act, c_slice=True))
    out.append(Case("epi-gelu_erf-cached", *S, 1, 0, act=ACT_GELU_ERF, c2=True, dact_cached=1))
    out.append(Case("epi-gelu_erf-cached-whole", *P, 1, 0, act=ACT_GELU_ERF, c2=True, dact_cached=1))
    out.append(Case("epi-gelu_erf-cached-cslice", *P, 1, 0, act=ACT_GELU_ERF, c2=True, dact_cached=1, c_slice=True))
    out.append(Case("epi-dact-cached", *S, 1, 1, EPI_DACT, act=ACT_GELU_ERF, dact_cached=1))
    out.append(Case("epi-dact-cached-whole", *P, 1, 1, EPI_DACT, act=ACT_GELU_ERF, dact_cached=1))
    out.append(Case("epi-dact-cached-cslice", *P, 1, 1, EPI_DACT, act=ACT_GELU_ERF, dact_cached=1, c_slice=True))
    # residual
    out.append(Case("epi-res-gate64", *T, res="gate", rps=64, mode=EPI_RESIDUAL, c2=True))
    out.append(Case("epi-res-gate64-whole", *P, res="gate", rps=64, mode=EPI_RESIDUAL, c2=True))
    out.append(Case("epi-res-gate64-whole-nn", 512, 256, 384, 1, 0, res="gate", rps=64, mode=EPI_RESIDUAL, gate_slice=True, c_slice=True))
    out.append(Case("epi-res-gate-slice", *T, res="gate", rps=64, mode=EPI_RESIDUAL, gate_slice=True, c_slice=True))
    out.append(Case("epi-res-gate8", *T, res="gate", rps=8, mode=EPI_RESIDUAL, variants=TWO_STAGE[:2] + PERSISTENT))
    out.append(Case("epi-res-gate77", *T, res="gate", rps=77, mode=EPI_RESIDUAL, c2=True, variants=TWO_STAGE[:2] + PERSISTENT))
    out.append(Case("epi-res-inplace", *T, 1, 0, res="inplace", mode=EPI_RESIDUAL))
    out.append(Case("epi-res-inplace-whole", *P, 1, 0, res="inplace", mode=EPI_RESIDUAL))
    out.append(Case("epi-res-bias", *T, res="gate", rps=64, mode=EPI_RESIDUAL, bias=True))
    out.append(Case("epi-res-plain-bias-whole", *P, res="plain", mode=EPI_RESIDUAL, bias=True))
    # fp32 outputs
    out.append(Case("epi-f32-store", *S, 0, 0, EPI_STORE_F32, bias=True, alpha=0.5))
    out.append(Case("epi-f32-accum", *S, 0, 0, EPI_ACCUM_F32, bias=True, alpha=-2.0))
    out.append(Case("epi-f32-accum-nt", *T, 1, 1, EPI_ACCUM_F32))
    out.append(Case("epi-f32-atomic-k1", *S, 0, 0, EPI_ATOMIC_F32, alpha=0.5))
    out.append(Case("epi-f32-atomic-k3", *T, 0, 0, EPI_ATOMIC_F32, ksplit=3))
    out.append(Case("epi-f32-accum-cslice", *S, 1, 0, EPI_ACCUM_F32, bias=True, c_slice=True))
    out.append(Case("epi-f32-atomic-cslice", *S, 0, 1, EPI_ATOMIC_F32, ksplit=2, c_slice=True))
    # the SwiGLU backward in the w3 data gradient: w4 only, every other family and every other shape refuses
    out.append(Case("epi-swiglu-256", 256, 256, 128, 1, 0, EPI_SWIGLU_BWD))
    out.append(Case("epi-swiglu-512", 512, 256, 384, 1, 0, EPI_SWIGLU_BWD))
    out.append(Case("epi-swiglu-cslice", 256, 256, 256, 1, 0, EPI_SWIGLU_BWD, c_slice=True))
    out.append(Case("epi-swiglu-ragged", 520, 256, 384, 1, 0, EPI_SWIGLU_BWD, variants=("w4",)))
    out.append(Case("epi-swiglu-nt", 256, 256, 128, 1, 1, EPI_SWIGLU_BWD, variants=("w4",)))
    out.append(Case("epi-swiglu-held", 256, 256, 128, 1, 0, EPI_SWIGLU_BWD, cu_limit=248, variants=("w4",)))
    return out


def _batched_cases():
    out = []
    out.append(Case("batch3-nn-gelu", 136, 136, 128, 1, 0, act=ACT_GELU_ERF, c2=True, bias=True, batch=3))
    out.append(Case("batch3-nt-bias", 264, 72, 104, 1, 1, bias=True, alpha=0.5, c2=True, batch=3))
    out.append(Case("batch3-shared-b", 264, 136, 128, 1, 1, batch=3, shared_b=True, c2=True))
    out.append(Case("batch3-dact-cached", 256, 256, 128, 1, 1, EPI_DACT, act=ACT_GELU_ERF, dact_cached=1, batch=3))
    out.append(Case("batch3-whole-nn-gelud", 256, 256, 128, 1, 0, act=ACT_GELU_ERF, c2=True, dact_cached=1, batch=3))
    out.append(Case("batch3-tn-f32", 136, 72, 192, 0, 0, EPI_STORE_F32, batch=3, ksplit=2))
    return out


def _splitk_cases():
    out = []
    for ks, K in ((2, 256), (3, 328), (4, 512), (3, 64)):      # 328 / 3: the last split is shorter; 64 / 3: two splits have no work
        out.append(Case(f"splitk{ks}-K{K}-tn", 136, 72, K, 0, 0, EPI_STORE_F32, ksplit=ks, variants=TWO_STAGE))
        out.append(Case(f"splitk{ks}-K{K}-nt", 264, 136, K, 1, 1, EPI_STORE_F32, ksplit=ks, variants=TWO_STAGE))
    for ks in (2, 3):                                          # persistent kernels: kspan 128
        out.append(Case(f"splitk{ks}-pers-tn", 256, 512, 128 * ks, 0, 0, EPI_STORE_F32, ksplit=ks, variants=PERSISTENT))
        out.append(Case(f"splitk{ks}-pers-tn-ragged", 520, 264, 128 * ks, 0, 0, EPI_STORE_F32, ksplit=ks, variants=PERSISTENT))
        out.append(Case(f"splitk{ks}-pers-nn", 256, 256, 128 * ks, 1, 0, EPI_STORE_F32, ksplit=ks, variants=PERSISTENT))
    return out


TAIL_SHAPE = (512, 1280, 512)  # 10 tiles on 8 workgroups: r = 2, 4 iterations, s = 4 with a 2 MiB workspace
TAIL_SPLIT = 4


def _tail_cases():
    out = []
    for tm in (1, 2):
        kw = dict(cu_limit=8, tail_mode=tm, variants=("pp256",), data="tail")
        out.append(Case(f"tail{tm}-plain", *TAIL_SHAPE, 1, 1, **kw))             # (one draw per epilogue: the shapes and fields differ)
        out.append(Case(f"tail{tm}-gelu-c2", *TAIL_SHAPE, 1, 0, act=ACT_GELU_ERF, c2=True, **kw))
        out.append(Case(f"tail{tm}-res-gate", *TAIL_SHAPE, 1, 1, EPI_RESIDUAL, res="gate", rps=64, c2=True, **kw))
        out.append(Case(f"tail{tm}-dact", *TAIL_SHAPE, 1, 1, EPI_DACT, act=ACT_GELU_ERF, **kw))
        out.append(Case(f"tail{tm}-dact-cached", *TAIL_SHAPE, 1, 1, EPI_DACT, act=ACT_GELU_ERF, dact_cached=1, **kw))
    return out


CASES = _layout_cases() + _persistent_cases() + _epilogue_cases() + _batched_cases() + _splitk_cases() + _tail_cases()
assert len({c.name for c in CASES}) == len(CASES)
CASE_BY_NAME = {c.name: c for c in CASES}
TABLE = [(c.name, v, expected(v, c)) for c in CASES for v in c.variants]


# ------------------------------------------------------------------------------------------------ problems
def _draw(gen, shape, choices):
    ch = torch.tensor(choices, dtype=torch.float64)
    return ch[torch.randint(0, len(choices), shape, generator=gen)]


class Problem:
    """One case with its storage, its launch arguments and its exact reference."""

    def __init__(self, case, device="cpu"):
        c = self.case = case
        gen = torch.Generator().manual_seed(c.seed)
        M, N, K, nb = c.M, c.N, c.K, c.batch
        frac = c.transcendental and c.mode == EPI_STORE_BF16       # forward activation: pre-activation = exact multiple of 1/8
        gate_choices = (-1, 0, 1) if K > 1024 else (-2, -1, 0, 1, 2)
        Av = _draw(gen, (nb, M, K), (-1, 0, 1))
        Bv = _draw(gen, (1 if c.shared_b else nb, N, K), (-0.125, 0, 0.125) if frac else (-1, 0, 1))
        self.logical = dict(A=Av, B=Bv)
        self.bufs, self.args = {}, {}
        a = self.args

        def planes(rows, ld, field, n=nb):
            stride = (rows + 1) * ld + STRIDE_EXTRA[field]
            return stride, tuple(b * stride for b in range(n))

        def operand(name, vals, kcontig, ldfield, sfield, n):
            mat = vals if kcontig else vals.transpose(1, 2)
            rows, cols = mat.shape[1], mat.shape[2]
            ld = round_up(cols, 8) + EXCESS[ldfield]
            stride, offs = planes(rows, ld, sfield, n)
            buf = Fenced(rows, cols, ld, torch.bfloat16, offs, device=device).fill(mat)
            self.bufs[name] = buf
            a[name] = Ptr(buf, buf.elem_offset())
            a[ldfield] = ld
            a[sfield] = stride

        operand("A", Av, c.akc, "lda", "sA", nb)
        operand("B", Bv, c.bkc, "ldb", "sB", 1 if c.shared_b else nb)
        if c.shared_b:
            a["sB"] = 0
        a.update(M=M, N=N, K=K, a_kcontig=c.akc, b_kcontig=c.bkc, mode=c.mode, act=c.act, alpha=c.alpha, batch=nb, ksplit=c.ksplit,
                 rows_per_sample=c.rps, dact_cached=c.dact_cached, cu_limit=c.cu_limit, tail_mode=c.tail_mode)

        # ---- epilogue operands
        if c.bias:
            bv = torch.randint(-8, 9, (nb, 1, N), generator=gen).double()
            ld = round_up(N, 8) + EXCESS["ldbias"]
            stride, offs = planes(1, ld, "sBias")
            self.bufs["bias"] = Fenced(1, N, ld, torch.float32, offs, device=device).fill(bv)
            a["bias"], a["sBias"] = Ptr(self.bufs["bias"], self.bufs["bias"].elem_offset()), stride
            self.logical["bias"] = bv
        else:
            bv = torch.zeros(nb, 1, N, dtype=torch.float64)
        wide = 2 * N if c.mode == EPI_SWIGLU_BWD else N           # SwiGLU backward: aux and C are [M, 2 N]
        if c.mode == EPI_RESIDUAL:
            assert nb == 1
            rv = torch.randint(-8, 9, (1, M, N), generator=gen).double()
            self.logical["res"] = rv
            if c.res == "gate":
                ns = (M + c.rps - 1) // c.rps
                gv = _draw(gen, (1, ns, N), gate_choices)
                if c.gate_slice:
                    ldg, col0 = 6 * round_up(N, 8), 4 * round_up(N, 8)
                else:
                    ldg, col0 = round_up(N, 8) + EXCESS["ldg"], 0
                self.bufs["gate"] = Fenced(ns, N, ldg, torch.bfloat16, col0=col0, device=device).fill(gv)
                a["gate"], a["ldg"] = Ptr(self.bufs["gate"], self.bufs["gate"].elem_offset()), ldg
                self.logical["gate"] = gv
        if c.mode in (EPI_DACT, EPI_SWIGLU_BWD):
            if c.mode == EPI_DACT and c.dact_cached:
                xv = _draw(gen, (nb, M, wide), (-2, -1, -0.5, 0, 0.5, 1, 2))
            else:
                xv = torch.randint(-32, 33, (nb, M, wide), generator=gen).double() / 8
            ld = round_up(wide, 8) + EXCESS["ldaux"]
            stride, offs = planes(M, ld, "sAux")
            self.bufs["aux"] = Fenced(M, wide, ld, torch.bfloat16, offs, device=device).fill(xv)
            a["aux"], a["ldaux"], a["sAux"] = Ptr(self.bufs["aux"], self.bufs["aux"].elem_offset()), ld, stride
            self.logical["aux"] = xv

        # ---- outputs
        f32 = c.mode in (EPI_STORE_F32, EPI_ACCUM_F32, EPI_ATOMIC_F32)
        if c.c_slice:
            ldc, col0 = 3 * round_up(wide, 8) + 8, 2 * round_up(wide, 8)
        else:
            ldc, col0 = round_up(wide, 8) + EXCESS["ldc"], 0
        nslice = c.ksplit if c.mode == EPI_STORE_F32 else 1
        s_split = (M + 1) * ldc + STRIDE_EXTRA["sSplit"]
        s_c = nslice * s_split + (M + 1) * ldc + STRIDE_EXTRA["sC"] if nslice > 1 else (M + 1) * ldc + STRIDE_EXTRA["sC"]
        offs = tuple(b * s_c + s * s_split for b in range(nb) for s in range(nslice))
        cbuf = Fenced(M, wide, ldc, torch.float32 if f32 else torch.bfloat16, offs, col0=col0, device=device)
        init = None
        if c.mode in (EPI_ACCUM_F32, EPI_ATOMIC_F32):
            init = torch.randint(-8, 9, (nb, M, N), generator=gen).double()          # a non-zero C
            self.logical["c_init"] = init
        elif c.mode == EPI_RESIDUAL and c.res == "inplace":
            init = self.logical["res"]
        cbuf.fill(init)
        self.bufs["C"] = cbuf
        a["C"], a["ldc"], a["sC"], a["sSplit"] = Ptr(cbuf, cbuf.elem_offset()), ldc, s_c, s_split
        if c.mode == EPI_RESIDUAL:
            if c.res == "inplace":
                a["res"], a["ldr"] = a["C"], ldc
            else:
                ldr = round_up(N, 8) + EXCESS["ldr"]
                self.bufs["res"] = Fenced(M, N, ldr, torch.bfloat16, device=device).fill(self.logical["res"])
                a["res"], a["ldr"] = Ptr(self.bufs["res"], self.bufs["res"].elem_offset()), ldr
        if c.c2:
            ld2 = round_up(N, 8) + EXCESS["ldc2"]
            stride, offs2 = planes(M, ld2, "sC2")
            self.bufs["C2"] = Fenced(M, N, ld2, torch.bfloat16, offs2, device=device).fill(None)
            a["C2"], a["ldc2"], a["sC2"] = Ptr(self.bufs["C2"], self.bufs["C2"].elem_offset()), ld2, stride
        self.outputs = ["C"] + (["C2"] if c.c2 else [])
        self._reference()

    # ---- the reference: from the LOGICAL values, in fp64 (every intermediate is an exact small integer or dyadic fraction)
    def _reference(self):
        c, L = self.case, self.logical
        A, B = L["A"], L["B"].expand(c.batch, -1, -1)
        bias = L.get("bias", torch.zeros(c.batch, 1, c.N, dtype=torch.float64))
        self.expect = {}       # name -> ("exact", tensor) | ("tol", f64 tensor, s tensor, a)
        if c.mode == EPI_STORE_F32:
            parts = [torch.einsum("bmk,bnk->bmn", A[:, :, k0:k1], B[:, :, k0:k1]) * c.alpha + bias for k0, k1 in split_ranges(c.K, c.ksplit)]
            ref = torch.stack(parts, 1).reshape(c.batch * c.ksplit, c.M, c.N)
            self.expect["C"] = ("exact", ref)
        acc = torch.einsum("bmk,bnk->bmn", A, B)
        self.acc = acc
        pre = acc * c.alpha + bias
        if c.mode == EPI_STORE_F32:
            pass
        elif c.mode in (EPI_ACCUM_F32, EPI_ATOMIC_F32):
            self.expect["C"] = ("exact", L["c_init"] + (pre if c.mode == EPI_ACCUM_F32 else acc * c.alpha))
        elif c.mode == EPI_STORE_BF16:
            if c.act == ACT_NONE:
                self.expect["C"] = ("exact", pre)
            else:
                self.expect["C"] = ("tol", act_fn(pre, c.act), torch.ones_like(pre), tolerance_a(c.act, False))
            if c.c2:
                if c.dact_cached:
                    self.expect["C2"] = ("tol", dact_fn(pre, c.act), torch.ones_like(pre), tolerance_a(c.act, True))
                else:
                    self.expect["C2"] = ("exact", pre)
        elif c.mode == EPI_RESIDUAL:
            g = L["gate"].repeat_interleave(c.rps, 1)[:, :c.M] if c.res == "gate" else 1.0
            self.expect["C"] = ("exact", L["res"] + g * pre)
            if c.c2:
                self.expect["C2"] = ("exact", pre)
        elif c.mode == EPI_DACT:
            if c.dact_cached:
                self.expect["C"] = ("exact", pre * L["aux"])
            else:
                self.expect["C"] = ("tol", pre * dact_fn(L["aux"], c.act), pre.abs(), tolerance_a(c.act, True))
        elif c.mode == EPI_SWIGLU_BWD:
            h1, h2 = L["aux"][:, :, :c.N], L["aux"][:, :, c.N:]
            f = torch.cat([acc * h2 * dact_fn(h1, ACT_SILU), acc * act_fn(h1, ACT_SILU)], 2)
            s = torch.cat([(acc * h2).abs(), acc.abs()], 2)
            self.expect["C"] = ("tol", f, s, max(tolerance_a(ACT_SILU, True), tolerance_a(ACT_SILU, False)))
        self.check_preconditions()

    def check_preconditions(self):
        """On the reference alone, before any comparison: a bf16 output's reference equals its own bf16 round trip and max |ref| <= 256
        (exact epilogues); the pre-activation of a transcendental epilogue is exact in bf16 with |x| <= 32."""
        c = self.case
        for name, e in self.expect.items():
            if e[0] == "exact":
                ref = e[1]
                assert float(ref.abs().max()) <= 256, (c.name, name, float(ref.abs().max()))
                if self.bufs[name].dtype == torch.bfloat16:
                    assert torch.equal(ref.to(torch.bfloat16).double(), ref), f"{c.name}: reference of {name} is not exact in bf16"
                else:
                    assert torch.equal(ref.float().double(), ref)
        if c.mode == EPI_STORE_BF16 and c.act != ACT_NONE:
            pre = self.acc * c.alpha + self.logical.get("bias", 0.0)
            assert float(pre.abs().max()) <= 32 and torch.equal(pre.to(torch.bfloat16).double(), pre), c.name
        if c.mode in (EPI_DACT, EPI_SWIGLU_BWD, EPI_RESIDUAL):         # the value the epilogue rounds to bf16 before it multiplies
            pa = self.acc * c.alpha + self.logical.get("bias", 0.0)
            assert float(pa.abs().max()) <= 256 and torch.equal(pa.to(torch.bfloat16).double(), pa), c.name

    # ---- launch arguments for micro_diffusion_amd.hip.gemm
    def launch_kwargs(self, args=None):
        a = dict(self.args if args is None else args)
        kw = {k: (v.address() if isinstance(v, Ptr) else v) for k, v in a.items()}
        for k in ("ldc2", "ldr", "ldg", "ldaux", "sC2", "sBias", "sAux"):
            kw.setdefault(k, 0)
        return kw

    # ---- comparison
    def mismatches(self, bufs=None):
        """One message per output that does not match the reference (empty list = all match)."""
        bufs = self.bufs if bufs is None else bufs
        c, out = self.case, []
        for name in self.outputs:
            e = self.expect[name]
            got = bufs[name].values().detach().cpu()
            if e[0] == "exact":
                ref = e[1].to(got.dtype)
                if torch.equal(got, ref):
                    continue
                bad = torch.nonzero(~(got == ref))
            else:
                f, s, a_ = e[1], e[2], e[3]
                err = (got.double() - f).abs()
                ok = err <= 2.0 ** -8 * f.abs() + a_ * s
                if bool(ok.all()):
                    continue
                bad = torch.nonzero(~ok)
            p, r, col = (int(v) for v in bad[0])
            nsl = c.ksplit if c.mode == EPI_STORE_F32 else 1
            want = float(e[1][p, r, col])
            out.append(f"{c.name}: {name} differs at {len(bad)} of {got.numel()} elements; first at batch {p // nsl}, k-split {p % nsl}, "
                       f"(row {r}, col {col}) = 128-tile ({r // 128}, {col // 128}), 256-tile ({r // 256}, {col // 256}): "
                       f"got {float(got[p, r, col])!r}, want {want!r}")
        return out

    def fence_violations(self, bufs=None):
        bufs = self.bufs if bufs is None else bufs
        out = []
        for name, b in bufs.items():
            d = b.dirty()
            if d.numel():
                out.append(f"{self.case.name}: {d.numel()} fence elements of {name} were written; first: {b.describe(d[0])}")
        return out

    def all_untouched(self):
        return [n for n, b in self.bufs.items() if not b.untouched()]


# ------------------------------------------------------------------------------------------------ the fp64 model of the contract
def _gather(ptr, base, rows, cols, ld, transposed=False):
    r = torch.arange(rows, dtype=torch.int64).view(-1, 1)
    c = torch.arange(cols, dtype=torch.int64).view(1, -1)
    idx = ptr.offset + base + (c * ld + r if transposed else r * ld + c)
    return ptr.buf.typed[idx.reshape(-1)].view(rows, cols).double()


def _scatter(ptr, base, ld, vals):
    rows, cols = vals.shape
    r = torch.arange(rows, dtype=torch.int64).view(-1, 1)
    c = torch.arange(cols, dtype=torch.int64).view(1, -1)
    ptr.buf.typed[(ptr.offset + base + r * ld + c).reshape(-1)] = vals.to(ptr.buf.dtype).reshape(-1)


def truncate_bf16(x):
    """fp64 -> bf16 by dropping the low bits of the fp32 value (round toward zero): the mutation, never the reference."""
    return (x.float().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def emulate(args, drop_k=None, double_k=None, to_bf16=None):
    """md_gemm_bf16 as include/microdit_hip.h states it, in fp64 on the CPU, addressing memory through the struct's pointers,
    leading dimensions and strides alone.  drop_k = (row, k): that product is left out; double_k = (row, k): counted twice;
    to_bf16: the conversion of bf16 outputs (default: round to nearest even) -- the knobs of the mutation tests."""
    a = args
    rd = to_bf16 or (lambda x: x.to(torch.bfloat16))
    M, N, K, mode = a["M"], a["N"], a["K"], a["mode"]
    for b in range(a["batch"]):
        A = _gather(a["A"], b * a["sA"], M, K, a["lda"], transposed=not a["a_kcontig"])
        B = _gather(a["B"], b * a["sB"], N, K, a["ldb"], transposed=not a["b_kcontig"])
        bias = _gather(a["bias"], b * a["sBias"], 1, N, N) if a.get("bias") is not None else torch.zeros(1, N, dtype=torch.float64)
        ranges = split_ranges(K, a["ksplit"]) if mode == EPI_STORE_F32 else [(0, K)]
        for s, (k0, k1) in enumerate(ranges):
            acc = A[:, k0:k1] @ B[:, k0:k1].t()
            for knob, sign in ((drop_k, -1.0), (double_k, 1.0)):
                if knob is not None and k0 <= knob[1] < k1:
                    acc[knob[0]] += sign * A[knob[0], knob[1]] * B[:, knob[1]]
            pre = acc * a["alpha"] + bias
            cb = b * a["sC"]
            if mode == EPI_STORE_F32:
                _scatter(a["C"], cb + s * a["sSplit"], a["ldc"], pre)
            elif mode in (EPI_ACCUM_F32, EPI_ATOMIC_F32):
                old = _gather(a["C"], cb, M, N, a["ldc"])
                _scatter(a["C"], cb, a["ldc"], old + (pre if mode == EPI_ACCUM_F32 else acc * a["alpha"]))
            elif mode == EPI_STORE_BF16:
                if a.get("C2") is not None:
                    raw = dact_fn(rd(pre).double(), a["act"]) if a["dact_cached"] else pre
                    _scatter(a["C2"], b * a["sC2"], a["ldc2"], rd(raw))
                _scatter(a["C"], cb, a["ldc"], rd(act_fn(pre, a["act"])))
            elif mode == EPI_RESIDUAL:
                res = _gather(a["res"], 0, M, N, a["ldr"])
                if a.get("C2") is not None:
                    _scatter(a["C2"], b * a["sC2"], a["ldc2"], rd(pre))
                g = 1.0
                if a.get("gate") is not None:
                    ns = (M + a["rows_per_sample"] - 1) // a["rows_per_sample"]
                    g = _gather(a["gate"], 0, ns, N, a["ldg"]).repeat_interleave(a["rows_per_sample"], 0)[:M]
                _scatter(a["C"], cb, a["ldc"], rd(res + g * rd(pre).double()))
            elif mode == EPI_DACT:
                aux = _gather(a["aux"], b * a["sAux"], M, N, a["ldaux"])
                _scatter(a["C"], cb, a["ldc"], rd(pre * (aux if a["dact_cached"] else dact_fn(aux, a["act"]))))
            elif mode == EPI_SWIGLU_BWD:
                h = _gather(a["aux"], b * a["sAux"], M, 2 * N, a["ldaux"])
                g = rd(acc).double()
                _scatter(a["C"], cb, a["ldc"], rd(torch.cat([g * h[:, N:] * dact_fn(h[:, :N], ACT_SILU), g * act_fn(h[:, :N], ACT_SILU)], 1)))
            else:
                raise ValueError(mode)


def splitk_reduce_ref(slices, out_init, accumulate):
    """md_splitk_reduce on exact inputs: slices [ksplit, ...] fp64; accumulate 0 = store, 1 = add to out, 2 = store as bf16."""
    s = slices.sum(0)
    return out_init + s if accumulate == 1 else s
