"""The MoE routing kernels of csrc/routing.hip at their edges -- the E > 8 template instances, widths past one 512-column trip, the
second grid-stride pass of the wave-per-row kernels, ties, sequence lengths off the multiple of 256 and at the accepted maximum,
the compaction corners -- each against the plain torch restatement of tests/moe_ref.py (kept honest by tests/test_moe_ref_cpu.py),
at the shapes tests/kernel_geometry.py names (their branches guarded by tests/test_kernel_geometry_cpu.py).

What is held to bits and what to a bound (U = 2^-24; comparison helpers of tests/test_kernel_geometry_gpu.py):
  * md_moe_route      probs within (E + 6 + |x_e - max x|) U relative + 2^-120 of the fp64 softmax of the bf16-rounded logits (E
                      additions, expf at 1 ulp, reciprocal, product, the argument's rounding through the exponential); padding
                      columns exactly 0; rowidx / gval / slot bit-equal to a stable descending sort of the kernel's own probabilities.
  * combine (+ _abs)  br and out bit-exact: every operation is a single IEEE rounding in a fixed order.
  * combine_bwd       dh2 bit-exact; dgval a sum: (8 ceil(C / 512) + 6 + 2) U of sum|terms| (a lane's serial chain + the six-step
                      wave reduction; the products of two bf16 values are exact).
  * dispatch_bwd      dx bit-exact; dlogits within ulp(ref) + (E + 3) U p_e (|dp_e| + sum|dp p|) (the E-term dot product, the
                      subtraction and the product in fp32, then one bf16 rounding); padding exactly 0.
  * compact_kept, get_mask   integer / copy work: bit-exact.

The tables handed to combine, the backward kernels and the compaction are synthetic (built by moe_ref on the host, not by
md_moe_route): a routing bug can neither hide an addressing bug nor be blamed for one.  Every index of a table is checked against the
buffer it addresses on the host before any launch.  Outputs are pre-filled with a sentinel (NaN, -7) and allocated between guard rows
that must keep it; input padding and unaddressed input rows hold NaN.

NaN and infinite logits are out of scope: the trainer's non-finite step guard skips such steps before routing matters."""
import pytest
import torch

from tests import kernel_geometry as kg
from tests import moe_ref as mr
from tests.test_kernel_geometry_gpu import U, assert_exact, assert_sum, assert_within, ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32, F32, BF16 = torch.int32, torch.float32, torch.bfloat16
NAN = float("nan")
GUARD = 3           # guard rows in front of and behind every output
PAD = 5             # unaddressed list positions in front of the absolute-position tables


# ---------------------------------------------------------------------------------------------------------------- plumbing
class Out:
    """An output buffer [rows, cols] between GUARD guard rows on either side, everything pre-filled with a sentinel."""

    def __init__(self, rows, cols, dtype):
        self.fill = NAN if dtype.is_floating_point else -7
        self.buf = torch.full((rows + 2 * GUARD, cols), self.fill, device=DEV, dtype=dtype)
        self.t = self.buf[GUARD:GUARD + rows]

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self, what):
        """The output on the host, after checking that the guard rows still hold the sentinel."""
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]]).cpu()
        ok = torch.isnan(g.float()).all() if self.buf.dtype.is_floating_point else (g == self.fill).all()
        assert bool(ok), f"{what}: a guard row was written"
        return self.t.cpu()


def untouched(t):
    """Elements (host tensor) that still hold the sentinel of Out."""
    return torch.isnan(t.float()) if t.dtype.is_floating_point else t == -7


def gpu(t):
    return t.to(DEV).contiguous()


def rand_bf16(g, *shape):
    return torch.randn(*shape, generator=g).to(BF16)


def check_slot_table(slot, B, S, E, k, stride, rows):
    """Host-side bounds check of a slot table against the list buffers it addresses (`rows` rows per expert)."""
    assert slot.shape == (B * S, E) and slot.dtype == I32
    lo, hi, n = mr.table_index_range(slot, B, S, k, stride)
    assert lo >= -1 and 0 <= hi < n == rows, (lo, hi, n, rows)
    if stride is None:
        assert int(slot.max()) < k


# ---------------------------------------------------------------------------------------------------------------- md_moe_route
def route(hip, logits_e, B, S, E, k, ld):
    """md_moe_route on logits [B * S, E] (host), padded with NaN to ld.  Host copies of probs [M, ld], rowidx, gval, slot."""
    M = B * S
    lg = torch.full((M, ld), NAN)
    lg[:, :E] = logits_e
    lg = gpu(lg)
    probs, rowidx, gval, slot = Out(M, ld, F32), Out(E, B * k, I32), Out(E, B * k, F32), Out(M, E, I32)
    hip.check(hip.lib().md_moe_route(lg.data_ptr(), probs.ptr(), ld, B, S, E, k, rowidx.ptr(), gval.ptr(), slot.ptr(), hip.stream_ptr()),
              "md_moe_route")
    torch.cuda.synchronize()
    return probs.cpu("probs"), rowidx.cpu("rowidx"), gval.cpu("gval"), slot.cpu("slot")


def route_logits(case):
    """fp32 logits that are not bf16 values (the kernel's own rounding is exercised).  special: token 0 all at the project's -1e30
    sentinel, token 1 all at 3e38, tokens 2 / 3 mixes of +-3e38 (one / two winners)."""
    g = torch.Generator().manual_seed(case.S * 31 + case.E)
    x = torch.randn(case.B * case.S, case.E, generator=g) * 3
    assert float((x.to(BF16).float() != x).float().mean()) > 0.9
    if case.special:
        assert case.E == 4
        x[0] = -1e30
        x[1] = 3e38
        x[2] = torch.tensor([-3e38, 3e38, -3e38, -3e38])
        x[3] = torch.tensor([3e38, -3e38, -3e38, 3e38])
    return x


_ROUTED = {}


def routed(hip, case):
    if case.id not in _ROUTED:
        x = route_logits(case)
        _ROUTED[case.id] = (x,) + route(hip, x, case.B, case.S, case.E, case.k, case.ld)
    return _ROUTED[case.id]


@pytest.mark.parametrize("case", kg.MOE_ROUTE, ids=[c.id for c in kg.MOE_ROUTE])
def test_route_probs(hip, case):
    """probs against the fp64 softmax of the bf16-rounded logits, per element within the bound of the module docstring; the padding
    columns exactly 0.  The special case adds a row of all -1e30 and one of all 3e38 (both 1 / E) and +-3e38 mixes (exact splits).
    Measured on the all -1e30 row before the softmax maximum started from the row itself: NaN in all E columns (the maximum
    started at -1e30f, above bf16(-1e30), so every exp was 0 and the row 0 * inf)."""
    E = case.E
    x, probs, _, _, _ = routed(hip, case)
    xb = mr.bf16_logits(x, E)
    ref = mr.softmax64(x, E)
    dist = (xb - xb.max(-1, keepdim=True).values).abs()
    bound = (E + 6 + dist) * U * ref + 2.0 ** -120
    if case.special:
        print("all -1e30 row:", probs[0, :E].tolist(), " all 3e38 row:", probs[1, :E].tolist())
        assert float((ref[:2] - 1 / E).abs().max()) < 1e-15, "the reference of a row of equal logits is 1 / E"
        assert_within(probs[:2, :E], ref[:2], bound[:2], f"{case.id}: uniform rows (all -1e30, all 3e38)")
        assert probs[2, :E].tolist() == [0.0, 1.0, 0.0, 0.0] and probs[3, :E].tolist() == [0.5, 0.0, 0.0, 0.5], "+-3e38 splits"
    assert_within(probs[:, :E], ref, bound, f"{case.id}: probs")
    assert bool((probs[:, E:] == 0).all()), "padding columns must be exactly 0"


@pytest.mark.parametrize("case", kg.MOE_ROUTE, ids=[c.id for c in kg.MOE_ROUTE])
def test_route_selection(hip, case):
    """rowidx / gval / slot are the stable descending sort of the kernel's own probabilities, bit for bit; every element written."""
    B, S, E, k = case.B, case.S, case.E, case.k
    _, probs, rowidx, gval, slot = routed(hip, case)
    assert bool(torch.isfinite(probs[:, :E]).all()), "probabilities must be finite for the order to be defined"
    for name, t in (("rowidx", rowidx), ("gval", gval), ("slot", slot)):
        assert not bool(untouched(t).any()), f"{case.id}: {name} has unwritten elements"
    w_rowidx, w_gval, w_slot = mr.topk_tables(probs, B, S, E, k)
    assert_exact(rowidx, w_rowidx, f"{case.id}: rowidx")
    assert_exact(gval, w_gval, f"{case.id}: gval")
    assert_exact(slot, w_slot, f"{case.id}: slot")
    lists = rowidx.view(E, B, k).long() - (torch.arange(B) * S).view(1, B, 1)
    assert int(lists.min()) >= 0 and int(lists.max()) < S, "a list holds a token of another sample"
    srt = lists.sort(-1).values
    assert k == 1 or bool((srt[..., 1:] != srt[..., :-1]).all()), "a list holds a token twice"


TIES = {"all-equal": lambda: (*mr.tie_all_equal(2, 300, 3, 77), 2, 300, 3, 77),
        "saturated": lambda: (*mr.tie_saturated(100, 4, 40), 1, 100, 4, 40),
        "pairs-straddle-k": lambda: (*mr.tie_pairs(64, 33), 1, 128, 2, 33)}


@pytest.mark.parametrize("which", list(TIES))
def test_route_ties(hip, which):
    """Descending, ties to the lower token, in closed form (moe_ref.tie_*): nothing here depends on a computed probability."""
    logits, lists, B, S, E, k = TIES[which]()
    probs, rowidx, gval, slot = route(hip, logits, B, S, E, k, 8)
    got = rowidx.view(E, B, k).permute(1, 0, 2).long() - (torch.arange(B) * S).view(B, 1, 1)
    assert_exact(got, lists, f"{which}: lists")
    want_slot = torch.full((B, E, S), -1, dtype=torch.int64)
    want_slot.scatter_(-1, lists, torch.arange(k).expand(B, E, k).contiguous())
    assert_exact(slot.long().view(B, S, E).permute(0, 2, 1), want_slot, f"{which}: slot")
    if which == "saturated":
        assert set(probs[:, :E].unique().tolist()) == {0.0, 1.0}
        assert set(gval.unique().tolist()) == {0.0, 1.0}


# ---------------------------------------------------------------------------------------------------------------- synthetic tables
class Tables:
    """Synthetic routing tables of a kg.MoeTable case (host tensors).  Token 0 of every sample is chosen by all E experts, token 1
    by none; the rest at random.  Dense form: rowidx / gval [E, B k], slot.  Absolute form: a list of stride = B k + PAD positions
    per expert, the dense list mirrored behind PAD unaddressed positions (gate values there NaN)."""

    def __init__(self, case):
        B, S, E, k = case.B, case.S, case.E, case.k
        self.g = g = torch.Generator().manual_seed(case.S * 13 + case.E * 7 + case.C)
        scores = torch.rand(B * S, E, generator=g)
        scores.view(B, S, E)[:, 0] = 2.0
        scores.view(B, S, E)[:, 1] = -1.0
        self.rowidx, _, self.slot = mr.topk_tables(scores, B, S, E, k)
        self.gval = torch.rand(E, B * k, generator=g) + 0.25
        self.Bk, self.stride = B * k, B * k + PAD
        smp = (torch.arange(B * S) // S).view(-1, 1)
        self.slot_abs = torch.where(self.slot >= 0, (self.stride - 1 - (smp * k + self.slot)).to(I32), self.slot)
        self.gval_abs = self.mirror(self.gval)
        chosen = (self.slot >= 0).sum(1).view(B, S)
        assert bool((chosen[:, 0] == E).all()) and bool((chosen[:, 1] == 0).all())

    def mirror(self, t):
        """A dense list tensor [E, B k, ...] in the absolute layout [E, stride, ...]: NaN, then the list reversed."""
        out = torch.full((t.shape[0], self.stride) + tuple(t.shape[2:]), NAN, dtype=t.dtype)
        out[:, PAD:] = t.flip(1)
        return out

    def form(self, which):
        """(slot table, stride argument of moe_ref, list length)"""
        return (self.slot, None, self.Bk) if which == "dense" else (self.slot_abs, self.stride, self.stride)


_TABLES = {}


def tables(case):
    if case.id not in _TABLES:
        _TABLES[case.id] = Tables(case)
    return _TABLES[case.id]


TABLE_IDS = [c.id for c in kg.MOE_TABLES]
SMALL_TABLES = [c for c in kg.MOE_TABLES if "second-pass" not in c.id]


# ---------------------------------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize("form", ["dense", "abs"])
@pytest.mark.parametrize("case", kg.MOE_TABLES, ids=TABLE_IDS)
def test_combine(hip, case, form):
    """md_moe_combine / md_moe_combine_abs: br and out bit-exact.  Token 0 of every sample sums +2^20, ordinary values, -2^20 (gate
    values 1): the fp32 sum there depends on the expert order, so the reversed-order reference must differ -- as must the reference
    with one contribution left out."""
    B, S, E, k, C = case.B, case.S, case.E, case.k, case.C
    M = B * S
    t = tables(case)
    slot, stride, n = t.form(form)
    g = torch.Generator().manual_seed(C + E)
    h2, gval = rand_bf16(g, E, t.Bk, C), t.gval.clone()
    for s in range(B):                          # token 0 of sample s: list entry s k + slot of every expert
        for e in range(E):
            j = s * k + int(t.slot[s * S, e])
            gval[e, j] = 1.0
            if e in (0, E - 1):
                h2[e, j] = 2.0 ** 20 * (1 if e == 0 else -1)
    if form == "abs":
        h2, gval = t.mirror(h2), t.mirror(gval)
    res, mod = rand_bf16(g, M, C), rand_bf16(g, B, 6 * C)
    gate = mod[:, 5 * C:]
    check_slot_table(slot, B, S, E, k, stride, n)
    assert h2.shape == (E, n, C) and gval.shape == (E, n)
    d_h2, d_gval, d_slot, d_res, d_mod = gpu(h2), gpu(gval), gpu(slot), gpu(res), gpu(mod)
    br, out = Out(M, C, BF16), Out(M, C, BF16)
    L, st = hip.lib(), hip.stream_ptr()
    if form == "dense":
        hip.check(L.md_moe_combine(d_h2.data_ptr(), d_gval.data_ptr(), d_slot.data_ptr(), d_res.data_ptr(), d_mod[:, 5 * C:].data_ptr(), 6 * C,
                                   br.ptr(), out.ptr(), B, S, E, k, C, st), "md_moe_combine")
    else:
        hip.check(L.md_moe_combine_abs(d_h2.data_ptr(), d_gval.data_ptr(), d_slot.data_ptr(), d_res.data_ptr(), d_mod[:, 5 * C:].data_ptr(),
                                       6 * C, br.ptr(), out.ptr(), B, S, E, stride, C, st), "md_moe_combine_abs")
    torch.cuda.synchronize()
    br, out = br.cpu("br"), out.cpu("out")
    w_br, w_out = mr.combine(h2, gval, slot, res, gate, B, S, E, k, stride=stride)
    assert_exact(br, w_br, f"{case.id} {form}: br")
    assert_exact(out, w_out, f"{case.id} {form}: out")
    none = (slot < 0).all(1)
    assert int(none.sum()) >= B
    assert_exact(br[none], torch.zeros_like(br[none]), "br of a token no expert chose is +0")
    assert_exact(out[none], res[none], "out of a token no expert chose is res")
    rev_br, _ = mr.combine(h2, gval, slot, res, gate, B, S, E, k, stride=stride, order=range(E - 1, -1, -1))
    assert not torch.equal(rev_br[0], br[0]), "the check does not see the expert order of the sum"
    tok = M - 1 - int((slot.flip(0) >= 0).any(1).nonzero()[0])              # the last token some expert chose (second pass)
    e = int((slot[tok] >= 0).nonzero()[-1])
    skip_br, skip_out = mr.combine(h2, gval, slot, res, gate, B, S, E, k, stride=stride, skip=(tok, e))
    assert not torch.equal(skip_br, br) and not torch.equal(skip_out, out), "the check does not see one left-out contribution"


# ---------------------------------------------------------------------------------------------------------------- combine backward
def dg_rtol(C):
    """A lane adds its 8 products of each 512-column trip serially, then the six-step wave reduction (+2: margin for the order)."""
    return (8 * kg.col_trips(C) + 6 + 2) * U


def _bwd_second_pass_flat():
    """R = 32768 + 17 routed rows over 977 tokens, C = 8."""
    R, M = kg.MOE_BWD_SECOND_PASS, 977
    g = torch.Generator().manual_seed(R)
    return R, M, 8, torch.randint(0, M, (R,), generator=g, dtype=I32), torch.rand(R, generator=g) + 0.25, g


@pytest.mark.parametrize("cid", [c.id for c in SMALL_TABLES] + ["R-second-pass-C8"])
def test_combine_bwd_flat(hip, cid):
    """md_moe_combine_bwd: dh2 = bf16(fp32(g dbr[token])) to the bit, dgval the dot product as a sum."""
    if cid == "R-second-pass-C8":
        R, M, C, rowidx, gval, g = _bwd_second_pass_flat()
    else:
        case = next(c for c in SMALL_TABLES if c.id == cid)
        t = tables(case)
        R, M, C, rowidx, gval = case.E * t.Bk, case.B * case.S, case.C, t.rowidx.reshape(-1), t.gval.reshape(-1)
        g = torch.Generator().manual_seed(C + 1)
    assert rowidx.shape == (R,) and int(rowidx.min()) >= 0 and int(rowidx.max()) < M
    dbr, h2 = rand_bf16(g, M, C), rand_bf16(g, R, C)
    d_dbr, d_h2, d_rowidx, d_gval = gpu(dbr), gpu(h2), gpu(rowidx), gpu(gval)
    dh2, dg = Out(R, C, BF16), Out(R, 1, F32)
    hip.check(hip.lib().md_moe_combine_bwd(d_dbr.data_ptr(), d_h2.data_ptr(), d_rowidx.data_ptr(), d_gval.data_ptr(), dh2.ptr(), dg.ptr(), R, C,
                                           hip.stream_ptr()), "md_moe_combine_bwd")
    torch.cuda.synchronize()
    w_dh2, w_dg, w_abs, terms = mr.combine_bwd(dbr, h2, rowidx, gval)
    assert_exact(dh2.cpu("dh2"), w_dh2, f"{cid}: dh2")
    assert_sum(dg.cpu("dgval").view(-1), w_dg, w_abs, dg_rtol(C), f"{cid}: dgval", dropped=w_dg - terms[:, C - 8])


@pytest.mark.parametrize("cid", [c.id for c in SMALL_TABLES] + ["cap-second-pass-C8"])
def test_combine_bwd_compact(hip, cid):
    """md_moe_combine_bwd_compact on lists of `stride` positions per expert of which the first cap < stride are processed: the
    routed rows, then pad rows (a valid token, gate 0 -> dh2 exactly 0).  Rows at and beyond cap -- whose h2 is NaN -- stay untouched."""
    if cid == "cap-second-pass-C8":
        E, cap, M, C = 2, kg.MOE_BWD_SECOND_PASS, 977, 8
        stride, real = cap + 23, cap - 40
        g = torch.Generator().manual_seed(cap)
        rowidx = torch.randint(0, M, (E, stride), generator=g, dtype=I32)
        gval = torch.rand(E, stride, generator=g) + 0.25
    else:
        case = next(c for c in SMALL_TABLES if c.id == cid)
        t = tables(case)
        E, M, C, real = case.E, case.B * case.S, case.C, t.Bk
        stride, cap = t.stride, t.Bk + 2
        g = torch.Generator().manual_seed(C + 2)
        rowidx, gval = torch.empty(E, stride, dtype=I32), torch.empty(E, stride)
        rowidx[:, :real], gval[:, :real] = t.rowidx, t.gval
    rowidx[:, real:] = rowidx[:, :1]                                        # pad rows: the expert's first routed row, gate 0
    gval[:, real:] = 0.0
    assert real < cap < stride and int(rowidx.min()) >= 0 and int(rowidx.max()) < M
    dbr, h2 = rand_bf16(g, M, C), torch.full((E, stride, C), NAN, dtype=BF16)
    h2[:, :cap] = rand_bf16(g, E, cap, C)
    d_dbr, d_h2, d_rowidx, d_gval = gpu(dbr), gpu(h2), gpu(rowidx), gpu(gval)
    dh2, dg = Out(E * stride, C, BF16), Out(E * stride, 1, F32)
    hip.check(hip.lib().md_moe_combine_bwd_compact(d_dbr.data_ptr(), d_h2.data_ptr(), d_rowidx.data_ptr(), d_gval.data_ptr(), dh2.ptr(), dg.ptr(),
                                                   E, cap, stride, C, hip.stream_ptr()), "md_moe_combine_bwd_compact")
    torch.cuda.synchronize()
    dh2, dg = dh2.cpu("dh2").view(E, stride, C), dg.cpu("dgval").view(E, stride)
    rows = (torch.arange(E).view(E, 1) * stride + torch.arange(cap)).reshape(-1)
    w_dh2, w_dg, w_abs, terms = mr.combine_bwd(dbr, h2, rowidx, gval, rows=rows)
    assert_exact(dh2[:, :cap], w_dh2.view(E, cap, C), f"{cid}: dh2")
    assert_sum(dg[:, :cap].reshape(-1), w_dg, w_abs, dg_rtol(C), f"{cid}: dgval", dropped=w_dg - terms[:, C - 8])
    assert bool(untouched(dh2[:, cap:]).all()) and bool(untouched(dg[:, cap:]).all()), "rows at and beyond cap must stay untouched"
    assert not bool(dh2[:, real:cap].float().abs().any()), "pad rows: gate value 0 -> dh2 = 0"


# ---------------------------------------------------------------------------------------------------------------- dispatch backward
@pytest.mark.parametrize("form", ["dense", "abs"])
@pytest.mark.parametrize("case", kg.MOE_TABLES, ids=TABLE_IDS)
def test_dispatch_bwd(hip, case, form):
    """md_moe_dispatch_bwd / _abs: dx bit-exact against the fp32 sum in expert order; dlogits against the fp64 softmax backward
    (bound in the module docstring), its padding exactly 0.  probs' padding columns [E, ldp) hold NaN: they must not be read."""
    B, S, E, k, C, ldp, ldo = case.B, case.S, case.E, case.k, case.C, case.ldp, case.ldo
    M = B * S
    t = tables(case)
    slot, stride, n = t.form(form)
    g = torch.Generator().manual_seed(C + E + 3)
    dxin, dgval = rand_bf16(g, E, t.Bk, C), torch.randn(E, t.Bk, generator=g)
    if form == "abs":
        dxin, dgval = t.mirror(dxin), t.mirror(dgval)
    probs = torch.full((M, ldp), NAN)
    probs[:, :E] = torch.softmax(torch.randn(M, E, generator=g) * 2, -1)
    check_slot_table(slot, B, S, E, k, stride, n)
    assert dxin.shape == (E, n, C) and dgval.shape == (E, n)
    d_dxin, d_dgval, d_slot, d_probs = gpu(dxin), gpu(dgval), gpu(slot), gpu(probs)
    dx, dl = Out(M, C, BF16), Out(M, ldo, BF16)
    L, st = hip.lib(), hip.stream_ptr()
    if form == "dense":
        hip.check(L.md_moe_dispatch_bwd(d_dxin.data_ptr(), d_slot.data_ptr(), dx.ptr(), d_probs.data_ptr(), ldp, d_dgval.data_ptr(), dl.ptr(), ldo,
                                        B, S, E, k, C, st), "md_moe_dispatch_bwd")
    else:
        hip.check(L.md_moe_dispatch_bwd_abs(d_dxin.data_ptr(), d_slot.data_ptr(), dx.ptr(), d_probs.data_ptr(), ldp, d_dgval.data_ptr(), dl.ptr(),
                                            ldo, B, S, E, stride, C, st), "md_moe_dispatch_bwd_abs")
    torch.cuda.synchronize()
    dx, dl = dx.cpu("dx"), dl.cpu("dlogits")
    assert_exact(dx, mr.scatter_sum(dxin, slot, B, S, E, k, stride=stride), f"{case.id} {form}: dx")
    none = (slot < 0).all(1)
    assert_exact(dx[none], torch.zeros_like(dx[none]), "dx of a token no expert chose is +0")
    ref, mag = mr.softmax_bwd64(probs, dgval, slot, B, S, E, k, ldo, stride=stride)
    assert not bool(dl[:, E:].float().abs().any()) and not bool(torch.isnan(dl.float()).any()), "dlogits padding must be exactly 0"
    assert_within(dl[:, :E], ref[:, :E], ulp(ref[:, :E]) + (E + 3) * U * mag[:, :E], f"{case.id} {form}: dlogits")


# ---------------------------------------------------------------------------------------------------------------- compaction
@pytest.mark.parametrize("case", kg.MOE_COMPACT, ids=[c.id for c in kg.MOE_COMPACT])
def test_compact_kept(hip, case):
    """md_moe_compact_kept against moe_ref.compact on synthetic lists: k distinct tokens of the sample per (sample, expert), in random
    order; a `dead` expert picks dropped tokens only (count 0: every position a pad row -- its first routed token, gate 0)."""
    B, S, E, k, Tk = case.B, case.S, case.E, case.k, case.len_keep
    M, Bk = B * S, B * k
    g = torch.Generator().manual_seed(S + E)
    _, ids_restore, mask = mr.mask_tables(torch.rand(B, S, generator=g), Tk)
    scores = torch.rand(M, E, generator=g)
    if case.dead is not None:
        scores[:, case.dead] += mask.view(-1)
    rowidx, _, _ = mr.topk_tables(scores, B, S, E, k)
    gval = torch.rand(E, Bk, generator=g) + 0.25
    assert int(rowidx.min()) >= 0 and int(rowidx.max()) < M == ids_restore.numel()
    nchunk = -(-Bk // 1024)
    d_rowidx, d_gval, d_restore = gpu(rowidx), gpu(gval), gpu(ids_restore)
    ws = torch.empty(E * nchunk, device=DEV, dtype=I32)
    rowidx_c, gval_c, count, slot_c = Out(E, Bk, I32), Out(E, Bk, F32), Out(E, 1, I32), Out(M, E, I32)
    hip.check(hip.lib().md_moe_compact_kept(d_rowidx.data_ptr(), d_gval.data_ptr(), d_restore.data_ptr(), Tk, B, S, E, k, rowidx_c.ptr(),
                                            gval_c.ptr(), count.ptr(), slot_c.ptr(), ws.data_ptr(), ws.numel(), hip.stream_ptr()),
              "md_moe_compact_kept")
    torch.cuda.synchronize()
    rowidx_c, gval_c, count, slot_c = rowidx_c.cpu("rowidx_c"), gval_c.cpu("gval_c"), count.cpu("count").view(-1), slot_c.cpu("slot_c")
    want = mr.compact(rowidx, gval, ids_restore, Tk, B, S, E, k)
    for name, a, b in zip(("rowidx_c", "gval_c", "count", "slot_c"), (rowidx_c, gval_c, count, slot_c), want):
        assert_exact(a, b, f"{case.id}: {name}")
    dropped = mask.view(-1) > 0
    assert bool((slot_c[dropped] == -1).all()), "dropped tokens: -1 in every column"
    for e in range(E):                                   # every kept (token, expert) points at its own list position
        toks = (slot_c[:, e] >= 0).nonzero().view(-1)
        assert toks.numel() == int(count[e])
        assert torch.equal(rowidx_c[e, slot_c[toks, e].long()].long(), toks)
    if case.dead is not None:
        e = case.dead
        assert int(count[e]) == 0 and bool((rowidx_c[e] == rowidx[e, 0]).all()) and not bool(gval_c[e].abs().any())
        assert int(count.max()) > 0


# ---------------------------------------------------------------------------------------------------------------- masking
@pytest.mark.parametrize("case", kg.MOE_MASK, ids=[c.id for c in kg.MOE_MASK])
def test_get_mask(hip, case):
    """md_get_mask bit-exact against the stable sort, on noise full of duplicates, one run of equal values placed across the
    len_keep boundary (the lower-numbered tokens of the run are kept)."""
    B, T, Tk = case.B, case.T, case.len_keep
    g = torch.Generator().manual_seed(T)
    noise = torch.floor(torch.rand(B, T, generator=g) * (T // 4)) / (T // 4) + 0.001
    if Tk < T:
        srt = torch.sort(noise, dim=1, stable=True)
        for b in range(B):                                # the tokens at ranks Tk - 1, Tk (and Tk + 1): one value
            for r in range(Tk, min(Tk + 2, T)):
                noise[b, srt.indices[b, r]] = srt.values[b, Tk - 1]
        s2 = torch.sort(noise, dim=1).values
        assert bool((s2[:, Tk - 1] == s2[:, Tk]).all()), "a run of duplicates must straddle the boundary"
    d_noise = gpu(noise)
    keep, restore, mask = Out(B * Tk, 1, I32), Out(B, T, I32), Out(B, T, F32)
    hip.check(hip.lib().md_get_mask(d_noise.data_ptr(), B, T, Tk, keep.ptr(), restore.ptr(), mask.ptr(), hip.stream_ptr()), "md_get_mask")
    torch.cuda.synchronize()
    w_keep, w_restore, w_mask = mr.mask_tables(noise, Tk)
    assert_exact(keep.cpu("keep_rows").view(-1), w_keep, f"{case.id}: keep_rows")
    assert_exact(restore.cpu("ids_restore"), w_restore, f"{case.id}: ids_restore")
    assert_exact(mask.cpu("mask"), w_mask, f"{case.id}: mask")
    assert int(w_mask.sum()) == B * (T - Tk)
