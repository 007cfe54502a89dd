"""The Muon kernels (csrc/muon.hip) against tests/muon_ref.py on the GPU.

Items: 64 x 64, 64 x 192, 192 x 64 (tall), 128 x 320 and a 3-D tensor [2, 64, 128] as two adjacent items, at non-adjacent offsets inside
one flat buffer whose padding holds sentinel NaNs that must come back untouched (tests/muon_ref.py: SHAPES, GAPS).

What is compared how:
  * m', p', the shadow and the EMA: bit for bit with the fp32 reference (every operation of the header is one IEEE rounding).
  * norms: |got - ref| <= 1e-12 ref against an fp64 sum (the kernel's fp64 chain is 10 + 8 + 16 additions long: 34 * 2^-53 = 4e-15).
  * X = bf16(u * inv): equal to the reference's except for at most 0.1 % of an item's elements, those by one bf16 ulp -- inv is the
    fp32 rounding of an fp64 number that may differ from the reference's in its last bits.
  * Newton-Schulz: with R = ns_fp64(X), e_gpu = ||O - R|| / ||R|| <= 2 e_emu, e_emu the same distance for the CPU emulation with the
    kernel's rounding points (fp32 products, bf16 after A, B and X).  The GPU rounds at the same points and differs in summation order
    only.
  * one iteration, element by element: |X - X_emu| <= 2 ulp_bf16(X_emu) on every element, the ones that cancel to a thousandth of their
    neighbours included.  That only holds because the kernel rounds to bf16 where the emulation does and nowhere else (the fp32 sums
    differ in their order alone); a form that rounds A A or B X to bf16 on the way, or keeps the iterate scaled by a^-k, is up to
    thousands of ulps away on such elements.
  * md_muon_axpby: bit for bit with fl(fl(a x) + fl(b y)) rounded to bf16, inside sentinel guard bands."""
import ctypes

import pytest
import torch

from tests import muon_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
A_, B_, C_ = ref.NS_COEFFS
LR, WD, ES = 2.0 ** -10, 0.25, 0.75          # decay = 1 - 2^-12 exactly, fused or not


class Problem:
    """The item set on the GPU: flat fp32 p / g / m / ema, bf16 gradient and shadow, the bf16 workspace, the two tables."""

    def __init__(self, hip, seed=1, scales=None):
        self.hip, self.L = hip, hip.lib()
        self.items, self.total = ref.layout()
        self.n = len(self.items)
        scales = scales or [0.2 * max(r, c) ** 0.5 * A_ ** 5 for _, r, c in self.items]
        self.host = (hip.MuonItem * self.n)(*[hip.MuonItem(o, r, c, 0, s, 0) for (o, r, c), s in zip(self.items, scales)])
        need = ctypes.c_int64(0)
        assert self.L.md_muon_ws_bytes(self.host, self.n, ctypes.byref(need)) == 0
        self.ws_offs, self.bf_elems, ws_bytes = ref.ws_layout(self.items)
        assert [it.ws_off for it in self.host] == self.ws_offs and need.value == ws_bytes
        self.ws_elems = ws_bytes // 2            # the whole workspace as bf16 words: [items | fp32 scratch]
        self.scales = [float(it.scale) for it in self.host]
        self.upload()
        gen = torch.Generator().manual_seed(seed)
        self.mask = ref.item_mask(self.items, self.total)
        self.cpu = {}
        for name in ("p", "g", "m", "ema"):
            t = ref.poisoned(self.total, torch.float32)
            t[self.mask] = torch.randn(int(self.mask.sum()), generator=gen) * (0.05 if name == "p" else 1.0)
            self.cpu[name] = t
        gb = ref.poisoned(self.total, torch.bfloat16)
        gb[self.mask] = torch.randn(int(self.mask.sum()), generator=gen).to(torch.bfloat16)
        self.cpu["gb"] = gb
        self.cpu["shadow"] = ref.poisoned(self.total, torch.bfloat16)
        self.cpu["ws"] = ref.poisoned(self.ws_elems, torch.bfloat16)
        self.dev = {k: v.to(DEV) for k, v in self.cpu.items()}
        self.partials = torch.full((self.n * hip.MUON_NORM_PARTS,), -7.0, device=DEV, dtype=torch.float64)
        self.norms = torch.full((self.n,), -7.0, device=DEV, dtype=torch.float64)

    def upload(self):
        import numpy as np
        self.table = torch.from_numpy(np.frombuffer(self.host, dtype=np.uint8).copy()).to(DEV)

    def item(self, name, i, src=None):
        o, r, c = self.items[i]
        return (self.cpu if src is None else src)[name][o:o + r * c]

    def slot(self, ws, i):
        """X of item i inside a workspace tensor, as [rows, cols]."""
        _, r, c = self.items[i]
        o = self.ws_offs[i]
        return ws[o:o + r * c].view(r, c)

    def back(self):
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in self.dev.items()}

    def momentum(self, gbf16, nesterov, gs, ss, max_norm, zero_grad=1, guard=None, mu=0.95, **over):
        d = self.dev
        a = dict(g=d["g"].data_ptr(), gb=d["gb"].data_ptr() if gbf16 else None, m=d["m"].data_ptr(), table=self.table.data_ptr(),
                 host=self.host, n=self.n, ss=ss.data_ptr() if ss is not None else None, guard=guard.data_ptr() if guard is not None else None,
                 ws=d["ws"].data_ptr(), partials=self.partials.data_ptr(), norms=self.norms.data_ptr())
        a.update(over)
        return self.L.md_muon_momentum(a["g"], a["gb"], a["m"], a["table"], a["host"], a["n"], mu, int(nesterov), gs, a["ss"], max_norm,
                                       zero_grad, a["guard"], a["ws"], a["partials"], a["norms"], self.hip.stream_ptr())

    def newton_schulz(self, steps, **over):
        a = dict(host=self.host, n=self.n, ws=self.dev["ws"].data_ptr())
        a.update(over)
        cnt = ctypes.c_int32(-1)
        rc = self.L.md_muon_newton_schulz(a["host"], a["n"], steps, A_, B_, C_, a["ws"], ctypes.byref(cnt), self.hip.stream_ptr())
        return rc, cnt.value

    def apply(self, ema_mode, guard=None, **over):
        d = self.dev
        a = dict(p=d["p"].data_ptr(), shadow=d["shadow"].data_ptr(), ema=d["ema"].data_ptr(), table=self.table.data_ptr(), host=self.host,
                 n=self.n, ws=d["ws"].data_ptr())
        a.update(over)
        return self.L.md_muon_apply(a["p"], a["shadow"], a["ema"], a["table"], a["host"], a["n"], LR, WD, ema_mode, ES,
                                    guard.data_ptr() if guard is not None else None, a["ws"], self.hip.stream_ptr())

    def outside_untouched(self, got, names):
        for k in names:
            assert torch.equal(ref.bits(got[k])[~self.mask], ref.bits(self.cpu[k])[~self.mask]), f"{k}: the padding between the items was written"


def _flag(v):
    return torch.tensor([v, 5, 6, 7], device=DEV, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------- md_muon_momentum
@pytest.mark.parametrize("gbf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("nesterov", [True, False], ids=["nesterov", "plain"])
@pytest.mark.parametrize("clip", ["clipped", "unclipped", "null"])
def test_momentum(hip, gbf16, nesterov, clip):
    P = Problem(hip, seed=3)
    gs, max_norm = 0.5, 0.25
    ssv = {"clipped": 37.0, "unclipped": 1e-4, "null": None}[clip]
    ss = torch.tensor([ssv], device=DEV) if ssv is not None else None
    coef = ref.clip_coef(gs, ssv, max_norm)
    assert (coef < gs) == (clip == "clipped")
    assert P.momentum(gbf16, nesterov, gs, ss, max_norm) == 0
    got = P.back()
    norms = P.norms.cpu()
    for i, (o, r, c) in enumerate(P.items):
        g = P.item("gb" if gbf16 else "g", i)
        m_ref, u = ref.momentum_ref(g, P.item("m", i), coef, 0.95, nesterov)
        assert torch.equal(ref.bits(P.item("m", i, got)), ref.bits(m_ref)), f"item {i}: m' differs from the reference bits"
        nrm, inv, x_ref = ref.normalise_ref(u)
        rel = abs(float(norms[i]) - nrm) / nrm
        x = P.slot(got["ws"], i).reshape(-1)
        d = (ref.bits(x).int() - ref.bits(x_ref).int()).abs()
        print(f"item {i} [{r} x {c}] {clip}: norm rel err {rel:.2e}, X elements off by one ulp {int((d == 1).sum())} of {d.numel()}")
        assert rel <= 1e-12
        assert int(d.max()) <= 1 and int((d != 0).sum()) <= d.numel() // 1000
        assert not bool(torch.isnan(x.float()).any())
        # the Gram matrices of the item (and, behind the last item, the fp32 scratch) are not this pass's
        lo, hi = P.ws_offs[i] + r * c, (P.ws_offs[i + 1] if i + 1 < P.n else P.ws_elems)
        assert torch.equal(ref.bits(got["ws"][lo:hi]), ref.bits(P.cpu["ws"][lo:hi]))
    assert bool((got["g"][P.mask] == 0).all()) and int(ref.bits(got["g"])[P.mask].abs().max()) == 0, "the accumulators of the items are zeroed"
    P.outside_untouched(got, ("g", "m"))
    for k in ("gb", "p", "ema", "shadow"):
        assert torch.equal(ref.bits(got[k]), ref.bits(P.cpu[k])), f"{k} is not this pass's to write"


def test_momentum_keeps_the_gradient_without_zero_grad_and_guard_one_is_a_plain_launch(hip):
    P, Q = Problem(hip, seed=4), Problem(hip, seed=4)
    assert P.momentum(False, True, 1.0, None, 0.0, zero_grad=0) == 0
    assert Q.momentum(False, True, 1.0, None, 0.0, zero_grad=0, guard=_flag(1)) == 0
    a, b = P.back(), Q.back()
    assert torch.equal(ref.bits(a["g"]), ref.bits(P.cpu["g"]))
    assert all(torch.equal(ref.bits(a[k]), ref.bits(b[k])) for k in a) and torch.equal(P.norms, Q.norms)
    assert not torch.equal(ref.bits(a["m"]), ref.bits(P.cpu["m"]))


@pytest.mark.parametrize("gbf16", [False, True], ids=["f32", "bf16"])
def test_momentum_guard_zero(hip, gbf16):
    P = Problem(hip, seed=5)
    assert P.momentum(gbf16, True, 0.5, torch.tensor([float("inf")], device=DEV), 0.25, guard=_flag(0)) == 0
    got = P.back()
    for k in ("m", "ws", "gb", "p", "ema", "shadow"):
        assert torch.equal(ref.bits(got[k]), ref.bits(P.cpu[k])), f"{k} must stay bit-identical on a skipped step"
    assert bool((P.norms == -7.0).all())
    assert int(ref.bits(got["g"])[P.mask].abs().max()) == 0
    P.outside_untouched(got, ("g",))


# ---------------------------------------------------------------------------------------------------- md_muon_newton_schulz
def _ns_run(hip, steps):
    P = Problem(hip)
    xs = ref.ns_inputs()
    ws = P.cpu["ws"].clone()
    for i, x in enumerate(xs):
        P.slot(ws, i).copy_(x)
    P.dev["ws"] = ws.to(DEV)
    rc, launches = P.newton_schulz(steps)
    assert rc == 0
    torch.cuda.synchronize()
    out = P.dev["ws"].cpu()
    return P, xs, ws, out, launches


@pytest.fixture(scope="module")
def ns5(hip):
    """Five iterations on the shared inputs, twice, and the CPU references, computed once."""
    P, xs, ws_in, out, launches = _ns_run(hip, 5)
    _, _, _, again, _ = _ns_run(hip, 5)
    R = [ref.ns_fp64(x) for x in xs]
    emu = [ref.ns_bf16_emulated(x) for x in xs]
    O = [P.slot(out, i).double() for i in range(P.n)]                         # in place
    return dict(P=P, xs=xs, ws_in=ws_in, out=out, again=again, launches=launches, R=R, emu=emu, O=O)


def test_newton_schulz_error_against_the_emulation(ns5):
    P = ns5["P"]
    for i, (_, r, c) in enumerate(P.items):
        e_gpu, e_emu = ref.rel_err(ns5["O"][i], ns5["R"][i]), ref.rel_err(ns5["emu"][i], ns5["R"][i])
        sv = torch.linalg.svdvals(ns5["O"][i])
        print(f"item {i} [{r} x {c}]: e_gpu {e_gpu:.4e}  e_emu {e_emu:.4e}  ratio {e_gpu / e_emu:.3f}  singular values of O in "
              f"[{float(sv.min()):.3f}, {float(sv.max()):.3f}]")
        assert e_gpu <= 2 * e_emu
        assert not bool(torch.isnan(ns5["O"][i]).any())


def test_newton_schulz_is_deterministic_and_stays_inside_the_workspace(ns5):
    assert torch.equal(ref.bits(ns5["out"]), ref.bits(ns5["again"])), "two runs must give identical bits"
    P = ns5["P"]
    assert not bool(torch.isnan(ns5["out"][:P.bf_elems].float()).any()), "every bf16 element of the workspace is written before it is read"
    # 4 single items: 3 GEMMs per iteration; the two adjacent 64 x 128 items: one batched Gram + 2 x 2
    assert ns5["launches"] == 5 * (4 * 3 + 1 + 4)


def test_newton_schulz_tall_is_the_transpose_of_wide(ns5):
    wide, tall = 1, 2
    assert torch.equal(ns5["xs"][tall], ns5["xs"][wide].t())
    e_emu = ref.rel_err(ns5["emu"][tall], ns5["R"][tall])
    e = ref.rel_err(ns5["O"][tall], ns5["R"][wide].t())
    d = ref.rel_err(ns5["O"][tall], ns5["O"][wide].t())
    print(f"tall 192 x 64 against the transposed wide reference: {e:.4e} (2 e_emu = {2 * e_emu:.4e}); against the GPU's wide result: {d:.4e}")
    assert e <= 2 * e_emu and d <= 2 * e_emu


def test_newton_schulz_one_iteration_element_by_element(hip):
    P, xs, _, out, launches = _ns_run(hip, 1)
    assert launches == 4 * 3 + 1 + 4
    worst = []
    for i, (_, r, c) in enumerate(P.items):
        want = ref.ns_bf16_emulated(xs[i], 1).double()
        got = P.slot(out, i).double()
        u = (got - want).abs() / ref.ulp_bf16(want)
        worst.append(float(u.max()))
        print(f"item {i} [{r} x {c}]: one iteration, worst |X - X_emu| = {worst[-1]:.3f} bf16 ulps, {int((u > 0).sum())} of {u.numel()} elements differ")
        assert not torch.equal(ref.bits(P.slot(out, i)), ref.bits(xs[i]))
    assert max(worst) <= 2.0, worst


# ---------------------------------------------------------------------------------------------------- md_muon_axpby
@pytest.mark.parametrize("n,inplace", [(8, False), (4096, True), (8 * (2048 * 256 + 37), False)])
def test_axpby(hip, n, inplace):
    """One vector, one workgroup pass, and a second grid-stride pass of 37 threads; guard bands of 64 sentinel elements."""
    gen = torch.Generator().manual_seed(n)
    PAD = 64
    x = ref.poisoned(n + 2 * PAD, torch.bfloat16)
    y = ref.poisoned(n + 2 * PAD, torch.float32)
    x[PAD:PAD + n] = torch.randn(n, generator=gen).to(torch.bfloat16)
    y[PAD:PAD + n] = torch.randn(n, generator=gen) * 0.3
    out = ref.poisoned(n + 2 * PAD, torch.bfloat16)
    a = torch.tensor(A_, dtype=torch.float32)
    b = torch.tensor(C_, dtype=torch.float32)
    want = (a * x[PAD:PAD + n].float() + b * y[PAD:PAD + n]).to(torch.bfloat16)       # fp32: product, product, sum; then bf16
    xd, yd, od = x.cuda(), y.cuda(), out.cuda()
    dst = xd if inplace else od
    L = hip.lib()
    assert L.md_muon_axpby(xd.data_ptr() + 2 * PAD, yd.data_ptr() + 4 * PAD, dst.data_ptr() + 2 * PAD, A_, C_, n, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = dst.cpu()
    assert torch.equal(ref.bits(got[PAD:PAD + n]), ref.bits(want))
    for t, t0 in ((got, x if inplace else out), (yd.cpu(), y)):
        assert torch.equal(ref.bits(t[:PAD]), ref.bits(t0[:PAD])) and torch.equal(ref.bits(t[PAD + n:]), ref.bits(t0[PAD + n:])), "guard band written"
    assert torch.equal(ref.bits(yd.cpu()), ref.bits(y))
    if not inplace:
        assert torch.equal(ref.bits(xd.cpu()), ref.bits(x))
    before = dst.clone()
    for args in ((None, yd.data_ptr(), od.data_ptr(), n), (xd.data_ptr(), None, od.data_ptr(), n), (xd.data_ptr(), yd.data_ptr(), None, n),
                 (xd.data_ptr(), yd.data_ptr(), od.data_ptr(), 0), (xd.data_ptr(), yd.data_ptr(), od.data_ptr(), 12),
                 (xd.data_ptr() + 2, yd.data_ptr(), od.data_ptr(), 8), (xd.data_ptr(), yd.data_ptr() + 4, od.data_ptr(), 8)):
        assert L.md_muon_axpby(args[0], args[1], args[2], A_, C_, args[3], hip.stream_ptr()) == ref.BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(ref.bits(dst), ref.bits(before))


# ---------------------------------------------------------------------------------------------------- md_muon_apply
def _apply_problem(hip, seed):
    P = Problem(hip, seed=seed)
    gen = torch.Generator().manual_seed(seed + 100)
    ws = P.cpu["ws"]
    for i in range(P.n):
        s = P.slot(ws, i)
        s.copy_((torch.randn(s.shape, generator=gen) * 0.1).to(torch.bfloat16))
    P.dev["ws"] = ws.to(DEV)
    return P


@pytest.mark.parametrize("ema_mode", [0, 1, 2])
def test_apply(hip, ema_mode):
    assert ref.decay_is_unambiguous(LR, WD)
    P = _apply_problem(hip, 20 + ema_mode)
    if ema_mode == 1:                   # mode 1 must overwrite whatever the buffer held
        P.dev["ema"] = ref.poisoned(P.total, torch.float32).to(DEV)
        P.cpu["ema"] = P.dev["ema"].cpu()
    assert P.apply(ema_mode) == 0
    got = P.back()
    for i, (o, r, c) in enumerate(P.items):
        oo = P.slot(P.cpu["ws"], i).reshape(-1)
        pn, sh, e = ref.apply_ref(P.item("p", i), oo, LR, WD, P.scales[i], ema_mode, ES, P.item("ema", i))
        assert torch.equal(ref.bits(P.item("p", i, got)), ref.bits(pn)), f"item {i} [{r} x {c}]: p' differs from the reference bits"
        assert torch.equal(ref.bits(P.item("shadow", i, got)), ref.bits(sh)), f"item {i}: shadow"
        if ema_mode:
            assert torch.equal(ref.bits(P.item("ema", i, got)), ref.bits(e)), f"item {i}: ema (mode {ema_mode})"
        assert not torch.equal(P.item("p", i, got), P.item("p", i))
    if ema_mode == 0:
        assert torch.equal(ref.bits(got["ema"]), ref.bits(P.cpu["ema"]))
    P.outside_untouched(got, ("p", "shadow", "ema"))
    for k in ("g", "m", "gb", "ws"):
        assert torch.equal(ref.bits(got[k]), ref.bits(P.cpu[k])), f"{k} is not this pass's to write"


@pytest.mark.parametrize("ema_mode", [0, 1, 2])
def test_apply_guard_zero(hip, ema_mode):
    P = _apply_problem(hip, 30 + ema_mode)
    assert P.apply(ema_mode, guard=_flag(0)) == 0
    got = P.back()
    assert torch.equal(ref.bits(got["p"]), ref.bits(P.cpu["p"])), "p must stay bit-identical on a skipped step"
    assert torch.equal(ref.bits(got["shadow"])[P.mask], ref.bits(P.cpu["p"].to(torch.bfloat16))[P.mask]), "the shadow is re-emitted from p"
    if ema_mode == 1:
        assert torch.equal(ref.bits(got["ema"])[P.mask], ref.bits(P.cpu["p"])[P.mask])
    else:
        assert torch.equal(ref.bits(got["ema"]), ref.bits(P.cpu["ema"])), "a live EMA must stay bit-identical on a skipped step"
    P.outside_untouched(got, ("p", "shadow", "ema"))
    # guard 1 is the plain launch
    Q, R = _apply_problem(hip, 30 + ema_mode), _apply_problem(hip, 30 + ema_mode)
    assert Q.apply(ema_mode, guard=_flag(1)) == 0 and R.apply(ema_mode) == 0
    a, b = Q.back(), R.back()
    assert all(torch.equal(ref.bits(a[k]), ref.bits(b[k])) for k in a)


# ---------------------------------------------------------------------------------------------------- bad arguments
def _broken_tables(hip, P):
    """name -> a host table with one misfit (the device table is never read on a refused call)."""
    def table(edit):
        t = (hip.MuonItem * P.n)(*[hip.MuonItem(it.flat_off, it.rows, it.cols, it.ws_off, it.scale, 0) for it in P.host])
        edit(t)
        return t
    return {"unaligned offset": table(lambda t: setattr(t[1], "flat_off", t[1].flat_off + 4)),
            "negative offset": table(lambda t: setattr(t[0], "flat_off", -8)),
            "rows not a multiple of 64": table(lambda t: setattr(t[3], "rows", 96)),
            "cols not a multiple of 64": table(lambda t: setattr(t[2], "cols", 72)),
            "zero rows": table(lambda t: setattr(t[0], "rows", 0)),
            "ws_off not md_muon_ws_bytes'": table(lambda t: setattr(t[2], "ws_off", t[2].ws_off + 8)),
            "ws_off never written": table(lambda t: [setattr(it, "ws_off", 0) for it in t])}


def test_bad_arguments_launch_nothing(hip):
    P = _apply_problem(hip, 40)
    calls = []
    for why, t in _broken_tables(hip, P).items():
        calls += [(f"momentum: {why}", lambda t=t: P.momentum(False, True, 1.0, None, 0.0, host=t)),
                  (f"newton_schulz: {why}", lambda t=t: P.newton_schulz(5, host=t)[0]),
                  (f"apply: {why}", lambda t=t: P.apply(2, host=t))]
    for k in ("g", "m", "table", "host", "ws", "partials", "norms"):
        calls.append((f"momentum: {k} NULL", lambda k=k: P.momentum(False, True, 1.0, None, 0.0, **{k: None})))
    for k in ("p", "shadow", "table", "host", "ws", "ema"):
        calls.append((f"apply: {k} NULL", lambda k=k: P.apply(2, **{k: None})))
    for k in ("host", "ws"):
        calls.append((f"newton_schulz: {k} NULL", lambda k=k: P.newton_schulz(5, **{k: None})[0]))
    calls += [("momentum: n = 0", lambda: P.momentum(False, True, 1.0, None, 0.0, n=0)),
              ("momentum: mu = 1", lambda: P.momentum(False, True, 1.0, None, 0.0, mu=1.0)),
              ("momentum: misaligned m", lambda: P.momentum(False, True, 1.0, None, 0.0, m=P.dev["m"].data_ptr() + 4)),
              ("momentum: misaligned bf16 g", lambda: P.momentum(True, True, 1.0, None, 0.0, gb=P.dev["gb"].data_ptr() + 2)),
              ("apply: misaligned shadow", lambda: P.apply(0, shadow=P.dev["shadow"].data_ptr() + 8)),
              ("apply: ema_mode 3", lambda: P.apply(3)),
              ("newton_schulz: steps 0", lambda: P.newton_schulz(0)[0]), ("newton_schulz: steps 9", lambda: P.newton_schulz(9)[0]),
              ("newton_schulz: misaligned ws", lambda: P.newton_schulz(5, ws=P.dev["ws"].data_ptr() + 2)[0])]
    for why, call in calls:
        assert call() == ref.BAD_ARG, why
    need = ctypes.c_int64(-3)
    L = hip.lib()
    for why, t in _broken_tables(hip, P).items():
        if "ws_off" not in why:
            assert L.md_muon_ws_bytes(t, P.n, ctypes.byref(need)) == ref.BAD_ARG, why
    assert L.md_muon_ws_bytes(None, P.n, ctypes.byref(need)) == ref.BAD_ARG and L.md_muon_ws_bytes(P.host, P.n, None) == ref.BAD_ARG
    assert L.md_muon_ws_bytes(P.host, 0, ctypes.byref(need)) == ref.BAD_ARG and need.value == -3
    got = P.back()
    for k in got:
        assert torch.equal(ref.bits(got[k]), ref.bits(P.cpu[k])), f"{k} was written by a refused call"
    assert bool((P.norms == -7.0).all()) and bool((P.partials == -7.0).all())
    assert P.apply(0, ema=None) == 0            # mode 0 does not need the buffer
    torch.cuda.synchronize()
