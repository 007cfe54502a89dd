"""The optimizer tail on the GPU -- md_sumsq / md_sumsq_finish, md_step_guard, md_adamw_step[_ranges][_guarded],
md_ema_power_update[_ranges], md_checksum_u16 -- against tests/optim_ref.py: the tables, references and bounds the CPU test
(tests/test_optim_ref_cpu.py) validates, through the real entry points.

  * reductions on inputs whose sum has no rounding error: one bit pattern, torch.equal; general inputs within g_D * sum g^2 with D
    the longest chain of roundings of the kernel's geometry; non-finite inputs and a finite gradient whose sum of squares overflows
    give NaN / +Inf, and md_step_guard then clears the go flag and counts the step;
  * md_sumsq runs into the middle slot of a sentinel-filled three-slot partials buffer: all 1024 partials written (also at n = 8),
    nothing outside them;
  * AdamW: m, v, p, ema per element within the counted-rounding bounds of optim_ref (no rtol, no atol) of an fp64 reference built
    on the kernel's own fp32 constants; shadow bit for bit the bf16 of the kernel's p; g bit-zero; mode-1 ema a bit copy of p;
    elements with g = m = v = 0 exactly fl(p * decay); everything outside the ranges, every input and every fence bit-identical;
  * every launch runs twice from the same state and must give identical bits;
  * refusals from the header: MD_BAD_ARG and every buffer untouched -- null pointers, sizes, modes, range tables, betas, and the
    pointer alignment md_sumsq and md_adamw_step* now check (16 bytes on fp32 buffers and md_sumsq's input, 8 on g_bf16 / shadow).

Five launches run at the large size, n = 4 * (8192 * 256 + 37) (a second grid-stride pass of 37 threads): AdamW flat, the guard-0
skip loop, the range form with a range boundary inside the second pass, EMA-power with K = 3, and the checksum (its own cap).

Worst error / bound measured on the MI355X over every case (the margin a later kernel change has to stay inside; the unfused fp32
emulation of the CPU test reaches 0.98 to 1.00 on every array, so the bounds are tight, not padded):
    AdamW      m 0.977   v 0.689   p 0.499   ema 0.556    (p and ema match the fused emulation: the compiler contracts p * decay - q)
    EMA-power  profiles 0.989 (K = 3 at the large size)
    md_sumsq   0.063 of g_D * sum g^2 (D = 29 or 37)
No kernel produced a wrong bit, touched a fence or failed to repeat its bits on any case; no refusal was missing once md_sumsq and
md_adamw_step* checked pointer alignment (before, a pointer off by 4 or 8 bytes went straight into 16-byte vector accesses).

What the GPU run showed that the CPU emulation had not: the first version of the reference formed the clip chain with float32 torch
operations on the host, and on the host that GPU run used torch.sqrt(float32) returned 0.24999902 (one ulp high) for ss = 0.062499505
where the kernel, numpy and fp64 all give 0.24999900 -- the 'above' clip edge then sat exactly AT max_norm for the kernel and the
reference clipped where the kernel did not (v at 1.01 of its bound).  The kernel was right.  optim_ref.r32 now forms every constant
in fp64 and rounds to fp32 after each operation, which is provably the correctly rounded fp32 result on any host.
"""
import ctypes

import pytest
import torch

from tests import optim_ref as ox

pytestmark = pytest.mark.gpu
dev = "cuda"
WORST = {}


def _note(kind, ratios):
    for k, r in ratios.items():
        key = (kind, "e" if k.startswith("e") and k[1:].isdigit() else k)
        WORST[key] = max(WORST.get(key, 0.0), r)


def _ok(problems):
    assert not problems, "\n".join(problems)


def _i64(v):
    return None if v is None else (ctypes.c_int64 * max(len(v), 1))(*v)


def launch(hip, d):
    """One call, given as the dict optim_ref builds, through the C entry point it names; returns the code."""
    L, st = hip.lib(), hip.stream_ptr()
    e = d["entry"]
    if e == "sumsq":
        return L.md_sumsq(d["g"], d["bf16"], d["n"], d["partials"], st)
    if e == "finish":
        return L.md_sumsq_finish(d["partials"], d["count"], d["out"], st)
    if e == "guard":
        return L.md_step_guard(d["sumsq"], d["state"], st)
    if e == "checksum":
        return L.md_checksum_u16(d["x"], d["n"], d["out"], st)
    if e in ("adamw", "adamw_ranges"):
        a = hip.AdamWArgs(**{f[0]: d[f[0]] for f in hip.AdamWArgs._fields_})
        if e == "adamw":
            return L.md_adamw_step_guarded(ctypes.byref(a), d["guard"], st) if d["guarded"] else L.md_adamw_step(ctypes.byref(a), st)
        fo, cn = _i64(d["flat_off"]), _i64(d["count"])
        if d["guarded"]:
            return L.md_adamw_step_ranges_guarded(ctypes.byref(a), fo, cn, d["n_ranges"], d["guard"], st)
        return L.md_adamw_step_ranges(ctypes.byref(a), fo, cn, d["n_ranges"], st)
    ev = None if d["ema"] is None else (ctypes.c_void_p * len(d["ema"]))(*d["ema"])
    bv = None if d["beta"] is None else (ctypes.c_float * len(d["beta"]))(*d["beta"])
    if e == "ema":
        return L.md_ema_power_update(d["p"], ev, bv, d["n_profiles"], d["n"], d["guard"], st)
    return L.md_ema_power_update_ranges(d["p"], ev, bv, d["n_profiles"], _i64(d["flat_off"]), _i64(d["count"]), d["n_ranges"], d["guard"], st)


def _twice(P, run):
    """Run, keep the bits, put the initial state back, run again: the bits must agree.  The second result stays in the buffers."""
    run()
    torch.cuda.synchronize()
    first = {k: b.raw.clone() for k, b in P.bufs.items()}
    P.restore()
    run()
    torch.cuda.synchronize()
    diff = [k for k, b in P.bufs.items() if not torch.equal(b.raw, first[k])]
    assert not diff, f"two launches from the same state differ in {diff}"


# ------------------------------------------------------------------------------------------------ reductions
def _sumsq_pipeline(hip, P):
    B, c = P.bufs, P.case
    slot = B["partials"].ptr(ox.SLOT * ox.SUMSQ_PARTIALS)

    def run():
        assert launch(hip, dict(entry="sumsq", g=B["g"].ptr(), bf16=int(c.bf16), n=c.n, partials=slot)) == 0
        assert launch(hip, dict(entry="finish", partials=slot, count=ox.SUMSQ_PARTIALS, out=B["out"].ptr())) == 0
        assert launch(hip, dict(entry="guard", sumsq=B["out"].ptr(), state=B["state"].ptr())) == 0
    _twice(P, run)
    problems, ratio = ox.sumsq_check(P)
    if ratio is not None:
        print(f"sumsq {c.name}: error / bound = {ratio:.3g} (D = {ox.sumsq_depth(c.n)})")
        _note("sumsq", {"sum": ratio})
    _ok(problems)


@pytest.mark.parametrize("case", ox.SUMSQ_CASES, ids=[c.name for c in ox.SUMSQ_CASES])
def test_sumsq(hip, case):
    _sumsq_pipeline(hip, ox.SumsqProblem(case, dev))


@pytest.mark.parametrize("case", ox.NONFINITE_CASES, ids=[c.name for c in ox.NONFINITE_CASES])
def test_sumsq_nonfinite_then_guard(hip, case):
    _sumsq_pipeline(hip, ox.SumsqProblem(case, dev))


@pytest.mark.parametrize("count", ox.FINISH_COUNTS)
def test_sumsq_finish(hip, count):
    P = ox.FinishProblem(count, dev)
    call = dict(entry="finish", partials=P.bufs["partials"].ptr(), count=count, out=P.bufs["out"].ptr())
    _twice(P, lambda: _ok([] if launch(hip, call) == 0 else ["md_sumsq_finish refused"]))
    _ok(P.check())


@pytest.mark.parametrize("n", ox.CHECKSUM_SIZES)
def test_checksum(hip, n):
    P = ox.ChecksumProblem(n, dev)
    call = dict(entry="checksum", x=P.bufs["x"].ptr(), n=n, out=P.bufs["out"].ptr())
    _twice(P, lambda: _ok([] if launch(hip, call) == 0 else ["md_checksum_u16 refused"]))
    _ok(P.check())


# ------------------------------------------------------------------------------------------------ AdamW
def _adamw(hip, case):
    P = ox.AdamProblem(case, dev)
    call = P.call()
    assert ox.contract_accepts(call)
    _twice(P, lambda: _ok([] if launch(hip, call) == 0 else [f"{case.name}: refused"]))
    problems, ratios, _ = ox.adamw_check(P)
    print(f"adamw {case.name}:", {k: round(v, 3) for k, v in ratios.items()})
    _note("adamw", ratios)
    _ok(problems)


FLAT = ox.ADAM_FLAT + [ox.ADAM_FLAT_LARGE]
RANGES = ox.ADAM_RANGES + [ox.ADAM_RANGES_LARGE]
GUARD0 = ox.ADAM_GUARD0 + [ox.ADAM_GUARD0_LARGE]


@pytest.mark.parametrize("case", FLAT, ids=[c.name for c in FLAT])
def test_adamw_flat(hip, case):
    _adamw(hip, case)


@pytest.mark.parametrize("case", RANGES, ids=[c.name for c in RANGES])
def test_adamw_ranges(hip, case):
    _adamw(hip, case)


@pytest.mark.parametrize("case", GUARD0, ids=[c.name for c in GUARD0])
def test_adamw_guard0(hip, case):
    _adamw(hip, case)


# ------------------------------------------------------------------------------------------------ EMA power
EMA = ox.EMA_CASES + [ox.EMA_LARGE]


@pytest.mark.parametrize("case", EMA, ids=[c.name for c in EMA])
def test_ema_power(hip, case):
    P = ox.EmaProblem(case, dev)
    call = P.call()
    assert ox.contract_accepts(call)
    _twice(P, lambda: _ok([] if launch(hip, call) == 0 else [f"{case.name}: refused"]))
    problems, ratios = ox.ema_check(P)
    print(f"ema_power {case.name}:", {k: round(v, 3) for k, v in ratios.items()})
    _note("ema_power", ratios)
    _ok(problems)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def refusal_base():
    return ox.RefusalBase(dev)


@pytest.mark.parametrize("name,base,change", ox.REFUSALS, ids=[r[0] for r in ox.REFUSALS])
def test_refusal(hip, refusal_base, name, base, change):
    call, bufs = refusal_base.base(base)
    change(call)
    assert not ox.contract_accepts(call)
    rc = launch(hip, call)
    torch.cuda.synchronize()
    assert rc == ox.BAD_ARG, f"{name}: the header refuses this call, the entry point returned {rc}"
    assert [k for k, b in bufs.items() if not b.untouched()] == [], f"{name}: a refused call wrote memory"


def test_print_worst_ratios():
    """(Runs last: the worst error / bound per array over the cases above.)"""
    for k in sorted(WORST):
        print(f"{k[0]:10s} {k[1]:4s} worst error / bound = {WORST[k]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
