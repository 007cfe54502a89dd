"""tests/optim_ref.py checked on the CPU: the storage helper, the constants, the range tables, every case through the fp64 model,
the bounds against two fp32 emulations of the kernels' statement order, and the sharpness of the checker.

Every case of the tables runs through the fp64 emulators in place of the kernels: all properties must hold and every fence must be
intact.  Then an fp32 torch emulation of the kernel's statements runs through the same checker, once with multiply and add separate
and once with the multiply-adds fused: the worst error / bound per array must stay <= 1 (printed; measured, unfused / fused:
m 0.977 / 0.576, v 0.689 / 0.689, p 0.985 / 0.937, ema 0.997 / 0.556, EMA-power profiles 0.989 / 0.857, md_sumsq 0.063 -- the worst
of 8.4 M elements comes within a few percent of the counted worst case, so no count has slack to give away).

Then the emulator is broken one thing at a time (MUTATIONS) and the checker must reject every mutation on every case named next to
it.  test_old_rule_misses evaluates the rule the suite had before (p alone, rtol 1e-5, atol 1e-6 against an fp32 reference) on the
same mutated results and asserts that it ACCEPTS at least: decay after the update at production hyperparameters (step 1), 1 - beta2
taken as 0.001 (step 1000), every mutation that only touches m or v (stale m, stale v, guard = 0 still updating m), and the EMA
and shadow mutations it never looked at.
"""
import numpy as np
import pytest
import torch

from tests import optim_ref as ox


def _ok(problems):
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------ helpers and tables
def test_constants_match_the_binding():
    from micro_diffusion_amd import hip
    assert (ox.SUMSQ_PARTIALS, ox.MAX_RANGES, ox.EMA_MAX) == (hip.SUMSQ_PARTIALS, hip.ADAMW_MAX_RANGES, hip.EMA_MAX_PROFILES)
    fields = [f[0] for f in hip.AdamWArgs._fields_]
    assert set(ox.scalar_fields(ox.HPS["loud"])) <= set(fields)
    call = ox.AdamProblem(ox.ADAM_BY_NAME["f32-ema2-loud-n1028"]).call()
    assert set(fields) <= set(call), set(fields) - set(call)


def test_buf_fences_and_restore():
    b = ox.Buf(12, torch.float32, values=torch.arange(12.0))
    assert b.fence_ok() and b.untouched() and b.ptr() % 16 == 0 and int(b.raw[0]) == ox.SENT_F32 and int(b.raw[-1]) == ox.SENT_F32
    b.body[3] = 7.0
    assert b.fence_ok() and not b.untouched()
    b.typed[b.lead + 12] = 0.0                               # the element just past the end
    assert not b.fence_ok()
    b.restore()
    b.raw[b.lead - 1] = 0x7FC00000                           # another NaN just before the start: a bitwise change
    assert not b.fence_ok()
    h = ox.Buf(8, torch.bfloat16)
    assert int(h.raw[h.lead]) == ox.SENT_BF16 and bool(torch.isnan(h.body.float()).all()) and h.ptr() % 16 == 0
    # clamped reads and dropped writes of the emulators
    idx = torch.tensor([-1000, 0, 11, 10 ** 6])
    assert b.read(idx, torch.float64).shape == (4,)
    b.restore()
    b.write(idx, torch.tensor([1.0, 2.0, 3.0, 4.0]))
    assert b.body[0] == 2.0 and b.body[11] == 3.0 and b.fence_ok()


def test_hyperparameters_have_one_bit_pattern_per_constant():
    for name, hp in ox.HPS.items():
        assert ox.decay_is_unambiguous(hp), name
        assert float(np.log2(hp.gs)).is_integer(), "grad_scale is a power of two: sqrt(ss) * gs + 1e-6 rounds once either way"
    loud = ox.scalar_fields(ox.HPS["loud"])
    assert len(set(loud.values())) == len(loud) == 10
    # 1.f - 0.999f is not 0.001: the constant the model must reproduce
    k = ox.kernel_constants(ox.HPS["prod1000"])
    assert k.omb2 == float(np.float32(1) - np.float32(0.999)) and abs(k.omb2 - 0.001) > 1e-8
    assert k.decay == float(np.float32(1) - np.float32(2.4e-4) * np.float32(0.1))
    assert k.step == float(np.float32(2.4e-4) / np.float32(1 - 0.9 ** 1000))
    assert abs(k.isb - (1 - 0.999 ** 1000) ** -0.5) < 4 * ox.U * k.isb and k.isb == float(np.float32(k.isb))
    assert k.coef == 1.0                                     # sumsq == NULL


@pytest.mark.parametrize("hp", ["prod1000", "loud"])
def test_clip_edges(hp):
    h = ox.HPS[hp]
    mx = h.max_norm
    x = {w: ox.clip_x(h, ox.clip_edge_ss(h, w)) for w in ("below", "at", "above")}
    assert x["below"] < mx and x["at"] == mx and x["above"] > mx
    assert abs(float(x["below"]) - h.max_norm) < 4e-7 * h.max_norm and abs(float(x["above"]) - h.max_norm) < 4e-7 * h.max_norm
    coef = {w: ox.kernel_constants(h, ox.clip_edge_ss(h, w)).coef for w in x}
    assert coef["below"] == coef["at"] == h.gs and coef["above"] < h.gs
    assert ox.kernel_constants(h, 0.0).coef == h.gs and ox.kernel_constants(h, 1e6, max_norm=0.0).coef == h.gs
    assert ox.kernel_constants(h, None).coef == h.gs


def test_range_tables():
    seen = set()
    for name, (off, cnt) in ox.RANGE_TABLES.items():
        d = dict(entry="ema_ranges", p=16, ema=[16], beta=[0.5], n_profiles=1, flat_off=off, count=cnt, n_ranges=len(off))
        assert ox.contract_accepts(d), name
        spans = sorted((o, o + c) for o, c in zip(off, cnt))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), f"{name}: ranges overlap"
        if name != "rbig":
            assert torch.equal(ox.range_lookup(off, cnt), ox.direct_index(off, cnt)), name
            seen |= set(cnt)
            for mut in ("range_lt", "last_range_never"):
                assert (len(off) == 1) == torch.equal(ox.range_lookup(off, cnt, mut=mut), ox.direct_index(off, cnt)), (name, mut)
    assert seen == {4, 8, 60, 64, 68, 1028}
    assert sorted(len(t[0]) for t in ox.RANGE_TABLES.values()) == [1, 2, 2, 3, 64]
    off, cnt = ox.RANGE_TABLES["r64"]
    spans = sorted((o, o + c) for o, c in zip(off, cnt))
    gaps = {b[0] - a[1] for a, b in zip(spans, spans[1:])}
    assert gaps == {0, 4} and off != sorted(off) and off != sorted(off, reverse=True)
    assert ox.RANGE_TABLES["r2-touch-desc"][0] == sorted(ox.RANGE_TABLES["r2-touch-desc"][0], reverse=True)
    # rbig: the boundary between its two ranges lies inside the second grid-stride pass
    off, cnt = ox.RANGE_TABLES["rbig"]
    first = 4 * ox.GRID_CAP * 256
    assert first < cnt[0] < sum(cnt) and sum(cnt) == ox.N_LARGE and (sum(cnt) - first) // 4 == 37


def test_case_tables_cover_what_they_must():
    forms = {(c.gbf16, c.ema_mode) for c in ox.ADAM_FLAT}
    assert forms == {(g, m) for g in (False, True) for m in (0, 1, 2)}
    assert {c.ema_mode for c in ox.ADAM_RANGES} == {0, 1, 2} and {c.ranges for c in ox.ADAM_RANGES} == set(ox.SMALL_TABLES)
    assert {c.n for c in ox.ADAM_FLAT} == set(ox.SIZES) and {c.hp for c in ox.ADAM_FLAT} >= {"prod1", "prod1000", "loud"}
    assert {c.clip for c in ox.ADAM_FLAT} == {"null", "maxnorm0", "ss0", "below", "at", "above", "clipped", "unclipped"}
    assert {len(c.betas) for c in ox.EMA_CASES} == {1, 2, 3, 4} and {c.guard for c in ox.EMA_CASES} == {None, 0, 1}
    assert all(0.0 in c.betas for c in ox.EMA_CASES if len(c.betas) > 1)
    assert {c.n for c in ox.SUMSQ_CASES} == set(ox.SUMSQ_SIZES)
    assert sum(c.n >= ox.N_LARGE or c.ranges == "rbig" for c in ox.ADAM_ALL) == 3
    n = ox.N_SUMSQ_2PASS
    assert ox.single_positions() == [0, 7, 8, 2047, 2048, 8 * 262144 - 1, 8 * 262144, n - 1]


# ------------------------------------------------------------------------------------------------ every case through the models
WORST = {}


def _note(kind, arith, ratios):
    for k, r in ratios.items():
        key = (kind, arith, k[0] if k.startswith("e") and k[1:].isdigit() else k)
        WORST[key] = max(WORST.get(key, 0.0), r)


SMALL_ADAM = ox.ADAM_FLAT + ox.ADAM_RANGES + ox.ADAM_GUARD0


@pytest.mark.parametrize("arith", ["f64", "f32", "f32fma"])
@pytest.mark.parametrize("case", SMALL_ADAM, ids=[c.name for c in SMALL_ADAM])
def test_adamw_model(case, arith):
    P = ox.AdamProblem(case)
    assert ox.contract_accepts(P.call())
    ox.adamw_emulate(P, arith)
    problems, ratios, _ = ox.adamw_check(P)
    print(case.name, arith, {k: round(v, 3) for k, v in ratios.items()})
    _ok(problems)
    _note("adamw", arith, ratios)


@pytest.mark.parametrize("case", ox.EMA_CASES, ids=[c.name for c in ox.EMA_CASES])
def test_ema_model(case):
    for arith in ("f64", "f32", "f32fma"):
        P = ox.EmaProblem(case)
        assert ox.contract_accepts(P.call())
        ox.ema_emulate(P, arith)
        problems, ratios = ox.ema_check(P)
        print(case.name, arith, {k: round(v, 3) for k, v in ratios.items()})
        _ok(problems)
        _note("ema_power", arith, ratios)


ALL_SUMSQ = ox.SUMSQ_CASES + ox.NONFINITE_CASES


@pytest.mark.parametrize("case", ALL_SUMSQ, ids=[c.name for c in ALL_SUMSQ])
def test_sumsq_model(case):
    P = ox.SumsqProblem(case)
    for arith in ("f64", "f32"):
        P.restore()
        ox.sumsq_pipeline_emulate(P, arith)
        problems, ratio = ox.sumsq_check(P)
        if ratio is not None:
            print(case.name, arith, f"error / bound {ratio:.3g} (D = {ox.sumsq_depth(case.n)})")
            _note("sumsq", arith, {"sum": ratio})
        _ok(problems)


@pytest.mark.parametrize("count", ox.FINISH_COUNTS)
def test_finish_model(count):
    for arith in ("f64", "f32"):
        P = ox.FinishProblem(count)
        ox.finish_emulate(P.bufs["partials"].body, count, P.bufs["out"].body, arith)
        _ok(P.check())
    if count % 256 and count > 256:
        P = ox.FinishProblem(count)
        ox.finish_emulate(P.bufs["partials"].body, count, P.bufs["out"].body, "f32", mut="drop_past_256")
        assert P.check(), "dropping the element past a multiple of 256 must show"
    # reading one element past the end meets the NaN fence
    P = ox.FinishProblem(count)
    ox.finish_emulate(P.bufs["partials"].typed[P.bufs["partials"].lead:], count + 1, P.bufs["out"].body, "f32")
    assert P.check()


@pytest.mark.parametrize("n", ox.CHECKSUM_SIZES)
def test_checksum_reference(n):
    P = ox.ChecksumProblem(n)
    w = P.bufs["x"].bits.numpy().view(np.uint16)
    assert w[-1] == 0xFFFF
    P.bufs["out"].body[:] = torch.from_numpy(ox.checksum_ref(w).view(np.int64))
    _ok(P.check())
    # one flipped bit, two swapped words, a skipped last word: each changes the reference
    v = w.copy()
    v[n // 2] ^= 1
    assert (ox.checksum_ref(v) != P.want).all()
    v = w.copy()
    v[[0, n - 1]] = v[[n - 1, 0]]
    assert ox.checksum_ref(v)[0] == P.want[0] and ox.checksum_ref(v)[1] != P.want[1]
    assert (ox.checksum_ref(w[:-1]) != P.want).all()
    if n > 8:                                                # the geometry the large size is there for: a ragged second pass
        assert n // 8 - ox.CHECKSUM_CAP * 256 == 37


def test_large_cases_and_second_pass_mutations():
    """The three AdamW launches and the EMA-power launch at the large size, through the fp64 model, the fp32 emulation and the two
    mutations only this size can show."""
    for case, muts in ((ox.ADAM_FLAT_LARGE, ("second_pass_dropped", "second_pass_twice")), (ox.ADAM_GUARD0_LARGE, ("second_pass_dropped",)),
                       (ox.ADAM_RANGES_LARGE, ("second_pass_dropped", "range_lt"))):
        P = ox.AdamProblem(case)
        for arith in ("f64", "f32"):
            P.restore()
            ox.adamw_emulate(P, arith)
            problems, ratios, _ = ox.adamw_check(P)
            print(case.name, arith, {k: round(v, 3) for k, v in ratios.items()})
            _ok(problems)
            _note("adamw", arith, ratios)
        for mut in muts:
            P.restore()
            ox.adamw_emulate(P, "f64", mut)
            assert ox.adamw_check(P)[0], f"{mut} must show on {case.name}"
    P = ox.EmaProblem(ox.EMA_LARGE)
    ox.ema_emulate(P, "f32")
    problems, ratios = ox.ema_check(P)
    _ok(problems)
    _note("ema_power", "f32", ratios)
    P.restore()
    ox.ema_emulate(P, "f64", "second_pass_dropped")
    assert ox.ema_check(P)[0]


# ------------------------------------------------------------------------------------------------ mutations
def _ranges(table):
    return [c.name for c in ox.ADAM_RANGES if c.ranges == table and c.shadow and c.guard is None]


LOUD, PROD = "f32-ema2-loud-n1028", "f32-ema2-prod1000-n1028"
# mutation -> the cases on which the checker must reject it (the loud case always; the production case where the issue asks for it)
MUTATIONS = {
    "decay_after": [LOUD, PROD, "bf16-ema0-prod1-n1028"],
    "decay_dropped": [LOUD, PROD],
    "betas_swapped": [LOUD, PROD],
    "omb2_exact": [LOUD, PROD],
    "eps_in_sqrt": [LOUD, PROD],
    "bc2_on_v": [LOUD, PROD],
    "clip_unscaled_norm": ["clip-clipped-loud"],
    "coef_missing_gs": ["clip-clipped-loud", "clip-unclipped-loud"],
    "min_dropped": ["clip-unclipped-loud", "clip-ss0-prod1000"],
    "ema_pre_update": [LOUD, PROD],
    "ema1_blend": ["f32-ema1-loud-n1028", "bf16-ema1-prod1000-n1028"],
    "shadow_old_p": [LOUD, PROD],
    "m_stale": [LOUD, PROD],
    "v_stale": [LOUD, PROD],
    "g_flat_index": [n for t in ox.SMALL_TABLES for n in _ranges(t)],
    "shadow_flat_index": [n for t in ox.SMALL_TABLES for n in _ranges(t)],
    "range_lt": _ranges("r2-touch-desc") + _ranges("r3-gap4-mixed") + _ranges("r64"),
    "last_range_never": _ranges("r2-touch-desc") + _ranges("r3-gap4-mixed") + _ranges("r64"),
    "guard0_updates_m": ["guard0-f32-ema0", "guard0-bf16-ema2", "guard0-ranges-r64-ema1"],
    "guard0_no_zero_g": ["guard0-f32-ema0", "guard0-bf16-ema1"],
    "guard0_no_shadow": ["guard0-f32-ema2", "guard0-ranges-r64-ema0"],
}
MUT_TABLE = [(m, n) for m, names in MUTATIONS.items() for n in names]
OLD_RULE = {}


def _mutated(mut, name):
    P = ox.AdamProblem(ox.ADAM_BY_NAME[name])
    if mut in ("m_stale", "v_stale"):
        ox.adamw_emulate(P, "f64")
        P.bufs[mut[0]].restore()
    else:
        ox.adamw_emulate(P, "f64", mut)
    return ox.adamw_check(P)


@pytest.mark.parametrize("mut,name", MUT_TABLE, ids=[f"{m}@{n}" for m, n in MUT_TABLE])
def test_adamw_mutation_is_rejected(mut, name):
    problems, ratios, old_ok = _mutated(mut, name)
    OLD_RULE[(mut, name)] = old_ok
    print(f"{mut} @ {name}: old rule {'ACCEPTS' if old_ok else 'rejects'}; new: {problems[:2]}")
    assert problems, f"{mut} passed the checker on {name}"


def test_old_rule_misses():
    """What the rule the suite had (p alone, rtol 1e-5, atol 1e-6) says about the same mutated results."""
    for mut, name in MUT_TABLE:
        if (mut, name) not in OLD_RULE:
            OLD_RULE[(mut, name)] = _mutated(mut, name)[2]
    accepted = sorted(k for k, ok in OLD_RULE.items() if ok)
    print("the old rule accepts:", *[f"  {m} @ {n}" for m, n in accepted], sep="\n")
    must = [("decay_after", "bf16-ema0-prod1-n1028"), ("omb2_exact", PROD),
            ("m_stale", LOUD), ("m_stale", PROD), ("v_stale", LOUD), ("v_stale", PROD), ("ema_pre_update", LOUD), ("shadow_old_p", LOUD)]
    must += [("guard0_updates_m", n) for n in MUTATIONS["guard0_updates_m"]]
    missing = [k for k in must if k not in accepted]
    assert not missing, missing


@pytest.mark.parametrize("mut,name", [("skip_last_vector", "f32-exact-n8"), ("skip_last_vector", "bf16-exact-n16777512"),
                                      ("skip_last_vector", "f32-single-16777511"), ("skip_last_vector", "bf16-randn-n2056"),
                                      ("idle_wg_no_write", "f32-exact-n8"), ("idle_wg_no_write", "bf16-exact-n2056")])
def test_sumsq_mutation_is_rejected(mut, name):
    name = name.replace("16777512", str(ox.N_SUMSQ_2PASS)).replace("16777511", str(ox.N_SUMSQ_2PASS - 1))
    P = ox.SumsqProblem(ox.SUMSQ_BY_NAME[name])
    ox.sumsq_pipeline_emulate(P, "f32", mut)
    assert ox.sumsq_check(P)[0], f"{mut} passed on {name}"


def test_sumsq_writes_only_its_slot_and_guard_keeps_reserved_words():
    P = ox.SumsqProblem(ox.SUMSQ_BY_NAME["f32-exact-n8"])
    ox.sumsq_pipeline_emulate(P)
    P.bufs["partials"].body[0] = 0.0                         # another call's slot
    assert ox.sumsq_check(P)[0]
    P.restore()
    ox.sumsq_pipeline_emulate(P)
    P.bufs["state"].body[2] = 0
    assert ox.sumsq_check(P)[0]


@pytest.mark.parametrize("mut,name", [("beta0_reads", "K2-n1028"), ("beta0_reads", "K1-beta0-n1028"), ("range_lt", "K3-ranges-r64"),
                                      ("last_range_never", "K2-ranges-r2-touch-desc")])
def test_ema_mutation_is_rejected(mut, name):
    P = ox.EmaProblem(ox.EMA_BY_NAME[name])
    ox.ema_emulate(P, "f64", mut)
    assert ox.ema_check(P)[0]


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def refusal_base():
    return ox.RefusalBase()


@pytest.mark.parametrize("name,base,change", ox.REFUSALS, ids=[r[0] for r in ox.REFUSALS])
def test_refusal_table_follows_the_header(refusal_base, name, base, change):
    call, _ = refusal_base.base(base)
    assert ox.contract_accepts(call), f"the base call of {name} must be accepted"
    before = dict(call)
    change(call)
    assert call != before and not ox.contract_accepts(call), name


def test_print_worst_ratios():
    """(Runs last: the worst error / bound per array over every case above.)"""
    for k in sorted(WORST):
        print(f"{k[0]:10s} {k[1]:7s} {k[2]:4s} worst error / bound = {WORST[k]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
