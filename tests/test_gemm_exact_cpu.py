"""tests/gemm_exact.py checked on the CPU: the storage helper, every case's reference and its preconditions, the case table, and
the sharpness of the comparison.

Every case of the table runs through gemm_exact.emulate -- an fp64 model of the md_gemm_bf16 contract that addresses memory
through the struct's pointers, leading dimensions and strides alone -- in place of the kernel: the exact comparison must pass and
every fence must be intact.  Then the model is broken one thing at a time and the comparison must reject each mutation.

Mutations, and what the old rule (|err| <= 2e-2 * max|ref| + 1e-3 on Gaussian operands, dense leading dimensions) says about the same
mutation at the same shape (264 x 136 x 1024, gated residual + bias + raw copy; test_old_rule_accepts prints and asserts this list):
    drop one k element in one row                     exact: rejected     old rule: ACCEPTED
    double-count the element at a split boundary      exact: rejected     old rule: ACCEPTED
    roll the gate by one sample                       exact: rejected     old rule: rejected
    roll the bias by one column                       exact: rejected     old rule: rejected (bias of order 1; ACCEPTED below ~2 % of max|ref|)
    swap ldr with ldc2                                exact: rejected     old rule: ACCEPTED (every leading dimension was N: the swap is a no-op)
    truncate instead of rounding to nearest           exact: rejected     old rule: ACCEPTED
Truncation is invisible on the exact epilogues by construction (nothing is rounded there); it is caught where something IS rounded:
the activated outputs, compared at one bf16 ulp per element.
"""
import dataclasses

import pytest
import torch

from tests import gemm_exact as gx


def test_constants_match_the_binding():
    from micro_diffusion_amd import hip
    assert (gx.ACT_NONE, gx.ACT_GELU_TANH, gx.ACT_GELU_ERF, gx.ACT_SILU) == (hip.ACT_NONE, hip.ACT_GELU_TANH, hip.ACT_GELU_ERF, hip.ACT_SILU)
    assert (gx.EPI_STORE_BF16, gx.EPI_RESIDUAL, gx.EPI_STORE_F32, gx.EPI_ACCUM_F32, gx.EPI_ATOMIC_F32, gx.EPI_DACT, gx.EPI_SWIGLU_BWD) == (
        hip.EPI_STORE_BF16, hip.EPI_RESIDUAL, hip.EPI_STORE_F32, hip.EPI_ACCUM_F32, hip.EPI_ATOMIC_F32, hip.EPI_DACT, hip.EPI_SWIGLU_BWD)
    assert gx.NOT_ELIGIBLE == hip.NOT_ELIGIBLE
    assert all(v in hip.GEMM_VARIANT_NAMES for v in gx.VARIANTS)


# ------------------------------------------------------------------------------------------------ storage
def test_fence_sees_one_element_and_allows_the_pad():
    f = gx.Fenced(5, 12, 40, torch.bfloat16, plane_offsets=(0, 320), col0=8).fill(torch.ones(2, 5, 12))
    assert f.dirty().numel() == 0 and f.untouched()
    assert torch.equal(f.values(), torch.ones(2, 5, 12, dtype=torch.bfloat16))
    # sentinel everywhere else, zero pad up to the next multiple of 8
    assert int(f.raw[0]) == gx.SENT_BF16 and float(f.typed[f.off + 12]) == 0.0 and int(f.raw[f.off + 16]) == gx.SENT_BF16
    f.typed[f.off + 13] = 7.0                              # pad column 13 < 16: may be written
    assert f.dirty().numel() == 0 and not f.untouched()
    f.typed[f.off + 16] = 7.0                              # first guard column
    assert f.dirty().tolist() == [f.off + 16]
    f.raw[f.off + 16] = gx.SENT_BF16
    f.typed[f.off - 8 - 1] = 0.0                           # the column just before the slice (col0 = 8) in the first row
    f.typed[f.off + 5 * 40] = 0.0                          # the row after the last one
    f.raw[0] = 0x7FC0                                      # another NaN: a bitwise change
    assert f.dirty().tolist() == sorted([0, f.off - 9, f.off + 200])
    g = gx.Fenced(2, 8, 16, torch.float32).fill(None)
    assert int(g.raw[g.off]) == gx.SENT_F32 and torch.isnan(g.values()).all()


def test_layout_fields_are_all_different():
    for c in gx.CASES:
        a = gx.Problem(c).args
        lds = [a[k] for k in ("lda", "ldb", "ldc", "ldc2", "ldr", "ldg", "ldaux") if k in a and not (k == "ldr" and c.res == "inplace")]
        ext = {"lda": c.K if c.akc else c.M, "ldb": c.K if c.bkc else c.N}
        for k in ("lda", "ldb"):
            assert a[k] > ext[k], (c.name, k)              # nothing dense
        assert a["ldc"] > c.N
        if c.akc == c.bkc and c.M == c.N:
            continue                                       # (equal extents: equal excess would be needed to collide -- they differ)
        strides = [a[k] for k in ("sA", "sB", "sC", "sC2", "sBias", "sAux") if k in a and a[k]]
        if c.batch > 1:
            assert len(set(strides)) == len(strides), (c.name, strides)
    # the excesses themselves
    assert len(set(gx.EXCESS.values())) == len(gx.EXCESS) and len(set(gx.STRIDE_EXTRA.values())) == len(gx.STRIDE_EXTRA)


# ------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("name", [c.name for c in gx.CASES])
def test_case_reference_holds_under_the_model(name):
    """Preconditions (asserted inside Problem), then: the fp64 model of the contract, reading through the strides, reproduces the
    reference computed from the logical values -- exactly -- and leaves every fence intact."""
    p = gx.Problem(gx.CASE_BY_NAME[name])
    p.check_preconditions()
    assert all(torch.isnan(p.bufs[o].values().float()).all() for o in p.outputs if p.case.mode not in (gx.EPI_ACCUM_F32, gx.EPI_ATOMIC_F32)
               and p.case.res != "inplace")
    gx.emulate(p.args)
    assert p.mismatches() == []
    assert p.fence_violations() == []
    assert "C" in p.all_untouched()


def test_split_ranges_follow_the_kernel():
    assert gx.split_ranges(328, 3) == [(0, 128), (128, 256), (256, 328)]          # 6 k-tiles, 2 per split, the last one shorter
    assert gx.split_ranges(64, 3) == [(0, 64), (64, 64), (64, 64)]                # two splits without work ...
    p = gx.Problem(gx.CASE_BY_NAME["splitk3-K64-tn"])
    ref = p.expect["C"][1]
    assert float(ref[1].abs().max()) == 0.0 and float(ref[2].abs().max()) == 0.0   # ... must be WRITTEN with zeros
    assert gx.split_ranges(384, 3) == [(0, 128), (128, 256), (256, 384)]          # = K / ksplit where the persistent kernels run


# ------------------------------------------------------------------------------------------------ the table
def _exp(name, variant):
    return gx.expected(variant, gx.CASE_BY_NAME[name])


def test_table_states_what_the_contract_states():
    # the 2-stage kernels take everything but the SwiGLU backward
    for n, v, e in gx.TABLE:
        if v in gx.TWO_STAGE:
            assert e == ("refuse" if gx.CASE_BY_NAME[n].mode == gx.EPI_SWIGLU_BWD else "run"), (n, v)
    # ragged edges: plain epilogues with A K-contiguous on both persistent kernels, fp32 with both K-strided on pp256 only
    for v in gx.PERSISTENT:
        assert _exp("pers-520x264x384-a1b1-bf16", v) == "run" and _exp("pers-520x264x384-a1b0-bf16", v) == "run"
        for tag in ("res", "res-nn", "dact", "dactc"):
            assert _exp(f"pers-520x264x384-{tag}", v) == "refuse"                  # only the interior form is built
            assert _exp(f"pers-256x512x384-{tag}", v) == "run"
        assert _exp("pers-256x256x128-a0b0-f32", v) == "run"
        assert _exp("pers-256x256x128-a0b0-bf16", v) == "refuse" and _exp("pers-256x256x128-a1b1-f32", v) == "refuse"
        assert _exp("epi-f32-atomic-k1", v) == "refuse" and _exp("epi-f32-accum", v) == "refuse"
        assert _exp("epi-gelu_tanh-c2-whole", v) == "refuse" and _exp("epi-silu-c2-whole", v) == "refuse"
        assert _exp("epi-res-gate8", v) == "refuse" and _exp("small-128x128x24-a1b1-bf16".replace("small", "small"), "reg128") == "run"
    assert _exp("pers-520x264x384-a0b0-f32", "pp256") == "run" and _exp("pers-520x264x384-a0b0-f32", "w4") == "refuse"
    assert _exp("pers-256x256x128-a1b0-f32", "pp256") == "run" and _exp("pers-256x256x128-a1b0-f32", "w4") == "refuse"
    # bias / alpha: pp256 plain epilogues only; w4 never
    assert _exp("epi-bias-c2-whole", "pp256") == "run" and _exp("epi-bias-c2-whole", "w4") == "refuse"
    assert _exp("epi-res-plain-bias-whole", "pp256") == "refuse" and _exp("epi-res-plain-bias-whole", "w4") == "refuse"
    # the SwiGLU backward: w4 on whole tiles, NN, free chip -- nothing else
    for v in gx.VARIANTS:
        assert _exp("epi-swiglu-256", v) == ("run" if v == "w4" else "refuse")
    for n in ("epi-swiglu-ragged", "epi-swiglu-nt", "epi-swiglu-held"):
        assert _exp(n, "w4") == "refuse"
    # split-K slices on the persistent kernels; w4 only whole tiles
    assert _exp("splitk3-pers-tn", "pp256") == "run" and _exp("splitk3-pers-tn", "w4") == "run"
    assert _exp("splitk2-pers-tn-ragged", "pp256") == "run" and _exp("splitk2-pers-tn-ragged", "w4") == "refuse"
    assert _exp("splitk2-pers-nn", "pp256") == "run" and _exp("splitk2-pers-nn", "w4") == "refuse"
    assert all(e in ("run", "refuse") for _, _, e in gx.TABLE)


def test_no_kernel_is_quietly_exempt():
    """Every variant RUNS at least one case of every epilogue it is built for (and is asked to refuse at least one case)."""
    ran = {v: set() for v in gx.VARIANTS}
    refused = {v: 0 for v in gx.VARIANTS}
    for n, v, e in gx.TABLE:
        if e == "run":
            ran[v].add((gx.epilogue_name(gx.CASE_BY_NAME[n]), gx.CASE_BY_NAME[n].akc, gx.CASE_BY_NAME[n].bkc))
        else:
            refused[v] += 1
    for v in gx.TWO_STAGE:
        epis = {e for e, _, _ in ran[v]}
        assert epis >= {"bf16", "bf16_act", "gelu", "gelu_d", "res", "f32", "accum", "atomic", "dact", "dact_gelu", "dact_mul"}, (v, epis)
        for lay in ((1, 1), (1, 0), (0, 1), (0, 0)):
            assert ("bf16", *lay) in ran[v] and ("f32", *lay) in ran[v], (v, lay)
    for v, built in (("pp256", gx.PP_BUILT), ("w4", gx.W4_BUILT)):
        want = {(e, *lay) for lay, es in built.items() for e in es}
        assert ran[v] == want, (v, want - ran[v], ran[v] - want)
    assert all(n > 0 for n in refused.values())


def test_measured_d_is_the_recorded_one():
    for (act, der), rec in gx.D_MEASURED.items():
        d = gx.measured_d(act, der)
        print(f"d[{gx.ACT_NAMES[act]}{chr(39) if der else ''}] = {d:.3e} (recorded {rec:.3e})")
        assert 0 < d <= rec * 1.0001 and rec <= 1.25 * d + 1e-8, (act, der, d, rec)
    assert gx.tolerance_a(gx.ACT_GELU_ERF, False) == gx.tolerance_a(gx.ACT_GELU_ERF, True) == 4e-6
    assert gx.tolerance_a(gx.ACT_SILU, False) == 8 * gx.D_MEASURED[(gx.ACT_SILU, False)]


# ------------------------------------------------------------------------------------------------ mutations
MUT = gx.Case("mutation-res", 264, 136, 1024, 1, 1, gx.EPI_RESIDUAL, res="gate", rps=64, bias=True, c2=True)
MUT_SPLIT = gx.Case("mutation-splitk", 264, 136, 256, 0, 0, gx.EPI_STORE_F32, ksplit=2)
MUT_GELU = gx.Case("mutation-gelu", 264, 136, 1024, 1, 0, act=gx.ACT_GELU_ERF, c2=True)


def _nonzero_k(p, row, k_from):
    A, B = p.logical["A"][0], p.logical["B"][0]
    for k in range(k_from, p.case.K):
        if A[row, k] != 0 and bool((B[:, k] != 0).any()):
            return k
    raise AssertionError("no k with a non-zero product")


def _roll(buf, dim):
    buf.typed[buf.index().reshape(-1)] = torch.roll(buf.values(), 1, dim).reshape(-1)


def _mutations():
    def drop(p):
        gx.emulate(p.args, drop_k=(77, _nonzero_k(p, 77, 500)))

    def double(p):
        gx.emulate(p.args, double_k=(130, _nonzero_k(p, 130, 128)))               # k = 128: the first element of the second split

    def gate(p):
        _roll(p.bufs["gate"], 1)
        gx.emulate(p.args)

    def bias(p):
        _roll(p.bufs["bias"], 2)
        gx.emulate(p.args)

    def swap(p):
        a = dict(p.args)
        a["ldr"], a["ldc2"] = a["ldc2"], a["ldr"]
        gx.emulate(a)

    def trunc(p):
        gx.emulate(p.args, to_bf16=gx.truncate_bf16)

    return [("drop one k element in one row", MUT, drop), ("double-count the element at a split boundary", MUT_SPLIT, double),
            ("roll the gate by one sample", MUT, gate), ("roll the bias by one column", MUT, bias), ("swap ldr with ldc2", MUT, swap),
            ("truncate instead of rounding to nearest", MUT_GELU, trunc)]


@pytest.mark.parametrize("what", [m[0] for m in _mutations()])
def test_exact_comparison_rejects(what):
    _, case, mutate = next(m for m in _mutations() if m[0] == what)
    clean = gx.Problem(case)
    gx.emulate(clean.args)
    assert clean.mismatches() == [] and clean.fence_violations() == []
    p = gx.Problem(case)
    mutate(p)
    found = p.mismatches() + p.fence_violations()
    print(what, "->", found[0] if found else "NOT DETECTED")
    assert found, f"the exact comparison accepts: {what}"
    if what.startswith("double"):
        assert "k-split 1" in found[0] and "row 130" in found[0]


def test_old_rule_accepts():
    """The same mutations at the same shape under the old regime: Gaussian bf16 operands, every leading dimension dense, compared with
    |err| <= 2e-2 * max|ref| + 1e-3.  Printed; the list in the module docstring is asserted."""
    g = torch.Generator().manual_seed(5)
    M, N, K, rps = 264, 136, 1024, 64
    bf = lambda t: t.to(torch.bfloat16).float()
    A, B = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g) * 0.05)
    res, gate, bias = bf(torch.randn(M, N, generator=g)), bf(torch.randn((M + rps - 1) // rps, N, generator=g)), torch.randn(N, generator=g)

    def run(drop=None, double=None, roll_gate=False, roll_bias=False, trunc=False, gelu=False):
        acc = A @ B.t()
        for knob, sign in ((drop, -1.0), (double, 1.0)):
            if knob:
                acc[knob[0]] += sign * A[knob[0], knob[1]] * B[:, knob[1]]
        rd = (lambda x: gx.truncate_bf16(x.double()).float()) if trunc else bf
        if gelu:
            return rd(torch.nn.functional.gelu(acc))
        gt = (torch.roll(gate, 1, 0) if roll_gate else gate).repeat_interleave(rps, 0)[:M]
        return rd(res + gt * rd(acc + (torch.roll(bias, 1, 0) if roll_bias else bias)))

    def accepted(out, ref):
        return float((out - ref).abs().max()) <= 2e-2 * float(ref.abs().max()) + 1e-3

    ref, ref_g = run(), run(gelu=True)
    verdict = {
        "drop one k element in one row": accepted(run(drop=(77, 500)), ref),
        "double-count the element at a split boundary": accepted(run(double=(130, 512)), ref),
        "roll the gate by one sample": accepted(run(roll_gate=True), ref),
        "roll the bias by one column": accepted(run(roll_bias=True), ref),
        "swap ldr with ldc2": True,            # ldr == ldc2 == N in every old test: the swapped launch is the same launch
        "truncate instead of rounding to nearest": accepted(run(trunc=True, gelu=True), ref_g),
    }
    for k, v in verdict.items():
        print(f"old rule, {k}: {'ACCEPTED' if v else 'rejected'}")
    assert [k for k, v in verdict.items() if v] == ["drop one k element in one row", "double-count the element at a split boundary",
                                                   "swap ldr with ldc2", "truncate instead of rounding to nearest"]


def test_comparator_reports_coordinates():
    p = gx.Problem(gx.CASE_BY_NAME["splitk3-K328-tn"])
    gx.emulate(p.args)
    c = p.bufs["C"]
    c.typed[c.elem_offset(2) + 130 * c.ld + 5] += 1.0      # batch 0, split 2, row 130, column 5
    msg = p.mismatches()
    assert len(msg) == 1 and "k-split 2" in msg[0] and "(row 130, col 5)" in msg[0] and "128-tile (1, 0)" in msg[0], msg
    q = gx.Problem(gx.CASE_BY_NAME["epi-gelu_erf-c2"])
    gx.emulate(q.args)
    assert q.mismatches() == []
    v = q.bufs["C"].values()
    big = int(torch.argmax(v.float().abs().reshape(-1)))
    q.bufs["C"].typed[q.bufs["C"].index().reshape(-1)[big]] *= 1.0 + 2.0 ** -6   # two bf16 ulps on one element
    assert len(q.mismatches()) == 1
