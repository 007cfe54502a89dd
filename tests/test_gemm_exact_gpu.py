"""Every kernel family behind md_gemm_bf16 -- reg128, dma128, paced256, pp256, w4 -- on inputs whose right answer has no rounding
error (tests/gemm_exact.py): strided operands, fenced outputs, every epilogue, the smallest shapes of every kernel.

  * exact epilogues (plain store, C2 raw copy, bias, alpha, gated / plain / in-place residual, fp32 store / accumulate / atomic,
    split-K slices + md_splitk_reduce, DACT from a cached derivative): torch.equal against the fp64 reference;
  * transcendental epilogues (GELU-tanh, GELU-erf, SiLU, their derivatives in DACT, the cached derivative on the forward side,
    SWIGLU_BWD): exact pre-activation, raw copy bit for bit, activated output per element within
    2^-8 |f64| + a * s  (s = |exact multiplicand|).  a = 4e-6 for the erf forms (twice the polynomial bound of md_common.h); for the
    others a = 8 d with d = max |torch fp32 - fp64| over every multiple of 1/8 in [-32, 32], measured on the CPU:
        d[gelu_tanh] = 2.48e-7   d[gelu_tanh'] = 4.81e-7   d[silu] = 1.14e-6   d[silu'] = 9.67e-7
        (d[gelu_erf] = 5.61e-7   d[gelu_erf'] = 8.82e-8: reported, not used)
  * nothing is dense: every leading dimension and batch stride has its own excess, outputs have guard rows and guard columns that
    are compared bit for bit after every launch; C also as a column slice of a packed-qkv-like matrix, the gate as a slice of
    [samples, 6 N];
  * no skips: the table of gemm_exact states for every (variant, case) whether the family must run it (chosen_variant is asserted)
    or refuse it (MD_NOT_ELIGIBLE and every allocation untouched).

Found while these tests were written (reading the shared epilogue for the strides a case may set) and pinned by them:
  * MD_EPI_ATOMIC_F32 with ksplit > 1 added split s into C + s * sSplit whenever the caller had left a value in sSplit (the header
    gives that field to STORE_F32 alone), i.e. outside C: md_gemm_bf16 now clears the field for every other mode
    (cases epi-f32-atomic-k3 and epi-f32-atomic-cslice set a non-zero sSplit).
No kernel produced a wrong bit or touched a fence on any case of the table.
"""
import ctypes

import pytest
import torch

from tests import gemm_exact as gx

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(scope="module")
def tail_ws():
    return torch.zeros(2 << 20 >> 2, device=dev, dtype=torch.float32)           # 2 MiB: 8 raw 256 x 256 fp32 tiles


def _launch(hip, p, variant, args=None, tail_ws=None):
    kw = p.launch_kwargs(args)
    chosen, used = [], []
    rc = hip.gemm(variant=hip.GEMM_VARIANT_NAMES[variant], expect=None, chosen=chosen, tail_used=used,
                  tail_ws=tail_ws if p.case.tail_mode else None, **kw)
    torch.cuda.synchronize()
    return rc, chosen[0], used[0]


def _assert_clean(p):
    problems = p.mismatches() + p.fence_violations()
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name,variant,outcome", gx.TABLE, ids=[f"{v}-{n}" for n, v, _ in gx.TABLE])
def test_table(hip, tail_ws, name, variant, outcome):
    p = gx.Problem(gx.CASE_BY_NAME[name], dev)
    rc, chosen, used = _launch(hip, p, variant, tail_ws=tail_ws)
    if outcome == "run":
        assert rc == 0, f"{variant} must run {name}: rc {rc}"
        assert chosen == hip.GEMM_VARIANT_NAMES[variant]
        if variant in gx.PERSISTENT:
            assert used == (gx.TAIL_SPLIT if p.case.tail_mode == 2 else 0)
        _assert_clean(p)
    else:
        assert rc == (gx.NOT_ELIGIBLE if outcome == "refuse" else gx.BAD_ARG), f"{variant} must refuse {name}: rc {rc}"
        assert p.all_untouched() == [], "a refused launch wrote memory"


@pytest.mark.parametrize("tag", ["plain", "gelu-c2", "res-gate", "dact", "dact-cached"])
def test_tail_form_is_bit_identical_to_whole_tiles(hip, tail_ws, tag):
    """(512, 1280, 512) on 8 workgroups: 10 tiles, r = 2 left over, 4 iterations -> 4 units per left-over tile.  The pre-activations
    are exact whatever the summation order, so the two forms must agree in every bit (both are compared with the reference by
    test_table)."""
    outs = []
    for tm in (1, 2):
        p = gx.Problem(gx.CASE_BY_NAME[f"tail{tm}-{tag}"], dev)
        rc, chosen, used = _launch(hip, p, "pp256", tail_ws=tail_ws)
        assert rc == 0 and chosen == hip.GEMM_PP256 and used == (gx.TAIL_SPLIT if tm == 2 else 0)
        outs.append({n: p.bufs[n].raw.clone() for n in p.outputs})
    for n in outs[0]:
        assert torch.equal(outs[0][n], outs[1][n]), f"{tag}: {n} differs between the tail form and whole tiles"


# ------------------------------------------------------------------------------------------------ negative controls
def _control(hip, name, variant, change):
    p = gx.Problem(gx.CASE_BY_NAME[name], dev)
    args = dict(p.args)
    change(args)
    rc, _, _ = _launch(hip, p, variant, args=args)
    assert rc == 0
    return p.mismatches()


def test_control_k_minus_8_is_seen(hip):
    """The real kernel with K - 8 on a K-contiguous layout, against the unmodified reference: the comparator must object."""
    def change(a):
        a["K"] -= 8
    assert _control(hip, "epi-bias", "reg128", change)
    assert _control(hip, "pers-256x512x384-a1b1-bf16", "dma128", change)


def test_control_gate_one_row_ahead_is_seen(hip):
    def change(a):
        a["gate"] = a["gate"].advanced(a["ldg"])               # the guard rows behind the gate keep this inside the allocation
    assert _control(hip, "epi-res-gate64", "reg128", change)
    assert _control(hip, "epi-res-gate64-whole", "pp256", change)


def test_control_bias_one_element_ahead_is_seen(hip):
    def change(a):
        a["bias"] = a["bias"].advanced(1)                      # inside its padded buffer
    msgs = _control(hip, "epi-bias", "paced256", change)
    assert msgs and "C differs" in msgs[0]


# ------------------------------------------------------------------------------------------------ split-K slices + md_splitk_reduce
def _dense_slices(hip, variant, M, N, K, ks, akc, bkc, batch=1):
    """A split-K launch into the DENSE fp32 slices md_splitk_reduce reads ([batch][ksplit][M, N], fenced as one block); returns the
    workspace and the exact slices."""
    c = gx.Case(f"reduce-{variant}-{M}x{N}x{K}-{ks}-{akc}{bkc}-{batch}", M, N, K, akc, bkc, gx.EPI_STORE_F32, ksplit=ks, batch=batch)
    p = gx.Problem(c, dev)
    ws = gx.Fenced(batch * ks * M, N, N, torch.float32, device=dev).fill(None)
    args = dict(p.args, C=gx.Ptr(ws, ws.elem_offset()), ldc=N, sSplit=M * N, sC=ks * M * N)
    rc, chosen, _ = _launch(hip, p, variant, args=args)
    assert rc == 0 and chosen == hip.GEMM_VARIANT_NAMES[variant]
    ref = p.expect["C"][1].reshape(batch, ks, M, N)
    got = ws.values().cpu().reshape(batch, ks, M, N)
    assert torch.equal(got, ref.float()), f"{c.name}: dense slices differ"
    assert ws.dirty().numel() == 0 and p.bufs["A"].untouched() and p.bufs["B"].untouched()
    return ws.refreeze(), ref


REDUCE = [("reg128", 136, 72, 256, 2, 0, 0, 1), ("reg128", 136, 72, 328, 3, 0, 0, 2), ("dma128", 136, 72, 512, 4, 1, 1, 1),
          ("paced256", 264, 136, 64, 3, 0, 0, 1), ("dma128", 264, 136, 328, 3, 1, 0, 1), ("paced256", 264, 136, 512, 4, 0, 0, 2),
          ("pp256", 256, 512, 256, 2, 0, 0, 1), ("pp256", 520, 264, 384, 3, 0, 0, 2), ("pp256", 256, 256, 384, 3, 1, 0, 1),
          ("w4", 256, 512, 256, 2, 0, 0, 2), ("w4", 256, 256, 384, 3, 0, 0, 1)]


@pytest.mark.parametrize("variant,M,N,K,ks,akc,bkc,batch", REDUCE)
def test_splitk_slices_and_reduce(hip, variant, M, N, K, ks, akc, bkc, batch):
    """ksplit 2 / 3 / 4 with a shorter last split (K = 328) and splits without work (K = 64: their slices are zeros, written);
    md_splitk_reduce with accumulate 0 / 1 / 2 into fenced outputs with ldo > N and a non-dense sOut, bit-exact (mode 2 as bf16)."""
    L, st = hip.lib(), hip.stream_ptr()
    ws, ref = _dense_slices(hip, variant, M, N, K, ks, akc, bkc, batch)
    gen = torch.Generator().manual_seed(M + K + ks)
    ldo = N + 24
    s_out = (M + 2) * ldo + 8
    for acc_mode in (0, 1, 2):
        out = gx.Fenced(M, N, ldo, torch.bfloat16 if acc_mode == 2 else torch.float32, tuple(b * s_out for b in range(batch)), device=dev)
        init = torch.randint(-8, 9, (batch, M, N), generator=gen).double() if acc_mode == 1 else None
        out.fill(init)
        want = gx.splitk_reduce_ref(ref.transpose(0, 1), init, acc_mode)
        assert float(want.abs().max()) <= 256
        hip.check(L.md_splitk_reduce(ws.ptr(), out.ptr(), M, N, ldo, s_out, ks, batch, acc_mode, st), "md_splitk_reduce")
        torch.cuda.synchronize()
        assert torch.equal(out.values().cpu(), want.to(out.dtype)), f"accumulate {acc_mode}"
        assert out.dirty().numel() == 0, f"accumulate {acc_mode}: fence of the output written"
        assert ws.untouched()
    # the flat form over batch 0: n = M * N elements per slice, slices M * N apart
    n = M * N
    for acc_mode in (0, 1, 2):
        out = gx.Fenced(1, n, n + 24, torch.bfloat16 if acc_mode == 2 else torch.float32, device=dev)
        init = torch.randint(-8, 9, (1, 1, n), generator=gen).double() if acc_mode == 1 else None
        out.fill(init)
        want = gx.splitk_reduce_ref(ref[0].reshape(ks, 1, 1, n), init, acc_mode)
        hip.check(L.md_splitk_reduce_flat(ws.ptr(), out.ptr(), n, n, ks, acc_mode, st), "md_splitk_reduce_flat")
        torch.cuda.synchronize()
        assert torch.equal(out.values().cpu(), want.to(out.dtype)), f"flat, accumulate {acc_mode}"
        assert out.dirty().numel() == 0 and ws.untouched()


# ------------------------------------------------------------------------------------------------ grouped problems, operand lists
def _kstrided(gen, T, rows, excess):
    """A K-strided operand [T, rows] of {-1, 0, 1} with a non-dense leading dimension."""
    v = gx._draw(gen, (1, T, rows), (-1, 0, 1))
    return v[0], gx.Fenced(T, rows, gx.round_up(rows, 8) + excess, torch.bfloat16, device=dev).fill(v)


def _check_grouped(hip, rc, chosen, variant, ks, shapes, offs, span, dys, xs, ws, before):
    L, st, T = hip.lib(), hip.stream_ptr(), 256
    assert rc == 0 and chosen == hip.GEMM_VARIANT_NAMES[variant]
    written = torch.zeros(ks * span, dtype=torch.bool)
    got = ws.view(torch.float32).cpu()
    kspan = T // ks
    for i, (m, n) in enumerate(shapes):
        for s in range(ks):
            ref = dys[i][0][s * kspan:(s + 1) * kspan].t() @ xs[i][0][s * kspan:(s + 1) * kspan]
            lo = s * span + offs[i]
            assert torch.equal(got[lo:lo + m * n].view(m, n), ref.float()), f"problem {i} ({m} x {n}), split {s}"
            written[lo:lo + m * n] = True
    assert torch.equal(ws.cpu()[~written], before.cpu()[~written]), "a grouped launch wrote outside its problems' slices"
    assert all(b.untouched() for _, b in dys + xs)
    # one md_splitk_reduce_flat per contiguous run, into fenced accumulators
    runs = [(offs[0], offs[1] + shapes[1][0] * shapes[1][1]), (offs[2], offs[-1] + shapes[-1][0] * shapes[-1][1])]
    for lo, hi in runs:
        n = hi - lo
        out = gx.Fenced(1, n, n + 24, torch.float32, device=dev).fill(torch.full((1, 1, n), 2.0))
        hip.check(L.md_splitk_reduce_flat(ws.data_ptr() + 4 * lo, out.ptr(), n, span, ks, 1, st), "md_splitk_reduce_flat")
        torch.cuda.synchronize()
        flat = out.values().cpu().reshape(-1)
        for i, (m, n_) in enumerate(shapes):
            if lo <= offs[i] < hi:
                ref = 2.0 + dys[i][0].t() @ xs[i][0]
                assert torch.equal(flat[offs[i] - lo:offs[i] - lo + m * n_].view(m, n_), ref.float()), f"reduced problem {i}"
        assert out.dirty().numel() == 0


@pytest.mark.parametrize("variant,ks,shapes,outcome", [
    ("pp256", 1, [(512, 256), (256, 264), (256, 256), (200, 72), (520, 264)], "run"),
    ("pp256", 2, [(512, 256), (256, 264), (256, 256), (200, 72), (520, 264)], "run"),
    ("w4", 1, [(512, 256), (256, 512), (256, 256)], "run"),
    ("w4", 2, [(512, 256), (256, 512), (256, 256)], "run"),
    ("w4", 2, [(512, 256), (200, 72)], "refuse"),              # w4 takes whole interior tiles only
    ("reg128", 1, [(512, 256), (256, 256)], "refuse"),         # a grouped launch exists on the persistent kernels only
])
def test_grouped_problems(hip, variant, ks, shapes, outcome):
    """md_gemm_args.problems at T = 256 tokens: per-problem non-dense lda / ldb, exact inputs, fp32 slices at their c_off inside every
    split's slice -- everything else of the workspace (the gap between two runs, the pad behind every problem, the space between the
    slices) must keep its sentinel bits."""
    L, st = hip.lib(), hip.stream_ptr()
    gen = torch.Generator().manual_seed(31 + ks + len(shapes))
    T = 256
    offs, o = [], 64
    for i, (m, n) in enumerate(shapes):
        offs.append(o)
        o += gx.round_up(m * n, 64) + (4096 if i == 1 else 0)  # a foreign tensor between problems 1 and 2
    span = o + 64
    dys = [_kstrided(gen, T, m, 8 + 16 * i) for i, (m, _) in enumerate(shapes)]
    xs = [_kstrided(gen, T, n, 16 + 16 * i) for i, (_, n) in enumerate(shapes)]
    probs = (hip.GemmProblem * len(shapes))()
    for i, (m, n) in enumerate(shapes):
        probs[i] = hip.GemmProblem(dys[i][1].ptr(), xs[i][1].ptr(), dys[i][1].ld, xs[i][1].ld, m, n, offs[i])
    ws = torch.full((ks * span,), gx.SENT_F32, dtype=torch.int32, device=dev)
    before = ws.clone()
    chosen = ctypes.c_int32(-1)
    a = hip.GemmArgs()
    for k, v in dict(A=dys[0][1].ptr(), B=xs[0][1].ptr(), C=ws.data_ptr(), M=shapes[0][0], N=shapes[0][1], K=T, lda=dys[0][1].ld,
                     ldb=xs[0][1].ld, ldc=shapes[0][1], sSplit=span, batch=1, ksplit=ks, a_kcontig=0, b_kcontig=0,
                     mode=hip.EPI_STORE_F32, act=0, alpha=1.0, problems=ctypes.addressof(probs), n_problems=len(shapes),
                     variant=hip.GEMM_VARIANT_NAMES[variant], chosen_variant=ctypes.addressof(chosen)).items():
        setattr(a, k, v)
    rc = L.md_gemm_bf16(ctypes.byref(a), st)
    torch.cuda.synchronize()
    refused = rc == gx.NOT_ELIGIBLE and torch.equal(ws, before)
    assert refused == (outcome == "refuse"), (rc, outcome)
    if outcome == "run":
        _check_grouped(hip, rc, chosen.value, variant, ks, shapes, offs, span, dys, xs, ws, before)


@pytest.mark.parametrize("segments,ks", [(1, 3), (3, 1), (3, 2)])
def test_operand_lists(hip, segments, ks):
    """md_gemm_args.A_list / B_list on pp256 (A K-contiguous, B K-strided, fp32 slices): item (batch, split) contracts `segments`
    operand pairs of 128 k each, every pair its own fenced allocation with non-dense lda / ldb (shared by the list: the struct has
    one of each).  w4 has no list form and must refuse."""
    gen = torch.Generator().manual_seed(7 * segments + ks)
    M, N, kseg = 264, 136, 128
    G = ks * segments
    lda, ldb = kseg + 8, N + 16
    As, Bs = [], []
    for _ in range(G):
        av, bv = gx._draw(gen, (1, M, kseg), (-1, 0, 1)), gx._draw(gen, (1, kseg, N), (-1, 0, 1))
        As.append((av[0], gx.Fenced(M, kseg, lda, torch.bfloat16, device=dev).fill(av)))
        Bs.append((bv[0], gx.Fenced(kseg, N, ldb, torch.bfloat16, device=dev).fill(bv)))
    al = torch.tensor([b.ptr() for _, b in As], dtype=torch.int64).to(dev)
    bl = torch.tensor([b.ptr() for _, b in Bs], dtype=torch.int64).to(dev)
    ldc = N + 24
    s_split = (M + 1) * ldc + 56
    C = gx.Fenced(M, N, ldc, torch.float32, tuple(s * s_split for s in range(ks)), device=dev).fill(None)
    kw = dict(A=As[0][1].ptr(), B=Bs[0][1].ptr(), C=C.ptr(), M=M, N=N, K=kseg * G, lda=lda, ldb=ldb, ldc=ldc, sC=ks * s_split + 64,
              sSplit=s_split, ksplit=ks, a_kcontig=1, b_kcontig=0, mode=hip.EPI_STORE_F32, A_list=al, B_list=bl, list_segments=segments,
              expect=None)
    assert hip.gemm(variant=hip.GEMM_W4, **kw) == gx.NOT_ELIGIBLE
    torch.cuda.synchronize()
    assert C.untouched()
    chosen = []
    assert hip.gemm(variant=hip.GEMM_PP256, chosen=chosen, **kw) == 0 and chosen == [hip.GEMM_PP256]
    torch.cuda.synchronize()
    want = torch.stack([sum(As[s * segments + j][0] @ Bs[s * segments + j][0] for j in range(segments)) for s in range(ks)])
    assert torch.equal(C.values().cpu(), want.float())
    assert C.dirty().numel() == 0 and all(b.untouched() for _, b in As + Bs)
