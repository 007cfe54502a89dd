"""md_attn_probs against an fp64 softmax of the same bf16 operands, at its edges: ragged query tiles and key blocks,
both addressing forms of DiTEngine._block_fwd, scores near +-100, guard rows and columns, the row table, accumulation, refusals.
The bound |got - ref| <= (2 E + 2^-16) ref + 2^-24 is derived in tests/attn_probs_ref.py from the kernel's arithmetic."""
import ctypes

import pytest
import torch

from tests import attn_probs_ref as ref_mod

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _st():
    return torch.cuda.current_stream().cuda_stream


def _qk(B, H, Sq, Skv, hd, seed):
    """Logical operands [B, H, S, hd] bf16 on the GPU, unit-variance entries (what the QK-LayerNorm leaves)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, Sq, hd, generator=g).to(BF16).cuda(), torch.randn(B, H, Skv, hd, generator=g).to(BF16).cuda())


def _packed(x, width_mult=1, col0=0, guard_rows=0, fill=float("nan")):
    """[B, H, S, hd] -> a buffer [B, S + guard_rows, width_mult * H * hd] holding head h of row s at columns col0 + h * hd; everything
    else is `fill`.  Returns (buffer, ld, sample stride)."""
    B, H, S, hd = x.shape
    hx = H * hd
    buf = torch.full((B, S + guard_rows, width_mult * hx), fill, device="cuda", dtype=BF16)
    buf[:, :S, col0:col0 + hx] = x.permute(0, 2, 1, 3).reshape(B, S, hx)
    return buf, width_mult * hx, (S + guard_rows) * width_mult * hx


def _args(hip, qbuf, qoff, ldq, sq, hsq, kbuf, koff, ldk, sk, hsk, B, H, Sq, Skv, hd):
    a = hip.AttnArgs()
    a.q, a.k = qbuf.data_ptr() + 2 * qoff, kbuf.data_ptr() + 2 * koff
    a.B, a.H, a.Sq, a.Skv, a.ldq, a.ldk, a.sq, a.sk, a.hsq, a.hsk = B, H, Sq, Skv, ldq, ldk, sq, sk, hsq, hsk
    a.scale, a.hd = ref_mod.f32_scale(hd), hd
    return a


def _run_packed(hip, q, k, out=None, ldo=None, out_rows=None, guard_rows=0, expect=0):
    """The packed form of _block_fwd: q rows [M, hx], k the first half of [Mc, 2 hx] rows.  Returns out [B * Sq, ldo] (fresh zeros when
    not given)."""
    B, H, Sq, hd = q.shape
    Skv = k.shape[2]
    qb, ldq, sq = _packed(q, guard_rows=guard_rows)
    kb, ldk, sk = _packed(k, width_mult=2, guard_rows=guard_rows)
    a = _args(hip, qb, 0, ldq, sq, 0, kb, 0, ldk, sk, 0, B, H, Sq, Skv, hd)
    if ldo is None:
        ldo = (Skv + 3) // 4 * 4
    if out is None:
        out = torch.zeros(B * Sq, ldo, device="cuda")
    rc = hip.lib().md_attn_probs(ctypes.byref(a), out.data_ptr(), ldo, None if out_rows is None else out_rows.data_ptr(), _st())
    assert rc == expect, rc
    return out


SQ = [1, 15, 16, 17, 63, 64, 65, 257]
SKV = [1, 16, 17, 77, 96, 97, 128]
CASES = sorted({(sq, 77, hd, 3, 3 if sq < 257 else 1) for sq in SQ for hd in (32, 64)}
               | {(65, skv, hd, 3, 1) for skv in SKV for hd in (32, 64)}
               | {(17, 97, 64, H, B) for H in (1, 3, 8) for B in (1, 3)}
               | {(63, 17, 32, H, B) for H in (1, 3, 8) for B in (1, 3)})


@pytest.mark.parametrize("Sq, Skv, hd, H, B", CASES)
def test_probabilities_meet_the_derived_bound_and_rows_sum_to_one(hip, Sq, Skv, hd, H, B):
    q, k = _qk(B, H, Sq, Skv, hd, 1000 + Sq * 131 + Skv)
    out = _run_packed(hip, q, k)
    got = out.view(B, Sq, -1)[:, :, :Skv]
    ref, E = ref_mod.reference(q, k, ref_mod.f32_scale(hd))
    ref_mod.assert_within_bound(got, ref, E, f"Sq={Sq} Skv={Skv} hd={hd} H={H} B={B}")
    assert (got.double().sum(-1) - 1).abs().max() <= 2.0 ** -16
    assert (out.view(B, Sq, -1)[:, :, Skv:] == 0).all()


def test_cases_cover_the_edges():
    assert 38 <= len(CASES) <= 44
    assert {c[0] for c in CASES} >= set(SQ) and {c[1] for c in CASES} >= set(SKV)
    assert {c[2] for c in CASES} == {32, 64} and {c[3] for c in CASES} == {1, 3, 8} and {c[4] for c in CASES} == {1, 3}


@pytest.mark.parametrize("hd", [32, 64])
def test_head_major_and_wide_rows_equal_packed(hip, hd):
    B, H, Sq, Skv = 3, 4, 65, 77
    q, k = _qk(B, H, Sq, Skv, hd, 7)
    packed = _run_packed(hip, q, k)
    ldo = packed.shape[1]
    # head-major: [B, H, S, hd] contiguous, as md_qkln_fwd_hm writes it
    qh, kh = q.contiguous(), k.contiguous()
    a = _args(hip, qh, 0, hd, H * Sq * hd, Sq * hd, kh, 0, hd, H * Skv * hd, Skv * hd, B, H, Sq, Skv, hd)
    hm = torch.zeros_like(packed)
    hip.check(hip.lib().md_attn_probs(ctypes.byref(a), hm.data_ptr(), ldo, None, _st()), "md_attn_probs")
    assert torch.equal(hm, packed)
    # q inside a wider row (the q third of a packed qkv row), k the first half of a kv row
    hx = H * hd
    qw, ldq, sq = _packed(q, width_mult=3, col0=hx)
    kw, ldk, sk = _packed(k, width_mult=2)
    a = _args(hip, qw, hx, ldq, sq, 0, kw, 0, ldk, sk, 0, B, H, Sq, Skv, hd)
    wide = torch.zeros_like(packed)
    hip.check(hip.lib().md_attn_probs(ctypes.byref(a), wide.data_ptr(), ldo, None, _st()), "md_attn_probs")
    assert torch.equal(wide, packed)
    assert packed.abs().max() > 0


@pytest.mark.parametrize("hd", [32, 64])
def test_hard_softmax_scores_near_a_hundred_stay_finite_and_in_bound(hip, hd):
    """One head carries the row's energy, as after the full-width QK-LayerNorm: its scores are near +-100 (|q_h| |k_h| scale), the
    other heads are silent.  Without the maximum subtracted, exp overflows here."""
    B, H, Sq, Skv = 2, 3, 33, 77
    g = torch.Generator().manual_seed(11)
    amp = 100.0 ** 0.5 * hd ** -0.25                 # amp^2 * hd * scale = 100
    base = torch.where(torch.rand(hd, generator=g) < 0.5, -amp, amp)
    q, k = torch.zeros(B, H, Sq, hd), torch.zeros(B, H, Skv, hd)
    sq = torch.where(torch.rand(B, Sq, 1, generator=g) < 0.5, -1.0, 1.0)
    sk = torch.where(torch.rand(B, Skv, 1, generator=g) < 0.5, -1.0, 1.0)
    q[:, 1] = sq * base + 0.05 * torch.randn(B, Sq, hd, generator=g)
    k[:, 1] = sk * base + 0.05 * torch.randn(B, Skv, hd, generator=g)
    q, k = q.to(BF16).cuda(), k.to(BF16).cuda()
    scale = ref_mod.f32_scale(hd)
    s = scale * (q[:, 1].double() @ k[:, 1].double().transpose(-1, -2))
    assert s.max() > 90 and s.min() < -90
    out = _run_packed(hip, q, k)
    got = out.view(B, Sq, -1)[:, :, :Skv]
    ref, E = ref_mod.reference(q, k, scale)
    ref_mod.assert_within_bound(got, ref, E, f"hard softmax hd={hd}")
    assert (got.double().sum(-1) - 1).abs().max() <= 2.0 ** -16


def test_guard_rows_and_pad_columns_stay_untouched_and_nan_rows_are_not_read(hip):
    """out: sentinel pad columns [Skv, ldo) and a sentinel row before and behind; q and k: two NaN rows behind the rows of every sample,
    inside the same allocation, and NaN in every column of the wider k row that is not K."""
    B, H, Sq, Skv, hd = 2, 3, 17, 77, 64
    q, k = _qk(B, H, Sq, Skv, hd, 13)
    ldo = 84                                        # 77 -> 80 would do; one more 16-byte group of padding
    store = torch.full((B * Sq + 2, ldo), -7.0, device="cuda")
    out = store[1:1 + B * Sq]
    out[:, :Skv] = 0
    _run_packed(hip, q, k, out=out, ldo=ldo, guard_rows=2)
    assert (store[0] == -7.0).all() and (store[-1] == -7.0).all(), "wrote a row the launch does not name"
    assert (out[:, Skv:] == -7.0).all(), "wrote a pad column"
    ref, E = ref_mod.reference(q, k, ref_mod.f32_scale(hd))
    ref_mod.assert_within_bound(out.view(B, Sq, ldo)[:, :, :Skv], ref, E, "guards")
    assert torch.equal(out[:, :Skv], _run_packed(hip, q, k)[:, :Skv]), "the guard rows changed the result"


def test_out_rows_scatters_into_a_larger_buffer(hip):
    B, H, Sq, Skv, hd = 3, 2, 21, 77, 32
    q, k = _qk(B, H, Sq, Skv, hd, 17)
    dense = _run_packed(hip, q, k)
    ldo, n = dense.shape[1], 2 * B * Sq + 5
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:B * Sq].to(torch.int32).cuda()
    big = torch.full((n, ldo), -7.0, device="cuda")
    big[rows.long()] = 0
    _run_packed(hip, q, k, out=big, out_rows=rows)
    assert torch.equal(big[rows.long()], dense)
    untouched = torch.ones(n, dtype=torch.bool, device="cuda")
    untouched[rows.long()] = False
    assert (big[untouched] == -7.0).all() and int(untouched.sum()) == n - B * Sq


def test_launches_accumulate_in_fp32_and_are_reproducible(hip):
    B, H, Sq, Skv, hd = 2, 3, 65, 97, 64
    q1, k1 = _qk(B, H, Sq, Skv, hd, 19)
    q2, k2 = _qk(B, H, Sq, Skv, hd, 23)
    o1, o2 = _run_packed(hip, q1, k1), _run_packed(hip, q2, k2)
    both = _run_packed(hip, q1, k1)
    _run_packed(hip, q2, k2, out=both)
    assert torch.equal(both, o1 + o2)
    assert not torch.equal(o1, o2)
    assert torch.equal(_run_packed(hip, q1, k1), o1)


def test_refuses_bad_arguments_and_writes_nothing(hip):
    L = hip.lib()
    B, H, Sq, hd = 1, 2, 16, 64
    q, k = _qk(B, H, Sq, 129, hd, 29)
    out = torch.full((B * Sq, 132), -7.0, device="cuda")
    _run_packed(hip, q, k, out=out, ldo=132, expect=-1)                                   # Skv = 129
    q48, k48 = _qk(B, H, Sq, 77, 48, 31)
    _run_packed(hip, q48, k48, out=out, ldo=132, expect=-1)                               # hd = 48
    q, k = _qk(B, H, Sq, 77, hd, 37)
    _run_packed(hip, q, k, out=out, ldo=76, expect=-1)                                    # ldo < Skv
    _run_packed(hip, q, k, out=out, ldo=78, expect=-1)                                    # ldo % 4 != 0
    qb, ldq, sq = _packed(q)
    kb, ldk, sk = _packed(k, width_mult=2)
    a = _args(hip, qb, 0, ldq, sq, 0, kb, 0, ldk, sk, 0, B, H, Sq, 77, hd)
    assert L.md_attn_probs(ctypes.byref(a), None, 80, None, _st()) == -1                  # NULL out
    assert L.md_attn_probs(None, out.data_ptr(), 80, None, _st()) == -1                   # NULL arguments
    a.q = None
    assert L.md_attn_probs(ctypes.byref(a), out.data_ptr(), 80, None, _st()) == -1
    a.q, a.k = qb.data_ptr(), None
    assert L.md_attn_probs(ctypes.byref(a), out.data_ptr(), 80, None, _st()) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all()
