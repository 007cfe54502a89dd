"""Masked-expert pruning on the GPU: md_moe_compact_kept against a torch restatement, the absolute-position and
compact-list entry points against the kernels they generalise, and the engine switch on against off on the Tiny config (whose last
patch-mixer block is MoE): forward, gradients, the dense fallback under route_override, and the unchanged launch log at mask 0."""
import pytest
import torch

from oracle import microdit_ref as orc
from tests.moe_ref import compact as _compact_ref

pytestmark = pytest.mark.gpu
I32, F32, BF16 = torch.int32, torch.float32, torch.bfloat16


def _st():
    return torch.cuda.current_stream().cuda_stream


def _route(hip, logits, B, S, E, k):
    L = hip.lib()
    ld = 8 if E <= 8 else 16
    lg = torch.zeros(B * S, ld, device="cuda", dtype=F32)
    lg[:, :E] = logits
    probs = torch.empty(B * S, ld, device="cuda", dtype=F32)
    rowidx = torch.empty(E, B * k, device="cuda", dtype=I32)
    gval = torch.empty(E, B * k, device="cuda", dtype=F32)
    slot = torch.empty(B * S, E, device="cuda", dtype=I32)
    hip.check(L.md_moe_route(lg.data_ptr(), probs.data_ptr(), ld, B, S, E, k, rowidx.data_ptr(), gval.data_ptr(), slot.data_ptr(), _st()), "route")
    return probs, rowidx, gval, slot, ld


def _mask(hip, noise, B, S, Tk):
    keep_rows = torch.empty(B * Tk, device="cuda", dtype=I32)
    ids_restore = torch.empty(B, S, device="cuda", dtype=I32)
    mask = torch.empty(B, S, device="cuda", dtype=F32)
    hip.check(hip.lib().md_get_mask(noise.contiguous().data_ptr(), B, S, Tk, keep_rows.data_ptr(), ids_restore.data_ptr(), mask.data_ptr(), _st()), "mask")
    return ids_restore, mask


def _compact(hip, rowidx, gval, ids_restore, Tk, B, S, E, k):
    rowidx_c = torch.full((E, B * k), -7, device="cuda", dtype=I32)
    gval_c = torch.full((E, B * k), -7.0, device="cuda", dtype=F32)
    count = torch.full((E,), -7, device="cuda", dtype=I32)
    slot_c = torch.full((B * S, E), -7, device="cuda", dtype=I32)
    ws = torch.empty(E * ((B * k + 1023) // 1024), device="cuda", dtype=I32)
    hip.check(hip.lib().md_moe_compact_kept(rowidx.data_ptr(), gval.data_ptr(), ids_restore.data_ptr(), Tk, B, S, E, k, rowidx_c.data_ptr(),
                                            gval_c.data_ptr(), count.data_ptr(), slot_c.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "compact")
    torch.cuda.synchronize()
    return rowidx_c, gval_c, count, slot_c


def _crafted(B, S, E, k, Tk):
    """Expert 0 of sample 0 picks tokens Tk .. Tk+k-1 (none kept); expert 1 picks tokens 0 .. k-1 of every sample (all kept: k <= Tk);
    the mask keeps tokens 0 .. Tk-1 of every sample."""
    g = torch.Generator().manual_seed(5)
    logits = torch.rand(B, S, E, generator=g) - 0.5
    logits[0, Tk:Tk + k, 0] = 6.0
    logits[:, :k, 1] = 6.0
    noise = torch.rand(B, S, generator=g) * 0.5 + 0.5
    noise[:, :Tk] = torch.rand(B, Tk, generator=g) * 0.4
    return logits.view(B * S, E).cuda(), noise.cuda()


@pytest.mark.parametrize("case", ["E8", "E4", "all_kept", "crafted", "two_chunks"])
def test_compact_kept_against_torch(hip, case):
    B, S, k = (5, 512, 256) if case == "two_chunks" else (3, 32, 8)     # two_chunks: 1280 list entries per expert, a ragged second chunk
    E = 4 if case == "E4" else 8
    Tk = S if case == "all_kept" else 128 if case == "two_chunks" else 8
    if case == "crafted":
        logits, noise = _crafted(B, S, E, k, Tk)
    else:
        g = torch.Generator().manual_seed(11 + E + Tk)
        logits, noise = torch.randn(B * S, E, generator=g).cuda(), torch.rand(B, S, generator=g).cuda()
    probs, rowidx, gval, slot, ld = _route(hip, logits, B, S, E, k)
    ids_restore, mask = _mask(hip, noise, B, S, Tk)
    got = _compact(hip, rowidx, gval, ids_restore, Tk, B, S, E, k)
    want = _compact_ref(rowidx, gval, ids_restore, Tk, B, S, E, k)
    for name, a, b in zip(("rowidx_c", "gval_c", "count", "slot_c"), got, want):
        assert torch.equal(a, b), (case, name)
    rowidx_c, gval_c, count, slot_c = got
    assert torch.equal(slot_c[mask.view(-1) > 0], torch.full((int((mask > 0).sum()), E), -1, device="cuda", dtype=I32)), "dropped tokens: -1 everywhere"
    if case == "all_kept":
        assert torch.equal(rowidx_c, rowidx) and torch.equal(gval_c, gval) and int(count.min()) == B * k
        n = (torch.arange(B * S, device="cuda") // S).view(-1, 1).to(I32)
        assert torch.equal(slot_c, torch.where(slot >= 0, n * k + slot, slot))
    if case == "crafted":
        assert int(count[1]) == B * k, "expert 1's picks are all kept"
        assert not bool(((rowidx_c[0, :int(count[0])] // S) == 0).any()), "expert 0 keeps nothing of sample 0"
        assert int(count[0]) < B * k


def _routed(hip, B, S, E, k, C, seed):
    g = torch.Generator().manual_seed(seed)
    probs, rowidx, gval, slot, ld = _route(hip, torch.randn(B * S, E, generator=g).cuda(), B, S, E, k)
    r = lambda *s: torch.randn(*s, generator=g).cuda().to(BF16)
    return g, probs, rowidx, gval, slot, ld, r


@pytest.mark.parametrize("E", [8, 4])
def test_absolute_position_kernels_equal_the_existing_ones_on_full_lists(hip, E):
    """Compact list = full list (everything kept): combine, scatter-sum and softmax backward must give the bits of the existing
    entry points on every token row."""
    L = hip.lib()
    B, S, k, C = 3, 32, 8, 128
    g, probs, rowidx, gval, slot, ld, r = _routed(hip, B, S, E, k, C, 21 + E)
    ids_restore, _ = _mask(hip, torch.rand(B, S, generator=g).cuda(), B, S, S)
    rowidx_c, gval_c, count, slot_c = _compact(hip, rowidx, gval, ids_restore, S, B, S, E, k)
    Bk, M = B * k, B * S
    h2, res, gate = r(E, Bk, C), r(M, C), r(B, 6 * C)
    out = {}
    for which in ("old", "abs"):
        br, x3 = torch.empty(M, C, device="cuda", dtype=BF16), torch.empty(M, C, device="cuda", dtype=BF16)
        if which == "old":
            hip.check(L.md_moe_combine(h2.data_ptr(), gval.data_ptr(), slot.data_ptr(), res.data_ptr(), gate.data_ptr() + 2 * 5 * C, 6 * C,
                                       br.data_ptr(), x3.data_ptr(), B, S, E, k, C, _st()), "combine")
        else:
            hip.check(L.md_moe_combine_abs(h2.data_ptr(), gval_c.data_ptr(), slot_c.data_ptr(), res.data_ptr(), gate.data_ptr() + 2 * 5 * C, 6 * C,
                                           br.data_ptr(), x3.data_ptr(), B, S, E, Bk, C, _st()), "combine_abs")
        out[which] = (br, x3)
    assert torch.equal(out["old"][0], out["abs"][0]) and torch.equal(out["old"][1], out["abs"][1])
    dxin, dgval = r(E, Bk, C), torch.randn(E, Bk, generator=g).cuda()
    for which in ("old", "abs"):
        dx, dlog = torch.empty(M, C, device="cuda", dtype=BF16), torch.empty(M, ld, device="cuda", dtype=BF16)
        if which == "old":
            hip.check(L.md_moe_dispatch_bwd(dxin.data_ptr(), slot.data_ptr(), dx.data_ptr(), probs.data_ptr(), ld, dgval.data_ptr(), dlog.data_ptr(),
                                            ld, B, S, E, k, C, _st()), "dispatch_bwd")
        else:
            hip.check(L.md_moe_dispatch_bwd_abs(dxin.data_ptr(), slot_c.data_ptr(), dx.data_ptr(), probs.data_ptr(), ld, dgval.data_ptr(),
                                                dlog.data_ptr(), ld, B, S, E, Bk, C, _st()), "dispatch_bwd_abs")
        out[which] = (dx, dlog)
    torch.cuda.synchronize()
    assert torch.equal(out["old"][0], out["abs"][0]) and torch.equal(out["old"][1], out["abs"][1])


def test_compact_lists_under_a_mask_against_torch(hip):
    """Tk < S at C = 128, cap < stride: the gather and the combine backward touch the first cap rows of every expert and give the bits
    of the flat entry points there; the combine and the dispatch backward write EVERY token row -- kept rows as a dense pass over the
    kept routed rows would, dropped rows br = 0, out = res, dx = 0, dlogits = 0 -- from buffers whose unused rows hold NaN."""
    L = hip.lib()
    B, S, E, k, C, Tk = 3, 32, 8, 8, 128, 8
    g, probs, rowidx, gval, slot, ld, r = _routed(hip, B, S, E, k, C, 31)
    ids_restore, mask = _mask(hip, torch.rand(B, S, generator=g).cuda(), B, S, Tk)
    rowidx_c, gval_c, count, slot_c = _compact(hip, rowidx, gval, ids_restore, Tk, B, S, E, k)
    Bk, M = B * k, B * S
    cap = (int(count.max()) + 3) // 4 * 4
    assert 0 < cap < Bk
    src = r(M, C)
    nan = float("nan")
    xin = torch.full((E, Bk, C), nan, device="cuda", dtype=BF16)
    hip.check(L.md_moe_gather_compact(src.data_ptr(), C, rowidx_c.data_ptr(), xin.data_ptr(), E, cap, Bk, C, _st()), "gather_compact")
    assert torch.equal(xin[:, :cap], src[rowidx_c[:, :cap].long()]) and bool(torch.isnan(xin[:, cap:].float()).all())
    # combine backward on the compact lists against the flat kernel on the same (rowidx_c, gval_c)
    dbr, h2 = r(M, C), torch.full((E, Bk, C), nan, device="cuda", dtype=BF16)
    h2[:, :cap] = r(E, cap, C)
    dh2 = torch.full((E, Bk, C), nan, device="cuda", dtype=BF16)
    dg = torch.full((E, Bk), nan, device="cuda", dtype=F32)
    hip.check(L.md_moe_combine_bwd_compact(dbr.data_ptr(), h2.data_ptr(), rowidx_c.data_ptr(), gval_c.data_ptr(), dh2.data_ptr(), dg.data_ptr(),
                                           E, cap, Bk, C, _st()), "combine_bwd_compact")
    h2f = torch.where(torch.isnan(h2.float()), torch.zeros((), device="cuda"), h2.float()).to(BF16)
    dh2f, dgf = torch.empty(E, Bk, C, device="cuda", dtype=BF16), torch.empty(E, Bk, device="cuda", dtype=F32)
    hip.check(L.md_moe_combine_bwd(dbr.data_ptr(), h2f.data_ptr(), rowidx_c.data_ptr(), gval_c.data_ptr(), dh2f.data_ptr(), dgf.data_ptr(), E * Bk, C,
                                   _st()), "combine_bwd")
    assert torch.equal(dh2[:, :cap], dh2f[:, :cap]) and torch.equal(dg[:, :cap], dgf[:, :cap])
    assert bool(torch.isnan(dh2[:, cap:].float()).all()) and bool(torch.isnan(dg[:, cap:]).all())
    for e in range(E):
        assert not bool(dh2[e, int(count[e]):cap].float().abs().any()), "pad rows: gate value 0 -> dh2 = 0"
    # combine: the dense entry point with the dropped rows' slots removed is the restatement
    slot_kept = torch.where(mask.view(-1, 1) > 0, torch.full_like(slot, -1), slot)
    h2d = torch.zeros(E, Bk, C, device="cuda", dtype=BF16)               # dense layout (e, n*k + rank) of the same expert rows
    n_of = (torch.arange(M, device="cuda") // S)
    for e in range(E):
        toks = rowidx_c[e, :int(count[e])].long()
        h2d[e, n_of[toks] * k + slot[toks, e].long()] = h2[e, :int(count[e])]
    res, gate = r(M, C), r(B, 6 * C)
    o = {}
    for which in ("dense", "abs"):
        br, x3 = torch.empty(M, C, device="cuda", dtype=BF16), torch.empty(M, C, device="cuda", dtype=BF16)
        if which == "dense":
            hip.check(L.md_moe_combine(h2d.data_ptr(), gval.data_ptr(), slot_kept.data_ptr(), res.data_ptr(), gate.data_ptr(), 6 * C, br.data_ptr(),
                                       x3.data_ptr(), B, S, E, k, C, _st()), "combine")
        else:
            hip.check(L.md_moe_combine_abs(h2.data_ptr(), gval_c.data_ptr(), slot_c.data_ptr(), res.data_ptr(), gate.data_ptr(), 6 * C, br.data_ptr(),
                                           x3.data_ptr(), B, S, E, Bk, C, _st()), "combine_abs")
        o[which] = (br, x3)
    assert torch.equal(o["dense"][0], o["abs"][0]) and torch.equal(o["dense"][1], o["abs"][1])
    drop = mask.view(-1) > 0
    assert not bool(o["abs"][0][drop].float().abs().any()) and torch.equal(o["abs"][1][drop], res[drop])
    # dispatch backward
    dxin = torch.full((E, Bk, C), nan, device="cuda", dtype=BF16)
    dxin[:, :cap] = r(E, cap, C)
    dgv = torch.full((E, Bk), nan, device="cuda", dtype=F32)
    dgv[:, :cap] = torch.randn(E, cap, generator=g).cuda()
    dxind, dgvd = torch.zeros(E, Bk, C, device="cuda", dtype=BF16), torch.zeros(E, Bk, device="cuda", dtype=F32)
    for e in range(E):
        toks = rowidx_c[e, :int(count[e])].long()
        dxind[e, n_of[toks] * k + slot[toks, e].long()] = dxin[e, :int(count[e])]
        dgvd[e, n_of[toks] * k + slot[toks, e].long()] = dgv[e, :int(count[e])]
    for which in ("dense", "abs"):
        dx, dlog = torch.empty(M, C, device="cuda", dtype=BF16), torch.empty(M, ld, device="cuda", dtype=BF16)
        if which == "dense":
            hip.check(L.md_moe_dispatch_bwd(dxind.data_ptr(), slot_kept.data_ptr(), dx.data_ptr(), probs.data_ptr(), ld, dgvd.data_ptr(), dlog.data_ptr(),
                                            ld, B, S, E, k, C, _st()), "dispatch_bwd")
        else:
            hip.check(L.md_moe_dispatch_bwd_abs(dxin.data_ptr(), slot_c.data_ptr(), dx.data_ptr(), probs.data_ptr(), ld, dgv.data_ptr(), dlog.data_ptr(),
                                                ld, B, S, E, Bk, C, _st()), "dispatch_bwd_abs")
        o[which] = (dx, dlog)
    torch.cuda.synchronize()
    assert torch.equal(o["dense"][0], o["abs"][0]) and torch.equal(o["dense"][1], o["abs"][1])
    assert not bool(o["abs"][0][drop].float().abs().any()) and not bool(o["abs"][1][drop].float().abs().any())


# ------------------------------------------------------------------------------------------------ engine, Tiny config
def _product(cfg, sd, ratio):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), train_mask_ratio=ratio)
    m.train()
    return m


def _close(a, b):
    """The per-tensor bound tests/test_trainer_gpu.py uses for "same math, other launch shape" (grouped against per-layer)."""
    a, b = a.double(), b.double()
    return float((a - b).norm()), 1e-2 * float(b.norm()) + 1e-12


def _engine_run(prune, *, ratio=0.75, backward, seed=61, override=None, mnoise=None, granule=8):
    cfg = orc.tiny_config()
    sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, seed))
    batch, rnd, epsn, mn = orc.synth_batch(cfg, 4, seed + 1)
    gb = {k: t.cuda() for k, t in batch.items()}
    noise = (rnd.cuda(), epsn.cuda(), (mn if mnoise is None else mnoise).cuda())
    m = _product(cfg, sd, ratio)
    eng = m.dit.engine
    assert eng.mixer[-1].moe, "the Tiny config's last patch-mixer block is MoE"
    assert eng.prune_masked_experts, "the switch is on by default"
    eng.prune_masked_experts, eng.prune_granule, eng.deterministic = prune, granule, True
    eng.gemm_log, eng.route_log, eng.keep_last_tape = [], [], True
    if override is not None:
        eng.route_override = {eng.mixer[-1].name: override}
    m._noise_fn = lambda b: noise
    if backward:
        loss = m.train_microbatch(gb)
    else:
        with torch.no_grad():
            loss = m.forward(gb)[0]
    torch.cuda.synchronize()
    tp = eng.last_tape
    bt = tp.mixer[-1] if tp.mixer else None
    return dict(loss=loss.detach().float().clone(), xout_in=tp.xout_in.clone(), cap=getattr(bt, "cap", None), Bk=4 * bt.k if bt is not None else None,
                grads={k: p.grad.clone() for k, p in m.dit.named_parameters()} if backward else None,
                gemm_log=list(eng.gemm_log), route_log=list(eng.route_log),
                routing={k: getattr(bt, k).clone() for k in ("probs", "rowidx", "gval", "slot")} if bt is not None else None)


def test_engine_forward_on_equals_off(hip):
    on, off = _engine_run(True, backward=False), _engine_run(False, backward=False)
    assert on["cap"] is not None and on["cap"] < on["Bk"], "pruning must engage at mask 0.75 with a small granule"
    assert off["cap"] is None and "compact_kept" in on["route_log"] and "compact_kept" not in off["route_log"]
    for k in on["routing"]:
        assert torch.equal(on["routing"][k], off["routing"][k]), f"the tape's {k} is that of the dense pass"
    assert len(on["gemm_log"]) == len(off["gemm_log"])
    same_family = all(a[0] == b[0] for a, b in zip(on["gemm_log"], off["gemm_log"]))
    for name in ("xout_in", "loss"):
        diff, bound = _close(on[name], off[name])
        print(f"forward {name}: |on - off| = {diff:.3e}, bound {bound:.3e}, same kernel families: {same_family}")
        if same_family:
            assert torch.equal(on[name], off[name]), name
        assert diff <= bound, name


def test_engine_gradients_on_equal_off(hip):
    on, off = _engine_run(True, backward=True), _engine_run(False, backward=True)
    assert on["cap"] is not None and on["cap"] < on["Bk"]
    assert "combine_bwd_compact" in on["route_log"] and "dispatch_bwd_abs" in on["route_log"]
    worst = max(((_close(on["grads"][k], off["grads"][k]), k) for k in on["grads"]), key=lambda t: t[0][0] / t[0][1])
    print("worst tensor:", worst)
    for k in on["grads"]:
        assert bool(torch.isfinite(on["grads"][k]).all()), k
        diff, bound = _close(on["grads"][k], off["grads"][k])
        assert diff <= bound, (k, diff, bound)


def test_dense_fallback_under_route_override_equals_off(hip):
    """Expert 0 of every sample takes tokens 0 .. k-1 and the mask keeps exactly those (k == Tk on the Tiny config): its compact list
    is as long as the full one, so the block runs dense -- the off run's launches, the off run's bits."""
    cfg = orc.tiny_config()
    B, T, E = 4, 256, cfg.num_experts
    k = int(cfg.expert_capacity * T / E)
    assert k == int(T * 0.25)
    ov = torch.stack([(torch.arange(k) + 5 * e) % T for e in range(E)]).view(1, E, k).expand(B, E, k).contiguous()
    mn = torch.rand(B, T, generator=torch.Generator().manual_seed(3)) * 0.5 + 0.5
    mn[:, :k] *= 0.1
    on = _engine_run(True, backward=True, override=ov, mnoise=mn)
    off = _engine_run(False, backward=True, override=ov, mnoise=mn)
    assert on["cap"] is None and "compact_kept" in on["route_log"] and "combine_abs" not in on["route_log"]
    assert on["gemm_log"] == off["gemm_log"]
    assert torch.equal(on["loss"], off["loss"]) and torch.equal(on["xout_in"], off["xout_in"])
    for kk in on["grads"]:
        assert torch.equal(on["grads"][kk], off["grads"][kk]), kk


def test_mask_zero_launch_log_is_unchanged(hip):
    on, off = _engine_run(True, ratio=0.0, backward=True), _engine_run(False, ratio=0.0, backward=True)
    assert on["gemm_log"] == off["gemm_log"] and on["route_log"] == off["route_log"] and len(on["route_log"]) > 0
    assert "compact_kept" not in on["route_log"]
    assert torch.equal(on["loss"], off["loss"])
