"""Model diagnostics on the GPU: md_loss_sigma_hist and md_moe_route_stats through the C ABI against torch fp64,
then the engine, the Trainer and two data-parallel ranks.

Bounds.  Counts are integers: exact.  Loss / marginal / gate sums are fp64 accumulations of at most a few thousand fp32 values, in
another order than torch's: each differs from the exact sum by at most n * 2^-53 relative (positive addends), ~5e-13 for n = 4096 --
1e-11 relative.  The entropy sum is an fp64 sum of per-token fp32 values -sum_e p ln p whose device logf and fp32 products are good
to a few ulp (~1e-7 relative per term, positive terms): 1e-5 relative against fp64 on the same fp32 probabilities."""
import ctypes
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_SUM, REL_ENT = 1e-11, 1e-5
LOG_LO, LOG_HI = -0.6 - 3.6, -0.6 + 3.6


def _close(got, want, rel):
    got, want = got.double().cpu(), want.double().cpu()
    return bool(((got - want).abs() <= rel * want.abs()).all())


# ------------------------------------------------------------------------------------------------ md_loss_sigma_hist
def _bins(sigma, nbins, dtype):
    """The bin rule of the header in `dtype` arithmetic (CPU)."""
    lo, hi = torch.tensor(LOG_LO, dtype=dtype), torch.tensor(LOG_HI, dtype=dtype)
    t = torch.floor((torch.log(sigma.to(dtype)) - lo) * nbins / (hi - lo))
    return t.clamp(0, nbins - 1).long()


def _hist_inputs(B, nbins, seed):
    """sigma a quarter of a bin or more inside its bin (device logf and torch's log then agree on the bin), a few far outside the
    range (the clamp), NaN and +inf losses when there is room for them."""
    g = torch.Generator().manual_seed(seed)
    w = (LOG_HI - LOG_LO) / nbins
    b = torch.randint(0, nbins, (B,), generator=g)
    u = 0.25 + 0.5 * torch.rand(B, generator=g, dtype=torch.float64)
    ln = LOG_LO + (b.double() + u) * w
    want_bin = b.clone()
    if B >= 8:
        ln[1], ln[B - 2], ln[B // 2] = -20.0, 15.0, LOG_HI + 3.0 * w
        want_bin[1], want_bin[B - 2], want_bin[B // 2] = 0, nbins - 1, nbins - 1
    sigma = torch.exp(ln).float()
    loss = (torch.rand(B, generator=g) * 10.0 + 0.01).float()
    if B >= 8:
        loss[0], loss[B - 1], loss[B // 3] = float("nan"), float("inf"), float("nan")
    # CPU check of the inputs themselves: fp32 and fp64 evaluation of the rule agree with the intended bin
    assert torch.equal(_bins(sigma, nbins, torch.float32), want_bin) and torch.equal(_bins(sigma, nbins, torch.float64), want_bin)
    return sigma, loss, want_bin


def _hist_ref(loss, bins, nbins):
    fin = torch.isfinite(loss)
    s = torch.zeros(nbins, dtype=torch.float64).index_add_(0, bins[fin], loss[fin].double())
    c = torch.zeros(nbins, dtype=torch.int64).index_add_(0, bins[fin], torch.ones(int(fin.sum()), dtype=torch.int64))
    return s, c, int((~fin).sum())


def _hist_call(hip, sigma, loss, nbins, tables=None, lo=LOG_LO, hi=LOG_HI, B=None):
    sm, cnt, nf = tables if tables is not None else (torch.zeros(nbins, device=DEV, dtype=torch.float64),
                                                    torch.zeros(nbins, device=DEV, dtype=torch.int64),
                                                    torch.zeros(1, device=DEV, dtype=torch.int64))
    rc = hip.lib().md_loss_sigma_hist(sigma.data_ptr(), loss.data_ptr(), sigma.numel() if B is None else B, lo, hi, nbins,
                                      sm.data_ptr(), cnt.data_ptr(), nf.data_ptr(), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, (sm, cnt, nf)


@pytest.mark.parametrize("nbins", [1, 16, 64])
@pytest.mark.parametrize("B", [1, 65, 1000])
def test_loss_sigma_hist_matches_fp64(hip, B, nbins):
    sigma, loss, bins = _hist_inputs(B, nbins, 100 * B + nbins)
    ref_s, ref_c, ref_nf = _hist_ref(loss, bins, nbins)
    assert int(ref_c.sum()) + ref_nf == B and (B < 8 or ref_nf == 3)
    sg, ls = sigma.to(DEV), loss.to(DEV)
    rc, (sm, cnt, nf) = _hist_call(hip, sg, ls, nbins)
    assert rc == 0
    print(f"B={B} nbins={nbins}: worst relative sum error {float(((sm.cpu() - ref_s).abs() / ref_s.abs().clamp(min=1e-300)).max()):.2e}")
    assert torch.equal(cnt.cpu(), ref_c), "counts are exact"
    assert int(nf) == ref_nf, "non-finite losses are counted, exactly"
    assert bool(torch.isfinite(sm).all()) and _close(sm, ref_s, REL_SUM), "a non-finite loss must not leak into the sums"
    # a second call into the same tables: everything is ADDED TO
    rc, _ = _hist_call(hip, sg, ls, nbins, (sm, cnt, nf))
    assert rc == 0 and torch.equal(cnt.cpu(), 2 * ref_c) and int(nf) == 2 * ref_nf and _close(sm, 2 * ref_s, REL_SUM)
    # two fresh calls: identical bits
    a, b = _hist_call(hip, sg, ls, nbins)[1], _hist_call(hip, sg, ls, nbins)[1]
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_loss_sigma_hist_refuses_bad_arguments(hip):
    sigma, loss, _ = _hist_inputs(65, 16, 7)
    sg, ls = sigma.to(DEV), loss.to(DEV)
    L, st = hip.lib(), hip.stream_ptr()

    def fresh():
        return (torch.full((16,), 3.5, device=DEV, dtype=torch.float64), torch.full((16,), 7, device=DEV, dtype=torch.int64),
                torch.full((1,), 9, device=DEV, dtype=torch.int64))

    def untouched(t):
        return bool((t[0] == 3.5).all()) and bool((t[1] == 7).all()) and int(t[2]) == 9
    t = fresh()
    for kw in (dict(B=0), dict(B=-3), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0)):
        rc, _ = _hist_call(hip, sg, ls, 16, t, **kw)
        assert rc == -1 and untouched(t), kw
    for nb in (0, 65, -1):
        assert L.md_loss_sigma_hist(sg.data_ptr(), ls.data_ptr(), 65, LOG_LO, LOG_HI, nb, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), st) == -1
    ptrs = [sg.data_ptr(), ls.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()]
    for i in range(5):
        p = list(ptrs)
        p[i] = None
        assert L.md_loss_sigma_hist(p[0], p[1], 65, LOG_LO, LOG_HI, 16, p[2], p[3], p[4], st) == -1, f"null pointer {i}"
    torch.cuda.synchronize()
    assert untouched(t)


# ------------------------------------------------------------------------------------------------ md_moe_route_stats
ROUTE_SHAPES = [(1, 8, 8, 1), (3, 64, 8, 8), (2, 256, 8, 32), (5, 100, 4, 25), (2, 64, 16, 4)]


def _route(hip, B, S, E, k, ldp, seed):
    """slot / probs / gval of the real md_moe_route on random logits (one row with -1e30 entries: some p exactly 0); the padding
    columns of probs are then filled with NaN."""
    g = torch.Generator().manual_seed(seed)
    M = B * S
    logits = (torch.randn(M, ldp, generator=g) * 2.0).float()
    logits[M // 2, 1:E - 1] = -1e30
    logits = logits.to(DEV)
    probs = torch.empty(M, ldp, device=DEV)
    rowidx = torch.empty(E, B * k, device=DEV, dtype=torch.int32)
    gval = torch.empty(E, B * k, device=DEV)
    slot = torch.empty(M, E, device=DEV, dtype=torch.int32)
    hip.check(hip.lib().md_moe_route(logits.data_ptr(), probs.data_ptr(), ldp, B, S, E, k, rowidx.data_ptr(), gval.data_ptr(),
                                     slot.data_ptr(), hip.stream_ptr()), "md_moe_route")
    probs[:, E:] = float("nan")
    torch.cuda.synchronize()
    assert int((probs[M // 2, :E] == 0).sum()) == E - 2, "the -1e30 logits must give probabilities that are exactly 0"
    return slot, probs, gval


def _route_ref(slot, probs, gval, E):
    hist = torch.bincount((slot >= 0).sum(1).cpu(), minlength=E + 1)
    p = probs[:, :E].double().cpu()
    ent = -(torch.where(p > 0, p * torch.log(p), torch.zeros_like(p))).sum()
    return hist, torch.cat([ent.reshape(1), p.sum(0), gval.double().cpu().sum(1)])


def _ws(hip, B, S, E):
    n = ctypes.c_int64(0)
    assert hip.lib().md_moe_route_stats_ws_floats(B, S, E, ctypes.byref(n)) == 0 and n.value > 0
    return torch.full((n.value,), float("nan"), device=DEV)             # NaN: the workspace needs no initialisation


def _stats_call(hip, slot, probs, gval, B, S, E, k, ws, hist=None, f=None, ws_floats=None):
    hist = torch.zeros(E + 1, device=DEV, dtype=torch.int64) if hist is None else hist
    f = torch.zeros(1 + 2 * E, device=DEV, dtype=torch.float64) if f is None else f
    rc = hip.lib().md_moe_route_stats(slot.data_ptr(), probs.data_ptr(), probs.shape[1], gval.data_ptr(), B, S, E, k, ws.data_ptr(),
                                      ws.numel() if ws_floats is None else ws_floats, hist.data_ptr(), f.data_ptr(), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, hist, f


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B,S,E,k", ROUTE_SHAPES)
def test_route_stats_match_torch(hip, B, S, E, k, pad):
    slot, probs, gval = _route(hip, B, S, E, k, E + pad, 1000 * S + 10 * E + pad)
    ref_h, ref_f = _route_ref(slot, probs, gval, E)
    rc, hist, f = _stats_call(hip, slot, probs, gval, B, S, E, k, _ws(hip, B, S, E))
    assert rc == 0
    err = ((f.cpu() - ref_f).abs() / ref_f.abs()).tolist()
    print(f"B={B} S={S} E={E} k={k} ldp={E + pad}: relative error entropy {err[0]:.2e}, marginals {max(err[1:1 + E]):.2e}, gates {max(err[1 + E:]):.2e}")
    assert torch.equal(hist.cpu(), ref_h), (hist.tolist(), ref_h.tolist())
    assert int((hist.cpu() * torch.arange(E + 1)).sum()) == E * B * k, "every chosen entry is some token's"
    assert bool(torch.isfinite(f).all()), "a padding column (NaN) or the workspace's NaN was read"
    assert _close(f[1:], ref_f[1:], REL_SUM), "marginal and gate sums"
    assert _close(f[:1], ref_f[:1], REL_ENT), "entropy sum"
    # identical bits from a second call (fresh tables, fresh NaN workspace)
    rc, hist2, f2 = _stats_call(hip, slot, probs, gval, B, S, E, k, _ws(hip, B, S, E))
    assert rc == 0 and torch.equal(hist2, hist) and torch.equal(f2, f)
    # accumulation into a table that is not zero
    h0 = torch.arange(5, 5 + E + 1, device=DEV, dtype=torch.int64)
    f0 = torch.linspace(1.5, 9.5, 1 + 2 * E, device=DEV, dtype=torch.float64)
    rc, h3, f3 = _stats_call(hip, slot, probs, gval, B, S, E, k, _ws(hip, B, S, E), h0.clone(), f0.clone())
    assert rc == 0 and torch.equal(h3, h0 + hist) and torch.equal(f3, f0 + f), "outputs are ADDED TO: table + this call's sums"


def test_route_stats_refuse_bad_arguments(hip):
    B, S, E, k = 3, 64, 8, 8
    slot, probs, gval = _route(hip, B, S, E, k, E, 5)
    ws = _ws(hip, B, S, E)
    L, st = hip.lib(), hip.stream_ptr()
    hist = torch.full((E + 1,), 7, device=DEV, dtype=torch.int64)
    f = torch.full((1 + 2 * E,), 3.5, device=DEV, dtype=torch.float64)
    rc, _, _ = _stats_call(hip, slot, probs, gval, B, S, E, k, ws, hist, f, ws_floats=ws.numel() - 1)
    assert rc == -1, "a workspace one float short"
    n = ctypes.c_int64(-5)
    assert L.md_moe_route_stats_ws_floats(B, S, 17, ctypes.byref(n)) == -1 and L.md_moe_route_stats_ws_floats(0, S, E, ctypes.byref(n)) == -1
    assert L.md_moe_route_stats_ws_floats(B, S, E, None) == -1 and n.value == -5
    args = [slot.data_ptr(), probs.data_ptr(), E, gval.data_ptr(), B, S, E, k, ws.data_ptr(), ws.numel(), hist.data_ptr(), f.data_ptr()]
    for i, bad in [(0, None), (1, None), (3, None), (8, None), (10, None), (11, None), (2, E - 1), (4, 0), (5, 0), (6, 0), (6, 17), (7, 0),
                   (7, S + 1), (8, ws.data_ptr() + 4)]:
        a = list(args)
        a[i] = bad
        assert L.md_moe_route_stats(*a, st) == -1, f"argument {i} = {bad}"
    torch.cuda.synchronize()
    assert bool((hist == 7).all()) and bool((f == 3.5).all()), "a refused call writes nothing"


# ------------------------------------------------------------------------------------------------ engine
def _model(cfg, sd, ratio):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd)
    m = LatentDiffusion(d.to(DEV), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), train_mask_ratio=ratio)
    m.train()
    return m


_CASES = {}


def _case(name):
    """(cfg, state dict, batch on the device, noise) of the small MoE configurations, built once."""
    if name not in _CASES:
        cfgf, seed, ratio, cap = {"micro": (orc.micro_config, 63, 0.5, 20), "tiny": (orc.tiny_config, 61, 0.75, 77)}[name]
        cfg = cfgf()
        sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, seed))
        batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 4, seed + 1, cap_len=cap)
        _CASES[name] = (cfg, sd, {k: t.to(DEV) for k, t in batch.items()}, (rnd.to(DEV), epsn.to(DEV), mnoise.to(DEV)), ratio)
    return _CASES[name]


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_engine_rows_equal_the_recomputation_from_the_tape(hip, name):
    from micro_diffusion_amd.diagnostics import RouteStats
    cfg, sd, gb, noise, ratio = _case(name)
    m = _model(cfg, sd, ratio)
    eng = m.dit.engine
    assert eng.route_stats is None and m.loss_by_sigma is None, "off by default"
    eng.route_stats = rs = RouteStats(eng)
    eng.keep_last_tape = True
    m._noise_fn = lambda b: noise
    with torch.no_grad():
        m.forward({k: v.clone() for k, v in gb.items()})
    torch.cuda.synchronize()
    tape = eng.last_tape
    routed = [(bp.name, t) for bp, t in zip(list(eng.mixer) + list(eng.backbone), tape.mixer + tape.blocks) if bp.moe]
    assert [n for n, _ in routed] == rs.names and len(routed) >= 1
    assert all(n.startswith(("patch_mixer.", "blocks.")) for n in rs.names)
    E = cfg.num_experts
    for i, (n, t) in enumerate(routed):
        ref_h, ref_f = _route_ref(t.slot, t.probs, t.gval, E)
        assert int(ref_h.sum()) == t.slot.shape[0]
        assert torch.equal(rs.cover_hist[i].cpu(), ref_h), n
        assert _close(rs.fstats[i, 1:], ref_f[1:], REL_SUM) and _close(rs.fstats[i, :1], ref_f[:1], REL_ENT), n


def test_engine_rows_describe_an_injected_routing(hip):
    """With the oracle-routing test hook the statistics are those of the routing the layer ran with."""
    from micro_diffusion_amd.diagnostics import RouteStats
    cfg, sd, gb, noise, ratio = _case("tiny")
    m = _model(cfg, sd, ratio)
    eng = m.dit.engine
    eng.route_stats = rs = RouteStats(eng)
    B, T, E = 4, eng.cfg.tokens, cfg.num_experts
    k = int(cfg.expert_capacity * T / E)
    # every expert of every sample takes tokens 0 .. k-1: those are covered E times, the rest never
    eng.route_override = {rs.names[0]: torch.arange(k).view(1, 1, k).expand(B, E, k).contiguous()}
    m._noise_fn = lambda b: noise
    with torch.no_grad():
        m.forward({k: v.clone() for k, v in gb.items()})
    torch.cuda.synchronize()
    want = torch.zeros(E + 1, dtype=torch.int64)
    want[0], want[E] = B * (T - k), B * k
    assert torch.equal(rs.cover_hist[0].cpu(), want), rs.cover_hist[0].tolist()


def _grad_run(name, arm):
    from micro_diffusion_amd.diagnostics import LossBySigma, RouteStats
    cfg, sd, gb, noise, ratio = _case(name)
    m = _model(cfg, sd, ratio)
    eng = m.dit.engine
    eng.use_arena = True
    if arm:
        eng.route_stats = RouteStats(eng)
        m.loss_by_sigma = LossBySigma(16)
    m._noise_fn = lambda b: noise
    addr = []
    for _ in range(2):                  # the first pass measures the arenas, the second runs inside them
        for p in m.dit.parameters():
            if p.grad is not None:
                p.grad.zero_()
        loss = m.train_microbatch(dict(gb))
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.dit.named_parameters()}
    return loss.detach().clone(), grads, (dict(eng._tape_arena.peaks), dict(eng._scratch_arena.peaks)), m


def test_armed_step_has_the_bits_and_the_arenas_of_an_unarmed_one(hip, monkeypatch):
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    loss0, g0, arenas0, m0 = _grad_run("micro", False)
    loss1, g1, arenas1, m1 = _grad_run("micro", True)
    assert m0.dit.engine.deterministic and m1.dit.engine.deterministic
    assert torch.equal(loss0, loss1), (loss0, loss1)
    differ = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not differ and len(g0) > 20, differ[:4]
    assert arenas0 == arenas1 and arenas0[0] and arenas0[1], "arena high-water marks"
    cnt, _ = m1.loss_by_sigma.tables("train", DEV)
    assert int(cnt[:-1].sum()) == 2 * 4 and int(cnt[-1]) == 0, "two passes of four samples went into the train table"
    assert int(m1.dit.engine.route_stats.cover_hist[0].sum()) > 0


def test_nothing_new_is_called_while_everything_is_off(hip):
    """Spy on the bound functions: an unarmed step (the default) calls none of the new symbols; an armed one calls them."""
    from micro_diffusion_amd.diagnostics import LossBySigma, RouteStats
    cfg, sd, gb, noise, ratio = _case("tiny")
    L = hip.lib()
    names = ("md_loss_sigma_hist", "md_moe_route_stats", "md_moe_route_stats_ws_floats")
    real = {n: getattr(L, n) for n in names}
    calls = {n: 0 for n in names}

    def spy(n):
        def f(*a):
            calls[n] += 1
            return real[n](*a)
        return f
    try:
        for n in names:
            setattr(L, n, spy(n))
        m = _model(cfg, sd, ratio)
        m._noise_fn = lambda b: noise
        m.train_microbatch(dict(gb))
        with torch.no_grad():
            m.forward({k: v.clone() for k, v in gb.items()})
        torch.cuda.synchronize()
        assert calls == {n: 0 for n in names}, calls
        m.dit.engine.route_stats = RouteStats(m.dit.engine)
        m.loss_by_sigma = LossBySigma(8)
        m.train_microbatch(dict(gb))
        torch.cuda.synchronize()
        assert calls["md_loss_sigma_hist"] == 1 and calls["md_moe_route_stats"] == len(m.dit.engine.route_stats.names) >= 1
        assert calls["md_moe_route_stats_ws_floats"] == 1, "the workspace is sized once per shape"
    finally:
        for n in names:
            setattr(L, n, real[n])


# ------------------------------------------------------------------------------------------------ Trainer
def _trainer(cfg, sd, ratio, microbatch, **kw):
    from micro_diffusion_amd.trainer import FusedAdamW, LRSchedule, Trainer
    model = _model(cfg, sd, ratio)
    opt = FusedAdamW(model.dit, lr=2.4e-4)
    return model, Trainer(model, opt, LRSchedule("constant", alpha=1.0), clip_norm=0.25, microbatch_size=microbatch, **kw)


def _mean_from(d, which):
    pre = f"loss_by_sigma/{which}/"
    tot = sum(m * c for m, c in zip(d[pre + "mean_loss"], d[pre + "count"]) if c)
    return tot / max(sum(d[pre + "count"]), 1)


def test_trainer_two_steps_of_two_microbatches(hip):
    cfg, sd, _, _, ratio = _case("tiny")
    model, tr = _trainer(cfg, sd, ratio, 2, diagnostics_interval=2, loss_by_sigma_bins=8, moe_routing=True)
    E, block = cfg.num_experts, "patch_mixer.1"
    assert model.loss_by_sigma is not None and model.loss_by_sigma.nbins == 8 and model.dit.engine.route_stats is None
    for step in range(2):
        batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 4, 170 + step)
        chunks = [(rnd[i:i + 2].to(DEV), epsn[i:i + 2].to(DEV), mnoise[i:i + 2].to(DEV)) for i in range(0, 4, 2)]
        model._noise_fn = lambda b, c=chunks: c.pop(0)
        loss = float(tr.train_step({k: t.to(DEV) for k, t in batch.items()}))
        assert model.dit.engine.route_stats is None, "routing statistics are armed for the microbatches of a report batch only"
        d = tr.diagnostics()
        pre = "loss_by_sigma/train/"
        assert sum(d[pre + "count"]) == 4 and d[pre + "nonfinite"] == 0, "one step's samples: the previous read zeroed the table"
        assert len(d[pre + "ln_sigma_edges"]) == 9 and d[pre + "ln_sigma_edges"][0] == pytest.approx(-4.2)
        got = _mean_from(d, "train")
        print(f"step {step}: loss {loss!r}, sum / count of the histogram {got!r}")
        assert abs(got - loss) <= 1e-5 * abs(loss)
        assert sum(d["loss_by_sigma/eval/count"]) == 0, "the eval table stays empty while training"
        moe = [k for k in d if k.startswith("moe/")]
        if step == 0:
            assert not moe, "batch 1 is no multiple of diagnostics_interval = 2"
        else:
            assert sorted(moe) == sorted(f"moe/{block}/{k}" for k in ("coverage", "dropped_frac", "router_entropy", "expert_prob_mean",
                                                                      "expert_gate_mean"))
            cov = d[f"moe/{block}/coverage"]
            assert len(cov) == E + 1 and abs(sum(cov) - 1) < 1e-12 and d[f"moe/{block}/dropped_frac"] == cov[0]
            assert abs(sum(c * v for c, v in enumerate(cov)) - cfg.expert_capacity) < 1e-12, "a token is served by `capacity` experts on average"
            assert abs(sum(d[f"moe/{block}/expert_prob_mean"]) - 1) < 1e-5 and 0 < d[f"moe/{block}/router_entropy"] <= 2.0795
        again = tr.diagnostics()
        assert sum(again[pre + "count"]) == 0 and not [k for k in again if k.startswith("moe/")], "reading the diagnostics zeroes them"
    # eval goes to its own table
    batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 4, 180)
    model._noise_fn = lambda b: (rnd.to(DEV), epsn.to(DEV), mnoise.to(DEV))
    model.eval()
    with torch.no_grad():
        ev = float(model.eval_forward({k: t.to(DEV) for k, t in batch.items()})[0])
    model.train()
    d = tr.diagnostics(tables=("eval",), routing=False)
    assert set(d) == {"loss_by_sigma/eval/" + k for k in ("ln_sigma_edges", "count", "mean_loss", "nonfinite")}
    assert sum(d["loss_by_sigma/eval/count"]) == 4 and abs(_mean_from(d, "eval") - ev) <= 1e-5 * abs(ev)
    assert sum(tr.diagnostics()["loss_by_sigma/train/count"]) == 0


# ------------------------------------------------------------------------------------------------ two ranks on one GPU (gloo)
DP_SEED, DP_BATCH = 61, 8


def _dp_trainer(lo, hi, microbatch):
    cfg = orc.tiny_config()
    sd = orc.synth_state_dict(cfg, DP_SEED)
    batch, rnd, epsn, mnoise = orc.synth_batch(cfg, DP_BATCH, DP_SEED + 1)
    model, tr = _trainer(cfg, sd, 0.75, microbatch, exchange="fp32", dp_mode="allreduce", diagnostics_interval=1, loss_by_sigma_bins=8,
                         moe_routing=True)
    calls = {"n": 0}

    def noise_fn(B):
        a = lo + (calls["n"] * B) % (hi - lo)
        calls["n"] += 1
        return rnd[a:a + B].to(DEV), epsn[a:a + B].to(DEV), mnoise[a:a + B].to(DEV)
    model._noise_fn = noise_fn
    return tr, {k: v[lo:hi].to(DEV) for k, v in batch.items()}


def _dp_rank(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        per = DP_BATCH // world
        tr, part = _dp_trainer(rank * per, (rank + 1) * per, per)
        assert tr.world == world
        tr.train_step(part)
        torch.save(tr.diagnostics(), os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_ranks_combine_to_the_tables_of_one(hip):
    tr, part = _dp_trainer(0, DP_BATCH, DP_BATCH // 2)        # one rank, the whole batch as two microbatches
    tr.train_step(part)
    one = tr.diagnostics()
    del tr
    torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as td:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, td)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
        assert [p.exitcode for p in procs] == [0, 0]
        two = [torch.load(os.path.join(td, f"r{r}.pt")) for r in range(2)]
    assert two[0] == two[1], "every rank holds the same combined tables, bit for bit"
    assert set(two[0]) == set(one) and any(k.startswith("moe/") for k in one)
    assert sum(one["loss_by_sigma/train/count"]) == DP_BATCH
    for key, a in one.items():
        b = two[0][key]
        if key.endswith(("/count", "/nonfinite", "/ln_sigma_edges")):
            assert a == b, key
            continue
        # sums divided by exact integer counts: the bound of the sums carries over (the entropy terms are the same fp32 values
        # on both sides, so its sum is held to the fp64 bound too)
        for x, y in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
            assert (x is None and y is None) or abs(x - y) <= REL_SUM * abs(x), (key, x, y)
