"""Dispersive loss through the engine: train_microbatch with the term armed against the CPU oracle of the COMBINED
objective L_edm + lambda * L_disp(output of blocks.0), on the cases of test_engine_gpu.py::test_train_step_parity (same configs, batch
sizes, seeds, mask ratios; k = 0 in each).

The oracle side adds the term without touching oracle/: oracle.microdit_ref.dit_block is wrapped so that the undetached output of
blocks.0 is kept, and lambda * L_disp of it (fp64, autograd) is added before backward().  tau and lambda are fixed from the oracle alone,
before anything runs on the GPU: tau = the oracle's mean off-diagonal D, lambda = ||g_edm|| / ||g_disp|| over the parameters of blocks.0
(so the term changes their gradient by 100 % in rel-RMS; the precondition asserted is >= 50 %), and the term must leave the oracle's
gradients of blocks.1... untouched.  A test whose term is invisible shows nothing.

Two microbatches: scaling a microbatch by grad_scale = 0.5 scales dL/dF and W' by an exact power of two and every backward op is linear in
them, so in deterministic mode the accumulated gradient is 0.5 gA + 0.5 gB up to the fp32 additions into the accumulators: per element
2^-21 (|gA| + |gB|) / 2 plus 2^-21 of the tensor's RMS (a few addends per element, cancellation at the scale of the tensor)."""
import json

import pytest
import torch

from micro_diffusion_amd import disperse as dsp
from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the cases of tests/test_engine_gpu.py::test_train_step_parity
CASES = [("tiny_mask75", orc.tiny_config, 4, 11, 0.75, -0.6, 1.2, 77),
         ("tiny_mask0", orc.tiny_config, 2, 12, 0.0, -0.6, 1.2, 77),
         ("micro_mask50", orc.micro_config, 3, 13, 0.5, 0.0, 0.6, 20)]
IDS = [c[0] for c in CASES]


def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)))


def _disp_loss(z, tau):
    """L_disp of z [B, K] as a differentiable fp64 expression (pairwise differences)."""
    z = z.double()
    d = (z[:, None, :] - z[None, :, :]).pow(2).sum(-1) / z.shape[1]
    return torch.log(torch.exp(-d / tau).mean())


def _oracle(monkeypatch, cfg, sd, batch, rnd, epsn, mnoise, ratio, pm, ps):
    """-> (EDM loss, tau, lambda, combined gradients {name: fp32}, L_disp) from the CPU oracle alone, with the preconditions asserted."""
    kept = {}
    inner = orc.dit_block

    def wrapped(sd_, spec, *a, **kw):
        out = inner(sd_, spec, *a, **kw)
        if spec.prefix == "blocks.0":
            kept["z"] = out
        return out

    monkeypatch.setattr(orc, "dit_block", wrapped)
    osd = {k: v.clone().requires_grad_(k not in ("pos_embed", "mask_token")) for k, v in sd.items()}
    oloss = orc.latent_diffusion_forward(osd, cfg, batch, rnd, epsn, mnoise, ratio, pm, ps)
    monkeypatch.setattr(orc, "dit_block", inner)
    names = [k for k, v in osd.items() if v.requires_grad]
    z = kept["z"].flatten(1)                                       # [B, Tk * D], each sample flattened token-major as the engine stores it
    tau = float(dsp.reference(z, 1.0)[2])                          # the oracle's mean off-diagonal D
    assert tau > 0
    Ld = _disp_loss(z, tau)
    Lr, gr, _ = dsp.reference(z, tau)
    assert abs(float(Ld.detach()) - float(Lr)) <= 1e-12
    gz = torch.autograd.grad(Ld, kept["z"], retain_graph=True)[0].flatten(1)
    assert float((gz.double() - gr).abs().max()) <= 1e-6 * float(gr.abs().max()), "the differentiable form is the reference (fp32 graph)"
    g_edm = dict(zip(names, torch.autograd.grad(oloss, [osd[k] for k in names], retain_graph=True, allow_unused=True)))
    g_dsp = dict(zip(names, torch.autograd.grad(Ld, [osd[k] for k in names], allow_unused=True)))
    zero = lambda k: torch.zeros_like(osd[k])   # noqa: E731
    g_edm = {k: (zero(k) if g is None else g) for k, g in g_edm.items()}
    g_dsp = {k: (zero(k) if g is None else g.float()) for k, g in g_dsp.items()}
    b0 = [k for k in names if k.startswith("blocks.0.")]
    later = [k for k in names if k.startswith("blocks.") and not k.startswith("blocks.0.")]
    assert b0 and later
    n_edm = torch.sqrt(sum(g_edm[k].double().pow(2).sum() for k in b0))
    n_dsp = torch.sqrt(sum(g_dsp[k].double().pow(2).sum() for k in b0))
    assert float(n_dsp) > 0
    lam = float(n_edm / n_dsp)
    change = lam * float(n_dsp) / float(n_edm)
    assert change >= 0.5, "precondition: the term moves the gradient of blocks.0 by at least 50 % rel-RMS"
    assert all(not g_dsp[k].any() for k in later), "precondition: the term does not reach the blocks behind k"
    comb = {k: g_edm[k] + lam * g_dsp[k] for k in names}
    return float(oloss.detach()), tau, lam, comb, float(Ld.detach())


def _model(cfg, sd, ratio, pm, ps):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd)
    m = LatentDiffusion(d.to(DEV), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), p_mean=pm, p_std=ps, train_mask_ratio=ratio)
    m.train()
    return m


def _run(cfg, sd, gb, noise, ratio, pm, ps, disperse="absent", det=False, steps=((None, 1.0),)):
    """A fresh model, one train_microbatch per entry of `steps` ((batch, noise) or None for the default pair, grad_scale).
    disperse="absent": the attribute is not touched at all.  -> dict(model, loss, grads, gemm_log, disperse_log, accum)"""
    m = _model(cfg, sd, ratio, pm, ps)
    eng = m.dit.engine
    eng.deterministic = det
    eng.keep_last_tape = True
    if disperse != "absent":
        m.disperse = disperse
        m.disperse_accum = torch.zeros(2, device=DEV)
    eng.gemm_log, eng.disperse_log = [], []
    loss = None
    for which, gs in steps:
        b, n = (gb, noise) if which is None else which
        m._noise_fn = lambda _b, n=n: n
        loss = m.train_microbatch(b, grad_scale=gs, accum_weight=gs)
    torch.cuda.synchronize()
    return dict(model=m, loss=float(loss), grads={k: p.grad.detach().clone() for k, p in m.dit.named_parameters()},
                gemm_log=list(eng.gemm_log), disperse_log=list(eng.disperse_log), accum=getattr(m, "disperse_accum", None))


def _inputs(cfgf, B, seed, ratio, cap):
    cfg = cfgf()
    sd = orc.synth_state_dict(cfg, seed)
    batch, rnd, epsn, mnoise = orc.synth_batch(cfg, B, seed + 1, cap_len=cap)
    gb = {k: v.to(DEV) for k, v in batch.items()}
    noise = (rnd.to(DEV), epsn.to(DEV), mnoise.to(DEV) if ratio > 0 else None)
    return cfg, sd, batch, rnd, epsn, mnoise, gb, noise


@pytest.mark.parametrize("tag,cfgf,B,seed,ratio,pm,ps,cap", CASES, ids=IDS)
def test_armed_step_matches_the_oracle_of_the_combined_objective(hip, monkeypatch, tag, cfgf, B, seed, ratio, pm, ps, cap):
    cfg, sd, batch, rnd, epsn, mnoise, gb, noise = _inputs(cfgf, B, seed, ratio, cap)
    oloss, tau, lam, ograd, oLd = _oracle(monkeypatch, cfg, sd, batch, rnd, epsn, mnoise, ratio, pm, ps)
    dl = dsp.DisperseLoss(weight=lam, tau=tau, block=0)
    r = _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dl)
    grads = {k: g.cpu() for k, g in r["grads"].items()}
    per = {k: _rel_rms(grads[k], ograd[k]) for k in grads}
    gn_h = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    gn_o = float(torch.sqrt(sum((ograd[k].double() ** 2).sum() for k in grads)))
    cos = float(sum((grads[k].double() * ograd[k].double()).sum() for k in grads)) / (gn_h * gn_o)
    # the reported term against the definition evaluated on the engine's own Z
    eng = r["model"].dit.engine
    d = eng.last_tape.disperse
    Tk = eng.last_tape.Tk
    z = d.z.reshape(B, Tk * cfg.dim)
    assert (d.k, d.B, d.K) == (0, B, Tk * cfg.dim) and d.z.data_ptr() == (eng.last_tape.blocks[1].x.data_ptr() if len(eng.backbone) > 1
                                                                         else eng.last_tape.xlast.data_ptr()), "Z is the next block's saved input"
    Lz, _, mdz = dsp.reference(z, tau)
    res = r["model"]._disperse_result.cpu()
    rep = {"case": tag, "tau": tau, "lambda": lam, "loss_hip": r["loss"], "loss_oracle": oloss, "disperse_hip": float(res[0]),
           "disperse_on_engine_z": float(Lz), "disperse_oracle": oLd, "mean_dist_hip": float(res[1]), "mean_dist_on_engine_z": float(mdz),
           "gnorm_hip": gn_h, "gnorm_oracle": gn_o, "cosine": cos, "paths": r["disperse_log"],
           "worst": sorted(per.items(), key=lambda kv: -kv[1])[:8]}
    print(json.dumps(rep, indent=1))
    assert [p[:2] for p in r["disperse_log"]] == [("gram", "gemm" if B % 8 == 0 else "small"), ("apply", "gemm")], r["disperse_log"]
    assert abs(r["loss"] - oloss) <= 0.01 * abs(oloss), "`loss` stays the raw EDM loss"
    assert cos >= 0.99, cos
    assert abs(gn_h - gn_o) <= 0.03 * gn_o, (gn_h, gn_o)
    bad = {k: v for k, v in per.items() if v > 0.15}
    assert not bad, bad
    assert abs(float(res[0]) - float(Lz)) <= 1e-5 * abs(float(Lz)) + 1e-6, (float(res[0]), float(Lz))
    assert abs(float(res[1]) - float(mdz)) <= 1e-5 * abs(float(mdz)) + 1e-6, (float(res[1]), float(mdz))
    acc = r["accum"].cpu()
    assert abs(float(acc[0]) - float(Lz)) <= 1e-5 * abs(float(Lz)) + 1e-6 and abs(float(acc[1]) - float(mdz)) <= 1e-5 * abs(float(mdz)) + 1e-6


@pytest.mark.parametrize("tag,cfgf,B,seed,ratio,pm,ps,cap", CASES, ids=IDS)
def test_blocks_behind_k_keep_their_gradients_and_runs_repeat(hip, tag, cfgf, B, seed, ratio, pm, ps, cap):
    """Deterministic mode: the parameters of blocks.1... (and the final layer) have bit for bit the gradients of an unarmed run, the
    parameters in front of them do not, and two armed runs are bit-identical."""
    cfg, sd, _, _, _, _, gb, noise = _inputs(cfgf, B, seed, ratio, cap)
    dl = dsp.DisperseLoss(weight=0.5, tau=0.5, block=0)
    off = _run(cfg, sd, gb, noise, ratio, pm, ps, det=True)
    on = _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dl, det=True)
    on2 = _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dl, det=True)
    assert on["loss"] == off["loss"] == on2["loss"]
    behind = [k for k in off["grads"] if (k.startswith("blocks.") and not k.startswith("blocks.0.")) or k.startswith("final_layer.")]
    assert len(behind) > 10
    differ = [k for k in behind if not torch.equal(on["grads"][k], off["grads"][k])]
    assert not differ, differ[:4]
    moved = [k for k in off["grads"] if k.startswith("blocks.0.") and not torch.equal(on["grads"][k], off["grads"][k])]
    assert moved, "the armed run must change the gradients of block k"
    differ = [k for k in on["grads"] if not torch.equal(on["grads"][k], on2["grads"][k])]
    assert not differ, f"two armed deterministic runs differ in {differ[:4]}"
    assert all(bool(torch.isfinite(g).all()) for g in on["grads"].values())
    # the same without deterministic mode: equal up to the atomic-order noise of the default mode (the project's 1e-2 per-tensor bound)
    on_d = _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dl)
    off_d = _run(cfg, sd, gb, noise, ratio, pm, ps)
    worst = max(_rel_rms(on_d["grads"][k], off_d["grads"][k]) for k in behind)
    assert worst <= 1e-2, worst


def test_off_is_the_launch_sequence_of_today(hip):
    tag, cfgf, B, seed, ratio, pm, ps, cap = CASES[0]
    cfg, sd, _, _, _, _, gb, noise = _inputs(cfgf, B, seed, ratio, cap)
    base = _run(cfg, sd, gb, noise, ratio, pm, ps, det=True)
    for dl in (None, dsp.DisperseLoss(weight=0.0)):
        r = _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dl, det=True)
        assert r["gemm_log"] == base["gemm_log"] and r["disperse_log"] == [] and len(base["gemm_log"]) > 50
        assert r["loss"] == base["loss"] and all(torch.equal(r["grads"][k], base["grads"][k]) for k in base["grads"])
        assert not r["accum"].any() and r["model"].dit.engine.last_tape.disperse is None
    on = _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dsp.DisperseLoss(block=0), det=True)
    assert len(on["gemm_log"]) == len(base["gemm_log"]) + 1, "armed with B % 8 != 0: one more GEMM launch (the injection)"
    one = _run(cfg, sd, {k: v[:1] for k, v in gb.items()}, tuple(None if n is None else n[:1] for n in noise), ratio, pm, ps,
               disperse=dsp.DisperseLoss(block=0), det=True)
    assert one["disperse_log"] == [] and not one["accum"].any(), "B = 1 launches nothing"
    with pytest.raises(ValueError, match="outside"):
        _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dsp.DisperseLoss(block=len(base["model"].dit.engine.backbone)))


def test_two_half_weight_microbatches_accumulate_to_the_mean(hip):
    tag, cfgf, B, seed, ratio, pm, ps, cap = CASES[0]
    cfg, sd, _, _, _, _, gb, noise = _inputs(cfgf, B, seed, ratio, cap)
    _, _, _, _, _, _, gb2, noise2 = _inputs(cfgf, B, seed + 50, ratio, cap)
    dl = dsp.DisperseLoss(weight=0.5, tau=0.5, block=0)
    a = _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dl, det=True)
    b = _run(cfg, sd, gb2, noise2, ratio, pm, ps, disperse=dl, det=True)
    both = _run(cfg, sd, gb, noise, ratio, pm, ps, disperse=dl, det=True, steps=(((gb, noise), 0.5), ((gb2, noise2), 0.5)))
    worst = 0.0
    for k, g in both["grads"].items():
        ga, gb_ = a["grads"][k].double(), b["grads"][k].double()
        err = (g.double() - 0.5 * (ga + gb_)).abs()
        bound = 2.0 ** -21 * 0.5 * (ga.abs() + gb_.abs()) + 2.0 ** -21 * g.double().pow(2).mean().sqrt()
        worst = max(worst, float((err / (bound + 1e-300)).max()))
        assert bool((err <= bound).all()), f"{k}: {float(err.max())} against a bound of {float(bound.max())}"
    print(json.dumps({"worst_error_over_bound": worst}))
    acc = both["accum"].cpu()
    want = 0.5 * (a["accum"].cpu() + b["accum"].cpu())
    assert float((acc - want).abs().max()) <= 1e-6, "disperse_accum holds the weighted mean of the two microbatches"


def test_trainer_reports_the_term(hip):
    """Trainer(disperse=...): `loss` stays the raw EDM loss, disperse_stats() is the mean over the step's microbatches, diagnostics()
    carries the last microbatch's result block; weight 0 disarms; a block outside the backbone is refused at construction."""
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    tag, cfgf, B, seed, ratio, pm, ps, cap = CASES[0]
    cfg, sd, batch, rnd, epsn, mnoise, gb, _ = _inputs(cfgf, B, seed, ratio, cap)
    losses = {}
    for name, dl in (("off", None), ("on", dsp.DisperseLoss(weight=0.5, tau=0.5, block=0))):
        model = _model(cfg, sd, ratio, pm, ps)
        model.dit.engine.deterministic = True
        tr = Trainer(model, FusedAdamW(model.dit, lr=1e-4), None, microbatch_size=2, **({} if dl is None else {"disperse": dl}))
        assert (model.disperse is dl) and tr.disperse_stats() is None and "disperse" not in tr.diagnostics()
        chunks = [(rnd[i:i + 2].to(DEV), epsn[i:i + 2].to(DEV), mnoise[i:i + 2].to(DEV)) for i in range(0, 4, 2)]
        model._noise_fn = lambda b, c=chunks: c.pop(0)
        model.dit.engine.disperse_log = log = []
        losses[name] = float(tr.train_step(gb))
        st = tr.disperse_stats()
        if dl is None:
            assert st is None and log == []
            continue
        assert [p[:3] for p in log] == [("gram", "small", 2), ("apply", "gemm", 2)] * 2, log
        assert set(st) == {"disperse_loss", "disperse_mean_dist"} and -0.6932 <= st["disperse_loss"] < 0 and st["disperse_mean_dist"] > 0
        d = tr.diagnostics()["disperse"]
        assert set(d) == {"loss", "mean_dist", "mean_offdiag_p_b2"} and d["loss"] < 0 and 0 < d["mean_offdiag_p_b2"] <= 1.0 + 1e-12
        assert model.dit.engine.disperse is None, "the engine is disarmed between microbatches"
    assert losses["on"] == losses["off"], "train_step returns the raw EDM loss with the term on"
    model = _model(cfg, sd, ratio, pm, ps)
    tr = Trainer(model, FusedAdamW(model.dit, lr=1e-4), None, microbatch_size=2, disperse=dsp.DisperseLoss(weight=0.0))
    assert tr.disperse is None and model.disperse is None, "weight 0 is off"
    with pytest.raises(ValueError, match="outside"):
        Trainer(model, FusedAdamW(model.dit, lr=1e-4), None, microbatch_size=2, disperse=dsp.DisperseLoss(block=99))
