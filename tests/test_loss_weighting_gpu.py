"""Learned per-noise-level loss weighting on the GPU: md_logvar_fwd, md_edm_loss_train_weighted and md_logvar_bwd against the fp64
restatement in micro_diffusion_amd/loss_weighting.py, a fit that runs only these kernels plus md_adamw_step, then the feature under the
Trainer: first step, off state, skipped step, two ranks, save / resume, weights-only load.

Bounds (U = 2^-24, the fp32 unit roundoff; every reference value is fp64 on the fp32 inputs).
  feature   a = c * freq + phase is formed in fp32 and cosf is evaluated on the rounded a, then one product with sqrt(2):
            dfeat = sqrt(2) * (2^-22 * (|c * freq| + |phase|) + K * U).  K is cosf's ulp bound; the HIP math documentation is not part of
            the ROCm install this was written against, so K = 4 is taken.
  u         du_ = sum_c |w[c]| * dfeat[b, c] + C * U * sum_c |w[c] * feat[b, c]|       (C products added in some fixed order)
  inv       du_ * inv + 2 ulp of expf, 2 * 2^-23 * inv
  dw        the sum: B * U * sum_b |du_b * feat[b, c]| -- the kernel adds the samples in one fma chain per channel that starts from the
            value already in dw, B roundings of at most U / 2 * (|dw before| + sum_b |du_b * feat|); the kernel test prefills dw with
            +-0.5 * sum_b |du_b * feat| (fp64, from the reference), so that chain is inside B * U * sum_b |du_b * feat|, and the trainer
            tests, where dw holds what the earlier microbatches left, use the chain form itself;
            plus the feature bound carried through: sum_b |du_b| * dfeat[b, c].  These two terms are the whole bound of the kernel
            test (u is an input there).  In the trainer tests the u a backward starts from carries an error du_ of its own (the
            forward's, and that of the w it was formed from), so there the per-sample factor adds sum_b ddu_b * |feat[b, c]| with
            ddu_b = gscale / B * (L_b * inv_b * (2^-22 + du_) + 2 * U * (1 + L_b * inv_b)): expf's 2 ulp as in the bound on inv, the
            error du_, and the two roundings of 1 - inv * L (one fma) and of the product with gscale / B.
  objective (1 / B) sum_b (L_b * inv_b * 2^-22 + U * (L_b * inv_b + |u_b|)) + (B + 2) * U * (1 / B) sum_b |L_b * inv_b + u_b|
  w         one AdamW step is elementwise in the gradient: the bound on dw is carried to w through the derivative of the fp64 update
            (autograd on loss_weighting.ref_adamw with the kernel's fp32 constants) plus 16 * U * lr per step for the update's own fp32
            arithmetic (about ten roundings on a step of size <= lr).
Everything else is compared bit for bit."""
import math
import os
import socket
import tempfile
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from micro_diffusion_amd import loss_weighting as lwm

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
K_COS = 4
PAD = 64
LR = 2.4e-4


# ---------------------------------------------------------------------------------------------------- bounds (fp64, on the CPU)
def feat_bound(c, freq, phase):
    c, freq, phase = c.double().cpu(), freq.double().cpu(), phase.double().cpu()
    return math.sqrt(2.0) * (2.0 ** -22 * ((c[:, None] * freq[None]).abs() + phase[None].abs()) + K_COS * U)


def u_bound(c, freq, phase, w):
    feat = lwm.ref_features(c.cpu(), freq.cpu(), phase.cpu())
    w = w.double().cpu()
    return feat_bound(c, freq, phase) @ w.abs() + w.numel() * U * (feat.abs() @ w.abs())


def dw_terms(c, freq, phase, u, loss, gscale, u_err=None):
    """(dw, sum_b |du_b feat|, feature bound carried through, objective, objective bound) of one md_logvar_bwd call, fp64 on the CPU.
    With u_err (the error of the u the call starts from: the trainer tests) the carried bound also holds the per-sample factor's."""
    c, freq, phase, u, loss = (t.detach().cpu() for t in (c, freq, phase, u, loss))
    B = c.numel()
    feat = lwm.ref_features(c, freq, phase)
    du, dw, obj = lwm.ref_backward(c, freq, phase, u, loss, gscale)
    inv, L = torch.exp(-u.double()), loss.double()
    sum_abs = du.abs() @ feat.abs()
    carried = du.abs() @ feat_bound(c, freq, phase)
    if u_err is not None:
        ddu = gscale / B * (L.abs() * inv * (2.0 ** -22 + u_err) + 2 * U * (1 + L.abs() * inv))
        carried = carried + ddu @ feat.abs()
    t = L * inv + u.double()
    obj_bound = float((L.abs() * inv * 2.0 ** -22 + U * (L.abs() * inv + u.double().abs())).mean() + (B + 2) * U * t.abs().mean())
    return dw, sum_abs, carried, float(obj), obj_bound


def _framed(n, fill=None):
    buf = torch.full((n + 2 * PAD,), 12345.0, device=DEV)
    buf[-PAD:] = -54321.0
    if fill is not None:
        buf[PAD:PAD + n] = fill
    return buf


def _frame_ok(buf):
    return bool((buf[:PAD] == 12345.0).all()) and bool((buf[-PAD:] == -54321.0).all())


# ---------------------------------------------------------------------------------------------------- md_logvar_fwd
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("B", [1, 3, 65, 257])
def test_logvar_fwd_against_fp64(hip, B, C):
    lw = lwm.LossWeighting(channels=C, seed=11, device=DEV)
    g = torch.Generator().manual_seed(100 * B + C)
    w = (0.1 * torch.randn(C, generator=g)).to(DEV)
    c = (0.6 * torch.randn(B, generator=g) / 4).to(DEV)
    u, inv = _framed(B), _framed(B)
    hip.check(hip.lib().md_logvar_fwd(c.data_ptr(), lw.freq.data_ptr(), lw.phase.data_ptr(), w.data_ptr(), u[PAD:].data_ptr(),
                                      inv[PAD:].data_ptr(), B, C, hip.stream_ptr()), "md_logvar_fwd")
    torch.cuda.synchronize()
    ur, ir = lwm.ref_forward(c.cpu(), lw.freq.cpu(), lw.phase.cpu(), w.cpu())
    ub = u_bound(c, lw.freq, lw.phase, w)
    ib = ub * ir + 2 * 2.0 ** -23 * ir
    wu = float(((u[PAD:PAD + B].double().cpu() - ur).abs() / ub).max())
    wi = float(((inv[PAD:PAD + B].double().cpu() - ir).abs() / ib).max())
    print(f"B {B} C {C}: worst |u - ref| / bound = {wu:.3f}, worst |inv - ref| / bound = {wi:.3f}")
    assert wu <= 1.0 and wi <= 1.0
    assert _frame_ok(u) and _frame_ok(inv)
    # the class wrapper launches the same kernel; w = 0 gives u = 0 and inv = 1 exactly
    lw.w.copy_(w)
    assert torch.equal(lw.forward(c), inv[PAD:PAD + B]) and torch.equal(lw._u, u[PAD:PAD + B])
    lw.w.zero_()
    assert bool((lw.forward(c) == 1.0).all()) and not lw._u.any()


def test_logvar_bad_arguments_launch_nothing(hip):
    L, st = hip.lib(), hip.stream_ptr()
    lw = lwm.LossWeighting(channels=128, seed=1, device=DEV)
    c, u, inv, loss = (torch.ones(4, device=DEV) for _ in range(4))
    dw, obj = torch.full((128,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    f, p, w = lw.freq.data_ptr(), lw.phase.data_ptr(), lw.w.data_ptr()
    assert L.md_logvar_fwd(c.data_ptr(), f, p, w, u.data_ptr(), inv.data_ptr(), 0, 128, st) == -1
    assert L.md_logvar_fwd(c.data_ptr(), f, p, w, u.data_ptr(), inv.data_ptr(), 4, 96, st) == -1
    assert L.md_logvar_fwd(c.data_ptr(), f, p, w, u.data_ptr(), inv.data_ptr(), 4, 320, st) == -1
    assert L.md_logvar_fwd(c.data_ptr(), f, p, None, u.data_ptr(), inv.data_ptr(), 4, 128, st) == -1
    assert L.md_logvar_fwd(c.data_ptr(), f, p, w, None, inv.data_ptr(), 4, 128, st) == -1
    assert L.md_logvar_bwd(c.data_ptr(), f, p, u.data_ptr(), loss.data_ptr(), 1.0, dw.data_ptr(), obj.data_ptr(), None, 0.0, 0, 128, st) == -1
    assert L.md_logvar_bwd(c.data_ptr(), f, p, u.data_ptr(), loss.data_ptr(), 1.0, dw.data_ptr(), obj.data_ptr(), None, 0.0, 4, 32, st) == -1
    assert L.md_logvar_bwd(c.data_ptr(), f, p, u.data_ptr(), loss.data_ptr(), 1.0, None, obj.data_ptr(), None, 0.0, 4, 128, st) == -1
    assert L.md_logvar_bwd(c.data_ptr(), f, p, u.data_ptr(), None, 1.0, dw.data_ptr(), obj.data_ptr(), None, 0.0, 4, 128, st) == -1
    assert L.md_logvar_bwd(c.data_ptr(), f, p, u.data_ptr(), loss.data_ptr(), 1.0, dw.data_ptr(), None, None, 0.0, 4, 128, st) == -1
    torch.cuda.synchronize()
    assert bool((u == 1).all()) and bool((inv == 1).all()) and bool((dw == 7).all()) and bool((obj == 7).all())


# ---------------------------------------------------------------------------------------------------- md_edm_loss_train_weighted
B_L, C_L, H_L, P_L, T_L, PV_L = 3, 4, 8, 2, 16, 16


def _loss_case(masked):
    g = torch.Generator().manual_seed(77)
    Tk = 4 if masked else T_L
    tok = torch.randn(B_L * Tk, PV_L, generator=g).to(torch.bfloat16).to(DEV)
    x0 = (0.8 * torch.randn(B_L, C_L, H_L, H_L, generator=g)).to(DEV)
    sigma = torch.exp(1.2 * torch.randn(B_L, generator=g) - 0.6).to(DEV)
    xn = x0 + sigma.view(-1, 1, 1, 1) * torch.randn(B_L, C_L, H_L, H_L, generator=g).to(DEV)
    keep = None
    if masked:                 # Tk distinct grid positions per sample, unsorted, as absolute rows b * T + t
        keep = torch.stack([torch.randperm(T_L, generator=g)[:Tk] + b * T_L for b in range(B_L)]).to(torch.int32).reshape(-1).to(DEV)
    return tok, keep, xn, x0, sigma, Tk


def _run_loss(hip, case, scale):
    """md_edm_loss_train (scale None) or its weighted form: (dtok frame, loss_per_sample, loss_mean, loss_accum)."""
    tok, keep, xn, x0, sigma, Tk = case
    n = B_L * Tk * PV_L
    dtok = torch.full((n + 2 * PAD,), 3.0, device=DEV, dtype=torch.bfloat16)
    lps, mean, accum = torch.zeros(B_L, device=DEV), torch.zeros(1, device=DEV), torch.full((1,), 1.5, device=DEV)
    args = [tok.data_ptr(), None if keep is None else keep.data_ptr(), xn.data_ptr(), x0.data_ptr(), sigma.data_ptr(), lps.data_ptr(),
            mean.data_ptr(), dtok[PAD:].data_ptr(), 0.5, accum.data_ptr(), 0.25, B_L, Tk, C_L, H_L, H_L, P_L, 0.9]
    if scale is None:
        hip.check(hip.lib().md_edm_loss_train(*args, hip.stream_ptr()), "md_edm_loss_train")
    else:
        hip.check(hip.lib().md_edm_loss_train_weighted(*args, scale.data_ptr(), hip.stream_ptr()), "md_edm_loss_train_weighted")
    torch.cuda.synchronize()
    assert bool((dtok[:PAD] == 3.0).all()) and bool((dtok[-PAD:] == 3.0).all())
    return dtok[PAD:PAD + n].clone(), lps, mean, accum


@pytest.mark.parametrize("masked", [True, False])
def test_weighted_loss_scales_only_the_gradient(hip, masked):
    case = _loss_case(masked)
    Tk = case[5]
    d0, l0, m0, a0 = _run_loss(hip, case, None)
    assert bool(torch.isfinite(l0).all()) and float(a0) != 1.5 and d0.float().abs().max() > 0
    d1, l1, m1, a1 = _run_loss(hip, case, torch.ones(B_L, device=DEV))
    assert torch.equal(d1, d0) and torch.equal(l1, l0) and torch.equal(m1, m0) and torch.equal(a1, a0), "sample_scale = 1 must give md_edm_loss_train's bits"
    for scales in ([0.25, 0.5, 2.0], [4.0, 0.25, 0.5], [2.0, 4.0, 0.25]):
        sc = torch.tensor(scales, device=DEV)
        d2, l2, m2, a2 = _run_loss(hip, case, sc)
        want = (d0.view(B_L, Tk * PV_L).float() * sc.view(-1, 1)).to(torch.bfloat16).view(-1)       # exact: powers of two
        assert torch.equal(d2, want), scales
        assert torch.equal(l2, l0) and torch.equal(m2, m0) and torch.equal(a2, a0), "the loss outputs stay the raw loss"


def test_weighted_loss_bad_arguments(hip):
    tok, keep, xn, x0, sigma, Tk = _loss_case(True)
    sc = torch.ones(B_L, device=DEV)
    dtok = torch.full((B_L * Tk * PV_L,), 3.0, device=DEV, dtype=torch.bfloat16)
    lps, mean = torch.full((B_L,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    ok = [tok.data_ptr(), keep.data_ptr(), xn.data_ptr(), x0.data_ptr(), sigma.data_ptr(), lps.data_ptr(), mean.data_ptr(), dtok.data_ptr(),
          0.5, None, 0.0, B_L, Tk, C_L, H_L, H_L, P_L, 0.9, sc.data_ptr(), hip.stream_ptr()]
    for k, v in ((0, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None), (18, None), (11, 0), (12, 0), (14, 7), (15, 7)):
        a = list(ok)
        a[k] = v
        assert hip.lib().md_edm_loss_train_weighted(*a) == -1, k
    torch.cuda.synchronize()
    assert bool((dtok == 3.0).all()) and bool((lps == 7.0).all()) and bool((mean == 7.0).all())


# ---------------------------------------------------------------------------------------------------- md_logvar_bwd
@pytest.mark.parametrize("B", [1, 65, 257])
def test_logvar_bwd_against_fp64(hip, B):
    C, gscale = 128, 0.5
    lw = lwm.LossWeighting(channels=C, seed=12, device=DEV)
    g = torch.Generator().manual_seed(300 + B)
    w = 0.1 * torch.randn(C, generator=g)
    c = 0.6 * torch.randn(B, generator=g) / 4
    loss = (torch.exp(-2 * c + 0.5) * (0.5 + torch.rand(B, generator=g))).float()
    u = lwm.ref_forward(c, lw.freq.cpu(), lw.phase.cpu(), w)[0].float()               # an input of the kernel: exact by definition
    dw_ref, sum_abs, carried, obj_ref, obj_bound = dw_terms(c, lw.freq, lw.phase, u, loss, gscale)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
    pre = (0.5 * sign * sum_abs).float()                                              # see the module docstring
    acc_pre = 0.75
    c_d, u_d, loss_d = c.to(DEV), u.to(DEV), loss.to(DEV)         # named: a temporary's memory is reused by the next one

    def run():
        dw, obj, acc = _framed(C, pre.to(DEV)), _framed(1, 0.0), _framed(1, acc_pre)
        hip.check(hip.lib().md_logvar_bwd(c_d.data_ptr(), lw.freq.data_ptr(), lw.phase.data_ptr(), u_d.data_ptr(),
                                          loss_d.data_ptr(), gscale, dw[PAD:].data_ptr(), obj[PAD:].data_ptr(), acc[PAD:].data_ptr(),
                                          0.25, B, C, hip.stream_ptr()), "md_logvar_bwd")
        torch.cuda.synchronize()
        assert _frame_ok(dw) and _frame_ok(obj) and _frame_ok(acc)
        return dw[PAD:PAD + C].clone(), obj[PAD:PAD + 1].clone(), acc[PAD:PAD + 1].clone()
    dw, obj, acc = run()
    bound = B * U * sum_abs + carried
    worst = float(((dw.double().cpu() - (pre.double() + dw_ref)).abs() / bound).max())
    wo = abs(float(obj) - obj_ref) / obj_bound
    acc_bound = 0.25 * obj_bound + 2 * U * (acc_pre + 0.25 * abs(obj_ref))
    wa = abs(float(acc) - (acc_pre + 0.25 * obj_ref)) / acc_bound
    print(f"B {B}: worst |dw - ref| / bound = {worst:.3f}, |objective - ref| / bound = {wo:.3f}, |obj_accum - ref| / bound = {wa:.3f}")
    assert worst <= 1.0 and wo <= 1.0 and wa <= 1.0
    assert not torch.equal(dw.cpu(), pre), "dw must have been added to"
    dw2, obj2, acc2 = run()
    assert torch.equal(dw, dw2) and torch.equal(obj, obj2) and torch.equal(acc, acc2), "two calls from identical buffers must agree bit for bit"
    # obj_accum is optional; a non-finite loss reaches dw (the step guard's business, not this kernel's)
    bad = loss.clone()
    bad[B // 2] = float("nan")
    bad_d, dw3, obj3 = bad.to(DEV), torch.zeros(C, device=DEV), torch.zeros(1, device=DEV)
    hip.check(hip.lib().md_logvar_bwd(c_d.data_ptr(), lw.freq.data_ptr(), lw.phase.data_ptr(), u_d.data_ptr(),
                                      bad_d.data_ptr(), gscale, dw3.data_ptr(), obj3.data_ptr(), None, 0.0, B, C, hip.stream_ptr()),
              "md_logvar_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw3).all()) and bool(torch.isnan(obj3).all())


# ---------------------------------------------------------------------------------------------------- fit
def test_fit_closes_the_gap(hip):
    """Only md_logvar_fwd, md_logvar_bwd and md_adamw_step run: 100 steps, B = 64, C = 128, lr 1e-2 on L = exp(-2c + 0.5); on 4096
    held-out levels the objective must close >= 0.9 of the gap between mean L (w = 0) and mean(1 + ln L) (its floor).  The fp64
    reference with torch.optim.AdamW closes 0.999 of it (tests/test_loss_weighting_cpu.py, the same data)."""
    from tests.test_loss_weighting_cpu import fit_problem, gap_closed
    lw = lwm.LossWeighting(channels=128, seed=0, device=DEV)
    train_c, held_c = fit_problem()
    for i in range(100):
        c = train_c[i].to(DEV)
        L = torch.exp(-2 * train_c[i].double() + 0.5).float().to(DEV)
        lw.forward(c)
        lw.backward(c, L, 1.0)
        lw.step(1e-2)
    torch.cuda.synchronize()
    assert lw.step_count == 100 and not lw.g.any(), "the AdamW launch zeroes the accumulator"
    closed = gap_closed(lw, held_c, lw.w)
    print(f"100 steps of the kernels: closes {closed:.4f} of the gap (bound 0.9)")
    assert closed >= 0.9


# ---------------------------------------------------------------------------------------------------- under the Trainer
def _product(cfg, sd, ratio=0.75):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), train_mask_ratio=ratio)
    m.train()
    return m


def _record(lw, log):
    """Keep (cnoise, loss_per_sample, gscale) of every md_logvar_bwd the Trainer issues, per step."""
    inner = lw.backward

    def backward(cnoise, lps, gscale, obj_accum=None, accum_weight=0.0):
        log[-1].append((cnoise.detach().clone(), lps.detach().clone(), float(gscale)))
        return inner(cnoise, lps, gscale, obj_accum, accum_weight)
    lw.backward = backward


def _step(model, tr, cfg, B, seed, log=None, poison=False):
    from oracle import microdit_ref as orc
    batch, rnd, epsn, mnoise = orc.synth_batch(cfg, B, seed)
    if poison:
        batch["image_latents"][1, 0, 0, 0] = float("nan")
    mb = tr.microbatch_size
    chunks = [(rnd[i:i + mb].cuda(), epsn[i:i + mb].cuda(), mnoise[i:i + mb].cuda()) for i in range(0, B, mb)]
    model._noise_fn = lambda b, c=chunks: c.pop(0)
    if log is not None:
        log.append([])
    loss = tr.train_step({k: t.cuda() for k, t in batch.items()})
    torch.cuda.synchronize()
    return loss


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_cpu(v) for v in x)
    return x


def _train(cfg, sd, steps, on, first_seed=700, resume=None, weights_only=False, **opt_kw):
    """`steps` deterministic Tiny steps (rank batch 4, microbatches of 2).  resume = a checkpoint as train.py writes it."""
    import train
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    model = _product(cfg, sd)
    opt = FusedAdamW(model.dit, lr=LR, **opt_kw)
    lw = lwm.LossWeighting(channels=128, seed=3, device=DEV) if on else None
    if resume is not None:
        model.dit.load_state_dict({k[len("dit."):]: v for k, v in resume["state"]["model"].items()})
        if not weights_only:
            opt.load_state_dict(resume["optimizer"])
        lwm.restore(lw, resume["state"], weights_only=weights_only)
    kw = dict(loss_weighting=lw) if on else {}
    tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2, **kw)
    assert model.dit.engine.deterministic is True
    log, after = [], []
    if on:
        _record(lw, log)
    f = model.dit.flat_buffers()
    for i in range(steps):
        _step(model, tr, cfg, 4, first_seed + opt.step_count, log if on else None)
        after.append({"p": f["p"].clone(), "m": opt.m.clone(), "v": opt.v.clone(),
                      "lw": None if lw is None else (lw.w.clone(), lw.m.clone(), lw.v.clone())})
    ckpt = {"state": train.checkpoint_state(model, opt), "optimizer": opt.state_dict()}
    return {"model": model, "opt": opt, "tr": tr, "lw": lw, "log": log, "after": after, "ckpt": _to_cpu(ckpt)}


@pytest.fixture(scope="module")
def runs(hip):
    """Computed once, in the engine's deterministic mode: four steps with the feature on, one with it off, and two + two steps through a
    checkpoint written the way train.py writes it."""
    from oracle import microdit_ref as orc
    old = os.environ.get("MD_DETERMINISTIC")
    os.environ["MD_DETERMINISTIC"] = "1"
    try:
        cfg = orc.tiny_config()
        sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, 71))
        on = _train(cfg, sd, 4, True)
        off = _train(cfg, sd, 1, False)
        half = _train(cfg, sd, 2, True)
        resumed = _train(cfg, sd, 2, True, resume=half["ckpt"])
        yield {"cfg": cfg, "sd": sd, "on": on, "off": off, "half": half, "resumed": resumed}
    finally:
        if old is None:
            os.environ.pop("MD_DETERMINISTIC", None)
        else:
            os.environ["MD_DETERMINISTIC"] = old


def w_reference(freq, phase, steps, lr, grad_scale=1.0):
    """fp64 trajectory of w over `steps` = [[(cnoise, loss_per_sample, gscale), ...] per optimiser step] (the md_logvar_bwd calls of a
    step accumulate into one gradient; grad_scale is the AdamW launch's), with the bound on w of the module docstring carried along.
    Returns [(w, bound)] after every step."""
    freq, phase = freq.detach().cpu(), phase.detach().cpu()
    C = freq.numel()
    w, m, v = (torch.zeros(C, dtype=torch.float64) for _ in range(3))
    werr = torch.zeros(C, dtype=torch.float64)
    leaves, gerrs, out = [], [], []
    for t, calls in enumerate(steps, 1):
        gsum, gerr = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        for c, loss, gscale in calls:
            c, loss = c.detach().cpu(), loss.detach().cpu()
            B = c.numel()
            feat = lwm.ref_features(c, freq, phase)
            u = feat @ w
            uerr = u_bound(c, freq, phase, w) + feat.abs() @ werr + U * u.abs()      # the kernel's u: its own error, w's, one fp32 store
            dw, sum_abs, carried, _, _ = dw_terms(c, freq, phase, u, loss, gscale, u_err=uerr)
            gerr = gerr + B * (U / 2) * (gsum.abs() + gerr + sum_abs) * (1 + B * U) + carried
            gsum = gsum + dw
        leaves.append(gsum.clone().requires_grad_(True))
        gerrs.append(gerr)
        wt, mt, vt = (torch.zeros(C, dtype=torch.float64) for _ in range(3))
        for s, gl in enumerate(leaves, 1):                        # AdamW is elementwise in every step's gradient
            wt, mt, vt = lwm.ref_adamw(wt, gl * grad_scale, mt, vt, s, lr, as_kernel=True)
        jac = torch.autograd.grad(wt.sum(), leaves)
        werr = sum(j.abs() * e for j, e in zip(jac, gerrs)) + t * 16 * U * lr
        w, m, v = lwm.ref_adamw(w, gsum * grad_scale, m, v, t, lr, as_kernel=True)
        out.append((w.clone(), werr.clone()))
    return out


def test_first_step_equals_the_unweighted_run(runs):
    on, off = runs["on"], runs["off"]
    for k in ("p", "m", "v"):
        assert torch.equal(on["after"][0][k], off["after"][0][k]), f"{k} after step 1 differs: w = 0 must make every scale exactly 1"
    w1 = on["after"][0]["lw"][0]
    assert bool(w1.any()) and len(on["log"][0]) == 2, "two microbatches, a non-zero update of w"
    lw = on["lw"]
    # From zero moments the first update is -lr * g / (|g| + eps) with eps = 1e-8 far below |g|: about -lr * sign(g).  This comparison
    # therefore pins the sign of dw and the update's own arithmetic (its bound is nearly all the 16 * U * lr term); the loop over all
    # four steps below is the one that is sensitive to the size of dw, through the moments.
    (wr, bound), = w_reference(lw.freq, lw.phase, on["log"][:1], LR)
    worst = float(((w1.double().cpu() - wr).abs() / bound).max())
    print(f"w after step 1 against one AdamW step on the reference dw: worst |w - ref| / bound = {worst:.3f} "
          f"(bound {float(bound.max()):.3g}, |w| up to {float(w1.abs().max()):.3g})")
    assert worst <= 1.0
    # all four steps, the same bound carried along
    for t, (wr, bound) in enumerate(w_reference(lw.freq, lw.phase, on["log"], LR)):
        worst = float(((on["after"][t]["lw"][0].double().cpu() - wr).abs() / bound).max())
        print(f"w after step {t + 1}: worst |w - ref| / bound = {worst:.3f}")
        assert worst <= 1.0
    assert not torch.equal(on["after"][3]["p"], on["after"][0]["p"])


def test_off_state_adds_nothing(runs):
    import train
    off, on = runs["off"], runs["on"]
    assert off["model"].loss_weighting is None and off["tr"].loss_weighting is None
    assert "loss_weighting" not in off["ckpt"]["state"] and set(off["ckpt"]["state"]) == {"model"}
    assert len(off["model"].dit.state_dict()) == len(on["model"].dit.state_dict()) == len(off["ckpt"]["state"]["model"])
    loss = torch.tensor(0.5, device=DEV)
    assert "weighted_loss" not in train.log_line(1, loss, LR, 1.0, None, off["tr"])
    assert "loss_weighting" not in off["tr"].diagnostics() and off["tr"].weighted_objective() is None
    # ... and the on state adds exactly these
    assert set(on["ckpt"]["state"]) == {"model", "loss_weighting"}
    line = train.log_line(4, loss, LR, 1.0, None, on["tr"])
    assert math.isfinite(line["weighted_loss"]) and line["loss"] == 0.5
    d = on["tr"].diagnostics()["loss_weighting"]
    ec = on["model"].edm_config
    assert len(d["ln_sigma"]) == len(d["u"]) == 16 and math.isfinite(d["objective"])
    assert abs(d["ln_sigma"][0] - (ec.P_mean - 3 * ec.P_std)) < 1e-12 and abs(d["ln_sigma"][-1] - (ec.P_mean + 3 * ec.P_std)) < 1e-12
    assert d["u"] == on["lw"].u_at(d["ln_sigma"]) and any(x != 0 for x in d["u"])


def test_diagnostics_follow_the_loss_by_sigma_bins(runs, monkeypatch):
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    model = _product(runs["cfg"], runs["sd"])
    lw = lwm.LossWeighting(device=DEV)
    tr = Trainer(model, FusedAdamW(model.dit, lr=LR), None, microbatch_size=2, loss_by_sigma_bins=6, loss_weighting=lw)
    d = tr.diagnostics()["loss_weighting"]
    e = model.loss_by_sigma.edges
    assert d["ln_sigma"] == [0.5 * (a + b) for a, b in zip(e[:-1], e[1:])] and d["u"] == [0.0] * 6 and d["objective"] is None


def test_autograd_surface_refuses_while_armed(runs):
    from oracle import microdit_ref as orc
    model = runs["on"]["model"]
    model._noise_fn = None                                        # the recorded draws of the fixture's steps are used up
    batch, _, _, _ = orc.synth_batch(runs["cfg"], 2, 5)
    x, y = batch["image_latents"].cuda(), batch["caption_latents"].cuda()
    with pytest.raises(RuntimeError, match="loss weighting"):
        model.edm_loss(x, y, mask_ratio=0.75)
    with torch.no_grad():                                         # evaluation ignores the weighting
        w = runs["on"]["lw"].w.clone()
        assert bool(torch.isfinite(model.edm_loss(x, y, mask_ratio=0.75)))
        assert torch.equal(runs["on"]["lw"].w, w) and not runs["on"]["lw"].g.any()


def test_skipped_step_leaves_w_alone(hip, monkeypatch):
    from oracle import microdit_ref as orc
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    cfg = orc.tiny_config()
    model = _product(cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 72)))
    opt = FusedAdamW(model.dit, lr=LR, skip_nonfinite=True)
    lw = lwm.LossWeighting(device=DEV)
    tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2, loss_weighting=lw)
    f = model.dit.flat_buffers()
    _step(model, tr, cfg, 4, 800)
    _step(model, tr, cfg, 4, 801)
    assert opt.skipped_steps() == 0 and bool(lw.w.any())
    before, p = (lw.w.clone(), lw.m.clone(), lw.v.clone()), f["p"].clone()
    _step(model, tr, cfg, 4, 802, poison=True)                    # one NaN latent
    assert opt.skipped_steps() == 1 and torch.equal(f["p"], p)
    for name, a, b in zip("wmv", (lw.w, lw.m, lw.v), before):
        assert torch.equal(a, b), f"{name} moved on a skipped step"
    assert not lw.g.any(), "the accumulator is zeroed on a skipped step too"
    _step(model, tr, cfg, 4, 803)
    assert opt.skipped_steps() == 1 and not torch.equal(lw.w, before[0]) and bool(torch.isfinite(lw.w).all())


def test_save_and_resume(runs):
    on, re_ = runs["on"], runs["resumed"]
    assert "loss_weighting" in runs["half"]["ckpt"]["state"] and re_["opt"].step_count == 4 and re_["lw"].step_count == 4
    for name, a, b in zip(("w", "m", "v"), re_["after"][-1]["lw"], on["after"][-1]["lw"]):
        assert torch.equal(a, b), f"loss weighting {name} differs after save at step 2 + resume"
    for k in ("p", "m", "v"):
        assert torch.equal(re_["after"][-1][k], on["after"][-1][k]), k
    assert not torch.equal(on["after"][-1]["lw"][0], on["after"][1]["lw"][0])


def test_weights_only_load_and_missing_key(runs, monkeypatch):
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    ck = runs["half"]["ckpt"]
    r = _train(runs["cfg"], runs["sd"], 0, True, resume=ck, weights_only=True)
    saved = ck["state"]["loss_weighting"]
    lw = r["lw"]
    assert torch.equal(lw.w.cpu(), saved["w"]) and torch.equal(lw.freq.cpu(), saved["freq"]) and torch.equal(lw.phase.cpu(), saved["phase"])
    assert bool(saved["m"].any()) and not lw.m.any() and not lw.v.any() and lw.step_count == 0
    # a checkpoint without the key, loaded with the feature on: w = 0 and one warning; the key with the feature off: ignored
    with pytest.warns(UserWarning, match="w = 0") as rec:
        fresh = _train(runs["cfg"], runs["sd"], 0, True, resume=runs["off"]["ckpt"])
    assert len([x for x in rec if "w = 0" in str(x.message)]) == 1 and not fresh["lw"].w.any()
    with warnings.catch_warnings(record=True) as quiet:
        warnings.simplefilter("always")
        assert _train(runs["cfg"], runs["sd"], 0, False, resume=ck)["lw"] is None
    assert not [x for x in quiet if "loss weighting" in str(x.message)]


# ---------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, mode, out_dir):
    """Two processes on cuda:0, gloo rendezvous (the pattern of tests/test_dp_gpu.py): two steps, rank batch 4 in one microbatch."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), MD_DETERMINISTIC="1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import microdit_ref as orc
        from micro_diffusion_amd.trainer import FusedAdamW, LRSchedule, Trainer
        cfg = orc.tiny_config()
        model = _product(cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 61)))
        opt = FusedAdamW(model.dit, lr=LR)
        lw = lwm.LossWeighting(channels=128, seed=3, device=DEV)
        kw = dict(exchange="bf16", dp_mode="sharded") if mode == "sharded" else dict(dp_mode="allreduce")
        tr = Trainer(model, opt, LRSchedule("constant", alpha=1.0), clip_norm=0.25, microbatch_size=4, loss_weighting=lw, **kw)
        assert tr.world == world and tr.sharded == (mode == "sharded")
        log = []
        _record(lw, log)
        in_sync, w_steps = [], []
        for i in range(2):
            batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 8, 900 + i)
            lo = rank * 4
            model._noise_fn = lambda b, lo=lo: (rnd[lo:lo + 4].cuda(), epsn[lo:lo + 4].cuda(), mnoise[lo:lo + 4].cuda())
            log.append([])
            tr.train_step({k: v[lo:lo + 4].cuda() for k, v in batch.items()})
            torch.cuda.synchronize()
            in_sync.append(tr.replicas_in_sync())
            w_steps.append(lw.w.detach().cpu().clone())
        w_end = lw.w.clone()
        if rank == 0:
            lw.w[5] += 1e-6                                       # one weight of one rank off by a little: the check must see it
        diverged_seen = not tr.replicas_in_sync()
        lw.w.copy_(w_end)
        d = tr.diagnostics()["loss_weighting"]
        torch.save({"w": w_end.cpu(), "w_steps": w_steps, "log": _to_cpu(log), "in_sync": in_sync, "diverged_seen": diverged_seen, "objective": d["objective"],
                    "freq": lw.freq.cpu(), "phase": lw.phase.cpu()}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_two_ranks(hip, mode, monkeypatch):
    """w is bit-identical on both ranks and replicas_in_sync() covers it.  Against one rank on the concatenated batch: the ranks' recorded
    (c_noise, loss_per_sample) are replayed through ONE LossWeighting with the whole batch of 8 per step (the kernels and md_adamw_step
    on this GPU); the two-rank w and the replayed w each lie within the bound on w of its fp64 trajectory, so they differ by at most the
    sum of the two (2 x the backward bound, carried to w).  The DiT itself is left out of that comparison on purpose: under the sharded
    exchange its gradients cross the ranks as bf16, which no one-rank run reproduces to fp32 rounding, and from step 2 on the fp32
    exchange too sums the ranks' gradients in another order than one rank's accumulation.  Step 1 has no such obstacle (w = 0, the
    same initial weights, a rank's microbatch of 4 is a microbatch of 4 of the one-rank run): in all-reduce mode it is compared with a
    REAL one-rank Trainer step on the 8-sample batch -- the per-sample losses must agree bit for bit and w within the same allowance."""
    with tempfile.TemporaryDirectory() as td:
        ctx = mp.get_context("spawn")
        port = _free_port()
        procs = [ctx.Process(target=_rank_main, args=(r, 2, port, mode, td)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
        codes = [p.exitcode for p in procs]
        assert codes == [0, 0], f"rank processes failed: {codes}"
        r0, r1 = (torch.load(os.path.join(td, f"rank{r}.pt")) for r in range(2))
    assert torch.equal(r0["w"], r1["w"]) and bool(r0["w"].any()), "w must be bit-identical on both ranks"
    assert r0["in_sync"] == r1["in_sync"] == [True, True] and r0["diverged_seen"] and r1["diverged_seen"]
    assert r0["objective"] == r1["objective"] and math.isfinite(r0["objective"])
    assert torch.equal(r0["freq"], r1["freq"]) and torch.equal(r0["phase"], r1["phase"])
    one = lwm.LossWeighting(channels=128, seed=3, device=DEV)
    two_rank_steps, one_rank_steps = [], []
    for a, b in zip(r0["log"], r1["log"]):
        (c0, l0, g0), (c1, l1, g1) = a[0], b[0]
        assert g0 == g1 == 1.0
        c, l = torch.cat([c0, c1]).to(DEV), torch.cat([l0, l1]).to(DEV)
        one.forward(c)
        one.backward(c, l, 1.0)
        one.step(LR)
        two_rank_steps.append([(c0, l0, 1.0), (c1, l1, 1.0)])         # the all-reduce adds the second rank's sum to the first's
        one_rank_steps.append([(c.cpu(), l.cpu(), 1.0)])
    torch.cuda.synchronize()
    (_, b2), (_, b1) = w_reference(one.freq, one.phase, two_rank_steps, LR, 0.5)[-1], w_reference(one.freq, one.phase, one_rank_steps, LR)[-1]
    worst = float(((r0["w"].double() - one.w.double().cpu()).abs() / (b1 + b2)).max())
    print(f"{mode}: worst |w(two ranks) - w(one rank, concatenated batch)| / (sum of the two bounds) = {worst:.3f}")
    assert worst <= 1.0

    if mode == "allreduce":
        from oracle import microdit_ref as orc
        from micro_diffusion_amd.trainer import FusedAdamW, LRSchedule, Trainer
        monkeypatch.setenv("MD_DETERMINISTIC", "1")
        cfg = orc.tiny_config()
        model = _product(cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 61)))
        lw1 = lwm.LossWeighting(channels=128, seed=3, device=DEV)
        tr = Trainer(model, FusedAdamW(model.dit, lr=LR), LRSchedule("constant", alpha=1.0), clip_norm=0.25, microbatch_size=4, loss_weighting=lw1)
        log = []
        _record(lw1, log)
        _step(model, tr, cfg, 8, 900, log)
        (c0, l0, _), (c1, l1, _) = r0["log"][0][0], r1["log"][0][0]
        (ca, la, ga), (cb, lb, gb) = log[0]
        assert ga == gb == 0.5
        assert torch.equal(ca.cpu(), c0) and torch.equal(cb.cpu(), c1), "c_noise of the one-rank microbatches differs from the ranks'"
        assert torch.equal(la.cpu(), l0) and torch.equal(lb.cpu(), l1), "per-sample losses of step 1 differ between one rank and two"
        (_, e2), (_, e1) = w_reference(one.freq, one.phase, two_rank_steps[:1], LR, 0.5)[0], w_reference(one.freq, one.phase, log, LR)[0]
        worst = float(((r0["w_steps"][0].double() - lw1.w.double().cpu()).abs() / (e1 + e2)).max())
        print(f"allreduce, step 1: worst |w(two ranks) - w(one-rank Trainer, batch of 8)| / (sum of the two bounds) = {worst:.3f}")
        assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------- train.py end to end
def test_train_py_switch_checkpoint_and_autoresume(hip, tmp_path, capsys):
    """train.py with misc.loss_uncertainty_weighting on synthetic data: the log line carries weighted_loss next to the raw loss, the
    checkpoint carries state["loss_weighting"] beside an unchanged model entry, and autoresume continues w, its moments and its step."""
    import json
    import train as train_mod
    target = "micro_diffusion.datasets.latents_loader.build_streaming_latents_dataloader"
    folder = os.path.join(tmp_path, "run")

    def cfg(max_ba, **trainer):
        return {
            "seed": 18,
            "model": {"_target_": "micro_diffusion.models.model.create_latent_diffusion", "dit_arch": "MicroDiT_Tiny_2", "latent_res": 32,
                      "in_channels": 4, "pos_interp_scale": 1.0, "dtype": "bfloat16", "precomputed_latents": True, "p_mean": -0.6,
                      "p_std": 1.2, "train_mask_ratio": 0.75, "vae_name": "x", "text_encoder_name": "openclip:hf-hub:apple/DFN5B-CLIP-ViT-H-14-378"},
            "optimizer": {"_target_": "torch.optim.AdamW", "lr": 1e-4, "weight_decay": 0.1, "eps": 1e-8, "betas": [0.9, 0.999]},
            "scheduler": {"_target_": "composer.optim.ConstantScheduler", "alpha": 1.0},
            "algorithms": {"gradient_clipping": {"clip_norm": 0.25, "clipping_type": "norm"}},
            "dataset": {"image_size": 256, "train_batch_size": 8, "eval_batch_size": 8, "cap_drop_prob": 0.1,
                        "train": {"_target_": target, "datadir": "synthetic"}},
            "trainer": dict({"max_duration": f"{max_ba}ba", "device_train_microbatch_size": 4, "save_interval": "2ba", "save_folder": folder}, **trainer),
            "misc": {"log_interval": 1, "loss_uncertainty_weighting": True, "loss_uncertainty_channels": 64, "loss_uncertainty_lr": 1e-3},
        }
    tr = train_mod.train(cfg(2))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    logged = [l for l in lines if "loss" in l]
    assert [l["batch"] for l in logged] == [1, 2] and all(math.isfinite(l["weighted_loss"]) and math.isfinite(l["loss"]) for l in logged)
    lw = tr.loss_weighting
    assert lw.channels == 64 and lw.lr == 1e-3 and lw.step_count == 2 and bool(lw.w.any()) and tr.model.loss_weighting is lw
    ck = torch.load(os.path.join(folder, "latest.pt"), map_location="cpu")
    saved = ck["state"]["loss_weighting"]
    assert set(ck["state"]) == {"model", "loss_weighting"} and len(ck["state"]["model"]) == len(tr.model.dit.state_dict())
    assert torch.equal(saved["w"], lw.w.cpu()) and torch.equal(saved["m"], lw.m.cpu()) and saved["step"] == 2 and saved["channels"] == 64
    tr2 = train_mod.train(cfg(3, autoresume=True))
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert any(l.get("resumed_from") for l in out) and [l["batch"] for l in out if "loss" in l] == [3]
    lw2 = tr2.loss_weighting
    assert lw2.step_count == 3 and torch.equal(lw2.freq.cpu(), saved["freq"]) and not torch.equal(lw2.w.cpu(), saved["w"])
    # one more AdamW step from the restored state moves every weight by at most lr (|m_hat| / sqrt(v_hat) <= 1 / sqrt(1 - beta2) only in
    # the first steps, where it is ~1): a restart from zero moments or zero w would not stay this close
    assert float((lw2.w.cpu() - saved["w"]).abs().max()) <= 1.5e-3
