"""Input gradients on the GPU: the three kernels against fp64 formulas on the same bf16 operands (derived bounds, guard
elements, same bits twice, refusals), then the gradients of x, t and y through the whole network against the CPU fp32 oracle's autograd
(the bounds tests/test_engine_gpu.py uses for parameter gradients), the bit-level invariants of the dgrad-only backward, forward_with_cfg,
model_forward_wrapper, edm_loss's caption gradient and a descent step with LearnedCaption.  Measured values go to
<report dir>/input_grads_<case>.json; the report dir is $MD_TEST_REPORT_DIR, or test_reports/ under the working directory."""
import ctypes
import json
import math
import os

import pytest
import torch

from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


def _st():
    return torch.cuda.current_stream().cuda_stream


def _report(case, rep):
    out = os.environ.get("MD_TEST_REPORT_DIR", "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"input_grads_{case}.json"), "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps(rep, indent=1))


# ------------------------------------------------------------------------------------------------ md_patch_embed_dgrad
# (B, C, H, W, p, D, kernel the shape must take: 1 = MFMA, 0 = plain FMA)
PED_SHAPES = [(3, 4, 6, 10, 2, 128, 1),        # odd batch, 15 rows per sample, 45 rows: fewer than one 64-row workgroup
              (2, 16, 8, 8, 2, 256, 1),        # patch_vec 64: four column tiles per wave
              (2, 3, 6, 10, 2, 128, 0),        # patch_vec 12: the plain path
              (2, 4, 32, 32, 2, 1024, 1)]      # XL/2 width and token grid: 32 workgroups, four passes over W


def _to_image(dpatch, B, C, H, W, p):
    """[B*T, C*p*p] with (c, ph, pw) columns -> [B, C, H, W]: the transpose of md_patchify's gather."""
    return dpatch.view(B, H // p, W // p, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


def _ped_call(hip, dtok, ld, w, scale, dx, B, C, H, W, p, D):
    path = ctypes.c_int32(-7)
    rc = hip.lib().md_patch_embed_dgrad(dtok.data_ptr(), ld, w.data_ptr(), None if scale is None else scale.data_ptr(), dx.data_ptr(), B, C, H,
                                        W, p, D, ctypes.byref(path), _st())
    return rc, path.value


@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("B,C,H,W,p,D,want_path", PED_SHAPES)
def test_patch_embed_dgrad_against_fp64(hip, B, C, H, W, p, D, want_path, scaled, pad):
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + D + pad)
    M, pv, ld = B * (H // p) * (W // p), C * p * p, D + pad
    buf = torch.randn(M, ld, generator=g).to(torch.bfloat16).cuda()
    dtok = buf[:, :D]                                          # row pitch ld: the pad columns hold other finite values
    w = (torch.randn(D, pv, generator=g) * 0.25).to(torch.bfloat16).cuda()
    scale = (0.25 + torch.rand(B, generator=g) * 2).cuda() if scaled else None
    n = B * C * H * W
    full = torch.full((64 + n + 64,), -77.0, device="cuda")  # guard elements in front of and behind dx
    dx = full[64:64 + n].view(B, C, H, W)
    rc, path = _ped_call(hip, buf, ld, w, scale, dx, B, C, H, W, p, D)
    torch.cuda.synchronize()
    assert rc == 0 and path == want_path, (rc, path)
    assert float(full[:64].min()) == -77.0 == float(full[:64].max()) and float(full[64 + n:].min()) == -77.0 == float(full[64 + n:].max())
    s64 = scale.double().view(B, 1, 1, 1) if scaled else 1.0
    ref = _to_image(dtok.double() @ w.double(), B, C, H, W, p) * s64
    # fp32 accumulation of D exact products, the scale multiply and the final rounding: (D + 2) u sum_d |dtok w|, times the scale
    bound = (D + 2) * U * _to_image(dtok.double().abs() @ w.double().abs(), B, C, H, W, p) * s64
    err = (dx.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"patch_embed_dgrad {(B, C, H, W, p, D)} scaled={scaled} pad={pad}: worst error / bound = {worst:.4f}, path = {path}")
    assert bool((err <= bound).all()), worst
    again = torch.full_like(full, 3.0)[64:64 + n].view(B, C, H, W)
    assert _ped_call(hip, buf, ld, w, scale, again, B, C, H, W, p, D)[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(again, dx), "a second call must give the same bits"


def test_patch_embed_dgrad_refusals_leave_the_output_untouched(hip):
    B, C, H, W, p, D = 2, 4, 8, 8, 2, 128
    dtok = torch.randn(B * 16, D, device="cuda").to(torch.bfloat16)
    w = torch.randn(D, 16, device="cuda").to(torch.bfloat16)
    dx = torch.full((B, 16, 8, 8), -5.0, device="cuda")        # large enough for every variant below
    L = hip.lib()

    def call(dtok_p=dtok.data_ptr(), ld=D, w_p=w.data_ptr(), dx_p=dx.data_ptr(), B=B, C=C, H=H, W=W, p=p, D=D):
        return L.md_patch_embed_dgrad(dtok_p, ld, w_p, None, dx_p, B, C, H, W, p, D, None, _st())
    bad = [dict(dtok_p=None), dict(w_p=None), dict(dx_p=None), dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(p=0), dict(D=0), dict(H=7),
           dict(W=9), dict(D=124, ld=124), dict(ld=D - 8), dict(C=17), dict(p=8)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert float(dx.min()) == -5.0 == float(dx.max())
    assert call() == 0                                        # the same call without a defect runs
    torch.cuda.synchronize()
    assert float(dx[:, :4].max()) != -5.0


# ------------------------------------------------------------------------------------------------ md_timestep_embed_bwd
def _temb_bwd_check(hip, t, seed):
    B, dim, half = t.numel(), 512, 256
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(B, dim, generator=g).to(torch.bfloat16).cuda()
    full = torch.full((B + 8,), -9.0, device="cuda")
    dt = full[:B]
    L = hip.lib()
    tc = t.float().cuda()
    assert L.md_timestep_embed_bwd(tc.data_ptr(), dout.data_ptr(), dt.data_ptr(), B, dim, _st()) == 0
    torch.cuda.synchronize()
    assert float(full[B:].min()) == -9.0 == float(full[B:].max()), "guard behind dt"
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = t.double().view(B, 1) * f
    d = dout.double().cpu()
    dcos, dsin = d[:, :half], d[:, half:]
    ref = (f * (a.cos() * dsin - a.sin() * dcos)).sum(1)
    # the sum of 512 rounded terms and a few ulps per sinf / cosf / expf: (512 + 16) u sum_k f_k (|dsin| + |dcos|)
    bound = (512 + 16) * U * (f * (dsin.abs() + dcos.abs())).sum(1)
    err = (dt.double().cpu() - ref).abs()
    print(f"timestep_embed_bwd t={t.tolist()}: error / bound = {(err / bound).tolist()}")
    assert bool((err <= bound).all()), (err / bound).tolist()
    again = torch.empty(B, device="cuda")
    assert L.md_timestep_embed_bwd(tc.data_ptr(), dout.data_ptr(), again.data_ptr(), B, dim, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(again, dt), "same bits twice"


@pytest.mark.parametrize("tval", [-2.0, -0.3, 0.0, 1.2])
def test_timestep_embed_bwd_one_sample(hip, tval):
    _temb_bwd_check(hip, torch.tensor([tval]), 31)


def test_timestep_embed_bwd_five_samples(hip):
    _temb_bwd_check(hip, torch.tensor([-2.0, -0.3, 0.0, 1.2, 0.55]), 32)       # a second workgroup with one live wave


# ------------------------------------------------------------------------------------------------ md_cast_rows_from_bf16
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16])
def test_caption_gradient_cast(hip, out_dtype):
    B, Lc, C = 3, 7, 40                                        # 840 elements: not a multiple of the 256-thread workgroup
    x = (torch.randn(B * Lc, C, generator=torch.Generator().manual_seed(9)) * 3).to(torch.bfloat16).cuda()
    rs = torch.tensor([1.0, 0.0, 0.37], device="cuda")
    full = torch.full((B * Lc * C + 16,), 5.0, device="cuda", dtype=out_dtype)
    y = full[:B * Lc * C].view(B * Lc, C)
    code = 0 if out_dtype == torch.float16 else 1
    assert hip.lib().md_cast_rows_from_bf16(x.data_ptr(), y.data_ptr(), code, B * Lc, C, rs.data_ptr(), Lc, _st()) == 0
    torch.cuda.synchronize()
    ref = (x.float() * rs.repeat_interleave(Lc).view(-1, 1)).to(out_dtype)
    assert torch.equal(y, ref)
    assert float(y[Lc:2 * Lc].abs().max()) == 0.0, "a dropped caption gets an exactly zero gradient"
    assert float(full[B * Lc * C:].min()) == 5.0 == float(full[B * Lc * C:].max())
    assert hip.lib().md_cast_rows_from_bf16(x.data_ptr(), y.data_ptr(), code, B * Lc, C, None, 0, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, x.float().to(out_dtype))


# ------------------------------------------------------------------------------------------------ through the network
def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)))


def _compare(got, ref):
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().flatten()
    ng, nr = float(got.norm()), float(ref.norm())
    return {"cosine": float(got @ ref) / (ng * nr), "norm": ng, "norm_oracle": nr, "rel_rms": _rel_rms(got, ref)}


def _within(m):
    """The bounds tests/test_engine_gpu.py sets for gradients against the oracle."""
    return m["cosine"] >= 0.99 and abs(m["norm"] - m["norm_oracle"]) <= 0.03 * m["norm_oracle"] and m["rel_rms"] <= 0.15


def build_product(cfg, sd, p_mean=-0.6, p_std=1.2, ratio=0.0):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd, strict=True)
    d = d.to("cuda")
    m = LatentDiffusion(d, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), p_mean=p_mean, p_std=p_std, train_mask_ratio=ratio)
    m.train()
    return m


def _inputs(cfg, B, cap, seed):
    g = torch.Generator().manual_seed(seed)
    T = (cfg.input_size // cfg.patch_size) ** 2
    x = torch.randn(B, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g)
    t = torch.rand(B, generator=g) * 3.2 - 2.0                 # ln(sigma) / 4 of the training and sampling noise levels
    y = torch.randn(B, 1, cap, cfg.caption_channels, generator=g)
    cot = torch.randn(B, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g)
    mnoise = torch.rand(B, T, generator=g)
    return x, t, y, cot, mnoise


_ORACLE = {}


def _oracle_grads(tag, cfgf, B, cap, seed, ratio):
    """The oracle's output and input gradients under the cotangent, computed once per case and left unchanged."""
    if tag not in _ORACLE:
        cfg = cfgf()
        sd = orc.synth_state_dict(cfg, seed)
        x, t, y, cot, mnoise = _inputs(cfg, B, cap, seed + 1)
        xo, to, yo = (v.clone().requires_grad_(True) for v in (x, t, y))
        sample, _ = orc.dit_forward(sd, cfg, xo, to, yo, ratio, mnoise if ratio > 0 else None)
        (sample * cot).sum().backward()
        _ORACLE[tag] = (cfg, sd, (x, t, y, cot, mnoise), sample.detach(), xo.grad, to.grad, yo.grad)
    return _ORACLE[tag]


NET_CASES = [("micro_mask0_cap8", orc.micro_config, 8, 8, 41, 0.0),
             ("micro_mask50_cap77", orc.micro_config, 8, 77, 42, 0.5),
             ("tiny_mask0_cap77", orc.tiny_config, 8, 77, 43, 0.0),
             ("tiny_mask50_cap8", orc.tiny_config, 8, 8, 44, 0.5)]


@pytest.mark.parametrize("tag,cfgf,B,cap,seed,ratio", NET_CASES)
def test_input_gradients_against_the_oracle(hip, tag, cfgf, B, cap, seed, ratio):
    """dx, dy and dt of forward_without_cfg on a frozen network against the oracle's autograd (CPU fp32).
    Measured on an MI355X (input_grads_<case>.json in the report dir): see DESIGN.md 4.17."""
    cfg, sd, (x, t, y, cot, mnoise), osample, odx, odt, ody = _oracle_grads(tag, cfgf, B, cap, seed, ratio)
    model = build_product(cfg, sd, ratio=ratio)
    dit = model.dit
    dit.requires_grad_(False)
    xg, tg, yg = (v.cuda().requires_grad_(True) for v in (x, t, y))
    log = dit.engine.input_grad_log = []
    out = dit.forward_without_cfg(xg, tg, yg, mask_ratio=ratio, mask_noise=mnoise.cuda() if ratio > 0 else None)
    (out["sample"] * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert xg.grad.shape == x.shape and tg.grad.shape == t.shape and yg.grad.shape == y.shape
    assert ("md_patch_embed_dgrad", 1) in log, log           # patch_vec 16: the MFMA kernel
    assert all(p.grad is None for p in dit.parameters())
    rep = {"case": tag, "sample_rel_rms": _rel_rms(out["sample"].detach().cpu(), osample),
           "dx": _compare(xg.grad, odx), "dy": _compare(yg.grad, ody), "dt": _compare(tg.grad, odt),
           "dt_product": tg.grad.cpu().tolist(), "dt_oracle": odt.tolist()}
    _report(tag, rep)
    assert rep["sample_rel_rms"] <= 0.03
    for k in ("dx", "dy", "dt"):
        assert _within(rep[k]), (k, rep[k])


def _dtok_of(cot, tape, cfg):
    """The token-space cotangent _DiTFunction.backward hands to the engine."""
    B, C, p = tape.B, cfg.in_channels, cfg.patch_size
    g = tape.H // p
    d = cot.contiguous().view(B, C, g, p, g, p).permute(0, 2, 4, 3, 5, 1).reshape(B * g * g, p * p * C)
    if tape.keep_rows is not None:
        d = d[tape.keep_rows.long()]
    return d.to(torch.bfloat16).contiguous()


@pytest.mark.parametrize("prune", [True, False])
def test_dgrad_only_backward_invariants(hip, prune):
    """Bit-level: the input gradients do not depend on whether parameter gradients are taken, the parameter gradients do not depend on
    whether input gradients are taken, a frozen network's backward touches no gradient storage, and a pass without input gradients
    is launch for launch the engine's plain backward.  Deterministic mode: two runs of one backward give the same bits."""
    cfg = orc.tiny_config()
    sd = orc.synth_state_dict(cfg, 51)
    ratio, B = 0.5, 3
    x, t, y, cot, mnoise = (v.cuda() for v in _inputs(cfg, B, 8, 52))
    y = y.half()                                               # an f16 caption tensor gets an f16 gradient
    dit = build_product(cfg, sd, ratio=ratio).dit
    eng = dit.engine
    eng.deterministic, eng.prune_masked_experts = True, prune

    def run(inputs_grad, params_grad):
        dit.requires_grad_(params_grad)
        for p_ in dit.parameters():
            p_.grad = None
        xs, ts, ys = (v.clone().requires_grad_(inputs_grad) for v in (x, t, y))
        eng.gemm_log = []
        out = dit.forward_without_cfg(xs, ts, ys, mask_ratio=ratio, mask_noise=mnoise)["sample"]
        n_fwd = len(eng.gemm_log)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        log, eng.gemm_log = eng.gemm_log, None
        pg = [None if p_.grad is None else p_.grad.clone() for p_ in dit.parameters()]
        return out.detach().clone(), pg, (xs.grad, ts.grad, ys.grad), log[n_fwd:]

    out_a, pg_a, ig_a, bwd_a = run(True, True)
    out_b, pg_b, ig_b, bwd_b = run(False, True)
    assert ig_a[2].dtype == torch.float16 and ig_a[2].shape == y.shape and ig_a[0].dtype == torch.float32 and ig_a[1].shape == t.shape
    assert all(g is None for g in ig_b)
    assert torch.equal(out_a, out_b) and all(torch.equal(a, b) for a, b in zip(pg_a, pg_b)), "p.grad must not depend on the input gradients"
    # frozen: nothing attached, the flat gradient buffer (pre-filled with a sentinel) bit-unchanged, the same input gradients
    flat_g = dit.flat_buffers()["g"]
    flat_g.fill_(123.5)
    out_c, pg_c, ig_c, bwd_c = run(True, False)
    assert all(g is None for g in pg_c), "a frozen network gets no p.grad"
    assert float(flat_g.min()) == 123.5 == float(flat_g.max()), "the dgrad-only backward must not write the gradient buffer"
    assert torch.equal(out_c, out_a) and all(torch.equal(a, c) for a, c in zip(ig_a, ig_c)), "dx, dt, dy must not depend on param_grads"
    assert len(bwd_c) < len(bwd_b), (len(bwd_c), len(bwd_b))
    flat_g.zero_()
    # the engine's plain backward, called the way the Trainer calls it: the same output, gradients and GEMM launches as run b
    dit.requires_grad_(True)
    for p_ in dit.parameters():
        p_.grad = None
    dit.attach_grads()
    eng.gemm_log = []
    tape = eng.forward(x, t, y, mask_ratio=ratio, mask_noise=mnoise, record_tape=True)
    out_d = eng.sample_image(tape)
    n_fwd = len(eng.gemm_log)
    res = eng.backward(tape, _dtok_of(cot, tape, cfg))
    torch.cuda.synchronize()
    bwd_d, eng.gemm_log = eng.gemm_log[n_fwd:], None
    assert res.dx is None and res.dt is None and res.dy is None
    assert torch.equal(out_d, out_b) and all(torch.equal(p_.grad, b) for p_, b in zip(dit.parameters(), pg_b))
    assert bwd_d == bwd_b, "without input gradients the backward launches the GEMMs of the plain backward"
    # a one-element t gets the batch sum
    dit.requires_grad_(False)
    t1 = t[:1].clone().requires_grad_(True)
    tB = t[:1].expand(B).clone().requires_grad_(True)
    for tt in (t1, tB):
        (dit.forward_without_cfg(x, tt, y, mask_ratio=ratio, mask_noise=mnoise)["sample"] * cot).sum().backward()
    assert t1.grad.shape == (1,) and torch.allclose(t1.grad, tB.grad.sum().view(1), rtol=1e-5, atol=1e-6)
    _report(f"invariants_prune{int(prune)}", {"gemm_launches_full_backward": len(bwd_b), "gemm_launches_dgrad_only": len(bwd_c),
                                               "gemm_launches_full_with_inputs": len(bwd_a)})


def test_cond_stays_inference_only(hip):
    cfg = orc.micro_config()
    dit = build_product(cfg, orc.synth_state_dict(cfg, 61)).dit
    dit.requires_grad_(False)
    x, t, y, _, _ = (v.cuda() for v in _inputs(cfg, 2, 8, 62))
    cond = dit.encode_condition(y)
    dit.forward_without_cfg(x, t, y, cond=cond)              # frozen, no input requires grad: allowed, as before
    with pytest.raises(RuntimeError, match="inference-only"):
        dit.forward_without_cfg(x.clone().requires_grad_(True), t, y, cond=cond)


def test_forward_with_cfg_gradient(hip):
    """x.grad of the batch-doubled guided pass against the gradient assembled from two forward_without_cfg calls (both bf16 paths)."""
    cfg = orc.tiny_config()
    dit = build_product(cfg, orc.synth_state_dict(cfg, 71)).dit
    dit.requires_grad_(False)
    dit.engine.deterministic = True
    w = 3.0
    x, t, y, cot, _ = (v.cuda() for v in _inputs(cfg, 2, 8, 72))
    xa = x.clone().requires_grad_(True)
    (dit.forward_with_cfg(xa, t, y, cfg=w)["sample"] * cot).sum().backward()
    xb = x.clone().requires_grad_(True)
    c = dit.forward_without_cfg(xb, t, y)["sample"]
    u = dit.forward_without_cfg(xb, t, torch.zeros_like(y))["sample"]
    ((u + w * (c - u)) * cot).sum().backward()
    torch.cuda.synchronize()
    rr = _rel_rms(xa.grad.cpu(), xb.grad.cpu())
    _report("forward_with_cfg", {"rel_rms": rr, "norm": float(xa.grad.norm())})
    assert float(xb.grad.norm()) > 0 and rr <= 1e-2, rr


def test_model_forward_wrapper_gradient(hip):
    """dD/dx of the EDM-preconditioned denoiser against the oracle: c_skip + c_out c_in dF/dx, here through the oracle's autograd on
    the same formula."""
    tag = "wrapper_tiny"
    cfg = orc.tiny_config()
    sd = orc.synth_state_dict(cfg, 81)
    B, sdata = 4, 0.9
    x, _, y, cot, _ = _inputs(cfg, B, 8, 82)
    sigma = torch.tensor([0.05, 0.4, 1.5, 20.0])
    xo = x.clone().requires_grad_(True)
    s4 = sigma.view(-1, 1, 1, 1)
    c_skip, c_out, c_in = sdata ** 2 / (s4 ** 2 + sdata ** 2), s4 * sdata / (s4 ** 2 + sdata ** 2).sqrt(), 1 / (sdata ** 2 + s4 ** 2).sqrt()
    Fo, _ = orc.dit_forward(sd, cfg, c_in * xo, (sigma.log() / 4), y)
    ((c_skip * xo + c_out * Fo) * cot).sum().backward()
    model = build_product(cfg, sd)
    model.dit.requires_grad_(False)
    xg = x.cuda().requires_grad_(True)
    out = model.model_forward_wrapper(xg, sigma.cuda(), y.cuda(), model.dit.forward_without_cfg, mask_ratio=0.0)
    (out["sample"] * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    rep = {"case": tag, "dx": _compare(xg.grad, xo.grad)}
    _report(tag, rep)
    assert _within(rep["dx"]), rep["dx"]


def _edm_case(seed, B=4, cap=8, ratio=0.5):
    cfg = orc.tiny_config()
    sd = orc.synth_state_dict(cfg, seed)
    batch, rnd, epsn, mnoise = orc.synth_batch(cfg, B, seed + 1, cap_len=cap)
    lat, y = batch["image_latents"].float(), batch["caption_latents"].float()
    return cfg, sd, lat, y, rnd, epsn, mnoise, ratio


def test_edm_loss_caption_gradient(hip):
    """d loss / d y of LatentDiffusion.edm_loss on a frozen network against the oracle's autograd, with injected noise and a row factor
    that drops one caption; then twice in deterministic mode."""
    pm, ps = -0.6, 1.2
    cfg, sd, lat, y, rnd, epsn, mnoise, ratio = _edm_case(91)
    rs = torch.tensor([1.0, 0.0, 1.0, 1.0])
    yo = y.clone().requires_grad_(True)
    oloss = orc.edm_loss(sd, cfg, lat, yo * rs.view(-1, 1, 1, 1), rnd, epsn, ratio, mnoise, pm, ps)
    oloss.backward()
    model = build_product(cfg, sd, pm, ps, ratio)
    model.dit.requires_grad_(False)
    noise = (rnd.cuda(), epsn.cuda(), mnoise.cuda())

    def run():
        yg = y.cuda().requires_grad_(True)
        loss = model.edm_loss(lat.cuda(), yg, mask_ratio=ratio, _noise=noise, _y_rowscale=rs.cuda())
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), yg.grad
    loss, dy = run()
    assert all(p.grad is None for p in model.dit.parameters())
    rep = {"case": "edm_loss_dy", "loss": float(loss), "loss_oracle": oloss.item(), "dy": _compare(dy, yo.grad)}
    _report("edm_loss_dy", rep)
    assert dy.shape == y.shape and float(dy[1].abs().max()) == 0.0, "the dropped caption's rows get an exactly zero gradient"
    assert abs(float(loss) - oloss.item()) <= 0.01 * abs(oloss.item())
    assert _within(rep["dy"]), rep["dy"]
    model.dit.engine.deterministic = True
    (l1, d1), (l2, d2) = run(), run()
    assert torch.equal(l1, l2) and torch.equal(d1, d2), "deterministic mode: two runs bit-identical"
    assert float(d1[1].abs().max()) == 0.0


def test_learned_caption_descent_step(hip):
    """One step along the product's own normalised gradient of the learned tokens lowers the product's loss by at least half the
    first-order prediction.  The step length comes from the oracle alone: the largest power of two for which the oracle's loss, stepped
    along the oracle's gradient, drops within 20 % of h |g|."""
    from micro_diffusion_amd.prompt_tuning import LearnedCaption
    pm, ps = -0.6, 1.2
    cfg, sd, lat, y, rnd, epsn, mnoise, _ = _edm_case(95)
    ratio = 0.0
    pos = torch.tensor([1, 2, 5])
    init = y[0, 0, pos].clone()

    def oracle_loss(tokens):
        lc = LearnedCaption(3, cfg.caption_channels, init=tokens)
        return orc.edm_loss(sd, cfg, lat, lc(y, pos), rnd, epsn, ratio, None, pm, ps), lc
    l0, lc = oracle_loss(init)
    l0.backward()
    go = lc.tokens.grad.clone()
    gon = float(go.norm())
    h = None
    with torch.no_grad():
        for k in range(4, -11, -1):
            drop = l0.item() - float(oracle_loss(init - 2.0 ** k * go / gon)[0])
            if abs(drop - 2.0 ** k * gon) <= 0.2 * 2.0 ** k * gon:
                h, odrop = 2.0 ** k, drop
                break
    assert h is not None, "the oracle's loss is not linear along its gradient at any step tried"
    model = build_product(cfg, sd, pm, ps, ratio)
    model.dit.requires_grad_(False)
    noise = (rnd.cuda(), epsn.cuda(), None)
    learned = LearnedCaption(3, cfg.caption_channels, init=init).cuda()
    yc, latc, posc = y.cuda(), lat.cuda(), pos.cuda()
    loss0 = model.edm_loss(latc, learned(yc, posc), _noise=noise)
    loss0.backward()
    g = learned.tokens.grad.clone()
    gn = float(g.norm())
    assert all(p.grad is None for p in model.dit.parameters())
    with torch.no_grad():
        learned.tokens -= h * g / gn
        loss1 = model.edm_loss(latc, learned(yc, posc), _noise=noise)
    torch.cuda.synchronize()
    pdrop = loss0.item() - loss1.item()
    rep = {"h": h, "oracle_gnorm": gon, "oracle_drop": odrop, "product_gnorm": gn, "product_drop": pdrop, "prediction": h * max(gn, gon),
           "loss0_product": loss0.item(), "loss0_oracle": l0.item(), "grad": _compare(g, go)}
    _report("learned_caption_descent", rep)
    assert pdrop >= 0.5 * h * max(gn, gon), rep
