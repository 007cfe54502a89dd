"""Measurement-guided sampling on the GPU: the kernels of guide.hip against fp64 restatements (derived bounds, token forms
bit-equal to the image forms, same bits twice, refusals), the engine's backward to the image on a frozen conditioning (bit-equal to the
uncached and to the full dgrad-only backward), one guided evaluation and the correction through the loop against the CPU fp32 oracle's
autograd, the agreement of the sampler's modes, the acceptance test (the residual falls as the oracle's does) and the compositions.
Measured values go to <report dir>/measurement_guidance_<case>.json; the report dir is $MD_TEST_REPORT_DIR, or test_reports/ under the
working directory."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as Fn

from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
SD = 0.9                # sigma_data
TINY = 1e-30


def _st():
    return torch.cuda.current_stream().cuda_stream


def _report(case, rep):
    out = os.environ.get("MD_TEST_REPORT_DIR", "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"measurement_guidance_{case}.json"), "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps(rep, indent=1))


# ------------------------------------------------------------------------------------------------ the kernels
# (B, C, H, W, p): an odd batch on a non-square grid; patch_vec 12 (token rows element by element); the XL/2 latent grid
SHAPES = [(3, 4, 8, 12, 2), (2, 3, 8, 8, 2), (2, 4, 32, 32, 2)]


def _coefs(t):
    """c_skip, c_out, c_in of level t in fp64."""
    return SD ** 2 / (t ** 2 + SD ** 2), t * SD / math.sqrt(t ** 2 + SD ** 2), 1.0 / math.sqrt(SD ** 2 + t ** 2)


def _shifted(n, dtype, shift, fill):
    """A buffer of n elements that starts `shift` elements behind a 16-byte boundary, with 16 guard elements on either side."""
    full = torch.full((16 + shift + n + 16,), fill, device="cuda", dtype=dtype)
    return full, full[16 + shift:16 + shift + n]


def _guards_intact(full, shift, n, fill):
    head, tail = full[:16 + shift], full[16 + shift + n:]
    return bool((head == fill).all()) and bool((tail == fill).all())


def _tok_to_image(tok, B, C, H, W, p):
    """[B*T, (ph, pw, c)] -> [B, C, H, W]: md_unpatchify in torch."""
    return tok.view(B, H // p, W // p, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)


def _image_to_tok(img, B, C, H, W, p):
    return img.view(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B * (H // p) * (W // p), p * p * C)


@pytest.mark.parametrize("B,C,H,W,p", SHAPES)
def test_denoised_against_fp64_and_token_form_bit_equal(hip, B, C, H, W, p):
    L = hip.lib()
    g = torch.Generator().manual_seed(B * 100 + C * 10 + W)
    n, per, rows, pv = B * C * H * W, C * H * W, B * (H // p) * (W // p), C * p * p
    w, t = 3.0, 1.7
    c_skip, c_out, _ = _coefs(t)
    x = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2).cuda()
    tok = torch.randn(2 * rows, pv, generator=g).to(torch.bfloat16).cuda()
    for hu in (0, 1):
        Be = 2 * B if hu else B
        F = torch.empty(Be, C, H, W, device="cuda")
        assert L.md_unpatchify(tok.data_ptr(), None, 0, None, F.data_ptr(), Be, C, H, W, p, _st()) == 0
        fc, fu = F[:B].double(), F[B:].double() if hu else None
        f = fu + w * (fc - fu) if hu else fc
        x32 = x.float().double()
        ref = c_skip * x32 + c_out * f
        # x -> fp32, the two coefficients (a few roundings each), the combine (2), the product and the fma: under 8 u on the absolute terms
        terms = (c_skip * x32).abs() + c_out * ((abs(w) * (fc.abs() + fu.abs()) + fu.abs()) if hu else fc.abs())
        outs = []
        for shift in (0, 1):                                          # 16-byte items / element by element
            full, D = _shifted(n, torch.float32, shift, -77.0)
            fullF, Fs = _shifted(F.numel(), torch.float32, shift, 5.0)
            Fs.copy_(F.flatten())
            assert L.md_edm_denoised(x.data_ptr(), Fs.data_ptr(), D.data_ptr(), B, per, w, hu, t, SD, _st()) == 0
            torch.cuda.synchronize()
            assert _guards_intact(full, shift, n, -77.0)
            err = (D.view(B, C, H, W).double() - ref).abs()
            worst = float((err / (8 * U * terms).clamp_min(1e-300)).max())
            print(f"denoised {(B, C, H, W)} has_uncond={hu} shift={shift}: worst error / bound = {worst:.3f}")
            assert bool((err <= 8 * U * terms).all()), worst
            outs.append(D.clone())
        assert torch.equal(outs[0], outs[1]), "the vector and the plain path give the same bits"
        full, Dt = _shifted(n, torch.float32, 0, -77.0)
        assert L.md_edm_denoised_tok(x.data_ptr(), tok.data_ptr(), Dt.data_ptr(), B, C, H, W, p, w, hu, t, SD, _st()) == 0
        torch.cuda.synchronize()
        assert _guards_intact(full, 0, n, -77.0)
        assert torch.equal(Dt, outs[0]), "the token form gives the bits of md_unpatchify + the image form"
        if hu:                                                        # token rows that start off a 16-byte boundary: element by element
            fullT, toks = _shifted(tok.numel(), torch.bfloat16, 1, 1.0)
            toks.copy_(tok.flatten())
            again = torch.empty(n, device="cuda")
            assert L.md_edm_denoised_tok(x.data_ptr(), toks.data_ptr(), again.data_ptr(), B, C, H, W, p, w, hu, t, SD, _st()) == 0
            torch.cuda.synchronize()
            assert torch.equal(again, outs[0])
        again = torch.full((n,), 3.0, device="cuda")
        assert L.md_edm_denoised_tok(x.data_ptr(), tok.data_ptr(), again.data_ptr(), B, C, H, W, p, w, hu, t, SD, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(again, Dt), "a second call must give the same bits"


@pytest.mark.parametrize("B,C,H,W,p", SHAPES)
def test_measure_residual_against_fp64(hip, B, C, H, W, p):
    L = hip.lib()
    g = torch.Generator().manual_seed(B * 100 + C * 10 + W + 1)
    n = B * C * H * W
    Dsrc = torch.randn(B, C, H, W, generator=g).cuda()
    for s in (1, 2, 4):
        Hs, Ws = H // s, W // s
        meas = torch.randn(B, C, Hs, Ws, generator=g).cuda()
        masks = {"none": None, "1": torch.rand(1, Hs * Ws, generator=g).cuda(), "B": (torch.rand(B, Hs * Ws, generator=g) < 0.6).float().cuda()}
        for kind, mask in masks.items():
            m = torch.ones(1, 1, Hs, Ws, device="cuda", dtype=torch.float64) if mask is None else mask.double().view(-1, 1, Hs, Ws)
            pooled = Fn.avg_pool2d(Dsrc.double(), s) if s > 1 else Dsrc.double()
            pooled_abs = Fn.avg_pool2d(Dsrc.double().abs(), s) if s > 1 else Dsrc.double().abs()
            r = m * (meas.double() - pooled)
            r_terms = m * (meas.double().abs() + pooled_abs)
            up = lambda v: v.repeat_interleave(s, -2).repeat_interleave(s, -1)        # noqa: E731
            q_ref, L_ref = up(-2.0 * m * r / (s * s)), (r * r).flatten(1).sum(1)
            # the window sum (s^2 - 1 roundings), its division, the difference and the mask product: (s^2 + 2) u on the absolute terms of r;
            # q adds three roundings; L sums r^2 with a relative error twice r's plus the rounding of the fp32 square (the fp64 sum adds nothing)
            dr = (s * s + 2) * U * r_terms
            q_bound = up(2.0 * m / (s * s) * (dr + 3 * U * r_terms))
            L_bound = (2 * r.abs() * dr + dr * dr + U * (r.abs() + dr) ** 2).flatten(1).sum(1)
            ref_bits = None
            for shift in (0, 1):
                fullq, q = _shifted(n, torch.float32, shift, -77.0)
                fullD, Ds = _shifted(n, torch.float32, shift, 9.0)
                Ds.copy_(Dsrc.flatten())
                Lb = torch.full((B + 2,), -5.0, device="cuda", dtype=torch.float64)
                rc = L.md_measure_residual(Ds.data_ptr(), meas.data_ptr(), None if mask is None else mask.data_ptr(),
                                           1 if mask is None else mask.shape[0], q.data_ptr(), Lb.data_ptr(), B, C, H, W, s, _st())
                torch.cuda.synchronize()
                assert rc == 0 and _guards_intact(fullq, shift, n, -77.0) and float(Lb[B]) == -5.0 == float(Lb[B + 1])
                eq, eL = (q.view(B, C, H, W).double() - q_ref).abs(), (Lb[:B] - L_ref).abs()
                print(f"measure_residual {(B, C, H, W)} s={s} mask={kind} shift={shift}: worst q error / bound = "
                      f"{float((eq / q_bound.clamp_min(1e-300)).max()):.3f}, L error / bound = {float((eL / L_bound.clamp_min(1e-300)).max()):.3f}")
                assert bool((eq <= q_bound).all()) and bool((eL <= L_bound).all())
                if mask is not None and kind == "B":
                    zero = up((m == 0).expand(B, C, Hs, Ws))
                    assert zero.any() and float(q.view(B, C, H, W)[zero].abs().max()) == 0.0, "an unmeasured cell gets an exactly zero gradient"
                if ref_bits is None:
                    ref_bits = q.clone()
                    q2, L2 = torch.full((n,), 1.0, device="cuda"), torch.zeros(B, device="cuda", dtype=torch.float64)
                    assert L.md_measure_residual(Ds.data_ptr(), meas.data_ptr(), None if mask is None else mask.data_ptr(),
                                                 1 if mask is None else mask.shape[0], q2.data_ptr(), L2.data_ptr(), B, C, H, W, s, _st()) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(q2, q) and torch.equal(L2, Lb[:B]), "a second call must give the same bits"
                else:
                    assert torch.equal(q, ref_bits), "every cell's arithmetic is the same on the vector and the plain path"


@pytest.mark.parametrize("B,C,H,W,p", SHAPES)
def test_cotangent_and_apply_against_fp64(hip, B, C, H, W, p):
    L = hip.lib()
    g = torch.Generator().manual_seed(B * 100 + C * 10 + W + 2)
    n, per, rows, pv = B * C * H * W, C * H * W, B * (H // p) * (W // p), C * p * p
    w, t, zeta = 3.0, 0.6, 2.0
    c_skip, c_out, c_in = _coefs(t)
    q = torch.randn(B, C, H, W, generator=g).cuda()
    for hu in (0, 1):
        Be = 2 * B if hu else B
        # ---- md_guide_cotangent_tok: one bf16 rounding (8 significand bits: unit roundoff 2^-8) on top of a few fp32 ones
        refc = _image_to_tok(q.double(), B, C, H, W, p) * ((w if hu else 1.0) * c_out)
        refs = [refc] + ([_image_to_tok(q.double(), B, C, H, W, p) * ((1.0 - w) * c_out)] if hu else [])
        ref = torch.cat(refs, 0)
        bits = None
        for shift in (0, 1):
            nrows = (2 if hu else 1) * rows
            full, dtok = _shifted(nrows * pv, torch.bfloat16, shift, -3.0)
            assert L.md_guide_cotangent_tok(q.data_ptr(), dtok.data_ptr(), B, C, H, W, p, w, hu, t, SD, _st()) == 0
            torch.cuda.synchronize()
            assert _guards_intact(full, shift, nrows * pv, -3.0)
            err = (dtok.view(nrows, pv).double() - ref).abs()
            bound = ref.abs() * (2.0 ** -8 + 8 * U)
            print(f"cotangent {(B, C, H, W)} has_uncond={hu} shift={shift}: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= bound).all())
            if bits is None:
                bits = dtok.clone()
            else:
                assert torch.equal(dtok, bits)
        # ---- md_edm_guide_apply: fp64 arithmetic on fp32 coefficients (a few roundings each)
        x = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 3).cuda()
        dx = torch.randn(Be, C, H, W, generator=g).cuda()
        Lb = torch.tensor([0.0, 2.5, 7.0][:B], dtype=torch.float64).cuda()            # a sample with no residual: the floor, not a division by 0
        qq = q.clone()
        qq[0], dx[0] = 0.0, 0.0
        if hu:
            dx[B] = 0.0
        coef = (zeta / Lb.sqrt().clamp_min(TINY)).view(B, 1, 1, 1)
        dsum = dx[:B].double() + (dx[B:].double() if hu else 0.0)
        ref = x - coef * (c_skip * qq.double() + c_in * dsum)
        terms = coef * (c_skip * qq.double().abs() + c_in * (dx[:B].double().abs() + (dx[B:].double().abs() if hu else 0.0)))
        bound = 8 * U * terms + 8 * 2.0 ** -53 * (x.abs() + terms)
        bits = None
        for shift in (0, 1):
            full, xs = _shifted(n, torch.float64, shift, -9.0)
            xs.copy_(x.flatten())
            assert L.md_edm_guide_apply(xs.data_ptr(), qq.data_ptr(), dx.data_ptr(), Lb.data_ptr(), B, per, hu, zeta, t, SD, _st()) == 0
            torch.cuda.synchronize()
            assert _guards_intact(full, shift, n, -9.0)
            err = (xs.view(B, C, H, W) - ref).abs()
            print(f"guide_apply {(B, C, H, W)} has_uncond={hu} shift={shift}: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= bound).all()) and torch.equal(xs.view(B, C, H, W)[0], x[0]), "no residual, no gradient: the sample stays"
            if bits is None:
                bits = xs.clone()
            else:
                assert torch.equal(xs, bits)


def test_refusals_leave_the_outputs_untouched(hip):
    L = hip.lib()
    B, C, H, W, p = 2, 4, 8, 8, 2
    n = B * C * H * W
    x = torch.randn(n, device="cuda", dtype=torch.float64)
    F, tok = torch.randn(2 * n, device="cuda"), torch.randn(2 * n, device="cuda").to(torch.bfloat16)
    meas, Dsrc = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    out32, out64, outbf = torch.full((2 * n,), -5.0, device="cuda"), torch.full((n,), -5.0, device="cuda", dtype=torch.float64), \
        torch.full((2 * n,), -5.0, device="cuda", dtype=torch.bfloat16)
    Lb = torch.full((B,), -5.0, device="cuda", dtype=torch.float64)
    nan = float("nan")
    calls = [L.md_edm_denoised(x.data_ptr(), F.data_ptr(), out32.data_ptr(), B, C * H * W, 3.0, 1, 0.0, SD, _st()),
             L.md_edm_denoised(x.data_ptr(), F.data_ptr(), out32.data_ptr(), B, C * H * W, nan, 1, 1.0, SD, _st()),
             L.md_edm_denoised_tok(x.data_ptr(), tok.data_ptr(), out32.data_ptr(), B, C, 7, W, p, 3.0, 1, 1.0, SD, _st()),
             L.md_edm_denoised_tok(x.data_ptr(), tok.data_ptr(), out32.data_ptr(), B, C, H, W, p, 3.0, 1, -1.0, SD, _st()),
             L.md_measure_residual(Dsrc.data_ptr(), meas.data_ptr(), None, 1, out32.data_ptr(), Lb.data_ptr(), B, C, H, W, 3, _st()),
             L.md_measure_residual(Dsrc.data_ptr(), meas.data_ptr(), meas.data_ptr(), 3, out32.data_ptr(), Lb.data_ptr(), B, C, H, W, 2, _st()),
             L.md_measure_residual(Dsrc.data_ptr(), None, None, 1, out32.data_ptr(), Lb.data_ptr(), B, C, H, W, 2, _st()),
             L.md_guide_cotangent_tok(Dsrc.data_ptr(), outbf.data_ptr(), B, C, H, 9, p, 3.0, 1, 1.0, SD, _st()),
             L.md_guide_cotangent_tok(Dsrc.data_ptr(), outbf.data_ptr(), B, C, H, W, p, 3.0, 1, nan, SD, _st()),
             L.md_edm_guide_apply(out64.data_ptr(), Dsrc.data_ptr(), F.data_ptr(), Lb.data_ptr(), B, C * H * W, 1, nan, 1.0, SD, _st()),
             L.md_edm_guide_apply(out64.data_ptr(), Dsrc.data_ptr(), F.data_ptr(), Lb.data_ptr(), B, C * H * W, 1, 1.0, 0.0, SD, _st()),
             L.md_edm_guide_apply(out64.data_ptr(), Dsrc.data_ptr(), None, Lb.data_ptr(), B, C * H * W, 1, 1.0, 1.0, SD, _st())]
    torch.cuda.synchronize()
    assert calls == [-1] * len(calls), calls
    for t in (out32, out64, outbf, Lb):
        assert float(t.double().min()) == -5.0 == float(t.double().max())


# ------------------------------------------------------------------------------------------------ the engine
def build_product(cfg, sd):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd, strict=True)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=cfg.input_size)
    m.eval()
    return m


@pytest.mark.parametrize("name,cfgf,cap", [("tiny", orc.tiny_config, 77), ("micro", orc.micro_config, 8)])
def test_backward_to_the_image_on_a_frozen_conditioning(hip, name, cfgf, cap):
    """dx of forward(patches=, cond=, input_tape=True) + backward == dx of the uncached record_tape pass stopped at the image == dx out of
    the full dgrad-only backward, bit for bit (deterministic mode); the gradient buffer keeps its sentinel; the early return launches
    strictly fewer GEMMs; what an input_tape cannot give is refused."""
    cfg = cfgf()
    dit = build_product(cfg, orc.synth_state_dict(cfg, 31)).dit
    dit.requires_grad_(False)
    eng = dit.engine
    eng.deterministic = True
    B, C, S, p = 2, cfg.in_channels, cfg.input_size, cfg.patch_size
    T, pv = (S // p) ** 2, cfg.in_channels * p * p
    g = torch.Generator().manual_seed(32)
    x = torch.randn(B, C, S, S, generator=g).cuda()
    t = (torch.rand(B, generator=g) * 3.2 - 2.0).cuda()
    y = torch.randn(B, 1, cap, cfg.caption_channels, generator=g).cuda()
    dtok = torch.randn(B * T, pv, generator=g).to(torch.bfloat16).cuda()
    flat_g = dit.flat_buffers()["g"]
    flat_g.fill_(123.5)
    cond = dit.encode_condition(y)
    patches = torch.empty(B * T, pv, device="cuda", dtype=torch.bfloat16)
    assert hip.lib().md_patchify(x.data_ptr(), None, patches.data_ptr(), B, C, S, S, p, _st()) == 0

    def run(cached, want):
        eng.gemm_log = []
        if cached:
            tape = eng.forward(None, t, None, cond=cond, patches=patches, input_tape=True)
        else:
            tape = eng.forward(x, t, y, record_tape=True)
        n_fwd = len(eng.gemm_log)
        res = eng.backward(tape, dtok, input_grads=want, param_grads=False)
        torch.cuda.synchronize()
        log, eng.gemm_log = eng.gemm_log[n_fwd:], None
        return tape.out_tok.clone(), res, log
    out_a, res_a, log_a = run(True, ("x",))
    out_b, res_b, log_b = run(False, ("x",))
    out_c, res_c, log_c = run(False, ("x", "t", "y"))
    assert torch.equal(out_a, out_b) and torch.equal(out_b, out_c)
    assert res_a.dx.shape == x.shape and res_a.dt is None and res_a.dy is None and res_b.dt is None and res_c.dt is not None
    assert float(res_a.dx.abs().max()) > 0 and torch.isfinite(res_a.dx).all()
    assert torch.equal(res_a.dx, res_b.dx), "a frozen conditioning changes nothing dx depends on"
    assert torch.equal(res_b.dx, res_c.dx), "the early return gives the bits of the full dgrad-only backward"
    assert float(flat_g.min()) == 123.5 == float(flat_g.max()), "no gradient storage is written"
    assert len(log_a) == len(log_b) < len(log_c), (len(log_a), len(log_b), len(log_c))
    _report(f"engine_{name}", {"gemm_launches_to_the_image": len(log_b), "gemm_launches_dgrad_only": len(log_c)})
    tape = eng.forward(None, t, None, cond=cond, patches=patches, input_tape=True)
    for kw in (dict(input_grads=("x", "y")), dict(input_grads=("y",)), dict(input_grads=("x", "t")), dict(input_grads=("x",), param_grads=True),
               dict(input_grads=())):
        with pytest.raises(RuntimeError, match="input_tape"):
            eng.backward(tape, dtok, **dict(dict(param_grads=False), **kw))
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.forward(None, t, None, cond=cond, patches=patches, record_tape=True)
    with pytest.raises(ValueError, match="input_tape"):
        eng.forward(x, t, y, input_tape=True)
    assert float(flat_g.min()) == 123.5 == float(flat_g.max())
    flat_g.zero_()


# ------------------------------------------------------------------------------------------------ against the oracle
def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)))


def _compare(got, ref):
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().flatten()
    ng, nr = float(got.norm()), float(ref.norm())
    return {"cosine": float(got @ ref) / (ng * nr), "norm": ng, "norm_oracle": nr, "rel_rms": _rel_rms(got, ref)}


def _within(m):
    """The bounds tests/test_input_grads_gpu.py sets for gradients against the oracle."""
    return m["cosine"] >= 0.99 and abs(m["norm"] - m["norm_oracle"]) <= 0.03 * m["norm_oracle"] and m["rel_rms"] <= 0.15


def _lm(truth, s, mask):
    from micro_diffusion_amd.inverse import LinearMeasurement
    return LinearMeasurement(Fn.avg_pool2d(truth, s) if s > 1 else truth.clone(), s, mask)


def _residual(lm, x):
    """||m * (meas - A(x))||^2 per sample, fp64 on the CPU."""
    x = x.detach().double().cpu()
    r = lm.meas.double().cpu() - (Fn.avg_pool2d(x, lm.pool) if lm.pool > 1 else x)
    if lm.mask is not None:
        r = lm.mask.double().cpu() * r
    return (r * r).flatten(1).sum(1)


def _oracle_denoise(sd, cfg, x64, sigma, y, w, lm=None):
    """The oracle's guided prediction at x64 (orc.edm_sampler's denoise) and, with a measurement, dL/dx and L by its autograd."""
    x = x64.to(torch.float32).detach().requires_grad_(lm is not None)
    s = torch.as_tensor(float(sigma), dtype=torch.float32).reshape(-1, 1, 1, 1)
    c_skip, c_out, c_in = SD ** 2 / (s ** 2 + SD ** 2), s * SD / (s ** 2 + SD ** 2).sqrt(), 1 / (SD ** 2 + s ** 2).sqrt()
    t = (s.log() / 4).flatten()
    with torch.set_grad_enabled(lm is not None):
        if w > 1.0:
            Fx, _ = orc.dit_forward(sd, cfg, torch.cat([c_in * x, c_in * x], 0), t, torch.cat([y, torch.zeros_like(y)], 0), 0.0)
            cond, uncond = Fx.chunk(2, 0)
            Fx = uncond + w * (cond - uncond)
        else:
            Fx, _ = orc.dit_forward(sd, cfg, c_in * x, t, y, 0.0)
        D = c_skip * x + c_out * Fx
        if lm is None:
            return D.to(torch.float64), None, None
        L = lm.loss_fn(x)(D)
        g, = torch.autograd.grad(L.sum(), x)
    return D.detach().to(torch.float64), g.to(torch.float64), L.detach().to(torch.float64)


def _oracle_loop(sd, cfg, latents, y, steps, w, sampler, lm=None, zeta=0.0, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """orc.edm_sampler (heun) restated with the euler solver and the correction of DESIGN.md 4.18: after the step (Heun's second
    evaluation not differentiated) x_next[b] -= zeta / max(sqrt(L_b), tiny) * g[b], at every step."""
    idx = torch.arange(steps, dtype=torch.float64)
    t_steps = (sigma_max ** (1 / rho) + idx / (steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    t_steps = torch.cat([t_steps, torch.zeros(1, dtype=torch.float64)])
    x_next = latents.to(torch.float64) * t_steps[0]
    for i in range(steps):
        t_cur, t_next = t_steps[i], t_steps[i + 1]
        x_hat = x_next
        D, g, L = _oracle_denoise(sd, cfg, x_hat, t_cur, y, w, lm)
        d_cur = (x_hat - D) / t_cur
        x_next = x_hat + (t_next - t_cur) * d_cur
        if sampler == "heun" and i < steps - 1:
            D2, _, _ = _oracle_denoise(sd, cfg, x_next, t_next, y, w)
            x_next = x_hat + (t_next - t_cur) * (0.5 * d_cur + 0.5 * (x_next - D2) / t_next)
        if lm is not None:
            x_next = x_next - (zeta / L.sqrt().clamp_min(TINY)).view(-1, 1, 1, 1) * g
    return x_next.to(torch.float32)


EVAL_CASES = [("micro_cap8_s1", orc.micro_config, 8, 1, 61), ("micro_cap8_s2", orc.micro_config, 8, 2, 62),
              ("tiny_cap77_s1", orc.tiny_config, 77, 1, 63), ("tiny_cap77_s2", orc.tiny_config, 77, 2, 64)]


@pytest.mark.parametrize("cond_cache", [False, True])
@pytest.mark.parametrize("tag,cfgf,cap,s,seed", EVAL_CASES)
def test_one_guided_evaluation_against_the_oracle(hip, tag, cfgf, cap, s, seed, cond_cache):
    """g and L of one cfg-doubled evaluation (w = 3) at sigma = 1 against the oracle's autograd.  A two-level schedule (80, 1, 0) started
    at its last step (strength 0.5) makes the run that one evaluation: plain returns D, guided returns D - zeta / sqrt(L) g, so
    g = (plain - guided) sqrt(L) / zeta with L taken from the plain run's own D."""
    cfg = cfgf()
    sd = orc.synth_state_dict(cfg, seed)
    B, w, zeta, sigma = 3, 3.0, 4.0, 1.0
    gen = torch.Generator().manual_seed(seed + 100)
    S = cfg.input_size
    noise = torch.randn(B, cfg.in_channels, S, S, generator=gen)
    y = torch.randn(B, 1, cap, cfg.caption_channels, generator=gen)
    init = 0.5 * torch.randn(B, cfg.in_channels, S, S, generator=gen)
    truth = 0.5 * torch.randn(B, cfg.in_channels, S, S, generator=gen)
    mask = torch.rand(B, 1, S // s, S // s, generator=gen) < 0.6
    lm = _lm(truth, s, mask)
    x_hat = init.double() + sigma * noise.double()
    _, og, oL = _oracle_denoise(sd, cfg, x_hat, sigma, y, w, lm)
    model = build_product(cfg, sd)
    model.dit.engine.deterministic = True
    saved = dict(model.edm_config)
    try:
        model.edm_config.update(sigma_min=sigma)
        kw = dict(steps=2, cfg=w, fused=True, cond_cache=cond_cache, sampler="euler", init_latents=init.cuda(), strength=0.5)
        plain = model.edm_sampler_loop(noise.cuda(), y.cuda(), **kw)
        guided = model.edm_sampler_loop(noise.cuda(), y.cuda(), measurement=lm, measurement_scale=zeta, **kw)
    finally:
        model.edm_config.update(saved)
    torch.cuda.synchronize()
    Lp = _residual(lm, plain)
    gp = (plain.double().cpu() - guided.double().cpu()) * (Lp.sqrt() / zeta).view(-1, 1, 1, 1)
    rep = {"case": tag, "cond_cache": cond_cache, "g": _compare(gp, og), "L": Lp.tolist(), "L_oracle": oL.tolist()}
    _report(f"eval_{tag}_cache{int(cond_cache)}", rep)
    assert all(p.grad is None for p in model.dit.parameters())
    assert _within(rep["g"]), rep["g"]
    assert bool(((Lp - oL).abs() <= 0.03 * oL).all()), (Lp.tolist(), oL.tolist())


@pytest.mark.parametrize("sampler", ["euler", "heun"])
def test_correction_through_the_loop_against_the_oracle(hip, sampler):
    """steps = 2, cfg 3, Micro: c = guided - plain of the fused loop against the same difference of the oracle's loop.  The evaluation after
    the first correction is at sigma = 0.002, where D ~ x and nothing amplifies: this checks the plumbing (zeta / sqrt(L), the c_skip term,
    both cfg halves, the correction at the last step), not chaos."""
    cfg = orc.micro_config()
    sd = orc.synth_state_dict(cfg, 71)
    B, w, zeta, s = 3, 3.0, 2.0, 2
    gen = torch.Generator().manual_seed(72)
    S = cfg.input_size
    noise = torch.randn(B, cfg.in_channels, S, S, generator=gen)
    y = torch.randn(B, 1, 8, cfg.caption_channels, generator=gen)
    truth = 0.5 * torch.randn(B, cfg.in_channels, S, S, generator=gen)
    lm = _lm(truth, s, torch.rand(B, 1, S // s, S // s, generator=gen) < 0.6)
    oc = _oracle_loop(sd, cfg, noise, y, 2, w, sampler, lm, zeta).double() - _oracle_loop(sd, cfg, noise, y, 2, w, sampler).double()
    model = build_product(cfg, sd)
    kw = dict(steps=2, cfg=w, fused=True, sampler=sampler)
    pc = model.edm_sampler_loop(noise.cuda(), y.cuda(), measurement=lm, measurement_scale=zeta, **kw).double() - \
        model.edm_sampler_loop(noise.cuda(), y.cuda(), **kw).double()
    rep = {"sampler": sampler, "correction": _compare(pc, oc)}
    _report(f"loop_{sampler}", rep)
    assert _within(rep["correction"]), rep["correction"]


# ------------------------------------------------------------------------------------------------ the sampler's modes
def _rel(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


@pytest.fixture(scope="module")
def tiny_model(hip):
    cfg = orc.tiny_config()
    m = build_product(cfg, orc.synth_state_dict(cfg, 43))
    m.dit.engine.deterministic = True
    return m


def _tiny_inputs(B=2, s=2):
    g = torch.Generator().manual_seed(10)
    lat, y = torch.randn(B, 4, 32, 32, generator=g).cuda(), torch.randn(B, 1, 77, 1024, generator=g).cuda()
    truth = (torch.randn(B, 4, 32, 32, generator=g) * 0.5).cuda()
    mask = (torch.rand(B, 1, 32 // s, 32 // s, generator=g) < 0.6).cuda()
    return lat, y, truth, _lm(truth, s, mask)


@pytest.mark.parametrize("sampler", ["heun", "dpmpp_2m"])
def test_modes_agree(tiny_model, sampler):
    """cond_cache on and off give the same bits (deterministic mode), the fused loop is within 2e-2 of the tensor-op definition (the bound
    of tests/test_edit_sampler_gpu.py through the real network), and the guided run is not the plain one: on the parent commit the
    argument fell into **kwargs and was ignored."""
    lat, y, _, lm = _tiny_inputs()
    kw = dict(steps=4, cfg=3.0, sampler=sampler, measurement=lm, measurement_scale=2.0)
    req = [p.requires_grad for p in tiny_model.dit.parameters()]
    a = tiny_model.edm_sampler_loop(lat, y, fused=True, cond_cache=False, **kw)
    c = tiny_model.edm_sampler_loop(lat, y, fused=True, cond_cache=True, **kw)
    b = tiny_model.edm_sampler_loop(lat, y, fused=False, **kw)
    plain = tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, sampler=sampler, fused=True)
    assert torch.equal(c, a), "cond_cache must not change a bit"
    rel, moved = _rel(a, b), _rel(a, plain)
    print(sampler, "fused against tensor-op", rel, "guided against plain", moved)
    assert torch.isfinite(a).all() and rel < 2e-2, rel
    assert moved > 1e-3, "the guided run must differ from the plain run"
    assert [p.requires_grad for p in tiny_model.dit.parameters()] == req and any(req), "requires_grad is restored"
    assert all(p.grad is None for p in tiny_model.dit.parameters()), "a parameter that requires grad is never given a .grad"


def test_not_done_combinations_are_refused(tiny_model):
    lat, y, _, lm = _tiny_inputs()
    with pytest.raises(NotImplementedError, match="not done"):
        tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, measurement=lm, guide=tiny_model.dit)
    with pytest.raises(NotImplementedError, match="not done"):
        tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, measurement=lm, guidance_mode="apg")
    with pytest.raises(NotImplementedError, match="not done"):
        tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, measurement=lm, some_forward_argument=1)
    with pytest.raises(ValueError, match="mutually exclusive"):
        tiny_model.edm_sampler_loop(lat, y, steps=4, measurement=lm, guidance_loss=lambda D: D.flatten(1).sum(1))
    with pytest.raises(ValueError, match="nothing to scale"):
        tiny_model.edm_sampler_loop(lat, y, steps=4, measurement_scale=2.0)


# ------------------------------------------------------------------------------------------------ acceptance
ACCEPT = [("euler", 2, False), ("euler", 1, True), ("heun", 4, True)]


@pytest.mark.parametrize("sampler,s,masked", ACCEPT)
def test_guidance_lowers_the_residual_as_the_oracle_does(hip, sampler, s, masked):
    """It does what it is for.  Micro, 6 steps, cfg 3, zeta = 2: for every sample the final residual ||m * (meas - A(x))||^2 over the plain
    run's residual is at most 1 - (1 - rho_b) / 2, rho_b the same ratio of the oracle's loop (CPU fp32).  The synthetic network is no
    denoiser, so the reductions are modest; the half margin absorbs bf16.  A guidance_loss callable stating the same L gives the
    measurement= run to 1e-5 relative."""
    cfg = orc.micro_config()
    sd = orc.synth_state_dict(cfg, 81)
    B, w, zeta, steps = 3, 3.0, 2.0, 6
    gen = torch.Generator().manual_seed(82)
    S = cfg.input_size
    noise = torch.randn(B, cfg.in_channels, S, S, generator=gen)
    y = torch.randn(B, 1, 8, cfg.caption_channels, generator=gen)
    truth = 0.5 * torch.randn(B, cfg.in_channels, S, S, generator=gen)
    mask = torch.rand(B, 1, S // s, S // s, generator=gen) < 0.6
    lm = _lm(truth, s, mask if masked else None)
    o_plain = _oracle_loop(sd, cfg, noise, y, steps, w, sampler)
    o_guided = _oracle_loop(sd, cfg, noise, y, steps, w, sampler, lm, zeta)
    rho = _residual(lm, o_guided) / _residual(lm, o_plain)
    model = build_product(cfg, sd)
    kw = dict(steps=steps, cfg=w, fused=True, sampler=sampler)
    plain = model.edm_sampler_loop(noise.cuda(), y.cuda(), **kw)
    guided = model.edm_sampler_loop(noise.cuda(), y.cuda(), measurement=lm, measurement_scale=zeta, **kw)
    ratio = _residual(lm, guided) / _residual(lm, plain)
    rep = {"sampler": sampler, "pool": s, "masked": masked, "ratio": ratio.tolist(), "ratio_oracle": rho.tolist()}
    _report(f"accept_{sampler}_s{s}", rep)
    assert torch.isfinite(guided).all() and bool((rho < 1).all()), rep
    assert bool((ratio <= 1 - 0.5 * (1 - rho)).all()), rep
    loss = lm.loss_fn(noise.cuda())
    same = model.edm_sampler_loop(noise.cuda(), y.cuda(), guidance_loss=loss, measurement_scale=zeta, **kw)
    assert _rel(same, guided) <= 1e-5, _rel(same, guided)


# ------------------------------------------------------------------------------------------------ compositions
def test_inpainting_keeps_the_known_region(tiny_model):
    lat, y, truth, lm = _tiny_inputs()
    hole = torch.zeros(32, 32, device="cuda")
    hole[8:24, 8:24] = 1.0
    for kw in (dict(sampler="heun", fused=True, cond_cache=True), dict(sampler="euler", fused=True, resample=2), dict(sampler="euler", fused=False)):
        torch.manual_seed(5)
        out = tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, init_latents=truth, inpaint_mask=hole, measurement=lm, measurement_scale=2.0,
                                          **kw)
        keep = (hole == 0).expand(out.shape)
        assert torch.isfinite(out).all() and torch.equal(out[keep], truth[keep]), "the kept region is init_latents, bit for bit"


def test_guidance_interval_runs_the_conditional_half_and_still_corrects(tiny_model):
    """Outside the interval an evaluation runs at batch B (one term, weight 1) and its step is corrected all the same."""
    from micro_diffusion_amd import samplers
    lat, y, _, lm = _tiny_inputs()
    B, T = lat.shape[0], 256
    t = samplers.edm_schedule(4)
    interval = (math.sqrt(t[2] * t[3]), math.sqrt(t[0] * t[1]))            # steps 1 and 2 are guided by cfg, steps 0 and 3 are not
    eng = tiny_model.dit.engine
    outs = {}
    for cache in (False, True):
        eng.gemm_log = []
        outs[cache] = tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, sampler="euler", fused=True, cond_cache=cache,
                                                  guidance_interval=interval, measurement=lm, measurement_scale=2.0)
        log, eng.gemm_log = eng.gemm_log, None
        rows = {int(e[1]) for e in log}                                  # (variant, M, N, K, batch) of every GEMM launch
        assert B * T in rows and 2 * B * T in rows, "token GEMMs ran at batch B and at batch 2B"
    assert torch.equal(outs[True], outs[False])
    only_last = tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, sampler="euler", fused=True, guidance_interval=interval)
    assert _rel(outs[False], only_last) > 1e-3
    ops = tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, sampler="euler", fused=False, guidance_interval=interval, measurement=lm,
                                      measurement_scale=2.0)
    assert _rel(outs[False], ops) < 2e-2


def test_churn_repeats_with_the_seed(tiny_model):
    from micro_diffusion_amd import samplers
    lat, y, _, lm = _tiny_inputs()
    ec = tiny_model.edm_config
    t = samplers.edm_schedule(4, ec.sigma_min, ec.sigma_max, ec.rho)
    saved = dict(ec)
    try:
        ec.update(S_churn=20, S_noise=1.003, S_min=math.sqrt(t[2] * t[3]), S_max=math.sqrt(t[0] * t[1]))
        outs = []
        for seed in (3, 3, 4):
            torch.manual_seed(seed)
            outs.append(tiny_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, sampler="heun", fused=True, cond_cache=True, measurement=lm,
                                                    measurement_scale=2.0))
    finally:
        ec.update(saved)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
