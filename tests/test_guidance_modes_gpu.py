"""Guidance modes on the GPU.  Kernel level: md_guidance_prepare against the formulas in torch fp64 (M, the five
moments, the coefficients), its token form against md_unpatchify + the image form (torch.equal), the four _coef update kernels against
torch fp64, against each other and against the cfg kernel, determinism, refusals.  Through edm_sampler_loop: fused against the tensor-op
loop (2e-6 with a smooth stand-in network, 2e-2 through the real bf16 network: the bounds and the reasons of
tests/test_sampler_ckpt_gpu.py), cached against uncached (torch.equal), the interval, a guide network, inpainting, and the default
run unchanged."""
import math

import pytest
import torch

from micro_diffusion_amd import samplers
from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu

P = 2
SD = 0.9                      # sigma_data
T_IN = 1.7
W_G = 3.0
NAN = float("nan")
SHAPES = [(3, 4, 6, 10),      # 240 elements per sample: fewer than one workgroup's threads, odd batch
          (2, 16, 8, 8),      # the 16-channel VAE: patch_vec 64
          (2, 3, 6, 10),      # patch_vec 12: no multiple of 8, the element-wise token path
          (2, 4, 64, 64)]     # 16,384 elements per sample: 64 rounds per thread
COEFS = {"no_history": (0.625, 0.375, 1.0, 0.0),               # an Euler step / the first 2M step
         "history": (0.625, 0.46, 1.4, 0.4),                   # a 2M step
         "last": (0.0, 1.0, 1.0, 0.0)}                         # the step onto sigma = 0


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _precond():
    """c_skip and c_out as the kernels form them: fp32 (model.py:144-179)."""
    sigma = torch.tensor(T_IN, dtype=torch.float64).to(torch.float32)
    return SD ** 2 / (sigma ** 2 + SD ** 2), sigma * SD / (sigma ** 2 + SD ** 2).sqrt()


def _denoised64(x, F):
    """D = c_skip * float(x) + c_out * F, the products and the sum in fp64: what the kernel's fp32 value is two roundings away from."""
    c_skip, c_out = _precond()
    return c_skip.double().item() * x.to(torch.float32).double() + c_out.double().item() * F.double()


def _kernel_inputs(shape, seed=3):
    """x (fp64 state), F_c, F_u (fp32 images; F_u's distance from F_c differs by sample), M_prev (fp32)."""
    B = shape[0]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 3
    Fc = torch.randn(shape, generator=g)
    Fu = 0.5 * Fc + torch.randn(shape, generator=g) * torch.tensor([0.3, 1.0, 2.5][:B]).view(B, 1, 1, 1)
    Mp = torch.randn(shape, generator=g) * 0.5
    return x.cuda(), Fc.cuda(), Fu.cuda(), Mp.cuda()


def _params(mode, r=None):
    """(mode, w, phi, eta, has_r, r, beta) as md_guidance_prepare takes them."""
    if mode == "apg":
        return (2, W_G, 0.0, 0.25, 0 if r is None else 1, 1.0 if r is None else r, -0.5)
    return (1, W_G, 0.7, 0.0, 0, 1.0, 0.0)


def _reference(mode, x, Fc, Fu, Mp, first):
    """M, moments, (alpha, gamma), r in torch fp64.  r: the median of the per-sample norms of M."""
    D_c, D_u = _denoised64(x, Fc), _denoised64(x, Fu)
    M = D_c - D_u
    if mode == "apg" and not first:
        M = M - 0.5 * Mp.double()
    r = None
    if mode == "apg":
        norms = M.flatten(1).norm(dim=1)
        r = float(norms.median())
        assert (norms > r).any() and (norms <= r).any(), "the clip must be active for one sample and inactive for another"
    mo = samplers.guidance_moments(D_c, M)
    alpha, gamma = samplers.guidance_coefficients(mode, mo, D_c[0].numel(), W_G, guidance_rescale=0.7, apg_eta=0.25, apg_norm_threshold=r)
    return D_c, M, mo, torch.stack([alpha, gamma], 1), r


def _prepare(L, x, Fc, Fu, M_buf, params, first, tok_geo=None):
    """One md_guidance_prepare(_tok) call with one guard element behind every output; returns (M buffer, coef buffer, moments buffer)."""
    B = x.shape[0]
    n = x.numel()
    coef = torch.full((2 * B + 1,), 7.0, device="cuda")
    mom = torch.full((5 * B + 1,), 7.0, device="cuda", dtype=torch.float64)
    if tok_geo is None:
        code = L.md_guidance_prepare(x.data_ptr(), Fc.data_ptr(), Fu.data_ptr(), M_buf.data_ptr(), coef.data_ptr(), mom.data_ptr(), B, n // B,
                                     T_IN, SD, *params, first, _st())
    else:
        code = L.md_guidance_prepare_tok(x.data_ptr(), Fc, Fu, M_buf.data_ptr(), coef.data_ptr(), mom.data_ptr(), *tok_geo, P, T_IN, SD, *params,
                                         first, _st())
    assert code == 0, code
    return M_buf, coef, mom


def _m_buffer(Mp, first):
    """n + 1 floats: M_prev (NaN where it must not be read) and the guard."""
    buf = torch.full((Mp.numel() + 1,), 7.0, device="cuda")
    buf[:-1] = torch.full_like(Mp, NAN).flatten() if first else Mp.flatten()
    return buf


# ------------------------------------------------------------------------------------------------ the prepare kernel
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("mode", ["apg", "rescale"])
@pytest.mark.parametrize("shape", SHAPES)
def test_prepare_against_torch_fp64(hip, shape, mode, first):
    L, B, n = hip.lib(), shape[0], math.prod(shape)
    x, Fc, Fu, Mp = _kernel_inputs(shape)
    D_c, M_ref, mo_ref, coef_ref, r = _reference(mode, x, Fc, Fu, Mp, first)
    # rescale keeps no momentum: it never reads M_prev, first or not
    M_buf, coef, mom = _prepare(L, x, Fc, Fu, _m_buffer(Mp, first or mode == "rescale"), _params(mode, r), first)
    M, got_coef, got_mo = M_buf[:n].view(shape), coef[:2 * B].view(B, 2), mom[:5 * B].view(B, 5)
    assert M_buf[n] == 7.0 and coef[2 * B] == 7.0 and mom[5 * B] == 7.0, "wrote behind an output"
    assert torch.isfinite(M).all() and torch.isfinite(got_coef).all() and torch.isfinite(got_mo).all(), "an unread M_prev reached an output"
    rm = _rel(M.double(), M_ref)
    # S_c, S_m, Q_cm: against the sum of the magnitudes of their terms; Q_cc, Q_mm (positive terms): relative
    dc, m = D_c.flatten(1), M_ref.flatten(1)
    scale = torch.stack([dc.abs().sum(1), m.abs().sum(1), mo_ref[:, 2], mo_ref[:, 3], (dc * m).abs().sum(1)], 1)
    mo_err = ((got_mo - mo_ref).abs() / scale).max(0).values
    coef_err = ((got_coef.double() - coef_ref).abs() / (1 + coef_ref.abs())).max().item()
    print(shape, mode, first, "M", rm, "moments", mo_err.tolist(), "coef", coef_err, "coef", got_coef.tolist())
    assert rm < 2e-6, rm
    assert (mo_err <= 1e-6).all(), mo_err
    assert coef_err <= 1e-5, coef_err
    if mode == "apg":
        s = got_coef[:, 1] / (W_G - 1)
        assert (s < 0.999).any() and (s > 0.999).any(), "the clip is active for one sample and inactive for another on the device too"


@pytest.mark.parametrize("mode", ["apg", "rescale"])
@pytest.mark.parametrize("shape", SHAPES)
def test_prepare_tok_equals_unpatchify_then_prepare_and_is_deterministic(hip, shape, mode):
    B, C, H, W = shape
    L, T, pv, n = hip.lib(), (H // P) * (W // P), C * P * P, math.prod(shape)
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 3).cuda()
    tok = torch.randn(2 * B * T, pv, generator=g).to(torch.bfloat16).cuda()
    Mp = (torch.randn(shape, generator=g) * 0.5).cuda()
    img = torch.empty(2 * B, C, H, W, device="cuda")
    hip.check(L.md_unpatchify(tok.data_ptr(), None, T, None, img.data_ptr(), 2 * B, C, H, W, P, _st()), "md_unpatchify")
    par = _params(mode, 4.0)
    ref = _prepare(L, x, img[:B], img[B:], _m_buffer(Mp, 0), par, 0)
    got = _prepare(L, x, tok.data_ptr(), tok.data_ptr() + B * T * pv * 2, _m_buffer(Mp, 0), par, 0, tok_geo=(B, C, H, W))
    again = _prepare(L, x, img[:B], img[B:], _m_buffer(Mp, 0), par, 0)
    for a, b, c, what in zip(ref, got, again, ("M", "coef", "moments")):
        assert torch.equal(a, b), f"{what}: the token form differs from the image form"
        assert torch.equal(a, c), f"{what}: two calls on the same inputs differ"
    assert ref[0][n] == 7.0 and got[0][n] == 7.0
    assert not torch.equal(ref[0][:n], Mp.flatten()) and torch.isfinite(ref[1]).all()


# ------------------------------------------------------------------------------------------------ the update kernels
def _update_inputs(shape, seed=5):
    B, C, H, W = shape
    T, pv = (H // P) * (W // P), C * P * P
    g = torch.Generator().manual_seed(seed)
    x_in = (torch.randn(shape, generator=g, dtype=torch.float64) * 3).cuda()
    x_hat = (torch.randn(shape, generator=g, dtype=torch.float64) * 3).cuda()
    d0 = torch.randn(shape, generator=g, dtype=torch.float64).cuda()
    tok = torch.randn(B * T, pv, generator=g).to(torch.bfloat16).cuda()
    M = (torch.randn(shape, generator=g) * 0.7).cuda()
    coef = torch.tensor([[1.1, 1.7], [0.8, 2.3], [0.95, 4.0]][:B]).cuda().contiguous()
    img = torch.empty(shape, device="cuda")
    return x_in, x_hat, d0, tok, M, coef, img


def _guided64(x_in, F, M, coef):
    """D = alpha_b * D_c + gamma_b * M with D_c in fp32 as the existing kernels' reference forms it, the combine in fp64."""
    c_skip, c_out = _precond()
    D_c = (c_skip.cuda() * x_in.to(torch.float32) + c_out.cuda() * F).double()
    B = x_in.shape[0]
    return coef[:, 0].double().view(B, 1, 1, 1) * D_c + coef[:, 1].double().view(B, 1, 1, 1) * M.double()


@pytest.mark.parametrize("mode", list(COEFS))
@pytest.mark.parametrize("shape", SHAPES)
def test_solver_update_coef_against_torch_fp64_and_tok_equals_image(hip, shape, mode):
    B, C, H, W = shape
    L, T, n, sc = hip.lib(), (H // P) * (W // P), math.prod(shape), COEFS[mode]
    x_in, _, h0, tok, M, coef, img = _update_inputs(shape)
    hip.check(L.md_unpatchify(tok.data_ptr(), None, T, None, img.data_ptr(), B, C, H, W, P, _st()), "md_unpatchify")
    a, b, c1, c2 = sc
    den = _guided64(x_in, img, M, coef)
    want = a * x_in + b * (c1 * den - c2 * h0 if c2 != 0 else c1 * den)
    start_h = lambda: h0.clone() if c2 != 0 else torch.full_like(h0, NAN)      # noqa: E731  unread history must not reach x_next
    h_img, out = start_h(), torch.full((n + 1,), 7.0, device="cuda", dtype=torch.float64)
    hip.check(L.md_edm_solver_update_coef(x_in.data_ptr(), img.data_ptr(), M.data_ptr(), coef.data_ptr(), h_img.data_ptr(), out.data_ptr(), B,
                                          n // B, T_IN, SD, *sc, _st()), "md_edm_solver_update_coef")
    x_img = out[:n].view(shape)
    rx, rh = _rel(x_img, want), _rel(h_img, den)
    print(shape, mode, "x_next", rx, "hist", rh)
    assert torch.isfinite(x_img).all() and rx < 2e-6 and rh < 2e-6, (rx, rh)
    assert out[n] == 7.0, "wrote behind the last element"
    h_tok, x_tok = start_h(), torch.zeros_like(x_in)
    hip.check(L.md_edm_solver_update_coef_tok(x_in.data_ptr(), tok.data_ptr(), M.data_ptr(), coef.data_ptr(), h_tok.data_ptr(), x_tok.data_ptr(),
                                              B, C, H, W, P, T_IN, SD, *sc, _st()), "md_edm_solver_update_coef_tok")
    assert torch.equal(x_tok, x_img) and torch.equal(h_tok, h_img)
    # x_next may alias x_in, in both forms
    for tok_form in (False, True):
        xa, ha = x_in.clone(), start_h()
        if tok_form:
            hip.check(L.md_edm_solver_update_coef_tok(xa.data_ptr(), tok.data_ptr(), M.data_ptr(), coef.data_ptr(), ha.data_ptr(), xa.data_ptr(),
                                                      B, C, H, W, P, T_IN, SD, *sc, _st()), "md_edm_solver_update_coef_tok")
        else:
            hip.check(L.md_edm_solver_update_coef(xa.data_ptr(), img.data_ptr(), M.data_ptr(), coef.data_ptr(), ha.data_ptr(), xa.data_ptr(), B,
                                                  n // B, T_IN, SD, *sc, _st()), "md_edm_solver_update_coef")
        assert torch.equal(xa, x_img) and torch.equal(ha, h_img), tok_form


@pytest.mark.parametrize("second", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_heun_update_coef_against_torch_fp64_and_tok_equals_image(hip, shape, second):
    B, C, H, W = shape
    L, T, n = hip.lib(), (H // P) * (W // P), math.prod(shape)
    x_in, x_hat, d0, tok, M, coef, img = _update_inputs(shape, 6)
    hip.check(L.md_unpatchify(tok.data_ptr(), None, T, None, img.data_ptr(), B, C, H, W, P, _st()), "md_unpatchify")
    t_hat, t_next = (2.1, T_IN) if second else (T_IN, 1.2)     # the first half-step evaluates at t_hat, the second at t_next
    tail = (T_IN, t_hat, t_next, SD, second, _st())
    d = (x_in - _guided64(x_in, img, M, coef)) / T_IN
    want = x_hat + (t_next - t_hat) * (0.5 * d0 + 0.5 * d if second else d)
    start_d = lambda: d0.clone() if second else torch.full_like(d0, NAN)       # noqa: E731  the first half-step writes d_cur, never reads it
    d_img, out = start_d(), torch.full((n + 1,), 7.0, device="cuda", dtype=torch.float64)
    hip.check(L.md_edm_heun_update_coef(x_hat.data_ptr(), x_in.data_ptr(), img.data_ptr(), M.data_ptr(), coef.data_ptr(), d_img.data_ptr(),
                                        out.data_ptr(), B, n // B, *tail), "md_edm_heun_update_coef")
    x_img = out[:n].view(shape)
    rx = _rel(x_img, want)
    rd = 0.0 if second else _rel(d_img, d)
    print(shape, second, "x_next", rx, "d_cur", rd)
    assert torch.isfinite(x_img).all() and rx < 2e-6 and rd < 2e-6, (rx, rd)
    assert out[n] == 7.0 and torch.equal(d_img, d0) == bool(second)
    d_tok, x_tok = start_d(), torch.zeros_like(x_in)
    hip.check(L.md_edm_heun_update_coef_tok(x_hat.data_ptr(), x_in.data_ptr(), tok.data_ptr(), M.data_ptr(), coef.data_ptr(), d_tok.data_ptr(),
                                            x_tok.data_ptr(), B, C, H, W, P, *tail), "md_edm_heun_update_coef_tok")
    assert torch.equal(x_tok, x_img) and torch.equal(d_tok, d_img)
    # x_next may alias x_in (the second half-step of the sampler) or x_hat, in both forms
    for tok_form in (False, True):
        for alias in ("x_in", "x_hat"):
            xi, xh, da = x_in.clone(), x_hat.clone(), start_d()
            xo = xi if alias == "x_in" else xh
            if tok_form:
                hip.check(L.md_edm_heun_update_coef_tok(xh.data_ptr(), xi.data_ptr(), tok.data_ptr(), M.data_ptr(), coef.data_ptr(), da.data_ptr(),
                                                        xo.data_ptr(), B, C, H, W, P, *tail), "md_edm_heun_update_coef_tok")
            else:
                hip.check(L.md_edm_heun_update_coef(xh.data_ptr(), xi.data_ptr(), img.data_ptr(), M.data_ptr(), coef.data_ptr(), da.data_ptr(),
                                                    xo.data_ptr(), B, n // B, *tail), "md_edm_heun_update_coef")
            assert torch.equal(xo, x_img) and torch.equal(da, d_img), (tok_form, alias)


@pytest.mark.parametrize("shape", SHAPES)
def test_neutral_coefficients_agree_with_the_cfg_kernels(hip, shape):
    """apg with eta = 1, no threshold and no momentum is plain guidance: coef = (1, w - 1) exactly and M = D_c - D_u, so the _coef
    kernels return what the cfg kernels return, up to the different order of the fp32 combine."""
    L, B, n = hip.lib(), shape[0], math.prod(shape)
    x, Fc, Fu, Mp = _kernel_inputs(shape, 7)
    M_buf, coef, _ = _prepare(L, x, Fc, Fu, _m_buffer(Mp, 1), (2, W_G, 0.0, 1.0, 0, 1.0, 0.0), 1)
    assert torch.equal(coef[:2 * B].view(B, 2), torch.tensor([[1.0, W_G - 1.0]] * B).cuda())
    F2 = torch.cat([Fc, Fu], 0).contiguous()
    sc = COEFS["history"]
    h0 = torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(8)).cuda()
    h_ref, x_ref, h_out, x_out = h0.clone(), torch.zeros_like(x), h0.clone(), torch.zeros_like(x)
    hip.check(L.md_edm_solver_update(x.data_ptr(), F2.data_ptr(), h_ref.data_ptr(), x_ref.data_ptr(), n, W_G, 1, T_IN, SD, *sc, _st()),
              "md_edm_solver_update")
    hip.check(L.md_edm_solver_update_coef(x.data_ptr(), Fc.data_ptr(), M_buf.data_ptr(), coef.data_ptr(), h_out.data_ptr(), x_out.data_ptr(), B,
                                          n // B, T_IN, SD, *sc, _st()), "md_edm_solver_update_coef")
    d_ref, y_ref, d_out, y_out = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    hip.check(L.md_edm_heun_update(x.data_ptr(), x.data_ptr(), F2.data_ptr(), d_ref.data_ptr(), y_ref.data_ptr(), n, W_G, 1, T_IN, T_IN, 1.2, SD, 0,
                                   _st()), "md_edm_heun_update")
    hip.check(L.md_edm_heun_update_coef(x.data_ptr(), x.data_ptr(), Fc.data_ptr(), M_buf.data_ptr(), coef.data_ptr(), d_out.data_ptr(),
                                        y_out.data_ptr(), B, n // B, T_IN, T_IN, 1.2, SD, 0, _st()), "md_edm_heun_update_coef")
    rels = (_rel(x_out, x_ref), _rel(h_out, h_ref), _rel(y_out, y_ref), _rel(d_out, d_ref))
    print(shape, rels)
    assert max(rels) < 2e-6, rels


def test_guidance_kernels_refuse_bad_arguments_and_write_nothing(hip):
    B, C, H, W = 2, 4, 6, 10
    L, T, pv, n = hip.lib(), 15, 16, 2 * 4 * 6 * 10
    x = torch.randn(B, C, H, W, dtype=torch.float64).cuda()
    tok = torch.randn(2 * B * T, pv).to(torch.bfloat16).cuda()
    F = torch.randn(2 * B, C, H, W).cuda()
    M, coef, mom = torch.full((B, C, H, W), 4.0).cuda(), torch.full((B, 2), 4.5).cuda(), torch.full((B, 5), 4.25, dtype=torch.float64).cuda()
    h, xn = torch.full_like(x, 5.0), torch.full_like(x, 6.0)
    xp, tp, Fp, Mp, cp, mp, hp, np_ = (t.data_ptr() for t in (x, tok, F, M, coef, mom, h, xn))
    good = (2, W_G, 0.0, 0.25, 1, 2.0, -0.5)                                   # mode, w, phi, eta, has_r, r, beta
    geo, st = (B, C, H, W, P), _st()
    # --- prepare: pointers, sizes, t_in
    ptrs = (xp, Fp, Fp, Mp, cp, mp)
    tptrs = (xp, tp, tp, Mp, cp, mp)
    for k in range(6):
        assert L.md_guidance_prepare(*(None if i == k else v for i, v in enumerate(ptrs)), B, n // B, T_IN, SD, *good, 0, st) == -1, k
        assert L.md_guidance_prepare_tok(*(None if i == k else v for i, v in enumerate(tptrs)), *geo, T_IN, SD, *good, 0, st) == -1, k
    for bad in ((0, n // B), (B, 0), (-1, n // B)):
        assert L.md_guidance_prepare(*ptrs, *bad, T_IN, SD, *good, 0, st) == -1, bad
    for bad in ((B, C, 7, W, P), (B, C, H, 9, P), (0, C, H, W, P), (B, 0, H, W, P), (B, C, H, W, 0)):
        assert L.md_guidance_prepare_tok(*tptrs, *bad, T_IN, SD, *good, 0, st) == -1, bad
    for t_in in (0.0, -1.0, NAN):
        assert L.md_guidance_prepare(*ptrs, B, n // B, t_in, SD, *good, 0, st) == -1, t_in
        assert L.md_guidance_prepare_tok(*tptrs, *geo, t_in, SD, *good, 0, st) == -1, t_in
    # --- prepare: the mode and its parameters
    inf = float("inf")
    for bad in ((0,) + good[1:], (3,) + good[1:],                               # an unknown mode ("cfg" has no prepare step)
                (1, W_G, -0.01, 0.0, 0, 1.0, 0.0), (1, W_G, 1.01, 0.0, 0, 1.0, 0.0), (1, W_G, NAN, 0.0, 0, 1.0, 0.0),   # phi outside [0, 1]
                (2, W_G, 0.0, 0.25, 1, 0.0, 0.0), (2, W_G, 0.0, 0.25, 1, -2.0, 0.0), (2, W_G, 0.0, 0.25, 1, inf, 0.0),  # r <= 0, not finite
                (2, W_G, 0.0, 0.25, 1, NAN, 0.0), (2, W_G, 0.0, 0.25, 0, 1.0, 1.0), (2, W_G, 0.0, 0.25, 0, 1.0, -1.0),  # |beta| >= 1
                (2, W_G, 0.0, NAN, 0, 1.0, 0.0), (2, inf, 0.0, 0.25, 0, 1.0, 0.0), (2, NAN, 0.0, 0.25, 0, 1.0, 0.0),
                (2, W_G, 0.0, 0.25, 0, 1.0, NAN)):
        assert L.md_guidance_prepare(*ptrs, B, n // B, T_IN, SD, *bad, 0, st) == -1, bad
        assert L.md_guidance_prepare_tok(*tptrs, *geo, T_IN, SD, *bad, 0, st) == -1, bad
    # --- the update kernels
    stail, htail = (T_IN, SD, 0.5, 0.5, 1.0, 0.0, st), (T_IN, 2.1, 1.2, SD, 0, st)
    sp, stp = (xp, Fp, Mp, cp, hp, np_), (xp, tp, Mp, cp, hp, np_)
    hpt, htp = (xp, xp, Fp, Mp, cp, hp, np_), (xp, xp, tp, Mp, cp, hp, np_)
    for k in range(6):
        assert L.md_edm_solver_update_coef(*(None if i == k else v for i, v in enumerate(sp)), B, n // B, *stail) == -1, k
        assert L.md_edm_solver_update_coef_tok(*(None if i == k else v for i, v in enumerate(stp)), *geo, *stail) == -1, k
    for k in range(7):
        assert L.md_edm_heun_update_coef(*(None if i == k else v for i, v in enumerate(hpt)), B, n // B, *htail) == -1, k
        assert L.md_edm_heun_update_coef_tok(*(None if i == k else v for i, v in enumerate(htp)), *geo, *htail) == -1, k
    for bad in ((0, n // B), (B, 0)):
        assert L.md_edm_solver_update_coef(*sp, *bad, *stail) == -1, bad
        assert L.md_edm_heun_update_coef(*hpt, *bad, *htail) == -1, bad
    for bad in ((B, C, 7, W, P), (B, C, H, 9, P), (0, C, H, W, P), (B, C, H, W, 0)):
        assert L.md_edm_solver_update_coef_tok(*stp, *bad, *stail) == -1, bad
        assert L.md_edm_heun_update_coef_tok(*htp, *bad, *htail) == -1, bad
    for t_in in (0.0, -1.0):
        assert L.md_edm_solver_update_coef(*sp, B, n // B, t_in, *stail[1:]) == -1
        assert L.md_edm_solver_update_coef_tok(*stp, *geo, t_in, *stail[1:]) == -1
        assert L.md_edm_heun_update_coef(*hpt, B, n // B, t_in, *htail[1:]) == -1
        assert L.md_edm_heun_update_coef_tok(*htp, *geo, t_in, *htail[1:]) == -1
    torch.cuda.synchronize()
    assert (M == 4.0).all() and (coef == 4.5).all() and (mom == 4.25).all() and (h == 5.0).all() and (xn == 6.0).all()


# ------------------------------------------------------------------------------------------------ the loops
def _model(cfg, sd=None, seed=None):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    if seed is not None:
        torch.manual_seed(seed)
    d = mdit.DiT(**cfg.__dict__)
    if sd is not None:
        d.load_state_dict(sd)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=cfg.input_size)
    m.eval()
    return m


def _inputs(B=3):
    g = torch.Generator().manual_seed(10)
    return torch.randn(B, 4, 32, 32, generator=g).cuda(), torch.randn(B, 1, 77, 1024, generator=g).cuda()


@pytest.fixture(scope="module")
def smooth_model(hip):
    """The stand-in network of tests/test_samplers_gpu.py, a smooth fp32 function of its inputs in both loops so that nothing amplifies
    round-off, with a caption term that varies over the image: a constant D_c - D_u would leave the standard deviation, and with it CFG
    rescale, where plain guidance has them."""
    model = _model(orc.tiny_config(), seed=11)

    def smooth(x, t, y, mask_ratio=0, **kw):
        x = x.float()
        cond = 20.0 * y.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)     # zeroed captions (the unconditional half) give 0
        return {"sample": torch.tanh(0.7 * x) * (1.0 + 0.1 * t.float().view(-1, 1, 1, 1)) + 0.05 * torch.roll(x, 1, -1)
                + cond * (1.0 + 0.5 * torch.tanh(0.3 * torch.roll(x, 1, -2))), "mask": None}
    model.dit.forward_without_cfg = smooth
    return model


@pytest.fixture(scope="module")
def real_model(hip):
    cfg = orc.tiny_config()
    return _model(cfg, orc.synth_state_dict(cfg, 43))


MODES = {"rescale": dict(guidance_mode="rescale", guidance_rescale=0.7),
         "apg": dict(guidance_mode="apg", apg_eta=0.25, apg_norm_threshold=0.5, apg_momentum=-0.5)}


@pytest.fixture(scope="module")
def smooth_cfg_runs(smooth_model):
    """Plain guidance with the smooth network, once per solver: what every mode must differ from."""
    lat, y = _inputs()
    return {s: smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=s) for s in samplers.SAMPLERS}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("sampler", ["heun", "euler", "dpmpp_2m"])
def test_fused_equals_tensor_op_with_a_smooth_network(smooth_model, smooth_cfg_runs, sampler, mode):
    lat, y = _inputs()
    a = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=sampler, **MODES[mode])
    b = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=False, sampler=sampler, **MODES[mode])
    rel, moved = _rel(a, b), _rel(a, smooth_cfg_runs[sampler])
    print(sampler, mode, rel, "against cfg", moved)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert rel < 2e-6, rel
    # five times the bound above: what the comparison resolves must be smaller than what the mode changes
    assert moved > 1e-5, "the mode must differ from plain guidance"
    if mode == "apg":                               # the threshold is finite in effect: without it the result is another one
        free = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=sampler, **dict(MODES[mode], apg_norm_threshold=None))
        assert _rel(a, free) > 1e-5


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("sampler", ["heun", "dpmpp_2m"])
def test_real_network_fused_equals_tensor_op_and_cached_equals_uncached(real_model, sampler, mode):
    """Through the real bf16 network: 2e-2 for the reason given in test_fused_sampler_equals_tensor_op_sampler; the cached path launches
    the same network kernels on the same operands as the uncached one and the token forms of the guidance kernels give the bits of the
    image forms, so those two are equal bit for bit."""
    lat, y = _inputs()
    kw = dict(steps=5, cfg=3.0, sampler=sampler, **MODES[mode])
    a = real_model.edm_sampler_loop(lat, y, fused=True, cond_cache=False, **kw)
    b = real_model.edm_sampler_loop(lat, y, fused=False, **kw)
    rel = _rel(a, b)
    print(sampler, mode, rel)
    assert torch.isfinite(a).all() and rel < 2e-2, rel
    c = real_model.edm_sampler_loop(lat, y, fused=True, cond_cache=True, **kw)
    assert torch.equal(c, a)
    assert not torch.equal(a, real_model.edm_sampler_loop(lat, y, steps=5, cfg=3.0, sampler=sampler, cond_cache=True))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cond_cache", [False, True])
def test_an_interval_without_a_level_and_cfg_one_run_unguided(real_model, cond_cache, mode):
    lat, y = _inputs(2)
    kw = dict(steps=4, sampler="heun", cond_cache=cond_cache)
    none = real_model.edm_sampler_loop(lat, y, cfg=1.0, **kw)
    assert torch.equal(real_model.edm_sampler_loop(lat, y, cfg=3.0, guidance_interval=(100.0, 200.0), **kw, **MODES[mode]), none)
    assert torch.equal(real_model.edm_sampler_loop(lat, y, cfg=1.0, **kw, **MODES[mode]), none)
    if not cond_cache:
        assert torch.equal(real_model.edm_sampler_loop(lat, y, cfg=3.0, guidance_interval=(100.0, 200.0), fused=False, steps=4, **MODES[mode]),
                           real_model.edm_sampler_loop(lat, y, cfg=1.0, fused=False, steps=4))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("sampler", ["heun", "dpmpp_2m"])
def test_interval_fused_equals_tensor_op_with_a_smooth_network(smooth_model, smooth_cfg_runs, sampler, mode):
    """Part of the evaluations guided: M carries over the unguided ones untouched, in both loops."""
    lat, y = _inputs()
    ec = smooth_model.edm_config
    t = samplers.edm_schedule(6, ec.sigma_min, ec.sigma_max, ec.rho)
    iv = (math.sqrt(t[4] * t[3]), math.sqrt(t[2] * t[1]))      # holds the levels t[2] and t[3]
    a = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=sampler, guidance_interval=iv, **MODES[mode])
    b = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=False, sampler=sampler, guidance_interval=iv, **MODES[mode])
    full = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=sampler, **MODES[mode])
    rel = _rel(a, b)
    print(sampler, mode, rel, "against guided everywhere", _rel(a, full))
    assert rel < 2e-6, rel
    assert _rel(a, full) > 1e-5


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fused", [True, False])
def test_main_with_null_captions_as_guide_is_the_doubled_batch_run(smooth_model, mode, fused):
    """guide = the model's own dit with zeroed captions is the second operand of the doubled batch, as two batch-B evaluations: the same
    mode gives the same result, to the bound tests/test_autoguidance_gpu.py holds the pair to under "cfg"."""
    lat, y = _inputs()
    kw = dict(steps=6, cfg=3.0, sampler="heun", **MODES[mode])
    doubled = smooth_model.edm_sampler_loop(lat, y, fused=True, **kw)
    a = smooth_model.edm_sampler_loop(lat, y, fused=fused, guide=smooth_model.dit, guide_captions="null", **kw)
    rel = _rel(a, doubled)
    print(mode, fused, rel)
    assert rel < 2e-6, rel


@pytest.mark.parametrize("cond_cache", [False, True])
def test_real_guide_network_in_a_mode(real_model, cond_cache):
    lat, y = _inputs(2)
    kw = dict(steps=4, cfg=3.0, sampler="heun", guide=real_model.dit, guide_captions="null", **MODES["apg"])
    a = real_model.edm_sampler_loop(lat, y, cond_cache=cond_cache, **kw)
    doubled = real_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, sampler="heun", cond_cache=cond_cache, **MODES["apg"])
    rel = _rel(a, doubled)
    print(cond_cache, rel)
    assert torch.isfinite(a).all() and rel < 2e-2, rel


def test_inpainting_in_apg_returns_the_kept_region_bit_for_bit(real_model):
    lat, y = _inputs(2)
    g = torch.Generator().manual_seed(12)
    init = torch.randn(2, 4, 32, 32, generator=g).cuda()
    hole = torch.zeros(1, 1, 32, 32, device="cuda")
    hole[..., 8:24, 4:20] = 1.0
    torch.manual_seed(24)
    a = real_model.edm_sampler_loop(lat, y, steps=4, cfg=3.0, cond_cache=True, init_latents=init, inpaint_mask=hole, **MODES["apg"])
    keep = (hole == 0).expand(a.shape)
    assert torch.isfinite(a).all() and torch.equal(a[keep], init[keep]) and not torch.equal(a[~keep], init[~keep])


@pytest.mark.parametrize("cond_cache", [False, True])
def test_default_mode_is_unchanged(real_model, cond_cache):
    lat, y = _inputs()
    kw = dict(steps=4, cfg=3.0, cond_cache=cond_cache)
    plain = real_model.edm_sampler_loop(lat, y, **kw)
    assert torch.equal(real_model.edm_sampler_loop(lat, y, guidance_mode="cfg", **kw), plain)
    assert torch.equal(real_model.edm_sampler_loop(lat, y, guidance_mode="cfg", guidance_rescale=0.0, apg_eta=0.0, apg_norm_threshold=None,
                                                   apg_momentum=0.0, **kw), plain)
