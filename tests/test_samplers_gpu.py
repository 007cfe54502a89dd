"""Sampler solvers on the GPU: md_edm_solver_update against the formula in torch fp64, its token-space form against
md_unpatchify + the image-space form (torch.equal), md_edm_churn, and the three solvers, the churn and the guidance interval through
edm_sampler_loop: fused against the tensor-op loop (2e-6 with a smooth stand-in network, 2e-2 through the real bf16 network: the bounds
and the reasons of tests/test_sampler_ckpt_gpu.py), cached against uncached (torch.equal where the same launches run)."""
import math

import pytest
import torch

from micro_diffusion_amd import samplers, sampling
from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu

P = 2
SD = 0.9                      # sigma_data
INF = float("inf")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


# ------------------------------------------------------------------------------------------------ the update kernel
COEFS = {"no_history": (0.625, 0.375, 1.0, 0.0),               # an Euler step / the first 2M step
         "history": (0.625, 0.46, 1.4, 0.4),                   # a 2M step
         "last": (0.0, 1.0, 1.0, 0.0)}                         # the step onto sigma = 0


def _torch_update(x, F, hist, cfg, has_uncond, t_in, coef):
    """The formula of the header in torch: fp32 guidance combine and preconditioning (dit.py:542-550, model.py:144-179), fp64 update."""
    a, b, c1, c2 = coef
    B = x.shape[0]
    f = F[B:] + cfg * (F[:B] - F[B:]) if has_uncond else F
    sigma = torch.tensor(t_in, dtype=torch.float64, device=x.device).to(torch.float32)
    c_skip = SD ** 2 / (sigma ** 2 + SD ** 2)
    c_out = sigma * SD / (sigma ** 2 + SD ** 2).sqrt()
    den = (c_skip * x.to(torch.float32) + c_out * f).to(torch.float64)
    return a * x + b * (c1 * den - c2 * hist if c2 != 0 else c1 * den), den


@pytest.mark.parametrize("mode", list(COEFS))
@pytest.mark.parametrize("has_uncond", [0, 1])
@pytest.mark.parametrize("shape", [(2, 4, 6, 10), (3, 4, 32, 32)])
def test_solver_update_against_torch_fp64(hip, shape, has_uncond, mode):
    B, C, H, W = shape
    L, n, coef = hip.lib(), B * C * H * W, COEFS[mode]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).cuda() * 3
    F = torch.randn(B * (2 if has_uncond else 1), C, H, W, generator=g).cuda()
    hist0 = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).cuda()
    cfg, t_in = 3.0, 1.7
    want_x, want_den = _torch_update(x, F, hist0, cfg, has_uncond, t_in, coef)
    hist = hist0.clone() if coef[3] != 0 else torch.full_like(hist0, float("nan"))      # unread history must not reach x_next
    out = torch.full((n + 1,), 7.0, device="cuda", dtype=torch.float64)                 # one guard element behind the output
    hip.check(L.md_edm_solver_update(x.data_ptr(), F.data_ptr(), hist.data_ptr(), out.data_ptr(), n, cfg, has_uncond, t_in, SD, *coef, _st()),
              "md_edm_solver_update")
    got = out[:n].view(B, C, H, W)
    assert torch.isfinite(got).all() and torch.isfinite(hist).all()
    rx, rh = _rel(got, want_x), _rel(hist, want_den)
    print(shape, has_uncond, mode, "x_next", rx, "hist", rh)
    assert rx < 2e-6 and rh < 2e-6, (rx, rh)
    assert out[n] == 7.0, "wrote behind the last element"
    if mode == "last":
        assert torch.equal(got, hist), "a = 0, b = 1: the step returns the denoised value itself"
    # x_next may alias x_in
    x2, h2 = x.clone(), (hist0.clone() if coef[3] != 0 else torch.full_like(hist0, float("nan")))
    hip.check(L.md_edm_solver_update(x2.data_ptr(), F.data_ptr(), h2.data_ptr(), x2.data_ptr(), n, cfg, has_uncond, t_in, SD, *coef, _st()),
              "md_edm_solver_update")
    assert torch.equal(x2, got) and torch.equal(h2, hist)


TOK_SHAPES = [(3, 4, 6, 10),      # patch_vec 16, 720 elements: no multiple of 256
              (2, 16, 8, 8),      # the 16-channel VAE: patch_vec 64
              (2, 3, 6, 10)]      # patch_vec 12: no multiple of 8, the element-wise form


@pytest.mark.parametrize("mode", list(COEFS))
@pytest.mark.parametrize("has_uncond", [0, 1])
@pytest.mark.parametrize("shape", TOK_SHAPES)
def test_solver_update_tok_equals_unpatchify_then_solver_update(hip, shape, has_uncond, mode):
    B, C, H, W = shape
    L, T, pv, n, coef = hip.lib(), (H // P) * (W // P), C * P * P, B * C * H * W, COEFS[mode]
    Bn = B * (2 if has_uncond else 1)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).cuda() * 3
    h0 = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).cuda()
    tok = torch.randn(Bn * T, pv, generator=g).to(torch.bfloat16).cuda()
    cfg, t_in = 3.0, 1.7
    img = torch.empty(Bn, C, H, W, device="cuda")
    hip.check(L.md_unpatchify(tok.data_ptr(), None, T, None, img.data_ptr(), Bn, C, H, W, P, _st()), "md_unpatchify")
    h_ref, x_ref = h0.clone(), torch.zeros_like(x)
    hip.check(L.md_edm_solver_update(x.data_ptr(), img.data_ptr(), h_ref.data_ptr(), x_ref.data_ptr(), n, cfg, has_uncond, t_in, SD, *coef,
                                     _st()), "md_edm_solver_update")
    h_out, x_out = h0.clone(), torch.zeros_like(x)
    hip.check(L.md_edm_solver_update_tok(x.data_ptr(), tok.data_ptr(), h_out.data_ptr(), x_out.data_ptr(), B, C, H, W, P, cfg, has_uncond,
                                         t_in, SD, *coef, _st()), "md_edm_solver_update_tok")
    assert torch.equal(x_out, x_ref) and torch.equal(h_out, h_ref)
    assert not torch.equal(h_ref, h0) and x_ref.abs().max() > 0                        # the history is always written
    # the sampler's aliasing is allowed too: x_next == x_in
    a_out, ha = x.clone(), h0.clone()
    hip.check(L.md_edm_solver_update_tok(a_out.data_ptr(), tok.data_ptr(), ha.data_ptr(), a_out.data_ptr(), B, C, H, W, P, cfg, has_uncond,
                                         t_in, SD, *coef, _st()), "md_edm_solver_update_tok")
    assert torch.equal(a_out, x_ref) and torch.equal(ha, h_ref)


def test_solver_kernels_refuse_bad_arguments_and_write_nothing(hip):
    B, C, H, W = 2, 4, 6, 10
    L, T, pv, n = hip.lib(), 15, 16, 2 * 4 * 6 * 10
    x = torch.randn(B, C, H, W, dtype=torch.float64).cuda()
    tok = torch.randn(B * T, pv).to(torch.bfloat16).cuda()
    F = torch.randn(B, C, H, W).cuda()
    h, xn = torch.full_like(x, 5.0), torch.full_like(x, 6.0)
    tail = (3.0, 0, 1.7, SD, 0.5, 0.5, 1.0, 0.0, _st())
    args = (B, C, H, W, P) + tail
    assert L.md_edm_solver_update_tok(None, tok.data_ptr(), h.data_ptr(), xn.data_ptr(), *args) == -1
    assert L.md_edm_solver_update_tok(x.data_ptr(), None, h.data_ptr(), xn.data_ptr(), *args) == -1
    assert L.md_edm_solver_update_tok(x.data_ptr(), tok.data_ptr(), None, xn.data_ptr(), *args) == -1
    assert L.md_edm_solver_update_tok(x.data_ptr(), tok.data_ptr(), h.data_ptr(), None, *args) == -1
    for bad in ((B, C, 7, W, P), (B, C, H, 9, P), (0, C, H, W, P), (B, C, H, W, 0)):
        assert L.md_edm_solver_update_tok(x.data_ptr(), tok.data_ptr(), h.data_ptr(), xn.data_ptr(), *(bad + tail)) == -1
    zero_sigma = (B, C, H, W, P, 3.0, 0, 0.0) + tail[3:]
    assert L.md_edm_solver_update_tok(x.data_ptr(), tok.data_ptr(), h.data_ptr(), xn.data_ptr(), *zero_sigma) == -1
    assert L.md_edm_solver_update(None, F.data_ptr(), h.data_ptr(), xn.data_ptr(), n, *tail) == -1
    assert L.md_edm_solver_update(x.data_ptr(), None, h.data_ptr(), xn.data_ptr(), n, *tail) == -1
    assert L.md_edm_solver_update(x.data_ptr(), F.data_ptr(), None, xn.data_ptr(), n, *tail) == -1
    assert L.md_edm_solver_update(x.data_ptr(), F.data_ptr(), h.data_ptr(), None, n, *tail) == -1
    assert L.md_edm_solver_update(x.data_ptr(), F.data_ptr(), h.data_ptr(), xn.data_ptr(), 0, *tail) == -1
    assert L.md_edm_churn(None, x.data_ptr(), xn.data_ptr(), n, 0.5, _st()) == -1
    assert L.md_edm_churn(x.data_ptr(), None, xn.data_ptr(), n, 0.5, _st()) == -1
    assert L.md_edm_churn(x.data_ptr(), x.data_ptr(), None, n, 0.5, _st()) == -1
    assert L.md_edm_churn(x.data_ptr(), x.data_ptr(), xn.data_ptr(), 0, 0.5, _st()) == -1
    torch.cuda.synchronize()
    assert (h == 5.0).all() and (xn == 6.0).all()


# ------------------------------------------------------------------------------------------------ churn
@pytest.mark.parametrize("shape", [(3, 4, 6, 10), (3, 4, 32, 32)])
def test_churn_is_one_fp64_fma(hip, shape):
    L, n = hip.lib(), math.prod(shape)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 80).cuda()
    # (1) noise and coefficient with 24-bit significands: the fp64 product is exact, so x + coef * noise rounds once however torch
    # evaluates it, and equals the fma bit for bit
    noise = torch.randn(shape, generator=g).to(torch.float64).cuda()
    coef = float(torch.tensor(math.sqrt(33.0 ** 2 - 24.0 ** 2) * 1.003, dtype=torch.float32))
    want = torch.addcmul(x, noise, torch.full_like(x, coef))
    out = torch.full((n + 1,), 7.0, device="cuda", dtype=torch.float64)
    hip.check(L.md_edm_churn(x.data_ptr(), noise.data_ptr(), out.data_ptr(), n, coef, _st()), "md_edm_churn")
    assert torch.equal(out[:n].view(shape), want) and out[n] == 7.0
    assert not torch.equal(want, x)
    xa = x.clone()                                                                      # in place, as the sampler calls it
    hip.check(L.md_edm_churn(xa.data_ptr(), noise.data_ptr(), xa.data_ptr(), n, coef, _st()), "md_edm_churn")
    assert torch.equal(xa, want)
    # (2) full 53-bit operands: fma and multiply-then-add differ by the rounding of the product at most
    noise = torch.randn(shape, generator=g, dtype=torch.float64).cuda()
    coef = math.sqrt(33.0 ** 2 - 24.0 ** 2) * 1.003
    hip.check(L.md_edm_churn(x.data_ptr(), noise.data_ptr(), out.data_ptr(), n, coef, _st()), "md_edm_churn")
    prod = coef * noise
    assert ((out[:n].view(shape) - (x + prod)).abs() <= 2.0 ** -52 * (x.abs() + prod.abs())).all()


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
    """The stand-in network of test_fused_sampler_arithmetic_exact_with_a_smooth_network: a smooth fp32 function of its inputs in both
    loops, so nothing amplifies round-off."""
    model = _model(orc.tiny_config(), seed=11)

    def smooth(x, t, y, mask_ratio=0, **kw):
        x = x.float()
        cond = y.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)            # zeroed captions (the unconditional half) give 0
        return {"sample": torch.tanh(0.7 * x) * (1.0 + 0.1 * t.float().view(-1, 1, 1, 1)) + 0.05 * torch.roll(x, 1, -1) + cond, "mask": None}
    model.dit.forward_without_cfg = smooth
    return model


@pytest.fixture(scope="module")
def real_model(hip):
    cfg = orc.tiny_config()
    return _model(cfg, orc.synth_state_dict(cfg, 43))


def _middle_third(model, steps):
    """(sigma_lo, sigma_hi) that holds exactly the middle third of the schedule's noise levels, the ends between two levels."""
    ec = model.edm_config
    t = samplers.edm_schedule(steps, ec.sigma_min, ec.sigma_max, ec.rho)
    k = steps // 3
    return math.sqrt(t[steps - k] * t[steps - k - 1]), math.sqrt(t[k] * t[k - 1])


@pytest.mark.parametrize("guidance", [1.0, 3.0])
@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
def test_fused_solver_arithmetic_exact_with_a_smooth_network(smooth_model, sampler, guidance):
    lat, y = _inputs()
    a = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=guidance, fused=True, sampler=sampler)
    b = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=guidance, fused=False, sampler=sampler)
    h = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=guidance, fused=False)
    rel = _rel(a, b)
    print(sampler, guidance, rel, "against heun", _rel(b, h))
    assert rel < 2e-6, rel
    assert torch.isfinite(b).all() and not torch.equal(b, h), "another solver: finite, and not the Heun loop under another name"


@pytest.mark.parametrize("guidance", [1.0, 3.0])
@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
def test_fused_solver_equals_tensor_op_solver_and_cached_equals_uncached(real_model, sampler, guidance):
    """Through the real bf16 network: 2e-2 for the reason given in test_fused_sampler_equals_tensor_op_sampler; the cached path launches
    the same network kernels on the same operands as the uncached one, so those two are equal bit for bit."""
    lat, y = _inputs()
    a = real_model.edm_sampler_loop(lat, y, steps=5, cfg=guidance, fused=True, sampler=sampler, cond_cache=False)
    b = real_model.edm_sampler_loop(lat, y, steps=5, cfg=guidance, fused=False, sampler=sampler)
    rel = _rel(a, b)
    print(sampler, guidance, rel)
    assert rel < 2e-2, rel
    c = real_model.edm_sampler_loop(lat, y, steps=5, cfg=guidance, fused=True, sampler=sampler, cond_cache=True)
    assert torch.equal(c, a)


@pytest.mark.parametrize("sampler", ["heun", "euler"])
def test_churn_runs_on_the_fused_loop(smooth_model, sampler):
    """S_churn > 0 with S_min / S_max such that some steps churn and some do not; both loops draw once per step from the same generator."""
    lat, y = _inputs()
    ec = smooth_model.edm_config
    t = samplers.edm_schedule(6, ec.sigma_min, ec.sigma_max, ec.rho)
    saved = dict(ec)
    try:
        plain = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=sampler)
        ec.update(S_churn=20, S_noise=1.003, S_min=math.sqrt(t[4] * t[5]), S_max=math.sqrt(t[0] * t[1]))
        hats = sampling.churned_levels(ec, t, 6)
        assert [h > s for h, s in zip(hats, t)] == [False, True, True, True, True, False]
        torch.manual_seed(21)
        a = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=sampler)
        torch.manual_seed(21)
        b = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=False, sampler=sampler)
        with pytest.raises(ValueError, match="S_churn"):
            smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, sampler="dpmpp_2m")
    finally:
        ec.update(saved)
    rel = _rel(a, b)
    print(sampler, rel, "churn moved the sample by", _rel(a, plain))
    assert rel < 2e-6, rel
    assert _rel(a, plain) > 1e-3, "the churn must have changed the sample"


# ------------------------------------------------------------------------------------------------ the guidance interval
@pytest.mark.parametrize("cond_cache", [False, True])
@pytest.mark.parametrize("sampler", ["heun", "dpmpp_2m"])
def test_interval_limits(real_model, sampler, cond_cache):
    lat, y = _inputs(2)
    kw = dict(steps=4, sampler=sampler, cond_cache=cond_cache)
    full = real_model.edm_sampler_loop(lat, y, cfg=3.0, **kw)
    assert torch.equal(real_model.edm_sampler_loop(lat, y, cfg=3.0, guidance_interval=(0, INF), **kw), full)
    none = real_model.edm_sampler_loop(lat, y, cfg=1.0, **kw)
    assert torch.equal(real_model.edm_sampler_loop(lat, y, cfg=3.0, guidance_interval=(100.0, 200.0), **kw), none)
    assert not torch.equal(full, none)


@pytest.mark.parametrize("sampler", ["heun", "euler", "dpmpp_2m"])
def test_interval_fused_equals_tensor_op_with_a_smooth_network(smooth_model, sampler):
    lat, y = _inputs()
    iv = _middle_third(smooth_model, 6)
    a = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=sampler, guidance_interval=iv)
    b = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=False, sampler=sampler, guidance_interval=iv)
    rel = _rel(a, b)
    full = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, fused=True, sampler=sampler)
    none = smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=1.0, fused=True, sampler=sampler)
    print(sampler, rel, "against guided everywhere", _rel(a, full), "against unguided", _rel(a, none))
    assert rel < 2e-6, rel
    # five times the bound above: what the comparison resolves must be smaller than what the interval changes
    assert _rel(a, full) > 1e-5 and _rel(a, none) > 1e-5, "the interval must differ from guidance everywhere and from none"


@pytest.mark.parametrize("sampler", ["heun", "dpmpp_2m"])
def test_interval_cached_equals_uncached_through_the_network(real_model, sampler):
    """No bit-equality here: a batch-B launch may tile differently from the first half of a batch-2B launch, and the cache is encoded
    once for 2B while the uncached path encodes B captions in the unguided evaluations."""
    lat, y = _inputs()
    iv = _middle_third(real_model, 6)
    a = real_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, sampler=sampler, guidance_interval=iv, cond_cache=True)
    b = real_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, sampler=sampler, guidance_interval=iv, cond_cache=False)
    rel = _rel(a, b)
    print(sampler, rel)
    assert rel < 2e-2, rel


@pytest.mark.parametrize("cond_cache", [False, True])
@pytest.mark.parametrize("sampler", ["heun", "dpmpp_2m"])
def test_out_of_interval_evaluations_run_at_batch_b(real_model, sampler, cond_cache):
    """The rows of the timestep MLP's first GEMM are the network batch of an evaluation (one launch per evaluation)."""
    lat, y = _inputs(2)
    eng = real_model.dit.engine
    iv = _middle_third(real_model, 6)
    ec = real_model.edm_config
    levels = samplers.evaluation_sigmas(sampler, samplers.edm_schedule(6, ec.sigma_min, ec.sigma_max, ec.rho))
    want = [4 if iv[0] <= s <= iv[1] else 2 for s in levels]
    assert len(want) == (11 if sampler == "heun" else 6) and 2 in want and 4 in want
    rows, orig = [], eng.lin_fwd

    def spy(x_, wname, out, M, *a, **k):
        if wname == "t_embedder.mlp.0":
            rows.append(M)
        return orig(x_, wname, out, M, *a, **k)
    eng.lin_fwd = spy
    try:
        real_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, sampler=sampler, guidance_interval=iv, cond_cache=cond_cache)
        got = list(rows)
        del rows[:]
        real_model.edm_sampler_loop(lat, y, steps=6, cfg=3.0, sampler=sampler, cond_cache=cond_cache)
        everywhere = list(rows)
    finally:
        del eng.lin_fwd
    assert got == want, (got, want)
    assert everywhere == [4] * len(want)


def test_narrowed_conditioning_is_checked_like_any_other(real_model):
    lat, y = _inputs(2)
    dit = real_model.dit
    cond = dit.encode_condition(torch.cat([y, torch.zeros_like(y)], 0))
    half = cond.narrow(2)
    assert half.B == 2 and half.version == cond.version and half.nbytes * 2 == cond.nbytes
    assert all(h[0].data_ptr() == c[0].data_ptr() for h, c in zip(half.kv.values(), cond.kv.values())), "views, no copy"
    t = torch.tensor([0.1], device="cuda")
    eng = dit.engine
    eng.forward(lat, t, None, cond=half)
    with pytest.raises(RuntimeError, match="batch"):
        eng.forward(lat, t, None, cond=cond)
    with pytest.raises(RuntimeError, match="batch"):
        eng.forward(torch.cat([lat, lat], 0), t, None, cond=half)


# ------------------------------------------------------------------------------------------------ the default
@pytest.mark.parametrize("cond_cache", [False, True])
def test_default_sampler_is_unchanged(real_model, cond_cache):
    lat, y = _inputs(2)
    a = real_model.edm_sampler_loop(lat, y, steps=4, cfg=4.0, cond_cache=cond_cache)
    b = real_model.edm_sampler_loop(lat, y, steps=4, cfg=4.0, cond_cache=cond_cache, sampler="heun", guidance_interval=None)
    assert torch.equal(a, b)
    assert real_model.edm_config.S_churn == 0
