"""Autoguidance on the GPU.  Kernel level: each of the four two-pointer update entry points against its existing
counterpart run with has_uncond = 1 on the concatenated buffer (torch.equal on every output buffer), misaligned token pointers, and the
refusals.  Loop level: edm_sampler_loop(guide=...) fused against the tensor-op loop (2e-6 with smooth stand-in networks, 2e-2 through the
real bf16 networks: the bounds and the reasons of tests/test_samplers_gpu.py), cached against uncached, the two degenerate guides
(main itself with the same captions: the unguided run; main itself with zeroed captions: classifier-free guidance), what is evaluated
at which batch, and churn."""
import math

import pytest
import torch

from micro_diffusion_amd import samplers
from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu

P = 2
SD = 0.9                      # sigma_data
W_AUTO = 2.5                  # the autoguidance weight of the kernel tests
SOLVERS = ["heun", "euler", "dpmpp_2m"]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


# ------------------------------------------------------------------------------------------------ the kernels: bit equality
COEFS = {"no_history": (0.625, 0.375, 1.0, 0.0),               # c2 = 0: an Euler step / the first 2M step
         "history": (0.625, 0.46, 1.4, 0.4)}                   # c2 != 0: a 2M step
T_IN, T_HAT, T_NEXT = 1.7, 1.9, 1.1


def _state(shape, seed):
    """x_hat, x_in, d_cur / hist (fp64) of one update."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(shape, generator=g, dtype=torch.float64) * 3).cuda() for _ in range(3)]


def _heun_pair(L, n, x_hat, x_in, d0, F, Fg, second):
    """(x_next, d_cur) of md_edm_heun_update(has_uncond = 1) on [F; Fg] and of md_edm_heun_update_guide on the two buffers."""
    cat = torch.cat([F.reshape(-1), Fg.reshape(-1)])
    d_ref, x_ref = d0.clone(), torch.zeros_like(x_in)
    assert L.md_edm_heun_update(x_hat.data_ptr(), x_in.data_ptr(), cat.data_ptr(), d_ref.data_ptr(), x_ref.data_ptr(), n, W_AUTO, 1, T_IN,
                                T_HAT, T_NEXT, SD, second, _st()) == 0
    d_out, x_out = d0.clone(), torch.zeros_like(x_in)
    assert L.md_edm_heun_update_guide(x_hat.data_ptr(), x_in.data_ptr(), F.data_ptr(), Fg.data_ptr(), d_out.data_ptr(), x_out.data_ptr(), n,
                                      W_AUTO, T_IN, T_HAT, T_NEXT, SD, second, _st()) == 0
    return (x_ref, d_ref), (x_out, d_out)


@pytest.mark.parametrize("second", [0, 1])
@pytest.mark.parametrize("shape", [(240,), (3, 4, 32, 32)])
def test_heun_update_guide_equals_has_uncond_on_the_concatenation(hip, shape, second):
    L, n = hip.lib(), math.prod(shape)
    x_hat, x_in, d0 = _state(shape, 3)
    g = torch.Generator().manual_seed(4)
    F, Fg = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    (x_ref, d_ref), (x_out, d_out) = _heun_pair(L, n, x_hat, x_in, d0, F, Fg, second)
    assert torch.equal(x_out, x_ref) and torch.equal(d_out, d_ref)
    assert x_ref.abs().max() > 0 and torch.equal(d_ref, d0) == bool(second)           # the first half-step writes d_cur, the second reads it
    # the guide moved the result, and the two read-only outputs may alias each other: F as its own guide is the plain update
    (x_plain, _), (x_self, _) = _heun_pair(L, n, x_hat, x_in, d0, F, F, second)
    assert torch.equal(x_self, x_plain) and not torch.equal(x_self, x_out)
    # x_next may alias x_in (the second half-step of the sampler) or x_hat
    xa, da = x_in.clone(), d0.clone()
    assert L.md_edm_heun_update_guide(x_hat.data_ptr(), xa.data_ptr(), F.data_ptr(), Fg.data_ptr(), da.data_ptr(), xa.data_ptr(), n, W_AUTO,
                                      T_IN, T_HAT, T_NEXT, SD, second, _st()) == 0
    assert torch.equal(xa, x_ref) and torch.equal(da, d_ref)


@pytest.mark.parametrize("mode", list(COEFS))
@pytest.mark.parametrize("shape", [(240,), (3, 4, 32, 32)])
def test_solver_update_guide_equals_has_uncond_on_the_concatenation(hip, shape, mode):
    L, n, coef = hip.lib(), math.prod(shape), COEFS[mode]
    _, x_in, h0 = _state(shape, 5)
    g = torch.Generator().manual_seed(6)
    F, Fg = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    cat = torch.cat([F.reshape(-1), Fg.reshape(-1)])
    h_ref, x_ref = h0.clone(), torch.zeros_like(x_in)
    assert L.md_edm_solver_update(x_in.data_ptr(), cat.data_ptr(), h_ref.data_ptr(), x_ref.data_ptr(), n, W_AUTO, 1, T_IN, SD, *coef, _st()) == 0
    h_out, x_out = h0.clone(), torch.zeros_like(x_in)
    assert L.md_edm_solver_update_guide(x_in.data_ptr(), F.data_ptr(), Fg.data_ptr(), h_out.data_ptr(), x_out.data_ptr(), n, W_AUTO, T_IN, SD,
                                        *coef, _st()) == 0
    assert torch.equal(x_out, x_ref) and torch.equal(h_out, h_ref)
    assert x_ref.abs().max() > 0 and not torch.equal(h_ref, h0)                        # the history is always written
    xa, ha = x_in.clone(), h0.clone()                                                  # the sampler's aliasing: x_next == x_in
    assert L.md_edm_solver_update_guide(xa.data_ptr(), F.data_ptr(), Fg.data_ptr(), ha.data_ptr(), xa.data_ptr(), n, W_AUTO, T_IN, SD, *coef,
                                        _st()) == 0
    assert torch.equal(xa, x_ref) and torch.equal(ha, h_ref)


TOK_SHAPES = [(3, 4, 32, 32),     # patch_vec 16: the 16-byte vector path
              (2, 3, 8, 12)]      # patch_vec 12: no multiple of 8, the element path


def _tokens(shape, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    rows, pv = B * (H // P) * (W // P), C * P * P
    return torch.randn(rows, pv, generator=g).to(torch.bfloat16).cuda(), torch.randn(rows, pv, generator=g).to(torch.bfloat16).cuda()


def _heun_tok_guide(L, shape, x_hat, x_in, d0, tok, tok_g, second):
    d, x = d0.clone(), torch.zeros_like(x_in)
    assert L.md_edm_heun_update_guide_tok(x_hat.data_ptr(), x_in.data_ptr(), tok.data_ptr(), tok_g.data_ptr(), d.data_ptr(), x.data_ptr(),
                                          *shape, P, W_AUTO, T_IN, T_HAT, T_NEXT, SD, second, _st()) == 0
    return x, d


def _solver_tok_guide(L, shape, x_in, h0, tok, tok_g, coef):
    h, x = h0.clone(), torch.zeros_like(x_in)
    assert L.md_edm_solver_update_guide_tok(x_in.data_ptr(), tok.data_ptr(), tok_g.data_ptr(), h.data_ptr(), x.data_ptr(), *shape, P, W_AUTO,
                                            T_IN, SD, *coef, _st()) == 0
    return x, h


@pytest.mark.parametrize("second", [0, 1])
@pytest.mark.parametrize("shape", TOK_SHAPES)
def test_heun_update_guide_tok_equals_has_uncond_on_the_concatenation(hip, shape, second):
    L = hip.lib()
    x_hat, x_in, d0 = _state(shape, 7)
    tok, tok_g = _tokens(shape, 8)
    cat = torch.cat([tok, tok_g], 0).contiguous()
    d_ref, x_ref = d0.clone(), torch.zeros_like(x_in)
    assert L.md_edm_heun_update_tok(x_hat.data_ptr(), x_in.data_ptr(), cat.data_ptr(), d_ref.data_ptr(), x_ref.data_ptr(), *shape, P, W_AUTO,
                                    1, T_IN, T_HAT, T_NEXT, SD, second, _st()) == 0
    x_out, d_out = _heun_tok_guide(L, shape, x_hat, x_in, d0, tok, tok_g, second)
    assert torch.equal(x_out, x_ref) and torch.equal(d_out, d_ref)
    assert x_ref.abs().max() > 0 and torch.equal(d_ref, d0) == bool(second)
    x_self, _ = _heun_tok_guide(L, shape, x_hat, x_in, d0, tok, tok, second)            # aliased read-only operands
    assert not torch.equal(x_self, x_out)
    xa, da = x_in.clone(), d0.clone()
    assert L.md_edm_heun_update_guide_tok(x_hat.data_ptr(), xa.data_ptr(), tok.data_ptr(), tok_g.data_ptr(), da.data_ptr(), xa.data_ptr(),
                                          *shape, P, W_AUTO, T_IN, T_HAT, T_NEXT, SD, second, _st()) == 0
    assert torch.equal(xa, x_ref) and torch.equal(da, d_ref)


@pytest.mark.parametrize("mode", list(COEFS))
@pytest.mark.parametrize("shape", TOK_SHAPES)
def test_solver_update_guide_tok_equals_has_uncond_on_the_concatenation(hip, shape, mode):
    L, coef = hip.lib(), COEFS[mode]
    _, x_in, h0 = _state(shape, 9)
    tok, tok_g = _tokens(shape, 10)
    cat = torch.cat([tok, tok_g], 0).contiguous()
    h_ref, x_ref = h0.clone(), torch.zeros_like(x_in)
    assert L.md_edm_solver_update_tok(x_in.data_ptr(), cat.data_ptr(), h_ref.data_ptr(), x_ref.data_ptr(), *shape, P, W_AUTO, 1, T_IN, SD,
                                      *coef, _st()) == 0
    x_out, h_out = _solver_tok_guide(L, shape, x_in, h0, tok, tok_g, coef)
    assert torch.equal(x_out, x_ref) and torch.equal(h_out, h_ref)
    assert x_ref.abs().max() > 0 and not torch.equal(h_ref, h0)
    xa, ha = x_in.clone(), h0.clone()
    assert L.md_edm_solver_update_guide_tok(xa.data_ptr(), tok.data_ptr(), tok_g.data_ptr(), ha.data_ptr(), xa.data_ptr(), *shape, P, W_AUTO,
                                            T_IN, SD, *coef, _st()) == 0
    assert torch.equal(xa, x_ref) and torch.equal(ha, h_ref)


# ------------------------------------------------------------------------------------------------ the kernels: alignment
def _shifted(t, off=4):
    """The same rows at an address `off` bf16 elements (8 bytes) behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


@pytest.mark.parametrize("which", ["guide_misaligned", "main_misaligned", "both_misaligned"])
def test_a_misaligned_token_pointer_takes_the_element_path(hip, which):
    """The one way two pointers can go wrong that one pointer cannot: the 16-byte path needs both aligned.  A vector load from an address
    that is 8 modulo 16 would fault or read the wrong rows; the element path gives the aligned result bit for bit."""
    L, shape = hip.lib(), TOK_SHAPES[0]
    x_hat, x_in, d0 = _state(shape, 11)
    tok, tok_g = _tokens(shape, 12)
    assert tok.data_ptr() % 16 == 0 and tok_g.data_ptr() % 16 == 0
    tok_s = _shifted(tok) if which != "guide_misaligned" else tok
    tok_gs = _shifted(tok_g) if which != "main_misaligned" else tok_g
    for second in (0, 1):
        want = _heun_tok_guide(L, shape, x_hat, x_in, d0, tok, tok_g, second)
        got = _heun_tok_guide(L, shape, x_hat, x_in, d0, tok_s, tok_gs, second)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ("heun", second)
    for mode, coef in COEFS.items():
        want = _solver_tok_guide(L, shape, x_in, d0, tok, tok_g, coef)
        got = _solver_tok_guide(L, shape, x_in, d0, tok_s, tok_gs, coef)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ("solver", mode)


# ------------------------------------------------------------------------------------------------ the kernels: refusals
def test_guide_kernels_refuse_bad_arguments_and_write_nothing(hip):
    B, C, H, W = 2, 4, 6, 10
    L, T, pv, n = hip.lib(), 15, 16, 2 * 4 * 6 * 10
    x = torch.randn(B, C, H, W, dtype=torch.float64).cuda()
    tok = torch.randn(B * T, pv).to(torch.bfloat16).cuda()
    F = torch.randn(B, C, H, W).cuda()
    h, xn = torch.full_like(x, 5.0), torch.full_like(x, 6.0)
    xp, tp, Fp, hp, np_ = x.data_ptr(), tok.data_ptr(), F.data_ptr(), h.data_ptr(), xn.data_ptr()
    geo = (B, C, H, W, P)
    bad_geo = ((B, C, 7, W, P), (B, C, H, 9, P), (0, C, H, W, P), (B, 0, H, W, P), (B, C, H, W, 0))

    # solver forms: (x_in, F, F_guide, hist, x_next)
    stail = (3.0, 1.7, SD, 0.5, 0.5, 1.0, 0.0, _st())
    for k in range(5):
        ptrs = [xp, tp, tp, hp, np_]
        ptrs[k] = None
        assert L.md_edm_solver_update_guide_tok(*ptrs, *geo, *stail) == -1, k
        ptrs = [xp, Fp, Fp, hp, np_]
        ptrs[k] = None
        assert L.md_edm_solver_update_guide(*ptrs, n, *stail) == -1, k
    for g in bad_geo:
        assert L.md_edm_solver_update_guide_tok(xp, tp, tp, hp, np_, *g, *stail) == -1, g
    for t_in in (0.0, -1.0):
        zs = (3.0, t_in) + stail[2:]
        assert L.md_edm_solver_update_guide_tok(xp, tp, tp, hp, np_, *geo, *zs) == -1
        assert L.md_edm_solver_update_guide(xp, Fp, Fp, hp, np_, n, *zs) == -1
    for bad_n in (0, -4):
        assert L.md_edm_solver_update_guide(xp, Fp, Fp, hp, np_, bad_n, *stail) == -1

    # heun forms: (x_hat, x_in, F, F_guide, d_cur, x_next)
    htail = (3.0, 1.7, 1.9, 1.1, SD, 0, _st())
    for k in range(6):
        ptrs = [xp, xp, tp, tp, hp, np_]
        ptrs[k] = None
        assert L.md_edm_heun_update_guide_tok(*ptrs, *geo, *htail) == -1, k
        ptrs = [xp, xp, Fp, Fp, hp, np_]
        ptrs[k] = None
        assert L.md_edm_heun_update_guide(*ptrs, n, *htail) == -1, k
    for g in bad_geo:
        assert L.md_edm_heun_update_guide_tok(xp, xp, tp, tp, hp, np_, *g, *htail) == -1, g
    for t_in in (0.0, -1.0):
        zh = (3.0, t_in) + htail[2:]
        assert L.md_edm_heun_update_guide_tok(xp, xp, tp, tp, hp, np_, *geo, *zh) == -1
        assert L.md_edm_heun_update_guide(xp, xp, Fp, Fp, hp, np_, n, *zh) == -1
    for bad_n in (0, -4):
        assert L.md_edm_heun_update_guide(xp, xp, Fp, Fp, hp, np_, bad_n, *htail) == -1
    torch.cuda.synchronize()
    assert (h == 5.0).all() and (xn == 6.0).all()


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
    """The stand-in network of tests/test_samplers_gpu.py: a smooth fp32 function of its inputs in both loops, so nothing amplifies
    round-off."""
    model = _model(orc.tiny_config(), seed=11)

    def smooth(x, t, y, mask_ratio=0, **kw):
        x = x.float()
        cond = y.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)            # zeroed captions (the unconditional half) give 0
        return {"sample": torch.tanh(0.7 * x) * (1.0 + 0.1 * t.float().view(-1, 1, 1, 1)) + 0.05 * torch.roll(x, 1, -1) + cond, "mask": None}
    model.dit.forward_without_cfg = smooth
    return model


@pytest.fixture(scope="module")
def smooth_guide(hip):
    """A second smooth stand-in, a different function of the same inputs (another tanh slope, no roll term, a weaker caption term): the
    'bad version' of smooth_model.  Only its dit is used."""
    model = _model(orc.tiny_config(), seed=12)

    def smooth(x, t, y, mask_ratio=0, **kw):
        x = x.float()
        cond = y.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)
        return {"sample": torch.tanh(0.4 * x) * (1.0 + 0.1 * t.float().view(-1, 1, 1, 1)) + 0.5 * cond, "mask": None}
    model.dit.forward_without_cfg = smooth
    return model.dit


@pytest.fixture(scope="module")
def real_model(hip):
    cfg = orc.tiny_config()
    return _model(cfg, orc.synth_state_dict(cfg, 43))


@pytest.fixture(scope="module")
def real_guide(hip):
    """The narrower network: tiny_config() at dim = 128 (half of main's 256) with weights of another seed.  The engine takes that width,
    so the dim = 256 / depth = 1 fallback is not used."""
    cfg = orc.tiny_config()
    cfg.dim = 128
    return _model(cfg, orc.synth_state_dict(cfg, 47)).dit


def _middle_third(model, steps):
    """(sigma_lo, sigma_hi) that holds exactly the middle third of the schedule's noise levels, the ends between two levels."""
    ec = model.edm_config
    t = samplers.edm_schedule(steps, ec.sigma_min, ec.sigma_max, ec.rho)
    k = steps // 3
    return math.sqrt(t[steps - k] * t[steps - k - 1]), math.sqrt(t[k] * t[k - 1])


@pytest.mark.parametrize("sampler", SOLVERS)
def test_autoguided_fused_equals_tensor_op_with_smooth_networks(smooth_model, smooth_guide, sampler):
    lat, y = _inputs()
    kw = dict(steps=6, sampler=sampler, guide=smooth_guide)
    a = smooth_model.edm_sampler_loop(lat, y, cfg=2.5, fused=True, **kw)
    b = smooth_model.edm_sampler_loop(lat, y, cfg=2.5, fused=False, **kw)
    none = smooth_model.edm_sampler_loop(lat, y, cfg=1.0, fused=True, **kw)
    rel = _rel(a, b)
    print(sampler, rel, "against unguided", _rel(a, none))
    assert rel < 2e-6, rel
    assert torch.isfinite(a).all() and _rel(a, none) > 1e-5, "the guide must have moved the sample (five times what the bound resolves)"


@pytest.mark.parametrize("sampler", SOLVERS)
def test_autoguided_real_networks_fused_equals_tensor_op_and_cached_equals_uncached(real_model, real_guide, sampler):
    """Main: tiny_config() with synth_state_dict(cfg, 43); guide: dim = 128, seed 47 (see real_guide).  2e-2 through the bf16 networks for
    the reason test_fused_sampler_equals_tensor_op_sampler gives.  The cached path runs the same network kernels on the same operands as
    the uncached one in both networks (each with its own Conditioning) and the token-space update gives the bits of unpatchify + the
    image-space update, so those two are equal bit for bit."""
    lat, y = _inputs()
    kw = dict(steps=5, cfg=2.5, sampler=sampler, guide=real_guide)
    a = real_model.edm_sampler_loop(lat, y, fused=True, cond_cache=False, **kw)
    b = real_model.edm_sampler_loop(lat, y, fused=False, **kw)
    rel = _rel(a, b)
    none = real_model.edm_sampler_loop(lat, y, steps=5, cfg=1.0, sampler=sampler, cond_cache=False)
    print(sampler, rel, "against unguided", _rel(a, none))
    assert rel < 2e-2, rel
    assert torch.isfinite(a).all() and not torch.equal(a, none)
    c = real_model.edm_sampler_loop(lat, y, fused=True, cond_cache=True, **kw)
    assert torch.equal(c, a)


@pytest.mark.parametrize("sampler", SOLVERS)
@pytest.mark.parametrize("which,cond_cache", [("smooth", False), ("real", False), ("real", True)])
def test_main_as_its_own_guide_is_the_unguided_run(smooth_model, real_model, which, sampler, cond_cache):
    """F_guide = F_main bit for bit (the same kernels on the same operands), so fma(w, 0, f) = f exactly for every w.  (The stand-in
    replaces forward_without_cfg, which the cached path does not call: smooth runs uncached only.)"""
    model = smooth_model if which == "smooth" else real_model
    lat, y = _inputs()
    kw = dict(steps=5, sampler=sampler, cond_cache=cond_cache)
    none = model.edm_sampler_loop(lat, y, cfg=1.0, **kw)
    for w in (1.5, 4.0):
        assert torch.equal(model.edm_sampler_loop(lat, y, cfg=w, guide=model.dit, guide_captions="same", **kw), none), w


@pytest.mark.parametrize("sampler", SOLVERS)
def test_main_with_null_captions_is_classifier_free_guidance_smooth(smooth_model, sampler):
    lat, y = _inputs()
    kw = dict(steps=6, cfg=3.0, sampler=sampler)
    cfg_run = smooth_model.edm_sampler_loop(lat, y, **kw)
    for fused in (True, False):
        a = smooth_model.edm_sampler_loop(lat, y, fused=fused, guide=smooth_model.dit, guide_captions="null", **kw)
        rel = _rel(a, cfg_run)
        print(sampler, fused, rel)
        assert rel < 2e-6, (fused, rel)
    assert _rel(cfg_run, smooth_model.edm_sampler_loop(lat, y, steps=6, cfg=1.0, sampler=sampler)) > 1e-5


@pytest.mark.parametrize("cond_cache", [False, True])
@pytest.mark.parametrize("sampler", SOLVERS)
def test_main_with_null_captions_is_classifier_free_guidance_real(real_model, sampler, cond_cache):
    """Two batch-B launches against one batch-2B launch: the same arithmetic, but a batch-B launch may tile differently from half of a
    batch-2B launch, so the bound is the one through the bf16 network."""
    lat, y = _inputs()
    kw = dict(steps=5, cfg=3.0, sampler=sampler, cond_cache=cond_cache)
    cfg_run = real_model.edm_sampler_loop(lat, y, **kw)
    a = real_model.edm_sampler_loop(lat, y, guide=real_model.dit, guide_captions="null", **kw)
    rel = _rel(a, cfg_run)
    print(sampler, cond_cache, rel)
    assert rel < 2e-2, rel


class _Spy:
    """Records the batch of every evaluation of a DiT: through forward_without_cfg (the uncached path and the tensor-op loop) and through
    the engine's forward (the cached path; forward_without_cfg calls it too, so one evaluation is recorded once per entry)."""

    def __init__(self, dit, log, tag):
        self.dit, self.eng = dit, dit.engine
        self.orig_eng = self.eng.forward

        def eng_forward(x_img, t, y=None, **k):
            patches = k.get("patches")
            batch = patches.shape[0] // self.eng.cfg.tokens if patches is not None else x_img.shape[0]
            log.append((tag, batch))
            return self.orig_eng(x_img, t, y, **k)
        self.eng.forward = eng_forward

    def close(self):
        del self.eng.forward


@pytest.mark.parametrize("cond_cache", [False, True])
@pytest.mark.parametrize("sampler", SOLVERS)
def test_what_runs_under_a_guidance_interval(real_model, real_guide, sampler, cond_cache):
    lat, y = _inputs(2)
    iv = _middle_third(real_model, 6)
    ec = real_model.edm_config
    levels = samplers.evaluation_sigmas(sampler, samplers.edm_schedule(6, ec.sigma_min, ec.sigma_max, ec.rho))
    inside = [iv[0] <= s <= iv[1] for s in levels]
    assert len(levels) == (11 if sampler == "heun" else 6) and any(inside) and not all(inside)
    want = [e for g in inside for e in ([("main", 2), ("guide", 2)] if g else [("main", 2)])]     # main, then the guide, never 2B
    kw = dict(steps=6, sampler=sampler, cond_cache=cond_cache)
    plain = real_model.edm_sampler_loop(lat, y, cfg=1.0, **kw)
    log = []
    spies = [_Spy(real_model.dit, log, "main"), _Spy(real_guide, log, "guide")]
    try:
        real_model.edm_sampler_loop(lat, y, cfg=3.0, guidance_interval=iv, guide=real_guide, **kw)
        got = list(log)
        del log[:]
        real_model.edm_sampler_loop(lat, y, cfg=3.0, guide=real_guide, **kw)
        everywhere = list(log)
        del log[:]
        unguided = real_model.edm_sampler_loop(lat, y, cfg=1.0, guide=real_guide, **kw)
        at_one = list(log)
    finally:
        for s in spies:
            s.close()
    assert got == want, (got, want)
    assert everywhere == [("main", 2), ("guide", 2)] * len(levels)
    assert at_one == [("main", 2)] * len(levels), "cfg = 1 never evaluates the guide"
    assert torch.equal(unguided, plain)


def test_out_of_interval_guide_is_the_unguided_run(real_model, real_guide):
    lat, y = _inputs(2)
    kw = dict(steps=4, sampler="dpmpp_2m")
    none = real_model.edm_sampler_loop(lat, y, cfg=1.0, **kw)
    assert torch.equal(real_model.edm_sampler_loop(lat, y, cfg=3.0, guidance_interval=(100.0, 200.0), guide=real_guide, **kw), none)


def test_churn_with_a_guide(smooth_model, smooth_guide):
    """S_churn > 0 on euler with a guide; both loops draw once per step from the same generator."""
    lat, y = _inputs()
    ec = smooth_model.edm_config
    t = samplers.edm_schedule(6, ec.sigma_min, ec.sigma_max, ec.rho)
    saved = dict(ec)
    kw = dict(steps=6, cfg=2.5, sampler="euler", guide=smooth_guide)
    try:
        plain = smooth_model.edm_sampler_loop(lat, y, fused=True, **kw)
        ec.update(S_churn=20, S_noise=1.003, S_min=math.sqrt(t[4] * t[5]), S_max=math.sqrt(t[0] * t[1]))
        torch.manual_seed(21)
        a = smooth_model.edm_sampler_loop(lat, y, fused=True, **kw)
        torch.manual_seed(21)
        b = smooth_model.edm_sampler_loop(lat, y, fused=False, **kw)
    finally:
        ec.update(saved)
    rel = _rel(a, b)
    print(rel, "churn moved the sample by", _rel(a, plain))
    assert rel < 2e-6, rel
    assert _rel(a, plain) > 1e-3, "the churn must have changed the sample"
