"""Image-conditioned sampling on the GPU: md_edm_blend_known against the formula in torch fp64 -- bit for bit where the
operands make the formula exact, within the roundings that separate two evaluation orders otherwise --, its refusals, and img2img,
inpainting and RePaint resampling through edm_sampler_loop: fused against the tensor-op loop (2e-6 with a smooth stand-in network, 2e-2
through the real bf16 network: the bounds and the reasons of tests/test_sampler_ckpt_gpu.py), the kept region bit for bit, cached against
uncached (torch.equal: the blend acts on the fp64 state only), with a guide network, and the default run unchanged."""
import math

import pytest
import torch

from micro_diffusion_amd import samplers
from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu

N = 6
INF, NAN = float("inf"), float("nan")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


# ------------------------------------------------------------------------------------------------ the kernel
SHAPES = [(3, 4, 6, 10),          # 720 elements: no multiple of 256 or 512
          (2, 3, 5, 7),           # odd HW: the element-wise path
          (3, 4, 32, 32),         # more than one workgroup
          (2, 16, 8, 8)]          # the 16-channel VAE


def _blend(hip, x, x0, noise, mask, shape, mask_B, sigma):
    B, C, H, W = shape
    return hip.lib().md_edm_blend_known(x.data_ptr(), x0.data_ptr(), None if noise is None else noise.data_ptr(),
                                        None if mask is None else mask.data_ptr(), B, C, H * W, mask_B, sigma, _st())


def _state(shape, g):
    """(the buffer with one guard element behind the state, the state as a view of it, a copy of the state)."""
    n = math.prod(shape)
    buf = torch.full((n + 1,), 7.0, device="cuda", dtype=torch.float64)
    buf[:n] = (torch.randn(n, generator=g, dtype=torch.float64) * 30).cuda()
    return buf, buf[:n].view(shape), buf[:n].view(shape).clone()


def _m(mask, shape, mask_B):
    """The fp32 mask [mask_B, HW] as the fp64 factor of every element of the state."""
    B, C, H, W = shape
    return mask.view(mask_B, 1, H, W).to(torch.float64).expand(B, C, H, W)


@pytest.mark.parametrize("per_sample", [False, True], ids=["mask_B=1", "mask_B=B"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_blend_known_against_torch_fp64(hip, shape, per_sample):
    B, C, H, W = shape
    n, mask_B = math.prod(shape), (B if per_sample else 1)
    g = torch.Generator().manual_seed(7)
    hard = (torch.rand(mask_B, H * W, generator=g) < 0.5).float().cuda()
    soft = torch.rand(mask_B, H * W, generator=g).cuda()
    soft[:, 0], soft[:, 1] = 0.0, 1.0
    # (1) mask in {0, 1}; sigma, noise and x0 with 24-bit significands: sigma * noise is exact in fp64, so x0 + sigma * noise rounds once
    # however torch evaluates it and equals the fma bit for bit (the construction of test_churn_is_one_fp64_fma)
    x0 = torch.randn(shape, generator=g).to(torch.float64).cuda()
    noise = torch.randn(shape, generator=g).to(torch.float64).cuda()
    sigma = float(torch.tensor(math.sqrt(33.0 ** 2 - 24.0 ** 2) * 1.003, dtype=torch.float32))
    buf, x, x_in = _state(shape, g)
    hip.check(_blend(hip, x, x0, noise, hard, shape, mask_B, sigma), "md_edm_blend_known")
    want = torch.where(_m(hard, shape, mask_B) == 1, x_in, x0 + sigma * noise)
    assert torch.equal(x, want) and buf[n] == 7.0, "wrong bits, or a write behind the last element"
    assert not torch.equal(want, x_in) and not torch.equal(want, x0 + sigma * noise), "both mask values must occur"
    # a state that is 8- but not 16-byte aligned goes element by element whatever HW is: the same bits, nothing outside it written
    off = torch.full((n + 2,), 7.0, device="cuda", dtype=torch.float64)
    off[1:n + 1] = x_in.reshape(-1)
    xo = off[1:n + 1].view(shape)
    assert xo.data_ptr() % 16 == 8
    hip.check(_blend(hip, xo, x0, noise, hard, shape, mask_B, sigma), "md_edm_blend_known")
    assert torch.equal(xo, want) and off[0] == 7.0 and off[n + 1] == 7.0
    # (4) the final paste: no noise, sigma = 0
    buf, x, x_in = _state(shape, g)
    hip.check(_blend(hip, x, x0, None, hard, shape, mask_B, 0.0), "md_edm_blend_known")
    assert torch.equal(x, torch.where(_m(hard, shape, mask_B) == 0, x0, x_in)) and buf[n] == 7.0
    # (3) no mask: the whole state is replaced and never read (NaN in it does not reach the result)
    buf, x, _ = _state(shape, g)
    x.fill_(NAN)
    hip.check(_blend(hip, x, x0, noise, None, shape, 1, sigma), "md_edm_blend_known")
    assert torch.equal(x, x0 + sigma * noise) and buf[n] == 7.0
    xa = noise.clone()                                              # in place on the noise, as the sampler's initialisation calls it
    hip.check(_blend(hip, xa, x0, xa, None, shape, 1, sigma), "md_edm_blend_known")
    assert torch.equal(xa, x)
    # (2) soft mask, full 53-bit operands: at most six roundings of 2^-53 each separate the two evaluation orders
    x0 = torch.randn(shape, generator=g, dtype=torch.float64).cuda()
    noise = torch.randn(shape, generator=g, dtype=torch.float64).cuda()
    sigma = math.sqrt(33.0 ** 2 - 24.0 ** 2) * 1.003
    buf, x, x_in = _state(shape, g)
    hip.check(_blend(hip, x, x0, noise, soft, shape, mask_B, sigma), "md_edm_blend_known")
    m = _m(soft, shape, mask_B)
    ref = m * x_in + (1 - m) * (x0 + sigma * noise)
    err, bound = (x - ref).abs(), 2.0 ** -50 * ((m * x_in).abs() + (1 - m) * (x0.abs() + (sigma * noise).abs()))
    print(shape, mask_B, "soft: largest error over its bound", (err / bound.clamp_min(1e-300)).max().item())
    assert (err <= bound).all() and buf[n] == 7.0
    sel = (m == 1)
    assert sel.any() and torch.equal(x[sel], x_in[sel]), "m = 1 returns x exactly"
    sel = (m == 0)
    assert sel.any() and ((x[sel] - (x0 + sigma * noise)[sel]).abs() <= 2.0 ** -52 * (x0.abs() + (sigma * noise).abs())[sel]).all()
    # the same without a mask
    buf, x, _ = _state(shape, g)
    hip.check(_blend(hip, x, x0, noise, None, shape, 1, sigma), "md_edm_blend_known")
    prod = sigma * noise
    assert ((x - (x0 + prod)).abs() <= 2.0 ** -52 * (x0.abs() + prod.abs())).all() and buf[n] == 7.0


def test_blend_known_refuses_bad_arguments_and_writes_nothing(hip):
    shape = B, C, H, W = 3, 4, 6, 10
    L, HW = hip.lib(), H * W
    x = torch.full(shape, 5.0, device="cuda", dtype=torch.float64)
    x0 = torch.randn(shape, dtype=torch.float64).cuda()
    noise = torch.randn(shape).to(torch.float64).cuda()               # 24-bit significands: 1.5 * noise is exact
    mask = torch.zeros(B, HW, device="cuda")                         # m = 0 everywhere: any launch would overwrite the sentinel
    X, X0, NZ, M = x.data_ptr(), x0.data_ptr(), noise.data_ptr(), mask.data_ptr()
    assert L.md_edm_blend_known(None, X0, NZ, M, B, C, HW, B, 1.5, _st()) == -1
    assert L.md_edm_blend_known(X, None, NZ, M, B, C, HW, B, 1.5, _st()) == -1
    for dims in ((0, C, HW), (-1, C, HW), (B, 0, HW), (B, -2, HW), (B, C, 0), (B, C, -HW)):
        assert L.md_edm_blend_known(X, X0, NZ, M, *dims, 1, 1.5, _st()) == -1, dims
    for mask_B in (2, 0, -1, B + 1):                                 # neither 1 nor B
        assert L.md_edm_blend_known(X, X0, NZ, M, B, C, HW, mask_B, 1.5, _st()) == -1, mask_B
    assert L.md_edm_blend_known(X, X0, None, M, B, C, HW, B, 1.5, _st()) == -1, "no noise, but sigma != 0"
    assert L.md_edm_blend_known(X, X0, None, None, B, C, HW, 1, 1.5, _st()) == -1
    for sigma in (-1.5, -1e-300, INF, -INF, NAN):
        assert L.md_edm_blend_known(X, X0, NZ, M, B, C, HW, B, sigma, _st()) == -1, sigma
        assert L.md_edm_blend_known(X, X0, NZ, None, B, C, HW, 1, sigma, _st()) == -1, sigma
    torch.cuda.synchronize()
    assert (x == 5.0).all()
    # and the call these were derived from is accepted
    assert L.md_edm_blend_known(X, X0, NZ, M, B, C, HW, B, 1.5, _st()) == 0
    assert torch.equal(x, x0 + 1.5 * noise)


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
    """(unit noise, captions, known latents, centred-hole mask [32, 32]: 1 inside the 16 x 16 hole)."""
    g = torch.Generator().manual_seed(10)
    lat, y = torch.randn(B, 4, 32, 32, generator=g).cuda(), torch.randn(B, 1, 77, 1024, generator=g).cuda()
    init = (torch.randn(B, 4, 32, 32, generator=g) * 0.5).cuda()
    hole = torch.zeros(32, 32, device="cuda")
    hole[8:24, 8:24] = 1.0
    return lat, y, init, hole


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
def plain(smooth_model):
    """The run from pure noise of every sampler, computed once."""
    lat, y, _, _ = _inputs()
    return {s: smooth_model.edm_sampler_loop(lat, y, steps=N, cfg=3.0, fused=True, sampler=s) for s in samplers.SAMPLERS}


@pytest.fixture(scope="module")
def real_model(hip):
    cfg = orc.tiny_config()
    return _model(cfg, orc.synth_state_dict(cfg, 43))


@pytest.fixture(scope="module")
def real_guide(hip):
    """The narrower network of tests/test_autoguidance_gpu.py: tiny_config() at dim = 128 with weights of another seed."""
    cfg = orc.tiny_config()
    cfg.dim = 128
    return _model(cfg, orc.synth_state_dict(cfg, 47)).dit


def _soft_mask(hole, B):
    """[B, 1, 32, 32]: the hole with a half-weight rim, another rim weight per sample (mask_B = B in the kernel)."""
    m = hole.clone()
    m[6:26, 6:26] = torch.maximum(m[6:26, 6:26], torch.tensor(0.5, device=m.device))
    out = m.view(1, 1, 32, 32).repeat(B, 1, 1, 1)
    for b in range(B):
        out[b][(out[b] > 0) & (out[b] < 1)] = 0.25 * (b + 1)
    return out


CASES = [("img2img", s, dict(strength=0.5), False) for s in samplers.SAMPLERS] + \
        [("hole", s, dict(mask="hole"), False) for s in samplers.SAMPLERS] + \
        [("soft", "heun", dict(mask="soft"), False)] + \
        [("resample2", s, dict(mask="hole", resample=2), False) for s in ("heun", "euler")] + \
        [("hole+churn", "heun", dict(mask="hole"), True)]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_fused_equals_tensor_op_with_a_smooth_network(smooth_model, plain, case):
    name, sampler, kw, churn = case
    lat, y, init, hole = _inputs()
    kw = dict(kw)
    which = kw.pop("mask", None)
    mask = {None: None, "hole": hole, "soft": _soft_mask(hole, lat.shape[0])}[which]
    ec = smooth_model.edm_config
    t = samplers.edm_schedule(N, ec.sigma_min, ec.sigma_max, ec.rho)
    saved = dict(ec)
    try:
        if churn:                                                   # the settings of test_churn_runs_on_the_fused_loop
            ec.update(S_churn=20, S_noise=1.003, S_min=math.sqrt(t[4] * t[5]), S_max=math.sqrt(t[0] * t[1]))
        run = lambda fused: smooth_model.edm_sampler_loop(lat, y, steps=N, cfg=3.0, fused=fused, sampler=sampler, init_latents=init,   # noqa: E731
                                                          inpaint_mask=mask, **kw)
        torch.manual_seed(21)
        a = run(True)
        torch.manual_seed(21)
        b = run(False)
    finally:
        ec.update(saved)
    rel, moved = _rel(a, b), _rel(a, plain[sampler])
    print(name, sampler, "fused against tensor-op", rel, "against the plain run", moved)
    assert torch.isfinite(a).all() and rel < 2e-6, rel
    assert moved > 1e-5, "the image-conditioned run must differ from the run from pure noise"
    if mask is not None:
        keep = (mask == 0).expand_as(a) if mask.dim() == 4 else (mask == 0).expand(a.shape)
        assert keep.any() and torch.equal(a[keep], init[keep]) and torch.equal(b[keep], init[keep]), "the kept region is init_latents, bit for bit"
        assert not torch.equal(a[~keep], init[~keep])


@pytest.mark.parametrize("sampler", ["heun", "euler"])
def test_real_network_cached_equals_uncached_and_fused_matches_tensor_op(real_model, sampler):
    """Through the real bf16 network: the cached path launches the same network kernels on the same operands as the uncached one and the
    blend acts on the fp64 state only, so those two are equal bit for bit; 2e-2 against the tensor-op loop for the reason given in
    test_fused_sampler_equals_tensor_op_sampler."""
    lat, y, init, hole = _inputs(2)
    kw = dict(steps=4, cfg=3.0, sampler=sampler, init_latents=init, inpaint_mask=hole)
    out = []
    for mode in (dict(fused=True, cond_cache=False), dict(fused=True, cond_cache=True), dict(fused=False)):
        torch.manual_seed(22)
        out.append(real_model.edm_sampler_loop(lat, y, **mode, **kw))
    a, c, b = out
    assert torch.equal(c, a)
    rel = _rel(a, b)
    print(sampler, "fused against tensor-op through the network", rel)
    assert torch.isfinite(a).all() and rel < 2e-2, rel
    keep = (hole == 0).expand(a.shape)
    assert torch.equal(a[keep], init[keep])


@pytest.mark.parametrize("cond_cache", [False, True])
def test_real_network_with_a_guide(real_model, real_guide, cond_cache):
    lat, y, init, hole = _inputs(2)
    torch.manual_seed(23)
    a = real_model.edm_sampler_loop(lat, y, steps=4, cfg=2.5, guide=real_guide, cond_cache=cond_cache, init_latents=init, inpaint_mask=hole,
                                    strength=0.75)
    keep = (hole == 0).expand(a.shape)
    assert torch.isfinite(a).all() and torch.equal(a[keep], init[keep]) and not torch.equal(a[~keep], init[~keep])


def test_the_callers_noise_is_not_written(smooth_model):
    """The fused loop writes the SDEdit start in place into its state; an fp64, contiguous x must not be that state."""
    lat, y, init, hole = _inputs()
    x64 = lat.to(torch.float64).contiguous()
    before = x64.clone()
    torch.manual_seed(24)
    a = smooth_model.edm_sampler_loop(x64, y, steps=N, cfg=3.0, fused=True, init_latents=init, inpaint_mask=hole, strength=0.5)
    assert torch.equal(x64, before), "the caller's noise was overwritten"
    torch.manual_seed(24)
    b = smooth_model.edm_sampler_loop(lat, y, steps=N, cfg=3.0, fused=True, init_latents=init, inpaint_mask=hole, strength=0.5)
    assert torch.equal(a, b), "fp32 noise widened by the caller or by the loop: the same run"


# ------------------------------------------------------------------------------------------------ the default
@pytest.mark.parametrize("cond_cache", [False, True])
def test_default_sampler_is_unchanged(real_model, cond_cache):
    lat, y, _, _ = _inputs(2)
    a = real_model.edm_sampler_loop(lat, y, steps=4, cfg=4.0, cond_cache=cond_cache)
    b = real_model.edm_sampler_loop(lat, y, steps=4, cfg=4.0, cond_cache=cond_cache, init_latents=None, strength=1.0, inpaint_mask=None,
                                    resample=1)
    assert torch.equal(a, b)
