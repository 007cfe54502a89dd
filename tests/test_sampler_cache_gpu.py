"""The cached sampling path: captions encoded once (`DiTEngine.encode_condition`), the sampler stepping in token space
(`md_edm_sampler_patchify`, `md_edm_heun_update_tok`).  Every comparison is `torch.equal`: the forward has no atomics (the four
atomic reductions of DESIGN.md section 4.4 are all in the backward) and the cached path launches the same kernels on the same
operands, so anything short of equality is a bug."""
import pytest
import torch

from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4, 6, 10),      # 720 elements: no multiple of 256, non-square; patch_vec 16
          (2, 16, 8, 8)]      # the 16-channel VAE: patch_vec 64
P = 2
SD = 0.9                      # sigma_data


def _st():
    return torch.cuda.current_stream().cuda_stream


def _model(cfg, seed):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(orc.synth_state_dict(cfg, seed))
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=cfg.input_size)
    m.eval()
    return m


def _engine_inputs(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda()
    x2 = torch.randn(B, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda()
    y = torch.randn(B, 1, 77, cfg.caption_channels, generator=g).cuda()
    return x, x2, y


# ------------------------------------------------------------------------------------------------ 1, 2: the two kernels
@pytest.mark.parametrize("sigma", [80.0, 0.002])
@pytest.mark.parametrize("duplicate", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_sampler_patchify_equals_sampler_input_then_patchify(hip, shape, duplicate, sigma):
    B, C, H, W = shape
    L, T, pv, n = hip.lib(), (H // P) * (W // P), C * P * P, B * C * H * W
    Bn = B * (2 if duplicate else 1)
    x = (torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * sigma).cuda()
    img = torch.empty(Bn, C, H, W, device="cuda")
    ref = torch.empty(Bn * T, pv, device="cuda", dtype=torch.bfloat16)
    hip.check(L.md_edm_sampler_input(x.data_ptr(), img.data_ptr(), n, sigma, SD, duplicate, _st()), "md_edm_sampler_input")
    hip.check(L.md_patchify(img.data_ptr(), None, ref.data_ptr(), Bn, C, H, W, P, _st()), "md_patchify")
    out = torch.full((Bn * T + 1, pv), 7.0, device="cuda", dtype=torch.bfloat16)     # one guard row behind the output
    hip.check(L.md_edm_sampler_patchify(x.data_ptr(), out.data_ptr(), B, C, H, W, P, sigma, SD, duplicate, _st()),
              "md_edm_sampler_patchify")
    assert torch.equal(out[:Bn * T], ref)
    assert (out[Bn * T] == 7.0).all(), "wrote behind the last row"
    assert ref.float().abs().max() > 0


@pytest.mark.parametrize("has_uncond", [0, 1])
@pytest.mark.parametrize("second", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_heun_update_tok_equals_unpatchify_then_heun_update(hip, shape, second, has_uncond):
    B, C, H, W = shape
    L, T, pv, n = hip.lib(), (H // P) * (W // P), C * P * P, B * C * H * W
    Bn = B * (2 if has_uncond else 1)
    g = torch.Generator().manual_seed(2)
    x_hat = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).cuda() * 3
    x_in = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).cuda() * 3
    d0 = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).cuda()
    tok = torch.randn(Bn * T, pv, generator=g).to(torch.bfloat16).cuda()
    cfg, t_in, t_hat, t_next = 3.0, 1.7, 2.5, 1.7
    img = torch.empty(Bn, C, H, W, device="cuda")
    hip.check(L.md_unpatchify(tok.data_ptr(), None, T, None, img.data_ptr(), Bn, C, H, W, P, _st()), "md_unpatchify")
    d_ref, x_ref = d0.clone(), torch.zeros_like(x_hat)
    hip.check(L.md_edm_heun_update(x_hat.data_ptr(), x_in.data_ptr(), img.data_ptr(), d_ref.data_ptr(), x_ref.data_ptr(), n, cfg,
                                   has_uncond, t_in, t_hat, t_next, SD, second, _st()), "md_edm_heun_update")
    d_out, x_out = d0.clone(), torch.zeros_like(x_hat)
    hip.check(L.md_edm_heun_update_tok(x_hat.data_ptr(), x_in.data_ptr(), tok.data_ptr(), d_out.data_ptr(), x_out.data_ptr(), B, C, H, W,
                                       P, cfg, has_uncond, t_in, t_hat, t_next, SD, second, _st()), "md_edm_heun_update_tok")
    assert torch.equal(x_out, x_ref) and torch.equal(d_out, d_ref)
    assert torch.equal(d_ref, d0) == bool(second)          # the first half-step writes d_cur, the second only reads it
    # the sampler's aliasing: x_hat == x_in on the first half-step, x_next == x_in on the second
    a_ref, a_out = x_in.clone(), x_in.clone()
    hat_r, hat_o = (x_hat, x_hat) if second else (a_ref, a_out)
    nxt_r, nxt_o = (a_ref, a_out) if second else (torch.zeros_like(x_hat), torch.zeros_like(x_hat))
    hip.check(L.md_edm_heun_update(hat_r.data_ptr(), a_ref.data_ptr(), img.data_ptr(), d_ref.data_ptr(), nxt_r.data_ptr(), n, cfg,
                                   has_uncond, t_in, t_hat, t_next, SD, second, _st()), "md_edm_heun_update")
    hip.check(L.md_edm_heun_update_tok(hat_o.data_ptr(), a_out.data_ptr(), tok.data_ptr(), d_out.data_ptr(), nxt_o.data_ptr(), B, C, H, W,
                                       P, cfg, has_uncond, t_in, t_hat, t_next, SD, second, _st()), "md_edm_heun_update_tok")
    assert torch.equal(nxt_o, nxt_r) and torch.equal(d_out, d_ref)


def test_token_kernels_refuse_bad_arguments_and_write_nothing(hip):
    B, C, H, W = 2, 4, 6, 10
    L, T, pv = hip.lib(), 15, 16
    x = torch.randn(B, C, H, W, dtype=torch.float64).cuda()
    tok = torch.randn(B * T, pv).to(torch.bfloat16).cuda()
    d, xn = torch.full_like(x, 5.0), torch.full_like(x, 6.0)
    args = (B, C, H, W, P, 3.0, 0, 1.7, 2.5, 1.7, SD, 0, _st())
    assert L.md_edm_heun_update_tok(None, x.data_ptr(), tok.data_ptr(), d.data_ptr(), xn.data_ptr(), *args) == -1
    assert L.md_edm_heun_update_tok(x.data_ptr(), x.data_ptr(), None, d.data_ptr(), xn.data_ptr(), *args) == -1
    assert L.md_edm_heun_update_tok(x.data_ptr(), x.data_ptr(), tok.data_ptr(), d.data_ptr(), None, *args) == -1
    bad_h = (B, C, 7, W, P) + args[5:]
    assert L.md_edm_heun_update_tok(x.data_ptr(), x.data_ptr(), tok.data_ptr(), d.data_ptr(), xn.data_ptr(), *bad_h) == -1
    out = torch.full((B * T, pv), 7.0, device="cuda", dtype=torch.bfloat16)
    assert L.md_edm_sampler_patchify(None, out.data_ptr(), B, C, H, W, P, 1.0, SD, 0, _st()) == -1
    assert L.md_edm_sampler_patchify(x.data_ptr(), None, B, C, H, W, P, 1.0, SD, 0, _st()) == -1
    assert L.md_edm_sampler_patchify(x.data_ptr(), out.data_ptr(), B, C, 7, W, P, 1.0, SD, 0, _st()) == -1
    torch.cuda.synchronize()
    assert (d == 5.0).all() and (xn == 6.0).all() and (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ 3 - 6: the engine
@pytest.fixture(scope="module", params=["tiny", "micro"])
def net(request, hip):
    """(model, x, second x, captions, uncached out_tok at two timesteps): the references are computed once and only read."""
    cfg = orc.tiny_config() if request.param == "tiny" else orc.micro_config()
    m = _model(cfg, 47)
    x, x2, y = _engine_inputs(cfg, 2, 13)
    ts = [torch.tensor([0.4, -0.2], device="cuda"), torch.tensor([-1.1, 0.9], device="cuda")]
    with torch.no_grad():
        m.dit.refresh_shadow()
        eng = m.dit._engine
        ref = [eng.forward(x, t, y.contiguous()).out_tok.clone() for t in ts]
        ref_x2 = eng.forward(x2, ts[0], y.contiguous()).out_tok.clone()
    return m, x, x2, y.contiguous(), ts, ref, ref_x2


def test_engine_cached_equals_uncached(net):
    """ONE cond at two different t (step-dependent state leaking into the cache would show at the second) and for a second x."""
    m, x, x2, y, ts, ref, ref_x2 = net
    eng = m.dit._engine
    assert not torch.equal(ref[0], ref[1])
    cond = m.dit.encode_condition(y)
    assert cond.B == 2 and cond.Lc == 77 and cond.nbytes > 0 and cond.version == eng.weights_version
    assert set(cond.kv) == {bp.name for bp in eng.mixer + eng.backbone}
    for t, r in zip(ts, ref):
        assert torch.equal(eng.forward(x, t, y, cond=cond).out_tok, r)
    assert torch.equal(eng.forward(x2, ts[0], None, cond=cond).out_tok, ref_x2)
    assert torch.equal(eng.forward(x, ts[0], y, cond=cond).out_tok, ref[0])          # and the cache is still intact
    with torch.no_grad():                                                             # the public wrapper takes it too
        img = m.dit.forward_without_cfg(x, ts[1], y, cond=cond)["sample"]
        assert torch.equal(img, m.dit.forward_without_cfg(x, ts[1], y)["sample"])


def test_engine_token_input_equals_image_input(net, hip):
    m, x, _, y, ts, ref, _ = net
    eng, cfg = m.dit._engine, m.dit.config
    B, T = x.shape[0], cfg.tokens
    patches = torch.empty(B * T, cfg.patch_vec, device="cuda", dtype=torch.bfloat16)
    hip.check(hip.lib().md_patchify(x.data_ptr(), None, patches.data_ptr(), B, cfg.in_channels, x.shape[2], x.shape[3], cfg.patch_size,
                                    _st()), "md_patchify")
    assert torch.equal(eng.forward(None, ts[0], y, patches=patches).out_tok, ref[0])
    cond = m.dit.encode_condition(y)
    assert torch.equal(eng.forward(None, ts[1], None, cond=cond, patches=patches).out_tok, ref[1])


def test_cached_forward_runs_no_caption_side_gemm(net):
    m, x, _, y, ts, _, _ = net
    eng = m.dit._engine
    cond = m.dit.encode_condition(y)
    names, orig = [], eng.lin_fwd

    def spy(x_, wname, *a, **k):
        names.append(wname)
        return orig(x_, wname, *a, **k)
    eng.lin_fwd = spy
    try:
        eng.forward(x, ts[0], y, cond=cond)
        cached = list(names)
        del names[:]
        eng.forward(x, ts[0], y)
        plain = list(names)
    finally:
        del eng.lin_fwd
    banned = ("kv_linear", "y_embedder", "y_emb_preprocess", "patch_mixer_map_y", "pooled_y_emb_process.fc1")
    assert not [n for n in cached if any(b in n for b in banned)]
    assert "pooled_y_emb_process.fc2" in cached
    assert any("kv_linear" in n for n in plain) and len(plain) > len(cached)          # the spy does see them when they run


def test_stale_or_mismatched_conditioning_raises(hip):
    cfg = orc.tiny_config()
    m = _model(cfg, 48)
    x, _, y = _engine_inputs(cfg, 2, 14)
    x3, _, _ = _engine_inputs(cfg, 3, 15)
    t = torch.tensor([0.1], device="cuda")
    eng = m.dit.engine
    cond = m.dit.encode_condition(y)
    eng.forward(x, t, None, cond=cond)
    with pytest.raises(RuntimeError, match="batch"):
        eng.forward(x3, t, None, cond=cond)
    with pytest.raises(RuntimeError, match="caption length"):
        eng.forward(x, t, y[:, :, :40].contiguous(), cond=cond)
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.forward(x, t, None, cond=cond, record_tape=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.forward(x, t, y, patches=torch.empty(2 * eng.cfg.tokens, eng.cfg.patch_vec, device="cuda", dtype=torch.bfloat16), mask_ratio=0.5)
    # The weights change.  An in-place update that autograd sees bumps the parameter's version counter and refresh_shadow()
    # re-derives the bf16 weights ...
    p = next(iter(m.dit.parameters()))
    with torch.no_grad():
        p.add_(0.01)
    m.dit.refresh_shadow()
    with pytest.raises(RuntimeError, match="weight version"):
        eng.forward(x, t, None, cond=cond)
    # ... a write through `.data` does not bump it (torch gives `.data` a version counter of its own), so a plain refresh_shadow()
    # leaves the bf16 weights -- and a conditioning derived from them -- as they were; writers of that kind force the refresh
    # (dit.refresh_shadow's contract), and that invalidates the cache as well.
    cond = m.dit.encode_condition(y)
    eng.forward(x, t, None, cond=cond)
    p.data.add_(0.01)
    m.dit.refresh_shadow(force=True)
    with pytest.raises(RuntimeError, match="weight version"):
        eng.forward(x, t, None, cond=cond)
    eng.forward(x, t, None, cond=m.dit.encode_condition(y))


# ------------------------------------------------------------------------------------------------ 7: the whole sampler
@pytest.mark.parametrize("guidance", [1.0, 4.0])
def test_cached_sampler_equals_uncached_sampler(hip, guidance):
    """The claim is bit-equality, and its basis is checked first: two uncached runs of the sampler are themselves equal (no atomics
    anywhere in the forward).  The oracle bound of test_sampler_ckpt_gpu.py on top, so equality to a broken baseline cannot pass."""
    cfg = orc.tiny_config()
    sd = orc.synth_state_dict(cfg, 41)
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(2, 4, 32, 32, generator=g)
    y = torch.randn(2, 1, 77, 1024, generator=g)
    model = _model(cfg, 41)
    a = model.edm_sampler_loop(lat.cuda(), y.cuda(), steps=4, cfg=guidance, cond_cache=False)
    b = model.edm_sampler_loop(lat.cuda(), y.cuda(), steps=4, cfg=guidance, cond_cache=False)
    assert torch.equal(a, b), "the uncached sampler is not reproducible: bit-equality of the cached path has no basis"
    c = model.edm_sampler_loop(lat.cuda(), y.cuda(), steps=4, cfg=guidance, cond_cache=True)
    assert torch.equal(c, a)
    ref = orc.edm_sampler(sd, cfg, lat, y, steps=4, guidance=guidance)
    rel = ((c.cpu() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    assert rel < 0.05, rel
