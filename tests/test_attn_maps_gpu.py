"""Cross-attention maps through the engine and the sampler: every recorded block against the fp64 softmax of that
block's taped q / k under the derived bound of tests/attn_probs_ref.py, both q / k layouts, cached conditioning, the guided batch
layout, a masked pass, both sampler loops, the step cache, disarming, and the mask helper feeding the inpainting sampler."""
import pytest
import torch

from oracle import microdit_ref as orc
from tests import attn_probs_ref as ref_mod

pytestmark = pytest.mark.gpu

B, LC = 3, 77


def _model(cfg, seed):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(orc.synth_state_dict(cfg, seed))
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=cfg.input_size)
    m.eval()
    return m


@pytest.fixture(scope="module")
def nets(hip):
    """name -> (model, x [B, C, H, W], captions [B, 1, 77, Dc], t [B]); built once, only read."""
    out = {}
    for name, cfg, seed in (("micro", orc.micro_config(), 61), ("tiny", orc.tiny_config(), 62)):
        m = _model(cfg, seed)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda()
        y = torch.randn(B, 1, LC, cfg.caption_channels, generator=g).cuda().contiguous()
        m.dit.refresh_shadow()
        out[name] = (m, x, y, torch.tensor([0.4, -0.2, 0.1], device="cuda"))
    return out


@pytest.fixture(autouse=True)
def _restore_engines(nets):
    yield
    for m, *_ in nets.values():
        eng = m.dit.engine
        eng.attn_probe, eng.keep_last_tape, eng.last_tape, eng.qk_head_major = None, False, None, False


def _blocks(eng, tape):
    return list(zip(list(eng.mixer) + list(eng.backbone), list(tape.mixer) + list(tape.blocks)))


def _taped_qk(eng, bp, bt, nb, S):
    """The normalised q [nb, H, S, hd] and k [nb, H, Lc, hd] the block's cross-attention read, from its tape (either layout)."""
    H, hd = bp.xheads, eng.cfg.head_dim
    if bt.q2n is not None:
        return bt.q2n.view(nb, H, S, hd), bt.k2n.view(nb, H, LC, hd)
    return (bt.q2.view(nb, S, H, hd).permute(0, 2, 1, 3), bt.kv[:, :H * hd].reshape(nb, LC, H, hd).permute(0, 2, 1, 3))


def _check_against_tape(am, eng, tapes, nb, what, first=None):
    """Every selected block's sums against the tape of the one evaluation recorded -- or the tapes of the several evaluations added
    into the buffer; first: only the leading samples were recorded."""
    T = eng.cfg.tokens
    tapes = tapes if isinstance(tapes, list) else [tapes]
    for i, bp in enumerate(list(eng.mixer) + list(eng.backbone)):
        if bp.name not in am.row:
            continue
        parts = []
        for tape in tapes:
            q, k = _taped_qk(eng, bp, _blocks(eng, tape)[i][1], nb, T)
            if first is not None:
                q, k = q[:first], k[:first]
            parts.append(ref_mod.reference(q, k, ref_mod.f32_scale(eng.cfg.head_dim)))
        got = am.buf[am.row[bp.name]][:, :, :LC]
        ref_mod.assert_within_bound(got, parts, what=f"{what} {bp.name}")


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("head_major", [False, True])
@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_engine_forward_records_every_block_within_the_bound(nets, name, head_major):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, x, y, t = nets[name]
    eng = m.dit.engine
    eng.qk_head_major, eng.keep_last_tape = head_major, True
    am = AttentionMaps().arm(eng)
    tape = eng.forward(x, t, y)
    AttentionMaps.disarm(eng)
    names = [bp.name for bp in list(eng.mixer) + list(eng.backbone)]
    assert am.names == names and am.counts == {n: 1 for n in names}
    assert am.buf.shape == (len(names), B, eng.cfg.tokens, 80) and (am.buf[..., LC:] == 0).all()
    _check_against_tape(am, eng, tape, B, f"{name} hm={head_major}")
    tm = am.token_mass()
    torch.testing.assert_close(tm.sum(1), torch.ones(len(names), device="cuda"), rtol=2e-5, atol=0)
    # cached conditioning: the same launches on the same operands
    cond = m.dit.encode_condition(y)
    am2 = AttentionMaps().arm(eng)
    eng.forward(x, t, None, cond=cond)
    AttentionMaps.disarm(eng)
    assert torch.equal(am2.buf, am.buf)
    # an unarmed pass afterwards gives the same output as the armed one: the recorder only reads
    assert torch.equal(eng.forward(x, t, y).out_tok, tape.out_tok)


def test_selection_records_only_the_selected_blocks(nets):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, x, y, t = nets["micro"]
    eng = m.dit.engine
    eng.keep_last_tape = True
    am = AttentionMaps(blocks=["blocks.2", "patch_mixer.1"]).arm(eng)
    tape = eng.forward(x, t, y)
    assert am.names == ["patch_mixer.1", "blocks.2"] and am.buf.shape[0] == 2 and am.counts == {"patch_mixer.1": 1, "blocks.2": 1}
    _check_against_tape(am, eng, tape, B, "selection")


def test_guided_layout_records_the_conditional_half_only(nets):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, x, y, t = nets["micro"]
    eng = m.dit.engine
    eng.keep_last_tape = True
    am = AttentionMaps().arm(eng)
    am.begin_evaluation(None, B)
    tape = eng.forward(torch.cat([x, x]).contiguous(), torch.cat([t, t]), torch.cat([y, torch.zeros_like(y)]).contiguous())
    assert am.buf.shape[1] == B
    _check_against_tape(am, eng, tape, 2 * B, "guided", first=B)


def test_masked_pass_scatters_backbone_rows_and_leaves_dropped_rows_zero(nets):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, x, y, t = nets["micro"]
    eng = m.dit.engine
    eng.keep_last_tape = True
    T, Tk = eng.cfg.tokens, eng.cfg.tokens // 2
    noise = torch.rand(B, T, generator=torch.Generator().manual_seed(9)).cuda()
    am = AttentionMaps().arm(eng)
    tape = eng.forward(x, t, y, mask_ratio=0.5, mask_noise=noise)
    assert tape.Tk == Tk and tape.keep_rows.numel() == B * Tk
    keep = tape.keep_rows.long()
    dropped = tape.mask.bool().reshape(B * T)
    assert int(dropped.sum()) == B * (T - Tk) and not dropped[keep].any()
    scale = ref_mod.f32_scale(eng.cfg.head_dim)
    for bp, bt in _blocks(eng, tape):
        rows = am.buf[am.row[bp.name]].view(B * T, -1)
        if bp in eng.mixer:                                             # all T tokens
            ref, E = ref_mod.reference(*_taped_qk(eng, bp, bt, B, T), scale)
            ref_mod.assert_within_bound(rows.view(B, T, -1)[:, :, :LC], ref, E, f"masked {bp.name}")
        else:                                                           # the kept tokens, scattered through keep_rows
            ref, E = ref_mod.reference(*_taped_qk(eng, bp, bt, B, Tk), scale)
            ref_mod.assert_within_bound(rows[keep].view(B, Tk, -1)[:, :, :LC], ref, E, f"masked {bp.name}")
            assert (rows[dropped] == 0).all(), f"{bp.name}: a dropped token's row was written"
    assert am.counts == {n: 1 for n in am.names}


# ------------------------------------------------------------------------------------------------ sampler
def _noise(m, seed):
    cfg = m.dit.config
    return torch.randn(B, cfg.in_channels, cfg.input_size, cfg.input_size, generator=torch.Generator().manual_seed(seed)).cuda()


def test_tensor_op_loop_accumulates_exactly_the_replayed_evaluations(nets):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, _, y, _ = nets["micro"]
    eng, x = m.dit.engine, _noise(m, 71)
    calls, orig = [], m.dit.forward

    def spy(x_, t_, y_, **kw):
        calls.append((x_.clone(), t_.clone(), y_.clone(), dict(kw)))
        return orig(x_, t_, y_, **kw)
    m.dit.forward = spy
    try:
        am = AttentionMaps()
        lat = m.edm_sampler_loop(x, y, steps=3, cfg=3.0, fused=False, attn_maps=am)
    finally:
        del m.dit.forward
    assert eng.attn_probe is None
    assert len(calls) == 5 and am.counts == {n: 5 for n in am.names} and am.buf.shape[1] == B
    total = torch.zeros_like(am.buf)
    am2 = AttentionMaps()
    for x_, t_, y_, kw in calls:
        am2.arm(eng)
        am2.begin_evaluation(None, B)
        with torch.no_grad():
            m.dit.forward(x_, t_, y_, **kw)
        total = total + am2.buf
    AttentionMaps.disarm(eng)
    assert torch.equal(total, am.buf)
    assert torch.equal(lat, m.edm_sampler_loop(x, y, steps=3, cfg=3.0, fused=False)), "the recorder changed the latents"
    torch.testing.assert_close(am.token_mass().sum(1), torch.ones(len(am.names), device="cuda"), rtol=2e-5, atol=0)


def test_fused_loop_is_reproducible_cache_invariant_and_read_only(nets):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, _, y, _ = nets["tiny"]
    x = _noise(m, 73)
    runs = []
    for cc in (False, False, True):
        am = AttentionMaps()
        runs.append((m.edm_sampler_loop(x, y, steps=3, cfg=3.0, cond_cache=cc, attn_maps=am), am))
        assert m.dit.engine.attn_probe is None
    (l0, a0), (l1, a1), (l2, a2) = runs
    assert torch.equal(a0.buf, a1.buf) and torch.equal(a0.buf, a2.buf) and a0.buf.abs().max() > 0
    assert a0.counts == {n: 5 for n in a0.names} == a2.counts
    plain = m.edm_sampler_loop(x, y, steps=3, cfg=3.0, cond_cache=False)
    assert torch.equal(l0, plain) and torch.equal(l1, plain) and torch.equal(l2, plain)
    maps = a0.maps()
    g = m.dit.config.input_size // m.dit.config.patch_size
    assert maps.shape == (B, LC, g, g)
    torch.testing.assert_close(maps.sum(1), torch.ones(B, g, g, device="cuda"), rtol=2e-5, atol=0)


def test_sigma_range_selects_evaluations_and_the_last_one_matches_its_tape(nets):
    from micro_diffusion_amd import samplers, sampling
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, _, y, _ = nets["tiny"]
    eng, x = m.dit.engine, _noise(m, 79)
    plan = sampling.sampler_plan(m.edm_config, 3, "heun")
    sig = samplers.evaluation_sigmas("heun", plan.t_steps)
    assert sig == plan.sigmas and len(sig) == 5
    # Heun's final step has a single evaluation, at the level its predecessor's second evaluation ran at: the narrowest range around
    # the last evaluation holds those two, the last two of the run
    last = sig[-1]
    assert sig[-2] == last and sig[-3] > last
    eng.keep_last_tape = True                                          # every evaluation keeps its tape
    tapes, orig = [], eng.forward

    def spy(*a, **kw):
        tapes.append(orig(*a, **kw))
        return tapes[-1]
    eng.forward = spy
    try:
        am = AttentionMaps(sigma_range=(last, last))
        m.edm_sampler_loop(x, y, steps=3, cfg=3.0, cond_cache=False, attn_maps=am)
    finally:
        del eng.forward
    assert len(tapes) == 5 and tapes[-1] is eng.last_tape
    assert am.counts == {n: len([s for s in sig if last <= s <= last]) for n in am.names} == {n: 2 for n in am.names}
    _check_against_tape(am, eng, tapes[-2:], 2 * B, "last two evaluations", first=B)
    # the euler solver visits every level once: the range of the last one selects the last evaluation alone
    am = AttentionMaps(sigma_range=(last, last))
    m.edm_sampler_loop(x, y, steps=3, cfg=3.0, cond_cache=False, sampler="euler", attn_maps=am)
    assert am.counts == {n: 1 for n in am.names}
    _check_against_tape(am, eng, eng.last_tape, 2 * B, "last evaluation (euler)", first=B)
    del tapes[:]
    eng.keep_last_tape, eng.last_tape = False, None
    lo, hi = 0.5 * (sig[2] + sig[3]), 0.5 * (sig[0] + sig[1])
    want = len([s for s in sig if lo <= s <= hi])
    assert 0 < want < len(sig)
    am = AttentionMaps(blocks="blocks", sigma_range=(lo, hi))
    m.edm_sampler_loop(x, y, steps=3, cfg=3.0, cond_cache=True, attn_maps=am)
    assert am.counts == {n: want for n in am.names} and all(n.startswith("blocks.") for n in am.names)


def test_step_cache_skipped_blocks_count_less(nets):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    from micro_diffusion_amd.step_cache import StepCache
    m, _, y, _ = nets["tiny"]
    x = _noise(m, 83)
    am, sc = AttentionMaps(), StepCache(interval=2)
    lat = m.edm_sampler_loop(x, y, steps=4, cfg=3.0, cond_cache=True, step_cache=sc, attn_maps=am)
    st = sc.stats
    assert st.evaluations == 7 and 0 < st.full < st.evaluations
    for n, c in am.counts.items():
        assert c == (st.evaluations if n.startswith("patch_mixer.") else st.full), (n, c)
    assert torch.equal(lat, m.edm_sampler_loop(x, y, steps=4, cfg=3.0, cond_cache=True, step_cache=StepCache(interval=2)))


def test_engine_is_disarmed_after_an_error_inside_the_loop(nets):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, _, y, _ = nets["micro"]
    eng, x = m.dit.engine, _noise(m, 89)
    orig, n = m.dit.forward_without_cfg, [0]

    def failing(*a, **kw):
        n[0] += 1
        if n[0] == 2:
            assert eng.attn_probe is not None
            raise RuntimeError("boom")
        return orig(*a, **kw)
    m.dit.forward_without_cfg = failing
    try:
        with pytest.raises(RuntimeError, match="boom"):
            m.edm_sampler_loop(x, y, steps=3, cfg=1.0, cond_cache=False, attn_maps=AttentionMaps())
    finally:
        del m.dit.forward_without_cfg
    assert n[0] == 2 and eng.attn_probe is None
    with pytest.raises(ValueError, match="selects no block"):
        m.edm_sampler_loop(x, y, steps=3, attn_maps=AttentionMaps(blocks="blocks.99"))
    assert eng.attn_probe is None


def test_mask_from_the_maps_drives_inpainting_and_the_kept_region_is_bit_exact(nets):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, _, y, _ = nets["micro"]
    x = _noise(m, 97)
    am = AttentionMaps()
    lat = m.edm_sampler_loop(x, y, steps=3, cfg=3.0, attn_maps=am)
    mask = am.mask(tokens=[1, 2], quantile=0.75, dilate=1)
    assert mask.shape == (B, 1, x.shape[2], x.shape[3]) and set(mask.unique().tolist()) == {0.0, 1.0}
    out = m.edm_sampler_loop(_noise(m, 101), y, steps=3, cfg=3.0, init_latents=lat, inpaint_mask=mask)
    kept = (mask == 0).expand_as(lat)
    assert torch.equal(out[kept], lat[kept]) and not torch.equal(out[~kept], lat[~kept])
