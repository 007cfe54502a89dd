"""Prompt control through the engine and the sampler: every block's biased cross-attention against the fp64 reference of
its taped operands (the FACTOR rule of tests/test_attention_edges_gpu.py), the refusals of a taping forward, and -- in both sampler
loops -- the identities (unit weights and a zero negative prompt are the plain guided run, bit for bit), loop parity, the layout of a
doubled evaluation, the attention maps of a run with removed positions, and disarming.  Micro and tiny configs, B = 3, Lc = 77."""
import pytest
import torch

from tests import attention_ref as ar
from tests import attn_kbias_ref as kr
from tests import test_attention_edges_gpu as edges
from tests import test_attn_maps_gpu as maps_t

pytestmark = pytest.mark.gpu

B, LC = maps_t.B, maps_t.LC
NEG = float("-inf")
LOOP_TOL = 2e-2          # fused against tensor-op loop through the real bf16 network: the bound tests/test_samplers_gpu.py uses for that pair
_rel = lambda a, b: ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()      # its measure


@pytest.fixture(scope="module")
def nets(hip):
    """name -> (model, x [B, C, H, W], captions [B, 1, 77, Dc], t [B], negative captions [B, 1, 77, Dc]); built once, only read."""
    from oracle import microdit_ref as orc
    out = {}
    for name, cfg, seed in (("micro", orc.micro_config(), 161), ("tiny", orc.tiny_config(), 162)):
        m = maps_t._model(cfg, seed)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda()
        y = torch.randn(B, 1, LC, cfg.caption_channels, generator=g).cuda().contiguous()
        neg = torch.randn(B, 1, LC, cfg.caption_channels, generator=g).cuda().contiguous()
        m.dit.refresh_shadow()
        out[name] = (m, x, y, torch.tensor([0.4, -0.2, 0.1], device="cuda"), neg)
    return out


@pytest.fixture(autouse=True)
def _restore_engines(nets):
    yield
    for m, *_ in nets.values():
        eng = m.dit.engine
        eng.attn_probe, eng.keep_last_tape, eng.last_tape, eng.qk_head_major, eng.caption_bias = None, False, None, False, None


def _weights(seed, rows=B):
    """[rows, 77]: row 0 all ones, row 1 the last 30 positions removed, the others random in [0, 3) with every fifth position removed."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(rows, LC, generator=g) * 3
    w[:, ::5] = 0
    w[:, 1] = 1
    w[0] = 1
    if rows > 1:
        w[1] = 1
        w[1, LC - 30:] = 0
    return w.cuda()


def _bias(w):
    from micro_diffusion_amd import samplers
    return samplers.caption_bias_buffer(w, None, w.shape[0], LC, False, "cuda")


def _check_blocks_against_tape(eng, tape, bias, nb, what):
    """Every mixer and backbone block's taped o2 against the biased attention of its taped q, k, v."""
    T = eng.cfg.tokens
    hd = eng.cfg.head_dim
    for bp, bt in maps_t._blocks(eng, tape):
        Hx = bp.xheads
        q, k = maps_t._taped_qk(eng, bp, bt, nb, T)
        v = bt.kv[:, Hx * hd:2 * Hx * hd].reshape(nb, LC, Hx, hd).permute(0, 2, 1, 3)
        o = bt.o2.view(nb, T, Hx, hd).permute(0, 2, 1, 3)
        scale = ar.scale_of(hd)
        R, E = kr.reference(q, k, v, bias[:nb, :LC], scale), kr.emulation(q, k, v, bias[:nb, :LC], scale)
        edges.judge(f"{what} {bp.name}", "randn", {"o": o}, R, E, ["o"])
        edges.judge_lse(f"{what} {bp.name}", bt.lse2, R)


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("head_major", [False, True])
@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_engine_blocks_run_the_biased_attention(nets, name, head_major):
    m, x, y, t, _ = nets[name]
    eng = m.dit.engine
    eng.qk_head_major, eng.keep_last_tape = head_major, True
    plain = eng.forward(x, t, y).out_tok.clone()
    bias = _bias(_weights(5))
    assert bias.shape == (B, 80) and bool((bias[0] == 0).all()) and bool(torch.isinf(bias[1, LC - 30:LC]).all())
    eng.caption_bias = bias
    tape = eng.forward(x, t, y)
    _check_blocks_against_tape(eng, tape, bias, B, f"{name} hm={head_major}")
    assert not torch.equal(tape.out_tok, plain), "the bias must change the output"
    # cached conditioning: the bias is per sample, independent of the cached K and V
    cond = m.dit.encode_condition(y)
    assert torch.equal(eng.forward(x, t, None, cond=cond).out_tok, tape.out_tok)
    # a batch below Bmax reads the leading rows
    t1 = eng.forward(x[:2].contiguous(), t[:2], y[:2].contiguous())
    _check_blocks_against_tape(eng, t1, bias, 2, f"{name} hm={head_major} B=2")
    # a zero bias is the plain pass, bit for bit; so is disarming
    eng.caption_bias = torch.zeros_like(bias)
    assert torch.equal(eng.forward(x, t, y).out_tok, plain)
    eng.caption_bias = None
    assert torch.equal(eng.forward(x, t, y).out_tok, plain)


def test_masked_pass_keeps_working_with_a_bias(nets):
    m, x, y, t, _ = nets["micro"]
    eng = m.dit.engine
    noise = torch.rand(B, eng.cfg.tokens, generator=torch.Generator().manual_seed(9)).cuda()
    eng.caption_bias = torch.zeros(B, 80, device="cuda")
    a = eng.forward(x, t, y, mask_ratio=0.5, mask_noise=noise).out_tok.clone()
    eng.caption_bias = None
    assert torch.equal(a, eng.forward(x, t, y, mask_ratio=0.5, mask_noise=noise).out_tok)


def test_taping_forwards_and_bad_buffers_are_refused_before_any_launch(nets):
    m, x, y, t, _ = nets["micro"]
    eng = m.dit.engine
    eng.caption_bias = _bias(_weights(6))
    log = eng.gemm_log = []
    try:
        for kw in (dict(record_tape=True), dict(arena=True), dict(record_tape=True, arena=True)):
            with pytest.raises(RuntimeError, match="caption_bias"):
                eng.forward(x, t, y, **kw)
        assert log == [], "a refused forward launched a GEMM"
        cond = m.dit.encode_condition(y)
        del log[:]
        with pytest.raises(RuntimeError, match="caption_bias"):
            eng.forward(x, t, None, cond=cond, input_tape=True)
        eng.caption_bias = _bias(_weights(6, rows=2))                    # B > Bmax
        with pytest.raises(ValueError, match="caption_bias"):
            eng.forward(x, t, y)
        eng.caption_bias = torch.zeros(B, 76, device="cuda")             # ldb < Lc
        with pytest.raises(ValueError, match="caption_bias"):
            eng.forward(x, t, y)
        assert log == [], "a refused forward launched a GEMM"
    finally:
        eng.gemm_log = None
    eng.caption_bias = _bias(_weights(6))
    eng.keep_last_tape = True                                            # the tests' tape is no backward's: it keeps working
    assert eng.forward(x, t, y) is eng.last_tape


# ------------------------------------------------------------------------------------------------ sampler: identities
@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_unit_weights_and_a_zero_negative_prompt_are_the_plain_guided_run(nets, name):
    m, _, y, _, _ = nets[name]
    x = maps_t._noise(m, 171)
    ones = torch.ones(B, LC)
    for kw in (dict(fused=True, cond_cache=True), dict(fused=True, cond_cache=False), dict(fused=False)):
        plain = m.edm_sampler_loop(x, y, steps=3, cfg=3.0, **kw)
        assert torch.equal(m.edm_sampler_loop(x, y, steps=3, cfg=3.0, caption_weights=ones, **kw), plain), kw
        assert torch.equal(m.edm_sampler_loop(x, y, steps=3, cfg=3.0, caption_weights=ones[0] > 0, **kw), plain), kw
        assert torch.equal(m.edm_sampler_loop(x, y, steps=3, cfg=3.0, negative=torch.zeros_like(y), **kw), plain), kw
        assert torch.equal(m.edm_sampler_loop(x, y, steps=3, cfg=3.0, negative=torch.zeros_like(y[:1]), **kw), plain), kw
        assert m.dit.engine.caption_bias is None


# ------------------------------------------------------------------------------------------------ sampler: loop parity
@pytest.mark.parametrize("sampler", ["heun", "dpmpp_2m"])
def test_loops_agree_with_weights_negative_and_an_interval(nets, sampler):
    from micro_diffusion_amd import sampling
    m, _, y, _, neg = nets["tiny"]
    x = maps_t._noise(m, 173)
    sig = sampling.sampler_plan(m.edm_config, 4, sampler).sigmas
    iv = (0.5 * (sig[-1] + min(s for s in sig if s > sig[-1])), 0.5 * (sig[0] + max(s for s in sig if s < sig[0])))   # drops the first and last level
    kw = dict(steps=4, cfg=3.0, sampler=sampler, guidance_interval=iv, caption_weights=_weights(7), negative=neg, negative_weights=_weights(8))
    a = m.edm_sampler_loop(x, y, fused=True, cond_cache=False, **kw)
    b = m.edm_sampler_loop(x, y, fused=False, **kw)
    rel = _rel(a, b)
    plain = m.edm_sampler_loop(x, y, steps=4, cfg=3.0, sampler=sampler, guidance_interval=iv, fused=True, cond_cache=False)
    print(sampler, "fused against tensor-op", rel, "against the run without prompt control", _rel(a, plain))
    assert rel < LOOP_TOL, rel
    assert _rel(a, plain) > LOOP_TOL, "prompt control must change the sample by more than the comparison resolves"
    assert torch.equal(a, m.edm_sampler_loop(x, y, fused=True, cond_cache=False, **kw)), "two runs differ"
    assert torch.isfinite(a).all() and m.dit.engine.caption_bias is None


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_cached_conditioning_gives_the_same_bits(nets, name):
    m, _, y, _, neg = nets[name]
    x = maps_t._noise(m, 175)
    kw = dict(steps=3, cfg=3.0, caption_weights=_weights(9), negative=neg, negative_weights=_weights(10))
    a = m.edm_sampler_loop(x, y, cond_cache=True, **kw)
    assert torch.equal(a, m.edm_sampler_loop(x, y, cond_cache=False, **kw))
    assert torch.equal(a, m.edm_sampler_loop(x, y, cond_cache=True, **kw))


# ------------------------------------------------------------------------------------------------ sampler: replay
def test_doubled_evaluations_carry_the_negative_prompt_and_their_own_bias_rows(nets):
    from micro_diffusion_amd import samplers
    m, _, y, _, neg = nets["micro"]
    eng, x = m.dit.engine, maps_t._noise(m, 177)
    cw, nw = _weights(11), _weights(12)
    calls, orig = [], m.dit.forward_without_cfg

    def spy(x_, t_, y_, *a, **kw):
        out = orig(x_, t_, y_, *a, **kw)
        calls.append((x_.clone(), t_.clone(), y_.clone(), a, dict(kw), eng.caption_bias, out["sample"].clone()))
        return out
    m.dit.forward_without_cfg = spy
    try:
        lat = m.edm_sampler_loop(x, y, steps=3, cfg=3.0, fused=False, caption_weights=cw, negative=neg, negative_weights=nw)
    finally:
        del m.dit.forward_without_cfg
    assert len(calls) == 5 and eng.caption_bias is None
    want = samplers.caption_bias_buffer(cw, nw, B, LC, True, "cuda")
    assert want.shape == (2 * B, 80) and not torch.equal(want[:B], want[B:])
    for x_, t_, y_, a, kw, bias, out in calls:
        assert x_.shape[0] == 2 * B and torch.equal(y_[:B], y) and torch.equal(y_[B:], neg), "the second half must be the negative prompt"
        assert torch.equal(bias.view(torch.int32), want.view(torch.int32))
    x_, t_, y_, a, kw, bias, out = calls[2]
    eng.caption_bias, eng.keep_last_tape = bias, True
    with torch.no_grad():
        again = orig(x_, t_, y_, *a, **kw)["sample"]
    assert torch.equal(again, out)
    _check_blocks_against_tape(eng, eng.last_tape, want, 2 * B, "replayed doubled evaluation")
    eng.caption_bias = None
    assert not torch.equal(lat, m.edm_sampler_loop(x, y, steps=3, cfg=3.0, fused=False))


# ------------------------------------------------------------------------------------------------ sampler: attention maps, other options
@pytest.mark.parametrize("fused", [True, False])
def test_attention_maps_record_exactly_zero_at_removed_positions(nets, fused):
    from micro_diffusion_amd.attn_maps import AttentionMaps
    m, _, y, _, neg = nets["tiny"]
    x = maps_t._noise(m, 179)
    w = torch.ones(LC)
    w[50:] = 0
    am = AttentionMaps()
    lat = m.edm_sampler_loop(x, y, steps=3, cfg=3.0, fused=fused, caption_weights=w, negative=neg, attn_maps=am)
    tm = am.token_mass()
    assert bool((tm[:, 50:] == 0).all()) and bool((tm[:, :50] > 0).all())
    assert bool((am.buf[..., 50:] == 0).all())
    torch.testing.assert_close(tm.sum(1), torch.ones(len(am.names), device="cuda", dtype=tm.dtype), rtol=2e-5, atol=0)
    for name, p in am.per_block().items():
        assert p.shape[:2] == (B, LC) and bool((p[:, 50:] == 0).all()), name
        torch.testing.assert_close(p.sum(1), torch.ones_like(p[:, 0]), rtol=2e-5, atol=0)      # every query row of every block
    assert torch.equal(lat, m.edm_sampler_loop(x, y, steps=3, cfg=3.0, fused=fused, caption_weights=w, negative=neg)), "the recorder only reads"
    assert m.dit.engine.attn_probe is None and m.dit.engine.caption_bias is None


def test_step_cache_and_inpainting_complete_and_reproduce(nets):
    from micro_diffusion_amd.step_cache import StepCache
    m, _, y, _, neg = nets["tiny"]
    x = maps_t._noise(m, 181)
    kw = dict(steps=4, cfg=3.0, caption_weights=_weights(13), negative=neg)
    a = m.edm_sampler_loop(x, y, cond_cache=True, step_cache=StepCache(interval=2), **kw)
    assert torch.isfinite(a).all() and torch.equal(a, m.edm_sampler_loop(x, y, cond_cache=True, step_cache=StepCache(interval=2), **kw))
    init = maps_t._noise(m, 183)
    mask = torch.zeros(1, 1, x.shape[2], x.shape[3], device="cuda")
    mask[..., : x.shape[2] // 2, :] = 1
    torch.manual_seed(5)
    b = m.edm_sampler_loop(x, y, init_latents=init, inpaint_mask=mask, **kw)
    torch.manual_seed(5)
    assert torch.equal(b, m.edm_sampler_loop(x, y, init_latents=init, inpaint_mask=mask, **kw))
    kept = (mask == 0).expand_as(b)
    assert torch.equal(b[kept], init[kept]) and torch.isfinite(b).all()


def test_engine_is_disarmed_after_an_error_inside_the_loop(nets):
    m, _, y, _, _ = nets["micro"]
    eng, x = m.dit.engine, maps_t._noise(m, 189)
    orig, n = m.dit.forward_without_cfg, [0]

    def failing(*a, **kw):
        n[0] += 1
        if n[0] == 2:
            assert eng.caption_bias is not None
            raise RuntimeError("boom")
        return orig(*a, **kw)
    m.dit.forward_without_cfg = failing
    try:
        with pytest.raises(RuntimeError, match="boom"):
            m.edm_sampler_loop(x, y, steps=3, cfg=3.0, cond_cache=False, caption_weights=_weights(14))
    finally:
        del m.dit.forward_without_cfg
    assert n[0] == 2 and eng.caption_bias is None


def test_negative_prompt_composes_with_measurement_guidance(nets):
    from micro_diffusion_amd.inverse import LinearMeasurement
    m, _, y, _, neg = nets["micro"]
    x = maps_t._noise(m, 191)
    meas = LinearMeasurement(torch.zeros(B, x.shape[1], x.shape[2] // 2, x.shape[3] // 2, device="cuda"), pool=2)
    a = m.edm_sampler_loop(x, y, steps=3, cfg=3.0, negative=neg, measurement=meas, cond_cache=True)
    assert torch.isfinite(a).all() and not torch.equal(a, m.edm_sampler_loop(x, y, steps=3, cfg=3.0, measurement=meas, cond_cache=True))
    with pytest.raises(ValueError, match="measurement"):
        m.edm_sampler_loop(x, y, steps=3, cfg=3.0, caption_weights=torch.ones(LC), measurement=meas)
