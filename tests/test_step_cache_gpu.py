"""Step cache on the GPU: the three kernels against exact torch references, the engine's full / reused passes against
the tape of plain passes, and the sampler under both policies.  Every kernel and engine comparison is `torch.equal`: the kernels
round once, the probe's test inputs make every sum exact, and the forward has no atomics."""
import ctypes
import math

import pytest
import torch

from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


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


# ------------------------------------------------------------------------------------------------ md_residual_delta
def _delta_sizes(hip):
    one_sweep = hip.STEP_DELTA_MAX_BLOCKS * 256          # 16-byte work items of a single sweep of the largest grid
    return [8, 8 * (256 + 3), 8 * (one_sweep + 3 * 256 + 5)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_residual_delta_is_the_rounded_difference_and_add_applies_it(hip, which):
    n = _delta_sizes(hip)[which]
    L = hip.lib()
    g = torch.Generator().manual_seed(3 + which)
    x_out = (torch.randn(n, generator=g) * 3).to(BF16).cuda()
    x_in = (torch.randn(n, generator=g) * 3).to(BF16).cuda()
    delta = torch.full((n + 8,), 7.0, device="cuda", dtype=BF16)         # one guard vector behind the output
    hip.check(L.md_residual_delta(x_out.data_ptr(), x_in.data_ptr(), delta.data_ptr(), n, _st()), "md_residual_delta")
    want = (x_out.float() - x_in.float()).bfloat16()
    assert torch.equal(delta[:n], want)
    assert (delta[n:] == 7.0).all(), "wrote behind the last element"
    assert want.float().abs().max() > 0
    x = torch.full((n + 8,), 5.0, device="cuda", dtype=BF16)
    hip.check(L.md_add_bf16(x_in.data_ptr(), delta.data_ptr(), x.data_ptr(), n, _st()), "md_add_bf16")
    assert torch.equal(x[:n], (x_in.float() + want.float()).bfloat16()) and (x[n:] == 5.0).all()


def test_residual_delta_refuses_bad_arguments_and_writes_nothing(hip):
    L = hip.lib()
    a, b = torch.ones(16, device="cuda", dtype=BF16), torch.ones(16, device="cuda", dtype=BF16)
    d = torch.full((16,), 7.0, device="cuda", dtype=BF16)
    assert L.md_residual_delta(a.data_ptr(), b.data_ptr(), d.data_ptr(), 12, _st()) == -1
    assert L.md_residual_delta(a.data_ptr(), b.data_ptr(), a.data_ptr(), 16, _st()) == -1
    assert L.md_residual_delta(a.data_ptr(), b.data_ptr(), b.data_ptr(), 16, _st()) == -1
    assert L.md_residual_delta(None, b.data_ptr(), d.data_ptr(), 16, _st()) == -1
    torch.cuda.synchronize()
    assert (d == 7.0).all() and (a == 1.0).all() and (b == 1.0).all()


# ------------------------------------------------------------------------------------------------ md_step_probe / _finish
def _grid_values(B, per, seed):
    """k / 64 with |k| <= 255: exact in bf16, every difference exact in fp32, every sum exact in fp64 in any order."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-255, 256, (B, per), generator=g).float() / 64).to(BF16)


def _probe(hip, x, ref_store, B, per):
    L = hip.lib()
    need = ctypes.c_int64(0)
    hip.check(L.md_step_probe_ws_doubles(B, per, ctypes.byref(need)), "md_step_probe_ws_doubles")
    ws = torch.full((need.value + 4,), -3.0, device="cuda", dtype=torch.float64)
    rel = torch.full((B + 1,), -1.0, device="cuda")
    rel_max = torch.full((2,), -1.0, device="cuda")
    hip.check(L.md_step_probe(x.data_ptr(), ref_store.data_ptr(), B, per, ws.data_ptr(), _st()), "md_step_probe")
    hip.check(L.md_step_probe_finish(ws.data_ptr(), B, rel.data_ptr(), rel_max.data_ptr(), _st()), "md_step_probe_finish")
    assert (ws[need.value:] == -3.0).all() and rel[B] == -1.0 and rel_max[1] == -1.0, "wrote behind a result"
    return rel[:B], rel_max[:1]


@pytest.mark.parametrize("B, per", [(3, 8 * 37), (2, 8 * (3 * 1024 + 5))])       # one ragged workgroup per sample; four, the last ragged
def test_step_probe_is_exact_and_moves_the_reference(hip, B, per):
    assert B == 3 or per // 8 > 3 * hip.STEP_PROBE_CHUNKS, "the second shape spans several workgroups per sample"
    x, ref = _grid_values(B, per, 5), _grid_values(B, per, 6)
    if B == 3:
        ref[1] = x[1]                               # identical to its reference: rel = 0
        ref[2] = 0                                  # a zero reference: +inf
        assert x[2].float().abs().sum() > 0
    x, ref = x.cuda(), ref.cuda()
    store = torch.full((B * per + 8,), 7.0, device="cuda", dtype=BF16)    # one guard vector behind ref
    store[:B * per] = ref.flatten()
    rel, rel_max = _probe(hip, x, store, B, per)
    want = ((x.float() - ref.float()).abs().double().sum(1) / ref.float().abs().double().sum(1)).float()
    assert torch.equal(rel, want), (rel, want)
    assert torch.equal(rel_max, want.max().reshape(1))
    assert torch.equal(store[:B * per].view(B, per), x), "ref was not overwritten with x"
    assert (store[B * per:] == 7.0).all(), "wrote behind ref"
    if B == 3:
        assert rel[1] == 0 and rel[2] == math.inf and rel_max[0] == math.inf and 0 < rel[0] < math.inf
    else:
        assert (rel > 0).all() and torch.isfinite(rel).all()
    # the reference now is x: a second probe of the same x measures nothing, of another x the distance from the first
    rel, rel_max = _probe(hip, x, store, B, per)
    assert (rel == 0).all() and rel_max[0] == 0
    x2 = _grid_values(B, per, 7).cuda()
    rel, rel_max = _probe(hip, x2, store, B, per)
    want = ((x2.float() - x.float()).abs().double().sum(1) / x.float().abs().double().sum(1)).float()
    assert torch.equal(rel, want) and torch.equal(rel_max, want.max().reshape(1))


def test_step_probe_refuses_bad_arguments_and_writes_nothing(hip):
    L = hip.lib()
    x, ref = torch.ones(2, 16, device="cuda", dtype=BF16), torch.full((2, 16), 3.0, device="cuda", dtype=BF16)
    ws = torch.full((16,), -3.0, device="cuda", dtype=torch.float64)
    assert L.md_step_probe(x.data_ptr(), ref.data_ptr(), 2, 12, ws.data_ptr(), _st()) == -1
    assert L.md_step_probe(x.data_ptr(), x.data_ptr(), 2, 16, ws.data_ptr(), _st()) == -1
    assert L.md_step_probe(x.data_ptr(), ref.data_ptr(), 0, 16, ws.data_ptr(), _st()) == -1
    assert L.md_step_probe(x.data_ptr(), ref.data_ptr(), 2, 16, None, _st()) == -1
    torch.cuda.synchronize()
    assert (ref == 3.0).all() and (ws == -3.0).all()


# ------------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def net(hip):
    """(model, inputs, and the out_tok / block inputs / xlast / before_segment log of plain passes at two (x, t)): computed once, only read."""
    cfg = orc.tiny_config()
    m = _model(cfg, 47)
    g = torch.Generator().manual_seed(13)
    xs = [torch.randn(2, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda() for _ in range(2)]
    y = torch.randn(2, 1, 77, cfg.caption_channels, generator=g).cuda().contiguous()
    ts = [torch.tensor([0.4, -0.2], device="cuda"), torch.tensor([-1.1, 0.9], device="cuda")]
    m.dit.refresh_shadow()
    eng = m.dit.engine
    assert len(eng.mixer) >= 1 and len(eng.backbone) >= 2
    plain = []
    eng.keep_last_tape = True
    try:
        for x, t in zip(xs, ts):
            log = []
            eng.before_segment = log.append
            tp = eng.forward(x, t, y)
            plain.append({"out": tp.out_tok.clone(), "xin": [bt.x.clone() for bt in tp.blocks], "xlast": tp.xlast.clone(), "log": log})
    finally:
        eng.keep_last_tape, eng.before_segment, eng.last_tape = False, None, None
    return m, xs, ts, y, plain


def test_full_evaluation_with_a_step_cache_is_neutral(net):
    from micro_diffusion_amd.engine import ResidualCache
    m, xs, ts, y, plain = net
    eng = m.dit.engine
    for probe in (False, True):
        rc = ResidualCache(probe=probe)
        for x, t, p in zip(xs, ts, plain):
            assert torch.equal(eng.forward(x, t, y, step_cache=rc).out_tok, p["out"])
            assert rc.valid(2, eng.cfg.tokens, eng.weights_version) and not rc.valid(3, eng.cfg.tokens, eng.weights_version)
        assert rc.nbytes == (2 if probe else 1) * 2 * 2 * eng.cfg.tokens * eng.cfg.dim
    cond = m.dit.encode_condition(y)
    assert torch.equal(eng.forward(xs[0], ts[0], None, cond=cond, step_cache=ResidualCache()).out_tok, plain[0]["out"])


@pytest.mark.parametrize("sub_range", [False, True])
def test_reused_evaluation_adds_the_cached_delta_and_skips_the_blocks(net, sub_range):
    from micro_diffusion_amd.engine import ResidualCache
    m, xs, ts, y, plain = net
    eng = m.dit.engine
    n = len(eng.backbone)
    lo, hi = (1, n) if sub_range else (0, n)
    rc = ResidualCache(blocks=(1, n)) if sub_range else ResidualCache()
    A, B_ = plain
    eng.keep_last_tape = True
    try:
        tpA = eng.forward(xs[0], ts[0], y, step_cache=rc)                       # full, at (x1, t1)
        assert (rc.lo, rc.hi) == (lo, hi)
        xin_A, xout_A = tpA.blocks[lo].x, tpA.xlast
        assert torch.equal(xin_A, A["xin"][lo]) and torch.equal(xout_A, A["xlast"])
        assert torch.equal(rc.delta, (xout_A.float() - xin_A.float()).bfloat16())
        log = []
        eng.before_segment = log.append
        tpR = eng.forward(xs[1], ts[1], y, step_cache=rc, reuse=True)           # reused, at (x2, t2)
    finally:
        eng.keep_last_tape, eng.before_segment, eng.last_tape = False, None, None
    want = (B_["xin"][lo].float() + (xout_A.float() - xin_A.float()).bfloat16().float()).bfloat16()
    assert torch.equal(tpR.xlast, want)
    skipped = {bp.name for bp in eng.backbone[lo:hi]}
    assert skipped and not skipped & set(log)
    assert log == [name for name in B_["log"] if name not in skipped], "every other segment is announced, in order"
    assert len(tpR.blocks) == n - (hi - lo) and tpR.reused
    assert not torch.equal(tpR.out_tok, B_["out"])
    assert torch.isfinite(tpR.out_tok.float()).all()
    # the cache is only read: a second reuse gives the same bits, and a full pass at (x2, t2) still equals the plain one
    assert torch.equal(eng.forward(xs[1], ts[1], y, step_cache=rc, reuse=True).out_tok, tpR.out_tok)
    assert torch.equal(eng.forward(xs[1], ts[1], y, step_cache=rc).out_tok, B_["out"])


def test_reuse_runs_no_backbone_gemm_and_no_kv_linear(net):
    from micro_diffusion_amd.engine import ResidualCache
    m, xs, ts, y, _ = net
    eng = m.dit.engine
    rc = ResidualCache()
    eng.forward(xs[0], ts[0], y, step_cache=rc)
    names, orig = [], eng.lin_fwd

    def spy(x_, wname, *a, **k):
        names.append(wname)
        return orig(x_, wname, *a, **k)
    eng.lin_fwd = spy
    try:
        eng.forward(xs[1], ts[1], y, step_cache=rc, reuse=True)
    finally:
        del eng.lin_fwd
    backbone = tuple(bp.name + "." for bp in eng.backbone)
    assert not [w for w in names if w.startswith(backbone)], "a backbone block launched a GEMM"
    assert any(w.startswith(eng.mixer[0].name + ".") for w in names) and "final_layer.linear" in names


def test_decision_callback_sees_the_probe_between_mixer_and_backbone(net):
    from micro_diffusion_amd.engine import ResidualCache
    m, xs, ts, y, plain = net
    eng = m.dit.engine
    rc = ResidualCache(probe=True)
    seen, log = [], []

    def decide(reuse):
        def cb(rel_max):
            seen.append(None if rel_max is None else float(rel_max.item()))
            log.append("decision")
            return reuse
        return cb
    eng.before_segment = log.append
    try:
        eng.forward(xs[0], ts[0], y, step_cache=rc, reuse=decide(False))
        eng.forward(xs[1], ts[1], y, step_cache=rc, reuse=decide(True))
        eng.forward(xs[1], ts[1], y, step_cache=rc, reuse=decide(False))
    finally:
        eng.before_segment = None
    assert seen[0] is None, "the first probe only fills the reference"
    A, B_ = plain[0]["xin"][0].view(2, -1).float(), plain[1]["xin"][0].view(2, -1).float()
    want = ((B_ - A).abs().double().sum(1) / A.abs().double().sum(1)).max().item()
    assert 0 < seen[1] < math.inf and abs(seen[1] - want) <= 1e-6 * want        # (fp64 sums of random data: order-dependent last bits)
    assert seen[2] == 0.0, "the same backbone input again"
    i = log.index("decision")
    assert log[i - 1] == eng.mixer[-1].name and log[i + 1] == eng.backbone[0].name
    rc.reset()
    eng.forward(xs[0], ts[0], y, step_cache=rc, reuse=decide(False))
    assert seen[3] is None and not rc.valid(3, eng.cfg.tokens, eng.weights_version)


def test_step_cache_refusals(hip):
    from micro_diffusion_amd.engine import ResidualCache
    cfg = orc.tiny_config()
    m = _model(cfg, 48)
    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda()
    x3 = torch.randn(3, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda()
    y = torch.randn(2, 1, 77, cfg.caption_channels, generator=g).cuda().contiguous()
    y3 = torch.randn(3, 1, 77, cfg.caption_channels, generator=g).cuda().contiguous()
    t = torch.tensor([0.1], device="cuda")
    m.dit.refresh_shadow()
    eng = m.dit.engine
    rc = ResidualCache()
    with pytest.raises(RuntimeError, match="empty cache"):
        eng.forward(x, t, y, step_cache=rc, reuse=True)
    with pytest.raises(RuntimeError, match="empty cache"):
        eng.forward(x, t, y, step_cache=rc, reuse=lambda rel_max: True)
    eng.forward(x, t, y, step_cache=rc)
    eng.forward(x, t, y, step_cache=rc, reuse=True)
    with pytest.raises(RuntimeError, match="batch 2"):
        eng.forward(x3, t, y3, step_cache=rc, reuse=True)
    for kwargs in (dict(record_tape=True), dict(mask_ratio=0.5, mask_noise=torch.rand(2, eng.cfg.tokens, device="cuda"))):
        with pytest.raises(RuntimeError, match="inference-only"):
            eng.forward(x, t, y, step_cache=rc, **kwargs)
    with pytest.raises(RuntimeError, match="inference-only"):
        eng.forward(x, t, None, cond=m.dit.encode_condition(y), step_cache=rc, input_tape=True)
    with pytest.raises(ValueError, match="needs a step_cache"):
        eng.forward(x, t, y, reuse=True)
    with pytest.raises(ValueError, match="outside the backbone"):
        eng.forward(x, t, y, step_cache=ResidualCache(blocks=(1, len(eng.backbone) + 1)))
    # the weights change behind the parameters' version counters: the forced refresh invalidates the cache
    eng.forward(x, t, y, step_cache=rc, reuse=True)
    next(iter(m.dit.parameters())).data.add_(0.01)
    m.dit.refresh_shadow(force=True)
    with pytest.raises(RuntimeError, match="weight version"):
        eng.forward(x, t, y, step_cache=rc, reuse=True)
    eng.forward(x, t, y, step_cache=rc)
    eng.forward(x, t, y, step_cache=rc, reuse=True)


# ------------------------------------------------------------------------------------------------ the sampler
STEPS, CFG = 5, 3.0


@pytest.fixture(scope="module")
def run(hip):
    """(sample(**kwargs) -> latents, the plain results by sampler): one model, the references computed once."""
    cfg = orc.tiny_config()
    model = _model(cfg, 41)
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(2, 4, 32, 32, generator=g).cuda()
    y = torch.randn(2, 1, 77, 1024, generator=g).cuda()

    def sample(**kwargs):
        kwargs.setdefault("cond_cache", True)
        return model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, **kwargs)
    plain = {s: sample(sampler=s) for s in ("heun", "euler", "dpmpp_2m")}
    return sample, plain


def test_policies_that_never_reuse_give_the_plain_bits(run):
    from micro_diffusion_amd.step_cache import StepCache
    sample, plain = run
    for sc in (StepCache(interval=1), StepCache(threshold=0.0)):
        for cond_cache in (True, False):
            assert torch.equal(sample(step_cache=sc, cond_cache=cond_cache), plain["heun"])
            assert sc.stats.decisions == [True] * 9 and sc.stats.reused == 0
    assert torch.equal(sample(cond_cache=False), plain["heun"])


def test_interval_two_follows_the_plan_with_and_without_cond_cache(run):
    from micro_diffusion_amd.step_cache import StepCache
    sample, plain = run
    sc = StepCache(interval=2)
    a = sample(step_cache=sc)
    assert sc.stats == sc.plan(9) and sc.stats.reused == 4 and sc.stats.distances == [None] * 9
    assert torch.isfinite(a).all() and not torch.equal(a, plain["heun"])
    b = sample(step_cache=sc, cond_cache=False)
    assert sc.stats == sc.plan(9), "the second run starts from a reset policy"
    assert torch.equal(a, b)


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
def test_interval_two_with_the_one_evaluation_solvers(run, sampler):
    from micro_diffusion_amd.step_cache import StepCache
    sample, plain = run
    sc = StepCache(interval=2)
    a = sample(step_cache=sc, sampler=sampler)
    assert sc.stats == sc.plan(5) and sc.stats.decisions == [True, False, True, False, True]
    assert torch.isfinite(a).all() and not torch.equal(a, plain[sampler])


def test_a_guidance_interval_that_ends_inside_the_run_forces_a_full_evaluation(run):
    from micro_diffusion_amd import samplers
    from micro_diffusion_amd.step_cache import StepCache
    sample, _ = run
    t = samplers.edm_schedule(STEPS)
    sig = samplers.evaluation_sigmas("heun", t)
    lo = math.sqrt(t[2] * t[3])                     # guided (batch 2B) down to t_2, the conditional half alone (batch B) from t_3 on
    guided = [s >= lo for s in sig]
    switch = guided.index(False)
    assert switch == 5 and all(guided[:switch]) and not any(guided[switch:])
    sc = StepCache(interval=2)
    assert sc.plan(9).decisions[switch] is False, "the schedule alone would reuse there"
    a = sample(step_cache=sc, guidance_interval=(lo, 100.0))
    valid = [e != switch for e in range(9)]
    assert sc.stats.decisions[switch] is True
    assert sc.stats == sc.plan(9, valid=valid)
    assert torch.isfinite(a).all()


def test_adaptive_decisions_replay_from_the_recorded_distances(run):
    from micro_diffusion_amd.step_cache import StepCache
    sample, plain = run
    probe = StepCache(threshold=0.0)                # every evaluation full: the distances of the plain trajectory
    sample(step_cache=probe)
    d = probe.stats.distances
    assert d[0] is None and all(isinstance(v, float) and 0 < v < math.inf for v in d[1:])
    sc = StepCache(threshold=1.5 * max(d[1:]))      # finite, and above every single distance: the evaluation after a full one is reused
    a = sample(step_cache=sc)
    s = sc.stats
    assert s.decisions == sc.plan(9, distances=s.distances).decisions
    assert s.decisions[0] and s.decisions[-1] and s.decisions[1] is False and s.reused >= 1
    assert s.distances[0] is None and s.distances[1] == d[1], "the first two evaluations are those of the plain trajectory"
    assert torch.isfinite(a).all() and not torch.equal(a, plain["heun"])


def test_inpainting_repetitions_are_counted_and_a_guidance_mode_composes(run):
    """img2img + inpainting + RePaint resampling under "apg": the loop counts every repetition's evaluation (samplers.edit_evaluations),
    the policy follows its plan for that count, and the kept region still comes back as init_latents bit for bit."""
    from micro_diffusion_amd import samplers
    from micro_diffusion_amd.step_cache import StepCache
    sample, _ = run
    g = torch.Generator().manual_seed(21)
    init = torch.randn(2, 4, 32, 32, generator=g).cuda()
    mask = torch.zeros(1, 1, 32, 32, device="cuda")
    mask[..., 8:24, 8:24] = 1
    sc = StepCache(interval=2)
    a = sample(step_cache=sc, sampler="euler", init_latents=init, strength=0.6, inpaint_mask=mask, resample=2, guidance_mode="apg",
               apg_norm_threshold=15.0)
    n = samplers.edit_evaluations("euler", STEPS, 0.6, 2)
    assert n == 5 and sc.stats == sc.plan(n) and sc.stats.reused == 2
    assert torch.isfinite(a).all()
    keep = (mask == 0).expand_as(a)
    assert torch.equal(a[keep], init[keep])


def test_sampler_refusals(run):
    from micro_diffusion_amd.step_cache import StepCache
    sample, _ = run
    sc = StepCache(interval=2)
    with pytest.raises(ValueError, match="guide"):
        sample(step_cache=sc, guide=object())
    with pytest.raises(ValueError, match="guidance_loss"):
        sample(step_cache=sc, guidance_loss=lambda D: D.flatten(1).sum(1))
    with pytest.raises(ValueError, match="fused"):
        sample(step_cache=sc, fused=False, cond_cache=False)
