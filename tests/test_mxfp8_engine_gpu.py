"""MXFP8 sampling through the engine and the sampler: Tiny widths, B = 2 and 3, 8 x 8 latents (16 tokens).

What is exact here is exact (torch.equal): nothing targeted gives the plain forward, one targeted linear equals the stand-alone kernel
calls, cond_cache on and off agree, a plain run after an MX run has the bits of one before it.  The whole forward against the bf16
forward is held to a relative L2 below 0.5: a wiring condition (an unrelated output sits near sqrt 2), not an accuracy claim --
accuracy is asserted per linear in tests/test_mxfp8_kernels_gpu.py."""
import os

import pytest
import torch

from oracle import microdit_ref as orc

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def model():
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    cfg = orc.tiny_config(input_size=8)
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(orc.synth_state_dict(cfg, 3))
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=cfg.input_size)
    m.eval()
    return m


@pytest.fixture(scope="module")
def mx(model):
    from micro_diffusion_amd.mxfp8 import ALL_TARGETS, MXWeights
    return MXWeights(model.dit, targets=ALL_TARGETS)


def _inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, 8, 8, generator=g).cuda()
    t = (torch.rand(B, generator=g) * 2 + 0.1).cuda()
    y = torch.randn(B, 1, 77, 1024, generator=g).cuda().contiguous()
    return x, t, y


def _forward(model, B, mx=None, log=None, seed=0):
    eng = model.dit.engine
    x, t, y = _inputs(B, seed)
    eng.mx, eng.mx_log = mx, log
    try:
        with torch.no_grad():
            return model.dit.forward_without_cfg(x, t, y)["sample"].clone()
    finally:
        eng.mx, eng.mx_log = None, None


@pytest.mark.parametrize("B", (2, 3))
def test_mx_log_names_every_targeted_linear_once(model, mx, B):
    from micro_diffusion_amd import mxfp8
    assert mx.entries and not mx.skipped, mx.skipped               # every Tiny width is eligible (K % 128 == 0, N % 16 == 0)
    log = []
    out = _forward(model, B, mx, log)
    assert bool(torch.isfinite(out).all())
    ran_mx = [n for n, how in log if how == "mx"]
    ran_bf16 = [n for n, how in log if how == "bf16"]
    targeted = set(mxfp8.target_names(model.dit.config, mxfp8.ALL_TARGETS))
    # a fused [w1; w2] runs (and is logged) under the name of w1
    expect = sorted(n for n in targeted if n in mx.entries)
    assert sorted(ran_mx) == expect, (sorted(set(expect) ^ set(ran_mx)))
    assert len(set(ran_mx)) == len(ran_mx)
    assert ran_bf16 and not (set(ran_bf16) & targeted)
    for n in ran_bf16:                                             # what stays bf16 is outside the quantisable set: adaLN, the MoE gate,
        assert not mxfp8._QUANTISABLE.match(n), n                  # the caption side, the embedders, the mixer's maps, the final layer
    assert any(".gate" in n for n in ran_bf16) and any("kv_linear" in n for n in ran_bf16)
    plain_log = []
    _forward(model, B, None, plain_log)
    assert plain_log and all(how == "bf16" for _, how in plain_log) and len(plain_log) == len(log)


def test_nothing_targeted_gives_the_plain_forward(model):
    from micro_diffusion_amd.mxfp8 import MXWeights
    none = MXWeights(model.dit, targets=r"$^")
    assert not none.entries and none.nbytes == 0
    assert torch.equal(_forward(model, 2, none), _forward(model, 2))


def test_one_half_of_a_stacked_pair_is_skipped_and_takes_no_memory(model):
    from micro_diffusion_amd.mxfp8 import MXWeights
    eng = model.dit.engine
    pre = next(bp.name for bp in eng.mixer + eng.backbone if not bp.moe) + ".mlp"
    assert eng._fused12(pre)
    half = MXWeights(model.dit, targets="^" + pre.replace(".", r"\.") + r"\.w1$")
    assert half.skipped == [pre + ".w1"] and not half.entries and half.nbytes == 0
    log = []
    assert torch.equal(_forward(model, 2, half, log), _forward(model, 2))
    assert (pre + ".w1", "bf16") in log


def test_one_targeted_linear_equals_the_standalone_kernels(model):
    from micro_diffusion_amd import hip
    from micro_diffusion_amd.mxfp8 import MXWeights
    eng = model.dit.engine
    name = eng.mixer[0].name
    one = MXWeights(model.dit, targets="^" + name.replace(".", r"\.") + r"\.attn\.proj$")
    assert list(one.entries) == [name + ".attn.proj"]
    eng.keep_last_tape = True
    try:
        _forward(model, 2, one)
        t = eng.last_tape.mixer[0]
    finally:
        eng.keep_last_tape, eng.last_tape = False, None
    ent = one.entries[name + ".attn.proj"]
    M, K, N = t.sa.o.shape[0], ent.K, ent.N
    S = M // 2
    q = torch.empty(M, K, dtype=torch.uint8, device="cuda")
    sc = torch.empty(M, K // 32, dtype=torch.uint8, device="cuda")
    hip.mx_quant_rows(t.sa.o, q, sc, M, K, ld=K, ldd=K, lds=K // 32)
    x1 = torch.empty(M, N, dtype=BF16, device="cuda")
    br1 = torch.empty(M, N, dtype=BF16, device="cuda")
    hip.gemm_mxfp8(q, sc, ent.q, ent.s, x1, M, N, K, lda=K, ldb=K, ldsa=K // 32, ldsb=K // 32, ldc=N, mode=hip.EPI_RESIDUAL,
                   bias=eng.P.get(name + ".attn.proj.bias"), res=t.x, ldr=N, gate=t.mp + 2 * 2 * N, ldg=t.ldm, rows_per_sample=S,
                   C2=br1, ldc2=N)
    torch.cuda.synchronize()
    assert torch.equal(br1, t.br1) and torch.equal(x1, t.x1)
    assert bool((x1 != t.x).any())


def test_mx_expert_block_leaves_no_unwritten_buffer_on_the_tape(model, mx):
    eng = model.dit.engine
    eng.keep_last_tape, eng.poison = True, True
    try:
        _forward(model, 2, mx)
        moe = [t for t in eng.last_tape.mixer + eng.last_tape.blocks if getattr(t, "hact", None) is not None]
    finally:
        eng.keep_last_tape, eng.last_tape, eng.poison = False, None, os.environ.get("MD_POISON", "0") == "1"
    assert moe and all(t.hpre is None and bool(torch.isfinite(t.hact.float()).all()) for t in moe)


def test_poisoned_allocations_stay_finite(model, mx):
    eng = model.dit.engine
    eng.poison = True
    try:
        out = _forward(model, 3, mx)
    finally:
        eng.poison = os.environ.get("MD_POISON", "0") == "1"
    assert bool(torch.isfinite(out).all())


def test_whole_forward_stays_near_the_bf16_forward(model, mx):
    a, b = _forward(model, 3, mx).double(), _forward(model, 3).double()
    rel = float((a - b).norm() / b.norm())
    print(f"MXFP8 forward against bf16 forward, Tiny, B = 3: relative L2 {rel:.4f}")
    assert 0.0 < rel < 0.5


def test_refused_with_a_tape_and_under_gradients(model, mx):
    eng = model.dit.engine
    x, t, y = _inputs(2)
    eng.mx = mx
    try:
        with pytest.raises(RuntimeError, match="inference-only"):
            eng.forward(x, t, y, record_tape=True)
        with pytest.raises(RuntimeError, match="inference-only"):
            model.dit.forward_without_cfg(x.requires_grad_(True), t, y)
    finally:
        eng.mx = None


# ------------------------------------------------------------------------------------------------------------------ sampler
STEPS, CFG = 4, 3.0


def _noise(B=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4, 8, 8, generator=g).cuda(), torch.randn(B, 1, 77, 1024, generator=g).cuda()


def test_sampler_cond_cache_on_and_off_agree_and_disarm(model, mx):
    lat, y = _noise()
    eng = model.dit.engine
    plain_before = model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG)
    on = model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, cond_cache=True, mxfp8=mx)
    assert eng.mx is None
    off = model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, cond_cache=False, mxfp8=mx)
    assert torch.equal(on, off) and bool(torch.isfinite(on).all())
    assert not torch.equal(on, plain_before)
    from micro_diffusion_amd import mxfp8
    made_here = model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, mxfp8=True)      # True: the default targets, quantised for the run
    assert torch.equal(made_here, on if mxfp8.target_names(model.dit.config) else plain_before) and eng.mx is None
    tensor_ops = model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, fused=False, mxfp8=mx)   # the other loop arms it too
    assert eng.mx is None and not torch.equal(tensor_ops, model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, fused=False))
    assert torch.equal(model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG), plain_before)   # a plain run after MX runs: its old bits


def test_sampler_step_cache_and_inpainting_run(model, mx):
    from micro_diffusion_amd.step_cache import StepCache
    lat, y = _noise(seed=2)
    out = model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, step_cache=StepCache(interval=2), mxfp8=mx)
    assert bool(torch.isfinite(out).all()) and model.dit.engine.mx is None
    g = torch.Generator().manual_seed(5)
    init = torch.randn(2, 4, 8, 8, generator=g).cuda()
    mask = torch.zeros(1, 1, 8, 8, device="cuda")
    mask[..., :, 4:] = 1
    out = model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, init_latents=init, inpaint_mask=mask, sampler="euler", mxfp8=mx)
    assert bool(torch.isfinite(out).all())
    assert torch.allclose(out[..., :, :4].double(), init[..., :, :4].double(), atol=1e-5)


def test_sampler_disarms_after_an_exception(model, mx):
    lat, y = _noise()
    eng = model.dit.engine
    calls = []

    def boom(*a, **k):
        calls.append(eng.mx)
        raise ZeroDivisionError("inside the run")

    orig = eng._forward
    eng._forward = boom
    try:
        with pytest.raises(ZeroDivisionError):
            model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, mxfp8=mx)
    finally:
        eng._forward = orig
    assert calls and calls[0] is mx and eng.mx is None


def test_sampler_refuses_measurement_and_stale_weights(model):
    from micro_diffusion_amd.mxfp8 import MXWeights
    lat, y = _noise()
    with pytest.raises(ValueError, match="measurement"):
        model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, mxfp8=True, guidance_loss=lambda d: d.flatten(1).pow(2).sum(1))
    stale = MXWeights(model.dit, targets=r"attn\.qkv$")
    before = {k: (e.q.data_ptr(), e.s.data_ptr()) for k, e in stale.entries.items()}
    model.dit.refresh_shadow(force=True)
    with pytest.raises(RuntimeError, match="MXWeights mismatch"):
        model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, mxfp8=stale)
    assert model.dit.engine.mx is None
    stale.requantize()                                                         # in place: same buffers, current version
    assert before == {k: (e.q.data_ptr(), e.s.data_ptr()) for k, e in stale.entries.items()}
    assert stale.nbytes == sum(e.N * e.K * e.batch * 33 // 32 for e in stale.entries.values())
    out = model.edm_sampler_loop(lat, y, steps=STEPS, cfg=CFG, mxfp8=stale)
    assert bool(torch.isfinite(out).all())
