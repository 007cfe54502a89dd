"""Image-conditioned sampling, host side (no GPU): md_edm_blend_known is declared, bound and documented, the four new
arguments default to today's behaviour and are named parameters (a name that lands in **kwargs would switch the fused loop off), the
step-count helpers agree with the table of the design, the tensor-op loop -- the definition of the feature -- keeps the known region,
moves the generated one with what surrounds it and stays closer to the known latents the lower the strength, every undefined request is
refused, and the kernel compiles for gfx950 without scratch, spill or LDS."""
import inspect
import os
import re

import pytest
import torch

from micro_diffusion_amd import samplers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "md_edm_blend_known", 10
EDIT_DEFAULTS = {"init_latents": None, "strength": 1.0, "inpaint_mask": None, "resample": 1}
N = 6


# ------------------------------------------------------------------------------------------------ the surface
def _header():
    return open(os.path.join(ROOT, "include", "microdit_hip.h")).read()


def test_entry_point_is_declared_bound_and_documented():
    from micro_diffusion_amd import hip
    header = _header()
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
    assert m, f"{NAME} is not declared in include/microdit_hip.h"
    assert NAME in hip.exported_symbols(), f"{NAME} is not bound in hip._SIGS"
    declared = [a for a in m.group(1).split(",") if a.strip()]
    restype, argtypes = hip._SIGS[NAME]
    assert len(declared) == len(argtypes) == NARGS, (len(declared), len(argtypes))
    assert declared[-1].split()[0] == "hipStream_t"
    assert "x[b,c,i] = fma(m, x[b,c,i], (1 - m) * k),  k = noise ? fma(sigma, noise[b,c,i], x0[b,c,i]) : x0[b,c,i]" in header
    assert "m = (double)mask[(mask_B == 1 ? 0 : b), i]" in header
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6, "one symbol added, none changed: the ABI version stays"
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_new_arguments_default_to_today_and_are_named_parameters():
    from micro_diffusion_amd.model import LatentDiffusion
    for fn in (LatentDiffusion.edm_sampler_loop, LatentDiffusion.generate):
        p = inspect.signature(fn).parameters
        names = list(p)
        var_kw = [k for k, v in p.items() if v.kind is inspect.Parameter.VAR_KEYWORD]
        assert var_kw == ["kwargs"]
        for name, default in EDIT_DEFAULTS.items():
            assert name in p, f"{fn.__name__}: {name} would land in **kwargs and switch the fused loop off"
            assert p[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and names.index(name) < names.index("kwargs")
            assert p[name].default == default and type(p[name].default) is type(default), (fn.__name__, name, p[name].default)


# ------------------------------------------------------------------------------------------------ the helpers
def test_start_index():
    assert samplers.edit_start_index(N, 1.0) == 0
    assert samplers.edit_start_index(N, 0.5) == 3
    assert samplers.edit_start_index(N, 0.17) == 4                   # ceil(1.02) = 2 steps
    assert samplers.edit_start_index(N, 1e-9) == N - 1               # at least one step runs
    assert samplers.edit_start_index(30, 0.5) == 15 and samplers.edit_start_index(30, 1 / 30) == 29
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            samplers.edit_start_index(N, bad)


def test_repetitions_and_evaluations_follow_the_table():
    t = samplers.edm_schedule(N)
    assert samplers.edit_repetitions(t, 0, 1) == [1] * N
    assert samplers.edit_repetitions(t, 0, 3) == [3] * (N - 1) + [1], "the step onto sigma = 0 runs once"
    assert samplers.edit_repetitions(t, 4, 2) == [2, 1]
    # the worked numbers of the design: n = 6
    assert [samplers.edit_evaluations("heun", N, 1.0, r) for r in (1, 2, 3)] == [11, 21, 31]
    assert [samplers.edit_evaluations("euler", N, 1.0, r) for r in (1, 2, 3)] == [6, 11, 16]
    assert samplers.edit_evaluations("heun", N, 0.5) == 5 and samplers.edit_evaluations("euler", N, 0.5) == 3
    assert samplers.edit_evaluations("dpmpp_2m", N, 0.5) == 3
    for n in (2, 6, 30):
        for strength in (1.0, 0.5, 0.17):
            k = n - samplers.edit_start_index(n, strength)
            for r in (1, 2, 4):
                assert samplers.edit_evaluations("heun", n, strength, r) == 2 * r * (k - 1) + 1
                assert samplers.edit_evaluations("euler", n, strength, r) == r * (k - 1) + 1
            assert samplers.edit_evaluations("dpmpp_2m", n, strength) == k
            assert samplers.edit_evaluations("heun", n, strength) == 2 * k - 1
    with pytest.raises(ValueError, match="history"):
        samplers.edit_evaluations("dpmpp_2m", N, 1.0, 2)
    # a default run: what evaluation_sigmas lists
    assert samplers.edit_evaluations("heun", N) == len(samplers.evaluation_sigmas("heun", t))


# ------------------------------------------------------------------------------------------------ the tensor-op loop on the CPU
B, C, H, W = 2, 4, 32, 32


def _cpu_model():
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(input_size=8, dim=64, depth=2, head_dim=32, caption_channels=32, multiple_of=32, patch_mixer_depth=1, patch_mixer_dim=64,
                 num_experts=2)
    return LatentDiffusion(d, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=8)


@pytest.fixture(scope="module")
def model():
    """A CPU LatentDiffusion whose network is the smooth stand-in of tests/test_samplers_gpu.py::smooth_model; it couples neighbours
    along w only (the roll term).  `model.calls` counts the network evaluations."""
    m = _cpu_model()
    m.calls = 0

    def smooth(x, t, y, mask_ratio=0, **kw):
        m.calls += 1
        x = x.float()
        cond = y.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)
        return {"sample": torch.tanh(0.7 * x) * (1.0 + 0.1 * t.float().view(-1, 1, 1, 1)) + 0.05 * torch.roll(x, 1, -1) + cond, "mask": None}
    m.dit.forward_without_cfg = smooth
    return m


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(10)
    x, y = torch.randn(B, C, H, W, generator=g), torch.randn(B, 1, 5, 32, generator=g)
    init = torch.randn(B, C, H, W, generator=g) * 0.5
    hole = torch.zeros(H, W)
    hole[8:24, 8:24] = 1.0                                           # centred 16 x 16 region to generate
    return x, y, init, hole


def _run(model, data, seed=3, **kw):
    x, y, init, hole = data
    kw.setdefault("init_latents", init)
    torch.manual_seed(seed)
    model.calls = 0
    return model.edm_sampler_loop(x, y, steps=N, cfg=1.0, fused=False, **kw)


def _rel(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("sampler", ["heun", "euler"])
def test_evaluation_counts(model, data, sampler):
    hole = data[3]
    for strength, resample in ((1.0, 1), (0.5, 1), (0.17, 1), (1.0, 2), (1.0, 3), (0.5, 2)):
        out = _run(model, data, sampler=sampler, strength=strength, inpaint_mask=hole, resample=resample)
        assert model.calls == samplers.edit_evaluations(sampler, N, strength, resample), (sampler, strength, resample, model.calls)
        assert torch.isfinite(out).all()
    _run(model, data, sampler="dpmpp_2m", strength=0.5)
    assert model.calls == samplers.edit_evaluations("dpmpp_2m", N, 0.5) == 3
    _run(model, data, sampler=sampler, init_latents=None)
    assert model.calls == (2 * N - 1 if sampler == "heun" else N), "the default run"


@pytest.mark.parametrize("sampler", ["heun", "euler"])
def test_the_kept_region_is_the_known_latents_bit_for_bit(model, data, sampler):
    x, y, init, hole = data
    for resample in (1, 2):
        out = _run(model, data, sampler=sampler, inpaint_mask=hole, resample=resample)
        keep = (hole == 0).expand(B, C, H, W)
        assert torch.equal(out[keep], init[keep])
        assert not torch.equal(out[~keep], init[~keep])
    assert torch.equal(_run(model, data, sampler=sampler, inpaint_mask=torch.zeros(H, W)), init), "an all-zero mask returns init_latents"
    soft = hole.clone()
    soft[8:24, 8:12] = 0.5
    out = _run(model, data, sampler=sampler, inpaint_mask=soft)
    assert torch.equal(out[(soft == 0).expand(B, C, H, W)], init[(soft == 0).expand(B, C, H, W)])


@pytest.mark.parametrize("sampler", ["heun", "euler"])
def test_an_all_ones_mask_is_the_run_without_a_mask(model, data, sampler):
    assert model.edm_config.S_churn == 0
    for strength in (1.0, 0.5):
        a = _run(model, data, sampler=sampler, strength=strength, inpaint_mask=torch.ones(H, W))
        b = _run(model, data, sampler=sampler, strength=strength)
        assert torch.equal(a, b)
    assert not torch.equal(b, _run(model, data, sampler=sampler, init_latents=None)), "init_latents must change the sample"


@pytest.mark.parametrize("sampler", ["heun", "euler"])
def test_mask_forms_agree(model, data, sampler):
    x, y, init, hole = data
    ref = _run(model, data, sampler=sampler, inpaint_mask=hole)
    for form in (hole.bool(), hole.view(1, H, W), hole.view(1, 1, H, W), hole.expand(B, H, W), hole.expand(B, 1, H, W).contiguous()):
        assert torch.equal(_run(model, data, sampler=sampler, inpaint_mask=form), ref), tuple(form.shape)
    per_sample = torch.stack([hole, torch.zeros(H, W)])              # sample 1 is kept whole
    out = _run(model, data, sampler=sampler, inpaint_mask=per_sample)
    assert torch.equal(out[1], init[1]) and torch.equal(out[0], ref[0])


@pytest.mark.parametrize("sampler", ["heun", "euler"])
def test_the_generated_region_follows_its_surroundings_along_w_only(model, data, sampler):
    """The stand-in couples along w (roll by one column), so kept columns left of the hole reach the generated region through the
    per-step blend and kept rows above it do not.  A mask applied along the wrong axis, or a blend that never ran, fails one of the two."""
    x, y, init, hole = data
    gen = (hole == 1).expand(B, C, H, W)
    ref = _run(model, data, sampler=sampler, inpaint_mask=hole)
    left = init.clone()
    left[:, :, 8:24, :8] += 1.0
    moved = _run(model, data, sampler=sampler, inpaint_mask=hole, init_latents=left)
    rel = _rel(moved[gen], ref[gen])
    print(sampler, "kept columns left of the hole move the generated region by", rel)
    assert rel > 1e-5, rel
    above = init.clone()
    above[:, :, :8, 8:24] += 1.0
    same = _run(model, data, sampler=sampler, inpaint_mask=hole, init_latents=above)
    assert torch.equal(same[gen], ref[gen])


def test_distance_to_the_known_latents_shrinks_with_strength(model, data):
    init = data[2]
    d = [_rel(_run(model, data, strength=s), init) for s in (1.0, 0.5, 0.17)]
    print("distance to init_latents at strength 1, 0.5, 0.17:", d)
    assert d[0] > d[1] > d[2] > 0


def test_new_arguments_do_not_reach_the_network(model, data):
    """edm_sampler_loop forwards **kwargs to the network and fuses only without them: the four names must stop at the sampler, at their
    defaults and at other values, and at their defaults change nothing."""
    x, y, init, hole = data
    seen, inner = [], model.dit.forward_without_cfg

    def spy(x_, t, y_, mask_ratio=0, **kw):
        seen.append(sorted(kw))
        return inner(x_, t, y_, mask_ratio, **kw)
    model.dit.forward_without_cfg = spy
    try:
        a = _run(model, data, init_latents=None)
        b = _run(model, data, init_latents=None, strength=1.0, inpaint_mask=None, resample=1)
        _run(model, data, strength=0.5, inpaint_mask=hole, resample=2)
    finally:
        model.dit.forward_without_cfg = inner
    assert torch.equal(a, b)
    assert len(seen) == 2 * (2 * N - 1) + samplers.edit_evaluations("heun", N, 0.5, 2) and all(kw == [] for kw in seen), seen


def test_strength_is_any_real_number(model, data):
    import numpy as np
    ref = _run(model, data, strength=0.5)
    for s in (np.float32(0.5), np.float64(0.5), torch.tensor(0.5)):
        assert torch.equal(_run(model, data, strength=s), ref), type(s)
    assert torch.equal(_run(model, data, strength=1), _run(model, data))
    for bad in (torch.tensor([0.5, 0.5]), "0.5", None, True, np.float32(1.5)):
        with pytest.raises(ValueError, match="strength"):
            _run(model, data, strength=bad)


# ------------------------------------------------------------------------------------------------ what is refused
def test_undefined_requests_raise(model, data):
    x, y, init, hole = data
    run = lambda **kw: model.edm_sampler_loop(x, y, steps=N, fused=False, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="strength"):
        run(strength=0.5)                                            # strength < 1 without init_latents
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            run(init_latents=init, strength=bad)
    with pytest.raises(ValueError, match="init_latents"):
        run(inpaint_mask=hole)                                       # a mask without init_latents
    with pytest.raises(ValueError, match="inpaint_mask"):
        run(init_latents=init, resample=2)                           # resampling without a mask
    with pytest.raises(ValueError, match="history"):
        run(init_latents=init, inpaint_mask=hole, resample=2, sampler="dpmpp_2m")
    for bad in (0, -1, 1.5, 2.0, True, "2"):
        with pytest.raises(ValueError, match="resample"):
            run(init_latents=init, inpaint_mask=hole, resample=bad)
    with pytest.raises(ValueError, match="shape"):
        run(init_latents=init[:, :, :16])
    with pytest.raises(ValueError, match="shape"):
        run(init_latents=init[:1])
    for bad in (torch.ones(H, W + 1), torch.ones(B + 1, H, W), torch.ones(B, C, H, W), torch.ones(H * W), torch.ones(1, 1, 1, H, W),
                torch.ones(W, H + 2)):
        with pytest.raises(ValueError, match="shape"):
            run(init_latents=init, inpaint_mask=bad)
    for bad in (hole * 1.5, hole - 0.25, torch.full((H, W), float("nan"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            run(init_latents=init, inpaint_mask=bad)
    # generate() refuses the same before it tokenises anything
    with pytest.raises(ValueError, match="strength"):
        model.generate(prompt=["a"], strength=0.5)
    with pytest.raises(ValueError, match="resample"):
        model.generate(prompt=["a"], init_latents=init, inpaint_mask=hole, resample=0)


# ------------------------------------------------------------------------------------------------ compiled resources
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_blend_kernels_compile_without_scratch_spill_or_lds(tmp_path):
    from micro_diffusion_amd import hip, native
    res = native.resource_usage("edit.hip", hip.HIPCC_FLAGS, tmp_path / "edit.o")
    assert len(res) == 2 and all("blend_known" in k for k in res), sorted(res)        # two elements per lane, and element-wise
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0 and v["spill"] == 0 and v["lds"] == 0, (k, v)
