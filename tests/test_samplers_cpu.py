"""Sampler solvers, host side (no GPU): the coefficients of `samplers.solver_coefficients` integrate an analytic problem at the order
they claim, the new entry points are declared, bound and documented, the public arguments default to today's behaviour and refuse
what is not defined, and the new kernels compile for gfx950 without scratch."""
import inspect
import math
import os
import re

import pytest
import torch

from micro_diffusion_amd import samplers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"md_edm_solver_update": 14, "md_edm_solver_update_tok": 18, "md_edm_churn": 6}
SD, SMIN, SMAX, RHO = 0.5, 0.002, 80.0, 7.0


# ------------------------------------------------------------------------------------------------ the analytic problem
def _denoiser(x, sigma):
    """E[x0 | x] for x0 ~ N(0, SD^2), x = x0 + sigma * noise."""
    return SD * SD / (SD * SD + sigma * sigma) * x


def _exact(x0):
    return x0 * math.sqrt(SD * SD / (SD * SD + SMAX * SMAX))


def _integrate(solver, n, x0=37.0):
    """(relative error at sigma = 0, evaluations, the last step's output, D(x; sigma_min) of the last step's input)."""
    t = samplers.edm_schedule(n, SMIN, SMAX, RHO)
    x, hist, evals, last = x0, 0.0, 0, None
    if solver == "heun":                                       # the reference's loop (model.py:231-297) on the scalar problem
        for i in range(n):
            tc, tn = t[i], t[i + 1]
            d = (x - _denoiser(x, tc)) / tc
            xn = x + (tn - tc) * d
            evals += 1
            if i < n - 1:
                dp = (xn - _denoiser(xn, tn)) / tn
                xn = x + (tn - tc) * (0.5 * d + 0.5 * dp)
                evals += 1
            x = xn
    else:
        coef = samplers.solver_coefficients(solver, t)
        assert len(coef) == n
        for i, (a, b, c1, c2) in enumerate(coef):
            den = _denoiser(x, t[i])
            evals += 1
            last = den
            x, hist = a * x + b * (c1 * den - c2 * hist), den
    return abs(x - _exact(x0)) / abs(_exact(x0)), evals, x, last


@pytest.fixture(scope="module")
def errs():
    return {(s, n): _integrate(s, n) for s in ("euler", "dpmpp_2m", "heun") for n in (16, 32, 64)}


def test_euler_is_first_order(errs):
    ratio = errs["euler", 32][0] / errs["euler", 64][0]
    print("euler", [errs["euler", n][0] for n in (16, 32, 64)], ratio)
    assert 1.8 <= ratio <= 2.2, ratio


def test_dpmpp_2m_is_second_order_and_beats_euler(errs):
    e = [errs["dpmpp_2m", n][0] for n in (16, 32, 64)]
    print("dpmpp_2m", e, e[1] / e[2])
    assert e[1] / e[2] >= 3.5, e
    for n in (16, 32, 64):
        assert errs["dpmpp_2m", n][0] < errs["euler", n][0], n


def test_dpmpp_2m_matches_heun_with_half_the_evaluations(errs):
    m, h = errs["dpmpp_2m", 64], errs["heun", 64]
    print("2M", m[:2], "heun", h[:2])
    assert (m[1], h[1]) == (64, 127)
    assert m[0] <= 1.1 * h[0], (m[0], h[0])


@pytest.mark.parametrize("solver", ["euler", "dpmpp_2m"])
def test_last_step_returns_the_denoised_value_exactly(errs, solver):
    for n in (16, 32, 64):
        _, _, x, last = errs[solver, n]
        assert x == last
    assert samplers.solver_coefficients(solver, samplers.edm_schedule(5))[-1] == (0.0, 1.0, 1.0, 0.0)


def test_coefficient_forms():
    t = samplers.edm_schedule(6)
    eu, m2 = samplers.solver_coefficients("euler", t), samplers.solver_coefficients("dpmpp_2m", t)
    for i in range(5):
        assert eu[i] == (t[i + 1] / t[i], 1.0 - t[i + 1] / t[i], 1.0, 0.0)
    assert m2[0][2:] == (1.0, 0.0), "the first 2M step has no history"
    for i in range(1, 5):
        a, b, c1, c2 = m2[i]
        h = math.log(t[i] / t[i + 1])
        r = math.log(t[i - 1] / t[i]) / h
        assert a == t[i + 1] / t[i] and b == pytest.approx(1.0 - math.exp(-h), rel=1e-14)
        assert c2 == pytest.approx(1 / (2 * r), rel=1e-12) and c1 == pytest.approx(1.0 + c2, rel=1e-15) and c2 > 0
    # a churned step starts from t_hat (euler); a history-carrying solver cannot
    hats = [1.2 * v for v in t[:-1]]
    assert samplers.solver_coefficients("euler", t, hats)[0] == (t[1] / hats[0], 1.0 - t[1] / hats[0], 1.0, 0.0)
    with pytest.raises(ValueError):
        samplers.solver_coefficients("dpmpp_2m", t, hats)
    with pytest.raises(ValueError):
        samplers.solver_coefficients("heun", t)


def test_schedule_matches_the_sampler_loop():
    n = 7
    idx = torch.arange(n, dtype=torch.float64)
    want = (SMAX ** (1 / RHO) + idx / (n - 1) * (SMIN ** (1 / RHO) - SMAX ** (1 / RHO))) ** RHO
    got = samplers.edm_schedule(n, SMIN, SMAX, RHO)
    assert got[-1] == 0.0 and len(got) == n + 1
    assert torch.allclose(torch.tensor(got[:-1], dtype=torch.float64), want, rtol=1e-13, atol=0)
    assert samplers.evaluation_sigmas("heun", got) == [got[0]] + [v for i in range(1, n) for v in (got[i], got[i])]
    assert samplers.evaluation_sigmas("dpmpp_2m", got) == got[:-1]


def test_guidance_rule():
    assert samplers.is_guided(1.0, 3.0, None) and not samplers.is_guided(1.0, 1.0, None)
    iv = samplers.guidance_interval_bounds((0.5, 2))
    assert iv == (0.5, 2.0)
    assert samplers.is_guided(0.5, 3.0, iv) and samplers.is_guided(2.0, 3.0, iv)          # both ends belong to the interval
    assert not samplers.is_guided(0.49, 3.0, iv) and not samplers.is_guided(2.01, 3.0, iv)
    assert not samplers.is_guided(1.0, 1.0, iv)
    assert samplers.guidance_interval_bounds(None) is None
    with pytest.raises(ValueError):
        samplers.guidance_interval_bounds((2.0, 1.0))


# ------------------------------------------------------------------------------------------------ the surface
def _header():
    return open(os.path.join(ROOT, "include", "microdit_hip.h")).read()


def test_solver_entry_points_are_declared_and_bound():
    from micro_diffusion_amd import hip
    header = _header()
    for name, nargs in NEW.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/microdit_hip.h"
        assert name in hip.exported_symbols(), f"{name} is not bound in hip._SIGS"
        declared = [a for a in m.group(1).split(",") if a.strip()]
        restype, argtypes = hip._SIGS[name]
        assert len(declared) == len(argtypes) == nargs, (name, len(declared), len(argtypes))
        assert declared[-1].split()[0] == "hipStream_t"
    assert "x_next = a * x_in + b * (c1 * den - c2 * hist)" in header and "x_hat = x + coef * noise" in header
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6, "three symbols added, none changed: the ABI version stays"


def test_solver_entry_points_are_in_the_integration_notes():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in text


def _cpu_model():
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(input_size=8, dim=64, depth=2, head_dim=32, caption_channels=32, multiple_of=32, patch_mixer_depth=1, patch_mixer_dim=64,
                 num_experts=2)
    return LatentDiffusion(d, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=8)


def test_defaults_are_heun_and_no_interval():
    from micro_diffusion_amd.model import LatentDiffusion
    for fn in (LatentDiffusion.edm_sampler_loop, LatentDiffusion.generate):
        p = inspect.signature(fn).parameters
        assert p["sampler"].default == "heun" and p["guidance_interval"].default is None
    assert samplers.SAMPLERS == ("heun", "euler", "dpmpp_2m")


def test_unknown_sampler_and_2m_with_churn_raise():
    m = _cpu_model()
    x, y = torch.randn(1, 4, 8, 8), torch.randn(1, 1, 5, 32)
    for fused in (None, False):
        with pytest.raises(ValueError, match="unknown sampler"):
            m.edm_sampler_loop(x, y, steps=3, sampler="dpm", fused=fused)
    with pytest.raises(ValueError):
        m.edm_sampler_loop(x, y, steps=3, sampler="euler", guidance_interval=(3.0, 1.0))
    m.edm_config.S_churn = 10
    with pytest.raises(ValueError, match="S_churn"):
        m.edm_sampler_loop(x, y, steps=3, sampler="dpmpp_2m")
    assert samplers.check_sampler("euler", 10) == "euler" and samplers.check_sampler("heun", 10) == "heun"


def test_narrow_is_a_view_of_the_leading_samples():
    from micro_diffusion_amd.engine import Conditioning
    B, Lc = 4, 3
    pooled = torch.arange(B * 8.0).view(B, 8)
    kv = {"a": (torch.arange(B * Lc * 6.0).view(B * Lc, 6), None), "b": (torch.ones(B * Lc, 4), torch.arange(B * Lc * 2.0).view(B * Lc, 2))}
    c = Conditioning(B, Lc, True, (1, 2), pooled, kv)
    h = c.narrow(2)
    assert (h.B, h.Lc, h.head_major, h.version) == (2, Lc, True, (1, 2))
    assert h.pooled.data_ptr() == pooled.data_ptr() and torch.equal(h.pooled, pooled[:2]) and h.pooled.is_contiguous()
    for name, (k, khm) in kv.items():
        hk, hh = h.kv[name]
        assert hk.data_ptr() == k.data_ptr() and torch.equal(hk, k[:2 * Lc]) and hk.is_contiguous()
        assert (hh is None) == (khm is None)
        if khm is not None:
            assert hh.data_ptr() == khm.data_ptr() and torch.equal(hh, khm[:2 * Lc])
    assert h.nbytes * 2 == c.nbytes and c.narrow(B) is c
    for bad in (0, 5):
        with pytest.raises(ValueError):
            c.narrow(bad)


# ------------------------------------------------------------------------------------------------ compiled resources
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_solver_kernels_compile_without_scratch(tmp_path):
    from micro_diffusion_amd import hip, native
    res = native.resource_usage("edm.hip", hip.HIPCC_FLAGS, tmp_path / "edm.o")
    # the update kernels are two templates (update_kernel, update_tok_kernel) over a source and a step: the ones meant here are the
    # solver step and the Heun step over the cfg pair
    cfg = {k: v for k, v in res.items() if "cfg_source" in k}
    new = {k: v for k, v in res.items() if "churn_kernel" in k or (k in cfg and "solver_step" in k)}
    assert len(new) == 4, sorted(res)                # image space, two token-space instantiations, churn
    heun = {k: v for k, v in cfg.items() if "heun_step" in k}
    assert len(heun) == 3, sorted(res)
    for k, v in new.items():
        print(k, v)
        assert v["scratch"] == 0 and v["spill"] == 0 and v["lds"] == 0, (k, v)
    # one history buffer and one state in place of d_cur, x_hat and x_in: no more registers than the Heun kernel of the same space
    for tag in ("update_kernelI", "update_tok_kernelI"):
        for k, v in new.items():
            if tag in k:
                ref = max(h["vgprs"] for hk, h in heun.items() if tag in hk)
                assert v["vgprs"] <= ref and v["occ"] >= min(h["occ"] for hk, h in heun.items() if tag in hk), (k, v, ref)
