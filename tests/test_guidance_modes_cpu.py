"""Guidance modes, host side (no GPU): samplers.guidance_coefficients against explicit tensor constructions of adaptive
projected guidance (clip, project, eta, momentum) and of CFG rescale in fp64, the properties the two modes promise, every request
check_guidance refuses, and the surface: the five arguments of edm_sampler_loop / generate, the six entry points in the header, the
binding and the built library."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from micro_diffusion_amd import samplers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("md_guidance_prepare", "md_guidance_prepare_tok", "md_edm_heun_update_coef", "md_edm_heun_update_coef_tok",
         "md_edm_solver_update_coef", "md_edm_solver_update_coef_tok")
B, N, W_G = 3, 256, 5.0


def _operands(seed=0):
    g = torch.Generator().manual_seed(seed)
    d_c = torch.randn(B, 4, 8, 8, generator=g, dtype=torch.float64) * 1.5 + 0.3
    d_u = d_c * 0.6 + torch.randn(B, 4, 8, 8, generator=g, dtype=torch.float64) * torch.tensor([0.2, 0.7, 2.0], dtype=torch.float64).view(B, 1, 1, 1)
    m_prev = torch.randn(B, 4, 8, 8, generator=g, dtype=torch.float64) * 0.5
    return d_c, d_u, m_prev


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _apg_explicit(d_c, d_u, m_prev, w, eta, r, beta):
    """APG as the paper states it: momentum on the difference, norm clip, split along D_c, eta on the parallel part."""
    diff = (d_c - d_u) + beta * m_prev
    if r is not None:
        norm = diff.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
        diff = diff * torch.minimum(torch.ones_like(norm), r / norm)
    unit = d_c / d_c.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    par = (diff * unit).flatten(1).sum(1).view(-1, 1, 1, 1) * unit
    orth = diff - par
    return d_c + (w - 1.0) * (orth + eta * par)


def _rescale_explicit(d_c, d_u, w, phi):
    """CFG rescale (Lin et al. 2024, eq. 15-16) on the denoised prediction: population standard deviations over [C, H, W]."""
    guided = d_u + w * (d_c - d_u)
    std_c = d_c.flatten(1).std(dim=1, unbiased=False).view(-1, 1, 1, 1)
    std_g = guided.flatten(1).std(dim=1, unbiased=False).view(-1, 1, 1, 1)
    return phi * (guided * std_c / std_g) + (1.0 - phi) * guided


def _combine(mode, d_c, m, w, **kw):
    alpha, gamma = samplers.guidance_coefficients(mode, samplers.guidance_moments(d_c, m), d_c[0].numel(), w, **kw)
    assert alpha.dtype == gamma.dtype == torch.float64 and alpha.shape == gamma.shape == (d_c.shape[0],)
    return alpha.view(-1, 1, 1, 1) * d_c + gamma.view(-1, 1, 1, 1) * m, alpha, gamma


# ------------------------------------------------------------------------------------------------ against the explicit constructions
@pytest.mark.parametrize("eta", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("beta", [0.0, -0.5])
def test_apg_coefficients_against_the_explicit_construction(eta, beta):
    d_c, d_u, m_prev = _operands()
    assert d_c[0].numel() == N
    m = (d_c - d_u) + beta * m_prev
    norms = m.flatten(1).norm(dim=1)
    r = float(norms.median())
    # on the reference alone: the clip is active for at least one sample and inactive for at least one
    assert (norms > r).any() and (norms <= r).any(), norms
    for thr in (r, None):
        want = _apg_explicit(d_c, d_u, m_prev, W_G, eta, thr, beta)
        got, _, _ = _combine("apg", d_c, m, W_G, apg_eta=eta, apg_norm_threshold=thr)
        assert _rel(got, want) < 1e-12, _rel(got, want)
    clipped = _apg_explicit(d_c, d_u, m_prev, W_G, eta, r, beta)
    assert _rel(clipped, _apg_explicit(d_c, d_u, m_prev, W_G, eta, None, beta)) > 1e-3, "the clip must change the result"


@pytest.mark.parametrize("phi", [0.0, 0.7, 1.0])
def test_rescale_coefficients_against_the_explicit_construction(phi):
    d_c, d_u, _ = _operands(1)
    want = _rescale_explicit(d_c, d_u, W_G, phi)
    got, _, _ = _combine("rescale", d_c, d_c - d_u, W_G, guidance_rescale=phi)
    assert _rel(got, want) < 1e-12, _rel(got, want)


# ------------------------------------------------------------------------------------------------ properties
def test_neutral_settings_give_plain_guidance():
    d_c, d_u, _ = _operands(2)
    m = d_c - d_u
    for mode, kw in (("apg", dict(apg_eta=1.0, apg_norm_threshold=None)), ("rescale", dict(guidance_rescale=0.0))):
        got, alpha, gamma = _combine(mode, d_c, m, W_G, **kw)
        assert torch.equal(alpha, torch.ones(B, dtype=torch.float64)) and torch.equal(gamma, torch.full((B,), W_G - 1.0, dtype=torch.float64))
        assert _rel(got, d_u + W_G * (d_c - d_u)) < 1e-14


def test_full_rescale_restores_the_conditional_standard_deviation():
    d_c, d_u, _ = _operands(3)
    got, _, _ = _combine("rescale", d_c, d_c - d_u, W_G, guidance_rescale=1.0)
    std = lambda t: t.flatten(1).std(dim=1, unbiased=False)
    assert torch.allclose(std(got), std(d_c), rtol=1e-12, atol=0)
    assert not torch.allclose(std(d_u + W_G * (d_c - d_u)), std(d_c), rtol=1e-2), "plain guidance must have changed it"


def test_apg_eta_zero_update_is_orthogonal_to_the_conditional_prediction():
    d_c, d_u, _ = _operands(4)
    m = d_c - d_u
    for r in (None, float(m.flatten(1).norm(dim=1).median())):
        got, _, _ = _combine("apg", d_c, m, W_G, apg_eta=0.0, apg_norm_threshold=r)
        upd = (got - d_c).flatten(1)
        cos = (upd * d_c.flatten(1)).sum(1) / (upd.norm(dim=1) * d_c.flatten(1).norm(dim=1))
        assert cos.abs().max() < 1e-12, cos


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_apg_norm_threshold_bounds_the_update(eta):
    d_c, d_u, _ = _operands(5)
    m = d_c - d_u
    r = float(m.flatten(1).norm(dim=1).min()) * 0.5            # active for every sample
    got, _, _ = _combine("apg", d_c, m, W_G, apg_eta=eta, apg_norm_threshold=r)
    assert ((got - d_c).flatten(1).norm(dim=1) <= (W_G - 1.0) * r * (1 + 1e-12)).all()


@pytest.mark.parametrize("mode,kw", [("apg", dict(apg_eta=0.25, apg_norm_threshold=2.0)), ("apg", dict(apg_eta=0.0)),
                                     ("rescale", dict(guidance_rescale=0.7)), ("rescale", dict(guidance_rescale=1.0))])
def test_degenerate_inputs_give_finite_coefficients(mode, kw):
    d_c, _, _ = _operands(6)
    zero = torch.zeros_like(d_c)
    const = torch.full_like(d_c, 0.1)                           # no variance: var_c may round below zero
    for dc, m in ((d_c, zero), (zero, d_c), (zero, zero), (const, zero), (const, const)):
        got, alpha, gamma = _combine(mode, dc, m, W_G, **kw)
        assert torch.isfinite(alpha).all() and torch.isfinite(gamma).all() and torch.isfinite(got).all()
        if not m.any():                                         # D_c = D_u: nothing to guide with, the prediction comes back
            assert torch.equal(alpha, torch.ones(B, dtype=torch.float64)), alpha
            assert torch.equal(got, dc)


def test_coefficients_refuse_the_mode_without_a_table():
    with pytest.raises(ValueError, match="cfg"):
        samplers.guidance_coefficients("cfg", torch.zeros(1, 5), 4, 3.0)


# ------------------------------------------------------------------------------------------------ the interface
def test_check_guidance_accepts_what_is_defined():
    assert samplers.GUIDANCE_MODES == ("cfg", "rescale", "apg")
    assert samplers.check_guidance() == "cfg"
    assert samplers.check_guidance("cfg", 5.0) == "cfg"
    assert samplers.check_guidance("rescale", 5.0, 0.7) == "rescale"
    assert samplers.check_guidance("rescale", 5.0, guidance_rescale=1.0) == "rescale"
    assert samplers.check_guidance("apg", 5.0, apg_eta=0.25, apg_norm_threshold=2.5, apg_momentum=-0.5) == "apg"
    assert samplers.check_guidance("apg", 1.0) == "apg"         # cfg <= 1 runs unguided; the request itself is legal


@pytest.mark.parametrize("args,kw,match", [
    (("dynamic",), {}, "unknown guidance_mode"),
    ((None,), {}, "unknown guidance_mode"),
    (("cfg", 5.0), dict(guidance_rescale=0.7), "needs guidance_mode='rescale'"),
    (("apg", 5.0), dict(guidance_rescale=0.7), "needs guidance_mode='rescale'"),
    (("cfg", 5.0), dict(apg_eta=0.5), "need guidance_mode='apg'"),
    (("cfg", 5.0), dict(apg_norm_threshold=2.0), "need guidance_mode='apg'"),
    (("rescale", 5.0, 0.5), dict(apg_momentum=-0.5), "need guidance_mode='apg'"),
    (("rescale", 5.0, -0.1), {}, r"\[0, 1\]"),
    (("rescale", 5.0, 1.5), {}, r"\[0, 1\]"),
    (("rescale", 5.0, float("nan")), {}, "finite"),
    (("apg", 5.0), dict(apg_norm_threshold=0.0), "> 0"),
    (("apg", 5.0), dict(apg_norm_threshold=-1.0), "> 0"),
    (("apg", 5.0), dict(apg_norm_threshold=float("inf")), "finite"),
    (("apg", 5.0), dict(apg_momentum=1.0), r"\(-1, 1\)"),
    (("apg", 5.0), dict(apg_momentum=-1.0), r"\(-1, 1\)"),
    (("apg", 5.0), dict(apg_momentum=-1.5), r"\(-1, 1\)"),
    (("apg", 5.0), dict(apg_eta=float("nan")), "finite"),
    (("apg", float("inf")), {}, "finite"),
])
def test_check_guidance_refuses(args, kw, match):
    with pytest.raises(ValueError, match=match):
        samplers.check_guidance(*args, **kw)


def test_new_arguments_default_to_today_and_are_named_parameters():
    from micro_diffusion_amd.model import LatentDiffusion
    want = dict(guidance_mode="cfg", guidance_rescale=0.0, apg_eta=0.0, apg_norm_threshold=None, apg_momentum=0.0)
    for fn in (LatentDiffusion.edm_sampler_loop, LatentDiffusion.generate):
        p = inspect.signature(fn).parameters
        for name, default in want.items():
            assert name in p, f"{fn.__name__} lacks {name}"
            assert p[name].default == default and type(p[name].default) is type(default), (fn.__name__, name, p[name].default)
            assert p[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert [k for k, v in p.items() if v.kind is inspect.Parameter.VAR_KEYWORD] == ["kwargs"]


def test_requests_are_refused_before_anything_runs():
    """Both public functions check the request first: no parameters, device or text encoder is touched (self is not even a model)."""
    from micro_diffusion_amd.model import LatentDiffusion

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    class Stub:
        edm_config = Cfg(S_churn=0, num_steps=4)
        dit = None
    x = torch.zeros(1, 4, 8, 8)
    for kw, match in ((dict(guidance_mode="nope"), "unknown guidance_mode"), (dict(guidance_rescale=0.5), "needs guidance_mode"),
                      (dict(guidance_mode="apg", apg_momentum=1.0), r"\(-1, 1\)")):
        with pytest.raises(ValueError, match=match):
            LatentDiffusion.edm_sampler_loop(Stub(), x, None, 4, 3.0, **kw)
        with pytest.raises(ValueError, match=match):
            LatentDiffusion.generate(Stub(), ["a prompt"], **kw)


def _declaration(header, name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/microdit_hip.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_entry_points_are_declared_and_bound():
    from micro_diffusion_amd import hip
    header = open(os.path.join(ROOT, "include", "microdit_hip.h")).read()
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6, "six symbols added, none changed: the ABI version stays"
    for name in NAMES:
        declared = _declaration(header, name)
        assert name in hip.exported_symbols() and name in hip._SIGS, f"{name} is not bound in hip._SIGS"
        restype, argtypes = hip._SIGS[name]
        assert len(declared) == len(argtypes), (name, len(declared), len(argtypes))
        assert declared[-1].split()[0] == "hipStream_t"
        for text, ctype in zip(declared, argtypes):             # pointers, integers and floating-point arguments line up
            kind = "P" if "*" in text or "hipStream_t" in text else text.split()[-2]
            assert {"P": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double,
                    "float": ctypes.c_float}[kind] is ctype, (name, text)
    assert re.search(r"#define MD_GUIDANCE_RESCALE 1\b", header) and hip.GUIDANCE_RESCALE == 1
    assert re.search(r"#define MD_GUIDANCE_APG 2\b", header) and hip.GUIDANCE_APG == 2
    for formula in ("M = (D_c - D_u) + beta * M_prev", "alpha = 1 - w1 * (1 - eta) * p;   gamma = w1 * s",
                    "k = var_g > 0 ? phi * sqrt(var_c / var_g) + 1 - phi : 1;   alpha = k;   gamma = k * w1"):
        assert formula in header, formula


def test_built_library_exports_the_entry_points():
    from micro_diffusion_amd import hip
    lib = ctypes.CDLL(hip.build())
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert lib.md_abi_version() == 6
