"""Measurement-guided sampling, host side: what samplers.check_measurement refuses, the measurement operator and its
adjoint, the ABI additions, the host-side argument checks of the five entry points, and the public signatures.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from micro_diffusion_amd import samplers
from micro_diffusion_amd.inverse import LinearMeasurement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"md_edm_denoised": 10, "md_edm_denoised_tok": 13, "md_measure_residual": 12, "md_guide_cotangent_tok": 12, "md_edm_guide_apply": 11}
SHAPE = (2, 4, 8, 8)


def _meas(s=2, B=2, C=4, H=8, W=8):
    return torch.zeros(B, C, H // s, W // s)


def test_check_measurement_accepts_what_is_defined():
    assert samplers.check_measurement(SHAPE) is False
    assert samplers.check_measurement(SHAPE, LinearMeasurement(_meas(1))) is True
    assert samplers.check_measurement(SHAPE, LinearMeasurement(_meas(2), 2), 0.0) is True
    assert samplers.check_measurement(SHAPE, guidance_loss=lambda D: D.flatten(1).sum(1), measurement_scale=3) is True
    for mshape in ((4, 4), (1, 4, 4), (2, 4, 4), (1, 1, 4, 4), (2, 1, 4, 4)):
        assert samplers.check_measurement(SHAPE, LinearMeasurement(_meas(2), 2, torch.rand(mshape) < 0.5))
        assert samplers.check_measurement(SHAPE, LinearMeasurement(_meas(2), 2, torch.rand(mshape)))
    assert samplers.check_measurement(None, LinearMeasurement(_meas(2), 2)) is True      # generate(): the state's shape is not known yet


@pytest.mark.parametrize("kw,match", [
    (dict(measurement=LinearMeasurement(_meas(2), 3)), "does not divide"),
    (dict(measurement=LinearMeasurement(_meas(2), 0)), "integer >= 1"),
    (dict(measurement=LinearMeasurement(_meas(2), 2.0)), "integer >= 1"),
    (dict(measurement=LinearMeasurement(_meas(2), True)), "integer >= 1"),
    (dict(measurement=LinearMeasurement(_meas(1), 2)), "expected"),                       # meas on the un-pooled grid
    (dict(measurement=LinearMeasurement(_meas(2, B=3), 2)), "expected"),
    (dict(measurement=LinearMeasurement(_meas(2).long(), 2)), "floating"),
    (dict(measurement=LinearMeasurement(_meas(2), 2, torch.ones(8, 8))), "mask has shape"),   # a mask on the un-pooled grid
    (dict(measurement=LinearMeasurement(_meas(2), 2, torch.ones(2, 4, 4, 4))), "mask has shape"),
    (dict(measurement=LinearMeasurement(_meas(2), 2, torch.ones(3, 1, 4, 4))), "mask has shape"),
    (dict(measurement=LinearMeasurement(_meas(2), 2, torch.full((4, 4), 1.5))), r"\[0, 1\]"),
    (dict(measurement=LinearMeasurement(_meas(2), 2, torch.full((4, 4), -0.1))), r"\[0, 1\]"),
    (dict(measurement=LinearMeasurement(_meas(2), 2, torch.ones(4, 4, dtype=torch.long))), r"\[0, 1\]"),
    (dict(measurement=object()), "LinearMeasurement"),
    (dict(measurement=LinearMeasurement(_meas(1)), measurement_scale=float("nan")), "finite"),
    (dict(measurement=LinearMeasurement(_meas(1)), measurement_scale=float("inf")), "finite"),
    (dict(measurement=LinearMeasurement(_meas(1)), measurement_scale=-1.0), ">= 0"),
    (dict(measurement=LinearMeasurement(_meas(1)), measurement_scale="2"), "finite"),
    (dict(measurement=LinearMeasurement(_meas(1)), guidance_loss=lambda D: D), "mutually exclusive"),
    (dict(measurement_scale=2.0), "nothing to scale"),
    (dict(guidance_loss=3), "callable"),
])
def test_check_measurement_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        samplers.check_measurement(SHAPE, **kw)


def _pool_np(z, s):
    B, C, H, W = z.shape
    return z.reshape(B, C, H // s, s, W // s, s).mean(axis=(3, 5))


def _pool_adjoint_np(v, s):
    return np.repeat(np.repeat(v, s, axis=2), s, axis=3) / (s * s)


@pytest.mark.parametrize("s", [1, 2, 4])
def test_measurement_operator_and_its_adjoint(s):
    """A and A^T in numpy: <A u, v> = <u, A^T v>; LinearMeasurement.apply / adjoint are those two; autograd of its loss is
    -2 A^T(m * m * (meas - A(D))), the q md_measure_residual writes."""
    rng = np.random.default_rng(7 + s)
    B, C, H, W = 3, 4, 8, 12
    f32 = lambda a: a.astype(np.float32).astype(np.float64)       # operands() holds meas and mask in fp32: values that survive it
    u, v = rng.standard_normal((B, C, H, W)), f32(rng.standard_normal((B, C, H // s, W // s)))
    lhs, rhs = (_pool_np(u, s) * v).sum(), (u * _pool_adjoint_np(v, s)).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(_pool_np(u, s) * v).sum() + np.abs(u * _pool_adjoint_np(v, s)).sum())
    meas = torch.from_numpy(v)
    mask = torch.from_numpy(f32(rng.random((B, 1, H // s, W // s))))
    lm = LinearMeasurement(meas, s, mask)
    ut = torch.from_numpy(u)
    assert np.allclose(lm.apply(ut).numpy(), _pool_np(u, s), rtol=0, atol=1e-14)
    assert np.allclose(lm.adjoint(meas).numpy(), _pool_adjoint_np(v, s), rtol=0, atol=1e-14)
    D = ut.clone().requires_grad_(True)
    L = lm.loss_fn(D)(D)
    m = mask.numpy()
    r = m * (v - _pool_np(u, s))
    assert np.allclose(L.detach().numpy(), (r * r).sum(axis=(1, 2, 3)), rtol=1e-12)
    q, = torch.autograd.grad(L.sum(), D)
    assert np.allclose(q.numpy(), -2.0 * _pool_adjoint_np(m * r, s), rtol=1e-12, atol=1e-14)


def test_operands_are_converted_once():
    lm = LinearMeasurement(torch.ones(2, 4, 4, 4, dtype=torch.float64), 2, torch.rand(4, 4) < 0.5)
    meas, mask = lm.operands(torch.zeros(1))
    assert meas.dtype == torch.float32 and meas.is_contiguous() and mask.dtype == torch.float32 and tuple(mask.shape) == (1, 16)
    assert LinearMeasurement(torch.ones(2, 4, 4, 4), 2, torch.ones(2, 1, 4, 4)).operands(torch.zeros(1))[1].shape == (2, 16)
    assert LinearMeasurement(torch.ones(2, 4, 4, 4), 2).operands(torch.zeros(1))[1] is None


def test_library_exports_the_entry_points():
    from micro_diffusion_amd import hip
    with open(os.path.join(ROOT, "include", "microdit_hip.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(hip.build())
    for name, nargs in NEW.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/microdit_hip.h"
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
        assert name in hip.exported_symbols(), f"{name} is not bound in hip._SIGS"
        declared = [a for a in m.group(1).split(",") if a.strip()]
        assert len(declared) == len(hip._SIGS[name][1]) == nargs, (name, len(declared))
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6 == lib.md_abi_version(), "symbols added, none changed"
    assert re.search(r"#define MD_GUIDE_TINY 1e-30\b", header) and hip.GUIDE_TINY == 1e-30 == samplers.GUIDE_TINY


def test_bad_arguments_are_refused_before_any_launch():
    """Fake addresses: a call that got past the checks would fault, so every one of these must return MD_BAD_ARG from the host."""
    from micro_diffusion_amd import hip
    L = hip.lib()
    a, b, c, d = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    nan, inf = float("nan"), float("inf")

    def denoised(x=a, F=b, D=c, B=2, per=64, cfg=3.0, hu=1, t=1.0, sd=0.9):
        return L.md_edm_denoised(x, F, D, B, per, cfg, hu, t, sd, None)

    def denoised_tok(x=a, F=b, D=c, B=2, C=4, H=8, W=8, p=2, cfg=3.0, hu=1, t=1.0, sd=0.9):
        return L.md_edm_denoised_tok(x, F, D, B, C, H, W, p, cfg, hu, t, sd, None)

    def residual(D=a, meas=b, mask=None, mB=1, q=c, Lp=d, B=2, C=4, H=8, W=8, s=2):
        return L.md_measure_residual(D, meas, mask, mB, q, Lp, B, C, H, W, s, None)

    def cotangent(q=a, dtok=b, B=2, C=4, H=8, W=8, p=2, cfg=3.0, hu=1, t=1.0, sd=0.9):
        return L.md_guide_cotangent_tok(q, dtok, B, C, H, W, p, cfg, hu, t, sd, None)

    def apply(x=a, q=b, dx=c, Lp=d, B=2, per=64, hu=1, zeta=1.0, t=1.0, sd=0.9):
        return L.md_edm_guide_apply(x, q, dx, Lp, B, per, hu, zeta, t, sd, None)
    level = [dict(t=0.0), dict(t=-1.0), dict(t=nan), dict(t=inf), dict(sd=nan), dict(sd=inf)]
    image = [dict(B=0), dict(C=0), dict(H=0), dict(W=-8)]
    for kw in [dict(x=None), dict(F=None), dict(D=None), dict(B=0), dict(per=0), dict(cfg=nan), dict(cfg=inf)] + level:
        assert denoised(**kw) == -1, kw
    for kw in [dict(x=None), dict(F=None), dict(D=None), dict(p=0), dict(H=7), dict(W=9), dict(p=3), dict(cfg=nan)] + image + level:
        assert denoised_tok(**kw) == -1, kw
    for kw in [dict(D=None), dict(meas=None), dict(q=None), dict(Lp=None), dict(s=0), dict(s=3), dict(s=16), dict(H=6, s=4), dict(W=12, s=8),
               dict(mask=d, mB=3), dict(mask=d, mB=0)] + image:
        assert residual(**kw) == -1, kw
    for kw in [dict(q=None), dict(dtok=None), dict(p=0), dict(H=7), dict(W=9), dict(cfg=nan)] + image + level:
        assert cotangent(**kw) == -1, kw
    for kw in [dict(x=None), dict(q=None), dict(dx=None), dict(Lp=None), dict(B=0), dict(per=0), dict(zeta=nan), dict(zeta=inf)] + level:
        assert apply(**kw) == -1, kw


def test_the_new_arguments_are_real_parameters():
    """An unknown keyword falls into **kwargs, switches the fused loop off and is then ignored by the forward: the three names must
    be parameters of their own, with defaults that mean 'not guided'."""
    from micro_diffusion_amd.model import LatentDiffusion
    for fn in (LatentDiffusion.edm_sampler_loop, LatentDiffusion.generate):
        par = inspect.signature(fn).parameters
        assert par["measurement"].default is None and par["guidance_loss"].default is None and par["measurement_scale"].default == 1.0
        assert all(par[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in ("measurement", "measurement_scale", "guidance_loss"))


def test_engine_signatures():
    from micro_diffusion_amd.engine import DiTEngine
    par = inspect.signature(DiTEngine.forward).parameters["input_tape"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
    assert DiTEngine._x_only is False and DiTEngine._param_grads is True
