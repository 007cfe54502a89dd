"""Dispersive loss, host side: the fp64 definition (disperse.reference) against torch autograd, its edge cases, the
switch's validation, the config keys, the ABI additions and the refusal of the autograd surface while the term is armed.  No GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

from micro_diffusion_amd import config as mdcfg
from micro_diffusion_amd import disperse as dsp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"md_disperse_ws_doubles": 2, "md_disperse_pairs": 15, "md_disperse_gram_small": 7}
SHAPES = [(1, 64), (2, 64), (3, 128), (5, 256), (65, 512)]


def _autograd(z, tau):
    z = z.clone().requires_grad_(True)
    K = z.shape[1]
    L = torch.log(torch.exp(-torch.cdist(z, z, compute_mode="donot_use_mm_for_euclid_dist") ** 2 / K / tau).mean())
    L.backward()
    return L.detach(), z.grad


@pytest.mark.parametrize("B,K", SHAPES)
def test_reference_agrees_with_autograd(B, K):
    torch.manual_seed(100 * B + K)
    z = torch.randn(B, K, dtype=torch.float64)
    for tau in (0.5, 1.7):
        L, g, md = dsp.reference(z, tau)
        La, ga = _autograd(z, tau)
        assert L.dtype == g.dtype == md.dtype == torch.float64
        assert abs(float(L - La)) <= 1e-12, (float(L), float(La))
        assert float((g - ga).abs().max()) <= 1e-12
        assert float(L) <= 0.0
        if B > 1:
            d = torch.cdist(z, z) ** 2 / K
            assert abs(float(md) - float(d.sum() / (B * (B - 1)))) <= 1e-12


def test_a_single_sample_gives_exactly_zero():
    L, g, md = dsp.reference(torch.randn(1, 64, dtype=torch.float64), 0.5)
    assert float(L) == 0.0 and not g.any() and float(md) == 0.0


@pytest.mark.parametrize("B,K", SHAPES[1:])
def test_saturated_and_identical_rows(B, K):
    torch.manual_seed(B)
    z = torch.randn(B, K, dtype=torch.float64)
    L, g, _ = dsp.reference(30.0 * z, 0.5)                       # every pair so far apart that exp underflows: only the diagonal is left
    assert abs(float(L) - math.log(1.0 / B)) <= 4 * 2.0 ** -52 * abs(math.log(1.0 / B))
    assert bool(torch.isfinite(g).all()) and not g.any(), "the saturated gradient is exactly 0, never NaN"
    same = z[:1].expand(B, K).contiguous()
    L, g, md = dsp.reference(same, 0.5)
    assert float(L) == 0.0 and not g.any() and float(md) == 0.0


def test_reference_takes_low_precision_input():
    z = torch.randn(4, 64).to(torch.bfloat16)
    L, g, _ = dsp.reference(z, 0.5)
    L64, g64, _ = dsp.reference(z.double(), 0.5)
    assert torch.equal(L, L64) and torch.equal(g, g64)


def test_switch_validation():
    d = dsp.DisperseLoss()
    assert (d.weight, d.tau, d.block, d.enabled) == (0.5, 0.5, None, True)
    assert d.resolve_block(28) == 7 and d.resolve_block(3) == 0 and dsp.DisperseLoss(block=2).resolve_block(3) == 2
    assert not dsp.DisperseLoss(weight=0).enabled, "weight 0 is off"
    for kw in (dict(weight=-0.1), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight="1"), dict(weight=True),
               dict(tau=0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")), dict(tau=None),
               dict(block=-1), dict(block=1.0), dict(block=True)):
        with pytest.raises(ValueError):
            dsp.DisperseLoss(**kw)
    with pytest.raises(ValueError, match="outside"):
        dsp.DisperseLoss(block=3).resolve_block(3)


# ------------------------------------------------------------------------------------------------ config
def _cfg(*overrides, name="res_256_pretrain.yaml"):
    return mdcfg.load_config(os.path.join(ROOT, "configs"), name, ["exp_name=t", *overrides])


def test_config_switches_parse():
    off = {"enabled": False, "weight": 0.0, "tau": 0.5, "block": None}
    for name in sorted(f for f in os.listdir(os.path.join(ROOT, "configs")) if f.endswith(".yaml")):
        assert mdcfg.disperse_options(_cfg(name=name)) == off, f"{name}: the stage configs parse unchanged, feature off"
    assert mdcfg.disperse_options(_cfg("misc.disperse_weight=0")) == off
    assert mdcfg.disperse_options(_cfg("misc.disperse_weight=0.5")) == {"enabled": True, "weight": 0.5, "tau": 0.5, "block": None}
    o = mdcfg.disperse_options(_cfg("misc.disperse_weight=0.25", "misc.disperse_tau=1", "misc.disperse_block=3"))
    assert o == {"enabled": True, "weight": 0.25, "tau": 1.0, "block": 3}


@pytest.mark.parametrize("overrides, match", [
    (["misc.disperse_weight=-0.5"], "disperse_weight"),
    (["misc.disperse_weight=much"], "disperse_weight"),
    (["misc.disperse_weight=true"], "disperse_weight"),
    (["misc.disperse_weight=0.5", "misc.disperse_tau=0"], "disperse_tau"),
    (["misc.disperse_weight=0.5", "misc.disperse_tau=-1"], "disperse_tau"),
    (["misc.disperse_weight=0.5", "misc.disperse_tau=warm"], "disperse_tau"),
    (["misc.disperse_weight=0.5", "misc.disperse_block=-1"], "disperse_block"),
    (["misc.disperse_weight=0.5", "misc.disperse_block=1.5"], "disperse_block"),
    (["misc.disperse_tau=0.5"], "disperse_weight"),
    (["misc.disperse_block=2"], "disperse_weight"),
    (["misc.disperse_weight=0", "misc.disperse_tau=0.5"], "disperse_weight"),
])
def test_train_py_refuses_before_anything_is_allocated(overrides, match):
    import train
    with pytest.raises(ValueError, match=match):
        mdcfg.disperse_options(_cfg(*overrides))
    with pytest.raises(ValueError, match=match):
        train.train(_cfg(*overrides))             # refused before a device or a dataset is touched


def test_log_line_adds_nothing_when_off():
    import train
    base = train.log_line(10, 0.5, 1e-4, 100.0)
    assert set(base) == {"batch", "loss", "lr", "samples_per_sec"}
    on = train.log_line(10, 0.5, 1e-4, 100.0, disperse={"disperse_loss": -0.25, "disperse_mean_dist": 1.5})
    assert on["loss"] == 0.5 and on["disperse_loss"] == -0.25 and on["disperse_mean_dist"] == 1.5


# ------------------------------------------------------------------------------------------------ ABI, argument checks
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
    assert re.search(r"#define MD_DISPERSE_MAX_B 4096\b", header) and hip.DISPERSE_MAX_B == 4096


def test_bad_arguments_are_refused_before_any_launch():
    """The argument checks run on the host in front of the launch: callable without a GPU (fake addresses)."""
    from micro_diffusion_amd import hip
    L = hip.lib()
    g = 1 << 20
    out = ctypes.c_int64(0)
    assert L.md_disperse_ws_doubles(65, ctypes.byref(out)) == 0 and out.value == 130
    assert L.md_disperse_ws_doubles(0, ctypes.byref(out)) == -1 and L.md_disperse_ws_doubles(4097, ctypes.byref(out)) == -1
    ok = [g, 8, 5, 64, 0.5, 1.0, g, 8, g, g, 10, None, None, 0.0, None]
    for k in (0, 6, 8, 9):                                        # G, W, result, ws
        a = list(ok)
        a[k] = None
        assert L.md_disperse_pairs(*a) == -1, k
    for k, v in ((1, 4), (2, 0), (2, 4097), (3, 0), (4, 0.0), (4, -1.0), (4, float("inf")), (5, float("nan")), (7, 4), (7, 12), (10, 9)):
        a = list(ok)
        a[k] = v
        assert L.md_disperse_pairs(*a) == -1, (k, v)
    ok = [g, 64, 5, 64, g, 8, None]
    for k, v in ((0, None), (4, None), (2, 0), (2, 4097), (3, 0), (3, 60), (1, 56), (1, 68), (5, 4), (0, g + 8)):
        a = list(ok)
        a[k] = v
        assert L.md_disperse_gram_small(*a) == -1, (k, v)


# ------------------------------------------------------------------------------------------------ the autograd surface
def test_autograd_surface_refuses_while_armed():
    """The term's gradient exists on train_microbatch alone: edm_loss with grad enabled raises before it touches a device."""
    from oracle import microdit_ref as orc
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    cfg = orc.tiny_config()
    model = LatentDiffusion(mdit.DiT(**cfg.__dict__), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), train_mask_ratio=0.75)
    assert model.disperse is None
    x, y = torch.zeros(2, 4, 32, 32), torch.zeros(2, 1, 77, cfg.caption_channels)
    model.disperse = dsp.DisperseLoss()
    with pytest.raises(RuntimeError, match="dispersive loss is armed"):
        model.edm_loss(x, y, mask_ratio=0.75)
