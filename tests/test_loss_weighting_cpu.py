"""Learned per-noise-level loss weighting without a GPU: the three entry points are declared, exported and bound; the config switches
parse and refuse; the fp64 restatement in micro_diffusion_amd/loss_weighting.py (the reference of tests/test_loss_weighting_gpu.py)
agrees with torch autograd on the objective; the state round-trips; and the reference alone meets the fit condition of the GPU test.

Tolerances.  The restatement and autograd evaluate the same fp64 expressions in another order: 1e-12 relative to the largest entry.
The fit condition is the one of the GPU test (>= 0.9 of the gap between mean L and mean(1 + ln L) closed on 4096 held-out levels)."""
import ctypes
import math
import os
import re
import warnings

import pytest
import torch

from micro_diffusion_amd import config as mdcfg
from micro_diffusion_amd import loss_weighting as lwm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"md_logvar_fwd": 9, "md_edm_loss_train_weighted": 20, "md_logvar_bwd": 13}


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
        assert declared[-1].split()[0] == "hipStream_t"
    # the weighted loss is the argument list of md_edm_loss_train plus sample_scale in front of the stream
    assert len(hip._SIGS["md_edm_loss_train_weighted"][1]) == len(hip._SIGS["md_edm_loss_train"][1]) + 1
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6 == lib.md_abi_version(), "three symbols added, none changed"


def test_bad_arguments_are_refused_before_any_launch():
    """The argument checks run on the host in front of the launch: callable without a GPU (fake addresses)."""
    from micro_diffusion_amd import hip
    L = hip.lib()
    g = 1 << 20
    assert L.md_logvar_fwd(g, g, g, g, g, g, 0, 128, None) == -1
    for C in (0, 32, 96, 320, 100, -64):
        assert L.md_logvar_fwd(g, g, g, g, g, g, 4, C, None) == -1, C
        assert L.md_logvar_bwd(g, g, g, g, g, 1.0, g, g, None, 0.0, 4, C, None) == -1, C
    for k in range(6):
        a = [g] * 6
        a[k] = None
        assert L.md_logvar_fwd(*a, 4, 128, None) == -1, k
    for k in (0, 1, 2, 3, 4, 6, 7):
        a = [g, g, g, g, g, 1.0, g, g, None, 0.0]
        a[k] = None
        assert L.md_logvar_bwd(*a, 4, 128, None) == -1, k
    assert L.md_logvar_bwd(g, g, g, g, g, 1.0, g, g, g, 0.0, 0, 128, None) == -1
    ok = [g, None, g, g, g, g, g, g, 0.5, None, 0.0, 3, 4, 4, 8, 8, 2, 0.9, g, None]
    for k in (0, 2, 3, 4, 5, 6, 7, 18):
        a = list(ok)
        a[k] = None
        assert L.md_edm_loss_train_weighted(*a) == -1, k
    for k, v in ((11, 0), (12, 0), (14, 7)):
        a = list(ok)
        a[k] = v
        assert L.md_edm_loss_train_weighted(*a) == -1, k


# ------------------------------------------------------------------------------------------------ config
def _cfg(*overrides):
    return mdcfg.load_config(os.path.join(ROOT, "configs"), "res_256_pretrain.yaml", ["exp_name=t", *overrides])


def test_config_switches_parse():
    assert mdcfg.loss_weighting_options(_cfg()) == {"enabled": False, "channels": 128, "lr": None}
    assert mdcfg.loss_weighting_options(_cfg("misc.loss_uncertainty_weighting=false")) == {"enabled": False, "channels": 128, "lr": None}
    assert mdcfg.loss_weighting_options(_cfg("misc.loss_uncertainty_weighting=true")) == {"enabled": True, "channels": 128, "lr": None}
    o = mdcfg.loss_weighting_options(_cfg("misc.loss_uncertainty_weighting=true", "misc.loss_uncertainty_channels=64",
                                          "misc.loss_uncertainty_lr=1e-3"))
    assert o == {"enabled": True, "channels": 64, "lr": 1e-3}
    assert mdcfg.loss_weighting_options(_cfg("misc.loss_uncertainty_weighting=true", "misc.loss_uncertainty_channels=256"))["channels"] == 256


@pytest.mark.parametrize("overrides, match", [
    (["misc.loss_uncertainty_weighting=true", "misc.loss_uncertainty_channels=96"], "loss_uncertainty_channels"),
    (["misc.loss_uncertainty_weighting=true", "misc.loss_uncertainty_channels=32"], "loss_uncertainty_channels"),
    (["misc.loss_uncertainty_weighting=true", "misc.loss_uncertainty_channels=512"], "loss_uncertainty_channels"),
    (["misc.loss_uncertainty_weighting=true", "misc.loss_uncertainty_channels=128.5"], "loss_uncertainty_channels"),
    (["misc.loss_uncertainty_weighting=true", "misc.loss_uncertainty_lr=-1e-4"], "loss_uncertainty_lr"),
    (["misc.loss_uncertainty_weighting=true", "misc.loss_uncertainty_lr=fast"], "loss_uncertainty_lr"),
    (["misc.loss_uncertainty_channels=128"], "loss_uncertainty_weighting"),
    (["misc.loss_uncertainty_lr=1e-4"], "loss_uncertainty_weighting"),
    (["misc.loss_uncertainty_weighting=false", "misc.loss_uncertainty_channels=64"], "loss_uncertainty_weighting"),
    (["misc.loss_uncertainty_weighting=maybe"], "loss_uncertainty_weighting"),
])
def test_train_py_refuses_before_anything_is_allocated(overrides, match):
    import train
    with pytest.raises(ValueError, match=match):
        mdcfg.loss_weighting_options(_cfg(*overrides))
    with pytest.raises(ValueError, match=match):
        train.train(_cfg(*overrides))             # refused before a device or a dataset is touched


def test_constructor_refuses_bad_values():
    for ch in (0, 96, 320, 64.0, True):
        with pytest.raises(ValueError):
            lwm.LossWeighting(channels=ch, device="cpu")
    for lr in (-1.0, float("nan"), "x"):
        with pytest.raises(ValueError):
            lwm.LossWeighting(lr=lr, device="cpu")


# ------------------------------------------------------------------------------------------------ the fp64 restatement
def _problem(B, C, seed, wscale=0.1):
    lw = lwm.LossWeighting(channels=C, seed=seed, device="cpu")
    g = torch.Generator().manual_seed(1000 + seed)
    c = 0.6 * torch.randn(B, generator=g) / 4
    w = wscale * torch.randn(C, generator=g, dtype=torch.float64)
    loss = torch.exp(-2 * c.double() + 0.5) * (0.5 + torch.rand(B, generator=g, dtype=torch.float64))
    return lw, c, w, loss


@pytest.mark.parametrize("B, C", [(1, 64), (5, 128), (33, 256)])
def test_reference_gradients_agree_with_autograd(B, C):
    lw, c, w, loss = _problem(B, C, 3)
    gscale = 0.5
    w = w.clone().requires_grad_(True)
    feat = math.sqrt(2.0) * torch.cos(c.double()[:, None] * lw.freq.double()[None] + lw.phase.double()[None])
    u = feat @ w
    u.retain_grad()
    obj = (loss * torch.exp(-u) + u).mean()
    (gscale * obj).backward()
    ur, inv = lwm.ref_forward(c, lw.freq, lw.phase, w.detach())
    du, dw, objr = lwm.ref_backward(c, lw.freq, lw.phase, ur, loss, gscale)
    for name, got, want in (("u", ur, u.detach()), ("inv", inv, torch.exp(-u.detach())), ("du", du, u.grad), ("dw", dw, w.grad),
                            ("objective", objr.reshape(1), obj.detach().reshape(1))):
        worst = float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))
        print(f"B {B} C {C} {name}: worst |ref - autograd| / max|autograd| = {worst:.3g} (bound 1e-12)")
        assert worst <= 1e-12, name


def test_buffers_are_seeded_on_the_cpu_and_w_starts_at_zero():
    a, b, c = (lwm.LossWeighting(seed=s, device="cpu") for s in (7, 7, 8))
    assert torch.equal(a.freq, b.freq) and torch.equal(a.phase, b.phase) and not torch.equal(a.freq, c.freq)
    assert a.freq.dtype == a.phase.dtype == a.w.dtype == torch.float32 and a.freq.shape == (128,)
    assert bool((a.phase >= 0).all()) and bool((a.phase < 2 * math.pi + 1e-6).all())
    assert 0.5 < float(a.freq.std()) / (2 * math.pi) < 1.5
    assert not a.w.any() and not a.m.any() and not a.v.any() and not a.g.any()
    assert a.u_at([-3.0, 0.0, 2.0]) == [0.0, 0.0, 0.0]           # u = 0: the unweighted loss


def test_state_dict_round_trip_and_weights_only():
    src = lwm.LossWeighting(channels=64, seed=5, lr=1e-3, device="cpu")
    g = torch.Generator().manual_seed(2)
    for t in (src.w, src.m, src.v):
        t.copy_(torch.randn(64, generator=g))
    src.v.abs_()
    src.step_count = 17
    sd = src.state_dict()
    assert set(sd) == {"channels", "seed", "freq", "phase", "w", "m", "v", "step"}
    dst = lwm.LossWeighting(channels=64, seed=99, device="cpu")          # other features: the checkpoint's must win
    dst.g.fill_(3.0)
    dst.load_state_dict(sd)
    for name in ("freq", "phase", "w", "m", "v"):
        assert torch.equal(getattr(dst, name), getattr(src, name)), name
    assert dst.step_count == 17 and not dst.g.any()
    assert dst.u_at([0.3, -1.0]) == src.u_at([0.3, -1.0])
    src.w.add_(1.0)
    assert not torch.equal(sd["w"], src.w), "state_dict() must hold copies, not views"
    wo = lwm.LossWeighting(channels=64, seed=99, device="cpu")
    wo.m.fill_(1.0)
    wo.load_state_dict(sd, weights_only=True)
    assert torch.equal(wo.w, sd["w"]) and torch.equal(wo.freq, sd["freq"]) and torch.equal(wo.phase, sd["phase"])
    assert not wo.m.any() and not wo.v.any() and wo.step_count == 0
    with pytest.raises(RuntimeError, match="channels"):
        lwm.LossWeighting(channels=128, device="cpu").load_state_dict(sd)


def test_restore_follows_the_checkpoint_rules():
    src = lwm.LossWeighting(channels=64, seed=5, device="cpu")
    src.w.fill_(0.25)
    src.m.fill_(0.5)
    state = {"model": {}, "loss_weighting": src.state_dict()}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lwm.restore(None, state)                                  # feature off: the key is ignored, nothing is said
        lwm.restore(None, {"model": {}})
        on = lwm.LossWeighting(channels=64, seed=1, device="cpu")
        lwm.restore(on, state)
        assert torch.equal(on.w, src.w) and torch.equal(on.m, src.m)
        wo = lwm.LossWeighting(channels=64, seed=1, device="cpu")
        lwm.restore(wo, state, weights_only=True)
        assert torch.equal(wo.w, src.w) and torch.equal(wo.freq, src.freq) and not wo.m.any()
    fresh = lwm.LossWeighting(channels=64, seed=1, device="cpu")
    with pytest.warns(UserWarning, match="w = 0") as rec:
        lwm.restore(fresh, {"model": {}})
    assert len(rec) == 1 and not fresh.w.any()


def test_checkpoint_state_and_log_line_add_nothing_when_off():
    """train.py's two helpers with the switch off: the keys of today (no GPU: stand-ins for the model and the optimiser)."""
    import train

    class _Dit:
        def state_dict(self):
            return {"a": torch.zeros(1)}

    class _Model:
        dit = _Dit()
        loss_weighting = None

    class _Opt:
        def ema_state_dict(self):
            return None

    class _Trainer:
        loss_weighting = None

    assert set(train.checkpoint_state(_Model(), _Opt())) == {"model"}
    line = train.log_line(3, torch.tensor(0.5), 1e-4, 10.0, None, _Trainer())
    assert set(line) == {"batch", "loss", "lr", "samples_per_sec"}
    m = _Model()
    m.loss_weighting = lwm.LossWeighting(channels=64, device="cpu")
    st = train.checkpoint_state(m, _Opt())
    assert set(st) == {"model", "loss_weighting"} and set(st["model"]) == {"dit.a"}


# ------------------------------------------------------------------------------------------------ the fit condition on the reference
def fit_problem(seed=0):
    """The synthetic fit of the GPU test: L = exp(-2 c + 0.5) with c = 0.6 N(0, 1) / 4; 100 batches of 64 and 4096 held-out levels."""
    g = torch.Generator().manual_seed(4242 + seed)
    train_c = 0.6 * torch.randn(100, 64, generator=g) / 4
    held_c = 0.6 * torch.randn(4096, generator=g) / 4
    return train_c, held_c


def gap_closed(lw, held_c, w):
    L = torch.exp(-2 * held_c.double() + 0.5)
    u, _ = lwm.ref_forward(held_c, lw.freq.cpu(), lw.phase.cpu(), w.cpu())
    top, floor = float(L.mean()), float((1 + torch.log(L)).mean())
    return (top - float(lwm.ref_objective(u, L))) / (top - floor)


def test_reference_meets_the_fit_condition():
    lw = lwm.LossWeighting(channels=128, seed=0, device="cpu")
    train_c, held_c = fit_problem()
    w = torch.zeros(128, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([w], lr=1e-2, betas=lwm.BETAS, eps=lwm.EPS, weight_decay=0.0)
    wr, m, v = torch.zeros(128, dtype=torch.float64), torch.zeros(128, dtype=torch.float64), torch.zeros(128, dtype=torch.float64)
    for i in range(100):
        c = train_c[i]
        L = torch.exp(-2 * c.double() + 0.5)
        u, _ = lwm.ref_forward(c, lw.freq, lw.phase, w.detach())
        _, dw, _ = lwm.ref_backward(c, lw.freq, lw.phase, u, L)
        opt.zero_grad()
        w.grad = dw.clone()
        opt.step()
        ur, _ = lwm.ref_forward(c, lw.freq, lw.phase, wr)
        wr, m, v = lwm.ref_adamw(wr, lwm.ref_backward(c, lw.freq, lw.phase, ur, L)[1], m, v, i + 1, 1e-2)
    closed = gap_closed(lw, held_c, w.detach())
    print(f"fp64 reference with torch.optim.AdamW, 100 steps: closes {closed:.4f} of the gap (bound 0.9)")
    assert closed >= 0.9
    # ref_adamw is torch.optim.AdamW without decay, restated (the same fp64 expressions: rounding-level agreement over 100 steps)
    worst = float((wr - w.detach()).abs().max())
    print(f"ref_adamw against torch.optim.AdamW after 100 steps: max |w - w'| = {worst:.3g} (bound 1e-12)")
    assert worst <= 1e-12


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernel_resources(tmp_path):
    """Tiny kernels on the step path of every microbatch: no scratch, no spills; the backward's three 256-float chunk arrays are its
    only LDS; the loss kernel has its two unweighted forms and the weighted one, none with scratch."""
    from micro_diffusion_amd import hip, native
    res = native.resource_usage("loss_weight.hip", hip.HIPCC_FLAGS, tmp_path / "loss_weight.o")
    fwd = [v for k, v in res.items() if "logvar_fwd_kernel" in k]
    bwd = [v for k, v in res.items() if "logvar_bwd_kernel" in k]
    assert len(fwd) == 1 and len(bwd) == 1, sorted(res)
    for v in fwd + bwd:
        assert v["spill"] == 0 and v["scratch"] == 0, v
    assert fwd[0]["lds"] == 0 and bwd[0]["lds"] == 3 * 256 * 4
    res = native.resource_usage("edm.hip", hip.HIPCC_FLAGS, tmp_path / "edm.o")
    loss = {k: v for k, v in res.items() if "edm_loss_kernel" in k}
    assert len(loss) == 3, sorted(loss)                   # f32 and bf16 gradients unweighted (as before), bf16 weighted
    assert all(v["scratch"] == 0 and v["spill"] == 0 for v in loss.values())
