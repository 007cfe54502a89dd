"""Post-hoc EMA without a GPU: the host maths (micro_diffusion_amd/posthoc_ema.py), the reconstruction on a random walk, the
exported symbols and the config switches.

Bounds.  sigma_rel <-> gamma: the two published pairs (0.05 -> 16.97, 0.10 -> 6.94: Karras et al. 2024, section 3.1) to 1e-3, the
round trip to 1e-12 (a cubic root polished by Newton steps in fp64).  profile_dot against a composite Simpson rule with 200001 nodes
(error ~ h^4 f'''' / 180, far below 1e-6 for these polynomials).  Reconstruction: || rec - target || / || target - theta_final ||
<= 0.01 on a 256-step random walk, where the two tracked averages themselves lie >= 0.2 away (asserted), so returning a tracked
average cannot pass; measured with numpy on the CPU: 4.3e-4 (0.075) and 4.9e-4 (0.15), the tracked averages 0.27 .. 0.66 away."""
import ctypes
import os
import re

import numpy as np
import pytest

from micro_diffusion_amd import config as mdcfg
from micro_diffusion_amd import posthoc_ema as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"md_ema_power_update": 7, "md_ema_power_update_ranges": 9}


# ------------------------------------------------------------------------------------------------ maths
def test_sigma_rel_gamma_round_trip_and_published_values():
    assert abs(ph.sigma_rel_to_gamma(0.05) - 16.972) <= 1e-3
    assert abs(ph.sigma_rel_to_gamma(0.10) - 6.937) <= 1e-3
    for s in (0.01, 0.05, 0.075, 0.10, 0.15, 0.25, 0.279):
        g = ph.sigma_rel_to_gamma(s)
        assert g > 0 and abs(ph.gamma_to_sigma_rel(g) - s) <= 1e-12 * s, (s, g)
    for g in (0.5, 3.0, 6.94, 16.97, 100.0):
        assert abs(ph.sigma_rel_to_gamma(ph.gamma_to_sigma_rel(g)) - g) <= 1e-9 * g
    for bad in (0.0, -0.1, 0.2887, 1.0):
        with pytest.raises(ValueError):
            ph.sigma_rel_to_gamma(bad)


def test_power_beta():
    assert ph.power_beta(1, 6.94) == 0.0
    assert ph.power_beta(2, 1.0) == 0.25
    assert abs(ph.power_beta(1000, 16.97) - (1 - 1e-3) ** 17.97) <= 1e-15
    with pytest.raises(ValueError):
        ph.power_beta(0, 1.0)


def _quad(t_a, g_a, t_b, g_b, nodes=200001):
    """Composite Simpson rule of p_a * p_b on [0, min(t_a, t_b)] (both profiles vanish beyond their own t)."""
    m = min(t_a, t_b)
    tau = np.linspace(0.0, m, nodes)
    f = (g_a + 1) * tau ** g_a / t_a ** (g_a + 1) * (g_b + 1) * tau ** g_b / t_b ** (g_b + 1)
    h = tau[1] - tau[0]
    return h / 3.0 * (f[0] + f[-1] + 4.0 * f[1:-1:2].sum() + 2.0 * f[2:-1:2].sum())


@pytest.mark.parametrize("t_a,g_a,t_b,g_b", [(256.0, 6.94, 256.0, 6.94), (256.0, 16.97, 256.0, 6.94), (100.0, 16.97, 256.0, 6.94),
                                             (256.0, 16.97, 48.0, 6.94), (16.0, 3.0, 17.0, 9.56)])
def test_profile_dot_matches_quadrature(t_a, g_a, t_b, g_b):
    got, ref = ph.profile_dot(t_a, g_a, t_b, g_b), _quad(t_a, g_a, t_b, g_b)
    print(f"profile_dot({t_a}, {g_a}, {t_b}, {g_b}) = {got:.12g}, quadrature {ref:.12g}, rel {abs(got - ref) / ref:.3g}")
    assert abs(got - ref) <= 1e-6 * ref
    assert ph.profile_dot(t_b, g_b, t_a, g_a) == pytest.approx(got, rel=1e-14)


def test_profile_dot_does_not_overflow_at_a_million_steps():
    a = ph.profile_dot(1.0e6, 16.97, 1.0e6, 16.97)
    assert np.isfinite(a) and abs(a - 17.97 ** 2 / (2 * 16.97 + 1) / 1.0e6) <= 1e-12 * a
    b = ph.profile_dot(9.0e5, 16.97, 1.0e6, 6.94)
    assert np.isfinite(b) and b > 0


def _snapshot_grid(last=256, every=16, sigma_rels=(0.05, 0.10)):
    ts, gs = [], []
    for t in range(every, last + 1, every):
        for s in sigma_rels:
            ts.append(float(t))
            gs.append(ph.sigma_rel_to_gamma(s))
    return ts, gs


# ------------------------------------------------------------------------------------------------ snapshot weights
def test_solve_weights_returns_a_unit_vector_for_a_snapshot():
    ts, gs = _snapshot_grid()
    for hit in (len(ts) - 1, len(ts) - 2, 11):
        w = ph.solve_weights(ts, gs, ts[hit], gs[hit])
        rest = np.delete(w, hit)
        print(f"target = snapshot {hit}: w[hit] - 1 = {w[hit] - 1:.3g}, max |other| = {np.abs(rest).max():.3g}")
        assert abs(w[hit] - 1.0) <= 1e-6 and np.abs(rest).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ reconstruction
def _random_walk():
    """256 steps of a 4096-parameter fp32 random walk (steps of 1e-3); the averages 0.05 and 0.10 tracked in fp32 with the kernel's
    expression e = beta * e + (1.f - beta) * p, snapshots every 16 steps; the targets tracked directly in fp64."""
    rng = np.random.default_rng(7)
    n, steps, every = 4096, 256, 16
    tracked = (0.05, 0.10)
    targets = (0.075, 0.15)
    theta = rng.standard_normal(n).astype(np.float32)
    ema = [np.full(n, np.nan, dtype=np.float32) for _ in tracked]
    direct = [np.zeros(n, dtype=np.float64) for _ in targets]
    snaps = []
    for t in range(1, steps + 1):
        theta = (theta + np.float32(1e-3) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
        for k, s in enumerate(tracked):
            b = np.float32(ph.power_beta(t, ph.sigma_rel_to_gamma(s)))
            ema[k] = theta.copy() if b == 0 else (b * ema[k] + (np.float32(1.0) - b) * theta).astype(np.float32)
        for k, s in enumerate(targets):
            b = ph.power_beta(t, ph.sigma_rel_to_gamma(s))
            direct[k] = b * direct[k] + (1.0 - b) * theta.astype(np.float64)
        if t % every == 0:
            for k, s in enumerate(tracked):
                snaps.append({"step": t, "sigma_rel": s, "gamma": ph.sigma_rel_to_gamma(s), "x": ema[k].copy()})
    return theta, ema, dict(zip(targets, direct)), snaps


def test_reconstruction_on_a_random_walk():
    import torch
    theta, ema, direct, snaps = _random_walk()
    assert len(snaps) == 32
    for target, want in direct.items():
        scale = np.linalg.norm(want - theta.astype(np.float64))
        # with numpy alone ...
        w = ph.solve_weights([s["step"] for s in snaps], [s["gamma"] for s in snaps], 256, ph.sigma_rel_to_gamma(target))
        rec = sum(x * s["x"].astype(np.float64) for x, s in zip(w, snaps))
        err = np.linalg.norm(rec - want) / scale
        away = [np.linalg.norm(e.astype(np.float64) - want) / scale for e in ema]
        print(f"sigma_rel {target}: reconstruction error {err:.3g}; the tracked averages lie {away[0]:.3g} and {away[1]:.3g} away; "
              f"sum of weights {w.sum():.6f}, max |w| {np.abs(w).max():.3g}")
        assert min(away) >= 0.2, away
        assert err <= 0.01, err
        # ... and through reconstruct() (torch tensors in, fp64 sums, fp32 out)
        sd = ph.reconstruct([{"state": {"w": torch.from_numpy(s["x"]).view(64, 64)}, "step": s["step"], "sigma_rel": s["sigma_rel"],
                              "gamma": s["gamma"]} for s in snaps], target)
        assert sd["w"].dtype == torch.float32 and tuple(sd["w"].shape) == (64, 64)
        err2 = np.linalg.norm(sd["w"].double().numpy().reshape(-1) - want) / scale
        assert err2 <= 0.01 and abs(err2 - err) <= 1e-4, (err, err2)


def test_reconstruct_ignores_the_future_and_refuses_an_empty_set():
    import torch
    _, _, _, snaps = _random_walk()
    items = [{"state": {"w": torch.from_numpy(s["x"])}, "step": s["step"], "sigma_rel": s["sigma_rel"], "gamma": s["gamma"]} for s in snaps]
    early = ph.reconstruct(items, 0.10, step=128)["w"]
    hit = next(s for s in snaps if s["step"] == 128 and s["sigma_rel"] == 0.10)
    assert np.abs(early.numpy() - hit["x"]).max() <= 1e-5      # a stored profile comes back (unit vector), later snapshots unused
    with pytest.raises(ValueError):
        ph.reconstruct(items, 0.10, step=8)
    with pytest.raises(ValueError):
        ph.reconstruct([], 0.10)


# ------------------------------------------------------------------------------------------------ library and config
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
    assert "#define MD_EMA_MAX_PROFILES 4" in header and hip.EMA_MAX_PROFILES == 4 == ph.MAX_PROFILES
    assert hip.ADAMW_MAX_RANGES == int(re.search(r"#define MD_ADAMW_MAX_RANGES (\d+)", header).group(1))
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6 == lib.md_abi_version(), "two symbols added, none changed"


def test_bad_arguments_are_refused_before_any_launch():
    """The argument checks run on the host in front of the launch: callable without a GPU (fake, aligned addresses)."""
    from micro_diffusion_amd import hip
    L = hip.lib()
    good = 1 << 20
    ev, bv = (ctypes.c_void_p * 4)(good, good, good, good), (ctypes.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    off, cnt = (ctypes.c_int64 * 2)(0, 64), (ctypes.c_int64 * 2)(32, 32)
    assert L.md_ema_power_update(None, ev, bv, 2, 64, None, None) == -1
    assert L.md_ema_power_update(good, None, bv, 2, 64, None, None) == -1
    assert L.md_ema_power_update(good, ev, None, 2, 64, None, None) == -1
    assert L.md_ema_power_update(good, ev, bv, 2, 66, None, None) == -1
    assert L.md_ema_power_update(good, ev, bv, 2, 0, None, None) == -1
    assert L.md_ema_power_update(good, ev, bv, 0, 64, None, None) == -1 and L.md_ema_power_update(good, ev, bv, 5, 64, None, None) == -1
    assert L.md_ema_power_update(good, (ctypes.c_void_p * 4)(good, None, good, good), bv, 2, 64, None, None) == -1
    for b in (1.0, -0.25, float("nan"), 1.5):
        assert L.md_ema_power_update(good, ev, (ctypes.c_float * 4)(0.5, b, 0.5, 0.5), 2, 64, None, None) == -1, b
    assert L.md_ema_power_update_ranges(good, ev, bv, 2, None, cnt, 2, None, None) == -1
    assert L.md_ema_power_update_ranges(good, ev, bv, 2, off, None, 2, None, None) == -1
    assert L.md_ema_power_update_ranges(good, ev, bv, 2, off, cnt, 0, None, None) == -1
    assert L.md_ema_power_update_ranges(good, ev, bv, 2, off, cnt, 65, None, None) == -1
    assert L.md_ema_power_update_ranges(good, ev, bv, 2, (ctypes.c_int64 * 2)(0, 66), cnt, 2, None, None) == -1
    assert L.md_ema_power_update_ranges(good, ev, bv, 2, off, (ctypes.c_int64 * 2)(32, 30), 2, None, None) == -1
    assert L.md_ema_power_update_ranges(good, ev, bv, 5, off, cnt, 2, None, None) == -1


def _cfg(*overrides):
    return mdcfg.load_config(os.path.join(ROOT, "configs"), "res_256_pretrain.yaml", ["exp_name=t", *overrides])


def test_config_switches_parse():
    assert mdcfg.posthoc_ema_options(_cfg()) == {"sigma_rels": (), "snapshot_interval": 0}
    o = mdcfg.posthoc_ema_options(_cfg("misc.posthoc_ema_sigma_rels=[0.05,0.10]", "misc.posthoc_ema_snapshot_interval=4096ba"))
    assert o == {"sigma_rels": (0.05, 0.10), "snapshot_interval": 4096}
    o = mdcfg.posthoc_ema_options(_cfg("misc.posthoc_ema_sigma_rels=[0.05,0.075,0.10,0.15]"))
    assert o == {"sigma_rels": (0.05, 0.075, 0.10, 0.15), "snapshot_interval": 0}
    with pytest.raises(ValueError):
        mdcfg.posthoc_ema_options(_cfg("misc.posthoc_ema_snapshot_interval=16ba"))          # an interval without profiles


@pytest.mark.parametrize("rels", ["[0.05,0.06,0.07,0.08,0.09]", "[0.05,0.28]", "[0.0]", "[-0.05,0.10]", "[0.05,0.3]", "[0.05,0.05]"])
def test_train_py_rejects_what_the_optimiser_cannot_honour(rels):
    import train
    with pytest.raises(ValueError, match="posthoc_ema_sigma_rels"):
        train.train(_cfg("misc.posthoc_ema_sigma_rels=" + rels))          # refused before a device or a dataset is touched


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernel_resources(tmp_path):
    """A bandwidth pass: no scratch, no spills, no LDS and full occupancy in all 8 forms (K = 1 .. 4, flat and ranges); the profile
    pointers are kernel arguments indexed by an unrolled loop, so nothing may land in private memory."""
    from micro_diffusion_amd import hip, native
    res = native.resource_usage("ema.hip", hip.HIPCC_FLAGS, tmp_path / "ema.o")
    kernels = {k: v for k, v in res.items() if "ema_power_kernel" in k}
    assert len(kernels) == 8, sorted(res)
    for name, v in kernels.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["lds"] == 0 and v["occ"] >= 8, (name, v)
