"""Post-hoc EMA, host side (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 3 and
App. C): the maths of the power-function averages the optimiser tracks (FusedAdamW(posthoc_sigma_rels=...), md_ema_power_update)
and the least-squares synthesis of the average for ANY EMA length from the snapshots train.py writes.

A power-function average with exponent gamma, after t steps, weights the weights of step tau <= t by the profile
    p_{t,gamma}(tau) = (gamma + 1) tau^gamma / t^(gamma + 1)       on [0, t],
which the update  e <- beta(t) e + (1 - beta(t)) theta,  beta(t) = (1 - 1/t)^(gamma + 1),  t = 1, 2, ...  realises.  Its width
relative to the training length is sigma_rel = (gamma + 1)^1/2 (gamma + 2)^-1 (gamma + 3)^-1/2, the number a user picks.  Any
target profile is approximated by the combination of the snapshot profiles that is closest to it in L2; the same coefficients
applied to the snapshot tensors give the synthesised weights.

Everything here is fp64 numpy; torch is only touched where snapshot tensors are read and summed (reconstruct)."""
from __future__ import annotations

import glob
import math
import os
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np

MAX_PROFILES = 4              # MD_EMA_MAX_PROFILES
SIGMA_REL_MAX = 0.28          # sigma_rel -> 12^-1/2 = 0.2887 as gamma -> 0: configurations stay clear of the pole


def gamma_to_sigma_rel(gamma: float) -> float:
    g = float(gamma)
    return math.sqrt(g + 1.0) / ((g + 2.0) * math.sqrt(g + 3.0))


def sigma_rel_to_gamma(sigma_rel: float) -> float:
    """The gamma > 0 whose profile has relative width sigma_rel: the largest real root of
    (g + 2)^2 (g + 3) - (g + 1) / sigma_rel^2 = g^3 + 7 g^2 + (16 - s) g + (12 - s),  s = sigma_rel^-2,
    polished by Newton steps on the defining equation."""
    s = float(sigma_rel)
    if not (0.0 < s < 12.0 ** -0.5):
        raise ValueError(f"sigma_rel must lie in (0, {12.0 ** -0.5:.4f}), got {sigma_rel}")
    t = s ** -2
    roots = np.roots([1.0, 7.0, 16.0 - t, 12.0 - t])
    g = float(max(r.real for r in roots if abs(r.imag) < 1e-9 * max(1.0, abs(r.real))))
    for _ in range(4):
        f = (g + 2.0) ** 2 * (g + 3.0) - t * (g + 1.0)
        df = 2.0 * (g + 2.0) * (g + 3.0) + (g + 2.0) ** 2 - t
        g -= f / df
    return g


def power_beta(t: int, gamma: float) -> float:
    """beta of step t (counted from 1): (1 - 1/t)^(gamma + 1); beta(1) = 0, the average starts as a copy of the weights."""
    if t < 1:
        raise ValueError("steps are counted from 1")
    return (1.0 - 1.0 / float(t)) ** (float(gamma) + 1.0)


def profile_dot(t_a: float, g_a: float, t_b: float, g_b: float) -> float:
    """Inner product of the continuous profiles p_{t_a,g_a} and p_{t_b,g_b}:
        (g_a + 1)(g_b + 1) min(t_a, t_b)^(g_a + g_b + 1) / ((g_a + g_b + 1) t_a^(g_a + 1) t_b^(g_b + 1)),
    evaluated as (m / t_a)^(g_a + 1) (m / t_b)^(g_b + 1) / m with m = min(t_a, t_b): both ratios are <= 1, so nothing overflows
    at t ~ 1e6 and gamma ~ 17 (t^(gamma + 1) itself would)."""
    t_a, g_a, t_b, g_b = float(t_a), float(g_a), float(t_b), float(g_b)
    m = min(t_a, t_b)
    return (g_a + 1.0) * (g_b + 1.0) / (g_a + g_b + 1.0) * (m / t_a) ** (g_a + 1.0) * (m / t_b) ** (g_b + 1.0) / m


def solve_weights(snap_t: Sequence[float], snap_gamma: Sequence[float], t_target: float, gamma_target: float) -> np.ndarray:
    """Least-squares coefficients x over ALL snapshots: minimise || sum_i x_i p_{t_i,g_i} - p_{t_target,gamma_target} ||_2, i.e.
    the normal equations A x = b with A_ij = <p_i, p_j>, b_i = <p_i, p_target>, under the constraint sum(x) = 1 (a Lagrange
    multiplier: x = A^-1 b - lambda A^-1 1).  The system is solved with unit diagonal
    (x = D^-1/2 y, (D^-1/2 A D^-1/2) y = D^-1/2 b): the profiles' norms span orders of magnitude over a run."""
    t = np.asarray(snap_t, dtype=np.float64)
    g = np.asarray(snap_gamma, dtype=np.float64)
    if t.ndim != 1 or t.shape != g.shape or t.size == 0:
        raise ValueError("snap_t and snap_gamma must be equally long, non-empty sequences")
    n = t.size
    A = np.empty((n, n), dtype=np.float64)
    b = np.empty(n, dtype=np.float64)
    for i in range(n):
        b[i] = profile_dot(t[i], g[i], t_target, gamma_target)
        for j in range(i, n):
            A[i, j] = A[j, i] = profile_dot(t[i], g[i], t[j], g[j])
    d = 1.0 / np.sqrt(np.diag(A))
    y = np.linalg.solve(A * d[:, None] * d[None, :], np.stack([b * d, d], axis=1)) * d[:, None]      # A^-1 b, A^-1 1
    # every profile integrates to 1, and so must the combination: without this constraint a residual sum(x) - 1 ~ 1e-4 multiplies
    # the WEIGHTS, not their drift over the run, and dominates the error of a trained model (|theta| >> |theta_t - theta_T|)
    lam = (y[:, 0].sum() - 1.0) / y[:, 1].sum()
    return y[:, 0] - lam * y[:, 1]


def snapshot_name(step: int, sigma_rel: float) -> str:
    return f"ema-{int(step):08d}-{float(sigma_rel):.3f}.pt"


def list_snapshots(folder: str) -> List[str]:
    return sorted(glob.glob(os.path.join(folder, "ema-*.pt")))


def reconstruct(snapshots: Union[str, Iterable], sigma_rel: float, step: Optional[int] = None) -> Dict[str, "object"]:
    """The state_dict of the average with relative width `sigma_rel` at training step `step` (default: the last snapshot's step),
    synthesised from the snapshots.  `snapshots`: a folder of train.py's `ema-<step>-<sigma_rel>.pt` files, or an iterable of such
    file names / of already loaded dicts {"state": {name: tensor}, "step", "sigma_rel", "gamma"[, "buffers"]}.
    Snapshots later than `step` are left out (the average at step N may not look at the future).  Tensors are summed in fp64 and returned as fp32."""
    import torch
    items = list_snapshots(snapshots) if isinstance(snapshots, str) else list(snapshots)
    if not items:
        raise ValueError("no snapshots to reconstruct from")

    def meta(it, mmap=False):
        d = torch.load(it, map_location="cpu", mmap=mmap) if isinstance(it, str) else it
        return d, int(d["step"]), float(d["gamma"]) if "gamma" in d else sigma_rel_to_gamma(d["sigma_rel"])
    heads = []
    for it in items:                              # header pass (memory-mapped: no tensor is read), then one snapshot in memory at a time
        d, s, g = meta(it, mmap=True)
        heads.append((s, g))
        del d
    t_target = max(s for s, _ in heads) if step is None else int(step)
    keep = [i for i, (s, _) in enumerate(heads) if s <= t_target]
    if not keep:
        raise ValueError(f"no snapshot at or before step {t_target}")
    w = solve_weights([heads[i][0] for i in keep], [heads[i][1] for i in keep], t_target, sigma_rel_to_gamma(sigma_rel))
    acc: Dict[str, torch.Tensor] = {}
    buffers = {}
    for x, i in zip(w, keep):
        d = meta(items[i])[0]
        state = d["state"]
        if heads[i][0] == max(heads[j][0] for j in keep):
            buffers = d.get("buffers") or buffers          # not averaged: copied from the latest snapshot used
        if acc and set(acc) != set(state):
            raise RuntimeError(f"snapshot {i} holds other parameter names than the first one")
        for k, v in state.items():
            term = v.detach().to("cpu", torch.float64) * float(x)
            acc[k] = term if k not in acc else acc[k].add_(term)
    out = {k: v.to(torch.float32) for k, v in acc.items()}
    out.update({k: v.detach().cpu() for k, v in buffers.items() if k not in out})
    return out
