"""Learned per-noise-level loss weighting for the EDM objective (opt-in): the uncertainty-based loss weighting of
Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 2.2.  No reference counterpart: the
reference trains with the fixed EDM weight (sigma^2 + sigma_d^2) / (sigma sigma_d)^2 alone, which equalises the loss over the noise
levels only at initialisation.

A function u(sigma) of C random Fourier features of c_noise = ln(sigma) / 4 is trained next to the network: every sample's loss is
divided by e^u and pays u for it,

    feat[b, c] = sqrt(2) cos(c_b freq[c] + phase[c])            freq = 2 pi N(0, 1), phase = 2 pi U[0, 1): fixed, drawn once on the CPU
    u_b        = sum_c w[c] feat[b, c]                          w: C trainable weights, zero at the start (u = 0: the unweighted loss)
    objective  = (1 / B) sum_b (L_b e^{-u_b} + u_b)
    dF         = dtok * e^{-u_b}                                per sample, inside md_edm_loss_train_weighted
    du_b       = gscale / B * (1 - e^{-u_b} L_b),   dw[c] += sum_b du_b feat[b, c]

so at its optimum u(sigma) = ln E[L | sigma] and every noise level contributes a gradient of unit magnitude.  On the device all of it
is fp32 HIP (md_logvar_fwd / md_edm_loss_train_weighted / md_logvar_bwd / md_adamw_step[_guarded]); the `ref_*` functions below restate
the formulas in fp64 torch for the tests and for u_at()."""
from __future__ import annotations

import math
import warnings
from typing import Optional

import torch

from . import hip

CHANNEL_CHOICES = (64, 128, 192, 256)        # what md_logvar_fwd / md_logvar_bwd accept: a multiple of 64, 64 <= C <= 256
BETAS, EPS = (0.9, 0.999), 1e-8              # AdamW on w: no weight decay, no clipping


def check_channels(channels) -> int:
    if isinstance(channels, bool) or not isinstance(channels, int) or channels not in CHANNEL_CHOICES:
        raise ValueError(f"loss weighting: channels must be one of {CHANNEL_CHOICES}, got {channels!r}")
    return channels


# ------------------------------------------------------------------------------------------------ fp64 restatement (the reference)
def ref_features(cnoise, freq, phase):
    """feat [B, C] in fp64 from the fp32 (or any) values of cnoise [B], freq [C], phase [C]."""
    a = cnoise.double().reshape(-1, 1) * freq.double().reshape(1, -1) + phase.double().reshape(1, -1)
    return math.sqrt(2.0) * torch.cos(a)


def ref_forward(cnoise, freq, phase, w):
    """(u [B], inv [B]) in fp64."""
    u = ref_features(cnoise, freq, phase) @ w.double()
    return u, torch.exp(-u)


def ref_objective(u, loss):
    """(1 / B) sum_b (L_b e^{-u_b} + u_b) in fp64."""
    return (loss.double() * torch.exp(-u.double()) + u.double()).mean()


def ref_backward(cnoise, freq, phase, u, loss, gscale: float = 1.0):
    """(du [B], dw [C], objective) in fp64 from u (as md_logvar_bwd takes it) and the per-sample losses."""
    feat = ref_features(cnoise, freq, phase)
    u, loss = u.double(), loss.double()
    du = gscale / u.numel() * (1.0 - torch.exp(-u) * loss)
    return du, du @ feat, ref_objective(u, loss)


def ref_adamw(w, g, m, v, step: int, lr: float, betas=BETAS, eps: float = EPS, as_kernel: bool = False):
    """One AdamW step without weight decay in fp64: (w, m, v) after step number `step` (counted from 1).  `as_kernel`: the constants
    as the fp32 numbers md_adamw_step holds (beta, 1.f - beta, the bias corrections, lr, eps: 1.f - 0.999f is 4.7e-5 off 0.001), the
    arithmetic still fp64 -- what the kernel's result is compared with."""
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    if as_kernel:
        f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
        one = torch.tensor(1.0, dtype=torch.float32)
        omb1 = float(one - torch.tensor(b1, dtype=torch.float32))
        omb2 = float(one - torch.tensor(b2, dtype=torch.float32))
        b1, b2, bc1, bc2, lr, eps = f32(b1), f32(b2), f32(bc1), f32(bc2), f32(lr), f32(eps)
    else:
        omb1, omb2 = 1 - b1, 1 - b2
    m = b1 * m.double() + omb1 * g.double()
    v = b2 * v.double() + omb2 * g.double() ** 2
    w = w.double() - lr / bc1 * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return w, m, v


class LossWeighting:
    """The C weights of u(sigma), their fp32 gradient accumulator and AdamW moments, and the fixed feature buffers.  `lr=None`: the
    Trainer passes the optimiser's learning rate (times the schedule factor).  `device="cpu"` holds the state only (state_dict round
    trips, u_at); the kernels need a GPU."""

    def __init__(self, channels: int = 128, seed: int = 0, lr: Optional[float] = None, device="cuda"):
        self.channels = check_channels(channels)
        if lr is not None and not (isinstance(lr, (int, float)) and not isinstance(lr, bool) and lr >= 0 and math.isfinite(lr)):
            raise ValueError(f"loss weighting: lr must be a non-negative number, got {lr!r}")
        self.seed, self.lr = int(seed), (None if lr is None else float(lr))
        gen = torch.Generator(device="cpu").manual_seed(self.seed)          # CPU draws: identical on every rank and every device
        self.freq = (2 * math.pi * torch.randn(channels, generator=gen, dtype=torch.float32)).to(device)
        self.phase = (2 * math.pi * torch.rand(channels, generator=gen, dtype=torch.float32)).to(device)
        self.w = torch.zeros(channels, device=device)
        self.g = torch.zeros(channels, device=device)                       # fp32 gradient accumulator (zeroed by the AdamW launch)
        self.m = torch.zeros(channels, device=device)
        self.v = torch.zeros(channels, device=device)
        self.objective = torch.zeros(1, device=device)                      # weighted objective of the last microbatch
        self.objective_accum = None                                         # set by the Trainer: 1-element f32, += weight * objective
        self.step_count = 0
        self._u = None                                                      # u of the last forward, read by backward

    # -------------------------------------------------------------------------------------------- step path (HIP)
    def forward(self, cnoise: torch.Tensor) -> torch.Tensor:
        """md_logvar_fwd: inv [B] = exp(-u(cnoise)), the per-sample factor of md_edm_loss_train_weighted; u is kept for backward()."""
        B = cnoise.numel()
        u, inv = torch.empty(B, device=cnoise.device), torch.empty(B, device=cnoise.device)
        hip.check(hip.lib().md_logvar_fwd(cnoise.data_ptr(), self.freq.data_ptr(), self.phase.data_ptr(), self.w.data_ptr(), u.data_ptr(),
                                          inv.data_ptr(), B, self.channels, hip.stream_ptr()), "md_logvar_fwd")
        self._u = u
        return inv

    def backward(self, cnoise: torch.Tensor, loss_per_sample: torch.Tensor, gscale: float, obj_accum: Optional[torch.Tensor] = None,
                 accum_weight: float = 0.0) -> torch.Tensor:
        """md_logvar_bwd on the u of the last forward(): g += dw, self.objective = the weighted objective of this microbatch,
        obj_accum (1-element f32 tensor, optional) += accum_weight * objective.  Returns self.objective."""
        if self._u is None or self._u.numel() != cnoise.numel():
            raise RuntimeError("LossWeighting.backward() needs the forward() of the same microbatch first")
        hip.check(hip.lib().md_logvar_bwd(cnoise.data_ptr(), self.freq.data_ptr(), self.phase.data_ptr(), self._u.data_ptr(),
                                          loss_per_sample.data_ptr(), float(gscale), self.g.data_ptr(), self.objective.data_ptr(),
                                          None if obj_accum is None else obj_accum.data_ptr(), float(accum_weight), cnoise.numel(),
                                          self.channels, hip.stream_ptr()), "md_logvar_bwd")
        self._u = None
        return self.objective

    def step(self, lr: float, grad_scale: float = 1.0, guard_state: Optional[torch.Tensor] = None) -> None:
        """One md_adamw_step launch over the C weights: no weight decay, no clipping, the accumulator zeroed.  `guard_state`: the
        optimiser's md_step_guard state -- the guarded launch leaves w and the moments untouched on a skipped step (the accumulator
        is still zeroed; step_count advances as FusedAdamW's does)."""
        self.step_count += 1
        hip.adamw_step(self.w, self.g, self.m, self.v, self.channels, lr=float(lr), betas=BETAS, eps=EPS, weight_decay=0.0,
                       step=self.step_count, grad_scale=float(grad_scale), guard=guard_state)

    # -------------------------------------------------------------------------------------------- host side
    def u_at(self, ln_sigmas) -> list:
        """u at the given ln(sigma) values, fp64 on the host (synchronises)."""
        c = torch.as_tensor(ln_sigmas, dtype=torch.float64).reshape(-1) / 4
        return ref_forward(c, self.freq.cpu(), self.phase.cpu(), self.w.cpu())[0].tolist()

    def state_dict(self) -> dict:
        return {"channels": self.channels, "seed": self.seed, "freq": self.freq.clone(), "phase": self.phase.clone(), "w": self.w.clone(),
                "m": self.m.clone(), "v": self.v.clone(), "step": self.step_count}

    def load_state_dict(self, sd: dict, weights_only: bool = False) -> None:
        """Restores the feature buffers and w (they belong together: w is meaningless under other features), and the moments and the
        step counter unless `weights_only` (a stage hand-off that does not carry the optimiser state: the moments restart at zero)."""
        if int(sd["channels"]) != self.channels:
            raise RuntimeError(f"the checkpoint's loss weighting has {int(sd['channels'])} channels, this run configures {self.channels}")
        for name in ("freq", "phase", "w"):
            getattr(self, name).copy_(sd[name])
        self.seed = int(sd.get("seed", self.seed))
        self.g.zero_()
        if weights_only:
            self.m.zero_()
            self.v.zero_()
            self.step_count = 0
        else:
            self.m.copy_(sd["m"])
            self.v.copy_(sd["v"])
            self.step_count = int(sd["step"])


def restore(lw: Optional[LossWeighting], state: dict, weights_only: bool = False) -> None:
    """What train.py does with the `loss_weighting` entry of a checkpoint's state: restored when the feature is on, ignored when it is
    off; a checkpoint without the entry, loaded with the feature on, starts from w = 0 with one warning."""
    if lw is None:
        return
    sd = state.get("loss_weighting") if isinstance(state, dict) else None
    if sd is None:
        warnings.warn("the checkpoint carries no loss weighting: u(sigma) starts from w = 0")
        return
    lw.load_state_dict(sd, weights_only=weights_only)
