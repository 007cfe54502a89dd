"""Measurement operators for measurement-guided sampling: what `edm_sampler_loop(..., measurement=)` is guided by.

A measurement states an inverse problem in the sampler's latent space: meas = A(x0) was observed, and the sampler is steered towards
latents whose denoised prediction reproduces it.  This module is torch only (importable without a GPU and without the native library):
the fused sampler reads the operands through `operands()` and runs md_measure_residual; the tensor-op loop and the tests use `loss()`.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


class LinearMeasurement:
    """A(z) = s x s average pooling of z [B, C, H, W] (pool = s; s = 1: the identity), observed as `meas` fp32 [B, C, H / s, W / s], with an
    optional `mask` on the pooled grid ([B or 1, 1, H / s, W / s], [B or 1, H / s, W / s] or [H / s, W / s]; bool, or float in [0, 1];
    broadcast over the channels; 1 = measured, 0 = ignored).  The per-sample loss is L_b = ||m * (meas - A(D))||^2.
      pool = 1, no mask      denoising towards / restoring from a full observation
      pool = 1, mask         restoring from a partial (bool) or blended (float) observation, without pasting it
      pool = s               super-resolution of a latent observed at 1 / s of the resolution
    samplers.check_measurement validates it against the sampler's state."""

    def __init__(self, meas: torch.Tensor, pool: int = 1, mask=None):
        self.meas, self.pool, self.mask = meas, pool, mask

    def apply(self, z: torch.Tensor) -> torch.Tensor:
        """A(z)."""
        return z if self.pool == 1 else F.avg_pool2d(z, self.pool)

    def adjoint(self, v: torch.Tensor) -> torch.Tensor:
        """A^T(v): every pooled value spread over its window, divided by s^2."""
        s = self.pool
        return v if s == 1 else v.repeat_interleave(s, -2).repeat_interleave(s, -1) / (s * s)

    def operands(self, x: torch.Tensor):
        """(meas fp32 contiguous, mask fp32 contiguous [mask_B, H / s * W / s] or None) on x's device, each converted once per run."""
        meas = self.meas.detach().to(device=x.device, dtype=torch.float32).contiguous()
        mask = None
        if self.mask is not None:
            Hs, Ws = meas.shape[-2], meas.shape[-1]
            mask = self.mask.detach().to(device=x.device, dtype=torch.float32).reshape(-1, Hs * Ws).contiguous()
        return meas, mask

    def loss_fn(self, x: torch.Tensor):
        """D [B, C, H, W] -> L [B] as differentiable torch ops on x's device (the tensor-op loop's statement of the loss)."""
        meas, mask = self.operands(x)
        m = None if mask is None else mask.view(mask.shape[0], 1, meas.shape[-2], meas.shape[-1])

        def loss(D):
            r = meas.to(D.dtype) - self.apply(D)
            if m is not None:
                r = m.to(D.dtype) * r
            return (r * r).flatten(1).sum(1)
        return loss
