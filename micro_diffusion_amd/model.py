"""Drop-in `LatentDiffusion` / `create_latent_diffusion` (reference micro_diffusion/models/model.py:22-405).

Training path (`forward(batch)` -> EDM loss): sigma sampling, noise add, preconditioning, the whole DiT, the
masked-patch loss and the complete backward run as HIP kernels (engine.py); PyTorch supplies the random draws (in
the reference's order: randn[B,1,1,1], randn_like(x), rand[B,T]) and the autograd hook (`loss.backward()`).
Sampling (`edm_sampler_loop` / `generate`) is inference-only glue around the same HIP forward.
"""
from __future__ import annotations

from functools import partial
import os
import warnings
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import dit as model_zoo
from . import hip
from . import samplers

DATA_TYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


def text_encoder_embedding_format(enc: str):
    """(sequence length, embedding dim) of the supported text encoders (reference utils.py:501-513)."""
    if enc in ("stabilityai/stable-diffusion-2-base", "runwayml/stable-diffusion-v1-5", "CompVis/stable-diffusion-v1-4",
               "openclip:hf-hub:apple/DFN5B-CLIP-ViT-H-14-378"):
        return 77, 1024
    if enc == "DeepFloyd/t5-v1_1-xxl":
        return 120, 4096
    raise ValueError(f"Please specify the sequence and embedding size of {enc} encoder")


def sampler_cache_enabled(flag: Optional[bool] = None) -> bool:
    """The `cond_cache` argument of the sampler: None reads the environment variable MD_SAMPLER_CACHE (default off)."""
    return os.environ.get("MD_SAMPLER_CACHE", "0") == "1" if flag is None else bool(flag)


class DistLoss:
    """Running mean of the per-batch losses (reference utils.py:598-614, without the torchmetrics dependency)."""

    def __init__(self):
        self.loss, self.batches = 0.0, 0

    def update(self, value):
        self.loss = self.loss + value.detach()
        self.batches += 1

    def compute(self):
        return self.loss.float() / self.batches


class _EDMConfig(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class LatentDiffusion(nn.Module):
    def __init__(self, dit: nn.Module, vae, text_encoder, tokenizer, image_key: str = "image", text_key: str = "captions",
                 image_latents_key: str = "image_latents", text_latents_key: str = "caption_latents",
                 precomputed_latents: bool = True, dtype: str = "bfloat16", latent_res: int = 32, p_mean: float = -0.6,
                 p_std: float = 1.2, train_mask_ratio: float = 0.0):
        super().__init__()
        self.dit = dit
        self.vae = vae
        self.image_key, self.text_key = image_key, text_key
        self.image_latents_key, self.text_latents_key = image_latents_key, text_latents_key
        self.precomputed_latents = precomputed_latents
        self.dtype = dtype
        self.latent_res = latent_res
        self.edm_config = _EDMConfig(sigma_min=0.002, sigma_max=80, P_mean=p_mean, P_std=p_std, sigma_data=0.9, num_steps=18,
                                     rho=7, S_churn=0, S_min=0, S_max=float("inf"), S_noise=1)
        self.train_mask_ratio = train_mask_ratio
        self.eval_mask_ratio = 0.0
        # Loss by noise level (opt-in): a diagnostics.LossBySigma; every EDM loss evaluation then adds its per-sample
        # losses to the train or eval table (one md_loss_sigma_hist launch).  None: no launch, no buffer.
        self.loss_by_sigma = None
        # Learned per-noise-level loss weighting (opt-in): a loss_weighting.LossWeighting; the Trainer's microbatch
        # step then runs md_logvar_fwd -> md_edm_loss_train_weighted -> md_logvar_bwd.  None: the launches of today.  Evaluation and
        # sampling never read it.
        self.loss_weighting = None
        # Dispersive loss (opt-in): a disperse.DisperseLoss; the Trainer's microbatch step then arms the engine, which
        # adds weight * L_disp(output of one backbone block) to the objective (Gram, md_disperse_pairs, one injection GEMM in the
        # backward).  None or weight 0: the launches of today.  Evaluation and sampling never read it.
        # disperse_accum: f32 [2] the Trainer hands in per step; += accum_weight * (L, mean off-diagonal D) per microbatch.
        self.disperse = None
        self.disperse_accum = None
        self._disperse_result = None
        assert self.train_mask_ratio >= 0, "Masking ratio must be non-negative!"
        self.randn_like = torch.randn_like
        self.latent_scale = self.vae.config.scaling_factor
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        for frozen in (self.text_encoder, self.vae):
            if isinstance(frozen, nn.Module):
                frozen.requires_grad_(False)

    # ---------------------------------------------------------------------------------------- training step
    def _inputs(self, batch: dict):
        """(latents, conditioning, per-sample caption scale or None) of a batch (model.py:105-135)."""
        if self.precomputed_latents and self.image_latents_key in batch:
            latents = batch[self.image_latents_key]        # already multiplied by the VAE scaling factor
        else:
            with torch.no_grad():
                images = batch[self.image_key]
                latents = self.vae.encode(images.to(DATA_TYPES[self.dtype]))["latent_dist"].sample().data
                latents *= self.latent_scale
        if self.precomputed_latents and self.text_latents_key in batch:
            conditioning = batch[self.text_latents_key]
        else:
            captions = batch[self.text_key]
            captions = captions.view(-1, captions.shape[-1])
            if "attention_mask" in batch:
                conditioning = self.text_encoder.encode(captions, attention_mask=batch["attention_mask"].view(-1, captions.shape[-1]))[0]
            else:
                conditioning = self.text_encoder.encode(captions)[0]
        # Dropped captions (model.py:131-135 multiplies the batch tensor by the 0/1 mask in place; forward() does the same).  For
        # the Trainer's microbatch loop the mask rides along as a per-sample row scale of the first kernel that touches the
        # captions (md_cast_rows_bf16): no torch op on the step path.
        drop = batch.get("drop_caption_mask") if hasattr(batch, "get") else None
        if drop is not None:
            drop = drop.reshape(-1)
            if drop.dtype != torch.float32 or not drop.is_contiguous():
                drop = drop.float().contiguous()
        return latents, conditioning, drop

    def forward(self, batch: dict):
        """(loss, latents, conditioning) as model.py:104-142, including its side effect: dropped captions are zeroed by an
        IN-PLACE multiply of the conditioning tensor (model.py:131-135), so the returned `conditioning` -- and, with precomputed
        latents, the caller's batch['caption_latents'], which is the same tensor -- hold zeros in the dropped rows, exactly what
        a Composer callback / update_metric sees from the reference.  (This is the drop-in surface.  The Trainer's microbatch
        loop, train_microbatch, leaves the batch as the loader produced it and applies the mask as a row scale inside the
        first kernel that reads the captions; the mask is 0 / 1, so applying it on both routes is idempotent.)"""
        latents, conditioning, drop = self._inputs(batch)
        if drop is not None:
            conditioning *= drop.to(conditioning.dtype).view([-1] + [1] * (conditioning.dim() - 1))
        loss = self.edm_loss(latents, conditioning, mask_ratio=self.train_mask_ratio if self.training else self.eval_mask_ratio)
        return (loss, latents, conditioning)

    def _draws(self, x: torch.Tensor, T: int, mask_ratio: float):
        """The three random draws in the reference's order (model.py:182,188, utils.py:390): randn[B,1,1,1], randn_like(x.float()),
        rand[B,T]."""
        B = x.shape[0]
        rnd = torch.randn([B, 1, 1, 1], device=x.device)
        if x.dtype == torch.float32:
            eps = self.randn_like(x)
        elif self.randn_like is torch.randn_like:
            eps = torch.randn_like(x, dtype=torch.float32)
        else:
            eps = self.randn_like(x.float())
        mnoise = torch.rand(B, T, device=x.device) if mask_ratio > 0 else None
        return rnd, eps, mnoise

    def _prep(self, x, y, mask_ratio, _noise):
        dit = self.dit
        dit._ensure_flat()
        dit.refresh_shadow()
        x = x.detach()
        if x.dtype not in (torch.float16, torch.float32):
            x = x.float()
        x = x.contiguous()
        B = x.shape[0]
        T = (x.shape[-2] // dit.patch_size) * (x.shape[-1] // dit.patch_size)
        if _noise is None and getattr(self, "_noise_fn", None) is not None:
            _noise = self._noise_fn(B)            # test hook: recorded (rnd_normal, eps, mask_noise) per call
        rnd, eps, mnoise = self._draws(x, T, mask_ratio) if _noise is None else _noise
        if mask_ratio > 0:
            assert dit.training, "Masking is only recommended during training"
        if not (torch.is_grad_enabled() and y.requires_grad):     # (a y that requires grad: the conversions stay differentiable torch ops)
            y = y.detach()
        if y.dtype not in (torch.float16, torch.float32):
            y = y.float()
        y = y.contiguous()
        rnd = rnd.reshape(B)
        if rnd.dtype != torch.float32 or not rnd.is_contiguous():
            rnd = rnd.float().contiguous()
        if eps.dtype != torch.float32 or not eps.is_contiguous():
            eps = eps.float().contiguous()
        return x, y, rnd, eps, mnoise

    def edm_loss(self, x: torch.Tensor, y: torch.Tensor, mask_ratio: float = 0, _noise=None, _y_rowscale=None, **kwargs) -> torch.Tensor:
        """model.py:181-210 on the HIP engine.  `_noise=(rnd_normal, eps, mask_noise)` injects the three random
        draws (parity tests); otherwise they are drawn here in the reference's order.  `_y_rowscale` [B] f32: per-sample
        factor on the caption rows (the caption-drop mask).
        Gradients: the parameters' (when they require grad) and d loss / d y when y requires grad -- through the same
        row factor, so a dropped caption gets an exactly zero gradient; with a frozen network the backward is the engine's dgrad-only
        one.  The gradient with respect to the clean latents x is NOT provided: x is detached here."""
        if self.disperse is not None and self.disperse.enabled and torch.is_grad_enabled() and next(self.dit.parameters()).requires_grad:
            raise RuntimeError("the dispersive loss is armed (LatentDiffusion.disperse): its gradient exists only on the "
                               "Trainer's microbatch path (train_microbatch); the autograd surface would train the network on the "
                               "unregularised loss.  Disarm it or run under torch.no_grad()")
        x, y, rnd, eps, mnoise = self._prep(x, y, mask_ratio, _noise)
        dit = self.dit
        need_grad = torch.is_grad_enabled() and dit._plist[0].requires_grad
        if need_grad and self.loss_weighting is not None:
            raise RuntimeError("the learned loss weighting is armed (LatentDiffusion.loss_weighting): its gradient exists only on the "
                               "Trainer's microbatch path (train_microbatch); the autograd surface would train the network on the "
                               "unweighted loss.  Disarm it or run under torch.no_grad()")
        args = (self, dit._grad_anchor, x, y, rnd, eps, mnoise, float(mask_ratio), _y_rowscale)
        if need_grad or (torch.is_grad_enabled() and y.requires_grad):
            return _EDMLossFunction.apply(*args)
        return _edm_forward(*args)[0]

    def train_microbatch(self, batch: dict, grad_scale: float = 1.0, loss_accum: Optional[torch.Tensor] = None,
                         accum_weight: float = 0.0, _noise=None) -> torch.Tensor:
        """forward + backward of one microbatch WITHOUT autograd: what `(model(batch)[0] * grad_scale).backward()` does
        (Composer's microbatch loop around model.py:104-142), as one explicit launch sequence — every operation on device
        data is a HIP kernel of libmicrodit_hip (the three random draws are torch's).  Parameter gradients accumulate in the
        flat fp32 buffer (the .grad views); `loss_accum` (1-element f32 tensor) += accum_weight * loss on the device.
        Returns the microbatch loss (device scalar)."""
        latents, conditioning, drop = self._inputs(batch)
        mask_ratio = self.train_mask_ratio if self.training else self.eval_mask_ratio
        x, y, rnd, eps, mnoise = self._prep(latents, conditioning, mask_ratio, _noise)
        dit = self.dit
        dl, eng = self.disperse, dit._engine
        if dl is not None and dl.enabled and dit.training:
            acc = self.disperse_accum
            eng.disperse = (dl.resolve_block(len(eng.backbone)), dl.weight, dl.tau)
            eng.disperse_train = (float(grad_scale), None if acc is None else acc[0:1], None if acc is None else acc[1:2],
                                  float(accum_weight))
        try:
            loss, tape, dtb = _edm_forward(self, None, x, y, rnd, eps, mnoise, float(mask_ratio), drop,
                                           train=(float(grad_scale), loss_accum, float(accum_weight)))
        finally:
            eng.disperse = None
        if getattr(tape, "disperse", None) is not None:
            self._disperse_result = tape.disperse.result
        dit.attach_grads()
        dit._engine.backward(tape, dtb, on_segment=getattr(dit, "_on_segment", None))
        return loss

    def model_forward_wrapper(self, x, sigma, y, model_forward_fxn, mask_ratio: float, **kwargs) -> dict:
        """EDM preconditioning around an arbitrary forward fn (model.py:144-179); used by the sampler."""
        sd = self.edm_config.sigma_data
        sigma = sigma.to(x.dtype).reshape(-1, 1, 1, 1)
        c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
        c_out = sigma * sd / (sigma ** 2 + sd ** 2).sqrt()
        c_in = 1 / (sd ** 2 + sigma ** 2).sqrt()
        c_noise = sigma.log() / 4
        out = model_forward_fxn((c_in * x).to(x.dtype), c_noise.flatten(), y, mask_ratio=mask_ratio, **kwargs)
        out["sample"] = c_skip * x + c_out * out["sample"]
        return out

    # Composer-style hooks (model.py:212-229)
    def loss(self, outputs, batch):
        return outputs[0]

    def eval_forward(self, batch, outputs=None):
        if outputs is not None:
            return outputs
        loss, _, _ = self.forward(batch)
        return loss, None, None

    def get_metrics(self, is_train: bool = False):
        return {"loss": DistLoss()}

    def update_metric(self, batch, outputs, metric):
        metric.update(outputs[0])

    # ---------------------------------------------------------------------------------------- sampling (inference glue)
    def _churned_levels(self, t_steps, n):
        """t_hat of every step (model.py:254-257) from the host-side noise levels: t_cur * (1 + gamma), gamma > 0 inside [S_min, S_max]."""
        ec = self.edm_config
        return [t + (min(ec.S_churn / n, np.sqrt(2) - 1) if ec.S_min <= t <= ec.S_max else 0) * t for t in t_steps[:-1]]

    @torch.no_grad()
    def edm_sampler_loop(self, x, y, steps: Optional[int] = None, cfg: float = 1.0, fused: Optional[bool] = None,
                         cond_cache: Optional[bool] = None, sampler: str = "heun", guidance_interval=None, guide=None,
                         guide_captions: str = "same", init_latents=None, strength: float = 1.0, inpaint_mask=None, resample: int = 1,
                         guidance_mode: str = "cfg", guidance_rescale: float = 0.0, apg_eta: float = 0.0, apg_norm_threshold=None,
                         apg_momentum: float = 0.0, measurement=None, measurement_scale: float = 1.0, guidance_loss=None, step_cache=None,
                         **kwargs):
        """EDM sampler, fp64 state (model.py:231-297).  `fused` (None = whenever possible) selects the loop whose per-step arithmetic
        runs in fused HIP kernels; False keeps the reference's tensor-op formulation (generic forward functions).
        `cond_cache` (None = the environment variable MD_SAMPLER_CACHE, default off): encode the captions once for the whole run
        and step in token space (see _edm_sampler_fused); needs the fused loop.  Results are bit-identical to the uncached loop.
        `sampler`: "heun" (the reference's 2nd-order loop, 2 * steps - 1 network evaluations), "euler" or "dpmpp_2m" (DPM-Solver++(2M),
        2nd order); the last two take one evaluation per step (samplers.py).  S_churn > 0 is defined for heun and euler.
        `guidance_interval` = (sigma_lo, sigma_hi): an evaluation at noise level sigma is guided (batch doubled) only while
        sigma_lo <= sigma <= sigma_hi; outside it the conditional half runs alone.  None: every evaluation is guided when cfg > 1.
        `guide`: a second, weaker DiT on the same device (autoguidance, Karras et al. 2024).  cfg is then the autoguidance weight w:
        a guided evaluation runs this model at batch B, then the guide at batch B on the same network input, and the update combines
        F = F_guide + w * (F_main - F_guide); no evaluation is batch-doubled.  Unguided evaluations (cfg <= 1, outside the interval)
        never run the guide.  `guide_captions`: "same" (the guide sees the captions) or "null" (zeroed captions; with guide = this
        model's own dit that is classifier-free guidance as two batch-B launches).
        Image-conditioned sampling (this loop with fused=False is the definition, the fused loop follows it):
        `init_latents` (fp32, the shape of x, in the sampler's space: VAE latents * latent_scale): image-to-image.  With
        k = max(1, min(n, ceil(strength * n))) and i0 = n - k the state starts as init_latents + t_i0 * x and steps i0 ... n - 1 run;
        euler / dpmpp_2m take their coefficients from the truncated schedule, so the first executed step has no history.
        `strength` in (0, 1]: 1 runs every step (the start is then init_latents + sigma_max * x).
        `inpaint_mask` ([B or 1, 1, H, W], [B or 1, H, W] or [H, W]; bool, or float in [0, 1]; broadcast over the channels): 1 = generate,
        0 = keep init_latents, values between blend.  At the start of every executed step i, before the churn,
        x_cur <- m * x_cur + (1 - m) * (init_latents + t_i * randn_like(x_cur)), and after the last step x <- m * x + (1 - m) * init_latents:
        where m == 0 the result is init_latents bit for bit.  Heun's second evaluation is not re-blended: it sees the first half-step's
        state as it is.  With a mask the churn draw is made only when S_churn > 0 (without one the loop keeps the reference's draw).
        `resample` = r >= 1 (RePaint, Lugmayr et al. 2022; needs a mask; heun and euler): every step with t_next > 0 runs r times, and
        after each repetition but the last x <- x + sqrt(t_i^2 - t_next^2) * randn_like(x) takes the state back to level t_i.  Draws of one
        repetition, in order: blend, churn (S_churn > 0), the step, re-noise.  samplers.edit_evaluations counts the evaluations.
        `guidance_mode`: how a guided evaluation combines the conditional denoised prediction D_c with the second operand
        D_u (the unconditional half, or the guide's).  "cfg": D_u + cfg * (D_c - D_u) inside the update kernel, the default (its
        launches and bits are untouched).  "rescale" (`guidance_rescale` = phi in [0, 1]): the cfg result scaled by phi * std(D_c) / std(result) + 1 - phi per
        sample.  "apg" (`apg_eta`, `apg_norm_threshold` = r or None, `apg_momentum` = beta in (-1, 1)): the update M = (D_c - D_u) +
        beta * M_prev of the previous guided evaluation, clipped to norm r per sample, its component parallel to D_c weighted by eta.
        Both are alpha_b * D_c + gamma_b * M with per-sample coefficients (samplers.guidance_coefficients); they compose with every
        argument above, and cfg <= 1 or an evaluation outside the interval runs unguided as in "cfg".
        Measurement-guided sampling (Chung et al. 2023; this loop with fused=False is the definition): `measurement`, an
        inverse.LinearMeasurement (A = s x s average pooling, an observation meas = A(x0), an optional mask), or `guidance_loss`, a callable
        taking the denoised prediction D (fp32 [B, C, H, W], requires grad) and returning per-sample losses [B] through differentiable torch
        ops; one of the two.  At the first evaluation of every executed step (state x_hat, after the blend and the churn) the guided
        prediction D gives L_b (for a measurement ||m * (meas - A(D))||^2), the solver computes x_next as without guidance (Heun's second
        evaluation is not differentiated, dpmpp_2m's history holds the uncorrected D), and then
        x_next[b] -= measurement_scale / max(sqrt(L_b), samplers.GUIDE_TINY) * dL_b/dx_hat, the gradient taken through the network, before
        the RePaint re-noise.  The network is frozen for the run (requires_grad is restored afterwards, no .grad is written).  Composes with
        the solvers, churn, guidance_interval, cond_cache, init_latents / inpaint_mask / resample; not done: with `guide`, with a
        guidance_mode other than "cfg", with extra forward arguments.
        `step_cache`: a step_cache.StepCache.  Evaluations its policy does not declare full skip the backbone blocks and
        add back what those blocks contributed in the last full evaluation; the embeddings, the patch mixer and the final layer always
        run.  Evaluations are counted from the run's own schedule (heun: two per step, resample repetitions included); the first and the
        last are always full, and so is the first at another network batch (the edge of a guidance_interval).  It needs the fused loop
        and composes with the solvers, churn, guidance_interval, the guidance modes, cond_cache and init_latents / inpaint_mask /
        resample; not defined with `guide`, `measurement` or `guidance_loss` (ValueError).  step_cache.stats describes the run.  None:
        the launches and bits of a run without the argument."""
        ec = self.edm_config
        samplers.check_sampler(sampler, ec.S_churn)
        caching = samplers.check_step_cache(step_cache, guide, measurement, guidance_loss)
        guided_by = samplers.check_measurement(tuple(x.shape), measurement, measurement_scale, guidance_loss)
        if guided_by:
            for bad, what in ((guide is not None, "a guide network (autoguidance)"), (guidance_mode != "cfg", f"guidance_mode={guidance_mode!r}"),
                              (bool(kwargs), f"extra forward arguments {sorted(kwargs)}")):
                if bad:
                    raise NotImplementedError(f"measurement / guidance_loss with {what}: not done (DESIGN.md 4.18)")
        interval = samplers.guidance_interval_bounds(guidance_interval)
        samplers.check_guide(self.dit, guide, guide_captions)
        samplers.check_guidance(guidance_mode, cfg, guidance_rescale, apg_eta, apg_norm_threshold, apg_momentum)
        gmode = None                                # (mode, phi, eta, r or None, beta) of a run that is guided in a mode other than "cfg"
        if guidance_mode != "cfg" and cfg > 1.0:
            gmode = (guidance_mode, float(guidance_rescale), float(apg_eta), None if apg_norm_threshold is None else float(apg_norm_threshold),
                     float(apg_momentum))
        samplers.check_edit(sampler, init_latents is not None, strength, inpaint_mask is not None, resample)
        n = ec.num_steps if steps is None else steps
        edit = None if init_latents is None else self._edit_operands(x, init_latents, strength, inpaint_mask, resample, n)
        can_fuse = not kwargs and x.is_cuda
        cond_cache = sampler_cache_enabled(cond_cache)
        if cond_cache and (fused is False or not can_fuse):
            raise RuntimeError("cond_cache needs the fused sampler: no extra forward arguments, CUDA tensors")
        if caching and (fused is False or not can_fuse):
            raise ValueError("step_cache needs the fused sampler: no extra forward arguments, CUDA tensors")
        if fused is None:
            fused = can_fuse
        if fused:
            assert can_fuse, "the fused sampler needs CUDA tensors and no extra forward arguments"
            if not guided_by:
                return self._edm_sampler_fused(x, y, steps, cfg, cond_cache, sampler, interval, guide, guide_captions == "null", edit, gmode,
                                               step_cache=step_cache)
            guidance = (measurement, guidance_loss, float(measurement_scale))
            with self._frozen_network():
                return self._edm_sampler_fused(x, y, steps, cfg, cond_cache, sampler, interval, None, False, edit, None, guidance)
        if guided_by:
            with self._frozen_network():
                return self._edm_sampler_guided_ops(x, y, n, cfg, sampler, interval, edit, measurement, guidance_loss, float(measurement_scale))
        if guide is not None:
            fwd = self._autoguided_forward(guide, torch.zeros_like(y) if guide_captions == "null" else y, cfg) if cfg > 1.0 else self.dit.forward
        else:
            fwd = partial(self.dit.forward, cfg=cfg) if cfg > 1.0 else self.dit.forward

        def denoise(xs, sigma):
            f = fwd if interval is None or interval[0] <= float(sigma) <= interval[1] else self.dit.forward
            return self.model_forward_wrapper(xs.to(torch.float32), sigma.to(torch.float32), y, f, mask_ratio=0, **kwargs)["sample"].to(torch.float64)
        if gmode is not None:
            denoise = self._mode_guided_denoise(denoise, y, cfg, interval, guide, guide_captions == "null", gmode, kwargs)
        idx = torch.arange(n, dtype=torch.float64, device=x.device)
        inv_rho = 1 / ec.rho
        t_steps = (ec.sigma_max ** inv_rho + idx / (n - 1) * (ec.sigma_min ** inv_rho - ec.sigma_max ** inv_rho)) ** ec.rho
        t_steps = torch.cat([t_steps, torch.zeros_like(t_steps[:1])])
        x0, m, i0, resample = (None, None, 0, 1) if edit is None else edit
        if m is not None:                           # [mask_B, H * W] fp32 -> broadcast over the channels of the fp64 state
            m = m.view(m.shape[0], 1, x.shape[-2], x.shape[-1]).to(torch.float64)
        if sampler != "heun":
            levels = t_steps.tolist()
            coef = samplers.solver_coefficients(sampler, levels[i0:], self._churned_levels(levels, n)[i0:])
        reps = samplers.edit_repetitions(t_steps.tolist(), i0, resample) if resample > 1 else [1] * (n - i0)
        draw_churn = m is None or ec.S_churn > 0
        x_next = x.to(torch.float64) * t_steps[0] if edit is None else x0 + t_steps[i0] * x.to(torch.float64)
        for i in range(i0, n):
            t_cur, t_next = t_steps[i], t_steps[i + 1]
            for rep in range(reps[i - i0]):
                x_cur = x_next
                if m is not None:
                    x_cur = m * x_cur + (1 - m) * (x0 + t_cur * self.randn_like(x_cur))
                gamma = min(ec.S_churn / n, np.sqrt(2) - 1) if ec.S_min <= t_cur <= ec.S_max else 0
                t_hat = torch.as_tensor(t_cur + gamma * t_cur)
                x_hat = x_cur + (t_hat ** 2 - t_cur ** 2).sqrt() * ec.S_noise * self.randn_like(x_cur) if draw_churn else x_cur
                den = denoise(x_hat, t_hat)
                if sampler != "heun":               # one evaluation per step: x_next = a x_hat + b (c1 D - c2 D_prev)
                    a, b, c1, c2 = coef[i - i0]
                    x_next = a * x_hat + b * (c1 * den - c2 * hist if c2 != 0 else c1 * den)
                    hist = den
                else:
                    d_cur = (x_hat - den) / t_hat
                    x_next = x_hat + (t_next - t_hat) * d_cur
                    if i < n - 1:
                        den = denoise(x_next, t_next)
                        d_prime = (x_next - den) / t_next
                        x_next = x_hat + (t_next - t_hat) * (0.5 * d_cur + 0.5 * d_prime)
                if rep < reps[i - i0] - 1:          # RePaint: back to level t_cur for the next repetition
                    x_next = x_next + (t_cur ** 2 - t_next ** 2).sqrt() * self.randn_like(x_next)
        if m is not None:
            x_next = m * x_next + (1 - m) * x0
        return x_next.to(torch.float32)

    def _edit_operands(self, x, init_latents, strength, inpaint_mask, resample, n):
        """(init_latents as fp64, the mask as contiguous fp32 [mask_B, H * W] or None, i0, resample) on x's device, each converted once;
        ValueError for latents of another shape, a mask that does not broadcast over [B, 1, H, W] or a float mask outside [0, 1]."""
        if tuple(init_latents.shape) != tuple(x.shape):
            raise ValueError(f"init_latents has shape {tuple(init_latents.shape)}, the noise {tuple(x.shape)}: they must agree")
        x0 = init_latents.detach().to(device=x.device, dtype=torch.float64).contiguous()
        m = None
        if inpaint_mask is not None:
            B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
            shape = tuple(inpaint_mask.shape)
            ok = (shape == (H, W) or (len(shape) == 3 and shape[0] in (1, B) and shape[1:] == (H, W))
                  or (len(shape) == 4 and shape[0] in (1, B) and shape[1] == 1 and shape[2:] == (H, W)))
            if not ok:
                raise ValueError(f"inpaint_mask has shape {shape}: expected [{B} or 1, 1, {H}, {W}], [{B} or 1, {H}, {W}] or [{H}, {W}]")
            m = inpaint_mask.detach().to(device=x.device, dtype=torch.float32).reshape(-1, H * W).contiguous()
            if inpaint_mask.dtype != torch.bool and not bool(((m >= 0) & (m <= 1)).all()):
                raise ValueError("inpaint_mask must be bool or hold values in [0, 1] (1 = generate, 0 = keep init_latents)")
        return x0, m, samplers.edit_start_index(n, strength), resample

    def _frozen_network(self):
        """Context of a guided sampling run: every parameter of the network has requires_grad False inside (the backward to the image
        is the engine's dgrad-only one and writes no .grad), and what it was before afterwards."""
        from contextlib import contextmanager

        @contextmanager
        def frozen():
            params = list(self.dit.parameters())
            was = [p.requires_grad for p in params]
            for p in params:
                p.requires_grad_(False)
            try:
                yield
            finally:
                for p, r in zip(params, was):
                    p.requires_grad_(r)
        return frozen()

    def _edm_sampler_guided_ops(self, x, y, n, cfg, sampler, interval, edit, measurement, guidance_loss, zeta):
        """The tensor-op loop of edm_sampler_loop with measurement guidance: the definition the fused loop follows.  The
        step's first evaluation runs model_forward_wrapper under torch.enable_grad() on the fp32 x_hat, torch.autograd.grad of L.sum() gives
        g = dL/dx_hat through the (frozen) network, and the correction is applied in fp64 to the solver's result."""
        ec = self.edm_config
        loss_fn = guidance_loss if measurement is None else measurement.loss_fn(x)
        fwd = partial(self.dit.forward, cfg=cfg) if cfg > 1.0 else self.dit.forward

        def pick(sigma):
            return fwd if interval is None or interval[0] <= float(sigma) <= interval[1] else self.dit.forward

        def denoise(xs, sigma):
            return self.model_forward_wrapper(xs.to(torch.float32), sigma.to(torch.float32), y, pick(sigma), mask_ratio=0)["sample"].to(torch.float64)

        def denoise_with_gradient(xs, sigma):
            """(D, g, L): the guided prediction at xs, dL/dxs and the per-sample losses, the last two in fp64."""
            with torch.enable_grad():
                x32 = xs.to(torch.float32).detach().requires_grad_(True)
                D = self.model_forward_wrapper(x32, sigma.to(torch.float32), y, pick(sigma), mask_ratio=0)["sample"]
                L = loss_fn(D)
                g, = torch.autograd.grad(L.sum(), x32)
            return D.detach().to(torch.float64), g.to(torch.float64), L.detach().to(torch.float64)
        idx = torch.arange(n, dtype=torch.float64, device=x.device)
        inv_rho = 1 / ec.rho
        t_steps = (ec.sigma_max ** inv_rho + idx / (n - 1) * (ec.sigma_min ** inv_rho - ec.sigma_max ** inv_rho)) ** ec.rho
        t_steps = torch.cat([t_steps, torch.zeros_like(t_steps[:1])])
        x0, m, i0, resample = (None, None, 0, 1) if edit is None else edit
        if m is not None:
            m = m.view(m.shape[0], 1, x.shape[-2], x.shape[-1]).to(torch.float64)
        if sampler != "heun":
            levels = t_steps.tolist()
            coef = samplers.solver_coefficients(sampler, levels[i0:], self._churned_levels(levels, n)[i0:])
        reps = samplers.edit_repetitions(t_steps.tolist(), i0, resample) if resample > 1 else [1] * (n - i0)
        draw_churn = m is None or ec.S_churn > 0
        x_next = x.to(torch.float64) * t_steps[0] if edit is None else x0 + t_steps[i0] * x.to(torch.float64)
        for i in range(i0, n):
            t_cur, t_next = t_steps[i], t_steps[i + 1]
            for rep in range(reps[i - i0]):
                x_cur = x_next
                if m is not None:
                    x_cur = m * x_cur + (1 - m) * (x0 + t_cur * self.randn_like(x_cur))
                gamma = min(ec.S_churn / n, np.sqrt(2) - 1) if ec.S_min <= t_cur <= ec.S_max else 0
                t_hat = torch.as_tensor(t_cur + gamma * t_cur)
                x_hat = x_cur + (t_hat ** 2 - t_cur ** 2).sqrt() * ec.S_noise * self.randn_like(x_cur) if draw_churn else x_cur
                den, g, L = denoise_with_gradient(x_hat, t_hat)
                if sampler != "heun":
                    a, b, c1, c2 = coef[i - i0]
                    x_next = a * x_hat + b * (c1 * den - c2 * hist if c2 != 0 else c1 * den)
                    hist = den                      # the uncorrected prediction
                else:
                    d_cur = (x_hat - den) / t_hat
                    x_next = x_hat + (t_next - t_hat) * d_cur
                    if i < n - 1:
                        den = denoise(x_next, t_next)
                        d_prime = (x_next - den) / t_next
                        x_next = x_hat + (t_next - t_hat) * (0.5 * d_cur + 0.5 * d_prime)
                x_next = x_next - (zeta / L.sqrt().clamp_min(samplers.GUIDE_TINY)).view(-1, 1, 1, 1) * g
                if rep < reps[i - i0] - 1:
                    x_next = x_next + (t_cur ** 2 - t_next ** 2).sqrt() * self.randn_like(x_next)
        if m is not None:
            x_next = m * x_next + (1 - m) * x0
        return x_next.to(torch.float32)

    def _mode_guided_denoise(self, unguided, y, w: float, interval, guide, guide_null: bool, gmode, kwargs):
        """denoise(xs, sigma) of the tensor-op loop in guidance mode "rescale" or "apg" (DESIGN.md 4.14), in plain torch: the
        preconditioning of model_forward_wrapper (fp32) around one doubled-batch forward without cfg=, or with a guide around two
        forwards; D_c = c_skip x + c_out F_c as everywhere, D_c - D_u = c_out (F_c - F_u) (c_skip x cancels), and the running difference,
        the moments and the combine in fp64.  Outside the interval `unguided` runs and M stays."""
        mode, phi, eta, r, beta = gmode
        sd = self.edm_config.sigma_data
        state = {"M": None}                         # the M of the previous guided evaluation of this run
        y_u = y if guide is not None and not guide_null else torch.zeros_like(y)

        def denoise(xs, sigma):
            if not (interval is None or interval[0] <= float(sigma) <= interval[1]):
                return unguided(xs, sigma)
            xs, sigma = xs.to(torch.float32), sigma.to(torch.float32).reshape(-1, 1, 1, 1)
            c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
            c_out = sigma * sd / (sigma ** 2 + sd ** 2).sqrt()
            net_in, c_noise = (1 / (sd ** 2 + sigma ** 2).sqrt()) * xs, (sigma.log() / 4).flatten()
            if guide is None:
                F = self.dit.forward(torch.cat([net_in, net_in], 0), c_noise, torch.cat([y, y_u], 0), mask_ratio=0, **kwargs)["sample"]
                F_c, F_u = torch.split(F.to(torch.float32), len(F) // 2, dim=0)
            else:
                F_c = self.dit.forward_without_cfg(net_in, c_noise, y, mask_ratio=0, **kwargs)["sample"].to(torch.float32)
                F_u = guide.forward_without_cfg(net_in, c_noise, y_u, mask_ratio=0, **kwargs)["sample"].to(torch.float32)
            D_c = (c_skip * xs + c_out * F_c).to(torch.float64)
            M = c_out.to(torch.float64) * (F_c.to(torch.float64) - F_u.to(torch.float64))
            if mode == "apg" and beta != 0.0 and state["M"] is not None:
                M = M + beta * state["M"]
            state["M"] = M
            alpha, gamma = samplers.guidance_coefficients(mode, samplers.guidance_moments(D_c, M), D_c[0].numel(), w, phi, eta, r)
            return alpha.view(-1, 1, 1, 1) * D_c + gamma.view(-1, 1, 1, 1) * M
        return denoise

    def _autoguided_forward(self, guide, y_guide, w: float):
        """The forward function of an autoguided evaluation for model_forward_wrapper: both networks on the same input at batch B, the
        guide with its own captions, combined in fp32 as the update kernels do (F = F_guide + w * (F_main - F_guide))."""
        def fwd(x, t, y, **kwargs):
            fm = self.dit.forward_without_cfg(x, t, y, **kwargs)["sample"].to(torch.float32)
            fg = guide.forward_without_cfg(x, t, y_guide, **kwargs)["sample"].to(torch.float32)
            return {"sample": fg + w * (fm - fg)}
        return fwd

    @torch.no_grad()
    def _edm_sampler_fused(self, x, y, steps: Optional[int], cfg: float, cond_cache: bool = False, sampler: str = "heun", interval=None,
                           guide=None, guide_null: bool = False, edit=None, gmode=None, guidance=None, step_cache=None):
        """The same loops with everything around the network evaluations in fused HIP kernels: md_edm_sampler_input (c_in scaling +
        guidance batch doubling) and md_edm_heun_update (guidance combine + preconditioning + fp64 Euler / Heun update) or, for
        euler / dpmpp_2m, md_edm_solver_update (the same with the linear-multistep update of samplers.solver_coefficients).
        S_churn > 0: the noise is drawn once per step as in the tensor-op loop and md_edm_churn adds it to the state in place.
        cond_cache: the captions (doubled under guidance) are encoded once (dit.encode_condition) and every evaluation runs
        md_edm_sampler_patchify -> engine.forward(patches=, cond=) -> md_edm_heun_update_tok / md_edm_solver_update_tok on the token
        output: no caption-side work per evaluation and no fp32 image between the fp64 state and the network's bf16 rows.
        interval: evaluations outside it run the conditional half alone (network batch B) on leading-row views of the same buffers.
        guide: nothing is doubled.  A guided evaluation writes the network input once (dup = 0), runs self.dit and then the guide on it
        at batch B (the guide with its own captions / its own Conditioning, encoded by the guide) and hands the two outputs to
        md_edm_*_update_guide(_tok).  Both outputs are fresh allocations that network() returns together, so main's is alive and
        untouched while the guide runs and until the update has been enqueued.
        edit = (init_latents fp64, mask fp32 [mask_B, H * W] or None, i0, resample) from _edit_operands: md_edm_blend_known writes the
        SDEdit start into the state (in place on the fp64 copy of x, which is its noise operand), blends the known latents at level t_i
        into x_cur at the start of every repetition (one draw, one launch) and pastes them after the last step; a repetition that is
        not the last ends with one draw and md_edm_churn in place on the state it produced (x_cur after the swap).  None: none of it.
        gmode = (mode, phi, eta, r or None, beta) of guidance mode "rescale" / "apg" (DESIGN.md 4.14): M (fp32, the state's layout), coef
        [B, 2] and moments [B, 5] are allocated once; every guided evaluation runs md_guidance_prepare(_tok) on the two outputs -- the
        halves of the doubled batch, or main's and the guide's -- and then the _coef form of its update kernel, which reads the
        conditional output, M and coef.  Nothing comes back to the host.  None ("cfg"): none of it.
        guidance = (inverse.LinearMeasurement or None, loss callable or None, scale) of measurement-guided sampling (no guide,
        no gmode): the first evaluation of every step keeps a tape -- cond_cache: engine.forward(patches=, cond=, input_tape=True), the
        captions stay frozen in the cache; otherwise engine.forward(net_in, y, record_tape=True) --, then md_edm_denoised(_tok) -> D,
        md_measure_residual -> q = dL/dD and L (or the callable under torch.enable_grad(), torch autograd supplying q),
        md_guide_cotangent_tok -> the bf16 cotangent of both halves of the output, engine.backward(("x",), param_grads=False) -> the
        gradient of the network input, which stops at the image; the tape is dropped, the step's usual update runs (Heun's second
        evaluation without a tape) and md_edm_guide_apply corrects its result in place.  None: none of it.
        step_cache: a step_cache.StepCache (no guide, no guidance): it is reset for the run's evaluation count, and every
        network() call hands the engine its ResidualCache and a decision callback (StepCache.engine_args) -- through engine.forward with
        cond_cache, through dit.forward_without_cfg without.  None: none of it."""
        ec, L, st = self.edm_config, hip.lib(), torch.cuda.current_stream().cuda_stream
        n = ec.num_steps if steps is None else steps
        idx = torch.arange(n, dtype=torch.float64)
        inv_rho = 1 / ec.rho
        t_steps = (ec.sigma_max ** inv_rho + idx / (n - 1) * (ec.sigma_min ** inv_rho - ec.sigma_max ** inv_rho)) ** ec.rho
        t_steps = torch.cat([t_steps, torch.zeros(1, dtype=torch.float64)]).tolist()
        heun, churn = sampler == "heun", ec.S_churn > 0
        t_hats = self._churned_levels(t_steps, n) if churn else t_steps[:-1]
        x0, mask, i0, resample = (None, None, 0, 1) if edit is None else edit
        levels = [s for i in range(i0, n) for s in ([t_hats[i]] + ([t_steps[i + 1]] if heun and i < n - 1 else []))]
        guided = any(samplers.is_guided(s, cfg, interval) for s in levels)      # no guided evaluation at all: the cfg = 1 run
        B, numel = x.shape[0], x.numel()
        if not guided:
            gmode = None
        if gmode is not None:
            g_kind = {"rescale": hip.GUIDANCE_RESCALE, "apg": hip.GUIDANCE_APG}[gmode[0]]
            g_par = (g_kind, float(cfg), gmode[1], gmode[2], 0 if gmode[3] is None else 1, 1.0 if gmode[3] is None else gmode[3], gmode[4])
            g_M = torch.empty(tuple(x.shape), device=x.device, dtype=torch.float32)
            g_coef = torch.empty(B, 2, device=x.device, dtype=torch.float32)
            g_moments = torch.empty(B, 5, device=x.device, dtype=torch.float64)
            g_evals = [0]                           # guided evaluations so far: the first one does not read M

        def blend_known(noise, m, sigma):
            """x_cur <- m * x_cur + (1 - m) * (x0 + sigma * noise); m None: the whole state, noise None: x0 itself."""
            hip.check(L.md_edm_blend_known(x_cur.data_ptr(), x0.data_ptr(), None if noise is None else noise.data_ptr(),
                                           None if m is None else m.data_ptr(), B, x.shape[1], x.shape[2] * x.shape[3],
                                           1 if m is None else m.shape[0], float(sigma), st), "md_edm_blend_known")
        if edit is None:
            x_cur = (x.to(torch.float64) * t_steps[0]).contiguous()
        else:
            # always a copy: the kernel writes the start into it in place, and an fp64 contiguous x would otherwise be the caller's tensor
            x_cur = x.to(torch.float64, copy=True, memory_format=torch.contiguous_format)
            blend_known(x_cur, None, t_steps[i0])
        x_nxt, d_cur = torch.empty_like(x_cur), torch.empty_like(x_cur)
        auto = guide is not None and guided         # with a guide the second operand comes from it: the batch is never doubled
        y2 = torch.cat([y, torch.zeros_like(y)], 0) if guided and not auto else y
        Bn = 2 * B if guided and not auto else B
        if auto:
            y_g = torch.zeros_like(y) if guide_null else y
        if cond_cache:
            dit = self.dit
            C, H, W, p = x.shape[1], x.shape[2], x.shape[3], dit.patch_size
            cond = dit.encode_condition(y2)
            if auto:
                cond_g = guide.encode_condition(y_g)
            patches = torch.empty(Bn * (H // p) * (W // p), dit.config.patch_vec, device=x.device, dtype=torch.bfloat16)
        else:
            net_in = torch.empty((Bn,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)

        if guidance is not None:
            g_meas, g_loss, g_zeta = guidance
            dit = self.dit
            C, H, W, p = x.shape[1], x.shape[2], x.shape[3], dit.patch_size
            g_T = (H // p) * (W // p)
            if g_meas is not None:
                g_m, g_mask = g_meas.operands(x)
            g_D, g_q = (torch.empty(tuple(x.shape), device=x.device, dtype=torch.float32) for _ in range(2))
            g_L = torch.empty(B, device=x.device, dtype=torch.float64)
            g_dtok = torch.empty(Bn * g_T, dit.config.patch_vec, device=x.device, dtype=torch.bfloat16)

        def network_with_gradient(xs, sigma):
            """network(xs, sigma) for a measurement-guided step's first evaluation, and the gradient of the network input under the
            loss: returns ((network output, dup, None), dx fp32 [B or 2B, C, H, W]); q and L are left in g_q and g_L."""
            c_noise = float(np.log(np.float32(sigma)) / 4)
            dup = 1 if guided and samplers.is_guided(sigma, cfg, interval) else 0
            Be = 2 * B if dup else B
            eng = dit.engine
            if cond_cache:
                pt = patches if Be == Bn else patches[:B * g_T]
                hip.check(L.md_edm_sampler_patchify(xs.data_ptr(), pt.data_ptr(), B, C, H, W, p, float(sigma), ec.sigma_data, dup, st),
                          "md_edm_sampler_patchify")
                t = torch.full((Be,), c_noise, device=x.device, dtype=torch.float32)
                tape = eng.forward(None, t, None, cond=cond.narrow(Be), patches=pt, input_tape=True)
                F = tape.out_tok
                hip.check(L.md_edm_denoised_tok(xs.data_ptr(), F.data_ptr(), g_D.data_ptr(), B, C, H, W, p, float(cfg), dup, float(sigma),
                                                ec.sigma_data, st), "md_edm_denoised_tok")
            else:
                hip.check(L.md_edm_sampler_input(xs.data_ptr(), net_in.data_ptr(), numel, float(sigma), ec.sigma_data, dup, st),
                          "md_edm_sampler_input")
                t = torch.full((1,), c_noise, device=x.device, dtype=torch.float32)
                dit.refresh_shadow()
                tape = eng.forward(net_in if Be == Bn else net_in[:B], t, dit._caption_input(y2 if Be == Bn else y), record_tape=True)
                F = eng.sample_image(tape)
                hip.check(L.md_edm_denoised(xs.data_ptr(), F.data_ptr(), g_D.data_ptr(), B, numel // B, float(cfg), dup, float(sigma),
                                            ec.sigma_data, st), "md_edm_denoised")
            if g_meas is not None:
                hip.check(L.md_measure_residual(g_D.data_ptr(), g_m.data_ptr(), None if g_mask is None else g_mask.data_ptr(),
                                                1 if g_mask is None else g_mask.shape[0], g_q.data_ptr(), g_L.data_ptr(), B, C, H, W,
                                                g_meas.pool, st), "md_measure_residual")
            else:
                with torch.enable_grad():
                    Dg = g_D.detach().clone().requires_grad_(True)
                    loss = g_loss(Dg)
                    gq, = torch.autograd.grad(loss.sum(), Dg)
                g_q.copy_(gq)
                g_L.copy_(loss.detach().reshape(B))
            dtok = g_dtok if Be == Bn else g_dtok[:B * g_T]
            hip.check(L.md_guide_cotangent_tok(g_q.data_ptr(), dtok.data_ptr(), B, C, H, W, p, float(cfg), dup, float(sigma), ec.sigma_data, st),
                      "md_guide_cotangent_tok")
            dx = eng.backward(tape, dtok, input_grads=("x",), param_grads=False).dx
            return (F, dup, None), dx

        def guide_apply(dx, dup, sigma):
            """The correction of the step's result x_nxt along g = c_skip q + c_in (dx_c + dx_u), the coefficients of level sigma."""
            hip.check(L.md_edm_guide_apply(x_nxt.data_ptr(), g_q.data_ptr(), dx.data_ptr(), g_L.data_ptr(), B, numel // B, dup, g_zeta,
                                           float(sigma), ec.sigma_data, st), "md_edm_guide_apply")

        def sc_args(Be):
            """The step-cache arguments of the main network's next evaluation at batch Be (none without a step cache)."""
            return {} if step_cache is None else step_cache.engine_args(self.dit.engine, Be)

        def network(xs, sigma):
            """(network output, dup, guide output) for state xs at noise level sigma: the fp32 image F, or (cond_cache) the bf16 token
            rows; dup = 1 when the evaluation is guided by batch doubling: the output holds the unconditional half behind the
            conditional.  With a guide dup is 0 and a guided evaluation returns the guide's output as well (else None)."""
            c_noise = float(np.log(np.float32(sigma)) / 4)
            g_eval = guided and samplers.is_guided(sigma, cfg, interval)
            dup = 1 if g_eval and not auto else 0
            Be = 2 * B if dup else B
            if cond_cache:
                pt = patches if Be == Bn else patches[:B * (H // p) * (W // p)]
                hip.check(L.md_edm_sampler_patchify(xs.data_ptr(), pt.data_ptr(), B, C, H, W, p, float(sigma), ec.sigma_data, dup, st),
                          "md_edm_sampler_patchify")
                t = torch.full((Be,), c_noise, device=x.device, dtype=torch.float32)
                F = dit._engine.forward(None, t, None, cond=cond.narrow(Be), patches=pt, **sc_args(Be)).out_tok
                Fg = guide._engine.forward(None, t, None, cond=cond_g, patches=pt).out_tok if auto and g_eval else None
                return F, dup, Fg
            hip.check(L.md_edm_sampler_input(xs.data_ptr(), net_in.data_ptr(), numel, float(sigma), ec.sigma_data, dup, st),
                      "md_edm_sampler_input")
            t = torch.full((1,), c_noise, device=x.device, dtype=torch.float32)
            if Be == Bn:
                F = self.dit.forward_without_cfg(net_in, t, y2, 0, **sc_args(Be))["sample"].contiguous()
            else:
                F = self.dit.forward_without_cfg(net_in[:B], t, y, 0, **sc_args(Be))["sample"].contiguous()
            Fg = guide.forward_without_cfg(net_in, t, y_g, 0)["sample"].to(torch.float32).contiguous() if auto and g_eval else None
            return F, dup, Fg

        def prepare(Fd, x_in, t_in):
            """In a guidance mode, for a guided evaluation: M, the moments and the coefficients from the two outputs; True when it ran."""
            F, dup, Fg = Fd
            if gmode is None or not (dup or Fg is not None):
                return False
            Fu = Fg.data_ptr() if Fg is not None else F.data_ptr() + (F.numel() // 2) * F.element_size()
            first = 1 if g_evals[0] == 0 else 0
            g_evals[0] += 1
            if cond_cache:
                hip.check(L.md_guidance_prepare_tok(x_in.data_ptr(), F.data_ptr(), Fu, g_M.data_ptr(), g_coef.data_ptr(), g_moments.data_ptr(),
                                                    B, C, H, W, p, t_in, ec.sigma_data, *g_par, first, st), "md_guidance_prepare_tok")
            else:
                hip.check(L.md_guidance_prepare(x_in.data_ptr(), F.data_ptr(), Fu, g_M.data_ptr(), g_coef.data_ptr(), g_moments.data_ptr(),
                                                B, numel // B, t_in, ec.sigma_data, *g_par, first, st), "md_guidance_prepare")
            return True

        def update(Fd, x_in, t_in, t_hat, t_next, second):
            """x_nxt (and, on the first half-step, d_cur) from x_cur, the evaluated state x_in and the network output F."""
            F, dup, Fg = Fd
            if prepare(Fd, x_in, t_in):
                if cond_cache:
                    hip.check(L.md_edm_heun_update_coef_tok(x_cur.data_ptr(), x_in.data_ptr(), F.data_ptr(), g_M.data_ptr(), g_coef.data_ptr(),
                                                            d_cur.data_ptr(), x_nxt.data_ptr(), B, C, H, W, p, t_in, t_hat, t_next,
                                                            ec.sigma_data, second, st), "md_edm_heun_update_coef_tok")
                else:
                    hip.check(L.md_edm_heun_update_coef(x_cur.data_ptr(), x_in.data_ptr(), F.data_ptr(), g_M.data_ptr(), g_coef.data_ptr(),
                                                        d_cur.data_ptr(), x_nxt.data_ptr(), B, numel // B, t_in, t_hat, t_next, ec.sigma_data,
                                                        second, st), "md_edm_heun_update_coef")
            elif Fg is not None and cond_cache:
                hip.check(L.md_edm_heun_update_guide_tok(x_cur.data_ptr(), x_in.data_ptr(), F.data_ptr(), Fg.data_ptr(), d_cur.data_ptr(),
                                                         x_nxt.data_ptr(), B, C, H, W, p, float(cfg), t_in, t_hat, t_next, ec.sigma_data,
                                                         second, st), "md_edm_heun_update_guide_tok")
            elif Fg is not None:
                hip.check(L.md_edm_heun_update_guide(x_cur.data_ptr(), x_in.data_ptr(), F.data_ptr(), Fg.data_ptr(), d_cur.data_ptr(),
                                                     x_nxt.data_ptr(), numel, float(cfg), t_in, t_hat, t_next, ec.sigma_data, second, st),
                          "md_edm_heun_update_guide")
            elif cond_cache:
                hip.check(L.md_edm_heun_update_tok(x_cur.data_ptr(), x_in.data_ptr(), F.data_ptr(), d_cur.data_ptr(), x_nxt.data_ptr(),
                                                   B, C, H, W, p, float(cfg), dup, t_in, t_hat, t_next, ec.sigma_data, second, st),
                          "md_edm_heun_update_tok")
            else:
                hip.check(L.md_edm_heun_update(x_cur.data_ptr(), x_in.data_ptr(), F.data_ptr(), d_cur.data_ptr(), x_nxt.data_ptr(), numel,
                                               float(cfg), dup, t_in, t_hat, t_next, ec.sigma_data, second, st), "md_edm_heun_update")

        def solver_update(Fd, t_in, coef):
            """x_nxt = a x_cur + b (c1 D - c2 hist), hist = D; d_cur is the history buffer."""
            F, dup, Fg = Fd
            if prepare(Fd, x_cur, t_in):
                if cond_cache:
                    hip.check(L.md_edm_solver_update_coef_tok(x_cur.data_ptr(), F.data_ptr(), g_M.data_ptr(), g_coef.data_ptr(), d_cur.data_ptr(),
                                                              x_nxt.data_ptr(), B, C, H, W, p, t_in, ec.sigma_data, *coef, st),
                              "md_edm_solver_update_coef_tok")
                else:
                    hip.check(L.md_edm_solver_update_coef(x_cur.data_ptr(), F.data_ptr(), g_M.data_ptr(), g_coef.data_ptr(), d_cur.data_ptr(),
                                                          x_nxt.data_ptr(), B, numel // B, t_in, ec.sigma_data, *coef, st),
                              "md_edm_solver_update_coef")
            elif Fg is not None and cond_cache:
                hip.check(L.md_edm_solver_update_guide_tok(x_cur.data_ptr(), F.data_ptr(), Fg.data_ptr(), d_cur.data_ptr(), x_nxt.data_ptr(),
                                                           B, C, H, W, p, float(cfg), t_in, ec.sigma_data, *coef, st),
                          "md_edm_solver_update_guide_tok")
            elif Fg is not None:
                hip.check(L.md_edm_solver_update_guide(x_cur.data_ptr(), F.data_ptr(), Fg.data_ptr(), d_cur.data_ptr(), x_nxt.data_ptr(), numel,
                                                       float(cfg), t_in, ec.sigma_data, *coef, st), "md_edm_solver_update_guide")
            elif cond_cache:
                hip.check(L.md_edm_solver_update_tok(x_cur.data_ptr(), F.data_ptr(), d_cur.data_ptr(), x_nxt.data_ptr(), B, C, H, W, p,
                                                     float(cfg), dup, t_in, ec.sigma_data, *coef, st), "md_edm_solver_update_tok")
            else:
                hip.check(L.md_edm_solver_update(x_cur.data_ptr(), F.data_ptr(), d_cur.data_ptr(), x_nxt.data_ptr(), numel, float(cfg), dup,
                                                 t_in, ec.sigma_data, *coef, st), "md_edm_solver_update")
        coefs = None if heun else samplers.solver_coefficients(sampler, t_steps[i0:], t_hats[i0:])
        reps = samplers.edit_repetitions(t_steps, i0, resample) if resample > 1 else [1] * (n - i0)
        if step_cache is not None:                  # the run's evaluations: every repetition of a step, heun twice but for the last step
            step_cache.reset(sum(r * (2 if heun and i < n - 1 else 1) for i, r in zip(range(i0, n), reps)))
        for i in range(i0, n):
            t_cur, t_next, t_hat = t_steps[i], t_steps[i + 1], t_hats[i]
            for rep in range(reps[i - i0]):
                # .to(float64).contiguous() on a draw, here and below, does nothing for torch.randn_like on the fp64 state: it is there for
                # a replaced self.randn_like (a recorded or fp32 generator), whose result the kernels must still read as contiguous fp64
                if mask is not None:                # the known region at this step's noise level, one fresh draw
                    blend_known(self.randn_like(x_cur).to(torch.float64).contiguous(), mask, t_cur)
                if churn:                           # one draw per step, churned or not: the draws of the tensor-op loop
                    noise = self.randn_like(x_cur)
                    if t_hat != t_cur:              # x_cur becomes x_hat (x_cur itself is not read again)
                        noise = noise.to(torch.float64).contiguous()
                        hip.check(L.md_edm_churn(x_cur.data_ptr(), noise.data_ptr(), x_cur.data_ptr(), numel,
                                                 float(np.sqrt(t_hat ** 2 - t_cur ** 2) * ec.S_noise), st), "md_edm_churn")
                Fd, g_dx = (network(x_cur, t_hat), None) if guidance is None else network_with_gradient(x_cur, t_hat)
                if heun:
                    update(Fd, x_cur, t_hat, t_hat, t_next, 0)
                    if i < n - 1:
                        update(network(x_nxt, t_next), x_nxt, t_next, t_hat, t_next, 1)      # not differentiated: no tape
                else:
                    solver_update(Fd, t_hat, coefs[i - i0])
                if g_dx is not None:
                    guide_apply(g_dx, Fd[1], t_hat)
                x_cur, x_nxt = x_nxt, x_cur
                if rep < reps[i - i0] - 1:          # RePaint: the state this repetition produced goes back to level t_cur
                    noise = self.randn_like(x_cur).to(torch.float64).contiguous()
                    hip.check(L.md_edm_churn(x_cur.data_ptr(), noise.data_ptr(), x_cur.data_ptr(), numel,
                                             float(np.sqrt(t_cur ** 2 - t_next ** 2)), st), "md_edm_churn")
        if mask is not None:
            blend_known(None, mask, 0.0)
        return x_cur.to(torch.float32)

    @torch.no_grad()
    def generate(self, prompt: Optional[list] = None, tokenized_prompts=None, attention_mask=None, guidance_scale: float = 5.0,
                 num_inference_steps: int = 30, seed: Optional[int] = None, return_only_latents: bool = False,
                 cond_cache: Optional[bool] = None, sampler: str = "heun", guidance_interval=None, guide=None,
                 guide_captions: str = "same", init_latents=None, strength: float = 1.0, inpaint_mask=None, resample: int = 1,
                 guidance_mode: str = "cfg", guidance_rescale: float = 0.0, apg_eta: float = 0.0, apg_norm_threshold=None,
                 apg_momentum: float = 0.0, measurement=None, measurement_scale: float = 1.0, guidance_loss=None, step_cache=None, **kwargs):
        """tokenise -> text encoder -> EDM sampler on the HIP DiT -> VAE decode (model.py:299-353).  cond_cache, sampler,
        guidance_interval, guide and guide_captions: as in edm_sampler_loop (with a guide, guidance_scale is the autoguidance weight).
        init_latents, strength, inpaint_mask and resample: image-to-image and inpainting as in edm_sampler_loop; the seeded draw below is
        then the unit noise added to init_latents.  init_latents are latents already (VAE latents * latent_scale, the space of the
        trainer's image_latents): encoding an image into them stays the caller's vae.encode, a frozen third-party model.
        guidance_mode, guidance_rescale, apg_eta, apg_norm_threshold and apg_momentum: CFG rescale and adaptive projected guidance as in
        edm_sampler_loop; they tame the over-saturation of plain guidance at this default guidance_scale.
        measurement, measurement_scale and guidance_loss: measurement-guided sampling as in edm_sampler_loop (the measurement lives in the
        sampler's latent space, like init_latents).
        step_cache: a step_cache.StepCache, as in edm_sampler_loop."""
        samplers.check_step_cache(step_cache, guide, measurement, guidance_loss)
        samplers.check_measurement(None, measurement, measurement_scale, guidance_loss)
        samplers.check_guide(self.dit, guide, guide_captions)
        samplers.check_guidance(guidance_mode, guidance_scale, guidance_rescale, apg_eta, apg_norm_threshold, apg_momentum)
        samplers.check_edit(sampler, init_latents is not None, strength, inpaint_mask is not None, resample)
        assert prompt or tokenized_prompts is not None, "Must provide either prompt or tokenized prompts"
        device = next(self.dit.parameters()).device
        gen = torch.Generator(device=device)
        if seed:
            gen = gen.manual_seed(seed)
        if tokenized_prompts is None:
            out = self.tokenizer.tokenize(prompt)
            tokenized_prompts = out["input_ids"]
            attention_mask = out.get("attention_mask")
        emb = self.text_encoder.encode(tokenized_prompts.to(device),
                                       attention_mask=attention_mask.to(device) if attention_mask is not None else None)[0]
        latents = torch.randn((len(emb), self.dit.in_channels, self.latent_res, self.latent_res), device=device, generator=gen)
        latents = self.edm_sampler_loop(latents, emb, num_inference_steps, cfg=guidance_scale, cond_cache=cond_cache, sampler=sampler,
                                        guidance_interval=guidance_interval, guide=guide, guide_captions=guide_captions,
                                        init_latents=init_latents, strength=strength, inpaint_mask=inpaint_mask, resample=resample,
                                        guidance_mode=guidance_mode, guidance_rescale=guidance_rescale, apg_eta=apg_eta,
                                        apg_norm_threshold=apg_norm_threshold, apg_momentum=apg_momentum, measurement=measurement,
                                        measurement_scale=measurement_scale, guidance_loss=guidance_loss, step_cache=step_cache)
        if return_only_latents:
            return latents
        image = self.vae.decode((latents / self.latent_scale).to(DATA_TYPES[self.dtype])).sample
        return (image / 2 + 0.5).clamp(0, 1).float().detach()


def _edm_forward(model: LatentDiffusion, anchor, x, y, rnd, eps, mnoise, mask_ratio, y_rowscale=None, train=None,
                 record_tape: bool = False):
    """Forward half of the fused training step.  Returns (loss scalar tensor, tape, dtok).
    train = (grad_scale, loss_accum, accum_weight): the Trainer's autograd-free form — the tape goes to the engine's
    fixed-address arena and dtok comes back as bf16, already multiplied by grad_scale (md_edm_loss_train).  Otherwise dtok is
    fp32 and unscaled (the autograd node scales it by the upstream gradient)."""
    dit = model.dit
    eng = dit._engine
    L = hip.lib()
    st = torch.cuda.current_stream().cuda_stream
    ec = model.edm_config
    B, C, H, W = x.shape
    dev = x.device
    xn = torch.empty(x.shape, device=dev, dtype=torch.float32)
    sigma, cin, cnoise = (torch.empty(B, device=dev) for _ in range(3))
    if x.dtype == torch.float16:
        x0 = torch.empty(x.shape, device=dev, dtype=torch.float32)
        hip.check(L.md_edm_prepare_f16(x.data_ptr(), eps.data_ptr(), rnd.data_ptr(), xn.data_ptr(), x0.data_ptr(), sigma.data_ptr(),
                                       cin.data_ptr(), cnoise.data_ptr(), B, C * H * W, ec.P_mean, ec.P_std, ec.sigma_data, st),
                  "md_edm_prepare_f16")
    else:
        x0 = x
        hip.check(L.md_edm_prepare(x.data_ptr(), eps.data_ptr(), rnd.data_ptr(), xn.data_ptr(), sigma.data_ptr(), cin.data_ptr(),
                                   cnoise.data_ptr(), B, C * H * W, ec.P_mean, ec.P_std, ec.sigma_data, st), "md_edm_prepare")
    tape = eng.forward(xn, cnoise, y, mask_ratio=mask_ratio, mask_noise=mnoise, in_scale=cin, y_rowscale=y_rowscale,
                       record_tape=record_tape or train is not None, arena=train is not None)
    lps = torch.empty(B, device=dev)
    loss = torch.empty(1, device=dev)
    keep = None if tape.keep_rows is None else tape.keep_rows.data_ptr()
    lw = model.loss_weighting if train is not None else None
    if train is not None:
        gscale, accum, aw = train
        dtok = torch.empty(B * tape.Tk, dit.config.patch_vec, device=dev, dtype=torch.bfloat16)
    if lw is not None:
        inv = lw.forward(cnoise)
        hip.check(L.md_edm_loss_train_weighted(tape.out_tok.data_ptr(), keep, xn.data_ptr(), x0.data_ptr(), sigma.data_ptr(), lps.data_ptr(),
                                               loss.data_ptr(), dtok.data_ptr(), gscale, None if accum is None else accum.data_ptr(), aw,
                                               B, tape.Tk, C, H, W, dit.patch_size, ec.sigma_data, inv.data_ptr(), st),
                  "md_edm_loss_train_weighted")
        lw.backward(cnoise, lps, gscale, lw.objective_accum, aw)
    elif train is not None:
        hip.check(L.md_edm_loss_train(tape.out_tok.data_ptr(), keep, xn.data_ptr(), x0.data_ptr(), sigma.data_ptr(), lps.data_ptr(),
                                      loss.data_ptr(), dtok.data_ptr(), gscale, None if accum is None else accum.data_ptr(), aw, B,
                                      tape.Tk, C, H, W, dit.patch_size, ec.sigma_data, st), "md_edm_loss_train")
    else:
        dtok = torch.empty(B * tape.Tk, dit.config.patch_vec, device=dev) if record_tape else None
        hip.check(L.md_edm_loss(tape.out_tok.data_ptr(), keep, xn.data_ptr(), x0.data_ptr(), sigma.data_ptr(), lps.data_ptr(),
                                loss.data_ptr(), None if dtok is None else dtok.data_ptr(), B, tape.Tk, C, H, W, dit.patch_size,
                                ec.sigma_data, st), "md_edm_loss")
    tape.loss_per_sample = lps
    if model.loss_by_sigma is not None:
        model.loss_by_sigma.accumulate(sigma, lps, dit.training)
    return loss.reshape(()), tape, dtok


class _EDMLossFunction(torch.autograd.Function):
    """loss = EDM(x, y) as one autograd node (the drop-in `loss.backward()` surface); backward runs the engine's hand-written
    backward and accumulates the parameter gradients straight into the flat fp32 grad buffer (the .grad views)."""

    @staticmethod
    def forward(ctx, model, anchor, x, y, rnd, eps, mnoise, mask_ratio, y_rowscale):
        loss, tape, dtok = _edm_forward(model, anchor, x, y, rnd, eps, mnoise, mask_ratio, y_rowscale, record_tape=True)
        ctx.model, ctx.tape, ctx.dtok, ctx.y_shape = model, tape, dtok, y.shape
        return loss

    @staticmethod
    def backward(ctx, gloss):
        model, tape, dtok = ctx.model, ctx.tape, ctx.dtok
        dit = model.dit
        pgrad = any(p.requires_grad for p in dit._plist)
        if pgrad:
            dit.attach_grads()
        g = gloss.detach().to(torch.float32).contiguous()
        dtb = torch.empty(dtok.shape, device=dtok.device, dtype=torch.bfloat16)
        hip.check(hip.lib().md_cast_f32_bf16(dtok.data_ptr(), dtb.data_ptr(), dtok.numel(), g.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "md_cast_f32_bf16")
        ig = dit._engine.backward(tape, dtb, on_segment=getattr(dit, "_on_segment", None),
                                  input_grads=("y",) if ctx.needs_input_grad[3] else (), param_grads=pgrad)
        ctx.tape = ctx.dtok = None
        dy = None if ig.dy is None else ig.dy.view(ctx.y_shape)
        return None, torch.zeros_like(dit._grad_anchor), None, dy, None, None, None, None, None


class _FrozenStub(nn.Module):
    """Placeholder for the frozen SDXL-VAE / text encoder when their libraries (diffusers / open_clip) are absent:
    enough for training on precomputed latents (train.py asserts precomputed_latents), loud on any real use."""

    def __init__(self, what: str, scaling_factor: float = 0.13025):
        super().__init__()
        self.what = what
        self.config = SimpleNamespace(scaling_factor=scaling_factor)

    def _fail(self, *a, **k):
        raise RuntimeError(f"{self.what} is not available in this environment (library not installed); "
                           "only precomputed-latent training is possible")

    encode = decode = forward = tokenize = _fail


def create_latent_diffusion(vae_name: str = "stabilityai/stable-diffusion-xl-base-1.0",
                            text_encoder_name: str = "openclip:hf-hub:apple/DFN5B-CLIP-ViT-H-14-378",
                            dit_arch: str = "MicroDiT_XL_2", latent_res: int = 32, in_channels: int = 4,
                            pos_interp_scale: float = 1.0, dtype: str = "bfloat16", precomputed_latents: bool = True,
                            p_mean: float = -0.6, p_std: float = 1.2, train_mask_ratio: float = 0.0) -> LatentDiffusion:
    """Same signature and behaviour as the reference factory (model.py:356-405); the DiT comes from this package's
    zoo; the frozen VAE / text encoder are loaded through diffusers / open_clip when those are installed."""
    s, d = text_encoder_embedding_format(text_encoder_name)
    dit = getattr(model_zoo, dit_arch)(input_size=latent_res, caption_channels=d, pos_interp_scale=pos_interp_scale,
                                       in_channels=in_channels)
    vae = text_encoder = tokenizer = None
    try:
        from diffusers import AutoencoderKL  # type: ignore
    except ImportError:
        warnings.warn(f"diffusers is not installed: VAE '{vae_name}' replaced by a stub (training on precomputed latents only)")
        vae = _FrozenStub(f"VAE '{vae_name}'")
    else:       # a real load error (bad name, no network) must surface, not turn into a stub with a made-up scaling factor
        vae = AutoencoderKL.from_pretrained(vae_name, subfolder=None if vae_name == "ostris/vae-kl-f8-d16" else "vae",
                                            torch_dtype=DATA_TYPES[dtype])
    # The reference's UniversalTextEncoder / UniversalTokenizer (utils.py:429-598: open_clip / T5 / CLIP wrappers around
    # frozen third-party models) are outside the training hot path and are NOT built here (out of
    # scope): generate(prompt=...) needs caller-supplied embeddings; training reads precomputed caption latents.
    text_encoder = _FrozenStub(f"text encoder '{text_encoder_name}' (wrapper not built: pass precomputed caption embeddings)")
    tokenizer = _FrozenStub(f"tokenizer '{text_encoder_name}' (wrapper not built)")
    return LatentDiffusion(dit=dit, vae=vae, text_encoder=text_encoder, tokenizer=tokenizer,
                           precomputed_latents=precomputed_latents, dtype=dtype, latent_res=latent_res, p_mean=p_mean,
                           p_std=p_std, train_mask_ratio=train_mask_ratio)
