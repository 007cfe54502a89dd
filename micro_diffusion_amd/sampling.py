"""The EDM sampler behind `LatentDiffusion.edm_sampler_loop` / `generate` (reference model.py:231-297): inference-only glue around the HIP
forward.  One request check (`Request.check`), one host-side plan (`sampler_plan`) and two loops that follow it: `tensor_op_loop`, the
reference's formulation in torch tensor ops and the definition of every option, and `FusedRun`, the same loop with everything around the
network evaluations in fused HIP kernels.

The arguments of `edm_sampler_loop`
-----------------------------------
EDM sampler, fp64 state (model.py:231-297).  `fused` (None = whenever possible) selects the loop whose per-step arithmetic
runs in fused HIP kernels; False keeps the reference's tensor-op formulation (generic forward functions).
`cond_cache` (None = the environment variable MD_SAMPLER_CACHE, default off): encode the captions once for the whole run
and step in token space (see FusedRun); needs the fused loop.  Results are bit-identical to the uncached loop.
`sampler`: "heun" (the reference's 2nd-order loop, 2 * steps - 1 network evaluations), "euler" or "dpmpp_2m" (DPM-Solver++(2M),
2nd order); the last two take one evaluation per step (samplers.py).  S_churn > 0 is defined for heun and euler.
`guidance_interval` = (sigma_lo, sigma_hi): an evaluation at noise level sigma is guided (batch doubled) only while
sigma_lo <= sigma <= sigma_hi; outside it the conditional half runs alone.  None: every evaluation is guided when cfg > 1.
`guide`: a second, weaker DiT on the same device (autoguidance, Karras et al. 2024).  cfg is then the autoguidance weight w:
a guided evaluation runs this model at batch B, then the guide at batch B on the same network input, and the update combines
F = F_guide + w * (F_main - F_guide); no evaluation is batch-doubled.  Unguided evaluations (cfg <= 1, outside the interval)
never run the guide.  `guide_captions`: "same" (the guide sees the captions) or "null" (zeroed captions; with guide = this
model's own dit that is classifier-free guidance as two batch-B launches).
Image-conditioned sampling (the tensor-op loop, fused=False, is the definition, the fused loop follows it):
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
Measurement-guided sampling (Chung et al. 2023; the tensor-op loop, fused=False, is the definition): `measurement`, an
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
the launches and bits of a run without the argument.
`attn_maps`: an attn_maps.AttentionMaps.  It is armed on the main network's engine for the run (and disarmed when the
run ends, an error included); both loops tell it the noise level and the batch B before every evaluation of the main network, and
behind every selected block's cross-attention one md_attn_probs launch adds the head-averaged probabilities of the first B samples (the
conditional half of a doubled batch) to its buffer.  A `guide` network is not recorded.  It only reads: it composes with every argument
above, both loops included, and the latents are the bits of the run without it.  None: the launches and bits of a run without the
argument.
Prompt control (the tensor-op loop, fused=False, is the definition).  `negative`: caption embeddings of the shape of y
(or with a leading 1 that is broadcast) that replace the zeroed captions as the second half of every batch-doubled evaluation -- in both
loops, in the guidance modes and in the conditioning cache (encode_condition then sees [y; negative]); needs cfg > 1.
`caption_weights` ([B, Lc], [1, Lc] or [Lc]; bool or floating point; host or device; finite, >= 0, a value > 0 in every row): weight
w_j of caption position j in every cross-attention of the main network, P_j = w_j e^{s_j} / sum_i w_i e^{s_i}: the bias ln w_j on the
logit (md_attn_fwd_kbias); 1 is today's softmax, 0 removes the position (a padding mask: the caption behaves as if it were shorter).
`negative_weights`: the same for the second half (needs `negative`).  The run's bias buffer (samplers.caption_bias_buffer: fp32
[2 B, ldb] when evaluations are doubled, else [B, ldb]) is armed as engine.caption_bias for the run, and what the attribute held before
(None, or a bias armed by hand) is put back when the run ends, an error included; evaluations outside a guidance_interval run at batch B and read its first B rows.  The weights act on the cross-attention only:
the pooled caption vector stays the plain mean over all positions, and the text encoder is not touched.  They compose with the solvers,
churn, guidance_interval, the guidance modes, cond_cache, the editing options, step_cache and attn_maps (which then records the
probabilities the run used: exactly 0 at a removed position); refused (ValueError): any of the three with `guide`, weights with
`measurement` / `guidance_loss` (the attention backward does not know the bias; `negative` alone composes with them).  None: the
launches and bits of a run without the arguments.

`mxfp8`: None, True, or an mxfp8.MXWeights.  The targeted block linears of the main network run in block-scaled fp8
(MXFP8: their input is quantised, md_gemm_mxfp8 multiplies) for the run: the MXWeights -- True makes them from the default targets
for this run -- are armed as engine.mx and what the attribute held before is put back when the run ends, an error included.  In both
loops; composes with every solver, churn, guidance_interval, the guidance modes, cond_cache (the caption side stays bf16, so the cache
is bit-identical on or off), step_cache, the editing options, attn_maps and prompt control; with `guide` only the main network is
quantised.  Refused (ValueError) with `measurement` / `guidance_loss`, which need a backward; MXWeights quantised at another weight
version raise.  None: the launches and bits of a run without the argument.
NOTE: the default target set is currently EMPTY -- every class of linear measured slower in MXFP8 than in bf16 (mxfp8.DEFAULT_EXCLUDED,
DESIGN.md 4.23) -- so `mxfp8=True` quantises nothing and the run issues the plain bf16 launches; to run MXFP8 pass
`MXWeights(model.dit, targets=mxfp8.ALL_TARGETS)` or a pattern of your own.
"""
from __future__ import annotations

import os
from contextlib import contextmanager, nullcontext
from dataclasses import dataclass
from functools import partial
from typing import Any, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import hip
from . import samplers


def sampler_cache_enabled(flag: Optional[bool] = None) -> bool:
    """The `cond_cache` argument of the sampler: None reads the environment variable MD_SAMPLER_CACHE (default off)."""
    return os.environ.get("MD_SAMPLER_CACHE", "0") == "1" if flag is None else bool(flag)


@contextmanager
def frozen_network(dit):
    """Context of a guided sampling run: every parameter of the network has requires_grad False inside (the backward to the image
    is the engine's dgrad-only one and writes no .grad), and what it was before afterwards."""
    params = list(dit.parameters())
    was = [p.requires_grad for p in params]
    for p in params:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p, r in zip(params, was):
            p.requires_grad_(r)


@contextmanager
def recording(dit, attn_maps, x):
    """Context of a run with attn_maps=: the recorder is armed on the main network's engine inside -- resolved against
    the model, the token grid of the state x, sums and counts cleared -- and the engine is disarmed afterwards, whatever ended the run.
    None: nothing."""
    if attn_maps is None:
        yield
        return
    engine, p = dit.engine, dit.patch_size
    attn_maps.arm(engine, (x.shape[-2] // p, x.shape[-1] // p))
    try:
        yield
    finally:
        attn_maps.disarm(engine)


@contextmanager
def caption_bias(dit, bias):
    """Context of a run with caption weights: the run's bias buffer is the main network's engine.caption_bias inside,
    and what the attribute held before (None, or a bias the caller armed by hand) is put back afterwards, whatever ended the run.
    None: nothing is touched, so a run without weights on an engine armed by hand runs under that bias."""
    if bias is None:
        yield
        return
    engine = dit.engine
    before, engine.caption_bias = engine.caption_bias, bias
    try:
        yield
    finally:
        engine.caption_bias = before


@contextmanager
def mx_armed(dit, mxfp8):
    """Context of a run with mxfp8=: the MXWeights -- made here from the main network's default targets when the
    argument is True -- are the main network's engine.mx inside, and what the attribute held before afterwards, whatever ended the
    run.  MXWeights quantised at another weight version raise before anything is armed.  None: nothing is touched."""
    if mxfp8 is None:
        yield
        return
    dit._ensure_flat()
    dit.refresh_shadow()
    if mxfp8 is True:
        from .mxfp8 import MXWeights
        mxfp8 = MXWeights(dit)
    engine = dit.engine
    mxfp8.check_fresh(engine.weights_version)
    before, engine.mx = engine.mx, mxfp8
    try:
        yield
    finally:
        engine.mx = before


def negative_captions(y, negative):
    """negative as the second half of [y; negative]: y's dtype and device, a leading 1 broadcast over the batch."""
    return negative.detach().to(device=y.device, dtype=y.dtype).expand_as(y)


# ---------------------------------------------------------------------------------------------------------------------
# The request: the options of one run, checked once
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Request:
    """The options of `edm_sampler_loop` / `generate` behind cfg, fused and cond_cache, with their defaults."""
    sampler: str = "heun"
    guidance_interval: Any = None
    guide: Any = None
    guide_captions: str = "same"
    init_latents: Any = None
    strength: float = 1.0
    inpaint_mask: Any = None
    resample: int = 1
    guidance_mode: str = "cfg"
    guidance_rescale: float = 0.0
    apg_eta: float = 0.0
    apg_norm_threshold: Any = None
    apg_momentum: float = 0.0
    measurement: Any = None
    measurement_scale: float = 1.0
    guidance_loss: Any = None
    step_cache: Any = None
    attn_maps: Any = None
    negative: Any = None
    caption_weights: Any = None
    negative_weights: Any = None
    mxfp8: Any = None

    def check(self, model, shape, cfg, extra=(), y_shape=None, has_negative=False, will_weight=False):
        """Refuse, before anything is tokenised, launched, allocated or drawn, a request that is not defined (the samplers.check_*
        functions, in this order).  shape: (B, C, H, W) of the state, or None when it is not known yet; extra: the names of the extra
        forward arguments; y_shape: the shape of the caption embeddings when known; has_negative / will_weight: a negative prompt will
        be encoded / caption weights will be made from the tokenizer's mask (generate, before it has tokenised).
        Returns (caching, guided_by, interval, gmode): whether the run uses the step cache, whether it is measurement-guided, the
        guidance interval's bounds or None, and (mode, phi, eta, r or None, beta) of a run that is guided in a mode other than "cfg"
        (else None)."""
        samplers.check_sampler(self.sampler, model.edm_config.S_churn)
        caching = samplers.check_step_cache(self.step_cache, self.guide, self.measurement, self.guidance_loss)
        samplers.check_mxfp8(self.mxfp8, self.measurement, self.guidance_loss)
        guided_by = samplers.check_measurement(shape, self.measurement, self.measurement_scale, self.guidance_loss)
        if guided_by:
            for bad, what in ((self.guide is not None, "a guide network (autoguidance)"),
                              (self.guidance_mode != "cfg", f"guidance_mode={self.guidance_mode!r}"),
                              (bool(extra), f"extra forward arguments {sorted(extra)}")):
                if bad:
                    raise NotImplementedError(f"measurement / guidance_loss with {what}: not done (DESIGN.md 4.18)")
        interval = samplers.guidance_interval_bounds(self.guidance_interval)
        samplers.check_guide(model.dit, self.guide, self.guide_captions)
        samplers.check_guidance(self.guidance_mode, cfg, self.guidance_rescale, self.apg_eta, self.apg_norm_threshold, self.apg_momentum)
        gmode = None
        if self.guidance_mode != "cfg" and cfg > 1.0:
            r = self.apg_norm_threshold
            gmode = (self.guidance_mode, float(self.guidance_rescale), float(self.apg_eta), None if r is None else float(r),
                     float(self.apg_momentum))
        samplers.check_edit(self.sampler, self.init_latents is not None, self.strength, self.inpaint_mask is not None, self.resample)
        if self.attn_maps is not None:
            samplers.check_attn_maps(self.attn_maps, model.dit.config)
        samplers.check_prompt_control(has_negative, self.caption_weights, self.negative_weights, cfg, self.guide, self.measurement,
                                      self.guidance_loss, self.negative, y_shape, will_weight)
        return caching, guided_by, interval, gmode


def edit_operands(x, init_latents, inpaint_mask):
    """(init_latents as fp64, the mask as contiguous fp32 [mask_B, H * W] or None) on x's device, each converted once;
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
    return x0, m


# ---------------------------------------------------------------------------------------------------------------------
# The plan: everything both loops derive on the host from the schedule, once per run
# ---------------------------------------------------------------------------------------------------------------------
def edm_levels(ec, n: int, device=None) -> torch.Tensor:
    """The EDM noise levels t_0 = sigma_max ... t_{n-1} = sigma_min and a final 0 (model.py:238-243): fp64 [n + 1], computed by torch
    on `device`.  The tensor-op loop computes them where its state lives and the fused loop on the host, as they always have; the golden
    files pin these bits, which samplers.edm_schedule (Python's **) need not reproduce in the last place."""
    idx = torch.arange(n, dtype=torch.float64, device=device)
    inv_rho = 1 / ec.rho
    t_steps = (ec.sigma_max ** inv_rho + idx / (n - 1) * (ec.sigma_min ** inv_rho - ec.sigma_max ** inv_rho)) ** ec.rho
    return torch.cat([t_steps, torch.zeros_like(t_steps[:1])])


def churn_gamma(ec, t, n: int):
    """gamma of the step that starts at noise level t (a float or a 0-dim tensor; model.py:254-257): > 0 inside [S_min, S_max]."""
    return min(ec.S_churn / n, np.sqrt(2) - 1) if ec.S_min <= t <= ec.S_max else 0


def churned_levels(ec, t_steps, n: int) -> List[float]:
    """t_hat of every step from the host-side noise levels: t_cur * (1 + gamma); t_cur itself where the step does not churn."""
    return [t + churn_gamma(ec, t, n) * t for t in t_steps[:-1]]


class Plan(NamedTuple):
    n: int                          # steps of the whole schedule
    heun: bool
    levels: torch.Tensor            # fp64 [n + 1] as edm_levels made them
    t_steps: List[float]            # the same on the host
    t_hats: List[float]             # [n] the level each step's first evaluation runs at
    i0: int                         # the first executed step (image-to-image; else 0)
    reps: List[int]                 # [n - i0] how often each executed step runs (RePaint; else 1)
    coefs: Optional[List[Tuple[float, float, float, float]]]      # [n - i0] of euler / dpmpp_2m (samplers.solver_coefficients); heun: None
    sigmas: List[float]             # the noise level of every evaluation of one pass over the executed steps
    evaluations: int                # network evaluations of the run, repetitions included


def sampler_plan(ec, steps: Optional[int], sampler: str, strength: float = 1.0, resample: int = 1, device=None) -> Plan:
    n = ec.num_steps if steps is None else steps
    heun = sampler == "heun"
    levels = edm_levels(ec, n, device)
    t_steps = levels.tolist()
    t_hats = churned_levels(ec, t_steps, n)
    i0 = samplers.edit_start_index(n, strength)
    reps = samplers.edit_repetitions(t_steps, i0, resample)
    coefs = None if heun else samplers.solver_coefficients(sampler, t_steps[i0:], t_hats[i0:])
    twice = [heun and i < n - 1 for i in range(i0, n)]         # heun evaluates every step but the last a second time, at t_next
    sigmas = [s for i, two in zip(range(i0, n), twice) for s in ([t_hats[i], t_steps[i + 1]] if two else [t_hats[i]])]
    return Plan(n, heun, levels, t_steps, t_hats, i0, reps, coefs, sigmas, sum(r * (2 if two else 1) for r, two in zip(reps, twice)))


# ---------------------------------------------------------------------------------------------------------------------
# The tensor-op loop: the definition
# ---------------------------------------------------------------------------------------------------------------------
def autoguided_forward(model, guide, y_guide, w: float, attn_maps=None):
    """The forward function of an autoguided evaluation for model_forward_wrapper: both networks on the same input at batch B, the
    guide with its own captions, combined in fp32 as the update kernels do (F = F_guide + w * (F_main - F_guide)).  attn_maps: the
    run's recorder, told that the guide's forward is not the main network's (the guide may share the engine)."""
    def fwd(x, t, y, **kwargs):
        fm = model.dit.forward_without_cfg(x, t, y, **kwargs)["sample"].to(torch.float32)
        if attn_maps is not None:
            attn_maps.skip_evaluation()
        fg = guide.forward_without_cfg(x, t, y_guide, **kwargs)["sample"].to(torch.float32)
        return {"sample": fg + w * (fm - fg)}
    return fwd


class TensorOpNetwork:
    """The network evaluations of the tensor-op loop: denoise(xs, sigma) -> the denoised prediction in fp64, in three forms."""

    def __init__(self, model, y, cfg: float, interval, guide, guide_null: bool, gmode, kwargs, attn_maps=None, negative=None):
        """negative: the second half of a doubled evaluation in place of the zeroed captions (no guide), already of y's shape."""
        self.model, self.y, self.cfg, self.interval, self.guide, self.gmode, self.kwargs = model, y, cfg, interval, guide, gmode, kwargs
        self.attn_maps = attn_maps
        dit = model.dit
        if cfg <= 1.0:
            self.guided_forward = dit.forward
        elif guide is not None:
            self.guided_forward = autoguided_forward(model, guide, torch.zeros_like(y) if guide_null else y, cfg, attn_maps)
        elif negative is not None:
            self.guided_forward = partial(dit.forward, cfg=cfg, negative=negative)
        else:
            self.guided_forward = partial(dit.forward, cfg=cfg)
        if gmode is not None:
            self.y_u = y if guide is not None and not guide_null else (torch.zeros_like(y) if negative is None else negative)
            self.M = None                           # the M of the previous guided evaluation of this run

    def inside(self, sigma) -> bool:
        return self.interval is None or self.interval[0] <= float(sigma) <= self.interval[1]

    def forward_at(self, sigma):
        return self.guided_forward if self.inside(sigma) else self.model.dit.forward

    def announce(self, xs, sigma):
        """Tell the attention-map recorder (if any) the noise level and the batch of the main network's next evaluation."""
        if self.attn_maps is not None:
            self.attn_maps.begin_evaluation(sigma, xs.shape[0])

    def denoise(self, xs, sigma):
        self.announce(xs, sigma)
        return self.model.model_forward_wrapper(xs.to(torch.float32), sigma.to(torch.float32), self.y, self.forward_at(sigma), mask_ratio=0,
                                                **self.kwargs)["sample"].to(torch.float64)

    def denoise_in_mode(self, xs, sigma):
        """denoise in guidance mode "rescale" or "apg" (DESIGN.md 4.14), in plain torch: the preconditioning of model_forward_wrapper
        (fp32) around one doubled-batch forward without cfg=, or with a guide around two forwards; D_c = c_skip x + c_out F_c as
        everywhere, D_c - D_u = c_out (F_c - F_u) (c_skip x cancels), and the running difference, the moments and the combine in fp64.
        Outside the interval the unguided evaluation runs and M stays."""
        if not self.inside(sigma):
            return self.denoise(xs, sigma)
        self.announce(xs, sigma)
        mode, phi, eta, r, beta = self.gmode
        dit, guide, y, kwargs, sd = self.model.dit, self.guide, self.y, self.kwargs, self.model.edm_config.sigma_data
        xs, sigma = xs.to(torch.float32), sigma.to(torch.float32).reshape(-1, 1, 1, 1)
        c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
        c_out = sigma * sd / (sigma ** 2 + sd ** 2).sqrt()
        net_in, c_noise = (1 / (sd ** 2 + sigma ** 2).sqrt()) * xs, (sigma.log() / 4).flatten()
        if guide is None:
            F = dit.forward(torch.cat([net_in, net_in], 0), c_noise, torch.cat([y, self.y_u], 0), mask_ratio=0, **kwargs)["sample"]
            F_c, F_u = torch.split(F.to(torch.float32), len(F) // 2, dim=0)
        else:
            F_c = dit.forward_without_cfg(net_in, c_noise, y, mask_ratio=0, **kwargs)["sample"].to(torch.float32)
            if self.attn_maps is not None:
                self.attn_maps.skip_evaluation()
            F_u = guide.forward_without_cfg(net_in, c_noise, self.y_u, mask_ratio=0, **kwargs)["sample"].to(torch.float32)
        D_c = (c_skip * xs + c_out * F_c).to(torch.float64)
        M = c_out.to(torch.float64) * (F_c.to(torch.float64) - F_u.to(torch.float64))
        if mode == "apg" and beta != 0.0 and self.M is not None:
            M = M + beta * self.M
        self.M = M
        alpha, gamma = samplers.guidance_coefficients(mode, samplers.guidance_moments(D_c, M), D_c[0].numel(), self.cfg, phi, eta, r)
        return alpha.view(-1, 1, 1, 1) * D_c + gamma.view(-1, 1, 1, 1) * M

    def denoise_with_correction(self, xs, sigma, loss_fn, zeta: float):
        """(D, correction) of a measurement-guided step's first evaluation: model_forward_wrapper under
        torch.enable_grad() on the fp32 xs, torch.autograd.grad of L.sum() gives g = dL/dxs through the (frozen) network, and the
        correction zeta / max(sqrt(L_b), GUIDE_TINY) * g, to subtract from the solver's result, is formed in fp64."""
        self.announce(xs, sigma)
        with torch.enable_grad():
            x32 = xs.to(torch.float32).detach().requires_grad_(True)
            D = self.model.model_forward_wrapper(x32, sigma.to(torch.float32), self.y, self.forward_at(sigma), mask_ratio=0)["sample"]
            L = loss_fn(D)
            g, = torch.autograd.grad(L.sum(), x32)
        L = L.detach().to(torch.float64)
        return D.detach().to(torch.float64), (zeta / L.sqrt().clamp_min(samplers.GUIDE_TINY)).view(-1, 1, 1, 1) * g.to(torch.float64)


def tensor_op_loop(model, x, plan: Plan, edit, denoise, first_evaluation=None):
    """The reference's loop in torch tensor ops on the fp64 state: blend, churn, Heun / linear-multistep step, RePaint re-noise, final
    paste.  denoise(x, t) -> D; first_evaluation(x_hat, t_hat) -> (D, correction or None), the step's first evaluation (None: denoise
    and no correction): a correction is subtracted from the solver's result before the re-noise, and dpmpp_2m's history holds the
    uncorrected D.  Every draw reads model.randn_like when it is made."""
    ec, n, t_steps, i0, reps, coef = model.edm_config, plan.n, plan.levels, plan.i0, plan.reps, plan.coefs
    x0, m = (None, None) if edit is None else edit
    if m is not None:                               # [mask_B, H * W] fp32 -> broadcast over the channels of the fp64 state
        m = m.view(m.shape[0], 1, x.shape[-2], x.shape[-1]).to(torch.float64)
    draw_churn = m is None or ec.S_churn > 0
    x_next = x.to(torch.float64) * t_steps[0] if edit is None else x0 + t_steps[i0] * x.to(torch.float64)
    for i in range(i0, n):
        t_cur, t_next = t_steps[i], t_steps[i + 1]
        for rep in range(reps[i - i0]):
            x_cur = x_next
            if m is not None:
                x_cur = m * x_cur + (1 - m) * (x0 + t_cur * model.randn_like(x_cur))
            t_hat = torch.as_tensor(t_cur + churn_gamma(ec, t_cur, n) * t_cur)
            x_hat = x_cur + (t_hat ** 2 - t_cur ** 2).sqrt() * ec.S_noise * model.randn_like(x_cur) if draw_churn else x_cur
            den, correction = (denoise(x_hat, t_hat), None) if first_evaluation is None else first_evaluation(x_hat, t_hat)
            if not plan.heun:                       # one evaluation per step: x_next = a x_hat + b (c1 D - c2 D_prev)
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
            if correction is not None:
                x_next = x_next - correction
            if rep < reps[i - i0] - 1:              # RePaint: back to level t_cur for the next repetition
                x_next = x_next + (t_cur ** 2 - t_next ** 2).sqrt() * model.randn_like(x_next)
    if m is not None:
        x_next = m * x_next + (1 - m) * x0
    return x_next.to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# The fused loop
# ---------------------------------------------------------------------------------------------------------------------
class FusedRun:
    """One run of the same loop with everything around the network evaluations in fused HIP kernels: md_edm_sampler_input (c_in scaling +
    guidance batch doubling) and md_edm_heun_update (guidance combine + preconditioning + fp64 Euler / Heun update) or, for
    euler / dpmpp_2m, md_edm_solver_update (the same with the linear-multistep update of samplers.solver_coefficients).
    S_churn > 0: the noise is drawn once per step as in the tensor-op loop and md_edm_churn adds it to the state in place.
    cond_cache: the captions (doubled under guidance) are encoded once (dit.encode_condition) and every evaluation runs
    md_edm_sampler_patchify -> engine.forward(patches=, cond=) -> md_edm_heun_update_tok / md_edm_solver_update_tok on the token
    output: no caption-side work per evaluation and no fp32 image between the fp64 state and the network's bf16 rows.
    interval: evaluations outside it run the conditional half alone (network batch B) on leading-row views of the same buffers.
    guide: nothing is doubled.  A guided evaluation writes the network input once (dup = 0), runs model.dit and then the guide on it
    at batch B (the guide with its own captions / its own Conditioning, encoded by the guide) and hands the two outputs to
    md_edm_*_update_guide(_tok).  Both outputs are fresh allocations that network() returns together, so main's is alive and
    untouched while the guide runs and until the update has been enqueued.
    edit = (init_latents fp64, mask fp32 [mask_B, H * W] or None) from edit_operands: md_edm_blend_known writes the
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
    negative (no guide): the second half of the doubled captions y2 in place of zeros, already of y's shape.  The
    caption bias of a run with weights is not this class's business: sample() arms it on the engine around run().
    step_cache: a step_cache.StepCache (no guide, no guidance): it is reset for the run's evaluation count, and every
    network() call hands the engine its ResidualCache and a decision callback (StepCache.engine_args) -- through engine.forward with
    cond_cache, through dit.forward_without_cfg without.  None: none of it.

    The constructor allocates the run's buffers (and writes the image-to-image start); run() steps."""

    def __init__(self, model, x, y, plan: Plan, cfg: float, cond_cache: bool = False, interval=None, guide=None, guide_null: bool = False,
                 edit=None, gmode=None, guidance=None, step_cache=None, attn_maps=None, negative=None):
        self.model, self.dit, self.guide, self.plan, self.step_cache = model, model.dit, guide, plan, step_cache
        self.attn_maps = attn_maps
        self.L, self.st, self.sd = hip.lib(), torch.cuda.current_stream().cuda_stream, model.edm_config.sigma_data
        self.x, self.y, self.cfg, self.interval, self.cond_cache = x, y, cfg, interval, cond_cache
        self.guided = any(samplers.is_guided(s, cfg, interval) for s in plan.sigmas)        # no guided evaluation at all: the cfg = 1 run
        B = self.B = x.shape[0]
        self.numel, dev = x.numel(), x.device
        self.gmode = gmode if self.guided else None
        if self.gmode is not None:
            mode, phi, eta, r, beta = gmode
            kind = {"rescale": hip.GUIDANCE_RESCALE, "apg": hip.GUIDANCE_APG}[mode]
            self.g_par = (kind, float(cfg), phi, eta, 0 if r is None else 1, 1.0 if r is None else r, beta)
            self.g_M = torch.empty(tuple(x.shape), device=dev, dtype=torch.float32)
            self.g_coef = torch.empty(B, 2, device=dev, dtype=torch.float32)
            self.g_moments = torch.empty(B, 5, device=dev, dtype=torch.float64)
            self.g_evals = 0                        # guided evaluations so far: the first one does not read M
        self.x0, self.mask = (None, None) if edit is None else edit
        if edit is None:
            self.x_cur = (x.to(torch.float64) * plan.t_steps[0]).contiguous()
        else:
            # always a copy: the kernel writes the start into it in place, and an fp64 contiguous x would otherwise be the caller's tensor
            self.x_cur = x.to(torch.float64, copy=True, memory_format=torch.contiguous_format)
            self.blend_known(self.x_cur, None, plan.t_steps[plan.i0])
        self.x_nxt, self.d_cur = torch.empty_like(self.x_cur), torch.empty_like(self.x_cur)
        self.auto = guide is not None and self.guided       # with a guide the second operand comes from it: the batch is never doubled
        doubled = self.guided and not self.auto
        self.y2 = torch.cat([y, torch.zeros_like(y) if negative is None else negative], 0) if doubled else y
        Bn = self.Bn = 2 * B if doubled else B
        if self.auto:
            self.y_g = torch.zeros_like(y) if guide_null else y
        if cond_cache or guidance is not None:
            p = self.dit.patch_size
            self.T = (x.shape[2] // p) * (x.shape[3] // p)
            self.tok = (B, x.shape[1], x.shape[2], x.shape[3], p)           # B, C, H, W, p: the geometry arguments of the token-space kernels
        if cond_cache:
            self.cond = self.dit.encode_condition(self.y2)
            if self.auto:
                self.cond_g = guide.encode_condition(self.y_g)
            self.patches = torch.empty(Bn * self.T, self.dit.config.patch_vec, device=dev, dtype=torch.bfloat16)
        else:
            self.net_in = torch.empty((Bn,) + tuple(x.shape[1:]), device=dev, dtype=torch.float32)
        self.guidance = guidance
        if guidance is not None:
            g_meas = guidance[0]
            if g_meas is not None:
                self.g_m, self.g_mask = g_meas.operands(x)
            self.g_D, self.g_q = (torch.empty(tuple(x.shape), device=dev, dtype=torch.float32) for _ in range(2))
            self.g_L = torch.empty(B, device=dev, dtype=torch.float64)
            self.g_dtok = torch.empty(Bn * self.T, self.dit.config.patch_vec, device=dev, dtype=torch.bfloat16)

    def blend_known(self, noise, m, sigma):
        """x_cur <- m * x_cur + (1 - m) * (x0 + sigma * noise); m None: the whole state, noise None: x0 itself."""
        x = self.x
        hip.check(self.L.md_edm_blend_known(self.x_cur.data_ptr(), self.x0.data_ptr(), None if noise is None else noise.data_ptr(),
                                            None if m is None else m.data_ptr(), self.B, x.shape[1], x.shape[2] * x.shape[3],
                                            1 if m is None else m.shape[0], float(sigma), self.st), "md_edm_blend_known")

    def churn(self, noise, scale):
        """x_cur += scale * noise, in place: the churn (x_cur becomes x_hat), and RePaint's way back to the step's level."""
        x_cur = self.x_cur
        hip.check(self.L.md_edm_churn(x_cur.data_ptr(), noise.data_ptr(), x_cur.data_ptr(), self.numel, float(scale), self.st), "md_edm_churn")

    def network_input(self, xs, sigma, dup):
        """The input stage of one evaluation: writes c_in * xs (twice when dup) as the network's input.  Returns (the input -- patch rows
        with cond_cache, else the fp32 image; leading-row views when the evaluation runs at batch B of a doubled run --, the c_noise
        tensor, the evaluation's network batch)."""
        B, L, x = self.B, self.L, self.x
        if self.attn_maps is not None:              # every evaluation of the main network passes here first
            self.attn_maps.begin_evaluation(sigma, B)
        c_noise = float(np.log(np.float32(sigma)) / 4)
        Be = 2 * B if dup else B
        if self.cond_cache:
            pt = self.patches if Be == self.Bn else self.patches[:B * self.T]
            hip.check(L.md_edm_sampler_patchify(xs.data_ptr(), pt.data_ptr(), *self.tok, float(sigma), self.sd, dup, self.st),
                      "md_edm_sampler_patchify")
            return pt, torch.full((Be,), c_noise, device=x.device, dtype=torch.float32), Be
        hip.check(L.md_edm_sampler_input(xs.data_ptr(), self.net_in.data_ptr(), self.numel, float(sigma), self.sd, dup, self.st),
                  "md_edm_sampler_input")
        return (self.net_in if Be == self.Bn else self.net_in[:B]), torch.full((1,), c_noise, device=x.device, dtype=torch.float32), Be

    def network(self, xs, sigma):
        """(network output, dup, guide output) for state xs at noise level sigma: the fp32 image F, or (cond_cache) the bf16 token
        rows; dup = 1 when the evaluation is guided by batch doubling: the output holds the unconditional half behind the
        conditional.  With a guide dup is 0 and a guided evaluation returns the guide's output as well (else None)."""
        g_eval = self.guided and samplers.is_guided(sigma, self.cfg, self.interval)
        dup = 1 if g_eval and not self.auto else 0
        inp, t, Be = self.network_input(xs, sigma, dup)
        # the step-cache arguments of the main network's evaluation at batch Be (none without a step cache)
        sc_args = {} if self.step_cache is None else self.step_cache.engine_args(self.dit.engine, Be)
        run_guide = self.auto and g_eval
        if self.cond_cache:
            F = self.dit._engine.forward(None, t, None, cond=self.cond.narrow(Be), patches=inp, **sc_args).out_tok
            if run_guide and self.attn_maps is not None:
                self.attn_maps.skip_evaluation()
            Fg = self.guide._engine.forward(None, t, None, cond=self.cond_g, patches=inp).out_tok if run_guide else None
            return F, dup, Fg
        F = self.dit.forward_without_cfg(inp, t, self.y2 if Be == self.Bn else self.y, 0, **sc_args)["sample"].contiguous()
        if run_guide and self.attn_maps is not None:
            self.attn_maps.skip_evaluation()
        Fg = self.guide.forward_without_cfg(inp, t, self.y_g, 0)["sample"].to(torch.float32).contiguous() if run_guide else None
        return F, dup, Fg

    def network_with_gradient(self, xs, sigma):
        """network(xs, sigma) for a measurement-guided step's first evaluation, and the gradient of the network input under the
        loss: returns ((network output, dup, None), dx fp32 [B or 2B, C, H, W]); q and L are left in g_q and g_L."""
        B, L, st, sd, cfg = self.B, self.L, self.st, self.sd, float(self.cfg)
        g_meas, g_loss, _ = self.guidance
        dit, eng, g_D, g_q, g_L = self.dit, self.dit.engine, self.g_D, self.g_q, self.g_L
        dup = 1 if self.guided and samplers.is_guided(sigma, self.cfg, self.interval) else 0
        inp, t, Be = self.network_input(xs, sigma, dup)
        if self.cond_cache:
            tape = eng.forward(None, t, None, cond=self.cond.narrow(Be), patches=inp, input_tape=True)
            F = tape.out_tok
            hip.check(L.md_edm_denoised_tok(xs.data_ptr(), F.data_ptr(), g_D.data_ptr(), *self.tok, cfg, dup, float(sigma), sd, st),
                      "md_edm_denoised_tok")
        else:
            dit.refresh_shadow()
            tape = eng.forward(inp, t, dit._caption_input(self.y2 if Be == self.Bn else self.y), record_tape=True)
            F = eng.sample_image(tape)
            hip.check(L.md_edm_denoised(xs.data_ptr(), F.data_ptr(), g_D.data_ptr(), B, self.numel // B, cfg, dup, float(sigma), sd, st),
                      "md_edm_denoised")
        if g_meas is not None:
            g_mask = self.g_mask
            hip.check(L.md_measure_residual(g_D.data_ptr(), self.g_m.data_ptr(), None if g_mask is None else g_mask.data_ptr(),
                                            1 if g_mask is None else g_mask.shape[0], g_q.data_ptr(), g_L.data_ptr(), *self.tok[:4],
                                            g_meas.pool, st), "md_measure_residual")
        else:
            with torch.enable_grad():
                Dg = g_D.detach().clone().requires_grad_(True)
                loss = g_loss(Dg)
                gq, = torch.autograd.grad(loss.sum(), Dg)
            g_q.copy_(gq)
            g_L.copy_(loss.detach().reshape(B))
        dtok = self.g_dtok if Be == self.Bn else self.g_dtok[:B * self.T]
        hip.check(L.md_guide_cotangent_tok(g_q.data_ptr(), dtok.data_ptr(), *self.tok, cfg, dup, float(sigma), sd, st),
                  "md_guide_cotangent_tok")
        dx = eng.backward(tape, dtok, input_grads=("x",), param_grads=False).dx
        return (F, dup, None), dx

    def guide_apply(self, dx, dup, sigma):
        """The correction of the step's result x_nxt along g = c_skip q + c_in (dx_c + dx_u), the coefficients of level sigma."""
        hip.check(self.L.md_edm_guide_apply(self.x_nxt.data_ptr(), self.g_q.data_ptr(), dx.data_ptr(), self.g_L.data_ptr(), self.B,
                                            self.numel // self.B, dup, self.guidance[2], float(sigma), self.sd, self.st), "md_edm_guide_apply")

    def prepare(self, Fd, x_in, t_in) -> bool:
        """In a guidance mode, for a guided evaluation: M, the moments and the coefficients from the two outputs; True when it ran."""
        F, dup, Fg = Fd
        if self.gmode is None or not (dup or Fg is not None):
            return False
        Fu = Fg.data_ptr() if Fg is not None else F.data_ptr() + (F.numel() // 2) * F.element_size()
        first = 1 if self.g_evals == 0 else 0
        self.g_evals += 1
        name, geometry = ("md_guidance_prepare_tok", self.tok) if self.cond_cache else ("md_guidance_prepare", (self.B, self.numel // self.B))
        hip.check(getattr(self.L, name)(x_in.data_ptr(), F.data_ptr(), Fu, self.g_M.data_ptr(), self.g_coef.data_ptr(), self.g_moments.data_ptr(),
                                        *geometry, t_in, self.sd, *self.g_par, first, self.st), name)
        return True

    def update(self, Fd, x_in, t_in, heun_step=None, coef=None):
        """x_nxt from x_cur, the evaluated state x_in and the network output: one of the twelve md_edm_*_update* entry points.
        heun_step = (t_hat, t_next, second): a Heun half-step (the first also writes d_cur).  coef = (a, b, c1, c2): the linear-multistep
        step x_nxt = a x_cur + b (c1 D - c2 hist), hist = D, with d_cur as the history buffer (x_in is x_cur).
        Three operand families, each in image and in token space (hip.py lists the signatures in this order); what follows the state and
        output pointers differs between them and is spelled out here:
          plain     F                  numel | B, C, H, W, p        then cfg, dup
          _guide    F, guide's F       numel | B, C, H, W, p        then cfg
          _coef     F, M, coef         B, numel / B | B, C, H, W, p"""
        F, dup, Fg = Fd
        L, tok, cfg = self.L, self.cond_cache, float(self.cfg)
        if self.prepare(Fd, x_in, t_in):
            heun, solver = (("md_edm_heun_update_coef_tok", "md_edm_solver_update_coef_tok") if tok else
                            ("md_edm_heun_update_coef", "md_edm_solver_update_coef"))
            outputs = (F.data_ptr(), self.g_M.data_ptr(), self.g_coef.data_ptr())
            geometry = self.tok if tok else (self.B, self.numel // self.B)
        elif Fg is not None:
            heun, solver = (("md_edm_heun_update_guide_tok", "md_edm_solver_update_guide_tok") if tok else
                            ("md_edm_heun_update_guide", "md_edm_solver_update_guide"))
            outputs = (F.data_ptr(), Fg.data_ptr())
            geometry = (*self.tok, cfg) if tok else (self.numel, cfg)
        else:
            heun, solver = (("md_edm_heun_update_tok", "md_edm_solver_update_tok") if tok else
                            ("md_edm_heun_update", "md_edm_solver_update"))
            outputs = (F.data_ptr(),)
            geometry = (*self.tok, cfg, dup) if tok else (self.numel, cfg, dup)
        x_cur, d_cur, x_nxt = self.x_cur.data_ptr(), self.d_cur.data_ptr(), self.x_nxt.data_ptr()
        if heun_step is not None:
            t_hat, t_next, second = heun_step
            hip.check(getattr(L, heun)(x_cur, x_in.data_ptr(), *outputs, d_cur, x_nxt, *geometry, t_in, t_hat, t_next, self.sd, second,
                                       self.st), heun)
        else:
            hip.check(getattr(L, solver)(x_cur, *outputs, d_cur, x_nxt, *geometry, t_in, self.sd, *coef, self.st), solver)

    def run(self):
        plan, model, ec, mask = self.plan, self.model, self.model.edm_config, self.mask
        n, i0, t_steps, churn = plan.n, plan.i0, plan.t_steps, self.model.edm_config.S_churn > 0
        if self.step_cache is not None:             # the run's evaluations: every repetition of a step, heun twice but for the last step
            self.step_cache.reset(plan.evaluations)
        for i in range(i0, n):
            t_cur, t_next, t_hat = t_steps[i], t_steps[i + 1], plan.t_hats[i]
            reps = plan.reps[i - i0]
            for rep in range(reps):
                # .to(float64).contiguous() on a draw, here and below, does nothing for torch.randn_like on the fp64 state: it is there for
                # a replaced model.randn_like (a recorded or fp32 generator), whose result the kernels must still read as contiguous fp64
                if mask is not None:                # the known region at this step's noise level, one fresh draw
                    self.blend_known(model.randn_like(self.x_cur).to(torch.float64).contiguous(), mask, t_cur)
                if churn:                           # one draw per step, churned or not: the draws of the tensor-op loop
                    noise = model.randn_like(self.x_cur)
                    if t_hat != t_cur:              # x_cur becomes x_hat (x_cur itself is not read again)
                        self.churn(noise.to(torch.float64).contiguous(), np.sqrt(t_hat ** 2 - t_cur ** 2) * ec.S_noise)
                x_cur = self.x_cur
                Fd, g_dx = (self.network(x_cur, t_hat), None) if self.guidance is None else self.network_with_gradient(x_cur, t_hat)
                if plan.heun:
                    self.update(Fd, x_cur, t_hat, heun_step=(t_hat, t_next, 0))
                    if i < n - 1:                   # not differentiated: no tape
                        self.update(self.network(self.x_nxt, t_next), self.x_nxt, t_next, heun_step=(t_hat, t_next, 1))
                else:
                    self.update(Fd, x_cur, t_hat, coef=plan.coefs[i - i0])
                if g_dx is not None:
                    self.guide_apply(g_dx, Fd[1], t_hat)
                self.x_cur, self.x_nxt = self.x_nxt, self.x_cur
                if rep < reps - 1:                  # RePaint: the state this repetition produced goes back to level t_cur
                    self.churn(model.randn_like(self.x_cur).to(torch.float64).contiguous(), np.sqrt(t_cur ** 2 - t_next ** 2))
        if mask is not None:
            self.blend_known(None, mask, 0.0)
        return self.x_cur.to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# The entry point behind LatentDiffusion.edm_sampler_loop
# ---------------------------------------------------------------------------------------------------------------------
def sample(model, x, y, steps, cfg, fused, cond_cache, req: Request, kwargs):
    """edm_sampler_loop: check the request, convert the edit operands, choose the loop, make the plan where that loop wants it, run."""
    caching, guided_by, interval, gmode = req.check(model, tuple(x.shape), cfg, kwargs, y_shape=None if y is None else tuple(y.shape))
    edit = None if req.init_latents is None else edit_operands(x, req.init_latents, req.inpaint_mask)
    can_fuse = not kwargs and x.is_cuda
    cond_cache = sampler_cache_enabled(cond_cache)
    if cond_cache and (fused is False or not can_fuse):
        raise RuntimeError("cond_cache needs the fused sampler: no extra forward arguments, CUDA tensors")
    if caching and (fused is False or not can_fuse):
        raise ValueError("step_cache needs the fused sampler: no extra forward arguments, CUDA tensors")
    if fused is None:
        fused = can_fuse
    guide, guide_null = req.guide, req.guide_captions == "null"
    zeta = float(req.measurement_scale)
    if fused:
        assert can_fuse, "the fused sampler needs CUDA tensors and no extra forward arguments"
    plan = sampler_plan(model.edm_config, steps, req.sampler, req.strength if edit is not None else 1.0, req.resample,
                        device=None if fused else x.device)
    am = req.attn_maps
    negative = None if req.negative is None else negative_captions(y, req.negative)
    bias = None
    if req.caption_weights is not None or req.negative_weights is not None:
        doubled = any(samplers.is_guided(s, cfg, interval) for s in plan.sigmas)       # (no guide: a guided evaluation is a doubled one)
        bias = samplers.caption_bias_buffer(req.caption_weights, req.negative_weights, x.shape[0], y.shape[-2], doubled, x.device)
    with frozen_network(model.dit) if guided_by else nullcontext(), recording(model.dit, am, x), caption_bias(model.dit, bias), \
            mx_armed(model.dit, req.mxfp8):
        if fused:
            guidance = (req.measurement, req.guidance_loss, zeta) if guided_by else None
            return FusedRun(model, x, y, plan, cfg, cond_cache, interval, guide, guide_null, edit, gmode, guidance, req.step_cache, am,
                            negative).run()
        net = TensorOpNetwork(model, y, cfg, interval, guide, guide_null, gmode, kwargs, am, negative)
        first = None
        if guided_by:
            loss_fn = req.guidance_loss if req.measurement is None else req.measurement.loss_fn(x)
            first = partial(net.denoise_with_correction, loss_fn=loss_fn, zeta=zeta)
        return tensor_op_loop(model, x, plan, edit, net.denoise if gmode is None else net.denoise_in_mode, first)
