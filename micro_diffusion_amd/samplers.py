"""Solvers of the EDM sampler, host side: names, the noise schedule and the per-step coefficients of the linear-multistep update
`x_next = a * x + b * (c1 * D - c2 * hist)` that `md_edm_solver_update(_tok)` applies (D: the denoised value of this step's one
network evaluation, hist: the previous step's D).  Pure Python in fp64: importable without a GPU and without the native library.

  heun      the reference's 2nd-order loop (model.py:231-297), 2 * steps - 1 evaluations; not of this form, it keeps its own kernels
  euler     1st order, one evaluation per step
  dpmpp_2m  DPM-Solver++(2M) (Lu et al. 2022, multistep data-prediction form) in the EDM parameterisation (alpha = 1, lambda = -ln sigma):
            2nd order, one evaluation per step
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

SAMPLERS = ("heun", "euler", "dpmpp_2m")
CHURN_SAMPLERS = ("heun", "euler")          # the churn of model.py:254-258 needs a solver without history


def check_sampler(sampler: str, S_churn: float = 0.0) -> str:
    if sampler not in SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r}: choose one of {', '.join(SAMPLERS)}")
    if S_churn > 0 and sampler not in CHURN_SAMPLERS:
        raise ValueError(f"sampler {sampler!r} is deterministic: S_churn > 0 is defined for {', '.join(CHURN_SAMPLERS)} only")
    return sampler


# ---------------------------------------------------------------------------------------------------------------------
# Image-conditioned sampling: image-to-image (SDEdit) starts the schedule late from known latents, inpainting holds the
# region where the mask is 0 at those latents, RePaint resampling repeats every step.  Both sampler loops take their step counts from
# the three helpers below.
# ---------------------------------------------------------------------------------------------------------------------
RESAMPLE_SAMPLERS = ("heun", "euler")       # the jump back to the step's own noise level needs a solver without history


def check_edit(sampler: str, has_init: bool, strength: float = 1.0, has_mask: bool = False, resample: int = 1) -> None:
    """Refuse, before anything is launched, allocated or drawn, an image-conditioned request that is not defined."""
    try:                                    # any real number: a Python or numpy scalar, a 0-dim tensor
        in_range = not isinstance(strength, (bool, str)) and 0.0 < float(strength) <= 1.0
    except (TypeError, ValueError, RuntimeError):     # not a number; a tensor of several elements
        in_range = False
    if not in_range:
        raise ValueError(f"strength must be a number in (0, 1], got {strength!r}")
    strength = float(strength)
    if strength < 1.0 and not has_init:
        raise ValueError(f"strength={strength!r} needs init_latents: without them the sampler starts from pure noise")
    if has_mask and not has_init:
        raise ValueError("inpaint_mask needs init_latents: the region where the mask is 0 is held at them")
    if isinstance(resample, bool) or not isinstance(resample, int) or resample < 1:
        raise ValueError(f"resample must be an integer >= 1, got {resample!r}")
    if resample > 1 and not has_mask:
        raise ValueError("resample > 1 harmonises the generated region with the kept one: it needs inpaint_mask")
    if resample > 1 and sampler not in RESAMPLE_SAMPLERS:
        raise ValueError(f"sampler {sampler!r} carries history across steps, which does not survive the jump back to the step's noise "
                         f"level: resample > 1 is defined for {', '.join(RESAMPLE_SAMPLERS)} only")


def edit_start_index(n: int, strength: float = 1.0) -> int:
    """i0, the first executed step of an n-step schedule: the last k = max(1, min(n, ceil(strength * n))) steps run."""
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must be in (0, 1], got {strength!r}")
    return n - max(1, min(n, math.ceil(strength * n)))


def edit_repetitions(t_steps: Sequence[float], i0: int = 0, resample: int = 1) -> List[int]:
    """How often each executed step i0 ... n - 1 runs (t_steps ends in 0): `resample` times, the step onto sigma = 0 once."""
    return [resample if t_steps[i + 1] > 0 else 1 for i in range(i0, len(t_steps) - 1)]


def edit_evaluations(sampler: str, n: int, strength: float = 1.0, resample: int = 1) -> int:
    """Network evaluations of a run: heun takes two per repetition (one for the step onto sigma = 0), the others one."""
    check_sampler(sampler)
    check_edit(sampler, True, strength, True, resample)
    reps = edit_repetitions(edm_schedule(n), edit_start_index(n, strength), resample)
    return sum(r * (2 if sampler == "heun" else 1) for r in reps[:-1]) + reps[-1]


def edm_schedule(steps: int, sigma_min: float = 0.002, sigma_max: float = 80.0, rho: float = 7.0) -> List[float]:
    """The EDM noise levels t_0 = sigma_max ... t_{steps-1} = sigma_min and a final 0 (model.py:238-243), fp64."""
    inv = 1.0 / rho
    t = [(sigma_max ** inv + i / (steps - 1) * (sigma_min ** inv - sigma_max ** inv)) ** rho for i in range(steps)]
    return t + [0.0]


def guidance_interval_bounds(guidance_interval) -> Optional[Tuple[float, float]]:
    if guidance_interval is None:
        return None
    lo, hi = guidance_interval
    lo, hi = float(lo), float(hi)
    if math.isnan(lo) or math.isnan(hi) or lo > hi:
        raise ValueError(f"guidance_interval must be (sigma_lo, sigma_hi) with sigma_lo <= sigma_hi, got {guidance_interval!r}")
    return lo, hi


def is_guided(sigma: float, cfg: float, interval: Optional[Tuple[float, float]]) -> bool:
    """Whether the evaluation at noise level sigma is guided: classifier-free guidance (network batch 2B) or, with a guide network,
    autoguidance (both networks at batch B)."""
    return cfg > 1.0 and (interval is None or interval[0] <= sigma <= interval[1])


# ---------------------------------------------------------------------------------------------------------------------
# Guidance modes.  A guided evaluation has the conditional denoised prediction D_c and a second operand D_u (the
# unconditional half of a doubled batch, or a guide network's).  "cfg" combines them as D_u + w (D_c - D_u).  "rescale" (Lin et al. 2024)
# and "apg" (Sadat et al. 2024) return alpha_b D_c + gamma_b M with M = (D_c - D_u) + beta M_prev the running difference and per-sample
# coefficients from five moments over [C, H, W]; guidance_coefficients is that table, shared by the tensor-op loop and the tests
# (md_guidance_prepare is its device form).
# ---------------------------------------------------------------------------------------------------------------------
GUIDANCE_MODES = ("cfg", "rescale", "apg")


def _finite_number(v) -> bool:
    try:
        return not isinstance(v, (bool, str)) and math.isfinite(float(v))
    except (TypeError, ValueError, RuntimeError):
        return False


def check_guidance(mode: str = "cfg", cfg: float = 1.0, guidance_rescale: float = 0.0, apg_eta: float = 0.0, apg_norm_threshold=None,
                   apg_momentum: float = 0.0) -> str:
    """Refuse, before anything is launched or allocated, a guidance request that is not defined: an unknown mode, a parameter of a
    mode that is not selected (a non-default guidance_rescale outside "rescale", a non-default apg_* outside "apg"), guidance_rescale
    outside [0, 1], apg_norm_threshold <= 0, |apg_momentum| >= 1, or anything that is not a finite number."""
    if mode not in GUIDANCE_MODES:
        raise ValueError(f"unknown guidance_mode {mode!r}: choose one of {', '.join(GUIDANCE_MODES)}")
    for name, v in (("cfg", cfg), ("guidance_rescale", guidance_rescale), ("apg_eta", apg_eta), ("apg_momentum", apg_momentum)):
        if not _finite_number(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if apg_norm_threshold is not None and not _finite_number(apg_norm_threshold):
        raise ValueError(f"apg_norm_threshold must be None or a finite number, got {apg_norm_threshold!r}")
    if mode != "rescale" and float(guidance_rescale) != 0.0:
        raise ValueError(f"guidance_rescale={guidance_rescale!r} needs guidance_mode='rescale' (got {mode!r})")
    if mode != "apg" and (float(apg_eta) != 0.0 or apg_norm_threshold is not None or float(apg_momentum) != 0.0):
        raise ValueError(f"apg_eta, apg_norm_threshold and apg_momentum need guidance_mode='apg' (got {mode!r})")
    if not 0.0 <= float(guidance_rescale) <= 1.0:
        raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale!r}")
    if apg_norm_threshold is not None and float(apg_norm_threshold) <= 0.0:
        raise ValueError(f"apg_norm_threshold must be None or > 0, got {apg_norm_threshold!r}")
    if abs(float(apg_momentum)) >= 1.0:
        raise ValueError(f"apg_momentum must be in (-1, 1), got {apg_momentum!r}")
    return mode


def guidance_moments(d_c, m):
    """[B, 5] fp64: (S_c, S_m, Q_cc, Q_mm, Q_cm) of every sample of two torch tensors [B, ...]."""
    import torch
    d_c, m = d_c.to(torch.float64).flatten(1), m.to(torch.float64).flatten(1)
    return torch.stack([d_c.sum(1), m.sum(1), (d_c * d_c).sum(1), (m * m).sum(1), (d_c * m).sum(1)], 1)


def guidance_coefficients(mode: str, moments, n: int, w: float, guidance_rescale: float = 0.0, apg_eta: float = 0.0, apg_norm_threshold=None):
    """(alpha, gamma), two fp64 tensors [B], of the guided prediction alpha_b D_c + gamma_b M from moments [B, 5] = (S_c, S_m, Q_cc,
    Q_mm, Q_cm) over the n elements of each sample.  The momentum is part of M, not of this table.
      apg      s = min(1, r / sqrt(Q_mm)) (1 without r or when Q_mm = 0);  p = s Q_cm / Q_cc (0 when Q_cc = 0);
               alpha = 1 - (w - 1)(1 - eta) p;  gamma = (w - 1) s
      rescale  var_c = max(Q_cc / n - (S_c / n)^2, 0);  var_g the same of D_c + (w - 1) M;  k = phi sqrt(var_c / var_g) + 1 - phi
               (1 when var_g <= 0);  alpha = k;  gamma = k (w - 1)"""
    import torch
    if mode not in ("rescale", "apg"):
        raise ValueError(f"no coefficients for guidance_mode {mode!r}: choose 'rescale' or 'apg'")
    mo = torch.as_tensor(moments, dtype=torch.float64)
    S_c, S_m, Q_cc, Q_mm, Q_cm = mo.unbind(-1)
    w1, one = float(w) - 1.0, torch.ones_like(S_c)
    if mode == "apg":
        s = one
        if apg_norm_threshold is not None:
            pos = Q_mm > 0
            s = torch.where(pos, torch.clamp(float(apg_norm_threshold) / torch.where(pos, Q_mm, one).sqrt(), max=1.0), one)
        pos = Q_cc > 0
        p = torch.where(pos, s * Q_cm / torch.where(pos, Q_cc, one), torch.zeros_like(S_c))
        return 1.0 - w1 * (1.0 - float(apg_eta)) * p, w1 * s
    phi = float(guidance_rescale)
    var_c = (Q_cc / n - (S_c / n) ** 2).clamp(min=0.0)
    S_g = S_c + w1 * S_m
    var_g = (Q_cc + 2.0 * w1 * Q_cm + w1 * w1 * Q_mm) / n - (S_g / n) ** 2
    pos = var_g > 0
    k = torch.where(pos, phi * (var_c / torch.where(pos, var_g, one)).sqrt() + 1.0 - phi, one)
    return k, k * w1


# ---------------------------------------------------------------------------------------------------------------------
# Measurement-guided sampling (Chung et al. 2023, "Diffusion Posterior Sampling").  At a step's first evaluation the
# guided denoised prediction D(x_hat) gives a per-sample loss L_b -- ||m * (meas - A(D))||^2 for an inverse.LinearMeasurement, or a
# caller's differentiable function --, and after the solver step x_next[b] -= scale / max(sqrt(L_b), GUIDE_TINY) * dL_b/dx_hat, the
# gradient taken through the network.
# ---------------------------------------------------------------------------------------------------------------------
GUIDE_TINY = 1e-30                          # floor of sqrt(L_b): MD_GUIDE_TINY of the native library


def _mask_shapes(B: int, H: int, W: int):
    return [(H, W), (1, H, W), (B, H, W), (1, 1, H, W), (B, 1, H, W)]


def check_measurement(shape, measurement=None, measurement_scale: float = 1.0, guidance_loss=None) -> bool:
    """Refuse, before anything is launched or allocated, a guided-sampling request that is not defined; True when the run is guided.
    shape: (B, C, H, W) of the sampler's state (None: only what does not depend on it is checked).  ValueError for a measurement_scale
    that is not a finite number >= 0, for measurement and guidance_loss together, for a measurement_scale other than 1 with nothing
    to scale, a guidance_loss that is not callable, and for a measurement (an object with meas, pool, mask: inverse.LinearMeasurement)
    whose pool is no integer >= 1 dividing H and W, whose meas is not a floating tensor [B, C, H / pool, W / pool], or whose mask is not
    [B or 1, 1, H / pool, W / pool] (or [B or 1, H / pool, W / pool], [H / pool, W / pool]), bool or float with values in [0, 1]."""
    if not _finite_number(measurement_scale) or float(measurement_scale) < 0.0:
        raise ValueError(f"measurement_scale must be a finite number >= 0, got {measurement_scale!r}")
    if measurement is not None and guidance_loss is not None:
        raise ValueError("measurement and guidance_loss are mutually exclusive: state the measurement's loss inside guidance_loss")
    if measurement is None and guidance_loss is None:
        if float(measurement_scale) != 1.0:
            raise ValueError(f"measurement_scale={measurement_scale!r} has nothing to scale: it needs measurement or guidance_loss")
        return False
    if guidance_loss is not None:
        if not callable(guidance_loss):
            raise ValueError(f"guidance_loss must be callable (D [B, C, H, W] -> losses [B]), got {type(guidance_loss).__name__}")
        return True
    for name in ("meas", "pool", "mask"):
        if not hasattr(measurement, name):
            raise ValueError(f"measurement must be an inverse.LinearMeasurement (meas, pool, mask), got {type(measurement).__name__}")
    s, meas, mask = measurement.pool, measurement.meas, measurement.mask
    if isinstance(s, bool) or not isinstance(s, int) or s < 1:
        raise ValueError(f"measurement.pool must be an integer >= 1, got {s!r}")
    if not hasattr(meas, "shape") or not getattr(meas, "is_floating_point", lambda: False)():
        raise ValueError("measurement.meas must be a floating-point tensor")
    if mask is not None and not hasattr(mask, "shape"):
        raise ValueError("measurement.mask must be a tensor or None")
    if shape is None:
        return True
    B, C, H, W = (int(v) for v in shape)
    if H % s or W % s:
        raise ValueError(f"measurement.pool={s} does not divide the latent grid {H} x {W}")
    Hs, Ws = H // s, W // s
    if tuple(meas.shape) != (B, C, Hs, Ws):
        raise ValueError(f"measurement.meas has shape {tuple(meas.shape)}: expected {(B, C, Hs, Ws)} (the pooled grid of {(B, C, H, W)})")
    if mask is not None:
        if tuple(mask.shape) not in _mask_shapes(B, Hs, Ws):
            raise ValueError(f"measurement.mask has shape {tuple(mask.shape)}: expected [{B} or 1, 1, {Hs}, {Ws}], [{B} or 1, {Hs}, {Ws}] or "
                             f"[{Hs}, {Ws}]")
        import torch
        if mask.dtype != torch.bool:
            if not mask.is_floating_point() or not bool(((mask >= 0) & (mask <= 1)).all()):
                raise ValueError("measurement.mask must be bool or hold float values in [0, 1] (1 = measured, 0 = ignored)")
    return True


GUIDE_CAPTIONS = ("same", "null")           # what an autoguidance guide is conditioned on: the captions, or zeroed captions
GUIDE_GEOMETRY = ("in_channels", "patch_size", "input_size", "caption_channels")


def _module_device(module):
    params = getattr(module, "parameters", None)
    first = next(iter(params()), None) if params is not None else None
    return None if first is None else first.device


def check_guide(main, guide, guide_captions: str = "same") -> None:
    """Refuse, before anything is launched or allocated, an autoguidance request the sampler cannot run: an unknown `guide_captions`,
    "null" without a guide, a guide whose latent / patch / caption geometry (config fields GUIDE_GEOMETRY) differs from main's -- the
    two networks read the same network input and their outputs are combined element by element --, or a guide on another device.
    A guide that is main itself is legal (with "same" the combine returns main's output for every weight)."""
    if guide_captions not in GUIDE_CAPTIONS:
        raise ValueError(f"unknown guide_captions {guide_captions!r}: choose one of {', '.join(GUIDE_CAPTIONS)}")
    if guide is None:
        if guide_captions != "same":
            raise ValueError(f"guide_captions={guide_captions!r} needs a guide")
        return
    if guide is main:
        return
    for name in GUIDE_GEOMETRY:
        a, b = getattr(main.config, name), getattr(guide.config, name)
        if a != b:
            raise ValueError(f"the guide's {name} ({b}) differs from the main network's ({a})")
    da, db = _module_device(main), _module_device(guide)
    if da != db:
        raise ValueError(f"the guide is on {db}, the main network on {da}: both must be on the same device")


def check_step_cache(step_cache=None, guide=None, measurement=None, guidance_loss=None) -> bool:
    """Refuse, before anything is launched or allocated, a step-cache request the sampler cannot run; True when the run
    caches.  ValueError for an object that is not a step_cache.StepCache (anything without its step / reset / engine_args), for a
    guide network (autoguidance: the second network would need a cache and a policy of its own), and for measurement / guidance_loss,
    whose taped evaluation needs every block."""
    if step_cache is None:
        return False
    for name in ("step", "reset", "engine_args"):
        if not callable(getattr(step_cache, name, None)):
            raise ValueError(f"step_cache must be a step_cache.StepCache, got {type(step_cache).__name__}")
    if guide is not None:
        raise ValueError("step_cache with guide= (autoguidance) is not defined: the guide network would need a cache of its own")
    if measurement is not None or guidance_loss is not None:
        raise ValueError("step_cache with measurement= / guidance_loss= is not defined: the taped evaluation of a guided step needs "
                         "every block")
    return True


def check_attn_maps(attn_maps=None, config=None) -> bool:
    """Refuse, before anything is tokenised, launched or allocated, an attention-map request the sampler cannot run; True
    when the run records.  ValueError for an object that is not an attn_maps.AttentionMaps (anything without its resolve / start_run /
    begin_evaluation / record) and, with the model's DiTConfig given, for a block selection that matches none of its blocks.  Nothing
    else is refused: the recorder only reads, so it composes with every other option."""
    if attn_maps is None:
        return False
    for name in ("resolve", "start_run", "begin_evaluation", "skip_evaluation", "record"):
        if not callable(getattr(attn_maps, name, None)):
            raise ValueError(f"attn_maps must be an attn_maps.AttentionMaps, got {type(attn_maps).__name__}")
    if config is not None:
        from .attn_maps import block_names, select_blocks
        select_blocks(block_names(config), attn_maps.blocks)
    return True


def check_mxfp8(mxfp8=None, measurement=None, guidance_loss=None) -> bool:
    """Refuse, before anything is quantised, launched or allocated, an MXFP8 request the sampler cannot run; True when
    the run quantises.  mxfp8: None, True (the sampler quantises the main network's default targets for this run) or an
    mxfp8.MXWeights.  ValueError for anything else (False included: leave the argument out instead) and for measurement= /
    guidance_loss=, whose backward through the network has no MXFP8 form.  Everything else composes: every solver, churn, the guidance
    interval and modes, cond_cache, step_cache, the editing options, attn_maps and prompt control; with guide= only the main network
    is quantised."""
    if mxfp8 is None:
        return False
    if mxfp8 is not True:
        if mxfp8 is False or not (isinstance(getattr(mxfp8, "entries", None), dict) and callable(getattr(mxfp8, "check_fresh", None))
                                  and callable(getattr(mxfp8, "requantize", None))):
            raise ValueError(f"mxfp8 must be None, True or an mxfp8.MXWeights, got {mxfp8!r}")
    if measurement is not None or guidance_loss is not None:
        raise ValueError("mxfp8 with measurement= / guidance_loss= is not defined: the guided step needs a backward through the network, "
                         "and the MXFP8 linears are forward-only (DESIGN.md 4.23)")
    return True


# ---------------------------------------------------------------------------------------------------------------------
# Prompt control: a negative prompt as the second operand of classifier-free guidance, and per-position caption
# weights w_j >= 0 that enter every cross-attention as the additive bias ln w_j on the logits: P_j = w_j e^{s_j} / sum_i w_i e^{s_i}
# (w = 1: today's softmax, w = 0: the position is removed).
# ---------------------------------------------------------------------------------------------------------------------
def _check_weights(name: str, w, B: Optional[int], Lc: Optional[int]) -> None:
    import torch
    if not torch.is_tensor(w):
        raise ValueError(f"{name} must be a tensor [B, Lc], [1, Lc] or [Lc], got {type(w).__name__}")
    if w.dtype != torch.bool and not w.dtype.is_floating_point:
        raise ValueError(f"{name} must be bool or floating point, got {w.dtype}")
    if w.dim() not in (1, 2) or w.shape[-1] < 1:
        raise ValueError(f"{name} has shape {tuple(w.shape)}: expected [B, Lc], [1, Lc] or [Lc]")
    if Lc is not None and (w.shape[-1] != Lc or (w.dim() == 2 and w.shape[0] not in (1, B))):
        raise ValueError(f"{name} has shape {tuple(w.shape)}: expected [{B}, {Lc}], [1, {Lc}] or [{Lc}]")
    v = w.detach().to(torch.float32)
    if not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
        raise ValueError(f"{name} must be finite and >= 0 (0 removes a caption position)")
    if not bool((v > 0).any(dim=-1).all()):
        raise ValueError(f"{name}: every row needs at least one weight > 0 (a caption with every position removed has no softmax)")


def check_prompt_control(has_negative: bool = False, caption_weights=None, negative_weights=None, cfg: float = 1.0, guide=None,
                         measurement=None, guidance_loss=None, negative=None, y_shape=None, will_weight: bool = False) -> bool:
    """Refuse, before anything is tokenised, launched or allocated, a prompt-control request that is not defined; True
    when the run arms a caption bias (any weights).
    has_negative: the run has a negative prompt; negative: its embeddings once they exist.  will_weight: weights will be made later
    (generate's mask_padding).  y_shape: the shape of the caption embeddings y once it is known; the shapes are then checked too:
    negative as y or with a leading 1, weights [B, Lc], [1, Lc] or [Lc].
    ValueError for a wrong shape, a negative or non-finite weight, a row without a positive weight, a negative prompt with cfg <= 1
    (there is no second operand to replace), negative_weights without a negative prompt, any of the three with guide= (the guide may
    share the engine and needs a bias of its own: not done), and weights with measurement= / guidance_loss= (their backward does not
    know the bias).  A negative prompt alone composes with those two."""
    has_negative = bool(has_negative) or negative is not None
    weights = caption_weights is not None or negative_weights is not None or bool(will_weight)
    if not has_negative and not weights:
        return False
    if guide is not None:
        raise ValueError("negative / caption_weights / negative_weights with guide= (autoguidance) is not done: the guide may share the "
                         "engine and needs a caption bias of its own (DESIGN.md 4.22)")
    if has_negative and not float(cfg) > 1.0:
        raise ValueError(f"a negative prompt replaces the second operand of classifier-free guidance: it needs cfg > 1, got {cfg!r}")
    if negative_weights is not None and not has_negative:
        raise ValueError("negative_weights needs negative= (a negative prompt): they weight its positions")
    if weights and (measurement is not None or guidance_loss is not None):
        raise ValueError("caption_weights / negative_weights with measurement= / guidance_loss= is not defined: the attention backward "
                         "does not know the caption bias (DESIGN.md 4.22)")
    B = Lc = None
    if y_shape is not None:
        B, Lc = int(y_shape[0]), int(y_shape[-2])
        if negative is not None and not (len(negative.shape) == len(y_shape) and tuple(negative.shape[1:]) == tuple(y_shape[1:])
                                         and negative.shape[0] in (1, B)):
            raise ValueError(f"negative has shape {tuple(negative.shape)}, the captions {tuple(y_shape)}: expected that shape, or a "
                             "leading 1 that is broadcast")
    for name, w in (("caption_weights", caption_weights), ("negative_weights", negative_weights)):
        if w is not None:
            _check_weights(name, w, B, Lc)
    return weights


def caption_log_bias(weights, B: int, Lc: int, device=None):
    """ln w of caption weights ([B, Lc], [1, Lc] or [Lc]; bool or floating point) as fp32 [B, Lc] on `device`: 0 at w = 1, -inf at 0."""
    import torch
    w = weights.detach().to(device=device, dtype=torch.float32).reshape(-1, Lc).expand(B, Lc)
    return torch.log(w)


def caption_bias_buffer(caption_weights, negative_weights, B: int, Lc: int, doubled: bool, device=None):
    """The caption bias of one run: fp32 [2 B, ldb] when the run doubles evaluations (rows [0, B): the captions, [B, 2 B): the second
    half), else [B, ldb]; ldb = Lc rounded up to 4.  A half without weights and the pad columns [Lc, ldb) hold 0."""
    import torch
    ldb = (Lc + 3) // 4 * 4
    buf = torch.zeros((2 * B if doubled else B), ldb, device=device, dtype=torch.float32)
    if caption_weights is not None:
        buf[:B, :Lc] = caption_log_bias(caption_weights, B, Lc, device)
    if doubled and negative_weights is not None:
        buf[B:, :Lc] = caption_log_bias(negative_weights, B, Lc, device)
    return buf


def evaluation_sigmas(sampler: str, t_steps: Sequence[float]) -> List[float]:
    """The noise level of every network evaluation of a run without churn, in order."""
    out = []
    for i, (t_cur, t_next) in enumerate(zip(t_steps[:-1], t_steps[1:])):
        out.append(t_cur)
        if sampler == "heun" and t_next > 0:
            out.append(t_next)
    return out


def solver_coefficients(solver: str, t_steps: Sequence[float], t_hat: Optional[Sequence[float]] = None) -> List[Tuple[float, float, float, float]]:
    """(a, b, c1, c2) of every step i: t_steps[i] -> t_steps[i + 1] (t_steps ends in 0; the step onto 0 returns D itself).
    t_hat (euler only): the churned noise level each step is evaluated at, in place of t_steps[i]."""
    if solver not in ("euler", "dpmpp_2m"):
        raise ValueError(f"no linear-multistep coefficients for sampler {solver!r}")
    t = [float(v) for v in t_steps]
    n = len(t) - 1
    cur = t[:-1] if t_hat is None else [float(v) for v in t_hat]
    if len(cur) != n:
        raise ValueError("t_hat needs one entry per step")
    if solver == "dpmpp_2m" and cur != t[:-1]:
        raise ValueError("dpmpp_2m carries history across steps: it cannot start a step from a churned noise level")
    out = []
    for i in range(n):
        t_cur, t_next = cur[i], t[i + 1]
        if t_next == 0.0:                                     # lambda_next = inf: a = 0, b = -expm1(-inf) = 1, no history
            out.append((0.0, 1.0, 1.0, 0.0))
            continue
        a = t_next / t_cur
        if solver == "euler":
            out.append((a, 1.0 - a, 1.0, 0.0))
            continue
        h = math.log(t_cur) - math.log(t_next)                # lambda_next - lambda_cur
        b = -math.expm1(-h)
        if i == 0:
            out.append((a, b, 1.0, 0.0))
            continue
        r = (math.log(t[i - 1]) - math.log(t_cur)) / h         # (lambda_cur - lambda_prev) / h
        out.append((a, b, 1.0 + 1.0 / (2.0 * r), 1.0 / (2.0 * r)))
    return out
