"""Hydra-free loader for the reference's YAML stage configs (reference configs/*.yaml, train.py:14-22):
`--config-path DIR --config-name FILE key.sub=value ...`, `${a.b}` interpolation, `_target_` instantiation with the
reference's class paths mapped onto this package's MI355X-native equivalents."""
from __future__ import annotations

import importlib
import os
import re
from typing import Any, Dict, List

import yaml

# reference `_target_` -> native implementation ("module:attr"); None = accepted and ignored (host-side observability
# that has no counterpart on the hot path: loggers / monitors; see DESIGN.md "out of scope").  Two of the ignored callbacks are
# honoured by train.py through switches instead of objects: OptimizerMonitor -> misc.optimizer_monitor_interval
# (names_target below tells whether the config lists it), NaNCatcher -> the per-step loss check or misc.skip_nonfinite_steps.
TARGETS = {
    "micro_diffusion.models.model.create_latent_diffusion": "micro_diffusion_amd.model:create_latent_diffusion",
    "torch.optim.AdamW": "micro_diffusion_amd.trainer:FusedAdamW",
    "composer.optim.CosineAnnealingWithWarmupScheduler": "micro_diffusion_amd.trainer:LRSchedule",
    "composer.optim.ConstantScheduler": "micro_diffusion_amd.trainer:LRSchedule",
    "composer.optim.ConstantWithWarmupScheduler": "micro_diffusion_amd.trainer:LRSchedule",
    "micro_diffusion.datasets.latents_loader.build_streaming_latents_dataloader":
        "micro_diffusion_amd.data:build_streaming_latents_dataloader",
    "composer.Trainer": "micro_diffusion_amd.trainer:Trainer",
    "composer.loggers.TensorboardLogger": None,
    "composer.loggers.wandb_logger.WandBLogger": None,
    "composer.callbacks.speed_monitor.SpeedMonitor": None,
    "composer.callbacks.lr_monitor.LRMonitor": None,
    "composer.callbacks.runtime_estimator.RuntimeEstimator": None,
    "composer.callbacks.OptimizerMonitor": None,
    "micro_diffusion.models.callbacks.LogDiffusionImages": None,
    "micro_diffusion.models.callbacks.NaNCatcher": None,
    "diffusion.algorithms.ema.EMA": None,
}


def _parse_scalar(text: str) -> Any:
    return yaml.safe_load(text)


def apply_overrides(cfg: Dict[str, Any], overrides: List[str]) -> None:
    """Hydra-style dot-list overrides: `a.b.c=value` (value parsed as YAML), `+a.b=value` adds a new key."""
    for ov in overrides:
        if "=" not in ov:
            raise ValueError(f"override '{ov}' is not of the form key=value")
        key, val = ov.split("=", 1)
        key = key.lstrip("+")
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            if p not in node or not isinstance(node[p], dict):
                node[p] = {}
            node = node[p]
        node[parts[-1]] = _parse_scalar(val)


_INTERP = re.compile(r"\$\{([^}]+)\}")
_FLOATISH = re.compile(r"[-+]?(\d+\.?\d*|\.\d+)[eE][-+]?\d+")


def coerce_numbers(cfg: Any) -> Any:
    """PyYAML (YAML 1.1) reads `8e-5` as a string; hydra/OmegaConf reads a float.  Match the latter."""
    if isinstance(cfg, dict):
        return {k: coerce_numbers(v) for k, v in cfg.items()}
    if isinstance(cfg, list):
        return [coerce_numbers(v) for v in cfg]
    if isinstance(cfg, str) and _FLOATISH.fullmatch(cfg.strip()):
        return float(cfg)
    return cfg


def _lookup(root: Dict[str, Any], dotted: str) -> Any:
    node: Any = root
    for p in dotted.split("."):
        node = node[p]
    return node


def resolve(cfg: Any, root: Dict[str, Any] = None) -> Any:
    """Resolve `${path.to.key}` references (whole-value references keep their type)."""
    root = cfg if root is None else root
    if isinstance(cfg, dict):
        return {k: resolve(v, root) for k, v in cfg.items()}
    if isinstance(cfg, list):
        return [resolve(v, root) for v in cfg]
    if isinstance(cfg, str):
        m = _INTERP.fullmatch(cfg.strip())
        if m:
            return resolve(_lookup(root, m.group(1)), root)
        return _INTERP.sub(lambda mm: str(resolve(_lookup(root, mm.group(1)), root)), cfg)
    return cfg


def load_config(config_path: str, config_name: str, overrides: List[str] = ()) -> Dict[str, Any]:
    fn = os.path.join(config_path, config_name)
    if not os.path.exists(fn) and not fn.endswith((".yaml", ".yml")):
        fn += ".yaml"
    with open(fn) as fh:
        cfg = coerce_numbers(yaml.safe_load(fh))
    apply_overrides(cfg, list(overrides))
    return coerce_numbers(resolve(cfg))


def names_target(cfg: Any, target: str) -> bool:
    """True when any node of the config carries `_target_: <target>`."""
    if isinstance(cfg, dict):
        return cfg.get("_target_") == target or any(names_target(v, target) for v in cfg.values())
    if isinstance(cfg, list):
        return any(names_target(v, target) for v in cfg)
    return False


def diagnostics_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The Trainer's diagnostics switches from the `misc` section, all off unless the config sets them:
    misc.diagnostics_interval (batches between reports), misc.loss_by_sigma_bins (0 = no loss-by-sigma histogram),
    misc.moe_routing_monitor (expert-choice routing statistics on the report batches)."""
    misc = cfg.get("misc") or {}
    return {"diagnostics_interval": int(misc.get("diagnostics_interval", 0) or 0),
            "loss_by_sigma_bins": int(misc.get("loss_by_sigma_bins", 0) or 0),
            "moe_routing": bool(misc.get("moe_routing_monitor", False))}


def posthoc_ema_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The post-hoc EMA switches of the `misc` section, off unless the config sets them:
    misc.posthoc_ema_sigma_rels=[0.05,0.10] (1 .. 4 relative widths, each inside (0, 0.28)) and
    misc.posthoc_ema_snapshot_interval=<N>ba (0 / absent: the averages are tracked and checkpointed, no snapshot is written).
    Returns {"sigma_rels": tuple, "snapshot_interval": batches}; raises ValueError on values the optimiser cannot honour."""
    from .posthoc_ema import MAX_PROFILES, SIGMA_REL_MAX
    misc = cfg.get("misc") or {}
    raw = misc.get("posthoc_ema_sigma_rels")
    if raw is None or raw == [] or raw == "":
        rels = ()
    elif isinstance(raw, (int, float)):
        rels = (float(raw),)
    elif isinstance(raw, (list, tuple)):
        rels = tuple(float(v) for v in raw)
    else:
        raise ValueError(f"misc.posthoc_ema_sigma_rels must be a list of numbers, got {raw!r}")
    if len(rels) > MAX_PROFILES:
        raise ValueError(f"misc.posthoc_ema_sigma_rels: at most {MAX_PROFILES} profiles (MD_EMA_MAX_PROFILES), got {len(rels)}")
    for s in rels:
        if not 0.0 < s < SIGMA_REL_MAX:
            raise ValueError(f"misc.posthoc_ema_sigma_rels: {s} is outside (0, {SIGMA_REL_MAX})")
    if len(set(rels)) != len(rels):
        raise ValueError(f"misc.posthoc_ema_sigma_rels: duplicate values in {list(rels)}")
    iv = misc.get("posthoc_ema_snapshot_interval", 0) or 0
    if not isinstance(iv, int):
        from .trainer import parse_batches
        iv = parse_batches(iv)
    if iv < 0:
        raise ValueError("misc.posthoc_ema_snapshot_interval must not be negative")
    if iv and not rels:
        raise ValueError("misc.posthoc_ema_snapshot_interval needs misc.posthoc_ema_sigma_rels")
    return {"sigma_rels": rels, "snapshot_interval": int(iv)}


def loss_weighting_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The learned loss-weighting switches of the `misc` section, off unless the config sets them:
    misc.loss_uncertainty_weighting (bool), misc.loss_uncertainty_channels (64 / 128 / 192 / 256, default 128) and
    misc.loss_uncertainty_lr (default: the optimiser's lr; the schedule factor applies to both).
    Returns {"enabled": bool, "channels": int, "lr": float or None}; raises ValueError on values the kernels cannot honour and on
    channels / lr given without the switch."""
    from .loss_weighting import CHANNEL_CHOICES, check_channels
    misc = cfg.get("misc") or {}
    on = misc.get("loss_uncertainty_weighting", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"misc.loss_uncertainty_weighting must be true or false, got {on!r}")
    ch, lr = misc.get("loss_uncertainty_channels"), misc.get("loss_uncertainty_lr")
    if not on:
        for key, v in (("loss_uncertainty_channels", ch), ("loss_uncertainty_lr", lr)):
            if v is not None:
                raise ValueError(f"misc.{key} needs misc.loss_uncertainty_weighting=true")
        return {"enabled": False, "channels": 128, "lr": None}
    try:
        ch = check_channels(128 if ch is None else ch)
    except ValueError:
        raise ValueError(f"misc.loss_uncertainty_channels must be one of {CHANNEL_CHOICES}, got {ch!r}") from None
    if lr is not None:
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not lr >= 0 or lr == float("inf"):
            raise ValueError(f"misc.loss_uncertainty_lr must be a non-negative number, got {lr!r}")
        lr = float(lr)
    return {"enabled": True, "channels": ch, "lr": lr}


def disperse_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The dispersive-loss switches of the `misc` section, off unless the config sets them: misc.disperse_weight
    (lambda; 0 / absent: off; the untuned starting value is 0.5), misc.disperse_tau (default 0.5) and misc.disperse_block (index of the
    backbone block whose output is regularised; default depth // 4, checked against the model by the Trainer).
    Returns {"enabled": bool, "weight": float, "tau": float, "block": int or None}; raises ValueError on values the kernels cannot honour
    and on tau / block given without a positive weight."""
    import math
    misc = cfg.get("misc") or {}
    w = misc.get("disperse_weight", 0.0)
    w = 0.0 if w is None else w
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or w < 0:
        raise ValueError(f"misc.disperse_weight must be a finite number >= 0, got {w!r}")
    tau, blk = misc.get("disperse_tau"), misc.get("disperse_block")
    if not w > 0:
        for key, v in (("disperse_tau", tau), ("disperse_block", blk)):
            if v is not None:
                raise ValueError(f"misc.{key} needs misc.disperse_weight > 0")
        return {"enabled": False, "weight": 0.0, "tau": 0.5, "block": None}
    tau = 0.5 if tau is None else tau
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not math.isfinite(tau) or not tau > 0:
        raise ValueError(f"misc.disperse_tau must be a finite number > 0, got {tau!r}")
    if blk is not None and (isinstance(blk, bool) or not isinstance(blk, int) or blk < 0):
        raise ValueError(f"misc.disperse_block must be a block index >= 0, got {blk!r}")
    return {"enabled": True, "weight": float(w), "tau": float(tau), "block": blk}


def lora_options(cfg: Dict[str, Any], world: Any = None) -> Dict[str, Any]:
    """The LoRA switches of the `misc` section, off unless the config sets them: misc.lora_rank (0 / absent: off; one of
    4, 8, 16, 32, 64), misc.lora_alpha (default: the rank), misc.lora_targets (regular expressions on parameter names; default: the five
    attention projections of every block), misc.lora_weight_decay (default 0) and misc.lora_load_path (an adapter file to start from).
    Returns {"enabled", "rank", "alpha", "targets", "weight_decay", "load_path"}.  Raises ValueError on values the kernels cannot
    honour, on the other keys given without a rank, and on what LoRA training does not cover: more than one rank (`world`, default the
    WORLD_SIZE environment variable) unless misc.lora_backward is "factored" (lora_backward_option), algorithms.ema, misc.posthoc_ema_* and misc.optimizer_monitor_interval > 0."""
    import os
    from .lora import DEFAULT_TARGETS, RANKS
    misc = cfg.get("misc") or {}
    rank = misc.get("lora_rank", 0)
    if rank is None:
        rank = 0
    if isinstance(rank, bool) or not isinstance(rank, int) or (rank != 0 and rank not in RANKS):
        raise ValueError(f"misc.lora_rank must be 0 (off) or one of {RANKS}, got {rank!r}")
    keys = ("lora_alpha", "lora_targets", "lora_weight_decay", "lora_load_path")
    if rank == 0:
        for k in keys:
            if misc.get(k) is not None:
                raise ValueError(f"misc.{k} needs misc.lora_rank")
        return {"enabled": False, "rank": 0, "alpha": None, "targets": list(DEFAULT_TARGETS), "weight_decay": 0.0, "load_path": None}
    alpha = misc.get("lora_alpha")
    if alpha is not None:
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or alpha != alpha or alpha in (float("inf"), float("-inf")):
            raise ValueError(f"misc.lora_alpha must be a finite number, got {alpha!r}")
        alpha = float(alpha)
    targets = misc.get("lora_targets")
    if targets is None:
        targets = list(DEFAULT_TARGETS)
    elif isinstance(targets, str):
        targets = [targets]
    elif isinstance(targets, (list, tuple)) and targets and all(isinstance(t, str) for t in targets):
        targets = list(targets)
    else:
        raise ValueError(f"misc.lora_targets must be a non-empty list of regular expressions, got {targets!r}")
    import re
    for t in targets:
        try:
            re.compile(t)
        except re.error as e:
            raise ValueError(f"misc.lora_targets: {t!r} is not a regular expression ({e})") from None
    wd = misc.get("lora_weight_decay", 0.0)
    wd = 0.0 if wd is None else wd
    if isinstance(wd, bool) or not isinstance(wd, (int, float)) or not wd >= 0 or wd == float("inf"):
        raise ValueError(f"misc.lora_weight_decay must be a non-negative number, got {wd!r}")
    path = misc.get("lora_load_path")
    if path is not None and not isinstance(path, str):
        raise ValueError(f"misc.lora_load_path must be a path, got {path!r}")
    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else int(world)
    if world > 1 and lora_backward_option(cfg) != "factored":
        raise ValueError(f"misc.lora_rank: LoRA training is single-GPU for now (WORLD_SIZE = {world}); data parallelism is a follow-up "
                         "of the projected backward; misc.lora_backward: factored trains data-parallel")
    if (cfg.get("algorithms") or {}).get("ema"):
        raise ValueError("misc.lora_rank with algorithms.ema: the adapter is a few MB, an average of the frozen base is not kept")
    for k in ("posthoc_ema_sigma_rels", "posthoc_ema_snapshot_interval"):
        if misc.get(k):
            raise ValueError(f"misc.lora_rank with misc.{k}: the post-hoc averages cover the base's masters, which LoRA leaves frozen")
    if int(misc.get("optimizer_monitor_interval", 0) or 0) > 0:
        raise ValueError("misc.lora_rank with misc.optimizer_monitor_interval > 0: the monitor's tables cover the base's optimiser pass")
    return {"enabled": True, "rank": rank, "alpha": alpha, "targets": targets, "weight_decay": float(wd), "load_path": path}


def lora_backward_option(cfg: Dict[str, Any]) -> str:
    """misc.lora_backward: "projected" (default: dA, dB projected once per step from the base's accumulated gradient) or
    "factored" (dA, dB straight from every targeted linear's dy and x; the base's gradient is never formed, data parallelism is
    available).  Its own function: lora_options' dict stays what it was.  Raises ValueError on another value and on the key without
    misc.lora_rank."""
    from .lora import BACKWARDS
    misc = cfg.get("misc") or {}
    mode = misc.get("lora_backward")
    if mode is None:
        return "projected"
    if not isinstance(mode, str) or mode not in BACKWARDS:
        raise ValueError(f"misc.lora_backward must be one of {BACKWARDS}, got {mode!r}")
    if not misc.get("lora_rank"):
        raise ValueError("misc.lora_backward needs misc.lora_rank")
    return mode


def muon_options(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The Muon switches of the `misc` section, off unless the config sets them: misc.muon (bool), misc.muon_momentum
    (default 0.95), misc.muon_nesterov (default true), misc.muon_ns_steps (1 .. 8, default 5), misc.muon_adjust ("rms" | "spectral"),
    misc.muon_targets (regular expressions on parameter names; default: the hidden projections of every block) and misc.muon_adamw_lr
    (learning rate of the AdamW part; default: the optimiser's lr).
    Returns {"enabled", "momentum", "nesterov", "ns_steps", "adjust", "targets", "adamw_lr"}.  Raises ValueError on values the optimiser
    cannot honour, on the other keys given without misc.muon=true, and with misc.lora_rank (the adapter assumes a frozen base)."""
    import re
    from .muon import DEFAULT_TARGETS, check_hyper
    misc = cfg.get("misc") or {}
    on = misc.get("muon", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"misc.muon must be true or false, got {on!r}")
    keys = ("muon_momentum", "muon_nesterov", "muon_ns_steps", "muon_adjust", "muon_targets", "muon_adamw_lr")
    off = {"enabled": False, "momentum": 0.95, "nesterov": True, "ns_steps": 5, "adjust": "rms", "targets": list(DEFAULT_TARGETS),
           "adamw_lr": None}
    if not on:
        for k in keys:
            if misc.get(k) is not None:
                raise ValueError(f"misc.{k} needs misc.muon=true")
        return off
    if misc.get("lora_rank"):
        raise ValueError("misc.muon with misc.lora_rank: the adapter is trained on a frozen base, which Muon would update")
    out = dict(off, enabled=True)
    for k in ("momentum", "nesterov", "ns_steps", "adjust", "adamw_lr"):
        if misc.get("muon_" + k) is not None:
            out[k] = misc["muon_" + k]
    try:
        check_hyper(out["momentum"], out["nesterov"], out["ns_steps"], out["adjust"], out["adamw_lr"])
    except ValueError as e:
        raise ValueError("misc.muon_*: " + str(e)) from None
    out["momentum"] = float(out["momentum"])
    if out["adamw_lr"] is not None:
        out["adamw_lr"] = float(out["adamw_lr"])
    targets = misc.get("muon_targets")
    if targets is not None:
        if isinstance(targets, str):
            targets = [targets]
        elif not (isinstance(targets, (list, tuple)) and targets and all(isinstance(t, str) for t in targets)):
            raise ValueError(f"misc.muon_targets must be a non-empty list of regular expressions, got {targets!r}")
        for t in targets:
            try:
                re.compile(t)
            except re.error as e:
                raise ValueError(f"misc.muon_targets: {t!r} is not a regular expression ({e})") from None
        out["targets"] = list(targets)
    return out


def locate(target: str):
    native = TARGETS.get(target, target)
    if native is None:
        return None
    if ":" in native:
        mod, attr = native.split(":")
    else:
        mod, attr = native.rsplit(".", 1)
    return getattr(importlib.import_module(mod), attr)


def instantiate(node: Dict[str, Any], **extra):
    """hydra.utils.instantiate for the subset the reference uses (flat kwargs, `_target_`)."""
    node = dict(node)
    target = node.pop("_target_")
    fn = locate(target)
    if fn is None:
        return None
    node.update(extra)
    return fn(**node)
