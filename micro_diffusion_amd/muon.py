"""Muon (opt-in): orthogonalised momentum for the hidden matrices of the DiT blocks (Jordan et al. 2024, "Muon: an
optimizer for hidden layers in neural networks"; Liu et al. 2025, "Muon is Scalable for LLM Training").  No reference counterpart: the
reference trains every tensor with AdamW.  Untuned for MicroDiT, no quality claim: the hyper-parameters are the papers'.

For every targeted matrix W with accumulated gradient g (every expert of a 3-D expert tensor is its own matrix):

    m <- mu m + g        u = g + mu m (Nesterov)        O = NewtonSchulz_k(u / ||u||_F)        W <- W (1 - lr wd) - lr s O

with s = 0.2 sqrt(max(rows, cols)) (adjust="rms", Liu et al.: the update then has AdamW's RMS, so lr and weight_decay are shared with
the AdamW part) or s = sqrt(max(1, rows / cols)) (adjust="spectral", Jordan).  Everything that is not targeted -- embedders, caption
stream, adaLN modulation, final layer, MoE router, biases, norms -- keeps AdamW: the unchanged md_adamw_step on the contiguous runs of
the flat buffers between the targets.  `Muon` is a FusedAdamW: the Trainer steps it through the same `opt.step(...)` call.

State: the Muon momentum lives in the `m` flat buffer on the targeted tensors; `v` stays zero there (the spare 4 bytes per targeted
parameter are accepted: freeing them would change the by-name state layout).  The workspace of the iteration holds, per matrix, the bf16
iterate and two Gram-sized bf16 matrices, plus one fp32 scratch the size of the largest matrix (md_muon_ws_bytes).  `device="cpu"` holds the state only (target resolution, state_dict
round trips); the kernels need a GPU.  The `ref_*` functions restate the shape factors for the tests."""
from __future__ import annotations

import math
import re
import warnings
from ctypes import byref, c_int32, c_int64
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .arch import ParamSpec
from .optim import FusedAdamW

_BLOCK = r"^(patch_mixer|blocks)\.\d+\."
# the hidden projections of every mixer and backbone block: the five attention projections, the dense SwiGLU and the 3-D expert tensors
# (not the caption block's y_emb_preprocess.*, not mlp.gate, not adaLN_modulation)
DEFAULT_TARGETS = tuple(_BLOCK + m + r"\.weight$" for m in (r"attn\.qkv", r"attn\.proj", r"cross_attn\.q_linear", r"cross_attn\.kv_linear",
                                                            r"cross_attn\.proj", r"mlp\.w1", r"mlp\.w2", r"mlp\.w3")) + (_BLOCK + r"mlp\.w[12]$",)
ADJUSTS = ("rms", "spectral")
NS_COEFFS = (3.4445, -4.7750, 2.0315)        # Jordan's quintic
NS_STEPS_MAX = 8
DIM_MULTIPLE = 64                            # what md_muon_* accept for rows and cols


def shape_scale(adjust: str, rows: int, cols: int) -> float:
    """The factor s of the update lr * s * O for a [rows, cols] matrix."""
    if adjust == "rms":
        return 0.2 * math.sqrt(max(rows, cols))
    if adjust == "spectral":
        return math.sqrt(max(1.0, rows / cols))
    raise ValueError(f"muon: adjust must be one of {ADJUSTS}, got {adjust!r}")


def resolve_targets(table: Sequence[ParamSpec], targets: Sequence[str]) -> List[ParamSpec]:
    """The parameters of `table` (arch.param_table) the regular expressions select (re.search on the parameter name), in table order.
    Muon takes 2-D nn.Linear weights and the 3-D expert tensors [experts, rows, cols] whose matrix dimensions are multiples of 64.  A
    pattern that matches nothing, or matches anything else (a buffer, the conv-shaped patch embedding, a bias, a norm weight), raises
    ValueError."""
    if isinstance(targets, str) or not targets:
        raise ValueError(f"muon: targets must be a non-empty list of regular expressions, got {targets!r}")
    pats = [re.compile(t) for t in targets]
    hit = [False] * len(pats)
    out = []
    for spec in table:
        which = [i for i, p in enumerate(pats) if p.search(spec.name)]
        if not which:
            continue
        for i in which:
            hit[i] = True
        linear = spec.ctor == "linear_w" and len(spec.shape) == 2
        experts = spec.ctor == "ones" and len(spec.shape) == 3
        if spec.buffer or not (linear or experts):
            raise ValueError(f"muon: target {targets[which[0]]!r} matches {spec.name} {tuple(spec.shape)} ({spec.ctor}"
                             f"{', a buffer' if spec.buffer else ''}): only 2-D linear weights and 3-D expert tensors are orthogonalised")
        r, c = spec.shape[-2:]
        if r % DIM_MULTIPLE or c % DIM_MULTIPLE:
            raise ValueError(f"muon: {spec.name} is {r} x {c}: both matrix dimensions must be multiples of {DIM_MULTIPLE}")
        out.append(spec)
    for t, h in zip(targets, hit):
        if not h:
            raise ValueError(f"muon: target {t!r} matches no parameter")
    return out


def matrices_of(specs: Sequence[ParamSpec], offs: Dict[str, int]) -> List[Tuple[int, int, int, str]]:
    """[(flat_off, rows, cols, name)] in flat order: one entry per matrix, every expert of a 3-D tensor its own."""
    out = []
    for s in specs:
        r, c = s.shape[-2:]
        for e in range(s.shape[0] if len(s.shape) == 3 else 1):
            out.append((offs[s.name] + e * r * c, r, c, s.name))
    return sorted(out)


def complement_runs(specs: Sequence[ParamSpec], offs: Dict[str, int], total: int) -> List[Tuple[int, int]]:
    """[(off, n)]: the maximal runs of [0, total) no targeted tensor covers -- what stays with AdamW, alignment padding included (zeros
    in every buffer: AdamW leaves them zero).  Adjacent targets leave no run between them."""
    spans = sorted((offs[s.name], offs[s.name] + int(np.prod(s.shape))) for s in specs)
    runs, at = [], 0
    for lo, hi in spans:
        if lo < at:
            raise ValueError("muon: targeted tensors overlap in the flat layout")
        if lo > at:
            runs.append((at, lo - at))
        at = hi
    if at < total:
        runs.append((at, total - at))
    return runs


def check_hyper(momentum, nesterov, ns_steps, adjust, adamw_lr=None) -> None:
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0.0 <= momentum < 1.0:
        raise ValueError(f"muon: momentum must be a number in [0, 1), got {momentum!r}")
    if not isinstance(nesterov, bool):
        raise ValueError(f"muon: nesterov must be true or false, got {nesterov!r}")
    if isinstance(ns_steps, bool) or not isinstance(ns_steps, int) or not 1 <= ns_steps <= NS_STEPS_MAX:
        raise ValueError(f"muon: ns_steps must be an integer in 1 .. {NS_STEPS_MAX}, got {ns_steps!r}")
    if adjust not in ADJUSTS:
        raise ValueError(f"muon: adjust must be one of {ADJUSTS}, got {adjust!r}")
    if adamw_lr is not None and (isinstance(adamw_lr, bool) or not isinstance(adamw_lr, (int, float)) or not adamw_lr >= 0
                                 or adamw_lr == float("inf")):
        raise ValueError(f"muon: adamw_lr must be a non-negative number, got {adamw_lr!r}")


class Muon(FusedAdamW):
    """Muon on the targeted matrices, FusedAdamW on everything else, on the DiT's flat buffers.  One step (same signature as
    FusedAdamW.step): norm / clip / guard over the WHOLE gradient exactly as FusedAdamW does, md_muon_momentum (two launches over the
    item table), md_adamw_step once per complement run, md_muon_newton_schulz (a C loop over md_gemm_bf16 and the axpby kernel), md_muon_apply (one launch),
    the post-hoc EMA pass over the whole buffer.  Refused: the sharded optimiser (a rank owns slices of buckets, not whole matrices)
    and a DiT with a LoRA adapter attached."""

    shardable = False       # read by the Trainer: dp_mode "auto" resolves to "allreduce", an explicit "sharded" raises

    def __init__(self, dit, lr: float = 2.4e-4, momentum: float = 0.95, nesterov: bool = True, ns_steps: int = 5, adjust: str = "rms",
                 targets: Sequence[str] = DEFAULT_TARGETS, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.1,
                 adamw_lr: Optional[float] = None, ema_smoothing: Optional[float] = None, ema_start: int = 0, skip_nonfinite: bool = False,
                 posthoc_sigma_rels=None, device="cuda"):
        """lr / weight_decay: of the Muon part and, with adamw_lr=None, of the AdamW part too (adjust="rms" gives both updates the same
        RMS).  adamw_lr: base learning rate of the AdamW part; a per-step `lr` passed to step() scales both by the same factor."""
        from .dit import flat_layout
        # every refusal comes before anything is allocated or changed
        check_hyper(momentum, nesterov, ns_steps, adjust, adamw_lr)
        self.dit = dit
        self._refuse_adapter()
        self.targets = [str(t) for t in targets] if not isinstance(targets, str) else targets
        self.specs = resolve_targets(dit._table, self.targets)
        self._offs, self._total = flat_layout(dit._table)
        self.matrices = matrices_of(self.specs, self._offs)
        self.runs = complement_runs(self.specs, self._offs, self._total)
        self.momentum, self.nesterov, self.ns_steps, self.adjust = float(momentum), bool(nesterov), int(ns_steps), adjust
        self.ns_coeffs = NS_COEFFS
        self.adamw_lr = None if adamw_lr is None else float(adamw_lr)
        targeted = {s.name for s in self.specs}
        self.rules = {s.name: ("muon" if s.name in targeted else "adamw") for s in dit._table if not s.buffer}
        self.device = torch.device(device)
        self._items_host = self._items_dev = self._ws = self._partials = self.norms = None
        self.ws_bytes = 0
        self.last_gemm_launches = 0
        # device="cpu": the state only -- what state_dict() / load_state_dict() touch
        super().__init__(dit, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, ema_smoothing=ema_smoothing, ema_start=ema_start,
                         skip_nonfinite=skip_nonfinite, posthoc_sigma_rels=posthoc_sigma_rels,
                         device=None if self.device.type == "cuda" else self.device)

    # -------------------------------------------------------------------------------------------- the item table
    def item_scale(self, rows: int, cols: int) -> float:
        """md_muon_item.scale: the shape factor of the update."""
        return shape_scale(self.adjust, rows, cols)

    def _items(self):
        """(host array, device tensor, n): built on first use; md_muon_ws_bytes checks the shapes and writes the workspace offsets."""
        if self._items_host is None:
            rows = self.matrices
            arr = (hip.MuonItem * len(rows))(*[hip.MuonItem(o, r, c, 0, self.item_scale(r, c), 0) for o, r, c, _ in rows])
            need = c_int64(0)
            hip.check(hip.lib().md_muon_ws_bytes(arr, len(rows), byref(need)), "md_muon_ws_bytes")
            dev = self.m.device
            self._items_host, self.ws_bytes = arr, int(need.value)
            self._items_dev = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(dev)
            self._ws = torch.zeros(self.ws_bytes, device=dev, dtype=torch.uint8)
            self._partials = torch.zeros(len(rows) * hip.MUON_NORM_PARTS, device=dev, dtype=torch.float64)
            self.norms = torch.zeros(len(rows), device=dev, dtype=torch.float64)        # ||u||_F^2 of the last step, per matrix
        return self._items_host, self._items_dev, len(self.matrices)

    # -------------------------------------------------------------------------------------------- the step
    def _refuse_adapter(self) -> None:
        if getattr(self.dit, "_lora", None) is not None:
            raise NotImplementedError("Muon on a DiT with a LoRA adapter attached: the adapter assumes a frozen base; fuse() / detach() it first")

    def step(self, lr: Optional[float] = None, max_norm: float = 0.0, grad_scale: float = 1.0, g_bf16: Optional[torch.Tensor] = None,
             norm_partials: int = 0) -> None:
        self._refuse_adapter()
        if self.device.type != "cuda":
            raise RuntimeError("muon: step() needs the optimiser on the GPU (HIP kernels; there is no CPU fallback)")
        f = self.dit.flat_buffers()
        L, st = hip.lib(), hip.stream_ptr()
        host, dev, n = self._items()
        ema_mode = self._begin_step(grad_scale)
        ss = self._norm_and_guard(max_norm, src=g_bf16 if g_bf16 is not None else f["g"], src_is_bf16=g_bf16 is not None, n=f["total"],
                                  have=norm_partials)                    # the whole gradient, as FusedAdamW.step
        lr_muon = self.lr if lr is None else lr
        lr_adamw = lr_muon if self.adamw_lr is None else (self.adamw_lr * (lr_muon / self.lr) if self.lr else 0.0)
        guard = self.guard_state.data_ptr() if self.skip_nonfinite else None
        gb = g_bf16.data_ptr() if g_bf16 is not None else None
        a, b, c = self.ns_coeffs
        hip.check(L.md_muon_momentum(f["g"].data_ptr(), gb, self.m.data_ptr(), dev.data_ptr(), host, n, self.momentum, int(self.nesterov),
                                     grad_scale, ss, max_norm or 0.0, 1, guard, self._ws.data_ptr(), self._partials.data_ptr(),
                                     self.norms.data_ptr(), st), "md_muon_momentum")
        for off, cnt in self.runs:                                       # the unchanged AdamW pass on everything else
            self._launch(off, cnt, lr_adamw, max_norm, grad_scale, ss, (gb + 2 * off) if gb is not None else None,
                         f["s"].data_ptr() + 2 * off, 1, ema_mode)
        launches = c_int32(0)
        hip.check(L.md_muon_newton_schulz(host, n, self.ns_steps, a, b, c, self._ws.data_ptr(), byref(launches), st), "md_muon_newton_schulz")
        self.last_gemm_launches = int(launches.value)
        hip.check(L.md_muon_apply(f["p"].data_ptr(), f["s"].data_ptr(), self.ema.data_ptr() if self.ema is not None else None, dev.data_ptr(),
                                  host, n, lr_muon, self.weight_decay, ema_mode, self.ema_smoothing or 0.0, guard, self._ws.data_ptr(),
                                  st), "md_muon_apply")
        if self.posthoc:
            self._posthoc_update(0, f["total"])
        self.dit.mark_shadow_fresh()

    def step_sharded(self, *args, **kwargs) -> None:
        raise NotImplementedError("Muon under the sharded optimiser: a rank owns slices of buckets, not whole matrices (a distributed "
                                  "Newton-Schulz is a follow-up); use dp_mode='allreduce'")

    # -------------------------------------------------------------------------------------------- state
    def hyper(self) -> dict:
        return {"momentum": self.momentum, "nesterov": self.nesterov, "ns_steps": self.ns_steps, "adjust": self.adjust,
                "ns_coeffs": list(self.ns_coeffs)}

    def state_dict(self):
        """FusedAdamW's by-name layout (on a targeted tensor `m` is the Muon momentum and `v` is zero) plus one entry, "muon": the rule
        of every tensor and the Muon hyper-parameters."""
        sd = super().state_dict()
        sd["muon"] = {"rules": dict(self.rules), **self.hyper()}
        return sd

    def load_state_dict(self, sd):
        mu = sd.get("muon") if isinstance(sd, dict) else None
        if mu is None:
            raise RuntimeError("muon: the optimizer state carries no rule table (a plain FusedAdamW checkpoint): its moments of the "
                               "targeted tensors are AdamW's, not a Muon momentum")
        if dict(mu["rules"]) != self.rules:
            diff = sorted(k for k in set(mu["rules"]) | set(self.rules) if mu["rules"].get(k) != self.rules.get(k))
            raise RuntimeError(f"muon: the checkpoint's rule table differs from this optimizer's on {len(diff)} tensors: {diff[:4]} ...")
        mine = self.hyper()
        other = {k: mu.get(k) for k in mine}
        if other != mine:
            warnings.warn(f"muon: the checkpoint was written with {other}, this run uses {mine}: the momentum continues under the new values")
        super().load_state_dict(sd)
