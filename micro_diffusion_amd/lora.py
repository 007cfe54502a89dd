"""LoRA fine-tuning (opt-in): low-rank adapters trained on a frozen base (Hu et al. 2021, "LoRA: Low-Rank Adaptation of
Large Language Models").  No reference counterpart: the reference fine-tunes every weight.

The engine reads the weights from the flat bf16 shadow only, and the flat fp32 gradient accumulator is read once per step, so LoRA needs
no change to the forward / backward launch sequences.  For a targeted matrix W [N, K] with A [r, K], B [N, r], scale = alpha / r:

    shadow_W = bf16(p_W + scale * B A)                     md_lora_merge, behind every writer of the shadow
    dB       = c * G_W A^T,   dA = c * B^T G_W             md_lora_grad, once per step from the accumulated gradient G_W = g_W

with c = scale * grad_scale: the chain rule through W_eff = W + scale * B A, exact, and linear in G -- so it is applied to the sum over
the microbatches.  The masters p never change.  LoRAAdamW is what the Trainer steps in place of FusedAdamW: projection, clear of g,
norm / guard, AdamW on the adapter's few million values, merge.  The `ref_*` functions restate the two formulas in fp64 torch for the
tests.

`backward="factored"` (opt-in; the default "projected" is the above) never forms G_W: the engine's backward(param_grads="lora") hands
every targeted linear's dy [M, N] and saved input x [M, K] to md_lora_wgrad, which adds

    dB += c * dy^T (x A^T),   dA += c * (dy B)^T x          c = scale

into the adapter's gradient buffer per microbatch (the same chain rule, linear in the microbatch); no other parameter gradient is
launched, the base's accumulator is neither written nor cleared, and what a data-parallel step exchanges is the adapter's gradient: one
fp32 all-reduce (Trainer).  `device="cpu"` holds the state only (target resolution, state_dict round trips); the kernels need a GPU."""
from __future__ import annotations

import math
import re
from ctypes import byref, c_int64
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import hip
from .arch import ParamSpec
from .optim import Optimizer

RANKS = (4, 8, 16, 32, 64)                   # what md_lora_merge / md_lora_grad / md_lora_wgrad accept
BACKWARDS = ("projected", "factored")        # how the adapter's gradient is formed ("Factored backward")
# the five attention projections of every mixer and backbone block (not the caption block's: y_emb_preprocess.attn.*)
DEFAULT_TARGETS = tuple(r"^(patch_mixer|blocks)\.\d+\." + m + r"\.weight$"
                        for m in (r"attn\.qkv", r"attn\.proj", r"cross_attn\.q_linear", r"cross_attn\.kv_linear", r"cross_attn\.proj"))
_ALIGN = 8                                   # elements: every A / B starts 32-byte aligned inside the adapter's flat buffer


def check_rank(rank) -> int:
    if isinstance(rank, bool) or not isinstance(rank, int) or rank not in RANKS:
        raise ValueError(f"lora: rank must be one of {RANKS}, got {rank!r}")
    return rank


def resolve_targets(table: Sequence[ParamSpec], targets: Sequence[str]) -> List[ParamSpec]:
    """The parameters of `table` (arch.param_table) the regular expressions select (re.search on the parameter name), in table order.
    Only 2-D nn.Linear weights with a row length that is a multiple of 8 can carry an adapter: a pattern that matches nothing, or matches
    anything else (the 3-D expert tensors of the MoE blocks, the conv-shaped patch embedding, biases, norm weights), raises ValueError."""
    if isinstance(targets, str) or not targets:
        raise ValueError(f"lora: targets must be a non-empty list of regular expressions, got {targets!r}")
    pats = [re.compile(t) for t in targets]
    hit = [False] * len(pats)
    out = []
    for spec in table:
        which = [i for i, p in enumerate(pats) if p.search(spec.name)]
        if not which:
            continue
        for i in which:
            hit[i] = True
        if spec.buffer or spec.ctor != "linear_w" or len(spec.shape) != 2:
            raise ValueError(f"lora: target {targets[which[0]]!r} matches {spec.name} {tuple(spec.shape)} ({spec.ctor}): only 2-D linear "
                             "weights can carry an adapter")
        if spec.shape[1] % 8:
            raise ValueError(f"lora: {spec.name} has rows of {spec.shape[1]} elements, not a multiple of 8")
        out.append(spec)
    for t, h in zip(targets, hit):
        if not h:
            raise ValueError(f"lora: target {t!r} matches no parameter")
    return out


def adapter_layout(specs: Sequence[ParamSpec], rank: int):
    """({name: (a_off, b_off)}, total) inside the adapter's flat fp32 buffer: A [rank, K] then B [N, rank] of every target, in table
    order, each start padded to _ALIGN elements (the padding stays zero: AdamW without a gradient leaves zeros alone)."""
    offs, total = {}, 0
    pad = lambda n: (n + _ALIGN - 1) // _ALIGN * _ALIGN
    for s in specs:
        n, k = s.shape
        a = total
        b = a + pad(rank * k)
        total = b + pad(n * rank)
        offs[s.name] = (a, b)
    return offs, total


def module_name(param: str) -> str:
    return param[:-len(".weight")] if param.endswith(".weight") else param


# ------------------------------------------------------------------------------------------------ fp64 restatement (the reference)
def ref_merge(p, A, B, scale: float):
    """p + scale * B A in fp64 from the fp32 (or any) values."""
    return p.double() + float(scale) * (B.double() @ A.double())


def ref_grad(G, A, B, scale: float, grad_scale: float = 1.0):
    """(dA [r, K], dB [N, r]) in fp64: the gradient of <grad_scale * G, W + scale * B A> with respect to A and B."""
    c = float(scale) * float(grad_scale)
    return c * (B.double().t() @ G.double()), c * (G.double() @ A.double().t())


def ref_wgrad_factored(dy, x, A, B, c: float):
    """(dA [r, K], dB [N, r]) in fp64 from one linear's dy [M, N] and x [M, K]: c * (dy B)^T x and c * dy^T (x A^T) -- ref_grad of
    G = dy^T x, without G."""
    dy, x, A, B = dy.double(), x.double(), A.double(), B.double()
    return float(c) * ((dy @ B).t() @ x), float(c) * (dy.t() @ (x @ A.t()))


def check_backward(backward) -> str:
    if backward not in BACKWARDS:
        raise ValueError(f"lora: backward must be one of {BACKWARDS}, got {backward!r}")
    return backward


class LoRA:
    """Adapters for the targeted matrices of one DiT: one flat fp32 buffer `w` for every A / B, one of the same layout `g` for their
    gradients, and the item table of the two kernels (a host copy and a device copy).  A is drawn on the CPU from `seed`
    (kaiming_uniform_(a=sqrt 5) per target, in table order: identical on every device), B = 0: a fresh adapter leaves the weights alone."""

    def __init__(self, dit, rank: int = 16, alpha: Optional[float] = None, targets: Sequence[str] = DEFAULT_TARGETS, seed: int = 0,
                 device="cuda", backward: str = "projected"):
        from .dit import flat_layout
        self.dit = dit
        self.rank = check_rank(rank)
        self.backward = check_backward(backward)     # not part of state_dict(): an adapter file loads into either mode
        if alpha is not None and not (isinstance(alpha, (int, float)) and not isinstance(alpha, bool) and math.isfinite(alpha)):
            raise ValueError(f"lora: alpha must be a finite number, got {alpha!r}")
        self.alpha = float(rank if alpha is None else alpha)
        self.targets = [str(t) for t in targets]
        self.seed = int(seed)
        self.specs = resolve_targets(dit._table, self.targets)
        self.names = [s.name for s in self.specs]
        self.offs, self.total = adapter_layout(self.specs, self.rank)
        self.flat_offs = flat_layout(dit._table)[0]
        self.device = torch.device(device)
        self._scale = self.alpha / self.rank
        self._enabled = True
        self.attached = False
        w = torch.zeros(self.total, dtype=torch.float32)
        gen = torch.Generator(device="cpu").manual_seed(self.seed)
        for s in self.specs:
            a = torch.empty(self.rank, s.shape[1], dtype=torch.float32)
            torch.nn.init.kaiming_uniform_(a, a=math.sqrt(5), generator=gen)
            o = self.offs[s.name][0]
            w[o:o + a.numel()] = a.reshape(-1)
        self.w = w.to(self.device)
        self.g = torch.zeros_like(self.w)
        self._items_host = None
        self._items_dev = None
        self._ws = None
        self.ws_floats = 0
        self._shape_of = {s.name: (int(s.shape[0]), int(s.shape[1])) for s in self.specs}
        self._wgrad_ws = None                        # factored backward: the workspace of md_lora_wgrad, grown on demand
        self._wgrad_need = {}                        # (M, N, K) -> md_lora_wgrad_ws_floats

    # -------------------------------------------------------------------------------------------- views
    def A(self, name: str) -> torch.Tensor:
        s = self._spec(name)
        o = self.offs[name][0]
        return self.w[o:o + self.rank * s.shape[1]].view(self.rank, s.shape[1])

    def B(self, name: str) -> torch.Tensor:
        s = self._spec(name)
        o = self.offs[name][1]
        return self.w[o:o + s.shape[0] * self.rank].view(s.shape[0], self.rank)

    def dA(self, name: str) -> torch.Tensor:
        s = self._spec(name)
        o = self.offs[name][0]
        return self.g[o:o + self.rank * s.shape[1]].view(self.rank, s.shape[1])

    def dB(self, name: str) -> torch.Tensor:
        s = self._spec(name)
        o = self.offs[name][1]
        return self.g[o:o + s.shape[0] * self.rank].view(s.shape[0], self.rank)

    def _spec(self, name: str) -> ParamSpec:
        for s in self.specs:
            if s.name == name:
                return s
        raise KeyError(f"lora: {name} is not a target")

    # -------------------------------------------------------------------------------------------- the item table
    def item_rows(self) -> List[tuple]:
        """[(w_off, a_off, b_off, rows, cols)] per target, in table order: what the item table holds (offsets in elements)."""
        return [(self.flat_offs[s.name], *self.offs[s.name], s.shape[0], s.shape[1]) for s in self.specs]

    def _items(self):
        """(host array, device tensor, n): built on first use; md_lora_grad_ws_floats checks the shapes and writes the workspace offsets."""
        if self._items_host is None:
            rows = self.item_rows()
            arr = (hip.LoraItem * len(rows))(*[hip.LoraItem(w, a, b, 0, n, k) for w, a, b, n, k in rows])
            need = c_int64(0)
            hip.check(hip.lib().md_lora_grad_ws_floats(arr, len(rows), self.rank, byref(need)), "md_lora_grad_ws_floats")
            self._items_host, self.ws_floats = arr, int(need.value)
            raw = np.frombuffer(arr, dtype=np.uint8).copy()
            self._items_dev = torch.from_numpy(raw).to(self.w.device)
        return self._items_host, self._items_dev, len(self.specs)

    # -------------------------------------------------------------------------------------------- HIP
    def _flat(self) -> dict:
        """The DiT's flat buffers without DiT.flat_buffers()' walk over the parameters (host time on the step path)."""
        f = self.dit._flat
        return f if f is not None else self.dit.flat_buffers()

    def merge_into(self, out: torch.Tensor, out_is_f32: bool) -> None:
        """md_lora_merge from the DiT's masters into `out` (the flat bf16 shadow, or a flat fp32 buffer: the masters themselves in fuse())."""
        host, dev, n = self._items()
        f = self._flat()
        hip.check(hip.lib().md_lora_merge(f["p"].data_ptr(), self.w.data_ptr(), dev.data_ptr(), host, n, self.rank, float(self._scale),
                                          out.data_ptr(), 1 if out_is_f32 else 0, hip.stream_ptr()), "md_lora_merge")

    def project_grad(self, grad_scale: float = 1.0) -> None:
        """md_lora_grad: g += (dA, dB) of every target from the DiT's accumulated flat gradient."""
        host, dev, n = self._items()
        if self._ws is None:
            self._ws = torch.empty(max(self.ws_floats, 4), device=self.w.device, dtype=torch.float32)
        f = self._flat()
        hip.check(hip.lib().md_lora_grad(f["g"].data_ptr(), self.w.data_ptr(), dev.data_ptr(), host, n, self.rank, float(self._scale),
                                         float(grad_scale), self.g.data_ptr(), self._ws.data_ptr(), self._ws.numel(), hip.stream_ptr()),
                  "md_lora_grad")

    @property
    def factored(self) -> bool:
        """The adapter's gradient comes from the engine's backward(param_grads="lora"), not from the base's accumulated gradient."""
        return self.backward == "factored" and self.active

    def is_target(self, name: str) -> bool:
        return name in self._shape_of

    def _wgrad_floats(self, M: int, N: int, K: int) -> int:
        key = (M, N, K)
        if key not in self._wgrad_need:
            need = c_int64(0)
            hip.check(hip.lib().md_lora_wgrad_ws_floats(M, N, K, self.rank, byref(need)), "md_lora_wgrad_ws_floats")
            self._wgrad_need[key] = int(need.value)
        return self._wgrad_need[key]

    def wgrad_workspace(self, M: int) -> torch.Tensor:
        """The workspace of md_lora_wgrad: the maximum over the targets at the largest M seen so far (the adapter's own buffer, not the
        engine's split-K workspace: it lives across the launches of one call only, but its size follows the adapter's targets)."""
        need = max(self._wgrad_floats(M, n, k) for n, k in set(self._shape_of.values()))
        if self._wgrad_ws is None or self._wgrad_ws.numel() < need:
            self._wgrad_ws = torch.empty(need, device=self.w.device, dtype=torch.float32)
        return self._wgrad_ws

    def wgrad(self, name: str, dy_ptr: int, lddy: int, x_ptr: int, ldx: int, M: int, c: Optional[float] = None) -> None:
        """md_lora_wgrad: g += (dA, dB) of target `name` from one linear's dy [M, N] / x [M, K] (device addresses of bf16 rows,
        column offsets included); c defaults to the adapter's scale."""
        N, K = self._shape_of[name]
        ws = self.wgrad_workspace(M)
        a, b = self.offs[name]
        hip.check(hip.lib().md_lora_wgrad(dy_ptr, lddy, x_ptr, ldx, M, N, K, self.w.data_ptr() + 4 * a, self.w.data_ptr() + 4 * b,
                                          self.rank, float(self._scale if c is None else c), self.g.data_ptr() + 4 * a,
                                          self.g.data_ptr() + 4 * b, ws.data_ptr(), ws.numel(), hip.stream_ptr()), "md_lora_wgrad")

    @property
    def active(self) -> bool:
        """Whether the shadow carries the adapter: attached, enabled and scale != 0 (otherwise the shadow is the plain bf16(p))."""
        return self.attached and self._enabled and self._scale != 0.0

    def apply_to_shadow(self) -> None:
        """Called by DiT.refresh_shadow behind the cast (and by LoRAAdamW.step): the targeted part of the shadow := bf16(p + scale B A)."""
        if self.active:
            self.merge_into(self._flat()["s"], False)

    # -------------------------------------------------------------------------------------------- attach / detach / fuse
    def attach(self) -> "LoRA":
        if getattr(self.dit, "_lora", None) not in (None, self):
            raise RuntimeError("lora: the DiT already has another adapter attached; detach() it first")
        if self.w.device.type != "cuda":
            raise RuntimeError("lora: attach() needs the adapter on the GPU (the merge is a HIP kernel; there is no CPU fallback)")
        self.dit._ensure_flat()
        self.dit._lora = self
        self.dit._engine.lora = self
        self.attached = True
        self.dit.refresh_shadow(force=True)
        return self

    def detach(self) -> None:
        if self.attached:
            self.dit._lora = None
            if self.dit._engine is not None:
                self.dit._engine.lora = None
            self.attached = False
            self.dit.refresh_shadow(force=True)

    @property
    def scale(self) -> float:
        return self._scale

    @scale.setter
    def scale(self, v: float) -> None:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"lora: scale must be a finite number, got {v!r}")
        self._scale = float(v)
        if self.attached:
            self.dit.refresh_shadow(force=True)

    @property
    def enabled(self) -> bool:
        return self._enabled

    @enabled.setter
    def enabled(self, v: bool) -> None:
        self._enabled = bool(v)
        if self.attached:
            self.dit.refresh_shadow(force=True)

    def fuse(self) -> None:
        """p_W := p_W + scale * B A in fp32 (md_lora_merge onto the masters), then detach: dit.state_dict() is a plain checkpoint.  The
        bf16 shadow afterwards holds the bits it held with the adapter attached (the bf16 merge rounds exactly what this stores)."""
        if not self.attached:
            raise RuntimeError("lora: fuse() needs an attached adapter")
        if self._enabled and self._scale != 0.0:
            self.merge_into(self.dit.flat_buffers()["p"], True)
        self.detach()

    # -------------------------------------------------------------------------------------------- host side
    def state_dict(self) -> dict:
        """`<module>.lora_A.weight` [r, K] / `<module>.lora_B.weight` [N, r] (the common adapter layout), and rank / alpha / targets."""
        sd: Dict[str, object] = {"rank": self.rank, "alpha": self.alpha, "targets": list(self.targets), "seed": self.seed}
        for s in self.specs:
            m = module_name(s.name)
            sd[m + ".lora_A.weight"] = self.A(s.name).clone()
            sd[m + ".lora_B.weight"] = self.B(s.name).clone()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        if int(sd["rank"]) != self.rank:
            raise RuntimeError(f"the adapter file has rank {int(sd['rank'])}, this adapter {self.rank}")
        want = {module_name(s.name) + k: sh for s in self.specs
                for k, sh in ((".lora_A.weight", (self.rank, s.shape[1])), (".lora_B.weight", (s.shape[0], self.rank)))}
        have = {k for k in sd if k.endswith((".lora_A.weight", ".lora_B.weight"))}
        if have != set(want):
            raise RuntimeError(f"the adapter file's tensors do not match this adapter's targets: {sorted(have ^ set(want))[:6]} ...")
        for k, sh in want.items():
            if tuple(sd[k].shape) != sh:
                raise RuntimeError(f"{k}: the adapter file holds {tuple(sd[k].shape)}, this model needs {sh}")
        for s in self.specs:
            m = module_name(s.name)
            self.A(s.name).copy_(sd[m + ".lora_A.weight"])
            self.B(s.name).copy_(sd[m + ".lora_B.weight"])
        self.alpha = float(sd.get("alpha", self.alpha))
        self._scale = self.alpha / self.rank
        self.g.zero_()
        if self.attached:
            self.dit.refresh_shadow(force=True)

    @classmethod
    def from_state_dict(cls, dit, sd: dict, device="cuda", backward: str = "projected") -> "LoRA":
        """An adapter built from a file (state_dict()): LoRA.from_state_dict(model.dit, torch.load(path)).attach()."""
        ad = cls(dit, rank=int(sd["rank"]), alpha=float(sd["alpha"]), targets=list(sd["targets"]), seed=int(sd.get("seed", 0)),
                 device=device, backward=backward)
        ad.load_state_dict(sd)
        return ad


class LoRAAdamW(Optimizer):
    """What the Trainer steps in place of FusedAdamW when an adapter is trained: AdamW on the adapter's flat buffer alone.  No buffer of
    the base's size is allocated (no base moments, EMA or post-hoc averages); the gradient norm that is clipped and guarded is the
    adapter's, since the base is frozen.  A NaN / Inf in the gradient of a targeted matrix reaches the adapter's gradient through the
    projection, so `skip_nonfinite` guards the step as it does for FusedAdamW: the adapter and its moments stay untouched bit for bit,
    both accumulators are still cleared, the step is counted.
    With a factored adapter (LoRA(backward="factored")) the adapter's gradient is already in adapter.g when step() runs: no projection
    and no clear of the base's accumulator (nothing wrote it); grad_scale goes into the AdamW launch, which also scales the norm it
    clips by and clears adapter.g -- on a guarded skipped step too."""

    def __init__(self, adapter: LoRA, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 skip_nonfinite: bool = False):
        self.adapter, self.dit = adapter, adapter.dit
        if not adapter.attached:
            adapter.attach()
        super().__init__(adapter.w.device, lr, betas, eps, weight_decay, skip_nonfinite)
        self.m = torch.zeros_like(adapter.w)
        self.v = torch.zeros_like(adapter.w)
        self._norm_unscaled = False                # the last step's sumsq was taken before grad_scale (the factored step)

    def state_buffers(self) -> list:
        return [self.m, self.v]

    def grad_norm(self) -> torch.Tensor:
        """||g||_2 of the adapter's gradient of the last step before clipping (valid after step() with max_norm > 0 or skip_nonfinite)."""
        n = self.sumsq.sqrt().reshape(())
        return n * self.last_grad_scale if self._norm_unscaled else n

    def step(self, lr: Optional[float] = None, max_norm: float = 0.0, grad_scale: float = 1.0, g_bf16: Optional[torch.Tensor] = None,
             norm_partials: int = 0) -> None:
        if g_bf16 is not None or norm_partials > 0:
            raise NotImplementedError("LoRAAdamW steps from the adapter's own gradient, not from an exchanged gradient buffer: the "
                                      "projected backward exchanges nothing, data parallelism needs LoRA(backward='factored'), which "
                                      "all-reduces the adapter's gradient")
        ad = self.adapter
        if not ad.attached or self.dit._lora is not ad:
            raise RuntimeError("LoRAAdamW.step: the adapter is not attached to its DiT")
        f = ad._flat()
        self.step_count += 1
        self.last_grad_scale = grad_scale
        factored = ad.backward == "factored"
        self._norm_unscaled = factored
        if not factored:
            ad.project_grad(grad_scale)                                                       # 1. dA, dB from the accumulated G
            hip.check(hip.lib().md_fill_zero(f["g"].data_ptr(), 4 * f["total"], hip.stream_ptr()), "md_fill_zero")  # 2. clear the accumulator
        ss = self._norm_and_guard(max_norm, src=ad.g, n=ad.total)                             # 3. the adapter's gradient norm, 4. the go flag
        # 5. AdamW on the adapter (grad_scale went into the projection -- factored: into this launch, which scales the norm it clips
        #    by with it; no shadow: the merge below writes it); zero_grad clears adapter.g, on a guarded skipped step too
        hip.adamw_step(ad.w, ad.g, self.m, self.v, ad.total, lr=float(self.lr if lr is None else lr), betas=self.betas, eps=self.eps,
                       weight_decay=self.weight_decay, step=self.step_count, sumsq=ss, max_norm=max_norm,
                       grad_scale=float(grad_scale) if factored else 1.0, guard=self.guard_state)
        ad.apply_to_shadow()                                                                  # 6. shadow_W = bf16(p_W + scale B A)
        self.dit.mark_shadow_fresh()                                                          # 7.

    def state_dict(self) -> dict:
        return {"m": self.m.clone(), "v": self.v.clone(), "step": self.step_count,
                "skipped": self.guard_state.clone() if self.guard_state is not None else None}

    def load_state_dict(self, sd: dict) -> None:
        if tuple(sd["m"].shape) != tuple(self.m.shape):
            raise RuntimeError(f"the optimiser state holds {tuple(sd['m'].shape)} moments, this adapter has {tuple(self.m.shape)}")
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.step_count = int(sd["step"])
        if self.guard_state is not None and sd.get("skipped") is not None:
            self.guard_state.copy_(sd["skipped"])


def allocated_floats(opt: LoRAAdamW) -> int:
    """fp32 elements the adapter and its optimiser hold (weights, gradients, moments, workspace, norm partials)."""
    ad = opt.adapter
    ad._items()
    wgrad = 0 if ad._wgrad_ws is None else ad._wgrad_ws.numel()          # the factored backward's workspace, once a backward has run
    return 2 * ad.total + 2 * opt.m.numel() + max(ad.ws_floats, 4) + wgrad + opt.partials.numel() + 1
