"""The optimisers the Trainer steps: what it may read of any of them (Optimizer) and the fused AdamW on the DiT's flat buffers
(FusedAdamW: torch.optim.AdamW + Composer's EMA + the post-hoc EMA profiles in one or two bandwidth passes).  muon.Muon derives from
FusedAdamW, lora.LoRAAdamW from Optimizer.  Every launch goes through hip.grad_sumsq / hip.adamw_step / hip.ema_power_update."""
from __future__ import annotations

import ctypes
import math
import warnings
from typing import Dict, Optional

import torch

from . import hip
from . import posthoc_ema


class Optimizer:
    """What the Trainer is entitled to read of an optimiser: the hyper-parameters, the step counter, the gradient-norm buffers and the
    step guard's state, and the hooks below.  A subclass provides step(lr, max_norm, grad_scale, g_bf16, norm_partials), grad_norm(),
    state_dict() / load_state_dict() and, when `shardable`, step_sharded()."""

    shardable = True        # runs under dp_mode="sharded" (a rank updates slices of buckets)
    adapter = None          # a lora.LoRA when the optimiser trains an adapter on a frozen base

    def __init__(self, device, lr: float, betas, eps: float, weight_decay: float, skip_nonfinite: bool, norm_slots: int = 1):
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.step_count = 0
        self.last_grad_scale = 1.0
        self.ema, self.posthoc = None, []          # the fixed-length EMA of the masters (a flat buffer) and the post-hoc EMA profiles
        self.sumsq = torch.zeros(1, device=device)
        self.partials = torch.zeros(norm_slots * hip.SUMSQ_PARTIALS, device=device)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guard_state = torch.zeros(4, device=device, dtype=torch.int32) if self.skip_nonfinite else None    # md_step_guard

    def skipped_steps(self) -> int:
        """Steps the device-side guard turned into a no-op so far (synchronises: the only host read of the guard)."""
        return int(self.guard_state[1].item()) if self.guard_state is not None else 0

    def ensure_norm_slots(self, n: int) -> None:
        """Room for `n` per-bucket partial sums of the exchanged gradient's norm; nothing to do for an optimiser that takes the norm
        itself."""

    def swap_ema(self, profile: Optional[int] = None):
        return None

    def ema_state_dict(self):
        return None

    def state_buffers(self) -> list:
        """The flat tensors Trainer.consolidate() gathers and Trainer.sync_replicas() broadcasts, next to the masters."""
        return []

    def _norm_and_guard(self, max_norm, src=None, src_is_bf16: bool = False, n: int = 0, have: int = 0, sharded=None) -> Optional[int]:
        """The squared gradient norm into self.sumsq, and the go flag from it under skip_nonfinite; returns the address of sumsq, or
        None when the step neither clips nor guards (nothing is launched).  `have` > 0: that many partial sums are already in
        self.partials (the exchange took them per bucket), else they are taken from the `n` elements of `src`.
        `sharded` = (GradSync, slots): the norm comes from the ranks' chunk norms instead."""
        if not ((max_norm and max_norm > 0) or self.skip_nonfinite):
            return None
        if sharded is not None:
            sharded[0].finish_sharded_norm(sharded[1], self.sumsq, guard=self.guard_state)
        else:
            hip.grad_sumsq(self.partials, self.sumsq, src=None if have > 0 else src, src_is_bf16=src_is_bf16, n=n,
                           count=have if have > 0 else hip.SUMSQ_PARTIALS, guard=self.guard_state)
        return self.sumsq.data_ptr()


class FusedAdamW(Optimizer):
    """torch.optim.AdamW semantics (train.py:39-43) on the DiT's flat buffers, one HIP kernel per step; optionally the
    EMA of the weights the res-512 configs name (configs/res_512_pretrain.yaml:4-9: smoothing 0.99975, every batch, from
    batch 25000 on) folded into the same pass."""

    MAX_BUCKETS = 64      # per-bucket partial sums of the gradient norm (data-parallel exchange), MD_SUMSQ_PARTIALS floats each

    def __init__(self, dit, lr: float = 2.4e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.1,
                 ema_smoothing: Optional[float] = None, ema_start: int = 0, skip_nonfinite: bool = False,
                 posthoc_sigma_rels=None, device=None):
        """`posthoc_sigma_rels`: a tuple of 1 .. 4 relative widths (e.g. (0.05, 0.10)) switches the post-hoc EMA on: one flat fp32
        buffer per value, each the size of the masters (4.66 GB per profile at XL/2), holds the power-function average with
        gamma = posthoc_ema.sigma_rel_to_gamma(value).  After the AdamW launch(es) of every step ONE md_ema_power_update pass reads
        the masters once and updates every profile with beta = (1 - 1/t)^(gamma + 1), t = step_count (computed on the host in
        fp64; t = 1 copies the weights).  Independent of `ema_smoothing`: both may be on.  With `skip_nonfinite` the pass takes the
        guard flag: a skipped step advances t and leaves the averages alone, the same convention as for the fixed-length EMA
        (ema_live / step_count advance, the average does not move).  None (default): no buffer, no launch, no state entry.
        `skip_nonfinite`: guard the step on the device.  The squared gradient norm is then taken on every step (also with
        max_norm == 0), md_step_guard derives a go flag from it and the AdamW pass runs in its guarded form: when the norm is not
        finite (a NaN or an Inf anywhere in the gradient) weights, moments and a live EMA stay untouched bit for bit, the
        accumulators are still zeroed and the bf16 weights re-emitted.  No host sync; skipped_steps() reads the device counter.
        A skipped step is a consumed batch with a zero update: the host-side step_count (bias corrections), the LR-schedule
        position (Trainer.batches_seen) and ema_live advance as on any other step.
        `device`: None = where the DiT's flat buffers live; a CPU device holds the state only (muon.Muon(device="cpu"))."""
        from .dit import flat_layout
        self.dit = dit
        self._refuse_adapter()
        self._offs, self._total = flat_layout(dit._table)
        if device is None:
            device = dit.flat_buffers()["p"].device
        super().__init__(device, lr, betas, eps, weight_decay, skip_nonfinite, norm_slots=self.MAX_BUCKETS)
        self.norm_slots = self.MAX_BUCKETS
        flat = lambda: torch.zeros(self._total, dtype=torch.float32, device=device)
        self.m, self.v = flat(), flat()
        self.ema_smoothing, self.ema_start = ema_smoothing, int(ema_start)
        self.ema = flat() if ema_smoothing is not None else None
        self.ema_live = False
        self.posthoc_sigma_rels = tuple(float(s) for s in (posthoc_sigma_rels or ()))
        if len(self.posthoc_sigma_rels) > hip.EMA_MAX_PROFILES:
            raise ValueError(f"at most {hip.EMA_MAX_PROFILES} post-hoc EMA profiles (MD_EMA_MAX_PROFILES), got {len(self.posthoc_sigma_rels)}")
        self.posthoc_gammas = tuple(posthoc_ema.sigma_rel_to_gamma(s) for s in self.posthoc_sigma_rels)
        self.posthoc = [flat() for _ in self.posthoc_sigma_rels]        # empty list: the feature is off
        self._range_key = self._range_off = self._range_cnt = None     # step_sharded's range table (ctypes), cached per plan

    def _refuse_adapter(self) -> None:
        """This pass emits the bf16 shadow itself and would overwrite a LoRA merge (and train the base the adapter assumes frozen)."""
        if getattr(self.dit, "_lora", None) is not None:
            raise RuntimeError("FusedAdamW on a DiT with a LoRA adapter attached: step the adapter with lora.LoRAAdamW, or fuse() / "
                               "detach() it first")

    def ensure_norm_slots(self, n: int) -> None:
        """Room for `n` per-bucket partial sums of the gradient norm (a model with more data-parallel buckets than MAX_BUCKETS:
        the sharded exchange has no other way to form ||g||)."""
        if n > self.norm_slots:
            self.partials = torch.zeros(n * hip.SUMSQ_PARTIALS, device=self.partials.device)
            self.norm_slots = n

    def state_buffers(self) -> list:
        return [self.m, self.v] + ([self.ema] if self.ema is not None else []) + list(self.posthoc)

    def _launch(self, off: int, n: int, lr: float, max_norm: float, grad_scale: float, ss, g_bf16_ptr, shadow_ptr, zero_grad: int,
                ema_mode: int, ranges=None) -> None:
        """AdamW on elements [off, off + n) of the flat buffers; the bf16 gradient / bf16 weight output may live elsewhere (the packed
        per-rank buffers of the sharded exchange).  `ranges`: one launch over a range table instead (hip.adamw_step)."""
        f = self.dit.flat_buffers()
        hip.adamw_step(f["p"].data_ptr() + 4 * off, f["g"].data_ptr() + 4 * off, self.m.data_ptr() + 4 * off, self.v.data_ptr() + 4 * off, n,
                       lr=lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, step=self.step_count, shadow=shadow_ptr,
                       sumsq=ss, g_bf16=g_bf16_ptr, ema=(self.ema.data_ptr() + 4 * off) if self.ema is not None else None,
                       ema_smoothing=self.ema_smoothing, max_norm=max_norm, grad_scale=grad_scale, zero_grad=zero_grad, ema_mode=ema_mode,
                       guard=self.guard_state, ranges=ranges)

    def _posthoc_update(self, off: int, n: int, flat_off=None, count=None) -> None:
        """md_ema_power_update on elements [off, off + n) of the masters and every profile, or (flat_off / count) its _ranges form
        over the whole buffers; beta of the step just taken."""
        betas = [posthoc_ema.power_beta(self.step_count, g) for g in self.posthoc_gammas]
        p = self.dit.flat_buffers()["p"]
        hip.ema_power_update(p.data_ptr() + 4 * off, [e.data_ptr() + 4 * off for e in self.posthoc], betas, n,
                             guard=self.guard_state, flat_off=flat_off, count=count)

    def _begin_step(self, grad_scale: float) -> int:
        self.step_count += 1
        self.last_grad_scale = grad_scale
        ema_mode = 0
        if self.ema is not None and self.step_count > self.ema_start:
            ema_mode = 2 if self.ema_live else 1          # first EMA batch: ema <- weights (the EMA model starts as a copy)
            self.ema_live = True
        return ema_mode

    def step(self, lr: Optional[float] = None, max_norm: float = 0.0, grad_scale: float = 1.0, g_bf16: Optional[torch.Tensor] = None,
             norm_partials: int = 0) -> None:
        """`g_bf16`: take the gradients from this bf16 flat buffer (data-parallel exchange buffer) instead of the fp32
        accumulators.  `norm_partials` > 0: that many per-bucket partial sums of squares are already in self.partials."""
        self._refuse_adapter()
        f = self.dit.flat_buffers()
        ema_mode = self._begin_step(grad_scale)
        ss = self._norm_and_guard(max_norm, src=g_bf16 if g_bf16 is not None else f["g"], src_is_bf16=g_bf16 is not None, n=f["total"],
                                  have=norm_partials)
        self._launch(0, f["total"], self.lr if lr is None else lr, max_norm, grad_scale, ss,
                     g_bf16.data_ptr() if g_bf16 is not None else None, f["s"].data_ptr(), 1, ema_mode)
        if self.posthoc:
            self._posthoc_update(0, f["total"])
        self.dit.mark_shadow_fresh()

    def step_sharded(self, sync, lr: Optional[float] = None, max_norm: float = 0.0, grad_scale: float = 1.0,
                     norm_slots: int = 0, chunk_of: Optional[int] = None) -> None:
        """The rank's share of the step under GradSync(mode='sharded'): ||g||^2 from the ranks' chunk norms (one scalar
        all-reduce), AdamW on this rank's chunk of every matrix-shaped bucket (gradient from the reduce-scattered bf16 buffer,
        fresh bf16 weights into the packed send buffer) and on the whole "small" region (every rank), then the asynchronous
        all-gather of the bf16 weights.  The fp32 accumulators were cleared by the staging cast.
        `chunk_of` (measurement aid, single rank): pretend to be one of `chunk_of` ranks — update only the first 1 / chunk_of of
        every bucket — to time the per-rank optimiser pass of an N-GPU run on one GPU; the model is NOT valid afterwards."""
        self._refuse_adapter()
        f = self.dit.flat_buffers()
        ema_mode = self._begin_step(grad_scale)
        lr = self.lr if lr is None else lr
        ss = self._norm_and_guard(max_norm, sharded=(sync, norm_slots))
        # ONE launch over the rank's chunks (md_adamw_step_ranges: the kernel walks the packed space the reduce-scattered gradient
        # and the send buffer live in, a range table maps it onto the flat masters / moments)
        ranges = [(lo + sync.rank * chunk, chunk if chunk_of is None else (hi - lo) // chunk_of // 64 * 64) for _, lo, hi, chunk, _ in sync.plan]
        ranges = [r for r in ranges if r[1] > 0]
        one_launch = len(ranges) <= hip.ADAMW_MAX_RANGES
        if one_launch:     # (with chunk_of the packed gradient / weight offsets no longer line up: timing only, as documented)
            if self._range_key != tuple(ranges):
                self._range_key = tuple(ranges)
                self._range_off = (ctypes.c_int64 * len(ranges))(*[r[0] for r in ranges])
                self._range_cnt = (ctypes.c_int64 * len(ranges))(*[r[1] for r in ranges])
            self._launch(0, 0, lr, max_norm, grad_scale, ss, sync.gred.data_ptr(), sync.ssend.data_ptr(), 0, ema_mode,
                         ranges=(self._range_off, self._range_cnt))
        else:                                   # more buckets than the kernel's table holds: chunk by chunk
            for _, lo, hi, chunk, olo in sync.plan:
                self._launch(lo + sync.rank * chunk, chunk, lr, max_norm, grad_scale, ss, sync.gred.data_ptr() + 2 * olo,
                             sync.ssend.data_ptr() + 2 * olo, 0, ema_mode)
        if sync.small is not None:
            lo, hi = sync.small
            self._launch(lo, hi - lo, lr, max_norm, grad_scale, ss, sync.gbf.data_ptr() + 2 * lo, f["s"].data_ptr() + 2 * lo, 0, ema_mode)
        sync.gather_shadows()
        if self.posthoc:
            # behind the AdamW launches (and the launch of the weight all-gathers, which only read the bf16 send buffer): the rank's
            # chunks through the cached range table, the small region flat
            if one_launch:
                if ranges:
                    self._posthoc_update(0, 0, self._range_off, self._range_cnt)
            else:
                for off, cnt in ranges:
                    self._posthoc_update(off, cnt)
            if sync.small is not None:
                self._posthoc_update(sync.small[0], sync.small[1] - sync.small[0])
        self.dit.mark_shadow_fresh()

    def grad_norm(self) -> torch.Tensor:
        """||g||_2 of the last step's (rank-averaged) gradient before clipping (device scalar; valid after step() with
        max_norm > 0 or skip_nonfinite).  The sum of squares is taken over the rank-SUMMED gradient; the 1 / world factor is applied here as in
        the optimiser kernel."""
        return self.sumsq.sqrt() * self.last_grad_scale

    def _by_name(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Views of a flat buffer keyed by parameter name, in table order (from the table alone: also without flat buffers on a GPU)."""
        return {s.name: flat[self._offs[s.name]:self._offs[s.name] + math.prod(s.shape)].view(s.shape)
                for s in self.dit._table if not s.buffer}

    def state_dict(self):
        """Moments (and EMA) keyed by parameter name, like torch.optim's per-parameter state: independent of the flat layout."""
        sd = {"m": self._by_name(self.m), "v": self._by_name(self.v), "step": self.step_count, "format": "by_name"}
        if self.ema is not None:
            sd["ema"], sd["ema_live"] = self._by_name(self.ema), self.ema_live
        if self.posthoc:
            sd["posthoc"] = {"sigma_rels": list(self.posthoc_sigma_rels), "ema": [self._by_name(e) for e in self.posthoc]}
        return sd

    def load_state_dict(self, sd):
        def put(dst_flat, src):
            if isinstance(src, dict):
                views = self._by_name(dst_flat)
                if set(views) != set(src):
                    raise RuntimeError(f"optimizer state names differ from the model's: {sorted(set(views) ^ set(src))[:4]} ...")
                for k, v in views.items():
                    v.copy_(src[k])
            else:                           # a flat tensor is only meaningful under the flat layout it was saved from, and the
                # layout has changed between rounds (dit.flat_layout: the adaLN weights moved to the front) -- a matching element
                # count proves nothing, so flat state is refused
                raise RuntimeError("flat-format optimizer state is not accepted: re-save it keyed by parameter name "
                                   "(FusedAdamW.state_dict(), format 'by_name')")
        put(self.m, sd["m"])
        put(self.v, sd["v"])
        self.step_count = int(sd["step"])
        if self.ema is not None and "ema" in sd:
            put(self.ema, sd["ema"])
            self.ema_live = bool(sd.get("ema_live", True))
        elif self.ema is not None and self.step_count > self.ema_start:
            # resuming past ema_start from a checkpoint that holds no EMA: the average would silently restart from the
            # current weights.  That is what Composer's EMA does when it is first enabled, but it must not go unnoticed.
            warnings.warn(f"optimizer state at step {self.step_count} (> ema_start {self.ema_start}) carries no EMA weights: "
                          "the EMA restarts from the current weights")
        elif self.ema is None and "ema" in sd:
            warnings.warn("the checkpoint carries EMA weights but this run configures no EMA: they are dropped")
        ph = sd.get("posthoc")
        if self.posthoc and ph is not None:
            if len(ph["ema"]) != len(self.posthoc):
                raise RuntimeError(f"the checkpoint carries {len(ph['ema'])} post-hoc EMA profiles, this run configures {len(self.posthoc)}")
            if any(abs(a - b) > 1e-12 for a, b in zip(ph["sigma_rels"], self.posthoc_sigma_rels)):
                warnings.warn(f"post-hoc EMA: the checkpoint's sigma_rels {list(ph['sigma_rels'])} differ from this run's "
                              f"{list(self.posthoc_sigma_rels)}: the loaded averages continue with the new exponents")
            for dst, src in zip(self.posthoc, ph["ema"]):
                put(dst, src)
        elif self.posthoc and self.step_count > 0:
            # beta(t > 1) would mix the zero-initialised buffers into the averages: start every profile as a copy of the weights
            warnings.warn(f"optimizer state at step {self.step_count} carries no post-hoc EMA profiles: they restart from the current weights")
            for e in self.posthoc:
                e.copy_(self.dit.flat_buffers()["p"])
        elif ph is not None:
            warnings.warn("the checkpoint carries post-hoc EMA profiles but this run configures none: they are dropped")

    # ------------------------------------------------------------------ EMA weights for evaluation / export
    def ema_state_dict(self):
        """The EMA weights as a model state_dict (same keys / shapes as dit.state_dict() for parameters), or None before the
        first EMA batch.  Saved by train.py next to the raw weights (Composer's EMA algorithm keeps them in its own state)."""
        return self._by_name(self.ema) if self.ema is not None and self.ema_live else None

    def posthoc_state_dict(self, k: int):
        """Post-hoc EMA profile k as a model state_dict (views of the profile buffer, keys / shapes of the parameters), or None
        before the first step.  Under the sharded optimiser call Trainer.consolidate() first."""
        if not 0 <= k < len(self.posthoc):
            raise IndexError(f"post-hoc EMA profile {k} of {len(self.posthoc)}")
        return self._by_name(self.posthoc[k]) if self.step_count > 0 else None

    class _EmaSwap:
        def __init__(self, opt, profile=None):
            self.opt, self.profile = opt, profile

        def _swap(self):
            """Off the step path: plain tensor swaps of the masters and the average, then re-derive the bf16 shadow."""
            o = self.opt
            buf, p = (o.ema if self.profile is None else o.posthoc[self.profile]), o.dit.flat_buffers()["p"]
            tmp = p.clone()
            p.copy_(buf)
            buf.copy_(tmp)
            o.dit.refresh_shadow(force=True)

        def __enter__(self):
            o = self.opt
            if self.profile is None:
                self.active = o.ema is not None and o.ema_live
            else:
                if not 0 <= self.profile < len(o.posthoc):
                    raise IndexError(f"post-hoc EMA profile {self.profile} of {len(o.posthoc)}")
                self.active = o.step_count > 0
            if self.active and getattr(o.dit, "shadow_is_authoritative", False):
                # sharded optimiser: the fp32 masters of the other ranks' chunks are stale and refresh_shadow() would refuse AFTER
                # the swap, leaving masters and EMA exchanged -- refuse here, before anything is touched
                raise RuntimeError("swap_ema() with stale fp32 masters (sharded optimiser): call Trainer.consolidate() first")
            if self.active:
                self._swap()
            return self.active

        def __exit__(self, *exc):
            if self.active:
                self._swap()
            return False

    def swap_ema(self, profile: Optional[int] = None):
        """Context manager: the model computes with the EMA weights inside (Composer's EMA swaps them in for evaluation);
        a no-op before the first EMA batch.  `profile` = k evaluates on post-hoc EMA profile k instead (a no-op before the first step)."""
        return FusedAdamW._EmaSwap(self, profile)
