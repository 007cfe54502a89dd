"""Training-step runtime for the MI355X MicroDiT path: what Composer's Trainer + FSDP + GradientClipping +
torch.optim.AdamW + the LR scheduler do around `LatentDiffusion.forward` in the reference (train.py:14-123,
configs/*.yaml), re-designed for one process per GPU with RCCL over xGMI:

  * the per-rank batch (global_batch / world_size, train.py:50) is split into microbatches of
    `device_train_microbatch_size` (yaml trainer.device_train_microbatch_size); microbatch i contributes with weight
    n_i / n_rank_batch (Composer semantics): `LatentDiffusion.train_microbatch` runs forward, loss and
    the hand-written backward as one launch sequence (no autograd graph), the weight folded into md_edm_loss_train;
    gradients accumulate in the flat fp32 buffer;
  * data parallelism = the reference's FSDP SHARD_GRAD_OP (yaml trainer.fsdp_config): during the LAST microbatch's backward
    each finished segment (final layer, one DiT block, ...) of the flat gradient buffer is staged as bf16 and reduce-scattered
    asynchronously — RCCL runs on its own stream and overlaps the remaining backward kernels; every rank updates its chunk of
    the weights / moments (FusedAdamW.step_sharded, one launch over a range table) and the fresh bf16 weights are all-gathered
    bucket by bucket under the next forward (GradSync; `dp_mode="allreduce"` keeps the all-reduce form where every rank runs
    the whole optimiser pass).  Transport: torch.distributed (default) or libmicrodit_comm.so (`transport="native"`);
  * the squared gradient norm is taken per reduced bucket on a side stream behind its collective (fixed-order partial sums:
    the clip coefficient is bit-identical on all ranks, no host sync), then one fused pass clips, applies AdamW, re-emits the
    bf16 shadow weights and (all-reduce form) zeroes the gradients;
  * training health (opt-in): `Trainer(monitor_interval=N)` takes per-tensor gradient / weight statistics every N batches
    (md_tensor_stats_*: Composer's OptimizerMonitor, configs/*.yaml callbacks.optimizer_monitor) and
    `FusedAdamW(skip_nonfinite=True)` turns a step whose gradient norm is not finite into a no-op on the device (md_step_guard:
    the reference's NaNCatcher, but before the update reaches the weights and without a host sync);
  * model diagnostics (opt-in): `Trainer(diagnostics_interval=N, loss_by_sigma_bins=n, moe_routing=True)` keeps the EDM loss split by
    noise level and, on every N-th batch, the token coverage / entropy / marginals of every expert-choice router
    (diagnostics.py, md_loss_sigma_hist / md_moe_route_stats); `Trainer.diagnostics()` reads them;
  * post-hoc EMA (opt-in): `FusedAdamW(posthoc_sigma_rels=(0.05, 0.10))` tracks up to four power-function averages of the masters in
    one extra bandwidth pass behind the AdamW pass (md_ema_power_update[_ranges]); train.py snapshots them and posthoc_ema.py
    synthesises the average for any EMA length afterwards (Karras et al. 2024, section 3);
  * learned loss weighting (opt-in): `Trainer(loss_weighting=LossWeighting())` trains u(sigma) next to the network (loss_weighting.py,
    Karras et al. 2024, section 2.2): two more tiny launches per microbatch, one fp32 all-reduce of its C gradient values per step and
    one C-element AdamW launch behind the main optimiser pass;
  * dispersive loss (opt-in): `Trainer(disperse=DisperseLoss())` adds a batch-repulsion term on one backbone block's output to every
    microbatch's objective (disperse.py, Wang & He 2025): a Gram, md_disperse_pairs and one injection GEMM per microbatch, no
    parameters, no collective on the step path;
  * Muon (opt-in): `Trainer(model, muon.Muon(model.dit, ...))` steps orthogonalised momentum on the hidden matrices of the blocks and
    the unchanged AdamW kernel on everything else through the same `opt.step(...)` call (muon.py); the exchange
    keeps the all-reduce form (`shardable = False`).
"""
from __future__ import annotations

import bisect
import collections
import os
import math
import re
import time
from ctypes import byref
from typing import Callable, Dict, List, Optional

import torch
import torch.distributed as dist

from . import hip
from . import diagnostics as mddiag
from . import posthoc_ema
from .disperse import DisperseLoss
from .loss_weighting import LossWeighting


def parse_batches(v) -> int:
    """'2500ba' -> 2500 (Composer time strings; only batch units appear in configs/*.yaml)."""
    if isinstance(v, (int, float)):
        return int(v)
    m = re.fullmatch(r"\s*(\d+)\s*ba\s*", str(v))
    if not m:
        raise ValueError(f"unsupported duration '{v}' (only '<N>ba' is used by the MicroDiT configs)")
    return int(m.group(1))


class LRSchedule:
    """Composer schedulers named in configs/*.yaml, as multiplicative factors of the base LR, stepped once per batch
    (SURVEY.md Appendix C.3 — Composer source is not available offline, formulas per its documentation):
      CosineAnnealingWithWarmupScheduler(t_warmup, alpha_f), ConstantScheduler(alpha),
      ConstantWithWarmupScheduler(t_warmup, alpha)."""

    def __init__(self, kind: str, t_warmup=0, t_max=1, alpha_f: float = 0.0, alpha: float = 1.0):
        self.kind, self.t_warmup, self.t_max = kind, parse_batches(t_warmup), parse_batches(t_max)
        self.alpha_f, self.alpha = alpha_f, alpha

    @staticmethod
    def from_target(target: str, t_max, **kw) -> "LRSchedule":
        name = target.split(".")[-1]
        kinds = {"CosineAnnealingWithWarmupScheduler": "cosine_with_warmup", "ConstantScheduler": "constant",
                 "ConstantWithWarmupScheduler": "constant_with_warmup"}
        if name not in kinds:
            raise ValueError(f"scheduler {target} not supported")
        kw = {k: v for k, v in kw.items() if k in ("t_warmup", "alpha_f", "alpha")}
        return LRSchedule(kinds[name], t_max=t_max, **kw)

    def factor(self, step: int) -> float:
        """`step` = optimiser steps already taken (the first batch trains at factor(0))."""
        if self.kind == "constant":
            return self.alpha
        if self.kind == "constant_with_warmup":
            return self.alpha * min(1.0, step / self.t_warmup) if self.t_warmup > 0 else self.alpha
        if step < self.t_warmup:
            return step / self.t_warmup
        frac = min(1.0, (step - self.t_warmup) / max(1, self.t_max - self.t_warmup))
        return self.alpha_f + (1 - self.alpha_f) * 0.5 * (1 + math.cos(math.pi * frac))


def stats_items(offs, numels, present, item_max: int = hip.STATS_ITEM_MAX):
    """Work items of md_tensor_stats_partial (pure host code).  `offs` / `numels`: flat offset and exact element count of every
    tensor, in the order of the result table.  `present`: [(flat_lo, count, src_off)] -- the stretches of the flat index space the
    source buffer holds, and where (in elements of that buffer): the whole flat buffer is [(0, total, 0)], a rank's packed chunk
    buffer [(lo + rank * chunk, chunk, olo) for ... in shard_plan(...)[0]], the small region inside the whole-size bf16 exchange
    buffer [(lo, hi - lo, lo)].  Every tensor's intersection with `present` is cut into pieces of at most `item_max` elements.
    Returns (items, item_begin): items = [(src_off, count, tensor)] sorted by tensor, item_begin[t] .. item_begin[t + 1] = the run of
    tensor t (empty when the buffer holds nothing of it)."""
    if item_max <= 0 or item_max % 8:
        raise ValueError("item_max must be a positive multiple of 8 (16-byte loads)")
    stretches = sorted(present)
    items, item_begin = [], [0]
    for t, (o, n) in enumerate(zip(offs, numels)):
        for lo, cnt, src in stretches:
            a, b = max(o, lo), min(o + n, lo + cnt)
            if a >= b:
                continue
            so = src + (a - lo)
            if so % 8:
                raise ValueError(f"tensor {t}: source offset {so} is not a multiple of 8 elements")
            while a < b:
                c = min(item_max, b - a)
                items.append((so, c, t))
                so += c
                a += c
        item_begin.append(len(items))
    return items, item_begin


def combine_rank_tables(table: torch.Tensor, small: torch.Tensor) -> torch.Tensor:
    """Per-rank statistics tables [world, 3, T] (rows: sum of squares, max |x|, non-finite count; rank r's table at index r) -> the
    table of the whole buffer [3, T]: rows reduced in RANK ORDER (sum, max, sum), the tensors of the small region (`small`: bool
    [T]), which every rank holds whole, taken from rank 0.  Every element is counted once; the order is fixed, so every rank that
    holds the same [world, 3, T] gets the same bits."""
    out = table[0].clone()
    for r in range(1, table.shape[0]):
        out[0] += table[r, 0]
        out[1] = torch.maximum(out[1], table[r, 1])
        out[2] += table[r, 2]
    return torch.where(small.unsqueeze(0), table[0], out)


class _StatsPlan:
    """Device-side item tables and result buffers of one statistics pass (cached per layout and exchange mode).
    sources = [(buffer, present)]: one md_tensor_stats_partial call each, into consecutive slices of the partial arrays."""

    def __init__(self, offs, numels, sources, device):
        import numpy as np
        self.sources, items_all = [], []
        for buf, present in sources:
            items, _ = stats_items(offs, numels, present)
            if items:
                self.sources.append((buf, 1 if buf.dtype == torch.bfloat16 else 0, len(items_all), len(items)))
                items_all += items
        if any(a[2] > b[2] for a, b in zip(items_all, items_all[1:])):
            raise RuntimeError("statistics items of the sources do not concatenate in tensor order")
        T = self.n_tensors = len(offs)
        begin = [0] * (T + 1)
        for _, _, t in items_all:
            begin[t + 1] += 1
        for t in range(T):
            begin[t + 1] += begin[t]
        arr = np.zeros(max(len(items_all), 1), dtype=np.dtype([("o", "<i8"), ("c", "<i4"), ("t", "<i4")]))    # md_stats_item
        for i, it in enumerate(items_all):
            arr[i] = it
        self.items = torch.from_numpy(arr.view(np.int64).reshape(-1, 2).copy()).to(device)
        self.item_begin = torch.tensor(begin, dtype=torch.int32, device=device)
        n = max(len(items_all), 1)
        self.part_f = torch.zeros(2, n, device=device)
        self.part_i = torch.zeros(n, device=device, dtype=torch.int32)
        self.out_f = torch.zeros(2, T, device=device)                       # sum of squares, max |x|
        self.out_i = torch.zeros(T, device=device, dtype=torch.int32)       # non-finite count

    def run(self):
        L, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        pf, pi = self.part_f, self.part_i
        for buf, is_bf16, first, n in self.sources:
            hip.check(L.md_tensor_stats_partial(buf.data_ptr(), is_bf16, self.items.data_ptr() + 16 * first, n,
                                                pf[0].data_ptr() + 4 * first, pf[1].data_ptr() + 4 * first, pi.data_ptr() + 4 * first, st),
                      "md_tensor_stats_partial")
        hip.check(L.md_tensor_stats_finish(pf[0].data_ptr(), pf[1].data_ptr(), pi.data_ptr(), self.item_begin.data_ptr(), self.n_tensors,
                                           self.out_f[0].data_ptr(), self.out_f[1].data_ptr(), self.out_i.data_ptr(), st),
                  "md_tensor_stats_finish")
        return self.out_f, self.out_i


class FusedAdamW:
    """torch.optim.AdamW semantics (train.py:39-43) on the DiT's flat buffers, one HIP kernel per step; optionally the
    EMA of the weights the res-512 configs name (configs/res_512_pretrain.yaml:4-9: smoothing 0.99975, every batch, from
    batch 25000 on) folded into the same pass."""

    MAX_BUCKETS = 64      # per-bucket partial sums of the gradient norm (data-parallel exchange), MD_SUMSQ_PARTIALS floats each

    def __init__(self, dit, lr: float = 2.4e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.1,
                 ema_smoothing: Optional[float] = None, ema_start: int = 0, skip_nonfinite: bool = False,
                 posthoc_sigma_rels=None):
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
        position (Trainer.batches_seen) and ema_live advance as on any other step."""
        self.dit = dit
        self._refuse_adapter()
        f = dit.flat_buffers()
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.m = torch.zeros_like(f["p"])
        self.v = torch.zeros_like(f["p"])
        self.sumsq = torch.zeros(1, device=f["p"].device)
        self.partials = torch.zeros(self.MAX_BUCKETS * hip.SUMSQ_PARTIALS, device=f["p"].device)
        self.norm_slots = self.MAX_BUCKETS
        self.step_count = 0
        self.ema_smoothing, self.ema_start = ema_smoothing, int(ema_start)
        self.ema = torch.zeros_like(f["p"]) if ema_smoothing is not None else None
        self.ema_live = False
        self.last_grad_scale = 1.0
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guard_state = torch.zeros(4, device=f["p"].device, dtype=torch.int32) if self.skip_nonfinite else None    # md_step_guard
        self.posthoc_sigma_rels = tuple(float(s) for s in (posthoc_sigma_rels or ()))
        if len(self.posthoc_sigma_rels) > hip.EMA_MAX_PROFILES:
            raise ValueError(f"at most {hip.EMA_MAX_PROFILES} post-hoc EMA profiles (MD_EMA_MAX_PROFILES), got {len(self.posthoc_sigma_rels)}")
        self.posthoc_gammas = tuple(posthoc_ema.sigma_rel_to_gamma(s) for s in self.posthoc_sigma_rels)
        self.posthoc = [torch.zeros_like(f["p"]) for _ in self.posthoc_sigma_rels]        # empty list: the feature is off

    def _refuse_adapter(self) -> None:
        """This pass emits the bf16 shadow itself and would overwrite a LoRA merge (and train the base the adapter assumes frozen)."""
        if getattr(self.dit, "_lora", None) is not None:
            raise RuntimeError("FusedAdamW on a DiT with a LoRA adapter attached: step the adapter with lora.LoRAAdamW, or fuse() / "
                               "detach() it first")

    def skipped_steps(self) -> int:
        """Steps the device-side guard turned into a no-op so far (synchronises: the only host read of the guard)."""
        return int(self.guard_state[1].item()) if self.guard_state is not None else 0

    def _guard(self, st) -> None:
        hip.check(hip.lib().md_step_guard(self.sumsq.data_ptr(), self.guard_state.data_ptr(), st), "md_step_guard")

    def ensure_norm_slots(self, n: int) -> None:
        """Room for `n` per-bucket partial sums of the gradient norm (a model with more data-parallel buckets than MAX_BUCKETS:
        the sharded exchange has no other way to form ||g||)."""
        if n > self.norm_slots:
            self.partials = torch.zeros(n * hip.SUMSQ_PARTIALS, device=self.partials.device)
            self.norm_slots = n

    def _launch(self, off: int, n: int, lr: float, max_norm: float, grad_scale: float, ss, g_bf16_ptr, shadow_ptr, zero_grad: int,
                ema_mode: int) -> None:
        """md_adamw_step on elements [off, off + n) of the flat buffers; the bf16 gradient / bf16 weight output may live elsewhere
        (the packed per-rank buffers of the sharded exchange)."""
        f = self.dit.flat_buffers()
        L, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        b1, b2 = self.betas
        a = hip.AdamWArgs(f["p"].data_ptr() + 4 * off, f["g"].data_ptr() + 4 * off, self.m.data_ptr() + 4 * off,
                          self.v.data_ptr() + 4 * off, shadow_ptr, ss, g_bf16_ptr,
                          (self.ema.data_ptr() + 4 * off) if self.ema is not None else None, n, lr, b1, b2, self.eps,
                          self.weight_decay, 1 - b1 ** self.step_count, 1 - b2 ** self.step_count, max_norm or 0.0, grad_scale,
                          self.ema_smoothing or 0.0, zero_grad, ema_mode)
        if self.skip_nonfinite:
            hip.check(L.md_adamw_step_guarded(byref(a), self.guard_state.data_ptr(), st), "md_adamw_step_guarded")
        else:
            hip.check(L.md_adamw_step(byref(a), st), "md_adamw_step")

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
        L, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        ema_mode = self._begin_step(grad_scale)
        ss = None
        if (max_norm and max_norm > 0) or self.skip_nonfinite:
            if norm_partials <= 0:
                src = g_bf16 if g_bf16 is not None else f["g"]
                hip.check(L.md_sumsq(src.data_ptr(), 1 if g_bf16 is not None else 0, f["total"], self.partials.data_ptr(), st), "md_sumsq")
                norm_partials = hip.SUMSQ_PARTIALS
            hip.check(L.md_sumsq_finish(self.partials.data_ptr(), norm_partials, self.sumsq.data_ptr(), st), "md_sumsq_finish")
            ss = self.sumsq.data_ptr()
            if self.skip_nonfinite:
                self._guard(st)
        self._launch(0, f["total"], self.lr if lr is None else lr, max_norm, grad_scale, ss,
                     g_bf16.data_ptr() if g_bf16 is not None else None, f["s"].data_ptr(), 1, ema_mode)
        if self.posthoc:
            self._posthoc_update(0, f["total"])
        self.dit.mark_shadow_fresh()

    def step_sharded(self, sync: "GradSync", lr: Optional[float] = None, max_norm: float = 0.0, grad_scale: float = 1.0,
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
        ss = None
        if (max_norm and max_norm > 0) or self.skip_nonfinite:
            sync.finish_sharded_norm(norm_slots, self.sumsq)
            ss = self.sumsq.data_ptr()
            if self.skip_nonfinite:
                self._guard(torch.cuda.current_stream().cuda_stream)
        # ONE launch over the rank's chunks (md_adamw_step_ranges: the kernel walks the packed space the reduce-scattered gradient
        # and the send buffer live in, a range table maps it onto the flat masters / moments)
        ranges = [(lo + sync.rank * chunk, chunk if chunk_of is None else (hi - lo) // chunk_of // 64 * 64) for _, lo, hi, chunk, _ in sync.plan]
        ranges = [r for r in ranges if r[1] > 0]
        if len(ranges) <= 64:        # (with chunk_of the packed gradient / weight offsets no longer line up: timing only, as documented)
            import ctypes
            key = tuple(ranges)
            if getattr(self, "_range_key", None) != key:
                self._range_key = key
                self._range_off = (ctypes.c_int64 * len(ranges))(*[r[0] for r in ranges])
                self._range_cnt = (ctypes.c_int64 * len(ranges))(*[r[1] for r in ranges])
            b1, b2 = self.betas
            a = hip.AdamWArgs(f["p"].data_ptr(), f["g"].data_ptr(), self.m.data_ptr(), self.v.data_ptr(), sync.ssend.data_ptr(), ss,
                              sync.gred.data_ptr(), self.ema.data_ptr() if self.ema is not None else None, 0, lr, b1, b2, self.eps,
                              self.weight_decay, 1 - b1 ** self.step_count, 1 - b2 ** self.step_count, max_norm or 0.0, grad_scale,
                              self.ema_smoothing or 0.0, 0, ema_mode)
            if self.skip_nonfinite:
                hip.check(hip.lib().md_adamw_step_ranges_guarded(byref(a), self._range_off, self._range_cnt, len(ranges),
                                                                 self.guard_state.data_ptr(), torch.cuda.current_stream().cuda_stream),
                          "md_adamw_step_ranges_guarded")
            else:
                hip.check(hip.lib().md_adamw_step_ranges(byref(a), self._range_off, self._range_cnt, len(ranges),
                                                         torch.cuda.current_stream().cuda_stream), "md_adamw_step_ranges")
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
            if len(ranges) <= hip.ADAMW_MAX_RANGES:
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
        f = self.dit.flat_buffers()
        return {name: flat[f["offs"][name]:f["offs"][name] + view.numel()].view(view.shape) for name, view in f["P"].items()}

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
            import warnings
            warnings.warn(f"optimizer state at step {self.step_count} (> ema_start {self.ema_start}) carries no EMA weights: "
                          "the EMA restarts from the current weights")
        elif self.ema is None and "ema" in sd:
            import warnings
            warnings.warn("the checkpoint carries EMA weights but this run configures no EMA: they are dropped")
        ph = sd.get("posthoc")
        if self.posthoc and ph is not None:
            if len(ph["ema"]) != len(self.posthoc):
                raise RuntimeError(f"the checkpoint carries {len(ph['ema'])} post-hoc EMA profiles, this run configures {len(self.posthoc)}")
            if any(abs(a - b) > 1e-12 for a, b in zip(ph["sigma_rels"], self.posthoc_sigma_rels)):
                import warnings
                warnings.warn(f"post-hoc EMA: the checkpoint's sigma_rels {list(ph['sigma_rels'])} differ from this run's "
                              f"{list(self.posthoc_sigma_rels)}: the loaded averages continue with the new exponents")
            for dst, src in zip(self.posthoc, ph["ema"]):
                put(dst, src)
        elif self.posthoc and self.step_count > 0:
            # beta(t > 1) would mix the zero-initialised buffers into the averages: start every profile as a copy of the weights
            import warnings
            warnings.warn(f"optimizer state at step {self.step_count} carries no post-hoc EMA profiles: they restart from the current weights")
            for e in self.posthoc:
                e.copy_(self.dit.flat_buffers()["p"])
        elif ph is not None:
            import warnings
            warnings.warn("the checkpoint carries post-hoc EMA profiles but this run configures none: they are dropped")

    # ------------------------------------------------------------------ EMA weights for evaluation / export
    def ema_state_dict(self):
        """The EMA weights as a model state_dict (same keys / shapes as dit.state_dict() for parameters), or None before the
        first EMA batch.  Saved by train.py next to the raw weights (Composer's EMA algorithm keeps them in its own state)."""
        if self.ema is None or not self.ema_live:
            return None
        f = self.dit.flat_buffers()
        out = {}
        for name, view in f["P"].items():
            o = f["offs"][name]
            out[name] = self.ema[o:o + view.numel()].view(view.shape)
        return out

    def posthoc_state_dict(self, k: int):
        """Post-hoc EMA profile k as a model state_dict (views of the profile buffer, keys / shapes of the parameters), or None
        before the first step.  Under the sharded optimiser call Trainer.consolidate() first."""
        if not 0 <= k < len(self.posthoc):
            raise IndexError(f"post-hoc EMA profile {k} of {len(self.posthoc)}")
        return self._by_name(self.posthoc[k]) if self.step_count > 0 else None

    class _EmaSwap:
        def __init__(self, opt, profile=None):
            self.opt, self.profile = opt, profile

        def _buf(self):
            return self.opt.ema if self.profile is None else self.opt.posthoc[self.profile]

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
            if self.active:                       # off the step path: plain tensor swaps, then re-derive the bf16 shadow
                f = o.dit.flat_buffers()
                tmp = f["p"].clone()
                f["p"].copy_(self._buf())
                self._buf().copy_(tmp)
                o.dit.refresh_shadow(force=True)
            return self.active

        def __exit__(self, *exc):
            if self.active:
                o = self.opt
                f = o.dit.flat_buffers()
                tmp = f["p"].clone()
                f["p"].copy_(self._buf())
                self._buf().copy_(tmp)
                o.dit.refresh_shadow(force=True)
            return False

    def swap_ema(self, profile: Optional[int] = None):
        """Context manager: the model computes with the EMA weights inside (Composer's EMA swaps them in for evaluation);
        a no-op before the first EMA batch.  `profile` = k evaluates on post-hoc EMA profile k instead (a no-op before the first step)."""
        return FusedAdamW._EmaSwap(self, profile)


RCCL_CHANNELS_DEFAULT = 8      # CUs handed to RCCL per rank: 8 channels move the 2 x 2 GB of a step at well over the ~30 GB/s the
#                                overlap needs (xGMI: 7 links x ~50 GB/s per direction); every channel costs the GEMMs 1 / 256


def cap_rccl_channels(n: int = RCCL_CHANNELS_DEFAULT) -> int:
    """Call BEFORE the process group / communicator is created: bounds the CUs RCCL's persistent kernels occupy
    (NCCL_MAX_NCHANNELS; a value the user exported wins).  Returns the cap in force."""
    import os
    os.environ.setdefault("NCCL_MAX_NCHANNELS", str(n))
    cap = rccl_channel_cap()          # tolerant parse: a non-numeric exported value counts as "no cap" (0)
    if cap > 0:
        os.environ.setdefault("NCCL_MIN_NCHANNELS", str(min(n, cap)))
    return cap


def rccl_channel_cap() -> int:
    import os
    try:
        return max(0, min(64, int(os.environ.get("NCCL_MAX_NCHANNELS", "0"))))
    except ValueError:
        return 0


def shard_plan(buckets, world: int):
    """Rank chunks of the data-parallel buckets.  `buckets` = [(key, lo, hi)] tiling the flat buffer (dit.bucket_ranges; every
    boundary is a multiple of dit._BUCKET_ALIGN, so (hi - lo) / world is a whole number of 128-byte lines for world <= 16).
    Returns [(key, lo, hi, chunk, olo)] for the matrix-shaped buckets in flat (= forward) order — rank r owns
    [lo + r * chunk, lo + (r + 1) * chunk) of bucket i and keeps its reduced gradient / fresh bf16 weights at [olo, olo + chunk)
    of a packed per-rank buffer — and the (lo, hi) of the "small" region every rank owns whole."""
    plan, olo, small = [], 0, None
    for key, lo, hi in buckets:
        if key == "small":
            small = (lo, hi)
            continue
        n = hi - lo
        if n % world or (n // world) % 64:
            raise ValueError(f"bucket {key} [{lo}, {hi}) does not split into {world} aligned chunks")
        plan.append((key, lo, hi, n // world, olo))
        olo += n // world
    return plan, small, olo


class GradSync:
    """Overlapped data-parallel gradient exchange (the reference's FSDP gradient reduction, configs/*.yaml fsdp_config:
    SHARD_GRAD_OP = gradients and optimiser state sharded, weights whole).

    As soon as the engine reports the backward of a segment (final layer, one DiT block, ...) as enqueued, that bucket of the
    flat gradient buffer is handed to RCCL (torch.distributed, backend "nccl" = RCCL over xGMI; async: the collective runs on
    RCCL's own stream behind an event on the compute stream) while the remaining backward kernels keep the CUs busy.

    mode "sharded" (default for N > 1 with the bf16 exchange): ZeRO-1 in the reference's sense —
      * a bucket is staged as bf16 (md_cast_f32_bf16_clear: the fp32 accumulators come back zeroed) and REDUCE-SCATTERED: rank r
        receives the sum of chunk r only (half the bytes an all-reduce moves per rank);
      * each rank takes the squared norm of ITS chunks on a side stream; one scalar all-reduce completes ||g||^2 (identical on
        all ranks);
      * FusedAdamW.step_sharded updates the rank's chunks of weights / moments (1 / N of the 34 B per parameter pass) and writes
        their fresh bf16 values into a packed send buffer;
      * the bf16 shadow weights are ALL-GATHERED bucket by bucket in forward order, asynchronously; the engine waits for a
        bucket right before the first kernel that reads it (DiTEngine.before_segment), so the gather hides under the next forward;
      * one-dimensional tensors (the "small" region: the engine reads them from the fp32 masters) are all-reduced as one bucket
        and updated by every rank.
      The fp32 masters / moments of foreign chunks go stale: Trainer.consolidate() all-gathers them before a checkpoint or an
      evaluation on EMA weights.
    mode "allreduce": every bucket all-reduced, every rank runs the whole optimiser pass (round 2's exchange; also the fp32 /
      gloo parity path).  Exchange formats: "bf16" (2.33 GB per step for XL/2; FSDP's default mixed precision reduces in the low
      precision too, SURVEY.md C.7 -- measured effect at 8 ranks: tests/test_abi_and_dp_cpu.py) or "fp32" in place.
    The squared norm of every reduced bucket is taken on a side stream right behind its collective (deterministic partial sums,
    md_sumsq), so the clip coefficient needs no extra pass after the last bucket and is bit-identical on all ranks."""

    def __init__(self, dit, process_group=None, exchange: str = "auto", single_rank_exchange: bool = False, mode: str = "auto",
                 transport: str = "torch", grad_exchange: bool = True):
        """`grad_exchange=False` (the Trainer under a factored LoRA adapter): the base's gradient is never formed, so
        there is nothing of its size to exchange -- no gbf / gred / ssend, on_segment a no-op, finish() returns 0 slots, no bf16 store
        path; the process group, rank / world, _all_reduce (all transports) and the Trainer's CU reservation work as always.
        `single_rank_exchange`: run the whole exchange path (staging cast, asynchronous collectives, side-stream norm) also on
        a process group of ONE rank, where every collective is the identity — the only way to drive the RCCL code path on a box
        with a single GPU (tests/test_dp_gpu.py); never set in production.
        `transport`: "torch" — the collectives are torch.distributed calls (backend "nccl" = RCCL); "native" — they go through
        libmicrodit_comm.so (include/microdit_comm.h: md_comm_*_bucket on the communicator's own high-priority HIP stream), and
        torch.distributed (any backend) only carries the 128-byte unique id at start-up."""
        self.dit = dit
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        self.enabled = self.world > 1 or (single_rank_exchange and dist.is_initialized())
        self.grad_exchange = bool(grad_exchange)
        if not self.grad_exchange:
            if mode == "sharded":
                raise ValueError("the sharded exchange needs the gradient exchange (grad_exchange=True)")
            exchange, mode = "fp32", "allreduce"
        assert transport in ("torch", "native")
        self.transport = transport if self.enabled else "torch"
        self.comm = None
        if exchange == "auto":
            exchange = "bf16" if (self.enabled and (dist.get_backend(process_group) == "nccl" or self.transport == "native")) else "fp32"
        assert exchange in ("bf16", "fp32")
        f = dit.flat_buffers()
        buckets = f.get("buckets")
        if buckets is None:                                   # a bare table (CPU tests): derive the ranges here
            from .dit import bucket_ranges
            buckets = bucket_ranges(dit._table, f["offs"], f["total"])
        self.bucket_list = list(buckets)
        self.mode_note = None
        if mode == "auto":
            mode = "sharded" if (self.enabled and exchange == "bf16") else "allreduce"
            if mode == "sharded":
                # buckets are multiples of dit._BUCKET_ALIGN = 1024 elements: they split into 64-element-aligned rank chunks when
                # the world size divides 16 (2, 4, 8, 16).  Any other world size (3, 5, 6, 7 GPUs) keeps the all-reduce exchange,
                # which has no such constraint; only an EXPLICIT mode="sharded" raises.
                try:
                    shard_plan(self.bucket_list, self.world)
                except ValueError as e:
                    mode = "allreduce"
                    self.mode_note = f"world size {self.world}: {e}; falling back to the all-reduce exchange"
                    import warnings
                    warnings.warn("GradSync: " + self.mode_note)
        assert mode in ("sharded", "allreduce")
        if mode == "sharded" and exchange != "bf16":
            raise ValueError("the sharded exchange stages gradients as bf16 (exchange='bf16')")
        self.exchange, self.mode = exchange, mode
        # segment name reported by the engine -> its ranges ("rest" also flushes "small": both complete with the last segment)
        self.ranges: Dict[str, List[tuple]] = {}
        for key, lo, hi in self.bucket_list:
            self.ranges.setdefault(key, []).append((lo, hi))
        self.pending = []
        self._adaln_b_sent = False           # the backbone's adaLN bucket went out with "blocks.0" in this backward
        self._wire = collections.deque()     # every collective handle in issue order, for in_flight()
        # in_flight() decides md_gemm_args.cu_limit, and the CU count decides whether a bf16-output GEMM takes the split-K tail form
        # (another fp32 summation order): a LIVE completion poll therefore makes a data-parallel run not bit-reproducible from run
        # to run (replicas stay identical: gradients are reduced).  MD_DP_DETERMINISTIC=1 answers from host state instead (issued
        # and not yet consumed): reproducible, the grids give up their CUs for longer.
        # MD_DETERMINISTIC=1 (the engine's deterministic mode, DiTEngine.deterministic) implies it; the Trainer also copies the engine's switch.
        self.deterministic = os.environ.get("MD_DP_DETERMINISTIC", "0") == "1" or os.environ.get("MD_DETERMINISTIC", "0") == "1"
        self.store_bf16 = os.environ.get("MD_DP_STORE_BF16", "1") != "0"    # one-microbatch steps: begin_backward() (A/B: 0 = off)
        self.last_stored = 0
        self.active = False
        self.buckets = 0                 # buckets handed over in the current step (= partial-sum slots in use)
        self.last_buckets = 0            # ... in the last finished step (bench.py dp block)
        self.step_bytes = self.last_bytes = 0   # bytes handed to the collectives in the current / last step
        self.norm_partials: Optional[torch.Tensor] = None     # set by the Trainer: FusedAdamW.partials
        on_gpu = f["g"].is_cuda
        dev = f["g"].device
        self.gbf = torch.zeros(f["total"], device=dev, dtype=torch.bfloat16) if (exchange == "bf16" and self.enabled) else None
        self.side = torch.cuda.Stream(device=dev) if (self.enabled and on_gpu) else None
        if self.transport == "native":
            if not on_gpu:
                raise ValueError("the native transport moves device buffers over RCCL")
            from . import comm as mdcomm
            self.comm = mdcomm.Comm.from_torch_distributed(process_group)
        # torch.distributed calls on GPU tensors need RCCL underneath; under gloo they bounce through the host
        self.torch_bounce = self.enabled and on_gpu and dist.get_backend(process_group) != "nccl"
        self.host_bounce = self.torch_bounce and self.comm is None
        self.plan = self.small = None
        self.gather_work: Dict[str, list] = {}
        if mode == "sharded":
            self.plan, self.small, own = shard_plan(self.bucket_list, self.world)
            self.by_range = {(lo, hi): (chunk, olo) for _, lo, hi, chunk, olo in self.plan}
            self.gred = torch.zeros(max(own, 8), device=dev, dtype=torch.bfloat16)     # reduced gradient of this rank's chunks
            self.ssend = torch.zeros(max(own, 8), device=dev, dtype=torch.bfloat16)    # fresh bf16 weights of this rank's chunks
            # [small-region partial sums (SUMSQ_PARTIALS floats) | sum over the ranks' chunk norms (1 float)] -> md_sumsq_finish
            self.fin = torch.zeros(hip.SUMSQ_PARTIALS + 8, device=dev)

    def norm_slots(self) -> int:
        return 0 if self.norm_partials is None else self.norm_partials.numel() // hip.SUMSQ_PARTIALS

    def _track(self, work):
        if work is not None:
            self._wire.append(work)
        return work

    def in_flight(self) -> bool:
        """A collective of this exchange may be resident on the GPU right now.  Every collective handle is also kept in issue
        order in `_wire`; handles that report completion are dropped from its front (one query per call in the steady state:
        collectives of one communicator finish in order), so the GEMM grids get their CUs back as soon as the wire is idle --
        not only when finish() / wait_gather() has consumed the handles."""
        if self.deterministic:         # host state only: issued and not yet consumed by finish() / wait_gather()
            return bool(self.pending) or bool(self.gather_work)
        w = self._wire
        while w:
            q = getattr(w[0], "is_completed", None)
            try:
                if q is None or not q():
                    return True
            except Exception:       # a handle that cannot be queried counts as busy
                return True
            w.popleft()
        return False

    def describe(self) -> str:
        if not self.enabled:
            return "none (single rank)"
        n = len(self.bucket_list)
        via = " [md_comm over RCCL]" if self.comm is not None else ""
        if self.mode == "sharded":
            return (f"bf16 reduce-scatter per backward segment ({n} buckets, 1-D tensors all-reduced), sharded AdamW, bf16 weights "
                    f"all-gathered under the next forward{via}")
        return f"{self.exchange} all-reduce per backward segment ({n} buckets), overlapped with backward{via}"

    # ------------------------------------------------------------------ collectives (RCCL, or a host bounce under gloo)
    def _all_reduce(self, buf):
        if self.comm is not None:
            return self.comm.all_reduce(buf)
        if self.host_bounce:
            h = buf.float().cpu() if buf.dtype == torch.bfloat16 else buf.cpu()
            dist.all_reduce(h, group=self.pg)
            buf.copy_(h.to(buf.dtype))
            return None
        return dist.all_reduce(buf, group=self.pg, async_op=True)

    def _reduce_scatter(self, out, buf):
        if self.comm is not None:
            return self.comm.reduce_scatter(out, buf)
        if self.host_bounce:               # gloo has no reduce-scatter: all-reduce on the host, keep this rank's chunk
            h = buf.float().cpu()
            dist.all_reduce(h, group=self.pg)
            c = out.numel()
            out.copy_(h[self.rank * c:(self.rank + 1) * c].to(out.dtype))
            return None
        return dist.reduce_scatter_tensor(out, buf, group=self.pg, async_op=True)

    def _all_gather(self, out, mine):
        if self.comm is not None:
            return self.comm.all_gather(out, mine)
        if self.host_bounce:
            h = mine.float().cpu()
            parts = [torch.empty_like(h) for _ in range(self.world)]
            dist.all_gather(parts, h, group=self.pg)
            out.copy_(torch.cat(parts).to(out.dtype))
            return None
        return dist.all_gather_into_tensor(out, mine, group=self.pg, async_op=True)

    def _norm_after(self, work, buf, is_bf16, slot_ptr):
        """||buf||^2 partial sums on the side stream, right behind the collective that produced buf."""
        if self.side is None:
            return
        if work is None:
            self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            if work is not None:
                work.wait()              # stream-side dependency under NCCL; the norm overlaps the remaining backward
            hip.check(hip.lib().md_sumsq(buf.data_ptr(), 1 if is_bf16 else 0, buf.numel(), slot_ptr, self.side.cuda_stream), "md_sumsq")

    # ------------------------------------------------------------------ one-microbatch steps: weight gradients stored as bf16
    def begin_backward(self, single_microbatch: bool) -> None:
        """Called by the Trainer in front of the step's LAST microbatch.  When that microbatch is also the first (a rank of the
        8-GPU run: device_train_microbatch_size 256 = the rank's batch, configs/res_256_pretrain.yaml:24,111) and the exchange is
        the sharded bf16 one, the engine stores every weight gradient straight into `gbf` (DiTEngine.wgrad_bf16): the fp32
        accumulators of those tensors are neither read nor written in this step and _exchange skips their cast + clear."""
        eng = self.dit.engine
        eng.wgrad_bf16 = None
        if not (single_microbatch and self.store_bf16 and self.enabled and self.mode == "sharded" and self.gbf is not None and self.gbf.is_cuda):
            return
        f = self.dit.flat_buffers()
        eng.wgrad_bf16 = {"g_lo": f["g"].data_ptr(), "g_hi": f["g"].data_ptr() + 4 * f["g"].numel(), "gbf": self.gbf.data_ptr(),
                          "written": {}}

    def end_backward(self) -> None:
        t = self.dit.engine.wgrad_bf16
        self.last_stored = len(t["written"]) if t is not None else 0      # gradient launches that went straight to the exchange buffer
        self.dit.engine.wgrad_bf16 = None

    def _tensors_of(self, lo: int, hi: int):
        """(flat offset, numel) of the parameters inside the range, in address order (cached)."""
        c = getattr(self, "_range_tensors", None)
        if c is None:
            c = self._range_tensors = {}
        if (lo, hi) not in c:
            f = self.dit.flat_buffers()
            c[(lo, hi)] = sorted((o, f["P"][n].numel()) for n, o in f["offs"].items() if n in f["P"] and lo <= o < hi)
        return c[(lo, hi)]

    def _exchange(self, lo: int, hi: int) -> None:
        f = self.dit.flat_buffers()
        g = f["g"][lo:hi]
        st = torch.cuda.current_stream().cuda_stream if g.is_cuda else None
        sharded = self.mode == "sharded"
        small = sharded and self.small is not None and (lo, hi) == tuple(self.small)
        stored = self.dit.engine.wgrad_bf16 if sharded else None
        if self.exchange == "bf16":
            buf = self.gbf[lo:hi]
            if stored is not None:
                # one-microbatch step: tensors the engine stored as bf16 are in `buf` already; what it did not store (one-dimensional
                # tensors, a tensor without a gradient this step, an fp32 fall-back) is cast + cleared tensor by tensor, runs merged
                # (alignment gaps between two such tensors are zero in both buffers: a run covers them)
                g0, runs, cur = f["g"].data_ptr(), [], None
                spans = sorted(((a - g0) // 4, (a - g0) // 4 + cnt) for a, cnt in stored["written"].items())
                starts = [a for a, _ in spans]
                for o, n in self._tensors_of(lo, hi):
                    i = bisect.bisect_right(starts, o) - 1
                    if i >= 0 and o + n <= spans[i][1]:            # inside a stored span (a span may cover adjacent tensors: [w1; w2])
                        cur = None
                    elif cur is None:
                        cur = [o, o + n]
                        runs.append(cur)
                    else:
                        cur[1] = o + n
                for a, b in runs:
                    hip.check(hip.lib().md_cast_f32_bf16_clear(g0 + 4 * a, self.gbf.data_ptr() + 2 * a, b - a, st), "cast_clear")
            elif sharded:                 # the fp32 accumulators come back cleared (no later pass visits all of them)
                hip.check(hip.lib().md_cast_f32_bf16_clear(g.data_ptr(), buf.data_ptr(), hi - lo, st), "cast_clear")
            else:
                hip.check(hip.lib().md_cast_f32_bf16(g.data_ptr(), buf.data_ptr(), hi - lo, None, st), "cast")
        else:
            buf = g
        self.step_bytes += buf.numel() * buf.element_size()
        if sharded and not small:
            chunk, olo = self.by_range[(lo, hi)]
            red = self.gred[olo:olo + chunk]
            work = self._reduce_scatter(red, buf)
            slot = self.buckets
            self.buckets += 1
            if self.norm_partials is not None:
                if slot >= self.norm_slots():
                    raise RuntimeError(f"{slot + 1} reduce-scattered buckets but {self.norm_slots()} norm slots: size them with "
                                       "FusedAdamW.ensure_norm_slots(len(bucket_list)) (the Trainer does)")
                self._norm_after(work, red, True, self.norm_partials.data_ptr() + 4 * slot * hip.SUMSQ_PARTIALS)
        elif small:
            work = self._all_reduce(buf)
            self._norm_after(work, buf, True, self.fin.data_ptr())        # identical on every rank: added once, after the scalar all-reduce
        else:
            work = self._all_reduce(buf)
            slot = self.buckets
            self.buckets += 1
            if self.norm_partials is not None and slot < self.norm_slots():
                self._norm_after(work, buf, self.exchange == "bf16", self.norm_partials.data_ptr() + 4 * slot * hip.SUMSQ_PARTIALS)
        if work is not None:
            self.pending.append(self._track(work))

    def on_segment(self, name: str) -> None:
        if not self.active or not self.enabled or not self.grad_exchange:
            return
        for lo, hi in self.ranges.get(name, []):
            self._exchange(lo, hi)
        # The modulation weights of all blocks live in two buckets of their own (arch.bucket_key): the backbone's part is complete
        # once the backward of the FIRST backbone block is enqueued (409 MB of the 2.33 GB at XL/2: handed over here, the mixer's
        # backward still covers it), the mixer's part (57 MB) and the one-dimensional tensors with the last segment.
        if name == "blocks.0" and not self._adaln_b_sent:
            self._adaln_b_sent = True
            for lo, hi in self.ranges.get("adaln.b", []):
                self._exchange(lo, hi)
        if name == "rest":
            for key in (() if self._adaln_b_sent else ("adaln.b",)) + ("adaln.m", "small"):
                for lo, hi in self.ranges.get(key, []):
                    self._exchange(lo, hi)
            self._adaln_b_sent = False

    def finish(self) -> int:
        """Wait for every bucket; returns the number of norm partial-sum slots filled (0 = the optimiser takes the norm itself;
        sharded mode: the finished ||g||^2 is written to `sumsq_out` by finish_sharded_norm instead)."""
        for w in self.pending:
            w.wait()
        self.pending = []
        if not self.gather_work:
            self._wire.clear()           # everything issued has been waited for (in_flight() may never be polled: world 1, gloo, cap 0)
        n = self.buckets if (self.norm_partials is not None and self.side is not None and 0 < self.buckets <= self.norm_slots()) else 0
        if self.side is not None and self.buckets:
            torch.cuda.current_stream().wait_stream(self.side)
        self.last_buckets, self.last_bytes = self.buckets, self.step_bytes
        self.buckets = self.step_bytes = 0
        return n

    def finish_sharded_norm(self, slots: int, sumsq_out: torch.Tensor) -> None:
        """||g||^2 of the rank-summed gradient from the ranks' chunk partial sums: local finish -> scalar all-reduce -> + the small
        region's partial sums (every rank holds the same ones) -> sumsq_out.  Fixed summation order everywhere: identical bits on
        all ranks."""
        L, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        P = hip.SUMSQ_PARTIALS
        tot = self.fin[P:P + 1]
        hip.check(L.md_sumsq_finish(self.norm_partials.data_ptr(), slots * P, tot.data_ptr(), st), "md_sumsq_finish")
        w = self._all_reduce(tot)
        if w is not None:
            w.wait()
        hip.check(L.md_sumsq_finish(self.fin.data_ptr(), P + 1, sumsq_out.data_ptr(), st), "md_sumsq_finish")

    def gather_shadows(self) -> None:
        """All-gather the fresh bf16 weights bucket by bucket in forward order (asynchronous); wait_gather(key) is the engine's
        hook in front of the first kernel that reads a bucket."""
        s = self.dit.flat_buffers()["s"]
        for key, lo, hi, chunk, olo in self.plan:
            w = self._all_gather(s[lo:hi], self.ssend[olo:olo + chunk])
            self.step_bytes += (hi - lo) * 2
            if w is not None:
                self.gather_work.setdefault(key, []).append(self._track(w))

    def wait_gather(self, key: Optional[str] = None) -> None:
        if not self.gather_work:
            return
        keys = [key] if key is not None else list(self.gather_work)
        for k in keys:
            for w in self.gather_work.pop(k, []):
                w.wait()
        if not self.gather_work and not self.pending:
            self._wire.clear()


class Trainer:
    def __init__(self, model, optimizer: FusedAdamW, schedule: Optional[LRSchedule] = None, clip_norm: float = 0.0,
                 microbatch_size: int = 256, process_group=None, log: Optional[Callable[[dict], None]] = None,
                 exchange: str = "auto", single_rank_exchange: bool = False, dp_mode: str = "auto", transport: str = "auto",
                 monitor_interval: int = 0, diagnostics_interval: int = 0, loss_by_sigma_bins: int = 0, moe_routing: bool = False,
                 loss_weighting: Optional[LossWeighting] = None, disperse: Optional[DisperseLoss] = None):
        """disperse (None or weight 0: off -- no launch, no buffer): a DisperseLoss armed as model.disperse; every microbatch then adds
        weight * L_disp(output of one backbone block) to its objective.  train_step's return value and the logged `loss`
        stay the raw EDM loss; disperse_stats() reports the term, diagnostics()["disperse"] the last microbatch's result block.
        loss_weighting (None: off -- no launch, no buffer, no collective): a LossWeighting armed as model.loss_weighting.  Its C
        gradient values are all-reduced (fp32 sum) after the main exchange in every exchange mode, its AdamW launch runs behind the
        main optimiser pass at `loss_weighting.lr` (default: the optimiser's lr) times the schedule factor, outside the clipped norm,
        under the optimiser's step guard when that is on; weighted_objective() is the rank-mean objective of the last step.
        diagnostics_interval / loss_by_sigma_bins / moe_routing (all off by default: no launch, no buffer): see diagnostics().
        loss_by_sigma_bins = n > 0 arms model.loss_by_sigma (n bins over P_mean +- 3 P_std in ln sigma): every microbatch of every
        step adds to the histogram.  moe_routing arms the engine's route_stats for the microbatches of the batches whose number is a
        multiple of diagnostics_interval (tables zeroed when armed, accumulated over the step's microbatches).
        monitor_interval: N > 0 takes the per-tensor statistics (collect_tensor_stats) on every batch whose number is a multiple
        of N, between the gradient exchange and the optimiser pass; 0 = never (no launch, no buffer).
        dp_mode: "sharded" (reduce-scatter + sharded AdamW + all-gather of the bf16 weights, the reference's SHARD_GRAD_OP;
        default for N > 1 over RCCL) or "allreduce" (every rank runs the whole optimiser pass); "auto" also honours the
        MD_DP_MODE environment variable."""
        import os
        self.model, self.opt, self.schedule, self.clip_norm = model, optimizer, schedule, clip_norm
        self.microbatch_size = microbatch_size
        if dp_mode == "auto" and os.environ.get("MD_DP_MODE"):
            dp_mode = os.environ["MD_DP_MODE"]
        if exchange == "auto" and os.environ.get("MD_DP_EXCHANGE"):
            exchange = os.environ["MD_DP_EXCHANGE"]
        if transport == "auto":                # MD_COMM=native: the exchange through libmicrodit_comm.so instead of torch.distributed
            transport = os.environ.get("MD_COMM", "torch")
        adapter = getattr(optimizer, "adapter", None)
        # a factored LoRA adapter: the base's gradient does not exist; what the ranks exchange is adapter.g, one all-reduce
        self.lora_factored = adapter is not None and getattr(adapter, "backward", "projected") == "factored"
        # muon.Muon: orthogonalises whole matrices, a rank of the sharded step owns slices; factored LoRA: nothing of the base's to shard
        if not getattr(optimizer, "shardable", True) or self.lora_factored:
            if dp_mode == "sharded":
                raise NotImplementedError(f"{type(optimizer).__name__} does not run under dp_mode='sharded' (a rank owns slices of "
                                          "buckets, not whole matrices); use dp_mode='allreduce'")
            dp_mode = "allreduce"
        model.dit._ensure_flat()
        self.sync = GradSync(model.dit, process_group, exchange=exchange, single_rank_exchange=single_rank_exchange, mode=dp_mode,
                             transport=transport, grad_exchange=not self.lora_factored)
        optimizer.ensure_norm_slots(len(self.sync.bucket_list))     # one slot per bucket: the sharded norm has no other source
        self.sync.norm_partials = optimizer.partials
        if getattr(model.dit.engine, "deterministic", False):
            self.sync.deterministic = True
        self.world = self.sync.world
        if adapter is not None and not self.lora_factored and self.world > 1:
            raise NotImplementedError("LoRA training with the projected backward is single-GPU: data parallelism needs "
                                      "LoRA(backward='factored') (misc.lora_backward: factored), which all-reduces the adapter gradient")
        self.sharded = self.sync.enabled and self.sync.mode == "sharded"
        self.stale_foreign_chunks = False    # sharded: fp32 masters / moments of the other ranks' chunks are out of date
        self.shard_chunk_of = None           # measurement aid, see FusedAdamW.step_sharded
        model.dit._on_segment = self.sync.on_segment
        # RCCL's kernels hold one CU per channel while a collective runs and a workgroup of the persistent GEMM needs a whole CU:
        # leave those CUs out of the GEMM grids for as long as a collective is in flight (md_gemm_args.cu_limit; the channel
        # count is capped by NCCL_MAX_NCHANNELS, which cap_rccl_channels() sets before the process group is created)
        # (a gloo / host-bounce exchange runs no RCCL kernel: nothing holds a CU, the grids stay whole)
        on_rccl = self.sync.comm is not None or not getattr(self.sync, "host_bounce", False)
        self.rccl_channels = rccl_channel_cap() if (self.sync.enabled and self.world > 1 and on_rccl) else 0
        if self.rccl_channels:
            lim = hip.NUM_CU - self.rccl_channels
            model.dit.engine.cu_limit_fn = lambda s=self.sync, lim=lim: (lim if s.in_flight() else 0)
        model.dit.engine.before_segment = self.sync.wait_gather if self.sharded else None
        # the Trainer runs forward -> backward strictly in turn: activations may live in the engine's fixed-address arenas
        model.dit._ensure_flat()
        model.dit.engine.use_arena = True
        self.batches_seen = 0
        self.monitor_interval = int(monitor_interval)
        self._stats_plans: Dict[str, _StatsPlan] = {}
        self._stats_last = None
        self.diagnostics_interval = int(diagnostics_interval)
        if loss_by_sigma_bins > 0 and model.loss_by_sigma is None:
            ec = model.edm_config
            model.loss_by_sigma = mddiag.LossBySigma(int(loss_by_sigma_bins), ec.P_mean, ec.P_std)
        self._route_stats = mddiag.RouteStats(model.dit.engine) if moe_routing else None     # armed by train_step on report batches
        self.loss_weighting = loss_weighting
        self._objective = None               # with the loss weighting: rank-mean weighted objective of the last step (device scalar)
        model.loss_weighting = loss_weighting      # unconditionally: a model armed by an earlier Trainer must not stay armed unstepped
        if disperse is not None:
            disperse.resolve_block(len(model.dit.engine.backbone))      # raises on a block outside the backbone
        self.disperse = disperse if (disperse is not None and disperse.enabled) else None     # weight 0 is off
        model.disperse = self.disperse             # unconditionally, as above
        model.disperse_accum = self._disperse_acc = None
        self.log = log
        self._win: List[tuple] = []
        self.measure_comm = False          # bench.py: event pairs around GradSync.finish() (exposed exchange time)
        self._comm_events: List[tuple] = []
        self._opt_events: List[tuple] = []

    def train_step(self, batch: dict) -> torch.Tensor:
        """One optimisation step on this rank's share of the global batch.  Returns the rank-mean loss (device scalar).
        Microbatch i contributes with weight n_i / n (Composer scales each microbatch loss by its share of the rank batch before
        backward): the weight goes into md_edm_loss_train, which pre-multiplies dL/dF and accumulates the
        weighted loss on the device — no autograd graph and no torch arithmetic on the step path."""
        model = self.model
        n = batch[model.image_latents_key if model.image_latents_key in batch else model.image_key].shape[0]
        mb = min(self.microbatch_size, n)
        starts = list(range(0, n, mb))
        total = torch.empty(1, device=model.dit.flat_buffers()["p"].device)       # a fresh scalar per step: callers keep them
        hip.check(hip.lib().md_fill_zero(total.data_ptr(), 4, torch.cuda.current_stream().cuda_stream), "md_fill_zero")
        lw = self.loss_weighting
        if lw is not None:                   # a fresh scalar per step, like `total`: the step's rank-mean weighted objective
            lw.objective_accum = self._objective = torch.empty(1, device=total.device)
            hip.check(hip.lib().md_fill_zero(self._objective.data_ptr(), 4, torch.cuda.current_stream().cuda_stream), "md_fill_zero")
        if self.disperse is not None:        # a fresh pair per step: the step's (L_disp, mean off-diagonal D), microbatches weighted like the loss
            model.disperse_accum = self._disperse_acc = torch.empty(2, device=total.device)
            hip.check(hip.lib().md_fill_zero(self._disperse_acc.data_ptr(), 8, torch.cuda.current_stream().cuda_stream), "md_fill_zero")
        if (self._route_stats is not None and self.diagnostics_interval > 0
                and (self.batches_seen + 1) % self.diagnostics_interval == 0):
            self._route_stats.zero()
            model.dit.engine.route_stats = self._route_stats
        for i, s in enumerate(starts):
            part = {k: (v[s:s + mb] if torch.is_tensor(v) and v.shape[0] == n else v) for k, v in batch.items()}
            self.sync.active = (i == len(starts) - 1)
            if self.sync.active:
                self.sync.begin_backward(single_microbatch=(len(starts) == 1))
            w = min(mb, n - s) / n
            model.train_microbatch(part, grad_scale=w, loss_accum=total, accum_weight=w)
        self.sync.active = False
        self.sync.end_backward()
        if self._route_stats is not None:
            model.dit.engine.route_stats = None
        if self.measure_comm:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()                                  # behind the last backward kernel on the compute stream
        slots = self.sync.finish()
        if self.measure_comm:
            e1.record()                                  # behind the waits on the collectives / side-stream norms
            self._comm_events.append((e0, e1))
        if lw is not None and self.world > 1:
            self._reduce_loss_weighting_grad()
        if self.lora_factored and self.world > 1:
            self._reduce_adapter_grad()
        if self.monitor_interval > 0 and (self.batches_seen + 1) % self.monitor_interval == 0:
            self.collect_tensor_stats()                  # reads the gradients the optimiser pass is about to consume and clear
        fac = self.schedule.factor(self.batches_seen) if self.schedule is not None else 1.0
        if self.measure_comm:
            o0, o1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            o0.record()
        if self.sharded:
            self.opt.step_sharded(self.sync, lr=self.opt.lr * fac, max_norm=self.clip_norm, grad_scale=1.0 / self.world,
                                  norm_slots=slots, chunk_of=self.shard_chunk_of)
            self.stale_foreign_chunks = self.world > 1
            self.model.dit.shadow_is_authoritative = self.stale_foreign_chunks
        else:
            self.opt.step(lr=self.opt.lr * fac, max_norm=self.clip_norm, grad_scale=1.0 / self.world,
                          g_bf16=self.sync.gbf, norm_partials=slots * hip.SUMSQ_PARTIALS)
        if lw is not None:                   # behind the main pass: its guard flag (skip_nonfinite) is set by now
            lw.step((self.opt.lr if lw.lr is None else lw.lr) * fac, grad_scale=1.0 / self.world, guard_state=self.opt.guard_state)
        if self.measure_comm:
            o1.record()                                  # norm finish + AdamW (+ the launch of the weight all-gathers)
            self._opt_events.append((o0, o1))
        self.batches_seen += 1
        return total.reshape(())

    # ------------------------------------------------------------------ learned loss weighting
    def _reduce_loss_weighting_grad(self) -> None:
        """One fp32 all-reduce (sum) of the C gradient values of u(sigma) on the trainer's process group, the same in all three
        exchange modes; the 1 / world factor goes into the AdamW launch's grad_scale as for the other gradients.  A sum of `world`
        addends per element: every rank receives the same bits."""
        w = self.sync._all_reduce(self.loss_weighting.g)
        if w is not None:
            w.wait()

    def _reduce_adapter_grad(self) -> None:
        """Factored LoRA under data parallelism: one fp32 all-reduce (sum) of the adapter's gradient between the last backward and the
        optimiser pass, the same in every transport; the 1 / world factor goes into the AdamW launch's grad_scale.  Every rank receives
        the same bits, so replicas that start identical (A from the CPU seed, B = 0) stay identical."""
        w = self.sync._all_reduce(self.opt.adapter.g)
        if w is not None:
            w.wait()

    def weighted_objective(self) -> Optional[torch.Tensor]:
        """The rank-mean weighted objective (1 / B) sum_b (L_b e^{-u_b} + u_b) of the last step (device scalar; None before the first
        step or without the loss weighting).  train_step's return value stays the raw loss."""
        return self._objective.reshape(()) if self.loss_weighting is not None and self._objective is not None else None

    # ------------------------------------------------------------------ dispersive loss
    def disperse_stats(self) -> Optional[dict]:
        """{"disperse_loss": mean of L_disp over the last step's microbatches (each weighted by its share of the rank batch, like the
        loss), "disperse_mean_dist": the same mean of the mean off-diagonal D}; None without the feature or before the first step.
        Synchronises; with more than one rank a collective (every rank calls it): the ranks' pairs are gathered and added in rank
        order, then divided by the world size -- the same numbers on every rank."""
        if self.disperse is None or self._disperse_acc is None:
            return None
        vals = self._disperse_acc.double()
        if self.world > 1:
            _, sums = mddiag.gather_rank_diagnostics(torch.empty(0, dtype=torch.int64, device=vals.device), vals, self.sync.pg)
            vals = sums / self.world
        vals = vals.tolist()
        return {"disperse_loss": vals[0], "disperse_mean_dist": vals[1]}

    # ------------------------------------------------------------------ per-tensor statistics (optimizer monitor)
    def _stats_names(self) -> List[str]:
        """Rows of the statistics tables: the parameters in FLAT order (matrix-shaped tensors first, the small region last), so the
        items of the sharded exchange's two gradient buffers concatenate in tensor order."""
        f = self.model.dit.flat_buffers()
        return sorted(f["P"], key=lambda n: f["offs"][n])

    def _stats_plan(self, kind: str) -> _StatsPlan:
        if kind not in self._stats_plans:
            f, s = self.model.dit.flat_buffers(), self.sync
            names = self._stats_names()
            offs, numels = [f["offs"][n] for n in names], [f["P"][n].numel() for n in names]
            if self.sharded:
                own = [(lo + s.rank * chunk, chunk, olo) for _, lo, hi, chunk, olo in s.plan]
                small = [(s.small[0], s.small[1] - s.small[0], s.small[0])] if s.small is not None else []
                if kind == "grad":          # reduced chunks packed in gred; the small region all-reduced inside the whole-size gbf
                    sources = [(s.gred, own), (s.gbf, small)]
                else:                       # fp32 masters: this rank's chunks and the small region are current, foreign chunks stale
                    sources = [(f["p"], [(lo, cnt, lo) for lo, cnt, _ in own] + small)]
            elif kind == "grad":
                sources = [(s.gbf if (s.enabled and s.gbf is not None) else f["g"], [(0, f["total"], 0)])]
            else:
                sources = [(f["p"], [(0, f["total"], 0)])]
            self._stats_plans[kind] = _StatsPlan(offs, numels, sources, f["p"].device)
        return self._stats_plans[kind]

    def collect_tensor_stats(self) -> None:
        """One statistics pass over the step's gradients and the fp32 masters (train_step calls it between GradSync.finish() and the
        optimiser pass on monitor steps).  Gradient source: the fp32 accumulators without an exchange, the bf16 exchange buffer in
        all-reduce mode, the packed reduced chunks plus the small region in sharded mode.  Sharded with more than one rank: every
        rank writes its rows into a zero [world, 3, T] table at its rank index, ONE SUM all-reduce (the exchange's transport)
        distributes it and combine_rank_tables reduces the rows in rank order -- bit-identical on all ranks, no MAX collective.
        Enqueues only; tensor_stats() reads."""
        last = {}
        for kind in ("grad", "param"):
            out_f, out_i = self._stats_plan(kind).run()
            if self.sharded and self.world > 1:
                T = out_f.shape[1]
                table = torch.zeros(self.world, 3, T, device=out_f.device)
                table[self.sync.rank, :2] = out_f
                table[self.sync.rank, 2] = out_i.float()
                w = self.sync._all_reduce(table.view(-1))
                if w is not None:
                    w.wait()
                f = self.model.dit.flat_buffers()
                lo = self.sync.small[0] if self.sync.small is not None else f["total"]
                small = torch.tensor([f["offs"][n] >= lo for n in self._stats_names()], device=out_f.device)
                comb = combine_rank_tables(table, small)
                out_f, out_i = comb[:2], comb[2].to(torch.int32)
            last[kind] = (out_f, out_i)
        last["grad_scale"] = 1.0 / self.world
        last["batch"] = self.batches_seen + 1
        self._stats_last = last

    def tensor_stats(self) -> dict:
        """The last statistics pass as Python numbers (synchronises; {} before the first pass), keyed Composer-style:
          l2_norm/grad/<name>, l2_norm/grad/global, l2_norm/param/<name>, absmax/grad/<name>, nonfinite/grad/<name>
        with the parameter names of dit.flat_buffers()["P"].  Gradient values describe the UNCLIPPED, rank-averaged gradient (the
        rank-summed buffer times 1 / world, as FusedAdamW.grad_norm()); non-finite elements are counted and left out of norm and
        maximum.  Composer's source is not available offline: the key names are pinned from memory of its OptimizerMonitor
        (`l2_norm/grad/<parameter>`, `l2_norm/grad/global`), in the same sense as SURVEY.md Appendix C; absmax/ and nonfinite/ have
        no Composer counterpart."""
        if self._stats_last is None:
            return {}
        last, names = self._stats_last, self._stats_names()
        (gf, gi), (pf, _) = last["grad"], last["param"]
        gf, gi, pf = gf.double().cpu(), gi.cpu(), pf.double().cpu()
        sc, out = last["grad_scale"], {}
        for t, n in enumerate(names):
            out[f"l2_norm/grad/{n}"] = math.sqrt(float(gf[0, t])) * sc
            out[f"absmax/grad/{n}"] = float(gf[1, t]) * sc
            out[f"nonfinite/grad/{n}"] = int(gi[t])
            out[f"l2_norm/param/{n}"] = math.sqrt(float(pf[0, t]))
        out["l2_norm/grad/global"] = math.sqrt(float(gf[0].sum())) * sc
        return out

    # ------------------------------------------------------------------ model diagnostics (loss by sigma, expert-choice routing)
    def diagnostics(self, tables=("train", "eval"), routing: bool = True) -> dict:
        """What the model diagnostics hold, as plain Python numbers, and ZERO what was read (synchronises; with more than one rank a
        collective over the exchange's process group: every rank calls it with the same arguments and gets the same numbers -- the
        ranks' tables are gathered and added in rank order, diagnostics.gather_rank_diagnostics).  Keys:
          loss_by_sigma/{train,eval}/ln_sigma_edges, /count, /mean_loss, /nonfinite      for every table named in `tables`
                                              (needs loss_by_sigma_bins; everything accumulated since the table was last read)
          moe/<block>/coverage, /dropped_frac, /router_entropy, /expert_prob_mean, /expert_gate_mean   for every routed layer
                                              (needs moe_routing; the microbatches of the last batch that was a multiple of
                                              diagnostics_interval, absent before the first)."""
        out, model, pg = {}, self.model, self.sync.pg
        lbs = getattr(model, "loss_by_sigma", None)
        dev = model.dit.flat_buffers()["p"].device
        if lbs is not None:
            for which in tables:
                cnt, sm = lbs.tables(which, dev)
                c, s = mddiag.gather_rank_diagnostics(cnt, sm, pg)
                lbs.zero(which)
                out.update(mddiag.format_loss_by_sigma(which, lbs.edges, s.tolist(), c[:-1].tolist(), int(c[-1])))
        rs = self._route_stats
        if routing and rs is not None:
            c, s = mddiag.gather_rank_diagnostics(rs.cover_hist.reshape(-1), rs.fstats.reshape(-1), pg)
            rs.zero()
            c, s = c.view(len(rs.names), -1), s.view(len(rs.names), -1)
            for i, name in enumerate(rs.names):
                out.update(mddiag.format_route_stats(name, c[i].tolist(), s[i].tolist()))
        lw = self.loss_weighting
        if lw is not None:
            # u(sigma) at the centres of the loss-by-sigma bins when that histogram is armed (the two tables line up), else at 16 points
            # over P_mean +- 3 P_std; w is identical on every rank, the objective of the last step is averaged over the ranks
            ec = model.edm_config
            if lbs is not None:
                e = [float(x) for x in lbs.edges]
                pts = [0.5 * (a + b) for a, b in zip(e[:-1], e[1:])]
            else:
                lo, hi = ec.P_mean - 3 * ec.P_std, ec.P_mean + 3 * ec.P_std
                pts = [lo + (hi - lo) * i / 15 for i in range(16)]
            obj = self.weighted_objective()
            if obj is not None and self.world > 1:              # the mean over the ranks: every rank reports the same number
                obj = obj.reshape(1).clone()
                wk = self.sync._all_reduce(obj)
                if wk is not None:
                    wk.wait()
                obj = obj / self.world
            out["loss_weighting"] = {"ln_sigma": pts, "u": lw.u_at(pts), "objective": None if obj is None else float(obj)}
        res = getattr(model, "_disperse_result", None)
        if self.disperse is not None and res is not None:
            # the result block of this rank's last microbatch: L, mean off-diagonal D, mean off-diagonal p B^2 (1 = uniform, -> 0 = saturated)
            r = res.tolist()
            out["disperse"] = {"loss": r[0], "mean_dist": r[1], "mean_offdiag_p_b2": r[2]}
        return out

    def exposed_comm_ms(self, last: int = 0) -> Optional[float]:
        """Mean time per step the compute stream spent waiting for the gradient exchange after the last backward kernel was
        enqueued (needs measure_comm; synchronises).  `last` > 0: only the most recent steps (skip warm-up)."""
        if not self._comm_events:
            return None
        torch.cuda.synchronize()
        ev = self._comm_events[-last:] if last > 0 else self._comm_events
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev)

    def consolidate(self) -> None:
        """Sharded optimiser only: all-gather the fp32 masters, both moments, the EMA and the post-hoc EMA profiles so that every rank
        holds the whole, current state (checkpoints, snapshots, evaluation on EMA weights, state_dict()).  A collective: every rank must
        call it.  Not on the step path (3 x 4.66 GB for XL/2, one more per average; at checkpoint / evaluation / snapshot intervals)."""
        if not self.sharded or not self.stale_foreign_chunks:
            return
        s = self.sync
        s.wait_gather()
        f = self.model.dit.flat_buffers()
        bufs = [f["p"], self.opt.m, self.opt.v] + ([self.opt.ema] if self.opt.ema is not None else []) + list(self.opt.posthoc)
        for t in bufs:
            for key, lo, hi, chunk, olo in s.plan:
                mine = t[lo + s.rank * chunk: lo + (s.rank + 1) * chunk].clone()
                w = s._all_gather(t[lo:hi], mine)
                if w is not None:
                    w.wait()
        self.stale_foreign_chunks = False
        self.model.dit.shadow_is_authoritative = False

    def optimizer_ms(self, last: int = 0) -> Optional[float]:
        """Mean compute-stream time per step of the gradient-norm finish + AdamW pass (needs measure_comm; synchronises)."""
        if not self._opt_events:
            return None
        torch.cuda.synchronize()
        ev = self._opt_events[-last:] if last > 0 else self._opt_events
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev)

    def sync_replicas(self) -> None:
        """Make every rank's weights and optimiser state bit-identical to rank 0's (call once after initialisation / resume).
        Data parallelism here replicates the weights and relies on identical updates from then on; nothing else would catch a
        replica that started from a different state."""
        if self.world <= 1:
            return
        self.consolidate()          # after a sharded step rank 0's masters of foreign chunks are stale: make them whole first
        f = self.model.dit.flat_buffers()
        bufs = [f["p"], self.opt.m, self.opt.v] + ([self.opt.ema] if self.opt.ema is not None else []) + list(self.opt.posthoc)
        if getattr(self.opt, "adapter", None) is not None:
            bufs.append(self.opt.adapter.w)
        if self.loss_weighting is not None:
            lw = self.loss_weighting
            bufs += [lw.freq, lw.phase, lw.w, lw.m, lw.v]
        for t in bufs:
            if self.sync.torch_bounce:
                h = t.cpu()
                dist.broadcast(h, src=0, group=self.sync.pg)
                t.copy_(h)
            else:
                dist.broadcast(t, src=0, group=self.sync.pg)
        self.model.dit.refresh_shadow(force=True)

    def replicas_in_sync(self) -> bool:
        """True when the weights of all ranks are bit-identical: an EXACT integer checksum (md_checksum_u16: sum of the bf16 bit
        patterns and an index-weighted sum, per data-parallel bucket) of the bf16 shadow every rank computes with (under the
        sharded optimiser the fp32 masters of foreign chunks are deliberately stale), compared across ranks by MIN / MAX
        all-reduces of the int64 sums.  One bf16 ulp in one weight, a sign flip or a permutation changes it (the fp32 sum of
        squares used before resolved only ~4e-3 of a bucket's 1e8 weights: ADVICE r4).  One bandwidth pass over 2.3 GB."""
        if self.world <= 1:
            return True
        self.sync.wait_gather()
        f = self.model.dit.flat_buffers()
        L, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        mine = torch.zeros(len(self.sync.bucket_list), 2, device=f["s"].device, dtype=torch.int64)
        for i, (_, blo, bhi) in enumerate(self.sync.bucket_list):
            n = (bhi - blo) // 8 * 8             # buckets start on 1024-element boundaries; a ragged end (none today) is left to the next check
            hip.check(L.md_checksum_u16(f["s"].data_ptr() + 2 * blo, n, mine.data_ptr() + 16 * i, st), "md_checksum_u16")
        mine = mine.reshape(-1)
        if self.loss_weighting is not None:      # the C weights of u(sigma): their fp32 bit patterns ride along in the same comparison
            mine = torch.cat([mine, self.loss_weighting.w.view(torch.int32).to(torch.int64)])
        lo, hi = mine.clone(), mine.clone()
        if self.sync.torch_bounce:
            lo, hi = lo.cpu(), hi.cpu()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.sync.pg)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.sync.pg)
        return bool(torch.equal(lo, hi))

    def throughput(self, global_batch: int, window: int = 3) -> Optional[float]:
        """Composer SpeedMonitor(window_size=3) definition: samples over the last `window` batches / wall time."""
        torch.cuda.synchronize()
        self._win.append((time.time(), self.batches_seen))
        self._win = self._win[-(window + 1):]
        if len(self._win) < 2:
            return None
        (t0, b0), (t1, b1) = self._win[0], self._win[-1]
        return (b1 - b0) * global_batch / max(t1 - t0, 1e-9)
