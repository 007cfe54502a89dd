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
    the weights / moments (optim.FusedAdamW.step_sharded, one launch over a range table) and the fresh bf16 weights are all-gathered
    bucket by bucket under the next forward (gradsync.GradSync; `dp_mode="allreduce"` keeps the all-reduce form where every rank runs
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

import contextlib
import os
import math
import re
import time
from typing import Callable, Dict, List, Optional

import torch
import torch.distributed as dist

from . import hip
from . import diagnostics as mddiag
from .disperse import DisperseLoss
# (GradSync and its helpers, and FusedAdamW, are re-exported: bench.py, train.py, the scripts and the tests import them from here)
from .gradsync import RCCL_CHANNELS_DEFAULT, GradSync, cap_rccl_channels, rccl_channel_cap, shard_plan     # noqa: F401
from .loss_weighting import LossWeighting
from .optim import FusedAdamW, Optimizer     # noqa: F401


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
        L, st = hip.lib(), hip.stream_ptr()
        pf, pi = self.part_f, self.part_i
        for buf, is_bf16, first, n in self.sources:
            hip.check(L.md_tensor_stats_partial(buf.data_ptr(), is_bf16, self.items.data_ptr() + 16 * first, n,
                                                pf[0].data_ptr() + 4 * first, pf[1].data_ptr() + 4 * first, pi.data_ptr() + 4 * first, st),
                      "md_tensor_stats_partial")
        hip.check(L.md_tensor_stats_finish(pf[0].data_ptr(), pf[1].data_ptr(), pi.data_ptr(), self.item_begin.data_ptr(), self.n_tensors,
                                           self.out_f[0].data_ptr(), self.out_f[1].data_ptr(), self.out_i.data_ptr(), st),
                  "md_tensor_stats_finish")
        return self.out_f, self.out_i


class Trainer:
    def __init__(self, model, optimizer: Optimizer, schedule: Optional[LRSchedule] = None, clip_norm: float = 0.0,
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
        self.model, self.opt, self.schedule, self.clip_norm = model, optimizer, schedule, clip_norm
        self.microbatch_size = microbatch_size
        if dp_mode == "auto" and os.environ.get("MD_DP_MODE"):
            dp_mode = os.environ["MD_DP_MODE"]
        if exchange == "auto" and os.environ.get("MD_DP_EXCHANGE"):
            exchange = os.environ["MD_DP_EXCHANGE"]
        if transport == "auto":                # MD_COMM=native: the exchange through libmicrodit_comm.so instead of torch.distributed
            transport = os.environ.get("MD_COMM", "torch")
        adapter = optimizer.adapter
        # a factored LoRA adapter: the base's gradient does not exist; what the ranks exchange is adapter.g, one all-reduce
        self.lora_factored = adapter is not None and adapter.backward == "factored"
        # muon.Muon: orthogonalises whole matrices, a rank of the sharded step owns slices; factored LoRA: nothing of the base's to shard
        if not optimizer.shardable or self.lora_factored:
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
        on_rccl = self.sync.comm is not None or not self.sync.host_bounce
        self.rccl_channels = rccl_channel_cap() if (self.sync.enabled and self.world > 1 and on_rccl) else 0
        if self.rccl_channels:
            lim = hip.NUM_CU - self.rccl_channels
            model.dit.engine.cu_limit_fn = lambda s=self.sync, lim=lim: (lim if s.in_flight() else 0)
        model.dit.engine.before_segment = self.sync.wait_gather if self.sharded else None
        # the Trainer runs forward -> backward strictly in turn: activations may live in the engine's fixed-address arenas
        model.dit._ensure_flat()
        model.dit.engine.use_arena = True
        self._device = model.dit.flat_buffers()["p"].device
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
        model, sync, eng = self.model, self.sync, self.model.dit.engine
        n = batch[model.image_latents_key if model.image_latents_key in batch else model.image_key].shape[0]
        mb = min(self.microbatch_size, n)
        starts = list(range(0, n, mb))
        eng.wgrad_bf16 = None                # (a step that raised must not have left the bf16 store armed: last_microbatch disarms it)
        total = self._fresh_zeros(1)         # a fresh scalar per step: callers keep them
        lw = self.loss_weighting
        if lw is not None:                   # the step's rank-mean weighted objective
            lw.objective_accum = self._objective = self._fresh_zeros(1)
        if self.disperse is not None:        # the step's (L_disp, mean off-diagonal D), microbatches weighted like the loss
            model.disperse_accum = self._disperse_acc = self._fresh_zeros(2)
        if (self._route_stats is not None and self.diagnostics_interval > 0
                and (self.batches_seen + 1) % self.diagnostics_interval == 0):
            self._route_stats.zero()
            eng.route_stats = self._route_stats
        try:
            for i, s in enumerate(starts):
                part = {k: (v[s:s + mb] if torch.is_tensor(v) and v.shape[0] == n else v) for k, v in batch.items()}
                w = min(mb, n - s) / n
                last = i == len(starts) - 1
                with sync.last_microbatch(single_microbatch=(len(starts) == 1)) if last else contextlib.nullcontext():
                    model.train_microbatch(part, grad_scale=w, loss_accum=total, accum_weight=w)
        finally:
            if self._route_stats is not None:
                eng.route_stats = None
        with self._timed(self._comm_events):             # from behind the last backward kernel on the compute stream to behind the
            slots = sync.finish()                        # waits on the collectives / side-stream norms
        if lw is not None and self.world > 1:
            self._reduce(lw.g)
        if self.lora_factored and self.world > 1:
            self._reduce(self.opt.adapter.g)
        if self.monitor_interval > 0 and (self.batches_seen + 1) % self.monitor_interval == 0:
            self.collect_tensor_stats()                  # reads the gradients the optimiser pass is about to consume and clear
        fac = self.schedule.factor(self.batches_seen) if self.schedule is not None else 1.0
        with self._timed(self._opt_events):              # norm finish + AdamW (+ the launch of the weight all-gathers)
            if self.sharded:
                self.opt.step_sharded(sync, lr=self.opt.lr * fac, max_norm=self.clip_norm, grad_scale=1.0 / self.world,
                                      norm_slots=slots, chunk_of=self.shard_chunk_of)
                self.stale_foreign_chunks = self.world > 1
                self.model.dit.shadow_is_authoritative = self.stale_foreign_chunks
            else:
                self.opt.step(lr=self.opt.lr * fac, max_norm=self.clip_norm, grad_scale=1.0 / self.world,
                              g_bf16=sync.gbf, norm_partials=slots * hip.SUMSQ_PARTIALS)
            if lw is not None:               # behind the main pass: its guard flag (skip_nonfinite) is set by now
                lw.step((self.opt.lr if lw.lr is None else lw.lr) * fac, grad_scale=1.0 / self.world, guard_state=self.opt.guard_state)
        self.batches_seen += 1
        return total.reshape(())

    def _fresh_zeros(self, n: int) -> torch.Tensor:
        """A new fp32 device buffer of n zeros, filled by a launch of ours (no torch kernel on the step path)."""
        t = torch.empty(n, device=self._device)
        hip.check(hip.lib().md_fill_zero(t.data_ptr(), 4 * n, hip.stream_ptr()), "md_fill_zero")
        return t

    @contextlib.contextmanager
    def _timed(self, events: list):
        """With measure_comm (bench.py): an event pair around the body on the compute stream, appended to `events`."""
        if not self.measure_comm:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        events.append((e0, e1))

    @staticmethod
    def _mean_ms(events: list, last: int) -> Optional[float]:
        if not events:
            return None
        torch.cuda.synchronize()
        ev = events[-last:] if last > 0 else events
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev)

    def _reduce(self, buf: torch.Tensor) -> None:
        """One fp32 all-reduce (sum) of a small gradient buffer next to the main exchange -- the C values of u(sigma), a factored LoRA
        adapter's gradient -- on the trainer's process group, the same in every exchange mode and transport; the 1 / world factor goes
        into the AdamW launch's grad_scale as for the other gradients.  A sum of `world` addends per element: every rank receives the
        same bits, so replicas that start identical stay identical."""
        self.sync.all_reduce_now(buf)

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
                self.sync.all_reduce_now(table.view(-1))
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
                self.sync.all_reduce_now(obj)
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
        return self._mean_ms(self._comm_events, last)

    def consolidate(self) -> None:
        """Sharded optimiser only: all-gather the fp32 masters, both moments, the EMA and the post-hoc EMA profiles so that every rank
        holds the whole, current state (checkpoints, snapshots, evaluation on EMA weights, state_dict()).  A collective: every rank must
        call it.  Not on the step path (3 x 4.66 GB for XL/2, one more per average; at checkpoint / evaluation / snapshot intervals)."""
        if not self.sharded or not self.stale_foreign_chunks:
            return
        s = self.sync
        s.wait_gather()
        for t in [self.model.dit.flat_buffers()["p"]] + self.opt.state_buffers():
            for key, lo, hi, chunk, olo in s.plan:
                s.all_gather_now(t[lo:hi], t[lo + s.rank * chunk: lo + (s.rank + 1) * chunk].clone())
        self.stale_foreign_chunks = False
        self.model.dit.shadow_is_authoritative = False

    def optimizer_ms(self, last: int = 0) -> Optional[float]:
        """Mean compute-stream time per step of the gradient-norm finish + AdamW pass (needs measure_comm; synchronises)."""
        return self._mean_ms(self._opt_events, last)

    def sync_replicas(self) -> None:
        """Make every rank's weights and optimiser state bit-identical to rank 0's (call once after initialisation / resume).
        Data parallelism here replicates the weights and relies on identical updates from then on; nothing else would catch a
        replica that started from a different state."""
        if self.world <= 1:
            return
        self.consolidate()          # after a sharded step rank 0's masters of foreign chunks are stale: make them whole first
        bufs = [self.model.dit.flat_buffers()["p"]] + self.opt.state_buffers()
        if self.opt.adapter is not None:
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
        L, st = hip.lib(), hip.stream_ptr()
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
