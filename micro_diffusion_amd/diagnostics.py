"""Model diagnostics (opt-in): the EDM loss split by noise level and the state of the expert-choice routers.

  LossBySigma   two tables (train / eval) of `nbins` bins over ln sigma; `LatentDiffusion.loss_by_sigma` (None = off).  One
                md_loss_sigma_hist launch behind every md_edm_loss(_train) adds the microbatch's per-sample losses to the table chosen
                by dit.training.
  RouteStats    one row per routed layer (block name, forward order); `DiTEngine.route_stats` (None = off).  One md_moe_route_stats
                call behind every md_moe_route adds the layer's token coverage, router entropy, router marginals and gate sums.

Both own their buffers (plain torch allocations: nothing comes from the engine's arenas, nothing goes on the tape) and only enqueue;
`Trainer.diagnostics()` reads (and synchronises).  The device tables hold integer counts and fp64 sums; ranks are combined by gathering every rank's tables and
adding them in RANK ORDER on every rank (combine_rank_diagnostics): identical bits everywhere, no floating all-reduce.  The functions
that turn tables into the logged keys are pure host code.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import hip

MAX_BINS = 64        # md_loss_sigma_hist: one lane per bin
SIGMA_RANGE_STDS = 3.0


def sigma_bin_range(p_mean: float, p_std: float, log_lo: Optional[float] = None, log_hi: Optional[float] = None) -> Tuple[float, float]:
    """ln sigma range of the histogram: P_mean +- 3 P_std of the log-normal the training sigmas are drawn from (99.7 % of the
    samples; the rest lands in the end bins) unless overridden."""
    lo = p_mean - SIGMA_RANGE_STDS * p_std if log_lo is None else float(log_lo)
    hi = p_mean + SIGMA_RANGE_STDS * p_std if log_hi is None else float(log_hi)
    if not hi > lo:
        raise ValueError(f"empty ln sigma range [{lo}, {hi}]")
    return lo, hi


def sigma_bin_edges(log_lo: float, log_hi: float, nbins: int) -> List[float]:
    """The nbins + 1 edges of the bins in ln sigma (bin b = [edge b, edge b + 1); the end bins also take what lies outside)."""
    return [log_lo + (log_hi - log_lo) * b / nbins for b in range(nbins)] + [log_hi]


def combine_rank_diagnostics(counts: torch.Tensor, sums: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """counts int64 [world, N], sums float64 [world, K] (rank r's tables at index r) -> (counts [N], sums [K]) of all ranks.  The
    sums are added in RANK ORDER starting from rank 0's: every rank that holds the same gathered tables gets the same bits (the idea
    of trainer.combine_rank_tables).  Integer counts are exact in any order."""
    if counts.dtype != torch.int64 or sums.dtype != torch.float64 or counts.shape[0] != sums.shape[0]:
        raise ValueError("combine_rank_diagnostics takes int64 counts and float64 sums with one leading rank dimension")
    c, s = counts[0].clone(), sums[0].clone()
    for r in range(1, counts.shape[0]):
        c += counts[r]
        s += sums[r]
    return c, s


def gather_rank_diagnostics(counts: torch.Tensor, sums: torch.Tensor, group=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """This rank's tables (int64 [N], float64 [K]) -> the combined tables of the process group, on the host, identical on every rank.
    ONE all-gather of the tables' bits (the sums travel as int64 words: no arithmetic on the wire), then combine_rank_diagnostics.
    Without a process group (or with one rank) the tables come back as they are.  A collective: every rank calls it."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return counts.cpu(), sums.cpu()
    world = dist.get_world_size(group)
    N = counts.numel()
    mine = torch.cat([counts.reshape(-1), sums.reshape(-1).view(torch.int64)])
    if dist.get_backend(group) == "nccl":
        out = torch.empty(world * mine.numel(), device=mine.device, dtype=torch.int64)
        dist.all_gather_into_tensor(out, mine, group=group)
        allr = out.cpu().view(world, -1)
    else:                                   # gloo: host tensors
        mine = mine.cpu()
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        allr = torch.stack(parts)
    return combine_rank_diagnostics(allr[:, :N].contiguous(), allr[:, N:].contiguous().view(torch.float64))


def format_loss_by_sigma(which: str, edges: Sequence[float], sums, counts, nonfinite: int) -> Dict[str, object]:
    """Logged keys of one loss-by-sigma table: loss_by_sigma/<which>/ln_sigma_edges [nbins + 1], /count [nbins], /mean_loss [nbins]
    (None for an empty bin), /nonfinite (samples whose loss was not finite: in no bin)."""
    sums, counts = [float(v) for v in sums], [int(v) for v in counts]
    pre = f"loss_by_sigma/{which}/"
    return {pre + "ln_sigma_edges": [float(e) for e in edges], pre + "count": counts,
            pre + "mean_loss": [s / c if c > 0 else None for s, c in zip(sums, counts)], pre + "nonfinite": int(nonfinite)}


def format_route_stats(block: str, cover_hist, fstats) -> Dict[str, object]:
    """Logged keys of one routed layer from its accumulated row (cover_hist [E + 1], fstats [1 + 2 E]):
      moe/<block>/coverage          [E + 1]: fraction of the tokens taken by exactly c experts, c = 0 .. E
      moe/<block>/dropped_frac      = coverage[0]: tokens no expert picked (they pass through the residual alone)
      moe/<block>/router_entropy    mean over tokens of -sum_e p ln p, nats (ln E = uniform router, 0 = collapsed)
      moe/<block>/expert_prob_mean  [E]: router marginal, mean over tokens of p_e (sums to 1)
      moe/<block>/expert_gate_mean  [E]: mean gate value of the entries expert e chose
    {} for a row nothing was added to."""
    hist = [int(v) for v in cover_hist]
    f = [float(v) for v in fstats]
    E = len(hist) - 1
    if len(f) != 1 + 2 * E:
        raise ValueError(f"fstats has {len(f)} entries, expected {1 + 2 * E} for {E} experts")
    tokens = sum(hist)
    if tokens == 0:
        return {}
    chosen = sum(c * h for c, h in enumerate(hist)) / E        # entries per expert: B * k of every microbatch
    pre = f"moe/{block}/"
    cov = [h / tokens for h in hist]
    return {pre + "coverage": cov, pre + "dropped_frac": cov[0], pre + "router_entropy": f[0] / tokens,
            pre + "expert_prob_mean": [v / tokens for v in f[1:1 + E]],
            pre + "expert_gate_mean": [v / chosen if chosen > 0 else None for v in f[1 + E:]]}


class LossBySigma:
    """The train / eval loss-by-sigma tables.  Device layout of one table: int64 [nbins + 1] = [count per bin | non-finite samples],
    float64 [nbins] = loss sum per bin (allocated at the first launch, on the device of its inputs)."""

    TABLES = ("train", "eval")

    def __init__(self, nbins: int, p_mean: float = -0.6, p_std: float = 1.2, log_lo: Optional[float] = None, log_hi: Optional[float] = None):
        if not 1 <= int(nbins) <= MAX_BINS:
            raise ValueError(f"loss-by-sigma bins must be 1 .. {MAX_BINS}, got {nbins}")
        self.nbins = int(nbins)
        self.log_lo, self.log_hi = sigma_bin_range(p_mean, p_std, log_lo, log_hi)
        self.edges = sigma_bin_edges(self.log_lo, self.log_hi, self.nbins)
        self._tab: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}

    def _tables(self, which: str, device=None):
        if which not in self._tab:
            if which not in self.TABLES:
                raise KeyError(which)
            if device is None:
                return None
            self._tab[which] = (torch.zeros(self.nbins + 1, device=device, dtype=torch.int64),
                                torch.zeros(self.nbins, device=device, dtype=torch.float64))
        return self._tab[which]

    def accumulate(self, sigma: torch.Tensor, loss_per_sample: torch.Tensor, training: bool) -> None:
        """One md_loss_sigma_hist launch on the current stream: sigma / loss_per_sample f32 [B] as md_edm_prepare / md_edm_loss leave them."""
        cnt, sm = self._tables("train" if training else "eval", sigma.device)
        hip.check(hip.lib().md_loss_sigma_hist(sigma.data_ptr(), loss_per_sample.data_ptr(), sigma.numel(), self.log_lo, self.log_hi,
                                               self.nbins, sm.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 8 * self.nbins,
                                               hip.stream_ptr()), "md_loss_sigma_hist")

    def zero(self, which: Optional[str] = None) -> None:
        for w in (self.TABLES if which is None else (which,)):
            t = self._tables(w)
            if t is not None:
                t[0].zero_()
                t[1].zero_()

    def tables(self, which: str, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(int64 [nbins + 1], float64 [nbins]) device tables of `which` (created empty when nothing was accumulated yet)."""
        return self._tables(which, device)


class RouteStats:
    """Routing statistics of every routed layer of an engine: cover_hist int64 [n_layers, E + 1] and fstats float64
    [n_layers, 1 + 2 E], rows in forward order (`names`: patch_mixer.N, blocks.N), plus the float workspace of md_moe_route_stats,
    sized once per (B, S) through md_moe_route_stats_ws_floats."""

    def __init__(self, engine):
        self.names = [bp.name for bp in list(engine.mixer) + list(engine.backbone) if bp.moe]
        if not self.names:
            raise ValueError("this model has no expert-choice layer to monitor")
        self.row = {n: i for i, n in enumerate(self.names)}
        self.E = E = int(engine.cfg.num_experts)
        self.dev = engine.dev
        self.cover_hist = torch.zeros(len(self.names), E + 1, device=self.dev, dtype=torch.int64)
        self.fstats = torch.zeros(len(self.names), 1 + 2 * E, device=self.dev, dtype=torch.float64)
        self._ws: Dict[Tuple[int, int], torch.Tensor] = {}

    def workspace(self, B: int, S: int) -> torch.Tensor:
        ws = self._ws.get((B, S))
        if ws is None:
            n = ctypes.c_int64(0)
            hip.check(hip.lib().md_moe_route_stats_ws_floats(B, S, self.E, ctypes.byref(n)), "md_moe_route_stats_ws_floats")
            ws = self._ws[(B, S)] = torch.empty(int(n.value), device=self.dev, dtype=torch.float32)
        return ws

    def record(self, name: str, slot: torch.Tensor, probs: torch.Tensor, ldp: int, gval: torch.Tensor, B: int, S: int, k: int) -> None:
        """Add one layer's routing of one microbatch to its row (enqueues md_moe_route_stats on the current stream)."""
        r = self.row[name]
        ws = self.workspace(B, S)
        hip.check(hip.lib().md_moe_route_stats(slot.data_ptr(), probs.data_ptr(), ldp, gval.data_ptr(), B, S, self.E, k, ws.data_ptr(),
                                               ws.numel(), self.cover_hist[r].data_ptr(), self.fstats[r].data_ptr(), hip.stream_ptr()),
                  "md_moe_route_stats")

    def zero(self) -> None:
        self.cover_hist.zero_()
        self.fstats.zero_()
