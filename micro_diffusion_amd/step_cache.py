"""Step cache: reuse the backbone's contribution to the residual stream across the network evaluations of a sampling
run (the Delta-DiT / FORA / TeaCache family).  A full evaluation runs every block and leaves delta = backbone output - backbone input
in an engine.ResidualCache; a reused evaluation runs the embeddings, the patch mixer, one add of that delta and the final layer.

This module is the policy -- which evaluations are full -- and the public argument `step_cache=StepCache(...)` of
LatentDiffusion.edm_sampler_loop / generate.  The decision logic is pure Python: importable and testable without a GPU.

Evaluation e of N (counted by the sampler loop from its own schedule) is FULL when
    e < warmup,  or  e >= N - tail,  or  the cache is not valid for this evaluation's batch, token count and weight version
(the last also covers the switch between batch B and 2B at the edge of a guidance interval); otherwise the policy decides:
    interval=k    full iff e - e_last_full >= k                       (FORA's fixed schedule; k = 1 never reuses)
    threshold=d   acc += rel_max_e;  full iff acc >= d, then acc = 0  (TeaCache's rule on the raw distance)
rel_max_e is the largest per-sample relative L1 distance of the backbone's input from the previous evaluation's (md_step_probe).  It
is used as measured: TeaCache's per-model polynomial rescaling of the distance is not applied, and there is no default threshold --
nobody has tuned one for MicroDiT.  The adaptive policy reads that one 4-byte scalar on the host in every evaluation: one host wait
per evaluation; the fixed policy reads nothing back.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence


@dataclass
class StepCacheStats:
    """evaluations = full + reused; decisions[e] is True where evaluation e was full; distances[e] is the probe's rel_max of evaluation e
    (None: fixed policy, or the probe only filled its reference)."""
    evaluations: int = 0
    full: int = 0
    reused: int = 0
    decisions: List[bool] = field(default_factory=list)
    distances: List[Optional[float]] = field(default_factory=list)


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


class StepCache:
    """StepCache(interval=k) or StepCache(threshold=d): exactly one of the two.  warmup >= 1 leading and tail >= 0 trailing evaluations
    are always full.  blocks = (lo, hi): the backbone blocks covered (None: all of them).  `stats` describes the last run."""

    def __init__(self, interval: Optional[int] = None, threshold: Optional[float] = None, warmup: int = 1, tail: int = 1, blocks=None):
        if (interval is None) == (threshold is None):
            raise ValueError("StepCache takes exactly one of interval= (fixed schedule) and threshold= (adaptive)")
        if interval is not None and (not _is_int(interval) or interval < 1):
            raise ValueError(f"interval must be an integer >= 1, got {interval!r}")
        if threshold is not None:
            try:
                ok = not isinstance(threshold, (bool, str)) and float(threshold) >= 0.0        # (NaN fails the comparison)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"threshold must be a number >= 0, got {threshold!r}")
            threshold = float(threshold)
        if not _is_int(warmup) or warmup < 1:
            raise ValueError(f"warmup must be an integer >= 1 (the first evaluation has nothing to reuse), got {warmup!r}")
        if not _is_int(tail) or tail < 0:
            raise ValueError(f"tail must be an integer >= 0, got {tail!r}")
        if blocks is not None:
            if len(tuple(blocks)) != 2 or not all(_is_int(v) for v in blocks) or not 0 <= blocks[0] < blocks[1]:
                raise ValueError(f"blocks must be (lo, hi) with 0 <= lo < hi, backbone block indices, got {blocks!r}")
            blocks = (blocks[0], blocks[1])
        self.interval, self.threshold, self.warmup, self.tail, self.blocks = interval, threshold, warmup, tail, blocks
        self.stats = StepCacheStats()
        self._n = 0
        self._last_full = None
        self._acc = 0.0
        self._rc = None                             # the engine.ResidualCache of the run (created on a GPU run)

    @property
    def adaptive(self) -> bool:
        return self.threshold is not None

    # ------------------------------------------------------------------------------------------ the policy (pure Python)
    def reset(self, evaluations: int = 0) -> None:
        """Start of a sampler run of `evaluations` network evaluations: fresh stats, no accumulated distance, an empty cache."""
        if not _is_int(evaluations) or evaluations < 0:
            raise ValueError(f"evaluations must be an integer >= 0, got {evaluations!r}")
        self.stats = StepCacheStats()
        self._n, self._last_full, self._acc = evaluations, None, 0.0
        if self._rc is not None:
            self._rc.reset()

    def step(self, valid: bool = True, distance: Optional[float] = None) -> bool:
        """Decide the next evaluation and record it: True = full, False = reused.  valid: whether the cache holds a delta for this
        evaluation's batch, token count and weight version.  distance: the probe's rel_max (adaptive policy; None when the probe only
        filled its reference, which makes the evaluation full)."""
        s, e = self.stats, self.stats.evaluations
        forced = e < self.warmup or e >= self._n - self.tail or not valid       # (warmup >= 1: evaluation 0 sets _last_full)
        if self.adaptive:
            if distance is None:
                forced = True
            else:
                self._acc += float(distance)
            full = forced or not self._acc < self.threshold       # (a NaN distance is never "close")
        else:
            full = forced or e - self._last_full >= self.interval
        if full:
            self._last_full, self._acc = e, 0.0
        s.evaluations += 1
        s.full += int(full)
        s.reused += int(not full)
        s.decisions.append(bool(full))
        s.distances.append(None if distance is None or not self.adaptive else float(distance))
        return full

    def plan(self, evaluations: int, valid: Optional[Sequence[bool]] = None, distances: Optional[Sequence[Optional[float]]] = None) -> StepCacheStats:
        """The stats of a run of `evaluations` evaluations under this policy, without running anything: valid[e] (default: always) and,
        for the adaptive policy, distances[e] are what evaluation e would see."""
        p = StepCache(self.interval, self.threshold, self.warmup, self.tail, self.blocks)
        p.reset(evaluations)
        for e in range(evaluations):
            p.step(True if valid is None else bool(valid[e]), None if distances is None else distances[e])
        return p.stats

    # ------------------------------------------------------------------------------------------ the sampler's side
    def engine_args(self, engine, B: int) -> dict:
        """step_cache= and reuse= of DiTEngine.forward for the next evaluation at network batch B.  The callback runs at the engine's
        decision point, between the mixer and the backbone; the adaptive policy's host read of rel_max happens there."""
        if self._rc is None:
            from .engine import ResidualCache
            self._rc = ResidualCache(self.blocks, probe=self.adaptive)
        rc = self._rc

        def reuse(rel_max):
            d = None
            if self.adaptive and rel_max is not None:
                d = float(rel_max.item())           # the one host wait of an adaptive evaluation
                if math.isnan(d):
                    d = float("inf")
            return not self.step(rc.valid(B, engine.cfg.tokens, engine.weights_version), d)
        return {"step_cache": rc, "reuse": reuse}
