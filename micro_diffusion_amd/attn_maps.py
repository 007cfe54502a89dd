"""Cross-attention maps: which caption position does each image token attend to?  Every mixer and backbone block runs a
cross-attention over the caption tokens; the fused md_attn_fwd never materialises its probabilities, so an armed recorder recomputes
them -- averaged over the heads -- from the normalised q and k that attention just read (md_attn_probs, one launch per block and
evaluation, no host wait) and adds them into a buffer of its own.  The recorder only reads: the latents of a run with it are the bits
of the run without.

This module is the policy -- which blocks, which noise levels -- the recorder the engine calls (`DiTEngine.attn_probe`), and the
read-out in plain torch, and the public argument `attn_maps=AttentionMaps(...)` of LatentDiffusion.edm_sampler_loop / generate.
Everything but `record` runs without a GPU.

    am = AttentionMaps(blocks=r"blocks\\.(8|9|10)$", sigma_range=(0.3, 5.0))
    latents = model.edm_sampler_loop(x, y, cfg=5.0, attn_maps=am)
    am.token_mass()                  # [n_selected, Lc]: the share of attention on each caption position (padding included: the softmax
                                     # runs over all of them, attention_mask reaches the text encoder only)
    m = am.mask(tokens=[4, 5], quantile=0.8, dilate=1)            # [B, 1, H, W], 1 = generate: an inpaint_mask
    edited = model.edm_sampler_loop(x2, y2, cfg=5.0, init_latents=latents, inpaint_mask=m)

State of a run: one fp32 buffer [n_selected, B, T, ldo] (ldo = Lc rounded up to 4), allocated at the first record and zeroed at the start
of every run, and a per-block record count on the host; blocks a reused step-cache evaluation skips simply count less.  Only the first B
samples of an evaluation are recorded: in a batch-doubled guided evaluation that is the conditional half, which the sampler puts
first.  A `guide=` network is not recorded.  Mapping words to caption positions stays the caller's job (the tokenizer is third-party).

Armed directly on an engine (`am.arm(engine)` ... `am.disarm(engine)`, diagnostics) every forward of that engine is recorded until
`start_run()` clears the state.  In a masked pass (mask_ratio > 0) the mixer blocks see all T tokens and the backbone blocks the kept
ones, whose rows are scattered through keep_rows: the rows of dropped tokens stay 0 in backbone blocks (and token_mass of such a block
sums to the kept fraction).
"""
from __future__ import annotations

import math
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as Fnn

BlockSelection = Union[None, str, Iterable[str]]


def block_names(cfg) -> List[str]:
    """The names of every mixer and backbone block of a DiTConfig, in forward order ("patch_mixer.0" ..., "blocks.0" ...)."""
    from .arch import plan_blocks
    mixer, backbone = plan_blocks(cfg)
    return [bp.name for bp in list(mixer) + list(backbone)]


def select_blocks(names: Sequence[str], blocks: BlockSelection) -> List[str]:
    """The entries of `names` the selection keeps, in the order of `names`.  None: all of them; a string: one regular expression
    (re.search on the name, the convention of lora_targets); any other iterable: block names.  ValueError for a name that is no block
    and for a selection that keeps nothing."""
    names = list(names)
    if blocks is None:
        chosen = names
    elif isinstance(blocks, str):
        try:
            pat = re.compile(blocks)
        except re.error as e:
            raise ValueError(f"blocks: {blocks!r} is not a regular expression ({e})") from None
        chosen = [n for n in names if pat.search(n)]
    else:
        try:
            want = list(blocks)
        except TypeError:
            raise ValueError(f"blocks must be None, a regular expression or an iterable of block names, got {blocks!r}") from None
        for w in want:
            if not isinstance(w, str) or w not in names:
                raise ValueError(f"blocks: {w!r} is not a block of this model (blocks: {', '.join(names)})")
        chosen = [n for n in names if n in want]
    if not chosen:
        raise ValueError(f"blocks={blocks!r} selects no block of this model (blocks: {', '.join(names)})")
    return chosen


def _check_sigma_range(sigma_range) -> Optional[Tuple[float, float]]:
    if sigma_range is None:
        return None
    try:
        lo, hi = sigma_range
        ok = not any(isinstance(v, (bool, str)) for v in (lo, hi))
        lo, hi = float(lo), float(hi)
        ok = ok and math.isfinite(lo) and math.isfinite(hi) and lo <= hi
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"sigma_range must be (lo, hi), two finite numbers with lo <= hi, got {sigma_range!r}")
    return lo, hi


class AttentionMaps:
    """AttentionMaps(blocks=None, sigma_range=None).  blocks: None = every mixer and backbone block, an iterable of block names
    ("patch_mixer.0", "blocks.12") or one regular expression.  sigma_range = (lo, hi): only evaluations at lo <= sigma <= hi are
    recorded; None: all of them."""

    def __init__(self, blocks: BlockSelection = None, sigma_range=None):
        if blocks is not None and not isinstance(blocks, str):
            try:
                blocks = tuple(blocks)
            except TypeError:
                raise ValueError(f"blocks must be None, a regular expression or an iterable of block names, got {blocks!r}") from None
            if not blocks or not all(isinstance(b, str) for b in blocks):
                raise ValueError(f"blocks must name at least one block, each by a string, got {blocks!r}")
        elif isinstance(blocks, str):
            try:
                re.compile(blocks)
            except re.error as e:
                raise ValueError(f"blocks: {blocks!r} is not a regular expression ({e})") from None
        self.blocks = blocks
        self.sigma_range = _check_sigma_range(sigma_range)
        self.names: List[str] = []                  # the selected blocks of the model the recorder was resolved against, forward order
        self.row: Dict[str, int] = {}
        self.buf: Optional[torch.Tensor] = None     # fp32 [n_selected, B, T, ldo]: the sums
        self.Lc = 0
        self.tokens = 0                             # T of the full grid
        self.grid: Optional[Tuple[int, int]] = None # (h, w) of the token grid, h * w == T
        self.patch_size = 1
        self._counts: List[int] = []
        self._active = True                         # whether the evaluation under way is inside sigma_range
        self._eval_B: Optional[int] = None          # samples of it to record (None: all)

    # ------------------------------------------------------------------------------------------ policy (no GPU)
    def resolve(self, cfg, grid: Optional[Tuple[int, int]] = None) -> List[str]:
        """Select the blocks of a model (its DiTConfig) and take its token grid; ValueError when the selection matches none.  A model
        with another selection or grid drops the recorded state."""
        names = select_blocks(block_names(cfg), self.blocks)
        if grid is None:
            g = int(cfg.input_size) // int(cfg.patch_size)
            grid = (g, g)
        grid = (int(grid[0]), int(grid[1]))
        if grid[0] * grid[1] != int(cfg.tokens):
            raise ValueError(f"the token grid {grid[0]} x {grid[1]} does not hold the model's {cfg.tokens} tokens")
        if names != self.names or grid != self.grid or int(cfg.patch_size) != self.patch_size:
            self.buf = None
        self.names, self.row = names, {n: i for i, n in enumerate(names)}
        self.tokens, self.grid, self.patch_size = int(cfg.tokens), grid, int(cfg.patch_size)
        if len(self._counts) != len(names):
            self._counts = [0] * len(names)
        return names

    def start_run(self) -> None:
        """Start of a run: zero sums and counts; every evaluation is recorded whole until begin_evaluation says otherwise."""
        if self.buf is not None:
            self.buf.zero_()
        self._counts = [0] * len(self.names)
        self._active, self._eval_B = True, None

    def wants(self, sigma) -> bool:
        r = self.sigma_range
        return r is None or sigma is None or r[0] <= float(sigma) <= r[1]

    def begin_evaluation(self, sigma, B: Optional[int]) -> None:
        """The sampler, before each evaluation of the main network: its noise level (None: not known, recorded) and the number of
        leading samples to record (the conditional half of a doubled batch)."""
        self._active, self._eval_B = self.wants(sigma), None if B is None else int(B)

    def arm(self, engine, grid: Optional[Tuple[int, int]] = None) -> "AttentionMaps":
        """Resolve against the engine's model, clear the state and become the engine's attn_probe."""
        self.resolve(engine.cfg, grid)
        self.start_run()
        engine.attn_probe = self
        return self

    @staticmethod
    def disarm(engine) -> None:
        engine.attn_probe = None

    def skip_evaluation(self) -> None:
        """The sampler, before a forward that is not the main network's (a guide that shares the engine): not recorded."""
        self._active = False

    # ------------------------------------------------------------------------------------------ the engine's side
    def record(self, name: str, ax, B: int, S: int, Lc: int, out_rows=None, kbias=None) -> None:
        """Behind the cross-attention of block `name`: add its head-averaged probabilities to the block's rows.  ax: the hip.AttnArgs
        attention ran with (both q / k layouts); B, S, Lc: samples, query rows per sample, caption positions; out_rows: int32 [B * S]
        rows of the full grid (a masked pass's keep_rows) or None when S is the full grid; kbias: the engine's caption_bias (fp32
        [>= B, ldb]) when attention ran with one -- the probabilities are then the biased ones, a removed position
        records exactly 0.  One launch on the current stream."""
        r = self.row.get(name)
        if r is None or not self._active:
            return
        from ctypes import byref
        from . import hip
        nb = B if self._eval_B is None else min(B, self._eval_B)
        if out_rows is None and S != self.tokens:
            raise RuntimeError(f"attn_maps: block {name} ran on {S} rows per sample, the grid has {self.tokens}, and no row table was given")
        ldo = (Lc + 3) // 4 * 4
        if self.buf is None:
            self.buf = torch.zeros(len(self.names), nb, self.tokens, ldo, device=torch.device("cuda", torch.cuda.current_device()),
                                   dtype=torch.float32)
            self.Lc = Lc
        elif (self.buf.shape[1] != nb or self.Lc != Lc) and not any(self._counts):      # a new run at another batch: a new buffer
            self.buf = torch.zeros(len(self.names), nb, self.tokens, ldo, device=self.buf.device, dtype=torch.float32)
            self.Lc = Lc
        elif self.buf.shape[1] != nb or self.Lc != Lc:
            raise RuntimeError(f"attn_maps: the run records {self.buf.shape[1]} samples of {self.Lc} caption positions, this evaluation has "
                               f"{nb} of {Lc}: one recorder follows one run (start a new AttentionMaps, or resolve() again)")
        a = ax
        if nb != B:
            a = hip.AttnArgs.from_buffer_copy(ax)
            a.B = nb
        rows = None if out_rows is None else out_rows.data_ptr()
        if kbias is None:
            hip.check(hip.lib().md_attn_probs(byref(a), self.buf[r].data_ptr(), ldo, rows, hip.stream_ptr()), "md_attn_probs")
        else:
            hip.check(hip.lib().md_attn_probs_kbias(byref(a), kbias.data_ptr(), kbias.shape[1], self.buf[r].data_ptr(), ldo, rows,
                                                    hip.stream_ptr()), "md_attn_probs_kbias")
        self._counts[r] += 1

    # ------------------------------------------------------------------------------------------ read-out (plain torch)
    @classmethod
    def from_buffer(cls, names: Sequence[str], buf: torch.Tensor, counts: Sequence[int], Lc: int, grid: Tuple[int, int],
                    patch_size: int = 1) -> "AttentionMaps":
        """A recorder holding given sums (fp32 [len(names), B, T, ldo >= Lc]) and counts: the read-out of a saved or synthetic state."""
        am = cls()
        names = list(names)
        if buf.dim() != 4 or buf.shape[0] != len(names) or len(counts) != len(names) or buf.shape[3] < Lc or buf.shape[2] != grid[0] * grid[1]:
            raise ValueError("from_buffer: buf must be [len(names), B, h * w, ldo >= Lc] with one count per name")
        am.names, am.row = names, {n: i for i, n in enumerate(names)}
        am.buf, am._counts, am.Lc = buf.to(torch.float32), [int(c) for c in counts], int(Lc)
        am.tokens, am.grid, am.patch_size = int(buf.shape[2]), (int(grid[0]), int(grid[1])), int(patch_size)
        return am

    @property
    def counts(self) -> Dict[str, int]:
        """name -> evaluations recorded for that block in this run."""
        return {n: int(c) for n, c in zip(self.names, self._counts)}

    def _need(self) -> torch.Tensor:
        if self.buf is None:
            raise RuntimeError("attn_maps: nothing has been recorded yet")
        return self.buf

    def per_block(self) -> Dict[str, torch.Tensor]:
        """name -> fp32 [B, Lc, h, w]: the block's sum divided by its count (blocks never recorded are left out)."""
        buf, (h, w) = self._need(), self.grid
        out = {}
        for i, n in enumerate(self.names):
            if self._counts[i] > 0:
                m = buf[i, :, :, :self.Lc] / float(self._counts[i])
                out[n] = m.permute(0, 2, 1).reshape(m.shape[0], self.Lc, h, w).contiguous()
        return out

    def maps(self, blocks: BlockSelection = None) -> torch.Tensor:
        """fp32 [B, Lc, h, w]: the mean of per_block() over the recorded blocks `blocks` keeps (None: all)."""
        pb = self.per_block()
        chosen = [n for n in select_blocks(self.names, blocks) if n in pb]
        if not chosen:
            raise RuntimeError("attn_maps: none of the selected blocks has been recorded")
        return torch.stack([pb[n] for n in chosen]).mean(0)

    def token_mass(self) -> torch.Tensor:
        """fp32 [n_selected, Lc]: the mean over samples and image tokens of every block's map -- the share of attention on each
        caption position; a row sums to 1 (NaN for a block never recorded)."""
        buf = self._need()
        cnt = torch.tensor([float(c) if c > 0 else float("nan") for c in self._counts], device=buf.device, dtype=torch.float64)
        return (buf[..., :self.Lc].to(torch.float64).mean(dim=(1, 2)) / cnt[:, None]).to(torch.float32)

    def mask(self, tokens: Sequence[int], quantile: Optional[float] = None, threshold: Optional[float] = None, dilate: int = 0,
             blocks: BlockSelection = None) -> torch.Tensor:
        """fp32 [B, 1, H, W] in {0, 1}, 1 = generate and 0 = keep: an `inpaint_mask` of the region the caption positions `tokens`
        attended to.  The heat of those positions is summed, divided by the per-sample maximum and compared (>=) with `threshold`, or
        with its own per-sample `quantile` (exactly one of the two, each in [0, 1]); the result grows by `dilate` cells of the token
        grid (a (2 dilate + 1)^2 max-pool) and every cell is repeated patch_size times in both directions."""
        if (quantile is None) == (threshold is None):
            raise ValueError("mask takes exactly one of quantile= and threshold=")
        v = quantile if threshold is None else threshold
        if isinstance(v, (bool, str)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"{'quantile' if threshold is None else 'threshold'} must be a number in [0, 1], got {v!r}")
        if isinstance(dilate, bool) or not isinstance(dilate, int) or dilate < 0:
            raise ValueError(f"dilate must be an integer >= 0, got {dilate!r}")
        tokens = [int(t) for t in tokens]
        if not tokens or any(not 0 <= t < self.Lc for t in tokens):
            raise ValueError(f"tokens must name at least one caption position in [0, {self.Lc}), got {tokens!r}")
        heat = self.maps(blocks)[:, tokens].sum(1)                                  # [B, h, w]
        heat = heat / heat.flatten(1).max(1).values.clamp_min(torch.finfo(torch.float32).tiny).view(-1, 1, 1)
        if threshold is None:
            level = torch.quantile(heat.flatten(1), float(quantile), dim=1).view(-1, 1, 1)
        else:
            level = float(threshold)
        m = (heat >= level).to(torch.float32).unsqueeze(1)
        if dilate:
            m = Fnn.max_pool2d(m, 2 * dilate + 1, stride=1, padding=dilate)
        p = self.patch_size
        return m.repeat_interleave(p, 2).repeat_interleave(p, 3).contiguous()
