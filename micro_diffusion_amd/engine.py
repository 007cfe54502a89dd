"""DiTEngine — the hand-written forward AND backward of MicroDiT as an explicit sequence of HIP kernel launches.

No autograd below this boundary: every backward op is launched by `backward()` in reverse order of `forward()`,
reading the activations `forward()` saved in a `Tape`.  Host code is Python; every operation on device data is a
call into libmicrodit_hip.so through ctypes (micro_diffusion_amd/hip.py).  PyTorch is used for device memory
(`torch.empty`), the current HIP stream and nothing else.

Reference being replaced (paths relative to /root/reference/micro_diffusion/models):
  DiT.forward_without_cfg dit.py:455-519, DiTBlock.forward dit.py:232-239, FeedForward dit.py:88-89,
  FeedForwardECMoe.forward dit.py:126-143, AttentionBlockPromptEmbedding dit.py:53-56, SelfAttention /
  CrossAttention utils.py:116-136,178-197, T2IFinalLayer utils.py:236-240, TimestepEmbedder utils.py:283-285,
  CaptionProjection/Mlp utils.py:63-68, get_mask / mask_out_token / unmask_tokens utils.py:382-426 — and the
  autograd backward of all of them (no reference source: derived from the forward).

Numerics contract (amp_bf16 + low-precision LayerNorm): bf16 storage for activations, weights
(shadow copies of the fp32 masters) and activation gradients; fp32 accumulation in every GEMM / reduction; fp32
LayerNorm statistics, softmax, MoE routing and weight gradients (accumulated into the fp32 `.grad` buffer).
"""
from __future__ import annotations

import ctypes
import math
import os
import time
from ctypes import byref
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch

from . import hip, splitk
from .arch import BlockPlan, DiTConfig, caption_ffn_hidden, plan_blocks

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
TAIL_WS_BYTES = 256 * 256 * 256 * 4     # md_gemm_args.tail_ws: one raw 256 x 256 fp32 tile per workgroup (64 MiB of the split-K workspace)


class Tape:
    """Activations saved by one forward pass (plain attribute bag)."""


def launch(lib, stream, symbol, *args):
    """One call into the native library, return code checked (hip.py: every launch function returns int and takes the stream last)."""
    hip.check(getattr(lib, symbol)(*args, stream), symbol)


def poison_(t: torch.Tensor) -> torch.Tensor:
    """Debug fill of a buffer nothing has written yet (DiTEngine.poison): NaN for floating dtypes, 0 for integer ones -- every
    integer buffer of the engine is an index table a kernel indexes with, and 0 is always inside the table.  One stream-ordered
    fill_ on the current stream."""
    if t.numel():
        t.fill_(float("nan") if t.dtype.is_floating_point else 0)
    return t


class _Arena:
    """Bump allocator over ONE device buffer.  With it the activations, gradients and scratch of a microbatch live at fixed
    addresses and the step path makes no allocator calls (no caching-allocator bookkeeping per launch, no at::native fill
    kernels; the launch sequence of a microbatch becomes capturable as a hipGraph).  The first pass through a new shape key
    runs in measuring mode — plain torch.empty, sizes recorded with the same mark / release discipline — and the buffer is
    then (re)allocated at the largest peak of all keys seen, so alternating shapes (a ragged last microbatch) do not
    re-measure.  A pass that raised is not recorded."""
    ALIGN = 256

    def __init__(self, dev):
        self.dev, self.buf, self.key = dev, None, None
        self.peaks = {}                 # shape key -> measured peak bytes
        self.top = self.peak = 0
        self.measuring = True

    def begin(self, key):
        """Start a pass of shape `key`.  The buffer is (re)allocated HERE, never at the end of a measuring pass: the tensors of
        the measuring pass (a whole activation tape: 156 GB for XL/2 at microbatch 1024) are still alive when it ends, and
        measured peak + buffer would not fit the HBM; by the next pass the caller has dropped them."""
        self.key = key
        need = self.peaks.get(key)
        if need is not None and (self.buf is None or self.buf.numel() < need + self.ALIGN):
            want = max(self.peaks.values()) + self.ALIGN
            self.buf = None             # release before re-allocating
            self.buf = torch.empty(want, device=self.dev, dtype=torch.uint8)
        self.measuring = need is None
        self.top = self.peak = 0

    def end(self, ok: bool = True):
        if self.measuring and ok:       # a pass that raised half-way did not reach the shape's peak: not recorded
            self.peaks[self.key] = self.peak

    def mark(self) -> int:
        return self.top

    def release(self, mark: int) -> None:
        self.top = mark

    def alloc(self, shape, dtype):
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        off = self.top
        self.top = (off + nbytes + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.peak = max(self.peak, self.top)
        if self.measuring:
            return torch.empty(*shape, device=self.dev, dtype=dtype)
        if self.top > self.buf.numel():
            raise RuntimeError("activation arena overflow: the launch sequence changed without a change of the shape key")
        return self.buf[off:off + nbytes].view(dtype).view(*shape)


class Conditioning:
    """What a forward pass derives from the captions alone (DiTEngine.encode_condition): computed once per prompt set and handed to
    every network evaluation of a sampling run (`forward(..., cond=...)`).
      kv      {block name: (kv [B*Lc, 2*hx] with K normalised and V raw -- the buffer _block_fwd leaves after md_qkln_fwd,
               head-major normalised K [B, H, Lc, hd] or None)} for every mixer and backbone block
      pooled  [B, D]: LayerNorm+GELU output of pooled_y_emb_process, the input of its fc2 (fc2 itself runs per evaluation, its
               epilogue adds the timestep embedding: c is rounded once, as in the uncached pass)
      B, Lc, head_major, version (DiTEngine.weights_version it was computed from), nbytes"""

    def __init__(self, B, Lc, head_major, version, pooled, kv):
        self.B, self.Lc, self.head_major, self.version, self.pooled, self.kv = B, Lc, head_major, version, pooled, kv

    @property
    def nbytes(self) -> int:
        ts = [self.pooled] + [t for pair in self.kv.values() for t in pair if t is not None]
        return sum(t.numel() * t.element_size() for t in ts)

    def narrow(self, B: int) -> "Conditioning":
        """The first B samples as a Conditioning of batch B: views of the same buffers (every buffer is sample-major, so the first B
        samples are its leading rows), same layout and weight version.  The sampler's guidance interval runs the conditional half of
        a cache encoded for [captions; zeroed captions] through it."""
        if not 0 < B <= self.B:
            raise ValueError(f"cannot narrow a conditioning of batch {self.B} to {B}")
        if B == self.B:
            return self
        kv = {name: (k[:B * self.Lc], None if khm is None else khm[:B * self.Lc]) for name, (k, khm) in self.kv.items()}
        return Conditioning(B, self.Lc, self.head_major, self.version, self.pooled[:B], kv)


class ResidualCache:
    """State of the step cache: what backbone blocks [lo, hi) added to the residual stream in the last full evaluation,
    handed to `DiTEngine.forward(..., step_cache=, reuse=)`.
      delta   [B*T, D] bf16 = bf16(output of block hi - 1 - input of block lo) (md_residual_delta), allocated on first use
      ref     [B*T, D] bf16, only with probe=True: the backbone's input of the previous evaluation (md_step_probe keeps it current)
      lo, hi  the block range inside the engine's backbone; blocks=None: all of it (resolved by the first forward)
      B, T, version   the batch, token count and DiTEngine.weights_version `delta` was filled at (None: empty)
    Each buffer takes 2 * B * T * D bytes.  One cache serves one batch shape at a time: a full evaluation at another shape refills it."""

    def __init__(self, blocks=None, probe: bool = False):
        if blocks is not None:
            lo, hi = blocks
            if any(isinstance(v, bool) or not isinstance(v, int) for v in (lo, hi)) or not 0 <= lo < hi:
                raise ValueError(f"blocks must be (lo, hi) with 0 <= lo < hi, backbone block indices, got {blocks!r}")
            blocks = (lo, hi)
        self.blocks, self.with_probe = blocks, bool(probe)
        self.lo = self.hi = None
        self.delta = self.ref = None
        self.B = self.T = self.version = None
        self._ref_key = None
        self._ws = self._rel = self._rel_max = None
        self.poison = False             # DiTEngine.forward copies its own switch here: new buffers are handed out poisoned

    def _new(self, shape, like: torch.Tensor, dtype=None) -> torch.Tensor:
        t = torch.empty(shape, device=like.device, dtype=like.dtype if dtype is None else dtype)
        return poison_(t) if self.poison else t

    def reset(self) -> None:
        """Forget the filled state and the probe reference (the buffers stay allocated): the start of a sampling run."""
        self.B = self.T = self.version = None
        self._ref_key = None

    def valid(self, B: int, T: int, version) -> bool:
        return self.delta is not None and (self.B, self.T, self.version) == (B, T, version)

    def resolve(self, n_backbone: int):
        """(lo, hi) inside a backbone of n_backbone blocks."""
        lo, hi = (0, n_backbone) if self.blocks is None else self.blocks
        if not 0 <= lo < hi <= n_backbone:
            raise ValueError(f"step cache: blocks [{lo}, {hi}) are outside the backbone's {n_backbone} blocks")
        self.lo, self.hi = lo, hi
        return lo, hi

    def store(self, x_out: torch.Tensor, x_in: torch.Tensor, B: int, T: int, version) -> None:
        """delta <- bf16(x_out - x_in): one launch."""
        if self.delta is None or self.delta.shape != x_in.shape or self.delta.device != x_in.device:
            self.delta = self._new(x_in.shape, x_in)
        launch(hip.lib(), torch.cuda.current_stream().cuda_stream, "md_residual_delta", x_out.data_ptr(), x_in.data_ptr(), self.delta.data_ptr(),
               x_in.numel())
        self.B, self.T, self.version = B, T, version

    def probe(self, x: torch.Tensor, B: int, version=None):
        """The relative L1 distance of x [B*T, D] (the backbone's input, B samples) from the previous evaluation's, as the device scalar
        rel_max = max_b sum |x_b - ref_b| / sum |ref_b| (fp32 [1]), and ref <- x: two launches, nothing returns
        to the host.  The first probe after a reset, or at another shape or weight version, only fills ref and returns None."""
        key = (tuple(x.shape), B, version)
        if self.ref is None or self.ref.shape != x.shape or self.ref.device != x.device:
            self.ref = self._new(x.shape, x)
            self._ref_key = None
        if self._ref_key != key:
            self.ref.copy_(x)
            self._ref_key = key
            return None
        L, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        per = x.numel() // B
        need = ctypes.c_int64(0)
        hip.check(L.md_step_probe_ws_doubles(B, per, byref(need)), "md_step_probe_ws_doubles")
        if self._ws is None or self._ws.numel() < need.value or self._ws.device != x.device:
            self._ws = self._new(need.value, x, torch.float64)
        if self._rel is None or self._rel.numel() != B or self._rel.device != x.device:
            self._rel = self._new(B, x, F32)
            self._rel_max = self._new(1, x, F32)
        launch(L, st, "md_step_probe", x.data_ptr(), self.ref.data_ptr(), B, per, self._ws.data_ptr())
        launch(L, st, "md_step_probe_finish", self._ws.data_ptr(), B, self._rel.data_ptr(), self._rel_max.data_ptr())
        return self._rel_max

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.delta, self.ref) if t is not None)


def _p(t):
    return None if t is None else t.data_ptr()


def _Deferred(buf):
    """What the blocks of one stack leave for ONE grouped launch behind the stack's backward: the bf16 matrix of the i-th block run in
    buf[i] (the next free one: buf[len(w)]), the address of the weight it is contracted with in w[i]."""
    return SimpleNamespace(buf=buf, w=[])


class InputGrads:
    """What DiTEngine.backward returns: the gradients of the network inputs that were asked for (the others None).
      dx f32 [B, C, H, W]; dt f32 [B]; dy [B*Lc, Dc] in the dtype of the forward's y (f32 | f16)"""
    __slots__ = ("dx", "dt", "dy")

    def __init__(self):
        self.dx = self.dt = self.dy = None


class DiTEngine:
    # False inside a dgrad-only backward (backward(param_grads=False)): the helpers that write self.G -- lin_wgrad,
    # _param_acc, _param_colsum, ln_bwd's weight reduction -- launch nothing; every data-gradient launch is the one of a full backward
    _param_grads = True
    # True inside backward(param_grads="lora") ("Factored backward"): a dgrad-only backward in which lin_wgrad hands the
    # operands of every linear the attached adapter targets to md_lora_wgrad (lora.LoRA.wgrad); self.G is not touched
    _lora_grads = False
    lora = None                         # the attached lora.LoRA (LoRA.attach / detach; LatentDiffusion.train_microbatch)
    # True inside a backward that stops at the image (input_grads=("x",), param_grads=False): nothing that dx does not
    # depend on is launched -- the K side of the cross-attention QK-LayerNorm, the caption-token and condition-vector contractions
    _x_only = False

    def __init__(self, cfg: DiTConfig, params: Dict[str, torch.Tensor], shadows: Dict[str, torch.Tensor],
                 grads: Dict[str, torch.Tensor], buffers: Dict[str, torch.Tensor]):
        """params: fp32 masters; shadows: bf16 copies (same names); grads: fp32 accumulators; buffers: pos_embed,
        mask_token.  All are views into flat device buffers owned by the DiT module."""
        self.cfg = cfg
        self.P, self.S, self.G, self.buf = params, shadows, grads, buffers
        self.mixer, self.backbone = plan_blocks(cfg)
        self.dev = next(iter(params.values())).device
        self.L = hip.lib()
        self.wgrad_target_blocks = 768
        self.gemm_profile = None
        self.kernel_profile = None         # bench.py: {class name: [(event0, event1, algorithmic bytes)]} for the bandwidth-bound kernels
        self.gemm_prefer = hip.GEMM_AUTO   # tests / A-B runs: a kernel to force wherever it accepts the problem (else the library's choice)
        self.attn_bwd_prefer = hip.ATTN_BWD_AUTO   # same for the attention backward (md_attn_args.bwd_split)
        # Head-major q / k (round 6): QK-LayerNorm writes q / k as [B, H, S, hd] (md_qkln_fwd_hm), attention returns dq / dk in that
        # layout and md_qkln_bwd_hm brings them back row-major.  Built, parity-tested and MEASURED NEUTRAL in the step (attention
        # -10.5 ms, QK-LayerNorm +7 ms of a 2,311 ms profile; same-box A/B 2,658 vs 2,659 images/s at microbatch 1024, -0.6 % at 256:
        # profiles/r6_head_major_qk.txt) -- v / o / dO / dv stay in packed rows unless the GEMM epilogues re-lay them.  Off by default
        # (it costs 2/3 of a qkv buffer per block of tape); MD_QK_HEAD_MAJOR=1 or this attribute turns it on.
        self.qk_head_major = os.environ.get("MD_QK_HEAD_MAJOR", "0") == "1"
        # Deterministic mode (opt-in: MD_DETERMINISTIC=1, or set this before the first step): the four float-atomic column reductions of
        # the training path (md_ln_bwd: dS / dshift and dw, md_gate_bwd: dgate, md_colsum: bias gradients) go through their _det entry
        # points -- per-workgroup partial sums in a workspace, added in a fixed order -- so two runs of one step on one GPU give
        # bit-identical gradients.  Off: the launch sequence is unchanged.  (DESIGN.md "Deterministic mode")
        self.deterministic = os.environ.get("MD_DETERMINISTIC", "0") == "1"
        # Poisoned allocations (opt-in: MD_POISON=1 or this attribute; debug only): every buffer empty() / fresh() hands
        # out is filled first -- NaN for floating dtypes, 0 for integer ones -- and the split-K / tail workspace is filled with NaN at
        # the start of every forward() and backward(), so a launch that reads what nothing wrote in this pass meets NaN (or index 0)
        # instead of what the previous, identical pass left at the same arena address.  Off: one attribute test, no launch.
        self.poison = os.environ.get("MD_POISON", "0") == "1"
        self._det_ws_floats = {}           # (kind, rows, rows per sample, rows per block, C) -> md_det_ws_floats
        self.gemm_log = None               # tests: list that receives (variant actually requested, M, N, K, batch) per launch
        self.before_segment = None         # data parallelism: callable(bucket key) run before the first kernel that reads the bf16
        #                                    weights of a bucket ("rest", block names, "final_layer"): waits for their all-gather
        self.keep_last_tape = False        # tests: keep the most recent forward's tape in self.last_tape (per-block activations)
        self.last_tape = None
        self.route_override = None         # tests: {block name: top-k token indices [B, E, k]} replacing the router's choice
        # Routing diagnostics (opt-in): a diagnostics.RouteStats; every routed layer then adds its coverage / entropy /
        # marginals to its row right behind md_moe_route (one md_moe_route_stats call).  None: no launch, no buffer.  Its tables and
        # workspace are its own allocations: arena sizes, addresses and the tape are those of an unarmed pass.
        self.route_stats = None
        # Cross-attention maps (opt-in): an attn_maps.AttentionMaps; right behind every cross-attention it recomputes the
        # head-averaged probabilities from the q / k attention just read (one md_attn_probs launch into its own fp32 buffer, no host
        # wait).  None: no launch, no buffer; arena sizes, addresses and the tape are those of an unarmed pass either way.
        self.attn_probe = None
        # Caption bias (opt-in): None, or an fp32 device tensor [Bmax, ldb] (ldb >= Lc, ldb % 4 == 0, 16-byte aligned rows)
        # added to the cross-attention logits of every mixer and backbone block: softmax_j(scale q . k_j + caption_bias[b, j]), one value per
        # (sample, caption position), shared by heads and queries; -inf removes a position.  An evaluation at batch B <= Bmax reads the
        # first B rows (sample-major, the convention of Conditioning.narrow).  The launches become md_attn_fwd_kbias (and, with an
        # attn_probe, md_attn_probs_kbias); self-attention, the cached K / V of cond= and the pooled caption vector (md_mean_tokens: the
        # plain mean over all positions) do not see it.  Inference only: the attention backward does not know the bias, so a forward
        # that records a tape for a backward raises while it is set.  None: the launches and bits of a pass without it.
        self.caption_bias = None
        # MXFP8 linears (opt-in): None, or an mxfp8.MXWeights -- block-scaled fp8 copies of the targeted block linears.
        # lin_fwd, the two expert GEMMs and the SwiGLU FFN then quantise their input (md_mx_quant_rows / md_swiglu_fwd_mx, buffers from
        # empty() like every activation) and launch md_gemm_mxfp8 wherever the weight is in `mx` and the problem is eligible (K % 128 ==
        # 0, N % 16 == 0); every other launch is the bf16 one, unchanged.  Inference only: a forward that records a tape raises while it
        # is set, and so does one whose MXWeights were built from another weight version.  None: the launches and bits of a pass without it.
        self.mx = None
        self.mx_log = None                 # tests: list that receives (weight name, "mx" | "bf16") per linear of lin_fwd / the expert GEMMs
        # Masked-expert pruning: the masking right behind the last patch-mixer block keeps Tk of T tokens, so when that block
        # is MoE its expert MLPs (forward, both data gradients, both weight gradients) run only on the routed rows whose token survives --
        # about (1 - mask_ratio) of them.  Routing stays dense and the tape's probs / rowidx / gval / slot are those of the dense pass.
        # Costs ONE host wait per microbatch (the per-expert counts, 4 E bytes): a microbatch is then not capturable as a hipGraph.
        # Off (MD_PRUNE_MASKED_EXPERTS=0 or this attribute): the launch sequence is that of the dense pass.
        self.prune_masked_experts = os.environ.get("MD_PRUNE_MASKED_EXPERTS", "1") != "0"
        self.prune_granule = 256           # the pruned GEMMs run on ceil(max count / granule) * granule rows per expert: whole 256-row tiles keep
        #                                    every launch on its dense counterpart's kernel family (w4), contraction a multiple of 128 for _ksplit
        self.prune_wait_us = None          # tests / profiling: list that receives the host time of every count readback, in microseconds
        self._prune_host = None            # pinned int32[16] the counts land in
        self.route_log = None              # tests: list that receives the name of every routing-family entry point a MoE block calls
        # Dispersive loss (opt-in): None, or (k, weight, tau) armed for the training forwards that follow (the model's
        # train_microbatch arms and disarms it): right behind backbone block k the Gram of its output over the microbatch and
        # md_disperse_pairs run, and the backward adds weight * grad_scale * dL/dZ to dx in front of block k's backward (one GEMM).
        # disperse_train = (grad_scale, loss_accum, dist_accum, accum_weight) of the microbatch.  None: the launches of an unarmed pass.
        self.disperse = None
        self.disperse_train = (1.0, None, None, 0.0)
        self.disperse_log = None           # tests: list that receives ("gram" | "apply", "gemm" | "small", B, K) per product
        self._disperse_on = False
        self._disperse_result = None       # fp64 [4] result block of md_disperse_pairs (L, mean D, mean p B^2, S): one fixed buffer
        self.ws = torch.empty(128 << 20, device=self.dev, dtype=F32)  # 512 MiB split-K workspace
        # Fixed-address activation memory (opt-in: the caller must run forward -> backward strictly in turn, as the Trainer
        # does; two forwards in flight would share the tape arena).
        self.use_arena = False
        self._tape_arena, self._scratch_arena = _Arena(self.dev), _Arena(self.dev)
        self._arena = None          # arena the next empty() / zeros() comes from (None = torch allocator)
        self._record = False        # current forward keeps per-block tapes
        self._chosen = ctypes.c_int32(-1)   # md_gemm_args.chosen_variant lands here
        self._ptr_cache = {}
        self.ksplit_min_items = 192  # work items a split-K factor must reach (A/B: 128 = the round-2 rule)
        self.splitk_force_pp = False  # A/B: force pp256 for every split-K launch it accepts, whatever the tile count
        self.short_k_accum = True   # A/B: False = split-K slices also for short contractions into large outputs
        self.group_wgrad = True     # the weight gradients of a block that contract over the same tokens as grouped launches (A/B: False)
        self._wgroup = None
        self.single_slice_ws = True  # launches with >= 192 tiles of their own: one fp32 slice through the workspace on pp256 (A/B: False = accumulate epilogue)
        self.group_dycond = True    # ONE launch for the caption-token gradients of all cross-attention kv projections of a group (A/B: False)
        self.group_adaln = True     # one launch for the condition-vector gradients of all adaLN layers of a group (A/B: False)
        self._posb = None
        self.moe_cache_dact = True  # the MoE fc1 epilogue stores gelu'(h) instead of h; the fc2 dgrad epilogue multiplies by it (A/B: False)
        self.batch_adaln = True     # the modulation of ALL blocks from one GEMM per forward (A/B: False = one small GEMM per block)
        self._adaln = self._adaln_region()
        self.gemm_tail_mode = int(os.environ.get("MD_GEMM_TAIL", "0"))   # md_gemm_args.tail_mode: 0 = the library decides, 1 = never, 2 = always (A/B)
        # One-microbatch steps of the data-parallel Trainer (a rank of the 8-GPU run: configs/res_256_pretrain.yaml:24,111): weight
        # gradients whose fp32 accumulator lies in [g_lo, g_hi) are STORED as bf16 at gbf + (addr - g_lo) / 2 -- the exchange buffer of
        # GradSync -- by the split-K reduction (or the GEMM epilogue when nothing is split): no read-modify-write of the fp32
        # accumulator, no cast + clear pass afterwards.  (g_lo, g_hi, gbf address, {fp32 address: elements stored} of this step)
        self.wgrad_bf16 = None
        self.fuse_swiglu_bwd = os.environ.get("MD_FUSE_SWIGLU_BWD", "1") != "0"   # A/B: 0 = data gradient + md_swiglu_bwd as two launches
        self.weights_version = 0    # set by the owning DiT whenever it rewrites the bf16 shadow: a Conditioning is valid for one version
        self.input_grad_log = None  # tests: list that receives (entry point, kernel path or None) of every input-gradient launch
        self.cu_limit_fn = None     # data parallelism: callable() -> CUs the persistent GEMM may occupy right now (0 = all): the
        #                             Trainer leaves the CUs of RCCL's channels free while a collective is in flight

    def _adaln_region(self):
        """The block adaLN Linear layers (dit.py:222-225: mod_l = W_l gelu(c) + b_l, the same input for every block) as ONE GEMM:
        dit.flat_layout keeps their weights contiguous in forward order (mixer blocks, then backbone blocks) and their biases
        likewise, so [W_0; W_1; ...] is a [sum 6 d_l, D] matrix.  Returns {"N", "w", "b", "col": {block name: first column}} or None
        when the tensors are not laid out that way (a foreign flat layout): the per-block GEMMs remain."""
        names = [bp.name for bp in self.mixer] + [bp.name for bp in self.backbone]
        col, n, w0, b0 = {}, 0, None, None
        for nm in names:
            w, b = self.S.get(nm + ".adaLN_modulation.1.weight"), self.P.get(nm + ".adaLN_modulation.1.bias")
            if w is None or b is None or w.dim() != 2 or w.shape[1] != self.cfg.dim:
                return None
            if w0 is None:
                w0, b0 = w, b
            elif w.data_ptr() != w0.data_ptr() + 2 * n * self.cfg.dim or b.data_ptr() != b0.data_ptr() + 4 * n:
                return None
            col[nm] = n
            n += w.shape[0]
        if w0 is None or n % 8:
            return None
        return {"N": n, "w": w0.data_ptr(), "b": b0.data_ptr(), "col": col}

    def _adaln_all(self, gc, B):
        """mod_all [B, N_all] bf16 = gelu(c) [W_0; W_1; ...]^T + [b_0; b_1; ...]: 780 output tiles at XL/2 instead of 34 launches
        of 18-24 tiles each (96 TFLOP/s at microbatch 256, profiles/r3_gemm_shapes_mb256.txt)."""
        r = self._adaln
        out = self.empty(B, r["N"])
        D = self.cfg.dim
        self._gemm(A=gc.data_ptr(), B=r["w"], C=out.data_ptr(), bias=r["b"], M=B, N=r["N"], K=D, lda=D, ldb=D, ldc=r["N"], batch=1, ksplit=1,
                   a_kcontig=1, b_kcontig=1, mode=hip.EPI_STORE_BF16, act=0, alpha=1.0)
        return out

    # ------------------------------------------------------------------------------------------ launch helpers
    def _st(self):
        return torch.cuda.current_stream().cuda_stream

    def empty(self, *shape, dtype=BF16):
        t = self._arena.alloc(shape, dtype) if self._arena is not None else torch.empty(*shape, device=self.dev, dtype=dtype)
        return poison_(t) if self.poison else t

    def fresh(self, *shape, dtype=F32):
        """Uninitialised memory of the torch allocator, never the arena: what outlives the pass (returned input gradients, the loss
        glue's per-sample buffers)."""
        t = torch.empty(*shape, device=self.dev, dtype=dtype)
        return poison_(t) if self.poison else t

    def _poison_ws(self):
        if self.poison:
            self.ws.fill_(float("nan"))

    def zeros(self, *shape, dtype=F32):
        t = self.empty(*shape, dtype=dtype)
        self._launch("md_fill_zero", t.data_ptr(), t.numel() * t.element_size())
        return t

    def _prof(self, name, nbytes, launch):
        """Run `launch()`; with kernel_profile set, bracket it with HIP events on the launch stream (bench.py roofline_hbm leg)."""
        kp = self.kernel_profile
        if kp is None:
            return launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        kp.setdefault(name, []).append((e0, e1, float(nbytes)))

    def _launch(self, symbol, *args, prof=None, nbytes=0.0):
        """self.L.<symbol>(*args, launch stream), checked; prof / nbytes: its kernel_profile class and algorithmic bytes (bench.py)."""
        if prof is None or self.kernel_profile is None:
            return launch(self.L, self._st(), symbol, *args)
        self._prof(prof, nbytes, lambda: launch(self.L, self._st(), symbol, *args))

    def _launch_det(self, symbol, ws_key, *args, prof, nbytes):
        """`symbol`, or -- deterministic mode -- `symbol`_det, which takes the workspace of _det_ws(*ws_key) and its size as well."""
        if self.deterministic:
            symbol, args = symbol + "_det", args + self._det_ws(*ws_key)
        self._launch(symbol, *args, prof=prof, nbytes=nbytes)

    def _det_ws(self, kind, rows, rps, rpb, C):
        """(pointer, floats) of the workspace a deterministic reduction of this shape needs ((None, 0): none).  The size is asked once
        per shape; the buffer comes from the current arena (or the allocator) and is dead when the launch has run."""
        key = (kind, rows, rps, rpb, C)
        n = self._det_ws_floats.get(key)
        if n is None:
            out = ctypes.c_int64(0)
            hip.check(self.L.md_det_ws_floats(kind, rows, rps, rpb, C, byref(out)), "md_det_ws_floats")
            n = self._det_ws_floats[key] = int(out.value)
        return (self.empty(n, dtype=F32).data_ptr(), n) if n else (None, 0)

    def _colsum(self, src_ptr, is_f32, ld, out_ptr, rows, C):
        """out[c] += column sums (bias gradients)."""
        self._launch_det("md_colsum", (hip.DET_COLSUM, rows, 0, 0, C), src_ptr, is_f32, ld, out_ptr, rows, C, prof="colsum",
                         nbytes=(4.0 if is_f32 else 2.0) * rows * C)

    def _gate_bwd(self, dx, br, gate_ptr, ldgate, dbr, dgate_ptr, lddg, M, d, S, rpb):
        """adaLN-Zero gate backward: dbr = gate * dx, dgate += per-sample column sums of dx * br."""
        self._launch_det("md_gate_bwd", (hip.DET_GATE_BWD, M, S, rpb, d), dx.data_ptr(), br.data_ptr(), gate_ptr, ldgate, dbr.data_ptr(), dgate_ptr,
                         lddg, M, d, S, rpb, prof="gate_bwd", nbytes=6.0 * M * d)

    def _qkln_fwd(self, ptr, rows, ld, off, width, rstd_ptr, nseg=1):
        """nseg = 2: the q and the k half (adjacent, `width` apart) of a packed qkv row in one launch; rstd [nseg][rows]."""
        self._launch("md_qkln_fwd", ptr, rows, ld, off, width, nseg, width, rstd_ptr, self.cfg.norm_eps, prof="qk_layernorm",
                     nbytes=4.0 * rows * width * nseg)

    def _qkln_bwd(self, dptr, ldd, doff, yptr, ldy, yoff, rows, width, rstd_ptr, nseg=1):
        self._launch("md_qkln_bwd", dptr, ldd, doff, yptr, ldy, yoff, rows, width, nseg, width, width, rstd_ptr, prof="qk_layernorm",
                     nbytes=6.0 * rows * width * nseg)

    def _qkln_fwd_hm(self, ptr, rows, ld, off, width, out, S, rstd_ptr, nseg=1):
        """As _qkln_fwd, the normalised values going head-major to out [nseg][B, H, S, hd]; the input stays as it is."""
        self._launch("md_qkln_fwd_hm", ptr, rows, ld, off, width, nseg, width, out.data_ptr(), rows * width, S, self.cfg.head_dim, rstd_ptr,
                     self.cfg.norm_eps, prof="qk_layernorm", nbytes=4.0 * rows * width * nseg)

    def _qkln_bwd_hm(self, dy, y, dptr, ldd, doff, rows, width, S, rstd_ptr, nseg=1):
        """dy, y: head-major [nseg][B, H, S, hd]; dL/dx goes row-major to dptr (segments `width` apart, as in _qkln_bwd)."""
        self._launch("md_qkln_bwd_hm", dy.data_ptr(), rows * width, y.data_ptr(), rows * width, dptr, ldd, doff, width, rows, width, nseg, S,
                     self.cfg.head_dim, rstd_ptr, prof="qk_layernorm", nbytes=6.0 * rows * width * nseg)

    def _attn_fwd(self, a, kbias=None):
        """kbias: the armed caption_bias for a cross-attention (its first a.B rows are read), else None."""
        nbytes = 2.0 * a.hd * (2 * a.Sq + 2 * a.Skv) * a.B * a.H
        if kbias is None:
            self._launch("md_attn_fwd", byref(a), prof="attention", nbytes=nbytes)
        else:
            self._launch("md_attn_fwd_kbias", byref(a), kbias.data_ptr(), kbias.shape[1], prof="attention", nbytes=nbytes + 4.0 * a.Skv * a.B)

    def _check_caption_bias(self, B, Lc, taping):
        """The armed caption_bias against an evaluation at batch B with Lc caption positions, before anything is launched."""
        kb = self.caption_bias
        if taping:
            raise RuntimeError("caption_bias is inference-only: the attention backward does not know the bias, so record_tape, arena and "
                               "input_tape cannot be combined with it (DESIGN.md 4.22)")
        if not (torch.is_tensor(kb) and kb.is_cuda and kb.dtype == F32 and kb.dim() == 2 and kb.is_contiguous()
                and kb.shape[1] % 4 == 0 and kb.data_ptr() % 16 == 0):
            raise ValueError("caption_bias must be a contiguous fp32 device tensor [Bmax, ldb] with ldb % 4 == 0, 16-byte aligned")
        if B > kb.shape[0] or kb.shape[1] < Lc:
            raise ValueError(f"caption_bias holds {kb.shape[0]} rows of {kb.shape[1]} positions; this evaluation has batch {B} and "
                             f"{Lc} caption positions")

    def _gemm(self, **kw):
        a = hip.GemmArgs()
        problems = kw.pop("_problems", None)      # grouped launch: the problem dicts (accounting only; the table is in kw["problems"])
        may_refuse = kw.pop("_try", False)        # True: a launch the library may refuse (NOT_ELIGIBLE, nothing launched) -> returns False
        for k, v in kw.items():
            setattr(a, k, v)
        if self.deterministic and a.mode == hip.EPI_ATOMIC_F32 and a.ksplit > 1:
            raise RuntimeError("deterministic mode: a split-K GEMM with the fp32-atomic epilogue sums in an order that changes from run "
                               "to run; use the workspace slices + md_splitk_reduce (gemm_f32_acc)")
        prof = self.gemm_profile
        if prof is not None:      # per-launch HIP events on the launch stream (bench.py roofline leg)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        chosen = self._chosen
        a.chosen_variant = ctypes.addressof(chosen)
        if self.cu_limit_fn is not None:
            a.cu_limit = self.cu_limit_fn()
        if self.gemm_tail_mode != 1 and a.mode in (hip.EPI_STORE_BF16, hip.EPI_RESIDUAL, hip.EPI_DACT):
            # whole rounds + split-K tail (md_gemm_args.tail_ws): bf16-output launches never use the split-K workspace themselves,
            # and everything that does is ordered behind them on this stream
            a.tail_ws, a.tail_ws_bytes, a.tail_mode = self.ws.data_ptr(), TAIL_WS_BYTES, self.gemm_tail_mode
        rc = hip.NOT_ELIGIBLE
        want = self.gemm_prefer if self.gemm_prefer != hip.GEMM_AUTO else a.variant
        if want != hip.GEMM_AUTO:
            a.variant = want
            rc = self.L.md_gemm_bf16(byref(a), self._st())      # NOT_ELIGIBLE: the forced kernel refuses this problem (nothing was launched)
            if rc == hip.NOT_ELIGIBLE:
                a.variant = hip.GEMM_AUTO
        if rc == hip.NOT_ELIGIBLE:
            rc = self.L.md_gemm_bf16(byref(a), self._st())
        if rc == hip.NOT_ELIGIBLE and may_refuse:
            return False
        hip.check(rc, "md_gemm_bf16")
        if self.gemm_log is not None:      # the kernel the library actually launched (written back through chosen_variant)
            self.gemm_log.append((chosen.value, a.M, a.N, a.K, a.batch))
        if prof is not None:
            e1.record()
            # algorithmic HBM bytes of the launch: both operands once, every output once (+ fused-epilogue operands)
            out_b = 4 if a.mode in (hip.EPI_STORE_F32, hip.EPI_ACCUM_F32, hip.EPI_ATOMIC_F32) else 2
            mn = a.M * a.N * a.batch
            byt = 2.0 * (a.M * a.K + a.N * a.K) * a.batch + mn * out_b * a.ksplit
            byt += mn * 2 * ((1 if a.C2 else 0) + (1 if a.res else 0) + (1 if a.aux else 0)) + (mn * 4 if a.mode == hip.EPI_ACCUM_F32 else 0)
            if a.mode == hip.EPI_SWIGLU_BWD:
                byt += mn * 2 * 2            # h2 beside h1, dh2 beside dh1
            fl = 2.0 * a.M * a.N * a.K * a.batch
            key = (a.M, a.N, a.K, a.batch, a.a_kcontig, a.b_kcontig, a.ksplit)
            if problems:
                mn = sum(g["M"] * g["N"] for g in problems)
                fl = 2.0 * mn * a.K
                byt = 2.0 * a.K * sum(g["M"] + g["N"] for g in problems) + mn * 4 * a.ksplit
                key = (-len(problems), mn // 1024, a.K, 1, 0, 0, a.ksplit)
            prof.append((e0, e1, fl, key, byt))
        return True

    def lin_fwd(self, x, wname, out, M, N, K, *, ldx=None, ldc=None, mode=hip.EPI_STORE_BF16, act=0, res=None,
                gate=None, ldg=0, rps=0, C2=None, ldc2=0, xoff=0, ooff=0, bias=True, xq=None):
        """out[M,N] = epilogue(x[M,K] @ W[N,K]^T + b).  x / out may be offset views (element offsets).
        xq: (elements, scales) of x already in MXFP8 (md_swiglu_fwd_mx), for a weight that is in self.mx; x is then not read."""
        b = self.P.get(wname + ".bias") if bias else None
        if self.mx is not None and mode in (hip.EPI_STORE_BF16, hip.EPI_RESIDUAL):
            ent = self.mx.entries.get(wname)
            # (the kernels move 16-byte pieces: an offset view that breaks their alignment keeps the bf16 launch)
            if ent is not None and ent.batch == 1 and (ent.N, ent.K) == (N, K) and ooff % 8 == 0 and (ldc or N) % 8 == 0 and \
                    (xq is not None or ((ldx or K) % 8 == 0 and xoff % 8 == 0)):
                if xq is None:
                    xq = self._mx_quant(x.data_ptr() + 2 * xoff, ldx or K, M, K)
                self._mx_gemm(xq, ent, out.data_ptr() + 2 * ooff, M, N, K, ldc=ldc or N, mode=mode, act=act, bias=_p(b), res=_p(res), ldr=N,
                              gate=gate, ldg=ldg, rps=rps, C2=_p(C2), ldc2=ldc2 or N)
                if self.mx_log is not None:
                    self.mx_log.append((wname, "mx"))
                return
        assert xq is None, f"{wname}: an MXFP8 input needs the weight in engine.mx"
        if self.mx_log is not None:
            self.mx_log.append((wname, "bf16"))
        self._gemm(A=x.data_ptr() + 2 * xoff, B=self.S[wname + ".weight"].data_ptr(),
                   C=out.data_ptr() + (4 if mode in (hip.EPI_STORE_F32, hip.EPI_ACCUM_F32) else 2) * ooff,
                   C2=_p(C2), bias=_p(b), res=_p(res), gate=gate, M=M, N=N, K=K, lda=ldx or K, ldb=K, ldc=ldc or N,
                   ldc2=ldc2 or N, ldr=N, ldg=ldg, rows_per_sample=rps, batch=1, ksplit=1, a_kcontig=1, b_kcontig=1,
                   mode=mode, act=act, alpha=1.0)

    # ------------------------------------------------------------------------------------------ MXFP8
    def _mx_quant(self, src_ptr, ld, M, K, batch=1, sSrc=0, rows_alloc=None):
        """bf16 rows -> (elements uint8 [batch, rows_alloc, K], scales uint8 [batch, rows_alloc, K / 32]); the first M rows of every
        batch entry are written."""
        R = rows_alloc or M
        q, sc = self.empty(batch, R, K, dtype=torch.uint8), self.empty(batch, R, K // 32, dtype=torch.uint8)
        self._launch("md_mx_quant_rows", src_ptr, ld, 1, q.data_ptr(), K, sc.data_ptr(), K // 32, M, K, batch, sSrc, R * K, R * (K // 32),
                     prof="mx_quant", nbytes=3.0 * M * K * batch)
        return q, sc

    def _mx_gemm(self, xq, ent, out_ptr, M, N, K, *, ldc, mode=hip.EPI_STORE_BF16, act=0, bias=None, res=None, ldr=0, gate=None, ldg=0,
                 rps=0, C2=None, ldc2=0, batch=1, sC=0):
        q, sc = xq
        rows = q.shape[1]
        a = hip.GemmMxArgs(q.data_ptr(), ent.q.data_ptr(), sc.data_ptr(), ent.s.data_ptr(), out_ptr, C2, bias, res, gate, M, N, K,
                           K, K, K // 32, K // 32, ldc, ldc2, ldr, ldg, rows * K, N * K, rows * (K // 32), N * (K // 32), sC, 0, 0, rps,
                           batch, mode, act, 0)
        self._launch("md_gemm_mxfp8", byref(a))

    def _expert_gemm(self, wname, A, C, M, N, K, Bk, E, *, act=0, C2=None, dact_cached=0):
        """C[e] = act(A[e] @ W[e]) for the expert tensor W [E, K, N] (contraction strided): MXFP8 when `wname` is in self.mx (the caller
        then passes no C2: inference), else the bf16 launch."""
        ent = self.mx.entries.get(wname) if self.mx is not None else None
        if ent is not None:
            assert ent.batch == E and (ent.N, ent.K) == (N, K) and C2 is None, wname
            xq = self._mx_quant(A.data_ptr(), K, M, K, batch=E, sSrc=Bk * K, rows_alloc=Bk)
            self._mx_gemm(xq, ent, C.data_ptr(), M, N, K, ldc=N, act=act, batch=E, sC=Bk * N)
            if self.mx_log is not None:
                self.mx_log.append((wname, "mx"))
            return
        if self.mx_log is not None:
            self.mx_log.append((wname, "bf16"))
        c2 = C2 is not None
        self._gemm(A=A.data_ptr(), B=self.S[wname].data_ptr(), C=C.data_ptr(), C2=_p(C2), M=M, N=N, K=K, lda=K, ldb=N, ldc=N,
                   ldc2=N if c2 else 0, sA=Bk * K, sB=K * N, sC=Bk * N, sC2=Bk * N if c2 else 0, batch=E, ksplit=1, a_kcontig=1, b_kcontig=0,
                   mode=hip.EPI_STORE_BF16, act=act, alpha=1.0, dact_cached=dact_cached)

    def lin_dgrad(self, dy, wname, dx, M, N, K, *, lddy=None, mode=hip.EPI_STORE_BF16, act=0, aux=None, res=None,
                  dyoff=0):
        """dx[M,K] (=|+=) dy[M,N] @ W[N,K]   (contraction over N; W is the K-strided operand)."""
        self._gemm(A=dy.data_ptr() + 2 * dyoff, B=self.S[wname + ".weight"].data_ptr(), C=dx.data_ptr(), aux=_p(aux),
                   res=_p(res), M=M, N=K, K=N, lda=lddy or N, ldb=K, ldc=K, ldaux=K, ldr=K, batch=1, ksplit=1,
                   a_kcontig=1, b_kcontig=0, mode=mode, act=act, alpha=1.0)

    def _fused12(self, pre):
        """True when w1.weight and w2.weight of a SwiGLU FFN are adjacent in the flat buffers (no biases in between), so
        [w1; w2] is one [2f, d] matrix: forward, dgrad and wgrad then run as ONE GEMM each."""
        w1, w2 = self.S.get(pre + ".w1.weight"), self.S.get(pre + ".w2.weight")
        if w1 is None or w2 is None or (pre + ".w1.bias") in self.P:
            return False
        return (w2.data_ptr() == w1.data_ptr() + w1.numel() * 2 and
                self.G[pre + ".w2.weight"].data_ptr() == self.G[pre + ".w1.weight"].data_ptr() + w1.numel() * 4)

    def _swiglu_ffn_fwd(self, pre, xin, rows, d, f, t, *, res, out=None, gate=None, ldg=0, rps=0, C2=None):
        """res + [gate *] w3(silu(w1 x) * w2 x) for xin [rows, d] (FeedForward, dit.py:88-89); saves h12 = [w1 x | w2 x] and a on tape t.
        out: the caller's buffer (the DiT block allocates it in front of the tape's), else allocated here, behind a."""
        t.h12 = self.empty(rows, 2 * f)
        if self._fused12(pre):
            self.lin_fwd(xin, pre + ".w1", t.h12, rows, 2 * f, d)          # [w1; w2] as one [2f, d] weight
        else:
            self.lin_fwd(xin, pre + ".w1", t.h12, rows, f, d, ldc=2 * f)
            self.lin_fwd(xin, pre + ".w2", t.h12, rows, f, d, ldc=2 * f, ooff=f)
        ent = self.mx.entries.get(pre + ".w3") if self.mx is not None else None
        if ent is not None and ent.batch == 1 and (ent.N, ent.K) == (d, f):
            # a = silu(h1) * h2 leaves the SwiGLU kernel as MXFP8, the form the w3 GEMM reads: the bf16 a is never written
            t.a = None
            aq, asc = self.empty(1, rows, f, dtype=torch.uint8), self.empty(1, rows, f // 32, dtype=torch.uint8)
            self._launch("md_swiglu_fwd_mx", t.h12.data_ptr(), 2 * f, aq.data_ptr(), f, asc.data_ptr(), f // 32, rows, f, prof="swiglu",
                         nbytes=5.0 * rows * f)
            if out is None:
                out = self.empty(rows, d)
            self.lin_fwd(None, pre + ".w3", out, rows, d, f, mode=hip.EPI_RESIDUAL, res=res, gate=gate, ldg=ldg, rps=rps, C2=C2, xq=(aq, asc))
            return out
        t.a = self.empty(rows, f)
        self._launch("md_swiglu_fwd", t.h12.data_ptr(), 2 * f, t.a.data_ptr(), f, rows, f, prof="swiglu", nbytes=6.0 * rows * f)
        if out is None:
            out = self.empty(rows, d)
        self.lin_fwd(t.a, pre + ".w3", out, rows, d, f, mode=hip.EPI_RESIDUAL, res=res, gate=gate, ldg=ldg, rps=rps, C2=C2)
        return out

    def _swiglu_ffn_bwd(self, pre, t, dout, xin, rows, d, f, *, defer, try_fused, dxin=None):
        """dout [rows, d], the gradient of the w3 output -> the gradient of xin (dxin: the caller's buffer, else allocated here), taking the
        weight gradients of w3 and [w1; w2] (defer: into the open group).  try_fused: first try da = dout @ W3 with the SwiGLU backward in
        the GEMM epilogue (EPI_SWIGLU_BWD; da never exists in memory); the library refuses ragged tiles or a CU hold: then two launches."""
        self.lin_wgrad(dout, t.a, pre + ".w3", rows, d, f, defer=defer)
        fused = False
        if try_fused:                      # (the two callers allocate in their own order: the arenas are bump allocators)
            dh12 = self.empty(rows, 2 * f)
            fused = self.fuse_swiglu_bwd and self._gemm(
                A=dout.data_ptr(), B=self.S[pre + ".w3.weight"].data_ptr(), C=dh12.data_ptr(), aux=t.h12.data_ptr(), M=rows, N=f, K=d, lda=d,
                ldb=f, ldc=2 * f, ldaux=2 * f, batch=1, ksplit=1, a_kcontig=1, b_kcontig=0, mode=hip.EPI_SWIGLU_BWD, act=0, alpha=1.0, _try=True)
        if not fused:
            da = self.empty(rows, f)
            self.lin_dgrad(dout, pre + ".w3", da, rows, d, f)
            if not try_fused:
                dh12 = self.empty(rows, 2 * f)
            self._launch("md_swiglu_bwd", da.data_ptr(), f, t.h12.data_ptr(), 2 * f, dh12.data_ptr(), 2 * f, rows, f, prof="swiglu",
                         nbytes=10.0 * rows * f)
        if dxin is None:
            dxin = self.empty(rows, d)
        if self._fused12(pre):
            if self._lora_grads:           # an adapter sits on w1 or w2, not on the stacked [w1; w2]: one call per half
                self.lin_wgrad(dh12, xin, pre + ".w1", rows, f, d, lddy=2 * f)
                self.lin_wgrad(dh12, xin, pre + ".w2", rows, f, d, lddy=2 * f, dyoff=f)
            else:
                self.lin_wgrad(dh12, xin, pre + ".w1", rows, 2 * f, d, defer=defer)
            self.lin_dgrad(dh12, pre + ".w1", dxin, rows, 2 * f, d)
        else:
            self.lin_wgrad(dh12, xin, pre + ".w1", rows, f, d, lddy=2 * f, defer=defer)
            self.lin_wgrad(dh12, xin, pre + ".w2", rows, f, d, lddy=2 * f, dyoff=f, defer=defer)
            self.lin_dgrad(dh12, pre + ".w1", dxin, rows, f, d, lddy=2 * f)
            self.lin_dgrad(dh12, pre + ".w2", dxin, rows, f, d, lddy=2 * f, dyoff=f, mode=hip.EPI_RESIDUAL, res=dxin)
        return dxin

    def _ksplit(self, out_rows, out_cols, contraction, batch=1):
        """Split-K factor of a GEMM too small to fill the chip: splitk.choose_ksplit with this engine's workspace and A/B switches."""
        return splitk.choose_ksplit(out_rows, out_cols, contraction, batch, ws_floats=self.ws.numel(), target_blocks=self.wgrad_target_blocks,
                                    min_items=self.ksplit_min_items, short_k_accum=self.short_k_accum)

    def gemm_f32_acc(self, *, out_ptr, M, N, K, ldo, batch=1, sOut=0, accumulate=True, **operands):
        """fp32 C (+)= A B^T with automatic split-K: partial products go to a workspace as dense fp32 slices and are
        summed by md_splitk_reduce (deterministic; float atomics measured 4-10x slower on this shape class)."""
        ks = self._ksplit(M, N, K, batch)
        via_ws = ks != 1
        if ks == -1:                      # enough tiles without splitting: one slice through the workspace on pp256
            ks, via_ws = 1, self.single_slice_ws
        bf_ptr = self._wgrad_bf16_target(out_ptr, M * N * batch if sOut in (0, M * N) and ldo == N else None) if accumulate else None
        if bf_ptr is not None and not via_ws and ldo % 8:
            via_ws = True                 # a bf16 row pitch the GEMM epilogue cannot store (16-byte pieces): one slice + the reduction
        if not via_ws:
            mode = hip.EPI_STORE_BF16 if bf_ptr is not None else hip.EPI_ACCUM_F32 if accumulate else hip.EPI_STORE_F32
            self._gemm(C=bf_ptr or out_ptr, M=M, N=N, K=K, ldc=ldo, sC=sOut, batch=batch, ksplit=1, mode=mode, act=0, alpha=1.0, **operands)
            return
        if self.splitk_force_pp and self.gemm_prefer == hip.GEMM_AUTO:
            operands = dict(operands, variant=hip.GEMM_PP256)
        self._gemm(C=self.ws.data_ptr(), M=M, N=N, K=K, ldc=N, sC=ks * M * N, sSplit=M * N, batch=batch, ksplit=ks,
                   mode=hip.EPI_STORE_F32, act=0, alpha=1.0, **operands)
        mode, nbytes = (2, M * N * batch * (4.0 * ks + 2)) if bf_ptr is not None else (int(accumulate), 4.0 * M * N * batch * (ks + 1 + int(accumulate)))
        self._launch("md_splitk_reduce", self.ws.data_ptr(), bf_ptr or out_ptr, M, N, ldo, sOut, ks, batch, mode, prof="splitk_reduce", nbytes=nbytes)

    def _acc_each(self, out_ptr, M, N, K, pairs, *, lda, ldb, a_kcontig):
        """out[M, N] += A_i B_i^T, one gemm_f32_acc per (A, B) pair with B K-strided: what a grouped launch falls back to."""
        for A, B in pairs:
            self.gemm_f32_acc(out_ptr=out_ptr, M=M, N=N, K=K, ldo=N, A=A, B=B, lda=lda, ldb=ldb, a_kcontig=a_kcontig, b_kcontig=0)

    def _wgrad_bf16_target(self, out_ptr, numel):
        """Address in the bf16 exchange buffer a weight gradient of this step is stored at, or None (not a one-microbatch step, the
        output is not a gradient accumulator, or the tensor is not dense).  A second gradient for the same tensor within one backward
        would have to be ADDED: no layer of the model does that; it raises instead of silently dropping the first."""
        t = self.wgrad_bf16
        if t is None or numel is None or not (t["g_lo"] <= out_ptr < t["g_hi"]):
            return None
        if out_ptr in t["written"]:
            raise RuntimeError("two weight gradients for one tensor in a one-microbatch step: the bf16 store path cannot accumulate")
        t["written"][out_ptr] = numel          # fp32 address -> elements stored from there (may span adjacent tensors: [w1; w2])
        return t["gbf"] + (out_ptr - t["g_lo"]) // 2

    def lin_wgrad(self, dy, x, wname, M, N, K, *, lddy=None, ldx=None, dyoff=0, xoff=0, bias_from=None, defer=False):
        """grad W[N,K] += dy[M,N]^T @ x[M,K]  (both operands K-strided; split-K over the token dimension);
        grad b[N] += column sums of dy.
        defer: with a weight-gradient group open (_wgrad_begin), only record the problem -- the whole group runs as ONE grouped
        launch at _wgrad_flush().  The caller guarantees that dy and x are not modified before the flush."""
        if not self._param_grads:
            if self._lora_grads and self.lora.is_target(wname + ".weight"):      # at once: dy and x are valid at the call
                self.lora.wgrad(wname + ".weight", dy.data_ptr() + 2 * dyoff, lddy or N, x.data_ptr() + 2 * xoff, ldx or K, M)
            return
        gb = self.G.get(wname + ".bias")
        if gb is not None:
            src = dy if bias_from is None else bias_from
            self._colsum(src.data_ptr() + (0 if bias_from is not None else 2 * dyoff), 1 if src.dtype == F32 else 0, lddy or N,
                         gb.data_ptr(), M, N)
        grp = self._wgroup
        if defer and grp is not None and M % 128 == 0 and K % 8 == 0 and (not grp or grp[0]["tokens"] == M) and len(grp) < hip.GEMM_MAX_PROBLEMS:
            grp.append(dict(tokens=M, A=dy.data_ptr() + 2 * dyoff, lda=lddy or N, B=x.data_ptr() + 2 * xoff, ldb=ldx or K, M=N, N=K,
                            out=self.G[wname + ".weight"].data_ptr(), keep=(dy, x)))
            return
        self._acc_each(self.G[wname + ".weight"].data_ptr(), N, K, M, [(dy.data_ptr() + 2 * dyoff, x.data_ptr() + 2 * xoff)],
                       lda=lddy or N, ldb=ldx or K, a_kcontig=0)

    def _param_acc(self, **kw):
        """gemm_f32_acc into a tensor of self.G (the weight gradients that are not a Linear's: experts, patch embedding)."""
        if self._param_grads:
            self.gemm_f32_acc(**kw)

    def _param_colsum(self, *a):
        if self._param_grads:
            self._colsum(*a)

    def _wgrad_begin(self):
        self._wgroup = [] if self.group_wgrad else None

    def _wgrad_flush(self):
        """Run the recorded weight gradients (same token count) as ONE grouped pp256 launch: their output tiles share the 256
        workgroups, so the split over the tokens only has to fill what ALL of them leave empty (ks = 2..8 instead of 8..16 each),
        the fp32 slices mirror the layout of the gradient tensors, and one flat reduction per contiguous run finishes them."""
        grp, self._wgroup = self._wgroup, ([] if self._wgroup is not None else None)
        if not grp:
            return
        grp.sort(key=lambda g: g["out"])
        plan = splitk.plan_wgrad_group([(g["out"], g["M"], g["N"]) for g in grp], grp[0]["tokens"], self.ws.numel())
        if plan is None:                                # a single problem, or the slices do not fit the workspace: one by one
            for g in grp:
                self._acc_each(g["out"], g["M"], g["N"], g["tokens"], [(g["A"], g["B"])], lda=g["lda"], ldb=g["ldb"], a_kcontig=0)
            return
        ks, base = plan.ks, grp[0]["out"]
        probs = (hip.GemmProblem * len(grp))(*(hip.GemmProblem(g["A"], g["B"], g["lda"], g["ldb"], g["M"], g["N"], off)
                                               for g, off in zip(grp, plan.offsets)))
        g0 = grp[0]
        self._gemm(A=g0["A"], B=g0["B"], C=self.ws.data_ptr(), M=g0["M"], N=g0["N"], K=g0["tokens"], lda=g0["lda"], ldb=g0["ldb"], ldc=g0["N"],
                   sSplit=plan.span, batch=1, ksplit=ks, a_kcontig=0, b_kcontig=0, mode=hip.EPI_STORE_F32, act=0, alpha=1.0,
                   problems=ctypes.addressof(probs), n_problems=len(grp), _problems=grp)
        bf = [self._wgrad_bf16_target(g["out"], g["M"] * g["N"]) for g in grp]
        to_bf16 = all(b is not None for b in bf)
        assert to_bf16 or not any(b is not None for b in bf)        # a group lies in the gradient buffer as a whole, or not at all
        t = self.wgrad_bf16
        for off, n in plan.runs:                                    # one flat reduction per contiguous run of gradient tensors
            lo = base + 4 * off
            dst, mode, nbytes = (t["gbf"] + (lo - t["g_lo"]) // 2, 2, n * (4.0 * ks + 2)) if to_bf16 else (lo, 1, 4.0 * n * (ks + 2))
            self._launch("md_splitk_reduce_flat", self.ws.data_ptr() + 4 * off, dst, n, plan.span, ks, mode, prof="splitk_reduce", nbytes=nbytes)

    def ln_args(self, x, wname, out, rows, C, *, shift=None, scale=None, ldmod=0, rps=0, mean=None, rstd=None, act=0,
                pos=None, pos_rows=0):
        return hip.LnArgs(x.data_ptr(), _p(self.P[wname + ".weight"]) if wname else None, shift, scale, _p(pos), _p(out),
                          _p(mean), _p(rstd), rows, C, C, C, ldmod, rps, pos_rows, self.cfg.norm_eps, act)

    def ln_fwd(self, a):
        self._launch("md_ln_fwd", byref(a), prof="layernorm", nbytes=4.0 * a.rows * a.C)

    @staticmethod
    def _rows_per_block(rows, rps, min_blocks=2048):
        """Rows of one sample per workgroup for the column-reducing backward kernels: aim at >= `min_blocks` workgroups
        (4 waves each) without dropping below 4 rows per workgroup (one per wave).  md_ln_bwd runs 4 workgroups per CU and ends each
        with an LDS reduction + 2 C atomics: 1024 workgroups (one full round) with twice the rows each beat 2048 -- 16,384 x 1024:
        35.5 -> 30.9 us, 65,536 x 1024: 100.3 -> 97.8, 65,536 x 768: 69.3 -> 68.1 (scripts/bench_norm.py --rpb-sweep)."""
        rpb = 64
        while rpb > 4 and (rows + rpb - 1) // rpb < min_blocks:
            rpb //= 2
        return int(max(1, min(rpb, rps)))

    def ln_bwd(self, a, dz, dx, *, accumulate, wname=None, dscale=None, dshift=None, ldg=0):
        """LayerNorm(+modulate) backward.  dscale / dshift: raw pointers into the (zeroed) fp32 adaLN gradient buffer for
        modulated norms; plain norms get a zeroed [samples, C] scratch for the per-sample sums the weight grad is
        finished from."""
        rps = a.rows_per_sample if a.rows_per_sample > 0 else a.rows
        rpb = self._rows_per_block(a.rows, rps, 1024)
        if not self._param_grads:
            wname = None                   # no weight gradient: a plain norm needs no per-sample sums either (dscale stays None)
        is_out = 1 if dscale is not None else 0
        if dscale is None and wname is not None:
            scratch = self.zeros(a.rows // rps, a.C)
            dscale, ldg = scratch.data_ptr(), a.C
        b = hip.LnBwdArgs(dz.data_ptr(), _p(dx), dscale, dshift, _p(self.G[wname + ".weight"]) if wname else None,
                          a.C, a.C, ldg, rpb, 1 if accumulate else 0, is_out)
        self._launch_det("md_ln_bwd", (hip.DET_LN_BWD, a.rows, rps, rpb, a.C), byref(a), byref(b), prof="layernorm",
                         nbytes=(8.0 if accumulate else 6.0) * a.rows * a.C)

    def attn_args(self, q, k, v, o, lse, B, H, Sq, Skv, ldq, ldk, ldv, hid, *, do=None, dq=None, dk=None, dv=None,
                  delta=None, lddq=0, lddk=0, lddv=0, hm_qk=False):
        """hm_qk: q, k (and dq, dk) are head-major [B, H, S, hd] buffers (ldq / ldk / lddq / lddk are ignored)."""
        hd = self.cfg.head_dim
        a = hip.AttnArgs(q, k, v, _p(o), _p(lse), _p(do), dq, dk, dv, _p(delta), B, H, Sq, Skv, ldq, ldk, ldv, hid,
                         Sq * ldq, Skv * ldk, Skv * ldv, Sq * hid, lddq, lddk, lddv, hid, Sq * lddq, Skv * lddk,
                         Skv * lddv, Sq * hid, 1.0 / math.sqrt(hd), hd, 0)
        if hm_qk:
            a.ldq = a.ldk = a.lddq = a.lddk = hd
            a.sq = a.sdq = H * Sq * hd
            a.sk = a.sdk = H * Skv * hd
            a.hsq = a.hsdq = Sq * hd
            a.hsk = a.hsdk = Skv * hd
        return a

    def _attn_bwd(self, a):
        self._prof("attention", 2.0 * a.hd * (4 * a.Sq + 4 * a.Skv) * a.B * a.H, lambda: self._attn_bwd_launch(a))

    def _attn_bwd_launch(self, a):
        rc = -1
        if self.attn_bwd_prefer != hip.ATTN_BWD_AUTO:
            a.bwd_split = self.attn_bwd_prefer
            rc = self.L.md_attn_bwd(byref(a), self._st())     # -1: the forced kernel does not cover this problem (nothing launched)
            a.bwd_split = hip.ATTN_BWD_AUTO
        if rc == -1:
            rc = self.L.md_attn_bwd(byref(a), self._st())
        hip.check(rc, "md_attn_bwd")

    # ------------------------------------------------------------------------------------------ attention layers
    def _self_attn_fwd(self, pre, xin, B, S, dim, hid, heads, t):
        """xin [B*S, dim] -> o [B*S, hid]; saves qkv (post-LN), rstd, lse on tape t."""
        M = B * S
        qkv = self.empty(M, 3 * hid)
        self.lin_fwd(xin, pre + ".qkv", qkv, M, 3 * hid, dim)
        rq = self.empty(2, M, dtype=F32)
        o = self.empty(M, hid)
        lse = self.empty(B, heads, S, dtype=F32)
        if self.qk_head_major:
            t.qk = self.empty(2, M, hid)          # normalised q, k: [2][B, H, S, hd]; qkv keeps the raw q / k (dead) and v
            self._qkln_fwd_hm(qkv.data_ptr(), M, 3 * hid, 0, hid, t.qk, S, rq.data_ptr(), nseg=2)
            a = self.attn_args(t.qk.data_ptr(), t.qk.data_ptr() + 2 * M * hid, qkv.data_ptr() + 4 * hid, o, lse, B, heads, S, S,
                               0, 0, 3 * hid, hid, hm_qk=True)
        else:
            t.qk = None
            self._qkln_fwd(qkv.data_ptr(), M, 3 * hid, 0, hid, rq.data_ptr(), nseg=2)
            a = self.attn_args(qkv.data_ptr(), qkv.data_ptr() + 2 * hid, qkv.data_ptr() + 4 * hid, o, lse, B, heads, S, S,
                               3 * hid, 3 * hid, 3 * hid, hid)
        self._attn_fwd(a)
        t.qkv, t.rq, t.o, t.lse = qkv, rq, o, lse
        return o

    def _self_attn_bwd(self, pre, xin, do, B, S, dim, hid, heads, t, defer=False):
        """do [M, hid] -> returns d_xin [M, dim]; accumulates the qkv weight grad."""
        M = B * S
        dqkv = self.empty(M, 3 * hid)
        delta = self.empty(B, heads, S, dtype=F32)
        qkv = t.qkv
        if t.qk is not None:
            dqk = self.empty(2, M, hid)           # dL/d(normalised q, k), head-major like t.qk
            a = self.attn_args(t.qk.data_ptr(), t.qk.data_ptr() + 2 * M * hid, qkv.data_ptr() + 4 * hid, t.o, t.lse, B, heads, S, S,
                               0, 0, 3 * hid, hid, do=do, dq=dqk.data_ptr(), dk=dqk.data_ptr() + 2 * M * hid,
                               dv=dqkv.data_ptr() + 4 * hid, delta=delta, lddv=3 * hid, hm_qk=True)
            self._attn_bwd(a)
            self._qkln_bwd_hm(dqk, t.qk, dqkv.data_ptr(), 3 * hid, 0, M, hid, S, t.rq.data_ptr(), nseg=2)
        else:
            a = self.attn_args(qkv.data_ptr(), qkv.data_ptr() + 2 * hid, qkv.data_ptr() + 4 * hid, t.o, t.lse, B, heads, S, S,
                               3 * hid, 3 * hid, 3 * hid, hid, do=do, dq=dqkv.data_ptr(), dk=dqkv.data_ptr() + 2 * hid,
                               dv=dqkv.data_ptr() + 4 * hid, delta=delta, lddq=3 * hid, lddk=3 * hid, lddv=3 * hid)
            self._attn_bwd(a)
            self._qkln_bwd(dqkv.data_ptr(), 3 * hid, 0, qkv.data_ptr(), 3 * hid, 0, M, hid, t.rq.data_ptr(), nseg=2)
        self.lin_wgrad(dqkv, xin, pre + ".qkv", M, 3 * hid, dim, defer=defer)
        dxin = self.empty(M, dim)
        self.lin_dgrad(dqkv, pre + ".qkv", dxin, M, 3 * hid, dim)
        return dxin

    # ------------------------------------------------------------------------------------------ DiT block
    def _kv_linear_fwd(self, n, ycond, Mc, hx, d):
        """Packed [K | V] rows of a block's cross-attention from the caption tokens (utils.py:172-176)."""
        kv = self.empty(Mc, 2 * hx)
        self.lin_fwd(ycond, n + ".cross_attn.kv_linear", kv, Mc, 2 * hx, d)
        return kv

    def _k_norm_fwd(self, kv, Mc, hx, Lc):
        """QK-LayerNorm of the K half of kv: in place, or (head-major layout) to a [B, H, Lc, hd] buffer.  Returns (rstd, that buffer or None)."""
        rk = self.empty(Mc, dtype=F32)
        if self.qk_head_major:
            kn = self.empty(Mc, hx)
            self._qkln_fwd_hm(kv.data_ptr(), Mc, 2 * hx, 0, hx, kn, Lc, rk.data_ptr())
            return rk, kn
        self._qkln_fwd(kv.data_ptr(), Mc, 2 * hx, 0, hx, rk.data_ptr())
        return rk, None

    def _block_fwd(self, bp: BlockPlan, x, ycond, B, S, Lc, gc, mod_all=None, kv=None, keep=None, out_rows=None):
        """kv: this block's entry of Conditioning.kv -- the caption-side projection and its K-LayerNorm are then skipped (ycond is not
        read; inference only: the tape holds no K rstd for a backward).
        keep: (ids_restore [B, S] int32, Tk) when only the tokens with ids_restore < Tk of this block's output are ever read (the
        last patch-mixer block under masking): a MoE block then runs its experts on the routed rows of those tokens alone.
        out_rows: tp.keep_rows when this block's S rows are the kept tokens of a masked pass (backbone blocks), else None: the row of the
        full token grid each of its rows stands for, which only attn_probe reads."""
        cfg = self.cfg
        d, h, hx, f = bp.dim, bp.attn_hidden, bp.xattn_hidden, bp.ffn_hidden
        M, Mc, D = B * S, B * Lc, cfg.dim
        n = bp.name
        t = Tape()
        t.x = x
        if mod_all is not None:              # this block's columns of the batched modulation GEMM (leading dimension N_all)
            mod, ldm = mod_all, mod_all.shape[1]
            mp = mod_all.data_ptr() + 2 * self._adaln["col"][n]
        else:
            mod, ldm = self.empty(B, 6 * d), 6 * d
            self.lin_fwd(gc, n + ".adaLN_modulation.1", mod, B, 6 * d, D)
            mp = mod.data_ptr()
        t.mod, t.mp, t.ldm = mod, mp, ldm
        # -- self attention: x1 = x + gate_msa * proj(attn(modulate(LN1(x))))
        t.xm1 = self.empty(M, d)
        t.st1 = self.empty(2, M, dtype=F32)
        a1 = self.ln_args(x, n + ".norm1", t.xm1, M, d, shift=mp, scale=mp + 2 * d, ldmod=ldm, rps=S, mean=t.st1[0], rstd=t.st1[1])
        self.ln_fwd(a1)
        t.sa = Tape()
        o = self._self_attn_fwd(n + ".attn", t.xm1, B, S, d, h, bp.heads, t.sa)
        t.br1 = self.empty(M, d)
        x1 = self.empty(M, d)
        self.lin_fwd(o, n + ".attn.proj", x1, M, d, h, mode=hip.EPI_RESIDUAL, res=x, gate=mp + 2 * 2 * d, ldg=ldm, rps=S,
                     C2=t.br1)
        t.x1 = x1
        # -- cross attention: x2 = x1 + proj(attn(q(LN2(x1)), kv(y)))
        t.xn2 = self.empty(M, d)
        t.st2 = self.empty(2, M, dtype=F32)
        self.ln_fwd(self.ln_args(x1, n + ".norm2", t.xn2, M, d, mean=t.st2[0], rstd=t.st2[1]))
        t.o2 = self.empty(M, hx)
        # head-major: the raw q is dead once md_qkln_fwd_hm has read it -- it is staged in the buffer attention then writes o into
        t.q2 = t.o2 if self.qk_head_major else self.empty(M, hx)
        self.lin_fwd(t.xn2, n + ".cross_attn.q_linear", t.q2, M, hx, d)
        if kv is None:
            t.kv = self._kv_linear_fwd(n, ycond, Mc, hx, d)
        else:
            t.kv, t.k2n = kv
            t.rk2 = None
        t.rq2 = self.empty(M, dtype=F32)
        t.lse2 = self.empty(B, bp.xheads, S, dtype=F32)
        if self.qk_head_major:
            t.q2n = self.empty(M, hx)                                   # normalised q [B, H, S, hd] (k: [B, H, Lc, hd])
            self._qkln_fwd_hm(t.q2.data_ptr(), M, hx, 0, hx, t.q2n, S, t.rq2.data_ptr())
            if kv is None:
                t.rk2, t.k2n = self._k_norm_fwd(t.kv, Mc, hx, Lc)
            ax = self.attn_args(t.q2n.data_ptr(), t.k2n.data_ptr(), t.kv.data_ptr() + 2 * hx, t.o2, t.lse2, B, bp.xheads, S, Lc,
                                0, 0, 2 * hx, hx, hm_qk=True)
        else:
            t.q2n = None
            self._qkln_fwd(t.q2.data_ptr(), M, hx, 0, hx, t.rq2.data_ptr())
            if kv is None:
                t.rk2, t.k2n = self._k_norm_fwd(t.kv, Mc, hx, Lc)
            ax = self.attn_args(t.q2.data_ptr(), t.kv.data_ptr(), t.kv.data_ptr() + 2 * hx, t.o2, t.lse2, B, bp.xheads, S, Lc,
                                hx, 2 * hx, 2 * hx, hx)
        self._attn_fwd(ax, self.caption_bias)
        if self.attn_probe is not None:
            self.attn_probe.record(n, ax, B, S, Lc, out_rows, self.caption_bias)
        x2 = self.empty(M, d)
        self.lin_fwd(t.o2, n + ".cross_attn.proj", x2, M, d, hx, mode=hip.EPI_RESIDUAL, res=x1)
        t.x2 = x2
        # -- feed-forward: x3 = x2 + gate_mlp * mlp(modulate(LN3(x2)))
        t.xm3 = self.empty(M, d)
        t.st3 = self.empty(2, M, dtype=F32)
        self.ln_fwd(self.ln_args(x2, n + ".norm3", t.xm3, M, d, shift=mp + 2 * 3 * d, scale=mp + 2 * 4 * d, ldmod=ldm,
                                 rps=S, mean=t.st3[0], rstd=t.st3[1]))
        x3 = self.empty(M, d)
        t.br3 = self.empty(M, d)
        gate_mlp = mp + 2 * 5 * d
        if not bp.moe:
            self._swiglu_ffn_fwd(n + ".mlp", t.xm3, M, d, f, t, out=x3, res=x2, gate=gate_mlp, ldg=ldm, rps=S, C2=t.br3)
        else:
            E = cfg.num_experts
            k = int(cfg.expert_capacity * S / E)
            ldl = 8 if E <= 8 else 16
            Bk = B * k
            t.k, t.ldl = k, ldl
            logits = self.empty(M, ldl, dtype=F32)
            self.lin_fwd(t.xm3, n + ".mlp.gate", logits, M, E, d, ldc=ldl, mode=hip.EPI_STORE_F32)
            t.probs = self.empty(M, ldl, dtype=F32)
            t.rowidx = self.empty(E, Bk, dtype=I32)
            t.gval = self.empty(E, Bk, dtype=F32)
            t.slot = self.empty(M, E, dtype=I32)
            self._launch("md_moe_route", logits.data_ptr(), t.probs.data_ptr(), ldl, B, S, E, k, t.rowidx.data_ptr(), t.gval.data_ptr(),
                         t.slot.data_ptr())
            if self.route_override is not None and n in self.route_override:
                self._override_routing(t, self.route_override[n], B, S, E, k)
            if self.route_stats is not None:    # after the injection: the statistics describe the routing the layer runs with
                self.route_stats.record(n, t.slot, t.probs, ldl, t.gval, B, S, k)
            # rows per expert the expert GEMMs run on: Bk, or -- pruned -- the first `cap` rows of the compact lists.  Buffer sizes do
            # not depend on cap (the arenas are sized on the first pass); only the launch extents do.
            t.cap = self._compact_kept(t, keep, B, S, E, k) if keep is not None else None
            rows = t.cap or Bk
            t.xin = self.empty(E, Bk, d)
            if t.cap is None:
                self._launch("md_gather_rows", t.xm3.data_ptr(), d, t.rowidx.data_ptr(), t.xin.data_ptr(), d, E * Bk, d)
            else:
                self._launch("md_moe_gather_compact", t.xm3.data_ptr(), d, t.rowidx_c.data_ptr(), t.xin.data_ptr(), E, rows, Bk, d)
            # the pre-activation -- or, with moe_cache_dact, gelu'(pre-activation): nothing but the backward's activation derivative ever
            # reads it (md_gemm_args.dact_cached), so an MXFP8 fc1 (inference only) neither allocates nor writes it
            mx_fc1 = self.mx is not None and (n + ".mlp.w1") in self.mx.entries
            t.hpre = None if mx_fc1 else self.empty(E, Bk, f)
            t.hact = self.empty(E, Bk, f)
            t.hpre_is_dact = 1 if self.moe_cache_dact else 0
            # w1 [E, d, f], w2 [E, f, d]: the contraction dimension is the strided one
            self._expert_gemm(n + ".mlp.w1", t.xin, t.hact, rows, f, d, Bk, E, act=hip.ACT_GELU_ERF, C2=t.hpre, dact_cached=t.hpre_is_dact)
            t.h2 = self.empty(E, Bk, d)
            self._expert_gemm(n + ".mlp.w2", t.hact, t.h2, rows, d, f, Bk, E)
            if t.cap is None:
                self._launch("md_moe_combine", t.h2.data_ptr(), t.gval.data_ptr(), t.slot.data_ptr(), x2.data_ptr(), gate_mlp, ldm, t.br3.data_ptr(),
                             x3.data_ptr(), B, S, E, k, d)
            else:       # every token row is written: a dropped token gets br3 = 0 and x3 = x2
                self._launch("md_moe_combine_abs", t.h2.data_ptr(), t.gval_c.data_ptr(), t.slot_c.data_ptr(), x2.data_ptr(), gate_mlp, ldm,
                             t.br3.data_ptr(), x3.data_ptr(), B, S, E, Bk, d)
            if self.route_log is not None:
                self.route_log += ["moe_route", "gather" if t.cap is None else "gather_compact", "combine" if t.cap is None else "combine_abs"]
        return x3, t

    def _compact_kept(self, t, keep, B, S, E, k):
        """Compact lists of the routed rows whose token survives the mask (md_moe_compact_kept; after any route_override) on the tape
        (rowidx_c, gval_c [E, B*k], slot_c [B*S, E]); returns the rows per expert the pruned GEMMs run on, or None: nothing to gain
        (the fullest expert needs all B*k rows once rounded up to the granule), the block runs dense.
        The per-expert counts come back through pinned memory and the host WAITS for them: the one synchronisation of the step path."""
        ids_restore, Tk = keep
        Bk = B * k
        t.rowidx_c = self.empty(E, Bk, dtype=I32)
        t.gval_c = self.empty(E, Bk, dtype=F32)
        t.slot_c = self.empty(B * S, E, dtype=I32)
        count = self.empty(16, dtype=I32)
        ws = self.empty(E * ((Bk + 1023) // 1024), dtype=I32)
        self._launch("md_moe_compact_kept", t.rowidx.data_ptr(), t.gval.data_ptr(), ids_restore.data_ptr(), Tk, B, S, E, k, t.rowidx_c.data_ptr(),
                     t.gval_c.data_ptr(), count.data_ptr(), t.slot_c.data_ptr(), ws.data_ptr(), ws.numel())
        if self.route_log is not None:
            self.route_log.append("compact_kept")
        if self._prune_host is None:
            self._prune_host = torch.empty(16, dtype=I32, pin_memory=True)
        t0 = time.perf_counter()
        self._prune_host[:E].copy_(count[:E], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        if self.prune_wait_us is not None:
            self.prune_wait_us.append((time.perf_counter() - t0) * 1e6)
        g = max(1, int(self.prune_granule))
        cap = max(1, -(-int(self._prune_host[:E].max()) // g)) * g
        return cap if cap < Bk else None

    def _override_routing(self, t, m_idx, B, S, E, k):
        """Parity-test hook (never on the product path): replace the expert-choice selection of one layer by given token
        indices [B, E, k] (the fp32 oracle's top-k), keeping this run's own probabilities as gate values, so that what remains
        of a difference to the oracle is arithmetic, not a slot ranked differently by bf16 gate logits."""
        m_idx = m_idx.to(self.dev).long()
        rows = (m_idx + (torch.arange(B, device=self.dev) * S).view(B, 1, 1)).permute(1, 0, 2).reshape(E, B * k)
        t.rowidx.copy_(rows.to(I32))
        ecol = torch.arange(E, device=self.dev).view(E, 1).expand(E, B * k)
        t.gval.copy_(t.probs[rows, ecol])
        slot = torch.full((B, S, E), -1, device=self.dev, dtype=I32)
        for e in range(E):
            slot[:, :, e].scatter_(1, m_idx[:, e, :], torch.arange(k, device=self.dev, dtype=I32).view(1, k).expand(B, k))
        t.slot.copy_(slot.view(B * S, E))

    def _block_bwd(self, bp: BlockPlan, t: Tape, dx, ycond, dycond_f32, B, S, Lc, gc, dgc_f32, group=None, kvgroup=None):
        """dx: grad w.r.t. the block output [M, d] (bf16), updated IN PLACE to the grad w.r.t. the block input."""
        cfg = self.cfg
        d, h, hx, f = bp.dim, bp.attn_hidden, bp.xattn_hidden, bp.ffn_hidden
        M, Mc, D = B * S, B * Lc, cfg.dim
        n = bp.name
        mp, ldm = t.mp, t.ldm
        self._wgrad_begin()
        dmod = self.zeros(B, 6 * d)          # fp32 grads of (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp)
        dmp = dmod.data_ptr()
        rpb = self._rows_per_block(M, S)
        # ---------------- feed-forward branch
        dbr3 = self.empty(M, d)
        self._gate_bwd(dx, t.br3, mp + 2 * 5 * d, ldm, dbr3, dmp + 4 * 5 * d, 6 * d, M, d, S, rpb)
        dxm3 = self.empty(M, d)
        if not bp.moe:
            self._swiglu_ffn_bwd(n + ".mlp", t, dbr3, t.xm3, M, d, f, defer=True, try_fused=True, dxin=dxm3)
        else:
            E, k, ldl = cfg.num_experts, t.k, t.ldl
            Bk = B * k
            w1, w2 = self.S[n + ".mlp.w1"], self.S[n + ".mlp.w2"]
            g1, g2 = self.G[n + ".mlp.w1"], self.G[n + ".mlp.w2"]
            dh2 = self.empty(E, Bk, d)
            dgval = self.empty(E, Bk, dtype=F32)
            # pruned (t.cap): the same launches on the first t.cap rows of every expert's compact list.  Pad rows have gate value 0, so
            # their dh2 -- and with it their dhpre, dxin and weight-gradient contributions -- is exactly 0; their dgval is never read.
            rows = t.cap or Bk
            if t.cap is None:
                self._launch("md_moe_combine_bwd", dbr3.data_ptr(), t.h2.data_ptr(), t.rowidx.data_ptr(), t.gval.data_ptr(), dh2.data_ptr(),
                             dgval.data_ptr(), E * Bk, d)
            else:
                self._launch("md_moe_combine_bwd_compact", dbr3.data_ptr(), t.h2.data_ptr(), t.rowidx_c.data_ptr(), t.gval_c.data_ptr(),
                             dh2.data_ptr(), dgval.data_ptr(), E, rows, Bk, d)
            # dW2[e][f, d] += hact[e]^T dh2[e]
            self._param_acc(out_ptr=g2.data_ptr(), M=f, N=d, K=rows, ldo=d, batch=E, sOut=f * d, A=t.hact.data_ptr(),
                            B=dh2.data_ptr(), lda=f, ldb=d, sA=Bk * f, sB=Bk * d, a_kcontig=0, b_kcontig=0)
            # dhpre = (dh2 @ W2[e]^T) * gelu'(hpre)
            dhpre = self.empty(E, Bk, f)
            self._gemm(A=dh2.data_ptr(), B=w2.data_ptr(), C=dhpre.data_ptr(), aux=t.hpre.data_ptr(), M=rows, N=f, K=d, lda=d,
                       ldb=d, ldc=f, ldaux=f, sA=Bk * d, sB=f * d, sC=Bk * f, sAux=Bk * f, batch=E, ksplit=1, a_kcontig=1,
                       b_kcontig=1, mode=hip.EPI_DACT, act=hip.ACT_GELU_ERF, alpha=1.0, dact_cached=t.hpre_is_dact)
            # dW1[e][d, f] += xin[e]^T dhpre[e]
            self._param_acc(out_ptr=g1.data_ptr(), M=d, N=f, K=rows, ldo=f, batch=E, sOut=d * f, A=t.xin.data_ptr(),
                            B=dhpre.data_ptr(), lda=d, ldb=f, sA=Bk * d, sB=Bk * f, a_kcontig=0, b_kcontig=0)
            # dxin = dhpre @ W1[e]^T
            dxin = self.empty(E, Bk, d)
            self._gemm(A=dhpre.data_ptr(), B=w1.data_ptr(), C=dxin.data_ptr(), M=rows, N=d, K=f, lda=f, ldb=f, ldc=d, sA=Bk * f,
                       sB=d * f, sC=Bk * d, batch=E, ksplit=1, a_kcontig=1, b_kcontig=1, mode=hip.EPI_STORE_BF16, act=0, alpha=1.0)
            dlog = self.empty(M, ldl)
            if t.cap is None:
                self._launch("md_moe_dispatch_bwd", dxin.data_ptr(), t.slot.data_ptr(), dxm3.data_ptr(), t.probs.data_ptr(), ldl, dgval.data_ptr(),
                             dlog.data_ptr(), ldl, B, S, E, k, d)
            else:       # every token row is written: a dropped token gets dxm3 = 0 and dlog = 0
                self._launch("md_moe_dispatch_bwd_abs", dxin.data_ptr(), t.slot_c.data_ptr(), dxm3.data_ptr(), t.probs.data_ptr(), ldl,
                             dgval.data_ptr(), dlog.data_ptr(), ldl, B, S, E, Bk, d)
            if self.route_log is not None:
                self.route_log += ["combine_bwd", "dispatch_bwd"] if t.cap is None else ["combine_bwd_compact", "dispatch_bwd_abs"]
            # gate: dWg[E, d] += dlog^T xm3 ; dxm3 += dlog @ Wg
            self.lin_wgrad(dlog, t.xm3, n + ".mlp.gate", M, E, d, lddy=ldl)
            self.lin_dgrad(dlog, n + ".mlp.gate", dxm3, M, E, d, lddy=ldl, mode=hip.EPI_RESIDUAL, res=dxm3)
        a3 = self.ln_args(t.x2, n + ".norm3", None, M, d, scale=mp + 2 * 4 * d, ldmod=ldm, rps=S, mean=t.st3[0], rstd=t.st3[1])
        self.ln_bwd(a3, dxm3, dx, accumulate=True, wname=n + ".norm3", dscale=dmp + 4 * 4 * d, dshift=dmp + 4 * 3 * d, ldg=6 * d)
        # ---------------- cross-attention branch (un-gated, un-modulated)
        self.lin_wgrad(dx, t.o2, n + ".cross_attn.proj", M, d, hx, defer=True)     # dx stays as it is until the flush below
        do2 = self.empty(M, hx)
        self.lin_dgrad(dx, n + ".cross_attn.proj", do2, M, d, hx)
        dq2 = self.empty(M, hx)
        dkv = self.empty(Mc, 2 * hx) if kvgroup is None else kvgroup.buf[len(kvgroup.w)]
        delta = self.empty(B, bp.xheads, S, dtype=F32)
        if t.q2n is not None:
            dq2n, dk2n = self.empty(M, hx), self.empty(Mc, hx)          # head-major like t.q2n / t.k2n
            ax = self.attn_args(t.q2n.data_ptr(), t.k2n.data_ptr(), t.kv.data_ptr() + 2 * hx, t.o2, t.lse2, B, bp.xheads, S, Lc, 0,
                                0, 2 * hx, hx, do=do2, dq=dq2n.data_ptr(), dk=dk2n.data_ptr(), dv=dkv.data_ptr() + 2 * hx,
                                delta=delta, lddv=2 * hx, hm_qk=True)
            self._attn_bwd(ax)
            self._qkln_bwd_hm(dq2n, t.q2n, dq2.data_ptr(), hx, 0, M, hx, S, t.rq2.data_ptr())
            if not self._x_only:
                self._qkln_bwd_hm(dk2n, t.k2n, dkv.data_ptr(), 2 * hx, 0, Mc, hx, Lc, t.rk2.data_ptr())
        else:
            ax = self.attn_args(t.q2.data_ptr(), t.kv.data_ptr(), t.kv.data_ptr() + 2 * hx, t.o2, t.lse2, B, bp.xheads, S, Lc, hx,
                                2 * hx, 2 * hx, hx, do=do2, dq=dq2.data_ptr(), dk=dkv.data_ptr(), dv=dkv.data_ptr() + 2 * hx,
                                delta=delta, lddq=hx, lddk=2 * hx, lddv=2 * hx)
            self._attn_bwd(ax)
            self._qkln_bwd(dq2.data_ptr(), hx, 0, t.q2.data_ptr(), hx, 0, M, hx, t.rq2.data_ptr())
            if not self._x_only:
                self._qkln_bwd(dkv.data_ptr(), 2 * hx, 0, t.kv.data_ptr(), 2 * hx, 0, Mc, hx, t.rk2.data_ptr())
        self.lin_wgrad(dq2, t.xn2, n + ".cross_attn.q_linear", M, hx, d, defer=True)
        # (stopping at the image, _x_only: dK / dV of the fused attention backward are not consumed -- no K-LayerNorm backward above, no
        # kv_linear gradient of either kind below, so a frozen conditioning needs neither the K rstd nor the caption tokens)
        if not self._x_only:
            self.lin_wgrad(dkv, ycond, n + ".cross_attn.kv_linear", Mc, 2 * hx, d)
        # d(ycond) accumulates in fp32 over all blocks that attend to these caption tokens: per block (split-K slices + a
        # reduction pass into the [B*L, d] fp32 buffer, 28 times), or -- kvgroup -- deferred: dkv of every block is kept and ONE
        # launch contracts the concatenation [dkv_0 | dkv_1 | ...] with [Wkv_0; Wkv_1; ...] (_dycond_grouped)
        if self._x_only:
            pass
        elif kvgroup is None:
            self._acc_each(dycond_f32.data_ptr(), Mc, d, 2 * hx, [(dkv.data_ptr(), self.S[n + ".cross_attn.kv_linear.weight"].data_ptr())],
                           lda=2 * hx, ldb=d, a_kcontig=1)
        else:
            kvgroup.w.append(self.S[n + ".cross_attn.kv_linear.weight"].data_ptr())
        dxn2 = self.empty(M, d)
        self.lin_dgrad(dq2, n + ".cross_attn.q_linear", dxn2, M, hx, d)
        self._wgrad_flush()                  # w3, [w1; w2], cross_attn.proj, q_linear -- before dx (cross_attn.proj's dy) is updated
        a2 = self.ln_args(t.x1, n + ".norm2", None, M, d, mean=t.st2[0], rstd=t.st2[1], rps=S)
        self.ln_bwd(a2, dxn2, dx, accumulate=True, wname=n + ".norm2")
        # ---------------- self-attention branch
        dbr1 = self.empty(M, d)
        self._gate_bwd(dx, t.br1, mp + 2 * 2 * d, ldm, dbr1, dmp + 4 * 2 * d, 6 * d, M, d, S, rpb)
        self.lin_wgrad(dbr1, t.sa.o, n + ".attn.proj", M, d, h, defer=True)
        do = self.empty(M, h)
        self.lin_dgrad(dbr1, n + ".attn.proj", do, M, d, h)
        dxm1 = self._self_attn_bwd(n + ".attn", t.xm1, do, B, S, d, h, bp.heads, t.sa, defer=True)
        self._wgrad_flush()                  # attn.proj, attn.qkv
        a1 = self.ln_args(t.x, n + ".norm1", None, M, d, scale=mp + 2 * d, ldmod=ldm, rps=S, mean=t.st1[0], rstd=t.st1[1])
        self.ln_bwd(a1, dxm1, dx, accumulate=True, wname=n + ".norm1", dscale=dmp + 4 * d, dshift=dmp, ldg=6 * d)
        self._wgroup = None
        # ---------------- adaLN linear: mod = W gelu(c) + b
        if not self._x_only:
            self._adaln_bwd(n + ".adaLN_modulation.1", dmod, B, 6 * d, gc, dgc_f32, group)

    def _adaln_bwd(self, wname, dmod_f32, B, N, gc, dgc_f32, group=None):
        """Backward of mod = W gelu(c) + b for one layer.  The weight / bias gradients are taken at once; the gradient w.r.t.
        the condition vector, dgc += dmod @ W (a [B, N] x [N, D] product per layer, too small to fill the chip: 62 launches of
        ~60 us per microbatch of 256 at ~50 TFLOP/s, profiles/r2_kernel_stats_bench_mb256.txt), is deferred when `group` is
        given: the bf16 dmod goes to the group's slot and ALL layers of the group are contracted by one launch over operand
        lists at the end of the backward (_adaln_dgrad_grouped)."""
        D = self.cfg.dim
        dmod = self.empty(B, N) if group is None else group.buf[len(group.w)]
        self._launch("md_cast_f32_bf16", dmod_f32.data_ptr(), dmod.data_ptr(), B * N, None)
        self.lin_wgrad(dmod, gc, wname, B, N, D, bias_from=dmod_f32)
        if group is not None:
            group.w.append(self.S[wname + ".weight"].data_ptr())
            return
        self._acc_each(dgc_f32.data_ptr(), B, D, N, [(dmod.data_ptr(), self.S[wname + ".weight"].data_ptr())], lda=N, ldb=D, a_kcontig=1)

    def _dycond_grouped(self, group, Mc, d, K, out_f32):
        """out[Mc, d] += sum_l dkv_l[Mc, K] @ Wkv_l[K, d] over the G blocks of a group: ONE pp256 launch whose items walk the
        operand lists segment by segment (md_gemm_args.list_segments) and keep the sum in their accumulators; split over
        `ks` groups of segments only as far as whole rounds of the 256 CUs need it (a handful of fp32 slices instead of
        2 x 28)."""
        G = len(group.w)
        if G == 0:
            return
        base = group.buf.data_ptr()
        plan = splitk.plan_dycond(G, Mc, d, K, self.ws.numel())
        if plan is None:
            return self._acc_each(out_f32.data_ptr(), Mc, d, K, [(group.buf[i].data_ptr(), w) for i, w in enumerate(group.w)],
                                  lda=K, ldb=d, a_kcontig=1)
        ks, segments = plan
        self._gemm_lists([base + 2 * i * Mc * K for i in range(G)], group.w, out_f32.data_ptr(), Mc, d, K * G, K, ks, list_segments=segments)

    def _gemm_lists(self, a_ptrs, b_ptrs, out_ptr, M, N, K, lda, ks, **kw):
        """out[M, N] += A B, the contraction walking the operand lists (md_gemm_args.A_list / B_list): ks fp32 slices, then their reduction."""
        al, bl = self._ptr_list(a_ptrs), self._ptr_list(b_ptrs)
        self._gemm(A=a_ptrs[0], B=b_ptrs[0], A_list=al.data_ptr(), B_list=bl.data_ptr(), C=self.ws.data_ptr(), M=M, N=N, K=K, lda=lda, ldb=N,
                   ldc=N, sC=ks * M * N, sSplit=M * N, batch=1, ksplit=ks, a_kcontig=1, b_kcontig=0, mode=hip.EPI_STORE_F32, act=0, alpha=1.0, **kw)
        self._launch("md_splitk_reduce", self.ws.data_ptr(), out_ptr, M, N, N, 0, ks, 1, 1)

    def _ptr_list(self, ptrs):
        """Device array of device pointers (md_gemm_args.A_list / B_list); cached by value: with the fixed-address arenas the
        same lists recur every microbatch, so the step path uploads nothing."""
        key = tuple(ptrs)
        t = self._ptr_cache.get(key)
        if t is None:
            if len(self._ptr_cache) > 256:
                self._ptr_cache.clear()
            t = torch.tensor(list(key), dtype=torch.int64).to(self.dev)
            self._ptr_cache[key] = t
        return t

    def _adaln_dgrad_grouped(self, group, B, N, dgc_f32):
        """dgc[B, D] += sum_l dmod_l[B, N] @ W_l[N, D] over the G layers of a group as ONE pp256 launch: every (layer, k-part)
        is an item with its own operand pair (md_gemm_args.A_list / B_list) writing an fp32 slice, then one md_splitk_reduce."""
        D, G = self.cfg.dim, len(group.w)
        if G == 0:
            return
        base = group.buf.data_ptr()
        plan = splitk.plan_adaln_dgrad(G, B, N, D, self.ws.numel())
        if plan is None:                                       # does not fit the workspace / the kernel: layer by layer
            return self._acc_each(dgc_f32.data_ptr(), B, D, N, [(group.buf[i].data_ptr(), w) for i, w in enumerate(group.w)],
                                  lda=N, ldb=D, a_kcontig=1)
        parts, kspan, ks = plan
        self._gemm_lists([base + 2 * (i * B * N + c * kspan) for i in range(G) for c in range(parts)],
                         [w + 2 * (c * kspan * D) for w in group.w for c in range(parts)], dgc_f32.data_ptr(), B, D, kspan * ks, N, ks)

    # ------------------------------------------------------------------------------------------ small MLPs (Mlp with norm)
    def _mlp_norm_hidden(self, pre, xin, rows, cin, rps):
        """The first half of _mlp_norm_fwd: tape with hn = gelu(LN(fc1(x))), the input of fc2."""
        D = self.cfg.dim
        t = Tape()
        t.xin = xin
        t.h = self.empty(rows, D)
        self.lin_fwd(xin, pre + ".fc1", t.h, rows, D, cin)
        t.hn = self.empty(rows, D)
        t.st = self.empty(2, rows, dtype=F32)
        self.ln_fwd(self.ln_args(t.h, pre + ".norm", t.hn, rows, D, mean=t.st[0], rstd=t.st[1], act=hip.ACT_GELU_TANH, rps=rps))
        return t

    def _mlp_norm_out(self, pre, hn, rows, res=None):
        """The second half: fc2(hn), optional residual add in the epilogue."""
        D = self.cfg.dim
        out = self.empty(rows, D)
        self.lin_fwd(hn, pre + ".fc2", out, rows, D, D, mode=hip.EPI_STORE_BF16 if res is None else hip.EPI_RESIDUAL, res=res)
        return out

    def _mlp_norm_fwd(self, pre, xin, rows, cin, rps, res=None):
        """fc2(LN(gelu(fc1(x)))) (utils.py:63-68); optional residual add on the output.  Returns (out, tape)."""
        t = self._mlp_norm_hidden(pre, xin, rows, cin, rps)
        return self._mlp_norm_out(pre, t.hn, rows, res), t

    def _mlp_norm_bwd(self, pre, t, dout, rows, cin, rps, need_dx):
        D = self.cfg.dim
        self.lin_wgrad(dout, t.hn, pre + ".fc2", rows, D, D)
        dhn = self.empty(rows, D)
        self.lin_dgrad(dout, pre + ".fc2", dhn, rows, D, D)
        dh = self.empty(rows, D)
        a = self.ln_args(t.h, pre + ".norm", None, rows, D, mean=t.st[0], rstd=t.st[1], act=hip.ACT_GELU_TANH, rps=rps)
        self.ln_bwd(a, dhn, dh, accumulate=False, wname=pre + ".norm")
        self.lin_wgrad(dh, t.xin, pre + ".fc1", rows, D, cin)
        if not need_dx:
            return None
        dx = self.empty(rows, cin)
        self.lin_dgrad(dh, pre + ".fc1", dx, rows, D, cin)
        return dx

    # ------------------------------------------------------------------------------------------ whole model
    def forward(self, x_img: Optional[torch.Tensor], t_in: torch.Tensor, y: Optional[torch.Tensor] = None, *, mask_ratio: float = 0.0,
                mask_noise: Optional[torch.Tensor] = None, in_scale: Optional[torch.Tensor] = None,
                y_rowscale: Optional[torch.Tensor] = None, record_tape: bool = False, arena: bool = False,
                cond: Optional[Conditioning] = None, patches: Optional[torch.Tensor] = None, input_tape: bool = False,
                step_cache: Optional[ResidualCache] = None, reuse=False) -> Tape:
        """x_img f32 [B,C,H,W] (multiplied by in_scale[b] if given), t_in f32 [B], y f16|f32 [B,(1,)L,Dc]
        (rows multiplied by y_rowscale[b] if given).  Returns the tape; tape.out_tok is the network output for the
        kept tokens, bf16 [B*Tk, p*p*C].
        record_tape: a backward() will follow — keep every block's activations (inference passes drop them as they go).
        arena: additionally place the tape in the fixed-address arena (needs `use_arena`; the caller promises forward ->
        backward strictly in turn).  Both are explicit arguments: torch disables grad mode inside autograd.Function.forward,
        so probing torch.is_grad_enabled() here would never see a training pass.
        cond: the result of encode_condition() for these captions -- the caption stream and every block's kv_linear / K-LayerNorm
        are skipped and the cached buffers used instead (y is not read and may be None).
        patches: bf16 [B*T, patch_vec] patch rows as md_patchify writes them -- used in place of patchifying x_img (which may be
        None: the latent grid is then the model's input_size).  cond and patches are inference-only.
        input_tape (with cond and / or patches): keep what a backward to the network input alone needs -- every block's
        activations and references to the cached K / V the blocks read; the conditioning is frozen.  backward() on such a tape takes
        input_grads=("x",), param_grads=False and nothing else.
        step_cache (a ResidualCache; inference-only, with or without cond / patches): with reuse false the pass is the
        one without the argument plus one md_residual_delta launch behind backbone block hi - 1, which leaves what blocks [lo, hi) added
        to the residual stream in the cache.  With reuse true those blocks are not launched (nor announced to before_segment): their
        input plus the cached delta (md_add_bf16) stands in for their output; the cache must be valid for this batch, token count and
        weight version.  reuse may be a callable: it is called once, between the mixer and the backbone, with the device scalar
        step_cache.probe() measured on the backbone's input (None without probe=True, or when the probe only filled its reference),
        and returns the decision.  The probe runs in every evaluation of a cache built with probe=True, before that point."""
        cfg = self.cfg
        if step_cache is not None:
            if record_tape or arena or input_tape or mask_ratio > 0:
                raise RuntimeError("step_cache is inference-only: it cannot be combined with record_tape, arena, input_tape or mask_ratio > 0")
            if not self.backbone:
                raise ValueError("step_cache: the model has no backbone blocks to cache")
            step_cache.resolve(len(self.backbone))
            step_cache.poison = self.poison
        elif reuse is not False:
            raise ValueError("reuse needs a step_cache")
        if cond is not None or patches is not None:
            if record_tape or arena or mask_ratio > 0:
                raise RuntimeError("cond / patches are inference-only: they cannot be combined with record_tape, arena or mask_ratio > 0")
        elif input_tape:
            raise ValueError("input_tape records a pass that reads cond= and / or patches=; without them use record_tape")
        if patches is not None:
            assert patches.dtype == BF16 and patches.is_contiguous() and patches.dim() == 2 and patches.shape[1] == cfg.patch_vec
            B, rem = divmod(patches.shape[0], cfg.tokens)
            assert rem == 0 and B > 0, "patches must hold whole samples of the model's token grid"
            H, W = (x_img.shape[-2], x_img.shape[-1]) if x_img is not None else (cfg.input_size, cfg.input_size)
        else:
            assert x_img.dtype == F32 and x_img.is_contiguous()
            B, H, W = x_img.shape[0], x_img.shape[-2], x_img.shape[-1]
        assert (H // cfg.patch_size) * (W // cfg.patch_size) == cfg.tokens, "input resolution does not match the model's position table"
        if step_cache is not None and reuse is True:            # (a callable decides later: _forward checks what it returns)
            self._check_reuse(step_cache, B, cfg.tokens)
        if cond is not None:
            if cond.B != B:
                raise RuntimeError(f"conditioning mismatch: encoded for batch {cond.B}, the input has batch {B}")
            if y is not None and y.shape[-2] != cond.Lc:
                raise RuntimeError(f"conditioning mismatch: encoded for caption length {cond.Lc}, y has {y.shape[-2]}")
            if cond.version != self.weights_version:
                raise RuntimeError(f"conditioning mismatch: encoded with weight version {cond.version}, the weights are now at "
                                   f"{self.weights_version} (encode_condition again after the weights change)")
            if cond.head_major != self.qk_head_major:
                raise RuntimeError("conditioning mismatch: encoded with another q / k layout (qk_head_major)")
            Lc, Dc, ydt = cond.Lc, 0, ""
        else:
            assert y.is_contiguous() and y.dtype in (torch.float16, F32)
            Lc, Dc, ydt = y.shape[-2], y.shape[-1], str(y.dtype)
        if self.caption_bias is not None:
            self._check_caption_bias(B, Lc, record_tape or arena or input_tape)
        if self.mx is not None:
            if record_tape or arena or input_tape:
                raise RuntimeError("mx (MXFP8 linears) is inference-only: nothing of it has a backward, so record_tape, arena and "
                                   "input_tape cannot be combined with it (DESIGN.md 4.23)")
            self.mx.check_fresh(self.weights_version)
        self._poison_ws()
        grad_pass = self.use_arena and arena and record_tape
        self._record = record_tape or input_tape or self.keep_last_tape
        dsp = self.disperse
        self._disperse_on = bool(record_tape and dsp is not None and dsp[1] > 0)
        if self._disperse_on and not 0 <= dsp[0] < len(self.backbone):
            raise ValueError(f"disperse: block {dsp[0]} is outside the backbone's {len(self.backbone)} blocks")
        if grad_pass:
            # an armed pass allocates the Gram, W' and the result block behind block k: part of the shape key
            self._tape_arena.begin((B, H, W, Lc, Dc, float(mask_ratio), ydt, bool(self.prune_masked_experts))
                                   + ((("disperse", int(dsp[0])),) if self._disperse_on else ()))
            self._arena = self._tape_arena
        ok = False
        try:
            tp = self._forward(x_img, t_in, y, mask_ratio, mask_noise, in_scale, y_rowscale, cond, patches, B, H, W, Lc, step_cache, reuse)
            tp.input_tape = bool(input_tape)
            ok = True
            return tp
        finally:
            if grad_pass:
                self._tape_arena.end(ok)
            self._arena = None

    def _check_reuse(self, sc: ResidualCache, B: int, T: int) -> None:
        if not sc.valid(B, T, self.weights_version):
            if sc.version is None:
                raise RuntimeError("step cache mismatch: reuse=True on an empty cache (run a full evaluation with step_cache= first)")
            raise RuntimeError(f"step cache mismatch: filled at batch {sc.B}, {sc.T} tokens, weight version {sc.version}; this evaluation "
                               f"has batch {B}, {T} tokens, weight version {self.weights_version}")

    def _caption_fwd(self, y, y_rowscale, B, Lc, tp) -> torch.Tensor:
        """Caption projection + caption block (dit.py:482-483) and the token mean the pooled MLP reads: everything that depends on
        the captions alone up to there.  Activations go to tp (ycap, yproj, y0, cb, y2, ymean); returns y2 [B*Lc, D]."""
        cfg = self.cfg
        D, Dc = cfg.dim, y.shape[-1]
        Mc = B * Lc
        tp.y_dtype, tp.y_rowscale = y.dtype, y_rowscale
        tp.ycap = self.empty(Mc, Dc)
        self._launch("md_cast_rows_bf16", y.data_ptr(), 0 if y.dtype == torch.float16 else 1, tp.ycap.data_ptr(), Mc, Dc, _p(y_rowscale), Lc)
        y0, tp.yproj = self._mlp_norm_fwd("y_embedder.y_proj", tp.ycap, Mc, Dc, Lc)
        tp.y0 = y0
        cb = Tape()
        cb.xn1 = self.empty(Mc, D)
        cb.st1 = self.empty(2, Mc, dtype=F32)
        self.ln_fwd(self.ln_args(y0, "y_emb_preprocess.norm1", cb.xn1, Mc, D, mean=cb.st1[0], rstd=cb.st1[1], rps=Lc))
        cb.sa = Tape()
        heads_c = D // cfg.head_dim
        o = self._self_attn_fwd("y_emb_preprocess.attn", cb.xn1, B, Lc, D, D, heads_c, cb.sa)
        y1 = self.empty(Mc, D)
        self.lin_fwd(o, "y_emb_preprocess.attn.proj", y1, Mc, D, D, mode=hip.EPI_RESIDUAL, res=y0)
        cb.y1 = y1
        cb.xn2 = self.empty(Mc, D)
        cb.st2 = self.empty(2, Mc, dtype=F32)
        self.ln_fwd(self.ln_args(y1, "y_emb_preprocess.norm2", cb.xn2, Mc, D, mean=cb.st2[0], rstd=cb.st2[1], rps=Lc))
        y2 = self._swiglu_ffn_fwd("y_emb_preprocess.mlp", cb.xn2, Mc, D, caption_ffn_hidden(cfg), cb, res=y1)
        tp.cb, tp.y2 = cb, y2
        tp.ymean = self.empty(B, D)
        self._launch("md_mean_tokens", y2.data_ptr(), tp.ymean.data_ptr(), B, Lc, D)
        return y2

    def _map_y_fwd(self, y2, Mc, tp) -> torch.Tensor:
        """Caption tokens in the patch mixer's width (patch_mixer_map_y, dit.py:489-493; only with has_maps)."""
        D, Dm = self.cfg.dim, self.cfg.patch_mixer_dim
        tp.y_ln = self.empty(Mc, D)
        tp.st_y = self.empty(2, Mc, dtype=F32)
        self.ln_fwd(self.ln_args(y2, "patch_mixer_map_y.0", tp.y_ln, Mc, D, mean=tp.st_y[0], rstd=tp.st_y[1], rps=tp.Lc))
        ym = self.empty(Mc, Dm)
        self.lin_fwd(tp.y_ln, "patch_mixer_map_y.1", ym, Mc, Dm, D)
        return ym

    def encode_condition(self, y: torch.Tensor) -> Conditioning:
        """The caption-only part of the forward pass, once (inference: nothing is kept for a backward): caption stream, pooled
        hidden, patch_mixer_map_y and, for every block, kv_linear + the QK-LayerNorm of K -- the same launches on the same operands
        as in _forward / _block_fwd, so a pass with `cond=` gives the bits of a pass without.  y as in forward()."""
        cfg = self.cfg
        assert y.is_contiguous() and y.dtype in (torch.float16, F32)
        Lc = y.shape[-2]
        B = y.numel() // (Lc * y.shape[-1])
        Mc, D = B * Lc, cfg.dim
        seg = self.before_segment if self.before_segment is not None else (lambda key: None)
        seg("rest")
        tp = Tape()
        tp.Lc = Lc
        y2 = self._caption_fwd(y, None, B, Lc, tp)
        pooled = self._mlp_norm_hidden("pooled_y_emb_process", tp.ymean, B, D, 1).hn
        ym = self._map_y_fwd(y2, Mc, tp) if (cfg.use_patch_mixer and cfg.has_maps) else y2
        kv = {}
        for blocks, ycond in ((self.mixer, ym), (self.backbone, y2)):
            for bp in blocks:
                seg(bp.name)
                k = self._kv_linear_fwd(bp.name, ycond, Mc, bp.xattn_hidden, bp.dim)
                kv[bp.name] = (k, self._k_norm_fwd(k, Mc, bp.xattn_hidden, Lc)[1])
        return Conditioning(B, Lc, self.qk_head_major, self.weights_version, pooled, kv)

    def _forward(self, x_img, t_in, y, mask_ratio, mask_noise, in_scale, y_rowscale, cond, patches, B, H, W, Lc, sc=None, reuse=False) -> Tape:
        cfg = self.cfg
        C, p = cfg.in_channels, cfg.patch_size
        T, D, Dm = (H // p) * (W // p), cfg.dim, cfg.patch_mixer_dim
        seg = self.before_segment if self.before_segment is not None else (lambda key: None)
        seg("rest")
        tp = Tape()
        tp.arena = self._arena is not None
        tp.B, tp.T, tp.Lc, tp.H, tp.W = B, T, Lc, H, W
        # ---- patch embedding (+ pos), dit.py:479
        tp.in_scale, tp.from_patches = in_scale, patches is not None      # (the image gradient multiplies by the same per-sample factor)
        if patches is None:
            tp.patches = self.empty(B * T, cfg.patch_vec)
            self._launch("md_patchify", x_img.data_ptr(), _p(in_scale), tp.patches.data_ptr(), B, C, H, W, p)
        else:
            tp.patches = patches
        tok = self.empty(B * T, D)
        self._gemm(A=tp.patches.data_ptr(), B=self.S["x_embedder.proj.weight"].data_ptr(), C=tok.data_ptr(),
                   bias=self.P["x_embedder.proj.bias"].data_ptr(), M=B * T, N=D, K=cfg.patch_vec, lda=cfg.patch_vec,
                   ldb=cfg.patch_vec, ldc=D, batch=1, ksplit=1, a_kcontig=1, b_kcontig=1, mode=hip.EPI_STORE_BF16, act=0, alpha=1.0)
        tp.tok = tok
        # ---- timestep embedding, dit.py:480
        tp.tfreq = self.empty(B, 512)
        t_f = t_in if (t_in.dtype == F32 and t_in.numel() == B and t_in.is_contiguous()) else t_in.to(F32).expand(B).contiguous()
        self._launch("md_timestep_embed", t_f.data_ptr(), tp.tfreq.data_ptr(), B, 512)
        tp.t_f = t_f
        tp.t_pre = self.empty(B, D)
        tp.t_h = self.empty(B, D)
        self.lin_fwd(tp.tfreq, "t_embedder.mlp.0", tp.t_h, B, D, 512, act=hip.ACT_GELU_TANH, C2=tp.t_pre)
        temb = self.empty(B, D)
        self.lin_fwd(tp.t_h, "t_embedder.mlp.2", temb, B, D, D)
        # ---- caption projection + caption block, dit.py:482-483; pooled caption -> condition vector c = t_emb + Mlp(mean(y)),
        # dit.py:484-485.  With `cond` everything up to the input of the pooled MLP's fc2 comes from the cache.
        Mc = B * Lc
        if cond is None:
            y2 = self._caption_fwd(y, y_rowscale, B, Lc, tp)
            tp.pool = self._mlp_norm_hidden("pooled_y_emb_process", tp.ymean, B, D, 1)
            pooled = tp.pool.hn
        else:
            y2, pooled = None, cond.pooled
            tp.y2 = None                            # (an input_tape's backward passes it on as the caption tokens nobody reads)
        c = self._mlp_norm_out("pooled_y_emb_process", pooled, B, res=temb)
        tp.c = c
        gc = self.empty(B, D)
        self._launch("md_act_fwd", c.data_ptr(), gc.data_ptr(), B * D, hip.ACT_GELU_TANH)
        tp.gc = gc
        # ---- patch mixer, dit.py:489-493
        pos = self.buf["pos_embed"]
        if cfg.use_patch_mixer and cfg.has_maps:
            tp.xin_ln = self.empty(B * T, D)
            tp.st_xin = self.empty(2, B * T, dtype=F32)
            self.ln_fwd(self.ln_args(tok, "patch_mixer_map_xin.0", tp.xin_ln, B * T, D, mean=tp.st_xin[0], rstd=tp.st_xin[1],
                                     pos=pos, pos_rows=T, rps=T))
            x = self.empty(B * T, Dm)
            self.lin_fwd(tp.xin_ln, "patch_mixer_map_xin.1", x, B * T, Dm, D)
            ym = self._map_y_fwd(y2, Mc, tp) if cond is None else None
        else:
            # Identity maps (patch_mixer_dim == dim, dit.py:389-392): x = tok + pos
            x = self.empty(B * T, D)
            if self._posb is None or self._posb.shape[0] != B:          # constant table: built once per batch size
                self._posb = pos.to(BF16).expand(B, T, D).contiguous()
            posb = self._posb
            self._launch("md_add_bf16", tok.data_ptr(), posb.data_ptr(), x.data_ptr(), B * T * D)
            ym = y2
        tp.ym = ym
        # ---- the modulation vectors of every block (mixer + backbone) from one GEMM on gelu(c), dit.py:222-225
        seg("adaln.m")
        seg("adaln.b")
        mod_all = self._adaln_all(gc, B) if (self.batch_adaln and self._adaln is not None) else None
        tp.mixer = []
        Tk = int(T * (1 - mask_ratio)) if mask_ratio > 0 else T

        def get_mask():
            assert mask_noise is not None and mask_noise.dtype == F32 and mask_noise.shape == (B, T)
            tp.keep_rows = self.empty(B * Tk, dtype=I32)
            tp.ids_restore = self.empty(B, T, dtype=I32)
            tp.mask = self.empty(B, T, dtype=F32)
            self._launch("md_get_mask", mask_noise.contiguous().data_ptr(), B, T, Tk, tp.keep_rows.data_ptr(), tp.ids_restore.data_ptr(),
                         tp.mask.data_ptr())

        # masked-expert pruning: the mask depends on the noise alone, so it is drawn before the last mixer block instead of behind it
        prune = mask_ratio > 0 and self.prune_masked_experts and bool(self.mixer) and self.mixer[-1].moe
        for bp in self.mixer:
            seg(bp.name)
            keep = None
            if prune and bp is self.mixer[-1]:
                get_mask()
                keep = (tp.ids_restore, Tk)
            x, bt = self._block_fwd(bp, x, ym, B, T, Lc, gc, mod_all, kv=cond.kv[bp.name] if cond is not None else None, keep=keep)
            if self._record:
                tp.mixer.append(bt)
        # ---- masking, dit.py:495-504
        Wd = x.shape[1]
        if mask_ratio > 0:
            if not prune:
                get_mask()
            xk = self.empty(B * Tk, Wd)
            self._launch("md_gather_rows", x.data_ptr(), Wd, tp.keep_rows.data_ptr(), xk.data_ptr(), Wd, B * Tk, Wd)
            x = xk
        else:
            tp.keep_rows = tp.ids_restore = tp.mask = None
        tp.Tk = Tk
        # ---- mixer -> backbone projection (after masking), dit.py:506-508
        if cfg.use_patch_mixer and cfg.has_maps:
            tp.xout_in = x
            tp.xout_ln = self.empty(B * Tk, Dm)
            tp.st_xout = self.empty(2, B * Tk, dtype=F32)
            self.ln_fwd(self.ln_args(x, "patch_mixer_map_xout.0", tp.xout_ln, B * Tk, Dm, mean=tp.st_xout[0],
                                     rstd=tp.st_xout[1], rps=Tk))
            xb = self.empty(B * Tk, D)
            self.lin_fwd(tp.xout_ln, "patch_mixer_map_xout.1", xb, B * Tk, D, Dm)
            x = xb
        tp.blocks = []
        tp.disperse = None
        # ---- step cache: the probe on the backbone's input, then the decision; Tk == T (mask_ratio > 0 is refused)
        lo = hi = -1
        if sc is not None:
            lo, hi = sc.lo, sc.hi
            rel_max = sc.probe(x, B, self.weights_version) if sc.with_probe else None
            if callable(reuse):
                reuse = bool(reuse(rel_max))
                if reuse:
                    self._check_reuse(sc, B, T)
        tp.reused = bool(sc is not None and reuse)
        x_lo = None
        for i, bp in enumerate(self.backbone):
            if lo <= i < hi and reuse:
                if i == lo:                         # blocks [lo, hi) are not launched: their input plus what they added last time
                    xr = self.empty(B * Tk, D)
                    self._launch("md_add_bf16", x.data_ptr(), sc.delta.data_ptr(), xr.data_ptr(), B * Tk * D)
                    x = xr
                continue
            if i == lo:
                x_lo = x
            seg(bp.name)
            x, bt = self._block_fwd(bp, x, y2, B, Tk, Lc, gc, mod_all, kv=cond.kv[bp.name] if cond is not None else None,
                                    out_rows=tp.keep_rows)
            if self._record:
                tp.blocks.append(bt)
            if self._disperse_on and i == self.disperse[0] and B > 1:       # B = 1: L = 0 and the gradient is 0 -- nothing to launch
                tp.disperse = self._disperse_fwd(x, B, Tk * D)
            if i == hi - 1:
                sc.store(x, x_lo, B, T, self.weights_version)
        # ---- final layer, dit.py:513
        seg("final_layer")
        tp.xlast = x
        tp.fmod = self.empty(B, 2 * D)
        self.lin_fwd(gc, "final_layer.adaLN_modulation.1", tp.fmod, B, 2 * D, D)
        fm = tp.fmod.data_ptr()
        tp.xf = self.empty(B * Tk, D)
        tp.st_f = self.empty(2, B * Tk, dtype=F32)
        self.ln_fwd(self.ln_args(x, "final_layer.norm_final", tp.xf, B * Tk, D, shift=fm, scale=fm + 2 * D, ldmod=2 * D, rps=Tk,
                                 mean=tp.st_f[0], rstd=tp.st_f[1]))
        pv = cfg.patch_vec
        tp.out_tok = self.empty(B * Tk, pv)
        self.lin_fwd(tp.xf, "final_layer.linear", tp.out_tok, B * Tk, pv, D)
        if self.keep_last_tape:
            self.last_tape = tp
        return tp

    # ------------------------------------------------------------------------------------------ dispersive loss
    def disperse_gram(self, z, B, K, G, ldg):
        """G [B, ldg] fp32 = Z Z^T for Z [B, K] bf16 (rows K apart).  B a multiple of 8: the GEMM family with its deterministic split-K
        (workspace slices + md_splitk_reduce need whole 16-byte column chunks of an N = B wide slice).  Otherwise md_disperse_gram_small:
        the family would only take such a B by reading rows of Z past the batch."""
        if B % 8 == 0:
            self.gemm_f32_acc(out_ptr=G.data_ptr(), M=B, N=B, K=K, ldo=ldg, accumulate=False, A=z.data_ptr(), B=z.data_ptr(), lda=K, ldb=K,
                              a_kcontig=1, b_kcontig=1)
            path = "gemm"
        else:
            self._launch("md_disperse_gram_small", z.data_ptr(), K, B, K, G.data_ptr(), ldg)
            path = "small"
        if self.disperse_log is not None:
            self.disperse_log.append(("gram", path, B, K))

    def disperse_apply(self, W, ldw, z, dx, B, K):
        """dx [B, K] += W' [B, ldw] Z [B, K]: a data-gradient-shaped launch (contraction over the batch, Z the K-strided operand) with the
        residual epilogue reading and writing dx.  res == C is safe in every kernel of the family: an output element is read (as the
        residual) and written by the one workgroup that owns its tile, the write depends on the read, and no other launch or workgroup
        touches it.  The family takes every B: a contraction that ends inside a k-tile is zero-filled per row (K-strided operand: rows
        >= B are never read) and per 16-byte chunk (W': the pad columns md_disperse_pairs writes as zero)."""
        self._gemm(A=W.data_ptr(), B=z.data_ptr(), C=dx.data_ptr(), res=dx.data_ptr(), M=B, N=K, K=B, lda=ldw, ldb=K, ldc=K, ldr=K,
                   batch=1, ksplit=1, a_kcontig=1, b_kcontig=0, mode=hip.EPI_RESIDUAL, act=0, alpha=1.0)
        if self.disperse_log is not None:
            self.disperse_log.append(("apply", "gemm", B, K))

    def disperse_pairs(self, G, ldg, B, K, tau, coef, W, ldw, result, loss_accum=None, dist_accum=None, accum_weight=0.0):
        ws = self.empty(2 * B, dtype=torch.float64)
        self._launch("md_disperse_pairs", G.data_ptr(), ldg, B, K, tau, coef, W.data_ptr(), ldw, result.data_ptr(), ws.data_ptr(), 2 * B,
                     _p(loss_accum), _p(dist_accum), accum_weight)

    def _disperse_fwd(self, x, B, K):
        """Behind backbone block k: Gram of its output x [B * Tk, D] seen as Z [B, K], then md_disperse_pairs.  Z is not copied: x is the
        next block's saved input (or tp.xlast) in the forward arena.  Returns what the backward needs."""
        k, lam, tau = self.disperse
        gscale, loss_accum, dist_accum, aw = self.disperse_train
        if B > hip.DISPERSE_MAX_B:
            raise ValueError(f"disperse: microbatch {B} exceeds {hip.DISPERSE_MAX_B} samples")
        ld = (B + 7) // 8 * 8
        d = Tape()
        d.k, d.z, d.B, d.K, d.ldw, d.tau = k, x, B, K, ld, tau
        G = self.empty(B, ld, dtype=F32)
        d.W = self.empty(B, ld)
        if self._disperse_result is None:
            self._disperse_result = torch.zeros(4, device=self.dev, dtype=torch.float64)
        d.result = self._disperse_result
        self.disperse_gram(x, B, K, G, ld)
        self.disperse_pairs(G, ld, B, K, tau, 4.0 * lam * gscale / (tau * K), d.W, ld, d.result, loss_accum, dist_accum, aw)
        return d

    def sample_image(self, tp: Tape) -> torch.Tensor:
        """unmask_tokens + unpatchify (utils.py:417-426, dit.py:566-575) -> f32 [B, C, H, W]."""
        cfg = self.cfg
        img = self.empty(tp.B, cfg.in_channels, tp.H, tp.W, dtype=F32)
        mt = self.buf["mask_token"]
        self._launch("md_unpatchify", tp.out_tok.data_ptr(), _p(tp.ids_restore), tp.Tk, mt.data_ptr(), img.data_ptr(), tp.B, cfg.in_channels, tp.H,
                     tp.W, cfg.patch_size)
        return img

    def backward(self, tp: Tape, dtok: torch.Tensor, on_segment=None, *, input_grads=(), param_grads=True) -> InputGrads:
        """dtok: bf16 [B*Tk, p*p*C] grad of the network output for the kept tokens.  Accumulates every parameter
        gradient into the fp32 grad buffers (self.G).  `on_segment(prefix)` is called as soon as every kernel that
        writes the gradients of the parameters under `prefix` has been enqueued (data-parallel bucket hand-off).
        input_grads: subset of {"x", "t", "y"} -- the returned InputGrads holds the gradients of those network inputs (DESIGN.md
        4.17); they are fresh tensors of the torch allocator, never arena memory.  Empty: the launches of a backward without them.
        param_grads=False: the dgrad-only backward -- nothing under self.G is written or zeroed and no weight-gradient, bias or
        LayerNorm-weight reduction is launched; every data-gradient launch is the one of a full backward.
        param_grads="lora": param_grads=False, plus one md_lora_wgrad per linear the attached factored adapter targets, into the
        adapter's own gradient buffer; raises without an attached, active adapter built with backward="factored".
        input_grads=("x",) with param_grads=False stops at the image: it returns right after md_patch_embed_dgrad and
        launches nothing dx does not depend on; dx has the bits of the full dgrad-only backward.  It is the only backward of an
        input_tape (forward(..., input_tape=True)), whose conditioning is frozen; a tape of a forward that read patches= gives the
        gradient with respect to the un-patchified network input."""
        want = frozenset(input_grads)
        if not want <= {"x", "t", "y"}:
            raise ValueError(f"input_grads must be a subset of {{'x', 't', 'y'}}, got {sorted(want)}")
        lora_grads = isinstance(param_grads, str)
        if lora_grads:
            if param_grads != "lora":
                raise ValueError(f"param_grads must be True, False or 'lora', got {param_grads!r}")
            if self.lora is None or not self.lora.factored:
                raise RuntimeError("backward(param_grads='lora') needs an attached, active adapter built with LoRA(backward='factored')")
            param_grads = False
        x_only = want == {"x"} and not param_grads and not lora_grads
        if getattr(tp, "input_tape", False) and not x_only:
            raise RuntimeError("an input_tape holds a frozen conditioning: its backward takes input_grads=('x',) and param_grads=False, "
                               f"got input_grads={sorted(want)}, param_grads={bool(param_grads)}")
        self._poison_ws()
        use = self.use_arena and getattr(tp, "arena", False)
        if use:
            self._scratch_arena.begin((tp.B, tp.T, tp.Tk, tp.Lc, tp.H, tp.W))
            self._arena = self._scratch_arena
        ok = False
        self._param_grads, self._x_only, self._lora_grads = bool(param_grads), x_only, lora_grads
        try:
            out = self._backward(tp, dtok, on_segment, want)
            ok = True
            return out
        finally:
            self._param_grads, self._x_only, self._lora_grads = True, False, False
            if use:
                self._scratch_arena.end(ok)
            self._arena = None

    def _block_bwd_scoped(self, *a):
        """One block's backward; its temporaries are released when it returns (bump-arena mark / release)."""
        if self._arena is None:
            return self._block_bwd(*a)
        m = self._arena.mark()
        self._block_bwd(*a)
        self._arena.release(m)

    def _backward(self, tp: Tape, dtok: torch.Tensor, on_segment=None, want=frozenset()) -> InputGrads:
        cfg = self.cfg
        out = InputGrads()
        seg = on_segment if on_segment is not None else (lambda name: None)
        B, T, Tk, Lc = tp.B, tp.T, tp.Tk, tp.Lc
        D, Dm, pv = cfg.dim, cfg.patch_mixer_dim, cfg.patch_vec
        Mc = B * Lc
        gc = tp.gc
        x_only = self._x_only                       # stop at the image: no condition-vector or caption-token gradient is formed
        dgc = None if x_only else self.zeros(B, D)          # fp32: sums the adaLN dgrads of all 6+28+1 layers
        dy2_f32 = None if x_only else self.zeros(Mc, D)     # fp32: caption-token grads from the 28 backbone kv_linears + pooling
        # per stack, None where not grouped: adaln (-> the condition vector, _adaln_dgrad_grouped), kv (-> the caption tokens, _dycond_grouped)
        stacks = [(SimpleNamespace(adaln=None, kv=None), blocks) for blocks in (self.backbone, self.mixer)]
        (sg_b, _), (sg_m, _) = stacks
        for sg, blocks in stacks:                   # bf16 dmod of every layer, kept until the grouped contraction below
            if self.group_adaln and not x_only and blocks:
                sg.adaln = _Deferred(self.empty(len(blocks), B, 6 * blocks[0].dim))
        for sg, blocks in stacks:                   # dkv of every block, kept until the concatenated contraction
            if self.group_dycond and not x_only and blocks:
                sg.kv = _Deferred(self.empty(len(blocks), Mc, 2 * blocks[0].xattn_hidden))
        # ---- final layer
        self.lin_wgrad(dtok, tp.xf, "final_layer.linear", B * Tk, pv, D)
        dxf = self.empty(B * Tk, D)
        self.lin_dgrad(dtok, "final_layer.linear", dxf, B * Tk, pv, D)
        dfm = self.zeros(B, 2 * D)
        fm = tp.fmod.data_ptr()
        dx = self.empty(B * Tk, D)
        af = self.ln_args(tp.xlast, "final_layer.norm_final", None, B * Tk, D, scale=fm + 2 * D, ldmod=2 * D, rps=Tk,
                          mean=tp.st_f[0], rstd=tp.st_f[1])
        self.ln_bwd(af, dxf, dx, accumulate=False, wname="final_layer.norm_final", dscale=dfm.data_ptr() + 4 * D,
                    dshift=dfm.data_ptr(), ldg=2 * D)
        if not x_only:
            self._adaln_bwd("final_layer.adaLN_modulation.1", dfm, B, 2 * D, gc, dgc)
        seg("final_layer")
        # ---- backbone
        dsp = getattr(tp, "disperse", None)
        for i, bp, bt in zip(reversed(range(len(self.backbone))), reversed(self.backbone), reversed(tp.blocks)):
            if dsp is not None and i == dsp.k:
                self.disperse_apply(dsp.W, dsp.ldw, dsp.z, dx, dsp.B, dsp.K)       # dx is dL/d(output of block k) here
            self._block_bwd_scoped(bp, bt, dx, tp.y2, dy2_f32, B, Tk, Lc, gc, dgc, sg_b.adaln, sg_b.kv)
            seg(bp.name)
        if sg_b.kv is not None:
            self._dycond_grouped(sg_b.kv, Mc, self.backbone[0].dim, 2 * self.backbone[0].xattn_hidden, dy2_f32)
        # ---- mixer -> backbone projection
        if cfg.use_patch_mixer and cfg.has_maps:
            self.lin_wgrad(dx, tp.xout_ln, "patch_mixer_map_xout.1", B * Tk, D, Dm)
            dln = self.empty(B * Tk, Dm)
            self.lin_dgrad(dx, "patch_mixer_map_xout.1", dln, B * Tk, D, Dm)
            dxk = self.empty(B * Tk, Dm)
            a = self.ln_args(tp.xout_in, "patch_mixer_map_xout.0", None, B * Tk, Dm, mean=tp.st_xout[0], rstd=tp.st_xout[1], rps=Tk)
            self.ln_bwd(a, dln, dxk, accumulate=False, wname="patch_mixer_map_xout.0")
            dx = dxk
        Wd = dx.shape[1]
        # ---- un-mask: scatter kept-token grads back to all T positions (zeros elsewhere)
        if tp.keep_rows is not None:
            dfull = self.zeros(B * T, Wd, dtype=BF16)
            self._launch("md_scatter_rows", dx.data_ptr(), Wd, tp.keep_rows.data_ptr(), dfull.data_ptr(), Wd, B * Tk, Wd)
            dx = dfull
        # ---- patch mixer
        has_maps = cfg.use_patch_mixer and cfg.has_maps
        dym_f32 = self.zeros(Mc, Dm) if has_maps and not x_only else dy2_f32
        for bp, bt in zip(reversed(self.mixer), reversed(tp.mixer)):
            self._block_bwd_scoped(bp, bt, dx, tp.ym, dym_f32, B, T, Lc, gc, dgc, sg_m.adaln, sg_m.kv)
            seg(bp.name)
        if sg_m.kv is not None:
            self._dycond_grouped(sg_m.kv, Mc, self.mixer[0].dim, 2 * self.mixer[0].xattn_hidden, dym_f32)
        # ---- map_xin / patch embedding
        if has_maps:
            self.lin_wgrad(dx, tp.xin_ln, "patch_mixer_map_xin.1", B * T, Dm, D)
            dln = self.empty(B * T, D)
            self.lin_dgrad(dx, "patch_mixer_map_xin.1", dln, B * T, Dm, D)
            dtok_e = self.empty(B * T, D)
            a = self.ln_args(tp.tok, "patch_mixer_map_xin.0", None, B * T, D, mean=tp.st_xin[0], rstd=tp.st_xin[1],
                             pos=self.buf["pos_embed"], pos_rows=T, rps=T)
            self.ln_bwd(a, dln, dtok_e, accumulate=False, wname="patch_mixer_map_xin.0")
        else:
            dtok_e = dx
        self._param_acc(out_ptr=self.G["x_embedder.proj.weight"].data_ptr(), M=D, N=pv, K=B * T, ldo=pv,
                        A=dtok_e.data_ptr(), B=tp.patches.data_ptr(), lda=D, ldb=pv, a_kcontig=0, b_kcontig=0)
        self._param_colsum(dtok_e.data_ptr(), 0, D, self.G["x_embedder.proj.bias"].data_ptr(), B * T, D)
        if "x" in want:
            # image: the transpose of md_patchify(in_scale) + the x_embedder.proj GEMM in one launch, fp32 straight from the accumulators
            # (a forward that read patches= has no in_scale: dx is then the gradient of the un-patchified network input)
            out.dx = self.fresh(B, cfg.in_channels, tp.H, tp.W)
            path = ctypes.c_int32(-1)
            self._launch("md_patch_embed_dgrad", dtok_e.data_ptr(), D, self.S["x_embedder.proj.weight"].data_ptr(), _p(tp.in_scale),
                         out.dx.data_ptr(), B, cfg.in_channels, tp.H, tp.W, cfg.patch_size, D, byref(path), prof="patch_embed_dgrad",
                         nbytes=2.0 * B * T * D)
            if self.input_grad_log is not None:
                self.input_grad_log.append(("md_patch_embed_dgrad", path.value))
        if x_only:
            return out
        # ---- condition vector: c = temb + pooled ; gc = gelu(c)
        for sg, blocks in stacks:
            if sg.adaln is not None:
                self._adaln_dgrad_grouped(sg.adaln, B, 6 * blocks[0].dim, dgc)
        dc = self.empty(B, D)
        self._launch("md_act_bwd", dgc.data_ptr(), tp.c.data_ptr(), dc.data_ptr(), B * D, hip.ACT_GELU_TANH)
        # timestep embedder
        self.lin_wgrad(dc, tp.t_h, "t_embedder.mlp.2", B, D, D)
        dtpre = self.empty(B, D)
        self.lin_dgrad(dc, "t_embedder.mlp.2", dtpre, B, D, D, mode=hip.EPI_DACT, act=hip.ACT_GELU_TANH, aux=tp.t_pre)
        self.lin_wgrad(dtpre, tp.tfreq, "t_embedder.mlp.0", B, D, 512)
        if "t" in want:
            dtfreq = self.empty(B, 512)
            self.lin_dgrad(dtpre, "t_embedder.mlp.0", dtfreq, B, D, 512)
            out.dt = self.fresh(B)
            self._launch("md_timestep_embed_bwd", tp.t_f.data_ptr(), dtfreq.data_ptr(), out.dt.data_ptr(), B, 512)
            if self.input_grad_log is not None:
                self.input_grad_log.append(("md_timestep_embed_bwd", None))
        # pooled-caption MLP -> mean over tokens
        dymean = self._mlp_norm_bwd("pooled_y_emb_process", tp.pool, dc, B, D, 1, need_dx=True)
        self._launch("md_mean_tokens_bwd", dymean.data_ptr(), dy2_f32.data_ptr(), B, Lc, D)
        # ---- caption tokens: total grad w.r.t. y2
        dy = self.empty(Mc, D)
        self._launch("md_cast_f32_bf16", dy2_f32.data_ptr(), dy.data_ptr(), Mc * D, None)
        if has_maps:
            dym = self.empty(Mc, Dm)
            self._launch("md_cast_f32_bf16", dym_f32.data_ptr(), dym.data_ptr(), Mc * Dm, None)
            self.lin_wgrad(dym, tp.y_ln, "patch_mixer_map_y.1", Mc, Dm, D)
            dyl = self.empty(Mc, D)
            self.lin_dgrad(dym, "patch_mixer_map_y.1", dyl, Mc, Dm, D)
            a = self.ln_args(tp.y2, "patch_mixer_map_y.0", None, Mc, D, mean=tp.st_y[0], rstd=tp.st_y[1], rps=Lc)
            self.ln_bwd(a, dyl, dy, accumulate=True, wname="patch_mixer_map_y.0")
        # ---- caption block (y2 = y1 + ffn(LN2(y1)); y1 = y0 + attn(LN1(y0)))
        cb = tp.cb
        dxn2 = self._swiglu_ffn_bwd("y_emb_preprocess.mlp", cb, dy, cb.xn2, Mc, D, caption_ffn_hidden(cfg), defer=False, try_fused=False)
        a = self.ln_args(cb.y1, "y_emb_preprocess.norm2", None, Mc, D, mean=cb.st2[0], rstd=cb.st2[1], rps=Lc)
        self.ln_bwd(a, dxn2, dy, accumulate=True, wname="y_emb_preprocess.norm2")
        heads_c = D // cfg.head_dim
        self.lin_wgrad(dy, cb.sa.o, "y_emb_preprocess.attn.proj", Mc, D, D)
        do = self.empty(Mc, D)
        self.lin_dgrad(dy, "y_emb_preprocess.attn.proj", do, Mc, D, D)
        dxn1 = self._self_attn_bwd("y_emb_preprocess.attn", cb.xn1, do, B, Lc, D, D, heads_c, cb.sa)
        a = self.ln_args(tp.y0, "y_emb_preprocess.norm1", None, Mc, D, mean=cb.st1[0], rstd=cb.st1[1], rps=Lc)
        self.ln_bwd(a, dxn1, dy, accumulate=True, wname="y_emb_preprocess.norm1")
        # ---- caption projection, then (asked for) the transpose of the caption cast: rows times the forward's y_rowscale
        Dc = tp.ycap.shape[1]
        dycap = self._mlp_norm_bwd("y_embedder.y_proj", tp.yproj, dy, Mc, Dc, Lc, need_dx="y" in want)
        if "y" in want:
            out.dy = self.fresh(Mc, Dc, dtype=tp.y_dtype)
            self._launch("md_cast_rows_from_bf16", dycap.data_ptr(), out.dy.data_ptr(), 0 if tp.y_dtype == torch.float16 else 1, Mc, Dc,
                         _p(tp.y_rowscale), Lc)
            if self.input_grad_log is not None:
                self.input_grad_log.append(("md_cast_rows_from_bf16", None))
        seg("rest")
        return out
