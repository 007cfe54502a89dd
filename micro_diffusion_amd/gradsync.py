"""Overlapped data-parallel gradient exchange (GradSync) for the Trainer: RCCL through torch.distributed or libmicrodit_comm.so, the
rank chunks of the sharded optimiser (shard_plan) and the cap on the CUs RCCL's kernels hold (cap_rccl_channels)."""
from __future__ import annotations

import bisect
import collections
import contextlib
import os
import warnings
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import hip


RCCL_CHANNELS_DEFAULT = 8      # CUs handed to RCCL per rank: 8 channels move the 2 x 2 GB of a step at well over the ~30 GB/s the
#                                overlap needs (xGMI: 7 links x ~50 GB/s per direction); every channel costs the GEMMs 1 / 256


def cap_rccl_channels(n: int = RCCL_CHANNELS_DEFAULT) -> int:
    """Call BEFORE the process group / communicator is created: bounds the CUs RCCL's persistent kernels occupy
    (NCCL_MAX_NCHANNELS; a value the user exported wins).  Returns the cap in force."""
    os.environ.setdefault("NCCL_MAX_NCHANNELS", str(n))
    cap = rccl_channel_cap()          # tolerant parse: a non-numeric exported value counts as "no cap" (0)
    if cap > 0:
        os.environ.setdefault("NCCL_MIN_NCHANNELS", str(min(n, cap)))
    return cap


def rccl_channel_cap() -> int:
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
        path; the process group, rank / world, all_reduce_now (all transports) and the Trainer's CU reservation work as always.
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
        self._range_tensors: Dict[tuple, list] = {}      # (lo, hi) -> _tensors_of
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
            # [small-region partial sums (SUMSQ_PARTIALS floats) | sum over the ranks' chunk norms (1 float)] -> finish_sharded_norm
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
    def all_reduce_now(self, buf) -> None:
        """Sum `buf` over the ranks in place; the compute stream continues behind the result."""
        w = self._all_reduce(buf)
        if w is not None:
            w.wait()

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

    def all_gather_now(self, out, mine) -> None:
        """`out` := the ranks' `mine`, in rank order; the compute stream continues behind the result."""
        w = self._all_gather(out, mine)
        if w is not None:
            w.wait()

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

    @contextlib.contextmanager
    def last_microbatch(self, single_microbatch: bool):
        """Around the step's LAST microbatch: on_segment hands its buckets to the collectives (`active`) and begin_backward may arm
        the engine's bf16 store.  Both are undone on the way out also when the microbatch raises (an OOM, the engine's "two weight
        gradients for one tensor"): a store left armed would swallow the gradients of the next step's earlier microbatches."""
        self.active = True
        try:
            self.begin_backward(single_microbatch)
            yield
        finally:
            self.end_backward()
            self.active = False

    def _tensors_of(self, lo: int, hi: int):
        """(flat offset, numel) of the parameters inside the range, in address order (cached)."""
        c = self._range_tensors
        if (lo, hi) not in c:
            f = self.dit.flat_buffers()
            c[(lo, hi)] = sorted((o, f["P"][n].numel()) for n, o in f["offs"].items() if n in f["P"] and lo <= o < hi)
        return c[(lo, hi)]

    def _exchange(self, lo: int, hi: int) -> None:
        f = self.dit.flat_buffers()
        g = f["g"][lo:hi]
        st = hip.stream_ptr() if g.is_cuda else None
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
        if small:
            work = self._all_reduce(buf)
            self._norm_after(work, buf, True, self.fin.data_ptr())        # identical on every rank: added once, after the scalar all-reduce
        else:
            if sharded:
                chunk, olo = self.by_range[(lo, hi)]
                normed = self.gred[olo:olo + chunk]
                work = self._reduce_scatter(normed, buf)
            else:
                normed, work = buf, self._all_reduce(buf)
            slot = self.buckets
            self.buckets += 1
            if sharded and self.norm_partials is not None and slot >= self.norm_slots():      # (all-reduce: the optimiser takes the norm itself)
                raise RuntimeError(f"{slot + 1} reduce-scattered buckets but {self.norm_slots()} norm slots: size them with "
                                   "FusedAdamW.ensure_norm_slots(len(bucket_list)) (the Trainer does)")
            if self.norm_partials is not None and slot < self.norm_slots():
                self._norm_after(work, normed, self.exchange == "bf16", self.norm_partials.data_ptr() + 4 * slot * hip.SUMSQ_PARTIALS)
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

    def finish_sharded_norm(self, slots: int, sumsq_out: torch.Tensor, guard: Optional[torch.Tensor] = None) -> None:
        """||g||^2 of the rank-summed gradient from the ranks' chunk partial sums: local finish -> scalar all-reduce -> + the small
        region's partial sums (every rank holds the same ones) -> sumsq_out (md_sumsq_finish twice, hip.grad_sumsq), then the step
        guard's go flag when `guard` (its state) is given.  Fixed summation order everywhere: identical bits on all ranks."""
        P = hip.SUMSQ_PARTIALS
        tot = self.fin[P:P + 1]
        hip.grad_sumsq(self.norm_partials, tot, count=slots * P)
        self.all_reduce_now(tot)
        hip.grad_sumsq(self.fin, sumsq_out, count=P + 1, guard=guard)

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
