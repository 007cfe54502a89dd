"""MXFP8 sampling (opt-in): block-scaled fp8 copies of the block linears for the sampler.

`MXWeights(dit)` quantises the bf16 shadow -- what the engine reads: LoRA-merged when an adapter is attached, complete under the sharded
optimiser -- of the targeted linears to OCP MX with e4m3fn elements (one e8m0 scale per 32 consecutive elements along the contraction
dimension; md_mx_quant_rows, the rule of include/microdit_hip.h).  Armed as `engine.mx` (the samplers' `mxfp8=` does that for a run),
those linears quantise their input and run on md_gemm_mxfp8; everything else stays bf16.  Inference only.

Never quantised, whatever `targets` says: adaLN_modulation, the MoE gate (routing must not move), everything on the caption side
(kv_linear, the caption projection and block, the pooled MLP -- cond_cache stays bit-identical on or off), the embedders and the final
layer.  `targets` selects among the rest.
"""
from __future__ import annotations

import re
from types import SimpleNamespace
from typing import Dict, List, Optional

from . import hip
from .arch import param_table

# the linears of every patch-mixer and backbone block that may be quantised, as the engine names them (dense: without ".weight")
_QUANTISABLE = re.compile(r"^(patch_mixer|blocks)\.\d+\.(attn\.(qkv|proj)|cross_attn\.(q_linear|proj)|mlp\.(w1|w2|w3))$")
ALL_TARGETS = r".*"            # every quantisable linear: MXWeights(dit, targets=ALL_TARGETS)
# Classes left OUT of the default set because, at XL/2 sampler shapes on one MI355X, MX GEMM + input quantisation loses to the bf16 launch
# on the same operands by more than the noise floor (scripts/bench_mxfp8.py, profiles/mxfp8.json; sum over bf16 / noise floor of the bf16
# rounds): qkv 2.04 / 0.03, attn.proj 2.11 / 0.04, q_linear 2.07 / 0.09, cross_attn.proj 2.02 / 0.02, [w1; w2] 1.90 / 0.05, w3 1.29 / 0.09,
# expert fc1 1.66 / 0.07, expert fc2 1.85 / 0.06.  That is every class: the first MX kernel (a two-barrier 128^2 tile at 0.11 - 0.19 of
# the fp8 peak) does not beat the tuned bf16 family (0.5 of the bf16 peak), so the default set is EMPTY until a kernel wins a class;
# a class is put back by deleting its alternative here.
DEFAULT_EXCLUDED = re.compile(r"\.(attn\.qkv|attn\.proj|cross_attn\.q_linear|cross_attn\.proj|mlp\.w1|mlp\.w2|mlp\.w3)$")


def target_names(config, targets: Optional[str] = None) -> List[str]:
    """The weights of a model with this DiTConfig that MXWeights(dit, targets) quantises, in parameter-table order, named as the engine
    names them ("blocks.0.attn.qkv" for the nn.Linear weight blocks.0.attn.qkv.weight, "blocks.1.mlp.w1" for an expert tensor).
    targets: a regular expression (re.search on that name) over the quantisable linears; None: the default set, the quantisable linears
    minus the classes of DEFAULT_EXCLUDED.  Pure Python: no GPU, no native library."""
    pat = re.compile(ALL_TARGETS if targets is None else targets)
    out = []
    for spec in param_table(config):
        if spec.buffer or len(spec.shape) < 2:
            continue
        name = spec.name[:-len(".weight")] if spec.name.endswith(".weight") else spec.name
        if _QUANTISABLE.match(name) and pat.search(name) and not (targets is None and DEFAULT_EXCLUDED.search(name)):
            out.append(name)
    return out


def eligible(N: int, K: int) -> bool:
    """What md_gemm_mxfp8 accepts: whole 128-deep k-tiles and whole 16-column output blocks."""
    return N % 16 == 0 and K % 128 == 0


class MXWeights:
    """entries: {engine weight name: namespace(q uint8 [batch, N, K], s uint8 [batch, N, K / 32], N, K, batch)}.  A dense SwiGLU FFN whose
    w1 and w2 are both targeted and adjacent in the shadow (DiTEngine._fused12) is held as the stacked [w1; w2] under the name of w1, the
    way the engine launches it.  Targeted weights md_gemm_mxfp8 does not accept (K % 128, N % 16), and one half of such a stacked pair targeted without the other, are
    listed in `skipped`, take no memory and stay bf16.
    version: the engine's weights_version the copies were made from; the engine refuses a stale one (check_fresh)."""

    def __init__(self, dit, targets: Optional[str] = None):
        dit._ensure_flat()
        self.dit = dit
        self.targets = targets
        names = target_names(dit.config, targets)
        eng = dit.engine
        self.entries: Dict[str, SimpleNamespace] = {}
        self.skipped: List[str] = []
        self._jobs = []                # (entry, source name, rows, K, ld, src_kcontig, batch, source stride, first destination row)
        chosen = set(names)
        for name in names:
            expert = (name + ".weight") not in eng.S
            w = eng.S[name if expert else name + ".weight"]
            if expert:                 # [E, K, N]: the contraction dimension is the strided one
                E, K, N = w.shape
                self._add(name, [(name, N)], K, batch=E, kcontig=False, ld=N, stride=K * N)
                continue
            N, K = w.shape
            pre, leaf = name.rsplit(".", 1)
            if leaf in ("w1", "w2") and pre.endswith(".mlp") and eng._fused12(pre):
                # the engine launches [w1; w2] as one matrix: both halves or neither
                if not {pre + ".w1", pre + ".w2"} <= chosen:
                    self.skipped.append(name)
                elif leaf == "w1":
                    self._add(name, [(pre + ".w1.weight", N), (pre + ".w2.weight", N)], K)
                continue
            self._add(name, [(name + ".weight", N)], K)
        self.version = None
        self.requantize()

    def _add(self, name, parts, K, batch=1, kcontig=True, ld=None, stride=0):
        import torch
        N = sum(n for _, n in parts)
        if not eligible(N, K):
            self.skipped.append(name)
            return
        dev = self.dit.engine.dev
        ent = SimpleNamespace(q=torch.empty(batch, N, K, dtype=torch.uint8, device=dev),
                              s=torch.empty(batch, N, K // hip.MX_BLOCK, dtype=torch.uint8, device=dev), N=N, K=K, batch=batch)
        self.entries[name] = ent
        row = 0
        for src, n in parts:
            self._jobs.append((ent, src, n, K, ld if ld is not None else K, kcontig, batch, stride, row))
            row += n

    def requantize(self) -> "MXWeights":
        """Quantise the current shadow into the existing buffers (no reallocation) and take its version."""
        self.dit.refresh_shadow()
        eng = self.dit.engine
        for ent, src, rows, K, ld, kcontig, batch, stride, row in self._jobs:
            kb = K // hip.MX_BLOCK
            hip.mx_quant_rows(eng.S[src], ent.q.data_ptr() + row * K, ent.s.data_ptr() + row * kb, rows, K, ld=ld, ldd=K, lds=kb,
                              src_kcontig=kcontig, batch=batch, sSrc=stride, sDst=ent.N * K, sScale=ent.N * kb)
        self.version = eng.weights_version
        return self

    def check_fresh(self, weights_version) -> None:
        if self.version != weights_version:
            raise RuntimeError(f"MXWeights mismatch: quantised at weight version {self.version}, the weights are now at {weights_version} "
                               "(call requantize() after the weights change)")

    @property
    def nbytes(self) -> int:
        return sum(e.q.numel() + e.s.numel() for e in self.entries.values())
