"""Dispersive loss (opt-in): a batch-repulsion regulariser on the output of one backbone block (Wang & He 2025, "Diffuse
and Disperse", the InfoNCE-l2 form).  For the B samples of a microbatch, Z [B, K] the block's bf16 output with each sample flattened
(K = kept tokens x width):

    D_ij = |z_i - z_j|^2 / K        L = log( mean_ij exp(-D_ij / tau) )        objective = L_edm + weight * L

L <= 0, = 0 for B = 1 or identical rows, -> log(1 / B) when every pair is far apart.  No parameters, no encoder, no extra data: the
cost is two skinny GEMMs per microbatch (the Gram Z Z^T and the injection dx += W' Z) around md_disperse_pairs.  Pairs are formed
inside one microbatch on one rank.  The term exists on the Trainer's microbatch path only (LatentDiffusion.train_microbatch); it is
never computed at evaluation.

OFF BY DEFAULT, and the starting values weight = 0.5, tau = 0.5, block = depth // 4 are the paper's for DiT / SiT: nobody has tuned
them for MicroDiT and nothing here claims a quality gain.

This module holds the switch (`DisperseLoss`) and the definition in torch fp64 (`reference`), which the tests compare the kernels with.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class DisperseLoss:
    """weight: lambda >= 0 (0 = off); tau > 0; block: index of the backbone block whose output is regularised (None: depth // 4)."""
    weight: float = 0.5
    tau: float = 0.5
    block: Optional[int] = None

    def __post_init__(self):
        for name in ("weight", "tau"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"DisperseLoss.{name} must be a finite number, got {v!r}")
            setattr(self, name, float(v))
        if self.weight < 0:
            raise ValueError(f"DisperseLoss.weight must not be negative, got {self.weight}")
        if not self.tau > 0:
            raise ValueError(f"DisperseLoss.tau must be positive, got {self.tau}")
        if self.block is not None:
            if isinstance(self.block, bool) or not isinstance(self.block, int) or self.block < 0:
                raise ValueError(f"DisperseLoss.block must be a block index >= 0 or None, got {self.block!r}")

    @property
    def enabled(self) -> bool:
        return self.weight > 0

    def resolve_block(self, depth: int) -> int:
        """The block index for a backbone of `depth` blocks (default depth // 4); raises when it is out of range."""
        if depth < 1:
            raise ValueError("the dispersive loss needs at least one backbone block")
        k = depth // 4 if self.block is None else self.block
        if not 0 <= k < depth:
            raise ValueError(f"DisperseLoss.block = {k} is outside the backbone's {depth} blocks")
        return k


def reference(z: torch.Tensor, tau: float):
    """The definition in fp64: z [B, K] (any float dtype) -> (L, dL/dz [B, K], mean off-diagonal D), all fp64.

        G = z z^T,  n_i = G_ii,  D_ij = max(0, n_i + n_j - 2 G_ij) / K (i != j),  D_ii = 0 exactly
        E = exp(-D / tau),  S = sum_ij E_ij (>= B: the diagonal is exp(0)),  L = log(S / B^2),  p = E / S
        dL/dz_a = 4 / (tau K) sum_j W_aj z_j,   W_aj = p_aj (j != a),  W_aa = -sum_{j != a} p_aj   (never p_aa - rho_a, which cancels)
    """
    z = z.detach().to(torch.float64)
    B, K = z.shape
    W, L, md = reference_weights(z @ z.t(), K, tau)
    # sum_j W_aj z_j written as sum_{j != a} p_aj (z_j - z_a): the same number, and exactly 0 for identical rows
    g = torch.stack([W[a] @ (z - z[a]) for a in range(B)])
    return L, (4.0 / (tau * K)) * g, md


def reference_weights(G: torch.Tensor, K: int, tau: float):
    """(W [B, B], L, mean off-diagonal D) of the definition from a Gram matrix, in fp64."""
    G = G.to(torch.float64)
    B = G.shape[0]
    n = torch.diagonal(G)
    off = ~torch.eye(B, dtype=torch.bool, device=G.device)
    D = torch.clamp(n[:, None] + n[None, :] - 2.0 * G, min=0.0) / K
    D = torch.where(off, D, torch.zeros_like(D))
    E = torch.exp(-D / tau)
    S = E.sum()
    L = torch.log(S / (B * B))
    P = torch.where(off, E / S, torch.zeros_like(E))
    W = P - torch.diag(P.sum(dim=1))
    md = D.sum() / (B * (B - 1)) if B > 1 else torch.zeros((), dtype=torch.float64, device=G.device)
    return W, L, md
