"""Learned caption tokens: textual inversion in embedding space, on a frozen network.

The first consumer of the caption gradient `LatentDiffusion.edm_loss` returns when `y.requires_grad`: a handful of token embeddings
are the only trainable tensor, the network's parameters stay frozen, and the engine runs its dgrad-only backward (no weight gradient
is computed, `p.grad` stays None).  No Trainer, config or checkpoint integration: the module is a plain `nn.Module` and its one
parameter is saved and loaded like any other.

    model.dit.requires_grad_(False)                       # freeze the network
    learned = LearnedCaption(n_tokens=4, caption_channels=1024, init=y[0, 0, 1:5]).to("cuda")
    opt = torch.optim.AdamW(learned.parameters(), lr=1e-3, weight_decay=0.0)
    pos = torch.tensor([1, 2, 3, 4], device="cuda")       # the token rows of every caption the learned tokens stand in
    for latents, y in loader:                             # y: text-encoder output [B, 1, L, Dc] (or [B, L, Dc])
        loss = model.edm_loss(latents, learned(y, pos))
        opt.zero_grad(set_to_none=True)
        loss.backward()                                   # dgrad-only backward; only learned.tokens.grad is written
        opt.step()
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn


class LearnedCaption(nn.Module):
    """`n_tokens` trainable caption-token embeddings, one fp32 parameter `tokens` [n_tokens, caption_channels].
    init: values to start from ([n_tokens, caption_channels], any float dtype; e.g. the encoder's embedding of a placeholder word);
    None: zeros."""

    def __init__(self, n_tokens: int, caption_channels: int, init: Optional[torch.Tensor] = None):
        super().__init__()
        if n_tokens <= 0 or caption_channels <= 0:
            raise ValueError("n_tokens and caption_channels must be positive")
        if init is None:
            start = torch.zeros(n_tokens, caption_channels, dtype=torch.float32)
        else:
            if tuple(init.shape) != (n_tokens, caption_channels):
                raise ValueError(f"init must be [{n_tokens}, {caption_channels}], got {tuple(init.shape)}")
            start = init.detach().to(torch.float32).clone()
        self.tokens = nn.Parameter(start)

    def forward(self, y: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        """y [B, L, Dc] or [B, 1, L, Dc] with the token rows `positions` (n_tokens distinct indices into L) of every sample replaced by
        the learned tokens.  Differentiable with respect to the tokens (each gets the sum of its row's gradient over the batch) and, if
        it requires grad, to the rows of y that were not replaced.  The result has y's shape and dtype; y itself is not modified."""
        n, Dc = self.tokens.shape
        if y.dim() not in (3, 4) or y.shape[-1] != Dc:
            raise ValueError(f"y must be [B, L, {Dc}] or [B, 1, L, {Dc}], got {tuple(y.shape)}")
        pos = torch.as_tensor(positions, device=y.device, dtype=torch.long).reshape(-1)
        if pos.numel() != n:
            raise ValueError(f"{n} learned tokens need {n} positions, got {pos.numel()}")
        L = y.shape[-2]
        if pos.numel() and (int(pos.min()) < 0 or int(pos.max()) >= L or torch.unique(pos).numel() != n):
            raise ValueError(f"positions must be {n} distinct indices in [0, {L})")
        rows = self.tokens.to(y.dtype).expand(*y.shape[:-2], n, Dc)
        return y.index_copy(-2, pos, rows)
