"""`BPR` - the reference's loss module (`/root/reference/model/bprloss.py:9-22`) on the fused HIP kernel.

Same constructor and `forward(u, pos, neg)` -> 0-dim tensor.  Kept quirks: the `abs` around both
scores (bprloss.py:18), the divisor is the constructor's `batch_size`, not the actual batch
(bprloss.py:22), and a `[1, D]` positive row broadcasts against `[B, D]` users
(experiment.py:96-100) while its squared norm is counted once.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import engine as _eng
from .autograd import BPRLoss, BPRMultiLoss


class BPR(nn.Module):
    def __init__(self, weight_decay, batch_size):
        super().__init__()
        self.weight_decay = weight_decay
        self.batch_size = batch_size
        self._ws = _eng.Workspace()

    def forward(self, u_idx, pos_idx, neg_idx):
        if torch.is_grad_enabled() and (u_idx.requires_grad or pos_idx.requires_grad or neg_idx.requires_grad):
            return BPRLoss.apply(u_idx, pos_idx, neg_idx, self.weight_decay, self.batch_size, self._ws)
        return _eng.bpr_loss(u_idx.detach(), pos_idx.detach(), neg_idx.detach(), self.weight_decay,
                             self.batch_size, self._ws)


class BPRMulti(nn.Module):
    """`BPR` against `m` negatives per positive row, on the fused HIP kernels of `engine.losses`: same `forward(u, pos, neg)` ->
    0-dim tensor with `u`, `pos` [B, D] and `neg` [B*m, D], rows b*m .. b*m + m - 1 the negatives of row b - what
    `model(..., neg_item=neg.reshape(-1))` returns for `neg` [B, m] ids - instead of a batch expanded to B*m triplets.  A row's
    term is the mean of BPR's over its negatives (`reduction="mean"`: with m = 1 it is `BPR` bit for bit, at any m the value of
    `BPR(weight_decay, batch_size * m)` on the expanded batch) or the softmax of the positive score among the row's scores
    (`"softmax"`: the hardest negatives dominate the gradient).  `BPR`'s kept quirks stay - the `abs` around every score and the
    constructor's `batch_size` as the divisor; nothing broadcasts, and the negatives' squared norms count 1/m each."""

    def __init__(self, weight_decay, batch_size, m, reduction="mean"):
        super().__init__()
        if int(m) != m or m < 1 or m > _eng.losses.M_MAX:
            raise ValueError(f"BPRMulti: m={m} outside [1, {_eng.losses.M_MAX}]")
        if reduction not in _eng.losses.REDUCTIONS:
            raise ValueError(f"BPRMulti: reduction={reduction!r} is not one of {sorted(_eng.losses.REDUCTIONS)}")
        self.weight_decay = weight_decay
        self.batch_size = batch_size
        self.m = int(m)
        self.reduction = reduction
        self._ws = _eng.Workspace()

    def forward(self, u_idx, pos_idx, neg_idx):
        if torch.is_grad_enabled() and (u_idx.requires_grad or pos_idx.requires_grad or neg_idx.requires_grad):
            return BPRMultiLoss.apply(u_idx, pos_idx, neg_idx, self.m, self.weight_decay, self.batch_size, self._ws, self.reduction)
        return _eng.losses.bpr_multi_loss(u_idx.detach().contiguous(), pos_idx.detach().contiguous(), neg_idx.detach().contiguous(),
                                          self.m, self.weight_decay, self.batch_size, self._ws, self.reduction)
