"""BPR against `m` negatives per positive row (`ngcf_bpr_multi_f32` / `ngcf_bpr_multi_backward_f32`: csrc/bpr_multi.hip; in the
header next to the BPR section): the loss of `[B, D]` users and positives and `[B*m, D]` negatives without expanding the batch to
`B*m` triplets, and its three gradients.  Like the wrappers of `layers`, no check here costs a host sync."""
from __future__ import annotations

from typing import Tuple

import torch

from .. import _lib
from ._plumbing import Workspace, _on, _ptr, _require_device, _require_dtype, _require_same_device, _stream

M_MAX = 64                                       # NGCF_BPR_MULTI_M_MAX: lane j of a row's wave keeps negative j
REDUCTIONS = {"mean": 0, "softmax": 1}           # NGCF_BPR_MULTI_MEAN, NGCF_BPR_MULTI_SOFTMAX


def _operands(fn: str, u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, m: int, reduction: str) -> Tuple[int, int, int]:
    """The refusals of both calls, before anything reaches the device: (B, D, the reduction's code)."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"{fn}: reduction={reduction!r} is not one of {sorted(REDUCTIONS)}")
    if int(m) != m or m < 1 or m > M_MAX:
        raise ValueError(f"{fn}: m={m} outside [1, {M_MAX}]")
    pairs = (("u", u), ("pos", p), ("neg", n))
    for nm, t in pairs:
        if t.dim() != 2:
            raise ValueError(f"{fn}: {nm} must be 2-D, got shape {tuple(t.shape)}")
    B, D = int(u.shape[0]), int(u.shape[1])
    if B < 1 or D < 1:
        raise ValueError(f"{fn}: u is {tuple(u.shape)}: at least one row and one column expected")
    if tuple(p.shape) != (B, D) or tuple(n.shape) != (B * int(m), D):
        raise ValueError(f"{fn}: u {tuple(u.shape)}, pos {tuple(p.shape)} and neg {tuple(n.shape)} are not [B, D], [B, D] and "
                         f"[B*m, D] with m={m} (no operand broadcasts)")
    _require_dtype(fn, torch.float32, pairs)
    for nm, t in pairs:
        if not t.is_contiguous():
            raise ValueError(f"{fn}: {nm} must be contiguous, got strides {t.stride()}")
    _require_device(u, "u")
    _require_same_device(fn, pairs, "u", u.device)
    return B, D, REDUCTIONS[reduction]


def bpr_multi_loss(u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, m: int, weight_decay: float, batch_size: float,
                   ws: Workspace, reduction: str = "mean") -> torch.Tensor:
    """The loss of `u` [B, D], `p` [B, D] and `n` [B*m, D] (rows b*m .. b*m + m - 1: the negatives of row b), float32 and
    contiguous, as a 0-dim device tensor.  With sp = |u_b.p_b| and sn_j = |u_b.n_bj| a row gives
    -(1/m) sum_j logsigmoid(sp - sn_j) under `reduction="mean"` and -log(e^sp / (e^sp + sum_j e^sn_j)) under "softmax"; the loss is
    (sum of the rows + weight_decay (|u|^2 + |p|^2 + |n|^2 / m)) / batch_size.  "mean" with m = 1 is `bpr_loss` bit for bit, and at
    any m the value of `bpr_loss` over the expanded batch (u and p rows repeated m times) with batch_size * m.  `m` in [1, 64]."""
    B, D, red = _operands("bpr_multi_loss", u, p, n, m, reduction)
    lib = _lib.load()
    w = ws.get(int(lib.ngcf_bpr_multi_workspace_bytes(B)), u.device)
    loss = torch.empty((), dtype=torch.float32, device=u.device)
    with _on(u.device):
        _lib.check(lib.ngcf_bpr_multi_f32(_ptr(u), B, _ptr(p), B, _ptr(n), B * int(m), int(m), D, red, float(weight_decay),
                                          float(batch_size), _ptr(loss), _ptr(w), w.numel(), _stream()))
    return loss


def bpr_multi_backward(u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, m: int, weight_decay: float, batch_size: float,
                       grad_out: torch.Tensor, reduction: str = "mean") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(du, dp, dn) of `bpr_multi_loss` times the upstream scalar `grad_out` (a float32 device tensor of one element); row
    b*m + j of dn belongs to the pair (b, j).  The scores are recomputed, nothing of the forward is kept."""
    B, D, red = _operands("bpr_multi_backward", u, p, n, m, reduction)
    if grad_out.numel() != 1 or grad_out.dtype != torch.float32 or grad_out.device != u.device:
        raise ValueError(f"bpr_multi_backward: grad_out must be one float32 on {u.device}")
    lib = _lib.load()
    du, dp, dn = torch.empty_like(u), torch.empty_like(p), torch.empty_like(n)
    with _on(u.device):
        _lib.check(lib.ngcf_bpr_multi_backward_f32(_ptr(u), B, _ptr(p), B, _ptr(n), B * int(m), int(m), D, red, float(weight_decay),
                                                   float(batch_size), _ptr(grad_out), _ptr(du), _ptr(dp), _ptr(dn), _stream()))
    return du, dp, dn
