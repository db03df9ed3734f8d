"""BPR against `m` negatives per positive row (`ngcf_bpr_multi_f32` / `ngcf_bpr_multi_backward_f32`: csrc/bpr_multi.hip; in the
header next to the BPR section): the loss of `[B, D]` users and positives and `[B*m, D]` negatives without expanding the batch to
`B*m` triplets, and its three gradients; the sampled softmax over the same operands with the logQ correction and a temperature
(`ngcf_sampled_softmax_f32` / `ngcf_sampled_softmax_backward_f32`: csrc/sampled_softmax.hip); and the limit of that series, the softmax over the WHOLE catalogue (`ngcf_softmax_full_f32`
/ `ngcf_softmax_full_backward_f32`: csrc/softmax_full.hip), whose [B, n_items] score matrix is never in memory; and the softmax with
shared (in-batch) negatives on the same kernels (`ngcf_inbatch_softmax_f32` / `ngcf_inbatch_softmax_backward_f32`:
csrc/inbatch_softmax.hip).  Like the wrappers of `layers`, no check here costs a host sync."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib
from ._plumbing import Workspace, _on, _ptr, _require_device, _require_dtype, _require_same_device, _status_word, _stream

M_MAX = 64                                       # NGCF_BPR_MULTI_M_MAX: lane j of a row's wave keeps negative j
REDUCTIONS = {"mean": 0, "softmax": 1}           # NGCF_BPR_MULTI_MEAN, NGCF_BPR_MULTI_SOFTMAX


# ---- stated once for several calls (`fn`, `pairs`: as in `_plumbing`); the order of refusals in the `_*operands` below is behaviour
def _require_m(fn: str, m) -> int:
    if int(m) != m or m < 1 or m > M_MAX:
        raise ValueError(f"{fn}: m={m} outside [1, {M_MAX}]")
    return int(m)


def _rows_cols(fn: str, pairs) -> Tuple[int, int]:
    """Every table of `pairs` is 2-D; (B, D) of the first, `u`, neither of them 0."""
    for nm, t in pairs:
        if t is not None and t.dim() != 2:
            raise ValueError(f"{fn}: {nm} must be 2-D, got shape {tuple(t.shape)}")
    u = pairs[0][1]
    B, D = int(u.shape[0]), int(u.shape[1])
    if B < 1 or D < 1:
        raise ValueError(f"{fn}: u is {tuple(u.shape)}: at least one row and one column expected")
    return B, D


def _require_rows(fn: str, pairs) -> None:
    """The strided layout of the full and in-batch calls' 2-D float32 tables (dimensions and types: refused before, with the sizes)."""
    for nm, t in pairs:
        if t is not None and t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError(f"{fn}: {nm} must have unit stride in its last dimension, got strides {t.stride()}")
        if t is not None and t.shape[0] > 1 and t.stride(0) < t.shape[1]:
            raise ValueError(f"{fn}: the rows of {nm} overlap, strides {t.stride()}")


def _require_corrections(fn: str, pairs) -> None:
    for nm, t in pairs:
        if t is not None and t.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{fn}: {nm} must be float32 or float64, got {t.dtype}")


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:     # (a correction as the kernels read it: the one cast per call)
    return None if t is None else t.to(torch.float32).contiguous()


def _require_inv_tau(fn: str, inv_tau: float) -> None:
    if not (inv_tau > 0 and inv_tau < float("inf")):
        raise ValueError(f"{fn}: inv_tau={inv_tau} is not a positive finite number")


def _require_lse(fn: str, lse: torch.Tensor, B: int, dev, nm: str = "lse") -> None:
    if lse.dtype != torch.float32 or tuple(lse.shape) != (B,) or lse.device != dev or not lse.is_contiguous():
        raise ValueError(f"{fn}: {nm} must be a contiguous float32 tensor of {B} elements on {dev}")


def _plan(entry: str, *shape: int):                                 # (the three (pieces, slabs) pairs of a host-only plan entry)
    import ctypes as C
    out = (C.c_int64 * 6)()
    _lib.check(getattr(_lib.load(), entry)(*(int(x) for x in shape), out))
    return (out[0], out[1]), (out[2], out[3]), (out[4], out[5])


def _launch(dev, entry, *args) -> None:                             # (`entry(*args, stream)` on `dev`, checked)
    with _on(dev):
        _lib.check(entry(*args, _stream()))


def _empty(dev, *shape: int, need: bool = True) -> Optional[torch.Tensor]:      # (an output; None for a gradient nobody needs)
    return torch.empty(shape, dtype=torch.float32, device=dev) if need else None


def _operands(fn: str, u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, m: int, reduction: str) -> Tuple[int, int, int]:
    """The refusals of both calls, before anything reaches the device: (B, D, the reduction's code)."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"{fn}: reduction={reduction!r} is not one of {sorted(REDUCTIONS)}")
    _require_m(fn, m)
    pairs = (("u", u), ("pos", p), ("neg", n))
    B, D = _rows_cols(fn, pairs)
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


def _require_grad_out(fn: str, grad_out: torch.Tensor, device: torch.device) -> None:
    if grad_out.numel() != 1 or grad_out.dtype != torch.float32 or grad_out.device != device:
        raise ValueError(f"{fn}: grad_out must be one float32 on {device}")


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
    loss = _empty(u.device)
    _launch(u.device, lib.ngcf_bpr_multi_f32, _ptr(u), B, _ptr(p), B, _ptr(n), B * int(m), int(m), D, red, float(weight_decay),
            float(batch_size), _ptr(loss), _ptr(w), w.numel())
    return loss


def bpr_multi_backward(u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, m: int, weight_decay: float, batch_size: float,
                       grad_out: torch.Tensor, reduction: str = "mean") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(du, dp, dn) of `bpr_multi_loss` times the upstream scalar `grad_out` (a float32 device tensor of one element); row
    b*m + j of dn belongs to the pair (b, j).  The scores are recomputed, nothing of the forward is kept."""
    B, D, red = _operands("bpr_multi_backward", u, p, n, m, reduction)
    _require_grad_out("bpr_multi_backward", grad_out, u.device)
    lib = _lib.load()
    du, dp, dn = torch.empty_like(u), torch.empty_like(p), torch.empty_like(n)
    _launch(u.device, lib.ngcf_bpr_multi_backward_f32, _ptr(u), B, _ptr(p), B, _ptr(n), B * int(m), int(m), D, red, float(weight_decay),
            float(batch_size), _ptr(grad_out), _ptr(du), _ptr(dp), _ptr(dn))
    return du, dp, dn


# ---- the sampled softmax with logQ correction (`ngcf_sampled_softmax_f32` / `ngcf_sampled_softmax_backward_f32`: csrc/sampled_softmax.hip)
def _corrections(fn: str, u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, logq: torch.Tensor, pos_logq: Optional[torch.Tensor],
                 m: int, inv_tau: float) -> Tuple[int, int, torch.Tensor, Optional[torch.Tensor]]:
    """The refusals of both sampled-softmax calls, before anything reaches the device, in the order of `_operands`, whose own come
    last because they end with the device: sizes (ValueError), types (TypeError), the temperature, the operands, the devices
    (RuntimeError).  -> (B, D, logq, pos_logq), the two corrections as contiguous float32 (a float64 one is cast once, here)."""
    if u.dim() == 2 and int(m) == m and m >= 1:                                 # (anything else: `_operands` below says so)
        rows = int(u.shape[0])
        if tuple(logq.shape) not in ((rows, int(m)), (rows * int(m),)):
            raise ValueError(f"{fn}: logq must be [B, m] or [B*m] with B={rows}, m={m}, got shape {tuple(logq.shape)}")
        if pos_logq is not None and tuple(pos_logq.shape) != (rows,):
            raise ValueError(f"{fn}: pos_logq must be [B] with B={rows}, got shape {tuple(pos_logq.shape)}")
    _require_corrections(fn, (("logq", logq), ("pos_logq", pos_logq)))
    _require_inv_tau(fn, inv_tau)
    B, D, _ = _operands(fn, u, p, n, m, "softmax")
    _require_same_device(fn, (("logq", logq), ("pos_logq", pos_logq)), "u", u.device)
    return B, D, _f32(logq.reshape(-1)), _f32(pos_logq)


def sampled_softmax_loss(u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, logq: torch.Tensor, m: int, inv_tau: float,
                         weight_decay: float, batch_size: float, ws: Workspace, pos_logq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The sampled softmax loss with the logQ correction of `u` [B, D], `p` [B, D] and `n` [B*m, D] (rows b*m .. b*m + m - 1: the
    negatives of row b; float32 and contiguous, as `bpr_multi_loss` takes them), as a 0-dim device tensor.  `logq` ([B, m] or [B*m],
    float32 or float64) holds the log proposal probability of every negative as its sampler drew it - for
    `sampling.weighted_negatives(..., return_logq=True)` the conditional log(w_j / U_j) of successive sampling, not a marginal
    inclusion probability - and `pos_logq` [B] the positives' correction (None: exactly 0).  With plain scores (no `abs`),
    z_0 = (u_b.p_b) inv_tau - pos_logq[b] and z_j = (u_b.n_bj) inv_tau - logq[b, j - 1], a row gives logsumexp(z_0 .. z_m) - z_0;
    the loss is (sum of the rows + weight_decay (|u|^2 + |p|^2 + |n|^2 / m)) / batch_size, `bpr_multi_loss`'s regulariser and
    divisor.  With inv_tau = 1, zero corrections and positive dot products it is `bpr_multi_loss(..., reduction="softmax")` bit
    for bit.  The corrections are data (no gradient); non-finite values in them are undefined.  `m` in [1, 64]."""
    B, D, logq, pos_logq = _corrections("sampled_softmax_loss", u, p, n, logq, pos_logq, m, inv_tau)
    lib = _lib.load()
    w = ws.get(int(lib.ngcf_sampled_softmax_workspace_bytes(B)), u.device)
    loss = _empty(u.device)
    _launch(u.device, lib.ngcf_sampled_softmax_f32, _ptr(u), B, _ptr(p), B, _ptr(n), B * int(m), int(m), D, _ptr(logq), _ptr(pos_logq),
            float(inv_tau), float(weight_decay), float(batch_size), _ptr(loss), _ptr(w), w.numel())
    return loss


def sampled_softmax_backward(u: torch.Tensor, p: torch.Tensor, n: torch.Tensor, logq: torch.Tensor, m: int, inv_tau: float,
                             weight_decay: float, batch_size: float, grad_out: torch.Tensor, pos_logq: Optional[torch.Tensor] = None
                             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(du, dp, dn) of `sampled_softmax_loss` times the upstream scalar `grad_out` (a float32 device tensor of one element); row
    b*m + j of dn belongs to the pair (b, j).  The scores are recomputed, nothing of the forward is kept."""
    B, D, logq, pos_logq = _corrections("sampled_softmax_backward", u, p, n, logq, pos_logq, m, inv_tau)
    _require_grad_out("sampled_softmax_backward", grad_out, u.device)
    lib = _lib.load()
    du, dp, dn = torch.empty_like(u), torch.empty_like(p), torch.empty_like(n)
    _launch(u.device, lib.ngcf_sampled_softmax_backward_f32, _ptr(u), B, _ptr(p), B, _ptr(n), B * int(m), int(m), D, _ptr(logq),
            _ptr(pos_logq), float(inv_tau), float(weight_decay), float(batch_size), _ptr(grad_out), _ptr(du), _ptr(dp), _ptr(dn))
    return du, dp, dn


# ---- the softmax over the whole catalogue (`ngcf_softmax_full_f32` / `ngcf_softmax_full_backward_f32`: csrc/softmax_full.hip) ------
def _full_operands(fn: str, u: torch.Tensor, items: torch.Tensor, pos: torch.Tensor, inv_tau: float) -> Tuple[int, int, int]:
    """The refusals of both full-catalogue calls, before anything reaches the device: (B, n_items, D, pos contiguous)."""
    rows = (("u", u), ("items", items))
    (B, D), n_items = _rows_cols(fn, rows), int(items.shape[0])
    if pos.dim() != 1:
        raise ValueError(f"{fn}: pos must be 1-D, got shape {tuple(pos.shape)}")
    if n_items < 1:
        raise ValueError(f"{fn}: items is {tuple(items.shape)}: at least one item expected")
    if int(items.shape[1]) != D:
        raise ValueError(f"{fn}: u {tuple(u.shape)} and items {tuple(items.shape)} differ in width")
    if int(pos.shape[0]) != B:
        raise ValueError(f"{fn}: pos has {int(pos.shape[0])} ids for {B} rows of u")
    _require_dtype(fn, torch.float32, rows)
    _require_dtype(fn, torch.int64, (("pos", pos),))
    _require_rows(fn, rows)
    _require_inv_tau(fn, inv_tau)
    _require_device(u, "u")
    _require_same_device(fn, (("items", items), ("pos", pos)), "u", u.device)
    return B, n_items, D, pos.contiguous()


def _ld(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def softmax_full_plan(B: int, n_items: int, D: int) -> dict:
    """How the three launches cut a shape (host only): pieces of the walked side and column slabs of the forward, dU and dI."""
    return dict(zip(("forward", "du", "ditems"), _plan("ngcf_softmax_full_plan", B, n_items, D)))


def softmax_full_loss(u: torch.Tensor, items: torch.Tensor, pos: torch.Tensor, inv_tau: float, weight_decay: float, batch_size: float,
                      ws: Workspace, status: Optional[torch.Tensor] = None, spos: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`(loss, lse)` of the softmax over the whole catalogue: `u` [B, D] and `items` [n_items, D] float32 rows (unit inner stride, any
    row stride: `model.all_items_emb` as it is), `pos` [B] int64.  With s_bj = <u_b, i_j> * inv_tau, `lse` [B] is logsumexp_j s_bj and
    the loss (sum_b (lse_b - s_b,pos_b) + weight_decay (|u|^2 + sum_b |i_pos_b|^2)) / batch_size as a 0-dim device tensor; no
    [B, n_items] matrix exists.  An id of `pos` outside the catalogue is never an index: its row has no positive term and bit 0 of
    `status` (an int32 device word, sticky; None: a word nobody reads) is set - no check here costs a host sync.  `spos` [B]
    float32, when given, receives the positives' scores."""
    B, n_items, D, pos = _full_operands("softmax_full_loss", u, items, pos, inv_tau)
    dev = u.device
    status, _ = _status_word("softmax_full_loss", status, dev)
    if spos is None:
        spos = _empty(dev, B)
    else:
        _require_lse("softmax_full_loss", spos, B, dev, "spos")
    lib = _lib.load()
    w = ws.get(int(lib.ngcf_softmax_full_workspace_bytes(B, n_items, D)), dev)
    loss, lse = _empty(dev), _empty(dev, B)
    _launch(dev, lib.ngcf_softmax_full_f32, _ptr(u), _ld(u), B, _ptr(items), _ld(items), n_items, D, _ptr(pos), float(inv_tau),
            float(weight_decay), float(batch_size), _ptr(loss), _ptr(lse), _ptr(spos), _ptr(status), _ptr(w), w.numel())
    return loss, lse


def softmax_full_backward(u: torch.Tensor, items: torch.Tensor, pos: torch.Tensor, lse: torch.Tensor, inv_tau: float,
                          weight_decay: float, batch_size: float, grad_out: torch.Tensor, ws: Workspace, need_u: bool = True,
                          need_items: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """`(du, ditems)` of `softmax_full_loss` times the upstream scalar `grad_out` (one float32 on the device), from the `lse` the
    forward returned: the scores are recomputed, two launches of one kernel with the roles swapped.  `ditems` is dense, [n_items, D]
    contiguous; a gradient that is not needed (`need_u` / `need_items` False) is not computed and comes back as None."""
    B, n_items, D, pos = _full_operands("softmax_full_backward", u, items, pos, inv_tau)
    dev = u.device
    _require_lse("softmax_full_backward", lse, B, dev)
    _require_grad_out("softmax_full_backward", grad_out, dev)
    if not (need_u or need_items):
        return None, None
    lib = _lib.load()
    w = ws.get(int(lib.ngcf_softmax_full_workspace_bytes(B, n_items, D)), dev)
    du, di = _empty(dev, B, D, need=need_u), _empty(dev, n_items, D, need=need_items)
    _launch(dev, lib.ngcf_softmax_full_backward_f32, _ptr(u), _ld(u), B, _ptr(items), _ld(items), n_items, D, _ptr(pos), _ptr(lse),
            float(inv_tau), float(weight_decay), float(batch_size), _ptr(grad_out), _ptr(du), D, _ptr(di), D, _ptr(w), w.numel())
    return du, di


# ---- the softmax with shared (in-batch) negatives (`ngcf_inbatch_softmax_f32` / `ngcf_inbatch_softmax_backward_f32`: csrc/inbatch_softmax.hip)
def _inbatch_operands(fn: str, u: torch.Tensor, p: torch.Tensor, inv_tau: float, ids, logq, pos_logq, extra, extra_ids, extra_logq):
    """The refusals of both in-batch calls, before anything reaches the device, in the order of `_full_operands` and `_corrections`:
    sizes (ValueError), types (TypeError), the temperature, the devices (RuntimeError).
    -> (B, E, D, extra or None, ids, extra_ids, logq, extra_logq, pos_logq), the corrections as contiguous float32 (a float64 one is
    cast once, here), the ids contiguous; what goes with the extras is None when there are none."""
    rows = (("u", u), ("pos", p), ("extra", extra))
    B, D = _rows_cols(fn, rows)
    if tuple(p.shape) != (B, D):
        raise ValueError(f"{fn}: u {tuple(u.shape)} and pos {tuple(p.shape)} are not both [B, D]")
    E = 0 if extra is None else int(extra.shape[0])
    if extra is not None and int(extra.shape[1]) != D:
        raise ValueError(f"{fn}: u {tuple(u.shape)} and extra {tuple(extra.shape)} differ in width")
    if B + E >= 2 ** 31:
        raise ValueError(f"{fn}: B + E = {B + E} columns, below 2^31 expected")
    for nm, t, n, of in (("ids", ids, B, "B"), ("logq", logq, B, "B"), ("pos_logq", pos_logq, B, "B"), ("extra_ids", extra_ids, E, "E"),
                         ("extra_logq", extra_logq, E, "E")):
        if t is not None and tuple(t.shape) != (n,):
            raise ValueError(f"{fn}: {nm} must be [{of}] with {of}={n}, got shape {tuple(t.shape)}")
    if ids is not None and E > 0 and extra_ids is None:
        raise ValueError(f"{fn}: ids given with {E} extra rows and no extra_ids: the mask needs the extras' ids too")
    _require_dtype(fn, torch.float32, rows)
    _require_dtype(fn, torch.int64, (("ids", ids), ("extra_ids", extra_ids)))
    _require_corrections(fn, (("logq", logq), ("pos_logq", pos_logq), ("extra_logq", extra_logq)))
    _require_rows(fn, rows)
    _require_inv_tau(fn, inv_tau)
    _require_device(u, "u")
    _require_same_device(fn, (("pos", p), ("extra", extra), ("ids", ids), ("extra_ids", extra_ids), ("logq", logq),
                              ("pos_logq", pos_logq), ("extra_logq", extra_logq)), "u", u.device)
    i64 = lambda t: None if t is None else t.contiguous()  # noqa: E731
    if E == 0:
        extra = extra_ids = extra_logq = None
    return B, E, D, extra, i64(ids), i64(extra_ids), _f32(logq), _f32(extra_logq), _f32(pos_logq)


def inbatch_softmax_plan(B: int, E: int, D: int) -> dict:
    """How the three launches cut a shape (host only): pieces of the walked side and column slabs of the forward, dU and the columns'
    gradient (dp over dx) - `softmax_full_plan(B, B + E, D)`."""
    return dict(zip(("forward", "du", "dcolumns"), _plan("ngcf_inbatch_softmax_plan", B, E, D)))


def inbatch_softmax_loss(u: torch.Tensor, p: torch.Tensor, inv_tau: float, weight_decay: float, batch_size: float, ws: Workspace, *,
                         ids: Optional[torch.Tensor] = None, logq: Optional[torch.Tensor] = None,
                         pos_logq: Optional[torch.Tensor] = None, extra: Optional[torch.Tensor] = None,
                         extra_ids: Optional[torch.Tensor] = None, extra_logq: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`(loss, lse)` of the softmax with shared (in-batch) negatives: `u` [B, D] user rows and `p` [B, D] their positives' rows,
    `extra` [E, D] further rows that every row of the batch takes as negatives (float32, unit inner stride, any row stride).  The
    columns are c_j = p_j (j < B), then the extras; `ids` [B] / `extra_ids` [E] int64 are their item ids, `logq` [B] / `extra_logq`
    [E] their corrections, `pos_logq` [B] the diagonal's (float32 or float64; None is exactly 0).  With plain scores
    s_bj = <u_b, c_j> * inv_tau: z_bb = s_bb - pos_logq[b], z_bj = s_bj - q_j off the diagonal; with `ids`, a column j != b whose id is
    ids[b] is a false negative and leaves row b's softmax.  `lse` [B] is the logsumexp of a row's unmasked z, the loss
    (sum_b (lse_b - z_bb) + weight_decay (|u|^2 + |p|^2)) / batch_size as a 0-dim device tensor - the extras are not regularised.
    No [B, B + E] matrix exists.  Ids are only compared, never an index.  Without ids and corrections it is
    `softmax_full_loss(u, cat(p, extra), arange(B), ...)` bit for bit."""
    B, E, D, x, ids, xids, logq, xlogq, pos_logq = _inbatch_operands("inbatch_softmax_loss", u, p, inv_tau, ids, logq, pos_logq, extra,
                                                                     extra_ids, extra_logq)
    dev = u.device
    lib = _lib.load()
    w = ws.get(int(lib.ngcf_inbatch_softmax_workspace_bytes(B, E, D)), dev)
    loss, lse = _empty(dev), _empty(dev, B)
    _launch(dev, lib.ngcf_inbatch_softmax_f32, _ptr(u), _ld(u), B, _ptr(p), _ld(p), _ptr(x), _ld(x) if E else D, E, D, _ptr(ids),
            _ptr(xids), _ptr(logq), _ptr(xlogq), _ptr(pos_logq), float(inv_tau), float(weight_decay), float(batch_size), _ptr(loss),
            _ptr(lse), _ptr(w), w.numel())
    return loss, lse


def inbatch_softmax_backward(u: torch.Tensor, p: torch.Tensor, inv_tau: float, weight_decay: float, batch_size: float, lse: torch.Tensor,
                             grad_out: torch.Tensor, ws: Workspace, need_u: bool = True, need_p: bool = True, need_extra: bool = True, *,
                             ids: Optional[torch.Tensor] = None, logq: Optional[torch.Tensor] = None,
                             pos_logq: Optional[torch.Tensor] = None, extra: Optional[torch.Tensor] = None,
                             extra_ids: Optional[torch.Tensor] = None, extra_logq: Optional[torch.Tensor] = None
                             ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """`(du, dp, dx)` of `inbatch_softmax_loss` times the upstream scalar `grad_out` (one float32 on the device), from the `lse` the
    forward returned: the scores are recomputed, two launches of one kernel with the roles swapped.  A gradient that is not needed
    (`need_u` / `need_p` / `need_extra` False) is not stored and comes back as None, and so does `dx` without extras; the others
    keep their bits.  The ids and corrections carry no gradient."""
    fn = "inbatch_softmax_backward"
    B, E, D, x, ids, xids, logq, xlogq, pos_logq = _inbatch_operands(fn, u, p, inv_tau, ids, logq, pos_logq, extra, extra_ids, extra_logq)
    dev = u.device
    _require_lse(fn, lse, B, dev)
    _require_grad_out(fn, grad_out, dev)
    need_extra = bool(need_extra) and E > 0
    if not (need_u or need_p or need_extra):
        return None, None, None
    lib = _lib.load()
    w = ws.get(int(lib.ngcf_inbatch_softmax_workspace_bytes(B, E, D)), dev)
    du, dp, dx = _empty(dev, B, D, need=need_u), _empty(dev, B, D, need=need_p), _empty(dev, E, D, need=need_extra)
    _launch(dev, lib.ngcf_inbatch_softmax_backward_f32, _ptr(u), _ld(u), B, _ptr(p), _ld(p), _ptr(x), _ld(x) if E else D, E, D, _ptr(ids),
            _ptr(xids), _ptr(logq), _ptr(xlogq), _ptr(pos_logq), _ptr(lse), float(inv_tau), float(weight_decay), float(batch_size),
            _ptr(grad_out), _ptr(du), D, _ptr(dp), D, _ptr(dx), D, _ptr(w), w.numel())
    return du, dp, dx
