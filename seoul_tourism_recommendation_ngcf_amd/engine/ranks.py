"""Exact held-out positions over the full catalogue and the metrics that follow from them (the header's section "exact held-out
positions", csrc/rank_position.hip): the rank of every held-out item among its user's eligible items, then MRR, MAP, AUC, the uncut
NDCG and Recall / NDCG / precision / hit rate at any K up to the catalogue size.  Reached as `engine.ranks.<name>`."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .. import _lib
from ._plumbing import _f32c, _on, _ptr, _require_device, _require_matmul, _row_major_ld, _status_word, _stream, _sums_slots, _unit_inner
from .ranking import ItemSets, _check_sets

POSITION_CAP = 64          # NGCF_RANK_POS_CAP: held-out entries ranked as one row; a longer truth row is cut into such chunks
POSITION_WAVE_ROW = 64     # NGCF_RANK_POS_WAVE_ROW: truth rows up to this length keep their positions in registers in the metrics
POSITION_KS_MAX = 8
NOT_RANKED = -2            # what a fresh position buffer holds until a call ranks the entry's user
_PER_K = ("recall", "ndcg", "precision", "hr")


def _cutoffs(fn: str, ks: Sequence[int], n_items: int):
    ks = [int(x) for x in ks]
    if len(ks) > POSITION_KS_MAX:
        raise ValueError(f"{fn}: at most {POSITION_KS_MAX} cut-offs, got {len(ks)}")
    for K in ks:
        if K < 1 or K > n_items:
            raise ValueError(f"{fn}: cut-off K={K} outside [1, n_items={n_items}]")
    return ks


def _user_ids(fn: str, user_ids: Optional[torch.Tensor], dev):
    if user_ids is None:
        return None
    if user_ids.dtype != torch.int64:
        raise TypeError(f"{fn}: user_ids must be int64, got {user_ids.dtype}")
    if user_ids.device != dev:
        raise RuntimeError(f"{fn}: user_ids is on {user_ids.device}, the other arguments on {dev}")
    return user_ids.reshape(-1).contiguous()


def rank_positions(user_emb: torch.Tensor, item_emb: torch.Tensor, truth: ItemSets, user_ids: Optional[torch.Tensor] = None,
                   exclude: Optional[ItemSets] = None, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """The exact position of every held-out item (ngcf_rank_positions_f32): int32 [truth nnz], aligned with `truth.colidx`.  Entry e
    of user r's truth row, item t, gets the number of r's eligible items i != t that sort before t in `rank_topk`'s order (score
    descending with `rank_topk`'s bits, NaN above +inf, equal scores lowest item first); eligible = not in r's `exclude` row, and
    r's other held-out items count.  So it is t's 0-based index in r's full ranking, and below 256 it is t's column in `rank_topk`'s
    list.  -1: t is in the exclusion row, or (flagged) outside [0, n_items).  With `user_ids`, only those users are ranked (batch row b
    ranks user_emb[user_ids[b]], no gather) and the other users' entries keep what `out` held: chunked calls fill one buffer.  A fresh
    buffer starts at -2, "not ranked".  No score is stored; integer counts only, so the result is identical from run to run and does
    not depend on the batch.  A user id or a held-out id out of range raises IndexError (one host sync); with a caller's int32
    `status` word it is only flagged there (bit 0 user, bit 1 held-out id, bit 2 workspace) and the call does not sync."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    _require_matmul(user_emb, item_emb)
    if user_emb.dtype != torch.float32 or item_emb.dtype != torch.float32:
        raise RuntimeError(f"rank_positions: expected float32 embeddings, got {user_emb.dtype} and {item_emb.dtype}")
    n_rows, D, n_items = int(user_emb.shape[0]), int(user_emb.shape[1]), int(item_emb.shape[0])
    if n_items < 1 or n_items >= 2 ** 31 or D < 1:
        raise ValueError(f"rank_positions: {n_items} items of width {D}")
    if not isinstance(truth, ItemSets):
        raise TypeError("rank_positions: truth must be an ItemSets")
    for what, s in (("truth", truth), ("exclusion", exclude)):
        if s is not None and s.n_items != n_items:
            raise RuntimeError(f"rank_positions: the {what} sets index {s.n_items} items, the item table has {n_items}")
    n_truth = int(truth.colidx.numel())
    if out is not None and (out.dtype != torch.int32 or out.dim() != 1 or int(out.numel()) != n_truth or not out.is_contiguous()):
        raise ValueError(f"rank_positions: out must be a contiguous int32 tensor of {n_truth} entries")
    if user_ids is not None and user_ids.dtype != torch.int64:
        raise TypeError(f"rank_positions: user_ids must be int64, got {user_ids.dtype}")
    _f32c(user_emb, "user_emb"), _f32c(item_emb, "item_emb")
    dev = user_emb.device
    if item_emb.device != dev:
        raise RuntimeError(f"rank_positions: item_emb is on {item_emb.device}, user_emb on {dev}")
    _check_sets(truth, dev, n_rows, "rank_positions")
    if exclude is not None:
        _check_sets(exclude, dev, n_rows, "rank_positions")
    if out is not None and out.device != dev:
        raise RuntimeError(f"rank_positions: out is on {out.device}, the embeddings on {dev}")
    user_ids = _user_ids("rank_positions", user_ids, dev)
    status, check_status = _status_word("rank_positions", status, dev)
    user_emb, item_emb = _unit_inner(user_emb), _unit_inner(item_emb)
    B = n_rows if user_ids is None else int(user_ids.numel())
    if out is None:
        out = torch.full((n_truth,), NOT_RANKED, dtype=torch.int32, device=dev)
    if B == 0 or n_truth == 0:
        return out
    nb = int(lib.ngcf_rank_positions_workspace_bytes(B, n_items, D, n_truth))
    if nb < 0:
        raise ValueError("rank_positions: bad sizes")
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_rank_positions_f32(
            _ptr(user_emb), _row_major_ld(user_emb, "user_emb"), _ptr(user_ids), n_rows, B, _ptr(item_emb),
            _row_major_ld(item_emb, "item_emb"), n_items, D, _ptr(truth.rowptr), _ptr(truth.colidx), truth.col_offset, n_truth,
            _ptr(None if exclude is None else exclude.rowptr), _ptr(None if exclude is None else exclude.colidx),
            0 if exclude is None else exclude.col_offset, _ptr(out), _ptr(status), _ptr(ws), nb, _stream()))
    if check_status:
        _raise_status("rank_positions", int(status.item()), n_rows, n_items)
    return out


def _raise_status(fn: str, word: int, n_rows: int, n_items: int):
    if word & 1:
        raise IndexError(f"{fn}: a user id lies outside [0, {n_rows})")
    if word & 2:
        raise IndexError(f"{fn}: a held-out id lies outside [0, {n_items})")
    if word & 4:
        raise RuntimeError(f"{fn}: the batch repeats users with long truth rows past the workspace; rank it in smaller chunks")


def position_metrics(position: torch.Tensor, truth: ItemSets, ks: Sequence[int], n_items: int, exclude: Optional[ItemSets] = None,
                     user_ids: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None, per_user: bool = False,
                     status: Optional[torch.Tensor] = None):
    """MRR, MAP, NDCG, AUC and Recall / NDCG / precision / hit rate @K (up to 8 K in [1, n_items]) from `rank_positions`' output
    (ngcf_rank_position_metrics), in fp64 on the device.  Batch row b is user user_ids[b] (or b).  T = the user's distinct held-out
    ids, E = n_items - the length of its `exclude` row; users with T = 0 are not evaluated, entries with a negative position are
    misses that stay in every denominator, users with E <= T are left out of the AUC.  The @K values have `ranking_metrics`'
    arithmetic: for K <= 256 they equal it bit for bit.  Returns {"mrr", "map", "ndcg", "auc", "recall@K", "ndcg@K", "precision@K",
    "hr@K", "users", "auc_users"}; with `sums` (a float64 device tensor of 4 + 4*len(ks) + 2 slots, see `position_metrics_from_sums`)
    the call adds into it and returns it instead - chunks of one ranking read back once.  With `per_user` also the float64
    [B, 4 + 4*len(ks)] per-row values (rr, ap, ndcg, auc, then the four @K values per K)."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    n_items = int(n_items)
    if n_items < 1 or n_items >= 2 ** 31:
        raise ValueError(f"position_metrics: n_items={n_items} outside [1, 2^31)")
    ks = _cutoffs("position_metrics", ks, n_items)
    if not isinstance(truth, ItemSets):
        raise TypeError("position_metrics: truth must be an ItemSets")
    n_truth = int(truth.colidx.numel())
    if position.dtype != torch.int32:
        raise TypeError(f"position_metrics: position must be int32, got {position.dtype}")
    if position.dim() != 1 or int(position.numel()) != n_truth:
        raise ValueError(f"position_metrics: position must be [truth nnz = {n_truth}], got {tuple(position.shape)}")
    if user_ids is not None and user_ids.dtype != torch.int64:
        raise TypeError(f"position_metrics: user_ids must be int64, got {user_ids.dtype}")
    _require_device(position, "position")
    dev = position.device
    _check_sets(truth, dev, 0, "position_metrics")
    if exclude is not None:
        _check_sets(exclude, dev, truth.n_rows, "position_metrics")
    user_ids = _user_ids("position_metrics", user_ids, dev)
    B = truth.n_rows if user_ids is None else int(user_ids.numel())
    n_slots = 4 + 4 * len(ks) + 2
    own = sums is None
    sums = _sums_slots("position_metrics", sums, n_slots, dev)
    status, check_status = _status_word("position_metrics", status, dev)
    position = position.contiguous()
    pu = torch.zeros((B, n_slots - 2), dtype=torch.float64, device=dev) if per_user else None
    ks_arr = (C.c_int32 * max(len(ks), 1))(*ks)
    with _on(dev):
        _lib.check(lib.ngcf_rank_position_metrics(
            _ptr(position), B, _ptr(user_ids), truth.n_rows, _ptr(truth.rowptr), _ptr(truth.colidx), n_truth,
            _ptr(None if exclude is None else exclude.rowptr), n_items, ks_arr, len(ks), _ptr(pu), _ptr(sums), _ptr(status), _stream()))
    if check_status and user_ids is not None:
        _raise_status("position_metrics", int(status.item()), truth.n_rows, n_items)
    if not own:
        return (sums, pu) if per_user else sums
    res = position_metrics_from_sums(sums, ks)
    return (res, pu) if per_user else res


def position_metrics_from_sums(sums, ks: Sequence[int]) -> dict:
    """The means of a `position_metrics` slot vector [rr, ap, ndcg, auc, (recall, ndcg, precision, hr) per K, users, auc_users] (one
    read-back): every entry its sum over `users`, "auc" over `auc_users`."""
    ks = [int(x) for x in ks]
    s = torch.as_tensor(sums).double().cpu().tolist()
    if len(s) != 4 + 4 * len(ks) + 2:
        raise ValueError(f"position_metrics_from_sums: {len(s)} slots for {len(ks)} cut-offs ({4 + 4 * len(ks) + 2} expected)")
    n, n_auc = int(round(s[-2])), int(round(s[-1]))
    out = {"mrr": s[0] / n if n else 0.0, "map": s[1] / n if n else 0.0, "ndcg": s[2] / n if n else 0.0,
           "auc": s[3] / n_auc if n_auc else 0.0}
    for q, K in enumerate(ks):
        for j, name in enumerate(_PER_K):
            out[f"{name}@{K}"] = s[4 + 4 * q + j] / n if n else 0.0
    out["users"], out["auc_users"] = n, n_auc
    return out
