"""Hard negatives on the device (`ngcf_sample_hard_f32`: csrc/sample_hard.hip; in the header next to `ngcf_sample_unseen`): of `m`
unseen draws per case, the one the current embeddings score highest - `sample_unseen`, `eval_candidates`' scores and an argmax in
one launch, with one item per case written to memory."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._plumbing import (_f32c, _on, _ptr, _require_device, _require_dtype, _require_matmul, _require_same_device, _row_major_ld,
                        _status_word, _stream, _unit_inner)
from .ranking import ItemSets, _check_sets

HARD_M_MAX = 64


def hard_unseen(seen: ItemSets, user_emb: torch.Tensor, item_emb: torch.Tensor, user_ids: torch.Tensor, m: int, seed: int, *,
                case_offset: int = 0, return_score: bool = False, return_slot: bool = False, out: Optional[torch.Tensor] = None,
                status: Optional[torch.Tensor] = None):
    """Per case the best-scoring of `m` unseen draws (ngcf_sample_hard_f32): case t of user u = `user_ids[t]` (int64 [T]) draws the
    row t of `sample_unseen(seen, user_ids, m, seed, case_offset=case_offset)`, scores every drawn item c against the user,
    <user_emb[u], item_emb[c]> with the bits of `eval_candidates`' scores, and keeps the largest in `topk_rows`' order (NaN above
    +inf; equal bits: the lowest column) - the composition of the two calls and an argmax, bit for bit, without the [T, m]
    candidates and scores in memory.  `m` in [1, 64]; with m = 1 it is `sample_unseen`'s one item, whatever the tables.  `user_emb`
    [>= seen.n_rows, D] and `item_emb` [>= seen.n_items, D] float32 on the sets' device; strided views (rows of all_E) are taken as
    they are, tables that require grad are detached.  Returns the int64 [T] items - or a tuple (items, score float32 [T] with
    `return_score`, slot int32 [T] with `return_slot`: the winner's score and its column of the draw).  `out`: a contiguous
    int64 [T] tensor to write the items into.  A user id outside the sets raises IndexError, a user with fewer than `m` unseen items
    ValueError, after one host sync; such a case gets item -1, slot -1 and a NaN score.  With a caller's int32 `status` word the
    bits (1, 2) are only OR-ed into it and the call neither syncs nor raises."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    m, seed = int(m), int(seed) & 0xFFFFFFFFFFFFFFFF
    if m < 1 or m > HARD_M_MAX:
        raise ValueError(f"hard_unseen: m={m} outside [1, {HARD_M_MAX}]")
    if seen.n_items < 1 or seen.n_items >= 2 ** 31:
        raise ValueError(f"hard_unseen: n_items={seen.n_items} outside [1, 2^31)")
    _require_dtype("hard_unseen", torch.int64, (("user_ids", user_ids), ("out", out)))
    _require_dtype("hard_unseen", torch.float32, (("user_emb", user_emb), ("item_emb", item_emb)))
    if user_ids.dim() != 1:
        raise ValueError(f"hard_unseen: user_ids must be [T], got {tuple(user_ids.shape)}")
    T = int(user_ids.numel())
    if out is not None and (out.dim() != 1 or int(out.numel()) != T or not out.is_contiguous()):
        raise ValueError(f"hard_unseen: out must be a contiguous [T = {T}] tensor, got {tuple(out.shape)}")
    _require_matmul(user_emb, item_emb)
    if int(item_emb.shape[0]) < seen.n_items:
        raise ValueError(f"hard_unseen: item_emb has {int(item_emb.shape[0])} rows, the item sets index {seen.n_items} items")
    if int(user_emb.shape[0]) < seen.n_rows:
        raise ValueError(f"hard_unseen: user_emb has {int(user_emb.shape[0])} rows, the item sets {seen.n_rows}")
    if int(user_emb.shape[1]) < 1:
        raise ValueError("hard_unseen: the embeddings have no columns")
    _require_device(seen.rowptr, "the item sets")
    dev = seen.rowptr.device
    _check_sets(seen, dev, 0, "hard_unseen")
    if seen.rowptr.dtype != torch.int64 or seen.colidx.dtype != torch.int32:
        raise TypeError("hard_unseen: the item sets must be int64 row pointers and int32 columns")
    _f32c(user_emb, "user_emb"), _f32c(item_emb, "item_emb")
    _require_same_device("hard_unseen", (("user_emb", user_emb), ("item_emb", item_emb), ("user_ids", user_ids), ("out", out),
                                         ("status", status)), "the item sets", dev)
    status, check_status = _status_word("hard_unseen", status, dev)
    user_emb, item_emb = _unit_inner(user_emb.detach()), _unit_inner(item_emb.detach())
    user_ids = user_ids.contiguous()
    neg = torch.empty(T, dtype=torch.int64, device=dev) if out is None else out
    score = torch.empty(T, dtype=torch.float32, device=dev) if return_score else None
    slot = torch.empty(T, dtype=torch.int32, device=dev) if return_slot else None
    # a set without entries has no column array to point at; its row pointers are all 0 and nothing is read through it
    colidx = seen.colidx if seen.colidx.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_sample_hard_f32(
            _ptr(seen.rowptr), _ptr(colidx), seen.col_offset, seen.n_rows, seen.n_items, _ptr(user_emb),
            _row_major_ld(user_emb, "user_emb"), int(user_emb.shape[0]), _ptr(item_emb), _row_major_ld(item_emb, "item_emb"),
            int(item_emb.shape[0]), int(user_emb.shape[1]), _ptr(user_ids), T, int(case_offset), m, seed, _ptr(neg), _ptr(score),
            _ptr(slot), _ptr(status), _stream()))
    if check_status and T:
        bits = int(status.item())
        if bits & 1:
            raise IndexError(f"hard_unseen: a user id lies outside [0, {seen.n_rows})")
        if bits & 2:
            raise ValueError(f"hard_unseen: a user has fewer than m={m} unseen items among {seen.n_items}")
    if not (return_score or return_slot):
        return neg
    return (neg,) + ((score,) if return_score else ()) + ((slot,) if return_slot else ())
