"""Certified two-stage ranking (csrc/rank_prefilter.hip; the header's section "certified two-stage ranking"): a bf16 MFMA shortlist
per user by an upper bound of the exact score, an exact fp32 re-score of the shortlist with `rank_topk`'s chain, and a per-user
certificate that the shortlist's top-k is the catalogue's.  `rank_topk_certified` returns `engine.rank_topk`'s values and indices
bit for bit: the rows whose certificate fails are ranked again by `rank_topk`."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

from .. import _lib
from ._plumbing import _f32c, _on, _ptr, _require_device, _require_matmul, _row_major_ld, _status_word, _stream, _unit_inner
from .ranking import RANK_K_MAX, ItemSets, _check_sets, rank_topk

POOL_MAX = 256          # NGCF_RANK_POOL_MAX
D_MAX = 4096            # NGCF_RANK_PREFILTER_DMAX
K_STEP = 16             # NGCF_RANK_PREFILTER_KSTEP: the packed rows are padded to it

PackedItems = namedtuple("PackedItems", "bf16 norm_up flags n_items D")


def beta(D: int) -> float:
    """The bound's constant: |s - s~| <= beta |u| |i| with room for the bound's own rounding (exact in float64)."""
    return 2.0 ** -7 + 2.0 ** -16 + (4 * int(D) + 2) * 2.0 ** -24


def default_pool(k: int) -> int:
    """128 for k <= 32, else 256 (a placeholder until tools/rank_prefilter_lab.py has settled it on the hardware)."""
    return 128 if int(k) <= 32 else 256


def _check_width(fn: str, D: int):
    if D > D_MAX:
        raise RuntimeError(f"{fn}: D={D} > {D_MAX} is not supported; rank_topk takes any D")


def _require_f32(fn: str, user_emb, item_emb):
    for nm, x in (("user_emb", user_emb), ("item_emb", item_emb)):
        if x is not None and x.dtype != torch.float32:
            raise RuntimeError(f"{fn}: {nm}: expected float32, got {x.dtype}")


def pack_items(item_emb: torch.Tensor) -> PackedItems:
    """The item table as the shortlist kernel reads it (ngcf_rank_pack_items): `.bf16` [n_items, Dp] (round to nearest even, D
    padded with zeros to a multiple of 16), `.norm_up` float32 [n_items] (every row's Euclidean norm rounded up), `.flags` int32
    [1] (1 iff an item is irregular: then no user is certified), `.n_items`, `.D`.  Reusable while the table is unchanged."""
    _require_f32("pack_items", None, item_emb)
    if item_emb.dim() != 2 or item_emb.shape[0] < 1 or item_emb.shape[1] < 1:
        raise RuntimeError(f"pack_items: expected a 2-D item table, got {tuple(item_emb.shape)}")
    n_items, D = int(item_emb.shape[0]), int(item_emb.shape[1])
    _check_width("pack_items", D)
    _require_device(item_emb, "item_emb")
    lib = _lib.load()
    item_emb = _unit_inner(item_emb)
    dev = item_emb.device
    Dp = (D + K_STEP - 1) // K_STEP * K_STEP
    image = torch.empty((n_items, Dp), dtype=torch.bfloat16, device=dev)
    norm_up = torch.empty((n_items,), dtype=torch.float32, device=dev)
    flags = torch.empty((1,), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_rank_pack_items(_ptr(item_emb), _row_major_ld(item_emb, "item_emb"), n_items, D, _ptr(image), _ptr(norm_up),
                                            _ptr(flags), _stream()))
    return PackedItems(image, norm_up, flags, n_items, D)


def _shortlist(lib, user_emb, ldu, user_ids, n_rows, B, packed, pool, exclude, status, debug):
    """ngcf_rank_shortlist_bf16 on checked arguments: (pool_idx int32 [B, pool], pool_thr float32 [B], user_flags int32 [B])."""
    dev = user_emb.device
    nb = int(lib.ngcf_rank_prefilter_workspace_bytes(B, packed.n_items, packed.D, pool))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    pool_idx = torch.empty((B, pool), dtype=torch.int32, device=dev)
    pool_thr = torch.empty((B,), dtype=torch.float32, device=dev)
    user_flags = torch.empty((B,), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_rank_shortlist_bf16(_ptr(user_emb), ldu, _ptr(user_ids), n_rows, B, _ptr(packed.bf16), _ptr(packed.norm_up),
                                                packed.n_items, packed.D, pool, _ptr(None if exclude is None else exclude.rowptr),
                                                _ptr(None if exclude is None else exclude.colidx),
                                                0 if exclude is None else exclude.col_offset, _ptr(pool_idx), _ptr(pool_thr),
                                                _ptr(user_flags), _ptr(debug), _ptr(status), _ptr(ws), nb, _stream()))
    return pool_idx, pool_thr, user_flags


def shortlist_scores(user_emb: torch.Tensor, item_emb: torch.Tensor, packed: Optional[PackedItems] = None):
    """What the shortlist kernel computes for every (user row, item) pair, as dense [B, n_items] float32 matrices (tests and the lab;
    small tables only): (s~, the bf16 MFMA score; ub = fmaf(bu, ni, s~), its key before the monotone map)."""
    lib = _lib.load()
    _f32c(user_emb, "user_emb"), _f32c(item_emb, "item_emb")
    _require_matmul(user_emb, item_emb)
    _check_width("shortlist_scores", int(user_emb.shape[1]))
    user_emb, item_emb = _unit_inner(user_emb), _unit_inner(item_emb)
    packed = pack_items(item_emb) if packed is None else packed
    B, dev = int(user_emb.shape[0]), user_emb.device
    debug = torch.zeros((2, B, packed.n_items), dtype=torch.float32, device=dev)
    if B:
        _shortlist(lib, user_emb, _row_major_ld(user_emb, "user_emb"), None, B, B, packed, 1, None,
                   torch.zeros(1, dtype=torch.int32, device=dev), debug)
    return debug[0], debug[1]


def rank_topk_certified(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, user_ids: Optional[torch.Tensor] = None,
                        exclude: Optional[ItemSets] = None, status: Optional[torch.Tensor] = None, *,
                        packed: Optional[PackedItems] = None, pool: Optional[int] = None, fallback: bool = True,
                        return_certified: bool = False):
    """`engine.rank_topk(user_emb, item_emb, k, user_ids, exclude, status)` - the same checks, refusals and result, bit for bit - by
    way of a shortlist: bf16 MFMA scores of every pair become upper bounds of the exact scores, the `pool` items with the largest
    bounds are re-scored with `rank_topk`'s chain, and a row is certified when no item outside its pool can reach its k-th score.
    `pool` lies in [k, 256] (default: `default_pool(k)`); `packed` is `pack_items(item_emb)` (packed here when None).
    With `fallback=True` the uncertified rows are ranked again by `engine.rank_topk(user_ids=those rows)` and patched in: that costs
    ONE read-back per call (the count of those rows).  `fallback=False` reads nothing back: it returns the pools' own answer, which
    equals `rank_topk`'s on the certified rows only (tests and the lab).  With `return_certified` the bool mask [B] comes third.
    A user id outside the table raises IndexError (one host sync); with a caller's int32 `status` it is only flagged there, and it
    is never used as an index.  D <= 4096."""
    # shapes, types and limits first (they hold on any device), then where the tensors live
    _require_f32("rank_topk_certified", user_emb, item_emb)
    _require_matmul(user_emb, item_emb)
    n_rows, D, n_items = int(user_emb.shape[0]), int(user_emb.shape[1]), int(item_emb.shape[0])
    k = int(k)
    if k < 1 or k > n_items:
        raise RuntimeError(f"selected index k out of range (k={k}, row length {n_items})")
    if k > RANK_K_MAX:
        raise RuntimeError(f"rank_topk: k={k} > {RANK_K_MAX} is not supported; recommend_topk takes k up to 1024")
    pool = default_pool(k) if pool is None else int(pool)
    if pool < k or pool > POOL_MAX:
        raise ValueError(f"rank_topk_certified: pool={pool} outside [k = {k}, {POOL_MAX}]")
    _check_width("rank_topk_certified", D)
    if packed is not None and (packed.n_items != n_items or packed.D != D or packed.bf16.device != item_emb.device):
        raise ValueError(f"rank_topk_certified: `packed` holds {packed.n_items} x {packed.D} items on {packed.bf16.device}, the item "
                         f"table is {n_items} x {D} on {item_emb.device}")
    _require_device(user_emb, "user_emb"), _require_device(item_emb, "item_emb")
    lib = _lib.load()
    dev = user_emb.device
    user_emb, item_emb = _unit_inner(user_emb), _unit_inner(item_emb)
    if user_ids is not None:
        user_ids = user_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        B = int(user_ids.numel())
    else:
        B = n_rows
    if exclude is not None:
        _check_sets(exclude, dev, n_rows, "rank_topk")
        if exclude.n_items != n_items:
            raise RuntimeError(f"rank_topk: the exclusion sets index {exclude.n_items} items, the item table has {n_items}")
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    idx = torch.empty((B, k), dtype=torch.int64, device=dev)
    cert = torch.zeros((B,), dtype=torch.uint8, device=dev)
    if B == 0:
        return (vals, idx, cert.bool()) if return_certified else (vals, idx)
    if packed is None:
        packed = pack_items(item_emb)
    status, check_status = _status_word("rank_topk_certified", status, dev)
    ldu, ldi = _row_major_ld(user_emb, "user_emb"), _row_major_ld(item_emb, "item_emb")
    pool_idx, pool_thr, user_flags = _shortlist(lib, user_emb, ldu, user_ids, n_rows, B, packed, pool, exclude, status, None)
    with _on(dev):
        _lib.check(lib.ngcf_rank_rescore(_ptr(user_emb), ldu, _ptr(user_ids), n_rows, B, _ptr(item_emb), ldi, n_items, D, k, pool,
                                         _ptr(pool_idx), _ptr(pool_thr), _ptr(user_flags), _ptr(packed.flags), _ptr(vals), _ptr(idx),
                                         _ptr(cert), _stream()))
    cert = cert.bool()
    if fallback:
        rows = (~cert).nonzero().flatten()                           # the call's one read-back: how many rows failed
        if rows.numel():
            ids = rows if user_ids is None else user_ids[rows]
            v2, i2 = rank_topk(user_emb, item_emb, k, user_ids=ids, exclude=exclude, status=status)
            vals[rows], idx[rows] = v2, i2
    if check_status and user_ids is not None and int(status.item()) != 0:
        raise IndexError(f"rank_topk: a user id lies outside [0, {n_rows})")
    return (vals, idx, cert) if return_certified else (vals, idx)
