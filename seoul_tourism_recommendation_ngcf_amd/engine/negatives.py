"""The draws of unseen items on the device, one module for the family.  Uniform (`ngcf_sample_unseen`:
csrc/sample.hip): `m` items per case the case's user has no entry for, without replacement - `engine.sample_unseen`, re-exported by
`engine.selection`.  Hard negatives (`ngcf_sample_hard_f32`: csrc/sample_hard.hip): of `m` such draws per case, the one the current
embeddings score highest - `sample_unseen`, `eval_candidates`' scores and an argmax in one launch, with one item per case written to
memory.  Popularity-weighted negatives (`ngcf_weighted_prepare`, `ngcf_sample_weighted`: csrc/sample_weighted.hip): `m` distinct
unseen items per case in proportion to an integer weight per item, with the weights and the unseen mass from which the proposal
probability follows exactly."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._plumbing import (_f32c, _on, _ptr, _require_device, _require_dtype, _require_matmul, _require_same_device, _row_major_ld,
                        _status_word, _stream, _unit_inner)
from .ranking import ItemSets, _check_sets


# ---- what the three draws share: one front (limits and types, which hold on any device, before where the sets live), the stand-in
# for an empty column array, and one back (the status bits) -----------------------------------------------------------------------------
def _check_draw(fn: str, seen: ItemSets, user_ids: torch.Tensor, m: int, m_max: int, int64s=(), float32s=()) -> int:
    """The checks every draw starts with, which hold on any device: the range of `m` and of the catalogue, the types of `user_ids`
    and of the wrapper's other tensors (`int64s`, `float32s`: (name, tensor or None) pairs), `user_ids` [T].  Returns T."""
    if m < 1 or m > m_max:
        raise ValueError(f"{fn}: m={m} outside [1, {m_max}]")
    if seen.n_items < 1 or seen.n_items >= 2 ** 31:
        raise ValueError(f"{fn}: n_items={seen.n_items} outside [1, 2^31)")
    _require_dtype(fn, torch.int64, (("user_ids", user_ids),) + tuple(int64s))
    _require_dtype(fn, torch.float32, float32s)
    if user_ids.dim() != 1:
        raise ValueError(f"{fn}: user_ids must be [T], got {tuple(user_ids.shape)}")
    return int(user_ids.numel())


def _sets_device(fn: str, seen: ItemSets):
    """The ROCm device the item sets live on, in the layout the kernels read: int64 row pointers, int32 columns."""
    _require_device(seen.rowptr, "the item sets")
    dev = seen.rowptr.device
    _check_sets(seen, dev, 0, fn)
    if seen.rowptr.dtype != torch.int64 or seen.colidx.dtype != torch.int32:
        raise TypeError(f"{fn}: the item sets must be int64 row pointers and int32 columns")
    return dev


def _colidx(seen: ItemSets) -> torch.Tensor:
    """The sets' column array for the library.  A set without entries has none to point at: its row pointers are all 0 and nothing
    is read through the one-element stand-in."""
    return seen.colidx if seen.colidx.numel() else torch.zeros(1, dtype=torch.int32, device=seen.rowptr.device)


def _raise_status(fn: str, status: torch.Tensor, seen: ItemSets, m: int, unseen: str = "unseen items"):
    """The one read-back of a draw's own status word: bit 1 a user id outside the sets, bit 2 a user with too few `unseen`."""
    bits = int(status.item())
    if bits & 1:
        raise IndexError(f"{fn}: a user id lies outside [0, {seen.n_rows})")
    if bits & 2:
        raise ValueError(f"{fn}: a user has fewer than m={m} {unseen} among {seen.n_items}")


# ---- unseen items per case, the reference's TourDataset._negative_sampling (ngcf_sample_unseen, csrc/sample.hip) -------------------
SAMPLE_M_MAX = 1023


def sample_unseen(seen: ItemSets, user_ids: torch.Tensor, m: int, seed: int, *, first: Optional[torch.Tensor] = None,
                  case_offset: int = 0, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`m` items per case that the case's user has no entry for in `seen`, uniform and without replacement (ngcf_sample_unseen):
    case t of user `user_ids[t]` (int64 [T] on the sets' device) is a pure function of (seed, case_offset + t, the user's seen row)
    - the draw is written out in include/ngcf_hip.h, so a case set drawn in chunks with `case_offset` equals the set drawn at
    once.  This is the distribution of the reference's `np.random.choice(neg_items, ng_ratio, replace=False)` (utils.py:262), not
    numpy's stream: the same seed does not give the reference's items.  Returns int64 [T, m], or [T, m + 1] with `first` (int64 [T],
    e.g. the held-out items) in column 0 - then the `candidates` of `eval_candidates`.  `out`: an int64 row-major tensor of T rows
    and at least that many columns to write into (the returned tensor is a view of its leading columns).  `seen` comes from
    `ItemSets.from_pairs` or `ItemSets.from_laplacian`.  A user id outside the sets raises IndexError, a user with fewer than `m`
    unseen items ValueError (np.random.choice raises there), after one host sync; the drawn slots of such a case are -1.  With a
    caller's int32 `status` word the bits (1, 2) are only OR-ed into it and the call neither syncs nor raises."""
    lib = _lib.load()
    m, seed = int(m), int(seed) & 0xFFFFFFFFFFFFFFFF
    T = _check_draw("sample_unseen", seen, user_ids, m, SAMPLE_M_MAX, (("first", first), ("out", out)))
    if first is not None and (first.dim() != 1 or int(first.numel()) != T):
        raise ValueError(f"sample_unseen: first must be [T = {T}], got {tuple(first.shape)}")
    width = m + (first is not None)
    if out is not None and (out.dim() != 2 or int(out.shape[0]) != T or int(out.shape[1]) < width):
        raise ValueError(f"sample_unseen: out must be [T = {T}, >= {width}], got {tuple(out.shape)}")
    dev = _sets_device("sample_unseen", seen)
    _require_same_device("sample_unseen", (("user_ids", user_ids), ("first", first), ("out", out), ("status", status)),
                         "the item sets", dev)
    status, check_status = _status_word("sample_unseen", status, dev)
    user_ids = user_ids.contiguous()
    first = None if first is None else first.contiguous()
    if out is None:
        out = torch.empty((T, width), dtype=torch.int64, device=dev)
    ld_out = _row_major_ld(out, "out")
    with _on(dev):
        _lib.check(lib.ngcf_sample_unseen(_ptr(seen.rowptr), _ptr(_colidx(seen)), seen.col_offset, seen.n_rows, seen.n_items,
                                          _ptr(user_ids), T, int(case_offset), m, seed, _ptr(first), _ptr(out), ld_out, _ptr(status),
                                          _stream()))
    if check_status and T:
        _raise_status("sample_unseen", status, seen, m)
    return out[:, :width]


# ---- hard negatives (ngcf_sample_hard_f32, csrc/sample_hard.hip) ----------------------------------------------------------------------
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
    m, seed = int(m), int(seed) & 0xFFFFFFFFFFFFFFFF
    T = _check_draw("hard_unseen", seen, user_ids, m, HARD_M_MAX, (("out", out),), (("user_emb", user_emb), ("item_emb", item_emb)))
    if out is not None and (out.dim() != 1 or int(out.numel()) != T or not out.is_contiguous()):
        raise ValueError(f"hard_unseen: out must be a contiguous [T = {T}] tensor, got {tuple(out.shape)}")
    _require_matmul(user_emb, item_emb)
    if int(item_emb.shape[0]) < seen.n_items:
        raise ValueError(f"hard_unseen: item_emb has {int(item_emb.shape[0])} rows, the item sets index {seen.n_items} items")
    if int(user_emb.shape[0]) < seen.n_rows:
        raise ValueError(f"hard_unseen: user_emb has {int(user_emb.shape[0])} rows, the item sets {seen.n_rows}")
    if int(user_emb.shape[1]) < 1:
        raise ValueError("hard_unseen: the embeddings have no columns")
    dev = _sets_device("hard_unseen", seen)
    _f32c(user_emb, "user_emb"), _f32c(item_emb, "item_emb")
    _require_same_device("hard_unseen", (("user_emb", user_emb), ("item_emb", item_emb), ("user_ids", user_ids), ("out", out),
                                         ("status", status)), "the item sets", dev)
    status, check_status = _status_word("hard_unseen", status, dev)
    user_emb, item_emb = _unit_inner(user_emb.detach()), _unit_inner(item_emb.detach())
    user_ids = user_ids.contiguous()
    neg = torch.empty(T, dtype=torch.int64, device=dev) if out is None else out
    score = torch.empty(T, dtype=torch.float32, device=dev) if return_score else None
    slot = torch.empty(T, dtype=torch.int32, device=dev) if return_slot else None
    with _on(dev):
        _lib.check(lib.ngcf_sample_hard_f32(
            _ptr(seen.rowptr), _ptr(_colidx(seen)), seen.col_offset, seen.n_rows, seen.n_items, _ptr(user_emb),
            _row_major_ld(user_emb, "user_emb"), int(user_emb.shape[0]), _ptr(item_emb), _row_major_ld(item_emb, "item_emb"),
            int(item_emb.shape[0]), int(user_emb.shape[1]), _ptr(user_ids), T, int(case_offset), m, seed, _ptr(neg), _ptr(score),
            _ptr(slot), _ptr(status), _stream()))
    if check_status and T:
        _raise_status("hard_unseen", status, seen, m)
    if not (return_score or return_slot):
        return neg
    return (neg,) + ((score,) if return_score else ()) + ((slot,) if return_slot else ())


# ---- popularity-weighted negatives (ngcf_weighted_prepare, ngcf_sample_weighted: csrc/sample_weighted.hip) ----------------------------
WEIGHTED_M_MAX = 64                              # NGCF_SAMPLE_WEIGHTED_M_MAX: lane j of a case's wave keeps drawn interval j
WEIGHT_MAX = 2 ** 40                             # the largest weight of one item
WEIGHT_TOTAL_MAX = 2 ** 62                       # the sum of all weights lies below it


class WeightedSets:
    """Seen sets with an integer weight per item, prepared for `weighted_unseen`: `cdf` int64 [n_items + 1] (the weight below every
    item, `torch.cumsum` - exact in int64), `gap` int64 (one per stored entry of `seen`: the unseen weight below that entry) and
    `mass` int64 [n_rows] (every user's unseen weight), the last two by ngcf_weighted_prepare.  `weights`: int64 [seen.n_items] on
    the sets' device, every value in [0, 2^40].  One read-back, of the total W with the weights' range, refuses W = 0, W >= 2^62
    and a weight that is negative or above 2^40 with ValueError.  Prepare once per (seen sets, weights); the draws only read it."""

    def __init__(self, seen: ItemSets, weights: torch.Tensor):
        lib = _lib.load()
        _require_dtype("WeightedSets", torch.int64, (("weights", weights),))
        if weights.dim() != 1 or int(weights.numel()) != seen.n_items:
            raise ValueError(f"WeightedSets: weights must be [n_items = {seen.n_items}], got {tuple(weights.shape)}")
        if seen.n_items < 1 or seen.n_items >= 2 ** 31:
            raise ValueError(f"WeightedSets: n_items={seen.n_items} outside [1, 2^31)")
        dev = _sets_device("WeightedSets", seen)
        _require_same_device("WeightedSets", (("weights", weights),), "the item sets", dev)
        self.seen = seen
        self.cdf = torch.zeros(seen.n_items + 1, dtype=torch.int64, device=dev)
        torch.cumsum(weights, 0, out=self.cdf[1:])
        self.gap = torch.empty(max(int(seen.colidx.numel()), 1), dtype=torch.int64, device=dev)
        self.mass = torch.empty(max(seen.n_rows, 1), dtype=torch.int64, device=dev)
        self._colidx = _colidx(seen)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        with _on(dev):
            # the kernel reads nothing through a value of cdf, so it may run before the weights' range is known
            _lib.check(lib.ngcf_weighted_prepare(_ptr(seen.rowptr), _ptr(self._colidx), seen.col_offset, seen.n_rows, seen.n_items,
                                                 _ptr(self.cdf), _ptr(self.gap), _ptr(self.mass), _ptr(status), _stream()))
        # the int64 sum wraps from 2^63 on: an fp64 sum, capped at 2^62, tells a wrapped total from a small one
        coarse = weights.sum(dtype=torch.float64).clamp(max=float(WEIGHT_TOTAL_MAX)).to(torch.int64)
        total, coarse, lowest, highest, bits = torch.stack((self.cdf[-1], coarse, weights.min(), weights.max(),
                                                            status[0].to(torch.int64))).tolist()
        if lowest < 0 or highest > WEIGHT_MAX:
            raise ValueError(f"WeightedSets: the weights span [{lowest}, {highest}], outside [0, 2^40]")
        if total < 1 or total >= WEIGHT_TOTAL_MAX or coarse >= WEIGHT_TOTAL_MAX:
            raise ValueError(f"WeightedSets: the weights sum to {total}, outside [1, 2^62)")
        if bits:
            raise IndexError(f"WeightedSets: a stored item id of the seen sets lies outside [0, {seen.n_items})")
        self.total = int(total)

    @property
    def n_rows(self) -> int:
        return self.seen.n_rows

    @property
    def n_items(self) -> int:
        return self.seen.n_items


def weighted_unseen(wsets: WeightedSets, user_ids: torch.Tensor, m: int, seed: int, *, case_offset: int = 0,
                    return_weights: bool = False, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """`m` distinct items per case that the case's user has no entry for in `wsets.seen`, drawn in proportion to the items' weights
    (ngcf_sample_weighted): slot 0 is item i with probability w_i / U over the user's unseen items (U: their weight, `wsets.mass`),
    slot j with probability w_i / U_j over those not drawn yet, U_j = U - (the weights of slots 0 .. j-1) - successive sampling, the
    law of `np.random.choice(p=w / w.sum(), replace=False)`, not numpy's stream; an item of weight 0 is never drawn.  Case t of
    user `user_ids[t]` (int64 [T] on the sets' device) is a pure function of (seed, case_offset + t, the user's seen row, the
    weights), written out in include/ngcf_hip.h: a case set drawn in chunks with `case_offset` equals the set drawn at once, and
    column 0 of a draw of m items is the draw of one.  With all weights 1 the law is `sample_unseen`'s uniform one, the items are
    not.  `m` in [1, 64].  Returns int64 [T, m] - with `return_weights` a tuple (items, draw_weight int64 [T, m], case_mass int64
    [T]): the weight of every drawn item and U, so slot j's proposal probability is exactly
    draw_weight[t, j] / (case_mass[t] - draw_weight[t, :j].sum()).  `out`: an int64 row-major tensor of T rows and at least m columns
    to write the items into (the returned tensor is a view of its leading columns).  A user id outside the sets raises IndexError,
    a user with fewer than `m` positive-weight unseen items ValueError, after one host sync; every slot of such a case is -1 and
    its weights 0.  With a caller's int32 `status` word the bits (1, 2) are only OR-ed into it and the call neither syncs nor
    raises."""
    m, seed = int(m), int(seed) & 0xFFFFFFFFFFFFFFFF
    if not isinstance(wsets, WeightedSets):
        raise TypeError(f"weighted_unseen: wsets must be a WeightedSets, got {type(wsets).__name__}")
    seen = wsets.seen
    T = _check_draw("weighted_unseen", seen, user_ids, m, WEIGHTED_M_MAX, (("out", out),))
    if out is not None and (out.dim() != 2 or int(out.shape[0]) != T or int(out.shape[1]) < m):
        raise ValueError(f"weighted_unseen: out must be [T = {T}, >= {m}], got {tuple(out.shape)}")
    lib = _lib.load()
    dev = wsets.cdf.device
    _require_device(wsets.cdf, "the weighted sets")
    _require_same_device("weighted_unseen", (("user_ids", user_ids), ("out", out), ("status", status)), "the weighted sets", dev)
    status, check_status = _status_word("weighted_unseen", status, dev)
    user_ids = user_ids.contiguous()
    if out is None:
        out = torch.empty((T, m), dtype=torch.int64, device=dev)
    draw_weight = torch.empty((T, m), dtype=torch.int64, device=dev) if return_weights else None
    case_mass = torch.empty(T, dtype=torch.int64, device=dev) if return_weights else None
    with _on(dev):
        _lib.check(lib.ngcf_sample_weighted(_ptr(seen.rowptr), _ptr(wsets._colidx), seen.col_offset, seen.n_rows, seen.n_items,
                                            _ptr(wsets.cdf), _ptr(wsets.gap), _ptr(wsets.mass), _ptr(user_ids), T, int(case_offset),
                                            m, seed, _ptr(out), _row_major_ld(out, "out"), _ptr(draw_weight), m, _ptr(case_mass),
                                            _ptr(status), _stream()))
    if check_status and T:
        _raise_status("weighted_unseen", status, seen, m, "unseen items of positive weight")
    return (out[:, :m], draw_weight, case_mass) if return_weights else out[:, :m]
