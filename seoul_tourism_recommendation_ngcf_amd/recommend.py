"""Trip recommendation on the device: what the reference's interactive recommender does after its topk (demo.py:233-313, 315-334,
378-398), for any number of parties.

A request row is one party member on one day: a user id and, optionally, the five features.  The reference turns three orderings
of the catalogue per request row - by predicted preference, by congestion on the day, by distance from the departure point - into
rank points (first place 100, then 99, ...), blends them with the traveller's weights, sums over the rows of a view's column (per
member and day, per day, per member, overall), filters by genre and prints the best `rec_num` destinations of every column; it
does so in a pandas loop with some twenty data-frame re-indexings per request row.  Here: one ranking launch per chunk of rows
(engine.rank_topk), one top list per context table (engine.topk_rows), one blend launch (engine.blend_points) and one read-back.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import engine
from .evaluate import _as_sets


def demo_views(user_ids: torch.Tensor, age: torch.Tensor, sex: torch.Tensor, month: torch.Tensor, day: torch.Tensor):
    """The columns of the reference's four views over R request rows (demo.py:276-313), as one CSR for `blended_ranking`:
    `df_daily_user` (one column per user id - the reference's ids are one per member and day -, the view the reference runs,
    demo.py:205), `df_day` (per (month, day)), `df_user` (per (age, sex)) and `df_total` (all rows), in this order, each view's
    columns in ascending key order.  Returns (col_rowptr int64 [G + 1], col_rows int64 [4 R], labels): the CSR on the device of
    `user_ids`, rows ascending within a column; labels on the host, one per column: ("user", id), ("day", month, day),
    ("person", age, sex), ("all",).  Set-up code in torch ops (as ItemSets.from_pairs), not a hot path."""
    user_ids = user_ids.reshape(-1).to(torch.int64)
    dev = user_ids.device
    R = int(user_ids.numel())
    age, sex, month, day = (t.reshape(-1).to(device=dev, dtype=torch.int64) for t in (age, sex, month, day))
    for t in (age, sex, month, day):
        if int(t.numel()) != R:
            raise ValueError(f"demo_views: {R} user ids, {int(t.numel())} entries of a feature")
    views = (("user", user_ids[:, None]), ("day", torch.stack((month, day), 1)), ("person", torch.stack((age, sex), 1)),
             ("all", torch.zeros((R, 0), dtype=torch.int64, device=dev)))
    counts, rows, labels = [], [], []
    for name, keys in views:
        if R == 0:
            break
        if keys.shape[1] == 0:
            uniq, inv = keys[:1], torch.zeros(R, dtype=torch.int64, device=dev)
        else:
            uniq, inv = torch.unique(keys, dim=0, return_inverse=True)           # rows in ascending lexicographic order
        rows.append(torch.sort(inv, stable=True).indices)
        counts.append(torch.bincount(inv, minlength=int(uniq.shape[0])))
        labels += [(name, *k) for k in uniq.cpu().tolist()]
    rowptr = torch.zeros(len(labels) + 1, dtype=torch.int64, device=dev)
    if R:
        rowptr[1:] = torch.cumsum(torch.cat(counts), 0)
    col_rows = torch.cat(rows) if R else torch.zeros(0, dtype=torch.int64, device=dev)
    return rowptr, col_rows, labels


def _columns_csr(columns, user_ids: torch.Tensor):
    """(rowptr, rows, ids or None) of the `columns` argument of `blended_ranking`."""
    dev, R = user_ids.device, int(user_ids.numel())
    ids = None
    if columns is None:
        ids, number = torch.unique(user_ids, return_inverse=True)               # ascending ids
        G = int(ids.numel())
    elif isinstance(columns, (tuple, list)):
        if len(columns) != 2:
            raise ValueError("blended_ranking: columns = (rowptr, rows)")
        return (columns[0].to(device=dev, dtype=torch.int64), columns[1].to(device=dev, dtype=torch.int64), None)
    else:
        number = columns.reshape(-1).to(device=dev, dtype=torch.int64)
        if int(number.numel()) != R:
            raise ValueError(f"blended_ranking: {int(number.numel())} column numbers for {R} request rows")
        if R and int(number.min()) < 0:
            raise IndexError("blended_ranking: a negative column number")
        G = int(number.max()) + 1 if R else 0
    rowptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    if R:
        rowptr[1:] = torch.cumsum(torch.bincount(number, minlength=G), 0)
    return rowptr, torch.sort(number, stable=True).indices, ids


def _context_lists(values, slot, R: int, Pl: int, n_item: int, dev, what: str):
    """The ascending top lists of a context table (values [S, n_item] fp32, smallest first) and its slot vector [R]."""
    if values is None:
        if slot is not None:
            raise ValueError(f"blended_ranking: {what}_slot without {what}")
        return None, None
    if slot is None:
        raise ValueError(f"blended_ranking: {what} needs {what}_slot, the table row of every request row")
    values = values.to(device=dev, dtype=torch.float32)
    if values.dim() != 2 or int(values.shape[1]) != n_item:
        raise ValueError(f"blended_ranking: {what} must be [S, n_item = {n_item}], got {tuple(values.shape)}")
    slot = slot.reshape(-1).to(device=dev, dtype=torch.int64)
    if int(slot.numel()) != R:
        raise ValueError(f"blended_ranking: {int(slot.numel())} {what} slots for {R} request rows")
    _, lists = engine.topk_rows(-values, Pl)
    return lists, slot


def blended_ranking(model, user_ids: torch.Tensor, *, features=None, year=None, columns=None,
                    weights: Sequence[float] = (1.0, 0.0, 0.0), congestion: Optional[torch.Tensor] = None,
                    congestion_slot: Optional[torch.Tensor] = None, distance: Optional[torch.Tensor] = None,
                    distance_slot: Optional[torch.Tensor] = None, item_mask: Optional[torch.Tensor] = None, top: int = 10,
                    points: int = 100, exclude=None, row_chunk: int = 65536, return_table: bool = False):
    """The recommendation lists of demo.py for R request rows (`user_ids` [R]; one member on one day each) in G columns.

    Per request row three lists of Pl = min(points, n_item) items: its best items by predicted preference (`engine.rank_topk` on
    the propagated tables: score descending, ties lowest item first, the items of `exclude` left out), the items of least
    congestion of its day and the nearest items of its departure point (`engine.topk_rows` on the negated tables: value ascending,
    ties lowest item first; +inf = missing, sorts last; a NaN sorts FIRST, as topk_rows documents for the negated value).  The
    item at position j of a list gets `points` - j points of that kind, every other item none: with n_item == points (the
    reference: 100 destinations, rank2rate = [100 .. 1]) every item gets points and this is demo.py:287-292 exactly; for larger
    catalogues it is the extension that needs no score matrix.  Per column g and item i the three kinds are summed over the
    column's rows (int32, exact), rating[g, i] = (sp * w_pref + sc * w_con) + sd * w_dis in fp64 without FMA - numpy's bits,
    independent of any order - and the column's list is its `top` items with item_mask[i] != 0 (the genre filter, demo.py:315-334),
    rating descending, ties lowest item first; slots past the eligible items are (-1, -inf).

      features    (age, sex, month, day, dow), one entry per request row, or None: no injection (NGCF.py:103-115; one
                  `engine.feature_inject` call for all rows, as `evaluate.candidate_ranking`).
      year        None (Laplacian slice 0) or one year: slice `model._year_index` of it (the demo passes [0]).
      columns     None: one column per distinct user id in ascending id order (`df_daily_user`, the reference's live view), the ids
                  are returned too; an int64 [R] vector of column numbers; or a (rowptr, rows) CSR, e.g. `demo_views`' - a row
                  may be in several columns, once in each.
      weights     (w_pref, w_con, w_dis): vis_rat, con_rat, dis_rat of the demo.
      congestion  float32 [S, n_item], one row per distinct day, with congestion_slot int64 [R], the table row of every request
                  row; distance / distance_slot likewise, one row per departure point.  None: no points of that kind.
      item_mask   uint8 / bool [n_item] or None.
      points      at most 256 (engine.RANK_K_MAX: the preference lists are rank_topk lists).
      exclude     engine.ItemSets or (users, items) pairs left out of the preference lists, or None.
      row_chunk   request rows per ranking launch.

    Returns (items int64 [G, top], rating float64 [G, top]) on the device; with columns=None (items, rating, ids [G]); with
    `return_table` the dense float64 [G, n_item] ratings are appended (small catalogues and tests).  The model runs in eval mode
    under no_grad; the caller's mode is restored.  The host reads back once, at the end: an id out of range (user, feature, slot,
    column row) raises IndexError then.

    Out of scope: the median filter of the reference's views 1, 2 and 4 (demo.py:341, 359, 408; unreachable there, rec_type is
    hard-coded to '3') and the quantile-0 filter of view 3 (always true).

    One deviation from the reference.  It adds points * weight into the rating row by row in fp64 (`rating += ...`, three times per
    request row); here the integer sums come first, then three products.  With weights that are exact in binary (0.5 / 0.25 /
    0.25) the two are equal; otherwise they differ by rounding only, at most 3 * rows_in_column * 2^-52 relative for non-negative
    weights (every term is then non-negative)."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            dev = model._dev()
            user_ids = user_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
            R = int(user_ids.numel())
            if len(weights) != 3:
                raise ValueError("blended_ranking: weights = (w_pref, w_con, w_dis)")
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            if features is not None:                                   # NGCF.py:103-115, all rows at once
                if len(features) != 5:
                    raise ValueError("blended_ranking: features = (age, sex, month, day, dow)")
                keep = engine.feature_inject(
                    model.user_embedding.weight.data,
                    (model.age_emb.weight.data, model.sex_emb.weight.data, model.month_emb.weight.data,
                     model.day_emb.weight.data, model.dow_emb.weight.data),
                    features, user_ids, model.emb_ratio, model._scratch_buf(dev), status)
                model._e0_cache.touch(user_ids)
                del keep
            year_h = None if year is None else torch.as_tensor(year).reshape(-1).cpu()
            if year_h is not None and int(year_h.numel()) != 1:
                raise ValueError("blended_ranking: year is a single value")
            model.propagate(0 if year_h is None else model._year_index(year_h))
            U, I = model.all_users_emb, model.all_items_emb
            n_user, n_item = int(U.shape[0]), int(I.shape[0])
            Pl = min(int(points), n_item)
            excl = None if exclude is None else _as_sets(exclude, n_user, n_item, dev)
            rowptr, rows, ids = _columns_csr(columns, user_ids)
            con, con_slot = _context_lists(congestion, congestion_slot, R, Pl, n_item, dev, "congestion")
            dis, dis_slot = _context_lists(distance, distance_slot, R, Pl, n_item, dev, "distance")
            if item_mask is not None:
                item_mask = item_mask.to(dev)
            pref = None
            for c0 in range(0, R, int(row_chunk)):
                _, idx = engine.rank_topk(U, I, Pl, user_ids=user_ids[c0:c0 + int(row_chunk)], exclude=excl, status=status)
                if R <= int(row_chunk):
                    pref = idx
                else:
                    if pref is None:
                        pref = torch.empty((R, Pl), dtype=torch.int64, device=dev)
                    pref[c0:c0 + int(row_chunk)] = idx
            if pref is None:
                pref = torch.empty((0, Pl), dtype=torch.int64, device=dev)
            out = engine.blend_points(pref, rowptr, rows, n_item, points=int(points), weights=weights, con=con, con_slot=con_slot,
                                      dis=dis, dis_slot=dis_slot, item_mask=item_mask, top=int(top), return_table=return_table,
                                      status=status)
            if int(status.item()) != 0:                                # the one read-back
                raise IndexError("blended_ranking: a user id, a feature id, a context slot or a column's row index is out of range")
            if ids is not None:
                out = out[:2] + (ids,) + out[2:]
            return out
    finally:
        model.train(was_training)
