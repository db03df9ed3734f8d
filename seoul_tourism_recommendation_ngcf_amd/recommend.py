"""Trip recommendation on the device: what the reference's interactive recommender does after its topk (demo.py:233-313, 315-334,
378-398), for any number of parties.

A request row is one party member on one day: a user id and, optionally, the five features.  The reference turns three orderings
of the catalogue per request row - by predicted preference, by congestion on the day, by distance from the departure point - into
rank points (first place 100, then 99, ...), blends them with the traveller's weights, sums over the rows of a view's column (per
member and day, per day, per member, overall), filters by genre and prints the best `rec_num` destinations of every column; it
does so in a pandas loop with some twenty data-frame re-indexings per request row.  Here: one ranking launch per chunk of rows
(engine.rank_topk), one top list per context table (engine.topk_rows), one blend launch (engine.blend_points) and one read-back.

What the reference does between loading its pickles and that loop is here too, from raw rows: `congestion_table` (the pivot of
demo.py:96-103 and the per-day slice of demo.py:270-274), `distance_table` (the haversine loop of demo.py:241-248), `party_rows`
(the party unrolled into request rows, demo.py:134-181), `context_slots` (the table row of every request row) and `order_table`
(fp64 tables as dense ranks, so that the cast to fp32 inside `blended_ranking` keeps the fp64 order and its ties).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import engine, serving


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
                  `NGCF._inject_features` call for all rows).
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
    with serving.inference(model):
        dev = model._dev()
        user_ids = user_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        R = int(user_ids.numel())
        if len(weights) != 3:
            raise ValueError("blended_ranking: weights = (w_pref, w_con, w_dis)")
        status = serving.status_word(dev)
        if features is not None:                                       # NGCF.py:103-115, all rows at once
            if len(features) != 5:
                raise ValueError("blended_ranking: features = (age, sex, month, day, dow)")
            model._inject_features(features, user_ids, status)         # (its keep-alive is dropped here, as before)
        y, _ = serving.year_slice(model, year)
        if y is None:
            raise ValueError("blended_ranking: year is a single value")
        t = serving.propagated(model, y)
        Pl = min(int(points), t.n_item)
        excl = None if exclude is None else serving.as_sets(exclude, t)
        rowptr, rows, ids = _columns_csr(columns, user_ids)
        con, con_slot = _context_lists(congestion, congestion_slot, R, Pl, t.n_item, dev, "congestion")
        dis, dis_slot = _context_lists(distance, distance_slot, R, Pl, t.n_item, dev, "distance")
        if item_mask is not None:
            item_mask = item_mask.to(dev)
        cuts = list(serving.chunks(R, row_chunk))
        pref = None if len(cuts) == 1 else torch.empty((R, Pl), dtype=torch.int64, device=dev)
        for sl in cuts:
            _, idx = engine.rank_topk(t.U, t.I, Pl, user_ids=user_ids[sl], exclude=excl, status=status)
            if pref is None:
                pref = idx                                             # one chunk: rank_topk's own tensor, no copy
            else:
                pref[sl] = idx
        out = engine.blend_points(pref, rowptr, rows, t.n_item, points=int(points), weights=weights, con=con, con_slot=con_slot,
                                  dis=dis, dis_slot=dis_slot, item_mask=item_mask, top=int(top), return_table=return_table,
                                  status=status)
        if serving.read_back(status)[0] != 0:
            raise IndexError("blended_ranking: a user id, a feature id, a context slot or a column's row index is out of range")
        if ids is not None:
            out = out[:2] + (ids,) + out[2:]
        return out


def diversified_ranking(model, user_ids: torch.Tensor, *, train=None, lam: float = 0.7, pool: int = 64, top: int = 10,
                        year_idx: int = 0, normalize: bool = True, user_chunk: int = 65536):
    """Top lists that are not ten near-duplicates in embedding space: per user the best `pool` items by predicted preference
    (`engine.rank_topk` on the propagated tables, the user's `train` items left out) re-ranked greedily by Maximal Marginal
    Relevance (`engine.lists.mmr_rerank`): pick 0 is the best item, every further pick the one with the greatest
    lam * relevance - (1 - lam) * (largest cosine to the items picked so far).  lam = 1 is `rank_topk`'s own order, smaller values
    trade accuracy for `evaluate.list_quality`'s `ild`, which takes the result as `lists=`.

      user_ids    int64 [B], one list per entry.
      train       engine.ItemSets or (users, items) pairs left out of the pools, or None.
      pool        candidates per user, at most engine.lists.MMR_POOL_MAX = 64; clipped to the catalogue size.
      top         picks per user, at most the (clipped) pool.
      normalize   scale a pool's scores to [0, 1] before they meet the cosines (scores of an inner-product model have no fixed range).
      user_chunk  users per ranking and re-ranking launch; the result does not depend on it.

    Returns (items int64 [B, top], keys float64 [B, top]) on the device: the picked ids and the key each was picked with; columns
    past a user's eligible items hold (-1, -inf).  One propagate in eval mode under no_grad, the caller's mode restored; one status
    word for the whole call, read back once at the end: a user id outside the table raises IndexError then.

    `blended_ranking`'s lists diversify the same way: `engine.lists.mmr_rerank(out_items, out_ratings, model.all_items_emb, top)`
    takes its float64 ratings as they are."""
    fn = "diversified_ranking"
    pool, top, user_chunk, lam = int(pool), int(top), int(user_chunk), float(lam)
    if pool < 1 or pool > engine.lists.MMR_POOL_MAX:
        raise ValueError(f"{fn}: pool={pool} outside [1, {engine.lists.MMR_POOL_MAX}]")
    if top < 1 or top > pool:
        raise ValueError(f"{fn}: top={top} outside [1, pool={pool}]")
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"{fn}: lam={lam} outside [0, 1]")
    if user_chunk < 1:
        raise ValueError(f"{fn}: user_chunk={user_chunk}")
    if not isinstance(user_ids, torch.Tensor) or user_ids.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{fn}: user_ids must be an int32 or int64 tensor")
    with serving.inference(model):
        t = serving.propagated(model, year_idx)
        n = min(pool, t.n_item)
        if top > n:
            raise ValueError(f"{fn}: top={top} above the pool of {n} entries (the catalogue has {t.n_item} items)")
        excl = None if train is None else serving.as_sets(train, t)
        user_ids = user_ids.reshape(-1).to(device=t.dev, dtype=torch.int64)
        B = int(user_ids.numel())
        status = serving.status_word(t.dev)
        items = torch.empty((B, top), dtype=torch.int64, device=t.dev)
        keys = torch.empty((B, top), dtype=torch.float64, device=t.dev)
        for sl in serving.chunks(B, user_chunk):
            vals, idx = engine.rank_topk(t.U, t.I, n, user_ids=user_ids[sl], exclude=excl, status=status)
            items[sl], keys[sl] = engine.lists.mmr_rerank(idx, vals, t.I, top, lam=lam, normalize=normalize, return_keys=True,
                                                          status=status)
        if serving.read_back(status)[0] != 0:
            raise IndexError(f"{fn}: a user id lies outside [0, {t.n_user})")
        return items, keys


# ---- the trip context from raw rows: what demo.py builds between its pickles and the blend -------------------------------------------
INF = float("inf")
MONTH_DAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)           # demo.py:114, month_info: no leap year


def congestion_table(month: torch.Tensor, day: torch.Tensor, dayofweek: torch.Tensor, item: torch.Tensor, values, *, n_item: int,
                     by: int = 0, wave_min: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The congestion pivot of demo.py:99-102 over raw rows, laid out as `blended_ranking` takes it: `month`, `day`, `dayofweek`,
    `item` int32 / int64 [T] (item: already the itemid) and `values`, one float64 [T] column or up to four (congestion_1,
    congestion_2, ...), on one device.  Returns `(table float64 [S, n_item], days int64 [S, 3])`: one table row per distinct
    (month, day, dayofweek), ascending, whose entry i is pandas' sum - its compensated sum, bit for bit - of column `by` over the
    rows of that day and item (`engine.context.group_sum_float`), +inf where the log has no such row: the per-day slice of
    demo.py:270-274, which `blended_ranking` sorts by that column.  The G group sums are scattered with torch indexing (distinct
    targets).  An item outside [0, n_item): IndexError."""
    fn = "congestion_table"
    n_item, by = int(n_item), int(by)
    if n_item < 1:
        raise ValueError(f"{fn}: n_item={n_item}")
    cols = [values] if isinstance(values, torch.Tensor) else list(values)
    if not 0 <= by < max(len(cols), 1):
        raise ValueError(f"{fn}: by={by} outside the {len(cols)} value columns")
    groups = engine.context.group_sum_float((month, day, dayofweek, item), cols, wave_min=wave_min)
    keys, dev = groups.keys, groups.keys[0].device
    G = int(keys[0].numel())
    if G == 0:
        return torch.empty((0, n_item), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev)
    if int(keys[3].min()) < 0 or int(keys[3].max()) >= n_item:
        raise IndexError(f"{fn}: an item lies outside [0, {n_item})")
    triple = torch.stack(keys[:3], 1)                                          # ascending: the groups are sorted by (month, day, dow, item)
    first = torch.ones(G, dtype=torch.bool, device=dev)
    first[1:] = (triple[1:] != triple[:-1]).any(1)
    slot = torch.cumsum(first, 0) - 1
    days = triple[first]
    table = torch.full((int(days.shape[0]), n_item), INF, dtype=torch.float64, device=dev)
    table[slot, keys[3]] = groups.sums[by]
    return table, days


def distance_table(departure_xy: torch.Tensor, item_xy: torch.Tensor) -> torch.Tensor:
    """float64 [S, n_item]: the metres between every departure point (float64 [S, 2]) and every destination (float64 [n_item, 2]),
    `haversine(dep, arr) * 1000` of demo.py:241-248 for all pairs in one launch (`engine.context.haversine_table`: the first
    coordinate is the latitude to the formula, as in the reference).  A NaN coordinate gives +inf."""
    return engine.context.haversine_table(departure_xy, item_xy)


def order_table(values: torch.Tensor) -> torch.Tensor:
    """float32 [S, n_item]: every entry of a context table (float [S, n_item], any device) replaced by its dense rank within its
    row - 0 for the smallest value, equal values equal ranks; +inf stays +inf and a NaN a NaN.  `blended_ranking` casts its tables
    to fp32, which can merge fp64 values that the reference's sort keeps apart (metres at 1e4 have an fp32 spacing of 1e-3); ranks
    are exact in fp32 for n_item < 2^24, so the fp64 order and its ties reach `engine.topk_rows` unchanged.  Set-up code in torch
    ops."""
    if values.dim() != 2 or not values.dtype.is_floating_point:
        raise ValueError(f"order_table: values must be a floating [S, n_item] table, got {values.dtype} {tuple(values.shape)}")
    S, n = int(values.shape[0]), int(values.shape[1])
    if n >= 2 ** 24:
        raise ValueError(f"order_table: n_item={n}: ranks are exact in float32 below 2^24 only")
    if n == 0:
        return values.to(torch.float32)
    ordered, idx = torch.sort(values, dim=1, stable=True)                      # NaNs last, after +inf
    step = torch.zeros((S, n), dtype=torch.int64, device=values.device)
    step[:, 1:] = ordered[:, 1:] != ordered[:, :-1]
    rank = torch.empty((S, n), dtype=torch.float32, device=values.device)
    rank.scatter_(1, idx, torch.cumsum(step, 1).to(torch.float32))
    rank[values == INF] = INF
    rank[values != values] = float("nan")
    return rank


class PartyRows(NamedTuple):
    """`party_rows`' result, every field int64 [R]: the request row's party and member (its position in the input), its user id
    (None without `user_codes`) and the five features."""
    party: torch.Tensor
    member: torch.Tensor
    user_ids: Optional[torch.Tensor]
    age: torch.Tensor
    sex: torch.Tensor
    month: torch.Tensor
    day: torch.Tensor
    dow: torch.Tensor

    @property
    def features(self):
        """(age, sex, month, day, dow), as `blended_ranking` takes them."""
        return (self.age, self.sex, self.month, self.day, self.dow)


def _per_party(fn: str, x, name: str, P: int, dev) -> torch.Tensor:
    t = torch.as_tensor(x).to(device=dev, dtype=torch.int64).reshape(-1)
    if int(t.numel()) == 1:
        t = t.expand(P)
    if int(t.numel()) != P:
        raise ValueError(f"{fn}: {name} has {int(t.numel())} entries for {P} parties")
    return t


def party_rows(party: torch.Tensor, age: torch.Tensor, sex: torch.Tensor, *, start_month, start_day, start_dow, duration,
               user_codes: Optional[torch.Tensor]) -> PartyRows:
    """The request rows of demo.py:134-181 for any number of parties.  `party`, `age` (in years), `sex` int64 [M], one entry per
    member: party[m] in [0, P) is the member's party; `start_month`, `start_day`, `start_dow`, `duration` are one int for all
    parties or [P] each.  Per member, in input order, one row per day k = 0 .. duration - 1 of its party's stay:
      age   (age // 10) * 10 + 5                                    (demo.py:152)
      date  the reference's walk from the start (a Feb 29 becomes Feb 28): a day past MONTH_DAYS[month] becomes
            day % MONTH_DAYS[month] and the month moves on           (demo.py:135-136, 154-165)
      dow   (start_dow + k) % 7
      id    the position of `engine.decimal_code((age, sex, month, day), (0, 0, 2, 2))` - the string str(age) + str(sex) + mm + dd -
            in `user_codes`, the sorted codes `preprocess.map_ids` produced (IdMaps.user_codes): `user_dict[u_feats]`.
    A row whose string is not in the dictionary raises IndexError naming the first such row (the reference's KeyError); so does a
    stay that walks past December (the reference reaches month 13 and fails on the same lookup) - before any device work.
    `user_codes` None: no lookup, `user_ids` is None and the rest, torch ops only, runs on any device."""
    fn = "party_rows"
    for nm, t in (("party", party), ("age", age), ("sex", sex)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{fn}: {nm} must be an int32 or int64 tensor")
        if t.dim() != 1 or int(t.numel()) != int(party.numel()):
            raise ValueError(f"{fn}: {nm} must be [M = {int(party.numel())}], got {tuple(t.shape)}")
    dev, M = party.device, int(party.numel())
    party, age, sex = (t.to(torch.int64) for t in (party, age, sex))
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)  # noqa: E731
    if M == 0:
        return PartyRows(*(i64(0) for _ in range(2)), None if user_codes is None else i64(0), *(i64(0) for _ in range(5)))
    if int(party.min()) < 0:
        raise IndexError(f"{fn}: a negative party number")
    if int(age.min()) < 0 or int(sex.min()) < 0:
        raise ValueError(f"{fn}: a negative age or sex")
    P = int(party.max()) + 1
    m0, d0, w0, dur = (_per_party(fn, x, nm, P, dev) for x, nm in ((start_month, "start_month"), (start_day, "start_day"),
                                                                   (start_dow, "start_dow"), (duration, "duration")))
    if int(dur.min()) < 0 or int(m0.min()) < 1 or int(m0.max()) > 12 or int(d0.min()) < 1:
        raise ValueError(f"{fn}: a negative duration, a start month outside [1, 12] or a start day below 1")
    d0 = torch.where((m0 == 2) & (d0 == 29), torch.full_like(d0, 28), d0)
    # the walk, once per party: [P, D] tables of the date on day k of the stay
    D = int(dur.max())
    lens = torch.tensor((0,) + MONTH_DAYS + (MONTH_DAYS[-1],), dtype=torch.int64, device=dev)      # index 13: never compared against
    month_k, day_k = torch.empty((P, max(D, 1)), dtype=torch.int64, device=dev), torch.empty((P, max(D, 1)), dtype=torch.int64, device=dev)
    mon, dd = m0.clone(), d0 - 1
    for k in range(D):
        dd = dd + 1
        ln = lens[mon.clamp(max=13)]
        over = (dd > ln) & (mon <= 12)                     # past December the reference has already failed: the month stays 13
        dd = torch.where(over, dd % ln, dd)
        mon = mon + over.to(torch.int64)
        month_k[:, k], day_k[:, k] = mon, dd
    per_member = dur[party]
    member = torch.repeat_interleave(torch.arange(M, device=dev), per_member)
    R = int(member.numel())
    start = torch.cumsum(per_member, 0) - per_member
    k = torch.arange(R, device=dev) - start[member]
    p = party[member]
    month, day = month_k[p, k], day_k[p, k]
    dow = (w0[p] + k) % 7
    age_r, sex_r = (age[member] // 10) * 10 + 5, sex[member]
    late = torch.nonzero(month > 12)
    if int(late.numel()):
        r = int(late[0])
        raise IndexError(f"{fn}: request row {r} (member {int(member[r])}, day {int(k[r])} of the stay) lies past December: "
                         "the reference's dictionary has no month 13")
    user_ids = None
    if user_codes is not None:
        if user_codes.dtype != torch.int64 or user_codes.dim() != 1:
            raise TypeError(f"{fn}: user_codes must be int64 [n_user], got {user_codes.dtype} {tuple(user_codes.shape)}")
        code = engine.decimal_code((age_r, sex_r, month, day), (0, 0, 2, 2))
        codes = user_codes.to(code.device).contiguous()
        n = int(codes.numel())
        user_ids = torch.searchsorted(codes, code)
        known = (user_ids < n) & (codes[user_ids.clamp(max=max(n - 1, 0))] == code) if n else torch.zeros_like(code, dtype=torch.bool)
        miss = torch.nonzero(~known)
        if int(miss.numel()):
            r = int(miss[0])
            raise IndexError(f"{fn}: request row {r}: '{int(age_r[r])}{int(sex_r[r])}{int(month[r]):02d}{int(day[r]):02d}' is not in "
                             "the user dictionary")
    return PartyRows(p, member, user_ids, age_r, sex_r, month, day, dow)


def context_slots(days: torch.Tensor, month: torch.Tensor, day: torch.Tensor, dow: torch.Tensor) -> torch.Tensor:
    """int64 [R]: the row of `congestion_table`'s `days` (int64 [S, 3], ascending (month, day, dayofweek)) that holds every request
    row's (month, day, dow) - the `congestion_slot` of `blended_ranking`.  A request row whose day the table does not have raises
    IndexError naming the first (the reference ends up with an empty frame there, demo.py:270-274).  Torch ops, any device."""
    fn = "context_slots"
    if days.dim() != 2 or int(days.shape[1]) != 3 or days.dtype != torch.int64:
        raise ValueError(f"{fn}: days must be int64 [S, 3], got {days.dtype} {tuple(days.shape)}")
    dev = days.device
    rows = torch.stack([t.reshape(-1).to(device=dev, dtype=torch.int64) for t in (month, day, dow)], 1)
    if int(rows.shape[0]) == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    every = torch.cat((days, rows))
    if int(every.min()) < 0 or int(every.max()) >= 2 ** 20:
        raise IndexError(f"{fn}: a month, day or dayofweek outside [0, 2^20)")
    pack = lambda t: (t[:, 0] * 2 ** 20 + t[:, 1]) * 2 ** 20 + t[:, 2]  # noqa: E731
    have, want = pack(days).contiguous(), pack(rows).contiguous()
    S = int(have.numel())
    if S > 1 and not bool((have[1:] > have[:-1]).all()):
        raise ValueError(f"{fn}: days is not in ascending order without repeats")
    slot = torch.searchsorted(have, want)
    found = (slot < S) & (have[slot.clamp(max=max(S - 1, 0))] == want) if S else torch.zeros_like(want, dtype=torch.bool)
    miss = torch.nonzero(~found)
    if int(miss.numel()):
        r = int(miss[0])
        raise IndexError(f"{fn}: request row {r}: the congestion table has no day (month, day, dayofweek) = {tuple(rows[r].tolist())}")
    return slot
