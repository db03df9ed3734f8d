"""A numpy statement of the rank-point blending (demo.py:285-292, 315-334, 378-398) for the blend tests.  It shares no code with the
library: np.lexsort for every ordering, integer point sums per column, the fp64 formula, the mask, a lexsort for the top list."""
import numpy as np


def lists_desc(scores, n):
    """Per row the n columns of largest value, value descending, ties lowest column first."""
    cols = np.arange(scores.shape[1])
    return np.stack([np.lexsort((cols, -row))[:n] for row in scores]).astype(np.int64)


def lists_asc(values, n):
    """Per row the n columns of smallest value, value ascending, ties lowest column first."""
    cols = np.arange(values.shape[1])
    return np.stack([np.lexsort((cols, row))[:n] for row in values]).astype(np.int64)


def _kinds(pref, con, con_slot, dis, dis_slot):
    return ((pref, None), (con, con_slot), (dis, dis_slot))


def point_sums(pref, con, con_slot, dis, dis_slot, rowptr, rows, n_items, P):
    """int64 [3, G, n_items]: the points of each kind per column and item.  An id out of range adds nothing: a row index outside
    [0, R), a slot outside its table, a list entry outside [0, n_items) (-1 is an empty slot)."""
    G, R = len(rowptr) - 1, pref.shape[0]
    pts = np.zeros((3, G, n_items), dtype=np.int64)
    for g in range(G):
        for r in rows[rowptr[g]:rowptr[g + 1]]:
            if not 0 <= r < R:
                continue
            for q, (lists, slot) in enumerate(_kinds(pref, con, con_slot, dis, dis_slot)):
                if lists is None:
                    continue
                s = r if slot is None else slot[r]
                if not 0 <= s < lists.shape[0]:
                    continue
                ids = lists[s]
                ok = (ids >= 0) & (ids < n_items)
                np.add.at(pts[q, g], ids[ok], (P - np.arange(len(ids)))[ok])
    return pts


def blend(pts, weights, mask, top):
    """(table float64 [G, n_items], items int64 [G, top], rating float64 [G, top]) from the point sums."""
    table = pts[0] * weights[0] + pts[1] * weights[1] + pts[2] * weights[2]       # fp64, left to right, one rounding per operation
    G, n_items = table.shape
    elig = np.arange(n_items) if mask is None else np.nonzero(mask)[0]
    items = np.full((G, top), -1, dtype=np.int64)
    rating = np.full((G, top), -np.inf)
    for g in range(G):
        best = elig[np.lexsort((elig, -table[g, elig]))[:top]]
        items[g, :len(best)] = best
        rating[g, :len(best)] = table[g, best]
    return table, items, rating


def row_by_row(pref, con, con_slot, dis, dis_slot, rowptr, rows, n_items, P, weights):
    """The reference's accumulation (demo.py:287-292): per request row `rating += rank2rate * weight`, three times, in fp64."""
    G = len(rowptr) - 1
    rank2rate = np.arange(P, 0, -1)
    rating = np.zeros((G, n_items))
    for g in range(G):
        for r in rows[rowptr[g]:rowptr[g + 1]]:
            for (lists, slot), w in zip(_kinds(pref, con, con_slot, dis, dis_slot), weights):
                if lists is None:
                    continue
                ids = lists[r if slot is None else slot[r]]
                ok = ids >= 0
                rating[g, ids[ok]] = rating[g, ids[ok]] + (np.array(rank2rate[:len(ids)]) * w)[ok]
    return rating
