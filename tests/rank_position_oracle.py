"""Exact held-out positions and their metrics (include/ngcf_hip.h, "exact held-out positions") in plain numpy, from a score matrix.
It shares no code with the kernels: the order is a lexsort by (-key, item) with the float key restated on uint32, the metrics are the
header's formulas in fp64 in the order the header gives (terms in ascending position)."""
import numpy as np


def rank_key(scores):
    """float32 -> uint32, monotone: a larger float has a larger key, -0.0 < +0.0, NaN (sign clear) above +inf."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def rank_before(ka, ia, kb, ib):
    return ka > kb or (ka == kb and ia < ib)


def _eligible(n_items, excl):
    ok = np.ones(n_items, dtype=bool)
    excl = np.asarray(excl, dtype=np.int64)
    ok[excl[(excl >= 0) & (excl < n_items)]] = False
    return ok


def positions(scores, truth_rows, excl_rows=None):
    """Per user the int position of every entry of its truth row: its index in the user's eligible items sorted by (-key, item);
    -1 for an entry that is excluded or outside [0, n_items)."""
    scores = np.asarray(scores, dtype=np.float32)
    B, n_items = scores.shape
    out = []
    for b in range(B):
        ok = _eligible(n_items, [] if excl_rows is None else excl_rows[b])
        ids = np.nonzero(ok)[0]
        key = rank_key(scores[b]).astype(np.int64)
        order = ids[np.lexsort((ids, -key[ids]))]
        index_of = np.full(n_items, -1, dtype=np.int64)
        index_of[order] = np.arange(order.size)
        t = np.asarray(truth_rows[b], dtype=np.int64)
        inside = (t >= 0) & (t < n_items)
        p = np.full(t.shape, -1, dtype=np.int64)
        p[inside] = index_of[t[inside]]
        out.append(p)
    return out


def positions_brute(scores, truth_rows, excl_rows=None):
    """The definition itself: count, item by item, the eligible i != t with rank_before(key_i, i, key_t, t)."""
    scores = np.asarray(scores, dtype=np.float32)
    B, n_items = scores.shape
    out = []
    for b in range(B):
        ok = _eligible(n_items, [] if excl_rows is None else excl_rows[b])
        key = [int(k) for k in rank_key(scores[b])]
        row = []
        for t in [int(x) for x in truth_rows[b]]:
            if t < 0 or t >= n_items or not ok[t]:
                row.append(-1)
                continue
            row.append(sum(1 for i in range(n_items) if ok[i] and i != t and rank_before(key[i], i, key[t], t)))
        out.append(np.asarray(row, dtype=np.int64))
    return out


def metrics(position_rows, truth_rows, excl_lens, n_items, ks):
    """(per_user float64 [B, 4 + 4*len(ks)], sums float64 [4 + 4*len(ks) + 2]) of the header's formulas; sums are plain sequential
    sums over the users in order."""
    ks = [int(k) for k in ks]
    n_out = 4 + 4 * len(ks)
    per_user = np.zeros((len(truth_rows), n_out))
    sums = np.zeros(n_out + 2)
    for b, (pos, ids) in enumerate(zip(position_rows, truth_rows)):
        T = len(set(int(t) for t in ids))
        if T == 0:
            continue
        valid = sorted(set(int(p) for p in pos if p >= 0))
        neg = float(n_items - int(excl_lens[b]) - T)
        rr = ap = dcg = below = 0.0
        hits, dcg_k = [0] * len(ks), [0.0] * len(ks)
        for j, p in enumerate(valid):
            g = 1.0 / np.log2(float(p) + 2.0)
            if j == 0:
                rr = 1.0 / (float(p) + 1.0)
            ap += float(j + 1) / (float(p) + 1.0)
            dcg += g
            below += neg - float(p - j)
            for q, K in enumerate(ks):
                if p < K:
                    hits[q] += 1
                    dcg_k[q] += g
        idcg, idcg_k = 0.0, [0.0] * len(ks)
        for j in range(T):
            g = 1.0 / np.log2(float(j) + 2.0)
            idcg += g
            for q, K in enumerate(ks):
                if j < K:
                    idcg_k[q] += g
        v = per_user[b]
        v[0], v[1], v[2] = rr, ap / float(T), dcg / idcg
        if neg > 0.0:
            v[3] = below / (float(T) * neg)
            sums[-1] += 1.0
        for q, K in enumerate(ks):
            v[4 + 4 * q:8 + 4 * q] = [hits[q] / float(T), dcg_k[q] / idcg_k[q], hits[q] / float(K), float(hits[q] > 0)]
        sums[:n_out] += v
        sums[-2] += 1.0
    return per_user, sums


def rows_of(rowptr, colidx, offset=0):
    """The rows of an item set in CSR form as a list of int64 arrays of item ids."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64) - int(offset)
    return [colidx[rowptr[r]:rowptr[r + 1]] for r in range(rowptr.size - 1)]
