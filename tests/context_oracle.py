"""The trip context in plain numpy / Python, written from the statements in include/ngcf_hip.h and from demo.py:96-103, 134-181,
241-248 of the reference (no code shared with the product, nothing here runs on a GPU): the sequential Kahan sum of pandas'
group_sum, the haversine formula twice (numpy's and `math`'s libm), the demo's party loop as the literal loop, dense ranks - and the
seeded inputs that the CPU tests pin to pandas and the GPU tests run on the device."""
import functools
import math

import numpy as np

MAGNITUDES = (1e-8, 1.0, 1e8, 1e16)
SEGMENT_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097)
MONTH_INFO = {1: 31, 2: 28, 3: 31, 4: 30, 5: 31, 6: 30, 7: 31, 8: 31, 9: 30, 10: 31, 11: 30, 12: 31}
EARTH_KM = 6371.0088
HALF_CIRCUMFERENCE_M = math.pi * EARTH_KM * 1000


# ---- Kahan -----------------------------------------------------------------------------------------------------------------------
def kahan(values):
    """pandas' group_sum recurrence over one group's values in the order given."""
    s = c = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in np.asarray(values, dtype=np.float64):
            if v != v:
                continue
            y = v - c
            t = s + y
            c = (t - s) - y
            if c != c:
                c = np.float64(0.0)
            s = t
    return s


def naive(values):
    """A plain left-to-right sum of the values that are not NaN: what a kernel without the compensation would give."""
    s = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in np.asarray(values, dtype=np.float64):
            if v == v:
                s = s + v
    return s


def segment_sums(rowptr, x, order=None, fn=kahan):
    pos = np.arange(len(x)) if order is None else np.asarray(order)
    return np.array([fn(x[pos[rowptr[u]:rowptr[u + 1]]]) for u in range(len(rowptr) - 1)], dtype=np.float64)


def _mixed(rng, n, nan_share=0.05):
    x = rng.standard_normal(n) * rng.choice(MAGNITUDES, n)
    x[rng.random(n) < nan_share] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def kahan_case(n_values, with_order, seed=0):
    """Segments of every length in SEGMENT_LENGTHS (in a seeded shuffle), an all-NaN one and one whose first value is +inf, with
    magnitudes from MAGNITUDES and NaNs.  `(rowptr, order or None, labels, columns, want, plain)`: labels[t] is row t's segment;
    with an order the rows of a segment are scattered over the log and `order` lists them in row order.  Read only."""
    rng = np.random.default_rng(100 * n_values + 10 * int(with_order) + seed)
    lengths = list(SEGMENT_LENGTHS) + [5, 70]
    kind = ["mixed"] * len(SEGMENT_LENGTHS) + ["nan", "inf"]
    perm = rng.permutation(len(lengths))
    lengths, kind = [lengths[i] for i in perm], [kind[i] for i in perm]
    rowptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    T = int(rowptr[-1])
    grouped = np.repeat(np.arange(len(lengths)), lengths)
    if with_order:
        labels = grouped[rng.permutation(T)]
        order = np.argsort(labels, kind="stable").astype(np.int64)
    else:
        labels, order = grouped, None
    pos = np.arange(T) if order is None else order
    columns = []
    for _ in range(n_values):
        x = _mixed(rng, T)
        for u, k in enumerate(kind):
            mine = pos[rowptr[u]:rowptr[u + 1]]
            if k == "nan":
                x[mine] = np.nan
            elif k == "inf":
                x[mine] = rng.standard_normal(len(mine)) * 1e8
                x[mine[0]] = np.inf
        columns.append(x)
    want = tuple(segment_sums(rowptr, x, order) for x in columns)
    plain = tuple(segment_sums(rowptr, x, order, naive) for x in columns)
    return rowptr, order, labels.astype(np.int64), tuple(columns), want, plain


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- the congestion log and its pivot --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def congestion_log(days, n_item, seed=0, absent=0.1):
    """A shuffled raw log: per (day, item) pair 1-30 rows, a share of the pairs absent; `days` a tuple of (month, day, dayofweek).
    Columns month, day, dayofweek, item int64 [T] and congestion_1, congestion_2 float64 [T].  Read only."""
    rng = np.random.default_rng(7000 + seed)
    rows = []
    for d, (mo, dy, dw) in enumerate(days):
        for i in range(n_item):
            if rng.random() < absent:
                continue
            rows += [(mo, dy, dw, i)] * int(rng.integers(1, 31))
    keys = np.array(rows, dtype=np.int64)[rng.permutation(len(rows))]
    T = len(keys)
    return dict(month=keys[:, 0].copy(), day=keys[:, 1].copy(), dayofweek=keys[:, 2].copy(), item=keys[:, 3].copy(),
                congestion_1=_mixed(rng, T, 0.02), congestion_2=_mixed(rng, T, 0.02))


def pivot_float(columns, values):
    """`(keys, sums, inverse)` of pd.pivot_table(index=columns, aggfunc='sum'): the distinct key rows ascending, the Kahan sum of
    every value column over a group's rows in row order."""
    table = np.stack([np.asarray(c, dtype=np.int64) for c in columns], axis=1)
    uniq, inverse = np.unique(table, axis=0, return_inverse=True)
    inverse = np.asarray(inverse, dtype=np.int64).reshape(-1)
    order = np.argsort(inverse, kind="stable")
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(inverse, minlength=len(uniq)))))
    sums = tuple(segment_sums(rowptr, np.asarray(v, dtype=np.float64), order) for v in values)
    return tuple(np.ascontiguousarray(uniq[:, k]) for k in range(table.shape[1])), sums, inverse


def congestion_table(log, n_item, by=0):
    """`(table [S, n_item], days [S, 3])`: the pivot's column `by` per distinct (month, day, dayofweek) ascending, +inf where absent."""
    keys, sums, _ = pivot_float([log[c] for c in ("month", "day", "dayofweek", "item")], [log["congestion_1"], log["congestion_2"]])
    days = np.unique(np.stack(keys[:3], 1), axis=0)
    index = {tuple(d): s for s, d in enumerate(days.tolist())}
    table = np.full((len(days), n_item), np.inf)
    for g in range(len(keys[0])):
        table[index[(int(keys[0][g]), int(keys[1][g]), int(keys[2][g]))], int(keys[3][g])] = sums[by][g]
    return table, days.astype(np.int64)


# ---- haversine -------------------------------------------------------------------------------------------------------------------
def haversine_numpy(dep, item):
    """[S, n_item] metres, the package's formula with numpy's sin / cos / arcsin; a NaN result is +inf."""
    k = math.pi / 180
    lat1, lng1 = (dep[:, 0] * k)[:, None], (dep[:, 1] * k)[:, None]
    lat2, lng2 = (item[:, 0] * k)[None, :], (item[:, 1] * k)[None, :]
    with np.errstate(invalid="ignore"):
        a, b = np.sin((lat2 - lat1) * 0.5), np.sin((lng2 - lng1) * 0.5)
        d = a * a + (np.cos(lat1) * np.cos(lat2)) * (b * b)
        out = ((2 * EARTH_KM) * np.arcsin(np.sqrt(d))) * 1000
    return np.where(out != out, np.inf, out)


def haversine_math(dep, item):
    """The same formula as the `haversine` package runs it: Python floats and the `math` module, pair by pair."""
    out = np.empty((len(dep), len(item)))
    for s, (x1, y1) in enumerate(dep.tolist()):
        for i, (x2, y2) in enumerate(item.tolist()):
            if any(v != v for v in (x1, y1, x2, y2)):
                out[s, i] = np.inf
                continue
            lat1, lng1, lat2, lng2 = map(math.radians, (x1, y1, x2, y2))
            d = math.sin((lat2 - lat1) * 0.5) ** 2 + math.cos(lat1) * math.cos(lat2) * math.sin((lng2 - lng1) * 0.5) ** 2
            out[s, i] = 2 * EARTH_KM * math.asin(math.sqrt(d)) * 1000
    return out


def ulps(got, want):
    """|got - want| in units of the spacing of the expected value (0 where both are equal, infinities included)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want) / np.spacing(np.abs(want))
    return np.where(got == want, 0.0, err)


@functools.lru_cache(maxsize=None)
def points(kind, S, n_item, seed=0):
    """`(dep [S, 2], item [n_item, 2])` degrees, latitude first: "seoul" inside (37.4-37.7, 126.8-127.2); "globe" anywhere, the
    items kept whose distance to every departure point is below 0.9 of half the circumference (the formula is ill-conditioned near
    antipodes).  Item 1 coincides with departure point 0 and item 2 with item 3."""
    rng = np.random.default_rng(300 + seed + (0 if kind == "seoul" else 50))
    box = ((37.4, 37.7), (126.8, 127.2)) if kind == "seoul" else ((-90.0, 90.0), (-180.0, 180.0))
    draw = lambda n: np.stack([rng.uniform(*box[0], n), rng.uniform(*box[1], n)], 1)  # noqa: E731
    dep = draw(S)
    item = draw(8 * n_item + 64)
    keep = (haversine_numpy(dep, item) < 0.9 * HALF_CIRCUMFERENCE_M).all(0)
    item = item[keep][:n_item].copy()
    assert len(item) == n_item
    if n_item > 3:
        item[1], item[2] = dep[0], item[3]
    return dep, item


# ---- the party loop, demo.py:134-181 ---------------------------------------------------------------------------------------------
def party_loop(ages, sexes, month, day, dow, duration, user_dict=None):
    """One party, the reference's loop as written: rows [uid, age, sex, month, day, dow], members in input order, days ascending.
    A string that `user_dict` does not hold raises KeyError, as there; without a dictionary the uid is -1."""
    dates = ["%02d" % month, "%02d" % day]
    if (dates[0] == '02') & (dates[1] == '29'):
        dates[1] = '28'
    month, day = int(dates[0]), int(dates[1])
    total_user_info = []
    for i in range(len(ages)):
        sex = int(sexes[i])
        age = ((int(ages[i]) // 10) * 10 + 5)
        day_tmp = day - 1
        month_tmp = month
        for length in range(int(duration)):
            dow_tmp = dow + length
            dow_tmp = dow_tmp % 7
            day_tmp = day_tmp + 1
            if day_tmp > MONTH_INFO[month_tmp]:
                day_tmp = day_tmp % MONTH_INFO[month_tmp]
                month_tmp += 1
            m_str = str(month_tmp)
            d_str = str(day_tmp)
            if month_tmp < 10:
                m_str = '0' + m_str
            if day_tmp < 10:
                d_str = '0' + d_str
            u_feats = str(age) + str(sex) + m_str + d_str
            uid = user_dict[u_feats] if user_dict is not None else -1
            total_user_info.append([uid, age, sex, month_tmp, day_tmp, dow_tmp])
    return total_user_info


# ---- dense ranks -----------------------------------------------------------------------------------------------------------------
def dense_ranks(values):
    """float32 [S, n]: per row the number of distinct smaller values; +inf stays +inf, a NaN a NaN."""
    values = np.asarray(values, dtype=np.float64)
    out = np.empty(values.shape, dtype=np.float32)
    for s, row in enumerate(values):
        distinct = sorted(set(v for v in row.tolist() if v == v and v != np.inf))
        rank = {v: r for r, v in enumerate(distinct)}
        out[s] = [np.inf if v == np.inf else (np.nan if v != v else rank[v]) for v in row.tolist()]
    return out
