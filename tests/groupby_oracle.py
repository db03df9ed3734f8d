"""The pivot, the id maps and the decimal string code in plain numpy, written from the statements in include/ngcf_hip.h and from
utils.py:46-48, 59-97 of the reference (no code shared with the product, nothing here runs on a GPU)."""
import numpy as np

MAX_CHARS = 18
MASK64 = (1 << 64) - 1


def pivot(columns, values=()):
    """`(keys, sums, inverse)`: the distinct rows of the K key columns ascending by (column 0, column 1, ...) as K int64 arrays,
    the V int64 sums per group (np.add.at: integer, modulo 2^64), and every row's group index."""
    K = len(columns)
    T = len(columns[0])
    table = np.stack([np.asarray(c, dtype=np.int64) for c in columns], axis=1) if T else np.zeros((0, K), dtype=np.int64)
    uniq, inverse = np.unique(table, axis=0, return_inverse=True)
    inverse = np.asarray(inverse, dtype=np.int64).reshape(-1)
    sums = []
    for v in values:
        s = np.zeros(len(uniq), dtype=np.int64)
        with np.errstate(over="ignore"):
            np.add.at(s, inverse, np.asarray(v, dtype=np.int64))
        sums.append(s)
    return tuple(np.ascontiguousarray(uniq[:, k]) for k in range(K)), tuple(sums), inverse


def user_strings(age, sex, month, day):
    """str(age) + str(sex) + '%m' + '%d', the `merged` series of utils.py:71."""
    return np.array([f"{int(a)}{int(s)}{int(m):02d}{int(d):02d}" for a, s, m, d in zip(age, sex, month, day)], dtype=object)


def id_maps(age, sex, month, day, destination):
    """`(userid, itemid, user_map, item_map)` exactly as utils.py:70-84: the dictionaries enumerate np.sort of the distinct values."""
    merged = user_strings(age, sex, month, day).astype(str)
    user_map = {item: i for i, item in enumerate(np.sort(np.unique(merged)))}
    item_map = {int(item): i for i, item in enumerate(np.sort(np.unique(np.asarray(destination))))}
    userid = np.array([user_map[m] for m in merged], dtype=np.int64)
    itemid = np.array([item_map[int(d)] for d in destination], dtype=np.int64)
    return userid, itemid, {str(k): v for k, v in user_map.items()}, item_map


def code_of_string(s: str) -> int:
    """Every character '0' + d is the base-11 digit d + 1 of a left-aligned number of 18 places, padding 0."""
    assert len(s) <= MAX_CHARS and s.isdigit()
    return sum((ord(ch) - ord("0") + 1) * 11 ** (MAX_CHARS - 1 - i) for i, ch in enumerate(s))


def decimal_code(columns, widths):
    out = np.empty(len(columns[0]), dtype=np.int64)
    for t in range(len(out)):
        s = "".join(str(int(c[t])) if w == 0 else str(int(c[t])).zfill(w) for c, w in zip(columns, widths))
        out[t] = code_of_string(s)
    return out


def fmix64(x: int) -> int:
    """The 64-bit finaliser of MurmurHash3: the table's hash."""
    x &= MASK64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & MASK64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & MASK64
    x ^= x >> 33
    return x


def reference_users():
    """`(age, sex, month, day)` of the reference's 5 840 users: 8 ages x 2 sexes x the 365 days of a year without a 29 February."""
    days = np.arange("2019-01-01", "2020-01-01", dtype="datetime64[D]")
    months = days.astype("datetime64[M]")
    month, day = months.astype(np.int64) % 12 + 1, (days - months).astype(np.int64) + 1
    age, sex, d = (a.reshape(-1) for a in np.meshgrid(np.arange(5, 85, 10), np.arange(2), np.arange(len(days)), indexing="ij"))
    return age.astype(np.int64), sex.astype(np.int64), month[d], day[d]
