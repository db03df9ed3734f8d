"""Exact host oracle of device-side node dropout (tests/test_dropout_paths_gpu.py), in plain numpy, written from the statements in
include/ngcf_hip.h and the comments of csrc/common.h - no code shared with the product, and nothing here runs on a GPU.
tests/test_dropout_oracle.py checks these helpers on the CPU.

Why the product is EXACT: matrix values are drawn from {1, 2, 3} and table values from +-{1..8}, so every fp32 partial sum of a row
is an integer of at most (entries of the longest row) * 3 * 8 - about 1 000 * 24 here, far below 2^24.  Such a sum is the same in
any order, with or without fma, so a kernel's result must equal the int64 product bit for bit (`torch.equal`): one entry kept or
dropped wrongly changes every column of its row by at least 1, and no tolerance has to be measured."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
TABLE_WIDTH = 770                  # the widest product of the tests: narrower ones use the first d columns of the same table


def drop_threshold(p):
    """The library takes drop_p as a C float and keeps an entry iff its hash >= (uint32_t)((double)drop_p * 2^32)."""
    return int(float(np.float32(p)) * 2 ** 32)


def _fmix64(x):
    """murmur3's 64-bit finaliser on a uint64 array (array arithmetic wraps modulo 2^64)."""
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def edge_hash(rows, cols, seed):
    """The 32-bit hash of entry (row, column) of L under one seed: low word of fmix64(seed ^ ((row << 32 | column) * golden))."""
    i = np.atleast_1d(np.asarray(rows)).astype(np.uint64)
    j = np.atleast_1d(np.asarray(cols)).astype(np.uint64)
    e = ((i << np.uint64(32)) | (j & np.uint64(0xFFFFFFFF))) * GOLDEN
    s = np.full(1, int(seed) & M64, dtype=np.uint64)
    return _fmix64(s ^ e) & np.uint64(0xFFFFFFFF)


def keep_mask(rows, cols, seeds, p, transposed=False):
    """Which stored entries survive: every seed's hash must be >= the threshold (cumulative over the seeds).  The key is always the
    entry's (row, column) in L; with `transposed` the arguments are the row and column of the CSR of L^T, and they are swapped."""
    if transposed:
        rows, cols = cols, rows
    thr = np.uint64(drop_threshold(p))
    keep = np.ones(np.atleast_1d(np.asarray(rows)).shape, dtype=bool)
    for s in seeds:
        keep &= edge_hash(rows, cols, s) >= thr
    return keep


def spmm_exact(rows, cols, vals, X, keep=None, n_rows=None):
    """out[r] = sum over the kept entries (r, c, v) of v * X[c], in int64 (rows sorted, one `reduceat` per block of columns)."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals, X = np.asarray(vals), np.asarray(X)
    assert np.array_equal(vals, np.rint(vals)) and np.array_equal(X, np.rint(X)), "integer-valued data only"
    vals, X = vals.astype(np.int64), X.astype(np.int64)
    n_rows = int(rows.max()) + 1 if n_rows is None else int(n_rows)
    out = np.zeros((n_rows, X.shape[1]), dtype=np.int64)
    if keep is not None:
        keep = np.asarray(keep, dtype=bool)
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    if rows.size == 0:
        return out
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
    for c0 in range(0, X.shape[1], 128):
        out[rows[starts], c0:c0 + 128] = np.add.reduceat(vals[:, None] * X[cols, c0:c0 + 128], starts, axis=0)
    return out


def splitmix_advance(words):
    """One step of ngcf_seeds_advance on every word: a splitmix64 step, shifted right by two (results below 2^62)."""
    # word by word: numpy would take a list that mixes values below and above 2^63 through float64
    words = words if isinstance(words, (list, tuple)) else np.atleast_1d(words).tolist()
    x = np.array([np.uint64(int(w) & M64) for w in words], dtype=np.uint64)
    x = x + GOLDEN
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return x >> np.uint64(2)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
S_USERS, S_ITEMS = 1536, 96
S_EMPTY_ROWS = (7, 700)            # user rows without entries
S_DUP_ROW = 41                     # a user row whose entries all sit on one column
W_N = 2048
W_HEAVY = ((100, 300), (1900, 1000))    # (row, entries)


def _values(rng, n):
    return rng.integers(1, 4, n)


def _by_row(rows, cols, vals):
    order = np.argsort(rows, kind="stable")
    return rows[order].astype(np.int64), cols[order].astype(np.int64), vals[order].astype(np.int64)


def _seoul(rng):
    """Matrix S, Seoul-shaped, N = 1536 + 96: user rows of 8..16 entries into the 96 item columns (a gathered table of <= 512 rows),
    item rows of 170..210 entries into the user columns (longer than the 64-entry segments of a small matrix: cut rows)."""
    rows, cols = [], []
    for u in range(S_USERS):
        if u in S_EMPTY_ROWS:
            continue
        if u == S_DUP_ROW:
            c = np.full(12, S_USERS + 17)
        else:
            c = S_USERS + rng.choice(S_ITEMS, int(rng.integers(8, 17)), replace=False)
            if u == 3 and S_USERS + 5 not in c:
                c[0] = S_USERS + 5                     # entry (3, item 5): the threshold witness of the tests
        rows.append(np.full(c.size, u))
        cols.append(c)
    for i in range(S_ITEMS):
        c = rng.choice(S_USERS, int(rng.integers(170, 211)), replace=False)
        rows.append(np.full(c.size, S_USERS + i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return rows, cols, _values(rng, rows.size), S_USERS + S_ITEMS, S_USERS + S_ITEMS


def _wide(rng):
    """Matrix W, 2048 x 2048: 8 random columns per row over the whole range (one sliceable row group that is no table group), two
    heavy rows of 300 and 1 000 entries, every 100th entry stored twice."""
    rows = np.repeat(np.arange(W_N), 8)
    cols = rng.integers(0, W_N, rows.size)
    for r, n in W_HEAVY:
        sel = rows != r
        rows, cols = np.r_[rows[sel], np.full(n, r)], np.r_[cols[sel], rng.integers(0, W_N, n)]
    vals = _values(rng, rows.size)
    dup = np.arange(0, rows.size, 100)
    return np.r_[rows, rows[dup]], np.r_[cols, cols[dup]], np.r_[vals, vals[dup]], W_N, W_N


def build_case(name):
    """COO arrays (sorted by row, int64) and an integer table of a named case: dict(rows, cols, vals, n_rows, n_cols, table).
    'S', 'W': see above; 'St', 'Wt': the CSR of their transposes (to be walked with transposed=True); 'Su': the user rows of S as a
    1536 x 96 matrix of their own (item columns 0..95: it holds entry (3, 5)); 'one': 1 x 1; 'tiny': 5 x 3 with 40 entries per row.
    `table` is [n_cols, TABLE_WIDTH] with values in +-{1..8}."""
    base = name[0] if name in ("St", "Wt", "Su") else name
    rng = np.random.default_rng({"S": 2019, "W": 2048, "one": 1, "tiny": 53}[base])
    if base == "S":
        rows, cols, vals, n_rows, n_cols = _seoul(rng)
    elif base == "W":
        rows, cols, vals, n_rows, n_cols = _wide(rng)
    elif base == "one":
        rows, cols, vals, n_rows, n_cols = np.zeros(1, int), np.zeros(1, int), np.array([2]), 1, 1
    else:
        rows, cols, n_rows, n_cols = np.repeat(np.arange(5), 40), rng.integers(0, 3, 200), 5, 3
        vals = _values(rng, 200)
    if name in ("St", "Wt"):
        rows, cols, n_rows, n_cols = cols, rows, n_cols, n_rows
    if name == "Su":
        sel = rows < S_USERS
        rows, cols, vals, n_rows, n_cols = rows[sel], cols[sel] - S_USERS, vals[sel], S_USERS, S_ITEMS
    rows, cols, vals = _by_row(rows, cols, vals)
    trng = np.random.default_rng(7 + n_cols)
    table = trng.integers(1, 9, (n_cols, TABLE_WIDTH)) * trng.choice(np.array([-1, 1]), (n_cols, TABLE_WIDTH))
    return {"rows": rows, "cols": cols, "vals": vals, "n_rows": n_rows, "n_cols": n_cols, "table": table.astype(np.int64)}
