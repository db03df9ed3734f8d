"""Matrices that put rows, row blocks and row groups on the branch points of the CSR's host plan (csrc/csr.hip: cut_rows,
build_row_groups; csrc/csr_filter.hip: the borrowed plan of a thinned copy; csrc/spmm_swept.hip: swept parts beside row-wise groups),
and the host formulas the tests hold the library to.  Plain numpy, nothing here runs on a GPU; tests/test_plan_cases.py checks on the
CPU that every case has the row lengths, segment counts, group classes and masks it was built for, tests/test_csr_plan_gpu.py runs them.

As in tests/dropout_oracle.py all data is integer valued (matrix values in {1, 2, 3}, table values in +-{1..8}), so every fp32 sum of
a product is an integer far below 2^24 and a kernel's result must equal dropout_oracle.spmm_exact bit for bit."""
import functools

import numpy as np

import dropout_oracle as orc

INT32_MAX = 2 ** 31 - 1
LDS_TABLE_ROWS = 512                     # kLdsTableRows (csrc/common.h)
MIN_SEG_LEN, MAX_SEG_LEN = 64, 2048


# ---- host formulas ---------------------------------------------------------------------------------------------------------------
def row_lengths(case):
    return np.bincount(case["rows"], minlength=case["n_rows"]).astype(np.int64)


def rowptr(case):
    return np.r_[0, np.cumsum(row_lengths(case))].astype(np.int64)


def default_seg_len(nnz):
    """default_seg_len of csrc/common.h: the smallest power of two from 64 to 2048 with seg_len * 4096 >= nnz."""
    s = MIN_SEG_LEN
    while s < MAX_SEG_LEN and s * 4096 < nnz:
        s *= 2
    return s


def segment_plan(lens, seg_len):
    """cut_rows: rows longer than seg_len are cut every seg_len entries -> (cut rows, segments, longest row)."""
    lens = np.asarray(lens, dtype=np.int64)
    cut = lens > seg_len
    return int(cut.sum()), int(((lens[cut] + seg_len - 1) // seg_len).sum()), int(lens.max()) if lens.size else 0


def slice_footprint_rows(slice_max_mb=48):
    """Largest column range of a sliceable row block: a 128-byte slice of every gathered row within slice_max_mb MiB."""
    return (slice_max_mb << 20) // 128


def block_rows(n_rows):
    return 64 if n_rows <= 65536 else 1024


def host_groups(case, slice_max_mb=48):
    """build_row_groups step by step: the class of every row block (2 table-in-LDS: at most 512 gathered columns; 1 sliceable, an
    empty block too; 0 neither), runs of one class, the demotion of a table group whose union is wider than 512, a non-table group of
    under 16 blocks takes a non-table neighbour's class, equal non-table neighbours fuse, column ranges.
    -> [dict(begin, end, sliceable, lds_table, col_lo, col_hi)]"""
    n_rows, B = case["n_rows"], block_rows(case["n_rows"])
    if n_rows == 0:
        return []
    nb = (n_rows + B - 1) // B
    bmin, bmax = np.full(nb, INT32_MAX, np.int64), np.full(nb, -1, np.int64)
    np.minimum.at(bmin, case["rows"] // B, case["cols"])
    np.maximum.at(bmax, case["rows"] // B, case["cols"])
    limit = slice_footprint_rows(slice_max_mb)

    def block_class(b):
        if bmax[b] < 0:
            return 1
        span = bmax[b] - bmin[b] + 1
        return 2 if span <= LDS_TABLE_ROWS else 1 if span <= limit else 0

    def col_range(g):
        blocks = [b for b in range(g["begin"] // B, nb) if b * B < g["end"] and bmax[b] >= 0]
        return (min(int(bmin[b]) for b in blocks), max(int(bmax[b]) for b in blocks)) if blocks else (INT32_MAX, -1)

    groups, cls = [], []
    for b in range(nb):
        k, lo, hi = block_class(b), b * B, min(n_rows, (b + 1) * B)
        if groups and cls[-1] == k:
            groups[-1]["end"] = hi
        else:
            groups.append({"begin": lo, "end": hi, "sliceable": k >= 1, "lds_table": k == 2})
            cls.append(k)
    for g in groups:
        lo, hi = col_range(g)
        if g["lds_table"] and hi >= 0 and hi - lo + 1 > LDS_TABLE_ROWS:
            g["lds_table"] = False
    for i, g in enumerate(groups):
        if g["lds_table"] or len(groups) == 1 or g["end"] - g["begin"] >= 16 * B:
            continue
        other = groups[i - 1] if i > 0 else groups[i + 1]
        if not other["lds_table"]:
            g["sliceable"] = other["sliceable"]
    k = 1
    while k < len(groups):
        a, b = groups[k - 1], groups[k]
        if a["sliceable"] == b["sliceable"] and not a["lds_table"] and not b["lds_table"]:
            a["end"] = b["end"]
            del groups[k]
        else:
            k += 1
    for g in groups:
        g["col_lo"], g["col_hi"] = col_range(g)
    return groups


def shape_of(groups):
    """[(begin, end, class)] with class 'T' table-in-LDS, 'S' sliceable, 'N' neither."""
    return [(g["begin"], g["end"], "T" if g["lds_table"] else "S" if g["sliceable"] else "N") for g in groups]


# ---- builders --------------------------------------------------------------------------------------------------------------------
def _table(n_cols, width, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 9, (n_cols, width)) * rng.choice(np.array([-1, 1]), (n_cols, width))
    return t.astype(np.int64)


def _assemble(seed, n_rows, n_cols, parts, planted=(), width=96):
    """parts: (row_lo, row_hi, entries per row, col_lo, col_hi) - uniform random columns in [col_lo, col_hi]; the first row of every
    64-row block of a part (and the part's first row) holds both col_lo and col_hi, so every block spans exactly the part's range.
    planted: (row, entries, col_lo, col_hi) replaces a row; its first two entries are col_lo and col_hi as well."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for lo, hi, k, c_lo, c_hi in parts:
        if k == 0:
            continue
        assert k >= 2 and 0 <= c_lo <= c_hi < n_cols and 0 <= lo < hi <= n_rows
        r = np.arange(lo, hi)
        c = rng.integers(c_lo, c_hi + 1, (hi - lo, k))
        pin = (r % 64 == 0) | (r == lo)
        c[pin, 0], c[pin, 1] = c_lo, c_hi
        rows.append(np.repeat(r, k))
        cols.append(c.reshape(-1))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    for r, n, c_lo, c_hi in planted:
        sel = rows != r
        c = rng.integers(c_lo, c_hi + 1, n)
        c[:2] = (c_lo, c_hi)[:n]
        rows, cols = np.r_[rows[sel], np.full(n, r)], np.r_[cols[sel], c]
    vals = rng.integers(1, 4, rows.size)
    order = np.argsort(rows, kind="stable")
    return {"rows": rows[order].astype(np.int64), "cols": cols[order].astype(np.int64), "vals": vals[order].astype(np.int64),
            "n_rows": n_rows, "n_cols": n_cols, "table": _table(n_cols, width, 7 + n_cols + n_rows), "slice_max_mb": 48}


# ---- part 2: segment boundaries --------------------------------------------------------------------------------------------------
SEG_N = 2048
SEG_TABLE_COLS = (256, 767)            # the rows of the lower half gather from these 512 columns: a table-in-LDS group
# (seg_len, planted set): which of the lengths 0, 1, L-1, L, L+1, 2L-1, 2L, 2L+1, 7L, 8L+1 are planted, and where.  Across the
# five cases: segment counts 25, 28, 9, 16, 9 (1 and 0 modulo 4) and 6, 7, 4, 5, 1 cut rows (segments and fix-up rows go four to a
# workgroup).  Cut rows sit at row 0, at the last row and on both sides of the block border 63 | 64 and of the group border 1023 | 1024.
SEG_CASES = {
    "64-all": (64, ("0", "1", "L-1", "L", "L+1", "2L-1", "2L", "2L+1", "7L", "8L+1")),
    "128-all-twice": (128, ("0", "1", "L-1", "L", "L+1", "2L-1", "2L", "2L+1", "7L", "8L+1", "2L+1 again")),
    "2048-to-2L+1": (2048, ("0", "1", "L-1", "L", "L+1", "2L-1", "2L", "2L+1")),
    "64-no-8L+1": (64, ("0", "1", "L-1", "L", "L+1", "2L-1", "2L", "2L+1", "7L")),
    "128-one-cut-row": (128, ("0", "1", "L-1", "L", "8L+1")),
}
SEG_EXPECT = {"64-all": (6, 25), "128-all-twice": (7, 28), "2048-to-2L+1": (4, 9), "64-no-8L+1": (5, 16), "128-one-cut-row": (1, 9)}
_SEG_ROW = {"8L+1": 0, "0": 5, "1": 6, "L+1": 63, "2L": 64, "L-1": 300, "L": 301, "2L-1": 1023, "7L": 1024, "2L+1 again": 1500,
            "2L+1": SEG_N - 1}


def seg_planted(name):
    """{row: entries} of the planted rows of a segment case."""
    L, chosen = SEG_CASES[name]
    length = {"0": 0, "1": 1, "L-1": L - 1, "L": L, "L+1": L + 1, "2L-1": 2 * L - 1, "2L": 2 * L, "2L+1": 2 * L + 1, "7L": 7 * L,
              "8L+1": 8 * L + 1, "2L+1 again": 2 * L + 1}
    return {_SEG_ROW[c]: length[c] for c in chosen}


@functools.lru_cache(maxsize=None)
def seg_case(name):
    """2048 x 2048: 4 random entries per row - the upper 1024 rows over all columns (a sliceable group of 1024 rows), the lower 1024
    rows within 512 columns (a table-in-LDS group) - and the planted rows of SEG_CASES[name], each within its group's columns."""
    half = SEG_N // 2
    parts = [(0, half, 4, 0, SEG_N - 1), (half, SEG_N, 4, *SEG_TABLE_COLS)]
    planted = []
    for r, n in sorted(seg_planted(name).items()):
        lo, hi = (0, SEG_N - 1) if r < half else SEG_TABLE_COLS
        planted.append((r, n, lo, hi))
    c = _assemble(SEG_CASES[name][0] + len(name), SEG_N, SEG_N, parts, planted, width=orc.TABLE_WIDTH)
    c["seg_len"] = SEG_CASES[name][0]
    return c


# ---- part 3: row groups ----------------------------------------------------------------------------------------------------------
WIDE = 16384                           # with slice_max_mb = 1 a block may gather from 8 192 columns: [0, WIDE) is "neither"
GROUP_EXPECT = {                       # the groups every case was built to produce
    "table512_513": [(0, 512, "T"), (512, 1024, "S")],
    "demoted": [(0, 640, "S")],
    "alternating": [(0, 128, "T"), (128, 256, "N"), (256, 384, "T"), (384, 484, "S")],
    "sliceable960": [(0, 128, "T"), (128, 1088, "S")],
    "sliceable1024": [(0, 128, "T"), (128, 1152, "S")],
    "absorbed": [(0, 2304, "S"), (2304, 3328, "N")],
    "absorbed_first": [(0, 1280, "S")],
    "empty_blocks": [(0, 320, "S"), (320, 448, "T"), (448, 548, "S")],
    "seoul": [(0, 5824, "T"), (5824, 5940, "S")],
    "rows65536": [(0, 64, "T"), (64, 65536, "S")],
    "rows65537": [(0, 65537, "S")],
}
SEOUL_USERS, SEOUL_ITEMS = 5840, 100


def _seoul_shaped():
    """5 840 user rows of 8..16 entries into the 100 item columns, 100 item rows of 600..800 entries into the user columns (cut
    rows): block 91 (rows 5 824..5 887) holds 16 user rows and 48 item rows."""
    rng = np.random.default_rng(5940)
    rows, cols = [], []
    for u in range(SEOUL_USERS):
        c = SEOUL_USERS + rng.choice(SEOUL_ITEMS, int(rng.integers(8, 17)), replace=False)
        rows.append(np.full(c.size, u)), cols.append(c)
    for i in range(SEOUL_ITEMS):
        c = rng.choice(SEOUL_USERS, int(rng.integers(600, 801)), replace=False)
        rows.append(np.full(c.size, SEOUL_USERS + i)), cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    N = SEOUL_USERS + SEOUL_ITEMS
    return {"rows": rows.astype(np.int64), "cols": cols.astype(np.int64), "vals": rng.integers(1, 4, rows.size).astype(np.int64),
            "n_rows": N, "n_cols": N, "table": _table(N, 96, 5941), "slice_max_mb": 48}


@functools.lru_cache(maxsize=None)
def group_case(name):
    """A matrix built for the groups GROUP_EXPECT[name]; 'slice_max_mb' is the library option its plan is to be built under."""
    if name == "table512_513":         # 512 gathered columns: a table group; 513 in every block: none.  A cut row in the table group
        c = _assemble(1, 1024, 4096, [(0, 512, 6, 100, 611), (512, 1024, 6, 2000, 2512)], [(5, 150, 100, 611)])
    elif name == "demoted":            # ten table blocks in a row - eight of 300 columns, 100 apart, two of 101 - whose union is 3 051 wide
        c = _assemble(2, 640, 4096, [(64 * b, 64 * b + 64, 6, 50 + 100 * b, 349 + 100 * b) for b in range(8)] + [(512, 640, 6, 3000, 3100)])
    elif name == "alternating":        # table / neither / table of exactly 512 / sliceable, ending in the middle of block 7
        c = _assemble(3, 484, WIDE, [(0, 128, 6, 300, 700), (128, 256, 6, 0, WIDE - 1), (256, 384, 6, 5000, 5511), (384, 484, 6, 1000, 5000)],
                      [(130, 200, 0, WIDE - 1), (483, 100, 1000, 5000)])
        c["slice_max_mb"] = 1
    elif name in ("sliceable960", "sliceable1024"):
        n = int(name[9:])
        c = _assemble(n, 128 + n, 2048, [(0, 128, 6, 10, 200), (128, 128 + n, 6, 0, 2047)], [(500, 300, 0, 2047)])
    elif name == "absorbed":           # 4 "neither" blocks between two sliceable groups of 16 blocks; 16 "neither" blocks stay
        c = _assemble(4, 3328, WIDE, [(0, 1024, 4, 0, 4000), (1024, 1280, 4, 0, WIDE - 1), (1280, 2304, 4, 6000, 12000),
                                      (2304, 3328, 4, 0, WIDE - 1)], [(1100, 130, 0, WIDE - 1)])
        c["slice_max_mb"] = 1
    elif name == "absorbed_first":     # the small group comes first: it takes its right neighbour's class
        c = _assemble(5, 1280, WIDE, [(0, 256, 4, 0, WIDE - 1), (256, 1280, 4, 0, 4000)])
        c["slice_max_mb"] = 1
    elif name == "empty_blocks":       # three empty blocks in the middle (they join the sliceable group), 100 empty rows at the end
        c = _assemble(6, 548, 2048, [(0, 128, 6, 0, 2047), (320, 448, 6, 100, 300)])
    elif name == "seoul":
        c = _seoul_shaped()
    else:                              # 64-row blocks up to 65 536 rows, 1 024-row blocks beyond: the table block [0, 64) exists only in the first
        n = int(name[4:])
        c = _assemble(n, n, n, [(0, 64, 2, 100, 400), (64, n, 2, 0, n - 1)], [(n - 1, 200, 0, n - 1)], width=64)
    order = np.argsort(c["rows"], kind="stable")
    for k in ("rows", "cols", "vals"):
        c[k] = c[k][order]
    return c


# ---- part 4: masks of thinned copies ---------------------------------------------------------------------------------------------
THIN_SEED = 20260
THIN_KS = ("0", "1", "L-1", "L", "L+1", "2L", "all")
THIN_MASKS = [f"{style}-{k}" for k in THIN_KS for style in ("first", "spread") if not (style == "spread" and k in ("0", "all"))]


def thin_mask(case, seg_len, name):
    """Keep flags by rule: a cut row (more than seg_len entries) keeps k of its entries - the first k, or k spread evenly over the
    row - for k in 0, 1, L-1, L, L+1, 2L, all (at most the row's length); the other rows keep what a hash mask at p = 0.3 leaves."""
    style, k = name.split("-", 1)
    L = seg_len
    want = {"0": 0, "1": 1, "L-1": L - 1, "L": L, "L+1": L + 1, "2L": 2 * L, "all": None}[k]
    keep = orc.keep_mask(case["rows"], case["cols"], [THIN_SEED], 0.3)
    rp, lens = rowptr(case), row_lengths(case)
    for r in np.flatnonzero(lens > L):
        n = int(lens[r])
        kk = n if want is None else min(want, n)
        idx = np.arange(kk) if style == "first" else (np.arange(kk) * n) // max(kk, 1)
        keep[rp[r]:rp[r + 1]] = False
        keep[rp[r] + idx] = True
    return keep


def thinned_arrays(case, keep):
    """(rowptr, colidx, vals, pos) a thinned copy must hold: the kept entries in order; pos[e] = kept entries before e."""
    rows = case["rows"][keep]
    rp = np.r_[0, np.cumsum(np.bincount(rows, minlength=case["n_rows"]))].astype(np.int64)
    pos = np.r_[0, np.cumsum(keep)].astype(np.int32)
    return rp, case["cols"][keep].astype(np.int32), case["vals"][keep].astype(np.float32), pos


def cut_row_states(case, seg_len, keep):
    """How the cut rows of the source come out under `keep`: the set of 'full' (still cut, every segment non-empty), 'trailing_empty'
    (still cut, some segments empty), 'at_L', 'at_L+1', 'twice' (1..L entries: the row kernels and the fix-up both write it),
    'emptied'."""
    lens = row_lengths(case)
    kept = np.bincount(case["rows"][keep], minlength=case["n_rows"])
    out = set()
    for r in np.flatnonzero(lens > seg_len):
        n_seg, k = -(-int(lens[r]) // seg_len), int(kept[r])
        if k == 0:
            out.add("emptied")
        elif k <= seg_len:
            out.add("twice")
        if k == seg_len:
            out.add("at_L")
        if k == seg_len + 1:
            out.add("at_L+1")
        if k > seg_len:
            out.add("full" if k > (n_seg - 1) * seg_len else "trailing_empty")
    return out


# ---- part 5: swept and row-wise groups in one product ----------------------------------------------------------------------------
MIXED_A_ROWS, MIXED_A_DEG, MIXED_COLS = 32768, 136, 40000
MIXED_B_ROWS, MIXED_B_COLS = 1536, (20000, 20095)
MIXED_LONG = ((MIXED_A_ROWS + 5, 2049), (MIXED_A_ROWS + 700, 5000), (MIXED_A_ROWS + MIXED_B_ROWS - 2, 4097),
              (MIXED_A_ROWS + MIXED_B_ROWS - 1, 2050))      # rows of group B longer than the default seg_len of 2 048


@functools.lru_cache(maxsize=None)
def mixed_case():
    """Group A: 32 768 rows of 136 random columns out of 40 000 (4.46 M entries: the swept plan of mode 3 takes it); group B: 1 536 rows
    that gather from 96 columns (a table-in-LDS group, far too small for the plan) with four rows beyond seg_len, two of them last."""
    n = MIXED_A_ROWS + MIXED_B_ROWS
    c = _assemble(55, n, MIXED_COLS, [(0, MIXED_A_ROWS, MIXED_A_DEG, 0, MIXED_COLS - 1), (MIXED_A_ROWS, n, 12, *MIXED_B_COLS)],
                  [(r, k, *MIXED_B_COLS) for r, k in MIXED_LONG], width=130)
    return c


def spmm_exact_blocked(case, width, keep=None, block=8):
    """dropout_oracle.spmm_exact over `block` table columns at a time (a few hundred MB of temporaries at 4.5 M entries)."""
    out = np.empty((case["n_rows"], width), np.int64)
    for c0 in range(0, width, block):
        out[:, c0:c0 + block] = orc.spmm_exact(case["rows"], case["cols"], case["vals"], case["table"][:, c0:min(width, c0 + block)], keep,
                                               n_rows=case["n_rows"])
    return out
