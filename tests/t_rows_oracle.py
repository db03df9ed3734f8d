"""Host oracles and branch-point cases of the row-sparse transposed product out = init + L^T . X (ngcf_spmm_t_rows_f32,
csrc/spmm_t_rows.hip), in plain numpy: written from include/ngcf_hip.h and the comments of the two kernels, no code shared with the
product, nothing here runs on a GPU.  tests/test_t_rows_oracle.py checks this file on the CPU; tests/test_t_rows_paths_gpu.py holds
both kernels - one wave per row on the slot table, and 16 rows per wave with the membership bitmap in LDS - to it.

(a) exact_product: integer data as in tests/dropout_oracle.py (matrix values in {1, 2, 3}, X and init in +-{1..8}); every fp32
    partial sum is an integer below 2^24, so a kernel must EQUAL the int64 product whatever its order.
(b) order_product: the header promises every sum "in entry order".  Non-integer data with 8-bit significands, whose products and
    running sums are exact in float64 - proven step by step with a TwoSum error term of 0 - so float32(float64(v) * float64(x) +
    float64(acc)) is rounded once and IS fmaf(v, x, acc).  The data is chosen so that fp32 does round (the sum in reverse order
    differs): a kernel that adds the same hits in another order, or without fma, fails.
(c) walk: a model of the bitmap kernel's control flow that counts how often each branch is taken; a case is only worth its name
    when the model says it reaches the branches it was built for (tests/test_t_rows_oracle.py asserts that).
(d) the named cases."""
import collections
import functools

import numpy as np

import dropout_oracle as orc

# the constants of spmm_t_rows_bm_kernel (csrc/spmm_t_rows.hip), as literals on purpose
UNIT_ROWS = 16          # kTrRows: consecutive rows a wave takes
WINDOW = 512            # 64 lanes x kTrU = 8 loads: entries scanned at a time
LIST = 84               # kTrList: parked hits per wave
GROUP = 8               # kTrGroup: hits whose X rows are loaded together
CHUNK = 32              # kTrChunk: units a workgroup takes from the device-wide counter
WORKGROUPS = 256        # kTrWGs
WAVES = 16              # kTrWaves
PANEL = 512             # columns per launch; kTrPanels = 8 counters
PANELS = 8
LDS_BYTES = 160 * 1024  # kTrLdsBytes
MIN_NNZ = 1 << 22       # stored entries from which option value 1 takes the bitmap kernel


def lds_bytes(n):
    """t_rows_lds_bytes: the bitmap (one bit per row, in 16-byte pieces), 16 hit lists of 84 16-byte entries, the unit pool."""
    return 4 * ((n + 127) // 128 * 4 + WAVES * LIST * 4) + 16


LDS_MAX_N = 1138560     # the largest N with lds_bytes(N) <= LDS_BYTES (asserted in tests/test_t_rows_oracle.py)


def fits(n, d):
    """The conditions of the bitmap kernel other than the option, the number of stored entries and the workspace."""
    return lds_bytes(n) <= LDS_BYTES and d <= PANEL * PANELS


# ---- (a) exact product -----------------------------------------------------------------------------------------------------------
def entry_rows(case):
    return np.repeat(np.arange(case["n"], dtype=np.int64), np.diff(case["rowptr"]))


def kept_hits(case, seeds=(), p=0.0):
    """Flags of the stored entries (c, r, v) that take part: slot[r] >= 0 and kept by the host mask (keyed by the entry of L)."""
    keep = case["slot"][case["colidx"]] >= 0
    if seeds and p > 0:
        keep &= orc.keep_mask(entry_rows(case), case["colidx"], seeds, p, transposed=True)
    return keep


def exact_product(case, X, init=None, seeds=(), p=0.0):
    """int64 [N, d]: (slot[c] >= 0 ? init[slot[c]] : 0) + sum of v * X[slot[r]] over the kept hits of row c."""
    keep = kept_hits(case, seeds, p)
    rows, cols, vals = entry_rows(case)[keep], case["colidx"][keep], case["vals"][keep]
    out = orc.spmm_exact(rows, case["slot"][cols], vals, X, None, n_rows=case["n"])
    absolute = orc.spmm_exact(rows, case["slot"][cols], vals, np.abs(X), None, n_rows=case["n"])
    if init is not None:
        out[case["sel"]] += init
        absolute[case["sel"]] += np.abs(init)
    assert np.abs(out).max(initial=0) < 2 ** 24 and absolute.max(initial=0) < 2 ** 24     # every partial sum in any order, too
    return out


def int_inputs(case, width, salt=0):
    """X and init, int64 [R, width] in +-{1..8}."""
    rng = np.random.default_rng(1000 + case["n"] + 7 * salt)
    R = case["sel"].size
    draw = lambda: rng.integers(1, 9, (R, width)) * rng.choice(np.array([-1, 1]), (R, width))  # noqa: E731
    return draw(), draw()


# ---- (b) order oracle ------------------------------------------------------------------------------------------------------------
def _significand_bits_8(a):
    m, _ = np.frexp(np.asarray(a, dtype=np.float64))
    return bool((m * 256 == np.rint(m * 256)).all())


def fma32(v, x, acc):
    """fmaf(v, x, acc) on float32 arrays: the product of two 8-bit significands is exact in float64 (16 bits); the sum with acc is
    exact too - TwoSum's error term is asserted to be 0 - so the rounding to float32 is the only one."""
    p = v.astype(np.float64) * x.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    assert not err.any(), "the float64 sum is not exact: the inputs are outside the oracle's range"
    return s.astype(np.float32)


def float_inputs(case, width, salt=0):
    """vals float32 [nnz] > 0, X and init float32 [R, width]: significands of 8 bits, exponents within 2^-12 .. 2^-6 of 128..255."""
    rng = np.random.default_rng(2000 + case["n"] + 7 * salt)
    R = case["sel"].size

    def draw(shape, signed):
        a = rng.integers(128, 256, shape) * np.exp2(rng.integers(-12, -5, shape).astype(np.float64))
        return (a * rng.choice(np.array([-1.0, 1.0]), shape) if signed else a).astype(np.float32)
    return draw(case["colidx"].shape, False), draw((R, width), True), draw((R, width), True)


def order_product(case, vals, X, init=None, keep=None, reverse=False):
    """float32 [N, d] as the header states it: per row c, acc = init[slot[c]] or 0, then acc = fmaf(v, x, acc) for each kept hit in
    entry order.  A row of more than seg_len entries is summed segment by segment (seg_len entries each, only the first starts from
    init) and its result is 0 + p0 + p1 + ... in segment order (spmm_fixup_kernel).  Vectorised over sums and columns, a loop over
    the hit position.  `reverse`: the hits of every sum in reverse order (for the CPU test that shows the data rounds)."""
    assert vals.dtype == X.dtype == np.float32 and _significand_bits_8(vals) and _significand_bits_8(X)
    assert init is None or (init.dtype == np.float32 and _significand_bits_8(init))
    n, rp, col, slot, L = case["n"], case["rowptr"], case["colidx"], case["slot"], case["seg_len"]
    d = X.shape[1]
    lens = np.diff(rp)
    rows = entry_rows(case)
    seg = np.where(lens[rows] > L, (np.arange(col.size) - rp[rows]) // L, 0)
    hit = slot[col] >= 0 if keep is None else (slot[col] >= 0) & keep
    e = np.flatnonzero(hit)
    key = rows[e] * (1 << 32) + seg[e]                                # one sum per (row, segment); entries are in order already
    ukey, start, count = np.unique(key, return_index=True, return_counts=True)
    urow, useg = ukey >> 32, ukey & 0xFFFFFFFF

    def start_value(r, s):
        """[len(r), d]: the init row of the sums that open a row of R."""
        acc = np.zeros((r.size, d), np.float32)
        if init is not None:
            opens = (s == 0) & (slot[r] >= 0)
            acc[opens] = init[slot[r[opens]]]
        return acc
    acc = start_value(urow, useg)
    for k in range(int(count.max(initial=0))):
        live = np.flatnonzero(count > k)
        at = e[start[live] + (count[live] - 1 - k if reverse else k)]
        acc[live] = fma32(vals[at][:, None], X[slot[col[at]]], acc[live])
    out = start_value(np.arange(n), np.zeros(n, np.int64))            # rows without a kept hit: init or zero
    whole = lens[urow] <= L
    out[urow[whole]] = acc[whole]
    for r in np.flatnonzero(lens > L):
        n_seg = -(-int(lens[r]) // L)
        part = start_value(np.full(n_seg, r), np.arange(n_seg))
        mine = np.flatnonzero(urow == r)
        part[useg[mine]] = acc[mine]
        total = np.zeros(d, np.float32)
        for s in range(n_seg):
            total = (total + part[s]).astype(np.float32)
        out[r] = total
    return out


# ---- (c) walk model of spmm_t_rows_bm_kernel -------------------------------------------------------------------------------------
def walk(rowptr, colidx, slot, seg_len):
    """Event counts of one launch (a collections.Counter; dropout does not change them: a dropped hit is parked like any other).
    A wave takes a unit of 16 rows; rows longer than seg_len are cut (their segments are walked 64 entries at a time elsewhere) and
    split the unit into runs of live rows; a run's entries are scanned in windows of 512; a window's hits are parked in a list of 84
    unless there are more than 84 (then applied one by one); the list is drained - eight hits at a time - before a window that would
    overflow it and at the end of the run."""
    ev = collections.Counter()
    rp = np.asarray(rowptr, dtype=np.int64)
    n = rp.size - 1
    lens = np.diff(rp)
    h = np.asarray(slot)[np.asarray(colidx, dtype=np.int64)] >= 0
    H = np.r_[0, np.cumsum(h)].astype(np.int64)
    row_hits = H[rp[1:]] - H[rp[:-1]]
    in_R = np.asarray(slot)[:n] >= 0
    n_units = (n + UNIT_ROWS - 1) // UNIT_ROWS
    ev["units"], ev["chunks"] = n_units, (n_units + CHUNK - 1) // CHUNK
    ev["row_len_eq_seg_len"] = int((lens == seg_len).sum())
    ev["row_len_seg_len_plus_1"] = int((lens == seg_len + 1).sum())
    for r in np.flatnonzero(lens > seg_len):
        ev["cut_rows"] += 1
        for b in range(int(rp[r]), int(rp[r + 1]), seg_len):
            ev["segments"] += 1
            ev["segments_without_hit"] += int(H[min(b + seg_len, rp[r + 1])] == H[b])
    for u in range(n_units):
        r0 = u * UNIT_ROWS
        nr = min(UNIT_ROWS, n - r0)
        live = lens[r0:r0 + nr] <= seg_len
        cut = ~live
        ev["short_units"] += int(nr < UNIT_ROWS)
        if cut.any():
            ev["cut_at_0"] += int(cut[0])
            ev["cut_at_15"] += int(nr == UNIT_ROWS and cut[15])
            ev["cut_between_live"] += int(any(cut[k] and live[:k].any() and live[k + 1:].any() for k in range(1, nr - 1)))
            ev["cut_adjacent"] += int((cut[1:] & cut[:-1]).any())
            ev["cut_in_short_unit"] += int(nr < UNIT_ROWS)
            ev["cut_row_in_R"] += int((cut & in_R[r0:r0 + nr]).any())
        if not live.any():
            ev["units_no_live"] += 1
            ev["units_all_16_cut"] += int(nr == UNIT_ROWS)
        edges = np.flatnonzero(np.diff(np.r_[0, live.astype(np.int8), 0]))
        ev[f"runs_per_unit={edges.size // 2}"] += 1
        for ka, kb in zip(edges[::2], edges[1::2]):
            begin, end = int(rp[r0 + ka]), int(rp[r0 + kb])
            ev[f"run_entries={end - begin}"] += 1
            ev["empty_runs"] += int(begin == end)
            rh, rin, rl = row_hits[r0 + ka:r0 + kb], in_R[r0 + ka:r0 + kb], lens[r0 + ka:r0 + kb]
            lone = rin & (rh == 0)
            ev["init_no_hit_rows"] += int(lone.sum())
            ev["init_no_hit_at_run_start"] += int(lone[0])
            ev["init_no_hit_at_run_end"] += int(lone.size > 1 and lone[-1])
            ev["init_no_hit_in_run_middle"] += int(lone[1:-1].any())
            ev["run_first_row_no_hit"] += int(rh[0] == 0)
            with_hit = np.flatnonzero(rh > 0)
            if with_hit.size >= 2:
                between = np.arange(with_hit[0], with_hit[-1] + 1)
                ev["no_hit_rows_between_hits"] += int((rh[between] == 0).sum())
                ev["empty_rows_between_hits"] += int((rl[between] == 0).sum())
            for r in range(ka + 1, kb):                              # a row that begins exactly where a window begins
                b = int(rp[r0 + r]) - begin
                if 0 < b < end - begin and b % WINDOW == 0 and lens[r0 + r] > 0 and rp[r0 + r] > rp[r0 + r - 1]:
                    ev["row_starts_on_window_boundary"] += 1
                    ev["hit_row_change_on_window_boundary"] += int(h[begin + b] and h[begin + b - 1])
            n_list, prev = 0, None
            for base in range(begin, end, WINDOW):
                top = min(base + WINDOW, end)
                n_new = int(H[top] - H[base])
                ev[f"window_hits={n_new}"] += 1
                ev["hit_last_of_window"] += int(top - base == WINDOW and top < end and h[top - 1])
                ev["hit_first_of_window"] += int(base > begin and h[base])
                if n_list > 0 and n_list + n_new > LIST:
                    ev["drains_forced"] += 1
                    ev[f"forced_at={n_list + n_new}"] += 1
                    ev[f"drain_mod8={n_list % GROUP}"] += 1
                    n_list = 0
                if n_new > LIST:
                    ev["windows_one_by_one"] += 1
                    ev["one_by_one_after_parked"] += int(prev == "parked")
                    prev = "one"
                elif n_new > 0:
                    ev["windows_parked"] += 1
                    n_list += n_new
                    ev["list_exactly_full"] += int(n_list == LIST)
                    prev = "parked"
                else:
                    ev["windows_without_hit"] += 1
                    prev = None
            if n_list > 0:
                ev["drains_end"] += 1
                ev[f"end_drain={n_list}"] += 1
                ev[f"drain_mod8={n_list % GROUP}"] += 1
    return ev


def panels(d):
    """Launches (and panel counters) a product of width d takes."""
    return (d + PANEL - 1) // PANEL


# ---- (d) named cases -------------------------------------------------------------------------------------------------------------
def _finish(name, n, rowptr, colidx, vals, sel, seg_len, built_for):
    sel = np.unique(np.asarray(sel, dtype=np.int64))
    slot = np.full(n, -1, np.int32)
    slot[sel] = np.arange(sel.size, dtype=np.int32)
    c = {"name": name, "n": int(n), "rowptr": np.asarray(rowptr, np.int64), "colidx": np.asarray(colidx, np.int64),
         "vals": np.asarray(vals, np.int64), "slot": slot, "sel": sel, "seg_len": int(seg_len), "built_for": tuple(built_for)}
    assert c["rowptr"][-1] == c["colidx"].size == c["vals"].size and (c["colidx"] < n).all() and (c["colidx"] >= 0).all()
    for a in ("rowptr", "colidx", "vals", "slot", "sel"):
        c[a].setflags(write=False)
    return c


def _from_patterns(name, n, patterns, sel, seg_len, seed, built_for):
    """patterns: {row: bool array, True = a hit (a column of R), False = a miss}; the other rows get 0..6 entries, a third of them
    hits.  Columns are drawn at random among the rows of R / the other rows."""
    rng = np.random.default_rng(seed)
    sel = np.unique(np.asarray(sel, dtype=np.int64))
    rest = np.setdiff1d(np.arange(n), sel)
    cols, lens = [], np.zeros(n, np.int64)
    for r in range(n):
        pat = patterns.get(r)
        if pat is None:
            pat = rng.random(int(rng.integers(0, 7))) < 0.33
        pat = np.asarray(pat, dtype=bool)
        if sel.size == 0 or rest.size == 0:
            c = np.full(pat.size, (sel if sel.size else rest)[0])
        else:
            c = np.where(pat, rng.choice(sel, pat.size), rng.choice(rest, pat.size))
        cols.append(c)
        lens[r] = pat.size
    colidx = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    return _finish(name, n, np.r_[0, np.cumsum(lens)], colidx, rng.integers(1, 4, colidx.size), sel, seg_len, built_for)


def _flags(rng, length, hits, first=None, last=None):
    """`length` entries with exactly `hits` hits at random places; first / last: force that entry to be a hit or a miss."""
    f = np.zeros(length, bool)
    free = np.arange(length)
    if first is not None:
        f[0], hits, free = first, hits - int(first), free[1:]
    if last is not None:
        f[-1], hits, free = last, hits - int(last), free[:-1]
    f[rng.choice(free, hits, replace=False)] = True
    return f


def _split(rng, flags, n_rows=UNIT_ROWS, cuts=None):
    """One stretch of entries as the patterns of n_rows consecutive rows (random row boundaries, empty rows allowed)."""
    if cuts is None:
        cuts = np.sort(rng.integers(0, flags.size + 1, n_rows - 1))
    return np.split(flags, cuts)


def _select(rng, n, share=0.25):
    return np.unique(np.r_[rng.choice(n, max(1, int(n * share)), replace=False), 0, n - 1])


def _rows_case(n):
    """Random small matrices whose row count puts the last unit and the chunks on their edges."""
    rng = np.random.default_rng(n)
    built = {1: ["short_units"], 15: ["short_units"], 16: [], 17: ["short_units"], 512: [], 513: ["short_units"]}[n]
    if n == 1:
        return _from_patterns("rows_1", 1, {0: [True, True, True]}, [0], 64, 1, built)
    return _from_patterns(f"rows_{n}", n, {}, _select(rng, n), 64, n, built)


REFILL_UNITS = 2 * WORKGROUPS * CHUNK + 9


def _refill_case():
    """More than 2 x 256 x 32 units of rows with one or two entries: every workgroup takes a second chunk that holds units."""
    n = REFILL_UNITS * UNIT_ROWS - 13
    rng = np.random.default_rng(8192)
    lens = rng.integers(1, 3, n)
    sel = _select(rng, n, 3000 / n)
    colidx = rng.integers(0, n, int(lens.sum()))
    at_hit = rng.random(colidx.size) < 0.05
    colidx[at_hit] = rng.choice(sel, int(at_hit.sum()))
    return _finish("rows_refill", n, np.r_[0, np.cumsum(lens)], colidx, rng.integers(1, 4, colidx.size), sel, 64, ["short_units"])


def _units_case(name, units, seg_len, seed, built_for, tail_rows=0, fillers=4, forced_sel=()):
    """`units`: lists of 16 row patterns (or None for a random filler unit), laid out unit after unit with `fillers` random units
    around them and `tail_rows` rows of a ragged last unit given as patterns in `units[-1]` when tail_rows > 0."""
    rng = np.random.default_rng(seed)
    patterns, r = {}, 0
    blocks = [None] * fillers + list(units) + ([None] * fillers if not tail_rows else [])
    for blk in blocks:
        if blk is not None:
            for k, pat in enumerate(blk):
                patterns[r + k] = pat
            r += len(blk)
        else:
            r += UNIT_ROWS
    n = r
    assert (n % UNIT_ROWS == tail_rows % UNIT_ROWS)
    sel = np.unique(np.r_[_select(rng, n), np.asarray(forced_sel, dtype=np.int64) + fillers * UNIT_ROWS])
    keep_out = np.asarray([x + fillers * UNIT_ROWS for x in built_for.get("not_in_R", ())], dtype=np.int64)
    sel = np.setdiff1d(sel, keep_out)
    return _from_patterns(name, n, patterns, sel, seg_len, seed, built_for["events"])


def _windows_case():
    """seg_len 2048 (no cut row): units whose single run is 0, 1, 511, 512, 513 and 1024 entries long; in the last a row boundary
    sits on entry 512 with a hit on either side of it; in the 513 one the hits 511 | 512 belong to one row."""
    rng = np.random.default_rng(512)
    F = lambda length, hits, **kw: _flags(rng, length, hits, **kw)  # noqa: E731
    units = [
        [np.zeros(0, bool)] * 16,
        _split(rng, F(1, 1), cuts=[0] * 5 + [1] * 10),
        _split(rng, F(511, 7)),
        _split(rng, F(512, 9, last=True)),
        _split(rng, np.r_[F(512, 6, last=True), F(1, 1)], cuts=[100, 300] + [513] * 13),
        _split(rng, np.r_[F(512, 5, last=True), F(512, 4, first=True)], cuts=[200, 512, 700] + [1024] * 12),
    ]
    return _units_case("windows", units, 2048, 512, {"events": [
        "run_entries=0", "run_entries=1", "run_entries=511", "run_entries=512", "run_entries=513", "run_entries=1024",
        "row_starts_on_window_boundary", "hit_row_change_on_window_boundary", "hit_last_of_window", "hit_first_of_window", "empty_runs"]})


HITS_WINDOWS = [                 # hits per window of a unit's run, (.., n): the last window is n entries long
    ([84], 512),                 # fills the list exactly; no forced drain; the end drains 84
    ([40, 44, 1], 512),          # 40 + 44 = 84: parked; + 1 = 85: drained first; the end drains 1
    ([85, 0, 512, 8], 512),      # one by one, nothing, one by one, the end drains 8
    ([9], 512),                  # the end drains 9: a group of eight and a group of one
    ([30, 100, 0, 1], 512),      # a one-by-one window behind a parked one: the 30 are drained first
    ([50, 35], 512),             # 85: drained first, the 35 follow in order
    ([84, 84], 512),             # full, drained, full again
    ([3, 0, 5], 300),            # the end drains 8 hits parked by two windows
    ([20, 7], 100),              # a short last window
]


def _hits_case():
    rng = np.random.default_rng(84)
    units = []
    for counts, last_len in HITS_WINDOWS:
        flags = np.concatenate([_flags(rng, last_len if i == len(counts) - 1 else WINDOW, c) for i, c in enumerate(counts)])
        units.append(_split(rng, flags))
    return _units_case("hits", units, 2048, 84, {"events": [
        "window_hits=0", "window_hits=1", "window_hits=84", "window_hits=85", "window_hits=512", "list_exactly_full", "forced_at=85",
        "drains_forced", "end_drain=1", "end_drain=8", "end_drain=9", "end_drain=84", "one_by_one_after_parked", "windows_one_by_one",
        "windows_parked", "drain_mod8=0", "drain_mod8=1", "drain_mod8=4"]})


def _runs_case():
    """seg_len 64: cut rows (65 .. 200 entries, a third of them hits) at position 0, at 15, in the middle, two in a row, all 16,
    one in the ragged last unit; a row of exactly 64 entries (not cut) and one of 65 (cut); a run without entries between two cut
    rows; cut rows in R (their init rides the first segment) and outside R."""
    rng = np.random.default_rng(64)
    short = lambda: rng.random(int(rng.integers(0, 11))) < 0.33      # noqa: E731
    long = lambda k: rng.random(k) < 0.33                              # noqa: E731

    def unit(cuts, n_rows=UNIT_ROWS, empty=()):
        return [long(cuts[k]) if k in cuts else np.zeros(0, bool) if k in empty else short() for k in range(n_rows)]
    units = [
        unit({0: 130}),
        unit({15: 70}),
        unit({7: 200}),
        unit({4: 129, 5: 128}),
        unit({k: 65 + 9 * k for k in range(16)}),
        unit({3: 64, 9: 65}),
        unit({0: 100, 3: 90}, empty=(1, 2)),
        unit({2: 150}, n_rows=5),
    ]
    forced = [0, 16 + 15, 3 * 16 + 4, 4 * 16 + 2, 5 * 16 + 9, 7 * 16 + 2]          # cut rows that are in R
    return _units_case("runs", units, 64, 64, {"events": [
        "cut_at_0", "cut_at_15", "cut_between_live", "runs_per_unit=2", "runs_per_unit=0", "cut_adjacent", "units_all_16_cut",
        "cut_in_short_unit", "cut_row_in_R", "row_len_eq_seg_len", "row_len_seg_len_plus_1", "empty_runs", "segments", "short_units"],
        "not_in_R": [2 * 16 + 7, 6 * 16 + 3]}, tail_rows=5, forced_sel=forced)


def _init_case():
    """seg_len 64: rows of R without a hit at the start, in the middle and at the end of a run; empty rows between two hit rows; runs
    whose first row has no hit; a run that starts behind a cut row with such a row."""
    rng = np.random.default_rng(7)
    hit = lambda k=4: np.r_[True, rng.random(k) < 0.4]                 # noqa: E731  (at least one hit)
    miss = lambda k=3: np.zeros(k, bool)                               # noqa: E731
    none = lambda: np.zeros(0, bool)                                   # noqa: E731
    units = [
        [miss(), hit(), none(), none(), hit(), miss(), none(), hit(), hit(), none(), miss(2), hit(), none(), none(), hit(), miss()],
        [none(), none(), hit(), rng.random(100) < 0.3, miss(), hit(), none(), hit(), none(), none(), none(), none(), none(), none(), none(), none()],
        [hit()] + [none()] * 14 + [hit()],
        [miss()] * 16,
    ]
    in_R = [0, 3, 5, 6, 15, 16 + 0, 16 + 4, 16 + 6, 16 + 15, 32 + 5, 32 + 6, 48 + 0, 48 + 8, 48 + 15]
    out_R = [2, 9, 16 + 1, 32 + 1]
    return _units_case("init", units, 64, 7, {"events": [
        "init_no_hit_at_run_start", "init_no_hit_in_run_middle", "init_no_hit_at_run_end", "empty_rows_between_hits",
        "no_hit_rows_between_hits", "run_first_row_no_hit", "runs_per_unit=2", "init_no_hit_rows"], "not_in_R": out_R}, forced_sel=in_R)


def _lds_case(n):
    """About two entries per row; R: 3 000 random rows, the first and the last (the last bit of the bitmap); both stored as columns."""
    rng = np.random.default_rng(n % 100003)
    lens = rng.integers(1, 4, n)
    sel = _select(rng, n, 3000 / n)
    colidx = rng.integers(0, n, int(lens.sum()))
    at_hit = rng.random(colidx.size) < 0.02
    colidx[at_hit] = rng.choice(sel, int(at_hit.sum()))
    colidx[:4] = (n - 1, 0, n - 1, 0)
    return _finish(f"lds_{n}", n, np.r_[0, np.cumsum(lens)], colidx, rng.integers(1, 4, colidx.size), sel, 64, [])


LDS_ODD_N = 70001               # a multiple of neither 32 nor 128: the last word of the bitmap is partly used
ROWS_N = (1, 15, 16, 17, 512, 513)
SMALL = tuple(f"rows_{n}" for n in ROWS_N) + ("windows", "hits", "runs", "init")
LARGE = ("rows_refill", f"lds_{LDS_MAX_N}", f"lds_{LDS_MAX_N + 1}", f"lds_{LDS_ODD_N}")
CASES = SMALL + LARGE


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, n, rowptr, colidx, vals, slot, sel, seg_len, built_for): a square CSR of L^T (int64 arrays, values in {1, 2, 3}), the
    slot table of the rows `sel` of R, the seg_len its plan is to be built with (LaplacianCSR.plan) and the walk events it exists
    for.  All arrays are read-only and shared."""
    if name.startswith("rows_") and name != "rows_refill":
        return _rows_case(int(name[5:]))
    if name.startswith("lds_"):
        return _lds_case(int(name[4:]))
    return {"rows_refill": _refill_case, "windows": _windows_case, "hits": _hits_case, "runs": _runs_case, "init": _init_case}[name]()
