"""CPU checks of tests/plan_cases.py: every case has the row lengths, segment counts, row groups and masks it was built for (by the
host formulas of that file, written from cut_rows and build_row_groups of csrc/csr.hip), the swept plan's `declined` answers what
part 5 of tests/test_csr_plan_gpu.py needs (csrc/swept_plan.h, compiled for the host as in tests/test_swept_plan.py), and every
oracle product stays below 2^24."""
import ctypes

import numpy as np
import pytest

import dropout_oracle as orc
import plan_cases as pc
from test_swept_plan import lib  # noqa: F401  (the fixture that compiles csrc/swept_plan.h)


def _bound(case, width=None):
    """Upper bound of |any partial sum| of the case's product: the longest row times the largest value times the largest table value."""
    t = case["table"] if width is None else case["table"][:, :width]
    return int(pc.row_lengths(case).max(initial=0)) * int(case["vals"].max(initial=0)) * int(np.abs(t).max())


def test_host_formulas():
    assert [pc.default_seg_len(n) for n in (0, 262144, 262145, 4 << 20, (8 << 20) + 1, 10 ** 9)] == [64, 64, 128, 1024, 2048, 2048]
    assert pc.segment_plan([0, 1, 64, 65, 128, 129], 64) == (3, 2 + 2 + 3, 129)
    assert pc.segment_plan([], 64) == (0, 0, 0)
    assert pc.slice_footprint_rows() == 393216 and pc.slice_footprint_rows(1) == 8192
    assert pc.block_rows(65536) == 64 and pc.block_rows(65537) == 1024


@pytest.mark.parametrize("name", list(pc.SEG_CASES))
def test_segment_cases(name):
    c = pc.seg_case(name)
    L = c["seg_len"]
    lens = pc.row_lengths(c)
    planted = pc.seg_planted(name)
    assert all(lens[r] == n for r, n in planted.items())
    assert (np.delete(lens, list(planted)) == 4).all()
    assert {0, 1, L - 1, L} <= set(planted.values())
    n_cut, n_seg, longest = pc.segment_plan(lens, L)
    assert (n_cut, n_seg) == pc.SEG_EXPECT[name] and longest == max(planted.values())
    assert n_seg == sum(-(-n // L) for n in planted.values() if n > L)
    # two groups, whatever is planted: a sliceable one of 1024 rows (the sliced kernel's threshold) and a table group; cut rows in both
    assert pc.shape_of(pc.host_groups(c)) == [(0, 1024, "S"), (1024, 2048, "T")]
    cut = np.flatnonzero(lens > L)
    assert (cut < 1024).any() and ((cut >= 1024).any() or n_cut == 1)
    assert c["rows"].size and (np.diff(c["rows"]) >= 0).all()
    assert _bound(c) < 2 ** 24


def test_segment_cases_cover_the_counts():
    counts = [pc.SEG_EXPECT[n] for n in pc.SEG_CASES]
    assert {1, 4, 5} <= {c for c, _ in counts}                     # cut rows: fix-up rows go four to a workgroup
    assert {0, 1} <= {s % 4 for _, s in counts}                    # segments go four to a workgroup
    assert {L for L, _ in pc.SEG_CASES.values()} == {64, 128, 2048}
    every = set().union(*(set(p) for _, p in pc.SEG_CASES.values()))
    assert every >= {"0", "1", "L-1", "L", "L+1", "2L-1", "2L", "2L+1", "7L", "8L+1"}
    # the border cut rows: row 0, the last row, both sides of the block border 63 | 64
    lens = pc.row_lengths(pc.seg_case("64-all"))
    assert all(lens[r] > 64 for r in (0, 63, 64, pc.SEG_N - 1))


@pytest.mark.parametrize("name", list(pc.GROUP_EXPECT))
def test_group_cases(name):
    c = pc.group_case(name)
    groups = pc.host_groups(c, c["slice_max_mb"])
    assert pc.shape_of(groups) == pc.GROUP_EXPECT[name]
    assert groups[0]["begin"] == 0 and groups[-1]["end"] == c["n_rows"]
    assert (np.diff(c["rows"]) >= 0).all() and c["cols"].min() >= 0 and c["cols"].max() < c["n_cols"]
    assert _bound(c) < 2 ** 24
    by = {g["begin"]: g for g in groups}
    lens = pc.row_lengths(c)
    if name == "table512_513":
        assert (by[0]["col_lo"], by[0]["col_hi"]) == (100, 611) and (by[512]["col_lo"], by[512]["col_hi"]) == (2000, 2512)
        assert lens[5] > pc.default_seg_len(c["rows"].size)         # a cut row inside the table group
    if name == "demoted":                                           # every block on its own is a table block
        for b in range(10):
            cols = c["cols"][c["rows"] // 64 == b]
            assert cols.max() - cols.min() + 1 <= pc.LDS_TABLE_ROWS
        assert by[0]["col_hi"] - by[0]["col_lo"] + 1 > pc.LDS_TABLE_ROWS
    if name == "alternating":
        assert c["n_rows"] % 64 != 0 and by[256]["col_hi"] - by[256]["col_lo"] + 1 == 512
        assert by[128]["col_hi"] - by[128]["col_lo"] + 1 > pc.slice_footprint_rows(c["slice_max_mb"])
    if name == "absorbed":                                          # without the absorption the four blocks would be a group
        mid = (c["rows"] >= 1024) & (c["rows"] < 1280)
        assert pc.shape_of(pc.host_groups({**c, "rows": c["rows"][mid] - 1024, "cols": c["cols"][mid], "n_rows": 256}, 1)) == [(0, 256, "N")]
    if name == "empty_blocks":
        assert not lens[128:320].any() and not lens[448:].any() and by[448]["col_hi"] < by[448]["col_lo"]
    if name == "seoul":
        mixed = np.arange(91 * 64, 92 * 64)
        assert (mixed < pc.SEOUL_USERS).any() and (mixed >= pc.SEOUL_USERS).any()
        assert (lens[pc.SEOUL_USERS:] > pc.default_seg_len(c["rows"].size)).all()
    if name.startswith("rows"):
        assert lens[-1] > pc.default_seg_len(c["rows"].size) and (np.delete(lens, -1) == 2).all()
        assert pc.block_rows(c["n_rows"]) == (64 if name == "rows65536" else 1024)


@pytest.mark.parametrize("name", ["S", "St", "W", "Su"])
def test_thin_masks(name):
    c = orc.build_case(name)
    L = pc.default_seg_len(c["rows"].size)
    assert L == 64
    lens, rp = pc.row_lengths(c), pc.rowptr(c)
    cut = np.flatnonzero(lens > L)
    assert (cut.size > 0) == (name != "Su")
    states = set()
    for m in pc.THIN_MASKS:
        keep = pc.thin_mask(c, L, m)
        style, k = m.split("-", 1)
        want = {"0": 0, "1": 1, "L-1": L - 1, "L": L, "L+1": L + 1, "2L": 2 * L, "all": 10 ** 9}[k]
        for r in cut:
            row = keep[rp[r]:rp[r + 1]]
            assert row.sum() == min(want, lens[r])
            if style == "first":
                assert row[:row.sum()].all()
            elif 1 < row.sum() < lens[r] // 2:
                assert not row[:row.sum()].all() and row[0]          # spread over the row, not its head
        short = np.repeat(lens <= L, lens)
        assert np.array_equal(keep[short], orc.keep_mask(c["rows"], c["cols"], [pc.THIN_SEED], 0.3)[short])
        states |= pc.cut_row_states(c, L, keep)
        rp2, ci, va, pos = pc.thinned_arrays(c, keep)
        assert rp2[-1] == keep.sum() == ci.size == va.size == pos[-1] and pos.size == keep.size + 1 and pos[0] == 0
    if name != "Su":
        assert states == {"full", "trailing_empty", "at_L", "at_L+1", "twice", "emptied"}
    assert _bound(c) < 2 ** 24


def test_mixed_case_and_declined(lib):  # noqa: F811
    c = pc.mixed_case()
    groups = pc.host_groups(c)
    n = pc.MIXED_A_ROWS + pc.MIXED_B_ROWS
    assert pc.shape_of(groups) == [(0, pc.MIXED_A_ROWS, "S"), (pc.MIXED_A_ROWS, n, "T")] and n <= 65536
    lens, rp = pc.row_lengths(c), pc.rowptr(c)
    assert (lens[:pc.MIXED_A_ROWS] == pc.MIXED_A_DEG).all() and all(lens[r] == k for r, k in pc.MIXED_LONG)
    L = pc.default_seg_len(c["rows"].size)
    assert L == 2048 and [r for r in np.flatnonzero(lens > L)] == [r for r, _ in pc.MIXED_LONG] and lens[-1] > L and lens[-2] > L
    assert groups[1]["col_hi"] - groups[1]["col_lo"] + 1 == 96
    declined = lambda g, lpe: bool(lib.swept_declined(ctypes.c_int64(g["end"] - g["begin"]),  # noqa: E731
                                                      ctypes.c_int64(int(rp[g["end"]] - rp[g["begin"]])), g["col_lo"], g["col_hi"], lpe, 0))
    for lpe in (16, 32):
        assert not declined(groups[0], lpe) and declined(groups[1], lpe)
    assert _bound(c) < 2 ** 24
