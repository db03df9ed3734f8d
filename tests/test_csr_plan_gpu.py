"""The CSR's host plan at its own branch points (csrc/csr.hip: ngcf_csr_from_coo / _from_arrays, cut_rows, build_row_groups;
csrc/csr_filter.hip: the borrowed plan of a thinned copy; csrc/spmm_swept.hip: swept parts beside row-wise groups), with exact products.

Method of tests/test_dropout_paths_gpu.py: integer-valued matrices and tables (tests/plan_cases.py, tests/dropout_oracle.py), so the
fp32 product must `torch.equal` the host's int64 product (every intermediate below 2^24: tests/test_plan_cases.py); outputs are
prefilled with NaN and nothing outside the [n_rows, d] view may be written.  Every case first asserts the precondition that names its
path: segment and cut-row counts by the host formula, the row groups through LaplacianCSR.groups(), swept_rows."""
import functools

import numpy as np
import pytest
import torch

import dropout_oracle as orc
import plan_cases as pc
from test_csr_filter_gpu import _arrays
from test_dropout_paths_gpu import _assert_exact, _t_rows_inputs, _view

pytestmark = pytest.mark.gpu

SEEDS = (2 ** 62 - 1, 0xC2B2AE3D27D4EB4F)
P = 0.3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _eng():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg.engine


_DEV = {}


def _on_dev(key, case, dev):
    """(rows, cols, vals, table) of a case on the device, once per key."""
    if ("coo", key) not in _DEV:
        _DEV["coo", key] = tuple(torch.from_numpy(case[k]).to(dev) for k in ("rows", "cols")) + (
            torch.from_numpy(case["vals"].astype(np.float32)).to(dev), torch.from_numpy(case["table"].astype(np.float32)).to(dev))
    return _DEV["coo", key]


def _build(key, case, dev):
    """LaplacianCSR.from_coo of a case, once per key (the plan is built under the options in force at the first call)."""
    if ("csr", key) not in _DEV:
        rows, cols, vals, _ = _on_dev(key, case, dev)
        _DEV["csr", key] = _eng().LaplacianCSR.from_coo(rows, cols, vals, case["n_rows"], case["n_cols"])
    return _DEV["csr", key]


def _product(csr, table, d, layout, dev, edge_drop=None):
    """eng.spmm of the first d table columns into a NaN-filled output in the given layout ('aligned' / 'odd', for both operands)."""
    _, E = _view(csr.n_cols, d, layout, dev)
    E.copy_(table[:, :d])
    buf, out = _view(csr.n_rows, d, layout, dev)
    got = _eng().spmm(csr, E, out=out, edge_drop=edge_drop)
    assert got.data_ptr() == out.data_ptr()
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[:, out.storage_offset():out.storage_offset() + d] = False
    assert bool(torch.isnan(buf[outside]).all()), "written outside the d columns of the output"
    return got


def _exact(case, keep=None, width=None):
    t = case["table"] if width is None else case["table"][:, :width]
    out = orc.spmm_exact(case["rows"], case["cols"], case["vals"], t, keep, n_rows=case["n_rows"])
    assert np.abs(out).max(initial=0) < 2 ** 24
    out = out.astype(np.float32)
    out.setflags(write=False)
    return out


def _assert_plan(csr, case, seg_len, slice_max_mb=48):
    """The segment plan by the host formula and the row groups by the host's replay of build_row_groups."""
    n_cut, n_seg, longest = pc.segment_plan(pc.row_lengths(case), seg_len)
    assert (csr.n_segments, csr.max_row_len) == (n_seg, longest)
    assert csr.groups() == pc.host_groups(case, slice_max_mb)
    return n_cut, n_seg


def _assert_arrays(csr, rp, ci, va):
    got_rp, got_ci, got_va = _arrays(csr)
    assert torch.equal(got_rp, torch.from_numpy(np.asarray(rp, np.int64)))
    assert torch.equal(got_ci, torch.from_numpy(np.asarray(ci, np.int32))) and torch.equal(got_va, torch.from_numpy(np.asarray(va, np.float32)))


# ---- 1. CSR arrays ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _coo_input(kind):
    """COO triplets in INPUT order (int64 rows / cols, integer values), 300 x 200, and a table."""
    rng = np.random.default_rng(300)
    n_rows, n_cols = (0, 7) if kind == "none-0-rows" else (5, 3) if kind == "none-5-rows" else (300, 200)
    n = 0 if kind.startswith("none") else 3000
    rows, cols, vals = np.sort(rng.integers(0, max(n_rows, 1), n)), rng.integers(0, n_cols, n), rng.integers(1, 4, n)
    if kind == "swapped":                                  # one pair out of order: the host path
        i, j = 10, 2000
        assert rows[i] != rows[j]
        for a in (rows, cols, vals):
            a[i], a[j] = a[j], a[i]
    if kind == "shuffled-duplicates":                      # every 10th entry stored again with another value, then shuffled
        rows, cols, vals = np.r_[rows, rows[::10]], np.r_[cols, cols[::10]], np.r_[vals, 4 - vals[::10]]
        order = rng.permutation(rows.size)
        rows, cols, vals = rows[order], cols[order], vals[order]
    if kind in ("empty-ends", "empty-ends-unsorted"):      # no entries in rows 0..2 and 290..299
        rows = 3 + rows * 287 // 300
        if kind.endswith("unsorted"):
            rows = rows[::-1].copy()
    table = rng.integers(1, 9, (n_cols, 68)) * rng.choice(np.array([-1, 1]), (n_cols, 68))
    return {"rows": rows.astype(np.int64), "cols": cols.astype(np.int64), "vals": vals.astype(np.int64), "n_rows": n_rows,
            "n_cols": n_cols, "table": table.astype(np.int64)}


@pytest.mark.parametrize("kind", ["sorted", "swapped", "shuffled-duplicates", "empty-ends", "empty-ends-unsorted", "none-0-rows", "none-5-rows"])
def test_csr_arrays_are_the_stable_sort_by_row(kind, dev):
    """ngcf_csr_from_coo on the device path (rows sorted) and the host path (not sorted): the arrays are the input in a stable sort by
    row - duplicates stay separate and in input order; ngcf_csr_from_arrays on the same arrays multiplies the same and BORROWS them."""
    eng = _eng()
    c = _coo_input(kind)
    is_sorted = bool((np.diff(c["rows"]) >= 0).all())
    assert is_sorted == (kind in ("sorted", "empty-ends", "none-0-rows", "none-5-rows"))
    if kind == "shuffled-duplicates":
        key = c["rows"] * c["n_cols"] + c["cols"]
        assert np.unique(key).size < key.size
    if kind.startswith("empty-ends"):
        lens = pc.row_lengths(c)
        assert not lens[:3].any() and not lens[290:].any()
    rows, cols, vals, table = _on_dev(kind, c, dev)
    csr = eng.LaplacianCSR.from_coo(rows, cols, vals, c["n_rows"], c["n_cols"])
    assert (csr.n_rows, csr.n_cols, csr.nnz) == (c["n_rows"], c["n_cols"], c["rows"].size)
    order = np.argsort(c["rows"], kind="stable")
    rp = np.r_[0, np.cumsum(np.bincount(c["rows"], minlength=c["n_rows"]))]
    _assert_arrays(csr, rp, c["cols"][order], c["vals"][order])
    assert csr.n_segments == 0 and csr.max_row_len == int(pc.row_lengths(c).max(initial=0))
    if c["n_rows"] == 0:
        assert csr.groups() == []
        return
    want = _exact(c)
    for d, layout in ((68, "aligned"), (5, "odd")):
        _assert_exact(_product(csr, table, d, layout, dev), want[:, :d], f"from_coo {kind} d={d}")
    d_rp, d_ci = torch.from_numpy(rp.astype(np.int64)).to(dev), torch.from_numpy(c["cols"][order].astype(np.int32)).to(dev)
    d_va = torch.from_numpy(c["vals"][order].astype(np.float32)).to(dev)
    borrowed = eng.LaplacianCSR.from_csr_arrays(d_rp, d_ci, d_va, c["n_cols"])
    assert (borrowed.n_rows, borrowed.nnz, borrowed.n_segments, borrowed.groups()) == (csr.n_rows, csr.nnz, 0, csr.groups())
    _assert_arrays(borrowed, rp, c["cols"][order], c["vals"][order])
    _assert_exact(_product(borrowed, table, 68, "aligned", dev), want, f"from_csr_arrays {kind}")
    d_va.mul_(2)                                           # the arrays are the caller's: the next product follows the edit
    _assert_exact(_product(borrowed, table, 68, "aligned", dev), 2 * want, f"from_csr_arrays {kind} after vals *= 2")
    _assert_exact(_product(csr, table, 68, "aligned", dev), want, f"from_coo {kind} owns its copy")


@pytest.mark.parametrize("unsorted", [False, True])
def test_out_of_range_ids_raise(unsorted, dev):
    """-1, n_rows (as a row) and n_cols (as a column), first, last or in the middle, on the sorted and the unsorted path."""
    eng = _eng()
    c = _coo_input("swapped" if unsorted else "sorted")
    n = c["rows"].size
    for which, bad in (("rows", -1), ("rows", c["n_rows"]), ("cols", -1), ("cols", c["n_cols"])):
        for at in (0, n // 2, n - 1):
            a = {k: c[k].copy() for k in ("rows", "cols")}
            a[which][at] = bad
            with pytest.raises(IndexError, match="out of range"):
                eng.LaplacianCSR.from_coo(torch.from_numpy(a["rows"]).to(dev), torch.from_numpy(a["cols"]).to(dev),
                                          torch.from_numpy(c["vals"].astype(np.float32)).to(dev), c["n_rows"], c["n_cols"])


# ---- 2. segment boundaries -------------------------------------------------------------------------------------------------------
_seg_want = functools.lru_cache(maxsize=None)(lambda name: _exact(pc.seg_case(name)))


def _seg_csr(name, dev):
    c = pc.seg_case(name)
    csr = _build(("seg", name), c, dev)
    csr.set_mode(0)
    csr.plan(c["seg_len"])
    assert _assert_plan(csr, c, c["seg_len"]) == pc.SEG_EXPECT[name]
    assert pc.shape_of(csr.groups()) == [(0, 1024, "S"), (1024, 2048, "T")]
    return csr


@pytest.mark.parametrize("d,layout", [
    (4, "aligned"),         # spmm_kernel<4, 8, 1, 4> + the table kernel
    (64, "aligned"),        # mode 0: spmm_sliced_kernel on the upper 1024 rows, the segments on spmm_kernel; mode 1: no slicing
    (65, "odd"),            # spmm_kernel<1, 64, 2, 4>
    (68, "aligned"),        # spmm_kernel<4, 32, 1, 8> + the table kernel
    (130, "aligned"),       # 128 + spmm_tail_kernel<2, false> over the CSR's own segments
    (516, "aligned"),       # one piece on spmm_kernel<4, 64, 3, 2>
    (770, "odd"),           # panels 512 + 258
])
@pytest.mark.parametrize("name", list(pc.SEG_CASES))
def test_segment_boundaries(name, d, layout, dev, lib_options):
    """Rows of 0, 1, L-1, L, L+1, 2L-1, 2L, 2L+1, 7L and 8L+1 entries under plan(L), L in 64, 128, 2048: a row of exactly L entries is
    a row, L+1 is two segments; segment counts of 1 and 0 modulo 4 and 1, 4, 5 cut rows (four to a workgroup)."""
    c = pc.seg_case(name)
    csr = _seg_csr(name, dev)
    table = _on_dev(("seg", name), c, dev)[3]
    want = _seg_want(name)[:, :d]
    for mode in (0, 1):
        csr.set_mode(mode)
        for no_ldstab in ((0, 1) if mode == 0 and d % 4 == 0 else (0,)):
            lib_options(no_ldstab=no_ldstab)
            _assert_exact(_product(csr, table, d, layout, dev), want, f"{name} d={d} mode={mode} no_ldstab={no_ldstab}")
    csr.set_mode(0)


@pytest.mark.parametrize("name", list(pc.SEG_CASES))
def test_segment_boundaries_under_device_dropout(name, dev):
    c = pc.seg_case(name)
    csr = _seg_csr(name, dev)
    keep = orc.keep_mask(c["rows"], c["cols"], SEEDS, P)
    got = _product(csr, _on_dev(("seg", name), c, dev)[3], 68, "aligned", dev, (list(SEEDS), P, False))
    _assert_exact(got, _exact(c, keep, 68), f"{name} dropout")


def test_replanning_gives_the_same_bits(dev):
    name = "64-all"
    c = pc.seg_case(name)
    csr = _seg_csr(name, dev)
    table = _on_dev(("seg", name), c, dev)[3]
    first = {d: _product(csr, table, d, layout, dev).clone() for d, layout in ((68, "aligned"), (65, "odd"), (130, "aligned"))}
    csr.plan(2048)
    assert _assert_plan(csr, c, 2048) == (0, 0)                # the longest row has 8 * 64 + 1 entries: nothing is cut
    for d, layout in ((68, "aligned"), (65, "odd"), (130, "aligned")):
        _assert_exact(_product(csr, table, d, layout, dev), _seg_want(name)[:, :d], f"replanned at 2048 d={d}")
    csr.plan(64)
    assert _assert_plan(csr, c, 64) == pc.SEG_EXPECT[name]
    for d, layout in ((68, "aligned"), (65, "odd"), (130, "aligned")):
        assert torch.equal(_product(csr, table, d, layout, dev), first[d])
    with pytest.raises(RuntimeError, match="seg_len"):
        csr.plan(63)
    assert _assert_plan(csr, c, 64) == pc.SEG_EXPECT[name]      # the refused call left the plan alone


# ---- 3. row groups ---------------------------------------------------------------------------------------------------------------
_group_want = functools.lru_cache(maxsize=None)(lambda name: _exact(pc.group_case(name)))
GROUP_PARAMS = [(n, d, layout) for n in pc.GROUP_EXPECT
                for d, layout in ([(64, "aligned")] if n.startswith("rows") else [(64, "aligned"), (96, "aligned"), (68, "aligned"), (65, "odd")])]


@pytest.mark.parametrize("name,d,layout", GROUP_PARAMS)
def test_row_groups(name, d, layout, dev, lib_options):
    """build_row_groups on matrices made for one branch each (plan_cases.GROUP_EXPECT; slice_max_mb = 1 brings the 'neither' class
    within reach of a 16 384-column matrix): the groups are the ones the case was built for, and every product is exact."""
    c = pc.group_case(name)
    lib_options(slice_max_mb=c["slice_max_mb"])
    csr = _build(("group", name), c, dev)
    _assert_plan(csr, c, pc.default_seg_len(c["rows"].size), c["slice_max_mb"])
    groups = csr.groups()
    assert pc.shape_of(groups) == pc.GROUP_EXPECT[name]
    table = _on_dev(("group", name), c, dev)[3]
    want = _group_want(name)[:, :d]
    for no_ldstab in ((0, 1) if d % 4 == 0 and any(g["lds_table"] for g in groups) else (0,)):
        lib_options(no_ldstab=no_ldstab)
        got = _product(csr, table, d, layout, dev)
        _assert_exact(got, want, f"{name} d={d} no_ldstab={no_ldstab}")
        if name == "empty_blocks":
            assert bool((got[128:320] == 0).all()) and bool((got[448:] == 0).all())


# ---- 4. thinned copies -----------------------------------------------------------------------------------------------------------
L_THIN = 64
_ocase = functools.lru_cache(maxsize=None)(orc.build_case)
THIN_WIDTHS = {              # (d, layout, no_ldstab values): one width per path family
    "S": [(64, "aligned", (0, 1)),      # table-in-LDS kernel on the user rows / the same rows on spmm_kernel<4, 16, 1, 8>
          (68, "aligned", (0,)),        # float4 + table kernel, a slice of 4 floats
          (65, "odd", (0,)),            # scalar
          (130, "aligned", (0,)),       # 128 + spmm_tail_kernel<2, false>
          (515, "odd", (0,)), (770, "odd", (0,))],     # panels
    "Su": [(64, "aligned", (0, 1)), (65, "odd", (0,))],
    "W": [(96, "aligned", (0,)),        # spmm_sliced_kernel
          (132, "aligned", (0,)),       # float4
          (65, "odd", (0,)), (130, "aligned", (0,)), (515, "odd", (0,))],
    "St": [(68, "aligned", (0, 1)), (65, "odd", (0,))],
}


def _src(name, dev):
    c = _ocase(name)
    csr = _build(("thin", name), c, dev)
    n_cut, _ = _assert_plan(csr, c, L_THIN)
    assert pc.default_seg_len(csr.nnz) == L_THIN and (n_cut > 0) == (name != "Su")
    classes = {k for _, _, k in pc.shape_of(csr.groups())}
    assert ("T" in classes) == (name != "W")
    if name == "W":
        assert pc.shape_of(csr.groups()) == [(0, orc.W_N, "S")]      # >= 1024 rows: the sliced kernel
    return csr


def _assert_thinned(thin, case, keep, src, exact_count=True):
    """The thinned copy's arrays, counts and scan against the host's compaction; it reports its source's plan."""
    rp, ci, va, pos = pc.thinned_arrays(case, keep)
    assert (thin.n_rows, thin.n_cols) == (case["n_rows"], case["n_cols"])
    assert thin.nnz == (int(keep.sum()) if exact_count else src.nnz)
    _assert_arrays(thin, rp, ci, va)
    from seoul_tourism_recommendation_ngcf_amd.engine._plumbing import _device_view
    assert torch.equal(_device_view(thin.filter_pos, keep.size + 1, torch.int32).cpu(), torch.from_numpy(pos))
    assert (thin.n_segments, thin.groups(), thin.swept_rows) == (src.n_segments, src.groups(), 0)


def _check_thinned_products(thin, case, keep, name, dev, lib_options, widths=None, what=""):
    widths = widths or THIN_WIDTHS[name]
    want = _exact(case, keep, max(d for d, _, _ in widths))
    table = _on_dev(("thin", name), _ocase(name), dev)[3]
    for d, layout, ldstab in widths:
        for no_ldstab in ldstab:
            lib_options(no_ldstab=no_ldstab)
            _assert_exact(_product(thin, table, d, layout, dev), want[:, :d], f"thinned {name} {what} d={d} no_ldstab={no_ldstab}")
    lib_options(no_ldstab=0)


def _keep_dev(keep, dev):
    return torch.from_numpy(keep).to(dev)


@pytest.mark.parametrize("mask", pc.THIN_MASKS)
@pytest.mark.parametrize("name", ["S", "St", "W", "Su"])
def test_thinned_copy_products(name, mask, dev, lib_options):
    """Masks by rule (plan_cases.thin_mask): every cut row keeps k entries, k in 0, 1, L-1, L, L+1, 2L, all - it stays cut with every
    segment non-empty, has trailing empty segments, sits at exactly L (a row again, produced by the row kernels AND the fix-up) or
    L+1, or is emptied.  Arrays and scan of ngcf_csr_filter, then the product on every path family of the case."""
    eng = _eng()
    c, src = _ocase(name), _src(name, dev)
    keep = pc.thin_mask(c, L_THIN, mask)
    thin = src.filtered(_keep_dev(keep, dev), None, int(keep.sum()))
    _assert_thinned(thin, c, keep, src)
    _check_thinned_products(thin, c, keep, name, dev, lib_options, what=mask)
    if name == "St":                                   # the row-sparse transposed product walks the thinned copy's segments too
        sel, X, init, slot = _t_rows_inputs(name)
        d = 65
        Xfull = np.zeros((c["n_cols"], d), np.int64)
        Xfull[sel] = X[:, :d]
        base = orc.spmm_exact(c["rows"], c["cols"], c["vals"], Xfull, keep & (slot[c["cols"]] >= 0), n_rows=c["n_rows"])
        Xd = torch.from_numpy(np.ascontiguousarray(X[:, :d]).astype(np.float32)).to(dev)
        for with_init in (False, True):
            want = base.copy()
            if with_init:
                want[sel] += init[:, :d]
            initd = torch.from_numpy(np.ascontiguousarray(init[:, :d]).astype(np.float32)).to(dev) if with_init else None
            buf, out = _view(c["n_rows"], d, "odd", dev)
            eng.spmm_t_rows(thin, torch.from_numpy(slot).to(dev), Xd, initd, out, eng.Workspace(), None)
            _assert_exact(out, want.astype(np.float32), f"t_rows on thinned St {mask} init={with_init}")
            assert bool(torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, 1 + d:]).all())


@pytest.mark.parametrize("name,mask", [("S", "first-L"), ("S", "spread-2L"), ("W", "spread-L+1"), ("St", "first-1")])
def test_thinned_copy_without_the_count(name, mask, dev, lib_options):
    """nnz_kept = -1: the copy reports the source's count as an upper bound and multiplies the same."""
    c, src = _ocase(name), _src(name, dev)
    keep = pc.thin_mask(c, L_THIN, mask)
    thin = src.filtered(_keep_dev(keep, dev), None, -1)
    _assert_thinned(thin, c, keep, src, exact_count=False)
    _check_thinned_products(thin, c, keep, name, dev, lib_options, what=mask + " uncounted")


@pytest.mark.parametrize("name", ["S", "W"])
def test_thinned_copy_reused_under_other_masks(name, dev, lib_options):
    """reuse= of the previous destination: a mask that keeps more entries, then fewer, then more again - nothing of the earlier
    contents (entries, row starts, segment starts) may show."""
    c, src = _ocase(name), _src(name, dev)
    thin, kept = None, []
    for mask in ("first-all", "spread-1", "spread-2L", "first-0", "first-L+1"):
        keep = pc.thin_mask(c, L_THIN, mask)
        kept.append(int(keep.sum()))
        prev = thin
        thin = src.filtered(_keep_dev(keep, dev), None, int(keep.sum()), reuse=prev)
        assert prev is None or not prev._h.value                  # the handle moved into the new object
        _assert_thinned(thin, c, keep, src)
        _check_thinned_products(thin, c, keep, name, dev, lib_options, widths=THIN_WIDTHS[name][:4], what=mask + " reused")
    assert kept[0] > kept[1] < kept[2] > kept[3] < kept[4]


@pytest.mark.parametrize("second", ["spread-L", "first-L+1", "first-1", "first-0"])
@pytest.mark.parametrize("name", ["S", "W"])
def test_thinned_copy_of_a_thinned_copy(name, second, dev, lib_options):
    """Two levels, as the reference's cumulative node dropout makes them: the second copy borrows the plan the first borrowed."""
    c, src = _ocase(name), _src(name, dev)
    keep1 = pc.thin_mask(c, L_THIN, "first-2L")
    one = src.filtered(_keep_dev(keep1, dev), None, int(keep1.sum()))
    c1 = {**c, "rows": c["rows"][keep1], "cols": c["cols"][keep1], "vals": c["vals"][keep1]}
    assert pc.segment_plan(pc.row_lengths(c1), L_THIN)[0] == pc.segment_plan(pc.row_lengths(c), L_THIN)[0]     # all still cut
    keep2 = pc.thin_mask(c1, L_THIN, second)
    two = one.filtered(_keep_dev(keep2, dev), None, int(keep2.sum()))
    _assert_thinned(two, c1, keep2, one)
    _check_thinned_products(two, c1, keep2, name, dev, lib_options, widths=THIN_WIDTHS[name][:4], what="first-2L then " + second)
    _assert_thinned(one, c, keep1, src)                            # the first level is untouched
    _check_thinned_products(one, c, keep1, name, dev, lib_options, widths=THIN_WIDTHS[name][:2], what="first-2L")


@pytest.mark.parametrize("mask", ["first-L", "spread-L+1", "spread-2L", "first-0"])
def test_thinned_transpose_through_the_entry_map(mask, dev, lib_options):
    """L^T thinned with the flags drawn for L through the entry map equals the transpose of the thinned L, arrays and product."""
    c, ct = _ocase("S"), _ocase("St")
    src_t = _src("St", dev)
    order = np.argsort(c["cols"], kind="stable")                  # entry j of L^T is entry order[j] of L
    assert np.array_equal(ct["rows"], c["cols"][order]) and np.array_equal(ct["cols"], c["rows"][order])
    keep = pc.thin_mask(c, L_THIN, mask)
    emap = torch.from_numpy(order.astype(np.int32)).to(dev)
    thin_t = src_t.filtered(_keep_dev(keep, dev), emap, int(keep.sum()))
    keep_t = keep[order]
    _assert_thinned(thin_t, ct, keep_t, src_t)
    o2 = np.argsort(c["cols"][keep], kind="stable")               # the transpose of the thinned L, built from L's kept entries
    _assert_arrays(thin_t, pc.thinned_arrays(ct, keep_t)[0], c["rows"][keep][o2], c["vals"][keep][o2])
    _check_thinned_products(thin_t, ct, keep_t, "St", dev, lib_options, what=mask + " via entry map")


@pytest.mark.parametrize("name,mask", [("S", "spread-2L"), ("S", "first-L"), ("W", "first-L+1")])
def test_device_dropout_on_a_thinned_copy(name, mask, dev):
    c, src = _ocase(name), _src(name, dev)
    keep = pc.thin_mask(c, L_THIN, mask)
    thin = src.filtered(_keep_dev(keep, dev), None, int(keep.sum()))
    both = keep & orc.keep_mask(c["rows"], c["cols"], SEEDS, P)
    assert 0 < both.sum() < keep.sum()
    got = _product(thin, _on_dev(("thin", name), c, dev)[3], 68, "aligned", dev, (list(SEEDS), P, False))
    _assert_exact(got, _exact(c, both, 68), f"dropout on thinned {name} {mask}")


# ---- 5. swept and row-wise groups in one product ---------------------------------------------------------------------------------
def test_swept_and_rowwise_groups_in_one_product(dev, lib_options):
    """Mode 3 on a matrix whose first group the swept plan takes (4.46 M entries) and whose second it declines (a table group with
    cut rows, some of them the last rows): swept parts, the segment set of the rest, the partial rows behind it and the skipped
    group in one product.  The one large case of this file: `declined` refuses a group under 2^22 entries."""
    c = pc.mixed_case()
    n_a, n = pc.MIXED_A_ROWS, pc.MIXED_A_ROWS + pc.MIXED_B_ROWS
    lens = pc.row_lengths(c)
    want = pc.spmm_exact_blocked(c, 130)
    keep = orc.keep_mask(c["rows"], c["cols"], SEEDS, P)
    want_drop = pc.spmm_exact_blocked(c, 64, keep)
    assert max(np.abs(want).max(), np.abs(want_drop).max()) < 2 ** 24
    want, want_drop = want.astype(np.float32), want_drop.astype(np.float32)
    rows, cols = torch.from_numpy(c["rows"]).to(dev), torch.from_numpy(c["cols"]).to(dev)
    vals, table = torch.from_numpy(c["vals"].astype(np.float32)).to(dev), torch.from_numpy(c["table"].astype(np.float32)).to(dev)
    lib_options(swept_lpe=16)
    csr = _eng().LaplacianCSR.from_coo(rows, cols, vals, n, c["n_cols"])
    n_cut, _ = _assert_plan(csr, c, 2048)
    assert n_cut == len(pc.MIXED_LONG) and pc.shape_of(csr.groups()) == [(0, n_a, "S"), (n_a, n, "T")]
    assert csr.swept_rows == 0
    rowwise = _product(csr, table, 64, "aligned", dev)
    _assert_exact(rowwise, want[:, :64], "mixed, mode 0")
    csr.set_mode(3)
    assert csr.swept_rows == n_a                                   # group A swept, group B declined ...
    assert (lens[n_a:] > 2048).sum() == n_cut and lens[-1] > 2048    # ... and the rest still has cut rows, the last row among them
    first = {}
    for d in (64,       # spmm_swept_kernel at 16 lanes per entry on A; table kernel + segments + fix-up on B
              130,      # 128 swept + spmm_tail_kernel<2> over the CSR's own segments
              68):      # 64 swept + spmm_tail_kernel<4>
        first[d] = _product(csr, table, d, "aligned", dev).clone()
        _assert_exact(first[d], want[:, :d], f"mixed, mode 3, d={d}")
    _assert_exact(_product(csr, table, 64, "aligned", dev, (list(SEEDS), P, False)), want_drop, "mixed, mode 3, dropout")
    csr.plan(64)                                                   # the mode is kept: parts and the rest's segments are rebuilt
    assert csr.swept_rows == n_a
    assert _assert_plan(csr, c, 64)[0] == n_a + int((lens[n_a:] > 64).sum())
    for d in (64, 130):
        assert torch.equal(_product(csr, table, d, "aligned", dev), first[d])
    csr.plan(2048)
    csr.set_mode(0)
    lib_options(swept_lpe=32)
    csr.set_mode(3)
    assert csr.swept_rows == n_a
    for d in (128,      # spmm_swept_kernel at 32 lanes per entry
              68):      # no multiple of 128 in it: swept_usable is false and every group runs row-wise, cut rows through the CSR's own segments
        _assert_exact(_product(csr, table, d, "aligned", dev), want[:, :d], f"mixed, mode 3, 32 lanes, d={d}")
    csr.close()
