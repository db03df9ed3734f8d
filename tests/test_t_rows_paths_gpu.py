"""Both kernels of ngcf_spmm_t_rows_f32 (csrc/spmm_t_rows.hip) on the branch-point cases of tests/t_rows_oracle.py: the bitmap-in-LDS
kernel, reached at any number of stored entries with the option t_rows_bitmap = 2, and the slot-table kernel (t_rows_bitmap = 0).
Per case and width: `spmm_t_rows_path` names the kernel that is meant to run (a comparison cannot pass because the dispatch quietly
stayed on the other one); the result EQUALS the exact integer product (`torch.equal`) with and without init, without dropout and
under the host's own mask; `out` has an odd leading dimension, starts at column 1 and is prefilled with NaN, X and init have ld > d.
On non-integer data both kernels equal the order oracle - every sum in entry order, one fmaf per hit - bit for bit, from which their
bit-identity to each other follows.  tests/test_t_rows_oracle.py shows on the CPU that every case reaches its branches."""
import functools

import numpy as np
import pytest
import torch

import t_rows_oracle as tro

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEEDS = (2 ** 62 - 1, 0xC2B2AE3D27D4EB4F, 0, 123456789)
DEFAULT = (SEEDS[:2], 0.3)
WIDTHS = (1, 64, 65, 128, 129, 256, 257, 512, 513, 600)        # NQ 1, 1, 2, 2, 4, 4, 8, 8, a second panel of 1 and of 88 columns
FULL = 600
MODES = (2, 0)                                                  # t_rows_bitmap: the bitmap kernel wherever it fits; never


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _eng():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg.engine


_DEV = {}


def _csr(name, dev, float_vals=False):
    """The case's CSR of L^T with its own seg_len, once per module (and once more with the order oracle's values)."""
    key = ("csr", name, float_vals)
    if key not in _DEV:
        c = tro.case(name)
        vals = tro.float_inputs(c, 1)[0] if float_vals else c["vals"].astype(np.float32)
        csr = _eng().LaplacianCSR.from_coo(torch.from_numpy(tro.entry_rows(c)).to(dev), torch.from_numpy(np.array(c["colidx"])).to(dev),
                                           torch.from_numpy(vals).to(dev), c["n"], c["n"])
        csr.plan(c["seg_len"])
        lens = np.diff(c["rowptr"])
        assert csr.n_segments == int((-(-lens[lens > c["seg_len"]] // c["seg_len"])).sum()) and csr.nnz == c["colidx"].size < tro.MIN_NNZ
        _DEV[key] = csr
    return _DEV[key]


def _slot(name, dev):
    if ("slot", name) not in _DEV:
        _DEV["slot", name] = torch.from_numpy(np.array(tro.case(name)["slot"])).to(dev)
    return _DEV["slot", name]


def _ws(dev):
    """One grow-only scratch for the module, as a training run has it; from the start larger than the few hundred bytes the smallest
    cases ask for (see test_the_documented_workspace_has_room_for_the_bitmap_from_17_rows_on)."""
    if "ws" not in _DEV:
        _DEV["ws"] = _eng().Workspace()
        _DEV["ws"].get(1 << 16, dev)
    return _DEV["ws"]


def _width(name, d):
    return 4 if name.startswith("lds_") else 128 if name == "rows_refill" else 4100 if d > FULL else FULL


@functools.lru_cache(maxsize=None)
def _ints(name, width):
    return tro.int_inputs(tro.case(name), width)


@functools.lru_cache(maxsize=None)
def _want(name, width, with_init, drop):
    """The exact product at the case's full width as float32 (every value an integer below 2^24), shared read-only."""
    X, init = _ints(name, width)
    seeds, p = drop if drop else ((), 0.0)
    out = tro.exact_product(tro.case(name), X, init if with_init else None, seeds, p)
    assert np.abs(out).max() < 2 ** 24
    out = out.astype(np.float32)
    out.setflags(write=False)
    return out


def _padded(a, d, dev):
    """The first d columns of a host matrix as a device view with ld = d + 3."""
    buf = torch.full((a.shape[0], d + 3), NAN, device=dev)
    buf[:, :d] = torch.from_numpy(np.ascontiguousarray(a[:, :d]).astype(np.float32)).to(dev)
    return buf[:, :d]


def _run(csr, name, d, X, init, drop, dev):
    """eng.spmm_t_rows into a NaN-filled buffer with an odd leading dimension, the view starting at column 1."""
    n = tro.case(name)["n"]
    buf = torch.full((n, d + 2 + (d + 1) % 2), NAN, device=dev)
    assert buf.shape[1] % 2 == 1
    out = buf[:, 1:1 + d]
    _eng().spmm_t_rows(csr, _slot(name, dev), X, init, out, _ws(dev), (list(drop[0]), drop[1]) if drop else None)
    assert bool(torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, 1 + d:]).all()), "written outside the d columns of the output"
    return out


def _assert_equal(got, want, what):
    want = torch.from_numpy(np.array(want)).to(got.device)           # (a copy: the shared reference stays read-only)
    assert got.shape == want.shape
    if torch.equal(got, want):
        return
    bad = ~(got == want)                                           # (a NaN left in the output counts)
    rows = torch.nonzero(bad.any(1)).flatten()
    r = int(rows[0])
    col = int(torch.nonzero(bad[r]).flatten()[0])
    pytest.fail(f"{what}: {int(bad.sum())} elements in {rows.numel()} rows differ from the oracle ({int(torch.isnan(got).sum())} NaN left); "
                f"rows {rows[:8].tolist()}; [{r}, {col}] got {float(got[r, col])!r} want {float(want[r, col])!r}")


def _set_mode(mode, name, d, dev, lib_options, csr):
    """Set t_rows_bitmap and hold the dispatch to the kernel the case is meant for."""
    lib_options(t_rows_bitmap=mode)
    meant = "bitmap" if mode == 2 and tro.fits(tro.case(name)["n"], d) else "slot"
    got = _eng().spmm_t_rows_path(csr, d, _ws(dev), dev)
    assert got == meant, f"{name} d={d} t_rows_bitmap={mode}: the dispatch takes the {got} kernel, the case is meant for {meant}"
    return meant


def _check_exact(name, d, dev, lib_options, drops=(None, DEFAULT), inits=(False, True)):
    csr, width = _csr(name, dev), _width(name, d)
    X, init = _ints(name, width)
    Xd, initd = _padded(X, d, dev), _padded(init, d, dev)
    for mode in MODES:
        kernel = _set_mode(mode, name, d, dev, lib_options, csr)
        for with_init in inits:
            for drop in drops:
                got = _run(csr, name, d, Xd, initd if with_init else None, drop, dev)
                _assert_equal(got, _want(name, width, with_init, drop)[:, :d],
                              f"{name} d={d} {kernel} kernel init={with_init} drop={drop[1] if drop else 0}")


# ---- the exact product -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", ["hits", "runs"])
def test_list_states_and_cut_rows_at_every_width(name, d, dev, lib_options):
    _check_exact(name, d, dev, lib_options)


@pytest.mark.parametrize("d", [65, 128])
@pytest.mark.parametrize("name", [c for c in tro.SMALL if c not in ("hits", "runs")] + ["rows_refill"])
def test_units_chunks_windows_and_init_rows(name, d, dev, lib_options):
    _check_exact(name, d, dev, lib_options)


@pytest.mark.parametrize("name", [c for c in tro.LARGE if c.startswith("lds_")])
def test_the_largest_bitmap_that_fits_the_lds(name, dev, lib_options):
    """N = 1 138 560 is the last row count whose bitmap fits beside the hit lists (bitmap kernel), N + 1 must stay on the slot
    table (_set_mode asserts both); 70 001 rows end in a partly used word.  d = 4."""
    _check_exact(name, 4, dev, lib_options)


@pytest.mark.parametrize("d", [4096, 4100])
def test_all_eight_panel_counters_and_the_width_beyond_them(d, dev, lib_options):
    """d = 4096: eight launches, one counter each; d = 4100 would need a ninth: the slot-table kernel (_set_mode asserts it)."""
    assert tro.panels(4096) == tro.PANELS < tro.panels(4100)
    _check_exact("rows_513", d, dev, lib_options, drops=(DEFAULT,), inits=(True,))


@pytest.mark.parametrize("d", [65, 128])
@pytest.mark.parametrize("seeds", [SEEDS, SEEDS[:1]], ids=["4seeds", "1seed"])
@pytest.mark.parametrize("name", ["init", "hits"])
def test_heavy_dropout(name, seeds, d, dev, lib_options):
    """p = 0.9: rows of R that keep their init term and lose every hit, rows whose first hit is dropped (the accumulator must not
    move to a row whose hit is dropped, and must start from init at the first hit that is kept)."""
    c = tro.case(name)
    hits, kept = tro.kept_hits(c), tro.kept_hits(c, seeds, 0.9)
    rows = tro.entry_rows(c)
    n_hits, n_kept = np.bincount(rows[hits], minlength=c["n"]), np.bincount(rows[kept], minlength=c["n"])
    in_R = c["slot"] >= 0
    assert (in_R & (n_hits > 0) & (n_kept == 0)).any(), "a row of R with init and every hit dropped"
    first_hit = np.full(c["n"], -1, np.int64)
    first_hit[rows[hits][::-1]] = np.flatnonzero(hits)[::-1]
    first_dropped = (first_hit >= 0) & ~kept[np.maximum(first_hit, 0)]
    assert first_dropped.any(), "a row whose first hit is dropped"
    if len(seeds) == 1:
        assert (first_dropped & (n_kept > 0)).any(), "... and a later one kept"
    _check_exact(name, d, dev, lib_options, drops=((seeds, 0.9),))


# ---- the order of every sum ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _floats(name):
    return tro.float_inputs(tro.case(name), 128)


@functools.lru_cache(maxsize=None)
def _want_order(name, with_init, drop):
    c = tro.case(name)
    vals, X, init = _floats(name)
    keep = tro.orc.keep_mask(tro.entry_rows(c), c["colidx"], drop[0], drop[1], transposed=True) if drop else None
    out = tro.order_product(c, vals, X, init if with_init else None, keep)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("d", [65, 128])
@pytest.mark.parametrize("name", ["hits", "runs", "windows"])
def test_every_sum_runs_in_entry_order_with_one_fma_per_hit(name, d, dev, lib_options):
    csr = _csr(name, dev, float_vals=True)
    _, X, init = _floats(name)
    Xd, initd = _padded(X, d, dev), _padded(init, d, dev)
    for mode in MODES:
        kernel = _set_mode(mode, name, d, dev, lib_options, csr)
        for with_init in (False, True):
            for drop in (None, DEFAULT):
                got = _run(csr, name, d, Xd, initd if with_init else None, drop, dev)
                _assert_equal(got, _want_order(name, with_init, drop)[:, :d], f"order: {name} d={d} {kernel} kernel init={with_init} drop={bool(drop)}")


# ---- which kernel runs -----------------------------------------------------------------------------------------------------------
def test_the_documented_workspace_has_room_for_the_bitmap_from_17_rows_on(dev, lib_options):
    """A scratch of exactly ngcf_spmm_workspace_bytes(csr_t, d) bytes: 1 280 at up to 16 rows, 16 short of the partial sums + bitmap +
    1 KiB the bitmap kernel asks for - the slot-table kernel runs, as include/ngcf_hip.h says; from 17 rows on there is room.  The
    default option value leaves every matrix below 2^22 stored entries on the slot table, 0 all of them."""
    eng = _eng()
    for name, meant in (("rows_1", "slot"), ("rows_16", "slot"), ("rows_17", "bitmap"), ("hits", "bitmap"), ("runs", "bitmap")):
        csr = _csr(name, dev)
        lib_options(t_rows_bitmap=2)
        assert eng.spmm_t_rows_path(csr, 65, eng.Workspace(), dev) == meant, name
        assert eng.spmm_t_rows_path(csr, 65, _ws(dev), dev) == "bitmap"
        for mode in (0, 1):
            lib_options(t_rows_bitmap=mode)
            assert eng.spmm_t_rows_path(csr, 65, _ws(dev), dev) == "slot"
    lib = eng._lib.load()
    lib_options(t_rows_bitmap=2)
    csr = _csr("runs", dev)                                          # cut rows: the partial sums come first
    n, d = tro.case("runs")["n"], 65
    room = (csr.n_segments * 68 * 4 + 255) // 256 * 256 + 256 + (n + 127) // 128 * 16 + 1024
    assert lib.ngcf_spmm_t_rows_path(csr._h, d, room) == b"bitmap" and lib.ngcf_spmm_t_rows_path(csr._h, d, room - 1) == b"slot"
    assert lib.ngcf_spmm_t_rows_path(csr._h, d, 0) == b"slot"
    assert lib.ngcf_spmm_t_rows_path(csr._h, 0, room) is None and "spmm_t_rows_path" in eng._lib.last_error()
    assert lib.ngcf_spmm_t_rows_path(csr._h, d, -1) is None
