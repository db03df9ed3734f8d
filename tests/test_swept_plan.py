"""csrc/swept_plan.h on the CPU: the host plan of the L2-swept SpMM is plain C++ over host arrays, so a host compiler builds it and
the plan is replayed here slot by slot, the way the kernel walks it.  Properties, not hashes: a planner that lays the entries out
differently but correctly still passes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from csr_cases import random_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc", "swept_plan.h")
SOURCE = r'''
#include "%s"
using namespace swept_plan;
static Params params(int lpe, int cut, int moments, int order_rows, int window_kb, int force)
{
    Params p;
    p.lpe = lpe, p.cut = cut, p.moments = moments != 0, p.order_rows = order_rows != 0, p.window_kb = window_kb, p.force = force != 0;
    return p;
}
extern "C" int swept_declined(int64_t n, int64_t nnz, int32_t col_lo, int32_t col_hi, int lpe, int force)
{
    return declined(n, nnz, col_lo, col_hi, params(lpe, 4, 1, 0, 0, force));
}
extern "C" void *plan_new(const int64_t *rp, int64_t n, const int32_t *col, const float *val, int64_t row_lo, int32_t col_lo,
                          int32_t col_hi, int lpe, int cut, int moments, int order_rows, int window_kb, int force)
{
    return new PartPlan(plan_part(rp, n, col, val, row_lo, col_lo, col_hi, params(lpe, cut, moments, order_rows, window_kb, force)));
}
#define PLAN_ARRAYS(p, f) (w == 0 ? f(p->tptr) : w == 1 ? f(p->e_pack) : w == 2 ? f(p->e_val) : w == 3 ? f(p->dst) : w == 4 ? f(p->prow) \
                           : w == 5 ? f(p->heavy_row) : f(p->heavy_ptr))
#define PLAN_SIZE(v) (int64_t)(v).size()
#define PLAN_DATA(v) (const void *)(v).data()
extern "C" int64_t plan_size(const PartPlan *p, int w) { return PLAN_ARRAYS(p, PLAN_SIZE); }
extern "C" const void *plan_data(const PartPlan *p, int w) { return PLAN_ARRAYS(p, PLAN_DATA); }
extern "C" int64_t plan_scalar(const PartPlan *p, int w)
{
    const int64_t s[7] = {p->rows_per_wave, p->n_rowpass, p->n_win, p->win_cols, p->n_slots, p->n_partial, p->waves};
    return s[w];
}
extern "C" const char *plan_error(const PartPlan *p) { return p->error.c_str(); }
extern "C" void plan_free(PartPlan *p) { delete p; }
extern "C" int plan_col_mask(void) { return kColMask; }
extern "C" int plan_row_bits(void) { return kRowBits; }
'''
ARRAYS = (("tptr", np.int64), ("e_pack", np.int32), ("e_val", np.float32), ("dst", np.int32), ("prow", np.int32),
          ("heavy_row", np.int32), ("heavy_ptr", np.int64))
SCALARS = ("rows_per_wave", "n_rowpass", "n_win", "win_cols", "n_slots", "n_partial", "waves")


def load(path):
    lib = ctypes.CDLL(path)
    lib.plan_new.restype = ctypes.c_void_p
    lib.plan_data.restype = ctypes.c_void_p
    lib.plan_size.restype = lib.plan_scalar.restype = ctypes.c_int64
    lib.plan_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: csrc/swept_plan.h cannot be checked")
    d = tmp_path_factory.mktemp("swept_plan")
    src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "libplan.so")
    with open(src, "w") as f:
        f.write(SOURCE % HEADER)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-pthread", "-o", so, src])   # the header alone
    return load(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_plan(lib, m, lpe, order, moments, cut=4, force=True):
    """plan_part on the matrix `m` taken as one row group; the seven arrays and the scalars as a dict."""
    h = ctypes.c_void_p(lib.plan_new(_ptr(m["rowptr"]), ctypes.c_int64(m["n_rows"]), _ptr(m["cols"]), _ptr(m["vals"]),
                                     ctypes.c_int64(m["row_lo"]), ctypes.c_int32(m["col_lo"]), ctypes.c_int32(m["col_hi"]), lpe, cut,
                                     int(moments), int(order == "rows"), m["window_kb"], int(force)))
    try:
        assert lib.plan_error(h) == b""
        out = {name: int(lib.plan_scalar(h, i)) for i, name in enumerate(SCALARS)}
        for i, (name, dt) in enumerate(ARRAYS):
            n = int(lib.plan_size(h, i))
            buf = (ctypes.c_char * (n * np.dtype(dt).itemsize)).from_address(lib.plan_data(h, i)) if n else b""
            out[name] = np.frombuffer(buf, dtype=dt).copy()
        return out
    finally:
        lib.plan_free(h)


def matrix(rowptr, cols, vals, row_lo=0, window_kb=0):
    """A row group as plan_part takes it: row pointer from 0, the column range its rows gather from; integer-valued values."""
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    return {"rowptr": np.ascontiguousarray(rowptr, dtype=np.int64), "cols": cols,
            "vals": np.ascontiguousarray(np.rint(np.asarray(vals, np.float64) * 10), dtype=np.float32),
            "n_rows": len(rowptr) - 1, "row_lo": row_lo, "window_kb": window_kb,
            "col_lo": int(cols.min()) if len(cols) else 0, "col_hi": int(cols.max()) if len(cols) else -1}


# the shapes of test_spmm_swept_degenerate_shapes (test_parity_gpu.py), drawn the same way
DEGENERATE = [(1, 1, 1, ()), (5, 3, 40, ()), (2000, 70000, 1, ()), (300, 50000, 3, ((0, 120000), (299, 9000))), (40, 17, 0, ((7, 5000),))]
_made = {}


def case(name):
    """Built once per name and left unchanged."""
    if name not in _made:
        if name == "two_row_passes":         # more rows than 256 workgroups x 16 waves x 18 rows hold at lpe 32; a group that starts at row 7
            rowptr, _, cols, vals = random_csr(np.random.default_rng(80000), 80000, 3000, 2, heavy=((11, 3000),))
            _made[name] = matrix(rowptr, cols, vals, row_lo=7)
        elif name == "many_windows":         # 16 KiB windows over 50 000 columns: hundreds of windows, most buckets empty
            rowptr, _, cols, vals = random_csr(np.random.default_rng(50300), 300, 50000, 3, heavy=((0, 120000), (299, 9000)))
            _made[name] = matrix(rowptr, cols, vals, window_kb=16)
        elif name == "one_entry":
            _made[name] = matrix([0, 1], [0], [0.3])
        else:
            n_rows, n_cols, deg, heavy = DEGENERATE[int(name)]
            rowptr, _, cols, vals = random_csr(np.random.default_rng(n_rows + n_cols), n_rows, n_cols, deg, heavy=heavy)
            _made[name] = matrix(rowptr, cols, vals)
    return _made[name]


CASES = [(str(i), lpe) for i in range(len(DEGENERATE)) for lpe in (16, 32)]
CASES += [("one_entry", 16), ("one_entry", 32), ("two_row_passes", 32), ("many_windows", 16), ("many_windows", 32)]


def check_plan(m, p, lpe):
    n, epr, RW = m["n_rows"], 64 // lpe, p["rows_per_wave"]
    row_bits, col_mask = 24, (1 << 24) - 1
    lens = np.diff(m["rowptr"])
    if len(m["cols"]) == 0:                  # nothing to multiply: declined even when forced
        assert p["waves"] == 0 and p["n_slots"] == 0
        return
    assert p["waves"] == 16 and RW == 576 // (lpe // 16) // 16
    n_tasks, n_win = p["n_rowpass"] * 256 * p["waves"], p["n_win"]
    tptr, e_pack, e_val, dst, prow = p["tptr"], p["e_pack"], p["e_val"], p["dst"], p["prow"]
    # buckets
    assert len(tptr) == n_tasks * n_win + 1 and tptr[0] == 0 and tptr[-1] == p["n_slots"] == len(e_pack) == len(e_val)
    blen = np.diff(tptr)
    assert (blen >= 0).all() and (blen % epr == 0).all()
    assert n_win == (m["col_hi"] - m["col_lo"]) // p["win_cols"] + 1
    lr, col = (e_pack >> row_bits) & 0x7f, e_pack & col_mask
    real = lr < RW
    assert (e_pack >= 0).all() and int(real.sum()) == len(m["cols"])
    window = np.repeat(np.arange(n_tasks * n_win) % n_win, blen)
    assert np.array_equal((col[real] - m["col_lo"]) // p["win_cols"], window[real])
    # rounds
    assert (lr[~real] == RW).all() and (e_val[~real] == 0).all()
    assert ((col[~real] >= m["col_lo"]) & (col[~real] <= m["col_hi"])).all()
    rl = np.where(real, lr, -1 - np.arange(len(lr)) % epr).reshape(-1, epr)      # empty slots: distinct dummies
    rs = np.sort(rl, axis=1)
    assert (rs[:, 1:] != rs[:, :-1]).all()
    # dst / prow
    assert len(dst) == len(prow) == n_tasks * RW
    heavy_row, heavy_ptr = p["heavy_row"].astype(np.int64) - m["row_lo"], p["heavy_ptr"]
    assert len(heavy_ptr) == len(heavy_row) + 1 and heavy_ptr[0] == 0 and heavy_ptr[-1] == p["n_partial"]
    assert (np.diff(heavy_ptr) >= 2).all() and (np.diff(heavy_row) > 0).all()
    uncut = np.setdiff1d(np.arange(n), heavy_row)
    assert np.array_equal(np.sort(dst[dst >= 0]) - m["row_lo"], uncut)
    assert np.array_equal(np.sort(-2 - dst[dst <= -2]), np.arange(p["n_partial"]))
    assert np.array_equal(prow[dst >= 0], dst[dst >= 0])
    part = -2 - dst[dst <= -2]
    assert np.array_equal(prow[dst <= -2] - m["row_lo"], heavy_row[np.searchsorted(heavy_ptr, part, side="right") - 1])
    # replay: every task adds its slots into its RW + 1 accumulator rows (the spare row last), rows leave through dst,
    # the partial rows of a cut row are added in heavy_ptr order.  Integers in float64: every sum is exact.
    E = np.random.default_rng(1).integers(-4, 5, (m["col_hi"] + 1, 2)).astype(np.float64)
    task = np.repeat(np.arange(n_tasks), tptr[n_win::n_win] - tptr[:-1:n_win])
    acc = np.zeros((n_tasks * (RW + 1), 2))
    np.add.at(acc, task * (RW + 1) + lr, e_val.astype(np.float64)[:, None] * E[col])
    acc = acc.reshape(n_tasks, RW + 1, 2)[:, :RW].reshape(n_tasks * RW, 2)
    out, partial = np.full((n, 2), np.nan), np.zeros((p["n_partial"], 2))
    out[dst[dst >= 0] - m["row_lo"]] = acc[dst >= 0]
    partial[part] = acc[dst <= -2]
    for h, r in enumerate(heavy_row):
        out[r] = partial[heavy_ptr[h]:heavy_ptr[h + 1]].sum(0)
    want = np.zeros((n, 2))
    np.add.at(want, np.repeat(np.arange(n), lens), m["vals"].astype(np.float64)[:, None] * E[m["cols"]])
    assert np.array_equal(out, want)


@pytest.mark.parametrize("moments", [True, False])
@pytest.mark.parametrize("order", ["cols", "rows"])
@pytest.mark.parametrize("name,lpe", CASES)
def test_plan_replays_to_the_csr_product(lib, name, lpe, order, moments):
    m = case(name)
    p = run_plan(lib, m, lpe, order, moments)
    if name == "two_row_passes":
        assert p["n_rowpass"] == 2 and p["n_partial"] > 0
    if name == "many_windows":
        assert p["n_win"] >= 200
    check_plan(m, p, lpe)


def test_decline(lib):
    assert lib.plan_col_mask() == (1 << lib.plan_row_bits()) - 1
    declined = lambda n, nnz, lo, hi, lpe, force: bool(lib.swept_declined(ctypes.c_int64(n), ctypes.c_int64(nnz), lo, hi, lpe, force))
    for lpe in (16, 32):
        assert declined(300, 1000, 0, 49999, lpe, 0)                       # small: launch-bound
        assert not declined(300, 1000, 0, 49999, lpe, 1)
        assert declined(300, 1000, 0, lib.plan_col_mask() + 1, lpe, 1)     # column does not fit the packed entry
        assert not declined(300, 1000, 0, lib.plan_col_mask(), lpe, 1)
        assert declined(0, 0, 0, 5, lpe, 1) and declined(5, 0, 0, 5, lpe, 1) and declined(5, 9, 3, 2, lpe, 1)
        assert not declined(150000, 1 << 23, 0, 149999, lpe, 0)            # large: a fetched table row is used 3 times or more
        assert declined(150000, 1 << 23, 0, 9999, lpe, 0)                  # the table slice fits the L2s
        assert declined(150000, 1 << 23, 0, (1 << 23) - 1, lpe, 0)         # one use per table row
    m = case("3")
    for order in ("cols", "rows"):
        p = run_plan(lib, m, 16, order, True, force=False)                 # a declined part: nothing is planned
        assert p["waves"] == 0 and p["n_slots"] == 0 and all(len(p[name]) == 0 for name, _ in ARRAYS)
