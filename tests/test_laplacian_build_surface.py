"""Host side of the HIP Laplacian builder: the C ABI symbols, the gfx950 kernels in the library, argument errors before any launch,
and the public switches of `Matrix`."""
import ctypes as C
import os
import re

import pandas as pd
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ngcf_laplacian_limits": ("int", 2), "ngcf_laplacian_workspace_bytes": ("int64_t", 2), "ngcf_laplacian_bucket": ("int", 16),
           "ngcf_laplacian_resolve": ("int", 23), "ngcf_laplacian_emit": ("int", 23), "ngcf_laplacian_item_rows": ("int", 8),
           "ngcf_laplacian_drop_zeros": ("int", 13)}
KERNELS = (b"lap_bucket_count_kernel", b"lap_bucket_scatter_kernel", b"lap_resolve_wave_kernel", b"lap_resolve_block_kernel",
           b"lap_resolve_long_kernel", b"lap_item_degree_kernel", b"lap_emit_kernel", b"lap_item_rows_kernel", b"lap_drop_zeros_kernel",
           b"lap_scan_write_kernel")


def test_header_declares_and_library_exports_the_family():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib, engine
    raw = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name, (ret, n_args) in SYMBOLS.items():
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert any(p.endswith("laplacian.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    for k in KERNELS:
        assert k in blob, k                                                       # gfx950 kernels of its own
    m = re.search(r"#define\s+NGCF_ABI_VERSION\s+(\d+)", raw)
    assert int(m.group(1)) == int(lib.ngcf_version()) == _lib.ABI_VERSION
    wave, group = engine.laplacian_limits()                                       # the branch points the GPU tests are built around
    assert wave == 64 and group > wave and group & (group - 1) == 0
    assert lib.ngcf_laplacian_workspace_bytes(10, 10) >= 8 and lib.ngcf_laplacian_workspace_bytes(2 ** 30, 2 ** 30) == -1
    assert lib.ngcf_laplacian_workspace_bytes(-1, 1) == -1


def test_c_abi_argument_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.int64)          # host memory: a call that got as far as a launch would not return ERR_ARG
    p = buf.data_ptr()
    big = 2 ** 31

    def bucket(userid=p, itemid=p, rating=p, T=5, n_user=3, n_item=4, old_rowptr=p, count=p, bptr=p, b_item=p, b_seq=p, b_rating=p, info=p,
               ws=p, nb=64):
        return lib.ngcf_laplacian_bucket(userid, itemid, rating, T, n_user, n_item, old_rowptr, count, bptr, b_item, b_seq, b_rating, info,
                                         ws, nb, None)

    def resolve(old_rowptr=p, old_item=p, old_rating=p, old_nnz=2, bptr=p, b_item=p, b_seq=p, b_rating=p, T=5, n_user=3, n_item=4,
                n_block=0, n_long=0, t_item=p, t_rating=p, deg=p, rowptr=p, tables=None, n_tables=0, status=p, ws=p, nb=64):
        return lib.ngcf_laplacian_resolve(old_rowptr, old_item, old_rating, old_nnz, bptr, b_item, b_seq, b_rating, T, n_user, n_item,
                                          n_block, n_long, t_item, t_rating, deg, rowptr, tables, n_tables, status, ws, nb, None)

    def emit(old_rowptr=p, old_item=p, old_rating=p, old_nnz=2, bptr=p, T=5, t_item=p, t_rating=p, n_user=3, n_item=4, deg=p, rowptr=p,
             ds=p, nnz=6, s_item=p, s_rating=p, s_user=p, colidx=p, vals=p, vals_item=p, zeros=p, status=p):
        return lib.ngcf_laplacian_emit(old_rowptr, old_item, old_rating, old_nnz, bptr, T, t_item, t_rating, n_user, n_item, deg, rowptr,
                                       ds, nnz, s_item, s_rating, s_user, colidx, vals, vals_item, zeros, status, None)

    def item_rows(order=p, s_user=p, vals_item=p, nnz=6, colidx=p, vals=p, status=p):
        return lib.ngcf_laplacian_item_rows(order, s_user, vals_item, nnz, colidx, vals, status, None)

    def drop_zeros(rowptr=p, colidx=p, vals=p, n_rows=7, nnz=12, count=p, out_rowptr=p, out_colidx=p, out_vals=p, out_nnz=11, ws=p, nb=64):
        return lib.ngcf_laplacian_drop_zeros(rowptr, colidx, vals, n_rows, nnz, count, out_rowptr, out_colidx, out_vals, out_nnz, ws, nb, None)

    sizes = ((dict(n_user=-1), "negative count"), (dict(n_item=-1), "negative count"), (dict(T=-1), "negative count"),
             (dict(n_user=big - 4, n_item=4), "does not fit 31 bits"), (dict(n_user=1, n_item=big - 1), "does not fit 31 bits"),
             (dict(n_user=big), "does not fit 31 bits"), (dict(T=big), "more than 2^31 - 1"))
    cases = [(bucket, kw, msg) for kw, msg in sizes] + [(resolve, kw, msg) for kw, msg in sizes] + [(emit, kw, msg) for kw, msg in sizes]
    cases += [(bucket, {k: None}, "null argument") for k in ("userid", "itemid", "rating", "old_rowptr", "count", "bptr", "b_item", "b_seq",
                                                             "b_rating", "info", "ws")]
    cases += [(resolve, {k: None}, "null argument") for k in ("old_rowptr", "old_item", "old_rating", "bptr", "b_item", "b_seq", "b_rating",
                                                              "t_item", "t_rating", "deg", "rowptr", "status", "ws")]
    cases += [(resolve, dict(old_nnz=-1), "negative count"), (resolve, dict(n_tables=-1), "negative count"),
              (resolve, dict(n_block=-1), "negative count"), (resolve, dict(n_long=-2), "negative count"),
              (resolve, dict(n_tables=2), "null argument"), (resolve, dict(n_long=1), "long rows and no table")]
    cases += [(emit, {k: None}, "null argument") for k in ("old_rowptr", "old_item", "old_rating", "bptr", "t_item", "t_rating", "deg", "rowptr",
                                                           "ds", "s_item", "s_rating", "s_user", "colidx", "vals", "vals_item", "zeros", "status")]
    cases += [(emit, dict(old_nnz=-1), "negative count"), (emit, dict(nnz=-1), "negative count")]
    cases += [(item_rows, {k: None}, "null argument") for k in ("order", "s_user", "vals_item", "colidx", "vals", "status")]
    cases += [(item_rows, dict(nnz=-1), "negative count")]
    cases += [(drop_zeros, {k: None}, "null argument") for k in ("rowptr", "colidx", "vals", "count", "out_rowptr", "out_colidx", "out_vals", "ws")]
    cases += [(drop_zeros, dict(n_rows=-1), "negative count"), (drop_zeros, dict(nnz=-1), "negative count"),
              (drop_zeros, dict(out_nnz=-1), "negative count"), (drop_zeros, dict(n_rows=big), "does not fit 31 bits")]
    for fn, kw, msg in cases:
        assert fn(**kw) == _lib.ERR_ARG, (fn.__name__, kw)
        err = _lib.last_error()
        assert err.startswith("laplacian: " + fn.__name__) and msg in err, (fn.__name__, kw, err)
    for fn in (bucket, resolve, drop_zeros):                                      # a short workspace is its own error, also before any launch
        assert fn(nb=0) == _lib.ERR_WORKSPACE and "laplacian:" in _lib.last_error()
    assert item_rows(nnz=0, order=None, s_user=None, vals_item=None, colidx=None, vals=None) == _lib.OK      # nothing to do is not an error
    with pytest.raises(RuntimeError, match="laplacian: bucket: null argument"):
        _lib.check(bucket(info=None))
    wave, group = C.c_int(0), C.c_int(0)
    assert lib.ngcf_laplacian_limits(C.byref(wave), None) == _lib.OK and lib.ngcf_laplacian_limits(None, C.byref(group)) == _lib.OK
    assert (wave.value, group.value) == (64, 2048)


def test_python_surface_refuses_the_cpu_and_unknown_builders():
    from seoul_tourism_recommendation_ngcf_amd import engine
    from seoul_tourism_recommendation_ngcf_amd.matrix import LaplacianSlice, Matrix, laplacian_csr_slices
    df = pd.DataFrame({"year": [18, 19], "userid": [0, 1], "itemid": [1, 0], "visitor": [1.0, 2.0]})
    args = (df, ["year", "userid", "itemid", "visitor"], "visitor", {"user": 2, "item": 2})
    with pytest.raises(RuntimeError, match="ROCm device"):
        Matrix(*args, builder="device", device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        Matrix(*args, builder="device")                                           # the default device is the CPU
    with pytest.raises(ValueError, match="builder='nonsense'"):
        Matrix(*args, builder="nonsense")
    m = Matrix(*args)
    assert m.builder == "torch" and len(m.create_matrix()) == 2                    # the default is the torch builder, as before
    with pytest.raises(RuntimeError, match="ROCm device"):
        laplacian_csr_slices(df["year"].values, df["userid"].values, df["itemid"].values, df["visitor"].values, 2, 2, "cpu")
    state = engine.empty_laplacian_state(2, "cpu")
    assert state[0].tolist() == [0, 0, 0] and state[1].dtype == torch.int32 and state[2].dtype == torch.float32
    i64, f32 = torch.zeros(2, dtype=torch.int64), torch.ones(2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        engine.build_laplacian_year(state, i64, i64, f32, 2, 2)
    with pytest.raises(TypeError, match="userid must be torch.int64"):
        engine.build_laplacian_year(state, i64.int(), i64, f32, 2, 2)
    with pytest.raises(ValueError, match="differ in length"):
        engine.build_laplacian_year(state, i64, i64[:1], f32, 2, 2)
    # a slice's COO view is plain torch: rows expanded from rowptr, columns widened
    sl = LaplacianSlice(torch.tensor([0, 2, 2, 3]), torch.tensor([1, 2, 0], dtype=torch.int32), torch.tensor([1.0, 2.0, 3.0]), 3)
    rows, cols, vals = sl.coo()
    assert rows.tolist() == [0, 0, 2] and cols.dtype == torch.int64 and cols.tolist() == [1, 2, 0] and sl.nnz == 3
    L = sl.sparse_coo()
    assert L.is_sparse and not L.is_coalesced() and tuple(L.shape) == (3, 3) and L.to_dense()[2, 0] == 3.0
    d = engine.inverse_sqrt_degree(torch.tensor([0, 1, 4], dtype=torch.int32).numpy())
    assert d.dtype.name == "float32" and d.tolist() == [0.0, 1.0, 0.5]
