"""Host side of the per-user quartile floor: the C ABI symbol, argument errors before any launch, the public module on CPU tensors,
and the test oracle (tests/quantile_oracle.py) pinned bit for bit to the reference-shaped pandas loop and to np.percentile."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import quantile_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "ngcf_segment_quantile_floor_f64"


def test_header_declares_and_library_exports_the_symbol():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    lib = _lib.load()
    assert hasattr(lib, SYMBOL) and SYMBOL in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES[SYMBOL][1]) == 14
    assert any(p.endswith("quantile.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    assert b"segment_quantile_wave_kernel" in blob and b"segment_quantile_block_kernel" in blob      # gfx950 kernels of its own
    assert int(lib.ngcf_version()) == _lib.ABI_VERSION


def test_c_abi_argument_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(8, dtype=torch.int64)          # host memory: a call that got as far as a launch would not return ERR_ARG
    p = buf.data_ptr()

    def call(rowptr=p, n_rows=3, order=p, x=p, T=5, mean=0.0, scale=1.0, shift=0.0, q4=1, wave_max=0, quant=p, out=p, status=p):
        return getattr(lib, SYMBOL)(rowptr, n_rows, order, x, T, mean, scale, shift, q4, wave_max, quant, out, status, None)
    assert call(T=0) == _lib.OK and call(n_rows=0) == _lib.OK                    # nothing to do is not an error
    assert call(T=0, rowptr=None, order=None, x=None, quant=None, out=None, status=None) == _lib.OK
    cases = ((dict(q4=0), "q4=0 outside [1, 3]"), (dict(q4=4), "q4=4 outside [1, 3]"), (dict(q4=-1), "outside [1, 3]"),
             (dict(wave_max=-1), "wave_max=-1 outside [0, 64]"), (dict(wave_max=65), "wave_max=65 outside [0, 64]"),
             (dict(scale=0.0), "not a finite positive number"), (dict(scale=-1.0), "not a finite positive number"),
             (dict(scale=float("inf")), "not a finite positive number"), (dict(scale=float("nan")), "not a finite positive number"),
             (dict(T=-1), "negative count"), (dict(n_rows=-1), "negative count"),
             (dict(rowptr=None), "null argument"), (dict(x=None), "null argument"), (dict(quant=None), "null argument"),
             (dict(out=None), "null argument"), (dict(status=None), "null argument"))
    for kw, msg in cases:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert "segment_quantile_floor" in _lib.last_error() and msg in _lib.last_error(), (kw, _lib.last_error())
    # the limits that pass reach the null check; `order` may be null
    assert call(q4=3, wave_max=64, scale=5e-324, order=None, out=None) == _lib.ERR_ARG and "null argument" in _lib.last_error()
    assert call(q4=0, T=0) == _lib.ERR_ARG                                      # an argument error even with nothing to do
    with pytest.raises(RuntimeError, match="outside"):
        _lib.check(call(q4=4))


def test_engine_wrappers_check_arguments_on_the_host():
    from seoul_tourism_recommendation_ngcf_amd import engine
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64)  # noqa: E731
    with pytest.raises(RuntimeError, match="ROCm device"):                        # CPU tensors: no fallback, and no launch
        engine.segment_quantile_floor(i64(4), f64(5))
    for args, kw, exc, msg in (((i64(4), f64(5)), dict(q=0.3), ValueError, "q=0.3 is not one of"),
                               ((i64(4), f64(5)), dict(wave_max=65), ValueError, "wave_max=65"),
                               ((i64(4), f64(5)), dict(scale=0.0), ValueError, "scale=0.0"),
                               ((i64(4), f64(5)), dict(scale=float("inf")), ValueError, "scale=inf"),
                               ((i64(4).int(), f64(5)), {}, TypeError, "rowptr must be int64"),
                               ((i64(4), f64(5).float()), {}, TypeError, "x must be float64"),
                               ((i64(4), f64(5)), dict(order=i64(5).int()), TypeError, "order must be int64"),
                               ((i64(4), f64(5)), dict(order=i64(4)), ValueError, r"order must be \[T = 5\]"),
                               ((i64(4), f64(5)), dict(out=f64(4)), ValueError, r"out must be \[T = 5\]"),
                               ((i64(4), f64(5)), dict(quant=f64(4)), ValueError, r"quant must be \[n_rows = 3\]"),
                               ((i64(4), f64(5)), dict(out=f64(5).float()), TypeError, "out must be float64"),
                               ((i64(0), f64(5)), {}, ValueError, "rowptr must be"),
                               ((i64(4), f64(5, 1)), {}, ValueError, r"x must be \[T\]")):
        with pytest.raises(exc, match=msg):
            engine.segment_quantile_floor(*args, **kw)
    sig = inspect.signature(engine.segment_quantile_floor)
    assert list(sig.parameters) == ["rowptr", "x", "order", "mean", "scale", "shift", "q", "wave_max", "out", "quant", "status"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert [sig.parameters[k].default for k in ("mean", "scale", "shift", "q", "wave_max")] == [0.0, 1.0, 0.0, 0.25, 0]
    assert list(inspect.signature(engine.segments_from_ids).parameters) == ["ids", "n_rows"]
    # segments_from_ids is plain torch plumbing: it runs where the ids live
    ids = torch.tensor([2, 0, 2, 4, 0, 2])
    rowptr, order = engine.segments_from_ids(ids, 6)
    assert rowptr.tolist() == [0, 2, 2, 5, 5, 6, 6] and order.tolist() == [1, 4, 0, 2, 5, 3]
    want = quantile_oracle.segments_of(ids.numpy(), 6)
    assert all(order[rowptr[u]:rowptr[u + 1]].tolist() == want[u].tolist() for u in range(6))
    rowptr, order = engine.segments_from_ids(i64(0), 3)
    assert rowptr.tolist() == [0, 0, 0, 0] and order.numel() == 0
    for bad in (torch.tensor([0, 6]), torch.tensor([-1, 0])):
        with pytest.raises(IndexError, match="outside"):
            engine.segments_from_ids(bad, 6)
    with pytest.raises(TypeError, match="int64"):
        engine.segments_from_ids(ids.int(), 6)


def test_preprocess_is_exported():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    assert "preprocess" in pkg.__all__
    pre = pkg.preprocess
    assert list(inspect.signature(pre.standard_stats).parameters) == ["x"]
    sig = inspect.signature(pre.scale_implicit)
    assert list(sig.parameters) == ["users", "visitors", "n_user", "scaler", "q", "stats"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("n_user", "scaler", "q", "stats"))
    assert sig.parameters["scaler"].default == "standard" and sig.parameters["q"].default == 0.25 and sig.parameters["stats"].default is None
    assert sig.parameters["n_user"].default is inspect.Parameter.empty
    assert list(inspect.signature(pre.positives).parameters) == ["ratings"]
    users, counts = torch.tensor([0, 1, 1, 2]), torch.tensor([3, 1, 4, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):                        # no CPU fallback
        pre.scale_implicit(users, counts, n_user=3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pre.scale_implicit(users, counts, n_user=3, scaler=None)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pre.scale_implicit(users, counts, n_user=3, stats=(0.0, 1.0, 0.0))
    with pytest.raises(RuntimeError, match="ROCm device"):
        pre.standard_stats(counts)
    with pytest.raises(NotImplementedError, match="Yeo-Johnson"):
        pre.scale_implicit(users, counts, n_user=3, scaler="power")
    with pytest.raises(ValueError, match="scaler='minmax'"):
        pre.scale_implicit(users, counts, n_user=3, scaler="minmax")
    with pytest.raises(ValueError, match="users \\[T\\] and visitors \\[T\\]"):
        pre.scale_implicit(users, counts[:3], n_user=3)
    assert pre.positives(torch.tensor([0.0, -0.0, 1e-300, 2.0], dtype=torch.float64)).tolist() == [False, False, True, True]
    for word in ("power", "map_ids", "split_train_test", "index-alignment"):     # the gaps are named where a user looks
        assert word in pre.__doc__


# ---- the oracle against the libraries the reference calls ---------------------------------------------------------------------------
LENGTHS = tuple(range(1, 10)) + (63, 64, 65, 66, 255, 256, 257, 258, 1025)


def _columns():
    """The two data sets, each with a user column whose segment lengths are LENGTHS, rows shuffled."""
    rng = np.random.default_rng(20240607)
    users = rng.permutation(np.repeat(np.arange(len(LENGTHS)), LENGTHS))
    T = len(users)
    counts = rng.integers(0, 50, T).astype(np.float64)                           # integer counts in 0-49 ...
    counts[rng.random(T) < 0.02] *= 1000.0                                       # ... 2 % scaled x1000
    normals = rng.standard_normal(T)
    normals[7::7] = normals[6:-1:7]                                              # every 7th value duplicated
    return users, {"counts": counts, "normals": normals}


def test_oracle_equals_the_reference_shaped_pandas_loop():
    pd = pytest.importorskip("pandas")
    StandardScaler = pytest.importorskip("sklearn.preprocessing").StandardScaler
    users, cols = _columns()
    segments = quantile_oracle.segments_of(users, len(LENGTHS))
    assert [len(s) for s in segments] == list(LENGTHS)
    for name, col in cols.items():
        # utils.py:110-121 on a frame of (userid, rating)
        df = pd.DataFrame({"userid": users, "rating": col})
        if name == "counts":
            scaler = StandardScaler()
            df[["rating"]] = pd.DataFrame(scaler.fit_transform(df[["rating"]]))
            v_min = np.abs(df["rating"].min())
            df["rating"] = df["rating"] + v_min
            stats = dict(mean=scaler.mean_[0], scale=scaler.scale_[0], shift=v_min)
        else:
            stats = {}
        quarters = {}
        for userid in df["userid"].unique():
            tmp = df.loc[df["userid"].isin([userid])]
            quarter = tmp["rating"].quantile(q=0.25)
            neg_tmp = tmp.loc[tmp["rating"] < quarter]
            df.loc[neg_tmp.index, "rating"] = 0
            quarters[int(userid)] = quarter
        out, quant = quantile_oracle.floor_segments(segments, col, 1, **stats)
        assert np.array_equal(out, df["rating"].to_numpy()), name
        assert np.array_equal(quant, np.array([quarters[u] for u in range(len(LENGTHS))])), name
        assert (out == 0).sum() > len(LENGTHS)                                    # the floor did something
        if name == "counts":
            assert out.min() == 0.0 and (out >= 0).all()


def test_oracle_equals_numpy_percentile_for_the_other_quartiles():
    pytest.importorskip("pandas")
    pytest.importorskip("sklearn")
    users, cols = _columns()
    segments = quantile_oracle.segments_of(users, len(LENGTHS))
    for name, col in cols.items():
        stats = dict(mean=col.mean(), scale=col.std(), shift=1.25) if name == "counts" else {}
        z = quantile_oracle.transform(col, **stats)
        for q4 in (1, 2, 3):
            out, quant = quantile_oracle.floor_segments(segments, col, q4, **stats)
            want_q = np.array([np.percentile(z[s], 25.0 * q4, method="linear") for s in segments])
            assert np.array_equal(quant, want_q), (name, q4)
            want = z.copy()
            for s, qv in zip(segments, want_q):
                want[s[z[s] < qv]] = 0.0
            assert np.array_equal(out, want), (name, q4)


def test_oracle_edges():
    out, quant = quantile_oracle.floor_segments([np.array([], dtype=np.int64), np.array([0]), np.array([1, 2])],
                                                np.array([5.0, np.nan, 1.0]))
    assert np.isnan(quant[0]) and quant[1] == 5.0 and np.isnan(quant[2])
    assert out[0] == 5.0 and np.isnan(out[1]) and out[2] == 1.0                   # a NaN segment passes through
    assert quantile_oracle.quantile_sorted(np.array([1.0, 2.0, 4.0, 8.0]), 1) == 1.75
    assert quantile_oracle.quantile_sorted(np.array([1.0, 2.0, 4.0, 8.0]), 3) == 5.0
