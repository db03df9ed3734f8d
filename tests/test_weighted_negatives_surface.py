"""Host-side surface of the popularity-weighted negatives: the two C ABI symbols, argument errors before any launch and before any
device work, `engine.negatives`, and `sampling.popularity_weights` on CPU tensors against hand values."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_weighted_draw():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib, engine
    text = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert re.search(r"^#define\s+NGCF_SAMPLE_WEIGHTED_M_MAX\s+64\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+NGCF_ABI_VERSION\s+11\s*$", text, flags=re.M)
    for line in ("r'  = mulhi64(fmix(a + (j + 1) * 0xD1B54A32D192ED03), U_j)", "K   = #{k : gap_k <= r}", "tgt = r + S_K",
                 "c_j = the largest i with cdf[i] <= tgt", "q_j = cdf[c_j] - S_K"):
        assert line in text, line                                                 # the recipe stands in the header in full
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, n_args in (("ngcf_weighted_prepare", 10), ("ngcf_sample_weighted", 20)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code)
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args
    assert any(p.endswith("sample_weighted.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    for kernel in (b"weighted_prepare_kernel", b"sample_weighted_one_kernel", b"sample_weighted_wave_kernel"):
        assert kernel in blob                                                     # gfx950 kernels of its own
    assert int(lib.ngcf_version()) == _lib.ABI_VERSION == 11
    assert engine.negatives.WEIGHTED_M_MAX == 64 and engine.negatives.WEIGHT_MAX == 2 ** 40
    for name in ("weighted_unseen", "WeightedSets", "WEIGHTED_M_MAX"):             # the flat namespace is pinned
        assert hasattr(engine.negatives, name) and not hasattr(engine, name)


def test_c_abi_limits_are_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    p = torch.zeros(4, dtype=torch.int64).data_ptr()     # host memory: a call that got as far as a launch would not return ERR_ARG

    def draw(m=8, n_items=100, T=3, n_rows=5, ld_out=None, ld_weight=None, rowptr=p, colidx=p, cdf=p, gap=p, mass=p, user_ids=p, out=p,
             draw_weight=None, case_mass=None, status=p):
        return lib.ngcf_sample_weighted(rowptr, colidx, 0, n_rows, n_items, cdf, gap, mass, user_ids, T, 0, m, 2024, out,
                                        m if ld_out is None else ld_out, draw_weight, m if ld_weight is None else ld_weight, case_mass,
                                        status, None)
    assert draw(T=0) == _lib.OK                                                   # no cases: nothing to do
    assert draw(T=0, rowptr=None, colidx=None, cdf=None, gap=None, mass=None, user_ids=None, out=None, status=None) == _lib.OK
    cases = ((dict(m=0), "m=0 outside [1, 64]"), (dict(m=65), "m=65 outside [1, 64]"), (dict(m=-1), "outside [1, 64]"),
             (dict(n_items=0), "n_items=0 outside [1, 2^31)"), (dict(n_items=2 ** 31), "outside [1, 2^31)"),
             (dict(ld_out=7), "ld_out=7 is below the 8 columns"), (dict(draw_weight=p, ld_weight=7), "ld_weight=7 is below the 8 columns"),
             (dict(T=-1), "bad argument"), (dict(n_rows=-1), "bad argument")) + tuple(
        (({name: None}), "null argument") for name in ("rowptr", "colidx", "cdf", "gap", "mass", "user_ids", "out", "status"))
    for kw, msg in cases:
        assert draw(**kw) == _lib.ERR_ARG, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    # the largest that pass the limits stop at the null `out`; a null draw_weight takes no ld_weight
    assert draw(m=64, n_items=2 ** 31 - 1, out=None) == _lib.ERR_ARG and "null argument" in _lib.last_error()
    assert draw(ld_weight=0, out=None) == _lib.ERR_ARG and "null argument" in _lib.last_error()

    def prepare(n_items=100, n_rows=5, rowptr=p, colidx=p, cdf=p, gap=p, mass=p, status=p):
        return lib.ngcf_weighted_prepare(rowptr, colidx, 0, n_rows, n_items, cdf, gap, mass, status, None)
    assert prepare(n_rows=0) == _lib.OK and prepare(n_rows=0, rowptr=None, cdf=None, gap=None, mass=None, status=None) == _lib.OK
    for kw, msg in ((dict(n_items=0), "n_items=0 outside [1, 2^31)"), (dict(n_items=2 ** 31), "outside [1, 2^31)"),
                    (dict(n_rows=-1), "bad argument")) + tuple(
            (({name: None}), "null argument") for name in ("rowptr", "colidx", "cdf", "gap", "mass", "status")):
        assert prepare(**kw) == _lib.ERR_ARG, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())


def _cpu_sets(n_rows=5, n_items=100):
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.ItemSets(torch.zeros(n_rows + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 0, n_items)


def _cpu_wsets(n_rows=5, n_items=100):
    """A WeightedSets with host arrays, as no constructor makes one: enough for the checks that come before any device work."""
    from seoul_tourism_recommendation_ngcf_amd import engine
    w = engine.negatives.WeightedSets.__new__(engine.negatives.WeightedSets)
    w.seen = _cpu_sets(n_rows, n_items)
    w.cdf, w.gap, w.mass = torch.arange(n_items + 1), torch.zeros(1, dtype=torch.int64), torch.full((n_rows,), n_items)
    w._colidx, w.total = torch.zeros(1, dtype=torch.int32), n_items
    return w


def test_wrapper_argument_errors_come_before_any_device_work():
    from seoul_tourism_recommendation_ngcf_amd import engine, sampling
    neg = engine.negatives
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)  # noqa: E731
    ones = torch.ones(100, dtype=torch.int64)
    # WeightedSets: the weights' type and length, then the device
    for weights, exc, msg in ((ones.double(), TypeError, "weights must be int64"), (ones.int(), TypeError, "weights must be int64"),
                              (ones[:99], ValueError, r"weights must be \[n_items = 100\]"), (ones[None], ValueError, "weights must be"),
                              (ones, RuntimeError, "ROCm device")):
        with pytest.raises(exc, match=msg):
            neg.WeightedSets(_cpu_sets(), weights)
    with pytest.raises(ValueError, match="n_items"):
        neg.WeightedSets(_cpu_sets(n_items=2 ** 31), torch.ones(1, dtype=torch.int64).expand(2 ** 31))
    # weighted_unseen
    w = _cpu_wsets()
    assert w.n_rows == 5 and w.n_items == 100
    for args, kw, exc, msg in (((w, i64(3), 0, 1), {}, ValueError, "m=0 outside"), ((w, i64(3), 65, 1), {}, ValueError, "m=65 outside"),
                               ((w.seen, i64(3), 8, 1), {}, TypeError, "must be a WeightedSets"),
                               ((w, i64(3).int(), 8, 1), {}, TypeError, "user_ids must be int64"),
                               ((w, i64(3, 1), 8, 1), {}, ValueError, r"user_ids must be \[T\]"),
                               ((w, i64(3), 8, 1), dict(out=i64(4, 8)), ValueError, r"out must be \[T = 3, >= 8\]"),
                               ((w, i64(3), 8, 1), dict(out=i64(3, 7)), ValueError, "out must be"),
                               ((w, i64(3), 8, 1), dict(out=i64(24)), ValueError, "out must be"),
                               ((w, i64(3), 8, 1), dict(out=i64(3, 8).int()), TypeError, "out must be int64"),
                               ((w, i64(3), 8, 1), {}, RuntimeError, "ROCm device")):      # CPU tensors: no fallback, and no launch
        with pytest.raises(exc, match=msg):
            neg.weighted_unseen(*args, **kw)
    sig = inspect.signature(neg.weighted_unseen)
    assert list(sig.parameters) == ["wsets", "user_ids", "m", "seed", "case_offset", "return_weights", "out", "status"]
    keyword_only = ("case_offset", "return_weights", "out", "status")
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keyword_only)
    assert [sig.parameters[k].default for k in keyword_only] == [0, False, None, None]
    # sampling: m, the weights' type and length before anything else
    rows = i64(3)
    kw = dict(seed=1, n_user=4, n_item=100)
    for weights, m, exc, msg in ((ones, 0, ValueError, "m=0 outside"), (ones, 65, ValueError, "m=65 outside"),
                                 (ones.float(), 8, TypeError, "weights must be int64"),
                                 (ones[:99], 8, ValueError, r"weights must be \[n_item = 100\]"), (ones, 8, RuntimeError, "ROCm device")):
        with pytest.raises(exc, match=msg):
            sampling.weighted_negatives(rows, rows, weights, m=m, **kw)
    with pytest.raises(TypeError, match="weights must be int64"):
        sampling.weighted_triplets(rows, rows, ones.float(), **kw)
    with pytest.raises(RuntimeError, match="ROCm device"):
        sampling.weighted_triplets(rows, rows, ones, **kw)
    for bad, exc in ((dict(m=0), ValueError), (dict(m=65), ValueError), (dict(batch_size=0), ValueError)):
        with pytest.raises(exc):
            sampling.WeightedNegativesLoader(rows, rows, ones, **{**dict(batch_size=2, m=4, seed=1), **bad})
    with pytest.raises(TypeError, match="weights must be an int64"):
        sampling.WeightedNegativesLoader(rows, rows, ones.float(), batch_size=2, m=4, seed=1)
    with pytest.raises(ValueError, match="every column"):
        sampling.WeightedNegativesLoader(rows, rows[:-1], ones, batch_size=2, m=4, seed=1)
    sig = inspect.signature(sampling.WeightedNegativesLoader.__init__)
    assert list(sig.parameters) == ["self", "users", "items", "weights", "columns", "batch_size", "m", "seed", "shuffle", "drop_last",
                                    "generator", "seen"]
    sig = inspect.signature(sampling.weighted_negatives)
    assert list(sig.parameters) == ["users", "items", "weights", "seen", "m", "seed", "epoch", "n_user", "n_item", "return_logq"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("m", "seed", "epoch", "n_user", "n_item", "return_logq"))


def test_popularity_weights_against_hand_values():
    from seoul_tourism_recommendation_ngcf_amd import sampling
    items = torch.tensor([0, 0, 0, 0, 2, 2, 5, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6])        # counts 4, 0, 2, 0, 0, 1, 16
    counts = [4, 0, 2, 0, 0, 1, 16, 0]
    assert sampling.popularity_weights(items, 8, alpha=1).tolist() == counts
    assert sampling.popularity_weights(items, 8, alpha=0).tolist() == [1] * 8
    # 4^0.75 = 2.8284.., 2^0.75 = 1.6817.., 16^0.75 = 8: times 1024 and rounded to nearest: 2896.3 -> 2896, 1722.2 -> 1722, 8192
    got = sampling.popularity_weights(items, 8)
    assert got.dtype == torch.int64 and got.tolist() == [2896, 0, 1722, 0, 0, 1024, 8192, 0]
    assert sampling.popularity_weights(items, 8, alpha=0.75, resolution=1024).tolist() == got.tolist()
    assert sampling.popularity_weights(items, 8, 0.75, 1).tolist() == [3, 0, 2, 0, 0, 1, 8, 0]
    # a flat exponent at resolution 1: 16^0.1 = 1.32, 4^0.1 = 1.15, 2^0.1 = 1.07 all round to 1; a count of 0 stays 0
    assert sampling.popularity_weights(items.int(), 8, 0.1, 1).tolist() == [1, 0, 1, 0, 0, 1, 1, 0]
    assert sampling.popularity_weights(items[:0], 3).tolist() == [0, 0, 0]
    with pytest.raises(IndexError):
        sampling.popularity_weights(items, 6)
    with pytest.raises(ValueError):
        sampling.popularity_weights(items.float(), 8)
    sig = inspect.signature(sampling.popularity_weights)
    assert list(sig.parameters) == ["items", "n_item", "alpha", "resolution"]
    assert sig.parameters["alpha"].default == 0.75 and sig.parameters["resolution"].default == 1024
