"""Host side of the train/test split: the C ABI symbols and their gfx950 kernels, the public functions of `engine` and `preprocess`,
`stratified_counts` against recorded and live sklearn results, the year quota against pandas' rule, the statistics of the numpy
oracle of tests/split_oracle.py (the device equals it bit for bit, tests/test_split_gpu.py), and the refusals that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import split_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ngcf_select_limits": ("int", 3), "ngcf_select_key": ("uint64_t", 2), "ngcf_select_per_group": ("int", 11)}
KERNELS = (b"select_hist_kernel", b"select_pick_kernel", b"select_mark_kernel")

# class sizes -> the test counts sklearn's train_test_split(test_size=0.3, stratify=) gave for three random states; none cuts a tie
RECORDED = [([1000, 3, 2, 17, 64, 65, 129, 700, 41, 5], [300, 1, 1, 5, 19, 20, 39, 210, 12, 1], 608, 2026),
            ([7, 11, 13, 29, 31, 2, 2, 97, 250, 3], [2, 3, 4, 9, 9, 1, 1, 29, 75, 1], 134, 445),
            ([10, 10, 10, 10], [3, 3, 3, 3], 12, 40),
            ([2037, 2, 300, 64, 5, 1000, 77], [611, 1, 90, 19, 2, 300, 23], 1046, 3485)]


def test_header_declares_and_library_exports_the_family():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib, engine
    raw = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name, (ret, n_args) in SYMBOLS.items():
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert any(p.endswith("select.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    for k in KERNELS:
        assert k in blob, k
    # the key and the rule are written out where a caller of the C ABI looks
    for word in ("0x9E3779B97F4A7C15", "k_t <= tau_g", "1 KiB + 16 B per group", "NGCF_SELECT_GROUP", "NGCF_SELECT_QUOTA"):
        assert word in raw, word
    lds_groups, nbytes = engine.select_limits(100)
    assert lds_groups >= 100 and lds_groups * 256 * 4 <= 160 * 1024          # the table of the LDS tier fits a CU's LDS
    assert nbytes == 100 * (1024 + 16) and engine.select_limits(lds_groups + 1)[1] == (lds_groups + 1) * 1040
    assert engine.select_limits(0)[1] == -1 and engine.select_limits(2 ** 31)[1] == -1
    for seed, t in ((0, 0), (1, 0), (5, 7), (2 ** 64 - 1, 2 ** 31 - 2), (1234567, 49_999_999)):
        x = (seed ^ (t * 0x9E3779B97F4A7C15)) & (2 ** 64 - 1)
        assert engine.select_key(seed, t) == int(orc.fmix(np.array([x], dtype=np.uint64))[0])
    assert [engine.select_key(77, t) for t in range(50)] == orc.keys(77, 50).tolist()
    _lib.set_option("select_no_lds", 1)                                    # the knob that forces the memory tier exists
    _lib.options_from_env()


def test_c_abi_argument_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(512, dtype=torch.int64)         # host memory: a call that got as far as a launch would not return ERR_ARG
    p = buf.data_ptr()
    assert p % 16 == 0

    def sel(group=p, T=5, G=2, quota=p, mask=p, thr=None, status=p, ws=p, nb=4096):
        return lib.ngcf_select_per_group(group, T, G, quota, 0, mask, thr, status, ws, nb, None)

    cases = [(dict(T=-1), "T=-1"), (dict(T=2 ** 31), "outside [0, 2^31)"), (dict(G=0), "G=0"), (dict(G=2 ** 31), "G=2147483648"),
             (dict(group=None), "one group"), (dict(quota=None), "null argument"), (dict(mask=None), "null argument"),
             (dict(status=None), "null argument"), (dict(ws=None), "null argument"), (dict(ws=p + 8), "16-byte aligned")]
    for kw, msg in cases:
        assert sel(**kw) == _lib.ERR_ARG, kw
        assert _lib.last_error().startswith("select: ") and msg in _lib.last_error(), (kw, _lib.last_error())
    assert sel(nb=2 * 1040 - 1) == _lib.ERR_WORKSPACE and "2080 needed" in _lib.last_error()


def test_python_surface_signatures_and_refusals():
    from seoul_tourism_recommendation_ngcf_amd import engine, preprocess
    sig = inspect.signature(engine.select_per_group)
    assert list(sig.parameters)[:5] == ["group", "quota", "seed", "n_rows", "return_thresholds"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("seed", "n_rows", "return_thresholds"))
    assert sig.parameters["seed"].default is inspect.Parameter.empty and sig.parameters["n_rows"].default is None
    assert sig.parameters["return_thresholds"].default is False
    assert callable(engine.select_limits)
    sig = inspect.signature(preprocess.stratified_counts)
    assert list(sig.parameters) == ["counts", "test_size", "seed"] and sig.parameters["test_size"].default == 0.3
    assert sig.parameters["seed"].default == 0 and sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(preprocess.split_stratified)
    assert list(sig.parameters) == ["strata", "test_size", "seed"] and sig.parameters["test_size"].default == 0.3
    assert sig.parameters["seed"].default is inspect.Parameter.empty
    sig = inspect.signature(preprocess.split_by_year)
    assert list(sig.parameters) == ["year", "train_year", "test_year", "frac", "seed"]
    assert [sig.parameters[n].default for n in ("train_year", "test_year", "frac")] == [18, 19, 0.3]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("train_year", "test_year", "frac", "seed"))
    doc = preprocess.__doc__
    assert "`split_by_year` / `split_stratified`" in doc and "`split_train_test` (`graphs.holdout_split` exists)" not in doc
    for fn in (preprocess.split_by_year, preprocess.split_stratified):
        assert "Deviation" in fn.__doc__ and "permuted order" in fn.__doc__
    assert "fmix(seed ^ class)" in preprocess.stratified_counts.__doc__

    g32 = torch.arange(6, dtype=torch.int32) % 2
    # error paths that need no device, in the order the arguments are looked at
    with pytest.raises(ValueError, match="a quota is negative"):
        engine.select_per_group(g32, [3, -1], seed=0)
    with pytest.raises(ValueError, match="a quota is negative"):
        engine.select_per_group(None, torch.tensor([-5]), seed=0, n_rows=9)
    with pytest.raises(TypeError, match="int32"):
        engine.select_per_group(g32.long(), [1, 1], seed=0)
    with pytest.raises(TypeError, match="integers"):
        engine.select_per_group(g32, [1.0, 1.0], seed=0)
    with pytest.raises(ValueError, match="n_rows says"):
        engine.select_per_group(None, [1], seed=0)
    with pytest.raises(ValueError, match="one group"):
        engine.select_per_group(None, [1, 1], seed=0, n_rows=4)
    with pytest.raises(ValueError, match="n_rows=5 beside"):
        engine.select_per_group(g32, [1, 1], seed=0, n_rows=5)
    with pytest.raises(ValueError, match="must be \\[T\\]"):
        engine.select_per_group(g32.view(2, 3), [1, 1], seed=0)
    with pytest.raises(ValueError, match="quota must be"):
        engine.select_per_group(g32, [], seed=0)
    with pytest.raises(ValueError, match="outside \\[0, 2\\^31\\)"):
        engine.select_per_group(None, [1], seed=0, n_rows=2 ** 31)
    with pytest.raises(ValueError, match="out must be"):
        engine.select_per_group(g32, [1, 1], seed=0, out=torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        engine.select_per_group(g32, [1, 1], seed=0)
    with pytest.raises(RuntimeError, match="ROCm device"):
        engine.select_per_group(None, [1], seed=0, n_rows=4, device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        preprocess.split_stratified(g32, seed=0)
    with pytest.raises(RuntimeError, match="ROCm device"):
        preprocess.split_by_year(g32 + 18, seed=0)
    # a class of one row; a test size outside (0, 1); fewer test rows than classes
    with pytest.raises(ValueError, match="fewer than 2 rows"):
        preprocess.stratified_counts([5, 1, 9])
    with pytest.raises(ValueError, match="fewer than 2 rows"):
        preprocess.stratified_counts([5, 0, 9])
    for ts in (0.0, 1.0, -0.3, 1.5):
        with pytest.raises(ValueError, match="\\(0, 1\\) range"):
            preprocess.stratified_counts([5, 5], ts)
        with pytest.raises(ValueError, match="\\(0, 1\\) range"):
            preprocess.split_stratified(g32, test_size=ts, seed=0)
    with pytest.raises(ValueError, match="test size 2 .* number of classes 3"):
        preprocess.stratified_counts([2, 2, 2])
    with pytest.raises(ValueError, match="train size 2 .* number of classes 3"):
        preprocess.stratified_counts([2, 2, 2], 0.6)
    with pytest.raises(ValueError, match="integer array"):
        preprocess.stratified_counts([2.5, 3.0])
    with pytest.raises(ValueError, match="frac=1.5"):
        preprocess.split_by_year(g32, frac=1.5, seed=0)
    with pytest.raises(ValueError, match="both 19"):
        preprocess.split_by_year(g32, train_year=19, seed=0)
    with pytest.raises(TypeError, match="int32 or int64"):
        preprocess.split_by_year(g32.double(), seed=0)
    with pytest.raises(TypeError, match="int32 or int64"):
        preprocess.split_stratified(g32.float(), seed=0)


@pytest.mark.parametrize("counts,test,n_test,n", RECORDED)
def test_stratified_counts_equal_the_recorded_sklearn_results(counts, test, n_test, n):
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    assert sum(counts) == n and sum(test) == n_test
    for seed in (0, 1, 42):                                                # no tie is cut: the seed has no say
        tr, te = preprocess.stratified_counts(counts, 0.3, seed=seed)
        assert tr.dtype == te.dtype == np.int64
        assert te.tolist() == test and tr.tolist() == [c - t for c, t in zip(counts, test)]
    tr, te = preprocess.stratified_counts(np.array(counts, dtype=np.int32))  # the default test size is the reference's 0.3
    assert te.tolist() == test


def test_stratified_counts_cut_ties_by_the_documented_order():
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    from seoul_tourism_recommendation_ngcf_amd.sampling import fmix
    # five classes of 4 rows: 14 train rows = 2 each and 4 of the 5 equal remainders; the class left out gets 2 test rows
    for seed in range(6):
        tr, te = preprocess.stratified_counts([4] * 5, 0.3, seed=seed)
        assert tr.sum() == 14 and te.sum() == 6 and (tr + te).tolist() == [4] * 5
        last = sorted(range(5), key=lambda c: fmix(seed ^ c))[-1]
        assert tr.tolist() == [2 if c == last else 3 for c in range(5)]
        drawn, cut = preprocess._approximate_mode(np.array([4] * 5), 14, seed)
        assert cut and drawn.tolist() == tr.tolist()
    assert len({tuple(preprocess.stratified_counts([4] * 5, seed=s)[0].tolist()) for s in range(40)}) == 5   # every class is left out by some seed


def test_stratified_counts_equal_live_sklearn_where_no_tie_is_cut():
    pytest.importorskip("sklearn")
    from sklearn.model_selection import train_test_split
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    rs = np.random.RandomState(7)
    done = 0
    for trial in range(40):
        C_ = int(rs.randint(2, 13))
        counts = rs.randint(2, 400, C_)
        ts = float(rs.choice([0.3, 0.25, 0.1, 0.5]))
        n = int(counts.sum())
        n_test = int(np.ceil(ts * n))
        if min(n_test, n - n_test) < C_:
            continue
        drawn, cut1 = preprocess._approximate_mode(counts, n - n_test, 0)
        _, cut2 = preprocess._approximate_mode(counts - drawn, n_test, 0)
        if cut1 or cut2:
            continue
        y = np.repeat(np.arange(C_), counts)
        tr, te = preprocess.stratified_counts(counts, ts)
        for state in (0, 1, 2):
            y_tr, y_te = train_test_split(y, test_size=ts, stratify=y, random_state=state)
            assert np.array_equal(np.bincount(y_te, minlength=C_), te), (counts, ts, state)
            assert np.array_equal(np.bincount(y_tr, minlength=C_), tr), (counts, ts, state)
        done += 1
    assert done >= 10


def test_year_quota_is_pandas_rounding():
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    ns, want = (5, 10, 15, 25, 35, 1001), (2, 3, 4, 8, 10, 300)
    assert [preprocess.year_quota(n) for n in ns] == list(want)
    assert preprocess.year_quota(0) == 0 and preprocess.year_quota(7, 1.0) == 7 and preprocess.year_quota(7, 0.0) == 0
    pd = pytest.importorskip("pandas")
    for n, w in zip(ns, want):
        assert len(pd.DataFrame({"a": np.arange(n)}).sample(frac=0.3, replace=False, random_state=0)) == w


def test_oracle_keys_are_distinct_and_inclusion_is_uniform():
    k = orc.keys(12345, 2 ** 20)
    assert k.dtype == np.uint64 and len(np.unique(k)) == 2 ** 20
    assert len(np.unique(np.concatenate([orc.keys(0, 4096), orc.keys(1, 4096)]))) == 8192
    T, quota, seeds = 2000, 600, range(1000, 1256)
    hits = np.zeros(T, dtype=np.int64)
    for seed in seeds:
        mask, tau = orc.select(None, [quota], seed, n_rows=T)
        assert int(mask.sum()) == quota and int((orc.keys(seed, T) <= tau[0]).sum()) == quota
        hits += mask
    mean, sd = 256 * 0.3, np.sqrt(256 * 0.3 * 0.7)
    assert abs(mean - 76.8) < 1e-9 and abs(sd - 7.33) < 0.01
    worst = float(np.abs(hits - mean).max() / sd)
    print(f"largest deviation of a row's inclusion count: {worst:.2f} standard deviations")
    assert worst <= 6.0                                                    # the oracle alone measured 3.5


def test_oracle_selects_exact_quotas_per_group():
    rs = np.random.RandomState(3)
    group = rs.randint(0, 7, 5000)
    sizes = np.bincount(group, minlength=9)                                # groups 7 and 8 are empty
    quota = np.array([0, 1, sizes[2] - 1, sizes[3], 17, sizes[5] // 2, 3, 0, 0])
    mask, tau = orc.select(group, quota, 99)
    assert np.array_equal(np.bincount(group, weights=mask, minlength=9).astype(np.int64), quota)
    assert tau[0] == 0 and tau[7] == 0 and np.all(tau[quota > 0] > 0)
    again, _ = orc.select(group, quota, 99)
    other, _ = orc.select(group, quota, 100)
    assert np.array_equal(mask, again) and not np.array_equal(mask, other)
