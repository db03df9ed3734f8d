"""Host-side surface of the unseen-item draw: the C ABI symbol, argument errors before any launch, the public module, and the
device-side loader on CPU tensors."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_sample_unseen():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib, engine
    text = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ngcf_sample_unseen\s*\(", text)
    lib = _lib.load()
    assert hasattr(lib, "ngcf_sample_unseen") and "ngcf_sample_unseen" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["ngcf_sample_unseen"][1]) == 15
    assert any(p.endswith("sample.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    assert b"sample_unseen_one_kernel" in blob and b"sample_unseen_wave_kernel" in blob     # gfx950 kernels of its own
    assert int(lib.ngcf_version()) == _lib.ABI_VERSION == 11
    assert engine.SAMPLE_M_MAX == 1023 == engine.CAND_MAX - 1


def test_c_abi_limits_are_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    one = torch.zeros(4, dtype=torch.int64)          # host memory: a call that got as far as a launch would not return ERR_ARG
    p = one.data_ptr()

    def call(m=24, n_items=100, T=3, ld=None, first=None, rowptr=p, colidx=p, user_ids=p, out=p, status=p, n_rows=5):
        ld = m + (first is not None) if ld is None else ld
        return lib.ngcf_sample_unseen(rowptr, colidx, 0, n_rows, n_items, user_ids, T, 0, m, 2024, first, out, ld, status, None)
    assert call(T=0) == _lib.OK                                                   # no cases: nothing to do
    assert call(T=0, rowptr=None, colidx=None, user_ids=None, out=None, status=None) == _lib.OK
    cases = ((dict(m=0), "m=0 outside [1, 1023]"), (dict(m=1024), "m=1024 outside [1, 1023]"), (dict(m=-1), "outside [1, 1023]"),
             (dict(n_items=0), "n_items=0 outside [1, 2^31)"), (dict(n_items=2 ** 31), "outside [1, 2^31)"),
             (dict(ld=23), "ld_out=23 is below the 24 columns"), (dict(ld=24, first=p), "ld_out=24 is below the 25 columns"),
             (dict(m=1, ld=0), "ld_out=0"), (dict(T=-1), "bad argument"), (dict(n_rows=-1), "bad argument"),
             (dict(rowptr=None), "null argument"), (dict(colidx=None), "null argument"), (dict(user_ids=None), "null argument"),
             (dict(out=None), "null argument"), (dict(status=None), "null argument"))
    for kw, msg in cases:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert call(m=1023, n_items=2 ** 31 - 1, out=None) == _lib.ERR_ARG and "null argument" in _lib.last_error()   # the largest that pass
    with pytest.raises(RuntimeError, match="outside"):
        _lib.check(call(m=1024))


def test_sample_unseen_argument_checks():
    from seoul_tourism_recommendation_ngcf_amd import engine
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)  # noqa: E731
    sets = engine.ItemSets(i64(6), torch.zeros(0, dtype=torch.int32), 0, 100)
    with pytest.raises(RuntimeError, match="ROCm device"):                        # CPU tensors: no fallback, and no launch
        engine.sample_unseen(sets, i64(3), 24, 1)
    for args, kw, exc, msg in (((i64(3), 0, 1), {}, ValueError, "m=0"), ((i64(3), 1024, 1), {}, ValueError, "m=1024"),
                               ((i64(3).int(), 24, 1), {}, TypeError, "user_ids must be int64"),
                               ((i64(3, 1), 24, 1), {}, ValueError, r"user_ids must be \[T\]"),
                               ((i64(3), 24, 1), dict(first=i64(4)), ValueError, r"first must be \[T = 3\]"),
                               ((i64(3), 24, 1), dict(first=i64(3).int()), TypeError, "first must be int64"),
                               ((i64(3), 24, 1), dict(out=i64(3, 23)), ValueError, r"out must be \[T = 3, >= 24\]"),
                               ((i64(3), 24, 1), dict(out=i64(3, 24), first=i64(3)), ValueError, r"out must be \[T = 3, >= 25\]"),
                               ((i64(3), 24, 1), dict(out=i64(2, 24)), ValueError, "out must be"),
                               ((i64(3), 24, 1), dict(out=i64(3, 24).int()), TypeError, "out must be int64")):
        with pytest.raises(exc, match=msg):
            engine.sample_unseen(sets, *args, **kw)
    with pytest.raises(ValueError, match="n_items"):
        engine.sample_unseen(engine.ItemSets(i64(6), torch.zeros(0, dtype=torch.int32), 0, 2 ** 31), i64(3), 24, 1)
    sig = inspect.signature(engine.sample_unseen)
    assert list(sig.parameters) == ["seen", "user_ids", "m", "seed", "first", "case_offset", "out", "status"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("first", "case_offset", "out", "status"))


def test_sampling_is_exported():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    assert "sampling" in pkg.__all__ and pkg.sampling.train_triplets and pkg.sampling.test_candidates and pkg.sampling.TripletLoader
    sig = inspect.signature(pkg.sampling.train_triplets)
    assert list(sig.parameters) == ["users", "items", "seen", "seed", "epoch", "n_user", "n_item"]
    assert sig.parameters["epoch"].default == 0 and sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(pkg.sampling.test_candidates)
    assert list(sig.parameters) == ["users", "items", "seen", "m", "seed", "n_user", "n_item"] and sig.parameters["m"].default == 24
    for fn in (pkg.sampling.train_triplets, pkg.sampling.test_candidates):       # no CPU fallback
        with pytest.raises(RuntimeError, match="ROCm device"):
            fn(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), seed=1, n_user=4, n_item=100)
    import sample_oracle
    for x in (0, 1, 2024, 2 ** 64 - 1, 0x9E3779B97F4A7C15):
        assert pkg.sampling.fmix(x) == sample_oracle.fmix(x)
    assert pkg.sampling.fmix(1) == 0xb456bcfc34c2cb2c                             # MurmurHash3's fmix64


def _loader(n=103, batch=10, seed=7, **kw):
    from seoul_tourism_recommendation_ngcf_amd import sampling
    rows = torch.arange(n)
    g = torch.Generator().manual_seed(seed)
    return sampling.TripletLoader(rows, rows + 1000, rows + 2000, batch_size=batch, generator=g, **kw)


def test_triplet_loader_epochs_on_cpu_tensors():
    loader = _loader()
    assert len(loader) == 10
    epochs = []
    for _ in range(2):
        batches = list(loader)
        assert len(batches) == 10 and all(len(b) == 3 and all(c.shape == (10,) for c in b) for b in batches)
        u = torch.cat([b[0] for b in batches])
        assert torch.equal(torch.cat([b[1] for b in batches]), u + 1000) and torch.equal(torch.cat([b[2] for b in batches]), u + 2000)
        assert u.unique().numel() == 100 and int(u.min()) >= 0 and int(u.max()) < 103     # every row at most once, the tail of 3 dropped
        epochs.append(u)
    assert not torch.equal(epochs[0], epochs[1])                                  # a new permutation per epoch
    again = torch.cat([b[0] for b in _loader()])
    assert torch.equal(again, epochs[0])                                          # the same generator seed, the same order
    whole = _loader(n=100)
    assert torch.equal(torch.cat([b[0] for b in whole]).sort().values, torch.arange(100))   # no tail: every row exactly once
    base = whole.table.clone()
    b0 = next(iter(whole))
    assert b0[0].data_ptr() != whole.table.data_ptr() and torch.equal(whole.table, base)  # batches are views of the epoch's copy
    assert b0[1].data_ptr() - b0[0].data_ptr() == 100 * 8


def test_triplet_loader_columns_and_options():
    from seoul_tourism_recommendation_ngcf_amd import sampling
    n = 25
    rows = torch.arange(n)
    cols = tuple(rows * 10 + q for q in range(7))                                 # year, u_id, age, sex, month, day, dow
    loader = sampling.TripletLoader(rows, rows + 1000, rows + 2000, cols, batch_size=8, generator=torch.Generator().manual_seed(1))
    assert len(loader) == 3
    for year, u_id, age, sex, month, day, dow, pos, neg in loader:
        r = year // 10
        for q, c in enumerate((year, u_id, age, sex, month, day, dow)):
            assert torch.equal(c, r * 10 + q)
        assert torch.equal(pos, r + 1000) and torch.equal(neg, r + 2000) and pos.dtype == torch.int64
    ordered = sampling.TripletLoader(rows, rows + 1000, rows + 2000, batch_size=8, shuffle=False, drop_last=False)
    assert len(ordered) == 4
    got = list(ordered)
    assert [int(b[0].numel()) for b in got] == [8, 8, 8, 1] and torch.equal(torch.cat([b[0] for b in got]), rows)
    with pytest.raises(ValueError, match="every column"):
        sampling.TripletLoader(rows, rows[:-1], rows, batch_size=8)
    with pytest.raises(ValueError, match="batch_size"):
        sampling.TripletLoader(rows, rows, rows, batch_size=0)
    with pytest.raises(TypeError):
        sampling.TripletLoader(rows, rows, rows)                                  # batch_size is required
