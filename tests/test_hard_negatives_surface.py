"""Host-side surface of the hard-negative draw: the C ABI symbol, argument errors before any launch, `engine.negatives`, and the
public functions of `sampling` on CPU tensors (the draw stubbed where no device is present)."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_sample_hard():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib, engine
    text = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert re.search(r"^#define\s+NGCF_SAMPLE_HARD_M_MAX\s+64\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+NGCF_ABI_VERSION\s+11\s*$", text, flags=re.M)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ngcf_sample_hard_f32\s*\(", text)
    lib = _lib.load()
    assert hasattr(lib, "ngcf_sample_hard_f32") and "ngcf_sample_hard_f32" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["ngcf_sample_hard_f32"][1]) == 22
    assert any(p.endswith("sample_hard.hip") for p in _build.SOURCES)
    for header in ("sample_device.h", "cand_device.h"):                           # a change to a shared header rebuilds the library
        assert any(p.endswith(header) for p in _build.HEADERS)
    blob = open(_lib.lib_path(), "rb").read()
    assert b"sample_hard_kernel" in blob                                          # a gfx950 kernel of its own
    assert int(lib.ngcf_version()) == _lib.ABI_VERSION == 11
    assert engine.negatives.HARD_M_MAX == 64
    assert not hasattr(engine, "hard_unseen") and not hasattr(engine, "HARD_M_MAX")   # the flat namespace is pinned


def test_shared_device_functions_are_defined_once():
    csrc = os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc")
    read = lambda f: open(os.path.join(csrc, f)).read()  # noqa: E731
    for name, header, users in (("sample_x", "sample_device.h", ("sample.hip",)), ("sample_chunk", "sample_device.h", ("sample.hip", "sample_hard.hip")),
                                ("seen_upto", "sample_device.h", ("sample.hip",)), ("cand_quad", "cand_device.h", ("eval_candidates.hip", "sample_hard.hip")),
                                ("group16_sum", "cand_device.h", ("eval_candidates.hip", "sample_hard.hip")),
                                ("cand_fma4", "cand_device.h", ("eval_candidates.hip", "sample_hard.hip"))):
        define = re.compile(r"__device__ inline \w+ " + name + r"\(")
        assert len(define.findall(read(header))) == 1
        for f in users:
            assert not define.search(read(f)) and re.search(r"\b" + name + r"\b", read(f)), (name, f)
    assert '#include "sample_device.h"' in read("sample.hip") and '#include "cand_device.h"' in read("eval_candidates.hip")


def test_c_abi_limits_are_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    one = torch.zeros(4, dtype=torch.int64)          # host memory: a call that got as far as a launch would not return ERR_ARG
    p = one.data_ptr()

    def call(m=8, n_items=100, T=3, D=16, ldu=None, ldi=None, n_rows=5, n_user_rows=5, n_item_rows=100, rowptr=p, colidx=p, users=p,
             items=p, user_ids=p, neg=p, score=None, slot=None, status=p):
        return lib.ngcf_sample_hard_f32(rowptr, colidx, 0, n_rows, n_items, users, D if ldu is None else ldu, n_user_rows, items,
                                        D if ldi is None else ldi, n_item_rows, D, user_ids, T, 0, m, 2024, neg, score, slot, status, None)
    assert call(T=0) == _lib.OK                                                   # no cases: nothing to do
    assert call(T=0, rowptr=None, colidx=None, users=None, items=None, user_ids=None, neg=None, status=None) == _lib.OK
    cases = ((dict(m=0), "m=0 outside [1, 64]"), (dict(m=65), "m=65 outside [1, 64]"), (dict(m=-1), "outside [1, 64]"),
             (dict(n_items=0, n_item_rows=0), "n_items=0 outside [1, 2^31)"), (dict(n_items=2 ** 31, n_item_rows=2 ** 31), "outside [1, 2^31)"),
             (dict(n_item_rows=99), "99 item rows for n_items=100"), (dict(n_user_rows=4), "4 user rows for n_rows=5"),
             (dict(n_rows=-1), "user rows"), (dict(D=0), "D=0 below 1"), (dict(ldu=15), "bad argument"), (dict(ldi=15), "bad argument"),
             (dict(T=-1), "bad argument"), (dict(rowptr=None), "null argument"), (dict(colidx=None), "null argument"),
             (dict(users=None), "null argument"), (dict(items=None), "null argument"), (dict(user_ids=None), "null argument"),
             (dict(neg=None), "null argument"), (dict(status=None), "null argument"))
    for kw, msg in cases:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    # the largest that pass the limits (score and slot may be null; they stop at the null `neg`)
    assert call(m=64, n_items=2 ** 31 - 1, n_item_rows=2 ** 31 - 1, D=1, neg=None) == _lib.ERR_ARG and "null argument" in _lib.last_error()
    with pytest.raises(RuntimeError, match="outside"):
        _lib.check(call(m=65))


def _cpu_sets(n_rows=5, n_items=100):
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.ItemSets(torch.zeros(n_rows + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 0, n_items)


def test_hard_unseen_argument_checks():
    from seoul_tourism_recommendation_ngcf_amd import engine
    hard_unseen = engine.negatives.hard_unseen
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)  # noqa: E731
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)  # noqa: E731
    sets = _cpu_sets()
    U, I = f32(5, 16), f32(100, 16)
    with pytest.raises(RuntimeError, match="ROCm device"):                        # CPU tensors: no fallback, and no launch
        hard_unseen(sets, U, I, i64(3), 8, 1)
    for args, kw, exc, msg in (((U, I, i64(3), 0, 1), {}, ValueError, "m=0 outside"), ((U, I, i64(3), 65, 1), {}, ValueError, "m=65 outside"),
                               ((U, I, i64(3).int(), 8, 1), {}, TypeError, "user_ids must be int64"),
                               ((U.double(), I, i64(3), 8, 1), {}, TypeError, "user_emb must be float32"),
                               ((U, I.half(), i64(3), 8, 1), {}, TypeError, "item_emb must be float32"),
                               ((U, I, i64(3, 1), 8, 1), {}, ValueError, r"user_ids must be \[T\]"),
                               ((U, I, i64(3), 8, 1), dict(out=i64(4)), ValueError, r"out must be a contiguous \[T = 3\]"),
                               ((U, I, i64(3), 8, 1), dict(out=i64(3, 1)), ValueError, "out must be"),
                               ((U, I, i64(3), 8, 1), dict(out=i64(6)[::2]), ValueError, "out must be"),
                               ((U, I, i64(3), 8, 1), dict(out=i64(3).int()), TypeError, "out must be int64"),
                               ((U, f32(99, 16), i64(3), 8, 1), {}, ValueError, "item_emb has 99 rows"),
                               ((f32(4, 16), I, i64(3), 8, 1), {}, ValueError, "user_emb has 4 rows"),
                               ((U, f32(100, 17), i64(3), 8, 1), {}, RuntimeError, "cannot be multiplied"),
                               ((U[0], I, i64(3), 8, 1), {}, RuntimeError, "cannot be multiplied")):
        with pytest.raises(exc, match=msg):
            hard_unseen(sets, *args, **kw)
    with pytest.raises(ValueError, match="n_items"):
        hard_unseen(_cpu_sets(n_items=2 ** 31), U, I, i64(3), 8, 1)
    sig = inspect.signature(hard_unseen)
    assert list(sig.parameters) == ["seen", "user_emb", "item_emb", "user_ids", "m", "seed", "case_offset", "return_score", "return_slot",
                                    "out", "status"]
    keyword_only = ("case_offset", "return_score", "return_slot", "out", "status")
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in keyword_only)
    assert [sig.parameters[k].default for k in keyword_only] == [0, False, False, None, None]


def test_sampling_exports_hard_triplets_and_loader():
    from seoul_tourism_recommendation_ngcf_amd import sampling
    sig = inspect.signature(sampling.hard_triplets)
    assert list(sig.parameters) == ["users", "items", "user_emb", "item_emb", "seen", "m", "seed", "epoch", "n_user", "n_item", "chunk"]
    assert sig.parameters["m"].default == 8 and sig.parameters["epoch"].default == 0 and sig.parameters["chunk"].default is None
    assert sig.parameters["seen"].default is None and sig.parameters["seen"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("m", "seed", "epoch", "n_user", "n_item", "chunk"))
    sig = inspect.signature(sampling.HardTripletLoader.__init__)
    assert list(sig.parameters) == ["self", "users", "items", "columns", "batch_size", "tables", "m", "seed", "shuffle", "drop_last", "generator"]
    assert sig.parameters["columns"].default == () and sig.parameters["m"].default == 8
    assert sig.parameters["shuffle"].default is True and sig.parameters["drop_last"].default is True
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
               for k in ("batch_size", "tables", "m", "seed", "shuffle", "drop_last", "generator"))
    rows = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device"):                        # no CPU fallback
        sampling.hard_triplets(rows, rows, torch.zeros(4, 8), torch.zeros(100, 8), seed=1, n_user=4, n_item=100)
    assert "all_users_emb" in sampling.hard_triplets.__doc__ and "fresh" in sampling.hard_triplets.__doc__


def _stub_draw(monkeypatch, calls):
    """In place of the device's draw: negative = 2000 + row + 10000 * (position of the call), and a record of what the loader asked for."""
    from seoul_tourism_recommendation_ngcf_amd import sampling

    def draw(users, user_emb, item_emb, seen, m, seed_e, chunk=None, out=None):
        calls.append((user_emb, item_emb, m, seed_e, seen))
        out.copy_(torch.arange(users.numel()) + 2000 + 10000 * (len(calls) - 1))
        return out
    monkeypatch.setattr(sampling, "_hard_draw", draw)


def test_hard_triplet_loader_bookkeeping(monkeypatch):
    from seoul_tourism_recommendation_ngcf_amd import sampling
    calls, served = [], []
    _stub_draw(monkeypatch, calls)
    U, I = torch.zeros(103, 4), torch.zeros(1200, 4)

    def tables():
        served.append(1)
        return U, I
    rows = torch.arange(103)
    loader = sampling.HardTripletLoader(rows, rows + 1000, batch_size=10, tables=tables, m=4, seed=7,
                                        generator=torch.Generator().manual_seed(3))
    assert len(loader) == 10 and loader.epoch == 0 and not served and not calls   # nothing is drawn before the first iter()
    orders = []
    for e in range(3):
        it = iter(loader)
        assert loader.epoch == e + 1 and len(served) == e + 1 and len(calls) == e + 1     # one tables() and one draw per iter()
        assert calls[e][0] is U and calls[e][1] is I and calls[e][2] == 4 and calls[e][3] == sampling.fmix(7 + e)
        batches = list(it)
        assert len(batches) == 10 and all(len(b) == 3 and all(c.shape == (10,) and c.dtype == torch.int64 for c in b) for b in batches)
        u = torch.cat([b[0] for b in batches])
        assert torch.equal(torch.cat([b[1] for b in batches]), u + 1000)
        assert torch.equal(torch.cat([b[2] for b in batches]), u + 2000 + 10000 * e)      # this epoch's negatives, row by row
        assert u.unique().numel() == 100                                                  # every row at most once, the tail of 3 dropped
        orders.append(u)
    assert not torch.equal(orders[0], orders[1])                                  # a new permutation per epoch
    assert calls[0][4] is calls[1][4] and calls[0][4].n_rows == 103 and calls[0][4].n_items == 1200   # the seen sets: built once
    assert torch.equal(calls[0][4].rowptr, torch.arange(104)) and torch.equal(calls[0][4].colidx, (rows + 1000).int())


def test_hard_triplet_loader_columns_and_options(monkeypatch):
    from seoul_tourism_recommendation_ngcf_amd import sampling
    calls = []
    _stub_draw(monkeypatch, calls)
    tables = lambda: (torch.zeros(25, 4), torch.zeros(1100, 4))  # noqa: E731
    n = 25
    rows = torch.arange(n)
    cols = tuple(rows * 10 + q for q in range(7))                                 # year, u_id, age, sex, month, day, dow
    loader = sampling.HardTripletLoader(rows, rows + 1000, cols, batch_size=8, tables=tables, seed=1, generator=torch.Generator().manual_seed(1))
    assert len(loader) == 3 and loader.m == 8
    for year, u_id, age, sex, month, day, dow, pos, neg in loader:
        r = year // 10
        for q, c in enumerate((year, u_id, age, sex, month, day, dow)):
            assert torch.equal(c, r * 10 + q)
        assert torch.equal(pos, r + 1000) and torch.equal(neg, r + 2000)
    ordered = sampling.HardTripletLoader(rows, rows + 1000, batch_size=8, tables=tables, seed=1, shuffle=False, drop_last=False)
    assert len(ordered) == 4
    got = list(ordered)
    assert [int(b[0].numel()) for b in got] == [8, 8, 8, 1] and torch.equal(torch.cat([b[0] for b in got]), rows)
    assert torch.equal(torch.cat([b[2] for b in got]), rows + 2000 + 10000) and ordered.epoch == 1
    with pytest.raises(ValueError, match="every column"):
        sampling.HardTripletLoader(rows, rows[:-1], batch_size=8, tables=tables, seed=1)
    with pytest.raises(ValueError, match="batch_size"):
        sampling.HardTripletLoader(rows, rows, batch_size=0, tables=tables, seed=1)
    for m in (0, 65):
        with pytest.raises(ValueError, match="outside"):
            sampling.HardTripletLoader(rows, rows, batch_size=8, tables=tables, seed=1, m=m)
    with pytest.raises(TypeError, match="callable"):
        sampling.HardTripletLoader(rows, rows, batch_size=8, tables=(None, None), seed=1)
    with pytest.raises(TypeError):
        sampling.HardTripletLoader(rows, rows, batch_size=8, seed=1)              # tables is required
