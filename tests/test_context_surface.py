"""Host side of the trip-context family: the C ABI symbols and their gfx950 kernels, refusals before any launch and before a device is
needed, and the parts of `recommend` that are plain torch, on CPU tensors against tests/context_oracle.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import context_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ngcf_segment_kahan_sum_f64": ("int", 10), "ngcf_haversine_table_f64": ("int", 6)}
KERNELS = (b"segment_kahan_lane_kernel", b"segment_kahan_wave_kernel", b"haversine_table_kernel")


def test_header_declares_and_library_exports_the_family():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    raw = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name, (ret, n_args) in SYMBOLS.items():
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert any(p.endswith("context.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    for k in KERNELS:
        assert k in blob, k
    assert "y = v - c" in raw and "c = (t - s) - y" in raw and "asin(sqrt(d))" in raw          # the recurrence and the formula are written out
    assert int(re.search(r"#define\s+NGCF_ABI_VERSION\s+(\d+)", raw).group(1)) == int(lib.ngcf_version()) == _lib.ABI_VERSION


def test_c_abi_argument_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float64)          # host memory: a call that got as far as a launch would not return ERR_ARG
    p = buf.data_ptr()
    one, none = (C.c_void_p * 1)(p), (C.c_void_p * 1)(None)

    def kahan(rowptr=p, n_rows=3, order=None, values=one, V=1, T=8, wave_min=0, sums=one, status=p):
        return lib.ngcf_segment_kahan_sum_f64(rowptr, n_rows, order, values, V, T, wave_min, sums, status, None)

    def hav(dep=p, S=2, item=p, n_item=3, out=p):
        return lib.ngcf_haversine_table_f64(dep, S, item, n_item, out, None)

    cases = [(kahan, dict(V=0), "0 value columns"), (kahan, dict(V=5), "5 value columns"), (kahan, dict(wave_min=-1), "wave_min=-1"),
             (kahan, dict(T=-1), "negative count"), (kahan, dict(n_rows=-1), "negative count"), (kahan, dict(rowptr=None), "null argument"),
             (kahan, dict(values=None), "null argument"), (kahan, dict(sums=None), "null argument"), (kahan, dict(status=None), "null argument"),
             (kahan, dict(values=none), "null argument"), (kahan, dict(sums=none), "null argument"),
             (hav, dict(S=-1), "negative count"), (hav, dict(n_item=-2), "negative count"), (hav, dict(dep=None), "null argument"),
             (hav, dict(item=None), "null argument"), (hav, dict(out=None), "null argument")]
    for fn, kw, msg in cases:
        assert fn(**kw) == _lib.ERR_ARG, (fn.__name__, kw)
        err = _lib.last_error()
        assert err.startswith({"kahan": "segment_kahan_sum: ", "hav": "haversine_table: "}[fn.__name__]) and msg in err, (kw, err)
    assert kahan(n_rows=0, rowptr=None, sums=None) == _lib.OK and hav(S=0, dep=None, out=None) == _lib.OK
    assert hav(n_item=0, item=None, out=None) == _lib.OK                                   # nothing to do is not an error


def test_python_surface_signatures_and_refusals_before_a_device_is_needed():
    from seoul_tourism_recommendation_ngcf_amd import engine, recommend
    ctx = engine.context
    sig = inspect.signature(ctx.segment_kahan_sum)
    assert list(sig.parameters) == ["rowptr", "values", "order", "wave_min"]
    assert sig.parameters["order"].default is None and sig.parameters["wave_min"].default == 0
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("order", "wave_min"))
    assert list(inspect.signature(ctx.group_sum_float).parameters) == ["columns", "values", "bounds", "wave_min"]
    assert list(inspect.signature(ctx.haversine_table).parameters) == ["dep", "item", "out"]
    assert list(inspect.signature(recommend.congestion_table).parameters)[:7] == ["month", "day", "dayofweek", "item", "values", "n_item", "by"]
    assert list(inspect.signature(recommend.party_rows).parameters) == ["party", "age", "sex", "start_month", "start_day", "start_dow",
                                                                        "duration", "user_codes"]
    assert recommend.PartyRows._fields == ("party", "member", "user_ids", "age", "sex", "month", "day", "dow")

    i64, f64 = torch.arange(6, dtype=torch.int64), torch.arange(6, dtype=torch.float64)
    rowptr = torch.tensor([0, 2, 6])
    for call in (lambda: ctx.segment_kahan_sum(rowptr, f64), lambda: ctx.segment_kahan_sum(rowptr, (f64, f64), order=i64, wave_min=1),
                 lambda: ctx.group_sum_float([i64], f64), lambda: ctx.haversine_table(f64.view(3, 2), f64.view(3, 2)),
                 lambda: recommend.congestion_table(i64, i64, i64, i64, (f64, f64), n_item=6, by=1),
                 lambda: recommend.distance_table(f64.view(3, 2), f64.view(3, 2))):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()
    for dt in (torch.float32, torch.int64, torch.bfloat16):
        with pytest.raises(TypeError, match="value column 0 must be float64"):
            ctx.segment_kahan_sum(rowptr, f64.to(dt))
        with pytest.raises(TypeError, match="value column 1 must be float64"):
            ctx.group_sum_float([i64], (f64, f64.to(dt)))
    with pytest.raises(TypeError, match="rowptr must be int64"):
        ctx.segment_kahan_sum(rowptr.int(), f64)
    with pytest.raises(TypeError, match="order must be int64"):
        ctx.segment_kahan_sum(rowptr, f64, order=i64.int())
    with pytest.raises(TypeError, match="key column 0 must be int32 or int64"):
        ctx.group_sum_float([f64], f64)
    with pytest.raises(ValueError, match="0 value columns"):
        ctx.segment_kahan_sum(rowptr, ())
    with pytest.raises(ValueError, match="5 value columns"):
        ctx.group_sum_float([i64], [f64] * 5)
    with pytest.raises(ValueError, match="must be \\[T\\]"):
        ctx.segment_kahan_sum(rowptr, f64.view(2, 3))
    with pytest.raises(ValueError, match="has 5 rows"):
        ctx.segment_kahan_sum(rowptr, (f64, f64[:5]))
    with pytest.raises(ValueError, match="key column 0 has 5"):
        ctx.group_sum_float([i64[:5]], f64)
    with pytest.raises(ValueError, match="order must be \\[T = 6\\]"):
        ctx.segment_kahan_sum(rowptr, f64, order=i64[:4])
    with pytest.raises(ValueError, match="rowptr must be"):
        ctx.segment_kahan_sum(rowptr.view(1, 3), f64)
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="wave_min="):
            ctx.segment_kahan_sum(rowptr, f64, wave_min=bad)
    with pytest.raises(TypeError, match="dep must be float64"):
        ctx.haversine_table(f64.view(3, 2).float(), f64.view(3, 2))
    with pytest.raises(ValueError, match="item must be \\[n, 2\\]"):
        ctx.haversine_table(f64.view(3, 2), f64.view(2, 3))
    with pytest.raises(ValueError, match="out must be"):
        ctx.haversine_table(f64.view(3, 2), f64.view(3, 2), out=torch.empty((3, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="by=2"):
        recommend.congestion_table(i64, i64, i64, i64, (f64, f64), n_item=6, by=2)
    # group_by keeps refusing floats, and now says where they are summed
    with pytest.raises(TypeError, match="compensated.*group_sum_float.*arrival order"):
        engine.group_by([i64], [f64])


def test_party_rows_on_cpu_tensors_equal_the_reference_loop():
    from seoul_tourism_recommendation_ngcf_amd import recommend
    parties = [dict(ages=[27, 61], sexes=[0, 1], month=2, day=29, dow=5, duration=3),          # Feb 29 -> Feb 28, into March
               dict(ages=[33], sexes=[1], month=7, day=30, dow=2, duration=4),                  # across a 31-day month end
               dict(ages=[9, 80, 45], sexes=[1, 0, 0], month=4, day=31, dow=6, duration=2),     # a start past the month's fixed length
               dict(ages=[50], sexes=[0], month=12, day=30, dow=0, duration=2)]
    want = [r + [p, m] for p, q in enumerate(parties) for m, r in
            enumerate(orc.party_loop(q["ages"], q["sexes"], q["month"], q["day"], q["dow"], q["duration"]))]
    party = torch.tensor([p for p, q in enumerate(parties) for _ in q["ages"]])
    age = torch.tensor([a for q in parties for a in q["ages"]])
    sex = torch.tensor([s for q in parties for s in q["sexes"]])
    start = {k: torch.tensor([q[n] for q in parties]) for k, n in (("start_month", "month"), ("start_day", "day"), ("start_dow", "dow"),
                                                                 ("duration", "duration"))}
    got = recommend.party_rows(party, age, sex, user_codes=None, **start)
    assert got.user_ids is None and got.features == (got.age, got.sex, got.month, got.day, got.dow)
    assert [list(r) for r in zip(*(t.tolist() for t in got.features))] == [r[1:6] for r in want]
    assert got.party.tolist() == [r[6] for r in want]
    first = np.cumsum([0] + [len(q["ages"]) for q in parties])
    assert got.member.tolist() == [m for p, q in enumerate(parties) for m in range(first[p], first[p + 1]) for _ in range(q["duration"])]
    # one value for all parties
    same = recommend.party_rows(torch.tensor([0, 1]), torch.tensor([20, 31]), torch.tensor([0, 1]), start_month=7, start_day=31, start_dow=3,
                                duration=2, user_codes=None)
    assert same.month.tolist() == [7, 8, 7, 8] and same.day.tolist() == [31, 1, 31, 1] and same.dow.tolist() == [3, 4, 3, 4]
    assert same.age.tolist() == [25, 25, 35, 35]
    with pytest.raises(IndexError, match="request row 2 .* past December"):
        recommend.party_rows(torch.tensor([0]), torch.tensor([30]), torch.tensor([0]), start_month=12, start_day=30, start_dow=0, duration=3,
                             user_codes=None)
    with pytest.raises(RuntimeError, match="ROCm device"):                                      # the lookup is the device's
        recommend.party_rows(torch.tensor([0]), torch.tensor([30]), torch.tensor([0]), start_month=1, start_day=1, start_dow=0, duration=1,
                             user_codes=torch.arange(4))
    with pytest.raises(TypeError, match="age must be"):
        recommend.party_rows(torch.tensor([0]), torch.tensor([30.0]), torch.tensor([0]), start_month=1, start_day=1, start_dow=0, duration=1,
                             user_codes=None)
    with pytest.raises(ValueError, match="duration has 3 entries for 1 parties"):
        recommend.party_rows(torch.tensor([0]), torch.tensor([30]), torch.tensor([0]), start_month=1, start_day=1, start_dow=0,
                             duration=[1, 2, 3], user_codes=None)
    empty = recommend.party_rows(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                                 start_month=1, start_day=1, start_dow=0, duration=1, user_codes=None)
    assert all(t.numel() == 0 for t in empty.features)


def test_order_table_and_context_slots_on_cpu_tensors():
    from seoul_tourism_recommendation_ngcf_amd import recommend
    rng = np.random.default_rng(3)
    table = rng.integers(0, 40, (4, 130)).astype(np.float64) * 0.1                              # many ties
    table[rng.random(table.shape) < 0.1] = np.inf
    table[0, 5], table[1, :] = -0.0, np.inf
    got = recommend.order_table(torch.from_numpy(table))
    want = orc.dense_ranks(table)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    # two fp64 distances that fp32 merges stay apart, and the row's order is the fp64 order
    close = torch.tensor([[10000.0 + 2.0 ** -20, 10000.0, float("inf"), 9999.0]], dtype=torch.float64)
    assert close.float()[0, 0] == close.float()[0, 1] and recommend.order_table(close)[0].tolist() == [2.0, 1.0, float("inf"), 0.0]
    assert bool(torch.isnan(recommend.order_table(torch.tensor([[1.0, float("nan")]]))[0, 1]))
    with pytest.raises(ValueError, match="floating"):
        recommend.order_table(torch.zeros((2, 3), dtype=torch.int64))
    days = torch.tensor([[7, 30, 2], [7, 31, 3], [8, 1, 4]])
    slots = recommend.context_slots(days, torch.tensor([8, 7, 7, 8]), torch.tensor([1, 30, 31, 1]), torch.tensor([4, 2, 3, 4]))
    assert slots.dtype == torch.int64 and slots.tolist() == [2, 0, 1, 2]
    with pytest.raises(IndexError, match="request row 1: .*\\(7, 31, 4\\)"):
        recommend.context_slots(days, torch.tensor([8, 7]), torch.tensor([1, 31]), torch.tensor([4, 4]))
    with pytest.raises(IndexError):
        recommend.context_slots(days[:0], torch.tensor([8]), torch.tensor([1]), torch.tensor([4]))
    with pytest.raises(ValueError, match="ascending"):
        recommend.context_slots(days.flip(0), torch.tensor([8]), torch.tensor([1]), torch.tensor([4]))
    assert recommend.context_slots(days, days[:0, 0], days[:0, 1], days[:0, 2]).numel() == 0
