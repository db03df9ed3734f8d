"""Host side of the group-by family: the C ABI symbols and their gfx950 kernels, refusals before any launch, the public functions of
`engine` and `preprocess`, and the numpy oracles of tests/groupby_oracle.py against pandas and against the reference's saved
dictionaries (tests/golden/id_maps.npz)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import groupby_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ngcf_groupby_hash": ("uint64_t", 1), "ngcf_groupby_limits": ("int", 3), "ngcf_groupby_workspace_bytes": ("int64_t", 1),
           "ngcf_groupby_insert": ("int", 8), "ngcf_groupby_count": ("int", 6), "ngcf_groupby_compact": ("int", 9),
           "ngcf_groupby_unpack": ("int", 12), "ngcf_groupby_lookup": ("int", 8), "ngcf_decimal_code": ("int", 8)}
KERNELS = (b"groupby_insert_kernel", b"groupby_count_kernel", b"groupby_scan_tiles_kernel", b"groupby_compact_kernel",
           b"groupby_unpack_kernel", b"groupby_lookup_kernel", b"decimal_code_kernel")


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "id_maps.npz"), allow_pickle=False)


def test_header_declares_and_library_exports_the_family():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib, engine
    raw = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name, (ret, n_args) in SYMBOLS.items():
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert any(p.endswith("groupby.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    for k in KERNELS:
        assert k in blob, k
    m = re.search(r"#define\s+NGCF_ABI_VERSION\s+(\d+)", raw)
    assert int(m.group(1)) == int(lib.ngcf_version()) == _lib.ABI_VERSION == 11
    chunk, probes, max_slots = engine.groupby_limits()
    assert chunk >= 256 and chunk % 256 == 0 and probes >= 1 and max_slots >= 64 and max_slots & (max_slots - 1) == 0
    assert engine.GROUPBY_LDS_SLOTS <= max_slots
    assert lib.ngcf_groupby_workspace_bytes(64) >= 8 and lib.ngcf_groupby_workspace_bytes(48) == -1
    assert lib.ngcf_groupby_workspace_bytes(0) == -1 and lib.ngcf_groupby_workspace_bytes(2 ** 37) == -1
    for key in (0, 1, 12345678901234567, 2 ** 63 - 1):                            # the documented hash is the library's
        assert engine.groupby_hash(key) == orc.fmix64(key)
    # the struct the kernels take by value has the layout the header gives it
    assert C.sizeof(engine._GroupbyCols) == 8 + 8 * 8 + 4 * 8 + 8 * 8 + 8 * 8 + 3 * 8 * 4 + 4 * 4


def _cols(engine, bounds, n_values=0, ptr=0):
    offsets, ranges, bits, shifts = engine.groupby_packing(bounds)
    c = engine._GroupbyCols()
    c.n_keys, c.n_values = len(bounds), n_values
    for k in range(len(bounds)):
        c.key[k], c.key_is64[k] = ptr, 1
        c.key_offset[k], c.key_range[k], c.key_bits[k], c.key_shift[k] = offsets[k], ranges[k], bits[k], shifts[k]
    for v in range(n_values):
        c.value[v], c.value_is64[v] = ptr, 1
    return c


def test_c_abi_argument_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib, engine
    lib = _lib.load()
    buf = torch.zeros(512, dtype=torch.int64)         # host memory: a call that got as far as a launch would not return ERR_ARG
    p = buf.data_ptr()
    good = _cols(engine, [(0, 9), (-3, 3)], n_values=1, ptr=p)

    def insert(cols=good, T=5, keys=p, sums=p, cap=64, lds=0, status=p):
        return lib.ngcf_groupby_insert(C.byref(cols) if cols is not None else None, T, keys, sums, cap, lds, status, None)

    def count(keys=p, cap=64, n=p, ws=p, nb=64):
        return lib.ngcf_groupby_count(keys, cap, n, ws, nb, None)

    def compact(keys=p, cap=64, G=3, out=p, slots=p, ws=p, nb=64, status=p):
        return lib.ngcf_groupby_compact(keys, cap, G, out, slots, ws, nb, status, None)

    outs = (C.c_void_p * 8)(*[p] * 8)

    def unpack(cols=good, sk=p, order=p, slots=p, sums=p, cap=64, G=3, ko=outs, so=outs, rank=None, status=p):
        return lib.ngcf_groupby_unpack(C.byref(cols) if cols is not None else None, sk, order, slots, sums, cap, G, ko, so, rank, status, None)

    def lookup(cols=good, T=5, keys=p, rank=p, cap=64, inv=p, status=p):
        return lib.ngcf_groupby_lookup(C.byref(cols) if cols is not None else None, T, keys, rank, cap, inv, status, None)

    wide = _cols(engine, [(0, 2 ** 40), (0, 2 ** 20)], ptr=p)
    wide.key_bits[0] = 44                                                          # 44 + 21 bits
    wide.key_range[0] = 2 ** 44 - 1
    skew = _cols(engine, [(0, 9), (0, 9)], ptr=p)
    skew.key_shift[0] = 3                                                          # overlaps column 1's four bits
    tight = _cols(engine, [(0, 9)], ptr=p)
    tight.key_range[0] = 16                                                        # does not fit its four bits
    none = _cols(engine, [(0, 9)], ptr=p)
    none.n_keys = 0
    many = _cols(engine, [(0, 9)], ptr=p)
    many.n_values = 5
    nullcol = _cols(engine, [(0, 9)], ptr=0)
    cases = [(insert, dict(cols=None), "null argument"), (insert, dict(T=-1), "negative count"), (insert, dict(keys=None), "null argument"),
             (insert, dict(sums=None), "null argument"), (insert, dict(status=None), "null argument"), (insert, dict(cols=nullcol), "null argument"),
             (insert, dict(cap=48), "not a power of two"), (insert, dict(cap=0), "not a power of two"), (insert, dict(cap=2 ** 37), "not a power of two"),
             (insert, dict(lds=8), "lds_slots=8"), (insert, dict(lds=96), "lds_slots=96"), (insert, dict(lds=4096), "lds_slots=4096"),
             (insert, dict(lds=-64), "lds_slots=-64"), (insert, dict(cols=wide), "above 63"), (insert, dict(cols=skew), "do not fit together"),
             (insert, dict(cols=tight), "do not fit together"), (insert, dict(cols=none), "0 key columns"), (insert, dict(cols=many), "5 value columns"),
             (count, dict(keys=None), "null argument"), (count, dict(n=None), "null argument"), (count, dict(ws=None), "null argument"),
             (count, dict(cap=3), "not a power of two"),
             (compact, dict(keys=None), "null argument"), (compact, dict(out=None), "null argument"), (compact, dict(slots=None), "null argument"),
             (compact, dict(ws=None), "null argument"), (compact, dict(status=None), "null argument"), (compact, dict(G=-1), "n_groups=-1"),
             (compact, dict(G=65), "n_groups=65"), (compact, dict(cap=6), "not a power of two"),
             (unpack, dict(cols=None), "null argument"), (unpack, dict(sk=None), "null argument"), (unpack, dict(order=None), "null argument"),
             (unpack, dict(slots=None), "null argument"), (unpack, dict(sums=None), "null argument"), (unpack, dict(ko=None), "null argument"),
             (unpack, dict(so=None), "null argument"), (unpack, dict(status=None), "null argument"), (unpack, dict(G=65), "n_groups=65"),
             (unpack, dict(ko=(C.c_void_p * 8)()), "null argument"), (unpack, dict(cols=wide), "above 63"),
             (lookup, dict(cols=None), "null argument"), (lookup, dict(T=-2), "negative count"), (lookup, dict(keys=None), "null argument"),
             (lookup, dict(rank=None), "null argument"), (lookup, dict(inv=None), "null argument"), (lookup, dict(status=None), "null argument"),
             (lookup, dict(cols=nullcol), "null argument"), (lookup, dict(cap=100), "not a power of two")]
    for fn, kw, msg in cases:
        assert fn(**kw) == _lib.ERR_ARG, (fn.__name__, kw)
        err = _lib.last_error()
        assert err.startswith("groupby: " + fn.__name__) and msg in err, (fn.__name__, kw, err)
    for fn in (count, compact):
        assert fn(nb=0) == _lib.ERR_WORKSPACE and "groupby:" in _lib.last_error()
    assert compact(G=0, out=None, slots=None) == _lib.OK and unpack(G=0, sk=None, order=None, slots=None) == _lib.OK
    assert lookup(T=0, inv=None, cols=nullcol) == _lib.OK                           # nothing to do is not an error

    ptrs, flags, widths = (C.c_void_p * 2)(p, p), (C.c_int32 * 2)(1, 1), (C.c_int32 * 2)(0, 2)

    def dec(cols=ptrs, is64=flags, w=widths, n=2, T=5, out=p, status=p):
        return lib.ngcf_decimal_code(cols, is64, w, n, T, out, status, None)

    dcases = [(dict(T=-1), "negative count"), (dict(n=0), "0 columns"), (dict(n=9), "9 columns"), (dict(cols=None), "null argument"),
              (dict(is64=None), "null argument"), (dict(w=None), "null argument"), (dict(out=None), "null argument"), (dict(status=None), "null argument"),
              (dict(cols=(C.c_void_p * 2)(p, None)), "null argument"), (dict(w=(C.c_int32 * 2)(0, -1)), "width -1"),
              (dict(w=(C.c_int32 * 2)(0, 19)), "width 19"), (dict(w=(C.c_int32 * 2)(9, 10)), "at least 19 characters")]
    for kw, msg in dcases:
        assert dec(**kw) == _lib.ERR_ARG, kw
        assert _lib.last_error().startswith("decimal_code: ") and msg in _lib.last_error(), (kw, _lib.last_error())
    assert dec(T=0, out=None) == _lib.OK


def test_python_surface_signatures_and_refusals():
    from seoul_tourism_recommendation_ngcf_amd import engine, preprocess
    sig = inspect.signature(engine.group_by)
    assert list(sig.parameters)[:6] == ["columns", "values", "inverse", "capacity", "lds_slots", "bounds"][:6]
    assert sig.parameters["values"].default == () and sig.parameters["inverse"].default is False
    assert sig.parameters["capacity"].default is None and sig.parameters["lds_slots"].default is None
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("inverse", "capacity", "lds_slots"))
    assert engine.Groups._fields == ("keys", "sums", "inverse")
    assert list(inspect.signature(engine.decimal_code).parameters) == ["columns", "widths"]
    assert list(inspect.signature(preprocess.aggregate_visits).parameters)[:6] == ["date", "destination", "dayofweek", "sex", "age", "visitor"]
    assert list(inspect.signature(preprocess.map_ids).parameters)[:5] == ["age", "sex", "month", "day", "destination"]
    assert list(inspect.signature(preprocess.num_dict).parameters) == ["ids", "sex", "age", "month", "day", "dayofweek"]
    assert preprocess.USER_KEY_WIDTHS == (0, 0, 2, 2)
    assert "Not here" in preprocess.__doc__ and "`map_ids` (pandas string" not in preprocess.__doc__

    i64 = torch.arange(6, dtype=torch.int64)
    i32 = i64.to(torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        engine.group_by([i64])
    with pytest.raises(RuntimeError, match="ROCm device"):
        engine.group_by([i64, i32], [i64], inverse=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        engine.decimal_code([i64, i32], (0, 2))
    with pytest.raises(RuntimeError, match="ROCm device"):
        preprocess.aggregate_visits(i64, i64, i64, i64, i64, i64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        preprocess.map_ids(i64, i64, i64, i64, i64)
    ids = preprocess.IdMaps(i64, i64, i64, i64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        preprocess.num_dict(ids, i64, i64, i64, i64, i64)
    # floating value columns: refused with the reason, before the device is looked at
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        with pytest.raises(TypeError, match="compensated.*arrival order"):
            engine.group_by([i64], [i64.to(dt)])
    with pytest.raises(TypeError, match="compensated"):
        preprocess.aggregate_visits(i64, i64, i64, i64, i64, i64.double())
    with pytest.raises(TypeError, match="key column 0 must be int32 or int64"):
        engine.group_by([i64.double()])
    with pytest.raises(TypeError, match="key column 1 must be int32 or int64"):
        engine.group_by([i64, i64.to(torch.int16)])
    with pytest.raises(TypeError, match="value column 0 must be int32 or int64"):
        engine.group_by([i64], [i64.to(torch.uint8)])
    with pytest.raises(TypeError, match="column 0 must be int32 or int64"):
        engine.decimal_code([i64.float()], (0,))
    with pytest.raises(ValueError, match="0 key columns"):
        engine.group_by([])
    with pytest.raises(ValueError, match="9 key columns"):
        engine.group_by([i64] * 9)
    with pytest.raises(ValueError, match="5 value columns"):
        engine.group_by([i64], [i64] * 5)
    with pytest.raises(ValueError, match="has 5 rows"):
        engine.group_by([i64, i64[:5]])
    with pytest.raises(ValueError, match="must be \\[T\\]"):
        engine.group_by([i64.view(2, 3)])
    for cap in (0, 48, -64, 2 ** 37):
        with pytest.raises(ValueError, match="capacity="):
            engine.group_by([i64], capacity=cap)
    for slots in (8, 96, 4096, -16):
        with pytest.raises(ValueError, match="lds_slots="):
            engine.group_by([i64], lds_slots=slots)
    with pytest.raises(ValueError, match="2 bounds for 1 columns"):
        engine.group_by([i64], bounds=[(0, 5), (0, 5)])
    with pytest.raises(ValueError, match="2 widths for 1 columns"):
        engine.decimal_code([i64], (0, 2))
    with pytest.raises(ValueError, match="widths .* outside"):
        engine.decimal_code([i64], (19,))
    with pytest.raises(ValueError, match="more than 18 characters"):
        engine.decimal_code([i64, i64], (9, 10))


def test_packing_is_lexicographic_and_stops_at_63_bits():
    from seoul_tourism_recommendation_ngcf_amd import engine
    off, rng, bits, shifts = engine.groupby_packing([(20180101, 20191231), (125452, 2505927), (0, 6), (1, 1), (-5, 75)])
    assert off == [20180101, 125452, 0, 1, -5] and rng == [11130, 2380475, 6, 0, 80]
    assert bits == [14, 22, 3, 0, 7] and shifts == [32, 10, 7, 7, 0]
    assert engine.groupby_packing([(-2 ** 63, -1)])[2] == [63]                      # exactly 63 bits pass
    assert engine.groupby_packing([(0, 2 ** 31 - 1), (0, 2 ** 32 - 1)])[2] == [31, 32]
    with pytest.raises(ValueError, match="64 bits"):
        engine.groupby_packing([(-2 ** 63, 2 ** 63 - 1)])
    with pytest.raises(ValueError, match="32 \\+ 32 = 64 bits"):
        engine.groupby_packing([(0, 2 ** 32 - 1), (0, 2 ** 32 - 1)])
    with pytest.raises(ValueError, match="below its minimum"):
        engine.groupby_packing([(3, 2)])
    rs = np.random.RandomState(5)
    bounds = [(-7, 9), (100, 100), (0, 1000), (-2 ** 40, 2 ** 40)]
    off, rng, bits, shifts = engine.groupby_packing(bounds)
    rows = [tuple(int(rs.randint(lo, hi + 1)) if hi - lo < 2 ** 31 else int(rs.randint(-2 ** 31, 2 ** 31)) * 512 for lo, hi in bounds)
            for _ in range(500)]
    packed = [sum((v - o) << s for v, o, s in zip(r, off, shifts)) for r in rows]
    assert max(packed) < 2 ** 63
    assert [r for _, r in sorted(zip(packed, rows))] == sorted(rows)


def test_decimal_strings_and_codes_round_trip():
    from seoul_tourism_recommendation_ngcf_amd import engine
    for s in ("0", "5", "50101", "1500101", "10501231", "9" * 18, "1" + "0" * 17):
        assert engine.decimal_string(orc.code_of_string(s)) == s
    assert orc.code_of_string("9" * 18) < 2 ** 63 and 11 ** 18 < 2 ** 63
    for bad in (-1, 11 ** 18, 11 ** 17 + 5):                                        # the last has padding inside the string
        with pytest.raises(ValueError):
            engine.decimal_string(bad)
    words = ["5", "45", "55", "450", "5000101", "4511231", "5500101", "15", "105", "1", "10", "100", "19", "2"]
    assert sorted(words) == [w for _, w in sorted((orc.code_of_string(w), w) for w in words)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_numpy_pivot_oracle_equals_pandas_pivot_table(seed):
    rs = np.random.RandomState(seed)
    T = 4000
    days = np.array([20180101, 20180102, 20181231, 20190101, 20190615, 20200229])
    df = pd.DataFrame({"date": days[rs.randint(0, len(days), T)], "destination": rs.choice([125452, 126480, 2505927, 130000], T),
                       "dayofweek": rs.randint(0, 7, T), "sex": rs.randint(0, 2, T), "age": rs.choice([5, 15, 25, 75], T),
                       "visitor": rs.randint(-50, 5000, T).astype(np.int64)})
    index = ["date", "destination", "dayofweek", "sex", "age"]
    want = pd.pivot_table(df, index=index, aggfunc={"visitor": "sum"}).reset_index()
    keys, sums, inverse = orc.pivot([df[c].values for c in index], [df["visitor"].values])
    assert len(want) == len(keys[0]) < T
    for k, name in enumerate(index):
        assert keys[k].dtype == np.int64 and np.array_equal(keys[k], want[name].values.astype(np.int64)), name
    assert sums[0].dtype == np.int64 and np.array_equal(sums[0], want["visitor"].values.astype(np.int64))
    for k, name in enumerate(index):
        assert np.array_equal(keys[k][inverse], df[name].values)
    # the reference pivots on datetimes: the integer yyyymmdd sorts the same way
    dt = pd.to_datetime(df["date"].astype("str"))
    want_dt = pd.pivot_table(df.assign(date=dt), index=index, aggfunc={"visitor": "sum"}).reset_index()
    assert np.array_equal(want_dt["date"].dt.strftime("%Y%m%d").astype(np.int64).values, keys[0])
    assert np.array_equal(want_dt["visitor"].values, sums[0])
    assert np.array_equal(want_dt["date"].dt.strftime("%y").astype(np.int64).values, (keys[0] // 10000) % 100)
    assert np.array_equal(want_dt["date"].dt.strftime("%m").astype(np.int64).values, (keys[0] // 100) % 100)
    assert np.array_equal(want_dt["date"].dt.strftime("%d").astype(np.int64).values, keys[0] % 100)


def test_id_map_oracle_and_base11_order_reproduce_the_saved_dictionaries():
    g = _golden()
    assert g["user_keys"].dtype.kind == "U" and len(g["user_keys"]) == 5840 and len(g["item_keys"]) == 100
    assert np.array_equal(g["user_ids"], np.arange(5840)) and np.array_equal(g["item_ids"], np.arange(100))
    age, sex, month, day = orc.reference_users()
    assert len(age) == 5840
    dest = g["item_keys"][np.arange(5840) % 100]
    perm = np.random.RandomState(0).permutation(5840)
    userid, itemid, user_map, item_map = orc.id_maps(age[perm], sex[perm], month[perm], day[perm], dest[perm])
    assert list(user_map.items()) == list(zip(g["user_keys"].tolist(), g["user_ids"].tolist()))          # entry for entry, in order
    assert list(item_map.items()) == list(zip(g["item_keys"].tolist(), g["item_ids"].tolist()))
    strings = orc.user_strings(age[perm], sex[perm], month[perm], day[perm])
    assert [user_map[s] for s in strings] == userid.tolist() and [item_map[int(d)] for d in dest[perm]] == itemid.tolist()
    # the base-11 code orders the 5 840 combinations as the saved dictionary does - not numerically: age 5 lies between 45 and 55
    code = orc.decimal_code((age, sex, month, day), (0, 0, 2, 2))
    assert len(set(code.tolist())) == 5840 and int(code.max()) < 2 ** 63
    order = np.argsort(code, kind="stable")
    assert orc.user_strings(age[order], sex[order], month[order], day[order]).tolist() == g["user_keys"].tolist()
    ages_in_order = [a for k, a in enumerate(age[order].tolist()) if k == 0 or a != age[order][k - 1]]
    assert ages_in_order == [15, 25, 35, 45, 5, 55, 65, 75]
    assert [orc.code_of_string(s) for s in g["user_keys"].tolist()] == sorted(code.tolist())
