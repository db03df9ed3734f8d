"""Host side of the delimited-text family: the C ABI symbols and their gfx950 kernels, the ABI version that stays 11, `engine.text` as
a submodule beside an unchanged flat `engine`, refusals before any launch and before a device is needed, and the signatures of
`preprocess.read_visits` / `preprocess.load_visits`."""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

import test_engine_surface as pinned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ngcf_text_limits": ("int", 3), "ngcf_text_count_rows": ("int", 5), "ngcf_text_row_starts": ("int", 7),
           "ngcf_text_parse_columns": ("int", 16)}
KERNELS = (b"text_count_kernel", b"text_starts_kernel", b"text_parse_kernel")


def test_header_declares_and_library_exports_the_family_and_the_abi_stays_11():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    raw = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name, (ret, n_args) in SYMBOLS.items():
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert any(p.endswith("text.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    for k in KERNELS:
        assert k in blob, k
    assert "---- delimited text" in raw and "m <= 2^53 and |e| <= 22" in raw                       # the section and its fast-path rule
    assert int(re.search(r"#define\s+NGCF_ABI_VERSION\s+(\d+)", raw).group(1)) == int(lib.ngcf_version()) == _lib.ABI_VERSION == 11


def test_engine_text_is_a_module_and_the_flat_names_are_unchanged():
    from seoul_tourism_recommendation_ngcf_amd import engine
    assert isinstance(engine.text, types.ModuleType) and engine.text.__name__.endswith("engine.text")
    assert pinned._public_names() == set(pinned.PUBLIC)
    for name in ("row_starts", "parse_columns", "read_table", "limits"):
        assert callable(getattr(engine.text, name)) and not hasattr(engine, name)
    assert str(inspect.signature(engine.text.row_starts)) == "(data: 'torch.Tensor') -> 'torch.Tensor'"
    sig = inspect.signature(engine.text.parse_columns)
    assert list(sig.parameters)[:7] == ["data", "starts", "fields", "kinds", "n_fields", "skip_rows", "sep"]
    assert sig.parameters["n_fields"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["n_fields"].default is inspect.Parameter.empty
    assert sig.parameters["skip_rows"].default == 0 and sig.parameters["sep"].default == "|"
    sig = inspect.signature(engine.text.read_table)
    assert list(sig.parameters) == ["data", "columns", "sep", "header"]
    assert sig.parameters["sep"].default == "|" and sig.parameters["header"].default is True
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("sep", "header"))
    rows, lds, block = engine.text.limits()
    assert rows >= 64 and rows % 64 == 0 and 1024 <= lds <= 160 * 1024 and block % 16 == 0 and block >= 16


def test_c_abi_argument_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.int64)            # host memory: a call that got as far as a launch would not return ERR_ARG
    p = buf.data_ptr()
    assert p % 16 == 0

    def parse(data=p, n=64, starts=p, n_rows=4, skip=0, n_fields=3, delim=ord("|"), fields=(0, 2), kinds=(0, 1), n_columns=None, out=(p, p),
              slow=p, cap=4, tier=0, status=p):
        n_columns = len(fields) if n_columns is None else n_columns
        fa, ka = (C.c_int32 * max(len(fields), 1))(*fields), (C.c_int32 * max(len(kinds), 1))(*kinds)
        oa = (C.c_void_p * max(len(out), 1))(*out)
        return lib.ngcf_text_parse_columns(data, n, starts, n_rows, skip, n_fields, delim, fa, ka, n_columns, oa, slow, cap, tier, status, None)

    cases = [(dict(delim=ord("1")), "delimiter"), (dict(delim=ord("e")), "delimiter"), (dict(delim=ord('"')), "delimiter"),
             (dict(delim=ord("\n")), "delimiter"), (dict(delim=0x80), "delimiter"), (dict(delim=0), "delimiter"), (dict(delim=ord(" ")), "delimiter"),
             (dict(n_fields=65), "65 fields"), (dict(n_fields=0), "0 fields"), (dict(n_columns=17), "17 selected columns"),
             (dict(n_columns=0), "0 selected columns"), (dict(fields=(0, 3)), "selects field 3"), (dict(fields=(1, 1)), "selected twice"),
             (dict(kinds=(0, 2)), "kind 2"), (dict(skip=5), "bad row counts"), (dict(n_rows=-1), "bad row counts"), (dict(n=-1), "negative count"),
             (dict(data=p + 8), "16-byte aligned"), (dict(data=None), "null argument"), (dict(status=None), "null argument"),
             (dict(starts=None), "null argument"), (dict(out=(p, None)), "null argument"), (dict(slow=None), "null argument"),
             (dict(tier=3), "tier=3"), (dict(cap=-1), "slow_capacity=-1")]
    for kw, msg in cases:
        assert parse(**kw) == _lib.ERR_ARG, kw
        err = _lib.last_error()
        assert err.startswith("text_parse_columns: ") and msg in err, (kw, err)
    assert parse(n_rows=2, skip=2) == _lib.OK                                              # nothing to parse is not an error
    assert lib.ngcf_text_count_rows(None, 0, None, p, None) == _lib.OK and lib.ngcf_text_count_rows(p, -1, p, p, None) == _lib.ERR_ARG
    assert lib.ngcf_text_count_rows(p + 4, 8, p, p, None) == _lib.ERR_ARG and "16-byte aligned" in _lib.last_error()
    assert lib.ngcf_text_row_starts(p, 8, p, 9, p, p, None) == _lib.ERR_ARG and "n_rows=9" in _lib.last_error()
    assert lib.ngcf_text_row_starts(p, 8, p, 1, None, p, None) == _lib.ERR_ARG and lib.ngcf_text_count_rows(p, 8, p, None, None) == _lib.ERR_ARG


def test_python_refusals_before_any_device_work():
    from seoul_tourism_recommendation_ngcf_amd import engine
    t = engine.text
    data, starts = torch.zeros(32, dtype=torch.uint8), torch.tensor([0, 32])               # CPU tensors: the device is asked for last
    for sep in ("1", "+", "-", ".", "e", "E", " ", "\t", "\r", "\n", '"', "||", "", "\x80", "é"):
        with pytest.raises(ValueError, match="sep="):
            t.parse_columns(data, starts, [0], [0], n_fields=1, sep=sep)
        with pytest.raises(ValueError, match="sep="):
            t.read_table(data, {"a": torch.int64}, sep=sep)
    with pytest.raises(ValueError, match="17 selected columns"):
        t.parse_columns(data, starts, list(range(17)), [0] * 17, n_fields=20)
    with pytest.raises(ValueError, match="17 selected columns"):
        t.read_table(data, {f"c{k}": torch.int64 for k in range(17)})
    with pytest.raises(ValueError, match="0 selected columns"):
        t.read_table(data, {})
    with pytest.raises(ValueError, match="n_fields=65"):
        t.parse_columns(data, starts, [0], [0], n_fields=65)
    with pytest.raises(ValueError, match="field 3 outside"):
        t.parse_columns(data, starts, [3], [0], n_fields=3)
    with pytest.raises(ValueError, match="selected twice"):
        t.parse_columns(data, starts, [1, 1], [0, 1], n_fields=3)
    with pytest.raises(ValueError, match="tier="):
        t.parse_columns(data, starts, [0], [0], n_fields=1, tier="registers")
    for bad in (torch.int8, torch.int64, torch.float32):
        with pytest.raises(TypeError, match="data must be uint8"):
            t.parse_columns(data.to(bad), starts, [0], [0], n_fields=1)
        with pytest.raises(TypeError, match="data must be uint8"):
            t.read_table(data.to(bad), {"a": torch.int64})
        with pytest.raises(TypeError, match="data must be uint8"):
            t.row_starts(data.to(bad))
    for bad in (torch.int32, torch.float32, torch.uint8, "int64", 2, None):
        with pytest.raises(TypeError, match="int64 .* or float64"):
            t.parse_columns(data, starts, [0], [bad], n_fields=1)
        with pytest.raises(TypeError, match="int64 .* or float64"):
            t.read_table(data, {"a": bad})
    with pytest.raises(TypeError, match="starts must be int64"):
        t.parse_columns(data, starts.int(), [0], [0], n_fields=1)
    with pytest.raises(ValueError, match="data must be \\[n\\]"):
        t.row_starts(data.view(4, 8))
    for call in (lambda: t.row_starts(data), lambda: t.parse_columns(data, starts, [0], [torch.float64], n_fields=1),
                 lambda: t.read_table(data, {"a": torch.int64, "b": torch.float64})):
        with pytest.raises(RuntimeError, match="ROCm device"):                          # every argument was fine: only now the device
            call()


def test_preprocess_read_visits_and_load_visits_signatures():
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    sig = inspect.signature(preprocess.read_visits)
    assert list(sig.parameters) == ["source", "device", "columns", "sep"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("device", "columns", "sep"))
    assert sig.parameters["device"].default is None and sig.parameters["sep"].default == "|"
    assert tuple(sig.parameters["columns"].default) == ("date", "destination", "dayofweek", "sex", "age", "visitor")
    assert tuple(sig.parameters["columns"].default) == tuple(inspect.signature(preprocess.aggregate_visits).parameters)[:6]
    sig = inspect.signature(preprocess.load_visits)
    assert list(sig.parameters) == ["source", "device", "lds_slots"] and sig.return_annotation in ("VisitTable", preprocess.VisitTable)
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[n].default is None for n in ("device", "lds_slots"))
    with pytest.raises(TypeError, match="path, bytes or a uint8 tensor"):
        preprocess.read_visits(12)
    with pytest.raises(TypeError, match="must be uint8"):
        preprocess.read_visits(torch.zeros(4, dtype=torch.int32), device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        preprocess.read_visits(b"date|visitor\n1|2\n", device="cpu")
    assert "Reading the CSV stays the caller's" not in preprocess.__doc__ and ".sample(100)" in preprocess.__doc__
