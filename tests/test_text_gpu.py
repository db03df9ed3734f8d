"""The delimited-text kernels on the device against tests/text_oracle.py, bit for bit: row starts, both tiers of the parse at their
boundaries (sizes from `engine.text.limits()`), the grammar with its slow fields, every error kind, and `preprocess.load_visits` end
to end.  Every error case here is one the kernel detects and reports through its status block; none reads out of bounds."""
import io

import numpy as np
import pandas as pd
import pytest
import torch

import text_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def text():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.text


def _dev(data: bytes) -> torch.Tensor:
    return torch.tensor(np.frombuffer(data, dtype=np.uint8), device=DEV)


def _dtypes(columns):
    return {c: {"int64": torch.int64, "float64": torch.float64}[k] for c, k in columns.items()}


def _check(text, data: bytes, columns, *, sep="|", header=True):
    """read_table on the device == the oracle, bit for bit; returns the oracle's (columns, n_slow)."""
    want, n_rows, n_slow = orc.read_table(data, columns, sep=sep.encode(), header=header)
    got, n_got = text.read_table(_dev(data), _dtypes(columns), sep=sep, header=header)
    assert n_got == n_rows and list(got) == list(columns)
    for c in columns:
        assert orc.same_bits(got[c].cpu().numpy(), want[c]), c
    return want, n_slow


def _table(columns, *, end=b"\n", final=True, header=None, sep=b"|"):
    lines = [sep.join(header)] if header is not None else []
    lines += [sep.join(fields) for fields in zip(*columns)]
    return end.join(lines) + (end if final else b"")


# ---- line starts -----------------------------------------------------------------------------------------------------------------------
def test_row_starts_small_buffers_line_ends_and_blank_lines(text):
    cases = [b"", b"a|1", b"a|1\n", b"a|1\r\n", b"a\r\nb\r\nc", b"\n\na\n\nb\n\n", b"\r\n\r\na\r\n\r\nb\r\n\r\n", b"a\nb\n\r", b"\r", b"\n", b"\r\n",
             b"a\n\r", b"a\rb\n", b"\n\r\n\rx", b"x" * 15 + b"\n", b"x" * 16 + b"\ny", b"x" * 14 + b"\r\n" + b"y" * 20, b"ab\n" * 200]
    for data in cases:
        got = text.row_starts(_dev(data))
        assert got.dtype == torch.int64 and got.tolist() == orc.row_starts(data), data


def test_row_starts_around_a_counting_block(text):
    block = text.limits()[2]
    rng = np.random.default_rng(21)
    for n in (block - 1, block, block + 1, 3 * block + 5):
        raw = rng.choice(np.frombuffer(b"ab|1\n\n\r", dtype=np.uint8), n)
        for tail in (None, (block - 1, 0x0A), (block, 0x0A)):                       # a newline as a block's last byte, and as the next one's first
            buf = raw.copy()
            if tail is not None and tail[0] < n:
                buf[max(tail[0] - 1, 0)], buf[tail[0]] = ord("a"), tail[1]
                if tail[0] + 1 < n:
                    buf[tail[0] + 1] = ord("b")
            data = buf.tobytes()
            assert text.row_starts(_dev(data)).tolist() == orc.row_starts(data), (n, tail)
    view = _dev(b"zz" + b"a\nb\n")[2:]                                             # a view that is not 16-byte aligned
    assert text.row_starts(view).tolist() == [0, 2, 4]


def test_rows_beyond_two_to_the_31_bytes(text):
    n = 2 ** 31 + 4096
    data = torch.full((n,), 0x0A, dtype=torch.uint8, device=DEV)                    # blank lines
    pieces = {0: b"a|b\n1|2.5\n", 2 ** 31 - 3: b"3|4.5\n", 2 ** 31 + 100: b"-5|1e-3"}
    for at, piece in pieces.items():
        data[at:at + len(piece)] = _dev(piece)
    starts = text.row_starts(data)
    assert starts.tolist() == [0, 4, 2 ** 31 - 3, 2 ** 31 + 100, n]
    got, n_rows = text.read_table(data, {"b": torch.float64, "a": torch.int64})
    assert n_rows == 3 and got["a"].tolist() == [1, 3, -5] and got["b"].tolist() == [2.5, 4.5, 1e-3]


# ---- parse tiers -----------------------------------------------------------------------------------------------------------------------
def _run_of(rng, n_rows, n_bytes):
    """`n_rows` rows 'int|float|pad' of `n_bytes` bytes in all (newlines included), the padding column taking up the slack."""
    ints = [str(int(v)).encode() for v in rng.integers(-10 ** 9, 10 ** 9, n_rows)]
    floats = orc.realistic_decimal(rng, n_rows)
    slack = n_bytes - sum(len(a) + len(b) + 3 for a, b in zip(ints, floats))
    assert slack >= n_rows
    pads = [b"7" * (slack // n_rows + (1 if r < slack % n_rows else 0)) for r in range(n_rows)]
    out = b"".join(a + b"|" + b + b"|" + p + b"\n" for a, b, p in zip(ints, floats, pads))
    assert len(out) == n_bytes
    return out


def test_parse_run_bytes_around_the_lds_budget(text):
    rows, lds, _ = text.limits()
    rng = np.random.default_rng(22)
    head = b"i|x|pad\n"
    for n_bytes in (lds - 1, lds, lds + 1):
        data = head + _run_of(rng, rows, n_bytes) + _run_of(rng, 3, 200)                 # a full run at the size, and a second workgroup
        want, n_slow = _check(text, data, {"x": "float64", "i": "int64"})
        assert n_slow == 0 and len(want["i"]) == rows + 3
        d, starts = _dev(data), text.row_starts(_dev(data))
        call = lambda tier: text.parse_columns(d, starts, [0, 1], [0, 1], n_fields=3, skip_rows=1, tier=tier)   # noqa: E731
        if n_bytes <= lds:
            lds_cols = call("lds")                                                       # every row ends inside the staged bytes
        else:
            with pytest.raises(RuntimeError, match="tier='lds'"):
                call("lds")
            lds_cols = call(None)
        for a, b in zip(lds_cols, call("memory")):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("where", ["first", "last"])
def test_one_row_longer_than_the_budget_among_short_rows(text, where):
    rows, lds, _ = text.limits()
    rng = np.random.default_rng(23)
    short = [b"%d|%s|7" % (v, f) for v, f in zip(rng.integers(-99, 99, rows - 1).tolist(), orc.realistic_decimal(rng, rows - 1))]
    long_row = b"12345|-0.5|" + b"7" * (lds + 100)
    body = [long_row] + short if where == "first" else short + [long_row]
    data = b"i|x|pad\n" + b"\n".join(body + [b"8|9.25|7"])                              # one more row: a second workgroup
    want, _ = _check(text, data, {"i": "int64", "x": "float64"})
    assert want["i"][0 if where == "first" else rows - 1] == 12345 and want["x"][-1] == 9.25


def test_row_counts_around_a_workgroup(text):
    rows = text.limits()[0]
    rng = np.random.default_rng(24)
    for n in (1, rows - 1, rows, rows + 1, 2 * rows + 1):
        cols = [[str(int(v)).encode() for v in rng.integers(-10 ** 12, 10 ** 12, n)], orc.realistic_decimal(rng, n)]
        for final in (True, False):
            _check(text, _table(cols, header=[b"a", b"b"], final=final), {"b": "float64", "a": "int64"})
    got, n_rows = text.read_table(_dev(b"a|b\n"), {"a": torch.int64, "b": torch.float64})    # a header and no rows
    assert n_rows == 0 and got["a"].numel() == 0 and got["b"].dtype == torch.float64


def test_both_tiers_give_equal_bits_on_50000_rows(text):
    rng = np.random.default_rng(25)
    n = 50000
    cols = [[str(int(v)).encode() for v in rng.integers(-2 ** 62, 2 ** 62, n)], orc.realistic_decimal(rng, n),
            [str(int(v)).encode() for v in rng.integers(0, 100, n)], orc.realistic_decimal(rng, n)]
    data = _table(cols, header=[b"a", b"b", b"c", b"d"])
    d = _dev(data)
    starts = text.row_starts(d)
    lds = text.parse_columns(d, starts, [3, 0, 1], [1, 0, 1], n_fields=4, skip_rows=1, tier="lds")
    mem = text.parse_columns(d, starts, [3, 0, 1], [1, 0, 1], n_fields=4, skip_rows=1, tier="memory")
    want, _, n_slow = orc.read_table(data, {"d": "float64", "a": "int64", "b": "float64"})
    assert n_slow == 0
    for a, b, w in zip(lds, mem, want.values()):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and orc.same_bits(a.cpu().numpy(), w)


# ---- grammar ---------------------------------------------------------------------------------------------------------------------------
def test_ints_floats_special_spellings_and_padding(text):
    ints = [b"0", b"-0", b"+7", b"007", b"-0012", b"9223372036854775807", b"-9223372036854775808", b" 5", b"6 ", b"\t8\t ", b"  -9"]
    floats = [b"", b"nan", b"NaN", b"NA", b"inf", b"-inf", b"+inf", b"Infinity", b"-Infinity", b"0", b"-0"]
    more = [b"-0.0", b"+0.0", b"0e5", b"-0e-5", b" 1.5 ", b"\t2.5", b"5.", b".5", b"-.5e1", b"1E5", b"  "]
    edges = [b"9007199254740992", b"-9007199254740992", b"9007199254740992e22", b"9007199254740992e-22", b"1e22", b"1e-22", b"3e22", b"7e-22",
             b"0.0000000000000000000001", b"00000000000000000000001.5", b"123456789012345e-22"]
    want, n_slow = _check(text, _table([ints, floats, more, edges], header=[b"i", b"f", b"g", b"h"]),
                          {"i": "int64", "f": "float64", "g": "float64", "h": "float64"})
    assert n_slow == 0 and want["i"].tolist() == [0, 0, 7, 7, -12, 2 ** 63 - 1, -2 ** 63, 5, 6, 8, -9]
    assert np.signbit(want["g"][0]) and not np.signbit(want["g"][1]) and np.signbit(want["g"][3]) and np.isnan(want["g"][-1])
    rng = np.random.default_rng(26)
    fields = orc.realistic_decimal(rng, 20000)
    want, n_slow = _check(text, _table([fields], header=[b"x"]), {"x": "float64"})
    assert n_slow == 0 and orc.same_bits(want["x"], np.array([float(f) for f in fields]))


def test_slow_fields_match_float_through_the_patch(text):
    slow = [b"9007199254740993", b"1e23", b"12345678901234567", b"123456789012345678", b"1234567890123456789", b"1.7976931348623157e308",
            b"5e-324", b"0.1234567890123456789", b"8.5e-23", b"123456789012345678901234567890", b"1e400", b"-1e-400"]
    fast = [b"1.5"] * len(slow)
    data = _table([slow, fast, slow[::-1]], header=[b"x", b"y", b"z"], end=b"\r\n")
    want, n_slow = _check(text, data, {"z": "float64", "y": "float64", "x": "float64"})
    assert n_slow == 2 * len(slow) and orc.same_bits(want["x"], np.array([float(f) for f in slow]))
    # more slow fields than the first list holds: the parse runs again with a list of the reported size
    n = text.TEXT_SLOW_CAPACITY + 300
    rng = np.random.default_rng(27)
    many = [b"%d.%017d" % (a, b) for a, b in zip(rng.integers(1, 99, n).tolist(), rng.integers(0, 10 ** 17, n).tolist())]
    want, n_slow = _check(text, _table([many, [b"1"] * n], header=[b"x", b"k"]), {"k": "int64", "x": "float64"})
    assert n_slow == n and orc.same_bits(want["x"], np.array([float(f) for f in many]))
    d = _dev(_table([slow], header=[b"x"]))
    small = text.parse_columns(d, text.row_starts(d), [0], [torch.float64], n_fields=1, skip_rows=1, slow_capacity=0)[0]
    assert orc.same_bits(small.cpu().numpy(), np.array([float(f) for f in slow]))


def test_column_choice_field_counts_delimiters_and_headers(text):
    rng = np.random.default_rng(28)
    cols = [[str(int(v)).encode() for v in rng.integers(-99, 99, 300)] for _ in range(64)]
    names = [b"c%d" % k for k in range(64)]
    _check(text, _table(cols, header=names), {"c63": "int64", "c0": "float64", "c31": "int64", "c5": "int64"})     # F = 64
    _check(text, _table(cols, header=names), {"c%d" % k: ("int64", "float64")[k % 2] for k in range(40, 24, -1)})   # 16 columns
    _check(text, _table(cols[:1], header=names[:1]), {"c0": "int64"})                                           # F = 1
    for sep in (",", ";", "\x01", "a"):
        _check(text, _table(cols[:3], header=[b"x", b"y", b"z"], sep=sep.encode()), {"z": "int64", "x": "float64"}, sep=sep)
    _check(text, _table(cols[:3], final=False), {2: "int64", 0: "float64"}, header=False)
    bom = b"\xef\xbb\xbf" + _table(cols[:3], header=["날짜".encode(), b" v\t", "Ortä".encode()])
    want, _ = _check(text, bom, {"v": "int64"})
    assert want["v"].tolist() == [int(v) for v in cols[1]]
    _check(text, b"\xef\xbb\xbf" + _table(cols[:2], header=[b"first", b"v"]), {"first": "int64"})
    d = _dev(_table(cols[:3], header=[b"x", b"y", b"x"]))
    with pytest.raises(KeyError, match="no column 'w'"):
        text.read_table(d, {"w": torch.int64})
    with pytest.raises(ValueError, match="2 columns 'x'"):
        text.read_table(d, {"x": torch.int64})
    with pytest.raises(ValueError, match="longer than 65536 bytes"):
        text.read_table(_dev(b"a|" + b"b" * 70000 + b"\n1|2\n"), {"a": torch.int64})
    with pytest.raises(ValueError, match="no header"):
        text.read_table(_dev(b"\n\r\n"), {"a": torch.int64})


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
ERRORS = [("too few fields", b"1|2|3\n4|5\n7|x|9\n", "wrong number of fields"), ("too many fields", b"1|2|3\n4|5|6|7\n7|x|9\n", "wrong number of fields"),
          ("a letter", b"1|2|3\n4|x5|6\n7|8\n", "bad byte"), ("an empty int", b"1|2|3\n4| |6\n7|x|9\n", "empty int field"),
          ("overflow by one", b"1|9223372036854775807|3\n1|9223372036854775808|3\n1|x|2\n", "int64 overflow"),
          ("underflow by one", b"1|-9223372036854775808|3\n1|-9223372036854775809|3\n1|x|2\n", "int64 overflow"),
          ("a quote", b"1|2|3\n4|5|\"6\"\n7|x|9\n", "quote"), ("2.5 in an int column", b"1|2|3\n4|2.5|6\n7|x|9\n", "bad byte"),
          ("a bad float", b"1|2|3\n4|5|1e\n7|x|9\n", "bad byte")]


@pytest.mark.parametrize("name,body,kind", ERRORS, ids=[e[0].replace(" ", "_") for e in ERRORS])
def test_errors_name_the_first_offending_row_column_and_kind(text, name, body, kind):
    rows = text.limits()[0]
    columns = {"a": "int64", "b": "int64", "c": "float64"}
    for filler in (0, rows + 7):                                                     # the offending row in the first and in a later workgroup
        data = b"a|b|c\n" + b"5|6|7\n" * filler + body + b"1|2\n"                    # and one more error at the end
        with pytest.raises(orc.TextError) as want:
            orc.read_table(data, columns)
        assert orc.KINDS[want.value.kind] == kind and want.value.row == filler + 1
        where = f"data row {want.value.row}" + ("" if want.value.kind == "fields" else f", column {'abc'[want.value.field]!r}")
        with pytest.raises(ValueError) as got:
            text.read_table(_dev(data), _dtypes(columns))
        assert f"{where}: {kind}" in str(got.value), str(got.value)
    with pytest.raises(ValueError, match="quote in the 1 leading rows"):
        text.read_table(_dev(b"a|\"b\"\n1|2\n"), {"a": torch.int64})


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_load_visits_equals_aggregate_visits_of_the_oracle_and_the_pandas_pivot(tmp_path):
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    data = orc.visit_log(np.random.default_rng(29), 200000)
    want, n_rows, _ = orc.read_table(data, {c: "int64" for c in orc.VISIT_KEYS})
    assert n_rows == 200000
    path = tmp_path / "visits.txt"
    path.write_bytes(data)
    cols = preprocess.read_visits(str(path))
    for c, got in zip(orc.VISIT_KEYS, cols):
        assert got.dtype == torch.int64 and got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), want[c]), c
    table = preprocess.load_visits(path)
    ref = preprocess.aggregate_visits(*(torch.from_numpy(want[c]).to(DEV) for c in orc.VISIT_KEYS))
    again = preprocess.load_visits(_dev(data).cpu())
    assert len(table) == len(ref) < n_rows                                          # the time-zone rows were folded
    for f in ("date", "destination", "dayofweek", "sex", "age", "visitor", "year", "month", "day"):
        assert torch.equal(getattr(table, f), getattr(ref, f)) and torch.equal(getattr(table, f), getattr(again, f)), f
    # a slice against pandas itself
    part = b"\n".join(data.split(b"\n")[:5001])
    keys = ["date", "destination", "dayofweek", "sex", "age"]
    df = pd.pivot_table(pd.read_csv(io.BytesIO(part), sep="|"), index=keys, aggfunc={"visitor": "sum"}).reset_index()
    small = preprocess.load_visits(part)
    assert len(small) == len(df)
    for f in keys + ["visitor"]:
        assert np.array_equal(getattr(small, f).cpu().numpy(), df[f].to_numpy()), f
