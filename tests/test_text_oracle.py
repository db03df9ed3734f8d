"""tests/text_oracle.py against pandas: the oracle of the delimited-text kernels reads what `pd.read_csv(sep='|', usecols=, dtype=)` reads,
integers equal and floats bit for bit, on the generated cases of tests/test_text_gpu.py; its fast-path arithmetic is `float()`'s."""
import io

import numpy as np
import pandas as pd
import pytest

import text_oracle as orc


def _table(columns, *, end=b"\n", final=True, header=None, sep=b"|"):
    """Rows out of equally long lists of byte fields."""
    lines = [sep.join(header)] if header is not None else []
    lines += [sep.join(fields) for fields in zip(*columns)]
    return end.join(lines) + (end if final else b"")


def _pin(data, columns, *, sep="|", header=True, float_precision=None):
    got, n_rows, n_slow = orc.read_table(data, columns, sep=sep.encode(), header=header)
    df = pd.read_csv(io.BytesIO(data), sep=sep, usecols=list(columns), dtype=dict(columns), header=0 if header else None,
                     float_precision=float_precision)
    assert n_rows == len(df)
    for c in columns:
        assert orc.same_bits(got[c], df[c].to_numpy()), c
    return got, n_slow


def test_realistic_decimals_are_fast_fields_and_pandas_reads_pythons_bits():
    rng = np.random.default_rng(11)
    fields = orc.realistic_decimal(rng, 20000)
    ints = [str(int(v)).encode() for v in rng.integers(-10 ** 6, 10 ** 6, len(fields))]
    data = _table([ints, fields, fields[::-1]], header=[b"k", b"x", b"y"])
    got, n_slow = _pin(data, {"x": "float64", "k": "int64", "y": "float64"})
    assert n_slow == 0                                                  # a condition on the generator, not a measurement
    assert all(orc.float_class(f)[0] in ("fast", "zero") for f in fields)
    assert orc.same_bits(got["x"], np.array([float(f) for f in fields]))
    assert {orc.float_class(f)[0] for f in fields} == {"fast", "zero"} and any(b"e" in f for f in fields) and any(f.startswith(b".") or b"-." in f for f in fields)


def test_fast_path_arithmetic_in_numpy_is_float():
    rng = np.random.default_rng(12)
    n = 100000
    m = np.where(rng.random(n) < 0.5, rng.integers(1, 2 ** 53 + 1, n), rng.integers(1, 10 ** 6, n))
    e = rng.integers(-22, 23, n)
    m[:4], e[:4] = (2 ** 53, 2 ** 53, 1, 2 ** 53 - 1), (22, -22, -22, 22)
    for mi, ei, neg in zip(m.tolist(), e.tolist(), (rng.random(n) < 0.3).tolist()):
        text = ("-" if neg else "") + f"{mi}e{ei}"
        assert orc.float_class(text.encode()) == ("fast", neg, mi, ei)
        want, got = float(text), orc.fast_value(neg, mi, ei)
        assert np.float64(want).view(np.int64) == got.view(np.int64), text


def test_classes_at_the_edges_of_the_fast_path():
    cls = lambda s: orc.float_class(s)[0]   # noqa: E731
    assert cls(b"9007199254740992") == "fast" and cls(b"9007199254740993") == "slow"
    assert cls(b"1e22") == "fast" and cls(b"1e23") == "slow" and cls(b"1e-22") == "fast" and cls(b"1e-23") == "slow"
    assert cls(b"0.0000000000000000000001") == "fast" and cls(b"00000000000000000000001.5") == "fast"
    assert cls(b"12345678901234567") == "slow" and cls(b"1234567890123456789") == "slow" and cls(b"12345678901234567890") == "slow"
    assert cls(b"1.7976931348623157e308") == "slow" and cls(b"5e-324") == "slow"
    assert cls(b"0e999") == "zero" and cls(b"-0.000") == "zero" and cls(b"-.0") == "zero"
    assert cls(b"") == "nan" and cls(b"NA") == "nan" and cls(b"+inf") == "inf" and cls(b"-Infinity") == "inf"
    for bad in (b".", b"+", b"1e", b"1e+", b"1.2.3", b"0x10", b"1_0", b"--1", b"nan1", b"-nan", b"INF", b"1 2", b"e5", b"1d5"):
        assert cls(bad) == "bad", bad


def test_special_spellings_signed_zeros_ints_and_padding_agree_with_pandas():
    ints = [b"0", b"-0", b"+7", b"007", b"-0012", b"9223372036854775807", b"-9223372036854775808", b" 5", b"6 ", b"\t8\t ", b"  -9"]
    floats = [b"", b"nan", b"NaN", b"NA", b"inf", b"-inf", b"+inf", b"Infinity", b"-Infinity", b"0", b"-0"]
    more = [b"-0.0", b"+0.0", b"0e5", b"-0e-5", b" 1.5 ", b"\t2.5", b"5.", b".5", b"-.5e1", b"1E5", b"+3"]
    data = _table([ints, floats, more], header=[b"i", b"f", b"g"])
    got, _ = _pin(data, {"i": "int64", "f": "float64", "g": "float64"})
    assert got["i"].tolist() == [0, 0, 7, 7, -12, 2 ** 63 - 1, -2 ** 63, 5, 6, 8, -9]
    assert np.signbit(got["g"][0]) and not np.signbit(got["g"][1]) and np.signbit(got["g"][3])


def test_slow_fields_follow_float_and_pandas_round_trip_parser():
    fields = [b"9007199254740993", b"1e23", b"12345678901234567", b"123456789012345678", b"1234567890123456789", b"1.7976931348623157e308",
              b"5e-324", b"0.1234567890123456789", b"8.5e-23", b"123456789012345678901234567890", b"-1e-400"]
    data = _table([fields], header=[b"x"])
    got, n_slow = _pin(data, {"x": "float64"}, float_precision="round_trip")
    assert n_slow == len(fields) and orc.same_bits(got["x"], np.array([float(f) for f in fields]))
    assert orc.parse_float(b"1e400") == (float("inf"), True)            # pandas refuses the column; this follows float()


@pytest.mark.parametrize("end,final", [(b"\n", True), (b"\n", False), (b"\r\n", True), (b"\r\n", False)])
def test_line_ends_blank_lines_and_row_starts(end, final):
    body = _table([[b"1", b"2", b"3"], [b"1.5", b"", b"-2"]], end=end, final=final, header=[b"a", b"b"])
    lines = body.split(end)
    blanks = end + end + end.join(lines[:2]) + end + end + end.join(lines[2:]) + end + (b"\r" if final else b"")
    for data in (body, blanks):
        got, _ = _pin(data, {"b": "float64", "a": "int64"})
        assert got["a"].tolist() == [1, 2, 3]
        starts = orc.row_starts(data)
        assert starts[-1] == len(data) and [data[s:s + 1] for s in starts[:-1]] == [b"a", b"1", b"2", b"3"]
    assert orc.row_starts(b"") == [0] and orc.row_starts(b"\n\r\n\r") == [4] and orc.row_starts(b"x") == [0, 1]
    assert orc.row_texts(b"a|b\r") == [b"a|b"] and orc.row_texts(b"\n\na\r\n\r\nb") == [b"a", b"b"]


def test_column_choice_field_counts_delimiters_and_headers():
    rng = np.random.default_rng(13)
    cols = [[str(int(v)).encode() for v in rng.integers(-99, 99, 50)] for _ in range(64)]
    names = [b"c%d" % k for k in range(64)]
    data = _table(cols, header=names)
    _pin(data, {"c63": "int64", "c0": "float64", "c31": "int64", "c5": "int64"})                 # first, last, apart, not in file order
    _pin(_table(cols[:1], header=names[:1]), {"c0": "int64"})                                    # F = 1
    for sep in (",", ";", ":", "\x01", "a"):
        _pin(_table(cols[:3], header=[b"x", b"y", b"z"], sep=sep.encode()), {"z": "int64", "x": "float64"}, sep=sep)
    _pin(_table(cols[:3]), {2: "int64", 0: "float64"}, header=False)
    bom = b"\xef\xbb\xbf" + _table(cols[:3], header=["날짜".encode(), b"v", "Ortä".encode()])
    got, _ = _pin(bom, {"v": "int64"})
    assert got["v"].tolist() == [int(v) for v in cols[1]]
    got, _ = _pin(b"\xef\xbb\xbf" + _table(cols[:2], header=[b"first", b"v"]), {"first": "int64"})  # the mark in front of a selected name
    assert got["first"].tolist() == [int(v) for v in cols[0]]


def test_visit_log_equals_pandas():
    data = orc.visit_log(np.random.default_rng(14), 5000)
    got, _ = _pin(data, {c: "int64" for c in orc.VISIT_KEYS})
    assert len(got["date"]) == 5000 and set(got["date"] // 10000) == {2018, 2019}


def test_errors_name_the_first_offending_field():
    head = b"a|b|c\n"
    cases = [(b"1|2|3\n4|5\n7|x|9\n", 1, 0, "fields"), (b"1|2|3\n4|5|6|7\n7|x|9\n", 1, 0, "fields"), (b"1|2|3\n4|x5|6\n7|8\n", 1, 1, "byte"),
             (b"1|2|3\n4| |6\n7|x|9\n", 1, 1, "empty"), (b"1|9223372036854775808|3\n1|x|2\n", 0, 1, "overflow"),
             (b"1|-9223372036854775809|3\n1|x|2\n", 0, 1, "overflow"), (b"1|2|3\n4|5|\"6\"\n7|x|9\n", 1, 2, "quote"),
             (b"1|2|3\n4|2.5|6\n7|x|9\n", 1, 1, "byte"), (b"1|99999999999999999999x|3\n", 0, 1, "byte")]
    for body, row, field, kind in cases:
        with pytest.raises(orc.TextError) as err:
            orc.read_table(head + body, {"a": "int64", "b": "int64"})
        assert (err.value.row, err.value.field, err.value.kind) == (row, field, kind), body
