"""The grammar of the header's section "delimited text" in plain Python, the oracle of tests/test_text_gpu.py; tests/test_text_oracle.py
pins it to `pd.read_csv` on every generated case.

Rows: position p starts a row if p == 0 or data[p-1] == '\\n', unless the line is blank ('\\n', '\\r\\n', or a '\\r' that ends the buffer); a
row's text ends before its '\\n' and before a '\\r' in front of that (or in front of the end of the buffer).  Fields: `split(sep)`, spaces
and tabs stripped, `int()` after a regex check, `float()` after one, with '', nan, NaN and NA for NaN.  A float field is FAST if, with
its digits read as an integer m (leading zeros dropped) and its decimal exponent e, m <= 2^53 and |e| <= 22 (or m == 0): then
`fast_value` restates the one fp64 multiply or divide of the kernel in numpy.  Everything else with a number's shape is SLOW.

What pandas does differently and the generators therefore leave out: a lone '\\r' inside the text ends a line for pandas; pandas pads
a row with too few fields with NaN (refused here); pandas knows more spellings of NaN (null, N/A, ...) and takes inf in any letter
case; a line of blanks only is a row here; a number beyond the doubles (1e400) is an infinity for `float()` and here, and makes
pandas refuse the column; on slow fields pandas' default parser is an ulp off here and there (0.1234567890123456789), its
`float_precision='round_trip'` is not, and that one the slow cases are pinned to."""
import re

import numpy as np

INT_RE = re.compile(rb"[+-]?[0-9]+\Z")
FLOAT_RE = re.compile(rb"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?\Z")
NAN_WORDS = (b"", b"nan", b"NaN", b"NA")
INF_RE = re.compile(rb"([+-]?)(?:inf|Infinity)\Z")
KINDS = {"fields": "wrong number of fields", "byte": "bad byte", "empty": "empty int field", "overflow": "int64 overflow", "quote": "quote"}
KIND_ORDER = ("fields", "byte", "empty", "overflow", "quote")          # the kernel's kind numbers 1..5
VISIT_HEADER = ("date", "date365", "dayofweek", "area", "destination", "sex", "age", "visitor", "total_num")
VISIT_KEYS = ("date", "destination", "dayofweek", "sex", "age", "visitor")


class TextError(Exception):
    """The first offending field: 0-based data row, field index (0 for a wrong field count) and kind (a key of KINDS)."""

    def __init__(self, row, field, kind):
        super().__init__(f"data row {row}, field {field}: {KINDS[kind]}")
        self.row, self.field, self.kind = row, field, kind


def row_starts(data: bytes):
    """[start of row 0, ..., start of the last row, len(data)]."""
    n, out = len(data), []
    for p in range(n):
        if p and data[p - 1] != 0x0A:
            continue
        c = data[p]
        blank = c == 0x0A or (c == 0x0D and (p + 1 == n or data[p + 1] == 0x0A))
        if not blank:
            out.append(p)
    return out + [n]


def row_texts(data: bytes):
    starts, n, out = row_starts(data), len(data), []
    for lo, hi in zip(starts, starts[1:]):
        cut = data.find(b"\n", lo, hi)
        end = hi if cut < 0 else cut
        if end > lo and data[end - 1] == 0x0D and (cut >= 0 or hi == n):
            end -= 1
        out.append(data[lo:end])
    return out


def float_class(field: bytes):
    """('nan' | 'inf' | 'zero' | 'fast' | 'slow' | 'bad', sign is '-', m, e) of a stripped field."""
    if field in NAN_WORDS:
        return "nan", False, 0, 0
    g = INF_RE.match(field)
    if g:
        return "inf", g.group(1) == b"-", 0, 0
    g = FLOAT_RE.match(field)
    if not g:
        return "bad", False, 0, 0
    whole, frac = (g.group(2), g.group(3) or b"") if g.group(2) is not None else (b"", g.group(4))
    digits = (whole + frac).lstrip(b"0")
    e = int(g.group(5) or 0) - len(frac)
    neg = g.group(1) == b"-"
    if not digits:
        return "zero", neg, 0, e
    if len(digits) > 19:
        return "slow", neg, 0, e
    m = int(digits)
    return ("fast" if m <= 2 ** 53 and abs(e) <= 22 else "slow"), neg, m, e


def fast_value(neg: bool, m: int, e: int) -> np.float64:
    """The kernel's fast path in numpy: one multiply or divide of two exact float64 values."""
    p = np.float64(float("1e%d" % abs(e)))
    v = np.float64(m) * p if e >= 0 else np.float64(m) / p
    return -v if neg else v


def parse_float(field: bytes):
    """(value, is_slow) of a raw field; ValueError for a bad byte."""
    field = field.strip(b" \t")
    cls, neg, m, e = float_class(field)
    if cls == "bad":
        raise ValueError("byte")
    if cls == "nan":
        return float("nan"), False
    return float(field.decode("ascii")), cls == "slow"


def parse_int(field: bytes) -> int:
    field = field.strip(b" \t")
    if not field:
        raise ValueError("empty")
    if not INT_RE.match(field):
        raise ValueError("byte")
    v = int(field)
    if not -2 ** 63 <= v < 2 ** 63:
        raise ValueError("overflow")
    return v


def read_table(data: bytes, columns, *, sep: bytes = b"|", header: bool = True):
    """`({name: numpy array}, n_rows, n_slow)` for `columns` = {name (or field index with header=False): 'int64' | 'float64'};
    TextError for the first offending field in (row, field, kind) order."""
    rows = row_texts(data)
    if header:
        head = rows[0][3:] if rows[0].startswith(b"\xef\xbb\xbf") else rows[0]
        names = [f.strip(b" \t").decode("utf-8", "replace") for f in head.split(sep)]
        rows = rows[1:]
    else:
        names = list(range(rows[0].count(sep) + 1)) if rows else []
    index = {c: names.index(c) for c in columns}
    out = {c: [] for c in columns}
    n_slow = 0
    for r, text in enumerate(rows):
        fields = text.split(sep)
        errors = []
        if len(fields) != len(names):
            errors.append((0, "fields"))
        for f, raw in enumerate(fields):
            if b'"' in raw:
                errors.append((f, "quote"))
        for c, kind in columns.items():
            raw = fields[index[c]] if index[c] < len(fields) else None
            try:
                if raw is None:
                    value = 0 if kind == "int64" else float("nan")
                elif kind == "int64":
                    value = parse_int(raw)
                else:
                    value, slow = parse_float(raw)
                    n_slow += slow
            except ValueError as exc:
                if b'"' not in raw:                                     # a quote is the field's error, whatever else it holds
                    errors.append((index[c], str(exc)))
                value = 0
            out[c].append(value)
        if errors:
            f, kind = min(errors, key=lambda fk: (fk[0], KIND_ORDER.index(fk[1])))
            raise TextError(r, f, kind)
    return {c: np.array(out[c], dtype=columns[c]) for c in columns}, len(rows), n_slow


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal dtype, shape and bytes; every NaN counts as the one NaN."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        a, b = (np.where(np.isnan(x), np.float64("nan"), x).view(np.int64) for x in (a, b))
    return bool(np.array_equal(a, b))


# ---- generators ------------------------------------------------------------------------------------------------------------------------
def realistic_decimal(rng, count):
    """Decimal fields as data files hold them: at most 15 significant digits, effective decimal exponent within +-22; plain, with a
    fraction, with an exponent, signed, with leading and trailing zeros.  Every one is a fast field."""
    out = []
    for _ in range(count):
        nd = int(rng.integers(1, 16))
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
        point = int(rng.integers(0, nd + 1))                           # digits after the point
        shape = int(rng.integers(0, 4))
        if shape == 0:                                                  # an integer
            body, point = digits, 0
        elif point == nd:
            body = ("0." if rng.integers(0, 2) else ".") + digits
        elif point == 0:
            body = digits + ("." if rng.integers(0, 2) else "")
        else:
            body = digits[:nd - point] + "." + digits[nd - point:]
        if shape == 3:
            ex = int(rng.integers(point - 22, 23))                      # the effective exponent ex - point stays within +-22
            sign = "-" if ex < 0 else ("", "+")[int(rng.integers(0, 2))]
            body += ("e", "E")[int(rng.integers(0, 2))] + sign + str(abs(ex))
        out.append((("", "-", "+")[int(rng.integers(0, 3))] + body).encode())
    return out


def visit_log(rng, n_lines, *, n_dest=40, n_days=60):
    """A Seoul-shaped log: the reference's nine column names, one line per (day, destination, sex, age, time zone) with the
    time-zone duplicates that the pivot folds; '\\n' line ends, no final newline."""
    day = rng.integers(0, n_days, n_lines)
    date = np.where(day < n_days // 2, 20180101, 20190101) + (day % (n_days // 2)) % 28 + 100 * ((day % (n_days // 2)) // 28)
    dest = 1000 + 7 * rng.integers(0, n_dest, n_lines)
    cols = {"date": date, "date365": day + 1, "dayofweek": day % 7, "area": rng.integers(1, 26, n_lines), "destination": dest,
            "sex": rng.integers(0, 2, n_lines), "age": 5 * rng.integers(0, 16, n_lines), "visitor": rng.integers(0, 5000, n_lines),
            "total_num": rng.integers(0, 100000, n_lines)}
    lines = ["|".join(VISIT_HEADER)] + ["|".join(str(int(cols[c][t])) for c in VISIT_HEADER) for t in range(n_lines)]
    return "\n".join(lines).encode()
