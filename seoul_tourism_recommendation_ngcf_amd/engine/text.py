"""Delimited text on the device, the reference's `pd.read_csv(path, sep='|')` (utils.py:38-39) for integer and float columns:
`ngcf_text_count_rows`, `ngcf_text_row_starts`, `ngcf_text_parse_columns` (csrc/text.hip; the header's section "delimited text", where
the grammar is written out).  Reached as `engine.text.<name>`."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Sequence, Tuple

import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _require_dtype, _require_same_device, _stream

TEXT_MAX_FIELDS = 64
TEXT_MAX_COLUMNS = 16
TEXT_HEADER_MAX_BYTES = 64 * 1024
TEXT_SLOW_CAPACITY = 4096                   # entries of the slow-field list of a first parse; a fuller one is parsed once more
TEXT_FIELDS, TEXT_BYTE, TEXT_EMPTY, TEXT_OVERFLOW, TEXT_QUOTE, TEXT_LOST, TEXT_TIER = 1, 2, 4, 8, 16, 32, 64
TEXT_KINDS = {1: "wrong number of fields", 2: "bad byte", 3: "empty int field", 4: "int64 overflow", 5: "quote"}
_TIERS = {None: 0, "memory": 1, "lds": 2}
_BOM = b"\xef\xbb\xbf"


def limits() -> Tuple[int, int, int]:
    """`(rows_per_workgroup, lds_bytes, count_block_bytes)`: the rows a workgroup of the parse owns, the bytes of its run it brings
    into LDS (a row that ends beyond them is walked from memory), and the bytes of one block of the two row passes.  Compiled into
    the library; placeholders until tools/text_lab.py has run."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().ngcf_text_limits(C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def _delimiter(fn: str, sep) -> int:
    """The delimiter's byte: one byte below 0x80 that cannot be part of a number, a blank, a line end or a quote."""
    raw = sep.encode("utf-8", "surrogatepass") if isinstance(sep, str) else bytes(sep)
    if len(raw) != 1 or raw[0] >= 0x80 or raw[0] == 0 or raw in b"0123456789+-.eE \t\r\n\"":
        raise ValueError(f"{fn}: sep={sep!r} must be a single byte below 0x80 that is no digit, '+', '-', '.', 'e', 'E', space, tab, "
                         "CR, LF or '\"'")
    return raw[0]


def _kinds(fn: str, kinds) -> list:
    """0 (int64) / 1 (float64) per column, given as that or as the torch dtype."""
    out = []
    for k, kind in enumerate(kinds):
        if kind is torch.int64 or (not isinstance(kind, torch.dtype) and kind == 0):
            out.append(0)
        elif kind is torch.float64 or (not isinstance(kind, torch.dtype) and kind == 1):
            out.append(1)
        else:
            raise TypeError(f"{fn}: column {k} asks for {kind}; the columns are int64 (0) or float64 (1)")
    return out


def _selection(fn: str, fields, kinds, n_fields) -> Tuple[list, list, int]:
    fields, kinds, n_fields = [int(f) for f in fields], _kinds(fn, kinds), int(n_fields)
    if not 1 <= n_fields <= TEXT_MAX_FIELDS:
        raise ValueError(f"{fn}: n_fields={n_fields} outside [1, {TEXT_MAX_FIELDS}]")
    if not 1 <= len(fields) <= TEXT_MAX_COLUMNS:
        raise ValueError(f"{fn}: {len(fields)} selected columns, outside [1, {TEXT_MAX_COLUMNS}]")
    if len(kinds) != len(fields):
        raise ValueError(f"{fn}: {len(fields)} fields and {len(kinds)} kinds")
    for f in fields:
        if not 0 <= f < n_fields:
            raise ValueError(f"{fn}: field {f} outside [0, n_fields = {n_fields})")
    if len(set(fields)) != len(fields):
        raise ValueError(f"{fn}: a field is selected twice: {fields}")
    return fields, kinds, n_fields


def _buffer_checks(fn: str, data) -> None:
    """Type and shape of the byte buffer, which hold on any device."""
    if not isinstance(data, torch.Tensor):
        raise TypeError(f"{fn}: data is not a tensor")
    _require_dtype(fn, torch.uint8, (("data", data),))
    if data.dim() != 1:
        raise ValueError(f"{fn}: data must be [n], got {tuple(data.shape)}")


def _buffer(fn: str, data: torch.Tensor) -> torch.Tensor:
    _buffer_checks(fn, data)
    _require_device(data, "data")
    data = data.contiguous()
    return data if data.data_ptr() % 16 == 0 else data.clone()          # the kernels load 16 bytes at a time (a fresh tensor is aligned)


def _new_status(dev) -> torch.Tensor:
    return torch.tensor([0, -1, 0, 0], dtype=torch.int64, device=dev)    # bits, first error (an unsigned minimum), slow count, spare


def _row_starts(data: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    n, dev = int(data.numel()), data.device
    block = limits()[2]
    counts = torch.empty((n + block - 1) // block, dtype=torch.int64, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_text_count_rows(_ptr(data), n, _ptr(counts), _ptr(status), _stream()))
        before = torch.cumsum(counts, 0)                                 # set-up: the scan of the block counts
        n_rows = int(before[-1].item()) if n else 0                      # the read-back that sizes `starts`
        before -= counts
        starts = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.ngcf_text_row_starts(_ptr(data), n, _ptr(before), n_rows, _ptr(starts), _ptr(status), _stream()))
    return starts


def row_starts(data: torch.Tensor) -> torch.Tensor:
    """`starts` int64 [n_rows + 1] of the uint8 [n] buffer `data` on the device: the positions where its rows start, ascending, and
    starts[n_rows] = n.  A position starts a row if it is 0 or follows a '\\n' and its line is not blank ('\\n', '\\r\\n', or a '\\r' that
    ends the buffer: pandas' skip_blank_lines); a final line without a newline is a row.  Two passes (ngcf_text_count_rows,
    ngcf_text_row_starts) around a `torch.cumsum` of the per-block counts; one read-back, the row count."""
    data = _buffer("row_starts", data)
    return _row_starts(data, _new_status(data.device))


def _raise_status(fn: str, bits: int, first: int, skip_rows: int, names) -> None:
    if first != -1:
        first &= 2 ** 64 - 1
        row, field, kind = first >> 16, (first >> 8) & 0xff, first & 0xff
        what = TEXT_KINDS.get(kind, f"error kind {kind}")
        if kind == 1:
            raise ValueError(f"{fn}: data row {row}: {what}")
        name = names[field] if names is not None and field < len(names) else field
        raise ValueError(f"{fn}: data row {row}, column {name!r}: {what}")
    if bits & TEXT_LOST:
        raise ValueError(f"{fn}: the row starts do not belong to the buffer (or it changed between two passes)")
    if bits & TEXT_TIER:
        raise RuntimeError(f"{fn}: tier='lds', and a row does not end inside the bytes its workgroup keeps in LDS")
    if bits & TEXT_QUOTE:
        raise ValueError(f"{fn}: a quote in the {skip_rows} leading rows that are not parsed (the header); quoting is not supported")
    raise ValueError(f"{fn}: status bits {bits}")


def _parse(fn: str, data, starts, fields, kinds, n_fields, skip_rows, delim, tier, slow_capacity, status, names):
    """The launch, the one read-back of the status block, the errors and the slow fields' patch.  Returns one tensor per column."""
    lib = _lib.load()
    dev, n, n_rows = data.device, int(data.numel()), int(starts.numel()) - 1
    n_data, n_col = n_rows - skip_rows, len(fields)
    f_slots = [s for s in range(n_col) if kinds[s] == 1]
    ints = {s: torch.empty(n_data, dtype=torch.int64, device=dev) for s in range(n_col) if kinds[s] == 0}
    floats = torch.empty((len(f_slots), n_data), dtype=torch.float64, device=dev)       # one buffer: the slow fields are one indexed write
    cols = [ints[s] if kinds[s] == 0 else floats[f_slots.index(s)] for s in range(n_col)]
    out = (C.c_void_p * n_col)(*[c.data_ptr() for c in cols])
    fa, ka = (C.c_int32 * n_col)(*fields), (C.c_int32 * n_col)(*kinds)
    initial = status.clone()
    capacity = int(slow_capacity)
    while True:
        slow_list = torch.empty(capacity, dtype=torch.int64, device=dev)
        with _on(dev):
            _lib.check(lib.ngcf_text_parse_columns(_ptr(data), n, _ptr(starts), n_rows, skip_rows, n_fields, delim, fa, ka, n_col, out,
                                                   _ptr(slow_list), capacity, tier, _ptr(status), _stream()))
        bits, first, n_slow, _ = status.tolist()                       # the read-back: bits, first error, slow count
        if bits or first != -1:
            _raise_status(fn, bits, first, skip_rows, names)
        if n_slow <= capacity:
            break
        status.copy_(initial)                                           # the list was too short: once more, with one of the reported size
        capacity = n_slow
    if n_slow:
        entries = slow_list[:n_slow]
        rows, slots = entries >> 8, entries & 0xff
        lo = starts[rows + skip_rows]
        lens = starts[rows + skip_rows + 1] - lo
        ends = torch.cumsum(lens, 0)
        where = torch.repeat_interleave(lo - (ends - lens), lens) + torch.arange(int(ends[-1].item()), device=dev)
        blob = data[where].cpu().numpy().tobytes()                      # the bytes of the rows that hold a slow field
        sep, values, at = bytes([delim]), [], 0
        slots_h = slots.tolist()
        for slot, ln in zip(slots_h, lens.tolist()):
            row = blob[at:at + ln].split(b"\n", 1)[0]
            at += ln
            if row.endswith(b"\r"):
                row = row[:-1]
            values.append(float(row.split(sep)[fields[slot]].strip(b" \t").decode("ascii")))
        f_index = torch.tensor([f_slots.index(s) for s in slots_h], dtype=torch.int64, device=dev)
        floats.view(-1)[f_index * n_data + rows] = torch.tensor(values, dtype=torch.float64, device=dev)
    return tuple(cols)


def parse_columns(data: torch.Tensor, starts: torch.Tensor, fields: Sequence[int], kinds: Sequence, *, n_fields: int, skip_rows: int = 0,
                  sep="|", tier: Optional[str] = None, slow_capacity: Optional[int] = None) -> Tuple[torch.Tensor, ...]:
    """Columns out of the rows of `data` (uint8 [n] on the device) that `starts` (`row_starts(data)`) delimits, less the `skip_rows`
    leading ones (the header): column s is field `fields[s]` of the `n_fields` <= 64 fields that `sep` separates in every row, parsed
    as `kinds[s]` - `torch.int64` (or 0) or `torch.float64` (or 1) - for up to 16 columns in any order; the other fields are never
    parsed.  Returns a tuple of int64 / float64 [n_rows - skip_rows] tensors (ngcf_text_parse_columns; the grammar is in
    include/ngcf_hip.h).  Spaces and tabs around a field are skipped.  An int field is [+-]?[0-9]+ inside int64.  A float field is
    a decimal number with an optional exponent; empty, nan, NaN and NA give NaN, [+-]?inf and [+-]?Infinity the infinities.  A number
    of at most 2^53 in its digits and at most 22 in its decimal exponent is one correctly rounded fp64 multiply or divide on the
    device: the bits of Python's `float()`.  Every other number is a slow field: the kernel lists it, and its text is read back,
    parsed with `float(bytes)` and patched in with one indexed write for all of them (a list fuller than `slow_capacity`, default
    4096 entries, is filled by one more parse with a list of the reported size).  The patches are independent of one another, so the
    result does not depend on the order of the list.  `float()` is correctly rounded; where pandas' own parser is an ulp off on such
    a field, this follows Python.  Read-backs: the status block (bits, first error, slow count), and for slow fields the list and
    their rows' bytes.  ValueError names the first offending 0-based data row, the field and the kind: a row with fewer or more than
    `n_fields` fields (pandas pads the first; here both are refused), a byte outside the grammar, an empty int field, an int
    outside int64, a quote.  `tier` is for tests and tools: None lets a workgroup keep its run's bytes in LDS (`limits()`) and walk
    the rows that do not fit from memory, 'memory' walks every row from memory, 'lds' is None and raises where a row was walked
    from memory; the columns do not depend on it."""
    fn = "parse_columns"
    fields, kinds, n_fields = _selection(fn, fields, kinds, n_fields)
    delim = _delimiter(fn, sep)
    if tier not in _TIERS:
        raise ValueError(f"{fn}: tier={tier!r} is neither None, 'lds' nor 'memory'")
    capacity = TEXT_SLOW_CAPACITY if slow_capacity is None else int(slow_capacity)
    if capacity < 0 or int(skip_rows) < 0:
        raise ValueError(f"{fn}: slow_capacity={slow_capacity} or skip_rows={skip_rows} is negative")
    _buffer_checks(fn, data)
    _require_dtype(fn, torch.int64, (("starts", starts),))
    if starts.dim() != 1 or starts.numel() < 1 or int(skip_rows) > int(starts.numel()) - 1:
        raise ValueError(f"{fn}: starts must be [n_rows + 1] with n_rows >= skip_rows = {skip_rows}, got {tuple(starts.shape)}")
    data = _buffer(fn, data)
    _require_same_device(fn, (("starts", starts),), "data", data.device)
    return _parse(fn, data, starts.contiguous(), fields, kinds, n_fields, int(skip_rows), delim, _TIERS[tier], capacity,
                  _new_status(data.device), None)


def _first_row(fn: str, data: torch.Tensor, starts: torch.Tensor) -> bytes:
    """The text of row 0, read back (its bounds, then its bytes)."""
    lo, hi = starts[:2].tolist()
    if hi - lo > TEXT_HEADER_MAX_BYTES + 2:
        raise ValueError(f"{fn}: the first row is longer than {TEXT_HEADER_MAX_BYTES} bytes")
    row = data[lo:hi].cpu().numpy().tobytes().split(b"\n", 1)[0]
    row = row[:-1] if row.endswith(b"\r") else row
    if len(row) > TEXT_HEADER_MAX_BYTES:
        raise ValueError(f"{fn}: the first row is longer than {TEXT_HEADER_MAX_BYTES} bytes")
    return row


def read_table(data: torch.Tensor, columns: Mapping, *, sep="|", header: bool = True) -> Tuple[Dict, int]:
    """`pd.read_csv(io.BytesIO(data), sep=sep, usecols=list(columns), dtype=columns)` for a uint8 [n] buffer on the device:
    `({name: tensor}, n_rows)` with int64 / float64 [n_rows] tensors, in the order of `columns`.  `columns` maps a column's name to
    `torch.int64` or `torch.float64`.  With `header=True` the first row is the header: its bytes (at most 64 KiB, ValueError
    otherwise) are read back, a UTF-8 byte order mark is stripped, and the names between the separators (blanks stripped) give the
    field indices and the field count; a name that is not there is a KeyError, one that is there twice a ValueError, both before
    the parse is launched.  With `header=False` `columns` maps field indices to dtypes and the field count is the first row's.
    Then `row_starts` and `parse_columns`, whose grammar, slow fields and errors these are; an error names the column.  Read-backs:
    the row count, the first row, and one status block (status bits, first error, slow count)."""
    fn = "read_table"
    names_wanted = list(columns)
    kinds = _kinds(fn, [columns[c] for c in names_wanted])
    if not 1 <= len(names_wanted) <= TEXT_MAX_COLUMNS:
        raise ValueError(f"{fn}: {len(names_wanted)} selected columns, outside [1, {TEXT_MAX_COLUMNS}]")
    delim = _delimiter(fn, sep)
    data = _buffer(fn, data)
    status = _new_status(data.device)
    starts = _row_starts(data, status)
    n_rows = int(starts.numel()) - 1
    if n_rows == 0:
        if header:
            raise ValueError(f"{fn}: the buffer has no rows, so no header")
        return {c: torch.empty(0, dtype=torch.int64 if k == 0 else torch.float64, device=data.device) for c, k in zip(names_wanted, kinds)}, 0
    row = _first_row(fn, data, starts)
    if header:
        row = row[len(_BOM):] if row.startswith(_BOM) else row
        names = [f.strip(b" \t").decode("utf-8", "replace") for f in row.split(bytes([delim]))]
        fields = []
        for c in names_wanted:
            if names.count(c) == 0:
                raise KeyError(f"{fn}: no column {c!r} in the header {names}")
            if names.count(c) > 1:
                raise ValueError(f"{fn}: the header has {names.count(c)} columns {c!r}")
            fields.append(names.index(c))
    else:
        names = list(range(row.count(bytes([delim])) + 1))
        for c in names_wanted:
            if not isinstance(c, int) or not 0 <= c < len(names):
                raise KeyError(f"{fn}: no field {c!r} in rows of {len(names)} fields")
        fields = names_wanted
    fields, kinds, n_fields = _selection(fn, fields, kinds, len(names))
    cols = _parse(fn, data, starts, fields, kinds, n_fields, 1 if header else 0, delim, 0, TEXT_SLOW_CAPACITY, status, names)
    return dict(zip(names_wanted, cols)), n_rows - (1 if header else 0)
