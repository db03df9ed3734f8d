"""Group-by-sum on packed integer keys and the decimal string code, the reference's pivot_table and id maps: `ngcf_groupby_*`,
`ngcf_decimal_code` (csrc/groupby.hip; the header's section "group-by-sum on packed integer keys, and the decimal string code")."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _stream

GROUPBY_MAX_KEYS, GROUPBY_MAX_VALUES = 8, 4
GROUPBY_FULL, GROUPBY_RANGE, GROUPBY_LOST = 1, 2, 4
GROUPBY_MIN_CAPACITY = 64
GROUPBY_LDS_SLOTS = 1024           # the default `lds_slots`; profiles/groupby_lab.txt records the run that sets it (none yet)
DECIMAL_MAX_CHARS = 18


class _GroupbyCols(C.Structure):
    """ngcf_groupby_cols_t of include/ngcf_hip.h."""
    _fields_ = [("n_keys", C.c_int32), ("n_values", C.c_int32), ("key", C.c_void_p * GROUPBY_MAX_KEYS),
                ("value", C.c_void_p * GROUPBY_MAX_VALUES), ("key_offset", C.c_int64 * GROUPBY_MAX_KEYS),
                ("key_range", C.c_uint64 * GROUPBY_MAX_KEYS), ("key_is64", C.c_int32 * GROUPBY_MAX_KEYS),
                ("key_bits", C.c_int32 * GROUPBY_MAX_KEYS), ("key_shift", C.c_int32 * GROUPBY_MAX_KEYS),
                ("value_is64", C.c_int32 * GROUPBY_MAX_VALUES)]


class Groups(NamedTuple):
    """`group_by`'s result: `keys` K int64 [G] columns in ascending (column 0, column 1, ...) order, `sums` V int64 [G] columns,
    `inverse` int64 [T] (row t belongs to group inverse[t]) or None."""
    keys: Tuple[torch.Tensor, ...]
    sums: Tuple[torch.Tensor, ...]
    inverse: Optional[torch.Tensor]


def groupby_limits():
    """`(chunk_rows, lds_probes, max_lds_slots)` of the insert kernel: the rows a workgroup takes per pass, the probes a row gets in
    the workgroup's LDS table before it goes to memory, and the largest `lds_slots`.  Compiled into the library."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().ngcf_groupby_limits(C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def groupby_hash(key: int) -> int:
    """The hash of a packed key (fmix64, the 64-bit finaliser of MurmurHash3): its home slot is `hash & (capacity - 1)`, its slot
    in a workgroup's LDS table `(hash >> 32) & (lds_slots - 1)`.  Host call."""
    return int(_lib.load().ngcf_groupby_hash(int(key) & (2 ** 64 - 1)))


def groupby_packing(bounds: Sequence[Tuple[int, int]]):
    """`(offsets, ranges, bits, shifts)` of key columns with the given (min, max): a field of bit_length(max - min) bits per column
    (none for a single-valued one), column 0 most significant.  More than 63 bits in all: ValueError (the all-ones word must stay
    free to mean an empty slot)."""
    offsets = [int(lo) for lo, _ in bounds]
    ranges = [int(hi) - int(lo) for lo, hi in bounds]
    if any(r < 0 for r in ranges):
        raise ValueError(f"group_by: bounds {list(bounds)}: a maximum below its minimum")
    bits = [r.bit_length() for r in ranges]
    if sum(bits) > 63:
        raise ValueError(f"group_by: the columns need {' + '.join(map(str, bits))} = {sum(bits)} bits, and a packed key has 63")
    shifts = [sum(bits[k + 1:]) for k in range(len(bits))]
    return offsets, ranges, bits, shifts


_NO_FLOAT_SUMS = ("only integer columns are summed here: pandas' float group sum is compensated and takes a group's rows in row order "
                  "(engine.context.group_sum_float does), and floating-point atomics would make the result depend on arrival order")


def _int_columns(fn: str, groups):
    """Types and shapes of every column first (they hold on any device), then where the columns live.  `groups`: (what, columns)
    pairs; returns the columns of each, contiguous."""
    T = None
    for what, cols in groups:
        for k, c in enumerate(cols):
            if not isinstance(c, torch.Tensor):
                raise TypeError(f"{fn}: {what} {k} is not a tensor")
            if c.dtype.is_floating_point and what == "value column":
                raise TypeError(f"{fn}: {what} {k} is {c.dtype}; {_NO_FLOAT_SUMS}")
            if c.dtype not in (torch.int32, torch.int64):
                raise TypeError(f"{fn}: {what} {k} must be int32 or int64, got {c.dtype}")
            if c.dim() != 1:
                raise ValueError(f"{fn}: {what} {k} must be [T], got {tuple(c.shape)}")
            if T is not None and int(c.numel()) != T:
                raise ValueError(f"{fn}: {what} {k} has {int(c.numel())} rows, {groups[0][0]} 0 has {T}")
            T = int(c.numel())
    dev = None
    for what, cols in groups:
        for k, c in enumerate(cols):
            _require_device(c, f"{fn}: {what} {k}")
            if dev is not None and c.device != dev:
                raise RuntimeError(f"{fn}: {what} {k} is on {c.device}, {groups[0][0]} 0 on {dev}")
            dev = c.device
    return [[c.contiguous() for c in cols] for _, cols in groups]


def group_by(columns: Sequence[torch.Tensor], values: Sequence[torch.Tensor] = (), *, inverse: bool = False,
             capacity: Optional[int] = None, lds_slots: Optional[int] = None,
             bounds: Optional[Sequence[Tuple[int, int]]] = None) -> Groups:
    """Group the T rows of `columns` (K <= 8 int32 / int64 [T] tensors on one device) by their values and sum `values` (V <= 4
    int32 / int64 [T]) per group: `pd.pivot_table(index=columns, aggfunc='sum').reset_index()`, or `np.unique(axis=0,
    return_inverse=True)` plus `np.add.at` (ngcf_groupby_*; the steps are in include/ngcf_hip.h).  Returns `Groups(keys, sums,
    inverse)`: the G distinct key rows ascending by (column 0, column 1, ...) as K int64 [G] tensors, the V int64 [G] sums (exact,
    modulo 2^64), and with `inverse=True` the int64 [T] group index of every row.  Integer atomics only: the same call returns the
    same tensors.  Floating value columns are a TypeError (`context.group_sum_float` sums them).  The columns' (min, max) are read back once to pack the keys into
    <= 63 bits (more: ValueError), or taken from `bounds` (K pairs; a value outside them: ValueError); G and the status word are the
    other read-back.  `capacity` (a power of two; default: the power of two >= 2 x min(T, product of the ranges), which cannot
    overflow) is doubled and the call run again while the table turns out too small; `lds_slots` (0: off; a power of two up to
    `groupby_limits()[2]`; default GROUPBY_LDS_SLOTS) sizes the per-workgroup LDS table and never changes the result."""
    lib = _lib.load()
    fn = "group_by"
    columns, values = list(columns), list(values)
    if not 1 <= len(columns) <= GROUPBY_MAX_KEYS:
        raise ValueError(f"{fn}: {len(columns)} key columns, outside [1, {GROUPBY_MAX_KEYS}]")
    if len(values) > GROUPBY_MAX_VALUES:
        raise ValueError(f"{fn}: {len(values)} value columns, more than {GROUPBY_MAX_VALUES}")
    if capacity is not None:
        capacity = int(capacity)
        if capacity < 1 or capacity & (capacity - 1) or capacity > 2 ** 36:
            raise ValueError(f"{fn}: capacity={capacity} is not a power of two in [1, 2^36]")
    lds_slots = GROUPBY_LDS_SLOTS if lds_slots is None else int(lds_slots)
    if lds_slots != 0 and (lds_slots < 16 or lds_slots & (lds_slots - 1) or lds_slots > 2048):
        raise ValueError(f"{fn}: lds_slots={lds_slots} is neither 0 nor a power of two in [16, 2048]")
    K, V = len(columns), len(values)
    if bounds is not None and len(bounds) != K:
        raise ValueError(f"{fn}: {len(bounds)} bounds for {K} columns")
    columns, values = _int_columns(fn, (("key column", columns), ("value column", values)))
    T, dev = int(columns[0].numel()), columns[0].device
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)  # noqa: E731
    if T == 0:
        return Groups(tuple(i64(0) for _ in range(K)), tuple(i64(0) for _ in range(V)), i64(0) if inverse else None)
    if bounds is None:                                                     # read-back 1: the K (min, max) pairs
        mm = torch.stack([f(c).to(torch.int64) for c in columns for f in (torch.min, torch.max)]).tolist()
        bounds = [(mm[2 * k], mm[2 * k + 1]) for k in range(K)]
    offsets, ranges, bits, shifts = groupby_packing(bounds)
    cols = _GroupbyCols()
    cols.n_keys, cols.n_values = K, V
    for k, c in enumerate(columns):
        cols.key[k], cols.key_is64[k] = c.data_ptr(), int(c.dtype == torch.int64)
        cols.key_offset[k], cols.key_range[k], cols.key_bits[k], cols.key_shift[k] = offsets[k], ranges[k], bits[k], shifts[k]
    for v, c in enumerate(values):
        cols.value[v], cols.value_is64[v] = c.data_ptr(), int(c.dtype == torch.int64)
    if capacity is None:
        prod = 1
        for r in ranges:
            prod = min(prod * (r + 1), T)                                  # min(T, product of the ranges): the most groups there can be
        capacity = max(GROUPBY_MIN_CAPACITY, 1 << (2 * prod - 1).bit_length())
    with _on(dev):
        stream = _stream()
        while True:
            table_keys, table_sums = i64(capacity), i64(max(V * capacity, 1))
            words = torch.zeros(2, dtype=torch.int64, device=dev)          # [0]: G, [1]: the status word
            status = words[1:].view(torch.int32)                           # its first int32 is the word
            nb = int(lib.ngcf_groupby_workspace_bytes(capacity))
            ws = i64(max(nb // 8, 1))
            _lib.check(lib.ngcf_groupby_insert(C.byref(cols), T, _ptr(table_keys), _ptr(table_sums), capacity, lds_slots, _ptr(status), stream))
            _lib.check(lib.ngcf_groupby_count(_ptr(table_keys), capacity, _ptr(words), _ptr(ws), nb, stream))
            G, st = words.tolist()                                         # read-back 2: G and the status word
            st &= 0xffffffff
            if st & GROUPBY_RANGE:
                raise ValueError(f"{fn}: a value lies outside the bounds {list(bounds)} its column was packed with")
            if not st & GROUPBY_FULL:
                break
            if capacity >= 2 ** 36:
                raise RuntimeError(f"{fn}: the groups do not fit a table of 2^36 slots")
            del table_keys, table_sums
            capacity *= 2
        keys_g, slots_g = i64(G), i64(G)
        _lib.check(lib.ngcf_groupby_compact(_ptr(table_keys), capacity, G, _ptr(keys_g), _ptr(slots_g), _ptr(ws), nb, _ptr(status), stream))
        sorted_keys, order = torch.sort(keys_g)                            # packed keys are below 2^63: the signed order is theirs
        key_out, sum_out = [i64(G) for _ in range(K)], [i64(G) for _ in range(V)]
        rank = i64(capacity) if inverse else None
        kp = (C.c_void_p * GROUPBY_MAX_KEYS)(*[t.data_ptr() for t in key_out])
        sp = (C.c_void_p * GROUPBY_MAX_VALUES)(*[t.data_ptr() for t in sum_out])
        _lib.check(lib.ngcf_groupby_unpack(C.byref(cols), _ptr(sorted_keys), _ptr(order), _ptr(slots_g), _ptr(table_sums), capacity, G, kp, sp,
                                           _ptr(rank), _ptr(status), stream))
        inv = None
        if inverse:
            inv = i64(T)
            _lib.check(lib.ngcf_groupby_lookup(C.byref(cols), T, _ptr(table_keys), _ptr(rank), capacity, _ptr(inv), _ptr(status), stream))
        st = int(status[0].item())                                         # the status word once more, after the last kernel
    if st:
        raise RuntimeError(f"{fn}: the columns changed while the call ran (status {st})")
    return Groups(tuple(key_out), tuple(sum_out), inv)


def decimal_code(columns: Sequence[torch.Tensor], widths: Sequence[int]) -> torch.Tensor:
    """One int64 [T] column whose numeric order is the lexicographic order of the strings `str(col0) + str(col1) + ...` (up to 8
    non-negative int32 / int64 [T] columns on one device; ngcf_decimal_code).  `widths[k] = 0`: the value's natural decimal length;
    `w > 0`: zero-padded on the left to w characters.  Every character '0' + d is the base-11 digit d + 1 of a left-aligned number
    of 18 places, padding 0 (11^18 < 2^63); `decimal_string` is the way back.  ValueError for a negative value, a value with more
    digits than its fixed width, and a string of more than 18 characters (one read-back of the status word)."""
    lib = _lib.load()
    fn = "decimal_code"
    columns, widths = list(columns), [int(w) for w in widths]
    if not 1 <= len(columns) <= GROUPBY_MAX_KEYS:
        raise ValueError(f"{fn}: {len(columns)} columns, outside [1, {GROUPBY_MAX_KEYS}]")
    if len(widths) != len(columns):
        raise ValueError(f"{fn}: {len(widths)} widths for {len(columns)} columns")
    if any(w < 0 or w > DECIMAL_MAX_CHARS for w in widths):
        raise ValueError(f"{fn}: widths {widths} outside [0, {DECIMAL_MAX_CHARS}]")
    if sum(max(w, 1) for w in widths) > DECIMAL_MAX_CHARS:
        raise ValueError(f"{fn}: widths {widths} make more than {DECIMAL_MAX_CHARS} characters")
    columns, = _int_columns(fn, (("column", columns),))
    n, T, dev = len(columns), int(columns[0].numel()), columns[0].device
    out = torch.empty(T, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * n)(*[c.data_ptr() for c in columns])
    is64 = (C.c_int32 * n)(*[int(c.dtype == torch.int64) for c in columns])
    wd = (C.c_int32 * n)(*widths)
    with _on(dev):
        _lib.check(lib.ngcf_decimal_code(ptrs, is64, wd, n, T, _ptr(out), _ptr(status), _stream()))
    st = int(status.item()) if T else 0
    if st & 1:
        raise ValueError(f"{fn}: a column holds a negative value")
    if st & 2:
        raise ValueError(f"{fn}: a value has more digits than its fixed width (widths {widths})")
    if st & 4:
        raise ValueError(f"{fn}: a row's string has more than {DECIMAL_MAX_CHARS} characters")
    return out


def decimal_string(code: int) -> str:
    """The string behind one `decimal_code` value (host, for the few distinct keys of a dictionary)."""
    code, chars = int(code), []
    if code < 0 or code >= 11 ** DECIMAL_MAX_CHARS:
        raise ValueError(f"decimal_string: {code} is not a code")
    for _ in range(DECIMAL_MAX_CHARS):
        code, d = divmod(code, 11)
        chars.append(d)
    chars.reverse()                                                        # most significant place first
    n = len(chars)
    while n and chars[n - 1] == 0:
        n -= 1
    if any(d == 0 for d in chars[:n]):
        raise ValueError("decimal_string: padding inside the string: not a code")
    return "".join(chr(ord("0") + d - 1) for d in chars[:n])
