"""Trip context of a recommendation request: the float group sum of the reference's congestion pivot and the table of distances
between departure points and destinations: `ngcf_segment_kahan_sum_f64`, `ngcf_haversine_table_f64` (csrc/context.hip; the header's
section "trip context").  Reached as `engine.context.<name>`."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _require_dtype, _require_same_device, _stream
from .groupby import GROUPBY_MAX_VALUES, Groups, group_by
from .scaling import segments_from_ids

KAHAN_MAX_VALUES = GROUPBY_MAX_VALUES


def _value_columns(fn: str, values) -> list:
    """1-4 float64 [T] columns: types and shapes, which hold on any device."""
    values = [values] if isinstance(values, torch.Tensor) else list(values)
    if not 1 <= len(values) <= KAHAN_MAX_VALUES:
        raise ValueError(f"{fn}: {len(values)} value columns, outside [1, {KAHAN_MAX_VALUES}]")
    for k, v in enumerate(values):
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"{fn}: value column {k} is not a tensor")
    _require_dtype(fn, torch.float64, [(f"value column {k}", v) for k, v in enumerate(values)])
    for k, v in enumerate(values):
        if v.dim() != 1:
            raise ValueError(f"{fn}: value column {k} must be [T], got {tuple(v.shape)}")
        if int(v.numel()) != int(values[0].numel()):
            raise ValueError(f"{fn}: value column {k} has {int(v.numel())} rows, value column 0 has {int(values[0].numel())}")
    return values


def _wave_min(fn: str, wave_min) -> int:
    wave_min = int(wave_min)
    if wave_min < 0 or wave_min >= 2 ** 31:
        raise ValueError(f"{fn}: wave_min={wave_min} outside [0, 2^31)")
    return wave_min


def segment_kahan_sum(rowptr: torch.Tensor, values, *, order: Optional[torch.Tensor] = None,
                      wave_min: int = 0) -> Tuple[torch.Tensor, ...]:
    """Per segment u = order[rowptr[u] : rowptr[u + 1]] (positions into the value columns; `order` None: the rows are already
    grouped) the compensated sum of every column the way pandas' `groupby().sum()` / `pivot_table(aggfunc='sum')` computes it: the
    Kahan recurrence in ascending position order, NaNs skipped (ngcf_segment_kahan_sum_f64; the recurrence is in
    include/ngcf_hip.h).  Bit-equal to pandas when a segment's positions are in row order.  `rowptr` int64 [n_rows + 1], `values`
    one float64 [T] tensor or a sequence of up to four, `order` int64 [T], all on one device.  Returns a tuple of float64 [n_rows],
    one per column; an empty or all-NaN segment sums to 0.0.  `wave_min` (0: the library's default) is the segment length from
    which a wave instead of a lane takes a segment; it never changes the result, and neither does the run: no float atomics.
    A rowptr that decreases or leaves [0, T], or an order entry outside [0, T), is never read through: IndexError after one host
    sync."""
    lib = _lib.load()
    fn = "segment_kahan_sum"
    values = _value_columns(fn, values)
    wave_min = _wave_min(fn, wave_min)
    _require_dtype(fn, torch.int64, (("rowptr", rowptr), ("order", order)))
    if rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError(f"{fn}: rowptr must be [n_rows + 1], got {tuple(rowptr.shape)}")
    n_rows, T, V = int(rowptr.numel()) - 1, int(values[0].numel()), len(values)
    if order is not None and (order.dim() != 1 or int(order.numel()) != T):
        raise ValueError(f"{fn}: order must be [T = {T}], got {tuple(order.shape)}")
    _require_device(values[0], "value column 0")
    dev = values[0].device
    _require_same_device(fn, [(f"value column {k}", v) for k, v in enumerate(values)] + [("rowptr", rowptr), ("order", order)],
                         "value column 0", dev)
    values = [v.contiguous() for v in values]
    rowptr = rowptr.contiguous()
    order = None if order is None else order.contiguous()
    sums = tuple(torch.empty(n_rows, dtype=torch.float64, device=dev) for _ in range(V))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    vp = (C.c_void_p * V)(*[v.data_ptr() for v in values])
    sp = (C.c_void_p * V)(*[s.data_ptr() for s in sums])
    with _on(dev):
        _lib.check(lib.ngcf_segment_kahan_sum_f64(_ptr(rowptr), n_rows, _ptr(order), vp, V, T, wave_min, sp, _ptr(status), _stream()))
    if n_rows and int(status.item()) & 1:
        raise IndexError(f"{fn}: a segment's row pointers or order entries lie outside the {T} rows")
    return sums


def group_sum_float(columns: Sequence[torch.Tensor], values, *, bounds: Optional[Sequence[Tuple[int, int]]] = None,
                    wave_min: int = 0) -> Groups:
    """`group_by` for float64 value columns: `pd.pivot_table(index=columns, aggfunc='sum').reset_index()` with pandas' bits.
    `group_by(columns, inverse=True)` finds the keys and every row's group, `segments_from_ids` the rows of every group in row
    order (a stable sort), `segment_kahan_sum` adds them in that order.  `columns`, `bounds` as for `group_by`; `values` one
    float64 [T] tensor or up to four; `wave_min` as for `segment_kahan_sum`.  Returns `Groups(keys, sums, inverse)` with float64
    sums; a group whose values are all NaN sums to 0.0, as in pandas."""
    fn = "group_sum_float"
    values = _value_columns(fn, values)
    wave_min = _wave_min(fn, wave_min)
    columns = list(columns)
    if columns and isinstance(columns[0], torch.Tensor) and columns[0].dim() == 1 and int(columns[0].numel()) != int(values[0].numel()):
        raise ValueError(f"{fn}: value column 0 has {int(values[0].numel())} rows, key column 0 has {int(columns[0].numel())}")
    groups = group_by(columns, inverse=True, bounds=bounds)
    _require_same_device(fn, [(f"value column {k}", v) for k, v in enumerate(values)], "key column 0", groups.inverse.device)
    rowptr, order = segments_from_ids(groups.inverse, int(groups.keys[0].numel()))
    return Groups(groups.keys, segment_kahan_sum(rowptr, values, order=order, wave_min=wave_min), groups.inverse)


def haversine_table(dep: torch.Tensor, item: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[s, i] = the great-circle distance in metres between departure point s and item i: `haversine(dep[s], item[i]) * 1000` of
    the `haversine` package, operation for operation in fp64 (ngcf_haversine_table_f64; the formula is in include/ngcf_hip.h).
    `dep` float64 [S, 2], `item` float64 [n_item, 2] in degrees on one device, the first coordinate taken as the latitude - as the
    package does with the tuples the reference hands it.  Returns float64 [S, n_item] (`out`, if given, contiguous).  A NaN
    coordinate gives +inf: "missing, sorts last" to `recommend.blended_ranking`."""
    lib = _lib.load()
    fn = "haversine_table"
    _require_dtype(fn, torch.float64, (("dep", dep), ("item", item), ("out", out)))
    for nm, t in (("dep", dep), ("item", item)):
        if t.dim() != 2 or int(t.shape[1]) != 2:
            raise ValueError(f"{fn}: {nm} must be [n, 2], got {tuple(t.shape)}")
    S, n_item = int(dep.shape[0]), int(item.shape[0])
    if out is not None and tuple(out.shape) != (S, n_item):
        raise ValueError(f"{fn}: out must be [S = {S}, n_item = {n_item}], got {tuple(out.shape)}")
    _require_device(dep, "dep")
    _require_same_device(fn, (("item", item), ("out", out)), "dep", dep.device)
    if out is None:
        out = torch.empty((S, n_item), dtype=torch.float64, device=dep.device)
    elif not out.is_contiguous():
        raise ValueError(f"{fn}: out must be contiguous")
    dep, item = dep.contiguous(), item.contiguous()
    with _on(dep.device):
        _lib.check(lib.ngcf_haversine_table_f64(_ptr(dep), S, _ptr(item), n_item, _ptr(out), _stream()))
    return out
