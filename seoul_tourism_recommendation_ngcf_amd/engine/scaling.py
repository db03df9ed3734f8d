"""The rating scalers of the reference's Preprocess.scale_implicit on the device: the per-segment quantile floor
(`ngcf_segment_quantile_floor_f64`: csrc/quantile.hip) and the Yeo-Johnson power transform (`ngcf_yeo_johnson_*`:
csrc/yeo_johnson.hip), both in the header's section "full-catalogue ranking and held-out metrics"."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _require_dtype, _require_same_device, _status_word, _stream

# ---- per-segment quantile floor, the core of the reference's Preprocess.scale_implicit (ngcf_segment_quantile_floor_f64, csrc/quantile.hip)
QUANTILE_WAVE_MAX = 64


def segments_from_ids(ids: torch.Tensor, n_rows: int):
    """Group positions by id: `(rowptr int64 [n_rows + 1], order int64 [T])` with segment u = order[rowptr[u] : rowptr[u + 1]], the
    positions t with ids[t] == u in ascending order - the `rowptr` / `order` of `segment_quantile_floor`.  One stable `torch.sort`
    plus `bincount` and `cumsum` on the ids' device (set-up, as `ItemSets.from_pairs`); an id with no position gets an empty
    segment.  An id outside [0, n_rows) raises IndexError."""
    if ids.dim() != 1:
        raise ValueError(f"segments_from_ids: ids must be [T], got {tuple(ids.shape)}")
    _require_dtype("segments_from_ids", torch.int64, (("ids", ids),))
    n_rows = int(n_rows)
    if n_rows < 0:
        raise ValueError(f"segments_from_ids: n_rows={n_rows}")
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_rows):
        raise IndexError(f"segments_from_ids: an id lies outside [0, {n_rows})")
    order = torch.sort(ids, stable=True).indices
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=ids.device)
    if n_rows:
        rowptr[1:] = torch.cumsum(torch.bincount(ids, minlength=n_rows), 0)
    return rowptr, order


def segment_quantile_floor(rowptr: torch.Tensor, x: torch.Tensor, *, order: Optional[torch.Tensor] = None, mean: float = 0.0,
                           scale: float = 1.0, shift: float = 0.0, q: float = 0.25, wave_max: int = 0,
                           out: Optional[torch.Tensor] = None, quant: Optional[torch.Tensor] = None,
                           status: Optional[torch.Tensor] = None):
    """Per segment u = order[rowptr[u] : rowptr[u + 1]] (positions into `x`; `order` None: x is already grouped): the `q` quantile
    of z = ((x - mean) / scale) + shift the way pandas' `quantile(q)` / numpy's `percentile(method="linear")` compute it, and every
    z below it set to 0 (ngcf_segment_quantile_floor_f64; the formulae are in include/ngcf_hip.h).  fp64 throughout, every operation
    rounded once: bit-equal to numpy up to the sign of a zero.  `rowptr` int64 [n_rows + 1], `x` float64 [T], `order` int64 [T] on one
    device.  Returns `(out float64 [T] in the order of x, quant float64 [n_rows])`; the quantile of an empty segment is NaN.  `out`
    may be `x` itself.  `q` is 0.25, 0.5 or 0.75.  `wave_max` (0: the default, 64) moves the switch between the kernel's two tiers
    and never the result.  A NaN in a segment sets status bit 2: the segment's quantile is NaN and its z pass through unfloored.
    A rowptr that decreases or leaves [0, T], or an order entry outside [0, T), sets bit 1 and leaves that segment's `out`
    unwritten: IndexError after one host sync - or, with a caller's int32 `status` word, the bits are only OR-ed into it and the
    call neither syncs nor raises."""
    lib = _lib.load()
    q4 = {0.25: 1, 0.5: 2, 0.75: 3}.get(float(q))
    if q4 is None:
        raise ValueError(f"segment_quantile_floor: q={q} is not one of 0.25, 0.5, 0.75")
    wave_max = int(wave_max)
    if wave_max < 0 or wave_max > QUANTILE_WAVE_MAX:
        raise ValueError(f"segment_quantile_floor: wave_max={wave_max} outside [0, {QUANTILE_WAVE_MAX}]")
    mean, scale, shift = float(mean), float(scale), float(shift)
    if not (0.0 < scale < float("inf")):
        raise ValueError(f"segment_quantile_floor: scale={scale} is not a finite positive number")
    _require_dtype("segment_quantile_floor", torch.int64, (("rowptr", rowptr), ("order", order)))
    _require_dtype("segment_quantile_floor", torch.float64, (("x", x), ("out", out), ("quant", quant)))
    if rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError(f"segment_quantile_floor: rowptr must be [n_rows + 1], got {tuple(rowptr.shape)}")
    if x.dim() != 1:
        raise ValueError(f"segment_quantile_floor: x must be [T], got {tuple(x.shape)}")
    n_rows, T = int(rowptr.numel()) - 1, int(x.numel())
    for t, nm, n, sym in ((order, "order", T, "T"), (out, "out", T, "T"), (quant, "quant", n_rows, "n_rows")):
        if t is not None and (t.dim() != 1 or int(t.numel()) != n):
            raise ValueError(f"segment_quantile_floor: {nm} must be [{sym} = {n}], got {tuple(t.shape)}")
    _require_device(x, "x")
    dev = x.device
    _require_same_device("segment_quantile_floor", (("rowptr", rowptr), ("order", order), ("out", out), ("quant", quant),
                                                    ("status", status)), "x", dev)
    status, check_status = _status_word("segment_quantile_floor", status, dev)
    for t, nm in ((x, "x"), (out, "out"), (quant, "quant")):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"segment_quantile_floor: {nm} must be contiguous")
    rowptr = rowptr.contiguous()
    order = None if order is None else order.contiguous()
    if out is None:
        out = torch.empty(T, dtype=torch.float64, device=dev)
    if quant is None:
        quant = torch.empty(n_rows, dtype=torch.float64, device=dev)
    if T == 0:
        quant.fill_(float("nan"))                  # the library does nothing without values: every segment is empty
    with _on(dev):
        _lib.check(lib.ngcf_segment_quantile_floor_f64(_ptr(rowptr), n_rows, _ptr(order), _ptr(x), T, mean, scale, shift, q4, wave_max,
                                                       _ptr(quant), _ptr(out), _ptr(status), _stream()))
    if check_status and T and n_rows and int(status.item()) & 1:
        raise IndexError(f"segment_quantile_floor: a segment's row pointers or order entries lie outside the {T} values")
    return out, quant


# ---- Yeo-Johnson power transform, the core of the reference's scaler='power' (ngcf_yeo_johnson_*_f64, csrc/yeo_johnson.hip) ----------
def yeo_johnson_launch(T: int):
    """`(blocks, threads, max_blocks)` of the moments kernel's first launch for a column of T rows (a function of T alone, which is
    what makes the reduction reproducible): a grid stride is blocks * threads rows, the workspace one partial per block."""
    blocks, threads, cap = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().ngcf_yeo_johnson_moments_launch(int(T), C.byref(blocks), C.byref(threads), C.byref(cap)))
    return blocks.value, threads.value, cap.value


def _yeo_johnson_args(fn: str, x: torch.Tensor, lam) -> float:
    lam = float(lam)
    if lam != lam:
        raise ValueError(f"{fn}: lam is NaN")
    _require_dtype(fn, torch.float64, (("x", x),))
    if x.dim() != 1:
        raise ValueError(f"{fn}: x must be [T], got {tuple(x.shape)}")
    _require_device(x, "x")
    if not x.is_contiguous():
        raise ValueError(f"{fn}: x must be contiguous")
    return lam


def yeo_johnson(x: torch.Tensor, lam: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """psi(x, lam) elementwise, sklearn's `_yeo_johnson_transform` operation for operation in fp64 (ngcf_yeo_johnson_f64; the
    formulae are in include/ngcf_hip.h): `x` float64 [T] on the device, the result float64 [T].  `out` may be `x` itself.  A NaN
    passes through."""
    lib = _lib.load()
    lam = _yeo_johnson_args("yeo_johnson", x, lam)
    T = int(x.numel())
    if out is None:
        out = torch.empty(T, dtype=torch.float64, device=x.device)
    else:
        _require_dtype("yeo_johnson", torch.float64, (("out", out),))
        if out.dim() != 1 or int(out.numel()) != T:
            raise ValueError(f"yeo_johnson: out must be [T = {T}], got {tuple(out.shape)}")
        _require_same_device("yeo_johnson", (("out", out),), "x", x.device)
        if not out.is_contiguous():
            raise ValueError("yeo_johnson: out must be contiguous")
    with _on(x.device):
        _lib.check(lib.ngcf_yeo_johnson_f64(_ptr(x), T, lam, _ptr(out), _stream()))
    return out


def yeo_johnson_moments(x: torch.Tensor, lam: float) -> torch.Tensor:
    """One evaluation of the likelihood that fits the Yeo-Johnson lambda, in one fused pass over `x` (float64 [T] on the device):
    a float64 [4] tensor on the device holding, over the rows that are not NaN, their count n, the mean of psi(x, lam),
    M2 = sum (psi - mean)^2 and c = sum sign(x) log1p|x| (ngcf_yeo_johnson_moments_f64).  Bit-identical from call to call."""
    lib = _lib.load()
    lam = _yeo_johnson_args("yeo_johnson_moments", x, lam)
    T = int(x.numel())
    result = torch.empty(4, dtype=torch.float64, device=x.device)
    nbytes = int(lib.ngcf_yeo_johnson_workspace_bytes(T))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=x.device)
    with _on(x.device):
        _lib.check(lib.ngcf_yeo_johnson_moments_f64(_ptr(x), T, lam, _ptr(result), _ptr(ws), nbytes, _stream()))
    return result
