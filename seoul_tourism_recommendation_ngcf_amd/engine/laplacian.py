"""Year-slice Laplacians straight into CSR, the reference's Matrix.create_matrix: `ngcf_laplacian_*` (csrc/laplacian.hip; the
header's section "year-slice Laplacians straight into CSR")."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _require_same_device, _stream

LAPLACIAN_LONG_TABLES = 16         # long rows resolved at a time: a table of 2 * n_item words each


def laplacian_limits():
    """`(wave_limit, workgroup_limit)`: the candidate counts (state entries + new records of a user) up to which a row is resolved
    by one wave in registers, and by one workgroup in LDS; longer rows take the table path.  Compiled into the library."""
    wave, group = C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().ngcf_laplacian_limits(C.byref(wave), C.byref(group)))
    return int(wave.value), int(group.value)


def inverse_sqrt_degree(deg: np.ndarray) -> np.ndarray:
    """float32 d^-1/2 with inf -> 0 by the reference's exact call (matrix.py:56): numpy's float32 power is not correctly rounded, so
    the same routine on the same [N, 1] shape is the only way to the same bits.  Host work on an N-sized vector."""
    with np.errstate(divide="ignore"):
        ds = np.power(deg.astype(np.float64)[:, None], -0.5, dtype=np.float32).squeeze(1)
    ds[np.isinf(ds)] = 0.0
    return ds


def empty_laplacian_state(n_user: int, device):
    """The state of R before the first year: `(rowptr int64 [n_user + 1], item int32 [0], rating float32 [0])`."""
    return (torch.zeros(int(n_user) + 1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int32, device=device),
            torch.empty(0, dtype=torch.float32, device=device))


def build_laplacian_year(state, userid: torch.Tensor, itemid: torch.Tensor, rating: torch.Tensor, n_user: int, n_item: int):
    """One year of `matrix.laplacian_slices` on the device (the five steps of include/ngcf_hip.h, ngcf_laplacian_*): `state` is the
    user-sorted CSR of R after the earlier years (`empty_laplacian_state` before the first), `userid` / `itemid` int64 [T] and `rating`
    float32 [T] the year's records in input order, contiguous, on one device.  Returns `(new_state, rowptr int64 [N + 1], colidx
    int32 [nnz], vals float32 [nnz])`: the slice as one [N, N] CSR, user rows then item rows.  Runs on the current stream.  Read back:
    the status word with two row counts that size the launches, the N degrees for the host's d^-1/2, and the count of zero values.
    An id outside [0, n_user) / [0, n_item) raises IndexError; such records are left out of the buckets, never read through."""
    lib = _lib.load()
    rowptr0, item0, rating0 = state
    n_user, n_item = int(n_user), int(n_item)
    for t, nm, dt in ((userid, "userid", torch.int64), (itemid, "itemid", torch.int64), (rating, "rating", torch.float32),
                      (rowptr0, "state rowptr", torch.int64), (item0, "state item", torch.int32), (rating0, "state rating", torch.float32)):
        if t.dtype != dt:
            raise TypeError(f"build_laplacian_year: {nm} must be {dt}, got {t.dtype}")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"build_laplacian_year: {nm} must be a contiguous 1-D tensor")
    T, old_nnz, N = int(userid.numel()), int(item0.numel()), n_user + n_item
    if int(itemid.numel()) != T or int(rating.numel()) != T:
        raise ValueError("build_laplacian_year: userid, itemid and rating differ in length")
    if n_user < 0 or n_item < 0 or int(rowptr0.numel()) != n_user + 1 or int(rating0.numel()) != old_nnz:
        raise ValueError(f"build_laplacian_year: the state does not belong to {n_user} users")
    _require_device(userid, "userid")
    dev = userid.device
    _require_same_device("build_laplacian_year", (("itemid", itemid), ("rating", rating), ("state rowptr", rowptr0),
                                                  ("state item", item0), ("state rating", rating0)), "userid", dev)
    nb = int(lib.ngcf_laplacian_workspace_bytes(n_user, n_item))
    if nb < 0:
        raise ValueError(f"build_laplacian_year: n_user + n_item = {N} does not fit 31 bits")
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)  # noqa: E731
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)
    bptr = torch.empty(n_user + 1, dtype=torch.int64, device=dev)
    count, b_item, b_seq, b_rating, info = i32(n_user), i32(T), i32(T), f32(T), i32(4)
    with _on(dev):
        stream = _stream()
        _lib.check(lib.ngcf_laplacian_bucket(_ptr(userid), _ptr(itemid), _ptr(rating), T, n_user, n_item, _ptr(rowptr0), _ptr(count),
                                             _ptr(bptr), _ptr(b_item), _ptr(b_seq), _ptr(b_rating), _ptr(info), _ptr(ws), nb, stream))
        bad, n_block, n_long, _ = info.tolist()
        if bad:
            raise IndexError(f"build_laplacian_year: a user id lies outside [0, {n_user}) or an item id outside [0, {n_item})")
        n_tables = min(n_long, LAPLACIAN_LONG_TABLES)
        tables = i32(n_tables * 2 * n_item) if n_tables else None
        t_item, t_rating, deg = i32(old_nnz + T), f32(old_nnz + T), i32(N)
        rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
        words = torch.zeros(2, dtype=torch.int64, device=dev)              # [0]: zero values of the slice, [1]: status
        status = words[1:].view(torch.int32)
        _lib.check(lib.ngcf_laplacian_resolve(_ptr(rowptr0), _ptr(item0), _ptr(rating0), old_nnz, _ptr(bptr), _ptr(b_item), _ptr(b_seq),
                                              _ptr(b_rating), T, n_user, n_item, n_block, n_long, _ptr(t_item), _ptr(t_rating), _ptr(deg),
                                              _ptr(rowptr), _ptr(tables), n_tables, _ptr(status), _ptr(ws), nb, stream))
        deg_host = deg.cpu().numpy()                                        # the year's one N-sized read-back
        nnz = int(deg_host[:n_user].sum(dtype=np.int64))
        ds = torch.from_numpy(inverse_sqrt_degree(deg_host)).to(dev)
        s_item, s_rating, s_user, vals_item = i32(nnz), f32(nnz), i32(nnz), f32(nnz)
        colidx, vals = i32(2 * nnz), f32(2 * nnz)
        _lib.check(lib.ngcf_laplacian_emit(_ptr(rowptr0), _ptr(item0), _ptr(rating0), old_nnz, _ptr(bptr), T, _ptr(t_item), _ptr(t_rating),
                                           n_user, n_item, _ptr(deg), _ptr(rowptr), _ptr(ds), nnz, _ptr(s_item), _ptr(s_rating), _ptr(s_user),
                                           _ptr(colidx), _ptr(vals), _ptr(vals_item), _ptr(words), _ptr(status), stream))
        del t_item, t_rating, b_item, b_seq, b_rating
        order = torch.sort(s_item, stable=True).indices                     # item rows by (item, user): one library sort of 32-bit keys
        _lib.check(lib.ngcf_laplacian_item_rows(_ptr(order), _ptr(s_user), _ptr(vals_item), nnz, _ptr(colidx[nnz:]), _ptr(vals[nnz:]),
                                                _ptr(status), stream))
        zeros, st = words.tolist()
        if st & 0xffffffff:
            raise RuntimeError(f"build_laplacian_year: the state handed in is not a CSR of {n_user} users over {n_item} items "
                               f"(status {st & 0xffffffff})")
        if zeros:                                                           # values that underflow to 0 leave the slice, not the state
            out_rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
            out_colidx, out_vals = i32(2 * nnz - zeros), f32(2 * nnz - zeros)
            _lib.check(lib.ngcf_laplacian_drop_zeros(_ptr(rowptr), _ptr(colidx), _ptr(vals), N, 2 * nnz, _ptr(deg), _ptr(out_rowptr),
                                                     _ptr(out_colidx), _ptr(out_vals), 2 * nnz - zeros, _ptr(ws), nb, stream))
            return (rowptr[:n_user + 1], s_item, s_rating), out_rowptr, out_colidx, out_vals
    return (rowptr[:n_user + 1], s_item, s_rating), rowptr, colidx, vals
