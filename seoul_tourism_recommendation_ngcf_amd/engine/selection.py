"""Exact draws on the device: unseen items per case (`ngcf_sample_unseen`: csrc/sample.hip; in the header's section
"full-catalogue ranking and held-out metrics") and rows per group (`ngcf_select_*`: csrc/select.hip; "exact per-group sampling")."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _require_dtype, _require_same_device, _row_major_ld, _status_word, _stream
from .ranking import ItemSets, _check_sets

# ---- unseen items per case, the reference's TourDataset._negative_sampling (ngcf_sample_unseen, csrc/sample.hip) -------------------
SAMPLE_M_MAX = 1023


def sample_unseen(seen: ItemSets, user_ids: torch.Tensor, m: int, seed: int, *, first: Optional[torch.Tensor] = None,
                  case_offset: int = 0, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`m` items per case that the case's user has no entry for in `seen`, uniform and without replacement (ngcf_sample_unseen):
    case t of user `user_ids[t]` (int64 [T] on the sets' device) is a pure function of (seed, case_offset + t, the user's seen row)
    - the draw is written out in include/ngcf_hip.h, so a case set drawn in chunks with `case_offset` equals the set drawn at
    once.  This is the distribution of the reference's `np.random.choice(neg_items, ng_ratio, replace=False)` (utils.py:262), not
    numpy's stream: the same seed does not give the reference's items.  Returns int64 [T, m], or [T, m + 1] with `first` (int64 [T],
    e.g. the held-out items) in column 0 - then the `candidates` of `eval_candidates`.  `out`: an int64 row-major tensor of T rows
    and at least that many columns to write into (the returned tensor is a view of its leading columns).  `seen` comes from
    `ItemSets.from_pairs` or `ItemSets.from_laplacian`.  A user id outside the sets raises IndexError, a user with fewer than `m`
    unseen items ValueError (np.random.choice raises there), after one host sync; the drawn slots of such a case are -1.  With a
    caller's int32 `status` word the bits (1, 2) are only OR-ed into it and the call neither syncs nor raises."""
    lib = _lib.load()
    m, seed = int(m), int(seed) & 0xFFFFFFFFFFFFFFFF
    if m < 1 or m > SAMPLE_M_MAX:
        raise ValueError(f"sample_unseen: m={m} outside [1, {SAMPLE_M_MAX}]")
    if seen.n_items < 1 or seen.n_items >= 2 ** 31:
        raise ValueError(f"sample_unseen: n_items={seen.n_items} outside [1, 2^31)")
    _require_dtype("sample_unseen", torch.int64, (("user_ids", user_ids), ("first", first), ("out", out)))
    if user_ids.dim() != 1:
        raise ValueError(f"sample_unseen: user_ids must be [T], got {tuple(user_ids.shape)}")
    T = int(user_ids.numel())
    if first is not None and (first.dim() != 1 or int(first.numel()) != T):
        raise ValueError(f"sample_unseen: first must be [T = {T}], got {tuple(first.shape)}")
    width = m + (first is not None)
    if out is not None and (out.dim() != 2 or int(out.shape[0]) != T or int(out.shape[1]) < width):
        raise ValueError(f"sample_unseen: out must be [T = {T}, >= {width}], got {tuple(out.shape)}")
    _require_device(seen.rowptr, "the item sets")
    dev = seen.rowptr.device
    _check_sets(seen, dev, 0, "sample_unseen")
    if seen.rowptr.dtype != torch.int64 or seen.colidx.dtype != torch.int32:
        raise TypeError("sample_unseen: the item sets must be int64 row pointers and int32 columns")
    _require_same_device("sample_unseen", (("user_ids", user_ids), ("first", first), ("out", out), ("status", status)),
                         "the item sets", dev)
    status, check_status = _status_word("sample_unseen", status, dev)
    user_ids = user_ids.contiguous()
    first = None if first is None else first.contiguous()
    if out is None:
        out = torch.empty((T, width), dtype=torch.int64, device=dev)
    ld_out = _row_major_ld(out, "out")
    # a set without entries has no column array to point at; its row pointers are all 0 and nothing is read through it
    colidx = seen.colidx if seen.colidx.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_sample_unseen(_ptr(seen.rowptr), _ptr(colidx), seen.col_offset, seen.n_rows, seen.n_items, _ptr(user_ids), T,
                                          int(case_offset), m, seed, _ptr(first), _ptr(out), ld_out, _ptr(status), _stream()))
    if check_status and T:
        bits = int(status.item())
        if bits & 1:
            raise IndexError(f"sample_unseen: a user id lies outside [0, {seen.n_rows})")
        if bits & 2:
            raise ValueError(f"sample_unseen: a user has fewer than m={m} unseen items among {seen.n_items}")
    return out[:, :width]


# ---- exact per-group sampling, the core of the reference's Preprocess.split_train_test (ngcf_select_per_group, csrc/select.hip) ------
SELECT_GROUP, SELECT_QUOTA, SELECT_LOST = 1, 2, 4          # the status bits of include/ngcf_hip.h
SELECT_GOLDEN = 0x9E3779B97F4A7C15


def select_limits(n_groups: int = 1):
    """`(lds_groups, workspace_bytes)`: the largest group count whose G x 256 table of counts a workgroup keeps in LDS (above it
    the rows count straight into memory), and the bytes of workspace a call with `n_groups` groups takes - 1 KiB + 16 B per group
    in both tiers (-1 for a count outside [1, 2^31)).  Compiled into the library."""
    a, b = C.c_int(0), C.c_int64(0)
    _lib.check(_lib.load().ngcf_select_limits(int(n_groups), C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def select_key(seed: int, t: int) -> int:
    """The key of row t, fmix(seed ^ (t * 0x9E3779B97F4A7C15)) in unsigned 64-bit arithmetic, as the library computes it.  Host call."""
    return int(_lib.load().ngcf_select_key(int(seed) & (2 ** 64 - 1), int(t)))


def select_per_group(group: Optional[torch.Tensor], quota, *, seed: int, n_rows: Optional[int] = None, return_thresholds: bool = False,
                     out: Optional[torch.Tensor] = None, device=None):
    """Mark exactly `quota[g]` rows of every group g, uniformly among all subsets of that size (ngcf_select_per_group; the keys and
    the rule are written out in include/ngcf_hip.h): row t of group g is marked iff its key is among the quota[g] smallest of the
    group.  `group`: int32 [T] on the device, ids in [0, G), in any order - or None for one group of `n_rows` rows (on `device`,
    default the current one).  `quota`: G integers (a sequence, an array or a tensor; it is checked on the host and uploaded).
    Returns the uint8 [T] mask (0 / 1), a pure function of (seed, group, quota) - or `(mask, thresholds)` with `return_thresholds`:
    int64 [G] holding the bits of the unsigned 64-bit tau_g, 0 for a group with nothing marked.  `out`: a contiguous uint8 [T] tensor
    to write the mask into.  A negative quota is a ValueError before anything runs.  One status read-back at the end: a group id
    outside [0, G) raises IndexError (and the mask, which `out` still shows, is all 0), a quota above its group's row count
    ValueError (np.random.choice and pandas' sample raise there; no row of that group is marked).  This is the reference's
    distribution, not numpy's or pandas' stream: the same seed does not give the reference's rows."""
    lib = _lib.load()
    fn = "select_per_group"
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if group is not None:
        if not isinstance(group, torch.Tensor) or group.dtype != torch.int32:
            raise TypeError(f"{fn}: group must be an int32 tensor, got {getattr(group, 'dtype', type(group))}")
        if group.dim() != 1:
            raise ValueError(f"{fn}: group must be [T], got {tuple(group.shape)}")
        if n_rows is not None and int(n_rows) != int(group.numel()):
            raise ValueError(f"{fn}: n_rows={n_rows} beside a group vector of {int(group.numel())} rows")
        T = int(group.numel())
    else:
        if n_rows is None:
            raise ValueError(f"{fn}: without a group vector n_rows says how many rows there are")
        T = int(n_rows)
    if T < 0 or T >= 2 ** 31:
        raise ValueError(f"{fn}: {T} rows, outside [0, 2^31)")
    q = quota.detach().cpu() if isinstance(quota, torch.Tensor) else torch.as_tensor(np.asarray(quota))
    if q.dim() != 1 or q.numel() < 1:
        raise ValueError(f"{fn}: quota must be [G >= 1], got {tuple(q.shape)}")
    if q.dtype.is_floating_point or q.dtype == torch.bool:
        raise TypeError(f"{fn}: quota must hold integers, got {q.dtype}")
    q = q.to(torch.int64).contiguous()
    G = int(q.numel())
    if group is None and G != 1:
        raise ValueError(f"{fn}: no group vector stands for one group, quota has {G} entries")
    if bool((q < 0).any()):
        raise ValueError(f"{fn}: a quota is negative")
    if out is not None and (out.dtype != torch.uint8 or out.dim() != 1 or int(out.numel()) != T or not out.is_contiguous()):
        raise ValueError(f"{fn}: out must be a contiguous uint8 [T = {T}] tensor")
    if group is not None:
        _require_device(group, "group")
        dev = group.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"{fn}: device '{dev}': the selection runs on a ROCm device only")
    _require_same_device(fn, (("out", out),), "the rows", dev)
    group = None if group is None else group.contiguous()
    mask = torch.empty(T, dtype=torch.uint8, device=dev) if out is None else out
    thresholds = torch.empty(G, dtype=torch.int64, device=dev) if return_thresholds else None
    quota_d = q.to(dev)
    nb = select_limits(G)[1]
    ws = torch.empty(nb // 16 * 2, dtype=torch.int64, device=dev)         # torch's allocations are 16-byte aligned and more
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_select_per_group(_ptr(group), T, G, _ptr(quota_d), seed, _ptr(mask), _ptr(thresholds), _ptr(status), _ptr(ws),
                                             nb, _stream()))
    bits = int(status.item())                                             # the one read-back
    if bits & SELECT_GROUP:
        raise IndexError(f"{fn}: a group id lies outside [0, {G})")
    if bits & SELECT_QUOTA:
        raise ValueError(f"{fn}: a quota is larger than its group's row count")
    if bits:
        raise RuntimeError(f"{fn}: the group vector changed while the call ran (status {bits})")
    return (mask, thresholds) if return_thresholds else mask
