"""Exact draws on the device: rows per group (`ngcf_select_*`: csrc/select.hip; in the header's section "exact per-group sampling").
The draw of unseen items per case lives with its siblings in `engine.negatives`; its names are re-exported here."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _lib
from ._plumbing import _on, _ptr, _require_device, _require_same_device, _stream
from .negatives import SAMPLE_M_MAX, sample_unseen  # noqa: F401

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
