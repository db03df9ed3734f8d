"""The reference's numeric stage between raw visitor counts and ratings on the device: Preprocess.scale_implicit (utils.py:103-122).

The reference standardises the one rating column (sklearn's StandardScaler, fp64), adds |min| so the smallest rating is exactly 0,
and then walks the users in Python: an `isin` over the whole frame, a `quantile(q=0.25)` of the user's ratings across all years and
items, and a masked write that sets every rating below that quartile to 0 - O(users x rows) of host work.  Users touch only their
own rows, so here one call (engine.segment_quantile_floor) does every user at once, with the same fp64 operations in the same
order: given the same (mean, scale, shift) the ratings are bit-equal to the reference's, up to the sign of a zero.

With it the chain runs on one device with no host loop: counts -> `scale_implicit` -> `matrix.laplacian_slices` / `positives` ->
`sampling.train_triplets` -> training step -> `evaluate.candidate_ranking` -> `recommend.blended_ranking`.

Not here: `scaler='power'` (Yeo-Johnson: its lambda needs an optimiser), `load_preprocess_data` and `map_ids` (pandas string keys,
host work), `split_train_test` (`graphs.holdout_split` exists), and the reference's index-alignment quirk when year-20 rows are
filtered before the scaler's output is assigned back.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import engine


def _pairwise_sum(v: torch.Tensor) -> torch.Tensor:
    """Sum of a 1-D tensor by halving: every value passes through ceil(log2 n) additions whatever the device's reduction does, which
    is the bound the tests hold `standard_stats` to.  A padding zero adds nothing."""
    while v.numel() > 1:
        if v.numel() & 1:
            v = torch.cat([v, v.new_zeros(1)])
        h = v.numel() // 2
        v = v[:h] + v[h:]
    return v


def standard_stats(x: torch.Tensor):
    """`(mean, scale, shift)` of a rating column as Python floats, from fp64 reductions on the column's device: StandardScaler's
    mean and scale = sqrt(population variance), and shift = |z(min x)| with z(v) = (v - mean) / scale, so that
    ((v - mean) / scale) + shift - the kernel's three operations - is exactly 0 at the minimum.  An integer column is summed in
    int64, so its mean is correctly rounded; the squared deviations are summed pairwise.  A constant (or empty) column has no scale:
    ValueError (sklearn would divide by 1 and return all zeros, which floors nothing)."""
    if x.dim() != 1:
        raise ValueError(f"standard_stats: x must be [T], got {tuple(x.shape)}")
    engine._require_device(x, "x")
    n = int(x.numel())
    if n == 0:
        raise ValueError("standard_stats: an empty column has no scale")
    xd = x.to(torch.float64)
    if x.dtype.is_floating_point:
        mean = float(_pairwise_sum(xd).item()) / n
    else:
        mean = int(x.to(torch.int64).sum().item()) / n             # Python's int / int rounds once
    dev = xd - mean
    var = float(_pairwise_sum(dev * dev).item()) / n
    if not var > 0.0 or not math.isfinite(var):
        raise ValueError("standard_stats: the column is constant (or not finite): it has no scale")
    scale = math.sqrt(var)
    shift = abs((float(xd.min().item()) - mean) / scale)
    return mean, scale, shift


def scale_implicit(users: torch.Tensor, visitors: torch.Tensor, *, n_user: int, scaler: Optional[str] = "standard", q: float = 0.25,
                   stats: Optional[Sequence[float]] = None):
    """The ratings of `Preprocess.scale_implicit`: row t belongs to user `users[t]` (int64 [T], ids in [0, n_user)) and carries the
    raw count `visitors[t]` (any real dtype, [T], same device).  Returns `(ratings float64 [T] in input order, quartiles float64
    [n_user])`: z = ((visitors - mean) / scale) + shift, floored to 0 below the user's `q` quantile (pandas' `quantile(q)`) of z
    over all of the user's rows; the quartile of a user without rows is NaN.  `scaler="standard"` takes (mean, scale, shift) from
    `standard_stats(visitors)`, or from `stats` when given - then the result is a pure function of its inputs, bit-equal to numpy's;
    `scaler=None` floors the raw values.  `scaler="power"` (the reference's PowerTransformer option) raises NotImplementedError: the
    Yeo-Johnson lambda needs an optimiser this package does not have yet.  `q` is 0.25 (the reference), 0.5 or 0.75.  A user id
    outside [0, n_user) raises IndexError.  A NaN count leaves its user's ratings unfloored (the comparison with a NaN quartile is
    false, as in pandas)."""
    if scaler == "power":
        raise NotImplementedError("scale_implicit: scaler='power' (PowerTransformer, Yeo-Johnson) is not implemented: its lambda is "
                                  "fitted by an optimiser; use scaler='standard' or transform the counts beforehand and pass scaler=None")
    if scaler not in ("standard", None):
        raise ValueError(f"scale_implicit: scaler={scaler!r} is neither 'standard', 'power' nor None")
    if users.dim() != 1 or visitors.dim() != 1 or users.numel() != visitors.numel():
        raise ValueError(f"scale_implicit: users [T] and visitors [T] expected, got {tuple(users.shape)} and {tuple(visitors.shape)}")
    engine._require_device(users, "users")
    if visitors.device != users.device:
        raise RuntimeError(f"scale_implicit: visitors is on {visitors.device}, users on {users.device}")
    if scaler is None:
        if stats is not None:
            raise ValueError("scale_implicit: stats are the standard scaler's; scaler=None takes none")
        mean, scale, shift = 0.0, 1.0, 0.0
    elif stats is not None:
        mean, scale, shift = (float(s) for s in stats)
    else:
        mean, scale, shift = standard_stats(visitors)
    rowptr, order = engine.segments_from_ids(users.to(torch.int64), int(n_user))
    x = visitors.to(torch.float64).contiguous()
    out = x if x.data_ptr() != visitors.data_ptr() else None              # a converted copy is floored in place
    return engine.segment_quantile_floor(rowptr, x, order=order, mean=mean, scale=scale, shift=shift, q=q, out=out)


def positives(ratings: torch.Tensor) -> torch.Tensor:
    """The mask `ratings > 0`, the reference's `pos_tmp` (utils.py:236): after the floor a user's positives are the rows whose
    rating survived.  `sampling.train_triplets(users[m], items[m], ...)` over the masked rows draws negatives among everything
    else, floored rows included, as the reference does; `matrix.laplacian_slices` takes the ratings whole, since its rule "an
    explicit 0 removes the edge" is what the floor's zeros mean."""
    return ratings > 0
