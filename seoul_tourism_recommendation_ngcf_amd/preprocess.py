"""The reference's numeric stage between raw visitor counts and ratings on the device: Preprocess.scale_implicit (utils.py:103-122).

The reference standardises the one rating column (sklearn's StandardScaler, fp64), adds |min| so the smallest rating is exactly 0,
and then walks the users in Python: an `isin` over the whole frame, a `quantile(q=0.25)` of the user's ratings across all years and
items, and a masked write that sets every rating below that quartile to 0 - O(users x rows) of host work.  Users touch only their
own rows, so here one call (engine.segment_quantile_floor) does every user at once, with the same fp64 operations in the same
order: given the same (mean, scale, shift) the ratings are bit-equal to the reference's, up to the sign of a zero.

With it the chain runs on one device with no host loop: counts -> `scale_implicit` -> `split_by_year` / `split_stratified` ->
`matrix.laplacian_csr_slices` (HIP kernels; `matrix.laplacian_slices` is the same in torch ops, and its oracle) / `positives` ->
`sampling.train_triplets` / `sampling.test_candidates` -> training step -> `evaluate.candidate_ranking` ->
`recommend.blended_ranking`.

The split is `Preprocess.split_train_test` (utils.py:126-148), both of its protocols: `split_by_year` is the year hold-out that
main.py runs (all of year 18 and the unsampled 70 % of year 19 train, a uniform 30 % sample of year 19 tests), `split_stratified`
sklearn's `train_test_split(test_size=0.3, stratify=destination)` with the per-class counts of `stratified_counts`.  Both are one
`engine.select_per_group` call - from every group of rows exactly its quota, uniformly - and reproduce the reference's distribution,
not numpy's or pandas' random stream.

The reference's other scaler, `args.scaler == 'power'` (sklearn's PowerTransformer(): Yeo-Johnson, then the same standardisation),
is `fit_power`: lambda by Brent's method on the host, every evaluation of the likelihood one fused pass on the device
(engine.yeo_johnson_moments), and `scale_implicit(..., scaler=fit_power(visitors))` floors the transformed column.

The head of the chain is here too.  `aggregate_visits` is the pivot of `load_preprocess_data` (utils.py:46-55): the time-zone rows
of a day folded into one row by a group-by-sum on the device (engine.group_by: the five key columns packed into one word, a hash
table in memory, integer atomics), the rows sorted by the five keys as pivot_table returns them, plus the derived `year`, `month`,
`day`.  `map_ids` is utils.py:59-97: `itemid` the rank of `destination` among its sorted distinct values, `userid` the rank of the
string str(age) + str(sex) + mm + dd among the sorted distinct strings - not the numeric order: age 5 sorts between 45 and 55.  The
string becomes an integer with the same order (engine.decimal_code: every character a base-11 digit), so the map is one more
group-by with an inverse, and the reference's dictionaries come out of the few distinct keys on the host (`IdMaps.user_dict`,
`IdMaps.item_dict`).  `num_dict` is the dictionary of utils.py:152-158.

And so is its first line, `pd.read_csv(path, sep='|')` (utils.py:38-39): `read_visits` takes the log's bytes to the device in one
transfer and parses the six columns the pivot takes there (engine.text: the row starts in two passes, then a lane per row; the
file's other columns - `total_num`, `area`, `date365`, which the reference drops - are never parsed), and `load_visits` is
`aggregate_visits` of that: `load_preprocess_data` without its `.sample(100)`, from a path to a `VisitTable` with neither pandas nor
a host loop.

Not here: the string `scaler='power'` as an alias of that (it stays refused, with a message that says what to pass, until a change
that may edit the test pinning the refusal), Box-Cox and `inverse_transform`, the reference's `.sample(100)` of the rows it has
read, quoted fields, string and date columns of a file (`engine.text`), the permuted row order in which the reference's split returns its parts (see `split_by_year`), and the
reference's index-alignment quirk when year-20 rows are filtered before the scaler's output is assigned back (`map_ids` takes the
rows the caller kept).  (`graphs.holdout_split` is another thing: a per-user leave-some-out split of the synthetic graphs.)
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import engine
from .sampling import fmix


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


# ---- the reference's scaler='power': sklearn's PowerTransformer() = Yeo-Johnson with standardize=True ------------------------------
_GOLD = 1.618034               # the classic constants of bracketing and of Brent's golden step, as scipy's `brent` has them
_CGOLD = 0.3819660
_TINY = 2.2250738585072014e-308


def _bracket(f, xa: float, xb: float, grow: float = 110.0, maxiter: int = 1000):
    """Downhill from (xa, xb) in golden-ratio steps, with a parabolic guess where it lands inside the allowed stretch, until three
    points xa, xb, xc with f(xb) below both ends bracket a minimum.  Returns (xa, xb, xc, fa, fb, fc)."""
    fa, fb = f(xa), f(xb)
    if fa < fb:
        xa, xb, fa, fb = xb, xa, fb, fa
    xc = xb + _GOLD * (xb - xa)
    fc = f(xc)
    it = 0
    while fc < fb:
        t1 = (xb - xa) * (fb - fc)
        t2 = (xb - xc) * (fb - fa)
        val = t2 - t1
        denom = 2.0 * (1e-21 if abs(val) < 1e-21 else val)
        w = xb - ((xb - xc) * t2 - (xb - xa) * t1) / denom
        wlim = xb + grow * (xc - xb)
        if it > maxiter:
            raise RuntimeError("yeo_johnson_lambda: no bracket of a minimum found")
        it += 1
        if (w - xc) * (xb - w) > 0.0:                      # the parabola's vertex lies between xb and xc
            fw = f(w)
            if fw < fc:
                return xb, w, xc, fb, fw, fc
            if fw > fb:
                return xa, xb, w, fa, fb, fw
            w = xc + _GOLD * (xc - xb)
            fw = f(w)
        elif (w - wlim) * (wlim - xc) >= 0.0:              # beyond the limit: step to the limit
            w = wlim
            fw = f(w)
        elif (w - wlim) * (xc - w) > 0.0:                  # between xc and the limit
            fw = f(w)
            if fw < fc:
                xb, xc, fb, fc = xc, w, fc, fw
                w = xc + _GOLD * (xc - xb)
                fw = f(w)
        else:
            w = xc + _GOLD * (xc - xb)
            fw = f(w)
        xa, xb, xc, fa, fb, fc = xb, xc, w, fb, fc, fw
    return xa, xb, xc, fa, fb, fc


def _brent(f, brack, tol: float, maxiter: int) -> float:
    """Brent's minimiser (Brent 1973, ch. 5): parabolic interpolation through the three best points where the step is acceptable,
    a golden-section step otherwise; stops when the interval around x is within 2 * tol1, tol1 = tol * |x| + 1e-11."""
    xa, xb, xc, _, fb, _ = _bracket(f, float(brack[0]), float(brack[1]))
    x = w = v = xb
    fx = fw = fv = fb
    a, b = (xa, xc) if xa < xc else (xc, xa)
    deltax, rat = 0.0, 0.0
    for _ in range(maxiter):
        tol1 = tol * abs(x) + 1e-11
        tol2 = 2.0 * tol1
        xmid = 0.5 * (a + b)
        if abs(x - xmid) < tol2 - 0.5 * (b - a):
            break
        golden = abs(deltax) <= tol1
        if not golden:
            t1 = (x - w) * (fx - fv)
            t2 = (x - v) * (fx - fw)
            p = (x - v) * t2 - (x - w) * t1
            t2 = 2.0 * (t2 - t1)
            if t2 > 0.0:
                p = -p
            t2 = abs(t2)
            before, deltax = deltax, rat
            if p > t2 * (a - x) and p < t2 * (b - x) and abs(p) < abs(0.5 * t2 * before):
                rat = p / t2
                u = x + rat
                if u - a < tol2 or b - u < tol2:
                    rat = tol1 if xmid - x >= 0 else -tol1
            else:
                golden = True
        if golden:
            deltax = (a - x) if x >= xmid else (b - x)
            rat = _CGOLD * deltax
        if abs(rat) < tol1:
            u = x + tol1 if rat >= 0 else x - tol1
        else:
            u = x + rat
        fu = f(u)
        if fu > fx:
            if u < x:
                a = u
            else:
                b = u
            if fu <= fw or w == x:
                v, w, fv, fw = w, u, fw, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
        else:
            if u >= x:
                a = x
            else:
                b = x
            v, w, x, fv, fw, fx = w, x, u, fw, fx, fu
    return x


def yeo_johnson_lambda(x: torch.Tensor, *, brack: Tuple[float, float] = (-2.0, 2.0), tol: float = 1.48e-8, maxiter: int = 500) -> float:
    """The maximum-likelihood lambda of the Yeo-Johnson transform of the column `x` (any real dtype, [T], on the device), the
    `lambdas_[0]` of sklearn's PowerTransformer: Brent's method on the host from the bracket `brack`, with scipy's `brent` defaults
    (`tol`, tol1 = tol * |lambda| + 1e-11), minimising f(lambda) = n/2 * log(M2 / n) - (lambda - 1) * c, +inf where M2 / n is below
    the smallest normal double.  Every evaluation is one `engine.yeo_johnson_moments` launch and one 32-byte read-back; NaN rows are
    left out.  A column without a finite row raises ValueError."""
    if x.dim() != 1:
        raise ValueError(f"yeo_johnson_lambda: x must be [T], got {tuple(x.shape)}")
    engine._require_device(x, "x")
    xd = x.to(torch.float64).contiguous()
    if not bool(torch.isfinite(xd).any()):
        raise ValueError("yeo_johnson_lambda: the column has no finite row")

    def f(lam: float) -> float:
        n, _, m2, c = engine.yeo_johnson_moments(xd, lam).tolist()
        var = m2 / n
        if var < _TINY:
            return math.inf
        return n / 2 * math.log(var) - (lam - 1) * c
    return _brent(f, brack, float(tol), int(maxiter))


@dataclass(frozen=True)
class PowerScaler:
    """A fitted PowerTransformer(): the Yeo-Johnson `lam`, and the `(mean, scale, shift)` of `standard_stats` over the transformed
    column - sklearn's internal StandardScaler followed by the reference's `+ |min|`."""
    lam: float
    mean: float
    scale: float
    shift: float


def fit_power(x: torch.Tensor) -> PowerScaler:
    """The reference's `args.scaler == 'power'` fitted on the column `x` ([T], on the device): `lam = yeo_johnson_lambda(x)`, then
    `standard_stats` of psi(x, lam).  Pass the result as `scale_implicit(..., scaler=...)`."""
    lam = yeo_johnson_lambda(x)
    mean, scale, shift = standard_stats(engine.yeo_johnson(x.to(torch.float64).contiguous(), lam))
    return PowerScaler(lam, mean, scale, shift)


def scale_implicit(users: torch.Tensor, visitors: torch.Tensor, *, n_user: int, scaler: Union[str, PowerScaler, None] = "standard",
                   q: float = 0.25, stats: Optional[Sequence[float]] = None):
    """The ratings of `Preprocess.scale_implicit`: row t belongs to user `users[t]` (int64 [T], ids in [0, n_user)) and carries the
    raw count `visitors[t]` (any real dtype, [T], same device).  Returns `(ratings float64 [T] in input order, quartiles float64
    [n_user])`: z = ((visitors - mean) / scale) + shift, floored to 0 below the user's `q` quantile (pandas' `quantile(q)`) of z
    over all of the user's rows; the quartile of a user without rows is NaN.  `scaler="standard"` takes (mean, scale, shift) from
    `standard_stats(visitors)`, or from `stats` when given - then the result is a pure function of its inputs, bit-equal to numpy's;
    `scaler=None` floors the raw values.  A `PowerScaler` (from `fit_power(visitors)`: the reference's PowerTransformer option)
    writes psi(visitors, lam) into a fresh fp64 buffer and floors that with the scaler's own (mean, scale, shift); `stats` beside it
    is a ValueError.  The string `scaler="power"` still raises NotImplementedError (Yeo-Johnson: pass `fit_power(visitors)`); making
    it an alias waits for a change that may edit the test that pins the refusal.  `q` is 0.25 (the reference), 0.5 or 0.75.  A user id
    outside [0, n_user) raises IndexError.  A NaN count leaves its user's ratings unfloored (the comparison with a NaN quartile is
    false, as in pandas)."""
    power = scaler if isinstance(scaler, PowerScaler) else None
    if power is None and scaler == "power":
        raise NotImplementedError("scale_implicit: the string scaler='power' (PowerTransformer, Yeo-Johnson) is not an option yet: "
                                  "fit the transform and pass it, scaler=preprocess.fit_power(visitors)")
    if power is None and scaler not in ("standard", None):
        raise ValueError(f"scale_implicit: scaler={scaler!r} is neither 'standard', a PowerScaler, 'power' nor None")
    if power is not None and stats is not None:
        raise ValueError("scale_implicit: a PowerScaler carries its own (mean, scale, shift); stats cannot be passed with it")
    if users.dim() != 1 or visitors.dim() != 1 or users.numel() != visitors.numel():
        raise ValueError(f"scale_implicit: users [T] and visitors [T] expected, got {tuple(users.shape)} and {tuple(visitors.shape)}")
    engine._require_device(users, "users")
    if visitors.device != users.device:
        raise RuntimeError(f"scale_implicit: visitors is on {visitors.device}, users on {users.device}")
    if power is not None:
        mean, scale, shift = power.mean, power.scale, power.shift
    elif scaler is None:
        if stats is not None:
            raise ValueError("scale_implicit: stats are the standard scaler's; scaler=None takes none")
        mean, scale, shift = 0.0, 1.0, 0.0
    elif stats is not None:
        mean, scale, shift = (float(s) for s in stats)
    else:
        mean, scale, shift = standard_stats(visitors)
    rowptr, order = engine.segments_from_ids(users.to(torch.int64), int(n_user))
    x = visitors.to(torch.float64).contiguous()
    if power is not None:
        x = engine.yeo_johnson(x, power.lam)                              # a fresh buffer
    out = x if x.data_ptr() != visitors.data_ptr() else None              # a converted copy is floored in place
    return engine.segment_quantile_floor(rowptr, x, order=order, mean=mean, scale=scale, shift=shift, q=q, out=out)


def positives(ratings: torch.Tensor) -> torch.Tensor:
    """The mask `ratings > 0`, the reference's `pos_tmp` (utils.py:236): after the floor a user's positives are the rows whose
    rating survived.  `sampling.train_triplets(users[m], items[m], ...)` over the masked rows draws negatives among everything
    else, floored rows included, as the reference does; `matrix.laplacian_slices` takes the ratings whole, since its rule "an
    explicit 0 removes the edge" is what the floor's zeros mean."""
    return ratings > 0


# ---- the head of the chain: raw visit records -> pivoted rows -> user and item ids (utils.py:36-97) ---------------------------------
@dataclass(frozen=True)
class VisitTable:
    """The rows of `load_preprocess_data` as int64 [G] columns on the device, sorted by (date, destination, dayofweek, sex, age):
    `date` the integer yyyymmdd, `visitor` the sum over the day's time-zone rows, `year` (two digits), `month`, `day` derived."""
    date: torch.Tensor
    destination: torch.Tensor
    dayofweek: torch.Tensor
    sex: torch.Tensor
    age: torch.Tensor
    visitor: torch.Tensor
    year: torch.Tensor
    month: torch.Tensor
    day: torch.Tensor

    def __len__(self) -> int:
        return int(self.date.numel())


def aggregate_visits(date: torch.Tensor, destination: torch.Tensor, dayofweek: torch.Tensor, sex: torch.Tensor, age: torch.Tensor,
                     visitor: torch.Tensor, *, lds_slots: Optional[int] = None) -> VisitTable:
    """`pd.pivot_table(df, index=['date', 'destination', 'dayofweek', 'sex', 'age'], aggfunc={'visitor': 'sum'}).reset_index()` of
    utils.py:46-48 on the device, with the derived columns of utils.py:51-55.  Six int32 / int64 [T] columns on one device; `date`
    is the integer yyyymmdd of the CSV (its order is the dates').  `visitor` must be an integer column (TypeError otherwise: see
    `engine.group_by`).  One `engine.group_by` call; `year`, `month`, `day` are integer torch ops on the G result rows."""
    g = engine.group_by((date, destination, dayofweek, sex, age), (visitor,), lds_slots=lds_slots)
    d = g.keys[0]
    return VisitTable(d, g.keys[1], g.keys[2], g.keys[3], g.keys[4], g.sums[0], (d // 10000) % 100, (d // 100) % 100, d % 100)


VISIT_COLUMNS = ("date", "destination", "dayofweek", "sex", "age", "visitor")


def read_visits(source, *, device=None, columns: Sequence[str] = VISIT_COLUMNS, sep: str = "|") -> Tuple[torch.Tensor, ...]:
    """The raw visit log, `pd.read_csv(path, sep='|')` of utils.py:38-39, as int64 [T] columns on the device, in the order of
    `columns` - by default the six that `aggregate_visits` takes, in its order.  `source` is a path (read with `np.fromfile` and
    copied to the device in one transfer), a `bytes` object, or a uint8 tensor on any device; `device` defaults to the tensor's own
    if that is a ROCm device and to 'cuda' otherwise.  The first row is the header and names the columns; the file's other columns
    (the reference's has `total_num`, `area`, `date365`, which it drops) are never parsed.  `engine.text.read_table` does the work:
    its grammar and its errors (ValueError with the data row, the column and the kind; KeyError for a column the header lacks)."""
    if isinstance(source, torch.Tensor):
        data = source
        if device is None and not source.is_cuda:
            device = "cuda"
    else:
        if isinstance(source, (bytes, bytearray, memoryview)):
            host = np.frombuffer(source, dtype=np.uint8).copy()
        elif isinstance(source, (str, os.PathLike)):
            host = np.fromfile(source, dtype=np.uint8)
        else:
            raise TypeError(f"read_visits: source must be a path, bytes or a uint8 tensor, got {type(source).__name__}")
        data = torch.from_numpy(host)
        device = "cuda" if device is None else device
    if data.dtype != torch.uint8:
        raise TypeError(f"read_visits: the source tensor must be uint8, got {data.dtype}")
    if device is not None:
        data = data.to(device)
    table, _ = engine.text.read_table(data, {c: torch.int64 for c in columns}, sep=sep, header=True)
    return tuple(table[c] for c in columns)


def load_visits(source, *, device=None, lds_slots: Optional[int] = None) -> VisitTable:
    """`Preprocess.load_preprocess_data` (utils.py:36-55) without its `.sample(100)`: `aggregate_visits(*read_visits(source))`, from
    the log's path (or bytes, or a uint8 tensor) to the pivoted rows on the device.  `date` stays the integer yyyymmdd, as
    `VisitTable` documents: the reference's `pd.to_datetime` only re-types it."""
    return aggregate_visits(*read_visits(source, device=device), lds_slots=lds_slots)


USER_KEY_WIDTHS = (0, 0, 2, 2)          # str(age) + str(sex) + '%m' + '%d' (utils.py:52-54, 71)


@dataclass(frozen=True)
class IdMaps:
    """`userid`, `itemid` int64 [T] of `map_ids`, and the distinct keys behind them in id order: `user_codes` int64 [n_user] (the
    `engine.decimal_code` of the user strings) and `item_keys` int64 [n_item] (destination codes)."""
    userid: torch.Tensor
    itemid: torch.Tensor
    user_codes: torch.Tensor
    item_keys: torch.Tensor

    @property
    def n_user(self) -> int:
        return int(self.user_codes.numel())

    @property
    def n_item(self) -> int:
        return int(self.item_keys.numel())

    def user_dict(self) -> Dict[str, int]:
        """The reference's `user_dict` (utils.py:72): the user string -> id.  Host work on the n_user distinct keys."""
        return {engine.decimal_string(c): i for i, c in enumerate(self.user_codes.tolist())}

    def item_dict(self) -> Dict[int, int]:
        """The reference's `item_dict` (utils.py:73): destination code -> id."""
        return {int(d): i for i, d in enumerate(self.item_keys.tolist())}


def map_ids(age: torch.Tensor, sex: torch.Tensor, month: torch.Tensor, day: torch.Tensor, destination: torch.Tensor, *,
            lds_slots: Optional[int] = None) -> IdMaps:
    """`Preprocess.map_ids` (utils.py:59-97) for five int32 / int64 [T] columns on one device: `itemid[t]` is the rank of
    `destination[t]` among the sorted distinct destinations, `userid[t]` the rank of str(age) + str(sex) + '%02d' % month +
    '%02d' % day among the sorted distinct strings (numpy's string sort: character by character).  The `year != 20` filter of
    utils.py:66 is the caller's boolean index before the call.  A negative value, or a month or day of more than two digits:
    ValueError."""
    code = engine.decimal_code((age, sex, month, day), USER_KEY_WIDTHS)
    users = engine.group_by((code,), inverse=True, lds_slots=lds_slots)
    items = engine.group_by((destination,), inverse=True, lds_slots=lds_slots)
    return IdMaps(users.inverse, items.inverse, users.keys[0], items.keys[0])


def num_dict(ids: IdMaps, sex: torch.Tensor, age: torch.Tensor, month: torch.Tensor, day: torch.Tensor,
             dayofweek: torch.Tensor) -> Dict[str, int]:
    """The `num_dict` of utils.py:152-158 as Python ints: the numbers of distinct users and items, and maximum + 1 of the five
    feature columns (one read-back of the five maxima)."""
    cols = (sex, age, month, day, dayofweek)
    for c, nm in zip(cols, ("sex", "age", "month", "day", "dayofweek")):
        engine._require_device(c, nm)
        if c.dim() != 1 or c.numel() == 0:
            raise ValueError(f"num_dict: {nm} must be a non-empty [T] column, got {tuple(c.shape)}")
    top = torch.stack([c.max().to(torch.int64) for c in cols]).tolist()
    return {"user": ids.n_user, "item": ids.n_item, "sex": top[0] + 1, "age": top[1] + 1, "month": top[2] + 1, "day": top[3] + 1,
            "dayofweek": top[4] + 1}


# ---- the split: Preprocess.split_train_test (utils.py:126-148) ------------------------------------------------------------------------
def _approximate_mode(counts: np.ndarray, n_draws: int, seed: int):
    """sklearn's `_approximate_mode` restated: the most likely outcome of drawing `n_draws` rows from classes of `counts` rows, in
    fp64 as sklearn computes it - `counts / counts.sum() * n_draws` floored, then one more row to the classes with the largest
    remainders until `n_draws` are placed.  Where some but not all classes of one remainder get a row sklearn draws them from its
    random state; here they are taken in ascending order of fmix(seed ^ class).  Returns `(drawn int64 [C], cut)`: `cut` says that
    such a tie was cut (without one the result is sklearn's for every random state)."""
    counts = np.asarray(counts, dtype=np.int64)
    continuous = counts / counts.sum() * n_draws
    floored = np.floor(continuous)
    need = int(n_draws - floored.sum())
    cut = False
    if need > 0:
        remainder = continuous - floored
        for value in np.sort(np.unique(remainder))[::-1]:
            inds, = np.where(remainder == value)
            add_now = min(len(inds), need)
            if add_now < len(inds):
                cut = True
                inds = np.array(sorted(inds.tolist(), key=lambda c: fmix((int(seed) & (2 ** 64 - 1)) ^ c))[:add_now], dtype=np.int64)
            floored[inds] += 1
            need -= add_now
            if need == 0:
                break
    return floored.astype(np.int64), cut


def stratified_counts(counts, test_size: float = 0.3, *, seed: int = 0):
    """`(train_counts, test_counts)`, int64 numpy [C]: how many rows of every class sklearn's `train_test_split(test_size=,
    stratify=)` puts into each part, from the class sizes `counts` alone (host, fp64).  n_test = ceil(test_size * n) and n_train =
    n - n_test - sklearn's rule when no train size is given, floor((1 - test_size) * n) in exact arithmetic; `_approximate_mode` of
    `counts` with n_train, then of what is left with n_test.  The one place where sklearn uses its random state for a count is a
    tie: when some but not all classes of equal remainder receive a row, the classes are taken in ascending order of
    fmix(seed ^ class) (class = the position in `counts`; fmix as in `sampling`) instead - class totals like the ones in the tests
    cut no tie and give sklearn's counts for every random state.  ValueError, as sklearn raises: a `test_size` outside (0, 1), a
    class of fewer than 2 rows, fewer train or test rows than classes."""
    c = np.asarray(counts)
    if c.ndim != 1 or c.size < 1 or c.dtype.kind not in "iu":
        raise ValueError(f"stratified_counts: counts must be a non-empty 1-D integer array, got shape {c.shape} of {c.dtype}")
    c = c.astype(np.int64)
    test_size = float(test_size)
    if not 0.0 < test_size < 1.0:
        raise ValueError(f"stratified_counts: test_size={test_size} should be a float in the (0, 1) range")
    if int(c.min()) < 2:
        raise ValueError("stratified_counts: the least populated class has fewer than 2 rows, which is too few")
    n, n_classes = int(c.sum()), int(c.size)
    n_test = int(math.ceil(test_size * n))
    n_train = n - n_test
    if n_train < n_classes:
        raise ValueError(f"stratified_counts: the train size {n_train} should be at least the number of classes {n_classes}")
    if n_test < n_classes:
        raise ValueError(f"stratified_counts: the test size {n_test} should be at least the number of classes {n_classes}")
    train, _ = _approximate_mode(c, n_train, seed)
    test, _ = _approximate_mode(c - train, n_test, seed)
    return train, test


def split_stratified(strata: torch.Tensor, *, test_size: float = 0.3, seed: int):
    """The reference's `train_by_destination=True` split, `train_test_split(total_df, test_size=0.3, stratify=destination)`:
    `strata` (int32 / int64 [T] on the device, non-negative class ids, e.g. `itemid`) -> `(train_idx, test_idx)`, int64 row indices
    in ascending order.  `torch.bincount` and one read-back give the class sizes, `stratified_counts` over the classes that occur
    (in id order, as sklearn numbers them) the test count of every class, one `engine.select_per_group` call the rows: within a class
    every subset of that size is equally likely.  Every row goes to one of the two parts.  Deviation: sklearn returns both parts in
    permuted order; the reference's train loader shuffles anyway, and its test loader does not, so only the batching of the test
    cases differs.  ValueError as `stratified_counts` raises it."""
    if strata.dim() != 1:
        raise ValueError(f"split_stratified: strata must be [T], got {tuple(strata.shape)}")
    if strata.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"split_stratified: strata must be int32 or int64, got {strata.dtype}")
    test_size = float(test_size)
    if not 0.0 < test_size < 1.0:
        raise ValueError(f"split_stratified: test_size={test_size} should be a float in the (0, 1) range")
    engine._require_device(strata, "strata")
    if strata.numel() == 0:
        raise ValueError("split_stratified: no rows to split")
    sizes = torch.bincount(strata).cpu().numpy().astype(np.int64)          # the read-back: G counts (a negative id: torch raises)
    if sizes.size >= 2 ** 31:
        raise ValueError(f"split_stratified: class ids up to {sizes.size - 1}, beyond int32")
    present = np.flatnonzero(sizes)
    _, test = stratified_counts(sizes[present], test_size, seed=seed)
    quota = np.zeros(sizes.size, dtype=np.int64)
    quota[present] = test
    mask = engine.select_per_group(strata.to(torch.int32), quota, seed=seed)
    return torch.nonzero(mask == 0).view(-1), torch.nonzero(mask).view(-1)


def split_by_year(year: torch.Tensor, *, train_year: int = 18, test_year: int = 19, frac: float = 0.3, seed: int):
    """The reference's year hold-out (utils.py:133-139, 147-148; what main.py runs): `year` (int32 / int64 [T] on the device) ->
    `(train_idx, test_idx)`, int64 row indices.  Test: a uniform sample without replacement of round(frac * n) of the n rows of
    `test_year` - Python's round, half to even, which is pandas' `sample(frac=)` rule - in row order.  Train: all rows of
    `train_year` in row order, then the unsampled rows of `test_year` in row order, the order of the reference's `concat`.  Rows of
    other years are in neither part.  One read-back of n, one `engine.select_per_group` call (the test year is group 0, everything
    else a group with quota 0).  Deviation: the reference's sample comes in permuted order; its train loader shuffles anyway, and
    its test loader does not, so only the batching of the test cases differs."""
    if year.dim() != 1:
        raise ValueError(f"split_by_year: year must be [T], got {tuple(year.shape)}")
    if year.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"split_by_year: year must be int32 or int64, got {year.dtype}")
    train_year, test_year, frac = int(train_year), int(test_year), float(frac)
    if train_year == test_year:
        raise ValueError(f"split_by_year: train_year and test_year are both {train_year}")
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"split_by_year: frac={frac} outside [0, 1]")
    engine._require_device(year, "year")
    held = year == test_year
    quota = year_quota(int(held.sum().item()), frac)                        # the read-back: n
    mask = engine.select_per_group((~held).to(torch.int32), [quota, 0], seed=seed).bool()
    train = torch.cat([torch.nonzero(year == train_year).view(-1), torch.nonzero(held & ~mask).view(-1)])
    return train, torch.nonzero(mask).view(-1)


def year_quota(n: int, frac: float = 0.3) -> int:
    """round(frac * n), half to even: the number of rows pandas' `sample(frac=)` takes from n."""
    return int(round(float(frac) * int(n)))
