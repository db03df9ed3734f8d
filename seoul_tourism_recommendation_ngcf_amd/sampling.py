"""The reference's data stage between "interactions" and "a trained, evaluated model" on the device: TourDataset._negative_sampling
(utils.py:213-275) and the DataLoader of main.py:39-42.

The reference walks the users in Python and calls `np.setxor1d` and `np.random.choice(neg_items, ng_ratio, replace=False)` once per
positive row - O(users x items) of host work before the first step.  Here one launch (engine.sample_unseen) draws the unseen items
of every row: 1 per training triplet, 24 per test case.  It is the reference's DISTRIBUTION (uniform over the user's unseen items,
without replacement), not numpy's random stream: no seed reproduces the reference's items, and every drawn value is instead a pure
function of (seed, row number, the user's seen items) that the tests recompute on the host (include/ngcf_hip.h has the formulae).
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch

from . import engine

_M64 = (1 << 64) - 1


def fmix(x: int) -> int:
    """The 64-bit finaliser of the library's counter-based hashes (csrc/common.h, fmix64) on Python integers."""
    x &= _M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x


def _rows(users: torch.Tensor, items: torch.Tensor, seen: Optional[engine.ItemSets], n_user: int, n_item: int, what: str):
    if users.dim() != 1 or items.dim() != 1 or users.numel() != items.numel():
        raise ValueError(f"{what}: users [T] and items [T] expected, got {tuple(users.shape)} and {tuple(items.shape)}")
    engine._require_device(users, "users")
    users = users.to(torch.int64)
    items = items.to(device=users.device, dtype=torch.int64)
    if seen is None:
        seen = engine.ItemSets.from_pairs(users, items, int(n_user), int(n_item))
    elif seen.n_items != int(n_item) or seen.n_rows < int(n_user):
        raise ValueError(f"{what}: the seen sets hold {seen.n_rows} users x {seen.n_items} items, expected {n_user} x {n_item}")
    return users, items, seen


def train_triplets(users: torch.Tensor, items: torch.Tensor, seen: Optional[engine.ItemSets] = None, *, seed: int, epoch: int = 0,
                   n_user: int, n_item: int):
    """The content of `TourDataset(train=True)`: for positive row t = (users[t], items[t]) one item the user has no entry for in
    `seen` (default: `ItemSets.from_pairs(users, items, n_user, n_item)`, the positives themselves).  Returns (users, items, neg),
    int64 [T] on the device of `users`.  The draw of row t depends on (seed_e, t, the user's seen row) with
    seed_e = fmix(seed + epoch), `fmix` the 64-bit finaliser above: the reference draws once, at construction - keep `epoch` = 0 for
    that - while a new `epoch` redraws every negative.  A user id outside the sets raises IndexError, a user who has seen every item
    ValueError."""
    users, items, seen = _rows(users, items, seen, n_user, n_item, "train_triplets")
    neg = engine.sample_unseen(seen, users, 1, fmix(int(seed) + int(epoch)))
    return users, items, neg[:, 0]


def _hard_draw(users: torch.Tensor, user_emb: torch.Tensor, item_emb: torch.Tensor, seen: engine.ItemSets, m: int, seed_e: int,
               chunk: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The hard negative of every row (engine.negatives.hard_unseen), in one launch or in pieces of `chunk` rows."""
    n = int(users.numel())
    if chunk is None or int(chunk) >= n:
        return engine.negatives.hard_unseen(seen, user_emb, item_emb, users, m, seed_e, out=out)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"hard_triplets: chunk={chunk}")
    neg = torch.empty(n, dtype=torch.int64, device=users.device) if out is None else out
    for r0 in range(0, n, chunk):
        engine.negatives.hard_unseen(seen, user_emb, item_emb, users[r0:r0 + chunk], m, seed_e, case_offset=r0, out=neg[r0:r0 + chunk])
    return neg


def hard_triplets(users: torch.Tensor, items: torch.Tensor, user_emb: torch.Tensor, item_emb: torch.Tensor,
                  seen: Optional[engine.ItemSets] = None, *, m: int = 8, seed: int, epoch: int = 0, n_user: int, n_item: int,
                  chunk: Optional[int] = None):
    """`train_triplets` with hard negatives (dynamic negative sampling): for positive row t the best-scoring of `m` items the user
    has no entry for in `seen`, under the tables `user_emb` [>= n_user, D] and `item_emb` [>= n_item, D] - in practice
    `model.all_users_emb` and `model.all_items_emb` after a propagation (a forward of the model), so the negatives are as fresh as
    those tables: tables from before the last optimizer steps pick the items that were hard then.  Returns (users, items, neg),
    int64 [T] on the device of `users`.  With seed_e = fmix(seed + epoch), exactly as in `train_triplets`: neg[t] is an element of
    row t of `engine.sample_unseen(seen, users, m, seed_e)` - the one with the largest <user_emb[users[t]], item_emb[.]> in the
    bits and order of `engine.negatives.hard_unseen`, one launch, nothing of size T x m in memory - and with m = 1 the result
    equals `train_triplets(...)`, whatever the tables.  `chunk` draws the rows in pieces of that many through `case_offset`, with the
    same result.  `m` in [1, 64].  A user id outside the sets raises IndexError, a user with fewer than `m` unseen items ValueError."""
    users, items, seen = _rows(users, items, seen, n_user, n_item, "hard_triplets")
    return users, items, _hard_draw(users, user_emb, item_emb, seen, int(m), fmix(int(seed) + int(epoch)), chunk)


def test_candidates(users: torch.Tensor, items: torch.Tensor, seen: Optional[engine.ItemSets] = None, *, m: int = 24, seed: int,
                    n_user: int, n_item: int) -> torch.Tensor:
    """The content of `TourDataset(train=False)`: for test row t = (users[t], items[t]) the candidate list [items[t], m items the
    user has no entry for in `seen`], int64 [T, m + 1] - exactly the `candidates` of `evaluate.candidate_ranking`, column 0 the
    held-out item.  The reference's quirk: it builds the test set from the test frame alone, so its negatives are unseen relative
    to the user's TEST positives only (utils.py:234-238) and may be items the user was trained on.  `seen` chooses: the default,
    `ItemSets.from_pairs(users, items, ...)` over the test rows, is the reference; sets over train and test rows together are the
    stricter protocol.  A user with fewer than `m` unseen items raises ValueError (np.random.choice raises there)."""
    users, items, seen = _rows(users, items, seen, n_user, n_item, "test_candidates")
    return engine.sample_unseen(seen, users, int(m), int(seed), first=items)


test_candidates.__test__ = False          # a public name of the reference's vocabulary, not a test


class _EpochLoader:
    """What the six loaders share: the columns' validation, the id table `[columns, n]` (int64; its last rows are the items and,
    with one negative per row, the negatives), `len()`, the epoch counter and the one permutation and gather per `iter()`.  A
    loader is a constructor and `_draw`, which fills this epoch's negatives: the table's last row, or `self.neg` int64 [n, m] where a
    row has m of them (None otherwise), which is gathered by the same permutation - and so is `self.logq`, a float array [n, m]
    that goes with `self.neg` slot by slot (None otherwise) and ends the batch."""

    def __init__(self, name: str, users: torch.Tensor, columns: Sequence[torch.Tensor], tail: Sequence[torch.Tensor], *, batch_size: int,
                 shuffle: bool, drop_last: bool, generator: Optional[torch.Generator], m: Optional[int] = None, m_max: int = 0):
        cols = (list(columns) if len(columns) else [users]) + list(tail)
        n = int(users.numel())
        for c in [users] + cols:
            if c.dim() != 1 or int(c.numel()) != n:
                raise ValueError(f"{name}: every column must be [n = {n}], got {tuple(c.shape)}")
            if c.device != users.device:
                raise RuntimeError(f"{name}: a column is on {c.device}, users on {users.device}")
        if int(batch_size) < 1:
            raise ValueError(f"{name}: batch_size={batch_size}")
        if m is not None and (int(m) < 1 or int(m) > m_max):
            raise ValueError(f"{name}: m={m} outside [1, {m_max}]")
        self.table = torch.stack([c.to(torch.int64) for c in cols])            # [columns, n]
        self.neg: Optional[torch.Tensor] = None
        self.logq: Optional[torch.Tensor] = None
        self.n, self.batch_size, self.m, self.epoch = n, int(batch_size), m if m is None else int(m), 0
        self.shuffle, self.drop_last, self.generator = bool(shuffle), bool(drop_last), generator

    def __len__(self) -> int:
        return self.n // self.batch_size if self.drop_last else -(-self.n // self.batch_size)

    def _draw(self):
        """This epoch's negatives (epoch number `self.epoch`), written in place; nothing where they are given."""

    def __iter__(self):
        self._draw()
        self.epoch += 1
        return self._batches()

    def _batches(self):
        used = len(self) * self.batch_size if self.drop_last else self.n
        table, per_slot = self.table, [a for a in (self.neg, self.logq) if a is not None]
        if self.shuffle:
            rows = torch.randperm(self.n, generator=self.generator, device=table.device)[:used]
            table = table[:, rows]                                              # the epoch's one gathered copy
            per_slot = [a[rows] for a in per_slot]
        for b0 in range(0, used, self.batch_size):
            ids = tuple(table[:, b0:b0 + self.batch_size].unbind(0))
            yield ids + tuple(a[b0:b0 + self.batch_size].reshape(-1) for a in per_slot)


class TripletLoader(_EpochLoader):
    """A device-side iterator in the shape of the reference's `DataLoader(train_dataset, batch_size, shuffle=True, drop_last=True)`
    (main.py:39-42) over the rows of `train_triplets`.  `columns` are the caller's per-row tensors in the reference's order (year,
    u_id, age, sex, month, day, dow): a batch is `(*columns[b], items[b], neg[b])`, so the loop body of `Experiment.train` runs
    against it unchanged; without `columns` it is `(users[b], items[b], neg[b])`.  Every epoch (every `iter()`) draws one
    `torch.randperm` on the tensors' device from `generator` (None: the device's default generator), gathers all columns once into
    one int64 copy and yields its batches as views.  `len()` is the number of batches: n // batch_size with `drop_last`.  Plain
    torch: it runs wherever the tensors live."""


    def __init__(self, users: torch.Tensor, items: torch.Tensor, neg: torch.Tensor, columns: Sequence[torch.Tensor] = (), *,
                 batch_size: int, shuffle: bool = True, drop_last: bool = True, generator: Optional[torch.Generator] = None):
        super().__init__("TripletLoader", users, columns, (items, neg), batch_size=batch_size, shuffle=shuffle, drop_last=drop_last,
                         generator=generator)


class HardTripletLoader(_EpochLoader):
    """`TripletLoader` whose negatives are redrawn every epoch as hard negatives: the batch shape, `columns`, `shuffle`, `drop_last`
    and `generator` are `TripletLoader`'s, the `neg` column is `hard_triplets(..., m=m, seed=seed, epoch=e)`.  `tables` is a callable
    returning `(user_emb, item_emb)`, e.g. `lambda: (model.all_users_emb, model.all_items_emb)` after a propagation; every `iter()`
    calls it once, draws all negatives with epoch e = 0, 1, 2, ... (`.epoch` is the number of the next one) against those tables,
    then shuffles and yields views as `TripletLoader` does: one kernel launch, one `torch.randperm` and one gather per epoch.  The
    seen sets are the positives themselves, `ItemSets.from_pairs(users, items, ...)` over as many users and items as the tables have
    rows, built at the first `iter()`.  Without `shuffle` the batches are views of the loader's own table, which the next `iter()`
    overwrites."""

    def __init__(self, users: torch.Tensor, items: torch.Tensor, columns: Sequence[torch.Tensor] = (), *, batch_size: int,
                 tables: Callable[[], Tuple[torch.Tensor, torch.Tensor]], m: int = 8, seed: int, shuffle: bool = True,
                 drop_last: bool = True, generator: Optional[torch.Generator] = None):
        super().__init__("HardTripletLoader", users, columns, (items, torch.full_like(users, -1, dtype=torch.int64)),
                         batch_size=batch_size, shuffle=shuffle, drop_last=drop_last, generator=generator, m=m,
                         m_max=engine.negatives.HARD_M_MAX)
        if not callable(tables):
            raise TypeError("HardTripletLoader: tables must be a callable returning (user_emb, item_emb)")
        self.users, self.items = users.to(torch.int64), self.table[-2]
        self.tables, self.seed = tables, int(seed)
        self._seen: Optional[engine.ItemSets] = None

    def _draw(self):
        user_emb, item_emb = self.tables()
        if self._seen is None:
            self._seen = engine.ItemSets.from_pairs(self.users, self.items, int(user_emb.shape[0]), int(item_emb.shape[0]))
        _hard_draw(self.users, user_emb, item_emb, self._seen, self.m, fmix(self.seed + self.epoch), out=self.table[-1])


def train_negatives(users: torch.Tensor, items: torch.Tensor, seen: Optional[engine.ItemSets] = None, *, m: int, seed: int,
                    epoch: int = 0, n_user: int, n_item: int):
    """`train_triplets` with `m` negatives per positive row, for a `BPRMulti` criterion: returns (users, items, neg) with `neg` int64
    [T, m], row t the m distinct items of row t of `engine.sample_unseen(seen, users, m, seed_e)`, seed_e = fmix(seed + epoch) as in
    `train_triplets` - so with m = 1 `neg[:, 0]` is `train_triplets`' column.  `model(..., neg_item=neg[b].reshape(-1))` gathers
    the rows in the order `BPRMulti` reads them.  A user id outside the sets raises IndexError, a user with fewer than `m` unseen
    items ValueError."""
    users, items, seen = _rows(users, items, seen, n_user, n_item, "train_negatives")
    return users, items, engine.sample_unseen(seen, users, int(m), fmix(int(seed) + int(epoch)))


class NegativesLoader(_EpochLoader):
    """`TripletLoader` with `m` negatives per row, redrawn every epoch: the batch protocol, `columns`, `shuffle`, `drop_last` and
    `generator` are `TripletLoader`'s, and a batch is `(*columns[b], items[b], neg[b].reshape(-1))` - `batch_size` ids per column,
    `batch_size * m` negative ids, the m of a row next to each other - so the loop body of `Experiment.train` runs against it
    unchanged with `criterion = BPRMulti(weight_decay, batch_size, m)`.  Every `iter()` draws all negatives with epoch e = 0, 1, 2, ...
    (`.epoch` is the number of the next one): `neg` = `train_negatives(users, items, seen, m=m, seed=seed, epoch=e, ...)[2]`,
    written straight into the loader's `.neg` [n, m], then one `torch.randperm` by which the id table and `.neg` are gathered once
    each; the batches are views of the gathered copies - without `shuffle`, of the loader's own arrays, which the next `iter()`
    overwrites.  `seen` (default: `ItemSets.from_pairs(users, items, users.max() + 1, items.max() + 1)`, the
    positives themselves over the ids that occur, which costs one host sync at construction) says what counts as seen and how
    large the catalogue is: pass sets over the full catalogue when some items have no positive row."""

    def __init__(self, users: torch.Tensor, items: torch.Tensor, columns: Sequence[torch.Tensor] = (), *, batch_size: int, m: int,
                 seed: int, shuffle: bool = True, drop_last: bool = True, generator: Optional[torch.Generator] = None,
                 seen: Optional[engine.ItemSets] = None):
        super().__init__("NegativesLoader", users, columns, (items,), batch_size=batch_size, shuffle=shuffle, drop_last=drop_last,
                         generator=generator, m=m, m_max=engine.losses.M_MAX)
        engine._require_device(users, "users")
        self.neg = torch.empty((self.n, self.m), dtype=torch.int64, device=users.device)
        self.users = users.to(torch.int64).contiguous()
        if seen is None and self.n:
            seen = engine.ItemSets.from_pairs(self.users, self.table[-1], int(self.users.max()) + 1, int(self.table[-1].max()) + 1)
        self.seen, self.seed = seen, int(seed)

    def _draw(self):
        if self.n:
            engine.sample_unseen(self.seen, self.users, self.m, fmix(self.seed + self.epoch), out=self.neg)


# ---- popularity-weighted negatives (engine.negatives.weighted_unseen) ----------------------------------------------------------------
def popularity_weights(items: torch.Tensor, n_item: int, alpha: float = 0.75, resolution: int = 1024) -> torch.Tensor:
    """Integer item weights from the items' counts in `items` (the positives' item column; ids in [0, n_item)), int64 [n_item] on the
    tensor's device: the counts themselves with `alpha` = 1, all ones with `alpha` = 0, otherwise
    floor(count^alpha * resolution + 0.5) in fp64 - at least 1 where the count is positive, 0 where it is 0, so an item nobody
    interacted with is never drawn.  alpha = 0.75 is the usual smoothing of a popularity sampler.  The weights are data: the draw is
    exact in them, and nothing downstream depends on how `pow` rounds.  Plain torch: it runs wherever `items` lives."""
    n_item, alpha, resolution = int(n_item), float(alpha), int(resolution)
    if items.dim() != 1 or items.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"popularity_weights: items must be an integer [T] tensor, got {items.dtype} {tuple(items.shape)}")
    if n_item < 1 or resolution < 1 or alpha < 0:
        raise ValueError(f"popularity_weights: n_item={n_item}, alpha={alpha}, resolution={resolution}")
    if alpha == 0:
        return torch.ones(n_item, dtype=torch.int64, device=items.device)
    if items.numel() and (int(items.min()) < 0 or int(items.max()) >= n_item):
        raise IndexError(f"popularity_weights: an item id lies outside [0, {n_item})")
    counts = torch.bincount(items.to(torch.int64), minlength=n_item)
    if alpha == 1:
        return counts
    scaled = torch.floor(counts.to(torch.float64).pow(alpha) * resolution + 0.5).to(torch.int64)
    return torch.where(counts > 0, scaled.clamp(min=1), torch.zeros_like(scaled))


def _weighted_sets(weights, seen: Optional[engine.ItemSets], what: str) -> "engine.negatives.WeightedSets":
    """`weights` as prepared sets: an int64 [n_item] tensor is prepared against `seen`, a `WeightedSets` is taken as it is."""
    if isinstance(weights, engine.negatives.WeightedSets):
        if seen is not None and seen is not weights.seen:
            raise ValueError(f"{what}: the prepared weights belong to other seen sets")
        return weights
    return engine.negatives.WeightedSets(seen, weights)


def weighted_negatives(users: torch.Tensor, items: torch.Tensor, weights, seen: Optional[engine.ItemSets] = None, *, m: int, seed: int,
                       epoch: int = 0, n_user: int, n_item: int, return_logq: bool = False):
    """`train_negatives` with popularity-weighted negatives: returns (users, items, neg) with `neg` int64 [T, m], row t the m distinct
    items of row t of `engine.negatives.weighted_unseen(wsets, users, m, seed_e)`, seed_e = fmix(seed + epoch) as in
    `train_triplets` - slot j is item i with probability w_i / U_j over the user's unseen items not drawn before, successive
    sampling.  `weights`: int64 [n_item] (e.g. `popularity_weights(items, n_item)`), prepared against `seen` (default: the positives
    themselves) in this call - or an `engine.negatives.WeightedSets`, prepared once and passed to every call.  It is this
    distribution, not anyone's random stream; with all-ones weights it is uniform but does not return `train_negatives`' items.
    With `return_logq` a fourth tensor, float64 [T, m]: logq[t, j] = log(w_j / U_j), the log proposal probability of slot j given
    the slots before it, formed in torch from the kernel's exact integers - what a sampled softmax subtracts from the negatives'
    scores: `SampledSoftmax` takes it as it is (the conditional probability of successive sampling, not the marginal probability
    that the item is among the m).  `m` in [1, 64].  A user id outside the sets raises
    IndexError, a user with fewer than `m` positive-weight unseen items ValueError."""
    m = int(m)
    if m < 1 or m > engine.negatives.WEIGHTED_M_MAX:
        raise ValueError(f"weighted_negatives: m={m} outside [1, {engine.negatives.WEIGHTED_M_MAX}]")
    prepared = isinstance(weights, engine.negatives.WeightedSets)
    if not prepared:
        if weights.dtype != torch.int64:
            raise TypeError(f"weighted_negatives: weights must be int64, got {weights.dtype}")
        if weights.dim() != 1 or int(weights.numel()) != int(n_item):
            raise ValueError(f"weighted_negatives: weights must be [n_item = {int(n_item)}], got {tuple(weights.shape)}")
    users, items, seen = _rows(users, items, weights.seen if prepared and seen is None else seen, n_user, n_item, "weighted_negatives")
    wsets = _weighted_sets(weights, seen, "weighted_negatives")
    seed_e = fmix(int(seed) + int(epoch))
    if not return_logq:
        return users, items, engine.negatives.weighted_unseen(wsets, users, m, seed_e)
    neg, w, mass = engine.negatives.weighted_unseen(wsets, users, m, seed_e, return_weights=True)
    left = mass[:, None] - (torch.cumsum(w, 1) - w)                                     # U_j, exact in int64
    return users, items, neg, torch.log(w.to(torch.float64) / left.to(torch.float64))


def weighted_triplets(users: torch.Tensor, items: torch.Tensor, weights, seen: Optional[engine.ItemSets] = None, *, seed: int,
                      epoch: int = 0, n_user: int, n_item: int, return_logq: bool = False):
    """`weighted_negatives` with one negative per row, the shape of `train_triplets`: (users, items, neg int64 [T]) - and with
    `return_logq` the float64 [T] log(w / U) of every negative."""
    got = weighted_negatives(users, items, weights, seen, m=1, seed=seed, epoch=epoch, n_user=n_user, n_item=n_item,
                             return_logq=return_logq)
    return got[:2] + tuple(t[:, 0] for t in got[2:])


class WeightedNegativesLoader(_EpochLoader):
    """`NegativesLoader` with popularity-weighted negatives: the batch protocol, `columns`, `shuffle`, `drop_last` and `generator`
    are `TripletLoader`'s, a batch is `(*columns[b], items[b], neg[b].reshape(-1))`, and every `iter()` redraws all negatives with
    epoch e = 0, 1, 2, ... (`.epoch` is the number of the next one): `neg` = `weighted_negatives(users, items, weights, seen, m=m,
    seed=seed, epoch=e, ...)[2]`, written straight into the loader's `.neg` [n, m].  `weights`: int64, one per item of `seen`
    (default: `ItemSets.from_pairs` over the positives and `weights.numel()` items), prepared once at construction
    (`.wsets`, an `engine.negatives.WeightedSets`)."""

    def __init__(self, users: torch.Tensor, items: torch.Tensor, weights: torch.Tensor, columns: Sequence[torch.Tensor] = (), *,
                 batch_size: int, m: int, seed: int, shuffle: bool = True, drop_last: bool = True,
                 generator: Optional[torch.Generator] = None, seen: Optional[engine.ItemSets] = None):
        super().__init__(type(self).__name__, users, columns, (items,), batch_size=batch_size, shuffle=shuffle,
                         drop_last=drop_last, generator=generator, m=m, m_max=engine.negatives.WEIGHTED_M_MAX)
        if weights.dtype != torch.int64 or weights.dim() != 1:
            raise TypeError(f"{type(self).__name__}: weights must be an int64 [n_item] tensor, got {weights.dtype} {tuple(weights.shape)}")
        engine._require_device(users, "users")
        self.neg = torch.empty((self.n, self.m), dtype=torch.int64, device=users.device)
        self.users = users.to(torch.int64).contiguous()
        if seen is None:
            seen = engine.ItemSets.from_pairs(self.users, self.table[-1], int(self.users.max()) + 1 if self.n else 1, int(weights.numel()))
        self.seen, self.seed = seen, int(seed)
        self.wsets = engine.negatives.WeightedSets(seen, weights)

    def _draw(self):
        if self.n:
            engine.negatives.weighted_unseen(self.wsets, self.users, self.m, fmix(self.seed + self.epoch), out=self.neg)


class LogQNegativesLoader(WeightedNegativesLoader):
    """`WeightedNegativesLoader` that also delivers the log proposal probability of every negative, for a `SampledSoftmax`
    criterion: same constructor, and a batch is `(*columns[b], items[b], neg[b].reshape(-1), logq[b].reshape(-1))` with `logq`
    float32, `batch_size * m` values next to the ids they belong to - so the loop body of `Experiment.train` runs against it with
    one more argument, `criterion(u, p, n, logq)`.  Every `iter()` calls `engine.negatives.weighted_unseen(..., return_weights=True)`
    once, written into the loader's `.neg` [n, m], and forms `.logq` [n, m] = log(w_j / U_j) exactly as `weighted_negatives` does -
    U_j from an int64 `cumsum`, the quotient and `log` in float64, then one cast to float32 - so under the epoch's permutation it
    equals `weighted_negatives(..., epoch=e, return_logq=True)[3].float()`.  It is the conditional probability of slot j given the
    slots before it (successive sampling), not the marginal probability that the item is among the m.  `.neg` is gathered by the
    permutation as in the other loaders and `.logq` next to it."""

    def _draw(self):
        if not self.n:
            return
        _, w, mass = engine.negatives.weighted_unseen(self.wsets, self.users, self.m, fmix(self.seed + self.epoch), return_weights=True,
                                                      out=self.neg)
        left = mass[:, None] - (torch.cumsum(w, 1) - w)                                     # U_j, exact in int64
        self.logq = torch.log(w.to(torch.float64) / left.to(torch.float64)).to(torch.float32)


# ---- shared (in-batch) negatives: no sampler, the batch's own positives (bprloss.InBatchSoftmax) ---------------------------------------
def item_logq(items: torch.Tensor, n_item: int) -> torch.Tensor:
    """The logQ table of in-batch negatives, float32 [n_item] on the tensor's device: log(count_i / T) for the T ids of `items` (the
    positives' item column; ids in [0, n_item)), the log of the chance that a row of a batch carries item i - formed in float64 from
    the exact integer counts, then cast once.  An item that never occurs gets -inf: it is never a batch column, and it MUST NOT be
    drawn as an extra under this table (a correction of -inf makes its z +inf); give drawn extras their own proposal's log
    probability, e.g. -log(n_item) for `torch.randint`.  Plain torch: it runs wherever `items` lives."""
    n_item = int(n_item)
    if items.dim() != 1 or items.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"item_logq: items must be an integer [T] tensor, got {items.dtype} {tuple(items.shape)}")
    if n_item < 1 or items.numel() < 1:
        raise ValueError(f"item_logq: n_item={n_item}, {items.numel()} ids")
    if int(items.min()) < 0 or int(items.max()) >= n_item:
        raise IndexError(f"item_logq: an item id lies outside [0, {n_item})")
    counts = torch.bincount(items.to(torch.int64), minlength=n_item)
    return torch.log(counts.to(torch.float64) / float(items.numel())).to(torch.float32)


class InBatchLoader(_EpochLoader):
    """`TripletLoader` without negatives, for an `InBatchSoftmax` criterion: the batch protocol, `columns`, `shuffle`, `drop_last` and
    `generator` are `TripletLoader`'s, and a batch is `(*columns[b], items[b])` - with `logq`, a float [n_item] table per item
    (`item_logq(items, n_item)`), followed by `logq[items[b]]` as float32, the column corrections of the batch.  The table is read
    once, at construction; every `iter()` draws one `torch.randperm` by which the id table and the corrections are gathered once
    each, and the batches are views.  Drawing extra shared negatives stays with the caller."""

    def __init__(self, users: torch.Tensor, items: torch.Tensor, columns: Sequence[torch.Tensor] = (), *, batch_size: int,
                 logq: Optional[torch.Tensor] = None, shuffle: bool = True, drop_last: bool = True,
                 generator: Optional[torch.Generator] = None):
        super().__init__("InBatchLoader", users, columns, (items,), batch_size=batch_size, shuffle=shuffle, drop_last=drop_last,
                         generator=generator)
        if logq is not None:
            if logq.dim() != 1 or not logq.is_floating_point():
                raise ValueError(f"InBatchLoader: logq must be a float [n_item] table, got {logq.dtype} {tuple(logq.shape)}")
            if logq.device != users.device:
                raise RuntimeError(f"InBatchLoader: logq is on {logq.device}, users on {users.device}")
            self.logq = logq[self.table[-1]].to(torch.float32)                  # [n]: row t's column correction
