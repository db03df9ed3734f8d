"""The reference's data stage between "interactions" and "a trained, evaluated model" on the device: TourDataset._negative_sampling
(utils.py:213-275) and the DataLoader of main.py:39-42.

The reference walks the users in Python and calls `np.setxor1d` and `np.random.choice(neg_items, ng_ratio, replace=False)` once per
positive row - O(users x items) of host work before the first step.  Here one launch (engine.sample_unseen) draws the unseen items
of every row: 1 per training triplet, 24 per test case.  It is the reference's DISTRIBUTION (uniform over the user's unseen items,
without replacement), not numpy's random stream: no seed reproduces the reference's items, and every drawn value is instead a pure
function of (seed, row number, the user's seen items) that the tests recompute on the host (include/ngcf_hip.h has the formulae).
"""
from __future__ import annotations

from typing import Optional, Sequence

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


class TripletLoader:
    """A device-side iterator in the shape of the reference's `DataLoader(train_dataset, batch_size, shuffle=True, drop_last=True)`
    (main.py:39-42) over the rows of `train_triplets`.  `columns` are the caller's per-row tensors in the reference's order (year,
    u_id, age, sex, month, day, dow): a batch is `(*columns[b], items[b], neg[b])`, so the loop body of `Experiment.train` runs
    against it unchanged; without `columns` it is `(users[b], items[b], neg[b])`.  Every epoch (every `iter()`) draws one
    `torch.randperm` on the tensors' device from `generator` (None: the device's default generator), gathers all columns once into
    one int64 copy and yields its batches as views.  `len()` is the number of batches: n // batch_size with `drop_last`.  Plain
    torch: it runs wherever the tensors live."""

    def __init__(self, users: torch.Tensor, items: torch.Tensor, neg: torch.Tensor, columns: Sequence[torch.Tensor] = (), *,
                 batch_size: int, shuffle: bool = True, drop_last: bool = True, generator: Optional[torch.Generator] = None):
        cols = list(columns) if len(columns) else [users]
        cols += [items, neg]
        n = int(users.numel())
        for c in cols:
            if c.dim() != 1 or int(c.numel()) != n:
                raise ValueError(f"TripletLoader: every column must be [n = {n}], got {tuple(c.shape)}")
            if c.device != users.device:
                raise RuntimeError(f"TripletLoader: a column is on {c.device}, users on {users.device}")
        if int(batch_size) < 1:
            raise ValueError(f"TripletLoader: batch_size={batch_size}")
        self.table = torch.stack([c.to(torch.int64) for c in cols])            # [columns, n]
        self.n, self.batch_size = n, int(batch_size)
        self.shuffle, self.drop_last, self.generator = bool(shuffle), bool(drop_last), generator

    def __len__(self) -> int:
        return self.n // self.batch_size if self.drop_last else -(-self.n // self.batch_size)

    def __iter__(self):
        used = len(self) * self.batch_size if self.drop_last else self.n
        table = self.table
        if self.shuffle:
            perm = torch.randperm(self.n, generator=self.generator, device=table.device)
            table = table[:, perm[:used]]                                       # the epoch's one gathered copy
        for b0 in range(0, used, self.batch_size):
            yield tuple(table[:, b0:b0 + self.batch_size].unbind(0))
