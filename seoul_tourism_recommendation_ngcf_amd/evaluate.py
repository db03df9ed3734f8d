"""Full-catalogue evaluation of the NGCF protocol: rank every item for every user, leave out the user's training items, score the
top lists against held-out items (Recall / NDCG / precision / hit rate @K).

The reference ranks with `torch.topk(torch.mm(u, all_items_emb.T), k)` (demo.py:233-235) and computes its metrics as host-side
bookkeeping (experiment.py:66-133); here both run on the device (engine.rank_topk, engine.ranking_metrics) and the host reads one
vector back at the end.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch

from . import engine

_Sets = Union["engine.ItemSets", tuple]


def _as_sets(s, n_user: int, n_item: int, dev) -> "engine.ItemSets":
    if isinstance(s, engine.ItemSets):
        return s
    users, items = s[0], s[1]                       # (users, items[, weights]) pairs
    return engine.ItemSets.from_pairs(users.to(dev), items.to(dev), n_user, n_item)


def full_ranking(model, train: _Sets, test: _Sets, ks: Sequence[int] = (20,), year_idx: int = 0,
                 users: Optional[torch.Tensor] = None, user_chunk: int = 65536) -> dict:
    """Metrics @K for every K in `ks` of a full ranking of `users` (default: all) by `model` (an NGCF), with the items of `train`
    excluded and `test` as the truth.  `train` / `test`: engine.ItemSets (e.g. `ItemSets.from_laplacian(model.laplacian_csr(y),
    n_user)` for the training graph) or (users, items[, weights]) pairs.  The embeddings come from `model.propagate(year_idx)` in
    eval mode under no_grad; the caller's train/eval mode is restored.  Users are ranked `user_chunk` at a time against strided
    views of all_E (no copies); the host reads back once.  Returns {"recall@K": .., "ndcg@K": .., "precision@K": .., "hr@K": ..,
    "users": number of users with a non-empty test row}."""
    ks = [int(x) for x in ks]
    k = max(ks)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            model.propagate(year_idx)
            U, I = model.all_users_emb, model.all_items_emb
            dev = U.device
            n_user, n_item = int(U.shape[0]), int(I.shape[0])
            excl = _as_sets(train, n_user, n_item, dev)
            truth = _as_sets(test, n_user, n_item, dev)
            if users is None:
                users = torch.arange(n_user, device=dev, dtype=torch.int64)
            users = users.reshape(-1).to(device=dev, dtype=torch.int64)
            sums = torch.zeros(4 * len(ks) + 1, dtype=torch.float64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            for c0 in range(0, int(users.numel()), int(user_chunk)):
                ids = users[c0:c0 + int(user_chunk)]
                _, top = engine.rank_topk(U, I, k, user_ids=ids, exclude=excl, status=status)
                engine.ranking_metrics(top, truth, ks, user_ids=ids, sums=sums, status=status)
            if int(status.item()) != 0:
                raise IndexError(f"full_ranking: a user id lies outside [0, {n_user})")
            return engine.metrics_from_sums(sums, ks)
    finally:
        model.train(was_training)
