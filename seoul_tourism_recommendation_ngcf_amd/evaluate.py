"""Full-catalogue evaluation of the NGCF protocol: rank every item for every user, leave out the user's training items, score the
top lists against held-out items (Recall / NDCG / precision / hit rate @K).

The reference ranks with `torch.topk(torch.mm(u, all_items_emb.T), k)` (demo.py:233-235) and computes its metrics as host-side
bookkeeping (experiment.py:66-133); here both run on the device (engine.rank_topk, engine.ranking_metrics) and the host reads one
vector back at the end.  `full_ranks` goes past the top list: the exact position of every held-out item (engine.ranks) and MRR, MAP,
AUC and the @K metrics for any K from those positions.  `list_quality` says what the top lists are made of: coverage, Gini, entropy
and novelty of the items' exposure and the intra-list diversity (engine.lists).

The reference's own test protocol - one user against a short candidate list whose first entry is the held-out item, Test-BPR / HR@3 /
NDCG@ks / RMSE (Experiment.eval, experiment.py:66-119) - is `candidate_ranking`: one propagation per year and one launch per chunk
of cases (engine.eval_candidates) in place of a forward, a mm, two topk and five read-backs per case.
What the four share with `recommend.py` - eval mode under no_grad and the caller's mode restored, the propagate, the chunk loop, the
status word and its one read-back - is `serving.py`; each body below is what is particular to it.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch

from . import engine, serving

_Sets = Union["engine.ItemSets", tuple]


def full_ranking(model, train: _Sets, test: _Sets, ks: Sequence[int] = (20,), year_idx: int = 0,
                 users: Optional[torch.Tensor] = None, user_chunk: int = 65536, *, prefilter: Optional[str] = None,
                 pool: Optional[int] = None) -> dict:
    """Metrics @K for every K in `ks` of a full ranking of `users` (default: all) by `model` (an NGCF), with the items of `train`
    excluded and `test` as the truth.  `train` / `test`: engine.ItemSets (e.g. `ItemSets.from_laplacian(model.laplacian_csr(y),
    n_user)` for the training graph) or (users, items[, weights]) pairs.  The embeddings come from `model.propagate(year_idx)` in
    eval mode under no_grad; the caller's train/eval mode is restored.  Users are ranked `user_chunk` at a time against strided
    views of all_E (no copies); the host reads back once.  Returns {"recall@K": .., "ndcg@K": .., "precision@K": .., "hr@K": ..,
    "users": number of users with a non-empty test row}.
    `prefilter="bf16"` ranks every chunk with `engine.shortlist.rank_topk_certified` (`pool`: its shortlist size) on an item table
    packed once per call: the same top lists bit for bit, so the same dict, plus "certified", the share of the users whose
    certificate held (the others were ranked again by `rank_topk`).  It adds ONE read-back per chunk (how many users fell back).
    None is the fp32 path; any other string is a ValueError."""
    if prefilter not in (None, "bf16"):
        raise ValueError(f"full_ranking: prefilter={prefilter!r} is neither None nor 'bf16'")
    ks = [int(x) for x in ks]
    k = max(ks)
    with serving.inference(model):
        t = serving.propagated(model, year_idx)
        excl, truth = serving.as_sets(train, t), serving.as_sets(test, t)
        users = serving.ids_or_all(users, t.n_user, t.dev)
        sums = torch.zeros(4 * len(ks) + 1, dtype=torch.float64, device=t.dev)
        status = serving.status_word(t.dev)
        if prefilter is not None:
            packed = engine.shortlist.pack_items(t.I)
            n_certified = torch.zeros((), dtype=torch.int64, device=t.dev)
        for sl in serving.chunks(users.numel(), user_chunk):
            ids = users[sl]
            if prefilter is None:
                _, top = engine.rank_topk(t.U, t.I, k, user_ids=ids, exclude=excl, status=status)
            else:
                _, top, cert = engine.shortlist.rank_topk_certified(t.U, t.I, k, user_ids=ids, exclude=excl, status=status, packed=packed,
                                                                    pool=pool, return_certified=True)
                n_certified += cert.sum()
            engine.ranking_metrics(top, truth, ks, user_ids=ids, sums=sums, status=status)
        if prefilter is None:
            word, host = serving.read_back(status)[0], None
        else:
            word, host = serving.read_back(status, n_certified.reshape(1).to(torch.int32))
        if word != 0:
            raise IndexError(f"full_ranking: a user id lies outside [0, {t.n_user})")
        out = engine.metrics_from_sums(sums, ks)
        if host is not None:
            out["certified"] = int(host[0]) / max(int(users.numel()), 1)
        return out


def full_ranks(model, train: _Sets, test: _Sets, ks: Sequence[int] = (20,), year_idx: int = 0,
               users: Optional[torch.Tensor] = None, user_chunk: int = 65536, return_positions: bool = False):
    """`full_ranking` without the top list's horizon: the exact position of every held-out item of `test` among its user's eligible
    items (engine.ranks.rank_positions; the items of `train` are not eligible) and from the positions MRR, MAP, AUC, the uncut
    NDCG and the @K metrics for any K in [1, n_item] (engine.ranks.position_metrics).  Same plumbing as `full_ranking` (`serving.py`):
    `user_chunk` users per launch against strided views of all_E, one read-back at the end.  Returns {"mrr", "map", "auc", "ndcg",
    "recall@K", "ndcg@K", "precision@K", "hr@K", "users", "auc_users"}; with `return_positions` the tuple (that dict, the int32
    positions - -2 for users that were not ranked -, the truth ItemSets whose `colidx` they align with)."""
    ks = [int(x) for x in ks]
    with serving.inference(model):
        t = serving.propagated(model, year_idx)
        excl, truth = serving.as_sets(train, t), serving.as_sets(test, t)
        users = serving.ids_or_all(users, t.n_user, t.dev)
        sums = torch.zeros(4 + 4 * len(ks) + 2, dtype=torch.float64, device=t.dev)
        status = serving.status_word(t.dev)
        position = torch.full((int(truth.colidx.numel()),), engine.ranks.NOT_RANKED, dtype=torch.int32, device=t.dev)
        for sl in serving.chunks(users.numel(), user_chunk):
            ids = users[sl]
            engine.ranks.rank_positions(t.U, t.I, truth, user_ids=ids, exclude=excl, out=position, status=status)
            engine.ranks.position_metrics(position, truth, ks, t.n_item, exclude=excl, user_ids=ids, sums=sums, status=status)
        word, host = serving.read_back(status, sums)
        if word & 4:
            raise RuntimeError("full_ranks: `users` repeats users with long test rows past the workspace; use a smaller user_chunk")
        if word != 0:
            raise IndexError(f"full_ranks: a user id lies outside [0, {t.n_user}) or a held-out item outside [0, {t.n_item})")
        out = engine.ranks.position_metrics_from_sums(host, ks)
        return (out, position, truth) if return_positions else out


def list_quality(model, train: _Sets, ks: Sequence[int] = (20,), year_idx: int = 0, user_ids: Optional[torch.Tensor] = None,
                 user_chunk: int = 65536, lists: Optional[torch.Tensor] = None) -> dict:
    """What the top-K lists are made of, next to `full_ranking`'s accuracy: for every K in `ks` the catalogue coverage, the Gini
    coefficient and the entropy (bits) of the items' exposure, the novelty (mean log2(n_user / popularity) of the shown entries,
    popularity = the items' degree in `train`) and the intra-list diversity `ild` (mean cosine distance of the item pairs of a list,
    averaged over the lists with at least two entries; NaN for K > 64, the diversity kernel's limit, and when no list has two).
    The lists are `engine.rank_topk`'s for `user_ids` (default: all users) with the user's `train` items excluded, `user_chunk`
    users per launch; with `lists` (int64 [G, >= max(ks)], -1 = empty slot: e.g. `blended_ranking`'s `out_items`) they are taken as
    given and nothing is ranked.  One propagate in eval mode under no_grad, the caller's mode restored; everything is accumulated on
    the device (engine.lists) and read back once.  Returns {K: {"coverage", "gini", "entropy", "novelty", "ild", "users"}}, `users`
    = the number of lists."""
    ks = [int(x) for x in ks]
    if not ks or min(ks) < 1:
        raise ValueError(f"list_quality: cut-offs {ks}")
    div_ks = [K for K in ks if 2 <= K <= engine.lists.DIVERSITY_K_MAX]
    if len(div_ks) > engine.lists.DIVERSITY_KS_MAX:
        raise ValueError(f"list_quality: at most {engine.lists.DIVERSITY_KS_MAX} cut-offs up to {engine.lists.DIVERSITY_K_MAX}")
    k = max(ks)
    with serving.inference(model):
        t = serving.propagated(model, year_idx)
        excl = serving.as_sets(train, t)
        status = serving.status_word(t.dev)
        popularity = engine.lists.exposure_counts((excl.colidx.to(torch.int64) - excl.col_offset).reshape(-1, 1), t.n_item, status=status)
        counts = [torch.zeros(t.n_item, dtype=torch.int64, device=t.dev) for _ in ks]
        div = torch.zeros(2 * len(div_ks), dtype=torch.float64, device=t.dev)

        def add(top):
            for K, c in zip(ks, counts):
                engine.lists.exposure_counts(top, t.n_item, k=K, out=c, status=status)
            if div_ks:
                engine.lists.list_diversity(top, t.I, div_ks, sums=div, status=status)

        if lists is not None:
            lists = lists.to(device=t.dev, dtype=torch.int64)
            if lists.dim() != 2 or int(lists.shape[1]) < k:
                raise ValueError(f"list_quality: lists must be [G, >= {k}], got {tuple(lists.shape)}")
            n_lists = int(lists.shape[0])
            add(lists)
        else:
            user_ids = serving.ids_or_all(user_ids, t.n_user, t.dev)
            n_lists = int(user_ids.numel())
            for sl in serving.chunks(n_lists, user_chunk):
                _, top = engine.rank_topk(t.U, t.I, k, user_ids=user_ids[sl], exclude=excl, status=status)
                add(top)
        words = [engine.lists.exposure_summary_launch(c, popularity, t.n_user) for c in counts]
        word, host = serving.read_back(status, *words, div.view(torch.int64))        # int64 words: the fp64 sums travel as their bits
        if word != 0:
            raise IndexError(f"list_quality: a user id lies outside [0, {t.n_user}) or a list entry is not below {t.n_item}")
        means = engine.lists.diversity_from_sums(host[6 * len(ks):].view(torch.float64), div_ks) if div_ks else {}
        out = {}
        for q, K in enumerate(ks):
            fig = engine.lists.exposure_figures(host[6 * q:6 * q + 6].tolist(), t.n_item)
            out[K] = {name: fig[name] for name in ("coverage", "gini", "entropy", "novelty")}
            out[K]["ild"] = means.get(f"ild@{K}", float("nan"))
            out[K]["users"] = n_lists
        return out


def candidate_ranking(model, user_ids: torch.Tensor, candidates: torch.Tensor, *, year=None, features=None,
                      ratings: Optional[torch.Tensor] = None, criterion=None, ks: Sequence[int] = (10,), hit_k: int = 3,
                      user_repeat: Optional[int] = None, case_chunk: int = 65536, return_scores: bool = False):
    """`Experiment.eval` (experiment.py:66-119) for T test cases at once.  Case t is user `user_ids[t]` against the items
    `candidates[t, :]` ([T, C], C <= 1024), column 0 the held-out item - one batch of the reference's test_dataloader, whose u_id
    repeats the user C times and whose pos_item is the candidate list.  Returns {"bpr", "hr@<hit_k>", "ndcg@K" for K in ks, "rmse",
    "cases"}: the four values `Experiment.eval` returns (means over the cases) and the case count; with `return_scores` the tuple
    (that dict, scores [T, C] = the reference's `pred_ratings[0]` per case, position int32 [T] = the rank of the held-out item).

      year       None (Laplacian slice 0), one year, or one year per case (tensor, list or array; expected on the host - a device
                 tensor costs one more read-back, before the launches); a case uses slice `model._year_index` of its year
                 (year % 18, NGCF.py:117; while a GraphedTrainStep holds the model, the slice that step was captured for, for
                 every case).  The model propagates once per distinct slice, not once per case.
      features   (age, sex, month, day, dow), one entry per case, or None: no injection.
      ratings    [T] the held-out rating of every case ("rmse" is 0 without).
      criterion  the test BPR module; its weight_decay and batch_size enter the loss.  None: no "bpr" entry.
      user_repeat  rows of the user in the loss's regulariser: C (default - the reference's batch) or 1.
      case_chunk   cases per launch.

    The model runs in eval mode under no_grad; the caller's mode is restored.  The host reads back once, at the end; an id out of
    range (user, candidate or feature) raises IndexError then.

    One deviation from the reference's sequential loop.  The reference injects the features of case i right before case i's
    forward (NGCF.py:103-115), so case i sees the injections of cases <= i only, and with emb_ratio != 1 a user that occurs in n
    cases is blended n times.  Here every case is injected ONCE, up front, in one `engine.feature_inject` call (a user that occurs
    in several cases: the last one wins, one blend), and every case is scored against that table.  The two agree exactly whenever
    the injected rows are already in the table - with emb_ratio = 1 and features that are a function of the user id (the
    reference's data) from the second epoch on; equivalently this function equals the SECOND pass of the reference's loop over the
    same cases."""
    ks = [int(x) for x in ks]
    with serving.inference(model):
        dev = model._dev()
        user_ids = user_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        candidates = candidates.to(device=dev, dtype=torch.int64)
        T = int(user_ids.numel())
        if candidates.dim() != 2 or int(candidates.shape[0]) != T:
            raise ValueError(f"candidate_ranking: candidates must be [T = {T}, C], got {tuple(candidates.shape)}")
        C = int(candidates.shape[1])
        if ratings is not None:
            ratings = ratings.reshape(-1).to(device=dev, dtype=torch.float32)
        wd, bs = (float(criterion.weight_decay), float(criterion.batch_size)) if criterion is not None else (0.0, 1.0)
        status = serving.status_word(dev)
        if features is not None:                                       # NGCF.py:103-115, all cases at once
            if len(features) != 5:
                raise ValueError("candidate_ranking: features = (age, sex, month, day, dow)")
            model._inject_features(features, user_ids, status)         # (its keep-alive is dropped here, as before)
        # cases by Laplacian slice
        one, year_h = serving.year_slice(model, year)
        if one is not None:
            groups = [(one, None)]
        else:
            if int(year_h.numel()) != T:
                raise ValueError(f"candidate_ranking: {int(year_h.numel())} years for {T} cases")
            idx_of = {int(v): serving.year_slice(model, int(v))[0] for v in torch.unique(year_h).tolist()}
            case_idx = torch.tensor([idx_of[int(v)] for v in year_h.tolist()], dtype=torch.int64)
            groups = [(y, (case_idx == y).nonzero().flatten().to(dev)) for y in sorted(set(idx_of.values()))]
        sums = torch.zeros(len(ks) + 4, dtype=torch.float64, device=dev)
        scores = torch.empty((T, C), dtype=torch.float32, device=dev) if return_scores else None
        position = torch.empty((T,), dtype=torch.int32, device=dev) if return_scores else None
        for y, sel in groups:
            t = serving.propagated(model, y)
            uid, cand, rat = ((user_ids, candidates, ratings) if sel is None else
                              (user_ids[sel], candidates[sel], None if ratings is None else ratings[sel]))
            for sl in serving.chunks(uid.numel(), case_chunk):
                _, pos, sc = engine.eval_candidates(t.U, t.I, uid[sl], cand[sl], None if rat is None else rat[sl], ks, hit_k, wd, bs,
                                                    user_repeat, sums=sums, status=status, return_scores=return_scores,
                                                    return_position=return_scores)
                if return_scores:
                    dst = sl if sel is None else sel[sl]
                    scores[dst], position[dst] = sc, pos
        word, host = serving.read_back(status, sums)
        if word != 0:
            raise IndexError("candidate_ranking: a user id, a candidate or a feature id is out of range")
        out = engine.candidate_metrics_from_sums(host, ks, hit_k)
        if criterion is None:
            del out["bpr"]
        return (out, scores, position) if return_scores else out
