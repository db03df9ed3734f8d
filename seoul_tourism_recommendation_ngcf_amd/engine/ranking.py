"""Ranking and evaluation on the device.  The header's section "top-k of score rows" (`topk_rows`, `recommend_topk`: csrc/ops.hip)
and, from "full-catalogue ranking and held-out metrics": the ranking with its metrics (csrc/rank.hip), the reference's
candidate-list test protocol (csrc/eval_candidates.hip) and its rank-point blending (csrc/blend.hip)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .. import _lib
from ._plumbing import (_device_view, _f32c, _on, _ptr, _require_device, _require_dtype, _require_matmul, _require_same_device,
                        _row_major_ld, _status_word, _stream, _sums_slots, _unit_inner)
from .csr import LaplacianCSR


def topk_rows(scores: torch.Tensor, k: int):
    """`torch.topk(scores, k)` for a 2-D fp32 score matrix (values, int64 indices), through ngcf_topk_rows_f32."""
    lib = _lib.load()
    _f32c(scores, "scores")
    if scores.dim() != 2:
        raise RuntimeError("topk_rows: expected a 2-D score matrix")
    n_rows, n_cols = int(scores.shape[0]), int(scores.shape[1])
    scores = _unit_inner(scores)
    vals = torch.empty((n_rows, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((n_rows, k), dtype=torch.int64, device=scores.device)
    with _on(scores.device):
        _lib.check(lib.ngcf_topk_rows_f32(_ptr(scores), _row_major_ld(scores, "scores"), n_rows, n_cols, int(k), _ptr(vals),
                                          _ptr(idx), _stream()))
    return vals, idx


def recommend_topk(u_emb: torch.Tensor, item_emb: torch.Tensor, k: int, return_scores: bool = False):
    """Scores of every item for every user row and their top-k (experiment.py:93,104-111; demo.py:233-235) in ONE launch of a
    hand-written kernel (ngcf_recommend_topk_f32): score tiles through LDS, then radix select + bitonic sort per row.
    Returns (values [B, k], int64 indices [B, k]); with `return_scores` also the [B, n_items] score matrix (what
    `torch.mm(u_emb, item_emb.T)` is in the reference)."""
    lib = _lib.load()
    _f32c(u_emb, "u_emb"), _f32c(item_emb, "item_emb")
    _require_matmul(u_emb, item_emb)
    B, D, n_items = int(u_emb.shape[0]), int(u_emb.shape[1]), int(item_emb.shape[0])
    u_emb, item_emb = _unit_inner(u_emb), _unit_inner(item_emb)
    scores = torch.empty((B, n_items), dtype=torch.float32, device=u_emb.device)
    vals = torch.empty((B, k), dtype=torch.float32, device=u_emb.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=u_emb.device)
    with _on(u_emb.device):
        _lib.check(lib.ngcf_recommend_topk_f32(_ptr(u_emb), _row_major_ld(u_emb, "u_emb"), B, _ptr(item_emb),
                                               _row_major_ld(item_emb, "item_emb"), n_items, D, int(k), _ptr(scores), n_items,
                                               _ptr(vals), _ptr(idx), _stream()))
    return (vals, idx, scores) if return_scores else (vals, idx)


# ---- full-catalogue ranking and held-out metrics (ngcf_rank_topk_f32 / ngcf_rank_metrics, csrc/rank.hip) --------------------------
RANK_K_MAX = 256


class ItemSets:
    """A sorted item list per user in CSR form - the exclusion set (train items) or the truth set (held-out items) of a full
    ranking.  `rowptr` int64 [n_rows + 1] and `colidx` int32 on the device; stored ids minus `col_offset` are item ids in
    [0, n_items).  Ids are ascending within every row (the kernels walk them with a cursor / binary search)."""

    def __init__(self, rowptr: torch.Tensor, colidx: torch.Tensor, col_offset: int, n_items: int, keep_alive=()):
        self.rowptr, self.colidx = rowptr, colidx
        self.col_offset, self.n_items = int(col_offset), int(n_items)
        self.n_rows = int(rowptr.numel()) - 1
        self._keep = keep_alive

    @classmethod
    def from_pairs(cls, users: torch.Tensor, items: torch.Tensor, n_user: int, n_item: int) -> "ItemSets":
        """From (user, item) pairs in any order, duplicates allowed: a sort and unique on the pairs' device (set-up, not hot path)."""
        users = users.reshape(-1).to(torch.int64)
        items = items.reshape(-1).to(device=users.device, dtype=torch.int64)
        if users.numel() != items.numel():
            raise RuntimeError("ItemSets.from_pairs: users and items differ in length")
        if users.numel() and (int(users.min()) < 0 or int(users.max()) >= n_user or int(items.min()) < 0 or int(items.max()) >= n_item):
            raise IndexError(f"ItemSets.from_pairs: a pair lies outside {n_user} users x {n_item} items")
        key = torch.unique(users * n_item + items)                   # sorted by (user, item), de-duplicated
        u, i = key // n_item, key % n_item
        rowptr = torch.zeros(n_user + 1, dtype=torch.int64, device=users.device)
        rowptr[1:] = torch.cumsum(torch.bincount(u, minlength=n_user), 0)
        return cls(rowptr, i.to(torch.int32).contiguous(), 0, n_item)

    @classmethod
    def from_laplacian(cls, csr: LaplacianCSR, n_user: int) -> "ItemSets":
        """The user rows of a model's Laplacian CSR (`model.laplacian_csr(year)`): row u holds columns n_user + item, so with
        col_offset = n_user they are the user's training items, borrowed with no copy.  The CSR's column array is never
        reordered after it is built (the swept plan keeps its own arrays), so the check below holds for the CSR's life."""
        lib = _lib.load()
        n_item = csr.n_cols - n_user
        if csr.n_rows < n_user or n_item < 1:
            raise RuntimeError(f"ItemSets.from_laplacian: a CSR of {csr.n_rows} x {csr.n_cols} has no {n_user} user rows")
        rp_ptr, ci_ptr = int(lib.ngcf_csr_rowptr(csr._h) or 0), int(lib.ngcf_csr_colidx(csr._h) or 0)
        rowptr_all = _device_view(rp_ptr, csr.n_rows + 1, torch.int64)
        nnz_user = int(rowptr_all[n_user])
        rowptr = rowptr_all[:n_user + 1]
        colidx = _device_view(ci_ptr, max(nnz_user, 1), torch.int32)[:nnz_user]
        if nnz_user > 1:
            row_of = torch.repeat_interleave(torch.arange(n_user, device=rowptr.device), rowptr.diff())
            same_row = row_of[1:] == row_of[:-1]
            if bool((same_row & (colidx[1:] < colidx[:-1])).any()):
                raise RuntimeError("ItemSets.from_laplacian: the CSR's columns are not ascending within its user rows")
        return cls(rowptr, colidx, n_user, n_item, keep_alive=(csr,))


def _check_sets(s: "ItemSets", dev, n_user_rows: int, what: str):
    if s.rowptr.device != dev or s.colidx.device != dev:
        raise RuntimeError(f"{what}: the item sets live on {s.rowptr.device}, the embeddings on {dev}")
    if s.n_rows < n_user_rows:
        raise RuntimeError(f"{what}: {s.n_rows} rows of item sets for {n_user_rows} users")


def rank_topk(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, user_ids: Optional[torch.Tensor] = None,
              exclude: Optional[ItemSets] = None, status: Optional[torch.Tensor] = None):
    """Top-k items of every item for every requested user, without a score matrix (ngcf_rank_topk_f32): fp32 MFMA scores with
    the bits of `recommend_topk`, a streaming selection per user, the user's `exclude` items left out.  With `user_ids`, batch row b
    ranks user_emb[user_ids[b]] (no gather); otherwise row b.  Returns (values [B, k], int64 indices [B, k]); slots past the
    eligible items are (-inf, -1).  Strided views (rows of all_E) are taken as they are.  A user id outside the table raises
    IndexError (one host sync); with a caller's int32 `status` word it is only flagged there and the call does not sync."""
    lib = _lib.load()
    _f32c(user_emb, "user_emb"), _f32c(item_emb, "item_emb")
    _require_matmul(user_emb, item_emb)
    n_rows, D, n_items = int(user_emb.shape[0]), int(user_emb.shape[1]), int(item_emb.shape[0])
    k = int(k)
    if k < 1 or k > n_items:
        raise RuntimeError(f"selected index k out of range (k={k}, row length {n_items})")
    if k > RANK_K_MAX:
        raise RuntimeError(f"rank_topk: k={k} > {RANK_K_MAX} is not supported; recommend_topk takes k up to 1024")
    dev = user_emb.device
    user_emb, item_emb = _unit_inner(user_emb), _unit_inner(item_emb)
    if user_ids is not None:
        user_ids = user_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        B = int(user_ids.numel())
    else:
        B = n_rows
    if exclude is not None:
        _check_sets(exclude, dev, n_rows, "rank_topk")
        if exclude.n_items != n_items:
            raise RuntimeError(f"rank_topk: the exclusion sets index {exclude.n_items} items, the item table has {n_items}")
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    idx = torch.empty((B, k), dtype=torch.int64, device=dev)
    if B == 0:
        return vals, idx
    nb = int(lib.ngcf_rank_workspace_bytes(B, n_items, D, k))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    status, check_status = _status_word("rank_topk", status, dev)
    with _on(dev):
        _lib.check(lib.ngcf_rank_topk_f32(_ptr(user_emb), _row_major_ld(user_emb, "user_emb"), _ptr(user_ids), n_rows, B,
                                          _ptr(item_emb), _row_major_ld(item_emb, "item_emb"), n_items, D, k,
                                          _ptr(None if exclude is None else exclude.rowptr),
                                          _ptr(None if exclude is None else exclude.colidx),
                                          0 if exclude is None else exclude.col_offset, _ptr(vals), _ptr(idx), _ptr(status),
                                          _ptr(ws), nb, _stream()))
    if check_status and user_ids is not None and int(status.item()) != 0:
        raise IndexError(f"rank_topk: a user id lies outside [0, {n_rows})")
    return vals, idx


def ranking_metrics(top_idx: torch.Tensor, truth: ItemSets, ks: Sequence[int], user_ids: Optional[torch.Tensor] = None,
                    sums: Optional[torch.Tensor] = None, per_user: bool = False, status: Optional[torch.Tensor] = None):
    """Recall / NDCG / precision / hit rate @K of top lists `top_idx` [B, k] (int64, -1 = empty slot) against `truth`
    (ngcf_rank_metrics).  Batch row b is user user_ids[b] (or b).  Users with an empty truth row are not evaluated.
    Returns {"recall@K": mean, "ndcg@K": ..., "precision@K": ..., "hr@K": ..., "users": n}.  With `sums` (a float64 device
    tensor of 4*len(ks) + 1 slots) the call adds into it and returns it instead - chunks of one ranking read back once."""
    lib = _lib.load()
    _require_device(top_idx, "top_idx")
    if top_idx.dim() != 2 or top_idx.dtype != torch.int64:
        raise RuntimeError("ranking_metrics: top_idx must be a 2-D int64 tensor")
    ks = [int(x) for x in ks]
    B, k = int(top_idx.shape[0]), int(top_idx.shape[1])
    if not ks or len(ks) > 8 or min(ks) < 1 or max(ks) > k:
        raise RuntimeError(f"ranking_metrics: between 1 and 8 cut-offs in [1, {k}], got {ks}")
    dev = top_idx.device
    top_idx = top_idx.contiguous()
    _check_sets(truth, dev, 0, "ranking_metrics")
    if user_ids is not None:
        user_ids = user_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        if int(user_ids.numel()) != B:
            raise RuntimeError("ranking_metrics: user_ids and top_idx differ in length")
    elif truth.n_rows < B:
        raise RuntimeError(f"ranking_metrics: {truth.n_rows} truth rows for {B} users")
    n_slots = 4 * len(ks) + 1
    own = sums is None
    sums = _sums_slots("ranking_metrics", sums, n_slots, dev, RuntimeError)
    pu = torch.empty((B, 4 * len(ks)), dtype=torch.float32, device=dev) if per_user else None
    status, check_status = _status_word("ranking_metrics", status, dev)
    ks_arr = (C.c_int32 * len(ks))(*ks)
    with _on(dev):
        _lib.check(lib.ngcf_rank_metrics(_ptr(top_idx), B, k, _ptr(user_ids), truth.n_rows, _ptr(truth.rowptr), _ptr(truth.colidx),
                                         truth.col_offset, ks_arr, len(ks), _ptr(pu), _ptr(sums), _ptr(status), _stream()))
    if check_status and user_ids is not None and int(status.item()) != 0:
        raise IndexError(f"ranking_metrics: a user id lies outside [0, {truth.n_rows})")
    if not own:
        return (sums, pu) if per_user else sums
    out = metrics_from_sums(sums, ks)
    return (out, pu) if per_user else out


def metrics_from_sums(sums: torch.Tensor, ks: Sequence[int]) -> dict:
    """The means of a `ranking_metrics` slot vector (one read-back)."""
    s = sums.double().cpu().tolist()
    n = int(round(s[-1]))
    out = {}
    for q, K in enumerate(ks):
        for j, name in enumerate(("recall", "ndcg", "precision", "hr")):
            out[f"{name}@{K}"] = s[4 * q + j] / n if n else 0.0
    out["users"] = n
    return out


# ---- candidate-list evaluation, the reference's test protocol (ngcf_eval_candidates_f32, csrc/eval_candidates.hip) ----------------
CAND_MAX = 1024


def _cand_cutoffs(ks: Sequence[int], hit_k: int, C: int):
    ks, hit_k = [int(x) for x in ks], int(hit_k)
    if len(ks) > 8:
        raise ValueError(f"eval_candidates: at most 8 NDCG cut-offs, got {len(ks)}")
    for k in ks + [hit_k]:
        if k < 1 or k > C:
            raise RuntimeError(f"selected index k out of range (k={k}, row length {C})")
    return ks, hit_k


def eval_candidates(user_emb: torch.Tensor, item_emb: torch.Tensor, user_ids: torch.Tensor, candidates: torch.Tensor,
                    ratings: Optional[torch.Tensor] = None, ks: Sequence[int] = (10,), hit_k: int = 3, weight_decay: float = 0.0,
                    batch_size: float = 1.0, user_repeat: Optional[int] = None, sums: Optional[torch.Tensor] = None,
                    status: Optional[torch.Tensor] = None, return_scores: bool = False, return_position: bool = True):
    """The reference's test protocol (experiment.py:92-116) for T cases x C candidates in one launch (ngcf_eval_candidates_f32):
    case t scores user_emb[user_ids[t]] against item_emb[candidates[t, :]], column 0 the held-out item.  `user_ids` int64 [T],
    `candidates` int64 [T, C] (C <= 1024), `ratings` float32 [T] or None, all on the embeddings' device; strided views (rows of
    all_E) are taken as they are.  Adds [hits@hit_k, ndcg@ks.., bpr sum, |s_0 - rating| sum, cases] into `sums` (float64,
    len(ks) + 4 slots; a fresh one if None) in a fixed order - see `candidate_metrics_from_sums`.  `user_repeat` (1 or C, default C)
    is how often the user row counts in the BPR regulariser.  Returns (sums, position int32 [T] or None, scores [T, C] or None);
    position = the number of candidates that sort above column 0 (ties: column 0 wins), -1 for a case with an id out of range.
    Such a case adds nothing; it raises IndexError (one host sync), or with a caller's int32 `status` word is only flagged there."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    _require_matmul(user_emb, item_emb)
    _require_dtype("eval_candidates", torch.int64, (("user_ids", user_ids), ("candidates", candidates)))
    if user_ids.dim() != 1 or candidates.dim() != 2 or candidates.shape[0] != user_ids.shape[0]:
        raise ValueError(f"eval_candidates: user_ids [T] and candidates [T, C] expected, got {tuple(user_ids.shape)} and {tuple(candidates.shape)}")
    T, n_cand = int(candidates.shape[0]), int(candidates.shape[1])
    if n_cand < 1 or n_cand > CAND_MAX:
        raise ValueError(f"eval_candidates: C={n_cand} candidates per case outside [1, {CAND_MAX}]")
    ks, hit_k = _cand_cutoffs(ks, hit_k, n_cand)
    user_repeat = n_cand if user_repeat is None else int(user_repeat)
    if user_repeat not in (1, n_cand):
        raise ValueError(f"eval_candidates: user_repeat={user_repeat} is neither 1 nor C={n_cand}")
    if float(batch_size) == 0.0:
        raise ValueError("eval_candidates: batch_size must not be 0")
    if ratings is not None and (ratings.dim() != 1 or int(ratings.numel()) != T):
        raise ValueError(f"eval_candidates: {tuple(ratings.shape)} ratings for {T} cases")
    _f32c(user_emb, "user_emb"), _f32c(item_emb, "item_emb")
    dev = user_emb.device
    if ratings is not None:
        ratings = _f32c(ratings, "ratings").contiguous()
    _require_same_device("eval_candidates", (("user_ids", user_ids), ("candidates", candidates), ("ratings", ratings)),
                         "the embeddings", dev)
    user_emb, item_emb, candidates = _unit_inner(user_emb), _unit_inner(item_emb), _unit_inner(candidates)
    user_ids = user_ids.contiguous()
    sums = _sums_slots("eval_candidates", sums, len(ks) + 4, dev)
    status, check_status = _status_word("eval_candidates", status, dev)
    scores = torch.empty((T, n_cand), dtype=torch.float32, device=dev) if return_scores else None
    position = torch.empty((T,), dtype=torch.int32, device=dev) if return_position else None
    ks_arr = (C.c_int32 * max(len(ks), 1))(*ks)
    with _on(dev):
        _lib.check(lib.ngcf_eval_candidates_f32(
            _ptr(user_emb), _row_major_ld(user_emb, "user_emb"), int(user_emb.shape[0]), _ptr(item_emb),
            _row_major_ld(item_emb, "item_emb"), int(item_emb.shape[0]), int(user_emb.shape[1]), _ptr(user_ids), _ptr(candidates),
            _row_major_ld(candidates, "candidates"), T, n_cand, _ptr(ratings), ks_arr, len(ks), hit_k, float(weight_decay),
            float(batch_size), user_repeat, _ptr(scores), _ptr(position), _ptr(sums), _ptr(status), _stream()))
    if check_status and int(status.item()) != 0:
        raise IndexError(f"eval_candidates: a user id lies outside [0, {int(user_emb.shape[0])}) or a candidate outside "
                         f"[0, {int(item_emb.shape[0])})")
    return sums, position, scores


def candidate_metrics_from_sums(sums, ks: Sequence[int], hit_k: int = 3) -> dict:
    """The means of an `eval_candidates` slot vector [hits, ndcg@ks.., bpr, abs_err, cases] (one read-back): {"bpr", "hr@<hit_k>",
    "ndcg@K".., "rmse", "cases"}, every entry its sum over `cases` - the reference's mean over len(test_dataloader),
    experiment.py:119 ("rmse" is the mean of the per-case sqrt(MSE) of two scalars, i.e. of |s_0 - rating|)."""
    ks = [int(x) for x in ks]
    s = torch.as_tensor(sums).double().cpu().tolist()
    if len(s) != len(ks) + 4:
        raise ValueError(f"candidate_metrics_from_sums: {len(s)} slots for {len(ks)} cut-offs ({len(ks) + 4} expected)")
    n = int(round(s[-1]))
    mean = lambda x: x / n if n else 0.0   # noqa: E731
    out = {"bpr": mean(s[len(ks) + 1]), f"hr@{int(hit_k)}": mean(s[0])}
    for q, K in enumerate(ks):
        out[f"ndcg@{K}"] = mean(s[1 + q])
    out["rmse"] = mean(s[len(ks) + 2])
    out["cases"] = n
    return out


# ---- rank-point blending, the reference's recommender after its topk (ngcf_blend_points, csrc/blend.hip) ---------------------------
BLEND_TOP_MAX = 256
BLEND_POINTS_MAX = 1024


def blend_points(pref: torch.Tensor, col_rowptr: torch.Tensor, col_rows: torch.Tensor, n_items: int, *, points: int = 100,
                 weights: Sequence[float] = (1.0, 0.0, 0.0), con: Optional[torch.Tensor] = None,
                 con_slot: Optional[torch.Tensor] = None, dis: Optional[torch.Tensor] = None,
                 dis_slot: Optional[torch.Tensor] = None, item_mask: Optional[torch.Tensor] = None, top: int = 10,
                 tile_items: int = 0, return_table: bool = False, status: Optional[torch.Tensor] = None):
    """The rank-point blending of demo.py:285-292, 315-334, 378-398 for R request rows in G columns in one launch
    (ngcf_blend_points).  `pref` int64 [R, Pl]: the preference list of every request row, best first (`rank_topk`'s indices; -1 =
    empty slot); `con` int64 [S_con, Pl] with `con_slot` int64 [R] (the list of row r is con[con_slot[r]]) and `dis` / `dis_slot`
    likewise, or None for no points of that kind (`topk_rows(-values, Pl)`'s indices).  Position j of a list is worth `points` - j.
    Column g is the set of rows col_rows[col_rowptr[g]:col_rowptr[g + 1]] (int64 CSR).  Per column and item the three kinds of
    points are summed over the rows (int32, exact) and rating = (sp * w_pref + sc * w_con) + sd * w_dis in fp64 without FMA - the
    bits numpy gives.  Returns (items int64 [G, top], rating float64 [G, top]): per column the best `top` items with
    `item_mask[i] != 0` (uint8 / bool [n_items], None: all), rating descending, ties lowest item first, (-1, -inf) past the
    eligible items; with `return_table` also the dense float64 [G, n_items] ratings (tests and small catalogues only).  The result
    does not depend on `tile_items` (items per workgroup, 0 = default).  An id out of range (row index, slot, list entry, column
    range) adds nothing and raises IndexError (one host sync); with a caller's int32 `status` word it is only flagged there."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    top, points, n_items, tile_items = int(top), int(points), int(n_items), int(tile_items)
    if top < 1 or top > BLEND_TOP_MAX:
        raise ValueError(f"blend_points: top={top} outside [1, {BLEND_TOP_MAX}]")
    if points < 1 or points > BLEND_POINTS_MAX:
        raise ValueError(f"blend_points: points={points} outside [1, {BLEND_POINTS_MAX}]")
    if n_items < 1 or n_items >= 2 ** 31:
        raise ValueError(f"blend_points: n_items={n_items} outside [1, 2^31)")
    if len(weights) != 3:
        raise ValueError("blend_points: weights = (w_pref, w_con, w_dis)")
    if (con is None) != (con_slot is None) or (dis is None) != (dis_slot is None):
        raise ValueError("blend_points: a context list table and its slot vector come together")
    ints = (("pref", pref), ("col_rowptr", col_rowptr), ("col_rows", col_rows), ("con", con), ("con_slot", con_slot), ("dis", dis),
            ("dis_slot", dis_slot))
    _require_dtype("blend_points", torch.int64, ints)
    if item_mask is not None and item_mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"blend_points: item_mask must be uint8 or bool, got {item_mask.dtype}")
    if pref.dim() != 2 or pref.shape[1] < 1 or pref.shape[1] > points:
        raise ValueError(f"blend_points: pref must be [R, Pl] with 1 <= Pl <= points = {points}, got {tuple(pref.shape)}")
    R, Pl = int(pref.shape[0]), int(pref.shape[1])
    if R * points >= 2 ** 31:
        raise ValueError(f"blend_points: R * points = {R} * {points} >= 2^31: the int32 point sums could overflow")
    for nm, lists, slot in (("con", con, con_slot), ("dis", dis, dis_slot)):
        if lists is not None and (lists.dim() != 2 or int(lists.shape[1]) != Pl):
            raise ValueError(f"blend_points: {nm} must be [S, Pl = {Pl}], got {tuple(lists.shape)}")
        if slot is not None and (slot.dim() != 1 or int(slot.numel()) != R):
            raise ValueError(f"blend_points: {nm}_slot must be [R = {R}], got {tuple(slot.shape)}")
    if col_rowptr.dim() != 1 or col_rowptr.numel() < 1 or col_rows.dim() != 1:
        raise ValueError(f"blend_points: col_rowptr [G + 1] and col_rows [nnz] expected, got {tuple(col_rowptr.shape)} and {tuple(col_rows.shape)}")
    if item_mask is not None and (item_mask.dim() != 1 or int(item_mask.numel()) != n_items):
        raise ValueError(f"blend_points: item_mask must be [n_items = {n_items}], got {tuple(item_mask.shape)}")
    G = int(col_rowptr.numel()) - 1
    nb = int(lib.ngcf_blend_workspace_bytes(G, n_items, top, tile_items))
    if nb < 0:
        raise ValueError(f"blend_points: tile_items={tile_items} outside [0, 4096] or too many tiles for {G} columns")
    _require_device(pref, "pref")
    dev = pref.device
    _require_same_device("blend_points", ints + (("item_mask", item_mask),), "pref", dev)
    status, check_status = _status_word("blend_points", status, dev)
    pref, con, dis = _unit_inner(pref), _unit_inner(con), _unit_inner(dis)
    con_slot = None if con_slot is None else con_slot.contiguous()
    dis_slot = None if dis_slot is None else dis_slot.contiguous()
    col_rowptr, col_rows = col_rowptr.contiguous(), col_rows.contiguous()
    if item_mask is not None:
        item_mask = item_mask.contiguous().view(torch.uint8)
    items = torch.empty((G, top), dtype=torch.int64, device=dev)
    rating = torch.empty((G, top), dtype=torch.float64, device=dev)
    table = torch.empty((G, n_items), dtype=torch.float64, device=dev) if return_table else None
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    ld = lambda t, nm: 0 if t is None else _row_major_ld(t, nm)   # noqa: E731
    with _on(dev):
        _lib.check(lib.ngcf_blend_points(
            _ptr(pref), ld(pref, "pref"), R, Pl, _ptr(con), ld(con, "con"), 0 if con is None else int(con.shape[0]), _ptr(con_slot),
            _ptr(dis), ld(dis, "dis"), 0 if dis is None else int(dis.shape[0]), _ptr(dis_slot), _ptr(col_rowptr), _ptr(col_rows),
            int(col_rows.numel()), G, points, n_items, float(weights[0]), float(weights[1]), float(weights[2]), _ptr(item_mask), top,
            tile_items, _ptr(items), _ptr(rating), _ptr(table), _ptr(status), _ptr(ws), nb, _stream()))
    if check_status and int(status.item()) != 0:
        raise IndexError(f"blend_points: a row index lies outside [0, {R}), a slot outside its table, a list entry outside "
                         f"[0, {n_items}) or a column range outside col_rows")
    return (items, rating, table) if return_table else (items, rating)
