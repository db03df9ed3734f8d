"""Beyond-accuracy figures of top lists (the header's section "beyond-accuracy figures of top lists", csrc/list_quality.hip): how
often every item is shown, what that exposure histogram looks like (coverage, Gini, entropy, novelty) and how different the items
within one list are (intra-list diversity).  A list is a row of an int64 `top_idx` - `rank_topk`'s indices, `blend_points`'
`out_items`, or a column slice of either -, negative entries are empty slots.  And what changes those figures: `mmr_rerank`, the
greedy diversifying re-rank of a pool of candidates (the header's section "diversified top lists", csrc/list_rerank.hip).  Reached
as `engine.lists.<name>`."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction
from typing import Optional, Sequence

import torch

from .. import _lib
from ._plumbing import _f32c, _on, _ptr, _require_device, _require_dtype, _require_same_device, _row_major_ld, _status_word, _stream, _sums_slots, _unit_inner

EXPOSURE_LDS_ITEMS = 16384     # NGCF_EXPOSURE_LDS_ITEMS: catalogues up to this size are counted in LDS tables
DIVERSITY_K_MAX = 64           # NGCF_LIST_DIV_K_MAX: the largest cut-off of list_diversity
DIVERSITY_KS_MAX = 8
MMR_POOL_MAX = 64              # NGCF_LIST_MMR_POOL_MAX: the largest pool of mmr_rerank
SUMMARY_OVERFLOW, SUMMARY_NEGATIVE = 1, 2     # the status bits of exposure_summary_launch's fourth word
_FIGURES = ("coverage", "gini", "entropy", "novelty")


def _lists(fn: str, top_idx: torch.Tensor, k: Optional[int]):
    """The k of an int64 [B, >= k] list tensor; shape and type checks only."""
    if top_idx.dtype != torch.int64:
        raise TypeError(f"{fn}: top_idx must be int64, got {top_idx.dtype}")
    if top_idx.dim() != 2:
        raise ValueError(f"{fn}: top_idx must be [B, k], got {tuple(top_idx.shape)}")
    width = int(top_idx.shape[1])
    k = width if k is None else int(k)
    if k < 1 or k > width:
        raise ValueError(f"{fn}: k={k} outside [1, {width}], the width of top_idx")
    return k


def _raise_bad_id(fn: str, word: int, n_items: int):
    if word & 1:
        raise IndexError(f"{fn}: a list entry is not below n_items = {n_items} (negative entries are empty slots)")


def exposure_counts(top_idx: torch.Tensor, n_items: int, k: Optional[int] = None, out: Optional[torch.Tensor] = None,
                    status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """How often every item is shown (ngcf_list_exposure): int64 [n_items], counts[i] = the number of entries equal to i in columns
    [0, k) of all rows of `top_idx` (k = None: every column).  The call ADDS into `out`, so a user set is counted in chunks into one
    tensor.  Integer atomics only: identical from run to run, and the same below and above EXPOSURE_LDS_ITEMS items (LDS tables /
    atomics in memory).  An entry >= n_items raises IndexError after the call's one read-back - the other counts are complete by
    then -; with a caller's int32 `status` word it is only flagged there (bit 0) and the call does not sync."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    k = _lists("exposure_counts", top_idx, k)
    n_items = int(n_items)
    if n_items < 1 or n_items >= 2 ** 31:
        raise ValueError(f"exposure_counts: n_items={n_items} outside [1, 2^31)")
    if out is not None and (out.dtype != torch.int64 or out.dim() != 1 or int(out.numel()) != n_items or not out.is_contiguous()):
        raise ValueError(f"exposure_counts: out must be a contiguous int64 tensor of {n_items} entries")
    _require_device(top_idx, "top_idx")
    dev = top_idx.device
    _require_same_device("exposure_counts", (("out", out),), "top_idx", dev)
    status, check_status = _status_word("exposure_counts", status, dev)
    if top_idx.stride(1) != 1:
        top_idx = top_idx.contiguous()
    if out is None:
        out = torch.zeros(n_items, dtype=torch.int64, device=dev)
    B = int(top_idx.shape[0])
    if B == 0:
        return out
    with _on(dev):
        _lib.check(lib.ngcf_list_exposure(_ptr(top_idx), _row_major_ld(top_idx, "top_idx"), B, k, n_items, _ptr(out), _ptr(status),
                                          _stream()))
    if check_status:
        _raise_bad_id("exposure_counts", int(status.item()), n_items)
    return out


def exposure_summary_launch(counts: torch.Tensor, popularity: Optional[torch.Tensor] = None, n_user: Optional[int] = None) -> torch.Tensor:
    """The device half of `exposure_summary` (one library sort, then ngcf_exposure_summary): an int64 [6] device tensor
    [covered, total, weighted, status, bits of clog, bits of nov] for `exposure_figures`; no read-back."""
    lib = _lib.load()
    _require_dtype("exposure_summary", torch.int64, (("counts", counts), ("popularity", popularity)))
    if counts.dim() != 1 or int(counts.numel()) < 1 or int(counts.numel()) >= 2 ** 31:
        raise ValueError(f"exposure_summary: counts must be [n_items] with 1 <= n_items < 2^31, got {tuple(counts.shape)}")
    n_items = int(counts.numel())
    if popularity is not None:
        if popularity.dim() != 1 or int(popularity.numel()) != n_items:
            raise ValueError(f"exposure_summary: popularity must be [n_items = {n_items}], got {tuple(popularity.shape)}")
        if n_user is None or int(n_user) < 1:
            raise ValueError("exposure_summary: popularity needs n_user >= 1")
    _require_device(counts, "counts")
    dev = counts.device
    _require_same_device("exposure_summary", (("popularity", popularity),), "counts", dev)
    counts = counts.contiguous()
    popularity = None if popularity is None else popularity.contiguous()
    ordered = torch.sort(counts).values
    out = torch.zeros(6, dtype=torch.int64, device=dev)
    with _on(dev):
        _lib.check(lib.ngcf_exposure_summary(_ptr(ordered), _ptr(None if popularity is None else counts), _ptr(popularity), n_items,
                                             0 if popularity is None else int(n_user), _ptr(out), _stream()))
    return out


def exposure_figures(six, n_items: int, with_novelty: bool = True) -> dict:
    """The figures of a histogram from the six host words of `exposure_summary_launch`: {"coverage", "gini", "entropy", "novelty",
    "covered", "total", "weighted", "clog", "nov"}.  The Gini coefficient is formed from the exact integers as a fraction and rounded
    once; `total` = 0 leaves every figure NaN.  RuntimeError for a negative count, OverflowError where n_items * total >= 2^62."""
    covered, total, weighted, word = (int(x) for x in six[:4])
    clog, nov = (float(x) for x in torch.as_tensor([int(six[4]), int(six[5])], dtype=torch.int64).view(torch.float64).tolist())
    if word & SUMMARY_NEGATIVE:
        raise RuntimeError("exposure_summary: a count is negative")
    if word & SUMMARY_OVERFLOW:
        raise OverflowError(f"exposure_summary: n_items * total = {n_items} * {total} >= 2^62, the weighted sum is not computed")
    n = int(n_items)
    res = {"covered": covered, "total": total, "weighted": weighted, "clog": clog, "nov": nov}
    if total == 0:
        res.update({name: math.nan for name in _FIGURES})
        return res
    res["coverage"] = covered / n
    res["gini"] = float(Fraction(2 * weighted, n * total) - Fraction(n + 1, n))
    res["entropy"] = math.log2(total) - clog / total
    res["novelty"] = nov / total if with_novelty else math.nan
    return res


def exposure_summary(counts: torch.Tensor, popularity: Optional[torch.Tensor] = None, n_user: Optional[int] = None) -> dict:
    """Coverage, Gini, entropy and novelty of an exposure histogram `counts` (int64 [n_items], `exposure_counts`' result) in one small
    read-back.  coverage = the share of items shown at all; gini = the concentration of the exposure, 0 for a uniform histogram,
    (n - 1) / n for a single item; entropy = log2(total) - (sum c log2 c) / total, in bits; novelty = the mean self-information
    log2(n_user / max(popularity_i, 1)) of the shown entries, with `popularity` int64 [n_items] (e.g. the items' degree in the training
    set) and `n_user`, NaN without.  The integers behind the figures are exact, the two fp64 sums are added in a fixed tree with a
    correctly rounded log2 (the header): identical from run to run.  The dict also carries the five reduced numbers."""
    six = exposure_summary_launch(counts, popularity, n_user).cpu().tolist()
    return exposure_figures(six, int(counts.numel()), popularity is not None)


def _cutoffs(ks: Sequence[int], k: int):
    ks = [int(x) for x in ks]
    if not 1 <= len(ks) <= DIVERSITY_KS_MAX:
        raise ValueError(f"list_diversity: between 1 and {DIVERSITY_KS_MAX} cut-offs, got {len(ks)}")
    for K in ks:
        if K < 2 or K > DIVERSITY_K_MAX:
            raise ValueError(f"list_diversity: cut-off K={K} outside [2, {DIVERSITY_K_MAX}]")
        if K > k:
            raise ValueError(f"list_diversity: cut-off K={K} above the list length k={k}")
    return ks


def list_diversity(top_idx: torch.Tensor, item_emb: torch.Tensor, ks: Sequence[int], per_user: bool = False,
                   sums: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """Intra-list diversity @K (ngcf_list_diversity_f32): the mean cosine distance 1 - cos(e_a, e_b) over the pairs of non-empty
    slots in the first K columns of a list, for up to 8 cut-offs 2 <= K <= min(k, 64) from one pass over the lists' Gram matrices
    (fp32 MFMA with `rank_topk`'s score bits, cosines and sums in fp64 in the order the header states).  `item_emb` [n_items, D]
    float32 with unit inner stride (a row range or column slice of a table works).  A list with fewer than 2 non-empty slots below K
    is not evaluated at K.  Returns {"ild@K": mean over the evaluated lists (NaN if none), "lists@K": their number}; with `sums` (a
    float64 device tensor of 2*len(ks) slots = [sum of ild@K per K, lists counted per K]) the call adds into it and returns it
    instead - chunks of one ranking read back once, `diversity_from_sums`.  With `per_user` also the float64 [B, len(ks)] per-list
    values (0 where a list is not evaluated).  An entry >= n_items raises IndexError after the read-back, or is flagged in a caller's
    `status` word (bit 0)."""
    lib = _lib.load()
    # shapes, types and limits first (they hold on any device), then where the tensors live
    k = _lists("list_diversity", top_idx, None)
    ks = _cutoffs(ks, k)
    if item_emb.dtype != torch.float32:
        raise TypeError(f"list_diversity: item_emb must be float32, got {item_emb.dtype}")
    if item_emb.dim() != 2 or int(item_emb.shape[0]) < 1 or int(item_emb.shape[1]) < 1 or int(item_emb.shape[0]) >= 2 ** 31:
        raise ValueError(f"list_diversity: item_emb must be [n_items, D], got {tuple(item_emb.shape)}")
    _f32c(item_emb, "item_emb")
    dev = item_emb.device
    _require_same_device("list_diversity", (("top_idx", top_idx),), "item_emb", dev)
    own = sums is None
    sums = _sums_slots("list_diversity", sums, 2 * len(ks), dev)
    status, check_status = _status_word("list_diversity", status, dev)
    if top_idx.stride(1) != 1:
        top_idx = top_idx.contiguous()
    if item_emb.stride(1) != 1:
        item_emb = item_emb.contiguous()
    B, n_items, D = int(top_idx.shape[0]), int(item_emb.shape[0]), int(item_emb.shape[1])
    pu = torch.zeros((B, len(ks)), dtype=torch.float64, device=dev) if per_user else None
    if B > 0:
        ks_arr = (C.c_int32 * len(ks))(*ks)
        with _on(dev):
            _lib.check(lib.ngcf_list_diversity_f32(_ptr(top_idx), _row_major_ld(top_idx, "top_idx"), B, k, _ptr(item_emb),
                                                   _row_major_ld(item_emb, "item_emb"), n_items, D, ks_arr, len(ks), _ptr(pu), _ptr(sums),
                                                   _ptr(status), _stream()))
    if check_status:
        _raise_bad_id("list_diversity", int(status.item()), n_items)
    if not own:
        return (sums, pu) if per_user else sums
    res = diversity_from_sums(sums, ks)
    return (res, pu) if per_user else res


def diversity_from_sums(sums, ks: Sequence[int]) -> dict:
    """The means of a `list_diversity` slot vector (one read-back): {"ild@K", "lists@K"}."""
    ks = [int(x) for x in ks]
    s = torch.as_tensor(sums).double().cpu().tolist()
    if len(s) != 2 * len(ks):
        raise ValueError(f"diversity_from_sums: {len(s)} slots for {len(ks)} cut-offs ({2 * len(ks)} expected)")
    out = {}
    for q, K in enumerate(ks):
        n = int(round(s[len(ks) + q]))
        out[f"ild@{K}"] = s[q] / n if n else math.nan
        out[f"lists@{K}"] = n
    return out


def mmr_rerank(pool_idx: torch.Tensor, relevance: torch.Tensor, item_emb: torch.Tensor, top: int, lam: float = 0.7,
               normalize: bool = True, return_slots: bool = False, return_keys: bool = False,
               status: Optional[torch.Tensor] = None):
    """Diversified top lists (ngcf_list_mmr_f32): greedy Maximal Marginal Relevance over a pool of candidates per request, one
    launch.  `pool_idx` int64 [B, n], n <= MMR_POOL_MAX, negative entries are empty slots - `rank_topk`'s indices, `blend_points`'
    `out_items`; `relevance` [B, n] float32 (`rank_topk`'s values) or float64 (`blended_ranking`'s ratings), the value of every
    pool entry; `item_emb` [n_items, D] float32.  Strided views are taken as they are where the inner stride is 1.  Pick 0 is the
    slot of the greatest lam * r; pick t >= 1 that of the greatest lam * r_a - (1 - lam) * max over the picked s of cos(e_a, e_s),
    ties to the lowest slot, a NaN key last; with `normalize` r is the relevance scaled to [0, 1] by the finite extremes of the
    row, otherwise the relevance as given (the header states every operation and its order).  lam = 1 keeps the pool's order by
    relevance, lam = 0 is farthest-first after the first pick.
    Returns the picked item ids int64 [B, top]; with `return_slots` / `return_keys` a tuple with their pool columns (int32) and the
    keys they were picked with (float64) appended in that order.  Columns past a row's non-empty slots hold (-1, -1, -inf).  An
    entry >= n_items raises IndexError after the call's one read-back - the other rows are complete by then -; with a caller's int32
    `status` word it is only flagged there (bit 0) and the call does not sync."""
    lib = _lib.load()
    fn = "mmr_rerank"
    # shapes, types and limits first (they hold on any device), then where the tensors live
    if pool_idx.dtype != torch.int64:
        raise TypeError(f"{fn}: pool_idx must be int64, got {pool_idx.dtype}")
    if relevance.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{fn}: relevance must be float32 or float64, got {relevance.dtype}")
    if item_emb.dtype != torch.float32:
        raise TypeError(f"{fn}: item_emb must be float32, got {item_emb.dtype}")
    if pool_idx.dim() != 2 or int(pool_idx.shape[1]) < 1:
        raise ValueError(f"{fn}: pool_idx must be [B, n], got {tuple(pool_idx.shape)}")
    n = int(pool_idx.shape[1])
    if tuple(relevance.shape) != tuple(pool_idx.shape):
        raise ValueError(f"{fn}: relevance must be [B, n] = {tuple(pool_idx.shape)} as pool_idx, got {tuple(relevance.shape)}")
    if item_emb.dim() != 2 or int(item_emb.shape[0]) < 1 or int(item_emb.shape[1]) < 1 or int(item_emb.shape[0]) >= 2 ** 31:
        raise ValueError(f"{fn}: item_emb must be [n_items, D], got {tuple(item_emb.shape)}")
    if n > MMR_POOL_MAX:
        raise ValueError(f"{fn}: a pool of n={n} entries, at most {MMR_POOL_MAX}")
    top = int(top)
    if top < 1 or top > n:
        raise ValueError(f"{fn}: top={top} outside [1, n={n}]")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"{fn}: lam={lam} outside [0, 1]")
    _require_device(item_emb, "item_emb")
    dev = item_emb.device
    _require_same_device(fn, (("pool_idx", pool_idx), ("relevance", relevance)), "item_emb", dev)
    status, check_status = _status_word(fn, status, dev)
    pool_idx, relevance, item_emb = _unit_inner(pool_idx), _unit_inner(relevance), _unit_inner(item_emb)
    B, n_items, D = int(pool_idx.shape[0]), int(item_emb.shape[0]), int(item_emb.shape[1])
    out_items = torch.empty((B, top), dtype=torch.int64, device=dev)
    out_slots = torch.empty((B, top), dtype=torch.int32, device=dev) if return_slots else None
    out_keys = torch.empty((B, top), dtype=torch.float64, device=dev) if return_keys else None
    if B > 0:
        with _on(dev):
            _lib.check(lib.ngcf_list_mmr_f32(_ptr(pool_idx), _row_major_ld(pool_idx, "pool_idx"), _ptr(relevance),
                                             int(relevance.dtype == torch.float64), _row_major_ld(relevance, "relevance"), B, n, top,
                                             _ptr(item_emb), _row_major_ld(item_emb, "item_emb"), n_items, D, lam, int(bool(normalize)),
                                             _ptr(out_items), _ptr(out_slots), _ptr(out_keys), _ptr(status), _stream()))
    if check_status:
        _raise_bad_id(fn, int(status.item()), n_items)
    if not (return_slots or return_keys):
        return out_items
    return (out_items,) + ((out_slots,) if return_slots else ()) + ((out_keys,) if return_keys else ())
