"""Host statement of the certified two-stage ranking (csrc/rank_prefilter.hip), in plain numpy: written from the section "certified
two-stage ranking" of include/ngcf_hip.h, no code shared with the kernels or their wrapper, nothing here runs on a GPU.
tests/test_rank_prefilter_oracle.py checks the recipe itself (ub >= s on every pair, certified answers = a brute-force exact top-k).
The s~ of this file is a float64 dot product of the bf16 images rounded to float32; the MFMA's own s~ may differ from it in its last
bits, so the GPU tests never compare ub, the threshold or the pool with this file - they compare results with engine.rank_topk, and
the tables below are the ones they run on."""
import numpy as np

REG_LO, REG_HI = 2.0 ** -40, 2.0 ** 40


def beta(D):
    return 2.0 ** -7 + 2.0 ** -16 + (4 * D + 2) * 2.0 ** -24


def bf16_rne(x):
    """float32 -> the float32 value of its bf16 image: round to nearest even, by integer arithmetic on the bits."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def fma32(a, b, c):
    """float32 fmaf(a, b, c) on arrays: the product is exact in float64, the sum is rounded to odd there (TwoSum says whether it was
    exact), and one rounding to float32 then gives the correctly rounded result."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p + c
        bb = t - p
        e = (p - (t - bb)) + (c - bb)
        odd = (t.view(np.int64) & 1) == 1
        fix = np.isfinite(t) & (e != 0) & ~odd
        t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
        return t.astype(np.float32)


def chain_scores(U, I):
    """rank_topk's score of every pair: one ascending-k fmaf chain from 0, float32 [B, n]."""
    acc = np.zeros((U.shape[0], I.shape[0]), dtype=np.float32)
    for k in range(U.shape[1]):
        acc = fma32(U[:, k:k + 1], I[None, :, k], acc)
    return acc


def float_key(x):
    """The monotone map float32 -> uint32 (larger float = larger key, NaN above +inf)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def round_up(v):
    """float64 >= 0 -> a float32 above it: its nearest float32, one ulp up."""
    return np.nextafter(np.asarray(v, dtype=np.float64).astype(np.float32), np.float32(np.inf))


def regular(X):
    """Per row: every element is 0 or has a magnitude in [2^-40, 2^40]."""
    a = np.abs(X.astype(np.float64))
    with np.errstate(invalid="ignore"):
        return np.all((a == 0) | ((a >= REG_LO) & (a <= REG_HI)), axis=1)


def upper_bounds(U, I):
    """(ub float32 [B, n], s~ float32 [B, n]): ni, bu, s~ and ub = fmaf(bu, ni, s~) in the header's operations."""
    D = U.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        ni = round_up(np.sqrt((I.astype(np.float64) ** 2).sum(1)))
        bu = round_up(beta(D) * np.sqrt((U.astype(np.float64) ** 2).sum(1)))
        approx = (bf16_rne(U).astype(np.float64) @ bf16_rne(I).astype(np.float64).T).astype(np.float32)
    return fma32(bu[:, None], ni[None, :], approx), approx


def _order(keys, ids):
    """Positions of the pairs in the output order: key descending, item ascending."""
    return np.lexsort((ids, -keys.astype(np.int64)))


def exact_topk(U, I, k, excluded=None):
    """Brute force: (values float32 [B, k], items int64 [B, k]) of rank_topk, (-inf, -1) past the eligible items."""
    s = chain_scores(U, I)
    vals = np.full((U.shape[0], k), -np.inf, dtype=np.float32)
    idx = np.full((U.shape[0], k), -1, dtype=np.int64)
    for b in range(U.shape[0]):
        ok = np.setdiff1d(np.arange(I.shape[0]), [] if excluded is None else excluded[b])
        top = ok[_order(float_key(s[b, ok]), ok)][:k]
        vals[b, :len(top)], idx[b, :len(top)] = s[b, top], top
    return vals, idx


def certified_topk(U, I, k, pool, excluded=None):
    """The recipe: (values [B, k], items [B, k], certified bool [B]) of the pools' own answer (no fallback)."""
    s = chain_scores(U, I)
    ub, _ = upper_bounds(U, I)
    table_regular = bool(regular(I).all())
    user_regular = regular(U)
    vals = np.full((U.shape[0], k), -np.inf, dtype=np.float32)
    idx = np.full((U.shape[0], k), -1, dtype=np.int64)
    cert = np.zeros(U.shape[0], dtype=bool)
    for b in range(U.shape[0]):
        ok = np.setdiff1d(np.arange(I.shape[0]), [] if excluded is None else excluded[b])
        by_bound = ok[_order(float_key(ub[b, ok]), ok)]
        members = by_bound[:pool]
        full = len(members) == pool
        thr = ub[b, members[-1]] if full else np.float32(-np.inf)
        top = members[_order(float_key(s[b, members]), members)][:k]
        vals[b, :len(top)], idx[b, :len(top)] = s[b, top], top
        above = len(top) == k and bool(s[b, top[-1]] > thr)
        cert[b] = table_regular and bool(user_regular[b]) and (not full or above)
    return vals, idx, cert


# ---- the tables of the tests (float32, seeded) ------------------------------------------------------------------------------------
def gaussian_tables(B, n_items, D, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((n_items, D)).astype(np.float32)


def popular_head_tables(B, n_items, D, seed, rank=8):
    """Low-rank embeddings with a log-normal popular head: item norms spread over two orders of magnitude."""
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((rank, D)) / np.sqrt(D)
    U = rng.standard_normal((B, rank)) @ basis + 0.05 * rng.standard_normal((B, D)) / np.sqrt(D)
    I = rng.standard_normal((n_items, rank)) @ basis + 0.05 * rng.standard_normal((n_items, D)) / np.sqrt(D)  # noqa: E741
    I *= rng.lognormal(0.0, 1.0, (n_items, 1))
    return U.astype(np.float32), I.astype(np.float32)


def cluster_tables(B=256, n_items=2000, D=64, seed=5):
    """Items 500..799 = 3 w (1 + 1e-4 eps) + 1e-3 noise for one unit direction w, `noise` a row of the generator every other item row
    comes from (N(0, 1) / sqrt(D) per component): near-identical, their exact scores ~2e-4 |u| apart, less than the bf16 error across
    them, so the bound cannot tell them apart and its order says little about the exact one.  The users' w-component is +0.5 / -0.5
    alternately: the even users rank the cluster on top and cannot be certified at pool < 300."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(D)
    w /= np.linalg.norm(w)
    I = rng.standard_normal((n_items, D)) / np.sqrt(D)  # noqa: E741
    I[500:800] = 3.0 * w * (1.0 + 1e-4 * rng.standard_normal((300, 1))) + 1e-3 * rng.standard_normal((300, D)) / np.sqrt(D)
    U = rng.standard_normal((B, D)) / np.sqrt(D)
    U -= np.outer(U @ w, w)
    U += np.outer(np.where(np.arange(B) % 2 == 0, 0.5, -0.5), w)
    return U.astype(np.float32), I.astype(np.float32)


IRREGULAR = (np.float32(np.nan), np.float32(np.inf), np.float32(2.0 ** 70), np.float32(2.0 ** -80))
