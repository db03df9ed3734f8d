"""Host oracle of the beyond-accuracy list figures (csrc/list_quality.hip), in plain numpy and Python: written from the section
"beyond-accuracy figures of top lists" of include/ngcf_hip.h, no code shared with the kernels or their wrappers, nothing here runs
on a GPU.  tests/test_list_quality_oracle.py checks this file against brute-force definitions on the CPU;
tests/test_list_quality_gpu.py holds the kernels to it.

(a) exposure_counts: a loop over the entries.
(b) summary_numbers / figures: the five reduced numbers - Python ints for the integers, math.fsum for the two float sums - and the
    figures formed from them; gini_mad is the Gini coefficient from its definition, the mean absolute difference.
(c) the Gram matrix of a list in three readings of the header's "one ascending-k fmaf chain from 0":
      gram_exact   integer tables whose partial sums stay below 2^24 (asserted): the chain is exact, any order gives the same bits
      gram_chain   8-bit significands in a narrow exponent window: float64 holds every product and every running sum exactly - the
                   TwoSum error term is asserted to be 0 - so float32(float64(x) * float64(y) + float64(acc)) rounds once and IS
                   fmaf(x, y, acc); the data does round in fp32, a reordered accumulation gives other bits
      gram_f64     the float64 Gram matrix and sum_k |x_k y_k|, for the error bound of arbitrary data
(d) ild_rows: cos, d, the s_b and S_K chains exactly as the header states them, in Python floats (IEEE double, math.sqrt)."""
import math
from fractions import Fraction

import numpy as np

K_MAX = 64          # NGCF_LIST_DIV_K_MAX, as a literal on purpose
KS_MAX = 8


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
def exposure_counts(lists, n_items, k=None):
    """counts[i] = entries equal to i in columns [0, k) of every row; negative entries are empty slots, entries >= n_items are bad
    (returned as a flag, never counted)."""
    lists = np.asarray(lists)
    k = lists.shape[1] if k is None else k
    counts, bad = [0] * n_items, False
    for row in lists:
        for v in row[:k]:
            v = int(v)
            if v < 0:
                continue
            if v >= n_items:
                bad = True
                continue
            counts[v] += 1
    return counts, bad


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def _log2(n):
    """numpy's log2 of an integer: tests/test_dd_log2.py pins that it has the bits of the kernels' correctly rounded log2 on the
    integers up to 5000, so on the GPU tests' counts kernel and oracle add the same terms."""
    return float(np.log2(np.float64(n)))


def summary_numbers(counts, popularity=None, n_user=None):
    """{"covered", "total", "weighted"} exact, {"clog", "nov"} by math.fsum, and the sums of the terms' absolute values
    {"clog_abs", "nov_abs"} that the error bound of any summation order is stated in."""
    counts = [int(c) for c in counts]
    ordered = sorted(counts)
    clog_terms = [float(c) * _log2(c) for c in counts if c > 0]
    out = {"covered": sum(1 for c in counts if c > 0), "total": sum(counts),
           "weighted": sum((i + 1) * c for i, c in enumerate(ordered)),
           "clog": math.fsum(clog_terms), "clog_abs": math.fsum(abs(t) for t in clog_terms), "nov": 0.0, "nov_abs": 0.0}
    if popularity is not None:
        log_users = _log2(n_user)
        terms = [float(c) * (log_users - _log2(max(int(p), 1))) for c, p in zip(counts, popularity) if c > 0]
        out["nov"], out["nov_abs"] = math.fsum(terms), math.fsum(abs(t) for t in terms)
    return out


def figures(numbers, n_items, with_novelty=True):
    """coverage, gini, entropy, novelty from the five numbers; gini rounded once from the exact fraction."""
    n, total = int(n_items), numbers["total"]
    if total == 0:
        return {"coverage": math.nan, "gini": math.nan, "entropy": math.nan, "novelty": math.nan}
    return {"coverage": numbers["covered"] / n,
            "gini": float(Fraction(2 * numbers["weighted"], n * total) - Fraction(n + 1, n)),
            "entropy": math.log2(total) - numbers["clog"] / total,
            "novelty": numbers["nov"] / total if with_novelty else math.nan}


def gini_mad(counts):
    """The Gini coefficient from its definition: half the relative mean absolute difference, sum_ij |c_i - c_j| / (2 n^2 mean), as
    an exact fraction."""
    counts = [int(c) for c in counts]
    n, total = len(counts), sum(counts)
    mad = sum(abs(a - b) for a in counts for b in counts)
    return Fraction(mad, 2 * n * total)


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def int_table(rng, n_items, D):
    """float32 [n_items, D] in +-{1..8}."""
    return (rng.integers(1, 9, (n_items, D)) * rng.choice(np.array([-1, 1]), (n_items, D))).astype(np.float32)


def chain_table(rng, n_items, D):
    """float32 [n_items, D]: 8-bit significands 128..255 times 2^-12 .. 2^-6, random signs."""
    a = rng.integers(128, 256, (n_items, D)) * np.exp2(rng.integers(-12, -5, (n_items, D)).astype(np.float64))
    return (a * rng.choice(np.array([-1.0, 1.0]), (n_items, D))).astype(np.float32)


def _rows(table, ids):
    """The item rows of one list [k, D]; an empty or bad slot is a row of zeros, as the kernel stages it."""
    ids = np.asarray(ids)
    ok = (ids >= 0) & (ids < table.shape[0])
    E = np.zeros((ids.size, table.shape[1]), dtype=table.dtype)
    E[ok] = table[ids[ok]]
    return E, ok


def gram_exact(table, ids):
    """float32 [k, k] of an integer table: every partial sum is an integer below 2^24 (asserted), so fp32 is exact in any order."""
    E, ok = _rows(table, ids)
    Ei = E.astype(np.int64)
    assert (Ei == E).all()
    assert int(np.abs(Ei).sum(axis=1).max(initial=0)) * int(np.abs(Ei).max(initial=0)) < 2 ** 24
    return (Ei @ Ei.T).astype(np.float32), ok


def fma32(x, y, acc):
    """fmaf(x, y, acc) on float32 arrays whose float64 product and sum are exact (TwoSum error term asserted 0)."""
    p = x.astype(np.float64) * y.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    assert not err.any(), "the float64 sum is not exact: the inputs are outside the oracle's range"
    return s.astype(np.float32)


def gram_chain(table, ids, reverse=False):
    """float32 [k, k]: G_ab = fmaf(e_a[D-1], e_b[D-1], .. fmaf(e_a[0], e_b[0], 0)), ascending k (`reverse`: descending, to show that
    the data tells the orders apart)."""
    E, ok = _rows(table, ids)
    G = np.zeros((E.shape[0], E.shape[0]), dtype=np.float32)
    order = range(E.shape[1] - 1, -1, -1) if reverse else range(E.shape[1])
    for kk in order:
        G = fma32(E[:, kk, None], E[None, :, kk], G)
    return G, ok


def gram_f64(table, ids):
    """(G64, T, ok): the float64 Gram matrix and T_ab = sum_k |e_a[k] e_b[k]|."""
    E, ok = _rows(table, ids)
    E = E.astype(np.float64)
    return E @ E.T, np.abs(E) @ np.abs(E).T, ok


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def pair_distance(g, gaa, gbb):
    """d_ab = 1.0 - cos_ab from three float32 Gram entries: every double operation on its own."""
    p = float(gaa) * float(gbb)
    c = 0.0 if p == 0.0 else float(g) / math.sqrt(p)         # a NaN product is not 0: it propagates
    return 1.0 - c


def ild_row(G, ok, ks):
    """[(ild@K, counted)] of one list from its float32 Gram matrix and the mask of non-empty slots: s_b over ascending valid a < b
    from 0.0, S_K over ascending valid b < K from 0.0, ild = S_K / (V_K (V_K - 1) / 2); V_K < 2: (0.0, 0)."""
    k = len(ok)
    s = [0.0] * k
    for b in range(k):
        if not ok[b]:
            continue
        acc = 0.0
        for a in range(b):
            if ok[a]:
                acc = acc + pair_distance(G[a, b], G[a, a], G[b, b])
        s[b] = acc
    out = []
    for K in ks:
        S, V = 0.0, 0
        for b in range(K):
            if ok[b]:
                S = S + s[b]
                V += 1
        out.append((S / float(V * (V - 1) // 2), 1) if V >= 2 else (0.0, 0))
    return out


def ild_rows(table, lists, ks, gram=gram_exact):
    """(per_user float64 [B, n_ks], counted int [B, n_ks]) of every list with the Gram reading `gram`."""
    lists = np.asarray(lists)
    per_user = np.zeros((lists.shape[0], len(ks)))
    counted = np.zeros((lists.shape[0], len(ks)), dtype=np.int64)
    for r, ids in enumerate(lists):
        G, ok = gram(table, ids)
        for q, (v, c) in enumerate(ild_row(G, ok, ks)):
            per_user[r, q], counted[r, q] = v, c
    return per_user, counted


def ild_brute(table, ids, K):
    """ild@K from the definition in float64: the mean of 1 - cos over the pairs of non-empty slots below K; None with fewer than 2."""
    E, ok = _rows(table, ids)
    E = E.astype(np.float64)
    slots = [a for a in range(K) if ok[a]]
    d = []
    for i, a in enumerate(slots):
        for b in slots[i + 1:]:
            na, nb = math.sqrt(float(E[a] @ E[a])), math.sqrt(float(E[b] @ E[b]))
            d.append(1.0 - (float(E[a] @ E[b]) / (na * nb) if na * nb else 0.0))
    return sum(d) / len(d) if len(slots) >= 2 else None


def ild_bound(table, ids, K):
    """How far ild@K computed from an fp32 fmaf-chain Gram matrix may lie from the float64 value (derivation: the docstring of
    test_list_quality_gpu.test_diversity_normal_tables_within_the_chain_bound).  (ild64, bound); None with fewer than 2 slots."""
    G, T, ok = gram_f64(table, ids)
    D = table.shape[1]
    gamma = D * 2.0 ** -24 / (1.0 - D * 2.0 ** -24)
    slots = [a for a in range(K) if ok[a]]
    if len(slots) < 2:
        return None
    d, e = [], []
    for i, a in enumerate(slots):
        for b in slots[i + 1:]:
            n = math.sqrt(G[a, a] * G[b, b])
            c = G[a, b] / n if n else 0.0
            d.append(1.0 - c)
            e.append((abs(c) + (T[a, b] / n if n else 0.0)) * gamma / (1.0 - gamma))
    pairs = len(d)
    return math.fsum(d) / pairs, math.fsum(e) / pairs + (pairs + 8) * 2.0 ** -51
