"""Host oracle of the greedy MMR re-rank (csrc/list_rerank.hip), in plain numpy and Python: written from the section "diversified
top lists" of include/ngcf_hip.h, no code shared with the kernel or its wrapper, nothing here runs on a GPU.
tests/test_rerank_oracle.py checks this file against a brute-force float64 MMR on the CPU; tests/test_rerank_gpu.py holds the kernel
to it.

The Gram matrix of a pool comes from tests/list_quality_oracle.py in one of its three readings of the header's "one ascending-k
fmaf chain from 0" (gram_exact, gram_chain: the kernel's bits; gram_f64: float64, for the error bound of arbitrary data).  From
there on every value is a Python float (IEEE double, math.sqrt) and every statement is one operation."""
import math
import struct

import numpy as np

from list_quality_oracle import chain_table, gram_chain, gram_exact, gram_f64, int_table  # noqa: F401  (re-exported to the tests)

POOL_MAX = 64          # NGCF_LIST_MMR_POOL_MAX, as a literal on purpose
NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]       # the quiet NaN a NaN key is written as
NEG_INF = -math.inf


def finite(v):
    return not (math.isnan(v) or math.isinf(v))


def relevance(values, ok, normalize):
    """r_a of every slot from the relevances as given (any float type; widened exactly) and the mask of non-empty slots."""
    v = [float(x) for x in values]
    if not normalize:
        return v
    fin = [x + 0.0 for x, o in zip(v, ok) if o and finite(x)]            # a zero of either sign enters as +0.0
    vmin = min(fin) if fin else math.inf
    vmax = max(fin) if fin else -math.inf
    out = []
    for x in v:
        if not finite(x):
            out.append(x)
        elif vmax > vmin:
            num = x - vmin
            den = vmax - vmin
            out.append(num / den)
        else:
            out.append(0.0)
    return out


def cosine(g, gaa, gbb):
    """cos_ab from three Gram entries: every double operation on its own; 0.0 where the product under the root is 0."""
    p = float(gaa) * float(gbb)
    if p == 0.0:
        return 0.0
    root = math.sqrt(p)                                      # p is a product of two sums of squares: >= 0, +inf or a NaN (a NaN stays)
    return float(g) / root


def beats(key, slot, best_key, best_slot):
    """Does candidate (key, slot) win against the best so far?  Greater key; a NaN below every other key; equal keys (+0.0 == -0.0) and
    NaN against NaN: the lowest slot."""
    a_nan, b_nan = math.isnan(key), math.isnan(best_key)
    if a_nan or b_nan:
        return (b_nan and not a_nan) or (a_nan and b_nan and slot < best_slot)
    return key > best_key or (key == best_key and slot < best_slot)


def mmr_row(G, ok, values, top, lam, normalize, cos=None):
    """(slots, keys) of one pool, `top` entries each, (-1, -inf) past the non-empty slots.  G: the pool's Gram matrix (any float
    type), or `cos`: a matrix of cosines to use as given."""
    n = len(ok)
    r = relevance(values, ok, normalize)
    oml = 1.0 - lam
    picked, m = [], [0.0] * n
    slots, keys = [], []
    steps = min(top, sum(1 for o in ok if o))
    for t in range(steps):
        best = None
        for a in range(n):
            if not ok[a] or a in picked:
                continue
            key = lam * r[a]
            if t > 0:
                pen = oml * m[a]
                key = key - pen
            if best is None or beats(key, a, best[0], best[1]):
                best = (key, a)
        key, s = best
        picked.append(s)
        slots.append(s)
        keys.append(NAN if math.isnan(key) else key)
        for a in range(n):
            c = float(cos[a][s]) if cos is not None else cosine(G[a][s], G[a][a], G[s][s])
            if t == 0:
                m[a] = c
            elif math.isnan(m[a]) or math.isnan(c):
                m[a] = NAN
            elif c > m[a]:
                m[a] = c
    slots += [-1] * (top - steps)
    keys += [NEG_INF] * (top - steps)
    return slots, keys


def mmr_rows(table, pools, values, top, lam, normalize, gram=gram_exact, poisoned=()):
    """(items int64 [B, top], slots int32 [B, top], keys float64 [B, top]) of every pool with the Gram reading `gram`.  An id
    >= n_items counts as an empty slot (the caller checks the flag).  `poisoned`: item ids whose table row holds a NaN - every Gram
    entry of their slots is a NaN (the chain meets the NaN whatever the other row holds); `table` is then the clean table."""
    pools = np.asarray(pools)
    B = pools.shape[0]
    items = np.full((B, top), -1, dtype=np.int64)
    slots = np.full((B, top), -1, dtype=np.int32)
    keys = np.full((B, top), NEG_INF, dtype=np.float64)
    for b, ids in enumerate(pools):
        G, ok = gram(table, ids)
        if poisoned:
            G = G.copy()
            hit = np.isin(ids, list(poisoned))
            G[hit, :] = np.nan
            G[:, hit] = np.nan
        s, k = mmr_row(G, ok, values[b], top, lam, normalize)
        slots[b], keys[b] = s, k
        items[b] = [int(ids[a]) if a >= 0 else -1 for a in s]
    return items, slots, keys


# ---- arbitrary data: the float64 reading and how far a key may lie from it -----------------------------------------------------------
def mmr_row_f64(table, ids, values, top, lam, normalize):
    """The greedy loop on the float64 Gram matrix of one pool, with the error bound of every key the kernel can form.  Returns
    (slots, keys, bounds, decided): `decided` is False when at some step with more than one candidate left the winner's key minus its
    bound does not exceed another candidate's key plus that candidate's bound - the fp32 chain may then pick otherwise, the row is not
    compared.  The bound of key_a at step t >= 1 is (1 - lam) * max over the picked s of (|c_as| + T_as / sqrt(G_aa G_ss)) * gamma_D /
    (1 - gamma_D), plus 2^-50 for the fp64 roundings (the largest of cosines moves by at most the largest of their errors); at step 0
    it is 2^-50.  gamma_D = D 2^-24 / (1 - D 2^-24): tests/test_list_quality_gpu.py derives the cosine's bound."""
    G, T, ok = gram_f64(table, ids)
    n, D = len(ok), table.shape[1]
    gamma = D * 2.0 ** -24 / (1.0 - D * 2.0 ** -24)
    nrm = np.sqrt(np.outer(np.diag(G), np.diag(G)))
    safe = np.where(nrm > 0, nrm, 1.0)
    cos = np.where(nrm > 0, G / safe, 0.0)
    err = np.where(nrm > 0, (np.abs(cos) + T / safe) * gamma / (1.0 - gamma), 0.0)
    r = relevance(values, ok, normalize)
    oml = 1.0 - lam
    picked, slots, keys, bounds, decided = [], [], [], [], True
    steps = min(top, int(ok.sum()))
    for t in range(steps):
        cands = []
        for a in range(n):
            if not ok[a] or a in picked:
                continue
            key, bound = lam * r[a], 2.0 ** -50
            if t > 0:
                key = key - oml * max(cos[a, s] for s in picked)
                bound = oml * max(err[a, s] for s in picked) + 2.0 ** -50
            cands.append((key, a, bound))
        key, s, bound = max(cands, key=lambda c: (c[0], -c[1]))
        for k2, a2, b2 in cands:
            if a2 != s and not key - bound > k2 + b2:
                decided = False
        picked.append(s)
        slots.append(s)
        keys.append(key)
        bounds.append(bound)
    return slots, keys, bounds, decided


def mmr_brute(table, ids, values, top, lam):
    """MMR from its definition in float64, without the oracle's structure: unit vectors, a fresh maximum over the picked set at every
    step, numpy's argmax.  For data without empty slots, ties, zero rows or NaNs; relevance as given."""
    E = table[np.asarray(ids)].astype(np.float64)
    E = E / np.linalg.norm(E, axis=1, keepdims=True)
    S = E @ E.T
    rel = np.asarray(values, dtype=np.float64)
    picked = [int(np.argmax(lam * rel))]
    keys = [float(lam * rel[picked[0]])]
    while len(picked) < top:
        score = lam * rel - (1.0 - lam) * S[:, picked].max(axis=1)
        score[picked] = -np.inf
        picked.append(int(np.argmax(score)))
        keys.append(float(score[picked[-1]]))
    return picked, keys


# ---- the fmaf chain of arbitrary float32 data ----------------------------------------------------------------------------------------
def fma32_any(x, y, acc):
    """fmaf(x, y, acc) on float32 arrays of any (normal-range) values.  The float64 product of two float32 is exact; the float64 sum
    is rounded TO ODD - where TwoSum's error term is not 0 and the rounded sum's last bit is even, the neighbour on the error's side
    is taken - and a round-to-odd value with 53 >= 24 + 2 bits rounds to float32 as the exact sum does: one rounding."""
    p = x.astype(np.float64) * y.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def gram_fma(table, ids):
    """float32 [k, k] of any table: G_ab = fmaf(e_a[D-1], e_b[D-1], .. fmaf(e_a[0], e_b[0], 0)), ascending k; (G, ok) like the three
    readings of tests/list_quality_oracle.py."""
    ids = np.asarray(ids)
    ok = (ids >= 0) & (ids < table.shape[0])
    E = np.zeros((ids.size, table.shape[1]), dtype=np.float32)
    E[ok] = table[ids[ok]]
    G = np.zeros((ids.size, ids.size), dtype=np.float32)
    for kk in range(E.shape[1]):
        G = fma32_any(E[:, kk, None], E[None, :, kk], G)
    return G, ok
