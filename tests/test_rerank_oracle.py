"""CPU tests of tests/rerank_oracle.py: the oracle the GPU tests hold csrc/list_rerank.hip to is itself checked against a brute-force
float64 MMR from the definition, against the two ends of lam whose result is known without any arithmetic, and on the rules the
header states in words: duplicates, NaNs, ties, the edge cases of `normalize`."""
import math

import numpy as np

import rerank_oracle as orc


def _case(seed, n_items=40, D=9, B=6, n=12):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((n_items, D)).astype(np.float32)
    pools = np.stack([rng.permutation(n_items)[:n] for _ in range(B)])
    rel = rng.standard_normal((B, n)).astype(np.float32)
    return table, pools, rel


def _gram32(table, ids):
    """A float32 Gram matrix by numpy: good enough where only near-equality with float64 is asked."""
    E, ok = orc.gram_f64(table, ids)[0], np.ones(len(ids), dtype=bool)
    return E.astype(np.float32), ok


def test_oracle_equals_the_brute_force_definition():
    for seed, lam in ((1, 0.5), (2, 0.9), (3, 0.1)):
        table, pools, rel = _case(seed)
        items, slots, keys = orc.mmr_rows(table, pools, rel, 7, lam, False, gram=_gram32)
        for b in range(pools.shape[0]):
            picked, want = orc.mmr_brute(table, pools[b], rel[b], 7, lam)
            assert slots[b].tolist() == picked and items[b].tolist() == pools[b][picked].tolist()
            assert np.allclose(keys[b], want, rtol=0, atol=1e-6)          # the float32 Gram entries against float64 ones
            # and the float64 reading agrees with the definition to rounding, every step decided or not
            s64, k64, bounds, _ = orc.mmr_row_f64(table, pools[b], rel[b], 7, lam, False)
            assert s64 == picked and np.allclose(k64, want, rtol=0, atol=1e-12) and all(x >= 2.0 ** -50 for x in bounds)


def test_normalised_relevance_is_the_min_max_scaling():
    table, pools, rel = _case(4)
    ok = np.ones(pools.shape[1], dtype=bool)
    for b in range(pools.shape[0]):
        r = orc.relevance(rel[b], ok, True)
        v = rel[b].astype(np.float64)
        assert r == ((v - v.min()) / (v.max() - v.min())).tolist() and min(r) == 0.0 and max(r) == 1.0
        assert orc.relevance(rel[b], ok, False) == v.tolist()
    # normalised MMR = MMR as given on the scaled relevances
    a = orc.mmr_rows(table, pools, rel, 5, 0.6, True, gram=_gram32)
    scaled = np.array([orc.relevance(rel[b], ok, True) for b in range(pools.shape[0])])
    b_ = orc.mmr_rows(table, pools, scaled, 5, 0.6, False, gram=_gram32)
    assert all(np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b_))


def test_lam_one_is_the_stable_descending_relevance_order():
    rng = np.random.default_rng(5)
    table = orc.int_table(rng, 30, 6)
    pools = np.stack([rng.permutation(30)[:10] for _ in range(5)])
    rel = rng.integers(0, 4, (5, 10)).astype(np.float64)                    # many ties
    rel[0] = np.arange(10, 0, -1)                                            # strictly descending: the pool itself
    for normalize in (False, True):
        items, slots, keys = orc.mmr_rows(table, pools, rel, 10, 1.0, normalize)
        assert items[0].tolist() == pools[0].tolist() and slots[0].tolist() == list(range(10))
        for b in range(5):
            assert slots[b].tolist() == np.argsort(-rel[b], kind="stable").tolist()
        if not normalize:
            assert np.array_equal(keys, -np.sort(-rel, axis=1))


def test_lam_zero_is_farthest_first_after_the_first_pick():
    table, pools, rel = _case(6, n=9)
    rel[:, :] = 0.0
    rel[:, 4] = 1.0
    for b in range(pools.shape[0]):
        G, ok = _gram32(table, pools[b])
        slots, keys = orc.mmr_row(G, ok, rel[b], 9, 0.0, False)
        assert slots[0] == 0 and keys[0] == 0.0                              # lam = 0: every key is 0 at step 0, the lowest slot wins
        E = table[pools[b]].astype(np.float64)
        E /= np.linalg.norm(E, axis=1, keepdims=True)
        S = E @ E.T
        picked = [0]
        for t in range(1, 9):
            rest = [a for a in range(9) if a not in picked]
            far = min(rest, key=lambda a: max(S[a, s] for s in picked))      # the smallest largest-cosine: farthest from the picked set
            assert slots[t] == far and abs(keys[t] + max(S[far, s] for s in picked)) < 1e-6
            picked.append(far)


def test_a_duplicated_id_is_picked_last_among_equals():
    rng = np.random.default_rng(7)
    table = orc.int_table(rng, 20, 8)
    ids = np.array([3, 5, 3, 9, 11])
    rel = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    for lam in (0.0, 0.3):
        items, slots, keys = orc.mmr_rows(table, ids[None], rel[None], 5, lam, False)
        # slot 0 goes first (all keys equal); its copy in slot 2 then has cosine 1 with a picked item: the worst key to the end
        assert slots[0, 0] == 0 and slots[0, -1] == 2 and keys[0, -1] == lam * 1.0 - (1.0 - lam) * 1.0
    # one id everywhere: every cosine is 1, the tie rule alone orders the picks
    items, slots, _ = orc.mmr_rows(table, np.full((1, 6), 4), np.ones((1, 6)), 4, 0.3, True)
    assert slots[0].tolist() == [0, 1, 2, 3] and items[0].tolist() == [4] * 4


def test_nan_and_tie_rules():
    G = np.eye(4, dtype=np.float32)
    ok = np.ones(4, dtype=bool)
    # a NaN key ranks below -inf; among NaN keys the lowest slot wins
    slots, keys = orc.mmr_row(G, ok, [math.nan, -math.inf, math.nan, 2.0], 4, 1.0, False)
    assert slots == [3, 1, 0, 2] and keys[0] == 2.0 and keys[1] == -math.inf and math.isnan(keys[2]) and math.isnan(keys[3])
    assert np.array(keys[2:]).view(np.int64).tolist() == [0x7FF8000000000000] * 2
    # +0.0 and -0.0 are equal keys: the lowest slot
    slots, _ = orc.mmr_row(G, ok, [-1.0, -0.0, 0.0, -0.0], 2, 1.0, False)
    assert slots == [1, 2]
    # a NaN cosine makes m_a a NaN for good: the slots that met it go last, in slot order
    Gn = np.array([[1, 0, 0, 0], [0, 1, np.nan, 0], [0, np.nan, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    slots, keys = orc.mmr_row(Gn, ok, [4.0, 3.0, 2.0, 1.0], 4, 0.5, False)
    assert slots == [0, 1, 3, 2] and math.isnan(keys[3]) and keys[2] == 0.5
    # empty slots are skipped wherever they stand; the tail is (-1, -inf)
    slots, keys = orc.mmr_row(G, np.array([False, True, False, True]), [9.0, 1.0, 9.0, 2.0], 3, 1.0, False)
    assert slots == [3, 1, -1] and keys == [2.0, 1.0, -math.inf]
    items, slots, keys = orc.mmr_rows(orc.int_table(np.random.default_rng(0), 5, 3), np.array([[-1, 7, -3]]), np.ones((1, 3)), 2, 0.5, True)
    assert items.tolist() == [[-1, -1]] and slots.tolist() == [[-1, -1]] and keys.tolist() == [[-math.inf, -math.inf]]
    # a zero row: its cosines are 0.0, not a NaN
    assert orc.cosine(0.0, 0.0, 5.0) == 0.0 and orc.cosine(2.0, 4.0, 1.0) == 1.0 and math.isnan(orc.cosine(math.nan, 1.0, 1.0))
    assert math.isnan(orc.cosine(math.nan, 0.0, math.nan))                   # 0 * NaN is a NaN, not 0


def test_normalize_edge_cases():
    ok = np.ones(4, dtype=bool)
    inf = math.inf
    assert orc.relevance([2.0, 2.0, 2.0, 2.0], ok, True) == [0.0] * 4       # all equal
    r = orc.relevance([inf, -inf, math.nan, inf], ok, True)                  # no finite value: they stay
    assert r[0] == inf and r[1] == -inf and math.isnan(r[2]) and r[3] == inf
    r = orc.relevance([inf, 1.0, 3.0, -inf], ok, True)                       # the finite ones are scaled among themselves
    assert r == [inf, 0.0, 1.0, -inf]
    r = orc.relevance([math.nan, 5.0, inf, 5.0], ok, True)                   # one finite value (twice): 0.0
    assert math.isnan(r[0]) and r[1:] == [0.0, inf, 0.0]
    # the extremes are taken over the non-empty slots only
    assert orc.relevance([100.0, 1.0, 2.0, 3.0], np.array([False, True, True, True]), True)[1:] == [0.0, 0.5, 1.0]
    # +inf relevance with lam = 0 is a NaN key (0 * inf): it goes last
    G = np.eye(3, dtype=np.float32)
    slots, keys = orc.mmr_row(G, np.ones(3, dtype=bool), [inf, 1.0, 2.0], 3, 0.0, True)
    assert slots == [1, 2, 0] and math.isnan(keys[2])


def test_the_fmaf_chain_of_arbitrary_data_rounds_once():
    from fractions import Fraction
    rng = np.random.default_rng(8)
    table = orc.chain_table(rng, 12, 37)
    ids = np.arange(12)
    assert np.array_equal(orc.gram_fma(table, ids)[0], orc.gram_chain(table, ids)[0])          # where both apply: the same bits
    # against exact rational arithmetic, on values chosen so that the float64 sum does round (wide exponent spread)
    x = (rng.standard_normal(4000) * np.exp2(rng.integers(-20, 20, 4000))).astype(np.float32)
    y = (rng.standard_normal(4000) * np.exp2(rng.integers(-20, 20, 4000))).astype(np.float32)
    a = (rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))).astype(np.float32)
    got = orc.fma32_any(x, y, a)
    inexact = 0
    for i in range(4000):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(a[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        d = abs(Fraction(float(got[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact)
        inexact += float(x[i]) * float(y[i]) + float(a[i]) != exact
    assert inexact > 100                                                      # the float64 sum was not exact: the odd rounding was at work
    # where plain double rounding goes wrong: acc = 2^14 + 2^-9 (float32 spacing 2^-9, last bit odd), x * y = 2^-10 - 2^-56, just below
    # half a spacing, so the sum rounds DOWN to acc; the float64 sum drops the 2^-56, lands on the midpoint and would tie to even, up
    f32 = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    x, y, acc = f32(2.0 ** -10 * (1.0 + 2.0 ** -23)), f32(1.0 - 2.0 ** -23), f32(2.0 ** 14 + 2.0 ** -9)
    assert float(x[0]) * float(y[0]) == 2.0 ** -10 - 2.0 ** -56
    assert np.float32(np.float64(x[0]) * np.float64(y[0]) + np.float64(acc[0])) == np.float32(2.0 ** 14 + 2.0 ** -8)      # the wrong way
    assert orc.fma32_any(x, y, acc)[0] == acc[0]
