"""CPU tests of tests/list_quality_oracle.py: the oracle the GPU tests hold csrc/list_quality.hip to is itself checked against
brute-force definitions - counts by numpy, the Gini coefficient from the mean absolute difference and on the two histograms whose
value is known in closed form, the diversity chains against plain pairwise loops - and the order oracle is shown to tell an
ascending accumulation from a descending one."""
import math
from fractions import Fraction

import numpy as np
import pytest

import list_quality_oracle as orc


def _lists(rng, B, k, n_items, empty=0.2):
    lists = rng.integers(0, n_items, (B, k))
    lists[rng.random((B, k)) < empty] = -1
    return lists


def test_exposure_counts_equal_bincount_and_flag_bad_ids():
    rng = np.random.default_rng(1)
    lists = _lists(rng, 50, 7, 13)
    counts, bad = orc.exposure_counts(lists, 13)
    assert not bad and counts == np.bincount(lists[lists >= 0], minlength=13).tolist()
    head, _ = orc.exposure_counts(lists, 13, k=3)
    assert head == np.bincount(lists[:, :3][lists[:, :3] >= 0], minlength=13).tolist()
    lists[4, 2] = 13
    other, bad = orc.exposure_counts(lists, 13)
    lists[4, 2] = -1
    assert bad and other == orc.exposure_counts(lists, 13)[0]


def test_gini_closed_form_equals_the_mean_absolute_difference():
    rng = np.random.default_rng(2)
    for n in (1, 2, 5, 40):
        counts = rng.integers(0, 30, n).tolist()
        counts[0] += 1
        num = orc.summary_numbers(counts)
        closed = Fraction(2 * num["weighted"], n * num["total"]) - Fraction(n + 1, n)
        assert closed == orc.gini_mad(counts)
        assert orc.figures(num, n)["gini"] == float(closed)


@pytest.mark.parametrize("n", [1, 2, 7, 100])
def test_gini_of_a_uniform_and_of_a_one_item_histogram(n):
    uniform = orc.figures(orc.summary_numbers([5] * n), n)
    assert uniform["gini"] == 0.0 and uniform["coverage"] == 1.0
    assert uniform["entropy"] == pytest.approx(math.log2(n), abs=1e-12)
    one = [0] * n
    one[n // 2] = 9
    single = orc.figures(orc.summary_numbers(one), n)
    assert single["gini"] == float(Fraction(n - 1, n)) and single["coverage"] == 1 / n and single["entropy"] == pytest.approx(0.0, abs=1e-12)


def test_summary_numbers_against_plain_sums():
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 50, 60)
    counts[::7] = 0
    pop = rng.integers(0, 400, 60)
    num = orc.summary_numbers(counts, pop, 1000)
    assert num["covered"] == int((counts > 0).sum()) and num["total"] == int(counts.sum())
    assert num["weighted"] == int((np.sort(counts) * np.arange(1, 61)).sum())
    c = counts[counts > 0].astype(np.float64)
    assert num["clog"] == pytest.approx(float((c * np.log2(c)).sum()), rel=1e-13)
    want = float((counts * (np.log2(1000.0) - np.log2(np.maximum(pop, 1)))).sum())
    assert num["nov"] == pytest.approx(want, rel=1e-13)
    fig = orc.figures(num, 60)
    p = c / c.sum()
    assert fig["entropy"] == pytest.approx(float(-(p * np.log2(p)).sum()), rel=1e-12)
    assert fig["novelty"] == pytest.approx(want / counts.sum(), rel=1e-13)
    empty = orc.figures(orc.summary_numbers([0, 0, 0]), 3)
    assert all(math.isnan(v) for v in empty.values()) and orc.summary_numbers([0, 0, 0])["covered"] == 0


@pytest.mark.parametrize("table_of, gram", [(orc.int_table, orc.gram_exact), (orc.chain_table, orc.gram_chain)])
def test_ild_chains_equal_pairwise_loops(table_of, gram):
    rng = np.random.default_rng(4)
    table = table_of(rng, 30, 37)
    table[0] = 0.0                                              # an all-zero item: cos = 0 with every partner
    lists = _lists(rng, 12, 9, 30)
    lists[0] = -1                                               # V = 0
    lists[1, 1:] = -1                                           # V = 1
    lists[2, 2:] = -1                                           # V = 2
    lists[3, :4] = [5, 5, 0, 5]                                 # duplicates and the zero row
    ks = (2, 5, 9)
    per_user, counted = orc.ild_rows(table, lists, ks, gram)
    for r, ids in enumerate(lists):
        for q, K in enumerate(ks):
            want = orc.ild_brute(table, ids, K)
            assert counted[r, q] == (want is not None)
            assert per_user[r, q] == pytest.approx(0.0 if want is None else want, abs=1e-5)
    G, ok = gram(table, lists[3])
    assert orc.pair_distance(G[0, 1], G[0, 0], G[1, 1]) == 0.0          # duplicate ids: cos exactly 1
    assert orc.pair_distance(G[0, 2], G[0, 0], G[2, 2]) == 1.0          # the zero row: cos = 0
    assert math.isnan(orc.pair_distance(np.float32("nan"), np.float32(1), np.float32(1)))
    # a cut-off is a prefix of one chain: the values of (2, 5, 9) at once equal the single calls
    for q, K in enumerate(ks):
        assert np.array_equal(orc.ild_rows(table, lists, (K,), gram)[0][:, 0], per_user[:, q])


def test_order_oracle_tells_ascending_from_descending():
    rng = np.random.default_rng(5)
    table = orc.chain_table(rng, 16, 130)
    ids = np.arange(16)
    up, _ = orc.gram_chain(table, ids)
    down, _ = orc.gram_chain(table, ids, reverse=True)
    assert (up != down).any()                                   # fp32 does round on this data
    assert np.array_equal(up, up.T)                             # fmaf(x, y, acc) = fmaf(y, x, acc)
    G64 = table.astype(np.float64) @ table.astype(np.float64).T
    assert np.abs(up - G64).max() <= 130 * 2.0 ** -24 * np.abs(G64).max() * 4


def test_ild_bound_covers_a_float32_gram():
    rng = np.random.default_rng(6)
    table = rng.standard_normal((40, 65)).astype(np.float32)
    ids = rng.integers(0, 40, 20)
    E = table[ids]
    G = np.zeros((20, 20), dtype=np.float32)
    for kk in range(65):                                        # numpy's fp32 multiply-add: two roundings a step, within 2 gamma
        G = G + E[:, kk, None] * E[None, :, kk]
    got = orc.ild_row(G, np.ones(20, dtype=bool), (20,))[0][0]
    want, bound = orc.ild_bound(table, ids, 20)
    assert abs(got - want) <= 2 * bound and bound < 1e-4
