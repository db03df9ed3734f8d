"""The numpy oracle of the exact held-out positions (tests/rank_position_oracle.py) against the definition stated pair by pair, and
its metrics against hand-computed values and an independent statement of every formula.  No device."""
import math

import numpy as np
import pytest

import rank_position_oracle as orc

NAN, INF = float("nan"), float("inf")


def test_key_orders_special_values_like_the_kernels():
    vals = np.array([-INF, -3.0, -0.0, 0.0, 1e-45, 2.0, INF, NAN], dtype=np.float32)
    keys = orc.rank_key(vals).astype(np.int64)
    assert np.all(np.diff(keys) > 0)                              # -0.0 below +0.0, NaN above +inf
    assert orc.rank_key(np.float32(-0.0)) != orc.rank_key(np.float32(0.0))


CASES = {
    "ties": (np.array([[1, 1, 1, 1, 0, 2, 2, 0], [5, 5, 5, 5, 5, 5, 5, 5]], dtype=np.float32),
             [[0, 3, 5, 6], [7, 0]], [[1], []]),
    "special": (np.array([[NAN, INF, -INF, -0.0, 0.0, 3.0, NAN, -2.0], [0.0, -0.0, 0.0, -0.0, INF, INF, -INF, NAN]], dtype=np.float32),
                [[0, 2, 3, 4, 6], [0, 1, 5, 7]], [[5], [4, 2]]),
    "empty rows, excluded and out-of-range targets, duplicates": (
        np.array([[3, 1, 2, 0, 1], [0, 0, 0, 0, 0], [4, 3, 2, 1, 0]], dtype=np.float32),
        [[], [1, 1, 2, -4, 9], [0, 4]], [[0, 1], [2, 3], [0, 1, 2, 3]]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_lexsort_positions_equal_the_double_loop(name):
    scores, truth, excl = CASES[name]
    fast, slow = orc.positions(scores, truth, excl), orc.positions_brute(scores, truth, excl)
    assert [p.tolist() for p in fast] == [p.tolist() for p in slow]
    fast, slow = orc.positions(scores, truth), orc.positions_brute(scores, truth)
    assert [p.tolist() for p in fast] == [p.tolist() for p in slow]


def test_positions_written_out():
    scores, truth, excl = CASES["ties"]
    # user 0, item 1 excluded: eligible order is 5 6 0 2 3 4 7 (score 2 2 1 1 1 0 0, ties by item)
    assert orc.positions(scores, truth, excl)[0].tolist() == [2, 4, 0, 1]
    assert orc.positions(scores, truth, excl)[1].tolist() == [7, 0]
    scores, truth, excl = CASES["special"]
    # user 0, item 5 excluded: NaN(0) NaN(6) inf(1) +0(4) -0(3) -2(7) -inf(2)
    assert orc.positions(scores, truth, excl)[0].tolist() == [0, 6, 4, 3, 1]
    scores, truth, excl = CASES["empty rows, excluded and out-of-range targets, duplicates"]
    got = orc.positions(scores, truth, excl)
    assert got[0].tolist() == [] and got[1].tolist() == [1, 1, -1, -1, -1] and got[2].tolist() == [-1, 0]


def test_metrics_hand_computed():
    # 10 items, 2 excluded (E = 8); held-out ids {1, 4, 4, 7, 9}: T = 4; item 9 is excluded (-1); positions 0, 3, 3, 5
    pos = [np.array([0, 3, 3, 5, -1])]
    truth = [np.array([1, 4, 4, 7, 9])]
    pu, sums = orc.metrics(pos, truth, [2], 10, [1, 4, 10])
    l2 = math.log2
    idcg4 = 1 / l2(2) + 1 / l2(3) + 1 / l2(4) + 1 / l2(5)
    want = [1.0,                                                    # rr
            (1 / 1 + 2 / 4 + 3 / 6) / 4,                            # ap
            (1 / l2(2) + 1 / l2(5) + 1 / l2(7)) / idcg4,            # ndcg
            ((4 - 0) + (4 - 2) + (4 - 3)) / (4 * 4),                # auc: negatives below each valid target; the miss adds 0
            1 / 4, (1 / l2(2)) / (1 / l2(2)), 1 / 1, 1.0,           # @1
            2 / 4, (1 / l2(2) + 1 / l2(5)) / idcg4, 2 / 4, 1.0,     # @4
            3 / 4, (1 / l2(2) + 1 / l2(5) + 1 / l2(7)) / idcg4, 3 / 10, 1.0]   # @10
    assert pu[0].tolist() == pytest.approx(want, rel=1e-15)
    assert sums.tolist() == pytest.approx(want + [1.0, 1.0], rel=1e-15)
    # an unevaluated user (T = 0) adds nothing; a user with E == T counts in users, not in auc_users
    pu, sums = orc.metrics([np.array([]), np.array([1, 0])], [np.array([]), np.array([0, 1])], [0, 8], 10, [1])
    assert pu[0].tolist() == [0.0] * 8 and sums[-2] == 1.0 and sums[-1] == 0.0 and pu[1][3] == 0.0
    assert pu[1][0] == 1.0 and pu[1][1] == 1.0 and pu[1][2] == pytest.approx(1.0)


def test_metrics_against_independent_statements():
    rng = np.random.default_rng(11)
    B, n_items = 40, 60
    scores = rng.integers(-2, 3, (B, n_items)).astype(np.float32)           # plenty of ties
    truth, excl = [], []
    for b in range(B):
        perm = rng.permutation(n_items)
        n_t, n_x = [0, 1, 3, 9][b % 4], int(rng.integers(0, 12))
        truth.append(np.sort(perm[:n_t]))
        excl.append(np.sort(perm[n_t:n_t + n_x]))                           # disjoint from the truth
    pos = orc.positions(scores, truth, excl)
    ks = [1, 5, n_items]
    pu, sums = orc.metrics(pos, truth, [len(x) for x in excl], n_items, ks)
    users = 0
    for b in range(B):
        T = set(truth[b].tolist())
        if not T:
            assert not pu[b].any()
            continue
        users += 1
        ok = np.ones(n_items, dtype=bool)
        ok[excl[b]] = False
        key = [int(k) for k in orc.rank_key(scores[b])]
        ranked = sorted(np.nonzero(ok)[0].tolist(), key=lambda i: (-key[i], i))     # the user's full list
        rel = [i in T for i in ranked]
        first = rel.index(True)
        assert pu[b, 0] == pytest.approx(1.0 / (first + 1), rel=1e-14)
        prec_at_hits = [sum(rel[:n + 1]) / (n + 1) for n in range(len(ranked)) if rel[n]]
        assert pu[b, 1] == pytest.approx(sum(prec_at_hits) / len(T), rel=1e-14)
        dcg = sum(1 / math.log2(n + 2) for n in range(len(ranked)) if rel[n])
        assert pu[b, 2] == pytest.approx(dcg / sum(1 / math.log2(j + 2) for j in range(len(T))), rel=1e-14)
        negatives = [i for i in ranked if i not in T]
        right = sum(1 for t in T for i in negatives if orc.rank_before(key[t], t, key[i], i))    # pair by pair
        assert pu[b, 3] == pytest.approx(right / (len(T) * len(negatives)), rel=1e-14)
        for q, K in enumerate(ks):
            hits = sum(rel[:K])
            idcg = sum(1 / math.log2(j + 2) for j in range(min(K, len(T))))
            want = [hits / len(T), sum(1 / math.log2(n + 2) for n in range(min(K, len(ranked))) if rel[n]) / idcg, hits / K, float(hits > 0)]
            assert pu[b, 4 + 4 * q:8 + 4 * q].tolist() == pytest.approx(want, rel=1e-14)
        assert pu[b, 4 + 4 * 2] == 1.0                                      # recall at K = n_items
    assert sums[-2] == users and sums[-1] == users
    assert sums[:-2].tolist() == pytest.approx(pu.sum(0).tolist(), rel=1e-13)
