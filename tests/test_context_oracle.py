"""The trip-context oracles (tests/context_oracle.py) checked on the CPU: the sequential Kahan sum against `pd.pivot_table` bit for bit
on the very inputs the GPU tests use, the discrimination those inputs must have, the two host evaluations of the haversine formula,
the party loop and the dense ranks."""
import math

import numpy as np
import pytest

import context_oracle as orc

pd = pytest.importorskip("pandas")

DAYS3 = ((7, 30, 2), (7, 31, 3), (8, 1, 4))


@pytest.mark.parametrize("with_order", [False, True])
@pytest.mark.parametrize("n_values", [1, 2])
def test_kahan_oracle_equals_pandas_on_the_gpu_cases_and_a_plain_sum_does_not(n_values, with_order):
    rowptr, order, labels, columns, want, plain = orc.kahan_case(n_values, with_order)
    lengths = np.diff(rowptr)
    assert sorted(lengths.tolist()) == sorted(list(orc.SEGMENT_LENGTHS) + [5, 70]) and rowptr[-1] <= 20000
    names = [f"v{k}" for k in range(n_values)]
    df = pd.DataFrame({"g": labels, **{n: c for n, c in zip(names, columns)}})
    got = pd.pivot_table(df, index=["g"], aggfunc={n: "sum" for n in names})
    present = np.nonzero(lengths)[0]
    assert got.index.tolist() == present.tolist()
    for n, w, p in zip(names, want, plain):
        assert orc.same_bits(got[n].values, w[present])
        assert orc.same_bits(df.groupby("g")[n].sum().values, w[present])
        assert (w[lengths == 0] == 0).all() and np.signbit(w[lengths == 0]).sum() == 0
        long = lengths >= 64
        assert (w[long].view(np.int64) != p[long].view(np.int64)).any()                  # dropping the compensation shows
    # the special segments: all NaN -> 0.0; +inf first, then finite values -> +inf through the c != c reset
    pos = np.arange(len(labels)) if order is None else order
    for u in range(len(lengths)):
        x = columns[0][pos[rowptr[u]:rowptr[u + 1]]]
        if len(x) == 5:
            assert np.isnan(x).all() and want[0][u] == 0.0
        if len(x) == 70:
            assert x[0] == np.inf and np.isfinite(x[1:]).all() and want[0][u] == np.inf


def test_kahan_recurrence_by_hand():
    assert orc.kahan([]) == 0.0 and orc.kahan([np.nan, np.nan]) == 0.0
    assert orc.kahan([1e16, 1.0, 1.0]) == 1e16 + 2 and orc.naive([1e16, 1.0, 1.0]) == 1e16
    assert orc.kahan([np.inf, 1.0, -2.0]) == np.inf and math.isnan(orc.kahan([np.inf, -np.inf]))
    assert orc.kahan([1.0, np.nan, 2.0]) == 3.0


def test_pivot_oracle_equals_pandas_pivot_table_on_the_gpu_log():
    for days, n_item in ((DAYS3, 130), (DAYS3 + ((8, 2, 5), (8, 3, 6)), 100)):
        log = orc.congestion_log(days, n_item)
        T = len(log["item"])
        assert 1000 < T <= 20000
        index = ["month", "day", "dayofweek", "item"]
        want = pd.pivot_table(pd.DataFrame(log), index=index, aggfunc={"congestion_1": "sum", "congestion_2": "sum"}).reset_index()
        keys, sums, inverse = orc.pivot_float([log[c] for c in index], [log["congestion_1"], log["congestion_2"]])
        assert len(want) == len(keys[0]) < len(days) * n_item                              # some pairs are absent
        for k, name in enumerate(index):
            assert np.array_equal(keys[k], want[name].values) and np.array_equal(keys[k][inverse], log[name])
        assert orc.same_bits(sums[0], want["congestion_1"].values) and orc.same_bits(sums[1], want["congestion_2"].values)
        table, tdays = orc.congestion_table(log, n_item, by=0)
        assert tdays.tolist() == [list(d) for d in sorted(days)] and table.shape == (len(days), n_item)
        assert np.isinf(table).sum() == len(days) * n_item - len(want)
        # the reference's per-day slice (demo.py:270-274): its item order is the table row's ascending order
        d = tdays[1]
        part = want.loc[(want["month"] == d[0]) & (want["day"] == d[1]) & (want["dayofweek"] == d[2])].set_index("item")
        part = part.sort_values(by="congestion_1", kind="stable")
        row = table[1]
        assert part.index.tolist() == [i for i in np.argsort(row, kind="stable").tolist() if row[i] != np.inf]


def test_two_host_evaluations_of_the_haversine_formula_agree_to_a_few_ulp():
    for kind in ("seoul", "globe"):
        dep, item = orc.points(kind, 3, 130)
        a, b = orc.haversine_numpy(dep, item), orc.haversine_math(dep, item)
        spread = orc.ulps(b, a).max()
        print(f"host spread numpy vs math, {kind}: {spread} ulp")
        assert spread <= 16, (kind, spread)
        assert a[0, 1] == 0.0 and b[0, 1] == 0.0 and np.array_equal(a[:, 2], a[:, 3])       # coincident points
        assert (a < 0.9 * orc.HALF_CIRCUMFERENCE_M).all()
    # a known distance: Lyon - Paris, the haversine package's own example (392.2172595594006 km)
    got = orc.haversine_math(np.array([[45.7597, 4.8422]]), np.array([[48.8567, 2.3508]]))[0, 0]
    assert abs(got - 392217.2595594006) < 1e-6
    nan = orc.haversine_numpy(np.array([[37.5, np.nan]]), np.array([[37.5, 127.0]]))
    assert nan[0, 0] == np.inf and orc.haversine_math(np.array([[37.5, np.nan]]), np.array([[37.5, 127.0]]))[0, 0] == np.inf


def test_party_loop_and_dense_ranks():
    rows = orc.party_loop([27, 61], [0, 1], 2, 29, 5, 3)
    assert rows == [[-1, 25, 0, 2, 28, 5], [-1, 25, 0, 3, 1, 6], [-1, 25, 0, 3, 2, 0],
                    [-1, 65, 1, 2, 28, 5], [-1, 65, 1, 3, 1, 6], [-1, 65, 1, 3, 2, 0]]
    with pytest.raises(KeyError):
        orc.party_loop([30], [0], 12, 31, 0, 2, user_dict={"3501231": 0})                 # '3501301': month 13
    got = orc.dense_ranks([[3.0, 1.0, np.inf, 1.0, np.nan, -2.0, 0.0, -0.0]])
    assert got.dtype == np.float32 and got[0, [0, 1, 3, 5, 6, 7]].tolist() == [3, 2, 2, 0, 1, 1]
    assert got[0, 2] == np.inf and np.isnan(got[0, 4])
