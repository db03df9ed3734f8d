"""The per-group selection on the device (csrc/select.hip, engine.select_per_group) and the two splits built on it
(preprocess.split_by_year / split_stratified) against the numpy oracle of tests/split_oracle.py: integer work throughout, so the
mask and the thresholds are compared for equality, bit for bit."""
import numpy as np
import pytest
import torch

import split_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_BIG = 70_001                       # nine chunks of 8 192 rows: several workgroups, and a ragged tail of 4 465 rows

# Seeds found on the host with the oracle (tests/split_oracle.py; `_branch_case` below, seeds 0, 1, 2, ... until the first hit): at
# SEED_LOW one group's tau ends in the byte 0x00 and another's in 0xFF; at SEED_MID the same holds for byte 3 (bits 24..31).  Bin 0
# and bin 255 are the ends of the pick's scan over a pass's 256 bins.
SEED_LOW, SEED_MID = 11, 5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _limit():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.select_limits()[0]


def _check(group, quota, seed, n_rows=None, **kw):
    """One call against the oracle: the mask, the thresholds, and the quotas met exactly."""
    from seoul_tourism_recommendation_ngcf_amd import engine
    want_mask, want_tau = orc.select(group, quota, seed, n_rows=n_rows)
    g = None if group is None else _dev(np.asarray(group, dtype=np.int32))
    mask, tau = engine.select_per_group(g, quota, seed=seed, n_rows=n_rows, return_thresholds=True, **kw)
    assert mask.dtype == torch.uint8 and tau.dtype == torch.int64
    got_mask, got_tau = mask.cpu().numpy(), tau.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_tau, want_tau), (seed, kw)
    assert np.array_equal(got_mask, want_mask), (seed, kw)
    if group is not None and len(group):
        assert np.array_equal(np.bincount(group, weights=got_mask, minlength=len(quota)).astype(np.int64), np.asarray(quota))
    return mask


def _quotas(sizes, rs):
    """0, 1, n - 1, n and random quotas in turn over the groups that have rows; 0 for the empty ones."""
    quota = np.zeros(len(sizes), dtype=np.int64)
    for j, g in enumerate(np.flatnonzero(sizes)):
        n = int(sizes[g])
        quota[g] = (0, 1, n - 1, n, int(rs.randint(0, n + 1)))[j % 5]
    return quota


def _branch_case(seed):
    rs = np.random.RandomState(11)
    group = rs.randint(0, 100, T_BIG)
    sizes = np.bincount(group, minlength=100)
    quota = np.array([int(rs.randint(1, n)) for n in sizes])
    return group, quota, orc.select(group, quota, seed)[1]


def test_edges_no_rows_one_row_and_no_group_vector():
    from seoul_tourism_recommendation_ngcf_amd import engine
    mask = _check(None, [0], 3, n_rows=0)
    assert mask.numel() == 0
    mask = _check(np.zeros(0, np.int64), [0, 0, 0], 3)                       # no rows, three groups
    assert mask.numel() == 0
    assert _check(None, [0], 4, n_rows=1).tolist() == [0]
    assert _check(None, [1], 4, n_rows=1).tolist() == [1]
    assert _check(np.array([2]), [0, 0, 1], 4).tolist() == [1]
    for T in (63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193):                # around a wave, a workgroup and a chunk
        for quota in (0, 1, T // 3, T - 1, T):
            _check(None, [quota], 100 + T, n_rows=T)
    plain = engine.select_per_group(None, [5], seed=8, n_rows=40)             # without thresholds: the mask alone
    assert isinstance(plain, torch.Tensor) and int(plain.sum()) == 5
    assert torch.equal(plain, engine.select_per_group(torch.zeros(40, dtype=torch.int32, device=DEV), [5], seed=8))


def test_quota_edges_and_empty_groups():
    rs = np.random.RandomState(0)
    group = rs.choice([0, 1, 2, 4, 5, 7, 8, 9, 11], 3001)                    # groups 3, 6, 10 and 12 have no rows
    sizes = np.bincount(group, minlength=13)
    quota = _quotas(sizes, rs)
    assert {0, 1}.issubset(quota.tolist()) and any(quota[g] == sizes[g] > 0 for g in range(13))
    assert any(quota[g] == sizes[g] - 1 for g in range(13))
    _check(group, quota, 21)
    _check(group, sizes, 22)                                                 # every row of every group
    _check(group, np.zeros(13, np.int64), 23)                                # nothing at all
    mask = _check(np.sort(group), quota, 21)                                 # contiguous groups are just another order
    assert int(mask.sum()) == int(quota.sum())


@pytest.mark.parametrize("G", [1, 3, 100, "limit", "limit+1", 5000])
def test_launch_geometry_against_the_oracle(G):
    lim = _limit()
    G = {"limit": lim, "limit+1": lim + 1}.get(G, G)
    rs = np.random.RandomState(G)
    if G == 5000:
        group = rs.choice(rs.choice(G, 40, replace=False), T_BIG)            # most groups empty
        group[:2] = (0, G - 1)                                               # the first and the last group have a row
    else:
        group = rs.randint(0, G, T_BIG)
    sizes = np.bincount(group, minlength=G)
    _check(group, _quotas(sizes, rs), 1000 + G)
    if G == 1:
        _check(None, [T_BIG * 3 // 10], 1001, n_rows=T_BIG)


def test_one_group_holds_most_rows():
    rs = np.random.RandomState(5)
    group = np.where(rs.rand(T_BIG) < 0.95, 3, rs.randint(0, 8, T_BIG))
    sizes = np.bincount(group, minlength=8)
    assert sizes[3] > 0.94 * T_BIG
    for q3 in (1, sizes[3] * 3 // 10, sizes[3]):                             # quota 1 and n_g in a large group: tau's top byte 0x00, 0xFF
        quota = np.array([2, 0, sizes[2], q3, 1, 7, 0, sizes[7] - 1])
        want = orc.select(group, quota, 77)[1]
        if q3 == 1:
            assert int(want[3]) >> 56 == 0x00
        if q3 == sizes[3]:
            assert int(want[3]) >> 56 == 0xFF
        _check(group, quota, 77)


def test_radix_branch_points_first_and_last_bin_in_low_and_middle_bytes(lib_options):
    for seed, shift in ((SEED_LOW, 0), (SEED_MID, 24)):
        group, quota, tau = _branch_case(seed)
        digits = {(int(t) >> shift) & 0xff for t in tau}
        assert 0x00 in digits and 0xFF in digits, (seed, shift)              # the recorded seeds do what they were recorded for
        _check(group, quota, seed)
        lib_options(select_no_lds=1)
        _check(group, quota, seed)
        lib_options(select_no_lds=0)


def test_two_runs_and_both_tiers_give_the_same_mask(lib_options):
    from seoul_tourism_recommendation_ngcf_amd import engine
    rs = np.random.RandomState(9)
    group = _dev(rs.randint(0, 100, T_BIG).astype(np.int32))
    quota = np.bincount(group.cpu().numpy(), minlength=100) * 3 // 10
    a, ta = engine.select_per_group(group, quota, seed=31, return_thresholds=True)
    b, tb = engine.select_per_group(group, quota, seed=31, return_thresholds=True)
    assert torch.equal(a, b) and torch.equal(ta, tb)
    lib_options(select_no_lds=1)                                             # the memory tier at G = 100
    c, tc = engine.select_per_group(group, quota, seed=31, return_thresholds=True)
    assert torch.equal(a, c) and torch.equal(ta, tc)
    lib_options(select_no_lds=0)
    other = engine.select_per_group(group, quota, seed=32)
    assert int(other.sum()) == int(a.sum()) == int(quota.sum()) and not torch.equal(a, other)
    out = torch.full((T_BIG,), 7, dtype=torch.uint8, device=DEV)
    assert engine.select_per_group(group, quota, seed=31, out=out) is out and torch.equal(out, a)


def test_status_word_raises_and_marks_nothing():
    from seoul_tourism_recommendation_ngcf_amd import engine
    rs = np.random.RandomState(2)
    group = rs.randint(0, 4, 5000).astype(np.int32)
    sizes = np.bincount(group, minlength=4)
    quota = sizes // 2
    for bad in (4, -1, 2 ** 31 - 1, -2 ** 31):                               # ordinary argument errors: an id of G, a negative id
        g = group.copy()
        g[1234] = bad
        out = torch.full((5000,), 1, dtype=torch.uint8, device=DEV)
        with pytest.raises(IndexError, match="outside \\[0, 4\\)"):
            engine.select_per_group(_dev(g), quota, seed=5, out=out)
        assert int(out.sum()) == 0                                           # nothing is marked
    over = quota.copy()
    over[2] = sizes[2] + 1
    out = torch.full((5000,), 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="larger than its group's row count"):
        engine.select_per_group(_dev(group), over, seed=5, out=out)
    got = out.cpu().numpy()                                                  # no row of the flagged group; the others as asked
    assert np.array_equal(np.bincount(group, weights=got, minlength=4).astype(np.int64), np.where(np.arange(4) == 2, 0, quota))
    with pytest.raises(ValueError, match="larger than its group's row count"):
        engine.select_per_group(None, [1], seed=5, n_rows=0)
    with pytest.raises(ValueError, match="larger than its group's row count"):
        engine.select_per_group(_dev(group), [1, 1, 1, 1, 1], seed=5)         # group 4 has no rows
    _check(group, quota, 5)                                                  # and the same rows pass when the arguments are right


@pytest.fixture(scope="module")
def frame():
    """3 000 rows with years {18, 19, 20}, 7 strata, and ids for the samplers."""
    rs = np.random.RandomState(17)
    T = 3000
    return {"year": rs.choice([18, 19, 20], T, p=[0.45, 0.45, 0.1]).astype(np.int64), "strata": rs.choice(7, T, p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.06, 0.04]),
            "users": rs.randint(0, 50, T).astype(np.int64), "T": T}


def test_split_by_year_against_the_oracle(frame):
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    year = frame["year"]
    rows = np.arange(frame["T"])
    n19 = int((year == 19).sum())
    for yt in (_dev(year), _dev(year.astype(np.int32))):
        train, test = preprocess.split_by_year(yt, seed=2024)
        assert train.dtype == test.dtype == torch.int64 and train.device == test.device == yt.device
        train, test = train.cpu().numpy(), test.cpu().numpy()
        assert len(test) == preprocess.year_quota(n19) == round(0.3 * n19)
        assert len(np.intersect1d(train, test)) == 0
        assert np.array_equal(np.sort(np.concatenate([train, test])), rows[year != 20])        # year 20 is in neither part
        assert np.all(year[test] == 19) and np.all(np.diff(test) > 0)                          # the sample, in row order
        n18 = int((year == 18).sum())
        assert np.array_equal(train[:n18], rows[year == 18])                                   # all of 18 first, in row order,
        assert np.all(year[train[n18:]] == 19) and np.all(np.diff(train[n18:]) > 0)            # then the rest of 19 in row order
        want, _ = orc.select((year != 19).astype(np.int64), [len(test), 0], 2024)
        assert np.array_equal(test, np.flatnonzero(want))
    tr2, te2 = preprocess.split_by_year(_dev(year), train_year=19, test_year=18, frac=0.5, seed=1)
    assert len(te2) == round(0.5 * int((year == 18).sum())) and np.all(year[te2.cpu().numpy()] == 18)
    tr3, te3 = preprocess.split_by_year(_dev(year), test_year=21, seed=1)                       # a year without rows: nothing to test
    assert te3.numel() == 0 and np.array_equal(tr3.cpu().numpy(), rows[year == 18])


def test_split_stratified_against_the_oracle(frame):
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    strata = frame["strata"]
    sizes = np.bincount(strata, minlength=7)
    want_train, want_test = preprocess.stratified_counts(sizes, 0.3, seed=7)
    train, test = preprocess.split_stratified(_dev(strata), seed=7)
    assert train.dtype == test.dtype == torch.int64
    train, test = train.cpu().numpy(), test.cpu().numpy()
    assert len(np.intersect1d(train, test)) == 0
    assert np.array_equal(np.sort(np.concatenate([train, test])), np.arange(frame["T"]))
    assert np.all(np.diff(train) > 0) and np.all(np.diff(test) > 0)
    assert np.array_equal(np.bincount(strata[test], minlength=7), want_test)
    assert np.array_equal(np.bincount(strata[train], minlength=7), want_train)
    assert len(test) == int(np.ceil(0.3 * frame["T"]))
    want, _ = orc.select(strata, want_test, 7)
    assert np.array_equal(test, np.flatnonzero(want)) and np.array_equal(train, np.flatnonzero(want == 0))
    # class ids with gaps: sklearn numbers the classes that occur
    sparse = np.array([0, 3, 4, 9, 10, 11, 20])[strata]
    tr2, te2 = preprocess.split_stratified(_dev(sparse.astype(np.int32)), seed=7)
    assert np.array_equal(te2.cpu().numpy(), test) and np.array_equal(tr2.cpu().numpy(), train)
    with pytest.raises(ValueError, match="fewer than 2 rows"):
        preprocess.split_stratified(_dev(np.array([0, 0, 0, 1, 2, 2])), seed=0)


def test_split_indices_feed_the_samplers(frame):
    from seoul_tourism_recommendation_ngcf_amd import engine, preprocess, sampling
    n_user, n_item = 50, 7
    users, items = _dev(frame["users"]), _dev(frame["strata"].astype(np.int64))
    train, test = preprocess.split_by_year(_dev(frame["year"]), seed=3)
    seen = engine.ItemSets.from_pairs(users, items, n_user, 40)
    u, i, neg = sampling.train_triplets(users[train], items[train], seen, seed=1, n_user=n_user, n_item=40)
    assert u.numel() == i.numel() == neg.numel() == train.numel()
    cand = sampling.test_candidates(users[test], items[test], seen, m=24, seed=1, n_user=n_user, n_item=40)
    assert tuple(cand.shape) == (test.numel(), 25) and torch.equal(cand[:, 0], items[test])
