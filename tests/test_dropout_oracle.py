"""The exact node-dropout oracle (tests/dropout_oracle.py) checked on the CPU: the threshold contract of include/ngcf_hip.h on the
entries where the float and the double reading of p = 0.3 disagree, the properties of the mask, the integer product against a dense
fp64 product, the seed step against literals worked out with Python integers, and the shapes the GPU tests rely on."""
import numpy as np
import pytest

import dropout_oracle as orc

M64 = (1 << 64) - 1
# (row, column, seed) whose hash lies in [int(0.3 * 2^32), int(float32(0.3) * 2^32)) = [1288490188, 1288490240): kept under the
# double reading of p = 0.3, dropped under the library's float reading.  Found by search on the CPU; the hashes are pinned below.
WITNESSES = [(3, 5, 8261496, 1288490193), (3, 5, 42259290, 1288490218), (3, 5, 101166772, 1288490238),
             (3, orc.S_USERS + 5, 17281162, 1288490203), (3, orc.S_USERS + 5, 123665870, 1288490232)]


def _hash_py(row, col, seed):
    """edge_keep's hash of csrc/common.h in Python integers (no numpy)."""
    x = (seed & M64) ^ ((((row << 32) | (col & 0xFFFFFFFF)) * 0x9E3779B97F4A7C15) & M64)
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x & 0xFFFFFFFF


@pytest.mark.parametrize("row,col,seed,want_hash", WITNESSES)
def test_threshold_is_the_float_reading_of_p(row, col, seed, want_hash):
    assert _hash_py(row, col, seed) == want_hash == int(orc.edge_hash(row, col, seed)[0])
    thr_double, thr_float = int(float(np.float64(0.3)) * 2 ** 32), int(float(np.float32(0.3)) * 2 ** 32)
    assert (thr_double, thr_float) == (1288490188, 1288490240) and orc.drop_threshold(0.3) == thr_float
    assert thr_double <= want_hash < thr_float                    # kept at the double 0.3, dropped at the float 0.3
    assert not orc.keep_mask([row], [col], [seed], 0.3)[0]        # the oracle follows the library: dropped
    assert not orc.keep_mask([col], [row], [seed], 0.3, transposed=True)[0]
    assert orc.keep_mask([row], [col], [seed], 0.25)[0] and orc.keep_mask([row], [col], [seed], 0.0)[0]


@pytest.mark.parametrize("row,col,seed", [(3, 5, 2668215134), (3, orc.S_USERS + 5, 11307657986)])
def test_hash_equal_to_the_threshold_is_kept(row, col, seed):
    """Seeds (found by search) whose hash is exactly the threshold of float32(0.3): kept iff hash >= threshold."""
    assert _hash_py(row, col, seed) == 1288490240 == orc.drop_threshold(0.3)
    assert orc.keep_mask([row], [col], [seed], 0.3)[0] and orc.keep_mask([col], [row], [seed], 0.3, transposed=True)[0]
    assert not orc.keep_mask([row], [col], [seed], np.nextafter(np.float32(0.3), np.float32(1)))[0]


def test_hash_matches_python_integers_on_random_keys_and_extreme_seeds():
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, 2 ** 31 - 1, 200), rng.integers(0, 2 ** 31 - 1, 200)
    for seed in (0, 1, 2 ** 62 - 1, 2 ** 63, M64, 0xC2B2AE3D27D4EB4F, -5):
        got = orc.edge_hash(rows, cols, seed)
        assert [int(g) for g in got] == [_hash_py(int(r), int(c), seed) for r, c in zip(rows, cols)]


def test_mask_properties():
    rng = np.random.default_rng(11)
    n = 200_000
    rows, cols = rng.integers(0, 50_000, n), rng.integers(0, 50_000, n)
    seeds = [2 ** 62 - 1, 0xC2B2AE3D27D4EB4F, 0, 123456789]
    for p in (0.25, 0.3, 0.9):
        prev = np.ones(n, bool)
        for k in range(1, 5):
            keep = orc.keep_mask(rows, cols, seeds[:k], p)
            assert not (keep & ~prev).any()                        # cumulative: seeds[:k] keeps a subset of seeds[:k-1]
            assert np.array_equal(keep, orc.keep_mask(cols, rows, seeds[:k], p, transposed=True))
            q = (1.0 - orc.drop_threshold(p) / 2 ** 32) ** k
            assert abs(keep.mean() - q) <= 4.0 * np.sqrt(q * (1 - q) / n), (p, k)
            prev = keep
    assert orc.keep_mask(rows, cols, seeds, 0.0).all() and orc.keep_mask(rows, cols, [], 0.3).all()
    # entries stored twice share one fate; the key is (row, column), not the position
    keep = orc.keep_mask(np.r_[rows, rows[::-1]], np.r_[cols, cols[::-1]], seeds[:2], 0.3)
    assert np.array_equal(keep[:n], keep[n:][::-1])
    assert not np.array_equal(orc.keep_mask(rows, cols, seeds[:1], 0.3), orc.keep_mask(cols, rows, seeds[:1], 0.3))


def test_exact_product_equals_dense_fp64():
    rng = np.random.default_rng(3)
    n_rows, n_cols, nnz, d = 50, 40, 700, 9
    rows, cols, vals = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz), rng.integers(1, 4, nnz)
    rows[rows == 17] = 18                                          # an empty row
    X = rng.integers(1, 9, (n_cols, d)) * rng.choice(np.array([-1, 1]), (n_cols, d))
    for keep in (None, orc.keep_mask(rows, cols, [7, 8], 0.3), np.zeros(nnz, bool)):
        A = np.zeros((n_rows, n_cols))
        sel = slice(None) if keep is None else keep
        np.add.at(A, (rows[sel], cols[sel]), vals[sel].astype(np.float64))      # duplicates add up
        got = orc.spmm_exact(rows, cols, vals, X, keep, n_rows=n_rows)
        assert got.dtype == np.int64 and np.array_equal(got.astype(np.float64), A @ X.astype(np.float64))
        assert not got[17].any()
    with pytest.raises(AssertionError):
        orc.spmm_exact(rows, cols, vals * 0.5, X)


def test_seed_step_matches_literals_and_stays_below_2_62():
    # splitmix64 from state 0 gives 0xE220A8397B1DCDAF (the generator's published first output); the others by Python integers
    pairs = [(0, 0xE220A8397B1DCDAF >> 2), (2 ** 62 - 1, 0x10F7C22154DA5E29), (0xC2B2AE3D27D4EB4F, 0x37CC3CDBDAE474A7),
             (1234567, 0x1667B405FEC23F21)]
    got = orc.splitmix_advance([a for a, _ in pairs])
    assert got.dtype == np.uint64 and [int(g) for g in got] == [b for _, b in pairs]
    assert int(orc.splitmix_advance([-1])[0]) == int(orc.splitmix_advance([M64])[0])
    words = np.random.default_rng(1).integers(0, 2 ** 63, 5000, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    out = orc.splitmix_advance(words)
    assert int(out.max()) < 2 ** 62 and np.unique(out).size == out.size


def test_cases_have_the_shapes_the_gpu_tests_rely_on():
    S, W = orc.build_case("S"), orc.build_case("W")
    for c in (S, W, orc.build_case("tiny")):
        assert set(np.unique(c["vals"])) <= {1, 2, 3} and np.all(np.diff(c["rows"]) >= 0)
        assert np.abs(c["table"]).min() >= 1 and np.abs(c["table"]).max() <= 8 and c["table"].shape == (c["n_cols"], orc.TABLE_WIDTH)
        assert np.bincount(c["rows"]).max() * 3 * 8 < 2 ** 24       # every partial sum is an exactly represented integer
    cnt = np.bincount(S["rows"], minlength=S["n_rows"])
    assert S["n_rows"] == 1632 and [r for r in range(1632) if cnt[r] == 0] == list(orc.S_EMPTY_ROWS)
    users = S["rows"] < orc.S_USERS
    assert S["cols"][users].min() >= orc.S_USERS and S["cols"][~users].max() < orc.S_USERS      # user rows gather from the 96 item rows only
    assert 8 <= cnt[:orc.S_USERS][cnt[:orc.S_USERS] > 0].min() and cnt[:orc.S_USERS].max() <= 16 and cnt[orc.S_USERS:].min() >= 170
    assert np.unique(S["cols"][S["rows"] == orc.S_DUP_ROW]).size == 1 and cnt[orc.S_DUP_ROW] == 12
    assert ((S["rows"] == 3) & (S["cols"] == orc.S_USERS + 5)).any()
    cnt = np.bincount(W["rows"], minlength=W["n_rows"])
    assert W["n_rows"] == W["n_cols"] == 2048 and cnt.min() >= 8 and all(cnt[r] >= n for r, n in orc.W_HEAVY)
    assert W["cols"].min() < 64 and W["cols"].max() >= 2048 - 64
    key = W["rows"] * 2048 + W["cols"]
    assert key.size - np.unique(key).size >= W["rows"].size // 101   # entries stored twice
    Su = orc.build_case("Su")
    assert Su["n_cols"] == 96 and ((Su["rows"] == 3) & (Su["cols"] == 5)).any()
    for name, t_name in (("S", "St"), ("W", "Wt")):                   # the transposes hold the same entries
        a, b = orc.build_case(name), orc.build_case(t_name)
        ka = np.sort(a["rows"] * 4096 * 3 + a["cols"] * 3 + a["vals"] - 1)
        kb = np.sort(b["cols"] * 4096 * 3 + b["rows"] * 3 + b["vals"] - 1)
        assert np.array_equal(ka, kb) and np.array_equal(a["table"], b["table"])
    assert np.bincount(orc.build_case("St")["rows"]).max() > 64       # St has cut rows too
