"""The dense layer's host oracle (tests/dense_oracle.py) checked on the CPU: the exact form against the fp64 form and against plain
Python integers, the 2^24 condition on every case the GPU file runs, the hash mask against Python integers and its drop rate, and
the coverage the case tables promise (importable and complete without a GPU)."""
import numpy as np
import pytest
import torch

import dense_oracle as do

M64 = (1 << 64) - 1


def _hash_py(seed, row, col):
    """msg_drop's hash of csrc/common.h in Python integers (no numpy)."""
    x = (seed & M64) ^ ((row * 0x9E3779B97F4A7C15 + col) & M64)
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x & 0xFFFFFFFF


def test_msg_keep_matches_python_integers_is_deterministic_and_drops_about_p():
    rows, cols = np.array([0, 1, 31, 32, 4099, 2 ** 31 + 7, 3_000_000_000]), np.array([0, 1, 31, 32, 127, 511])
    thr = int(float(np.float32(0.3)) * 2 ** 32)
    assert thr == 1288490240
    for seed in (0, 1, do.SEED_HI, 2 ** 63, M64, 2 ** 62 - 1):
        h = do.msg_hash(seed, rows, cols)
        want = np.array([[_hash_py(seed, int(r), int(c)) for c in cols] for r in rows], dtype=np.uint64)
        assert np.array_equal(h, want)
        assert np.array_equal(do.msg_keep(seed, rows, cols, 0.3), want >= thr)
        assert np.array_equal(do.msg_keep(seed, rows, cols, 0.3), do.msg_keep(seed, rows, cols, 0.3))
    assert do.SEED_HI >= 2 ** 63 and do.SEED_HI >> 48 != 0xD5ED
    for seed in (0, do.SEED_HI):
        keep = do.msg_keep(seed, np.arange(1000), np.arange(128), 0.3)
        assert abs(1 - keep.mean() - 0.3) < 0.01                 # 128 000 draws: 0.01 is 7.8 sigma
        assert do.msg_keep(seed, np.arange(1000), np.arange(128), 0.0).all()
        # a function of (row, column): a row subset reproduces the rows of the full mask
        sel = np.array([999, 3, 500])
        assert np.array_equal(do.msg_keep(seed, sel, np.arange(128), 0.3), keep[sel])
    assert not np.array_equal(do.msg_keep(0, np.arange(64), np.arange(64), 0.3), do.msg_keep(1, np.arange(64), np.arange(64), 0.3))
    assert not np.array_equal(do.msg_keep(0, np.arange(64), np.arange(64), 0.3), do.msg_keep(0, np.arange(64), np.arange(64), 0.3).T)


def test_keep_scale_is_formed_in_float32():
    ks = do.keep_scale(0.3)
    assert ks.dtype == np.float32
    assert np.float32(1.0) - np.float32(0.3) == np.float32(11744051 * 2.0 ** -24)          # the subtraction is exact
    assert float(ks) == float(np.float32(1.0 / (11744051 * 2.0 ** -24)))                   # one correctly rounded division
    assert float(ks) != 1 / 0.7 and do.keep_scale(0.0) == np.float32(1.0)


def test_exact_layer_matches_python_integers_on_a_tiny_case():
    LE, E, W1, b1, W2, b2 = do.exact_inputs(3, 5, 4, seed=1)
    keep = np.array([[True, False, True, True]] * 3)
    carry, M, scale = do.exact_layer(LE, E, W1, b1, W2, b2, p=0.3, keep=keep)
    for r in range(3):
        for j in range(4):
            m = sum((int(LE[r, k]) + int(E[r, k])) * int(W1[j, k]) + int(LE[r, k]) * int(E[r, k]) * int(W2[j, k]) for k in range(5))
            m += 2 * int(b1[j]) + int(b2[j])
            assert M[r, j] == m
            v = np.float32(m) if m >= 0 else np.float32(0.2) * np.float32(m)
            want = np.float32(v * do.keep_scale(0.3)) if keep[r, j] else np.float32(0)
            assert carry[r, j] == want and carry.dtype == np.float32
    assert (scale[:, 1] == 0).all() and (scale[:, 0] > 0).all()


@pytest.mark.parametrize("c", do.ALL_CASES, ids=do.case_id)
def test_every_gpu_case_meets_the_2_24_condition_and_the_two_forms_agree(c):
    """exact_layer asserts |A|.|B| + |bias| < 2^24 itself; on these integer inputs the fp64 form gives the same values up to the
    float32 rounding of the activation (0.2f against 0.2, the keep scale: 3.3 units, see carry_k)."""
    (LE, E, W1, b1, W2, b2), keep, mask, carry, M, scale = do.case_expected(c)
    assert carry.shape == (c.n, c.d_out) and np.abs(M).max() < 2 ** 24
    t = [torch.from_numpy(a.astype(np.float32)) for a in (LE, E, W1, b1, W2, b2)]
    k = None if keep is None and mask is None else torch.from_numpy(keep if keep is not None else mask != 0)
    ref = do.fp64_layer(*t, keep=k)
    assert ref.err_carry(torch.from_numpy(carry)) <= 3.3 * do.U32
    if k is not None:
        assert np.array_equal(carry == 0, ~k.numpy() | (M == 0))
    for r in do.zero_rows_of(c):
        assert not carry[r].any()
    err, zero = do.norm_error(ref.nrm.float(), carry, scale)
    assert err <= do.norm_k(c.d_in, c.d_out)
    assert all(zero[r] for r in do.zero_rows_of(c))


def test_case_tables_cover_what_the_gpu_tests_promise():
    ids = [do.case_id(c) for c in do.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert {c.d_out for c in do.ALL_CASES} >= {1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 200, 256, 257, 512}
    assert {c.d_in for c in do.ALL_CASES} >= {1, 3, 4, 15, 16, 17, 65, 130, 144, 145, 515}
    assert max(c.n for c in do.ALL_CASES) <= 261 and max(c.d_out for c in do.ALL_CASES) == 512
    for path, (opts, T, d_outs, d_ins) in do.PADDED_PATHS.items():
        mine = [c for c in do.ALL_CASES if c.path == path and c.d_in != 145]
        assert {c.n for c in mine} == {1, T - 1, T, T + 1, 2 * T + 5}, path
        assert {c.d_out for c in mine} == set(d_outs) and {c.d_in for c in mine} == set(d_ins), path
        a, b, x = d_ins[:3]
        assert a % 16 == 0 and b % 4 == 0 and b % 16 != 0 and x % 4 != 0
        assert {c.mode for c in mine} == set(do.MODES), path
        P = d_outs[0]
        assert P in (32, 64, 96, 128, 256, 512) and d_outs[1] == P - 1
        full = {c.mode for c in mine if c.d_out == P and c.n >= T}                        # the full-tile arm runs
        guarded = {c.mode for c in mine if c.d_out < P or c.n % T}                        # the guarded arm runs
        assert full >= {"eval", "hash0", "mask", "last"} and guarded >= {"eval", "hash_hi", "mask"}, path
        assert sum(c.special for c in mine) == 1
    for cfg in do.STAGED_CONFIGS:
        assert {c.layout for c in do.ALL_CASES if c.path == cfg + "/unaligned"} == {"odd"}
        tight = [c for c in do.ALL_CASES if c.path == cfg + "/aligned"]
        assert tight and all(c.layout == "tight" and c.d_in < 4 for c in tight) and any(c.d_in == 3 for c in tight)
    assert {c.path for c in do.ALL_CASES if c.d_in == 145} == {"staged<1,4,1>/padded"}
    paths = {p for p, *_ in do.FP64_CASES}
    assert paths == {c.path for c in do.ALL_CASES} and len(do.FP64_CASES) == len(paths)
