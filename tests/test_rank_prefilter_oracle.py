"""CPU tests of tests/prefilter_oracle.py, the numpy statement of the certified two-stage ranking: its arithmetic primitives against
independent ones, ub >= s on every pair of the tables the GPU tests run on, and certified answers = a brute-force exact top-k."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import prefilter_oracle as po

TABLES = {
    "gauss33": lambda: po.gaussian_tables(9, 300, 33, 1),
    "gauss64": lambda: po.gaussian_tables(9, 700, 64, 2),
    "gauss130": lambda: po.gaussian_tables(5, 300, 130, 3),
    "head64": lambda: po.popular_head_tables(9, 700, 64, 4),
}


def test_bf16_is_round_to_nearest_even_and_fma_is_correctly_rounded():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 20, 4096))).astype(np.float32)
    x[:4] = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 0.0], dtype=np.float32)    # ties: to even
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(po.bf16_rne(x), want)
    assert po.bf16_rne(x[:4]).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, 0.0]
    assert np.all(np.abs(po.bf16_rne(x).astype(np.float64) - x) <= 2.0 ** -8 * np.abs(x.astype(np.float64)))
    a, b, c = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    c[:500] = (-a[:500].astype(np.float64) * b[:500]).astype(np.float32)                                 # cancellation
    got = po.fma32(a, b, c)
    for j in range(2000):
        exact = Fraction(float(a[j])) * Fraction(float(b[j])) + Fraction(float(c[j]))
        lo, hi = np.nextafter(got[j], np.float32(-np.inf)), np.nextafter(got[j], np.float32(np.inf))
        assert abs(Fraction(float(got[j])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    assert Fraction(po.beta(512)) == Fraction(1, 2 ** 7) + Fraction(1, 2 ** 16) + Fraction(4 * 512 + 2, 2 ** 24)       # exact in float64


def test_keys_and_rounding_up():
    x = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-30, 2.0, np.inf], dtype=np.float32)
    k = po.float_key(x)
    assert np.all(k[1:] > k[:-1]) and po.float_key(np.array([np.nan], dtype=np.float32))[0] > k[-1]
    v = np.array([0.0, 1.0, 1.0 + 2.0 ** -30, 3.3], dtype=np.float64)
    up = po.round_up(v)
    assert up.dtype == np.float32 and np.all(up.astype(np.float64) > v) and up[1] == np.float32(1.0 + 2.0 ** -23)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_upper_bound_holds_on_every_pair(name):
    U, I = TABLES[name]()  # noqa: E741
    s = po.chain_scores(U, I)
    ub, approx = po.upper_bounds(U, I)
    assert np.all(ub >= s)
    s64 = U.astype(np.float64) @ I.astype(np.float64).T
    norms = np.linalg.norm(U.astype(np.float64), axis=1)[:, None] * np.linalg.norm(I.astype(np.float64), axis=1)[None, :]
    b = po.beta(U.shape[1])
    assert np.all(np.abs(approx - s) <= b * norms) and np.all(np.abs(s - s64) <= U.shape[1] * 2.0 ** -24 * norms)
    assert float((np.abs(approx - s) / norms).max()) <= 0.5 * b       # observed error: a fraction of the bound


@pytest.mark.parametrize("name,k,pool", [("gauss33", 1, 32), ("gauss64", 20, 128), ("gauss64", 20, 64), ("gauss130", 100, 256),
                                         ("head64", 20, 128), ("gauss33", 256, 256)])
def test_certified_answers_equal_the_exact_topk(name, k, pool):
    U, I = TABLES[name]()  # noqa: E741
    rng = np.random.default_rng(7)
    excluded = [np.sort(rng.choice(I.shape[0], size, replace=False)) for size in
                rng.choice([0, 5, I.shape[0] - 3, I.shape[0] - pool + 5, I.shape[0]], U.shape[0])]
    for ex in (None, excluded):
        want_v, want_i = po.exact_topk(U, I, k, ex)
        v, i, cert = po.certified_topk(U, I, k, pool, ex)
        assert cert.any() or (k == pool and ex is None)               # k = pool: only a pool that is not full certifies
        assert np.array_equal(v[cert].view(np.uint32), want_v[cert].view(np.uint32)) and np.array_equal(i[cert], want_i[cert])
        if ex is not None:                                            # a pool that is not full is always certified
            short = np.array([I.shape[0] - len(e) < pool for e in ex])
            assert cert[short].all()
    if name.startswith("gauss") and pool >= 64 and k <= 20:
        assert cert.all()


def test_the_cluster_defeats_the_certificate_and_only_the_certificate():
    U, I = po.cluster_tables(B=64)  # noqa: E741
    want_v, want_i = po.exact_topk(U, I, 20)
    v, i, cert = po.certified_topk(U, I, 20, 128)
    differs = (i != want_i).any(1)
    assert cert[1::2].all() and not cert[0::2].any()                 # exactly the users that rank the cluster on top
    assert differs.mean() >= 0.25 and not differs[cert].any()        # the pool's own answer is wrong for most of them: the fallback is needed


@pytest.mark.parametrize("bad", po.IRREGULAR)
def test_irregular_rows_are_never_certified(bad):
    U, I = po.gaussian_tables(6, 300, 33, 9)  # noqa: E741
    U2 = U.copy()
    U2[2, 5] = bad
    with np.errstate(invalid="ignore", over="ignore"):
        cert = po.certified_topk(U2, I, 10, 64)[2]
        assert not cert[2] and cert[[0, 1, 3, 4, 5]].all()
        I2 = I.copy()
        I2[17, 0] = bad
        assert not po.certified_topk(U, I2, 10, 64)[2].any()
