"""CPU: the float64 oracle of the sampled softmax loss with logQ correction (tests/sampled_softmax_oracle.py) against central finite
differences of itself, against the multi-negative BPR oracle's softmax where the two definitions meet, and the two properties of the
correction that need no device: a per-row constant cancels, and one negative without correction is BPR's -logsigmoid."""
import numpy as np
import pytest

import bpr_multi_oracle as bpr_orc
import sampled_softmax_oracle as orc

SHAPES = [(1, 1, 1), (3, 2, 5), (4, 3, 65), (5, 24, 7), (2, 64, 3)]


def _case(B, m, D, seed, pos=True):
    rng = np.random.default_rng(seed)
    u, p, n = bpr_orc.cases(B, m, D, seed)
    logq = rng.uniform(-12.0, 0.0, (B, m))
    return u, p, n, logq, (rng.uniform(-12.0, 0.0, B) if pos else None)


def _logsigmoid(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


@pytest.mark.parametrize("tau", [1.0, 0.25])
@pytest.mark.parametrize("pos", [False, True])
@pytest.mark.parametrize("B,m,D", SHAPES)
def test_gradients_are_the_central_differences_of_the_loss(B, m, D, pos, tau):
    """(f(x + h) - f(x - h)) / 2h in float64 with h = 1e-6: truncation ~ h^2 f''' and rounding ~ eps |f| / h, both near 1e-10 for a
    loss of order 1 - held to 1e-7 of the largest gradient entry."""
    u, p, n, logq, pos_logq = _case(B, m, D, seed=31 * B + 7 * m + D, pos=pos)
    wd, bs, gout, h = 0.025, B + 3, 3.0, 1e-6
    args = [np.asarray(t, dtype=np.float64) for t in (u, p, n)]
    f = lambda: gout * orc.loss(*args, logq, m, 1 / tau, wd, bs, pos_logq)  # noqa: E731
    got = orc.grads(u, p, n, logq, m, 1 / tau, wd, bs, gout, pos_logq)
    rng = np.random.default_rng(B + m + D)
    for t, g in zip(args, got):
        assert g.shape == t.shape and np.isfinite(g).all()
        flat = t.reshape(-1)
        for i in rng.choice(flat.size, size=min(flat.size, 12), replace=False):
            keep = flat[i]
            flat[i] = keep + h
            hi = f()
            flat[i] = keep - h
            lo = f()
            flat[i] = keep
            assert abs((hi - lo) / (2 * h) - g.reshape(-1)[i]) <= 1e-7 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("B,m,D", SHAPES)
def test_without_correction_and_with_non_negative_scores_it_is_the_multi_negative_softmax(B, m, D):
    rng = np.random.default_rng(B * 100 + m + D)
    u, p, n = (np.abs(rng.standard_normal(s)).astype(np.float32) for s in ((B, D), (B, D), (B * m, D)))
    zero = np.zeros((B, m))
    wd, bs = 0.025, B + 1
    assert orc.loss(u, p, n, zero, m, 1.0, wd, bs) == pytest.approx(bpr_orc.loss(u, p, n, m, wd, bs, "softmax"), rel=1e-13)
    for a, b in zip(orc.grads(u, p, n, zero, m, 1.0, wd, bs, 2.0), bpr_orc.grads(u, p, n, m, wd, bs, "softmax", 2.0)):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("tau", [1.0, 0.25])
@pytest.mark.parametrize("B,m,D", SHAPES)
def test_a_constant_per_row_in_both_corrections_cancels(B, m, D, tau):
    u, p, n, logq, pos_logq = _case(B, m, D, seed=B + m + D)
    k = np.random.default_rng(5).uniform(-7.0, 7.0, B)
    wd, bs = 0.025, B + 1
    assert (orc.loss(u, p, n, logq + k[:, None], m, 1 / tau, wd, bs, pos_logq + k)
            == pytest.approx(orc.loss(u, p, n, logq, m, 1 / tau, wd, bs, pos_logq), rel=1e-13))
    assert (orc.loss(u, p, n, logq.reshape(-1), m, 1 / tau, wd, bs, np.zeros(B))          # [B*m] is [B, m]; no pos_logq is zeros
            == orc.loss(u, p, n, logq, m, 1 / tau, wd, bs, None))
    for a, b in zip(orc.grads(u, p, n, logq + k[:, None], m, 1 / tau, wd, bs, 1.0, pos_logq + k),
                    orc.grads(u, p, n, logq, m, 1 / tau, wd, bs, 1.0, pos_logq)):
        np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-16)


@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_one_negative_without_correction_is_minus_logsigmoid_of_the_difference(tau):
    u, p, n = bpr_orc.cases(5, 1, 9, seed=11)
    u64, p64, n64 = (t.astype(np.float64) for t in (u, p, n))
    z0, z1 = (u64 * p64).sum(1) / tau, (u64 * n64).sum(1) / tau                # plain scores: no abs
    want = -_logsigmoid(z0 - z1).sum() / 5
    assert orc.loss(u, p, n, np.zeros((5, 1)), 1, 1 / tau, 0.0, 5) == pytest.approx(want, rel=1e-13)
    a = orc.coefficients(u, p, n, np.zeros((5, 1)), 1, 1 / tau)[:, 0]
    np.testing.assert_allclose(a, np.exp(_logsigmoid(z1 - z0)), rtol=1e-12)


def test_scores_and_corrections_of_several_hundred_stay_finite():
    u = np.array([[10.0], [10.0]])
    p = np.array([[30.0], [-30.0]])
    n = np.array([[29.0], [-31.0], [31.0], [0.0]])
    logq = np.array([[-300.0, 0.0], [300.0, -2.0]])
    got = orc.loss(u, p, n, logq, 2, 1.0, 0.0, 1.0)
    # row 0: z = (300, 590, -310) -> 290 + log1p(..) ~ 290;  row 1: z = (-300, 10, 2) -> 310 + log(1 + e^-8 + e^-310)
    assert got == pytest.approx(290.0 + 310.0 + np.log1p(np.exp(-8.0)), rel=1e-12)
    assert all(np.isfinite(g).all() for g in orc.grads(u, p, n, logq, 2, 1.0, 0.0, 1.0))
