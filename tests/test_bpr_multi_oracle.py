"""CPU: the float64 oracle of the multi-negative BPR loss (tests/bpr_multi_oracle.py) against torch.autograd on a float64 composition
of the definition, and against identity (b) - the existing single-negative definition over the expanded batch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bpr_multi_oracle as orc

SHAPES = [(1, 1, 1), (3, 2, 5), (4, 3, 65), (5, 24, 7), (2, 64, 3)]


def _torch_loss(u, p, n, m, wd, bs, reduction):
    B, D = u.shape
    sp = (u * p).sum(1).abs()
    sn = torch.einsum("bd,bjd->bj", u, n.reshape(B, m, D)).abs()
    if reduction == "mean":
        rows = -F.logsigmoid(sp[:, None] - sn).mean(1)
    else:
        rows = -F.logsigmoid(sp - torch.logsumexp(sn, 1))
    return (rows.sum() + wd * (u.pow(2).sum() + p.pow(2).sum() + n.pow(2).sum() / m)) / bs


def _check_against_autograd(u, p, n, m, wd, bs, reduction, grad_out=1.0):
    t = [torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True) for x in (u, p, n)]
    want = _torch_loss(*t, m, wd, bs, reduction)
    (grad_out * want).backward()
    assert np.isfinite(float(want.detach()))
    assert orc.loss(u, p, n, m, wd, bs, reduction) == pytest.approx(float(want.detach()), rel=1e-13, abs=1e-300)
    for got, leaf in zip(orc.grads(u, p, n, m, wd, bs, reduction, grad_out), t):
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, leaf.grad.numpy(), rtol=1e-11, atol=1e-15 * max(1.0, float(leaf.grad.abs().max())))


@pytest.mark.parametrize("reduction", ["mean", "softmax"])
@pytest.mark.parametrize("B,m,D", SHAPES)
def test_oracle_is_autograd_of_the_definition(B, m, D, reduction):
    u, p, n = orc.cases(B, m, D, seed=B * 1000 + m * 10 + D)
    assert float(u[0] @ p[0]) == 0.0 and float(u[0] @ n[0]) == 0.0          # the sign-0 rows are what they claim to be
    if B > 1:
        assert float(u[1] @ p[1]) < 0.0
    _check_against_autograd(u, p, n, m, 0.025, B + 3, reduction, grad_out=3.0)


@pytest.mark.parametrize("reduction", ["mean", "softmax"])
def test_zero_dot_products_pass_no_gradient_through_their_score(reduction):
    u, p, n = orc.cases(3, 4, 6, seed=7)
    du, dp, dn = orc.grads(u, p, n, 4, 0.0, 1.0, reduction)
    assert not dp[0].any() and not dn[0].any()                              # sgn(0) = 0 and no weight decay: nothing arrives
    assert dn[1].any() and dp[1].any()
    # du_0 is the sum over the negatives whose dot product is not zero
    want = orc.grads(u[:1], p[:1], n[1:4], 3, 0.0, 1.0, reduction)[0] if reduction == "mean" else None
    if want is not None:
        np.testing.assert_allclose(du[0], want[0] * 3 / 4, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_softmax_stays_finite_for_scores_of_several_hundred(sign):
    rng = np.random.default_rng(3)
    B, m, D = 4, 8, 16
    u = rng.standard_normal((B, D))
    u *= np.sqrt(300.0) / np.linalg.norm(u, axis=1, keepdims=True)
    p = sign * u * np.array([1.0, 0.98, 1.02, 0.5])[:, None]              # u.p = +-300, +-294, +-306, +-150
    n = np.repeat(u, m, axis=0) * rng.uniform(-1.05, 1.05, (B * m, 1))     # |u.n| up to 315, both signs
    got = orc.loss(u, p, n, m, 0.0, 1.0, "softmax")
    assert np.isfinite(got) and got > 0
    _check_against_autograd(u, p, n, m, 0.01, B, "softmax")
    # a positive far below the hardest negative: the row's loss is their distance, the softmax weight of the hardest is 1
    u1, p1 = np.array([[10.0]]), np.array([[1.0]])
    n1 = np.array([[40.0], [-5.0], [1.0]])
    assert orc.loss(u1, p1, n1, 3, 0.0, 1.0, "softmax") == pytest.approx(390.0, rel=1e-12)
    a = orc.grads(u1, p1, n1, 3, 0.0, 1.0, "softmax")[2][:, 0] / 10.0
    np.testing.assert_allclose(a, [1.0, 0.0, 0.0], atol=1e-100)


@pytest.mark.parametrize("B,m,D", SHAPES)
def test_mean_is_the_existing_loss_over_the_expanded_batch(B, m, D):
    """Identity (b): `mean` at any m = the single-negative definition over the B*m expanded triplets with batch_size * m; the
    gradients of a repeated row add up."""
    u, p, n = orc.cases(B, m, D, seed=B + m + D)
    wd, bs = 0.025, B + 1
    ue, pe = orc.expand(u, p, m)
    assert orc.loss(u, p, n, m, wd, bs, "mean") == pytest.approx(orc.bpr_loss(ue, pe, n, wd, bs * m), rel=1e-13)
    du, dp, dn = orc.grads(u, p, n, m, wd, bs, "mean", grad_out=2.0)
    due, dpe, dne = orc.bpr_grads(ue, pe, n, wd, bs * m, grad_out=2.0)
    np.testing.assert_allclose(du, due.reshape(B, m, D).sum(1), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(dp, dpe.reshape(B, m, D).sum(1), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(dn, dne, rtol=1e-12, atol=1e-18)


def test_mean_and_softmax_agree_at_one_negative():
    u, p, n = orc.cases(5, 1, 9, seed=11)
    assert orc.loss(u, p, n, 1, 0.1, 5, "softmax") == pytest.approx(orc.loss(u, p, n, 1, 0.1, 5, "mean"), rel=1e-13)
    for a, b in zip(orc.grads(u, p, n, 1, 0.1, 5, "softmax"), orc.grads(u, p, n, 1, 0.1, 5, "mean")):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-18)
