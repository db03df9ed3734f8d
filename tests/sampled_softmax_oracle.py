"""The definition of the sampled softmax loss with logQ correction (include/ngcf_hip.h, "Sampled softmax with logQ correction") and its
analytic gradients in numpy float64 - the oracle of tests/test_sampled_softmax_gpu.py, itself checked in
tests/test_sampled_softmax_oracle.py.  Test infrastructure: it imports nothing of the package."""
import numpy as np


def _z(u, p, n, logq, m, inv_tau, pos_logq):
    """-> n3 [B, m, D], z [B, 1 + m]: column 0 the positive's corrected score, then the negatives'."""
    B, D = u.shape
    n3 = n.reshape(B, m, D)
    c = np.zeros(B) if pos_logq is None else np.asarray(pos_logq, dtype=np.float64).reshape(B)
    z0 = np.einsum("bd,bd->b", u, p) * inv_tau - c
    zj = np.einsum("bd,bjd->bj", u, n3) * inv_tau - np.asarray(logq, dtype=np.float64).reshape(B, m)
    return n3, np.concatenate((z0[:, None], zj), axis=1)


def loss(u, p, n, logq, m, inv_tau, wd, batch_size, pos_logq=None):
    """u [B, D], p [B, D], n [B*m, D] (rows b*m .. b*m + m - 1: the negatives of row b), logq [B, m] or [B*m], pos_logq [B] or None
    -> the loss, a float."""
    u, p, n = (np.asarray(t, dtype=np.float64) for t in (u, p, n))
    _, z = _z(u, p, n, logq, m, float(inv_tau), pos_logq)
    M = z.max(1)
    rows = M + np.log(np.exp(z - M[:, None]).sum(1)) - z[:, 0]
    reg = (u * u).sum() + (p * p).sum() + (n * n).sum() / m
    return float((rows.sum() + wd * reg) / batch_size)


def coefficients(u, p, n, logq, m, inv_tau, pos_logq=None):
    """a [B, m]: the softmax weight of every negative among the row's 1 + m corrected scores."""
    u, p, n = (np.asarray(t, dtype=np.float64) for t in (u, p, n))
    _, z = _z(u, p, n, logq, m, float(inv_tau), pos_logq)
    e = np.exp(z - z.max(1)[:, None])
    return e[:, 1:] / e.sum(1)[:, None]


def grads(u, p, n, logq, m, inv_tau, wd, batch_size, grad_out=1.0, pos_logq=None):
    """(du, dp, dn) of `loss`, times grad_out; logq and pos_logq are data."""
    u, p, n = (np.asarray(t, dtype=np.float64) for t in (u, p, n))
    B, D = u.shape
    n3 = n.reshape(B, m, D)
    a = coefficients(u, p, n, logq, m, inv_tau, pos_logq) * float(inv_tau)    # dl_b/d(u.n_j)
    A = a.sum(1)                                                               # -dl_b/d(u.p)
    g = grad_out / batch_size
    du = -A[:, None] * p + np.einsum("bj,bjd->bd", a, n3) + 2 * wd * u
    dp = -A[:, None] * u + 2 * wd * p
    dn = a[:, :, None] * u[:, None, :] + (2 * wd / m) * n3
    return g * du, g * dp, (g * dn).reshape(n.shape)
