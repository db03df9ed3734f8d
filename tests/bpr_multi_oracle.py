"""The definition of the BPR loss against m negatives per positive row (include/ngcf_hip.h, "BPR, m negatives per positive") and its
analytic gradients in numpy float64 - the oracle of tests/test_bpr_multi_gpu.py, itself checked in tests/test_bpr_multi_oracle.py.
Test infrastructure: it imports nothing of the package."""
import numpy as np


def _logsigmoid(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def _scores(u, p, n, m):
    B, D = u.shape
    n3 = n.reshape(B, m, D)
    up = np.einsum("bd,bd->b", u, p)
    un = np.einsum("bd,bjd->bj", u, n3)
    return n3, up, un


def loss(u, p, n, m, wd, batch_size, reduction="mean"):
    """u [B, D], p [B, D], n [B*m, D] (rows b*m .. b*m + m - 1: the negatives of row b) -> the loss, a float."""
    u, p, n = (np.asarray(t, dtype=np.float64) for t in (u, p, n))
    _, up, un = _scores(u, p, n, m)
    sp, sn = np.abs(up), np.abs(un)
    if reduction == "mean":
        rows = -_logsigmoid(sp[:, None] - sn).sum(1) / m
    elif reduction == "softmax":
        M = sn.max(1)
        lse = M + np.log(np.exp(sn - M[:, None]).sum(1))
        rows = -_logsigmoid(sp - lse)
    else:
        raise ValueError(reduction)
    reg = (u * u).sum() + (p * p).sum() + (n * n).sum() / m
    return float((rows.sum() + wd * reg) / batch_size)


def grads(u, p, n, m, wd, batch_size, reduction="mean", grad_out=1.0):
    """(du, dp, dn) of `loss`, times grad_out; sgn(0) = 0 like torch.abs."""
    u, p, n = (np.asarray(t, dtype=np.float64) for t in (u, p, n))
    n3, up, un = _scores(u, p, n, m)
    sp, sn = np.abs(up), np.abs(un)
    if reduction == "mean":
        x = sp[:, None] - sn
        a = np.exp(_logsigmoid(-x)) / m                            # (1/m) / (1 + exp(sp - sn_j)), without overflow
    elif reduction == "softmax":
        M = np.maximum(sp, sn.max(1))
        e = np.exp(sn - M[:, None])
        a = e / (np.exp(sp - M) + e.sum(1))[:, None]
    else:
        raise ValueError(reduction)
    A = a.sum(1)
    sgp, sgn = np.sign(up), np.sign(un)
    g = grad_out / batch_size
    du = -(A * sgp)[:, None] * p + np.einsum("bj,bjd->bd", a * sgn, n3) + 2 * wd * u
    dp = -(A * sgp)[:, None] * u + 2 * wd * p
    dn = (a * sgn)[:, :, None] * u[:, None, :] + (2 * wd / m) * n3
    return g * du, g * dp, (g * dn).reshape(n.shape)


def expand(u, p, m):
    """The expanded batch of identity (b): every u and p row repeated m times, next to each other."""
    return np.repeat(u, m, axis=0), np.repeat(p, m, axis=0)


def bpr_loss(u, p, n, wd, batch_size):
    """The existing single-negative definition (bprloss.py:15-22) on equal row counts, float64."""
    u, p, n = (np.asarray(t, dtype=np.float64) for t in (u, p, n))
    x = np.abs((u * p).sum(1)) - np.abs((u * n).sum(1))
    return float((-_logsigmoid(x).sum() + wd * ((u * u).sum() + (p * p).sum() + (n * n).sum())) / batch_size)


def bpr_grads(u, p, n, wd, batch_size, grad_out=1.0):
    u, p, n = (np.asarray(t, dtype=np.float64) for t in (u, p, n))
    up, un = (u * p).sum(1), (u * n).sum(1)
    s = -np.exp(_logsigmoid(-(np.abs(up) - np.abs(un))))         # d(-logsigmoid(x))/dx
    sgp, sgn = np.sign(up), np.sign(un)
    g = grad_out / batch_size
    du = (s * sgp)[:, None] * p - (s * sgn)[:, None] * n + 2 * wd * u
    dp = (s * sgp)[:, None] * u + 2 * wd * p
    dn = -(s * sgn)[:, None] * u + 2 * wd * n
    return g * du, g * dp, g * dn


def cases(B, m, D, seed, scale=1.0):
    """Inputs with the rows the definition is sensitive to (float32, what the kernels read): row 0's positive dot product is exactly
    zero and so is its first negative's (sign 0), row 1's positive dot product is negative, row 2's negatives are all equal (as far
    as B goes).  Small integers in a few columns make the zero dot products exact in any summation order."""
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal((B, D)) * scale).astype(np.float32)
    p = (rng.standard_normal((B, D)) * scale).astype(np.float32)
    n = (rng.standard_normal((B, m, D)) * scale).astype(np.float32)
    u[0] = 0
    u[0, 0] = 2.0
    p[0, 0] = 0.0                                                 # u_0.p_0 = 0
    n[0, 0, 0] = 0.0                                              # u_0.n_00 = 0
    if B > 1:
        p[1] = -np.abs(p[1]) * np.sign(u[1] + (u[1] == 0))        # every product negative: u_1.p_1 < 0
    if B > 2:
        n[2, :] = n[2, 0]
    # |t| has a kink at 0: a random dot product within float32 rounding of zero takes either sign depending on the summation order,
    # and the gradient through it flips with it.  Only the two planted zeros may sit there; every other dot product is moved to at
    # least `margin` from zero by adding a multiple of the row's u (equal rows stay equal).
    margin = 1e-3
    rows = np.concatenate((p[:, None, :], n), axis=1)                        # [B, 1 + m, D]: the positive, then the negatives
    u64 = u.astype(np.float64)
    s = np.einsum("bd,bjd->bj", u64, rows.astype(np.float64))
    near = np.abs(s) < margin
    near[0, :2] = False                                                       # the planted zeros
    for b, j in zip(*np.nonzero(near)):
        rows[b, j] += ((4 * margin if s[b, j] >= 0 else -4 * margin) / (u64[b] @ u64[b]) * u64[b]).astype(np.float32)
        assert abs(u64[b] @ rows[b, j]) >= margin
    return u, rows[:, 0].copy(), rows[:, 1:].reshape(B * m, D).copy()
