"""Host oracle of the full-catalogue softmax loss (csrc/softmax_full.hip), plain numpy in float64: the loss, `lse`, dU and dI from
float64 dot products of the float32 inputs, with the regulariser, duplicate positives and ids outside the catalogue (no positive
term, as the kernels treat them)."""
import numpy as np


def softmax_full(u, items, pos, inv_tau, weight_decay, batch_size, grad_out=1.0):
    """-> dict(loss, lse [B], spos [B], du [B, D], ditems [n_items, D]), all float64."""
    u = np.asarray(u, dtype=np.float64)
    it = np.asarray(items, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.int64)
    B, n = u.shape[0], it.shape[0]
    s = (u @ it.T) * float(inv_tau)
    m = s.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(s - m).sum(axis=1, keepdims=True)))[:, 0]
    ok = (pos >= 0) & (pos < n)
    rows = np.nonzero(ok)[0]
    spos = np.zeros(B)
    spos[rows] = s[rows, pos[rows]]
    reg = (u * u).sum() + (it[pos[rows]] ** 2).sum()
    loss = ((lse - spos).sum() + float(weight_decay) * reg) / float(batch_size)
    g0 = float(grad_out) / float(batch_size)
    g = np.exp(s - lse[:, None])
    g[rows, pos[rows]] -= 1.0
    g *= g0 * float(inv_tau)
    cnt = np.bincount(pos[rows], minlength=n).astype(np.float64)
    du = g @ it + 2.0 * float(weight_decay) * g0 * u
    di = g.T @ u + 2.0 * float(weight_decay) * g0 * cnt[:, None] * it
    return dict(loss=loss, lse=lse, spos=spos, du=du, ditems=di)
