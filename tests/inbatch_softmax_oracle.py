"""Host oracle of the softmax loss with shared (in-batch) negatives (csrc/inbatch_softmax.hip; include/ngcf_hip.h, "In-batch
softmax"), plain numpy in float64: the loss, `lse`, dU, dp and dx from float64 dot products of the float32 inputs, with the
corrections, the mask of false negatives and the extra shared rows.  Test infrastructure: it imports nothing of the package."""
import numpy as np


def _vec(t, n):
    return np.zeros(n) if t is None else np.asarray(t, dtype=np.float64).reshape(n)


def mask(B, ids=None, xids=None, E=None):
    """[B, B + E] bool: column j is a false negative of row b - ids given, j != b and the column's id equals ids[b]."""
    E = (0 if xids is None else len(xids)) if E is None else E
    if ids is None:
        return np.zeros((B, B + E), dtype=bool)
    ids = np.asarray(ids, dtype=np.int64).reshape(B)
    cid = ids if E == 0 else np.concatenate((ids, np.asarray(xids, dtype=np.int64).reshape(E)))
    hit = cid[None, :] == ids[:, None]
    hit[np.arange(B), np.arange(B)] = False
    return hit


def inbatch_softmax(u, p, inv_tau, weight_decay, batch_size, grad_out=1.0, x=None, ids=None, xids=None, logq=None, xlogq=None,
                    pos_logq=None):
    """u [B, D], p [B, D], x [E, D] or None; ids [B] / xids [E] or None; logq [B], xlogq [E], pos_logq [B] or None (exactly 0).
    -> dict(loss, lse [B], z [B, B + E] (masked entries -inf), du [B, D], dp [B, D], dx [E, D]), all float64."""
    u, p = np.asarray(u, dtype=np.float64), np.asarray(p, dtype=np.float64)
    B, D = u.shape
    x = np.zeros((0, D)) if x is None else np.asarray(x, dtype=np.float64).reshape(-1, D)
    E = x.shape[0]
    if ids is not None and E > 0 and xids is None:
        raise ValueError("ids with extras and no xids")
    c = np.concatenate((p, x), axis=0)
    q = np.concatenate((_vec(logq, B), _vec(xlogq, E)))
    z = (u @ c.T) * float(inv_tau) - q[None, :]
    d = np.arange(B)
    z[d, d] = np.einsum("bd,bd->b", u, p) * float(inv_tau) - _vec(pos_logq, B)
    z[mask(B, ids, xids if E else None, E)] = -np.inf
    m = z.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]
    loss = ((lse - z[d, d]).sum() + float(weight_decay) * ((u * u).sum() + (p * p).sum())) / float(batch_size)
    g0 = float(grad_out) / float(batch_size)
    g = np.exp(z - lse[:, None])                                            # exp(-inf) = 0: a masked pair has no gradient
    g[d, d] -= 1.0
    g *= g0 * float(inv_tau)
    du = g @ c + 2.0 * float(weight_decay) * g0 * u
    dc = g.T @ u
    dc[:B] += 2.0 * float(weight_decay) * g0 * p
    return dict(loss=loss, lse=lse, z=z, du=du, dp=dc[:B], dx=dc[B:])
