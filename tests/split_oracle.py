"""The per-group selection (ngcf_select_per_group) in plain numpy for the split tests: the keys from uint64 array
arithmetic, tau_g from a sort per group.  It shares no code with the library."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
C1, C2, S33 = np.uint64(0xff51afd7ed558ccd), np.uint64(0xc4ceb9fe1a85ec53), np.uint64(33)


def fmix(x):
    """The 64-bit finaliser on a uint64 array (the products wrap modulo 2^64, which is the arithmetic the header asks for)."""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> S33
        x *= C1
        x ^= x >> S33
        x *= C2
        x ^= x >> S33
    return x


def keys(seed, T):
    """k_t = fmix(seed ^ (t * GOLDEN)) for t in [0, T)."""
    with np.errstate(over="ignore"):
        return fmix(np.uint64(int(seed) & (2 ** 64 - 1)) ^ (np.arange(T, dtype=np.uint64) * GOLDEN))


def select(group, quota, seed, n_rows=None):
    """`(mask uint8 [T], thresholds uint64 [G])`: row t of group g is marked iff quota[g] > 0 and its key is at most the quota[g]-th
    smallest key of the group; the threshold of a group with quota 0 is 0.  `group` None: one group of n_rows rows.  The ids must
    lie in [0, G) and no quota may exceed its group's size (the library's error paths are not modelled)."""
    quota = np.asarray(quota, dtype=np.int64)
    G = len(quota)
    T = int(n_rows) if group is None else len(group)
    group = np.zeros(T, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    assert T == 0 or (group.min() >= 0 and group.max() < G)
    k = keys(seed, T)
    mask, tau = np.zeros(T, dtype=np.uint8), np.zeros(G, dtype=np.uint64)
    order = np.argsort(group, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=G))])
    for g in range(G):
        if quota[g] == 0:
            continue
        rows = order[bounds[g]:bounds[g + 1]]
        assert quota[g] <= len(rows)
        tau[g] = np.sort(k[rows])[quota[g] - 1]
        mask[rows[k[rows] <= tau[g]]] = 1
    return mask, tau
