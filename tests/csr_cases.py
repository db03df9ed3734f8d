"""Random CSR matrices shared by the GPU parity tests and the CPU test of the swept plan."""
import numpy as np


def random_csr(rng, n_rows, n_cols, mean_deg, heavy=(), empty=()):
    deg = rng.poisson(mean_deg, n_rows)
    for r, k in heavy:
        deg[r] = k
    for r in empty:
        deg[r] = 0
    rowptr = np.zeros(n_rows + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    nnz = int(rowptr[-1])
    cols = rng.integers(0, n_cols, nnz).astype(np.int64)
    vals = rng.normal(0, 0.3, nnz).astype(np.float32)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), deg)
    return rowptr, rows, cols, vals
