"""The per-segment quantile floor in plain numpy, written from the statement in include/ngcf_hip.h (no code shared with the product):
per segment an `np.sort`, the two order statistics, numpy's two-sided linear blend - every operation a separately rounded fp64 one.
tests/test_preprocess_surface.py pins it to pandas' `quantile` and `np.percentile` where those libraries exist."""
import numpy as np


def quantile_sorted(s, q4):
    """The q4/4 quantile of the ascending fp64 array `s` (n >= 1)."""
    n = len(s)
    r = (n - 1) * q4
    lo, t = r // 4, np.float64((r % 4) * 0.25)
    a, b = np.float64(s[lo]), np.float64(s[min(lo + 1, n - 1)])
    d = np.subtract(b, a)
    if t < 0.5:
        return np.add(a, np.multiply(d, t))
    return np.subtract(b, np.multiply(d, np.subtract(np.float64(1.0), t)))


def transform(x, mean=0.0, scale=1.0, shift=0.0):
    """z = ((x - mean) / scale) + shift, three rounded operations."""
    x = np.asarray(x, dtype=np.float64)
    return np.add(np.divide(np.subtract(x, np.float64(mean)), np.float64(scale)), np.float64(shift))


def floor_segments(segments, x, q4=1, mean=0.0, scale=1.0, shift=0.0):
    """`segments`: one integer position array per segment (into x).  Returns (out, quant): z floored below each segment's quantile,
    a position in no segment keeps its z; the quantile of an empty segment is NaN.  A segment that holds a
    NaN has a NaN quantile and passes through."""
    z = transform(x, mean, scale, shift)
    out = z.copy()
    quant = np.full(len(segments), np.nan)
    with np.errstate(invalid="ignore"):
        for u, pos in enumerate(segments):
            pos = np.asarray(pos, dtype=np.int64)
            if len(pos) == 0:
                continue
            v = z[pos]
            if np.isnan(v).any():
                continue
            quant[u] = quantile_sorted(np.sort(v), q4)
            out[pos[v < quant[u]]] = 0.0
    return out, quant


def segments_of(ids, n_rows):
    """Positions grouped by id, ascending within each group."""
    ids = np.asarray(ids, dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    bounds = np.searchsorted(ids[order], np.arange(n_rows + 1))
    return [order[bounds[u]:bounds[u + 1]] for u in range(n_rows)]
