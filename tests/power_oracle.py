"""The Yeo-Johnson power scaler in plain numpy, written from the statement in include/ngcf_hip.h (no code shared with the product):
psi with every operation a separately rounded fp64 one, the likelihood that fits lambda (in fp64, or in np.longdouble for a second
opinion), a Brent minimiser, and the reference's unfloored ratings.  tests/test_power_surface.py pins psi and lambda to sklearn's
PowerTransformer where that library exists; `python tests/power_oracle.py --write` regenerates tests/golden/power.npz (needs sklearn), `--measure`
prints the oracle's own largest psi error against mpmath, the figure the device tests' tolerance starts from."""
import os
import sys

import numpy as np

EPS = 2.0 ** -52
TINY = 2.2250738585072014e-308
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "power.npz")
# the segment lengths of the end-to-end tests (those of the quantile tests); two columns have exactly their sum of rows
LENGTHS = tuple(range(1, 10)) + (63, 64, 65, 66, 255, 256, 257, 258, 1025)
NAMES = ("counts", "signed", "ints", "leftskew")


def psi(x, lam, dtype=np.float64):
    """psi(x, lam) elementwise; a NaN stays a NaN.  `dtype` np.longdouble evaluates the same statement in extended precision."""
    x = np.asarray(x, dtype=dtype)
    lam = dtype(lam)
    one, two = dtype(1), dtype(2)
    out = np.array(x, dtype=dtype, copy=True)
    pos, neg = x >= 0, x < 0
    with np.errstate(all="ignore"):
        if abs(lam) < EPS:
            out[pos] = np.log1p(x[pos])
        else:
            out[pos] = np.divide(np.subtract(np.power(np.add(x[pos], one), lam), one), lam)
        if abs(lam - two) <= EPS:
            out[neg] = np.negative(np.log1p(np.negative(x[neg])))
        else:
            e = np.subtract(two, lam)
            out[neg] = np.divide(np.negative(np.subtract(np.power(np.add(np.negative(x[neg]), one), e), one)), e)
    return out


def pow_parts(x, lam):
    """Per element, what the error bound of psi is stated in: (p, d, is_pow) with p the pow result and d the denominator of the
    branch the element takes (lam, or 2 - lam for negative x); is_pow False on the log1p branches."""
    x = np.asarray(x, dtype=np.float64)
    lam = np.float64(lam)
    pos = x >= 0
    d = np.where(pos, lam, np.subtract(np.float64(2), lam))
    base = np.where(pos, np.add(x, 1.0), np.add(np.negative(x), 1.0))
    is_pow = np.where(pos, not abs(lam) < EPS, not abs(lam - 2.0) <= EPS)
    with np.errstate(all="ignore"):
        p = np.power(base, d)
    return p, d, is_pow


def log_term(x, dtype=np.float64):
    """c = sum sign(x) log1p|x| over the rows that are not NaN."""
    x = np.asarray(x, dtype=dtype)
    x = x[~np.isnan(x)]
    return np.sum(np.sign(x) * np.log1p(np.abs(x)))


def neg_log_likelihood(x, lam, dtype=np.float64):
    """f(lam) = n/2 log(M2 / n) - (lam - 1) c over the rows that are not NaN; +inf where M2 / n is below the smallest normal double."""
    x = np.asarray(x, dtype=dtype)
    x = x[~np.isnan(x)]
    y = psi(x, lam, dtype)
    n = len(x)
    var = np.sum(np.square(y - np.sum(y) / n)) / n
    if var < TINY:
        return np.inf
    return float(n / dtype(2) * np.log(var) - (dtype(lam) - 1) * log_term(x, dtype))


def tol1(lam, tol=1.48e-8):
    return tol * abs(lam) + 1e-11


class _Point:
    __slots__ = ("x", "f")

    def __init__(self, x, f):
        self.x, self.f = x, f


def brent_min(f, lo=-2.0, hi=2.0, tol=1.48e-8, maxiter=500):
    """Brent's minimiser from the bracket (lo, hi): golden-section expansion to three points around a minimum, then parabolic steps
    with golden-section fall-backs; stops at tol1 = tol |x| + 1e-11.  Returns (x, evaluations)."""
    gold, cgold, calls = 1.618034, 0.3819660, [0]

    def ev(x):
        calls[0] += 1
        return _Point(x, f(x))

    # --- bracket
    A, B = ev(lo), ev(hi)
    if A.f < B.f:
        A, B = B, A
    Cp = ev(B.x + gold * (B.x - A.x))
    rounds = 0
    while Cp.f < B.f:
        r = (B.x - A.x) * (B.f - Cp.f)
        q = (B.x - Cp.x) * (B.f - A.f)
        diff = q - r
        den = 2.0 * (1e-21 if abs(diff) < 1e-21 else diff)
        w = B.x - ((B.x - Cp.x) * q - (B.x - A.x) * r) / den
        limit = B.x + 110.0 * (Cp.x - B.x)
        rounds += 1
        if rounds > 1000:
            raise RuntimeError("no bracket")
        if (w - Cp.x) * (B.x - w) > 0.0:
            W = ev(w)
            if W.f < Cp.f:
                A, B = B, W
                break
            if W.f > B.f:
                Cp = W
                break
            W = ev(Cp.x + gold * (Cp.x - B.x))
        elif (w - limit) * (limit - Cp.x) >= 0.0:
            W = ev(limit)
        elif (w - limit) * (Cp.x - w) > 0.0:
            W = ev(w)
            if W.f < Cp.f:
                B, Cp = Cp, W
                W = ev(Cp.x + gold * (Cp.x - B.x))
        else:
            W = ev(Cp.x + gold * (Cp.x - B.x))
        A, B, Cp = B, Cp, W

    # --- minimise inside [a, b]
    a, b = min(A.x, Cp.x), max(A.x, Cp.x)
    X = Wp = V = B
    step = prev = 0.0
    for _ in range(maxiter):
        t1 = tol1(X.x, tol)
        mid = 0.5 * (a + b)
        if abs(X.x - mid) < 2.0 * t1 - 0.5 * (b - a):
            break
        use_golden = True
        if abs(prev) > t1:
            r = (X.x - Wp.x) * (X.f - V.f)
            q = (X.x - V.x) * (X.f - Wp.f)
            p = (X.x - V.x) * q - (X.x - Wp.x) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            older, prev = prev, step
            if p > q * (a - X.x) and p < q * (b - X.x) and abs(p) < abs(0.5 * q * older):
                step = p / q
                u = X.x + step
                if u - a < 2.0 * t1 or b - u < 2.0 * t1:
                    step = t1 if mid - X.x >= 0 else -t1
                use_golden = False
        if use_golden:
            prev = a - X.x if X.x >= mid else b - X.x
            step = cgold * prev
        if abs(step) < t1:
            U = ev(X.x + t1 if step >= 0 else X.x - t1)
        else:
            U = ev(X.x + step)
        if U.f > X.f:
            if U.x < X.x:
                a = U.x
            else:
                b = U.x
            if U.f <= Wp.f or Wp.x == X.x:
                V, Wp = Wp, U
            elif U.f <= V.f or V.x == X.x or V.x == Wp.x:
                V = U
        else:
            if U.x >= X.x:
                a = X.x
            else:
                b = X.x
            V, Wp, X = Wp, X, U
    return X.x, calls[0]


def fit_lambda(x, dtype=np.float64):
    """The fitted lambda of the column x, the likelihood evaluated in `dtype`."""
    return brent_min(lambda lam: neg_log_likelihood(x, lam, dtype))[0]


def standardise(y):
    """StandardScaler's (mean, scale) of the transformed column, and the reference's shift |min z|."""
    y = np.asarray(y, dtype=np.float64)
    mean = np.mean(y)
    scale = np.sqrt(np.mean(np.square(np.subtract(y, mean))))
    shift = np.abs(np.min(np.divide(np.subtract(y, mean), scale)))
    return float(mean), float(scale), float(shift)


def ratings_unfloored(x, lam):
    """z = ((psi(x, lam) - mean) / scale) + shift with the stats of that psi: the reference's ratings before the per-user floor."""
    y = psi(x, lam)
    mean, scale, shift = standardise(y)
    return np.add(np.divide(np.subtract(y, mean), scale), shift)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def columns():
    """The four columns, from fixed seeds."""
    T = sum(LENGTHS)
    rng = np.random.default_rng(20250914)
    counts = np.floor(np.exp(rng.normal(3.0, 1.5, T)))                    # heavy-tailed visitor counts
    signed = rng.standard_t(3, 2000) * 5.0
    ints = rng.integers(0, 50, T).astype(np.float64)                      # many ties at every quartile
    leftskew = -np.exp(rng.normal(0.0, 0.6, 1500)) - 0.25                 # all negative, long tail to the left
    return dict(zip(NAMES, (counts, signed, ints, leftskew)))


def users():
    """A user per row for the columns of sum(LENGTHS) rows: segment lengths LENGTHS, rows shuffled."""
    return np.random.default_rng(20250915).permutation(np.repeat(np.arange(len(LENGTHS)), LENGTHS))


def sklearn_fit(col):
    """(lambdas_[0], standardised output) of sklearn's PowerTransformer() on one column."""
    from sklearn.preprocessing import PowerTransformer
    pt = PowerTransformer()
    z = pt.fit_transform(np.asarray(col, dtype=np.float64).reshape(-1, 1))[:, 0]
    return float(pt.lambdas_[0]), z


def build_fixture():
    out = {}
    for name, col in columns().items():
        lam, z = sklearn_fit(col)
        out["x_" + name], out["lam_" + name], out["z_" + name] = col, np.float64(lam), z
    return out


def load_fixture():
    return dict(np.load(FIXTURE, allow_pickle=False))


# ---- the inputs of the psi tests, and the oracle's own error on them -----------------------------------------------------------------
SPECIALS = (0.0, -0.0, 1e-300, -1e-300, 1e300, -1e300, np.nan, np.inf, -np.inf)
PSI_SIZES = (1, 63, 64, 65, 257)
PSI_LAMBDAS = (0.0, 2.0 ** -53, 2.0 ** -51, 2.0, 2.0 + 2.0 ** -51, 1.0, -2.0, 0.5, 3.5)


def psi_cases():
    """{name: x}: a column per size of PSI_SIZES (values of both signs over six decades, the specials first as far as they fit) and
    the fixture's columns with the specials appended."""
    rng = np.random.default_rng(20250916)
    cases = {}
    for T in PSI_SIZES:
        x = rng.standard_normal(T) * 10.0 ** rng.uniform(-3, 3, T)
        k = min(T - 1, len(SPECIALS))
        x[T - k:] = SPECIALS[:k]
        cases[f"T{T}"] = x
    fx = load_fixture()
    for name in NAMES:
        cases[name] = np.concatenate([fx["x_" + name], SPECIALS])
    return cases


def psi_lambdas():
    fx = load_fixture()
    return PSI_LAMBDAS + tuple(float(fx["lam_" + name]) for name in NAMES)


def psi_unit(x, lam):
    """The unit the error of psi is counted in, per element: 2^-52 (|p| + |p - 1|) / |d| on the pow branch, the spacing of psi on
    the log1p branches.  Elements whose psi is not finite have unit NaN: they are compared exactly."""
    p, d, is_pow = pow_parts(x, lam)
    y = psi(x, lam)
    with np.errstate(all="ignore"):
        unit = np.where(is_pow, EPS * (np.abs(p) + np.abs(p - 1.0)) / np.abs(d), np.spacing(np.abs(y)))
    return np.where(np.isfinite(y) & np.isfinite(p), unit, np.nan)


def reference_error_units():
    """The largest error of psi() above, in psi_unit's units, over psi_cases() x psi_lambdas(), against mpmath at 50 digits given the
    same rounded base x + 1 (or -x + 1): what is measured is pow / log1p and the two operations after it."""
    import mpmath
    mpmath.mp.dps = 50
    worst = 0.0
    for lam in psi_lambdas():
        for name, x in psi_cases().items():
            y, unit = psi(x, lam), psi_unit(x, lam)
            p, d, is_pow = pow_parts(x, lam)
            for i in np.flatnonzero(np.isfinite(unit) & (unit > 0)):
                if is_pow[i]:
                    base = np.add(x[i], 1.0) if x[i] >= 0 else np.add(np.negative(x[i]), 1.0)
                    exact = (mpmath.power(mpmath.mpf(float(base)), mpmath.mpf(float(d[i]))) - 1) / mpmath.mpf(float(d[i]))
                else:
                    exact = mpmath.log1p(mpmath.mpf(float(abs(x[i]))))
                if x[i] < 0:
                    exact = -exact
                worst = max(worst, float(abs(mpmath.mpf(float(y[i])) - exact) / mpmath.mpf(float(unit[i]))))
    return worst


if __name__ == "__main__":
    if sys.argv[1:] == ["--measure"]:
        print(f"numpy's largest psi error against mpmath: {reference_error_units():.3f} units")
        sys.exit(0)
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/power_oracle.py --write | --measure")
    np.savez(FIXTURE, **build_fixture())
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
