"""The Yeo-Johnson power scaler on the device (csrc/yeo_johnson.hip, engine.yeo_johnson / yeo_johnson_moments, preprocess.fit_power,
scale_implicit with a PowerScaler) against the plain-numpy statement (tests/power_oracle.py), which tests/test_power_surface.py
pins to sklearn's PowerTransformer.

psi is compared in the unit of power_oracle.psi_unit - 2^-52 (|p| + |p - 1|) / |d| where pow runs (p the pow result, d the branch's
denominator), one spacing of psi on the log1p branches - with K_PSI units allowed: the oracle's own largest error against mpmath at
50 digits on the same inputs (`python tests/power_oracle.py --measure`: 0.648 units), rounded up to an integer, plus 2.
Measured on an MI355X: DEVICE_FIGURES below."""
import functools
import math

import numpy as np
import pytest
import torch

import power_oracle
import quantile_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REF_PSI_ERROR = 0.648                      # numpy against mpmath, in psi_unit's units
K_PSI = math.ceil(REF_PSI_ERROR) + 2
EPS = 2.0 ** -52
DEVICE_FIGURES = """
psi, largest |dev - oracle| in units (allowed 3):  T1 0.558, T63 1.000, T64 1.000, T65 1.000, T257 1.000,
                                                   counts 0.775, signed 1.000, ints 0.614, leftskew 1.000
moments, largest error as a share of the bound:    sizes around the launch constants 0.116, fixture columns and NaNs 0.046
lambda, dev - sklearn (tau):                       counts +1.85e-08 (1.03e-07), signed +1.11e-09 (6.23e-08),
                                                   ints +3.63e-08 (2.33e-07), leftskew -5.00e-08 (5.76e-07)
  the references among themselves, - sklearn:      fp64 Brent +2.52e-08 / +1.12e-09 / +3.63e-08 / -9.69e-08,
                                                   fp80 Brent +1.76e-08 / +1.12e-09 / +4.72e-08 / -5.00e-08
end to end, max |r - z_ref| over kept rows (eps):  ints 5.88e-08 (7.53e-07), counts 9.41e-08 (1.05e-06)
"""


def _mods():
    from seoul_tourism_recommendation_ngcf_amd import engine, preprocess
    return engine, preprocess


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64)).to(DEV)               # a copy: the shared arrays are read-only


@functools.lru_cache(maxsize=None)
def _fixture():
    return power_oracle.load_fixture()


@functools.lru_cache(maxsize=None)
def _psi_cases():
    return power_oracle.psi_cases()


# ---- psi ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T1", "T63", "T64", "T65", "T257"] + list(power_oracle.NAMES))
def test_psi_against_the_oracle(name):
    engine, _ = _mods()
    x = _psi_cases()[name]
    x_d = _dev(x)
    worst = 0.0
    for lam in power_oracle.psi_lambdas():
        want, unit = power_oracle.psi(x, lam), power_oracle.psi_unit(x, lam)
        got_d = engine.yeo_johnson(x_d, lam)
        got = got_d.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(want), np.isnan(x)), lam
        exact = ~np.isfinite(unit) | (unit == 0)                                  # infinities (and pow results that overflow)
        assert np.array_equal(got[exact], want[exact], equal_nan=True), (lam, x[exact][got[exact] != want[exact]][:8])
        err = np.abs(got[~exact] - want[~exact]) / unit[~exact]
        if err.size:
            worst = max(worst, float(err.max()))
            assert err.max() <= K_PSI, (lam, x[~exact][np.argmax(err)], float(err.max()))
        alias = x_d.clone()
        assert engine.yeo_johnson(alias, lam, out=alias) is alias and torch.equal(alias.view(torch.int64), got_d.view(torch.int64)), lam
    print(f"psi {name}: largest |dev - oracle| = {worst:.3f} units (allowed {K_PSI})")
    assert np.array_equal(x_d.cpu().numpy(), x, equal_nan=True)                   # the input is not written


# ---- moments -----------------------------------------------------------------------------------------------------------------------
def _fsum_ld(terms):
    """math.fsum of extended-precision terms: each as a double plus its remainder."""
    hi = terms.astype(np.float64)
    lo = (terms - hi).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def _moment_sizes():
    engine, _ = _mods()
    _, threads, cap = engine.yeo_johnson_launch(0)
    sizes = {0, 1, 2, 63, 64, 65, 255, 256, 257, threads - 1, threads, threads + 1, 2 * cap * threads + 1}
    assert engine.yeo_johnson_launch(2 * cap * threads + 1)[0] == cap             # the grid is full: a third pass of one element
    return sorted(sizes)


def _check_moments(x, lam, what):
    """n exact; mean, M2 and c against math.fsum over the device's own psi and numpy's log1p, within (ceil(log2 T) + 8) 2^-52 of
    the sum of the terms' magnitudes - the rule of the standard_stats tests; two calls give the same bits."""
    engine, _ = _mods()
    x_d = _dev(x)
    res_d = engine.yeo_johnson_moments(x_d, lam)
    assert res_d.dtype == torch.float64 and res_d.shape == (4,) and res_d.device == x_d.device
    assert torch.equal(engine.yeo_johnson_moments(x_d, lam).view(torch.int64), res_d.view(torch.int64)), what
    n, mean, m2, c = res_d.tolist()
    keep = ~np.isnan(x)
    assert n == keep.sum(), what
    if n == 0:
        assert (mean, m2, c) == (0.0, 0.0, 0.0), what
        return 0.0
    y = engine.yeo_johnson(x_d, lam).cpu().numpy()[keep]
    L = (math.ceil(math.log2(len(x))) if len(x) > 1 else 0) + 8
    want_mean = math.fsum(y.tolist()) / n
    dev = y.astype(np.longdouble) - np.longdouble(want_mean)
    want_m2 = _fsum_ld(dev * dev)
    t = np.sign(x[keep]) * np.log1p(np.abs(x[keep]))
    want_c = math.fsum(t.tolist())
    figures = (abs(mean - want_mean) / (L * EPS * math.fsum(np.abs(y).tolist()) / n) if np.abs(y).max() > 0 else float(mean != 0),
               abs(m2 - want_m2) / (L * EPS * want_m2) if want_m2 > 0 else float(m2 != 0),
               abs(c - want_c) / (L * EPS * math.fsum(np.abs(t).tolist())) if np.abs(t).max() > 0 else float(c != 0))
    assert max(figures) <= 1.0, (what, figures, (mean, want_mean), (m2, want_m2), (c, want_c))
    return max(figures)


def test_moments_sizes_around_the_launch_constants():
    rng = np.random.default_rng(5)
    worst = 0.0
    for T in _moment_sizes():
        x = np.floor(np.exp(rng.normal(3.0, 1.5, T))) * np.where(rng.random(T) < 0.3, -1.0, 1.0)      # both branches of psi
        for lam in (0.5,) if T > 100000 else (0.5, -0.0413, 2.0, 3.17):
            worst = max(worst, _check_moments(x, lam, (T, lam)))
    print(f"moments: largest error = {worst:.3f} of the bound")


def test_moments_with_nans_and_fixture_columns():
    rng = np.random.default_rng(6)
    fx = _fixture()
    worst = 0.0
    for name in power_oracle.NAMES:
        x = fx["x_" + name]
        worst = max(worst, _check_moments(x, float(fx["lam_" + name]), name))
        holes = x.copy()
        holes[rng.random(len(x)) < 0.1] = np.nan                                  # NaN rows are left out, as sklearn leaves them out
        worst = max(worst, _check_moments(holes, float(fx["lam_" + name]), name + " with NaNs"))
    for T in (1, 64, 257, 1000):
        _check_moments(np.full(T, np.nan), 0.5, f"all NaN {T}")
    one = np.full(300, np.nan)
    one[171] = 7.0                                                                # a single row among NaNs: M2 exactly 0
    engine, _ = _mods()
    n, mean, m2, c = engine.yeo_johnson_moments(_dev(one), 1.0).tolist()
    assert (n, mean, m2) == (1.0, 7.0, 0.0) and c == np.log1p(7.0)
    print(f"moments (fixture, NaNs): largest error = {worst:.3f} of the bound")


# ---- the fit -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lambda_tolerance(name):
    """tau = 4 tol1(lambda) + 4 s, s the spread of three reference computations: sklearn's stored lambda, the oracle's Brent in fp64,
    and the oracle's Brent with the likelihood in np.longdouble."""
    fx = _fixture()
    x, lam = fx["x_" + name], float(fx["lam_" + name])
    l64, l80 = power_oracle.fit_lambda(x), power_oracle.fit_lambda(x, np.longdouble)
    s = max(abs(l64 - lam), abs(l80 - lam), abs(l64 - l80))
    return lam, 4 * power_oracle.tol1(lam) + 4 * s


@pytest.mark.parametrize("name", power_oracle.NAMES)
def test_fitted_lambda_against_sklearns(name):
    _, preprocess = _mods()
    lam_ref, tau = _lambda_tolerance(name)
    x_d = _dev(_fixture()["x_" + name])
    lam = preprocess.yeo_johnson_lambda(x_d)
    print(f"lambda {name}: dev - sklearn = {lam - lam_ref:+.2e} (tau {tau:.2e})")
    assert abs(lam - lam_ref) <= tau
    ps = preprocess.fit_power(x_d)
    assert isinstance(ps, preprocess.PowerScaler) and ps.lam == lam               # the fit is reproducible
    mean, scale, shift = power_oracle.standardise(power_oracle.psi(_fixture()["x_" + name], lam))
    assert abs(ps.mean - mean) <= 1e-12 * (1 + abs(mean)) and abs(ps.scale / scale - 1) <= 1e-12 and abs(ps.shift - shift) <= 1e-12 * (1 + shift)


def test_fit_refuses_a_column_without_finite_rows():
    _, preprocess = _mods()
    for x in (np.zeros(0), np.full(5, np.nan), np.array([np.nan, np.inf, -np.inf])):
        with pytest.raises(ValueError, match="no finite row"):
            preprocess.yeo_johnson_lambda(_dev(x))


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ints", "counts"])
def test_end_to_end_scale_implicit_with_a_fitted_scaler(name):
    engine, preprocess = _mods()
    x = _fixture()["x_" + name]
    users = power_oracle.users()
    n_user = len(power_oracle.LENGTHS)
    segments = quantile_oracle.segments_of(users, n_user)
    assert sorted(len(s) for s in segments) == sorted(power_oracle.LENGTHS)
    lam_ref, tau = _lambda_tolerance(name)
    z_ref = power_oracle.ratings_unfloored(x, lam_ref)
    # eps: the psi tolerance carried through / scale, plus what the lambda tolerance moves the oracle's ratings by
    _, scale_ref, _ = power_oracle.standardise(power_oracle.psi(x, lam_ref))
    eps = K_PSI * float(np.nanmax(power_oracle.psi_unit(x, lam_ref))) / scale_ref \
        + float(np.abs(power_oracle.ratings_unfloored(x, lam_ref + tau) - power_oracle.ratings_unfloored(x, lam_ref - tau)).max())

    users_d, x_d = torch.as_tensor(users).to(DEV), _dev(x)
    ps = preprocess.fit_power(x_d)
    ratings, quart = preprocess.scale_implicit(users_d, x_d, n_user=n_user, scaler=ps)
    assert ratings.dtype == torch.float64 and ratings.shape == (len(x),) and quart.shape == (n_user,)
    assert np.array_equal(x_d.cpu().numpy(), x)                                   # the caller's column is not written
    r, qd = ratings.cpu().numpy(), quart.cpu().numpy()
    floored = r == 0
    kept = ~floored
    qrow = qd[users]
    print(f"end to end {name}: eps {eps:.2e}, max |r - z_ref| over kept rows {np.abs(r - z_ref)[kept].max():.2e}, floored {floored.sum()}")
    assert (np.abs(r - z_ref)[kept] <= eps).all() and (z_ref[kept] >= qrow[kept] - eps).all()
    assert (z_ref[floored] <= qrow[floored] + eps).all()
    want_q = np.array([quantile_oracle.quantile_sorted(np.sort(z_ref[s]), 1) for s in segments])
    assert (np.abs(qd - want_q) <= eps).all()
    for s in segments:                                                            # equal counts of one user: equal ratings
        _, inv = np.unique(x[s], return_inverse=True)
        for g in range(inv.max() + 1):
            assert len(set(r[s][inv == g].tolist())) == 1
    assert r[np.argmin(x)] == 0.0 and r.min() == 0.0                              # the global minimum: exactly 0 (or floored)
    assert 0.1 * len(x) < floored.sum() < 0.3 * len(x)

    # a hand-built scaler: bit-equal to the two engine calls by hand
    hand = preprocess.PowerScaler(0.37, -1.5, 2.25, 0.75)
    ratings, quart = preprocess.scale_implicit(users_d, x_d, n_user=n_user, scaler=hand)
    rowptr, order = engine.segments_from_ids(users_d, n_user)
    want, want_quart = engine.segment_quantile_floor(rowptr, engine.yeo_johnson(x_d, hand.lam), order=order, mean=hand.mean,
                                                     scale=hand.scale, shift=hand.shift, q=0.25)
    assert torch.equal(ratings.view(torch.int64), want.view(torch.int64)) and torch.equal(quart.view(torch.int64), want_quart.view(torch.int64))
    # an integer column is converted, transformed and floored without touching the caller's tensor
    xi = torch.as_tensor(x.astype(np.int64)).to(DEV)
    ri, _ = preprocess.scale_implicit(users_d, xi, n_user=n_user, scaler=hand)
    assert torch.equal(ri.view(torch.int64), want.view(torch.int64)) and xi.dtype == torch.int64
