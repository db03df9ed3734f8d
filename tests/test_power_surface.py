"""Host side of the Yeo-Johnson power scaler: the C ABI symbols and their argument errors before any launch, the public functions on
CPU tensors (no fallback), the host Brent loop against scipy's, and the test oracle (tests/power_oracle.py) pinned to sklearn's
PowerTransformer and to the committed fixture."""
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

import power_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ngcf_yeo_johnson_f64": 5, "ngcf_yeo_johnson_workspace_bytes": 1, "ngcf_yeo_johnson_moments_launch": 4,
           "ngcf_yeo_johnson_moments_f64": 7}


def test_header_declares_and_library_exports_the_symbols():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert "pow(x + 1, l) - 1) / l" in text and "log1p(|x|)" in text              # the formulae are written out
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for sym, n_args in SYMBOLS.items():
        assert re.search(r"\b(int|int64_t)\s+" + sym + r"\s*\(", text), sym
        assert hasattr(lib, sym) and len(_lib.PROTOTYPES[sym][1]) == n_args, sym
    assert any(p.endswith("yeo_johnson.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    for kernel in (b"yeo_johnson_kernel", b"yeo_johnson_moments_kernel", b"yeo_johnson_moments_final_kernel"):
        assert kernel in blob                                                     # gfx950 kernels of its own
    m = re.search(r"#define\s+NGCF_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "ngcf_hip.h")).read())
    assert int(m.group(1)) == int(lib.ngcf_version()) == _lib.ABI_VERSION


def test_c_abi_argument_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    p = torch.zeros(8, dtype=torch.float64).data_ptr()   # host memory: a call that got as far as a launch would not return ERR_ARG
    nan = float("nan")
    assert lib.ngcf_yeo_johnson_f64(None, 0, 0.5, None, None) == _lib.OK          # nothing to do is not an error
    for args, msg in (((p, -1, 0.5, p, None), "negative count"), ((None, 5, 0.5, p, None), "null argument"),
                      ((p, 5, 0.5, None, None), "null argument"), ((p, 5, nan, p, None), "lambda is NaN")):
        assert lib.ngcf_yeo_johnson_f64(*args) == _lib.ERR_ARG, args
        assert "yeo_johnson:" in _lib.last_error() and msg in _lib.last_error()
    for args, rc, msg in (((p, -1, 0.5, p, p, 64, None), _lib.ERR_ARG, "negative count"),
                          ((None, 5, 0.5, p, p, 64, None), _lib.ERR_ARG, "null argument"),
                          ((p, 5, 0.5, None, p, 64, None), _lib.ERR_ARG, "null argument"),
                          ((p, 5, 0.5, p, None, 64, None), _lib.ERR_ARG, "null argument"),
                          ((None, 0, 0.5, None, None, 0, None), _lib.ERR_ARG, "null argument"),      # the result is always written
                          ((p, 5, nan, p, p, 64, None), _lib.ERR_ARG, "lambda is NaN"),
                          ((p, 5, 0.5, p, p, 31, None), _lib.ERR_WORKSPACE, "32 needed"),
                          ((p, 5, 0.5, p, p + 4, 64, None), _lib.ERR_ARG, "not 8-byte aligned")):
        assert lib.ngcf_yeo_johnson_moments_f64(*args) == rc, args
        assert "yeo_johnson_moments:" in _lib.last_error() and msg in _lib.last_error(), (args, _lib.last_error())
    # the launch constants are queryable, the grid is a function of T alone, and the workspace is one 32-byte partial per workgroup
    import ctypes as C
    from seoul_tourism_recommendation_ngcf_amd import engine
    assert lib.ngcf_yeo_johnson_workspace_bytes(-1) == -1 and lib.ngcf_yeo_johnson_moments_launch(-1, None, None, None) == _lib.ERR_ARG
    _, threads, cap = engine.yeo_johnson_launch(0)
    assert threads % 64 == 0 and threads >= 64 and cap >= 1
    for T, blocks in ((0, 0), (1, 1), (threads, 1), (threads + 1, 2), (cap * threads, cap), (cap * threads + 1, cap), (2 ** 40, cap)):
        assert engine.yeo_johnson_launch(T) == (blocks, threads, cap)
        assert lib.ngcf_yeo_johnson_workspace_bytes(T) == 32 * blocks
    b = C.c_int(-1)
    assert lib.ngcf_yeo_johnson_moments_launch(5, C.byref(b), None, None) == _lib.OK and b.value == 1


def test_public_functions_exports_signatures_and_no_cpu_fallback():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    pre, engine = pkg.preprocess, pkg.engine
    assert list(inspect.signature(engine.yeo_johnson).parameters) == ["x", "lam", "out"]
    assert inspect.signature(engine.yeo_johnson).parameters["out"].default is None
    assert list(inspect.signature(engine.yeo_johnson_moments).parameters) == ["x", "lam"]
    sig = inspect.signature(pre.yeo_johnson_lambda)
    assert list(sig.parameters) == ["x", "brack", "tol", "maxiter"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("brack", "tol", "maxiter"))
    assert [sig.parameters[k].default for k in ("brack", "tol", "maxiter")] == [(-2.0, 2.0), 1.48e-8, 500]
    assert list(inspect.signature(pre.fit_power).parameters) == ["x"]
    assert [f.name for f in dataclasses.fields(pre.PowerScaler)] == ["lam", "mean", "scale", "shift"]
    ps = pre.PowerScaler(0.5, 1.0, 2.0, 3.0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        ps.lam = 1.0

    x = torch.tensor([3.0, 1.0, 4.0, 1.0], dtype=torch.float64)
    users = torch.tensor([0, 1, 1, 2])
    for call in (lambda: engine.yeo_johnson(x, 0.5), lambda: engine.yeo_johnson_moments(x, 0.5), lambda: pre.yeo_johnson_lambda(x),
                 lambda: pre.fit_power(x), lambda: pre.scale_implicit(users, x, n_user=3, scaler=ps)):
        with pytest.raises(RuntimeError, match="ROCm device"):                    # CPU tensors: no fallback, and no launch
            call()
    with pytest.raises(ValueError, match="carries its own"):
        pre.scale_implicit(users, x, n_user=3, scaler=ps, stats=(0.0, 1.0, 0.0))
    with pytest.raises(NotImplementedError, match=r"Yeo-Johnson.*scaler=preprocess\.fit_power\(visitors\)"):
        pre.scale_implicit(users, x, n_user=3, scaler="power")                    # the string is not an alias yet
    for fn in (engine.yeo_johnson, engine.yeo_johnson_moments):
        with pytest.raises(TypeError, match="x must be float64"):
            fn(x.float(), 0.5)
        with pytest.raises(ValueError, match=r"x must be \[T\]"):
            fn(x.reshape(2, 2), 0.5)
        with pytest.raises(ValueError, match="lam is NaN"):
            fn(x, float("nan"))
    with pytest.raises(ValueError, match=r"x must be \[T\]"):
        pre.yeo_johnson_lambda(x.reshape(2, 2))
    assert "fit_power" in pre.__doc__ and "power" in pre.__doc__ and "fit_power" in pre.scale_implicit.__doc__
    src = inspect.getsource(pre)
    assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", src, flags=re.M)     # the package needs neither


def test_host_brent_equals_scipys_on_the_oracle_likelihood():
    """The product's host loop and the oracle's, two independent writings of the algorithm, walk scipy's iterates: bit-equal minima."""
    optimize = pytest.importorskip("scipy.optimize")
    from seoul_tourism_recommendation_ngcf_amd import preprocess
    fx = power_oracle.load_fixture()
    for name in power_oracle.NAMES:
        f = lambda lam: power_oracle.neg_log_likelihood(fx["x_" + name], lam)  # noqa: E731
        want = optimize.brent(f, brack=(-2, 2))
        assert preprocess._brent(f, (-2.0, 2.0), 1.48e-8, 500) == want, name
        assert power_oracle.brent_min(f)[0] == want, name
    for f, brack in ((lambda v: (v - 3.0) ** 2 + 1.0, (-2.0, 2.0)), (lambda v: np.cosh(v + 7.5), (-2.0, 2.0)),
                     (lambda v: abs(v - 0.25) ** 1.5, (0.0, 1.0)), (lambda v: v ** 4 - 3 * v, (5.0, 4.0))):
        want = optimize.brent(f, brack=brack)
        assert preprocess._brent(f, brack, 1.48e-8, 500) == want
        assert power_oracle.brent_min(f, *brack)[0] == want


def test_oracle_equals_sklearn():
    PowerTransformer = pytest.importorskip("sklearn.preprocessing").PowerTransformer
    fx = power_oracle.load_fixture()
    pt = PowerTransformer()
    for name in power_oracle.NAMES:
        x, lam, z = fx["x_" + name], float(fx["lam_" + name]), fx["z_" + name]
        for l in (lam, 0.0, 2.0, 1.0, -2.0, 3.5):
            assert np.array_equal(power_oracle.psi(x, l), pt._yeo_johnson_transform(x, l)), (name, l)      # bit for bit
        # lambda: within the tolerance of the device tests, tau = 4 tol1 + 4 s
        l64, l80 = power_oracle.fit_lambda(x), power_oracle.fit_lambda(x, np.longdouble)
        s = max(abs(l64 - lam), abs(l80 - lam), abs(l64 - l80))
        print(f"{name}: sklearn {lam:.6f}, fp64 Brent {l64 - lam:+.2e}, fp80 Brent {l80 - lam:+.2e}")
        assert abs(l64 - lam) <= 4 * power_oracle.tol1(lam) + 4 * s
        assert s < 1e-6                                                           # honest computations agree to about sqrt(eps)
        # the unfloored ratings at sklearn's lambda are sklearn's standardised output plus |min|
        assert np.array_equal(power_oracle.ratings_unfloored(x, lam), z + np.abs(z.min())), name


def test_fixture_is_what_write_produces():
    fx = power_oracle.load_fixture()
    cols = power_oracle.columns()
    assert sorted(fx) == sorted(p + n for n in power_oracle.NAMES for p in ("x_", "lam_", "z_"))
    T = sum(power_oracle.LENGTHS)
    assert [len(cols[n]) for n in power_oracle.NAMES] == [T, 2000, T, 1500]
    for name, col in cols.items():
        assert 1000 <= len(col) <= 3000 and np.array_equal(fx["x_" + name], col), name
    assert (cols["counts"] >= 0).all() and (cols["counts"] == np.floor(cols["counts"])).all() and cols["counts"].max() > 1000
    assert (cols["signed"] < 0).any() and (cols["signed"] > 0).any()
    assert set(cols["ints"]) == set(range(50)) and (cols["leftskew"] < 0).all()
    assert sorted(np.bincount(power_oracle.users()).tolist()) == sorted(power_oracle.LENGTHS)
    pytest.importorskip("sklearn")
    now = power_oracle.build_fixture()
    for key, val in now.items():
        assert np.array_equal(fx[key], val), key


def test_oracle_edges_and_its_error_unit():
    x = np.array(power_oracle.SPECIALS)
    for lam in power_oracle.PSI_LAMBDAS:
        y = power_oracle.psi(x, lam)
        assert np.isnan(y[6]) and np.isnan(y).sum() == 1                          # only the NaN is a NaN
        assert y[0] == 0 and y[1] == 0 and y[2] >= 0 and y[3] <= 0
    assert power_oracle.psi(x, 0.0)[4] == np.log1p(1e300) and power_oracle.psi(x, 2.0)[5] == -np.log1p(1e300)
    assert power_oracle.psi(x, 3.5)[7] == np.inf and power_oracle.psi(x, -2.0)[7] == 0.5 and power_oracle.psi(x, 3.5)[8] == -2.0 / 3.0
    assert power_oracle.psi(x, 2.0 ** -53)[4] == np.log1p(1e300) and power_oracle.psi(x, 2.0 ** -51)[4] != np.log1p(1e300)
    # the unit: 2^-52 (|p| + |p - 1|) / |d| where pow runs, one spacing of psi on the log1p branches, NaN where psi is not finite
    u = power_oracle.psi_unit(np.array([3.0, -3.0, np.inf, 3.0]), 0.5)
    assert u[0] == 2.0 ** -52 * (2.0 + 1.0) / 0.5 and u[1] == 2.0 ** -52 * (8.0 + 7.0) / 1.5 and np.isnan(u[2])
    assert power_oracle.psi_unit(np.array([3.0]), 0.0)[0] == np.spacing(np.log1p(3.0))
    cases = power_oracle.psi_cases()
    assert [len(cases[f"T{T}"]) for T in power_oracle.PSI_SIZES] == list(power_oracle.PSI_SIZES)
    assert np.isnan(cases["T63"]).sum() == 1 and np.isinf(cases["counts"]).sum() == 2
    assert len(power_oracle.psi_lambdas()) == len(power_oracle.PSI_LAMBDAS) + 4
