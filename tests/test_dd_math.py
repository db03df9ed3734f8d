"""csrc/dd_math.h on the CPU: the header the haversine kernel takes its sin, cos and asin from is plain C++ out of IEEE operations, so a
host compiler builds the same text, and mpmath says whether every result is the correctly rounded one."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import context_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc", "dd_math.h")
SOURCE = r'''
#include "%s"
#include <cstdint>
extern "C" void dd_fn(int which, const double *x, int64_t n, double *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = which == 0 ? ddm::sin_cr(x[i]) : which == 1 ? ddm::cos_cr(x[i]) : ddm::asin_cr(x[i]);
}
// the kernel's formula, operation for operation
extern "C" void dd_table(const double *dep, int64_t S, const double *item, int64_t n, double *out)
{
    const double k = 3.14159265358979323846 / 180.0, two_r = 2 * 6371.0088;
    for (int64_t s = 0; s < S; ++s)
        for (int64_t i = 0; i < n; ++i) {
            const double lat1 = dep[2 * s] * k, lng1 = dep[2 * s + 1] * k, lat2 = item[2 * i] * k, lng2 = item[2 * i + 1] * k;
            const double dlat = lat2 - lat1, dlng = lng2 - lng1;
            const double a = ddm::sin_cr(dlat * 0.5), b = ddm::sin_cr(dlng * 0.5);
            const double aa = a * a, bb = b * b;
            const double cc = ddm::cos_cr(lat1) * ddm::cos_cr(lat2);
            const double ccbb = cc * bb;
            const double d = aa + ccbb;
            const double km = two_r * ddm::asin_cr(sqrt(d));
            out[s * n + i] = km * 1000.0;
        }
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: csrc/dd_math.h cannot be checked")
    d = tmp_path_factory.mktemp("dd_math")
    src, so = os.path.join(d, "dd.cpp"), os.path.join(d, "libdd.so")
    with open(src, "w") as f:
        f.write(SOURCE % HEADER)
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", so, src])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _fn(lib, which, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lib.dd_fn(which, _ptr(x), ctypes.c_int64(len(x)), _ptr(out))
    return out


def test_sin_cos_asin_are_correctly_rounded_against_mpmath(lib):
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng(11)
    half_pi = np.arange(-6, 7) * (np.pi / 2)                                           # doubles next to the multiples of pi/2
    near = np.concatenate([half_pi, np.nextafter(half_pi, 9.0), np.nextafter(half_pi, -9.0)])
    cases = ((0, mp.sin, np.concatenate([rng.uniform(-4, 4, 1500), rng.uniform(-1e-3, 1e-3, 1000), rng.uniform(-9e4, 9e4, 300), near,
                                         [5e-324, 1e-300, -1e-200]])),
             (1, mp.cos, np.concatenate([rng.uniform(-4, 4, 1500), rng.uniform(-9e4, 9e4, 300), near, [0.0, 1e-300]])),
             (2, mp.asin, np.concatenate([rng.uniform(0, 1, 1500), rng.uniform(0, 1e-2, 1000), 1 - rng.uniform(0, 1e-9, 200),
                                          [1.0, 1 - 2.0 ** -53, 5e-324, 1e-300, 0.5]])))
    with mp.workprec(250):
        for which, f, xs in cases:
            want = np.array([float(f(mp.mpf(float(v)))) for v in xs])
            got = _fn(lib, which, xs)
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (which, xs[got != want][:5])
    # what the functions pass on to the maths library, and the signed zero
    for which in (0, 1, 2):
        assert np.isnan(_fn(lib, which, [np.nan, np.inf])).all()
    assert np.isnan(_fn(lib, 2, [1.0000000000000002, -2.0])).all() and _fn(lib, 2, [0.0])[0] == 0.0
    z = _fn(lib, 0, [0.0, -0.0])
    assert z[0] == 0 and z[1] == 0 and not np.signbit(z[0]) and np.signbit(z[1])
    assert np.allclose(_fn(lib, 0, [1e6, -3e8]), np.sin([1e6, -3e8]), rtol=0, atol=1e-15)


def test_the_formula_with_these_functions_has_the_bits_of_pythons_math(lib):
    """glibc's sin, cos and asin round correctly on all but a few arguments in a thousand: on the GPU tests' points the formula gives
    Python's bits everywhere, and numpy's wherever numpy's arcsin agrees with `math`."""
    for kind, S, n_item in (("seoul", 3, 130), ("globe", 3, 130), ("seoul", 17, 257)):
        dep, item = orc.points(kind, S, n_item)
        got = np.empty((S, n_item))
        lib.dd_table(_ptr(np.ascontiguousarray(dep)), ctypes.c_int64(S), _ptr(np.ascontiguousarray(item)), ctypes.c_int64(n_item), _ptr(got))
        by_math, by_numpy = orc.haversine_math(dep, item), orc.haversine_numpy(dep, item)
        assert np.array_equal(got, by_math), kind
        assert orc.ulps(got, by_numpy).max() <= orc.ulps(by_math, by_numpy).max()
