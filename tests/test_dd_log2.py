"""csrc/dd_log2.h on the CPU: the log2 behind the position metrics' 1/log2(rank + 2) terms is plain C++ out of IEEE operations, so a
host compiler builds the same text, and mpmath says whether every result is the correctly rounded one."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc", "dd_log2.h")
SOURCE = r'''
#include "%s"
#include <cstdint>
extern "C" void dd_log2(const double *x, int64_t n, double *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = ddm::log2_cr(x[i]);
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: csrc/dd_log2.h cannot be checked")
    d = tmp_path_factory.mktemp("dd_log2")
    src, so = os.path.join(d, "dd.cpp"), os.path.join(d, "libddlog2.so")
    with open(src, "w") as f:
        f.write(SOURCE % HEADER)
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", so, src])
    return ctypes.CDLL(so)


def _log2(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lib.dd_log2(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(x)), out.ctypes.data_as(ctypes.c_void_p))
    return out


def test_log2_is_correctly_rounded_against_mpmath(lib):
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng(5)
    sqrt2 = np.sqrt(2.0)
    xs = np.concatenate([np.arange(1, 20001, dtype=np.float64),                              # every rank + 2 of a small catalogue
                         rng.integers(20001, 2 ** 31 + 2, 3000).astype(np.float64), [2.0 ** 31, 2.0 ** 31 + 1.0],
                         rng.uniform(0.5, 2.0, 3000), 1.0 + rng.uniform(-1e-9, 1e-9, 500), 2.0 ** rng.uniform(-1000, 1000, 1000),
                         [np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), sqrt2, np.nextafter(sqrt2, 0.0), np.nextafter(sqrt2, 2.0),
                          sqrt2 / 2, np.nextafter(sqrt2 / 2, 0.0), 2.0 ** -1022, np.finfo(np.float64).max]])
    with mp.workprec(300):
        want = np.array([float(mp.log(mp.mpf(float(v)), 2)) for v in xs])
    got = _log2(lib, xs)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), xs[got != want][:5]
    # exact powers of two, and what goes to the maths library as it is
    k = np.arange(-1022, 1024, dtype=np.float64)
    assert np.array_equal(_log2(lib, 2.0 ** k), k)
    assert np.isnan(_log2(lib, [np.nan, -1.0])).all() and _log2(lib, [0.0])[0] == -np.inf and _log2(lib, [np.inf])[0] == np.inf
    assert _log2(lib, [5e-324])[0] == -1074.0


def test_numpy_log2_has_these_bits_on_the_gpu_tests_range(lib):
    """numpy's log2 (the oracle's) rounds correctly on all but a handful of integers - none of them below 7957 -, so on the ranks the
    GPU tests reach, kernel and oracle add the same terms."""
    n = np.arange(2, 100002, dtype=np.float64)
    differ = n[_log2(lib, n) != np.log2(n)]
    assert differ.size == 0 or differ.min() > 5000
