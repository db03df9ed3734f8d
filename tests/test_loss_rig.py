"""`loss_rig.held`, the tolerance rule of the loss family's GPU tests, on made-up numbers: it has to be able to fail.  The oracle
value 1.0 has a float32 ulp of 2^-23; every error below is an exact multiple of it in float64."""
import numpy as np
import pytest

from loss_rig import held, ulp32

ULP = 2.0 ** -23


def _case(e_fused, e_other, want=1.0):
    """(fused, other, want) as 3-vectors whose largest magnitude is `want` and whose largest errors are the given ones."""
    w = np.array([want, want / 4, -want / 2])
    return w + np.array([0.0, e_fused, 0.0]), w + np.array([-e_other, 0.0, e_other / 2]), w


def test_ulp32_is_the_float32_spacing_at_the_magnitude():
    assert ulp32(1.0) == ulp32(-1.0) == ULP and ulp32(1.5) == ULP and ulp32(2.0) == 2 * ULP and ulp32(1024.0) == 1024 * ULP


def test_an_error_just_above_the_bound_is_reported_and_just_below_is_not():
    e = 3 * ULP                                                               # bound: 2 e + 4 ulp = 10 ulp
    ratios = {}
    assert held("t", *_case(10 * ULP, e), ratios) is None and ratios["t"] == 1.0     # the bound itself holds
    assert held("t", *_case(9.75 * ULP, e), ratios) is None
    bad = held("t", *_case(10.25 * ULP, e), ratios)
    assert bad is not None and bad.startswith("t: fused error") and "bound" in bad
    assert ratios["t"] == 10.25 / 10                                          # the largest ratio seen stays
    assert held("t", *_case(ULP, e), ratios) is None and ratios["t"] == 10.25 / 10
    assert held("other", *_case(ULP, e), ratios) is None and ratios["other"] == 0.1


def test_with_an_exact_comparator_the_four_ulp_alone_decide():
    assert held("t", *_case(4 * ULP, 0.0), {}) is None
    assert held("t", *_case(4.5 * ULP, 0.0), {}) is not None
    assert held("loss", 1.0 + 4 * ULP, 1.0, 1.0, {}) is None and held("loss", 1.0 + 5 * ULP, 1.0, 1.0, {}) is not None    # 0-dim too


def test_the_ulp_is_taken_at_the_oracles_largest_magnitude_not_at_the_error():
    """At max|want| = 1024 the 4 ulp are 4096 times the 4 ulp at 0.25: an error of 2^-13 holds there and fails here, whatever
    the error's own size, and the element that carries the error is not the largest one."""
    err = 2.0 ** -13
    assert held("t", *_case(err, 0.0, want=1024.0), {}) is None               # bound 4 * 2^-13
    assert held("t", *_case(err, 0.0, want=0.25), {}) is not None             # bound 4 * 2^-25
    assert ulp32(err) < err / 1e6                                             # (4 ulp of the error itself would refuse both)


def test_a_fused_value_that_is_not_finite_or_not_of_the_oracles_shape_raises():
    w = np.ones(3)
    for poison in (np.nan, np.inf, -np.inf):
        with pytest.raises(AssertionError):
            held("t", np.array([1.0, poison, 1.0]), w, w, {})
    with pytest.raises(AssertionError):
        held("t", np.ones(2), w, w, {})
    assert held("t", w, np.array([np.nan, 1.0, 1.0]), w, {}) is not None      # a comparator that is not finite gives no allowance
    assert held("dx", np.zeros((0, 5)), np.zeros((0, 5)), np.zeros((0, 5)), {}) is None      # a gradient without rows holds
