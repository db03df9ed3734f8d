"""CPU tests of tests/row_oracle.py: the emulation of the gather backward's summation order, and the preconditions that make the
float64 references of the BPR and LeakyReLU/normalise backward unambiguous on the inputs tests/test_row_kernels_gpu.py uses."""
import numpy as np
import pytest
import torch

import ngcf_oracle as orc
import row_oracle as ro


def _one_segment(length, d=7, seed=0):
    rng = np.random.default_rng(seed + length)
    g = (rng.standard_normal((length + 3, d)) * 10.0 ** rng.integers(-3, 4, (length + 3, 1))).astype(np.float32)
    order = rng.permutation(length + 3)[:length].astype(np.int64)
    return g, order, np.array([0, length], dtype=np.int64)


@pytest.mark.parametrize("length", [0, 1, 2, 3])
def test_chains_of_a_short_segment_are_a_left_to_right_sum(length):
    g, order, segptr = _one_segment(length)
    want = np.zeros(g.shape[1], dtype=np.float32)
    for k in order:
        want = want + g[k]
    got = ro.segment_sum_chains(g, order, segptr)
    assert got.dtype == np.float32 and np.array_equal(got[0], want)


def test_chains_follow_the_documented_order_on_a_hand_worked_segment():
    """Six entries chosen so that every other association rounds differently: 2^24 absorbs a lone 1 but not 1 + 1.
    n4 = 4: s0 = g0, s1 = g1, s2 = g2, s3 = g3, then the tail g4, g5 -> s0; result (s0 + s1) + (s2 + s3)."""
    big = np.float32(2.0 ** 24)
    g = np.array([[big], [1.0], [1.0], [1.0], [1.0], [-big]], dtype=np.float32)
    # s0 = (2^24 + 1) - 2^24 = 0 (the 1 is absorbed); (0 + 1) + (1 + 1) = 3.  The exact sum is 4 (also what a tail on chain 1
    # gives), left to right gives 0
    got = ro.segment_sum_chains(g, np.arange(6), np.array([0, 6]))
    assert got[0, 0] == np.float32(3.0)


@pytest.mark.parametrize("length", sorted(set(ro.SEG_LENGTHS) | {2, 6, 7, 8, 9}))
def test_chains_stay_within_the_float64_bound(length):
    g, order, segptr = _one_segment(length, d=33)
    got = ro.segment_sum_chains(g, order, segptr)
    want, bound = ro.segment_sum_f64(g, order, segptr)
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound)


def test_segment_case_holds_every_length_and_a_permutation():
    g, order, segptr = ro.segment_case(5, seed=1)
    assert sorted(np.diff(segptr).tolist()) == sorted(ro.SEG_LENGTHS)
    assert np.array_equal(np.sort(order), np.arange(len(g))) and not np.all(np.diff(order) > 0)


@pytest.mark.parametrize("R,D,broadcast", [(R, D, "") for R, D in ro.BPR_SHAPES] + [(1029, 65, b) for b in ro.BPR_BROADCAST])
def test_bpr_inputs_keep_the_reference_away_from_the_kink(R, D, broadcast):
    """Every u.p and u.n is exactly 0 or at least 1e-3 of its sum of magnitudes; the scores reach both saturated regimes and the
    neighbourhood of 0; the float64 gradients are finite, and zero where both signs are zero."""
    u, p, n = ro.bpr_inputs(R, D, seed=R + D, broadcast=broadcast)
    assert u.shape == (1 if "u" in broadcast else R, D) and p.shape == (1 if "p" in broadcast else R, D)
    up, un, margin = ro.bpr_scores(u, p, n)
    assert margin >= 1e-3
    x = up.abs() - un.abs()
    assert float(x.abs().max()) <= 125.0
    if R >= 1023:
        assert float(x.min()) < -90 and float(x.max()) > 90 and float(x.abs().min()) < 1.0
    if not broadcast and R >= 3:
        assert float(up[1]) == 0.0 and float(un[1]) == 0.0 and float(up[2]) == 0.0 and float(un[2]) != 0.0
    t = [v.double().requires_grad_(True) for v in (u, p, n)]
    orc.bpr_torch(*t, 0.025, 64).backward()
    assert all(bool(torch.isfinite(v.grad).all()) for v in t)
    if not broadcast and R >= 3:
        assert bool((t[0].grad[1] == 0).all())                      # sign(0) = 0 twice, and the weight decay of a zero row


@pytest.mark.parametrize("d", ro.PRE_D)
def test_pre_inputs_keep_c_away_from_its_kink_and_the_reference_finite(d):
    for drop_p in (0.0, 0.3):
        M, dN, dC, mask = ro.pre_inputs(5, d, seed=d, drop_p=drop_p, zero_row=3)
        C, dM = ro.pre_reference(M, mask, dN, dC, 0.2)
        assert not bool(((C != 0) & (C.abs() < 1e-6)).any()) and bool((C[3] == 0).all())
        assert bool(torch.isfinite(dM).all())
        # the clamped row: N = C / eps there, so dM = slope * (dN / eps + dC) * mask
        want = 0.2 * (dN[3].double() / 1e-12 + dC[3].double()) * mask[3].double()
        assert torch.allclose(dM[3], want, rtol=1e-12, atol=0.0)
        if drop_p > 0:
            assert set(np.unique(mask.numpy()).tolist()) <= {0.0, np.float32(1 / 0.7).item()}
