"""The per-segment quantile floor on the device (ngcf_segment_quantile_floor_f64, engine.segment_quantile_floor, preprocess): every
quantile and every output value against the plain-numpy statement (tests/quantile_oracle.py), which tests/test_preprocess_surface.py
pins to pandas and np.percentile.  Quantiles are compared with ==, outputs with np.array_equal: bit for bit up to the sign of a zero."""
import functools
import math

import numpy as np
import pytest
import torch

import quantile_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# both sides of the 64-value switch between the tiers, (n - 1) % 4 in all four classes, the empty segment, one that fits the
# workgroup tier's LDS (1025) and one that does not (9000)
LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 66, 255, 256, 257, 1025, 9000)
QS = {0.25: 1, 0.5: 2, 0.75: 3}
TIERS = (0, 1)                            # wave_max: the default switch, and everything longer than 1 on the workgroup tier


def _eng():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)            # a copy: the shared arrays are read-only


def _layout(lengths, seed):
    """Segments of the given lengths over shuffled positions: (list of position arrays, rowptr, order)."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    segments = quantile_oracle.segments_of(ids, len(lengths))
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    order = np.concatenate(segments).astype(np.int64) if len(ids) else np.zeros(0, dtype=np.int64)
    return segments, rowptr, order


def _run(rowptr, order, x, q=0.25, **kw):
    out, quant = _eng().segment_quantile_floor(_dev(rowptr), _dev(x, torch.float64), order=None if order is None else _dev(order), q=q, **kw)
    return out, quant


def _same(out, quant, want_out, want_q, what=""):
    """Exact agreement with the oracle; NaN quantiles (empty segments) in the same places."""
    out, quant = out.cpu().numpy(), quant.cpu().numpy()
    nan = np.isnan(want_q)
    assert np.array_equal(np.isnan(quant), nan), what
    assert (quant[~nan] == want_q[~nan]).all(), (what, np.flatnonzero(quant != want_q)[:8])
    assert np.array_equal(out, want_out, equal_nan=True), (what, np.flatnonzero(out != want_out)[:8])


@functools.lru_cache(maxsize=None)
def _lengths_case():
    segments, rowptr, order = _layout(LENGTHS, 1)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(len(order))
    x[7::7] = x[6:-1:7]                                                          # ties
    x.setflags(write=False)
    return segments, rowptr, order, x


@pytest.mark.parametrize("q", sorted(QS))
def test_lengths(q):
    segments, rowptr, order, x = _lengths_case()
    want_out, want_q = quantile_oracle.floor_segments(segments, x, QS[q])
    assert np.isnan(want_q[0]) and not np.isnan(want_q[1:]).any()
    out, quant = _run(rowptr, order, x, q)
    _same(out, quant, want_out, want_q)
    assert 0 < int((out == 0).sum()) < len(x)


def test_tier_independence():
    segments, rowptr, order, x = _lengths_case()
    base_out, base_q = _run(rowptr, order, x)
    for wave_max in (1, 8, 64):
        out, quant = _run(rowptr, order, x, wave_max=wave_max)
        assert torch.equal(out.view(torch.int64), base_out.view(torch.int64)), wave_max      # the same bits, zeros and NaN included
        assert torch.equal(quant.view(torch.int64), base_q.view(torch.int64)), wave_max


def _tie_segments():
    """Sorted value lists whose two order statistics tie with each other or with their neighbours, at a wave-tier and a
    workgroup-tier length (q = 0.25: lo = 1 of 6 values, lo = 17 of 70)."""
    segs = []
    for n, lo in ((6, 1), (70, 17)):
        base = np.arange(n, dtype=np.float64) * 1.5 - 7.0
        for tied in ((lo, lo + 1), (lo - 1, lo), (lo + 1, lo + 2), (lo - 1, lo, lo + 1), (lo, lo + 1, lo + 2)):
            s = base.copy()
            s[list(tied)] = s[tied[0]]
            segs.append(s)
        segs.append(np.full(n, 3.25))                                            # all equal
        segs.append(np.full(n, -0.0))
    return segs


def test_ties_and_edges():
    tiny = 5e-324
    segs = _tie_segments() + [
        np.array([-3.5, -1.0, -2.25, -8.0, -1.0, -0.5, -100.0]),                 # negative values
        -np.arange(1.0, 81.0) / 3.0,
        np.array([tiny, 3 * tiny, -tiny, 0.0, 1e-310, -1e-310, 2 * tiny, 2.2250738585072014e-308, tiny]),      # subnormals
        np.concatenate([np.array([tiny, -tiny, 1e-310, 2 * tiny]), np.arange(70) * tiny]),
        np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, -0.0]),                       # -0.0 among zeros
        np.concatenate([np.zeros(40), -np.zeros(40), [1.0, -1.0, 2.0]]),
        np.array([1e150, -1e150, 1e-150, 3.0, -1e149, 1e149, 7e149, -1e-150]),   # b - a stays finite up to 1e150
        np.concatenate([np.linspace(-1e150, 1e150, 67), [1e-150, -1e-150, 0.5]]),
    ]
    lengths = [len(s) for s in segs]
    segments, rowptr, order = _layout(lengths, 3)
    x = np.zeros(sum(lengths))
    rng = np.random.default_rng(4)
    for s, pos in zip(segs, segments):
        x[pos] = rng.permutation(s)
    for q, q4 in QS.items():
        want_out, want_q = quantile_oracle.floor_segments(segments, x, q4)
        for wave_max in TIERS:
            out, quant = _run(rowptr, order, x, q, wave_max=wave_max)
            _same(out, quant, want_out, want_q, (q, wave_max))


def test_rounding_of_the_transform_and_the_blend():
    """Integer counts standardised with numpy's stats passed in: every output bit depends on the subtraction, the division and the
    addition each rounding once, which an inexact (reciprocal) division or a fused operation would change."""
    lengths = (2, 3, 4, 65, 257) * 8
    segments, rowptr, order = _layout(lengths, 5)
    rng = np.random.default_rng(6)
    x = rng.integers(0, 50, len(order)).astype(np.float64)
    x[rng.random(len(x)) < 0.02] *= 1000.0
    mean, scale = float(x.mean()), float(x.std())
    shift = float(np.abs(quantile_oracle.transform(x, mean, scale).min()))
    stats = dict(mean=mean, scale=scale, shift=shift)
    for q, q4 in QS.items():
        want_out, want_q = quantile_oracle.floor_segments(segments, x, q4, **stats)
        assert want_out.min() == 0.0
        for wave_max in TIERS:
            out, quant = _run(rowptr, order, x, q, wave_max=wave_max, **stats)
            _same(out, quant, want_out, want_q, (q, wave_max))


def test_layout():
    eng = _eng()
    segments, rowptr, order, x = _lengths_case()
    out, quant = _run(rowptr, order, x)
    # pre-grouped input, order = None
    out_g, quant_g = _run(rowptr, None, x[order])
    assert torch.equal(out_g.view(torch.int64), out[_dev(order)].view(torch.int64))
    assert torch.equal(quant_g.view(torch.int64), quant.view(torch.int64))
    # out aliasing x, both tiers, grouped and not
    for wave_max in TIERS:
        for o, xs, ref in ((order, x, out), (None, x[order], out_g)):
            xd = _dev(xs, torch.float64)
            got, q2 = eng.segment_quantile_floor(_dev(rowptr), xd, order=None if o is None else _dev(o), out=xd, wave_max=wave_max)
            assert got.data_ptr() == xd.data_ptr()
            assert torch.equal(got.view(torch.int64), ref.view(torch.int64)) and torch.equal(q2.view(torch.int64), quant.view(torch.int64))
    # segments_from_ids: the oracle's grouping, users without rows included
    rng = np.random.default_rng(7)
    ids = rng.integers(0, 50, 3000)
    ids[ids % 9 == 4] = 11                                                       # users 4, 13, 22, .. have no rows; user 11 many
    rp, od = eng.segments_from_ids(_dev(ids), 50)
    want = quantile_oracle.segments_of(ids, 50)
    assert rp.cpu().tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    assert od.cpu().tolist() == np.concatenate(want).tolist()
    assert any(len(s) == 0 for s in want) and max(len(s) for s in want) > 64
    v = rng.standard_normal(3000)
    want_out, want_q = quantile_oracle.floor_segments(want, v)
    got_out, got_q = eng.segment_quantile_floor(rp, _dev(v, torch.float64), order=od)
    _same(got_out, got_q, want_out, want_q)
    with pytest.raises(IndexError):
        eng.segments_from_ids(_dev(np.array([0, 50])), 50)


def test_status():
    eng = _eng()
    lengths = (9, 70, 5, 100, 64, 300)
    segments, rowptr, order = _layout(lengths, 8)
    T = len(order)
    x = np.random.default_rng(9).standard_normal(T)
    want_out, want_q = quantile_oracle.floor_segments(segments, x)

    def run(rowptr_, order_, x_, status=True):
        out = torch.full((T,), -7.0, dtype=torch.float64, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV) if status else None
        _, quant = eng.segment_quantile_floor(_dev(rowptr_), _dev(x_, torch.float64), order=_dev(order_), out=out, status=st)
        return out.cpu().numpy(), quant.cpu().numpy(), None if st is None else int(st.item())

    def check(out, quant, bad, what):
        for u, pos in enumerate(segments):
            if u in bad:
                assert (out[pos] == -7.0).all() and np.isnan(quant[u]), (what, u)            # untouched
            else:
                assert np.array_equal(out[pos], want_out[pos]) and quant[u] == want_q[u], (what, u)

    out, quant, st = run(rowptr, order, x)
    assert st == 0
    check(out, quant, (), "clean")
    # an order entry equal to T, in a wave-tier and in a workgroup-tier segment
    bad_order = order.copy()
    bad_order[rowptr[0] + 3] = T
    bad_order[rowptr[3] + 77] = T
    out, quant, st = run(rowptr, bad_order, x)
    assert st == 1
    check(out, quant, (0, 3), "order")
    bad_order[rowptr[3] + 77] = -1
    assert run(rowptr, bad_order, x)[2] == 1
    with pytest.raises(IndexError, match="outside"):
        run(rowptr, bad_order, x, status=False)
    # row pointers that decrease (segments 0 and 1 become [80, 79) and the empty [79, 79); the rest are as before) or leave [0, T]
    dec = rowptr.copy()
    dec[0], dec[1] = 80, 79
    out, quant, st = run(dec, order, x)
    assert st == 1 and np.isnan(quant[1])
    check(out, quant, (0, 1), "decreasing")
    past = rowptr.copy()
    past[-1] = T + 1
    out, quant, st = run(past, order, x)
    assert st == 1
    check(out, quant, (5,), "past the end")
    with pytest.raises(IndexError, match="outside"):
        run(dec, order, x, status=False)
    # a NaN: bit 2, the segment passes through, the others are exact; the wrapper does not raise for it
    xn = x.copy()
    xn[segments[2][1]] = np.nan
    xn[segments[5][200]] = np.nan
    want_out_n, want_q_n = quantile_oracle.floor_segments(segments, xn)
    assert np.isnan(want_q_n[[2, 5]]).all() and np.array_equal(want_out_n[segments[5]], xn[segments[5]], equal_nan=True)
    out, quant, st = run(rowptr, order, xn)
    assert st == 2
    _same(torch.as_tensor(out), torch.as_tensor(quant), want_out_n, want_q_n)
    out2, quant2, _ = run(rowptr, order, xn, status=False)
    assert np.array_equal(out2, out, equal_nan=True)
    assert run(rowptr, bad_order, xn)[2] == 3


@functools.lru_cache(maxsize=None)
def _visits():
    """300 users x 40 items over two years, about half of the combinations present, integer counts with a heavy tail."""
    rng = np.random.default_rng(10)
    n_user, n_item = 300, 40
    year, user, item = (a.reshape(-1) for a in np.meshgrid([18, 19], np.arange(n_user), np.arange(n_item), indexing="ij"))
    keep = rng.permutation(np.flatnonzero(rng.random(len(user)) < 0.5))
    year, user, item = year[keep], user[keep], item[keep]
    counts = rng.integers(0, 50, len(user))
    counts[rng.random(len(user)) < 0.02] *= 1000
    assert len(np.unique(user)) == n_user
    return n_user, n_item, year, user, item, counts


def test_end_to_end_scale_implicit():
    from seoul_tourism_recommendation_ngcf_amd import matrix, preprocess, sampling
    n_user, n_item, year, user, item, counts = _visits()
    n = len(counts)
    x = counts.astype(np.float64)
    mean, scale = float(x.mean()), float(np.sqrt(np.mean((x - x.mean()) ** 2)))           # StandardScaler's formulae
    shift = float(np.abs(quantile_oracle.transform(x, mean, scale).min()))
    segments = quantile_oracle.segments_of(user, n_user)
    want, want_q = quantile_oracle.floor_segments(segments, x, 1, mean, scale, shift)
    users_d, counts_d = _dev(user), _dev(counts)

    # device-computed stats: the same zeros, values within the derived bound (eps = 2^-52, L = ceil(log2 n) + 8)
    eps, L = 2.0 ** -52, math.ceil(math.log2(n)) + 8
    d_mean, d_scale, d_shift = preprocess.standard_stats(counts_d)
    assert d_mean == mean                                                         # an integer column: exact sum, one rounding
    print(f"scale dev/ref - 1 = {d_scale / scale - 1:.3e} (bound {L * eps:.3e})")
    assert abs(d_scale / scale - 1) <= L * eps
    ratings, quart = preprocess.scale_implicit(users_d, counts_d, n_user=n_user)
    assert ratings.dtype == torch.float64 and ratings.shape == (n,) and quart.shape == (n_user,)
    got = ratings.cpu().numpy()
    assert np.array_equal(got == 0, want == 0) and 0.2 * n < (want == 0).sum() < 0.3 * n
    bound = 2 * L * eps * max(1.0, np.abs(want).max())
    print(f"max |z_dev - z_ref| = {np.abs(got - want).max():.3e} (bound {bound:.3e})")
    assert np.abs(got - want).max() <= bound
    assert got.min() == 0.0 and int(np.argmin(x)) in np.flatnonzero(got == 0)

    # stats passed in: a pure function of its inputs, bit-equal
    ratings, quart = preprocess.scale_implicit(users_d, counts_d, n_user=n_user, stats=(mean, scale, shift))
    _same(ratings, quart, want, want_q)
    raw, raw_q = preprocess.scale_implicit(users_d, counts_d, n_user=n_user, scaler=None)
    _same(raw, raw_q, *quantile_oracle.floor_segments(segments, x))
    assert counts_d.cpu().tolist() == counts.tolist()                             # the caller's column is not written

    # downstream: the Laplacian slices from these ratings on the device equal the CPU builder's from the oracle's
    dev_slices = matrix.laplacian_slices(_dev(year), users_d, _dev(item), ratings, n_user, n_item, device=DEV)
    cpu_slices = matrix.laplacian_slices(year, user, item, want, n_user, n_item)
    assert sorted(dev_slices) == sorted(cpu_slices) == [0, 1]
    for k, parts in cpu_slices.items():
        for a, b in zip(dev_slices[k], parts):
            assert torch.equal(a.cpu(), b)
    # and the triplets over the positives: no negative is an item whose floored rating is > 0 for that user
    pos = preprocess.positives(ratings)
    assert pos.dtype == torch.bool and np.array_equal(pos.cpu().numpy(), want > 0)
    u, i, neg = sampling.train_triplets(users_d[pos], _dev(item)[pos], seed=11, n_user=n_user, n_item=n_item)
    liked = np.zeros((n_user, n_item), dtype=bool)
    liked[user[want > 0], item[want > 0]] = True
    u, neg = u.cpu().numpy(), neg.cpu().numpy()
    assert len(neg) == int((want > 0).sum()) and neg.min() >= 0 and neg.max() < n_item
    assert not liked[u, neg].any()
