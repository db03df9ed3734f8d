"""The certified two-stage ranking on the device (csrc/rank_prefilter.hip through engine.shortlist): every comparison is torch.equal with
engine.rank_topk on the same inputs - values as int32 bit patterns, indices as they are - with the fallback doing the work and
without it (then on the certified rows).  The tables are tests/prefilter_oracle.py's, which tests/test_rank_prefilter_oracle.py
checks on the host; ub, the threshold and the pool are never compared with that file (the MFMA's last bits are its own)."""
import functools

import numpy as np
import pytest
import torch

import prefilter_oracle as po

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _eng():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine


def _views(U, I):  # noqa: E741
    """Both tables as strided views of one all_E-like buffer (rows users then items, the columns off by one)."""
    B, D = U.shape
    all_e = torch.zeros((B + I.shape[0] + 1, D + 3), dtype=torch.float32, device=DEV)
    all_e[:B, 1:1 + D] = torch.from_numpy(U).to(DEV)
    all_e[B:-1, 1:1 + D] = torch.from_numpy(I).to(DEV)
    return all_e[:B, 1:1 + D], all_e[B:-1, 1:1 + D]


def _same(a, b, rows=None):
    (av, ai), (bv, bi) = a[:2], b[:2]
    if rows is not None:
        av, ai, bv, bi = av[rows], ai[rows], bv[rows], bi[rows]
    return torch.equal(av.view(torch.int32), bv.view(torch.int32)) and torch.equal(ai, bi)


def _sets(rows, n_items):
    eng = _eng()
    rowptr = torch.tensor([0] + np.cumsum([len(r) for r in rows]).tolist(), dtype=torch.int64, device=DEV)
    colidx = torch.tensor(np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, dtype=np.int64)]), dtype=torch.int32,
                          device=DEV)
    return eng.ItemSets(rowptr, colidx, 0, n_items)


def _check(u, items, k, pool, want_share=None, **kw):
    """Both modes against rank_topk; returns the certified mask."""
    eng = _eng()
    want = eng.rank_topk(u, items, k, **kw)
    got = eng.shortlist.rank_topk_certified(u, items, k, pool=pool, **kw)
    assert _same(got, want)
    v, i, cert = eng.shortlist.rank_topk_certified(u, items, k, pool=pool, fallback=False, return_certified=True, **kw)
    assert cert.dtype == torch.bool and _same((v, i), want, cert)
    if want_share is not None:
        assert float(cert.float().mean()) >= want_share
    return cert, (v, i), want


# D: padding of K (33), whole steps (64), more than one K chunk (130, 260); n_items = 100 < pool: the whole catalogue is the pool;
# 4 500 items with B = 40: two item splits and the merge; B = 257: five user tiles, the last one a single row
@pytest.mark.parametrize("B,n_items,D,k,pool", [(1, 100, 33, 1, 32), (40, 100, 64, 20, 128), (40, 700, 64, 20, 128), (40, 4500, 130, 20, 64),
                                                (257, 2000, 260, 100, 256), (40, 700, 33, 256, 256), (257, 700, 130, 20, 64)])
def test_equal_to_rank_topk_on_gaussian_tables(B, n_items, D, k, pool):
    u, items = _views(*po.gaussian_tables(B, n_items, D, B + D))
    # k = pool certifies only a pool that is not full; 100 < pool: always certified; else the observed error is a quarter of the bound
    share = None if k == pool else 1.0 if n_items < pool else 0.95
    _check(u, items, k, pool, share)
    rng = np.random.default_rng(B)
    rows = [np.sort(rng.choice(n_items, n_items // 5, replace=False)) for _ in range(B)]
    _check(u, items, k, pool, share, exclude=_sets(rows, n_items))
    ids = torch.tensor(rng.integers(0, B, 50), device=DEV)                 # repeats, any order
    _check(u, items, k, pool, share, user_ids=ids, exclude=_sets(rows, n_items))


def test_popular_head_table_is_certified():
    u, items = _views(*po.popular_head_tables(257, 2000, 64, 11))
    _check(u, items, 20, 128, 0.95)
    _check(u, items, 1, 32, 0.95)


def test_exclusion_edges():
    """n_items = 4500, B = 40: two splits of 2304 items.  All items excluded; fewer eligible than k; between k and pool eligible (a
    pool that is not full: certified); rows that hold both sides of a tile boundary and of the split boundary; ids out of range."""
    n, k, pool = 4500, 20, 64
    u, items = _views(*po.gaussian_tables(40, n, 64, 3))
    rng = np.random.default_rng(4)
    every = np.arange(n)
    edge = np.array([127, 128, 2303, 2304])
    rows = []
    for b in range(40):
        kind = b % 5
        if kind == 0:
            rows.append(every)
        elif kind == 1:
            rows.append(np.setdiff1d(every, rng.choice(n, 7, replace=False)))
        elif kind == 2:
            rows.append(np.setdiff1d(every, np.union1d(rng.choice(n, 40, replace=False), edge[:2])))
        elif kind == 3:
            rows.append(np.union1d(edge, rng.choice(n, 300, replace=False)))
        else:
            rows.append(np.concatenate([[-7], np.sort(rng.choice(n, 30, replace=False)), [n, n + 1000]]))
    cert, (v, i), _ = _check(u, items, k, pool, exclude=_sets(rows, n))
    kinds = torch.arange(40, device=DEV) % 5
    assert bool(cert[kinds <= 2].all())                                    # pools that are not full
    assert bool((i[kinds == 0] == -1).all()) and bool((v[kinds == 0] == float("-inf")).all())
    assert bool(((i[kinds == 1] >= 0).sum(1) == 7).all()) and bool(((i[kinds == 2] >= 0).sum(1) == 20).all())
    assert not bool(torch.isin(i[kinds == 3], torch.tensor(edge, device=DEV)).any())


@functools.lru_cache(maxsize=None)
def _cluster_run():
    """256 users, 2 000 items of which 300 are near-identical and on top for every other user; pool = 128, k = 20, no fallback:
    (rank_topk's answer, certified mask, rows whose pool answer differs from it)."""
    eng = _eng()
    u, items = _views(*po.cluster_tables())
    want = eng.rank_topk(u, items, 20)
    v, i, cert = eng.shortlist.rank_topk_certified(u, items, 20, pool=128, fallback=False, return_certified=True)
    differs = ((v.view(torch.int32) != want[0].view(torch.int32)) | (i != want[1])).any(1)
    print("cluster: uncertified", float((~cert).float().mean()), "rows that differ", float(differs.float().mean()))
    return u, items, want, cert, differs


def test_the_cluster_defeats_the_certificate_and_the_fallback_repairs_it():
    """tests/prefilter_oracle.py gives 50 % uncertified and 48 - 50 % differing rows on this table (seeds 5, 6, 7)."""
    eng = _eng()
    u, items, want, cert, differs = _cluster_run()
    assert not bool(differs[cert].any())
    assert float((~cert).float().mean()) >= 0.40
    assert float(differs.float().mean()) >= 0.25                           # the pool's own answer is wrong there: the fallback is needed
    assert _same(eng.shortlist.rank_topk_certified(u, items, 20, pool=128), want)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 2.0 ** 70, 2.0 ** -80])
def test_irregular_values_fall_back_and_stay_exact(bad):
    eng = _eng()
    U, I = po.gaussian_tables(40, 700, 64, 8)  # noqa: E741
    U2 = U.copy()
    U2[5, 9] = bad
    u, items = _views(U2, I)
    cert, _, _ = _check(u, items, 20, 128)
    assert not bool(cert[5]) and bool(cert[torch.arange(40, device=DEV) != 5].all())
    I2 = I.copy()
    I2[333, 0] = bad
    u, items = _views(U, I2)
    cert, _, _ = _check(u, items, 20, 128)
    assert not bool(cert.any())
    assert int(eng.shortlist.pack_items(items).flags.item()) == 1 and int(eng.shortlist.pack_items(_views(U, I)[1]).flags.item()) == 0


@functools.lru_cache(maxsize=None)
def _bound_cases():
    return [po.gaussian_tables(40, 700, D, 20 + D) for D in (33, 64, 130, 260)] + [po.popular_head_tables(40, 700, 64, 5)]


def test_the_measured_error_is_within_the_bound_and_ub_is_an_upper_bound():
    """max |s~ - s_fp64| / (|u| |i|) over the regular tables <= beta (s~ as the kernel computed it), and ub >= rank_topk's score."""
    eng = _eng()
    worst = 0.0
    for U, I in _bound_cases():  # noqa: E741
        u, items = _views(U, I)
        approx, ub = eng.shortlist.shortlist_scores(u, items)
        exact = eng.recommend_topk(u, items, 1, return_scores=True)[2]            # the chain rank_topk is pinned to, bit for bit
        assert bool((ub >= exact).all())
        s64 = U.astype(np.float64) @ I.astype(np.float64).T
        norms = np.linalg.norm(U.astype(np.float64), axis=1)[:, None] * np.linalg.norm(I.astype(np.float64), axis=1)[None, :]
        ratio = float((np.abs(approx.cpu().numpy().astype(np.float64) - s64) / norms).max()) / po.beta(U.shape[1])
        print(f"D={U.shape[1]}: measured error / beta = {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0
        packed = eng.shortlist.pack_items(items)
        assert torch.equal(packed.bf16.float().cpu()[:, :U.shape[1]], torch.from_numpy(po.bf16_rne(I)))
        assert bool((packed.bf16[:, U.shape[1]:] == 0).all()) and packed.bf16.shape[1] % 16 == 0
        assert bool((packed.norm_up.cpu().double() >= torch.from_numpy(np.linalg.norm(I.astype(np.float64), axis=1))).all())
    assert worst <= 1.0


def test_two_runs_give_identical_bits():
    eng = _eng()
    u, items = _views(*po.gaussian_tables(257, 4500, 64, 13))
    runs = [eng.shortlist.rank_topk_certified(u, items, 20, pool=64, fallback=False, return_certified=True) for _ in range(2)]
    assert _same(runs[0], runs[1]) and torch.equal(runs[0][2], runs[1][2])


def test_a_user_id_out_of_range_raises_or_is_flagged():
    eng = _eng()
    u, items = _views(*po.gaussian_tables(5, 300, 16, 1))
    for bad in ([0, 5], [-1]):
        with pytest.raises(IndexError):
            eng.shortlist.rank_topk_certified(u, items, 5, user_ids=torch.tensor(bad, device=DEV))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids = torch.tensor([3, 99, 0], device=DEV)
    v, i, cert = eng.shortlist.rank_topk_certified(u, items, 5, user_ids=ids, status=status, return_certified=True)
    assert int(status.item()) == 1 and not bool(cert[1])
    want = eng.rank_topk(u, items, 5, user_ids=torch.tensor([3, 0], device=DEV))
    assert _same((v[[0, 2]], i[[0, 2]]), want)


def test_full_ranking_with_the_prefilter_returns_the_default_dict():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = _eng()
    u_, i_, w_ = pkg.graphs.synthetic_interactions(2000, 150, 30000, seed=2, device=DEV)
    (tu, ti, tw), (hu, hi, _) = pkg.graphs.holdout_split(u_, i_, w_, 0.2, seed=9)
    num_dict = {"user": 2000, "item": 150, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    coo = pkg.graphs.bipartite_from_interactions(tu, ti, tw, 2000, 150)
    model = pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, [pkg.graphs.to_sparse_coo(coo)], num_dict, 8, DEV).to(DEV)
    train = eng.ItemSets.from_pairs(tu, ti, 2000, 150)
    test = eng.ItemSets.from_pairs(hu, hi, 2000, 150)
    want = pkg.evaluate.full_ranking(model, train, test, ks=(5, 20), user_chunk=700)
    got = pkg.evaluate.full_ranking(model, train, test, ks=(5, 20), user_chunk=700, prefilter="bf16", pool=64)
    assert 0.0 <= got.pop("certified") <= 1.0 and got == want
