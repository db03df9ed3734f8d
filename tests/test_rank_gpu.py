"""Full-catalogue ranking (ngcf_rank_topk_f32) and held-out metrics (ngcf_rank_metrics) on the device."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _eng():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine


def _tables(B, n_items, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    u = torch.randn((B + 2, D + 3), generator=g, device=DEV)[2:, 1:1 + D]             # strided, offset views
    items = torch.randn((n_items + 3, D + 5), generator=g, device=DEV)[3:, 2:2 + D]
    return u, items


def _random_sets(B, n_items, per_user, seed):
    eng = _eng()
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = B * per_user
    users = torch.randint(0, B, (n,), generator=g, device=DEV)
    items = torch.randint(0, n_items, (n,), generator=g, device=DEV)
    return eng.ItemSets.from_pairs(users, items, B, n_items)


def _mask(sets, B, n_items):
    m = torch.zeros((B, n_items), dtype=torch.bool)
    rp, ci = sets.rowptr.cpu(), sets.colidx.cpu().long() - sets.col_offset
    for b in range(B):
        c = ci[rp[b]:rp[b + 1]]
        c = c[(c >= 0) & (c < n_items)]
        m[b, c] = True
    return m


@pytest.mark.parametrize("B,n_items,D,k", [(1, 100, 193, 20), (7, 257, 33, 100), (64, 5000, 65, 100), (300, 20000, 128, 50),
                                           (5840, 100, 193, 20), (9, 3000, 515, 256)])
def test_rank_bit_identical_to_recommend_topk(B, n_items, D, k):
    eng = _eng()
    u, items = _tables(B, n_items, D, B * 7 + D)
    rv, ri, scores = eng.recommend_topk(u, items, k, return_scores=True)
    v, i = eng.rank_topk(u, items, k)
    assert torch.equal(v, rv) and torch.equal(i, ri)
    # with exclusions: the existing kernel's score matrix, excluded entries at -inf, top-k of it over the valid slots
    sets = _random_sets(B, n_items, max(1, n_items // 5), B + k)
    v, i = eng.rank_topk(u, items, k, exclude=sets)
    m = _mask(sets, B, n_items).to(DEV)
    wv, wi = eng.topk_rows(scores.masked_fill(m, float("-inf")), k)
    valid = i >= 0
    assert torch.equal(valid.sum(1).cpu(), torch.clamp((~m).sum(1), max=k).cpu())
    assert torch.equal(v[valid], wv[valid]) and torch.equal(i[valid], wi[valid])
    assert bool((v[~valid] == float("-inf")).all())
    assert not bool(torch.gather(m, 1, i.clamp(min=0))[valid].any())


def _boundary_rows(B, n_items, keep, seed):
    """Exclusion rows that hold items 127, 128, 2175 and 2176 - the two sides of a tile boundary and of the item-split boundary of
    (33, 4224): 33 tiles, 2 splits of 2176 items - and everything else but `keep` random items per user."""
    rng = np.random.default_rng(seed)
    edge = np.array([127, 128, 2175, 2176])
    rows = []
    for _ in range(B):
        stay = np.setdiff1d(rng.permutation(n_items)[:keep], edge)
        rows.append(np.setdiff1d(np.arange(n_items), stay))
    return rows


@pytest.mark.parametrize("k", [128, 129])
def test_rank_every_branch_of_the_tile_walk_at_once(k):
    """B = 33, n_items = 4224, D = 33: one 64-user tile at k = 128, two 32-user tiles at k = 129, the last one partly filled either
    way; two item splits of 2176 items; a second K chunk of one column; exclusion rows across the tile and the split boundary.  4224 is
    33 whole tiles, so n_items = 4223 follows: the same split, and a last tile that the item range cuts short."""
    eng = _eng()
    for n_items in (4224, 4223):
        u, items = _tables(33, n_items, 33, 41)
        rv, ri, scores = eng.recommend_topk(u, items, k, return_scores=True)
        v, i = eng.rank_topk(u, items, k)
        assert torch.equal(v, rv) and torch.equal(i, ri)
        for keep in (n_items - 40, 100):                                  # few exclusions; fewer than k eligible items
            rows = _boundary_rows(33, n_items, keep, 42 + keep)
            rowptr = torch.tensor([0] + np.cumsum([len(r) for r in rows]).tolist(), dtype=torch.int64, device=DEV)
            sets = eng.ItemSets(rowptr, torch.tensor(np.concatenate(rows), dtype=torch.int32, device=DEV), 0, n_items)
            v, i = eng.rank_topk(u, items, k, exclude=sets)
            m = _mask(sets, 33, n_items).to(DEV)
            wv, wi = eng.topk_rows(scores.masked_fill(m, float("-inf")), k)
            valid = i >= 0
            assert torch.equal(valid.sum(1).cpu(), torch.clamp((~m).sum(1), max=k).cpu())
            assert torch.equal(v[valid], wv[valid]) and torch.equal(i[valid], wi[valid])
            assert bool((v[~valid] == float("-inf")).all()) and not bool(torch.gather(m, 1, i.clamp(min=0))[valid].any())


def test_rank_exact_selection_with_ties():
    eng = _eng()
    g = torch.Generator().manual_seed(5)
    B, n_base, D, k = 37, 600, 24, 40
    u = torch.randint(-3, 4, (B, D), generator=g).float()
    base = torch.randint(-3, 4, (n_base, D), generator=g).float()
    items = torch.cat([base, base[torch.randperm(n_base, generator=g)[:900 % n_base]], base[:300]])   # duplicated rows: exact ties
    n_items = items.shape[0]
    users_p = torch.randint(0, B, (B * 50,), generator=g)
    items_p = torch.randint(0, n_items, (B * 50,), generator=g)
    sets = eng.ItemSets.from_pairs(users_p.to(DEV), items_p.to(DEV), B, n_items)
    v, i = eng.rank_topk(u.to(DEV), items.to(DEV), k, exclude=sets)
    s = (u.double() @ items.double().T).numpy()
    m = _mask(sets, B, n_items).numpy()
    for b in range(B):
        ok = np.nonzero(~m[b])[0]
        order = ok[np.lexsort((ok, -s[b, ok]))][:k]
        assert i[b].cpu().numpy().tolist() == order.tolist()
        assert np.array_equal(v[b].cpu().double().numpy(), s[b, order])


def test_rank_exclusion_edges():
    eng = _eng()
    u, items = _tables(4, 300, 40, 3)
    n = 300
    rows = [torch.arange(n), torch.arange(3, n), torch.tensor([5, 5, 5, -7, 400, 299, 299, 1000]), torch.tensor([], dtype=torch.int64)]
    # sorted rows with duplicates and out-of-range ids, written directly (from_pairs would drop them)
    colidx = torch.cat([torch.sort(r).values for r in rows]).to(torch.int32)
    rowptr = torch.tensor([0] + np.cumsum([len(r) for r in rows]).tolist(), dtype=torch.int64)
    sets = eng.ItemSets(rowptr.to(DEV), colidx.to(DEV), 0, n)
    v, i = eng.rank_topk(u, items, 20, exclude=sets)
    assert bool((i[0] == -1).all()) and bool((v[0] == float("-inf")).all())
    assert (i[1] >= 0).sum() == 3 and set(i[1, :3].tolist()) == {0, 1, 2} and bool((i[1, 3:] == -1).all())
    assert not ({5, 299} & set(i[2].tolist())) and bool((i[2] >= 0).all())
    want_v, want_i = eng.rank_topk(u[3:4], items, 20)
    assert torch.equal(i[3:4], want_i) and torch.equal(v[3:4], want_v)
    # offset: ids shifted by 1000 mean the same items
    sets2 = eng.ItemSets(rowptr.to(DEV), (colidx + 1000).to(DEV), 1000, n)
    v2, i2 = eng.rank_topk(u, items, 20, exclude=sets2)
    assert torch.equal(v2, v) and torch.equal(i2, i)


def _model(coo, n_user, n_item):
    import seoul_tourism_recommendation_ngcf_amd as pkg
    num_dict = {"user": n_user, "item": n_item, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    return pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, [pkg.graphs.to_sparse_coo(coo)], num_dict, 8, DEV).to(DEV)


def test_rank_from_laplacian_equals_from_pairs():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = _eng()
    u_, i_, w_ = pkg.graphs.synthetic_interactions(2000, 150, 30000, seed=4, device=DEV)
    model = _model(pkg.graphs.bipartite_from_interactions(u_, i_, w_, 2000, 150), 2000, 150).eval()
    with torch.no_grad():
        model.propagate(0)
    a = eng.ItemSets.from_laplacian(model.laplacian_csr(0), 2000)
    b = eng.ItemSets.from_pairs(u_, i_, 2000, 150)
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.colidx.long() - a.col_offset, b.colidx.long())
    r1 = eng.rank_topk(model.all_users_emb, model.all_items_emb, 20, exclude=a)
    r2 = eng.rank_topk(model.all_users_emb, model.all_items_emb, 20, exclude=b)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


def test_rank_split_and_batch_independence():
    eng = _eng()
    u, items = _tables(4096, 100_000, 64, 11)
    sets = _random_sets(4096, 100_000, 30, 12)
    v, i = eng.rank_topk(u, items, 100, exclude=sets)
    for rows in ([17], [0, 2049, 4095]):
        ids = torch.tensor(rows, device=DEV)
        v1, i1 = eng.rank_topk(u, items, 100, user_ids=ids, exclude=sets)          # B = 1 / 3: the item-split path
        assert torch.equal(v1, v[ids]) and torch.equal(i1, i[ids])
    perm = torch.randperm(4096, device=DEV)[:1000]
    v2, i2 = eng.rank_topk(u, items, 100, user_ids=perm, exclude=sets)
    assert torch.equal(v2, v[perm]) and torch.equal(i2, i[perm])
    v3, i3 = eng.rank_topk(u[perm], items, 100)                                      # pre-gathered rows, no exclusion
    v4, i4 = eng.rank_topk(u, items, 100, user_ids=perm)
    assert torch.equal(v3, v4) and torch.equal(i3, i4)
    v5, i5 = eng.rank_topk(u, items, 100, exclude=sets)
    assert torch.equal(v5, v) and torch.equal(i5, i)


def _np_metrics(top, truth_rows, ks):
    out = np.zeros(4 * len(ks) + 1)
    for b, T in enumerate(truth_rows):
        T = set(int(t) for t in T if t >= 0)
        if not T:
            continue
        out[-1] += 1
        for q, K in enumerate(ks):
            L = [int(x) for x in top[b, :K]]
            hit = [j for j, x in enumerate(L) if x >= 0 and x in T]
            dcg = sum(1 / math.log2(j + 2) for j in hit)
            idcg = sum(1 / math.log2(j + 2) for j in range(min(K, len(T))))
            out[4 * q:4 * q + 4] += [len(hit) / len(T), dcg / idcg, len(hit) / K, float(len(hit) > 0)]
    return out


def test_ranking_metrics_vs_numpy():
    eng = _eng()
    rng = np.random.default_rng(3)
    B, n_items, k, ks = 3000, 60, 30, [1, 5, 20, 30]
    top = np.stack([rng.permutation(n_items)[:k] for _ in range(B)])
    top[rng.random((B, k)) < 0.1] = -1
    truth_rows = []
    for b in range(B):
        n = [0, 1, 3, 40][b % 4]
        truth_rows.append(np.sort(np.concatenate([rng.choice(n_items, n, replace=False), rng.choice(n_items, n // 3)])).astype(np.int64))
    rowptr = torch.tensor([0] + np.cumsum([len(t) for t in truth_rows]).tolist(), dtype=torch.int64, device=DEV)
    colidx = torch.tensor(np.concatenate(truth_rows), dtype=torch.int32, device=DEV)
    truth = eng.ItemSets(rowptr, colidx, 0, n_items)
    top_t = torch.tensor(top, device=DEV)
    got = eng.ranking_metrics(top_t, truth, ks)
    want = _np_metrics(top, truth_rows, ks)
    assert got["users"] == int(want[-1])
    for q, K in enumerate(ks):
        for j, name in enumerate(("recall", "ndcg", "precision", "hr")):
            assert got[f"{name}@{K}"] == pytest.approx(want[4 * q + j] / want[-1], rel=1e-12, abs=1e-15)
    s1 = torch.zeros(4 * len(ks) + 1, dtype=torch.float64, device=DEV)
    s2 = torch.zeros_like(s1)
    eng.ranking_metrics(top_t, truth, ks, sums=s1)
    eng.ranking_metrics(top_t, truth, ks, sums=s2)
    assert torch.equal(s1, s2)
    s3 = torch.zeros_like(s1)
    ids = torch.arange(B, device=DEV)
    for c in range(4):
        sl = slice(c * 750, (c + 1) * 750)
        eng.ranking_metrics(top_t[sl], truth, ks, user_ids=ids[sl], sums=s3)
    torch.testing.assert_close(s3, s1, rtol=1e-12, atol=0)


def test_full_ranking_end_to_end():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = _eng()
    u_, i_, w_ = pkg.graphs.synthetic_interactions(2000, 150, 30000, seed=2, device=DEV)
    (tu, ti, tw), (hu, hi, _) = pkg.graphs.holdout_split(u_, i_, w_, 0.2, seed=9)
    model = _model(pkg.graphs.bipartite_from_interactions(tu, ti, tw, 2000, 150), 2000, 150)
    model.train()
    train = eng.ItemSets.from_pairs(tu, ti, 2000, 150)
    test = eng.ItemSets.from_pairs(hu, hi, 2000, 150)
    got = pkg.evaluate.full_ranking(model, train, test, ks=(20,))
    assert model.training
    got_lap = pkg.evaluate.full_ranking(model, eng.ItemSets.from_laplacian(model.laplacian_csr(0), 2000), (hu, hi), ks=(20,))
    assert got_lap == got
    with torch.no_grad():
        model.eval()
        model.propagate(0)
        U, I = model.all_users_emb.cpu(), model.all_items_emb.cpu()
        model.train()
    s = torch.mm(U, I.T)
    s[_mask(train, 2000, 150)] = float("-inf")
    sv, si = torch.topk(s, 21)
    clear = ((sv[:, 19] - sv[:, 20]) > 1e-4).nonzero().flatten().to(DEV)
    assert clear.numel() > 1000
    want = eng.ranking_metrics(si[:, :20].to(DEV)[clear], test, [20], user_ids=clear)
    _, top = eng.rank_topk(model.all_users_emb, model.all_items_emb, 20, user_ids=clear, exclude=train)
    sub = eng.ranking_metrics(top, test, [20], user_ids=clear)
    assert sub["users"] == want["users"]
    for name in ("recall@20", "precision@20", "hr@20"):          # set-based: exact on users with a clear k-th score
        assert sub[name] == pytest.approx(want[name], rel=1e-12)
    assert sub["ndcg@20"] == pytest.approx(want["ndcg@20"], rel=1e-3)   # near-ties inside the list may swap ranks
    _, top_all = eng.rank_topk(model.all_users_emb, model.all_items_emb, 20, exclude=train)
    assert eng.ranking_metrics(top_all, test, [20]) == got
    assert got["users"] == int((test.rowptr.diff() > 0).sum())
    assert 0.0 <= got["recall@20"] <= 1.0 and 0.0 <= got["ndcg@20"] <= 1.0


def test_rank_medium_scale_vs_fp64():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = _eng()
    n_user, n_item, D, k = 100_000, 20_000, 512, 20
    g = torch.Generator(device=DEV).manual_seed(21)
    U = torch.randn((n_user, D), generator=g, device=DEV) * 0.1
    I = torch.randn((n_item, D), generator=g, device=DEV) * 0.1
    u_, i_, _ = pkg.graphs.synthetic_interactions(n_user, n_item, 2_000_000, seed=22, device=DEV)
    sets = eng.ItemSets.from_pairs(u_, i_, n_user, n_item)
    v, i = eng.rank_topk(U, I, k, exclude=sets)
    pick = torch.randperm(n_user, generator=torch.Generator().manual_seed(1))[:256]
    s = U[pick.to(DEV)].cpu().double() @ I.cpu().double().T
    rp, ci = sets.rowptr.cpu(), sets.colidx.cpu().long()
    for r, b in enumerate(pick.tolist()):
        s[r, ci[rp[b]:rp[b + 1]]] = float("-inf")
    sv, si = torch.topk(s, k + 1)
    got_v, got_i = v[pick.to(DEV)].cpu(), i[pick.to(DEV)].cpu()
    torch.testing.assert_close(got_v.double(), sv[:, :k], atol=1e-4, rtol=0)
    clear = (sv[:, k - 1] - sv[:, k]) > 1e-4
    assert int(clear.sum()) > 128
    for r in clear.nonzero().flatten().tolist():
        assert set(got_i[r].tolist()) == set(si[r, :k].tolist())


def test_rank_errors():
    eng = _eng()
    u, items = _tables(5, 300, 16, 1)
    for bad_k in (0, 301):
        with pytest.raises(RuntimeError, match="out of range"):
            eng.rank_topk(u, items, bad_k)
    with pytest.raises(RuntimeError, match="recommend_topk"):
        eng.rank_topk(u, items, 257)
    with pytest.raises(RuntimeError, match="cannot be multiplied"):
        eng.rank_topk(u, items[:, :15], 1)
    with pytest.raises(IndexError):
        eng.rank_topk(u, items, 5, user_ids=torch.tensor([0, 5], device=DEV))
    with pytest.raises(IndexError):
        eng.rank_topk(u, items, 5, user_ids=torch.tensor([-1], device=DEV))
    # unsorted columns in a CSR's user rows are refused by ItemSets.from_laplacian
    rowptr = torch.tensor([0, 2, 4, 4, 4], dtype=torch.int64, device=DEV)
    colidx = torch.tensor([3, 2, 2, 3], dtype=torch.int32, device=DEV)
    csr = eng.LaplacianCSR.from_csr_arrays(rowptr, colidx, torch.ones(4, device=DEV), 4)
    with pytest.raises(RuntimeError, match="not ascending"):
        eng.ItemSets.from_laplacian(csr, 2)
