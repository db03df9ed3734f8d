"""Exact held-out positions (ngcf_rank_positions_f32) and the metrics from them (ngcf_rank_position_metrics) on the device, against
the numpy oracle run on the score matrix of `recommend_topk` (whose bits an existing test pins to `rank_topk`'s) and against
`rank_topk` / `ranking_metrics` themselves."""
import numpy as np
import pytest
import torch

import rank_position_oracle as orc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CAP = 64


def _eng():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine


def _tables(B, n_items, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    u = torch.randn((B + 2, D + 3), generator=g, device=DEV)[2:, 1:1 + D]             # strided, offset views
    items = torch.randn((n_items + 3, D + 5), generator=g, device=DEV)[3:, 2:2 + D]
    return u, items


def _sets_of(rows, n_items, offset=0):
    rowptr = torch.tensor([0] + np.cumsum([len(r) for r in rows]).tolist(), dtype=torch.int64, device=DEV)
    flat = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, dtype=np.int64)]) + offset
    return _eng().ItemSets(rowptr, torch.tensor(flat, dtype=torch.int32, device=DEV), offset, n_items)


def _random_rows(B, n_items, seed, max_excl=40, max_truth=30, lengths=None):
    """Per user an exclusion row of 0..max_excl items and a disjoint truth row of 0..max_truth (or lengths[b]) items, ascending."""
    rng = np.random.default_rng(seed)
    excl, truth = [], []
    for b in range(B):
        perm = rng.permutation(n_items)
        n_x = int(rng.integers(0, min(max_excl, n_items // 3) + 1))
        n_t = int(rng.integers(0, min(max_truth, n_items // 3) + 1)) if lengths is None else lengths[b]
        excl.append(np.sort(perm[:n_x]))
        truth.append(np.sort(perm[n_x:n_x + n_t]))
    return excl, truth


def _split(flat, rows):
    cuts = np.cumsum([len(r) for r in rows])[:-1]
    return np.split(flat.cpu().numpy().astype(np.int64), cuts)


def _check_against_oracle(u, items, excl, truth, check_topk=True):
    eng = _eng()
    B, n_items = int(u.shape[0]), int(items.shape[0])
    k = min(256, n_items)
    excl_s, truth_s = _sets_of(excl, n_items), _sets_of(truth, n_items)
    _, _, scores = eng.recommend_topk(u, items, k, return_scores=True)
    pos = eng.ranks.rank_positions(u, items, truth_s, exclude=excl_s)
    assert pos.dtype == torch.int32 and pos.shape == (sum(len(t) for t in truth),)
    got = _split(pos, truth)
    want = orc.positions(scores.cpu().numpy(), truth, excl)
    for b in range(B):
        assert got[b].tolist() == want[b].tolist(), f"user {b}"
    if check_topk:
        top = eng.rank_topk(u, items, k, exclude=excl_s)[1].cpu().numpy()
        for b in range(B):
            for t, p in zip(truth[b].tolist(), got[b].tolist()):
                if 0 <= p < k:
                    assert top[b, p] == t
                else:
                    assert t not in top[b]
    return pos


@pytest.mark.parametrize("B,n_items,D", [(1, 100, 193), (7, 257, 33), (64, 5000, 65), (300, 20000, 128)])
def test_positions_exact_against_recommend_topk_and_rank_topk(B, n_items, D):
    u, items = _tables(B, n_items, D, 3 * B + D)
    excl, truth = _random_rows(B, n_items, B + D)
    _check_against_oracle(u, items, excl, truth)


def test_positions_with_ties_and_special_values():
    g = torch.Generator().manual_seed(5)
    B, n_base, D = 37, 300, 24
    u = torch.randint(-3, 4, (B, D), generator=g).float()
    base = torch.randint(-3, 4, (n_base, D), generator=g).float()
    special = torch.stack([torch.full((D,), float("nan")), torch.full((D,), float("inf")), torch.full((D,), -0.0)])
    items = torch.cat([base, base[torch.randperm(n_base, generator=g)[:200]], special, base[:100]])   # duplicated rows: exact ties
    n_items = int(items.shape[0])
    rng = np.random.default_rng(6)
    excl, truth = [], []
    for b in range(B):
        # targets and exclusions drawn from the duplicated rows and the special ones: they tie with each other and with ordinary items
        pool = rng.permutation(np.concatenate([np.arange(0, 100), np.arange(n_base, n_base + 203), np.arange(n_base + 203, n_items)]))
        truth.append(np.sort(np.unique(np.concatenate([pool[:12], [n_base + 200, n_base + 201, n_base + 202][:b % 4]]))))
        excl.append(np.sort(np.setdiff1d(pool[12:40], truth[-1])))
    _check_against_oracle(u.to(DEV), items.to(DEV), excl, truth)


def test_positions_at_the_tier_boundaries():
    lengths = [1, 0, CAP - 1, CAP, 0, 0, CAP + 1, 2 * CAP + 3, 0, CAP, 1]
    n_items = 2 * CAP + 40
    u, items = _tables(len(lengths), n_items, 20, 8)
    rng = np.random.default_rng(9)
    truth = [np.sort(rng.permutation(n_items)[:n]) for n in lengths]
    excl = [np.sort(np.setdiff1d(rng.permutation(n_items)[:10], t)) for t in truth]
    _check_against_oracle(u, items, excl, truth)


@pytest.mark.parametrize("B,n_items,D", [(1, 127, 1), (31, 128, 31), (32, 129, 32), (33, 300, 33)])
def test_positions_at_the_tile_boundaries(B, n_items, D):
    u, items = _tables(B, n_items, D, 5 * B + D)
    excl, truth = _random_rows(B, n_items, 2 * B + D)
    _check_against_oracle(u, items, excl, truth)


@pytest.mark.parametrize("n_items", [4224, 4223])
def test_positions_every_branch_of_the_tile_walk_at_once(n_items):
    """B = 33, D = 33, 33 item tiles in two splits of 2176 (the last tile cut short at 4223): a partly filled row tile, a second K
    chunk of one column, and exclusion rows that hold 127, 128, 2175, 2176 - both sides of a tile boundary and of the split boundary -
    while their neighbours 126, 129, 2174, 2177 are held out.  First against the oracle and rank_topk's top 256, then, with fewer
    than 256 eligible items per user, against the positions read off rank_topk's full order."""
    eng = _eng()
    B, D = 33, 33
    u, items = _tables(B, n_items, D, 41)
    rng = np.random.default_rng(43)
    edge, near = np.array([127, 128, 2175, 2176]), np.array([126, 129, 2174, 2177])
    rest = np.setdiff1d(np.arange(n_items), np.concatenate([edge, near]))
    pools = [rng.permutation(rest) for _ in range(B)]
    _check_against_oracle(u, items, [np.sort(np.concatenate([edge, p[:20]])) for p in pools],
                          [np.sort(np.concatenate([near, p[20:40]])) for p in pools])
    truth = [np.sort(np.concatenate([near, p[:30]])) for p in pools]
    excl = [np.setdiff1d(np.arange(n_items), np.concatenate([near, p[:240]])) for p in pools]
    excl_s, truth_s = _sets_of(excl, n_items), _sets_of(truth, n_items)
    top = eng.rank_topk(u, items, 256, exclude=excl_s)[1]
    assert bool(((top >= 0).sum(1) == 244).all())                              # every eligible item, in order
    found = [top[b][:, None] == torch.tensor(truth[b], device=DEV)[None, :] for b in range(B)]
    assert all(bool(f.any(0).all()) for f in found)
    want = torch.cat([f.int().argmax(0) for f in found]).int()
    assert torch.equal(eng.ranks.rank_positions(u, items, truth_s, exclude=excl_s), want)


def test_positions_do_not_depend_on_batch_chunks_strides_or_runs():
    eng = _eng()
    B, n_items, D = 300, 20000, 64
    u, items = _tables(B, n_items, D, 17)
    excl, truth = _random_rows(B, n_items, 18)
    excl_s, truth_s = _sets_of(excl, n_items), _sets_of(truth, n_items)
    full = eng.ranks.rank_positions(u, items, truth_s, exclude=excl_s)
    assert int(full.min()) >= 0
    assert torch.equal(eng.ranks.rank_positions(u, items, truth_s, exclude=excl_s), full)            # run to run
    rp = truth_s.rowptr.cpu().tolist()
    row = max(range(B), key=lambda b: rp[b + 1] - rp[b])
    alone = eng.ranks.rank_positions(u, items, truth_s, user_ids=torch.tensor([row], device=DEV), exclude=excl_s)   # item range split
    want = torch.full_like(full, eng.ranks.NOT_RANKED)
    want[rp[row]:rp[row + 1]] = full[rp[row]:rp[row + 1]]
    assert torch.equal(alone, want)
    buf = torch.full_like(full, eng.ranks.NOT_RANKED)
    ids = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(DEV)
    for lo, hi in ((0, 100), (100, 250), (250, 300)):
        assert eng.ranks.rank_positions(u, items, truth_s, user_ids=ids[lo:hi], exclude=excl_s, out=buf) is buf
    assert torch.equal(buf, full)
    twice = eng.ranks.rank_positions(u, items, truth_s, user_ids=torch.tensor([row, 3, row], device=DEV), exclude=excl_s)
    assert torch.equal(twice[rp[row]:rp[row + 1]], full[rp[row]:rp[row + 1]])
    assert torch.equal(eng.ranks.rank_positions(u.contiguous(), items.contiguous(), truth_s, exclude=excl_s), full)   # ld == D
    assert torch.equal(eng.ranks.rank_positions(u, items, truth_s, exclude=_sets_of(excl, n_items, offset=B)), full)  # column offset


def _model(coo, n_user, n_item):
    import seoul_tourism_recommendation_ngcf_amd as pkg
    num_dict = {"user": n_user, "item": n_item, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    return pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, [pkg.graphs.to_sparse_coo(coo)], num_dict, 8, DEV).to(DEV)


def test_positions_from_laplacian_exclusions_equal_from_pairs():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = _eng()
    u_, i_, w_ = pkg.graphs.synthetic_interactions(2000, 150, 30000, seed=4, device=DEV)
    (tu, ti, tw), (hu, hi, _) = pkg.graphs.holdout_split(u_, i_, w_, 0.2, seed=5)
    model = _model(pkg.graphs.bipartite_from_interactions(tu, ti, tw, 2000, 150), 2000, 150).eval()
    with torch.no_grad():
        model.propagate(0)
    a = eng.ItemSets.from_laplacian(model.laplacian_csr(0), 2000)
    b = eng.ItemSets.from_pairs(tu, ti, 2000, 150)
    truth = eng.ItemSets.from_pairs(hu, hi, 2000, 150)
    pa = eng.ranks.rank_positions(model.all_users_emb, model.all_items_emb, truth, exclude=a)
    pb = eng.ranks.rank_positions(model.all_users_emb, model.all_items_emb, truth, exclude=b)
    assert a.col_offset == 2000 and torch.equal(pa, pb) and int(pa.min()) >= 0


def test_position_flags():
    eng = _eng()
    n = 300
    u, items = _tables(5, n, 16, 1)
    truth_rows = [[3, 7], [5, 5, 9], [-7, 8, 299, 1000], [], [1, 2]]
    excl_rows = [[], [9, 20], [], [4], [0]]
    truth, excl = _sets_of(truth_rows, n), _sets_of(excl_rows, n)
    for bad in ([0, 5], [-1]):
        with pytest.raises(IndexError, match="user id"):
            eng.ranks.rank_positions(u, items, truth, user_ids=torch.tensor(bad, device=DEV), exclude=excl)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    pos = eng.ranks.rank_positions(u, items, truth, user_ids=torch.tensor([1, 7, 4], device=DEV), exclude=excl, status=status)
    assert int(status.item()) == 1                                            # only flagged
    p = pos.cpu().tolist()
    assert p[0:2] == [-2, -2] and p[5:9] == [-2] * 4                          # users outside the batch keep "not ranked"
    assert p[2] == p[3] and p[2] >= 0 and p[4] == -1                          # duplicate ids: equal; 9 is excluded: -1
    assert min(p[9:11]) >= 0
    with pytest.raises(IndexError, match="held-out id"):
        eng.ranks.rank_positions(u, items, truth, exclude=excl)
    status.zero_()
    pos = eng.ranks.rank_positions(u, items, truth, exclude=excl, status=status)
    assert int(status.item()) == 2
    p = pos.cpu().tolist()
    assert p[5] == -1 and p[8] == -1 and p[6] >= 0 and p[7] >= 0
    scores = eng.recommend_topk(u, items, 10, return_scores=True)[2].cpu().numpy()
    want = orc.positions(scores, [np.asarray(r, dtype=np.int64) for r in truth_rows], excl_rows)
    assert p == [int(x) for r in want for x in r]


_CASE = {}


def _metrics_case():
    """One ranking and one metrics launch, shared by the tests below and left unchanged by them."""
    if _CASE:
        return _CASE
    eng = _eng()
    B, n_items, D = 300, 400, 32
    u, items = _tables(B, n_items, D, 23)
    excl, truth = _random_rows(B, n_items, 24)
    truth[5] = np.array([3, 77])
    excl[5] = np.setdiff1d(np.arange(n_items), truth[5])                       # E == T: no negatives, no AUC
    for b in (11, 12, 13):                                                     # held-out items inside the exclusion row: -1
        both = np.array([b + 100, b + 200])
        excl[b], truth[b] = np.union1d(excl[b], both), np.union1d(truth[b], both)
    truth[20] = np.sort(np.random.default_rng(2).permutation(n_items)[:2 * CAP + 9])   # a row past the register tier
    excl[20] = np.setdiff1d(excl[20], truth[20])
    excl_s, truth_s = _sets_of(excl, n_items), _sets_of(truth, n_items)
    pos = eng.ranks.rank_positions(u, items, truth_s, exclude=excl_s)
    rows = _split(pos, truth)
    assert any(-1 in r.tolist() for r in rows)
    ks = (1, 5, 20, 256, n_items)
    got, per_user = eng.ranks.position_metrics(pos, truth_s, ks, n_items, exclude=excl_s, per_user=True)
    want_pu, want_sums = orc.metrics(rows, truth, [len(x) for x in excl], n_items, ks)
    _CASE.update(eng=eng, u=u, items=items, excl=excl, truth=truth, excl_s=excl_s, truth_s=truth_s, pos=pos, rows=rows, ks=ks, got=got,
                 per_user=per_user, want_pu=want_pu, want_sums=want_sums, B=B, n_items=n_items)
    return _CASE


def test_position_metrics_per_user_within_one_ulp_of_the_oracle():
    """The kernel and the oracle add the same terms in the same order, and every operation but log2 is exactly rounded.  The kernel
    takes log2 from csrc/dd_log2.h (correctly rounded; tests/test_dd_log2.py), not from the device's maths library, whose fp64 log2
    differs from numpy's by 1 ulp at 129 of the integers 2..100001, the first of them 3 - with it the ndcg columns were 2 ulp off."""
    c = _metrics_case()
    pu, want_pu = c["per_user"].cpu().numpy(), c["want_pu"]
    ulps = np.abs(pu - want_pu) / np.spacing(np.maximum(np.abs(want_pu), np.finfo(np.float64).tiny))
    print("per-user max ulp distance per column:", ulps.max(0).tolist())
    assert float(ulps.max()) <= 1.0


def test_position_metrics_means_and_ranking_metrics_bits():
    c = _metrics_case()
    eng, u, items, truth, excl_s, truth_s, pos, rows, ks = (c[k] for k in ("eng", "u", "items", "truth", "excl_s", "truth_s", "pos", "rows", "ks"))
    got, per_user, want_sums, B, n_items = c["got"], c["per_user"], c["want_sums"], c["B"], c["n_items"]
    pu = per_user.cpu().numpy()
    exact = [j for j in range(pu.shape[1]) if j not in (2, 5, 9, 13, 17, 21)]                 # every column without a log2
    assert np.array_equal(pu[:, exact], c["want_pu"][:, exact])
    n, n_auc = int(want_sums[-2]), int(want_sums[-1])
    assert got["users"] == n and got["auc_users"] == n_auc and n - n_auc == 1          # the user with E == T
    names = ["mrr", "map", "ndcg", "auc"] + [f"{m}@{K}" for K in ks for m in ("recall", "ndcg", "precision", "hr")]
    for j, name in enumerate(names):
        want = want_sums[j] / (n_auc if name == "auc" else n)
        err = abs(got[name] - want) / abs(want) if want else abs(got[name])
        print(name, got[name], want, err)
        assert err <= B * 2.0 ** -53
    # @K for K <= 256: rank_metrics' values bit for bit
    top = eng.rank_topk(u, items, 256, exclude=excl_s)[1]
    _, ref = eng.ranking_metrics(top, truth_s, ks[:4], per_user=True)
    assert torch.equal(per_user[:, 4:20].float(), ref)
    # K = n_items: every user without a miss has all its held-out items inside
    recall_all = pu[:, 4 + 4 * 4]
    for b in range(B):
        if len(truth[b]) and -1 not in rows[b].tolist():
            assert recall_all[b] == 1.0
    # chunks into one slot vector, and run to run
    sums = torch.zeros(4 + 4 * len(ks) + 2, dtype=torch.float64, device=DEV)
    ids = torch.arange(B, device=DEV)
    for lo, hi in ((0, 70), (70, 300)):
        assert eng.ranks.position_metrics(pos, truth_s, ks, n_items, exclude=excl_s, user_ids=ids[lo:hi], sums=sums) is sums
    once = eng.ranks.position_metrics(pos, truth_s, ks, n_items, exclude=excl_s, sums=torch.zeros_like(sums))
    again = eng.ranks.position_metrics(pos, truth_s, ks, n_items, exclude=excl_s, sums=torch.zeros_like(sums))
    assert torch.equal(once, again)
    torch.testing.assert_close(sums, once, rtol=1e-12, atol=0)
    with pytest.raises(IndexError, match="user id"):
        eng.ranks.position_metrics(pos, truth_s, ks, n_items, user_ids=torch.tensor([B], device=DEV))


def test_full_ranks_end_to_end():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = _eng()
    u_, i_, w_ = pkg.graphs.synthetic_interactions(2000, 150, 30000, seed=2, device=DEV)
    (tu, ti, tw), (hu, hi, _) = pkg.graphs.holdout_split(u_, i_, w_, 0.2, seed=9)
    model = _model(pkg.graphs.bipartite_from_interactions(tu, ti, tw, 2000, 150), 2000, 150)
    model.train()
    train = eng.ItemSets.from_pairs(tu, ti, 2000, 150)
    test = eng.ItemSets.from_pairs(hu, hi, 2000, 150)
    ref = pkg.evaluate.full_ranking(model, train, test, ks=(5, 20))
    got, pos, truth = pkg.evaluate.full_ranks(model, train, (hu, hi), ks=(5, 20), user_chunk=700, return_positions=True)
    assert model.training
    assert set(got) == {"mrr", "map", "auc", "ndcg", "users", "auc_users"} | {f"{m}@{K}" for K in (5, 20) for m in ("recall", "ndcg", "precision", "hr")}
    for name, want in ref.items():
        assert got[name] == pytest.approx(want, rel=1e-12, abs=1e-15), name
    assert pkg.evaluate.full_ranks(model, train, test, ks=(5, 20)) == pytest.approx(got, rel=1e-12)
    assert 0.0 < got["mrr"] <= 1.0 and 0.0 < got["auc"] <= 1.0 and got["auc_users"] == got["users"]
    with torch.no_grad():
        model.eval()
        model.propagate(0)
        direct = eng.ranks.rank_positions(model.all_users_emb, model.all_items_emb, test, exclude=train)
        model.train()
    assert torch.equal(truth.colidx, test.colidx) and torch.equal(pos, direct)
    some = torch.tensor([5, 1999, 42], device=DEV)
    sub, pos_sub, _ = pkg.evaluate.full_ranks(model, train, test, ks=(5,), users=some, return_positions=True)
    rp = test.rowptr.cpu().tolist()
    ranked = torch.zeros_like(pos, dtype=torch.bool)
    for r in some.tolist():
        ranked[rp[r]:rp[r + 1]] = True
    assert torch.equal(pos_sub[ranked], pos[ranked]) and bool((pos_sub[~ranked] == -2).all())
    assert sub["users"] == sum(1 for r in some.tolist() if rp[r + 1] > rp[r])
