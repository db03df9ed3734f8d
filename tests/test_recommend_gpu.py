"""recommend.blended_ranking end to end on the Seoul-shaped graph against the numpy statement of demo.py in blend_oracle.py."""
import functools

import numpy as np
import pytest
import torch

import blend_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N_USER, N_ITEM, TOP, POINTS = 5840, 100, 10, 100
WEIGHTS = (0.5, 0.3, 0.2)


def _pkg():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg


def _model():
    pkg = _pkg()
    laps = [pkg.graphs.to_sparse_coo(s) for s in pkg.graphs.seoul_standin(DEV)]
    num_dict = {"user": N_USER, "item": N_ITEM, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(1801)
    return pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, laps, num_dict, 25, DEV).to(DEV)


@functools.lru_cache(maxsize=None)
def _case():
    """Two parties: 2 members x 3 days (on day 2 both have the same age and sex, hence one id for two rows), and 1 member x 2 days
    plus a member of the first party's id on a fourth day - columns of 1, 2 and 3 rows coexist.  Read only."""
    uid = torch.tensor([40, 17, 23, 23, 5, 31, 4000, 4001, 40])
    age = torch.tensor([25, 35, 30, 30, 25, 35, 45, 45, 25])
    sex = torch.tensor([0, 1, 1, 1, 0, 1, 0, 0, 0])
    month = torch.tensor([7, 7, 7, 7, 8, 8, 7, 7, 8])
    day = torch.tensor([30, 30, 31, 31, 1, 1, 30, 31, 1])
    dow = torch.tensor([2, 2, 3, 3, 4, 4, 2, 3, 4])
    day_slot = torch.tensor([0, 0, 1, 1, 2, 2, 0, 1, 2])
    g = torch.Generator().manual_seed(7)
    congestion, distance = torch.rand((3, N_ITEM), generator=g), torch.rand((1, N_ITEM), generator=g) * 20000
    for t in (congestion, distance):                               # a condition on the inputs: no ties inside a slot
        assert all(len(set(row.tolist())) == N_ITEM for row in t)
    mask = torch.rand(N_ITEM, generator=g) < 0.5
    assert 30 < int(mask.sum()) < 70
    feats = (age, sex, month, day, dow)
    model = _model()
    model.train()
    pkg = _pkg()
    kw = dict(features=feats, year=[0], weights=WEIGHTS, congestion=congestion.to(DEV), congestion_slot=day_slot.to(DEV),
              distance=distance.to(DEV), distance_slot=torch.zeros(9, dtype=torch.int64), item_mask=mask.to(DEV), top=TOP,
              points=POINTS, return_table=True)
    by_user = pkg.recommend.blended_ranking(model, uid.to(DEV), **kw)
    assert model.training                                          # the caller's mode is restored
    rowptr, rows, labels = pkg.recommend.demo_views(uid, age, sex, month, day)
    views = pkg.recommend.blended_ranking(model, uid, columns=(rowptr, rows), row_chunk=4, **kw)
    assert model.training
    # the oracle's inputs: the score matrix of those tables (its bits are specified to equal rank_topk's), sorted by numpy
    model.eval()
    with torch.no_grad():
        model.propagate(0)
        U, I = model.all_users_emb, model.all_items_emb
        _, _, scores = pkg.engine.recommend_topk(U[uid.to(DEV)].contiguous(), I, POINTS, return_scores=True)
        want64 = U[uid.to(DEV)].cpu().double() @ I.cpu().double().T
    return dict(model=model, uid=uid, by_user=by_user, views=views, rowptr=rowptr.numpy(), rows=rows.numpy(), labels=labels,
                scores=scores.cpu(), want64=want64, congestion=congestion.numpy(), distance=distance.numpy(),
                day_slot=day_slot.numpy(), mask=mask.numpy(), kw=kw)


def _oracle(c, rowptr, rows):
    pref = oracle.lists_desc(c["scores"].numpy(), POINTS)
    con, dis = oracle.lists_asc(c["congestion"], POINTS), oracle.lists_asc(c["distance"], POINTS)
    pts = oracle.point_sums(pref, con, c["day_slot"], dis, np.zeros(9, dtype=np.int64), rowptr, rows, N_ITEM, POINTS)
    assert (pts.sum(2)[:, np.diff(rowptr) > 0] > 0).all()
    return oracle.blend(pts, WEIGHTS, c["mask"], TOP)


def _same(got, want):
    table, items, rating = want
    for g, w in ((got[0], items), (got[1], rating), (got[-1], table)):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.int64), w.view(np.int64))


def test_score_matrix_of_the_oracle_matches_fp64():
    c = _case()
    torch.testing.assert_close(c["scores"].double(), c["want64"], atol=1e-5, rtol=1e-5)    # tests/test_topk_gpu.py at this width (193)


def test_one_column_per_user_id_equals_the_oracle():
    c = _case()
    items, rating, ids, table = c["by_user"]
    assert ids.tolist() == sorted(set(c["uid"].tolist())) == [5, 17, 23, 31, 40, 4000, 4001]
    number = np.searchsorted(np.array(ids.tolist()), c["uid"].numpy())
    cols = [np.nonzero(number == g)[0] for g in range(len(ids))]
    assert sorted(len(x) for x in cols) == [1, 1, 1, 1, 1, 2, 2]
    rowptr = np.concatenate(([0], np.cumsum([len(x) for x in cols])))
    _same(c["by_user"], _oracle(c, rowptr, np.concatenate(cols)))
    assert items.shape == (7, TOP) and bool((items >= 0).all()) and bool(torch.from_numpy(c["mask"])[items.cpu()].all())


def test_the_four_views_equal_the_oracle():
    c = _case()
    assert len(c["views"]) == 3 and len(c["labels"]) == 7 + 3 + 4 + 1
    assert sorted(set(np.diff(c["rowptr"]).tolist())) == [1, 2, 3, 9]
    _same(c["views"], _oracle(c, c["rowptr"], c["rows"]))
    # the per-user columns of the views are the default's columns
    assert torch.equal(c["views"][0][:7], c["by_user"][0]) and torch.equal(c["views"][1][:7], c["by_user"][1])


def test_column_numbers_and_a_bad_user_id():
    c = _case()
    pkg, model = _pkg(), c["model"]
    kw = {k: v for k, v in c["kw"].items() if k != "return_table"}
    ids = c["by_user"][2]
    number = torch.searchsorted(ids.cpu(), c["uid"])
    model.eval()
    items, rating = pkg.recommend.blended_ranking(model, c["uid"], columns=number, **kw)
    assert not model.training
    assert torch.equal(items, c["by_user"][0]) and torch.equal(rating, c["by_user"][1])
    bad = c["uid"].clone()
    bad[4] = N_USER
    with pytest.raises(IndexError):
        pkg.recommend.blended_ranking(model, bad, **kw)
    assert not model.training
    torch.cuda.synchronize()
