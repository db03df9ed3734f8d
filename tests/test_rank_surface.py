"""Host-side surface of the full-catalogue ranking: item sets, the held-out split, argument checks before any launch."""
import ast
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_item_sets_from_pairs_on_cpu():
    from seoul_tourism_recommendation_ngcf_amd import engine
    users = torch.tensor([2, 0, 2, 0, 2, 3, 0])
    items = torch.tensor([4, 1, 0, 1, 3, 2, 0])
    s = engine.ItemSets.from_pairs(users, items, 5, 6)
    assert s.rowptr.tolist() == [0, 2, 2, 5, 6, 6]
    assert s.colidx.tolist() == [0, 1, 0, 3, 4, 2]
    assert s.rowptr.dtype == torch.int64 and s.colidx.dtype == torch.int32
    assert s.col_offset == 0 and s.n_items == 6 and s.n_rows == 5
    with pytest.raises(IndexError):
        engine.ItemSets.from_pairs(torch.tensor([5]), torch.tensor([0]), 5, 6)


def test_holdout_split_deterministic_disjoint_complete():
    from seoul_tourism_recommendation_ngcf_amd import graphs
    u, i, w = graphs.synthetic_interactions(500, 80, 6000, seed=3, device="cpu")
    tr, te = graphs.holdout_split(u, i, w, 0.2, seed=7)
    tr2, te2 = graphs.holdout_split(u, i, w, 0.2, seed=7)
    assert all(torch.equal(a, b) for a, b in zip(tr + te, tr2 + te2))
    _, te3 = graphs.holdout_split(u, i, w, 0.2, seed=8)
    assert not torch.equal(te[1], te3[1]) or not torch.equal(te[0], te3[0])
    k_tr = set((tr[0] * 80 + tr[1]).tolist())
    k_te = set((te[0] * 80 + te[1]).tolist())
    assert not (k_tr & k_te)
    assert k_tr | k_te == set((u * 80 + i).tolist())
    cnt = torch.bincount(u, minlength=500)
    cnt_te = torch.bincount(te[0], minlength=500)
    want = torch.where(cnt >= 2, torch.clamp(torch.ceil(cnt.double() * 0.2).long(), max=cnt - 1), torch.zeros_like(cnt))
    assert torch.equal(cnt_te, want)
    coo = graphs.bipartite_from_interactions(tr[0], tr[1], tr[2], 500, 80)
    assert coo["interactions"] == tr[0].numel() and coo["nnz"] == 2 * tr[0].numel()
    full = graphs.synthetic_bipartite(500, 80, 6000, seed=3, device="cpu")
    same = graphs.bipartite_from_interactions(u, i, w, 500, 80)
    assert all(torch.equal(full[k], same[k]) for k in ("rows", "cols", "vals"))


def test_rank_argument_errors_before_launch():
    from seoul_tourism_recommendation_ngcf_amd import engine
    with pytest.raises(RuntimeError, match="ROCm device"):
        engine.rank_topk(torch.zeros(2, 4), torch.zeros(5, 4), 2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        engine.ranking_metrics(torch.zeros(2, 4, dtype=torch.int64), None, [2])
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    assert lib.ngcf_rank_workspace_bytes(4, 100_000, 64, 100) > 0          # a small batch splits the item range
    assert lib.ngcf_rank_workspace_bytes(1_000_000, 100_000, 512, 20) == 0
    assert lib.ngcf_rank_workspace_bytes(4, 100, 64, 257) == -1
    for k in (0, 101, 257):
        rc = lib.ngcf_rank_topk_f32(None, 64, None, 4, 4, None, 64, 100, 64, k, None, None, 0, None, None, None, None, 0, None)
        assert rc == _lib.ERR_ARG
        assert "out of range" in _lib.last_error() or "recommend_topk" in _lib.last_error()
    import ctypes as C
    arr = (C.c_int32 * 1)(30)
    assert lib.ngcf_rank_metrics(None, 4, 20, None, 4, None, None, 0, arr, 1, None, None, None, None) == _lib.ERR_ARG
    assert "cut-off" in _lib.last_error()


def test_evaluate_is_exported_and_stands_alone():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    assert "evaluate" in pkg.__all__ and callable(pkg.evaluate.full_ranking)
    src = open(os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "evaluate.py")).read()
    names = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add(node.module or "")
    assert not any("oracle" in n for n in names)
