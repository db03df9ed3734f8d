"""The greedy MMR re-rank on the device (csrc/list_rerank.hip through engine.lists.mmr_rerank and recommend.diversified_ranking)
against the host oracle of tests/rerank_oracle.py: picks, pool columns and the keys' bits on data whose fp32 Gram matrix is known bit
for bit, at the kernel's branch points (one tile / three tiles, both load paths, chunk edges of D); independence of the batch; the
NaN rules and the bad-id flag; arbitrary data within the bound the fmaf chain implies."""
import functools
import math

import numpy as np
import pytest
import torch

import rerank_oracle as orc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N_ITEMS = 50
NS = (1, 2, 3, 31, 32, 33, 63, 64)
DS = (1, 31, 32, 33, 130)
LAMS = (0.0, 0.3, 1.0)


def _lists():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.lists


def _layouts(table):
    """The same float32 table twice on the device: rows padded to a multiple of 4 floats from a 16-byte aligned base (the 16-byte
    loads), and an odd-offset column slice of a wider buffer (the dword loads)."""
    t = torch.from_numpy(table)
    n, D = t.shape
    padded = torch.full((n, (D + 3) // 4 * 4 + 4), float("nan"), device=DEV)
    padded[:, :D] = t.to(DEV)
    odd = torch.full((n + 1, D + 3), float("nan"), device=DEV)
    odd[1:, 1:1 + D] = t.to(DEV)
    a, b = padded[:, :D], odd[1:, 1:1 + D]
    assert a.data_ptr() % 16 == 0 and a.stride(0) % 4 == 0 and (b.data_ptr() % 16 != 0 or b.stride(0) % 4 != 0)
    return {"aligned": a, "odd": b}


def _pools(rng, B, n, n_items=N_ITEMS):
    """Random ids in [1, n_items) (item 0 is the all-zero row, placed on purpose) with random float32 relevances and, from 10 rows on,
    the special rows: all empty, one non-empty slot, interior empty slots, one id everywhere, the zero row, a duplicate pair, a
    trailing empty slot (with a huge relevance that must not count), equal relevances throughout, small-integer relevances (ties)."""
    pools = rng.integers(1, n_items, (B, n))
    rel = rng.standard_normal((B, n)).astype(np.float32)
    if B >= 10:
        pools[0] = -1
        rel[0] = -np.inf
        pools[1] = -1
        pools[1, n - 1] = 3
        pools[2, ::2] = -1
        rel[2, ::2] = -np.inf
        pools[3] = 7
        pools[4, 0] = 0
        pools[5, n // 2] = 0
        pools[5, 0] = pools[5, n - 1]
        pools[6, n - 1] = -1
        rel[6, n - 1] = 1e30
        rel[7] = 0.25
        rel[8] = rng.integers(0, 3, n)
    return pools, rel


def _tops(n):
    return tuple(sorted({t for t in (1, n // 2, n) if 1 <= t <= n}))


def _same(got, want, what):
    items, slots, keys = (x.cpu().numpy() for x in got)
    assert np.array_equal(items, want[0]), (what, items, want[0])
    assert slots.dtype == np.int32 and np.array_equal(slots, want[1]), (what, slots, want[1])
    assert np.array_equal(keys.view(np.int64), want[2].view(np.int64)), (what, keys, want[2])


def _run_exact(n, D, table_of, gram, seed):
    lists = _lists()
    rng = np.random.default_rng(seed + 1000 * n + D)
    table = table_of(rng, N_ITEMS, D)
    table[0] = 0.0
    pools, rel32 = _pools(rng, 10, n)
    rel64 = rel32.astype(np.float64)
    fin = np.isfinite(rel64)
    rel64[fin] = rel64[fin] + rng.standard_normal(int(fin.sum())) * 2.0 ** -30       # values no float32 holds
    rel64[7] = 0.25
    grams = [gram(table, ids) for ids in pools]                                      # once per case, shared by every combination
    pool_d = torch.from_numpy(pools).to(DEV)
    rels = {np.float32: (rel32, torch.from_numpy(rel32).to(DEV)), np.float64: (rel64, torch.from_numpy(rel64).to(DEV))}
    embs = _layouts(table)
    for ti, top in enumerate(_tops(n)):
        for li, lam in enumerate(LAMS):
            for ni, normalize in enumerate((False, True)):
                rel_h, rel_d = rels[np.float64 if (ti + li + ni) % 2 else np.float32]
                want = (np.full((10, top), -1, dtype=np.int64), np.full((10, top), -1, dtype=np.int32), np.full((10, top), -np.inf))
                for b, (G, ok) in enumerate(grams):
                    s, k = orc.mmr_row(G, ok, rel_h[b], top, lam, normalize)
                    want[1][b], want[2][b] = s, k
                    want[0][b] = [int(pools[b][a]) if a >= 0 else -1 for a in s]
                assert (want[0][0] == -1).all() and (want[2][0] == -np.inf).all() and want[0][1, 0] == 3 and (want[0][1, 1:] == -1).all()
                for name, emb in embs.items():
                    got = lists.mmr_rerank(pool_d, rel_d, emb, top, lam=lam, normalize=normalize, return_slots=True, return_keys=True)
                    _same(got, want, (n, D, top, lam, normalize, rel_h.dtype, name))
                    assert torch.equal(lists.mmr_rerank(pool_d, rel_d, emb, top, lam=lam, normalize=normalize), got[0])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_mmr_integer_tables_bit_for_bit(n, D):
    """Item tables in +-{1..8}: the Gram matrix is exact in any accumulation order (orc.gram_exact asserts it), everything after it is
    the header's fp64 arithmetic and its ordering rules: items, pool columns and the keys' bits equal the oracle on both load paths,
    for top in {1, n // 2, n}, lam in {0, 0.3, 1}, normalize off and on, fp32 and fp64 relevances."""
    _run_exact(n, D, orc.int_table, orc.gram_exact, 21)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_mmr_pins_the_ascending_fmaf_chain(n, D):
    """8-bit significands in a narrow exponent window: orc.gram_chain is fmaf step by step in ascending k and the data does round in
    fp32, so a reordered or unfused accumulation gives other cosines and other key bits."""
    _run_exact(n, D, orc.chain_table, orc.gram_chain, 22)


@functools.lru_cache(maxsize=None)
def _big_case():
    """300 pools of 33 (read only): the oracle's result once, shared by the tests below."""
    rng = np.random.default_rng(23)
    table = orc.chain_table(rng, N_ITEMS, 65)
    table[0] = 0.0
    pools, rel = _pools(rng, 300, 33)
    want = orc.mmr_rows(table, pools, rel, 20, 0.3, True, gram=orc.gram_chain)
    return table, pools, rel, want


def test_mmr_does_not_depend_on_the_batch_or_the_row_order():
    lists = _lists()
    table, pools, rel, want = _big_case()
    emb = _layouts(table)["aligned"]
    pool_d, rel_d = torch.from_numpy(pools).to(DEV), torch.from_numpy(rel).to(DEV)
    kw = dict(lam=0.3, normalize=True, return_slots=True, return_keys=True)
    whole = lists.mmr_rerank(pool_d, rel_d, emb, 20, **kw)
    _same(whole, want, "300 rows")
    for lo, B in ((8, 1), (11, 5)):                              # a row's result whatever the batch it is in
        few = lists.mmr_rerank(pool_d[lo:lo + B], rel_d[lo:lo + B], emb, 20, **kw)
        assert all(torch.equal(f, w[lo:lo + B]) for f, w in zip(few, whole))
    perm = torch.from_numpy(np.random.default_rng(0).permutation(300)).to(DEV)
    shuffled = lists.mmr_rerank(pool_d[perm], rel_d[perm], emb, 20, **kw)
    assert all(torch.equal(s, w[perm]) for s, w in zip(shuffled, whole))
    again = lists.mmr_rerank(pool_d, rel_d, emb, 20, **kw)
    assert all(torch.equal(a, w) for a, w in zip(again, whole))
    # a column slice of wider tensors (row pitch > n) is taken as it is
    wide_p = torch.cat((pool_d, torch.full((300, 7), 1, dtype=torch.int64, device=DEV)), 1)
    wide_r = torch.cat((rel_d, torch.full((300, 7), 9.0, device=DEV)), 1)
    assert wide_p[:, :33].stride(0) == 40
    sliced = lists.mmr_rerank(wide_p[:, :33], wide_r[:, :33], emb, 20, **kw)
    assert all(torch.equal(s, w) for s, w in zip(sliced, whole))
    assert tuple(lists.mmr_rerank(pool_d[:0], rel_d[:0], emb, 20).shape) == (0, 20)


def test_mmr_nan_rules_and_a_bad_id_is_flagged():
    lists = _lists()
    rng = np.random.default_rng(24)
    table = orc.int_table(rng, N_ITEMS, 37)
    table[0] = 0.0
    pools, rel = _pools(rng, 12, 20)
    poisoned = table.copy()
    poisoned[9, 30] = np.nan
    pools[pools == 9] = 11
    pools[9, 2], pools[10, 19], pools[11, 0] = 9, 9, 9           # the NaN item row early, last and first in a pool
    rel[11, 0] = 10.0                                             # ... where it is the most relevant: picked first
    rel[10, 5] = np.nan                                           # and a NaN relevance
    rel[4, 3] = np.nan
    pool_d, rel_d = torch.from_numpy(pools).to(DEV), torch.from_numpy(rel).to(DEV)
    for lam, normalize in ((0.3, True), (0.3, False), (1.0, True), (0.0, False)):
        want = orc.mmr_rows(table, pools, rel, 20, lam, normalize, poisoned=(9,))
        got = lists.mmr_rerank(pool_d, rel_d, torch.from_numpy(poisoned).to(DEV), 20, lam=lam, normalize=normalize, return_slots=True,
                               return_keys=True)
        _same(got, want, (lam, normalize))
        if lam == 0.3:
            assert np.isnan(want[2][11, 1:]).all() and not np.isnan(want[2][11, 0])     # picked first: every later key is a NaN
            assert want[1][4, -1] == 3 and np.isnan(want[2][4, -1])                      # the NaN relevance goes last
    # an id past the catalogue: flagged through the status word, its slot empty, every other row as before
    clean = orc.mmr_rows(table, pools, rel, 20, 0.3, True, poisoned=(9,))
    pools[3, 1], pools[6, 0] = N_ITEMS, 2 ** 40
    bad = torch.from_numpy(pools).to(DEV)
    with pytest.raises(IndexError, match="n_items"):
        lists.mmr_rerank(bad, rel_d, torch.from_numpy(poisoned).to(DEV), 20, lam=0.3)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = lists.mmr_rerank(bad, rel_d, torch.from_numpy(poisoned).to(DEV), 20, lam=0.3, return_slots=True, return_keys=True, status=status)
    as_empty = orc.mmr_rows(table, pools, rel, 20, 0.3, True, poisoned=(9,))
    assert int(status) == 1
    _same(got, as_empty, "bad id")
    rest = [r for r in range(12) if r not in (3, 6)]
    assert all(np.array_equal(a[rest], c[rest]) for a, c in zip(as_empty[:2], clean[:2]))


@pytest.mark.parametrize("lam", [0.5, 0.9])
@pytest.mark.parametrize("n, D, top", [(20, 64, 10), (33, 130, 20)])
def test_mmr_normal_tables_within_the_chain_bound(n, D, top, lam):
    """N(0, 1) tables, 256 pools, normalize on.  The kernel's G_ab is a chain of D rounding fmaf, so no exact oracle exists; the
    cosine computed from it lies within (|c| + T_ab / sqrt(G_aa G_bb)) gamma_D / (1 - gamma_D) of the float64 one
    (tests/test_list_quality_gpu.py derives it).  m_a is the largest of such cosines and moves by at most the largest of their
    bounds; the key takes it times (1 - lam), the relevance term is the same fp64 arithmetic on both sides, and 2^-50 covers the
    fp64 roundings.  A row is compared only if at every step with more than one candidate left the winner's key minus its bound
    exceeds every other candidate's key plus its bound (at least as strict as the gap to the second best); rows left out may be 5 % of
    a case at most.  Compared rows equal the float64 oracle's items exactly and their keys lie within the bound.

    Rows left out by the oracle on these seeds (a property of the data, computed on the CPU): (20, 64, 10): 0 of 256 at lam = 0.5 and
    at lam = 0.9; (33, 130, 20): 1 of 256 (0.4 %) at lam = 0.5, 0 of 256 at lam = 0.9."""
    lists = _lists()
    rng = np.random.default_rng(25 + n)
    table = rng.standard_normal((N_ITEMS, D)).astype(np.float32)
    pools = np.stack([rng.permutation(N_ITEMS)[:n] for _ in range(256)])
    rel = rng.standard_normal((256, n)).astype(np.float32)
    got = lists.mmr_rerank(torch.from_numpy(pools).to(DEV), torch.from_numpy(rel).to(DEV), torch.from_numpy(table).to(DEV), top, lam=lam,
                           normalize=True, return_slots=True, return_keys=True)
    items, slots, keys = (x.cpu().numpy() for x in got)
    left_out, worst = 0, 0.0
    for b in range(256):
        s, k, bounds, decided = orc.mmr_row_f64(table, pools[b], rel[b], top, lam, True)
        if not decided:
            left_out += 1
            continue
        assert slots[b].tolist() == s and items[b].tolist() == pools[b][s].tolist(), b
        for t in range(top):
            worst = max(worst, abs(keys[b, t] - k[t]) / bounds[t])
            assert abs(keys[b, t] - k[t]) <= bounds[t], (b, t, keys[b, t], k[t], bounds[t])
    print(n, D, top, lam, "left out", left_out, "of 256; largest |key - key64| / bound", worst)
    assert left_out <= 256 * 5 // 100


# ---- recommend.diversified_ranking ---------------------------------------------------------------------------------------------------
N_USER, N_ITEM = 600, 30


@functools.lru_cache(maxsize=None)
def _model():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    laps = [pkg.graphs.to_sparse_coo(s) for s in pkg.graphs.seoul_standin(DEV, seed=6, n_user=N_USER, n_item=N_ITEM)]
    num_dict = {"user": N_USER, "item": N_ITEM, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(1801)
    return pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, laps, num_dict, 25, DEV).to(DEV)


def _oracle_from_catalogue_gram(G_all, pools, values, top, lam, normalize):
    """Every pool draws from the same small catalogue: its Gram matrix is a sub-matrix of the catalogue's."""
    B = pools.shape[0]
    items, keys = np.full((B, top), -1, dtype=np.int64), np.full((B, top), -np.inf)
    for b, ids in enumerate(pools):
        ok = ids >= 0
        safe = np.where(ok, ids, 0)
        s, k = orc.mmr_row(G_all[np.ix_(safe, safe)], ok, values[b], top, lam, normalize)
        keys[b] = k
        items[b] = [int(ids[a]) if a >= 0 else -1 for a in s]
    return items, keys


def test_diversified_ranking_equals_rank_topk_then_the_oracle():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    from seoul_tourism_recommendation_ngcf_amd import engine as eng
    model = _model()
    model.train()
    train = eng.ItemSets.from_laplacian(model.laplacian_csr(0), N_USER)
    users = torch.arange(N_USER, device=DEV)
    got_items, got_keys = pkg.recommend.diversified_ranking(model, users, train=train, lam=0.7, pool=64, top=10)
    assert model.training and tuple(got_items.shape) == tuple(got_keys.shape) == (N_USER, 10)
    assert got_items.dtype == torch.int64 and got_keys.dtype == torch.float64
    with torch.no_grad():
        model.eval()
        model.propagate(0)
        table_d = model.all_items_emb
        vals, idx = eng.rank_topk(model.all_users_emb, table_d, N_ITEM, exclude=train)          # pool = 64 is clipped to the catalogue
        model.train()
    table = table_d.cpu().numpy().copy()
    G_all, _ = orc.gram_fma(table, np.arange(N_ITEM))                                            # the fmaf chain of arbitrary data, exactly
    pools, values = idx.cpu().numpy(), vals.cpu().numpy()
    assert (pools[:, -1] == -1).any()                                                            # short pools: trailing empty slots
    want_items, want_keys = _oracle_from_catalogue_gram(G_all, pools, values, 10, 0.7, True)
    assert np.array_equal(got_items.cpu().numpy(), want_items)
    assert np.array_equal(got_keys.cpu().numpy().view(np.int64), want_keys.view(np.int64))
    assert (want_items[:, 0] == pools[:, 0]).all() and (want_items != pools[:, :10]).any()      # the best item first; then it re-orders
    # unchanged by the chunking; a user subset in any order; eval mode stays eval
    model.eval()
    chunked = pkg.recommend.diversified_ranking(model, users, train=train, lam=0.7, pool=64, top=10, user_chunk=7)
    assert not model.training and torch.equal(chunked[0], got_items) and torch.equal(chunked[1], got_keys)
    some = torch.tensor([5, 599, 42, 5], device=DEV)
    sub = pkg.recommend.diversified_ranking(model, some, train=train, lam=0.7, pool=64, top=10)
    assert torch.equal(sub[0], got_items[some]) and torch.equal(sub[1], got_keys[some])
    # lam = 1: rank_topk's own order
    plain = pkg.recommend.diversified_ranking(model, users, train=train, lam=1.0, pool=20, top=10, normalize=False)
    assert torch.equal(plain[0], idx[:, :10]) and torch.equal(plain[1][idx[:, :10] >= 0], vals[:, :10].double()[idx[:, :10] >= 0])
    with pytest.raises(IndexError):
        pkg.recommend.diversified_ranking(model, torch.tensor([N_USER], device=DEV))
    with pytest.raises(ValueError, match="top=31"):
        pkg.recommend.diversified_ranking(model, users, pool=40, top=31)
    # the result is what evaluate.list_quality takes as lists=: diversifying does not lower the diversity it measures
    before = pkg.evaluate.list_quality(model, train, ks=(10,), lists=idx[:, :10])[10]["ild"]
    after = pkg.evaluate.list_quality(model, train, ks=(10,), lists=got_items)[10]["ild"]
    print("ild@10 before", before, "after", after)
    assert after >= before


def test_blended_ranking_lists_rerank_with_their_fp64_ratings():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    model = _model()
    model.eval()
    users = torch.arange(0, N_USER, 3, device=DEV)
    out_items, out_ratings, _ = pkg.recommend.blended_ranking(model, users, top=20, points=N_ITEM)
    assert out_ratings.dtype == torch.float64 and tuple(out_items.shape) == (int(users.numel()), 20)
    with torch.no_grad():
        model.propagate(0)
        table_d = model.all_items_emb
    got = pkg.engine.lists.mmr_rerank(out_items, out_ratings, table_d, 10, lam=0.5, return_keys=True)
    G_all, _ = orc.gram_fma(table_d.cpu().numpy().copy(), np.arange(N_ITEM))
    want_items, want_keys = _oracle_from_catalogue_gram(G_all, out_items.cpu().numpy(), out_ratings.cpu().numpy(), 10, 0.5, True)
    assert np.array_equal(got[0].cpu().numpy(), want_items)
    assert np.array_equal(got[1].cpu().numpy().view(np.int64), want_keys.view(np.int64))
