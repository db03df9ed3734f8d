"""The beyond-accuracy list figures on the device (csrc/list_quality.hip through engine.lists and evaluate.list_quality) against
the host oracle of tests/list_quality_oracle.py: exposure counts exactly on both tiers and at the tier boundary, the summary's
integers exactly and its two fp64 sums within the bound of any summation order, the intra-list diversity bit for bit on data whose
fp32 Gram matrix is known bit for bit and within a derived bound on arbitrary data."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import list_quality_oracle as orc
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CSRC = os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc")
DIV_KS = (2, 3, 20, 32, 33, 63, 64)
DIV_DS = (1, 3, 4, 5, 63, 64, 65, 130, 515)
N_ITEMS = 50


def _eng():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine


def _source_constant(name, file="list_quality.hip"):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", open(os.path.join(CSRC, file)).read(), flags=re.M)
    assert m, (name, file)
    return int(m.group(1))


LDS_ITEMS = _source_constant("NGCF_EXPOSURE_LDS_ITEMS")


# ---- exposure ----------------------------------------------------------------------------------------------------------------------
def _random_lists(rng, B, k, n_items):
    """Random ids with interior empty slots and a random number of trailing ones per row."""
    lists = rng.integers(0, n_items, (B, k))
    lists[rng.random((B, k)) < 0.15] = -1
    tail = rng.integers(0, k + 1, B)
    lists[np.arange(k)[None, :] >= (k - tail // 2)[:, None]] = -1
    return lists


@pytest.mark.parametrize("n_items", [1, 100, LDS_ITEMS - 1, LDS_ITEMS, LDS_ITEMS + 1])
def test_exposure_counts_equal_the_loop_on_both_tiers(n_items):
    lists_mod = _eng().lists
    rng = np.random.default_rng(n_items)
    for B, k in ((0, 20), (1, 1), (1, 256), (257, 20), (257, 256), (3000, 1), (3000, 20)):
        lists = _random_lists(rng, B, k, n_items)
        want, bad = orc.exposure_counts(lists, n_items)
        assert not bad
        got = lists_mod.exposure_counts(torch.from_numpy(lists).to(DEV), n_items)
        assert got.dtype == torch.int64 and got.cpu().tolist() == want, (B, k)


@pytest.mark.parametrize("n_items", [100, LDS_ITEMS, LDS_ITEMS + 1])
def test_exposure_one_item_takes_every_add_and_chunks_add_up(n_items):
    lists_mod = _eng().lists
    hot = n_items - 1
    same = torch.full((3000, 20), hot, dtype=torch.int64, device=DEV)
    got = lists_mod.exposure_counts(same, n_items)
    assert int(got[hot]) == 60000 and int(got.sum()) == 60000
    # a column slice of a wider tensor (row pitch > k), the k argument, and two chunks into one `out`
    rng = np.random.default_rng(7 + n_items)
    wide = _random_lists(rng, 700, 27, n_items)
    wide_d = torch.from_numpy(wide).to(DEV)
    view = wide_d[:, 3:3 + 20]
    assert view.stride(0) == 27
    want = orc.exposure_counts(wide[:, 3:23], n_items)[0]
    assert lists_mod.exposure_counts(view, n_items).cpu().tolist() == want
    assert lists_mod.exposure_counts(wide_d[:, 3:], n_items, k=20).cpu().tolist() == want
    assert lists_mod.exposure_counts(view, n_items, k=5).cpu().tolist() == orc.exposure_counts(wide[:, 3:8], n_items)[0]
    out = torch.zeros(n_items, dtype=torch.int64, device=DEV)
    assert lists_mod.exposure_counts(view[:300], n_items, out=out) is out
    lists_mod.exposure_counts(view[300:], n_items, out=out)
    assert out.cpu().tolist() == want
    assert torch.equal(lists_mod.exposure_counts(view, n_items), lists_mod.exposure_counts(view, n_items))


@pytest.mark.parametrize("n_items", [100, LDS_ITEMS + 1])
def test_exposure_flags_an_id_past_the_catalogue_and_counts_the_rest(n_items):
    """The bad entry goes through the status word by design: it is compared with n_items before anything else is done with it
    (tests/test_list_quality_surface.py reads that in the source) and is never an index."""
    lists_mod = _eng().lists
    rng = np.random.default_rng(3)
    lists = _random_lists(rng, 257, 20, n_items)
    lists[100, 7], lists[256, 19] = n_items, 2 ** 40
    want, bad = orc.exposure_counts(lists, n_items)
    assert bad
    out = torch.zeros(n_items, dtype=torch.int64, device=DEV)
    with pytest.raises(IndexError, match="n_items"):
        lists_mod.exposure_counts(torch.from_numpy(lists).to(DEV), n_items, out=out)
    assert out.cpu().tolist() == want
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    again = lists_mod.exposure_counts(torch.from_numpy(lists).to(DEV), n_items, status=status)
    assert int(status) == 1 and again.cpu().tolist() == want


# ---- summary -----------------------------------------------------------------------------------------------------------------------
def _histogram(n_items, seed):
    """Counts and popularities below 5000, where the oracle's log2 has the kernels' bits (tests/test_dd_log2.py); n_items = 1 uses
    powers of two."""
    rng = np.random.default_rng(seed)
    if n_items == 1:
        return np.array([8]), np.array([2]), 1024
    counts = rng.integers(0, 4000, n_items)
    counts[rng.random(n_items) < 0.3] = 0
    counts[0] = 17
    pop = rng.integers(0, 3000, n_items)
    return counts, pop, 3001


@pytest.mark.parametrize("n_items", [1, 2, 100, 257, 70001])
def test_summary_integers_exactly_floats_within_the_summation_bound(n_items):
    """clog and nov are sums of n_items terms in a fixed tree; whatever the order, a sum of n floats lies within
    (n - 1) * 2^-53 * sum |term| (to first order) of the exact sum, which math.fsum returns.  That is the bound, as stated: it is not
    fitted to what the kernel returns."""
    lists_mod = _eng().lists
    counts, pop, n_user = _histogram(n_items, n_items)
    want = orc.summary_numbers(counts, pop, n_user)
    got = lists_mod.exposure_summary(torch.from_numpy(counts).to(DEV), torch.from_numpy(pop).to(DEV), n_user)
    assert (got["covered"], got["total"], got["weighted"]) == (want["covered"], want["total"], want["weighted"])
    for name in ("clog", "nov"):
        bound = (n_items - 1) * 2.0 ** -53 * want[name + "_abs"]
        print(name, got[name], want[name], abs(got[name] - want[name]), bound)
        assert abs(got[name] - want[name]) <= bound
    fig = orc.figures(want, n_items)
    assert got["gini"] == fig["gini"] and got["coverage"] == fig["coverage"]               # bit for bit: formed from exact integers
    total = want["total"]
    assert got["entropy"] == math.log2(total) - got["clog"] / total and got["novelty"] == got["nov"] / total
    # against the oracle's figures: the sums' bound divided by total, and the roundings of the divide and the subtraction
    assert abs(got["entropy"] - fig["entropy"]) <= (n_items - 1) * 2.0 ** -53 * want["clog_abs"] / total + 2.0 ** -50 * math.log2(total)
    assert abs(got["novelty"] - fig["novelty"]) <= (n_items - 1) * 2.0 ** -53 * want["nov_abs"] / total + 2.0 ** -52 * abs(fig["novelty"])
    # without popularity: the same four numbers, no novelty; and identical from run to run
    plain = lists_mod.exposure_summary(torch.from_numpy(counts).to(DEV))
    assert plain["clog"] == got["clog"] and plain["weighted"] == got["weighted"] and math.isnan(plain["novelty"]) and plain["nov"] == 0.0
    assert lists_mod.exposure_summary(torch.from_numpy(counts).to(DEV), torch.from_numpy(pop).to(DEV), n_user) == got


def test_summary_of_an_empty_histogram_and_the_status_bits():
    lists_mod = _eng().lists
    empty = lists_mod.exposure_summary(torch.zeros(100, dtype=torch.int64, device=DEV))
    assert empty["covered"] == 0 and empty["total"] == 0
    assert all(math.isnan(empty[n]) for n in ("coverage", "gini", "entropy", "novelty"))
    # n_items * total = 4 * 2^60 = 2^62: the weighted sum is not computed, the rest is
    big = torch.tensor([2 ** 60, 0, 0, 0], dtype=torch.int64, device=DEV)
    six = lists_mod.exposure_summary_launch(big).cpu().tolist()
    assert six[:4] == [1, 2 ** 60, 0, lists_mod.SUMMARY_OVERFLOW]
    with pytest.raises(OverflowError):
        lists_mod.exposure_summary(big)
    below = torch.tensor([2 ** 60 - 1, 0, 0, 0], dtype=torch.int64, device=DEV)           # 4 * (2^60 - 1) < 2^62
    assert lists_mod.exposure_summary_launch(below).cpu().tolist()[:4] == [1, 2 ** 60 - 1, 4 * (2 ** 60 - 1), 0]
    with pytest.raises(RuntimeError, match="negative"):
        lists_mod.exposure_summary(torch.tensor([3, -1, 2], dtype=torch.int64, device=DEV))


# ---- diversity ---------------------------------------------------------------------------------------------------------------------
def _div_lists(rng, B, k, n_items=N_ITEMS):
    """Random ids in [1, n_items) (item 0 is the all-zero row, placed on purpose) and, from 8 rows on, the special rows: V = 0, 1 and
    2, interior empty slots, one id everywhere, the zero row, a duplicate pair, a trailing empty slot."""
    lists = rng.integers(1, n_items, (B, k))
    if B >= 8:
        lists[0] = -1
        lists[1] = -1
        lists[1, k - 1] = 3
        lists[2] = -1
        lists[2, 0], lists[2, k - 1] = 4, 5
        lists[3, ::2] = -1
        lists[4] = 7
        lists[5, 0] = 0
        lists[6, k // 2] = 0
        lists[6, 0] = lists[6, k - 1]
        lists[7, k - 1] = -1
    return lists


def _cutoffs(k):
    return tuple(sorted({K for K in (2, 3, k // 2, k - 1, k) if 2 <= K <= k}))


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


def _check_sums(sums, per_user, counted):
    """sums = [sum of ild@K, rows counted]: the counters exactly; the sums of non-negative terms within the bound of any summation
    order, (B - 1) * 2^-53 * sum |term|, of math.fsum."""
    n_ks = per_user.shape[1]
    sums = sums.cpu().tolist()
    for q in range(n_ks):
        assert sums[n_ks + q] == float(counted[:, q].sum())
        want = math.fsum(per_user[:, q].tolist())
        assert abs(sums[q] - want) <= (per_user.shape[0] - 1) * 2.0 ** -53 * math.fsum(np.abs(per_user[:, q]).tolist())


def _run_exact(k, table_of, gram, seed):
    lists_mod = _eng().lists
    ks = _cutoffs(k)
    for D in DIV_DS:
        rng = np.random.default_rng(seed + 1000 * k + D)
        table = table_of(rng, N_ITEMS, D)
        table[0] = 0.0
        lists = _div_lists(rng, 10, k)
        want, counted = orc.ild_rows(table, lists, ks, gram)
        top = torch.from_numpy(lists).to(DEV)
        for name, emb in _layouts(table).items():
            (sums, per_user) = lists_mod.list_diversity(top, emb, ks, per_user=True, sums=torch.zeros(2 * len(ks), dtype=torch.float64, device=DEV))
            got = per_user.cpu().numpy()
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (k, D, name, got, want)
            _check_sums(sums, want, counted)
        assert want[4].max() == 0.0 and (counted[0] == 0).all() and (counted[1] == 0).all() and (counted[2] == (np.array(ks) == k)).all()


@pytest.mark.parametrize("k", DIV_KS)
def test_diversity_integer_tables_bit_for_bit(k):
    """Item tables in +-{1..8}: every partial sum of a Gram entry is an integer below 2^24 (orc.gram_exact asserts it), so G is exact in
    any accumulation order and everything after it is the header's fp64 chain: per-user values equal the oracle bit for bit on both
    load paths, the row counters are exact, the sums lie within the bound of any order."""
    _run_exact(k, orc.int_table, orc.gram_exact, 11)


@pytest.mark.parametrize("k", DIV_KS)
def test_diversity_pins_the_ascending_fmaf_chain(k):
    """8-bit significands in a narrow exponent window: orc.gram_chain is fmaf step by step (TwoSum error asserted 0) in ascending k,
    and the data does round in fp32 - tests/test_list_quality_oracle.py shows the descending order gives other bits - so a
    reordered or unfused accumulation fails here."""
    _run_exact(k, orc.chain_table, orc.gram_chain, 12)


@pytest.mark.parametrize("k", [3, 20, 33, 64])
def test_diversity_normal_tables_within_the_chain_bound(k):
    """N(0, 1) tables.  The kernel's G_ab is a chain of D fmaf, each one rounding, so |G_ab - G64_ab| <= gamma_D T_ab with
    T_ab = sum_k |x_k y_k| and gamma_D = D 2^-24 / (1 - D 2^-24).  On the diagonal T_aa = G64_aa, so G_aa = G64_aa (1 + e_a) with
    |e_a| <= gamma_D.  With N = sqrt(G64_aa G64_bb) and c = G64_ab / N the computed cosine is
    (G64_ab + eps) / (N sqrt((1 + e_a)(1 + e_b))), |eps| <= gamma_D T_ab, and 1 / sqrt((1 + e_a)(1 + e_b)) lies in
    [1 / (1 + gamma_D), 1 / (1 - gamma_D)], so
        |cos - c| <= |c| (1 / (1 - gamma_D) - 1) + gamma_D T_ab / (N (1 - gamma_D)) = (|c| + T_ab / N) gamma_D / (1 - gamma_D).
    ild is the mean of 1 - cos over the pairs: its error is at most the mean of the pairs' bounds, plus the fp64 roundings (four
    per pair and one per addition of terms <= 2: below (pairs + 8) 2^-51).  orc.ild_bound computes exactly that."""
    lists_mod = _eng().lists
    ks = _cutoffs(k)
    for D in (5, 65, 515):
        rng = np.random.default_rng(13 + 1000 * k + D)
        table = rng.standard_normal((N_ITEMS, D)).astype(np.float32)
        table[0] = 0.0
        lists = _div_lists(rng, 10, k)
        top = torch.from_numpy(lists).to(DEV)
        outs = []
        for name, emb in _layouts(table).items():
            res, per_user = lists_mod.list_diversity(top, emb, ks, per_user=True)
            outs.append(per_user.cpu().numpy())
            for r in range(lists.shape[0]):
                for q, K in enumerate(ks):
                    ref = orc.ild_bound(table, lists[r], K)
                    if ref is None:
                        assert outs[-1][r, q] == 0.0
                        continue
                    print(k, D, name, r, K, outs[-1][r, q], ref[0], abs(outs[-1][r, q] - ref[0]), ref[1])
                    assert abs(outs[-1][r, q] - ref[0]) <= ref[1]
            assert res[f"lists@{k}"] == sum(orc.ild_bound(table, ids, k) is not None for ids in lists)
        assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))   # the two load paths: the same bits


@functools.lru_cache(maxsize=None)
def _big_case(k, D):
    """300 lists (read only): the oracle's values once, shared by the tests below."""
    rng = np.random.default_rng(14 + k + D)
    table = orc.chain_table(rng, N_ITEMS, D)
    table[0] = 0.0
    lists = _div_lists(rng, 300, k)
    ks = _cutoffs(k)
    want, counted = orc.ild_rows(table, lists, ks, orc.gram_chain)
    return table, lists, ks, want, counted


@pytest.mark.parametrize("k, D", [(20, 65), (33, 5)])
def test_diversity_does_not_depend_on_the_batch_or_the_row_order(k, D):
    lists_mod = _eng().lists
    table, lists, ks, want, counted = _big_case(k, D)
    emb = _layouts(table)["aligned"]
    top = torch.from_numpy(lists).to(DEV)
    sums, per_user = lists_mod.list_diversity(top, emb, ks, per_user=True, sums=torch.zeros(2 * len(ks), dtype=torch.float64, device=DEV))
    got = per_user.cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    _check_sums(sums, want, counted)
    for B in (1, 2):                                            # a row's value whatever the batch it is in
        _, few = lists_mod.list_diversity(top[8:8 + B], emb, ks, per_user=True)
        assert torch.equal(few, per_user[8:8 + B])
    perm = torch.from_numpy(np.random.default_rng(0).permutation(300)).to(DEV)
    _, shuffled = lists_mod.list_diversity(top[perm], emb, ks, per_user=True)
    assert torch.equal(shuffled, per_user[perm])
    # several cut-offs in one call equal the single-cut-off calls, bit for bit; two runs give identical bits, sums included
    for q, K in enumerate(ks):
        _, single = lists_mod.list_diversity(top, emb, (K,), per_user=True)
        assert torch.equal(single[:, 0], per_user[:, q])
    again, per_user2 = lists_mod.list_diversity(top, emb, ks, per_user=True, sums=torch.zeros(2 * len(ks), dtype=torch.float64, device=DEV))
    assert torch.equal(again, sums) and torch.equal(per_user2, per_user)
    # chunks into one slot vector; the means of the public call
    acc = torch.zeros(2 * len(ks), dtype=torch.float64, device=DEV)
    for lo, hi in ((0, 70), (70, 300)):
        assert lists_mod.list_diversity(top[lo:hi], emb, ks, sums=acc) is acc
    assert torch.equal(acc[len(ks):], sums[len(ks):])
    torch.testing.assert_close(acc, sums, rtol=1e-13, atol=0)
    res = lists_mod.list_diversity(top, emb, ks)
    for q, K in enumerate(ks):
        n = int(counted[:, q].sum())
        assert res[f"lists@{K}"] == n and res[f"ild@{K}"] == float(sums[q]) / n
    # a longer list than the limit, cut-offs within it: the first columns alone count
    wide = torch.cat((top, torch.full((300, 70), 1, dtype=torch.int64, device=DEV)), 1)
    assert wide.shape[1] > 64
    _, from_wide = lists_mod.list_diversity(wide, emb, ks, per_user=True)
    assert torch.equal(from_wide, per_user)
    assert lists_mod.list_diversity(top[:0], emb, ks)[f"lists@{k}"] == 0


def test_diversity_nan_propagates_and_a_bad_id_is_flagged():
    lists_mod = _eng().lists
    rng = np.random.default_rng(15)
    table = orc.int_table(rng, N_ITEMS, 37)
    table[0] = 0.0
    lists = _div_lists(rng, 12, 20)
    ks = (5, 20)
    poisoned = table.copy()
    poisoned[9, 30] = np.nan
    lists[8:][lists[8:] == 9] = 11
    lists[8, 2], lists[10, 19] = 9, 9
    clean, _ = orc.ild_rows(table, lists, ks, orc.gram_exact)
    _, per_user = lists_mod.list_diversity(torch.from_numpy(lists).to(DEV), torch.from_numpy(poisoned).to(DEV), ks, per_user=True)
    got = per_user.cpu().numpy()
    assert np.isnan(got[8]).all() and np.isnan(got[10, 1]) and got[10, 0] == clean[10, 0]
    rest = [r for r in range(12) if r not in (8, 10) and 9 not in lists[r]]
    assert len(rest) >= 6 and np.array_equal(got[rest], clean[rest])
    # an id past the catalogue: flagged through the status word, its slot empty, every other row as before
    lists[3, 1] = N_ITEMS
    bad = torch.from_numpy(lists).to(DEV)
    with pytest.raises(IndexError, match="n_items"):
        lists_mod.list_diversity(bad, torch.from_numpy(table).to(DEV), ks)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, flagged = lists_mod.list_diversity(bad, torch.from_numpy(table).to(DEV), ks, per_user=True, status=status,
                                          sums=torch.zeros(4, dtype=torch.float64, device=DEV))
    lists[3, 1] = -1
    as_empty, _ = orc.ild_rows(table, lists, ks, orc.gram_exact)
    assert int(status) == 1 and np.array_equal(flagged.cpu().numpy(), as_empty)


# ---- evaluate.list_quality ---------------------------------------------------------------------------------------------------------
N_USER, N_ITEM = 600, 30


@functools.lru_cache(maxsize=None)
def _model():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    laps = [pkg.graphs.to_sparse_coo(s) for s in pkg.graphs.seoul_standin(DEV, seed=6, n_user=N_USER, n_item=N_ITEM)]
    num_dict = {"user": N_USER, "item": N_ITEM, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(1801)
    return pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, laps, num_dict, 25, DEV).to(DEV)


def _compose(top, table, pop, ks):
    """rank_topk's lists read back -> the oracle: per K the summary numbers, the figures and the mean ild."""
    out = {}
    for K in ks:
        counts, bad = orc.exposure_counts(top, N_ITEM, k=K)
        assert not bad
        num = orc.summary_numbers(counts, pop, N_USER)
        out[K] = dict(orc.figures(num, N_ITEM), numbers=num)
        if 2 <= K <= orc.K_MAX:
            bounds = [orc.ild_bound(table, ids, K) for ids in top]
            bounds = [b for b in bounds if b is not None]
            out[K]["ild"] = math.fsum(b[0] for b in bounds) / len(bounds) if bounds else math.nan
            out[K]["ild_bound"] = math.fsum(b[1] for b in bounds) / len(bounds) + len(bounds) * 2.0 ** -52 if bounds else 0.0
            out[K]["lists"] = len(bounds)
    return out


def _same_figures(got, want, n_lists):
    for K, w in want.items():
        g = got[K]
        num = w["numbers"]
        assert g["users"] == n_lists
        assert g["coverage"] == w["coverage"] and g["gini"] == w["gini"]                   # from exact integers: bit for bit
        total = num["total"]
        # entropy = log2(total) - clog / total, novelty = nov / total: the sums' bound divided by total, and one rounding each
        assert abs(g["entropy"] - w["entropy"]) <= (N_ITEM - 1) * 2.0 ** -53 * num["clog_abs"] / total + 2.0 ** -50 * math.log2(total)
        assert abs(g["novelty"] - w["novelty"]) <= (N_ITEM - 1) * 2.0 ** -53 * num["nov_abs"] / total + 2.0 ** -52 * abs(w["novelty"])
        if "ild" in w and w["lists"]:
            print(K, g["ild"], w["ild"], abs(g["ild"] - w["ild"]), w["ild_bound"])
            assert abs(g["ild"] - w["ild"]) <= w["ild_bound"]
        else:
            assert math.isnan(g["ild"])


def test_list_quality_equals_rank_topk_then_the_oracle():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = _eng()
    model = _model()
    model.train()
    train = eng.ItemSets.from_laplacian(model.laplacian_csr(0), N_USER)
    ks = (1, 5, 20)
    got = pkg.evaluate.list_quality(model, train, ks=ks, user_chunk=250)
    assert model.training and set(got) == set(ks)
    assert all(set(v) == {"coverage", "gini", "entropy", "novelty", "ild", "users"} for v in got.values())
    with torch.no_grad():
        model.eval()
        model.propagate(0)
        items = model.all_items_emb
        _, top = eng.rank_topk(model.all_users_emb, items, 20, exclude=train)
        model.train()
    top_h, table = top.cpu().numpy(), items.cpu().numpy().copy()
    assert (top_h[:, -1] == -1).any()                                                       # short lists: trailing empty slots
    pop = np.bincount(train.colidx.cpu().numpy().astype(np.int64) - train.col_offset, minlength=N_ITEM)
    want = _compose(top_h, table, pop, ks)
    _same_figures(got, want, N_USER)
    assert math.isnan(got[1]["ild"]) and 0.0 < got[20]["ild"] < 2.0 and 0.0 < got[5]["coverage"] <= 1.0
    # one chunk or three, the same users: the integers do not move, the sums to rounding
    whole = pkg.evaluate.list_quality(model, train, ks=ks)
    for K in ks:
        assert whole[K]["gini"] == got[K]["gini"] and whole[K]["coverage"] == got[K]["coverage"]
        assert whole[K]["entropy"] == got[K]["entropy"] and whole[K]["novelty"] == got[K]["novelty"]
        assert whole[K]["ild"] == pytest.approx(got[K]["ild"], rel=1e-13, nan_ok=True)
    # a user subset
    some = torch.tensor([5, 599, 42, 5], device=DEV)
    sub = pkg.evaluate.list_quality(model, train, ks=(5,), user_ids=some)
    _same_figures(sub, _compose(top_h[[5, 599, 42, 5], :5], table, pop, (5,)), 4)
    with pytest.raises(IndexError):
        pkg.evaluate.list_quality(model, train, ks=(5,), user_ids=torch.tensor([N_USER], device=DEV))


def test_list_quality_takes_given_lists():
    """`lists=` with blended_ranking-shaped input (int64 [G, top], -1 padded): nothing is ranked, the figures equal the direct
    calls' and the oracle's."""
    import seoul_tourism_recommendation_ngcf_amd as pkg
    eng = _eng()
    model = _model()
    model.eval()
    train = eng.ItemSets.from_laplacian(model.laplacian_csr(0), N_USER)
    rng = np.random.default_rng(16)
    given = _random_lists(rng, 40, 10, N_ITEM)
    given[0] = -1
    ks = (3, 10)
    got = pkg.evaluate.list_quality(model, train, ks=ks, lists=torch.from_numpy(given).to(DEV))
    with torch.no_grad():
        model.propagate(0)
        items = model.all_items_emb
    pop_d = eng.lists.exposure_counts((train.colidx.to(torch.int64) - train.col_offset).reshape(-1, 1), N_ITEM)
    pop = np.bincount(train.colidx.cpu().numpy().astype(np.int64) - train.col_offset, minlength=N_ITEM)
    assert pop_d.cpu().tolist() == pop.tolist()
    _same_figures(got, _compose(given, items.cpu().numpy().copy(), pop, ks), 40)
    top = torch.from_numpy(given).to(DEV)
    div = eng.lists.list_diversity(top, items, ks)
    for K in ks:
        direct = eng.lists.exposure_summary(eng.lists.exposure_counts(top, N_ITEM, k=K), pop_d, N_USER)
        assert all(got[K][name] == direct[name] for name in ("coverage", "gini", "entropy", "novelty"))
        assert got[K]["ild"] == div[f"ild@{K}"]
    with pytest.raises(ValueError, match="lists must be"):
        pkg.evaluate.list_quality(model, train, ks=(11,), lists=torch.from_numpy(given).to(DEV))
