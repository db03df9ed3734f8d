"""Popularity-weighted negatives on the device (ngcf_weighted_prepare, ngcf_sample_weighted, engine.negatives.WeightedSets /
weighted_unseen, sampling.weighted_negatives / weighted_triplets / WeightedNegativesLoader): items, weights and masses EQUAL to the
host oracle's integers (tests/weighted_oracle.py, whose law tests/test_weighted_oracle.py establishes by enumeration) on every path of
the kernels - a lane or a wave per case, seen rows in the lanes or in memory, one or several rounds of the searches."""
import functools
import os
import re

import pytest
import torch

import weighted_oracle as wo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc")
SEED = 0x5EED0123456789AB                 # a seed with its high bits set
OFFSET = 1_000_003                        # a non-zero case_offset
N_ITEMS = 200
# seen-row lengths: both sides of the 64-entry switch (rows held in lanes / searched in memory), the empty row, and for every m of
# MS a user with exactly m unseen items (200 - 136 = 64, .., 200 - 199 = 1)
LENGTHS = (0, 1, 64, 65, 136, 137, 176, 198, 199)
MS = (1, 2, 24, 63, 64)
PATTERNS = ("ones", "zipf", "half_zeros", "one_huge", "all_huge")


def _neg():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.negatives


def _source_constant(name, file):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", open(os.path.join(CSRC, file)).read(), flags=re.M)
    assert m, (name, file)
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def _seen_rows():
    g = torch.Generator().manual_seed(N_ITEMS)
    return tuple(tuple(sorted(torch.randperm(N_ITEMS, generator=g)[:n].tolist())) for n in LENGTHS)


def _item_sets(rows, n_items):
    from seoul_tourism_recommendation_ngcf_amd import engine
    users = torch.tensor([u for u, r in enumerate(rows) for _ in r], dtype=torch.int64, device=DEV)
    items = torch.tensor([c for r in rows for c in r], dtype=torch.int64, device=DEV)
    return engine.ItemSets.from_pairs(users, items, len(rows), n_items)


@functools.lru_cache(maxsize=None)
def _sets():
    return _item_sets(_seen_rows(), N_ITEMS)


@functools.lru_cache(maxsize=None)
def _weights(pattern):
    """The weights as a tuple of Python integers."""
    g = torch.Generator().manual_seed(len(pattern))
    if pattern == "ones":
        return (1,) * N_ITEMS
    if pattern == "zipf":                                    # 1000 / rank^0.75 in a random order of the items: ties in the tail
        return tuple(max(1, int(1000 / (r + 1) ** 0.75)) for r in torch.randperm(N_ITEMS, generator=g).tolist())
    if pattern == "half_zeros":
        zero = set(torch.randperm(N_ITEMS, generator=g)[:N_ITEMS // 2].tolist())
        return tuple(0 if i in zero else 1 + i % 5 for i in range(N_ITEMS))
    if pattern == "one_huge":                                # item 77 is in no row's draw but by its 2^40 : 1 odds
        return tuple(2 ** 40 if i == 77 else 1 for i in range(N_ITEMS))
    assert pattern == "all_huge"
    return (2 ** 40,) * N_ITEMS


@functools.lru_cache(maxsize=None)
def _wsets(pattern):
    return _neg().WeightedSets(_sets(), torch.tensor(_weights(pattern), dtype=torch.int64, device=DEV))


def _positive_unseen(pattern, user):
    w, row = _weights(pattern), set(_seen_rows()[user])
    return [i for i in range(N_ITEMS) if i not in row and w[i] > 0]


def _uid(pattern, m, reps=3):
    """Every user with at least m positive-weight unseen items, each `reps` times and not in order."""
    legal = [u for u in range(len(LENGTHS)) if len(_positive_unseen(pattern, u)) >= m]
    assert {0, 1, 2, 3} <= set(legal)                                      # seen rows of 0, 1, 64 and 65 ids in every call
    g = torch.Generator().manual_seed(m)
    return torch.tensor(legal * reps)[torch.randperm(len(legal) * reps, generator=g)]


def check(wsets, weights, rows, uid, m, seed=SEED, case_offset=OFFSET):
    """One call against the oracle: items, weights and masses equal; returns the items."""
    want_items, want_w, want_mass, status = wo.sample(weights, rows, uid.tolist(), m, seed, case_offset)
    assert status == 0
    items, w, mass = _neg().weighted_unseen(wsets, uid.to(DEV), m, seed, case_offset=case_offset, return_weights=True)
    assert items.dtype == w.dtype == mass.dtype == torch.int64
    assert items.shape == w.shape == (uid.numel(), m) and mass.shape == uid.shape
    assert items.cpu().tolist() == want_items
    assert w.cpu().tolist() == want_w and mass.cpu().tolist() == want_mass
    alone = _neg().weighted_unseen(wsets, uid.to(DEV), m, seed, case_offset=case_offset)          # without weights: the items alone
    assert torch.equal(alone, items)
    return items.cpu()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_prepared_arrays_equal_the_oracle(pattern):
    ws, w = _wsets(pattern), _weights(pattern)
    rowptr = _sets().rowptr.cpu().tolist()
    gap, mass = ws.gap.cpu().tolist(), ws.mass.cpu().tolist()
    for u, row in enumerate(_seen_rows()):
        cdf, want_gap, S = wo.prepare(w, row)
        assert ws.cdf.cpu().tolist() == cdf
        assert gap[rowptr[u]:rowptr[u + 1]] == want_gap and mass[u] == cdf[-1] - S[-1]
    assert ws.total == sum(w) and ws.n_rows == len(LENGTHS) and ws.n_items == N_ITEMS


@pytest.mark.parametrize("pattern", PATTERNS)
def test_equal_to_the_oracle(pattern):
    """Every m of MS (a lane per case at m = 1, a wave above) over seen rows of 0, 1, 64, 65 ids and every longer one that leaves
    m positive-weight items: items, draw_weight and case_mass are the oracle's integers."""
    w = _weights(pattern)
    for m in MS:
        uid = _uid(pattern, m)
        items = check(_wsets(pattern), w, _seen_rows(), uid, m)
        for t, u in enumerate(uid.tolist()):
            row = items[t].tolist()
            assert len(set(row)) == m and not set(row) & set(_seen_rows()[u]) and all(w[i] > 0 for i in row)


def test_one_huge_weight_is_drawn_first_by_those_who_have_not_seen_it():
    """2^40 : 1 odds: the heavy item is slot 0 for every user who has not seen it (all but one in 2^32 cases), never for one who has."""
    uid = _uid("one_huge", 2, reps=20)
    items = _neg().weighted_unseen(_wsets("one_huge"), uid.to(DEV), 2, SEED).cpu()
    saw = torch.tensor([77 in _seen_rows()[u] for u in uid.tolist()])
    assert bool(saw.any()) and bool((~saw).any())
    assert bool((items[~saw, 0] == 77).all()) and not bool((items[saw] == 77).any())


@pytest.mark.parametrize("pattern", ["zipf", "half_zeros"])
def test_column_0_is_the_draw_of_one_item(pattern):
    """Slot 0 of the wave-per-case kernel (m > 1) equals the lane-per-case kernel's item (m = 1), case by case."""
    uid = _uid(pattern, 24).to(DEV)
    one = _neg().weighted_unseen(_wsets(pattern), uid, 1, SEED, case_offset=OFFSET, return_weights=True)
    for m in (2, 24):
        many = _neg().weighted_unseen(_wsets(pattern), uid, m, SEED, case_offset=OFFSET, return_weights=True)
        assert torch.equal(many[0][:, :1], one[0]) and torch.equal(many[1][:, :1], one[1]) and torch.equal(many[2], one[2])


@pytest.mark.parametrize("m", [1, 8])
def test_chunks_equal_the_whole_and_runs_repeat(m):
    neg = _neg()
    uid = torch.randint(0, 5, (300,), generator=torch.Generator().manual_seed(3)).to(DEV)          # more than one workgroup of either kernel
    whole = neg.weighted_unseen(_wsets("zipf"), uid, m, SEED, return_weights=True)
    again = neg.weighted_unseen(_wsets("zipf"), uid, m, SEED, return_weights=True)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))                                    # two runs are identical
    out = torch.full((300, m + 3), -7, dtype=torch.int64, device=DEV)                              # a wider table: the leading columns
    parts = [neg.weighted_unseen(_wsets("zipf"), uid[r0:r0 + 128], m, SEED, case_offset=r0, return_weights=True, out=out[r0:r0 + 128])
             for r0 in range(0, 300, 128)]
    for q in range(3):
        assert torch.equal(torch.cat([p[q] for p in parts]), whole[q])
    assert torch.equal(out[:, :m], whole[0]) and bool((out[:, m:] == -7).all()) and parts[0][0].data_ptr() == out.data_ptr()
    shifted = neg.weighted_unseen(_wsets("zipf"), uid, m, SEED, case_offset=1)
    assert not torch.equal(shifted, whole[0])                                                      # the case number is part of the draw
    want = wo.sample(_weights("zipf"), _seen_rows(), uid.tolist(), m, SEED)[0]
    assert whole[0].cpu().tolist() == want


def test_grid_stride_of_the_wave_kernel():
    """Five cases more than one pass of the capped grid takes (cap and waves per workgroup read from the source)."""
    per_pass = _source_constant("NGCF_SAMPLE_BLOCKS_MAX", "sample_device.h") * _source_constant(
        "NGCF_SAMPLE_WEIGHTED_WAVES", "sample_weighted.hip")
    uid = torch.randint(0, 7, (per_pass + 5,), generator=torch.Generator().manual_seed(5))        # users 0..6: at least 24 unseen items
    check(_wsets("zipf"), _weights("zipf"), _seen_rows(), uid, 2)


@pytest.mark.parametrize("m", MS)
def test_exactly_m_items_are_all_drawn_and_one_fewer_is_refused(m):
    neg = _neg()
    user = next(u for u, n in enumerate(LENGTHS) if N_ITEMS - n == m)
    unseen = sorted(set(range(N_ITEMS)) - set(_seen_rows()[user]))
    assert len(unseen) == m
    uid = torch.full((16,), user, dtype=torch.int64)
    items = check(_wsets("zipf"), _weights("zipf"), _seen_rows(), uid, m)
    assert torch.equal(items.sort(1).values, torch.tensor(unseen).expand(16, m))                   # every case draws the whole set
    assert m == 1 or len({tuple(r) for r in items.tolist()}) > 1                                   # .. in another order per case
    # one of the user's unseen items at weight 0: m - 1 are left
    w = list(_weights("zipf"))
    w[unseen[m // 2]] = 0
    short = neg.WeightedSets(_sets(), torch.tensor(w, dtype=torch.int64, device=DEV))
    mixed = torch.tensor([0, user, 3], device=DEV)
    with pytest.raises(ValueError, match=f"fewer than m={m} unseen items of positive weight"):
        neg.weighted_unseen(short, mixed, m, SEED)
    status = torch.full((1,), 8, dtype=torch.int32, device=DEV)
    got = neg.weighted_unseen(short, mixed, m, SEED, return_weights=True, status=status)
    want = wo.sample(w, _seen_rows(), mixed.tolist(), m, SEED)
    assert int(status) == 8 | 2 and want[3] == 2                                                   # OR-ed into, never cleared
    assert got[0].cpu().tolist() == want[0] and got[1].cpu().tolist() == want[1] and got[2].cpu().tolist() == want[2]
    assert got[0][1].tolist() == [-1] * m and got[1][1].tolist() == [0] * m and int(got[0][0].min()) >= 0


@pytest.mark.parametrize("m", [1, 8])
def test_user_ids_outside_the_sets(m):
    neg = _neg()
    good = torch.tensor([0, 3, 2, 1], device=DEV)
    base = neg.weighted_unseen(_wsets("zipf"), good, m, SEED, return_weights=True)
    for bad_user in (-1, len(LENGTHS)):
        uid = torch.tensor([0, 3, bad_user, 1], device=DEV)
        with pytest.raises(IndexError, match="a user id lies outside"):
            neg.weighted_unseen(_wsets("zipf"), uid, m, SEED)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = neg.weighted_unseen(_wsets("zipf"), uid, m, SEED, return_weights=True, status=status)
        assert int(status) == 1
        assert got[0][2].tolist() == [-1] * m and got[1][2].tolist() == [0] * m and int(got[2][2]) == 0
        keep = [0, 1, 3]
        assert all(torch.equal(g[keep], b[keep]) for g, b in zip(got, base))                       # nothing else changes
    assert neg.weighted_unseen(_wsets("zipf"), good[:0], m, SEED).shape == (0, m)                  # no cases: nothing to do


def test_weights_out_of_range_are_refused():
    neg = _neg()
    w = torch.ones(N_ITEMS, dtype=torch.int64, device=DEV)
    for bad, msg in ((torch.zeros_like(w), "sum to 0"), (w.clone().index_fill_(0, torch.tensor([5], device=DEV), -1), "outside \\[0, 2\\^40\\]"),
                     (w.clone().index_fill_(0, torch.tensor([5], device=DEV), 2 ** 40 + 1), "outside \\[0, 2\\^40\\]")):
        with pytest.raises(ValueError, match=msg):
            neg.WeightedSets(_sets(), bad)
    # 2^22 items of 2^40 sum to 2^62: no weight is out of range, the total is
    from seoul_tourism_recommendation_ngcf_amd import engine
    empty = engine.ItemSets(torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), 0, 2 ** 22)
    with pytest.raises(ValueError, match="outside \\[1, 2\\^62\\)"):
        neg.WeightedSets(empty, torch.full((2 ** 22,), 2 ** 40, dtype=torch.int64, device=DEV))
    ok = neg.WeightedSets(empty, torch.full((2 ** 22,), 2 ** 40 - 1, dtype=torch.int64, device=DEV))
    assert ok.total == 2 ** 22 * (2 ** 40 - 1) and ok.mass.tolist() == [ok.total]


# ---- a longer case: a seen row past the lanes and past one round of its search, a cdf past one round ------------------------------
N_LONG = 5000


@functools.lru_cache(maxsize=None)
def _long_world():
    g = torch.Generator().manual_seed(N_LONG)
    rows = (tuple(sorted(torch.randperm(N_LONG, generator=g)[:3000].tolist())), ())
    w = tuple(max(1, int(100000 / (r + 1) ** 0.75)) for r in torch.randperm(N_LONG, generator=g).tolist())
    return rows, w, _neg().WeightedSets(_item_sets(rows, N_LONG), torch.tensor(w, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("m", [1, 64])
def test_long_rows_and_a_long_cdf(m):
    rows, w, wsets = _long_world()
    cdf, gap, S = wo.prepare(w, rows[0])
    assert wsets.gap.cpu().tolist() == gap and wsets.mass.cpu().tolist() == [cdf[-1] - S[-1], cdf[-1]]
    items = check(wsets, w, rows, torch.tensor([0, 1, 1, 0, 0, 1, 0, 1]), m)
    assert not set(items[0].tolist()) & set(rows[0])


# ---- sampling.weighted_negatives / weighted_triplets / WeightedNegativesLoader ------------------------------------------------------
N_USER, N_ITEM, N_POS = 300, 100, 2000


@functools.lru_cache(maxsize=None)
def _positives():
    """Positives with a popular head: item ids are the squares of uniform draws, scaled."""
    g = torch.Generator().manual_seed(11)
    users = torch.randint(0, N_USER, (N_POS,), generator=g)
    items = (torch.rand(N_POS, generator=g) ** 2 * N_ITEM).long().clamp(max=N_ITEM - 1)
    return users.to(DEV), items.to(DEV)


def test_weighted_negatives_and_logq():
    from seoul_tourism_recommendation_ngcf_amd import engine, sampling
    users, items = _positives()
    weights = sampling.popularity_weights(items, N_ITEM)
    assert weights.device == users.device and int(weights.min()) >= 0
    kw = dict(seed=2024, n_user=N_USER, n_item=N_ITEM)
    m = 8
    u, p, neg, logq = sampling.weighted_negatives(users, items, weights, m=m, return_logq=True, **kw)
    assert torch.equal(u, users) and torch.equal(p, items) and neg.shape == logq.shape == (N_POS, m)
    assert neg.dtype == torch.int64 and logq.dtype == torch.float64
    # the oracle's integers; log(w / U_j) with torch's fp64 division and log on the same operands, on the same device
    seen_rows = [[] for _ in range(N_USER)]
    for a, b in sorted(set(zip(users.tolist(), items.tolist()))):
        seen_rows[a].append(b)
    want_items, want_w, want_mass, status = wo.sample(weights.tolist(), seen_rows, users.tolist(), m, sampling.fmix(2024))
    assert status == 0 and neg.cpu().tolist() == want_items
    left = [[U - sum(row[:j]) for j in range(m)] for row, U in zip(want_w, want_mass)]
    want_logq = torch.log(torch.tensor(want_w, dtype=torch.int64, device=DEV).double() / torch.tensor(left, dtype=torch.int64, device=DEV).double())
    assert torch.equal(logq, want_logq) and bool((logq < 0).all())
    # no drawn item is in the user's seen row
    seen = engine.ItemSets.from_pairs(users, items, N_USER, N_ITEM)
    key = torch.unique(users * N_ITEM + items)
    assert not bool(torch.isin(users[:, None] * N_ITEM + neg, key).any())
    # the same through prepared sets; without logq; one negative per row
    wsets = engine.negatives.WeightedSets(seen, weights)
    assert torch.equal(sampling.weighted_negatives(users, items, wsets, m=m, **kw)[2], neg)
    assert torch.equal(sampling.weighted_negatives(users, items, weights, seen, m=m, **kw)[2], neg)
    tri = sampling.weighted_triplets(users, items, wsets, return_logq=True, **kw)
    assert tri[2].shape == tri[3].shape == (N_POS,) and torch.equal(tri[2], neg[:, 0]) and torch.equal(tri[3], logq[:, 0])
    assert len(sampling.weighted_triplets(users, items, weights, **kw)) == 3
    # another epoch: another draw, that of fmix(seed + epoch)
    other = sampling.weighted_negatives(users, items, wsets, m=m, epoch=1, **kw)[2]
    assert not torch.equal(other, neg)
    assert torch.equal(other, engine.negatives.weighted_unseen(wsets, users, m, sampling.fmix(2025)))
    # popular items are drawn more often than the tail: the head quarter of the catalogue takes a quarter of uniform draws (16 000
    # draws: +- 0.004) and, at weights ~ x^-0.375 over the catalogue, about 0.25^0.625 = 0.42 of these
    assert float((neg < N_ITEM // 4).float().mean()) > 0.33


def test_weighted_negatives_loader():
    from seoul_tourism_recommendation_ngcf_amd import sampling
    users, items = _positives()
    weights = sampling.popularity_weights(items, N_ITEM)
    m = 4
    cols = tuple(torch.arange(N_POS, device=DEV) * 10 + q for q in range(7))           # year, u_id, age, sex, month, day, dow
    kw = dict(m=m, seed=99)
    loader = sampling.WeightedNegativesLoader(users, items, weights, cols, batch_size=512, shuffle=False, drop_last=False, **kw)
    shuffled = sampling.WeightedNegativesLoader(users, items, weights, batch_size=512, generator=torch.Generator(device=DEV).manual_seed(4), **kw)
    assert len(loader) == 4 and len(shuffled) == 3 and loader.epoch == 0
    for e in range(2):
        want = sampling.weighted_negatives(users, items, weights, epoch=e, n_user=N_USER, n_item=N_ITEM, **kw)[2]
        batches = list(loader)
        assert loader.epoch == e + 1 and [len(b) for b in batches] == [9] * 4
        assert [int(b[0].numel()) for b in batches] == [512, 512, 512, N_POS - 1536]
        assert all(b[8].shape == (b[0].numel() * m,) and b[8].dtype == torch.int64 for b in batches)
        for q in range(7):
            assert torch.equal(torch.cat([b[q] for b in batches]), cols[q])
        assert torch.equal(torch.cat([b[7] for b in batches]), items)
        assert torch.equal(torch.cat([b[8] for b in batches]).view(N_POS, m), want)
        # shuffled, without columns: (users, items, negatives) of the same epoch under the epoch's permutation
        got = list(shuffled)
        assert all(len(b) == 3 and b[0].shape == (512,) and b[2].shape == (512 * m,) for b in got)
        su, si, sn = torch.cat([b[0] for b in got]), torch.cat([b[1] for b in got]), torch.cat([b[2] for b in got]).view(-1, m)
        assert not torch.equal(su, users[:1536])
        # rows are identified by (user, item, negatives): every served row is a row of the epoch's table
        table = torch.cat((users[:, None], items[:, None], want), 1)
        served = torch.cat((su[:, None], si[:, None], sn), 1)
        assert {tuple(r) for r in served.tolist()} <= {tuple(r) for r in table.tolist()}
        assert len({tuple(r) for r in served.tolist()}) > 1400


@pytest.mark.parametrize("name", ("NegativesLoader", "WeightedNegativesLoader"))
def test_loader_batches_are_the_epochs_draw_at_the_generators_permutation(name):
    """Both loaders with m negatives per row: an unshuffled epoch is the module function's draw of that epoch number, row for row,
    and a shuffled one is that draw at the rows `torch.randperm` gives from an equally seeded device generator."""
    from seoul_tourism_recommendation_ngcf_amd import engine, sampling
    users, items = _positives()
    m, bs = 4, 512
    used = N_POS // bs * bs
    seen = engine.ItemSets.from_pairs(users, items, N_USER, N_ITEM)
    kw = dict(m=m, seed=99)
    if name == "NegativesLoader":
        make = lambda **options: sampling.NegativesLoader(users, items, batch_size=bs, seen=seen, **kw, **options)  # noqa: E731
        draw = lambda e: sampling.train_negatives(users, items, seen, epoch=e, n_user=N_USER, n_item=N_ITEM, **kw)[2]  # noqa: E731
    else:
        weights = sampling.popularity_weights(items, N_ITEM)
        make = lambda **options: sampling.WeightedNegativesLoader(users, items, weights, batch_size=bs, seen=seen, **kw, **options)  # noqa: E731
        draw = lambda e: sampling.weighted_negatives(users, items, weights, seen, epoch=e, n_user=N_USER, n_item=N_ITEM, **kw)[2]  # noqa: E731
    ordered = make(shuffle=False, drop_last=False)
    shuffled = make(generator=torch.Generator(device=DEV).manual_seed(4))
    again = torch.Generator(device=DEV).manual_seed(4)
    for e in range(2):
        want = draw(e)
        got = list(ordered)
        assert ordered.epoch == e + 1 and [int(b[0].numel()) for b in got] == [bs] * (N_POS // bs) + [N_POS - used]
        assert torch.equal(torch.cat([b[0] for b in got]), users) and torch.equal(torch.cat([b[1] for b in got]), items)
        assert torch.equal(torch.cat([b[2] for b in got]).view(N_POS, m), want)
        rows = torch.randperm(N_POS, generator=again, device=DEV)[:used]
        got = list(shuffled)
        assert len(got) == used // bs
        assert torch.equal(torch.cat([b[0] for b in got]), users[rows]) and torch.equal(torch.cat([b[1] for b in got]), items[rows])
        assert torch.equal(torch.cat([b[2] for b in got]).view(used, m), want[rows])
