"""Hard negatives on the device (ngcf_sample_hard_f32, engine.negatives.hard_unseen, sampling.hard_triplets / HardTripletLoader):
item, slot and score bits EQUAL to the composition of the two tested kernels - engine.sample_unseen, then engine.eval_candidates'
scores, then a host-side argmax under the documented order - on every path of the kernel, plus the properties that lean on
neither: a brute-force argmax where the whole unseen set is drawn, and an fp64 bound on random tables."""
import functools
import os
import re

import pytest
import torch

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
DS = (1, 3, 4, 5, 63, 64, 65, 130, 515)


def _eng():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine


def _source_constant(name, file):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", open(os.path.join(CSRC, file)).read(), flags=re.M)
    assert m, (name, file)
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def _seen_rows():
    g = torch.Generator().manual_seed(N_ITEMS)
    return tuple(tuple(sorted(torch.randperm(N_ITEMS, generator=g)[:n].tolist())) for n in LENGTHS)


@functools.lru_cache(maxsize=None)
def _sets():
    rows = _seen_rows()
    users = torch.tensor([u for u, r in enumerate(rows) for _ in r], dtype=torch.int64, device=DEV)
    items = torch.tensor([c for r in rows for c in r], dtype=torch.int64, device=DEV)
    return _eng().ItemSets.from_pairs(users, items, len(rows), N_ITEMS)


@functools.lru_cache(maxsize=None)
def _tables(D, seed=0):
    """(user_emb, item_emb) N(0,1), contiguous, and the same values as column slices at an odd offset of wider tensors: rows that are
    not 16-byte aligned, so the dword loads run."""
    g = torch.Generator().manual_seed(1000 * D + seed)
    U = torch.randn(len(LENGTHS), D, generator=g).to(DEV)
    I = torch.randn(N_ITEMS, D, generator=g).to(DEV)
    wide_u = torch.full((len(LENGTHS), D + 3), 7.0, device=DEV)
    wide_i = torch.full((N_ITEMS, D + 3), 7.0, device=DEV)
    wide_u[:, 1:1 + D] = U
    wide_i[:, 1:1 + D] = I
    return U, I, wide_u[:, 1:1 + D], wide_i[:, 1:1 + D]


def _aligned_slice(t):
    """The same values as the leading columns of a tensor whose row pitch is a multiple of 4 floats: 16-byte aligned rows of any
    width, so the float4 loads run and the last quad of a width that is no multiple of 4 is read element by element."""
    wide = torch.full((t.shape[0], (t.shape[1] + 3) // 4 * 4 + 4), 7.0, device=t.device)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def _uid(m, reps=3):
    """Every user with at least m unseen items, each `reps` times and not in order."""
    legal = [u for u, n in enumerate(LENGTHS) if N_ITEMS - n >= m]
    assert {0, 1, 2, 3} <= set(legal) and (m not in MS or any(N_ITEMS - LENGTHS[u] == m for u in legal))   # lengths 0, 1, 64, 65 and n == m in one call
    g = torch.Generator().manual_seed(m)
    return torch.tensor(legal * reps)[torch.randperm(len(legal) * reps, generator=g)].to(DEV)


def float_key(bits):
    """The project's order on fp32 bits (csrc/common.h, float_key) as int64: larger float = larger key, NaN above +inf."""
    u = bits.to(torch.int64) & 0xFFFFFFFF
    return torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)


def oracle(sets, U, I, uid, m, seed=SEED, case_offset=OFFSET):
    """(neg, slot, score bits, candidates) of the composition: the draw, the candidate evaluation's scores, and on the host the
    largest key per row with ties to the lowest column."""
    eng = _eng()
    cand = eng.sample_unseen(sets, uid, m, seed, case_offset=case_offset)
    scores = eng.eval_candidates(U, I, uid, cand, ks=(), hit_k=1, return_scores=True)[2]
    bits = scores.view(torch.int32).cpu()
    word = float_key(bits) * 64 + (63 - torch.arange(m))                   # unique per row: the largest is the winner
    win = word.argmax(1, keepdim=True)
    return cand.cpu().gather(1, win)[:, 0], win[:, 0].to(torch.int32), bits.gather(1, win)[:, 0], cand.cpu()


def check(sets, U, I, uid, m, seed=SEED, case_offset=OFFSET, oracle_tables=None):
    """One fused call against the oracle: item, slot and score bits equal."""
    want_neg, want_slot, want_bits, cand = oracle(sets, *(oracle_tables or (U, I)), uid, m, seed, case_offset)
    neg, score, slot = _eng().negatives.hard_unseen(sets, U, I, uid, m, seed, case_offset=case_offset, return_score=True, return_slot=True)
    assert neg.dtype == torch.int64 and score.dtype == torch.float32 and slot.dtype == torch.int32
    assert neg.shape == score.shape == slot.shape == uid.shape
    assert torch.equal(slot.cpu(), want_slot)
    assert torch.equal(neg.cpu(), want_neg)
    assert torch.equal(score.view(torch.int32).cpu(), want_bits)
    return neg.cpu(), slot.cpu(), score.cpu(), cand


@pytest.mark.parametrize("D", DS)
def test_bit_equal_to_the_composition(D):
    """Every m of MS (seen rows of 0, 1, 64, 65 ids and a user with exactly m unseen items in each call) at widths on both sides of a
    quad, of one pass of a 16-lane group (64 floats) and of two; float4 loads on the contiguous tables, dword loads on the
    column slices - which must give the contiguous tables' bits."""
    U, I, Us, Is = _tables(D)
    assert I.data_ptr() % 16 == 0 and (Is.data_ptr() % 16 != 0 or Is.stride(0) % 4 != 0) and not Is.is_contiguous()
    for m in MS:
        uid = _uid(m)
        neg, slot, score, cand = check(_sets(), U, I, uid, m)
        check(_sets(), Us, Is, uid, m, oracle_tables=(U, I))
        Ia = _aligned_slice(I)
        assert Ia.data_ptr() % 16 == 0 and Ia.stride(0) % 4 == 0
        check(_sets(), U, Ia, uid, m, oracle_tables=(U, I))
        plain = _eng().negatives.hard_unseen(_sets(), U, I, uid, m, SEED, case_offset=OFFSET)       # without score and slot: the item alone
        assert torch.equal(plain.cpu(), neg)
        if m == 1:
            assert torch.equal(slot, torch.zeros_like(slot)) and torch.equal(neg, cand[:, 0])


@pytest.mark.parametrize("T", [1, 5])
def test_few_cases(T):
    U, I, Us, Is = _tables(65)
    for m in (2, 24):
        check(_sets(), U, I, _uid(m)[:T].contiguous(), m)
        check(_sets(), Us, Is, _uid(m)[:T].contiguous(), m, oracle_tables=(U, I))


@pytest.mark.parametrize("where", ["last_in_lds", "first_in_memory"])
def test_user_row_at_the_lds_budget(where):
    """The widest user row a wave stages in its LDS, and the first multiple of 4 past it, which is read from global memory: the same
    bits as the composition on both sides (T = 3)."""
    budget = _source_constant("NGCF_CAND_LDS_FLOATS", "cand_device.h")
    D = budget if where == "last_in_lds" else budget + 4
    U, I, Us, Is = _tables(D)
    uid = _uid(24)[:3].contiguous()
    check(_sets(), U, I, uid, 24)
    check(_sets(), Us, Is, uid, 24, oracle_tables=(U, I))


def test_grid_stride():
    """Five cases more than one pass of the capped grid takes (cap and waves per workgroup read from the source)."""
    per_pass = _source_constant("NGCF_SAMPLE_BLOCKS_MAX", "sample_device.h") * _source_constant("NGCF_SAMPLE_HARD_WAVES", "sample_hard.hip")
    T = per_pass + 5
    U, I, _, _ = _tables(4)
    uid = torch.randint(0, 7, (T,), generator=torch.Generator().manual_seed(5)).to(DEV)       # users 0..6: at least 2 unseen items
    neg, slot, _, _ = check(_sets(), U, I, uid, 2)
    assert set(slot.tolist()) == {0, 1} and int(neg.min()) >= 0


@pytest.mark.parametrize("m", MS)
def test_whole_unseen_set_is_a_brute_force_argmax(m):
    """The user with exactly m unseen items draws all of them, so the winner is the best unseen item outright: an argmax over the
    user's unseen items in fp64 on the host.  Scores separated by construction: user row e_0, item i's row (p(i) / 2, 0, 0, 0) with
    p a permutation - exact in fp32 and pairwise different."""
    user = next(u for u, n in enumerate(LENGTHS) if N_ITEMS - n == m)
    g = torch.Generator().manual_seed(m)
    U = torch.zeros(len(LENGTHS), 4)
    U[:, 0] = 1.0
    I = torch.zeros(N_ITEMS, 4)
    I[:, 0] = torch.randperm(N_ITEMS, generator=g).double().sub(N_ITEMS // 2).div(2).float()
    unseen = torch.tensor(sorted(set(range(N_ITEMS)) - set(_seen_rows()[user])))
    assert unseen.numel() == m
    best = unseen[(I.double()[unseen] @ U.double()[user]).argmax()]
    uid = torch.full((16,), user, dtype=torch.int64, device=DEV)
    neg, slot, score, cand = check(_sets(), U.to(DEV), I.to(DEV), uid, m)
    assert torch.equal(cand.sort(1).values, unseen.expand(16, m))                                  # every case draws the whole set
    assert torch.equal(neg, best.expand(16)) and torch.equal(score, I[best, 0].expand(16))
    assert m == 1 or len(set(slot.tolist())) > 1                                                   # .. in another order per case


@functools.lru_cache(maxsize=None)
def _order_world():
    """Nine items under one user row u = (2^-100, ..) of 64 floats, and users who see different parts of them:
    items 0, 1 share one row A (a tie); 2 holds a NaN with the sign bit clear, which the arithmetic passes on (a NaN score); 3 holds
    one +inf (+inf score); 4 is all zeros (+0.0); 5 is all -2^-100: every product underflows to -0.0 in every lane, so the score is
    -0.0; 6, 7 = A - 1, A - 2 score below A; 8 holds +inf and -inf in two lanes' quads, which the butterfly adds: the NaN that the
    hardware makes of an invalid operation, whatever its sign."""
    D = 64
    A = torch.randn(D, generator=torch.Generator().manual_seed(8))
    I = torch.zeros(9, D)
    I[0] = I[1] = A
    I[2, 0] = torch.tensor(0x7FC00000, dtype=torch.int32).view(torch.float32)
    I[3, 0] = float("inf")
    I[5] = -(2.0 ** -100)
    I[6], I[7] = A - 1, A - 2
    I[8, 0], I[8, 16] = float("inf"), float("-inf")
    seen = ((), (2, 8), (2, 3, 8), (0, 1, 2, 3, 6, 7, 8), (2, 3, 4, 5, 8))
    U = torch.full((len(seen), D), 2.0 ** -100)
    users = torch.tensor([u for u, r in enumerate(seen) for _ in r], dtype=torch.int64, device=DEV)
    items = torch.tensor([c for r in seen for c in r], dtype=torch.int64, device=DEV)
    return _eng().ItemSets.from_pairs(users, items, len(seen), 9), U.to(DEV), I.to(DEV), seen


def test_order_rules():
    """The order is float_key's on the score bits: NaN (sign bit clear) above +inf above the finite scores, +0.0 above -0.0, and equal
    bits to the lowest slot - each against the oracle, and against what the rule says outright from every item's score on its own."""
    sets, U, I, seen = _order_world()
    reps = 16
    alone = _eng().eval_candidates(U, I, torch.zeros(1, dtype=torch.int64, device=DEV), torch.arange(9, device=DEV)[None], ks=(), hit_k=1,
                                   return_scores=True)[2][0].cpu()
    alone_bits = alone.view(torch.int32)
    assert bool(alone[[2, 8]].isnan().all()) and float(alone[3]) == float("inf")
    assert int(alone_bits[4]) == 0 and int(alone_bits[5]) == -2 ** 31 and int(alone_bits[0]) == int(alone_bits[1])   # +0.0, -0.0, the tie
    assert bool(alone[[0, 1, 6, 7]].isfinite().all()) and float(alone[0]) > float(alone[6]) > float(alone[7])
    keys = float_key(alone_bits)
    for user, row in enumerate(seen):
        uid = torch.full((reps,), user, dtype=torch.int64, device=DEV)
        full = 9 - len(row)
        for m in sorted({2, full}):
            neg, slot, score, cand = check(sets, U, I, uid, m)
            if m != full:
                continue
            assert len({tuple(r) for r in cand.tolist()}) > 1                     # the whole unseen set, in several orders
            unseen = [i for i in range(9) if i not in row]
            top = max(unseen, key=lambda i: int(keys[i]))
            assert set(neg.tolist()) <= {i for i in unseen if int(keys[i]) == int(keys[top])}
            if user == 0:                                                          # a NaN with the sign bit clear is above +inf, one with it set below -inf
                print("NaN score bits: passed on", hex(int(alone_bits[2]) & 0xFFFFFFFF), "made by inf - inf", hex(int(alone_bits[8]) & 0xFFFFFFFF))
                assert top == 3 if int(alone_bits[2]) < 0 and int(alone_bits[8]) < 0 else top in (2, 8)
                assert bool(score.isnan().all()) == (top != 3)
            if user == 1:
                assert top == 3 and torch.equal(score, torch.full((reps,), float("inf"))) and set(neg.tolist()) == {3}
            if user == 3:                                                          # only +0.0 and -0.0 are left
                assert top == 4 and set(neg.tolist()) == {4} and set(score.view(torch.int32).tolist()) == {0}
            if user == 4:                                                          # the tie of items 0 and 1: whichever was drawn first
                first = (cand == 0).int().argmax(1), (cand == 1).int().argmax(1)
                assert torch.equal(slot.long(), torch.minimum(*first)) and set(neg.tolist()) == {0, 1}


def test_choice_is_the_fp64_maximum_within_the_dot_product_bound():
    """Independent of the score recipe: on N(0,1) tables the chosen candidate's fp64 score is at least the row's fp64 maximum minus
    2 (D + 6) 2^-24 sum_k |u_k| max_j |i_jk| - the standard bound (n + log2-depth terms, unit roundoff 2^-24) on an fp32 dot
    product of D terms followed by a 4-step butterfly, once for each of the two scores compared."""
    D, m = 130, 24
    U, I, _, _ = _tables(D, seed=1)
    uid = _uid(m, reps=8)
    eng = _eng()
    cand = eng.sample_unseen(_sets(), uid, m, SEED, case_offset=OFFSET).cpu()
    neg = eng.negatives.hard_unseen(_sets(), U, I, uid, m, SEED, case_offset=OFFSET).cpu()
    u64, i64 = U.double().cpu()[uid.cpu()], I.double().cpu()[cand]                       # [T, D], [T, m, D]
    s64 = torch.einsum("td,tmd->tm", u64, i64)
    bound = 2 * (D + 6) * 2.0 ** -24 * (u64.abs() * i64.abs().amax(1)).sum(1)
    assert bool((cand == neg[:, None]).sum(1).eq(1).all())                               # the choice is one of the row's draws
    chosen = s64.gather(1, (cand == neg[:, None]).int().argmax(1, keepdim=True))[:, 0]
    print("largest shortfall", float((s64.amax(1) - chosen).max()), "smallest bound", float(bound.min()))
    assert bool((chosen >= s64.amax(1) - bound).all())
    assert bool((chosen == s64.amax(1)).float().mean() > 0.9)                            # and nearly always the maximum itself


def test_chunks_equal_the_whole():
    U, I, _, _ = _tables(65)
    eng = _eng()
    uid = torch.randint(0, 5, (300,), generator=torch.Generator().manual_seed(3)).to(DEV)
    whole = eng.negatives.hard_unseen(_sets(), U, I, uid, 8, SEED, return_score=True, return_slot=True)
    out = torch.empty(300, dtype=torch.int64, device=DEV)
    parts = [eng.negatives.hard_unseen(_sets(), U, I, uid[r0:r0 + 128], 8, SEED, case_offset=r0, return_score=True, return_slot=True,
                                       out=out[r0:r0 + 128]) for r0 in range(0, 300, 128)]
    for q in range(3):
        assert torch.equal(torch.cat([p[q] for p in parts]), whole[q])
    assert torch.equal(out, whole[0]) and parts[0][0].data_ptr() == out.data_ptr()
    shifted = eng.negatives.hard_unseen(_sets(), U, I, uid, 8, SEED, case_offset=1)
    assert not torch.equal(shifted, whole[0])                                            # the case number is part of the draw


def test_status_bits_and_exceptions():
    eng = _eng()
    U, I, _, _ = _tables(65)
    good = torch.tensor([0, 3, 2, 1], device=DEV)
    base = eng.negatives.hard_unseen(_sets(), U, I, good, 8, SEED, return_score=True, return_slot=True)
    with pytest.raises(IndexError, match="a user id lies outside"):
        eng.negatives.hard_unseen(_sets(), U, I, torch.tensor([0, len(LENGTHS)], device=DEV), 8, SEED)
    with pytest.raises(IndexError, match="a user id lies outside"):
        eng.negatives.hard_unseen(_sets(), U, I, torch.tensor([-1, 0], device=DEV), 8, SEED)
    with pytest.raises(ValueError, match="fewer than m=8 unseen items"):
        eng.negatives.hard_unseen(_sets(), U, I, torch.tensor([0, 7], device=DEV), 8, SEED)          # user 7 has 2 unseen items
    for bad_user, bit in ((len(LENGTHS), 1), (-5, 1), (7, 2)):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        uid = torch.tensor([0, 3, bad_user, 1], device=DEV)
        neg, score, slot = eng.negatives.hard_unseen(_sets(), U, I, uid, 8, SEED, return_score=True, return_slot=True, status=status)
        assert int(status) == bit
        assert int(neg[2]) == -1 and int(slot[2]) == -1 and bool(score[2].isnan())
        keep = [0, 1, 3]
        for got, want in zip((neg, score.view(torch.int32), slot), (base[0], base[1].view(torch.int32), base[2])):
            assert torch.equal(got[keep], want[keep])                                    # the good rows of the same call: unchanged
        status.fill_(4)
        eng.negatives.hard_unseen(_sets(), U, I, uid, 8, SEED, status=status)
        assert int(status) == 4 | bit                                                    # OR-ed into, never cleared
    assert eng.negatives.hard_unseen(_sets(), U, I, good[:0], 8, SEED).shape == (0,)       # no cases: nothing to do


def test_tables_that_require_grad_are_detached():
    U, I, _, _ = _tables(65)
    uid = _uid(8)
    want = _eng().negatives.hard_unseen(_sets(), U, I, uid, 8, SEED)
    got = _eng().negatives.hard_unseen(_sets(), U.clone().requires_grad_(), I.clone().requires_grad_(), uid, 8, SEED)
    assert torch.equal(got, want) and not got.requires_grad


# ---- sampling.hard_triplets / HardTripletLoader -------------------------------------------------------------------------------------
N_USER, N_ITEM, N_POS = 300, 100, 2000


@functools.lru_cache(maxsize=None)
def _positives():
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, N_USER, (N_POS,), generator=g).to(DEV), torch.randint(0, N_ITEM, (N_POS,), generator=g).to(DEV)


@functools.lru_cache(maxsize=None)
def _random_tables():
    g = torch.Generator().manual_seed(12)
    return torch.randn(N_USER, 65, generator=g).to(DEV), torch.randn(N_ITEM, 65, generator=g).to(DEV)


def test_hard_triplets_invariants():
    from seoul_tourism_recommendation_ngcf_amd import sampling
    users, items = _positives()
    U, I = _random_tables()
    kw = dict(seed=2024, n_user=N_USER, n_item=N_ITEM)
    # m = 1 is train_triplets, whatever the tables
    want = sampling.train_triplets(users, items, epoch=3, **kw)
    got = sampling.hard_triplets(users, items, U, I, m=1, epoch=3, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # m = 8: an element of the row of sample_unseen under seed_e, and the same tensors on a second run
    seen = _eng().ItemSets.from_pairs(users, items, N_USER, N_ITEM)
    u, p, neg = sampling.hard_triplets(users, items, U, I, seen, epoch=0, **kw)
    assert torch.equal(u, users) and torch.equal(p, items) and neg.dtype == torch.int64 and neg.shape == users.shape
    rows = _eng().sample_unseen(seen, users, 8, sampling.fmix(2024 + 0))
    assert bool((rows == neg[:, None]).sum(1).eq(1).all())
    again = sampling.hard_triplets(users, items, U, I, seen, epoch=0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, (u, p, neg)))
    assert torch.equal(sampling.hard_triplets(users, items, U, I, **kw)[2], neg)          # the default sets are the positives' own
    # they are the hard ones: never below the uniform draw (column 0 of the same rows), and above it for most rows
    score = lambda it: (U[users] * I[it]).sum(1)  # noqa: E731
    assert bool((score(neg) >= score(rows[:, 0]) - 1e-4).all()) and float((score(neg) > score(rows[:, 0])).float().mean()) > 0.5
    # another epoch: another draw; chunks: the same draw
    other = sampling.hard_triplets(users, items, U, I, seen, epoch=1, **kw)[2]
    assert not torch.equal(other, neg)
    assert bool((_eng().sample_unseen(seen, users, 8, sampling.fmix(2024 + 1)) == other[:, None]).any(1).all())
    for chunk in (1999, 700, 5000):
        assert torch.equal(sampling.hard_triplets(users, items, U, I, seen, chunk=chunk, **kw)[2], neg)
    with pytest.raises(ValueError, match="chunk"):
        sampling.hard_triplets(users, items, U, I, seen, chunk=0, **kw)


def test_hard_triplet_loader_over_a_models_tables():
    """Two epochs over a tiny model's propagated tables (views of all_E that require grad): unshuffled, the batches' rows are
    hard_triplets(epoch=e); shuffled, the same rows in another order."""
    import seoul_tourism_recommendation_ngcf_amd as pkg
    from seoul_tourism_recommendation_ngcf_amd import sampling
    torch.manual_seed(0)
    lap = pkg.graphs.to_sparse_coo(pkg.graphs.synthetic_bipartite(N_USER, N_ITEM, 3000, seed=1, device=DEV))
    num_dict = {"user": N_USER, "item": N_ITEM, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    model = pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, [lap], num_dict, 64, DEV).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    B = 64
    batch = dict(year=torch.full((B,), 18), u_id=torch.randperm(N_USER, generator=g)[:B], age=torch.randint(0, 76, (B,), generator=g),
                 sex=torch.randint(0, 2, (B,), generator=g), month=torch.randint(0, 13, (B,), generator=g),
                 day=torch.randint(0, 32, (B,), generator=g), dow=torch.randint(0, 7, (B,), generator=g),
                 pos_item=torch.randint(0, N_ITEM, (B,), generator=g), neg_item=torch.randint(0, N_ITEM, (B,), generator=g))
    model(node_flag=False, **{k: v.to(DEV) for k, v in batch.items()})                   # a propagation: sets the tables
    served = []

    def tables():
        served.append(1)
        return model.all_users_emb, model.all_items_emb
    assert model.all_users_emb.shape[0] == N_USER and model.all_items_emb.shape[0] == N_ITEM
    users, items = _positives()
    kw = dict(m=8, seed=99)
    loader = sampling.HardTripletLoader(users, items, batch_size=512, tables=tables, shuffle=False, drop_last=False, **kw)
    shuffled = sampling.HardTripletLoader(users, items, batch_size=512, tables=tables, generator=torch.Generator(device=DEV).manual_seed(4), **kw)
    assert len(loader) == 4 and len(shuffled) == 3
    for e in range(2):
        want = sampling.hard_triplets(users, items, *tables(), epoch=e, n_user=N_USER, n_item=N_ITEM, **kw)
        got = [torch.cat(c) for c in zip(*loader)]
        assert loader.epoch == e + 1 and len(got) == 3
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        rows = torch.stack([torch.cat(c) for c in zip(*shuffled)], 1)                    # [1536, 3]: a subset of the epoch's rows, reordered
        assert rows.shape == (1536, 3) and not torch.equal(rows[:, 0], users[:1536])
        key = lambda t: (t[:, 0] * N_ITEM + t[:, 1]) * N_ITEM + t[:, 2]  # noqa: E731
        assert bool(torch.isin(key(rows), key(torch.stack(want, 1))).all())
    assert len(served) == 2 * 3                                                          # one tables() per iter(), and the test's own
