"""Inputs of the Laplacian-builder tests (tests/test_laplacian_build_gpu.py), built on the host from seeds, and the checks that an
input really contains what it was built for - run against the torch builder on the CPU before a device result is compared."""
import numpy as np
import torch

# (year, user, item, rating): three years interleaved, a year-19 record first, so the years are taken as 19, 18, 20.
# 6 users x 7 items; user 5 and item 6 never appear.
SEMANTICS_DIMS = (6, 7)
UNDERFLOW = 1.4e-45                                   # the smallest float32 denormal
SEMANTICS_RECORDS = [
    (19, 0, 0, 1.0),
    (18, 1, 1, 2.0),
    (19, 4, 5, UNDERFLOW),                            # year 19: user 4 has degree 2, item 5 degree 3: the value underflows to 0
    (20, 2, 2, 3.0),
    (19, 4, 0, 0.5),
    (19, 0, 5, 2.5),
    (19, 1, 5, 1.5),
    (18, 4, 0, 0.0),                                  # 0.0 deletes a carried-over edge (user 4: degree 1 in year 18)
    (18, 0, 5, -0.0),                                 # -0.0 deletes a carried-over edge (item 5: degree 2 in year 18)
    (19, 2, 3, 1.0),                                  # one pair three times in one year: the last rating stands
    (19, 2, 3, 4.0),
    (19, 2, 3, 2.0),
    (20, 2, 3, 7.0),                                  # re-rated in a later year
    (19, 3, 1, 1.0),
    (19, 3, 2, 2.0),
    (18, 3, 1, 0.0),                                  # user 3 loses every edge in year 18 ...
    (18, 3, 2, -0.0),
    (20, 1, 4, 5.0),
    (20, 1, 4, 0.0),                                  # 0.0 deletes an edge of the same year
    (20, 0, 3, 2.0),
    (20, 0, 3, -0.0),                                 # -0.0 deletes an edge of the same year
    (18, 0, 1, 0.25),
    (18, 2, 0, 0.75),
    (20, 3, 4, 1.25),                                 # ... and comes back in year 20
    (19, 1, 0, 3.5),
    (18, 1, 2, 0.0),                                  # deleting what is not there
    (20, 4, 1, 2.25),
    (19, 0, 2, 1.75),
    (18, 0, 2, 9.0),
    (20, 0, 0, 0.0),
    (19, 1, 3, 0.0),                                  # deleted, then set again in the same year
    (19, 1, 3, 6.0),
    (18, 2, 4, 1.0),
    (20, 2, 4, 8.0),
    (18, 2, 2, 3.0),
    (20, 1, 1, -0.0),
    (19, 2, 1, 0.125),
    (18, 1, 0, 4.5),
    (20, 4, 5, 1.0),
    (18, 0, 4, 1.0),
]


def semantics_input():
    rec = SEMANTICS_RECORDS
    return (np.array([r[0] for r in rec], dtype=np.int64), np.array([r[1] for r in rec], dtype=np.int64),
            np.array([r[2] for r in rec], dtype=np.int64), np.array([r[3] for r in rec], dtype=np.float32))


def branch_point_input(wave_limit: int, group_limit: int, seed: int = 20240911):
    """Two years (18 then 19).  For every count c in {L - 1, L, L + 1 : L = 1, wave_limit, group_limit} one user whose row has c
    candidates in year 19 from the state only (c entries set in year 18, no record in 19), one from new records only (c records in
    year 19, none before) and one mixed (c // 2 entries from year 18, the rest records of year 19, half of them re-rating or
    deleting items the user has); counts too small for a mode are left out.  One more user's year-19 bucket holds every item twice
    (2 * n_item records, more candidates than n_item; about twice the workgroup limit, since n_item has to exceed it for the
    counts above).  300 random users fill in around them.  Returns `(year, userid, itemid, rating, n_user, n_item, plan)`, plan =
    [(user, mode, c)], everything shuffled with a year-18 record first."""
    rng = np.random.default_rng(seed)
    n_item = group_limit + 52
    counts = sorted({c for L in (1, wave_limit, group_limit) for c in (L - 1, L, L + 1)})
    rec, plan, user = [], [], 0

    def rate(n):
        return rng.uniform(0.5, 5.0, n).astype(np.float32)

    def add(y, u, items, ratings):
        rec.extend((y, u, int(i), float(r)) for i, r in zip(items, ratings))

    for c in counts:
        if c >= 1:
            add(18, user, rng.choice(n_item, c, replace=False), rate(c))
            plan.append((user, "old", c))
            user += 1
            add(19, user, rng.choice(n_item, c, replace=False), rate(c))
            plan.append((user, "new", c))
            user += 1
        else:
            plan.append((user, "none", 0))                          # a user that never appears
            user += 1
        if c >= 2:
            a = c // 2
            old_items = rng.choice(n_item, a, replace=False)
            add(18, user, old_items, rate(a))
            b = c - a
            again = rng.choice(old_items, min(b // 2, a), replace=False)               # re-rated or deleted
            fresh = rng.choice(np.setdiff1d(np.arange(n_item), old_items), b - again.size, replace=False)
            r_again = rate(again.size)
            r_again[::3] = 0.0
            r_again[1::7] = -0.0
            add(19, user, np.concatenate([again, fresh]), np.concatenate([r_again, rate(fresh.size)]))
            plan.append((user, "mixed", c))
            user += 1
    long_user = user
    add(18, user, rng.choice(n_item, 40, replace=False), rate(40))
    twice = np.concatenate([rng.permutation(n_item), rng.permutation(n_item)])
    r_twice = rate(twice.size)
    r_twice[::5] = 0.0
    add(19, user, twice, r_twice)
    plan.append((user, "long", 40 + 2 * n_item))
    user += 1
    for _ in range(300):
        for y in (18, 19):
            n = int(rng.integers(0, 41))
            r = rate(n)
            r[rng.random(n) < 0.1] = 0.0
            add(y, user, rng.integers(0, n_item, n), r)             # repeats allowed
        user += 1
    n_user = user + 1                                               # and one user that never appears at the end
    order = rng.permutation(len(rec))
    first18 = int(np.flatnonzero(np.array([rec[k][0] for k in order]) == 18)[0])
    order[[0, first18]] = order[[first18, 0]]
    rec = [rec[k] for k in order]
    cols = (np.array([r[0] for r in rec], dtype=np.int64), np.array([r[1] for r in rec], dtype=np.int64),
            np.array([r[2] for r in rec], dtype=np.int64), np.array([r[3] for r in rec], dtype=np.float32))
    assert plan[-1][0] == long_user
    return cols + (n_user, n_item, plan)


def check_branch_point_plan(oracle, year, userid, plan, n_user, n_item, wave_limit, group_limit):
    """The planned users have the planned candidate counts in year 19: entries of the user's row in the oracle's year-18 slice (= the
    state; the ratings are far from underflow) plus records of year 19.  And the counts straddle both limits."""
    rows18 = oracle[0][0].cpu().numpy()
    state = np.bincount(rows18[rows18 < n_user], minlength=n_user)
    new = np.bincount(userid[year == 19], minlength=n_user)
    seen = set()
    for u, mode, c in plan:
        assert state[u] + new[u] == c, (u, mode, c, state[u], new[u])
        assert {"old": new[u] == 0, "new": state[u] == 0, "none": c == 0}.get(mode, state[u] > 0 and new[u] > 0), (u, mode)
        seen.add((mode, c))
    for L in (1, wave_limit, group_limit):
        for c in (L - 1, L, L + 1):
            for mode in ("old", "new", "mixed"):
                if c >= (2 if mode == "mixed" else 1):
                    assert (mode, c) in seen, (mode, c)
    assert plan[-1][1] == "long" and new[plan[-1][0]] == 2 * n_item > group_limit           # more candidates than items


def unique_pairs_input(n_user=500, n_item=300, per_year=8000, seed=77):
    """Two years without a repeated (user, item) inside a year (years do overlap), some zero ratings, shuffled, year 18 first."""
    rng = np.random.default_rng(seed)
    ys, us, its, rs = [], [], [], []
    for y in (18, 19):
        keys = rng.choice(n_user * n_item, per_year, replace=False)
        r = rng.uniform(0.5, 5.0, per_year).astype(np.float32)
        r[rng.random(per_year) < 0.05] = 0.0
        ys.append(np.full(per_year, y, dtype=np.int64))
        us.append(keys // n_item)
        its.append(keys % n_item)
        rs.append(r)
    year, userid, itemid, rating = (np.concatenate(a) for a in (ys, us, its, rs))
    order = permutation_first_year_first(year, rng)
    return year[order], userid[order].astype(np.int64), itemid[order].astype(np.int64), rating[order], n_user, n_item


def permutation_first_year_first(year, rng):
    """A random order of the records whose first record is of the year that comes first now."""
    order = rng.permutation(year.size)
    k = int(np.flatnonzero(year[order] == year[0])[0])
    order[[0, k]] = order[[k, 0]]
    return order


def oracle_slices(year, userid, itemid, rating, n_user, n_item):
    from seoul_tourism_recommendation_ngcf_amd.matrix import laplacian_slices
    return laplacian_slices(year, userid, itemid, rating, n_user, n_item, device="cpu")


def assert_slices_equal(got, want):
    """got: {idx: LaplacianSlice} from the device; want: {idx: (rows, cols, vals)} on the CPU.  Bit for bit."""
    assert sorted(got) == sorted(want)
    for k in want:
        rows, cols, vals = (t.cpu() for t in got[k].coo())
        assert rows.dtype == torch.int64 and cols.dtype == torch.int64 and vals.dtype == torch.float32
        assert torch.equal(rows, want[k][0]), k
        assert torch.equal(cols, want[k][1]), k
        assert np.array_equal(vals.numpy().view(np.uint32), want[k][2].numpy().view(np.uint32)), k
