"""The draw of unseen items (ngcf_sample_unseen) in pure Python integers for the sampling tests.  It shares no code with
the library: a dict for the sparse Fisher-Yates map, a linear count for the rank -> item step."""

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
STEP = 0xD1B54A32D192ED03


def fmix(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def ranks(t, seed, n, m):
    """The m distinct ranks in [0, n) of global case t: an ordered uniform sample without replacement."""
    assert 1 <= m <= n
    a = fmix((seed & M64) ^ ((t * GOLDEN) & M64))
    swapped, out = {}, []
    for j in range(m):
        h = fmix(a + (j + 1) * STEP)
        x = j + ((h * (n - j)) >> 64)
        out.append(swapped.get(x, x))
        swapped[x] = swapped.get(j, j)
    return out


def item_of_rank(r, seen_sorted):
    """The r-th item, counting from 0 in ascending order, that is not in `seen_sorted` (ascending, distinct item ids)."""
    return r + sum(1 for k, c in enumerate(seen_sorted) if c - k <= r)


def sample(seen_rows, n_items, user_ids, m, seed, first=None, case_offset=0):
    """Rows of the library's `out`: [first[t]] + the m drawn items; the drawn slots are -1 where the user id is outside the table or
    the user has fewer than m unseen items.  `seen_rows[u]`: ascending item ids.  Returns (rows, status word)."""
    rows, status = [], 0
    for t, u in enumerate(user_ids):
        head = [] if first is None else [int(first[t])]
        if not 0 <= u < len(seen_rows):
            status |= 1
            rows.append(head + [-1] * m)
            continue
        row = [int(c) for c in seen_rows[u]]
        n = n_items - len(row)
        if n < m:
            status |= 2
            rows.append(head + [-1] * m)
            continue
        rows.append(head + [item_of_rank(r, row) for r in ranks(case_offset + t, seed, n, m)])
    return rows, status
