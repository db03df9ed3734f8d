"""The weighted draw of unseen items (ngcf_weighted_prepare / ngcf_sample_weighted) in pure Python integers for the
weighted-negative tests.  It shares no code with the library: lists and `bisect` for the two searches, a sorted walk over the drawn
intervals for the skip."""
import bisect

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


def prepare(weights, seen_sorted):
    """(cdf [n + 1], gap [len], S [len + 1]) of one user: cdf[i] the weight below item i, S[k] the weight of the first k seen items,
    gap[k] = cdf[c_k] - S[k] the unseen weight below the k-th seen item.  The user's unseen mass is cdf[-1] - S[-1]."""
    cdf = [0]
    for w in weights:
        cdf.append(cdf[-1] + int(w))
    gap, S = [], [0]
    for c in seen_sorted:
        gap.append(cdf[c] - S[-1])
        S.append(S[-1] + int(weights[c]))
    return cdf, gap, S


def item_at(cdf, gap, S, r):
    """(item, q) of the point r in [0, U) of the user's unseen coordinate: the item whose interval [q, q + w) holds r."""
    K = bisect.bisect_right(gap, r)                       # #{k : gap_k <= r}
    tgt = r + S[K]
    c = bisect.bisect_right(cdf, tgt) - 1                 # the largest i with cdf[i] <= tgt
    return c, cdf[c] - S[K]


def skip_drawn(drawn, rp):
    """The point r' of the coordinate with the drawn intervals (q, w) cut out, as a point of the full unseen coordinate."""
    r, before = rp, 0
    for q, w in sorted(drawn):
        if q - before <= rp:                              # e_i = q_i - (widths drawn below q_i)
            r += w
        before += w
    return r


def draw_points(weights, cdf, gap, S, points):
    """The items of successive points r'_j in [0, U_j): what `draw` does after hashing.  Returns (items, q's)."""
    drawn, items = [], []
    for rp in points:
        c, q = item_at(cdf, gap, S, skip_drawn(drawn, rp))
        items.append(c)
        drawn.append((q, int(weights[c])))
    return items, [q for q, _ in drawn]


def draw(weights, seen_sorted, t, seed, m, prepared=None):
    """The m items of global case t, or None when the user has fewer than m positive-weight unseen items.
    Returns (items, weights of the items, U)."""
    cdf, gap, S = prepared or prepare(weights, seen_sorted)
    U = cdf[-1] - S[-1]
    a = fmix((seed & M64) ^ ((t * GOLDEN) & M64))
    drawn, items, Uj = [], [], U
    for j in range(m):
        if Uj == 0:
            return None, None, U
        rp = (fmix(a + (j + 1) * STEP) * Uj) >> 64
        c, q = item_at(cdf, gap, S, skip_drawn(drawn, rp))
        w = int(weights[c])
        items.append(c)
        drawn.append((q, w))
        Uj -= w
    return items, [w for _, w in drawn], U


def sample(weights, seen_rows, user_ids, m, seed, case_offset=0):
    """Rows of the library's outputs: (items [T][m], draw_weight [T][m], case_mass [T], status word); a user id outside the table
    gives (-1.., 0.., 0) and bit 1, a user with fewer than m positive-weight unseen items (-1.., 0.., U) and bit 2."""
    prepared = {}
    items, ws, mass, status = [], [], [], 0
    for t, u in enumerate(user_ids):
        if not 0 <= u < len(seen_rows):
            status |= 1
            items.append([-1] * m), ws.append([0] * m), mass.append(0)
            continue
        if u not in prepared:
            prepared[u] = prepare(weights, [int(c) for c in seen_rows[u]])
        it, w, U = draw(weights, None, case_offset + t, seed, m, prepared[u])
        if it is None:
            status |= 2
            it, w = [-1] * m, [0] * m
        items.append(it), ws.append(w), mass.append(U)
    return items, ws, mass, status
