"""Partition and layout helpers of the sharded engine: pure index arithmetic on any device, no `torch.distributed`."""

from typing import List, Optional, Sequence, Tuple

import torch

from .. import engine as _eng


def ld32(d: int) -> int:
    """Leading dimension of a row of `d` floats padded to a 128-byte line (32 floats), as `all_e._padded_rows` allocates."""
    return (d + 31) // 32 * 32


def row_counts(rows: torch.Tensor, n_rows: int) -> torch.Tensor:
    return torch.bincount(rows, minlength=n_rows)


def balanced_bounds(counts: torch.Tensor, begin: int, end: int, world: int) -> List[int]:
    """Contiguous cut of rows [begin, end) into `world` ranges with ~equal stored entries (ngcf_shard_plan)."""
    rp = torch.zeros(counts.numel() + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(counts.to("cpu", torch.int64), 0)
    return _eng.shard_plan(rp, begin, end, world)


def even_bounds(begin: int, end: int, world: int) -> List[int]:
    n = end - begin
    return [begin + (n * w) // world for w in range(world + 1)]


def chunk_bounds(counts: torch.Tensor, rank_bounds: Sequence[int], chunks: int) -> List[int]:
    """Every rank's range cut again into `chunks` entry-balanced row chunks: W*chunks+1 ascending bounds."""
    out = [rank_bounds[0]]
    for r in range(len(rank_bounds) - 1):
        out += balanced_bounds(counts, rank_bounds[r], rank_bounds[r + 1], chunks)[1:]
    return out


def owner_index(bounds, x: torch.Tensor) -> torch.Tensor:
    """The range [bounds[q], bounds[q+1]) holding each element of `x`; `bounds` (a sequence or a tensor) is moved to `x.device`.
    Empty ranges repeat a bound: right=True picks the last range that starts at or before the element, the one holding it."""
    b = torch.as_tensor(bounds, device=x.device)
    return (torch.searchsorted(b, x, right=True) - 1).clamp(0, b.numel() - 2)


def owner_of(bounds, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(owner, local): `owner_index` and the element's offset inside its owner's range.  (Two functions: a caller that needs the
    owners alone - `gathers._owner_index` - must not pay the two launches of the offset.)"""
    b = torch.as_tensor(bounds, device=x.device)
    owner = owner_index(b, x)                                  # (`b` is a tensor on the device by now: passed through as it is)
    return owner, x - b[owner]


class ShardLayout:
    """Padded numbering of the N = U + I nodes for the all-gather scheme.

    Rank r owns users [ub[r], ub[r+1]) and items [ib[r], ib[r+1]) (global node ids; items are U-based); its user
    range is cut into C chunks [cb[r*C+j], cb[r*C+j+1]).  Padded position of the k-th user of chunk j of rank r:
    j*W*mc + r*mc + k (chunk-major, then rank-major: the region of chunk j is what ONE all-gather of that chunk
    fills); of rank r's k-th item: W*C*mc + r*mi + k, with mc / mi the largest user chunk / item range.  A replica of E
    in this numbering has P = W*(C*mc + mi) rows; padding rows are never referenced by any column index.
    With C = 1 this is the plain rank-major layout.
    """

    def __init__(self, n_user: int, n_item: int, user_bounds: Sequence[int], item_bounds: Sequence[int],
                 user_chunk_bounds: Optional[Sequence[int]] = None):
        assert len(user_bounds) == len(item_bounds) and user_bounds[0] == 0 and user_bounds[-1] == n_user
        assert item_bounds[0] == n_user and item_bounds[-1] == n_user + n_item
        self.n_user, self.n_item = n_user, n_item
        self.world = len(user_bounds) - 1
        self.ub, self.ib = list(user_bounds), list(item_bounds)
        self.cb = list(user_chunk_bounds) if user_chunk_bounds is not None else list(user_bounds)
        assert (len(self.cb) - 1) % self.world == 0
        self.chunks = (len(self.cb) - 1) // self.world
        assert [self.cb[r * self.chunks] for r in range(self.world + 1)] == self.ub, "chunk bounds must refine the rank bounds"
        assert all(a <= b for a, b in zip(self.cb, self.cb[1:]))
        self.mc = max(max(b - a for a, b in zip(self.cb, self.cb[1:])), 1)
        self.mi = max(max(self.ib[r + 1] - self.ib[r] for r in range(self.world)), 1)
        self.n_user_pos = self.world * self.chunks * self.mc
        self.P = self.n_user_pos + self.world * self.mi

    def n_users_of(self, r, j=None):
        if j is None:
            return self.ub[r + 1] - self.ub[r]
        return self.cb[r * self.chunks + j + 1] - self.cb[r * self.chunks + j]

    def n_items_of(self, r): return self.ib[r + 1] - self.ib[r]
    def user_pos(self, r, j=0): return (j * self.world + r) * self.mc
    def item_pos(self, r): return self.n_user_pos + r * self.mi
    def chunk_region(self, j): return j * self.world * self.mc, (j + 1) * self.world * self.mc
    def chunk_range(self, r, j): return self.cb[r * self.chunks + j], self.cb[r * self.chunks + j + 1]

    def to_padded(self, node: torch.Tensor) -> torch.Tensor:
        """Global node id -> padded position (vectorised)."""
        ci, ku = owner_of(self.cb, node)
        ri, ki = owner_of(self.ib, node)
        r, j = ci // self.chunks, ci % self.chunks
        pu = (j * self.world + r) * self.mc + ku
        pi = self.n_user_pos + ri * self.mi + ki
        return torch.where(node >= self.n_user, pi, pu)

    def owner_of_user(self, u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return owner_of(self.ub, u)

    def owner_of_item(self, i: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """`i` is an item index in [0, I) (as in pos_item/neg_item)."""
        return owner_of(self.ib, i + self.n_user)


def padded_item_pos(item: torch.Tensor, item_bounds: Sequence[int], mi: int) -> torch.Tensor:
    """bipartite scheme: item index -> position in the owner-major padded numbering: item i of owner q (item_bounds[q] <= i <
    item_bounds[q+1]) sits at q*mi + (i - item_bounds[q]), mi = the largest owner range.  One all-gather of [mi, d] per rank then
    IS the item replica of the next layer, and a reduce-scatter over [W*mi, d] hands every owner its rows."""
    q, k = owner_of(item_bounds, item)
    return q * mi + k


def slab_coo(rows, cols, vals, lo: int, hi: int):
    """Entries of rows [lo, hi) of a row-sorted COO, row ids made slab-relative."""
    a, b = (int(x) for x in torch.searchsorted(rows, torch.tensor([lo, hi], device=rows.device)))
    return rows[a:b] - lo, cols[a:b], vals[a:b]


def laplacian_values(u: torch.Tensor, i: torch.Tensor, w: torch.Tensor, n_user: int, n_item: int):
    """Values of the symmetric-normalised Laplacian for the interaction triplets, the way `Matrix.create_matrix` forms
    them (matrix.py:55-62: count degrees, d^-1/2 in float32, product in float64, cast to float32); also the degrees."""
    deg_u = torch.bincount(u, minlength=n_user)
    deg_i = torch.bincount(i, minlength=n_item)
    ds_u = deg_u.to(torch.float32).pow(-0.5)
    ds_i = deg_i.to(torch.float32).pow(-0.5)
    ds_u[torch.isinf(ds_u)] = 0
    ds_i[torch.isinf(ds_i)] = 0
    return (ds_u[u].double() * w.double() * ds_i[i].double()).float(), deg_u, deg_i


def cut_slabs(u: torch.Tensor, i: torch.Tensor, v: torch.Tensor, n_user: int, user_lo: int, user_hi: int,
              item_lo: int, item_hi: int):
    """This rank's part of L = [[0, R], [R^T, 0]] from the interaction triplets sorted by (u, i) with Laplacian values v:
    the user rows [user_lo, user_hi) (a contiguous slice of the triplets) and the item rows [item_lo, item_hi) (item
    INDICES, a masked selection re-sorted by (i, u)).  Returns two (rows, cols, vals) triplets with GLOBAL node ids,
    row-sorted, entries inside a row in ascending column order - the same entries and order as the matching rows of
    the full COO of `graphs._normalise`, without ever forming it."""
    a, b = (int(x) for x in torch.searchsorted(u, torch.tensor([user_lo, user_hi], device=u.device)))
    user_rows = (u[a:b], i[a:b] + n_user, v[a:b])
    sel = (i >= item_lo) & (i < item_hi)
    iu, ii, iv = u[sel], i[sel], v[sel]
    order = torch.sort(ii, stable=True).indices           # (u, i) order -> (i, u) order
    item_rows = (ii[order] + n_user, iu[order], iv[order])
    return user_rows, item_rows
