"""`ShardedPropagation`: what a rank holds (its slabs as CSRs, the layout, the exchange buffers, the previous result) and how it
was set up.  The loops that use it live beside it: `bipartite`, `allgather` (propagation) and `gathers` (the batch rows)."""

import os
from typing import Optional

import torch
import torch.distributed as dist

from .. import engine as _eng
from . import allgather as _ag, bipartite as _bp, gathers as _ga
from .functions import _CabiAllGather
from .p2p import P2PExchange
from .partition import (ShardLayout, balanced_bounds, chunk_bounds, cut_slabs, even_bounds, laplacian_values, ld32, padded_item_pos,
                        row_counts, slab_coo)

SCHEME_NOTES = {
    "allgather": "row partition (users and items, cut by stored entries) + RCCL all-gather of the carry per layer, user slab "
                 "pipelined in row chunks (BASELINE config 4)",
    "bipartite": "row partition of the users (cut by stored entries), item carry replicated: item rows = partial sums over the local "
                 "users, reduce-scattered to the item's owner (dense half there only), then an all-gather of the owned items' carry "
                 "rows - the neighbour embeddings of the next layer - per layer (~10x fewer exchanged bytes than gathering the users)",
}


def _alias(name):
    """A property that reads and writes the instance attribute `name` (None while it is unset)."""
    return property(lambda self: self.__dict__.get(name), lambda self, v: setattr(self, name, v))


class ShardedPropagation:
    """NGCF.py:120-156 over `world` GPUs for one Laplacian slice.

    Build with `from_interactions` (this rank keeps only its slabs; the triplets may live on the host) or `from_coo`
    (a row-sorted COO of the [N, N] Laplacian: tests and small graphs).  Parameters are replicated: pass the same `NGCF`
    module (same seed / same state_dict) on every rank.
    """

    def __init__(self, model, rows: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor,
                 mode: str = "allgather", group=None, chunks: Optional[int] = None):
        """From the FULL row-sorted COO (every rank builds or loads the same one and keeps only its part)."""
        U, I = model.n_user, model.n_item
        n_ue = int(torch.searchsorted(rows, torch.tensor([U], device=rows.device)))
        if n_ue and (int(cols[:n_ue].min()) < U or (n_ue < rows.numel() and int(cols[n_ue:].max()) >= U)):
            raise RuntimeError("the sharded engine needs L = [[0, R], [R^T, 0]] (matrix.py:49-52)")
        if n_ue * 2 != rows.numel():
            raise RuntimeError("the sharded engine needs both triangles of L stored (matrix.py:51-52)")
        if mode == "bipartite":
            # the item rows of this scheme are formed as the transpose of the user rows: the lower triangle must BE that transpose
            # (the reference's Laplacian is symmetric, matrix.py:51-62; a re-weighted or thinned lower triangle is not supported)
            order = torch.sort(cols[:n_ue], stable=True).indices
            if not (torch.equal(cols[:n_ue][order], rows[n_ue:]) and torch.equal(rows[:n_ue][order], cols[n_ue:])
                    and torch.equal(vals[:n_ue][order], vals[n_ue:])):
                raise RuntimeError("the bipartite exchange scheme needs a symmetric L (R^T stored as the exact transpose of R, "
                                   "matrix.py:51-62); use mode='allgather' for anything else")
        cnt = row_counts(rows, U + I)

        def cut(user_lo, user_hi, item_lo, item_hi):
            a = slab_coo(rows, cols, vals, user_lo, user_hi)
            b = slab_coo(rows, cols, vals, U + item_lo, U + item_hi)
            return (a[0] + user_lo, a[1], a[2]), (b[0] + U + item_lo, b[1], b[2])
        self._setup(model, cnt[:U], cnt[U:], cut, mode, group, chunks, rows.device)

    @classmethod
    def from_coo(cls, model, rows, cols, vals, mode: str = "allgather", group=None, chunks: Optional[int] = None):
        return cls(model, rows, cols, vals, mode, group, chunks)

    @classmethod
    def from_interactions(cls, model, u: torch.Tensor, i: torch.Tensor, w: torch.Tensor, mode: str = "allgather",
                          group=None, chunks: Optional[int] = None, device=None):
        """From the unique interaction triplets (u, i, w) sorted by (u, i), on any device (host tensors included): the
        degrees and the Laplacian values are formed where the triplets live, and only this rank's slabs - about 2/W of
        the stored entries - reach the compute device.  The doubled [N, N] COO is never materialised."""
        self = cls.__new__(cls)
        v, deg_u, deg_i = laplacian_values(u, i, w, model.n_user, model.n_item)
        self._setup(model, deg_u, deg_i, lambda ul, uh, il, ih: cut_slabs(u, i, v, model.n_user, ul, uh, il, ih),
                    mode, group, chunks, device if device is not None else model._dev())
        return self

    def _setup(self, model, deg_u, deg_i, cut, mode, group, chunks, dev):
        assert mode in ("bipartite", "allgather")
        self.model, self.mode, self.group = model, mode, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self.U, self.I = model.n_user, model.n_item
        self.N = self.U + self.I
        self.dev = dev = torch.device(dev)
        self.ws = _eng.Workspace()
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        U, I, W, r = self.U, self.I, self.world, self.rank
        swept_mode = int(os.environ.get("NGCF_SPMM_MODE", "3"))
        to_dev = lambda t: t.to(dev, non_blocking=True)            # noqa: E731
        self.backend = self._pick_backend(group, dev)
        widths = self._widths()
        cnt = torch.cat([deg_u.to("cpu", torch.int64), deg_i.to("cpu", torch.int64)])
        if mode == "bipartite":
            self.ub = balanced_bounds(cnt, 0, U, W)                # user ranges with ~equal stored entries
            self.ib = even_bounds(0, I, W)                         # item OWNER ranges (item indices): reduce + dense + carry of those rows
            self.mi = mi = max(max(self.ib[q + 1] - self.ib[q] for q in range(W)), 1)
            self.PI = W * mi                                       # padded item numbering: item i of owner q sits at q*mi + (i - ib[q])
            lo, hi = self.ub[r], self.ub[r + 1]
            self.nu, self.ni = hi - lo, self.ib[r + 1] - self.ib[r]
            (ur, uc, uv), _ = cut(lo, hi, 0, 0)
            ur, uc, uv = to_dev(ur), to_dev(uc), to_dev(uv)
            pos = self.item_pos(uc - U)
            # user rows: local users x all items (replicated item carry, padded numbering)
            self.csr_u = _eng.LaplacianCSR.from_coo(ur - lo, pos, uv, self.nu, self.PI)
            # item rows restricted to local user columns -> partial sums: the transpose of the same slice
            order = torch.sort(pos, stable=True).indices
            self.csr_it = _eng.LaplacianCSR.from_coo(pos[order], ur[order] - lo, uv[order], self.PI, max(self.nu, 1))
            # The item partial sums run alone on the GPU: L2-swept kernel where it pays.  The user rows overlap with the exchange:
            # over copy engines (p2p) nothing else occupies a CU and they are swept too; beside an RCCL kernel the persistent
            # one-workgroup-per-CU sweep loses 3.4-4x (profiles/r02_c4_rank_lab.txt), so there they stay on the row-wise kernels.
            self.csr_it.set_mode(swept_mode)
            if self.backend == "p2p" or W == 1:
                self.csr_u.set_mode(swept_mode)
            self.local_nnz = self.csr_u.nnz + self.csr_it.nnz
            self._ld_in, self._ld_out = max(ld32(d) for d in widths[:-1]), max(ld32(d) for d in widths[1:])
            if self.backend == "p2p":
                # exchange buffer: per LAYER a region for the partial sums of all items and one for the carry rows of the owned
                # items.  Nothing is overwritten inside a pass, so the peers acknowledge once per pass (not per pull round): a
                # pass starts by waiting for the previous pass's acknowledgements.
                nl = len(widths) - 1
                self._off_part = [k * self.PI * self._ld_in for k in range(nl)]
                self._off_carry = [nl * self.PI * self._ld_in + k * mi * self._ld_out for k in range(nl)]
                self.p2p = self._open_p2p(group, dev, nl * (self.PI * self._ld_in + mi * self._ld_out))
        else:
            ub = balanced_bounds(cnt, 0, U, W)
            ib = balanced_bounds(cnt, U, self.N, W)
            if chunks is None:      # pipeline depth of the user slab; one chunk when there is nobody to exchange with
                chunks = int(os.environ.get("NGCF_DIST_CHUNKS", "4")) if W > 1 else 1
            self.chunks = chunks = max(1, int(chunks))
            self.layout = lay = ShardLayout(U, I, ub, ib, chunk_bounds(cnt, ub, chunks))
            (ur, uc, uv), (ir, ic, iv) = cut(ub[r], ub[r + 1], ib[r] - U, ib[r + 1] - U)
            ur, uc, uv, ir, ic, iv = (to_dev(t) for t in (ur, uc, uv, ir, ic, iv))
            self.nu, self.ni = lay.n_users_of(r), lay.n_items_of(r)
            self.csr_u = []                                        # one CSR per row chunk of the user slab
            for j in range(chunks):
                lo, hi = lay.chunk_range(r, j)
                cr, cc, cv = slab_coo(ur, uc, uv, lo, hi)
                self.csr_u.append(_eng.LaplacianCSR.from_coo(cr, lay.to_padded(cc), cv, hi - lo, lay.P))
            self.csr_i = _eng.LaplacianCSR.from_coo(ir - ib[r], lay.to_padded(ic), iv, self.ni, lay.P)
            # the item slab runs with no collective in flight (the layer's gathers have all been waited for): swept kernel
            # where it pays.  With one chunk and one rank nothing overlaps the user slab either.
            self.csr_i.set_mode(swept_mode)
            if W == 1 or self.backend == "p2p":
                for c in self.csr_u:
                    c.set_mode(swept_mode)
            self.local_nnz = sum(c.nnz for c in self.csr_u) + self.csr_i.nnz
            if self.backend == "p2p":
                # exchange buffer: the carry rows this rank produces (item slab + every user chunk), two layers in turn
                self._ld_out = max(ld32(d) for d in widths[1:])
                per_layer = (lay.mi + chunks * lay.mc) * self._ld_out
                self._off_send = [0, per_layer]
                self.p2p = self._open_p2p(group, dev, 2 * per_layer)
        self._bufs = {}
        self._cabi = None
        self._last_pub = {}
        self._calls = 0
        if self.backend == "cabi":
            self._cabi = _CabiAllGather(group, dev)

    # this rank's rows of all_E (NGCF.py:147-149): stored under the attribute names all_e.E0Cache looks at, so that the same
    # hold detection decides whether the previous pass's buffer may be written again
    allE_u, allE_i = _alias("all_users_emb"), _alias("all_items_emb")

    def item_pos(self, item: torch.Tensor) -> torch.Tensor:
        """bipartite scheme: item index -> position in the padded item numbering (owner-major)."""
        return padded_item_pos(item, self.ib, self.mi)

    def _widths(self):
        """Column widths of all_E's blocks: E0, then one per layer."""
        return [self.model.emb_size] + list(self.model.weight_size)

    def _bounds(self):
        """(user bounds, item bounds as item INDICES) per rank, in either scheme (the all-gather layout keeps items as node ids)."""
        if self.mode == "bipartite":
            return self.ub, self.ib
        return self.layout.ub, [b - self.U for b in self.layout.ib]

    def _user_csrs(self):
        """The CSRs of this rank's user rows: one in the bipartite scheme, one per chunk in the all-gather scheme."""
        return [self.csr_u] if self.mode == "bipartite" else list(self.csr_u)

    def _csrs(self):
        """This rank's CSRs in the order of a layer's SpMM launches: the item slab first."""
        return [self.csr_it if self.mode == "bipartite" else self.csr_i] + self._user_csrs()

    def _pick_backend(self, group, dev) -> str:
        """How the rows travel: "p2p" = copy engines + host-side waiting (ngcf_p2p_*, one node), "torch" = torch.distributed
        collectives (RCCL under the nccl backend), "cabi" = ngcf_allgather_rows on the process group's communicator.
        NGCF_DIST_COLLECTIVES picks one; the default is p2p on device tensors with more than one rank (it falls back to "torch"
        on every rank together if the exchange cannot be set up or its self-test fails)."""
        want = os.environ.get("NGCF_DIST_COLLECTIVES", "p2p" if self.world > 1 else "torch")
        if want == "cabi" and dist.get_backend(group) != "nccl":
            want = "torch"
        if want not in ("p2p", "torch", "cabi"):
            raise ValueError("NGCF_DIST_COLLECTIVES must be p2p, torch or cabi")
        if want == "p2p" and (self.world == 1 or torch.device(dev).type != "cuda"):
            want = "torch"
        return want

    def _open_p2p(self, group, dev, n_floats):
        ex, ok = None, 1
        try:
            ex = P2PExchange(group, dev, n_floats)
        except Exception as exc:  # noqa: BLE001
            ok = 0
            self.p2p_error = repr(exc)[:300]
        t = torch.tensor([ok], dtype=torch.int32, device=dev if dist.get_backend(group) == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
        if int(t.item()) == 1 and not ex.selftest():
            t.zero_()
            self.p2p_error = f"self-test failed ({getattr(ex, 'last_error', None)})"
        if int(t.item()) != 1:                                    # every rank takes the same decision
            if ex is not None:
                ex.close()
            self.backend = "torch"
            for c in self._user_csrs():                           # beside RCCL kernels: row-wise again
                c.set_mode(0)
            return None
        return ex

    def _buf(self, name, shape):
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != tuple(shape):
            b = torch.empty(shape, dtype=torch.float32, device=self.dev)
            self._bufs[name] = b
        return b

    def _params(self):
        m = self.model
        return ([l.weight.detach() for l in m.w1_list], [l.bias.detach() for l in m.w1_list],
                [l.weight.detach() for l in m.w2_list], [l.bias.detach() for l in m.w2_list])

    def spmm_shapes(self):
        """(nnz, rows, cols) of this rank's SpMM launches of one layer (for the roofline's algorithmic bytes)."""
        return [(c.nnz, c.n_rows, c.n_cols) for c in self._csrs()]

    def swept_rows(self):
        return [c.swept_rows for c in self._csrs()]

    def propagate(self):
        """(all_E rows of this rank's users, all_E rows of its items).  When autograd is recording and a parameter of the model
        requires a gradient and the scheme is `bipartite`, the differentiable path runs: `loss.backward()` then leaves in every
        parameter's `.grad` the gradient summed over all ranks (experiment.py:57 across GPUs)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.model.parameters()) and self.mode == "bipartite":
            return _bp.propagate_bipartite_train(self)
        # (the all-gather scheme has no differentiable path: its results carry no gradient, like any call under torch.no_grad())
        with torch.no_grad():
            return _bp.propagate_bipartite(self) if self.mode == "bipartite" else _ag.propagate_allgather(self)

    def _train_comm(self):
        return _bp.train_comm(self)

    def gather(self, u_id: torch.Tensor, pos_item: torch.Tensor, neg_item: torch.Tensor):
        """(u, pos, neg) `[B, D]` on every rank.  Rows are served by their owning rank and summed."""
        return _ga.gather(self, u_id, pos_item, neg_item)

    def p2p_stats(self, reset: bool = False):
        """Host time this rank spent blocked inside the exchanges' waits (propagation + gathers), as a dict; None without p2p."""
        exs = [e for e in (getattr(self, "p2p", None), getattr(self, "_gx", None)) if e is not None]
        if not exs:
            return None
        got = [e.stats(reset) for e in exs]
        return {"host_blocked_ms": sum(g[0] for g in got), "waits": sum(g[1] for g in got), "waits_blocked": sum(g[2] for g in got)}

    def invalidate_e0(self):
        """Forget that block 0 of the retained result buffers and the layer-0 item replica hold the current tables: the next pass
        copies them again.  Needed only after a write to an embedding table through `.data` (invisible to the version counters)."""
        self._ei0_tag = None
        if "_e0" in self.__dict__:
            self._e0.invalidate()
