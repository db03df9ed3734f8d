"""The loops of the ``allgather`` exchange scheme (inference only), over torch.distributed / the C-ABI all-gather and over the CU-free
exchange: the same pieces (`layer_piece`), another way to the peers' replicas.  `sh` is the `ShardedPropagation`; it keeps all state."""

import torch

from .. import engine as _eng
from .functions import allgather_rows
from .partition import ld32


def _gather_async(sh, region: torch.Tensor, send: torch.Tensor):
    if sh._cabi is not None:
        return sh._cabi(region, send)
    return allgather_rows(region, send, sh.group, async_op=True)


def propagate_allgather(sh):
    m, lay, r, W, Cn = sh.model, sh.layout, sh.rank, sh.world, sh.chunks
    w1, b1, w2, b2 = sh._params()
    widths = sh._widths()
    D, n_layer = sum(widths), len(w1)
    nu, ni = sh.nu, sh.ni
    allE_u = torch.empty((nu, D), dtype=torch.float32, device=sh.dev)
    allE_i = torch.empty((ni, D), dtype=torch.float32, device=sh.dev)
    d0 = widths[0]
    uw, iw = m.user_embedding.weight.detach(), m.item_embedding.weight.detach()
    _eng.copy_rows(uw[lay.ub[r]:lay.ub[r + 1]], allE_u[:, :d0])
    _eng.copy_rows(iw[lay.ib[r] - sh.U:lay.ib[r + 1] - sh.U], allE_i[:, :d0])
    # layer-0 replica from the replicated parameter tables: local copies, no communication
    full = sh._buf(("full", 0), (lay.P, d0))
    for q in range(W):
        for j in range(Cn):
            lo, hi = lay.chunk_range(q, j)
            if hi > lo:
                _eng.copy_rows(uw[lo:hi], full[lay.user_pos(q, j):lay.user_pos(q, j) + hi - lo])
        if lay.n_items_of(q):
            _eng.copy_rows(iw[lay.ib[q] - sh.U:lay.ib[q + 1] - sh.U],
                           full[lay.item_pos(q):lay.item_pos(q) + lay.n_items_of(q)])
    first_row = [lay.chunk_range(r, j)[0] - lay.ub[r] for j in range(Cn)]      # chunk j's rows inside allE_u

    def layer_piece(k, piece, full, carry_out):
        """Layer k for one piece of this rank's rows - 0 = the item slab, 1 + j = user chunk j - gathering from the replica
        `full`: the norm block goes to its place in allE_*, the carry rows (None in the last layer) to the top of `carry_out`."""
        d_out, off = widths[k + 1], sum(widths[:k + 1])
        if piece == 0:
            csr, pos, n, table, row0 = sh.csr_i, lay.item_pos(r), ni, allE_i, 0
        else:
            j = piece - 1
            csr, pos, n, table, row0 = sh.csr_u[j], lay.user_pos(r, j), lay.n_users_of(r, j), allE_u, first_row[j]
        _eng.layer_fused(csr, full, full[pos:pos + n], w1[k], b1[k], w2[k], b2[k],
                         None if carry_out is None else carry_out[:n, :d_out], table[row0:row0 + n, off:off + d_out], sh.ws)

    if sh.backend == "p2p":
        _allgather_layers_p2p(sh, full, widths, layer_piece)
    else:
        for k in range(n_layer):
            d_out = widths[k + 1]
            last = k == n_layer - 1
            nxt = None if last else sh._buf(("full", (k + 1) % 2 + 1), (lay.P, d_out))
            works = []
            # item slab first, alone on the GPU; its (small) all-gather overlaps with the first user chunk
            si = None if last else sh._buf(("si", k % 2), (lay.mi, d_out))
            layer_piece(k, 0, full, si)
            if not last:
                works.append(_gather_async(sh, nxt[lay.n_user_pos:], si))
            # user slab, chunk by chunk: chunk j's all-gather is in flight while chunk j+1 computes
            for j in range(Cn):
                sj = None if last else sh._buf(("su", k % 2, j), (lay.mc, d_out))
                layer_piece(k, 1 + j, full, sj)
                if not last:
                    a, b = lay.chunk_region(j)
                    works.append(_gather_async(sh, nxt[a:b], sj))
            for wk in works:                                       # only now: the next layer reads the whole replica
                wk.wait()
            if not last:
                full = nxt
    sh.allE_u, sh.allE_i = allE_u, allE_i
    return allE_u, allE_i


def _allgather_layers_p2p(sh, full, widths, layer_piece):
    """The layers of the all-gather scheme over the CU-free exchange: every piece of carry rows this rank produces (item slab,
    then the user chunks) is written into its exchange buffer and published; the peers - and this rank itself - pull it
    into their replica of the next layer while the following piece computes.  No kernel of the exchange shares the CUs, so
    every piece runs on the L2-swept kernel where its plan pays."""
    lay, Cn, ex = sh.layout, sh.chunks, sh.p2p
    n_layer = len(widths) - 1
    sh._calls += 1
    base = sh._calls * (n_layer + 1)
    for k in range(n_layer):
        d_out = widths[k + 1]
        last = k == n_layer - 1
        seq, par = base + k + 1, k % 2
        ld = ld32(d_out)
        nxt = None if last else sh._buf(("fullp", (k + 1) % 2 + 1), (lay.P, ld))
        if not last:
            ex.fence()
        # pieces: 0 = item slab, 1 + j = user chunk j; their rows inside the exchange buffer and inside every replica
        send_off = [sh._off_send[par]] + [sh._off_send[par] + (lay.mi + j * lay.mc) * ld for j in range(Cn)]
        rows = [lay.mi] + [lay.mc] * Cn

        def region(q, piece):
            a = lay.item_pos(q) if piece == 0 else lay.user_pos(q, piece - 1)
            return nxt[a:a + rows[piece]]

        def pull_piece(piece):
            slot = par * (Cn + 1) + piece
            ex.pull_from_all(slot, seq, send_off[piece], lambda q: region(q, piece), ack=(slot, seq))

        for piece in range(Cn + 1):
            slot = par * (Cn + 1) + piece
            send = None
            if not last:
                ex.wait_acks(slot, sh._last_pub.get(slot, 0))
                send = ex.floats(send_off[piece], rows[piece] * ld).view(rows[piece], ld)
            layer_piece(k, piece, full, send)
            if not last:
                ex.publish(slot, seq)
                sh._last_pub[slot] = seq
                if piece > 0:
                    pull_piece(piece - 1)                      # the previous piece travels while this one computes
        if not last:
            pull_piece(Cn)
            ex.join()                                          # only now: the next layer reads the whole replica
            full = nxt[:, :d_out]
