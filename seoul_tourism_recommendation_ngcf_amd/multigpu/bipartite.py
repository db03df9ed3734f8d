"""The loops of the ``bipartite`` exchange scheme: inference (`propagate_bipartite`) and the differentiable composition
(`propagate_bipartite_train`).  Module functions over a `ShardedPropagation` `sh`, which keeps all state."""

import torch
import torch.distributed as dist

from .. import engine as _eng
from ..all_e import E0Cache
from .functions import AllGatherRows, DenseLayerFn, ReduceScatterRows, SpmmFn, _SumGrads
from .p2p import P2PCollectives, sum_slots
from .partition import ld32


def train_comm(sh):
    """What the differentiable exchange steps run on: the process group (torch.distributed collectives), or - when this
    object's transport is p2p - a `P2PCollectives` over an exchange buffer of its own, created on first use."""
    if sh.backend != "p2p":
        return sh.group
    if getattr(sh, "_p2p_train", None) is None:
        sh._p2p_train = P2PCollectives(sh.group, sh.dev, sh.PI * max(ld32(d) for d in sh._widths()))
    return sh._p2p_train


def propagate_bipartite_train(sh):
    """The bipartite scheme as a composition of differentiable pieces: `SpmmFn` (the two CSRs of a rank are each other's
    transposes), `DenseLayerFn` (hand-written backward kernels), `ReduceScatterRows` / `AllGatherRows` (each the other's
    adjoint).  Eval-mode semantics (no dropout).  The exchange steps run over this object's transport in both directions
    (`train_comm`: the CU-free p2p collectives, or torch.distributed).
    Gradients: every rank's backward yields the contribution of the rows it owns; `_SumGrads` adds them over the ranks, so
    after `loss.backward()` all ranks hold the same, complete `.grad` for every parameter - as after a single-GPU step."""
    m, g = sh.model, sh.group
    comm = train_comm(sh)
    r, mi, PI = sh.rank, sh.mi, sh.PI
    lo, nu, ni = sh.ub[r], sh.nu, sh.ni
    n_layer = m.n_layer
    # parameters enter through one Function whose backward all-reduces their gradients (once per step)
    params = [m.user_embedding.weight, m.item_embedding.weight] + [l.weight for l in m.w1_list] + [l.bias for l in m.w1_list] + \
             [l.weight for l in m.w2_list] + [l.bias for l in m.w2_list]
    outs = _SumGrads.apply(g, {0: list(sh.ub)}, *params)       # the user table is read through the rank's own slab only
    uw, iw = outs[0], outs[1]
    w1, b1 = outs[2:2 + n_layer], outs[2 + n_layer:2 + 2 * n_layer]
    w2, b2 = outs[2 + 2 * n_layer:2 + 3 * n_layer], outs[2 + 3 * n_layer:]
    eu = uw[lo:lo + nu]
    # item replica in the padded numbering (a gather of the replicated table; padding rows read item 0 and are never used)
    src = torch.zeros(PI, dtype=torch.int64, device=sh.dev)
    src[sh.item_pos(torch.arange(sh.I, device=sh.dev))] = torch.arange(sh.I, device=sh.dev)
    ei = iw[src]
    own = slice(r * mi, r * mi + ni)
    blocks_u, blocks_i = [eu], [ei[own]]
    for k in range(n_layer):
        part = SpmmFn.apply(eu, sh.csr_it, sh.csr_u, sh.ws)                     # item partial sums over the local users
        le_own = ReduceScatterRows.apply(part, comm)                             # [mi, d]: the owned items, summed over ranks
        le_u = SpmmFn.apply(ei, sh.csr_u, sh.csr_it, sh.ws)                     # user rows, fully local
        cu, nrm_u = DenseLayerFn.apply(le_u, eu, w1[k], b1[k], w2[k], b2[k], sh.ws)
        ci, nrm_i = DenseLayerFn.apply(le_own[:ni], ei[own], w1[k], b1[k], w2[k], b2[k], sh.ws)
        blocks_u.append(nrm_u)
        blocks_i.append(nrm_i)
        if k + 1 < n_layer:
            send = torch.zeros((mi, ci.shape[1]), dtype=torch.float32, device=sh.dev)
            send = torch.cat([ci, send[ni:]], 0) if ni < mi else ci
            ei = AllGatherRows.apply(send, comm)
        eu = cu
    sh.allE_u, sh.allE_i = torch.cat(blocks_u, 1), torch.cat(blocks_i, 1)
    return sh.allE_u, sh.allE_i


def propagate_bipartite(sh):
    """Users partitioned, item block replicated.  Per layer:  A  item partial sums over the local users (swept SpMM on the
    transposed user slab)  ->  reduce-scatter: every rank receives the partial sums of the items it OWNS and adds them in
    rank order  ->  B  user rows (fully local, overlaps with that exchange)  ->  C  dense half for the owned items only  ->
    all-gather of their carry rows into every rank's item replica (overlaps with the next layer's A).  The exchanged bytes
    per rank and layer are 2 x (W-1)/W x I x d x 4 (C3, W = 8: 2 x 45 MB) against (W-1)/W x N x d x 4 (493 MB) for the all-gather
    of users; nothing is computed twice (r02 ran the item dense replicated after an all-reduce)."""
    m = sh.model
    w1, b1, w2, b2 = sh._params()
    widths = sh._widths()
    D, n_layer = sum(widths), len(w1)
    r, W, mi, PI = sh.rank, sh.world, sh.mi, sh.PI
    lo, nu, ni = sh.ub[r], sh.nu, sh.ni
    d0 = widths[0]
    iw = m.item_embedding.weight.detach()
    uwp, iwp = m.user_embedding.weight, m.item_embedding.weight
    # r04: ONE result buffer [nu + ni, D] (users first; the three served gathers then read one table in one launch), and the
    # previous pass's buffer is written again - its block 0 (E0, NGCF.py:120) NOT copied again - while both tables are the same
    # tensors at the same version and nobody else holds the previous result (all_e.E0Cache.only_the_modules: a caller who
    # kept it gets a fresh buffer, as before).  At W = 8 that is the rank's share of the E0 copy per pass (23 us of a 2 ms step).
    e0_tag = (uwp.data_ptr(), int(uwp._version), iwp.data_ptr(), int(iwp._version), tuple(widths), nu, ni)
    cache = sh.__dict__.setdefault("_e0", E0Cache())
    keep = cache.tag == e0_tag and cache.only_the_modules(sh)
    if keep:
        allE = cache.all_E
    else:
        cache.invalidate()
        sh._all_E = sh.all_users_emb = sh.all_items_emb = None
        allE = torch.empty((nu + ni, D), dtype=torch.float32, device=sh.dev)
        _eng.copy_rows(uwp.detach()[lo:lo + nu], allE[:nu, :d0])
        _eng.copy_rows(iw[sh.ib[r]:sh.ib[r + 1]], allE[nu:, :d0])
        cache.all_E, cache.tag = allE, e0_tag
    allE_u, allE_i = allE[:nu], allE[nu:]                       # this rank's users / the items this rank owns
    # layer-0 item replica from the replicated parameter table (padded numbering): local copies, no communication - and none at
    # all while the table is the same tensor at the same version as in the previous pass (inference loops)
    ei = sh._buf(("ei", 0), (PI, ld32(d0)))[:, :d0]
    tag = (iw.data_ptr(), m.item_embedding.weight._version, tuple(iw.shape))
    if getattr(sh, "_ei0_tag", None) != tag:
        for q in range(W):
            n_q = sh.ib[q + 1] - sh.ib[q]
            if n_q:
                _eng.copy_rows(iw[sh.ib[q]:sh.ib[q + 1]], ei[q * mi:q * mi + n_q])
        sh._ei0_tag = tag
    eu = allE_u[:, :d0]
    if d0 % 4 or D % 4:                                        # rows of all_E are not 16-byte aligned: an aligned copy to gather from
        eu = sh._buf(("eu0",), (nu, ld32(d0)))[:, :d0]
        if not keep:
            _eng.copy_rows(uwp.detach()[lo:lo + nu], eu)
    ex = sh.p2p if sh.backend == "p2p" else None
    sh._calls += 1
    base = sh._calls * (n_layer + 1)
    gloo = dist.get_backend(sh.group) != "nccl"
    off = d0
    pending = None                                             # the all-gather of the previous layer's item carry
    ACK = 62                                                   # the one acknowledgement slot: "I have read everything of pass n"
    if ex is not None:
        ex.wait_acks(ACK, sh._calls - 1)                       # every peer is done with what the previous pass left in my buffer
    for k in range(n_layer):
        d_in, d_out = widths[k], widths[k + 1]
        last = k == n_layer - 1
        seq = base + k + 1
        sp, sc = 2 * k, 2 * k + 1                              # sequence slots: partial sums / carry of this layer
        if ex is not None:
            ex.fence()                                         # copies of this layer start after the previous layer's readers
            # -- A: item partial sums over the local users, into the exchange buffer
            part = ex.floats(sh._off_part[k], PI * ld32(d_in)).view(PI, ld32(d_in))[:, :d_in]
            _eng.spmm(sh.csr_it, eu, out=part, ws=sh.ws)
            ex.publish(sp, seq)
            # -- the previous layer's item carry arrives while A runs; no acknowledgement: the pass's one ack follows its last pull
            if pending is not None:
                nxt_ei, pseq, psc = pending
                ex.pull_from_all(psc, pseq, sh._off_carry[k - 1], lambda q: nxt_ei[q * mi:(q + 1) * mi])
                ex.join()
                ei = nxt_ei[:, :d_in]
                pending = None
        else:
            if pending is not None:
                pending.wait()
            part = sh._buf(("part", k), (PI, ld32(d_in)))[:, :d_in]
            _eng.spmm(sh.csr_it, eu, out=part, ws=sh.ws)
        # -- B: user rows, fully local (gathers from the item replica); overlaps with the reduce-scatter
        if ex is None:
            le_own = sh._buf(("le_own", k), (mi, ld32(d_in)))
            full_part = sh._bufs[("part", k)]
            if gloo:                                           # gloo has no reduce-scatter: all-reduce and keep the own rows
                work = dist.all_reduce(full_part, group=sh.group, async_op=True)
            else:
                work = dist.reduce_scatter_tensor(le_own, full_part, group=sh.group, async_op=True)
        cu = None if last else sh._buf(("cu", k), (nu, ld32(d_out)))[:, :d_out]
        _eng.layer_fused(sh.csr_u, ei, eu, w1[k], b1[k], w2[k], b2[k], cu, allE_u[:, off:off + d_out], sh.ws)
        # -- reduce-scatter: the partial sums of the owned items from every rank, added in rank order
        if ex is not None:
            slots = sh._buf(("slots", k), (W, mi, ld32(d_in)))
            # (acknowledged in the last layer only: the last copy of this pass from rank q is enqueued)
            ex.pull_from_all(sp, seq, sh._off_part[k] + r * mi * ld32(d_in), lambda q: slots[q],
                             ack=(ACK, sh._calls) if last else None)
            ex.join()
            le_own = sh._buf(("le_own", k), (mi, ld32(d_in)))
            sum_slots(slots, le_own)
        else:
            work.wait()
            if gloo:
                le_own = full_part[r * mi:(r + 1) * mi]
        # -- C: dense half for the owned items; their carry rows go to every rank's replica of the next layer
        if last:
            ci = None
        elif ex is not None:
            ci = ex.floats(sh._off_carry[k], mi * ld32(d_out)).view(mi, ld32(d_out))
        else:
            ci = sh._buf(("ci", k), (mi, ld32(d_out)))
        if ni:
            _eng.layer_dense(le_own[:ni, :d_in], ei[r * mi:r * mi + ni], w1[k], b1[k], w2[k], b2[k],
                             None if last else ci[:ni, :d_out], allE_i[:, off:off + d_out], sh.ws)
        if not last:
            nxt_ei = sh._buf(("ei", k + 1), (PI, ld32(d_out)))
            if ex is not None:
                ex.publish(sc, seq)
                pending = (nxt_ei, seq, sc)                    # pulled at the top of the next layer, under its A
            else:
                pending = dist.all_gather_into_tensor(nxt_ei, ci, group=sh.group, async_op=True)
                # (waited for before the next layer's swept A: an RCCL kernel beside the sweep costs more than the wait)
                ei = nxt_ei[:, :d_out]
        eu = cu
        off += d_out
    sh._all_E, sh.all_users_emb, sh.all_items_emb = allE, allE_u, allE_i
    return allE_u, allE_i
