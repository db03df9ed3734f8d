"""The batch gathers of both schemes (NGCF.py:151-156): rows are served by the rank that owns them.  Module functions over a
`ShardedPropagation` `sh`, which keeps all state."""

import os
import weakref

import torch
import torch.distributed as dist

from .. import _lib, engine as _eng
from .functions import OwnerRowsSum, owner_rows_sum
from .p2p import P2PExchange
from .partition import owner_index, owner_of


def _local_index(sh, ix: torch.Tensor, lo: int) -> torch.Tensor:
    """ix - lo as a contiguous int64 device tensor, computed once per index tensor OBJECT and version (a loop over fixed
    batches pays no launch for it)."""
    memo = sh.__dict__.setdefault("_loc_idx", {})
    key = (id(ix), int(ix._version), int(lo))
    hit = memo.get(key)
    if hit is not None and hit[0]() is ix:
        return hit[1]
    if len(memo) > 16:
        memo.clear()
    loc = (ix.to(device=sh.dev, dtype=torch.int64) - lo).contiguous()
    memo[key] = (weakref.ref(ix), loc)
    return loc


def _owned_rows(sh, out, sets):
    """The rows of the batch this rank owns, gathered into their positions of `out` [sum of sizes, D]; positions other ranks own
    are left alone (the gather kernels skip ids outside the range: the status word of that call is a throw-away).  One launch
    when this rank's rows live in one buffer (the bipartite inference path), else one per index vector."""
    lib = _lib.load()
    D = int(out.shape[1])
    scrap = sh._buf(("scrap_status",), (1,)).view(torch.int32)
    base = sh.__dict__.get("_all_E")
    one = (base is not None and all(t._base is base for t, _, _, _ in sets) and len(sets) <= 3
           and sh.__dict__.get("all_users_emb") is sets[0][0])
    with _eng._on(sh.dev):
        if one:
            args, at = [], 0
            for table, ix, lo, n_rows in sets:
                b = int(ix.numel())
                row_off = 0 if table is sh.all_users_emb else int(sh.all_users_emb.shape[0])
                args += [_eng._ptr(_local_index(sh, ix, lo)) if b and n_rows else None, b if n_rows else 0, row_off, n_rows,
                         _eng._ptr(out[at:at + b]) if b and n_rows else None]
                at += b
            args += [None, 0, 0, 0, None] * (3 - len(sets))
            _lib.check(lib.ngcf_gather_rows3_f32(_eng._ptr(base), _eng._row_major_ld(base, "all_E"), D, *args, D, _eng._ptr(scrap),
                                                 _eng._stream()))
            return
        at = 0
        for table, ix, lo, n_rows in sets:
            b = int(ix.numel())
            if n_rows and b:
                loc = _local_index(sh, ix, lo)
                _lib.check(lib.ngcf_gather_rows_f32(_eng._ptr(table), _eng._row_major_ld(table, "table"), D, _eng._ptr(loc), b, 0, n_rows,
                                                    _eng._ptr(out[at:at + b]), D, _eng._ptr(scrap), _eng._stream()))
            at += b


def _owner_index(sh, u_id, pos_item, neg_item, Btot):
    """int64[Btot]: position b of the batch is row owner(b) * Btot + b of the [W * Btot, D] block of pulled rows.  Computed once
    per set of index tensors (same objects at the same version: a loop over fixed batches pays nothing)."""
    ids = (u_id, pos_item) + ((neg_item,) if neg_item is not None else ())
    key = tuple((id(t), int(t._version), int(t.numel())) for t in ids)
    hit = getattr(sh, "_owner_idx", None)
    if hit is not None and hit[0] == key and all(a() is b for a, b in zip(hit[2], ids)):
        return hit[1]
    ub, ib = (torch.tensor(b, device=sh.dev) for b in sh._bounds())
    own = [owner_index(ub, u_id)] + [owner_index(ib, t) for t in ids[1:]]
    idx = (torch.cat(own) * Btot + torch.arange(Btot, device=sh.dev)).contiguous()
    sh._owner_idx = (key, idx, [weakref.ref(t) for t in ids])
    return idx


def _gather_p2p(sh, sets, sizes, D, u_id, pos_item, neg_item):
    """The three row gathers over the CU-free exchange (r04; r03 used an all-reduce of a zero-filled [B, D] buffer - an RCCL
    kernel on the CUs at the end of every pass): every rank gathers the rows it OWNS into its exchange buffer and publishes;
    every rank pulls every peer's block (copy engines; W blocks of sum(sizes) x D floats = 6.3 MB each at C3's batch, all links
    at once) and one gather kernel picks position b out of its owner's block.  Bit-exact copies of the owners' rows.  Two
    regions in turn, so that a rank overwrites a block only after every peer has read it (acknowledgements per pass)."""
    Btot = sum(sizes)
    need = Btot * D
    gx = getattr(sh, "_gx", None)
    if gx is None or sh._gx_region < need:                     # (collective: every rank sees the same sizes in the same call)
        if gx is not None:
            for reg_ in (0, 1):                                # every peer has finished reading the old buffer before it goes
                last = sh._gx_calls - ((sh._gx_calls - 1 - reg_) % 2)
                gx.wait_acks(reg_, max(last, 0))
            gx.close()
        sh._gx_region = need
        sh._gx, sh._gx_calls = None, 0
        try:       # (a failure is a failure on every rank: the constructor and the self-test share their verdicts)
            gx = P2PExchange(sh.group, sh.dev, max(2 * need, 1024))
            if not gx.selftest():
                err = getattr(gx, "last_error", "self-test failed")
                gx.close()
                raise RuntimeError(err)
            sh._gx = gx
        except Exception as exc:  # noqa: BLE001
            sh.gather_p2p_error = repr(exc)[:300]             # the gathers keep the all-reduce; bench.py quotes the reason
            return None
    reg = sh._gx_calls % 2
    sh._gx_calls += 1
    seq = sh._gx_calls
    gx.wait_acks(reg, max(seq - 2, 0))                         # the previous contents of this region have been read by everyone
    mine = gx.floats(reg * sh._gx_region, need).view(Btot, D)
    _owned_rows(sh, mine, sets)
    gx.publish(reg, seq)
    slots = sh._buf(("gather_slots",), (sh.world, Btot, D))
    gx.fence()                                                 # the pulls land after the previous pass's reader of `slots`
    gx.pull_from_all(reg, seq, reg * sh._gx_region, lambda q: slots[q], ack=(reg, seq))
    gx.join()
    idx = _owner_index(sh, u_id, pos_item, neg_item, Btot)
    out = _eng.gather_rows(slots.view(sh.world * Btot, D), idx, sh.status)
    return torch.split(out, sizes)


def _gather_inference(sh, u_id, pos_item, neg_item):
    """The three row gathers with ONE exchange.  p2p transport: `_gather_p2p`.  torch.distributed: every rank copies the rows it
    owns into a zero-filled [Bu + Bp + Bn, D] buffer and one all-reduce adds the buffers - x + 0 is exact, so every rank ends
    up with the owners' bits."""
    u_lo, i_lo = (b[sh.rank] for b in sh._bounds())
    sets = [(sh.allE_u, u_id, u_lo, sh.nu), (sh.allE_i, pos_item, i_lo, sh.ni)]
    if neg_item is not None:
        sets.append((sh.allE_i, neg_item, i_lo, sh.ni))
    D = int(sh.allE_u.shape[1])
    sizes = [int(ix.numel()) for _, ix, _, _ in sets]
    outs = None
    if (sh.backend == "p2p" and sum(sizes) > 0 and os.environ.get("NGCF_DIST_GATHER", "p2p") == "p2p"
            and getattr(sh, "gather_p2p_error", None) is None):
        outs = _gather_p2p(sh, sets, sizes, D, u_id, pos_item, neg_item)
    if outs is None:
        buf = torch.zeros((sum(sizes), D), dtype=torch.float32, device=sh.dev)
        _owned_rows(sh, buf, sets)
        dist.all_reduce(buf, group=sh.group)
        outs = torch.split(buf, sizes)
    return outs[0], outs[1], (outs[2] if neg_item is not None else torch.empty(0))


def gather(sh, u_id: torch.Tensor, pos_item: torch.Tensor, neg_item: torch.Tensor):
    """(u, pos, neg) `[B, D]` on every rank.  Rows are served by their owning rank and summed."""
    dev = sh.dev
    u_id, pos_item = u_id.to(dev), pos_item.to(dev)
    if not (torch.is_grad_enabled() and (sh.allE_u.requires_grad or sh.allE_i.requires_grad)):
        return _gather_inference(sh, u_id, pos_item, neg_item.to(dev) if len(neg_item) > 0 else None)

    def served(table, owner, local, n_rows):
        mine = owner == sh.rank
        idx = torch.where(mine, local, torch.zeros_like(local))
        if table.requires_grad:                                # training path: torch indexing carries the gradient
            rows = table[idx] if n_rows else torch.zeros((idx.numel(), table.shape[1]), device=dev)
            return OwnerRowsSum.apply(rows, mine, sh.group)
        rows = _eng.gather_rows(table, idx, sh.status, 0, max(n_rows, 1)) if n_rows else \
            torch.zeros((idx.numel(), table.shape[1]), device=dev)
        return owner_rows_sum(rows, mine, sh.group)

    ub, ib = (torch.tensor(b, device=dev) for b in sh._bounds())
    sets = [(sh.allE_u, u_id, ub, sh.nu), (sh.allE_i, pos_item, ib, sh.ni)]
    if len(neg_item) > 0:
        sets.append((sh.allE_i, neg_item, ib, sh.ni))
    out = [served(table, *owner_of(bounds, ids.to(dev)), n_rows) for table, ids, bounds, n_rows in sets]
    return out[0], out[1], (out[2] if len(out) > 2 else torch.empty(0))
