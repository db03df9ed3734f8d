"""Forward drivers of the propagation engine and the autograd seam of the propagation for training.

`propagate_forward` issues the HIP layer kernels for NGCF.py:120-147 (inference path, nothing saved).  `Propagate` and `GatherTriple`
are `torch.autograd.Function`s so that `loss.backward()` (experiment.py:57) reaches every parameter: their backward runs the HIP
kernels of the "backward pass" section of include/ngcf_hip.h through `engine.backward` - weight and input gradients on the fp32
matrix cores, `L^T . dLE` on the SpMM kernels; no library GEMM at any width.  all_E itself (allocation, `E0Cache`, the graph
runners' hold detection) is `all_e`'s and the five losses' Functions are `loss_functions`'s; their names are imported here for the
tests that take them from this module."""
from __future__ import annotations

from typing import Sequence

import torch

from . import engine as _eng
from .all_e import (E0Cache, _all_E_with_e0, _alloc_all_E, _final_rows, _padded_rows, _static_result_held,  # noqa: F401
                    _write_e0, static_result_baseline, static_result_counts)
from .engine.backward import (add_rows as _add_rows, bwd_input as _bwd_input, bwd_pre as _bwd_pre, bwd_weight as _bwd_weight,
                              rows_sort_unique, segment_sum_rows)
from .loss_functions import BPRLoss, BPRMultiLoss, InBatchSoftmaxLoss, SampledSoftmaxLoss, SoftmaxFullLoss  # noqa: F401

SPARSE_LAST_LAYER = True        # row-sparse backward of the last layer (Propagate.backward); False: always the dense path
DENSE_GRAD_MAX_BYTES = 32 << 20  # all_E up to this size: GatherTriple hands over a dense gradient (no host sync in the backward)
sparse_last_layer_calls = 0     # how often the row-sparse path ran (tests)


def propagate_forward(owner, csrs: Sequence["_eng.LaplacianCSR"], user_w: torch.Tensor, item_w: torch.Tensor,
                      w1, b1, w2, b2, drop: Sequence[float], seeds: Sequence[int], edge_drops=None, masks=None):
    """all_E [N, D] = [E0 | norm(E1) | ... | norm(En)] (NGCF.py:120-147), inference path.

    E0 is written once into its column block of all_E (this is both the `cat` of NGCF.py:120 and
    the one of NGCF.py:147); each layer reads its input in place and writes its normalised output
    straight into its own column block, the un-normalised carry into a ping-pong buffer.
    """
    dev = user_w.device
    U, I = int(user_w.shape[0]), int(item_w.shape[0])
    N = U + I
    d0 = int(user_w.shape[1])
    n_layer = len(w1)
    widths = [d0] + [int(w.shape[0]) for w in w1]
    all_E, prev = _all_E_with_e0(owner, user_w, item_w, N, widths, dev)
    off = d0
    for k in range(n_layer):
        d_out = widths[k + 1]
        carry = None
        if k < n_layer - 1:
            buf = owner._carry[k % 2]
            if buf is None or buf.device != dev or tuple(buf.shape) != (N, d_out):
                buf = _padded_rows(N, d_out, dev)
                owner._carry[k % 2] = buf
            carry = buf
        mk = None if masks is None else masks[k]
        if edge_drops is None:
            _eng.layer_fused(csrs[k], prev, prev, w1[k].detach(), b1[k].detach(), w2[k].detach(), b2[k].detach(),
                             carry, all_E[:, off:off + d_out], owner._ws, drop[k], seeds[k], mk)
        else:   # device-side node dropout: thinned SpMM, then the dense half
            LE = _eng.spmm(csrs[k], prev, ws=owner._ws, edge_drop=(edge_drops[k][0], edge_drops[k][1], False))
            _eng.layer_dense(LE, prev, w1[k].detach(), b1[k].detach(), w2[k].detach(), b2[k].detach(), carry,
                             all_E[:, off:off + d_out], owner._ws, drop[k], seeds[k], mk)
        prev = carry
        off += d_out
    return all_E


class Propagate(torch.autograd.Function):
    """all_E = propagate(E0; W) with a hand-written backward (NGCF.py:120-147)."""

    @staticmethod
    def forward(ctx, owner, csrs, csrs_t, drop, seeds, edge_drops, masks, n_layer, user_w, item_w, *params):
        seeds, ctx.seed_words = seeds if isinstance(seeds, tuple) else (seeds, None)
        w1, b1 = params[:n_layer], params[n_layer:2 * n_layer]
        w2, b2 = params[2 * n_layer:3 * n_layer], params[3 * n_layer:]
        dev = user_w.device
        U, I = int(user_w.shape[0]), int(item_w.shape[0])
        N, d0 = U + I, int(user_w.shape[1])
        widths = [d0] + [int(w.shape[0]) for w in w1]
        if getattr(owner, "_e0_cache", None) is not None:
            owner._e0_cache.invalidate()       # (the module's all_E is about to be replaced by one this node saves for its backward)
        all_E = _alloc_all_E(N, widths, dev)
        prev = _write_e0(owner, user_w, item_w, all_E, U, d0)
        off = d0
        ins, les, carries = [], [], []
        for k in range(n_layer):
            d_out = widths[k + 1]
            ed = None if edge_drops is None else (edge_drops[k][0], edge_drops[k][1], False)
            LE = _eng.spmm(csrs[k], prev, ws=owner._ws, edge_drop=ed)        # saved for the backward
            carry = _padded_rows(N, d_out, dev)
            _eng.layer_dense(LE, prev, w1[k].detach(), b1[k].detach(), w2[k].detach(), b2[k].detach(), carry,
                             all_E[:, off:off + d_out], owner._ws, drop[k], seeds[k], None if masks is None else masks[k])
            ins.append(prev)
            les.append(LE)
            carries.append(carry)
            prev = carry
            off += d_out
        ctx.owner, ctx.csrs, ctx.csrs_t, ctx.drop, ctx.seeds, ctx.n_layer = owner, csrs, csrs_t, drop, seeds, n_layer
        ctx.edge_drops, ctx.masks = edge_drops, masks
        ctx.widths, ctx.U = widths, U
        ctx.save_for_backward(all_E, *les, *carries, *[p.detach() for p in params])
        return all_E

    @staticmethod
    def backward(ctx, g_all):
        n, widths, U = ctx.n_layer, ctx.widths, ctx.U
        lease = getattr(ctx.csrs, "lease", None)           # reference-mode node dropout: the thinned CSRs are this forward's on loan
        if lease is not None and lease.recycled:
            raise RuntimeError("NGCF: a second backward through a forward with host-drawn node dropout, after a later forward took over "
                               "its thinned Laplacians (they are handed on once a backward has run); run the backward passes before the "
                               "next forward, or set node_dropout_mode = 'device'")
        saved = ctx.saved_tensors
        all_E = saved[0]
        les, carries = saved[1:1 + n], saved[1 + n:1 + 2 * n]
        params = saved[1 + 2 * n:]
        w1, w2 = params[:n], params[2 * n:3 * n]
        ws = ctx.owner._ws
        gw1, gb1, gw2, gb2 = [None] * n, [None] * n, [None] * n, [None] * n
        dC = None
        offs = [sum(widths[:k + 1]) for k in range(n)]
        # The gradient that reaches all_E from the row gathers is non-zero on at most 3 B rows, and GatherTriple hands it over as a
        # row-sparse tensor (rows + a compact [R, D] block of values; autograd densifies it only if another consumer of all_E
        # adds a dense gradient).  The LAST layer's backward then involves those rows only: normalise/LeakyReLU backward, both
        # weight gradients and the input gradients on a compacted [R, d] problem, and L^T . dLE as one pass over the stored entries
        # of L^T that picks the R non-zero rows of dLE through a slot table (ngcf_spmm_t_rows_f32: fixed summation order) -
        # instead of a full SpMM and four passes over 1.1 M rows.  Earlier layers are dense (their dC is), but the part of their incoming
        # gradient that comes through the normalised all_E block is still confined to the R rows: the dense pass runs with
        # dN = 0 and the R rows are redone with their dN.
        rows = gv = None
        if g_all.is_sparse:
            if SPARSE_LAST_LAYER:
                g = g_all.coalesce()
                rows, gv = g.indices()[0].contiguous(), g.values().contiguous()
            else:
                g_all = g_all.to_dense()
        if rows is None:
            g_all = g_all.contiguous()
        for k in reversed(range(n)):
            d_in, d_out = widths[k], widths[k + 1]
            E_k = all_E[:, :widths[0]] if k == 0 else carries[k - 1]
            LE_k, C_k = les[k], carries[k]
            mask_k = None if ctx.masks is None else ctx.masks[k]
            if dC is None and rows is not None:
                global sparse_last_layer_calls
                sparse_last_layer_calls += 1
                dM = _bwd_pre(gv[:, offs[k]:offs[k] + d_out], None, C_k[rows], _eng.LEAKY_SLOPE, ctx.drop[k], ctx.seeds[k],
                              None if mask_k is None else mask_k[rows], rows)
                LE_c, E_c = LE_k[rows], E_k[rows]
                gw1[k], gb1[k], gw2[k], gb2[k] = _bwd_weight(dM, LE_c, E_c, ws)
                dLE_c, dE_c = _bwd_input(dM, w1[k], w2[k], LE_c, E_c, ws)
                N = int(all_E.shape[0])
                dE = _final_rows(N, d_in, all_E.device) if k == 0 else _padded_rows(N, d_in, all_E.device)
                slot = torch.full((N,), -1, dtype=torch.int32, device=all_E.device)
                slot[rows] = torch.arange(rows.numel(), dtype=torch.int32, device=all_E.device)
                ed = None if ctx.edge_drops is None else (ctx.edge_drops[k][0], ctx.edge_drops[k][1])
                _eng.spmm_t_rows(ctx.csrs_t[k], slot, dLE_c, dE_c, dE, ws, ed)     # dE = dE_direct + (thinned L)^T . dLE, fixed order
                dC = dE
                continue
            if rows is not None:
                dM = _bwd_pre(None, dC, C_k, _eng.LEAKY_SLOPE, ctx.drop[k], ctx.seeds[k], mask_k)
                dM[rows] = _bwd_pre(gv[:, offs[k]:offs[k] + d_out], dC[rows], C_k[rows], _eng.LEAKY_SLOPE, ctx.drop[k], ctx.seeds[k],
                                    None if mask_k is None else mask_k[rows], rows)
            else:
                dM = _bwd_pre(g_all[:, offs[k]:offs[k] + d_out], dC, C_k, _eng.LEAKY_SLOPE, ctx.drop[k], ctx.seeds[k], mask_k)
            gw1[k], gb1[k], gw2[k], gb2[k] = _bwd_weight(dM, LE_k, E_k, ws)      # MFMA kernel, operand formed on the fly; biases too
            dLE, dE = _bwd_input(dM, w1[k], w2[k], LE_k, E_k, ws)                 # one MFMA kernel at any width, dS/dP never stored
            del dM
            ed = None if ctx.edge_drops is None else (ctx.edge_drops[k][0], ctx.edge_drops[k][1], True)
            S = _eng.spmm(ctx.csrs_t[k], dLE, ws=ws, edge_drop=ed)                # (thinned L)^T . dLE
            if k == 0 and dE.stride(0) != d_in:
                # The gradient of the embedding tables leaves as the row blocks dE0[:U], dE0[U:].  At a width that is not a multiple
                # of 32 (65, 130, 515: the reference's own) dE is a view of padded rows, and autograd's AccumulateGrad CLONES a
                # gradient that is not laid out like its parameter (r04 trace: 0.24 ms per step at C3, two copy kernels per step at
                # the Seoul shape); the last sum is therefore written into a contiguous matrix, whose row blocks it takes as they are.
                dE = torch.add(dE, S, out=_final_rows(int(dE.shape[0]), d_in, dE.device))
            else:
                _add_rows(dE, S)                                                  # dE += ...
            del S
            dC = dE
        dE0 = dC
        if lease is not None:
            lease.done = True                              # the next forward may take the thinned CSRs over
        if rows is not None:
            dE0.index_add_(0, rows, gv[:, :widths[0]])                           # the all_E block of E0 itself, R rows
        else:
            _add_rows(dE0, g_all[:, :widths[0]])
        return (None, None, None, None, None, None, None, None, dE0[:U], dE0[U:], *gw1, *gb1, *gw2, *gb2)


class GatherTriple(torch.autograd.Function):
    """(u, pos, neg) row gathers of NGCF.py:151-155; backward scatters into one dense gradient of all_E."""

    @staticmethod
    def forward(ctx, all_E, n_user, status, u_idx, p_idx, n_idx):
        U = int(n_user)
        n_item = int(all_E.shape[0]) - U
        u, p, n = _eng.gather_rows3(all_E, ((u_idx, 0, U), (p_idx, U, n_item), (n_idx, U, n_item)), status)
        ctx.shape, ctx.U, ctx.has_n = tuple(all_E.shape), U, n_idx is not None
        ctx.save_for_backward(u_idx, p_idx, *([n_idx] if n_idx is not None else []))
        return (u, p, n) if n is not None else (u, p)

    @staticmethod
    def backward(ctx, *grads):
        idx = ctx.saved_tensors
        N, D = ctx.shape
        offs = (0, ctx.U, ctx.U)
        live = [(g.contiguous(), ix + off) for g, ix, off in zip(grads, idx, offs) if g is not None]
        dev = idx[0].device
        if not live:
            return (torch.zeros((N, D), dtype=torch.float32, device=dev), None, None, None, None, None)
        # The gradient of all_E is non-zero on the gathered rows only (<= 3 B of N): it is handed over as a row-sparse tensor -
        # the sorted unique rows (one host sync for their count) and a compact [R, D] block the duplicates are added into -
        # instead of a zero-filled [N, D] matrix (2.3 GB at C3).  Propagate.backward works on those rows; any other consumer of
        # all_E gets the dense sum from autograd.
        # Duplicates (the same user or item several times in a batch) are added in batch order, row by row, by one kernel with a
        # fixed summation order (ngcf_segment_sum_rows_f32; r02 used float atomics and the gradients differed from run to run).
        pos_all = live[0][1] if len(live) == 1 else torch.cat([r for _, r in live])
        g_all = live[0][0] if len(live) == 1 else torch.cat([g for g, _ in live], dim=0)
        M = int(pos_all.numel())
        if M <= 8192 and N * D * 4 <= DENSE_GRAD_MAX_BYTES:
            # A SMALL graph (the Seoul data: all_E is 6 MB): a dense gradient costs nothing and the whole backward then runs
            # without a single host sync - the distinct rows, their count and the group bounds stay on the device between the
            # sort and the scatter of the segment sums into a zero-filled [N, D] matrix, and Propagate.backward takes its dense
            # path (no compaction gathers, no index_put: ~15 launches fewer per step than the row-sparse path)
            order, rows, segptr, cnt = rows_sort_unique(pos_all, N - 1)
            G = torch.zeros((N, D), dtype=torch.float32, device=dev)
            segment_sum_rows(g_all, order, segptr, M, G, rows, cnt)
            return (G, None, None, None, None, None)
        if M <= 8192 and N < (1 << 50):
            # one launch: sorted distinct rows, the positions grouped by row in batch order, the group bounds (ngcf_rows_sort_unique)
            order, rows, segptr, cnt = rows_sort_unique(pos_all, N - 1)
            R = int(cnt.item())                                    # (the one host sync of the backward: sizes the compacted problem)
            rows, segptr = rows[:R], segptr[:R + 1]
        else:
            rows, inv, counts = torch.unique(pos_all, return_inverse=True, return_counts=True)
            R = int(rows.numel())
            order = torch.sort(inv, stable=True).indices
            segptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts, 0, out=segptr[1:])
        vals = torch.empty((R, D), dtype=torch.float32, device=dev)
        segment_sum_rows(g_all, order, segptr, R, vals)
        G = torch.sparse_coo_tensor(rows[None], vals, (N, D), is_coalesced=True)
        return (G, None, None, None, None, None)


def propagate_with_grad(owner, csrs, csrs_t_fn, user_w, item_w, w1, b1, w2, b2, drop, seeds, edge_drops=None,
                        masks=None, keep_alive=None) -> torch.Tensor:
    """Inference path unless a gradient can flow; then the autograd Function (needs the CSRs of L^T)."""
    params = list(w1) + list(b1) + list(w2) + list(b2)
    need = torch.is_grad_enabled() and any(t.requires_grad for t in [user_w, item_w] + params)
    if not need:
        with torch.no_grad():
            return propagate_forward(owner, csrs, user_w, item_w, w1, b1, w2, b2, drop, seeds, edge_drops, masks)
    # (`keep_alive`: the device words behind tagged seeds - stored on the ctx so that they live as long as the backward can run)
    return Propagate.apply(owner, csrs, csrs_t_fn(), list(drop), (list(seeds), keep_alive), edge_drops, masks, len(w1), user_w, item_w,
                           *params)
