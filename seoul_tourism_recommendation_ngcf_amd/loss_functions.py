"""The five losses as `torch.autograd.Function`s: each pairs the forward and the gradient wrapper of `engine.bpr_loss` / `engine.losses`;
the modules of `bprloss` apply them when a gradient can flow.  A float64 correction goes to the wrappers as it is: they cast it."""
from __future__ import annotations

import torch

from . import engine as _eng


class BPRLoss(torch.autograd.Function):
    """Fused BPR (bprloss.py:15-22) with its gradient kernel."""

    @staticmethod
    def forward(ctx, u, p, n, weight_decay, batch_size, ws):
        ctx.wd, ctx.bs = float(weight_decay), float(batch_size)
        ctx.save_for_backward(u, p, n)
        return _eng.bpr_loss(u, p, n, weight_decay, batch_size, ws)

    @staticmethod
    def backward(ctx, g):
        return (*_eng.layers.bpr_backward(*ctx.saved_tensors, ctx.wd, ctx.bs, g), None, None, None)


class BPRMultiLoss(torch.autograd.Function):
    """BPR against m negatives per positive row (engine.losses) with its gradient kernel."""

    @staticmethod
    def forward(ctx, u, p, n, m, weight_decay, batch_size, ws, reduction):
        u, p, n = u.contiguous(), p.contiguous(), n.contiguous()
        ctx.m, ctx.wd, ctx.bs, ctx.reduction = int(m), float(weight_decay), float(batch_size), reduction
        ctx.save_for_backward(u, p, n)
        return _eng.losses.bpr_multi_loss(u, p, n, m, weight_decay, batch_size, ws, reduction)

    @staticmethod
    def backward(ctx, g):
        grads = _eng.losses.bpr_multi_backward(*ctx.saved_tensors, ctx.m, ctx.wd, ctx.bs, g.to(torch.float32).contiguous(), ctx.reduction)
        return (*grads, None, None, None, None, None)


class SampledSoftmaxLoss(torch.autograd.Function):
    """The sampled softmax with logQ correction (engine.losses) with its gradient kernel; `logq` and `pos_logq` are data."""

    @staticmethod
    def forward(ctx, u, p, n, logq, pos_logq, m, inv_tau, weight_decay, batch_size, ws):
        u, p, n = u.contiguous(), p.contiguous(), n.contiguous()
        ctx.m, ctx.inv_tau, ctx.wd, ctx.bs = int(m), float(inv_tau), float(weight_decay), float(batch_size)
        ctx.save_for_backward(u, p, n, logq, *(() if pos_logq is None else (pos_logq,)))
        return _eng.losses.sampled_softmax_loss(u, p, n, logq, m, inv_tau, weight_decay, batch_size, ws, pos_logq)

    @staticmethod
    def backward(ctx, g):
        t = ctx.saved_tensors                  # (u, p, n, logq and, when one was given, pos_logq: the wrapper's last argument)
        grads = _eng.losses.sampled_softmax_backward(*t[:4], ctx.m, ctx.inv_tau, ctx.wd, ctx.bs, g.to(torch.float32).contiguous(), *t[4:])
        return (*grads, None, None, None, None, None, None, None)


class SoftmaxFullLoss(torch.autograd.Function):
    """The softmax over the whole catalogue (engine.losses): the forward keeps `lse`, the backward recomputes the scores.  The item
    table's gradient is dense ([n_items, D]): autograd adds it to the row-sparse one of `GatherTriple` on the way to `all_E`."""

    @staticmethod
    def forward(ctx, u, items, pos, inv_tau, weight_decay, batch_size, ws, status):
        ctx.inv_tau, ctx.wd, ctx.bs, ctx.ws = float(inv_tau), float(weight_decay), float(batch_size), ws
        loss, lse = _eng.losses.softmax_full_loss(u, items, pos, inv_tau, weight_decay, batch_size, ws, status)
        ctx.save_for_backward(u, items, pos, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        grads = _eng.losses.softmax_full_backward(*ctx.saved_tensors, ctx.inv_tau, ctx.wd, ctx.bs, g.to(torch.float32).contiguous(), ctx.ws,
                                                  need_u=ctx.needs_input_grad[0], need_items=ctx.needs_input_grad[1])
        return (*grads, None, None, None, None, None, None)


class InBatchSoftmaxLoss(torch.autograd.Function):
    """The softmax with shared (in-batch) negatives (engine.losses): the forward keeps `lse`, the backward recomputes the scores and
    computes only the gradients autograd asks for.  The ids and the corrections are data; `extra` may be None."""

    @staticmethod
    def forward(ctx, u, p, extra, ids, logq, pos_logq, extra_ids, extra_logq, inv_tau, weight_decay, batch_size, ws):
        ctx.inv_tau, ctx.wd, ctx.bs, ctx.ws = float(inv_tau), float(weight_decay), float(batch_size), ws
        opt = (extra, ids, logq, pos_logq, extra_ids, extra_logq)
        ctx.given = tuple(t is not None for t in opt)
        loss, lse = _eng.losses.inbatch_softmax_loss(u, p, inv_tau, weight_decay, batch_size, ws, ids=ids, logq=logq, pos_logq=pos_logq,
                                                     extra=extra, extra_ids=extra_ids, extra_logq=extra_logq)
        ctx.save_for_backward(u, p, lse, *(t for t in opt if t is not None))
        return loss

    @staticmethod
    def backward(ctx, g):
        u, p, lse = ctx.saved_tensors[:3]
        rest = iter(ctx.saved_tensors[3:])
        extra, ids, logq, pos_logq, extra_ids, extra_logq = (next(rest) if has else None for has in ctx.given)
        du, dp, dx = _eng.losses.inbatch_softmax_backward(u, p, ctx.inv_tau, ctx.wd, ctx.bs, lse, g.to(torch.float32).contiguous(), ctx.ws,
                                                          *ctx.needs_input_grad[:3], ids=ids, logq=logq, pos_logq=pos_logq, extra=extra,
                                                          extra_ids=extra_ids, extra_logq=extra_logq)
        return (du, dp, dx) + (None,) * 9
