"""`BPR` - the reference's loss module (`/root/reference/model/bprloss.py:9-22`) on the fused HIP kernel.

Same constructor and `forward(u, pos, neg)` -> 0-dim tensor.  Kept quirks: the `abs` around both
scores (bprloss.py:18), the divisor is the constructor's `batch_size`, not the actual batch
(bprloss.py:22), and a `[1, D]` positive row broadcasts against `[B, D]` users
(experiment.py:96-100) while its squared norm is counted once.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import engine as _eng
from .loss_functions import BPRLoss, BPRMultiLoss, InBatchSoftmaxLoss, SampledSoftmaxLoss, SoftmaxFullLoss


def _require_temperature(name, temperature) -> float:
    t = float(temperature)
    if not (t > 0 and t < float("inf")):
        raise ValueError(f"{name}: temperature={temperature} is not a positive finite number")
    return t


def _needs_grad(*rows) -> bool:                  # (can a gradient flow into an operand?  Then the module applies its Function)
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in rows)


class BPR(nn.Module):
    def __init__(self, weight_decay, batch_size):
        super().__init__()
        self.weight_decay, self.batch_size, self._ws = weight_decay, batch_size, _eng.Workspace()

    def forward(self, u_idx, pos_idx, neg_idx):
        if _needs_grad(u_idx, pos_idx, neg_idx):
            return BPRLoss.apply(u_idx, pos_idx, neg_idx, self.weight_decay, self.batch_size, self._ws)
        return _eng.bpr_loss(u_idx.detach(), pos_idx.detach(), neg_idx.detach(), self.weight_decay,
                             self.batch_size, self._ws)


class BPRMulti(nn.Module):
    """`BPR` against `m` negatives per positive row, on the fused HIP kernels of `engine.losses`: same `forward(u, pos, neg)` ->
    0-dim tensor with `u`, `pos` [B, D] and `neg` [B*m, D], rows b*m .. b*m + m - 1 the negatives of row b - what
    `model(..., neg_item=neg.reshape(-1))` returns for `neg` [B, m] ids - instead of a batch expanded to B*m triplets.  A row's
    term is the mean of BPR's over its negatives (`reduction="mean"`: with m = 1 it is `BPR` bit for bit, at any m the value of
    `BPR(weight_decay, batch_size * m)` on the expanded batch) or the softmax of the positive score among the row's scores
    (`"softmax"`: the hardest negatives dominate the gradient).  `BPR`'s kept quirks stay - the `abs` around every score and the
    constructor's `batch_size` as the divisor; nothing broadcasts, and the negatives' squared norms count 1/m each."""

    def __init__(self, weight_decay, batch_size, m, reduction="mean"):
        super().__init__()
        self.m = _eng.losses._require_m("BPRMulti", m)
        if reduction not in _eng.losses.REDUCTIONS:
            raise ValueError(f"BPRMulti: reduction={reduction!r} is not one of {sorted(_eng.losses.REDUCTIONS)}")
        self.weight_decay, self.batch_size, self.reduction, self._ws = weight_decay, batch_size, reduction, _eng.Workspace()

    def forward(self, u_idx, pos_idx, neg_idx):
        if _needs_grad(u_idx, pos_idx, neg_idx):
            return BPRMultiLoss.apply(u_idx, pos_idx, neg_idx, self.m, self.weight_decay, self.batch_size, self._ws, self.reduction)
        return _eng.losses.bpr_multi_loss(u_idx.detach().contiguous(), pos_idx.detach().contiguous(), neg_idx.detach().contiguous(),
                                          self.m, self.weight_decay, self.batch_size, self._ws, self.reduction)


class SampledSoftmax(nn.Module):
    """The sampled softmax loss with the logQ correction, on the fused HIP kernels of `engine.losses`: the consumer of the `logq`
    that `sampling.weighted_negatives(..., return_logq=True)` and `sampling.LogQNegativesLoader` deliver.
    `forward(u, pos, neg, logq, pos_logq=None)` -> 0-dim tensor with `u`, `pos` [B, D] and `neg` [B*m, D] as `BPRMulti` takes them
    (what `model(..., neg_item=neg.reshape(-1))` returns), `logq` [B, m] or [B*m] and `pos_logq` [B] (float32 or float64).  With
    plain scores (no `abs`, as in `SoftmaxFull`) z_0 = <u_b, p_b> / temperature - pos_logq[b] and
    z_j = <u_b, n_bj> / temperature - logq[b, j - 1], a row gives logsumexp(z_0 .. z_m) - z_0: a popular item, proposed often,
    has its score lowered by the log of how often.  The regulariser and the divisor are `BPRMulti`'s: weight_decay (|u|^2 + |p|^2
    + |n|^2 / m) and the constructor's `batch_size`.

    `logq` is the log proposal probability of every slot AS ITS SAMPLER DREW IT: for the successive sampling of
    `weighted_negatives` the conditional log(w_j / U_j) given the slots before, not the marginal probability that the item is among
    the m.  No unbiasedness of the estimator of `SoftmaxFull` is claimed.  The corrections carry no gradient; non-finite values
    in them are undefined."""

    def __init__(self, weight_decay, batch_size, m, temperature=1.0):
        super().__init__()
        self.m, self.temperature = _eng.losses._require_m("SampledSoftmax", m), _require_temperature("SampledSoftmax", temperature)
        self.weight_decay, self.batch_size, self._ws = weight_decay, batch_size, _eng.Workspace()

    def forward(self, u_idx, pos_idx, neg_idx, logq, pos_logq=None):
        inv_tau = 1.0 / self.temperature
        if _needs_grad(u_idx, pos_idx, neg_idx):
            return SampledSoftmaxLoss.apply(u_idx, pos_idx, neg_idx, logq, pos_logq, self.m, inv_tau, self.weight_decay, self.batch_size,
                                            self._ws)
        return _eng.losses.sampled_softmax_loss(u_idx.detach().contiguous(), pos_idx.detach().contiguous(), neg_idx.detach().contiguous(),
                                                logq, self.m, inv_tau, self.weight_decay, self.batch_size, self._ws, pos_logq)


class SoftmaxFull(nn.Module):
    """The softmax loss over the WHOLE catalogue, the limit of `BPR` (one negative) and `BPRMulti` (m <= 64): with
    s_bj = <u_b, i_j> / temperature the loss is (sum_b (logsumexp_j s_bj - s_b,pos_b) + weight_decay (|u|^2 + sum_b |i_pos_b|^2)) /
    batch_size, on the fused HIP kernels of `engine.losses` - the [B, n_items] score matrix and its gradient are never in memory.
    Scores are plain: the `abs` of the reference's BPR is not applied (the ranking of `evaluate` has none either).

    `forward(u_embeds, pos_item, item_table)` -> 0-dim tensor: `u_embeds` [B, D] are the user rows the model returns, `pos_item`
    [B] int64 item ids, `item_table` [n_items, D] the propagated item rows.  A training loop:

        u, _, _ = model(..., pos_item=pos, neg_item=torch.empty(0), node_flag=True)
        loss = crit(u, pos, model.all_items_emb)

    The item table's gradient reaches `all_E` as a dense block and meets the row-sparse one of the gathers in autograd.  A forward
    replayed from the model's captured training graphs hands out a DETACHED `model.all_items_emb`, so the item table would silently
    get no gradient: that raises a RuntimeError - set `model.auto_train_graph = False` for loops that use this loss.

    `check_indices=True` reads the status word back after the launch and raises IndexError naming the first id outside the
    catalogue (one host sync per call, the trade of `model.check_indices`); False never syncs and leaves the sticky int32 word in
    `.status` (bit 0: some positive was out of range; such a row has no positive term)."""

    def __init__(self, weight_decay, batch_size, temperature=1.0, check_indices=True):
        super().__init__()
        self.temperature = _require_temperature("SoftmaxFull", temperature)
        self.weight_decay, self.batch_size, self._ws = weight_decay, batch_size, _eng.Workspace()
        self.check_indices, self.status = bool(check_indices), None

    def forward(self, u_embeds, pos_item, item_table):
        grad = _needs_grad(u_embeds, item_table)
        if grad and u_embeds.requires_grad and item_table.grad_fn is None and not item_table.requires_grad:
            raise RuntimeError("SoftmaxFull: item_table carries no gradient although u_embeds does - a forward replayed from the "
                               "captured training graphs returns a detached model.all_items_emb; set model.auto_train_graph = False "
                               "for loops that use this loss")
        inv_tau = 1.0 / self.temperature
        if u_embeds.is_cuda and (self.status is None or self.status.device != u_embeds.device):
            self.status = torch.zeros(1, dtype=torch.int32, device=u_embeds.device)
        if grad:
            loss = SoftmaxFullLoss.apply(u_embeds, item_table, pos_item, inv_tau, self.weight_decay, self.batch_size, self._ws, self.status)
        else:
            loss, _ = _eng.losses.softmax_full_loss(u_embeds.detach(), item_table.detach(), pos_item, inv_tau, self.weight_decay,
                                                    self.batch_size, self._ws, self.status)
        if self.check_indices and int(self.status.item()) != 0:
            self.status.zero_()
            bad = pos_item[(pos_item < 0) | (pos_item >= item_table.shape[0])]
            raise IndexError(f"SoftmaxFull: pos_item holds {int(bad[0])}, outside the catalogue of {int(item_table.shape[0])} items")
        return loss


class InBatchSoftmax(nn.Module):
    """The softmax loss with SHARED (in-batch) negatives, the default of two-tower recommenders, on the fused HIP kernels of
    `engine.losses`: every row's positive item is a negative of every other row of the batch, so no sampler is needed, a batch
    gathers 2 B rows and every row has B - 1 negatives; the [B, B + E] score matrix and its gradient are never in memory.

    `forward(u, pos, item_ids=None, logq=None, pos_logq=None, extra=None, extra_ids=None, extra_logq=None)` -> 0-dim tensor with
    `u`, `pos` [B, D] the rows the model returns and `extra` [E, D] further rows shared by the whole batch (mixed negative sampling:
    drawn by the caller, e.g. uniformly, so that an item nobody bought can be a negative too).  The columns are the positives, then
    the extras.  With plain scores (no `abs`, as in `SoftmaxFull`) s_bj = <u_b, c_j> / temperature:
        z_bb = s_bb - pos_logq[b]        z_bj = s_bj - logq[j]  or  s_bj - extra_logq[j - B]        (a correction left out is 0)
        row b gives logsumexp over its unmasked columns of z_bj, minus z_bb
    and the loss is (sum of the rows + weight_decay (|u|^2 + |pos|^2)) / batch_size: the extras are not regularised.  `logq` is the
    log of the chance that the column's item is in a batch, its popularity (`sampling.item_logq`, delivered per batch by
    `sampling.InBatchLoader`); `pos_logq = logq` is the form of Yi et al. (2019).  With `item_ids` [B] int64 (and `extra_ids` [E],
    required next to them when there are extras) a column whose item is row b's own positive - another row of the batch that bought
    the same item, or an extra that drew it - is a false negative: it leaves row b's softmax and gets no gradient from it.  The
    diagonal is never masked.  Ids are only compared, never an index; the ids and corrections carry no gradient.

    Only the gathered rows are touched, which carry their gradients through the model's captured training graphs: a loop keeps
    `model.auto_train_graph` at its default, unlike `SoftmaxFull`:

        for year, u_id, age, sex, month, day, dow, pos_item, lq in loader:                  # sampling.InBatchLoader(..., logq=table)
            u, p, x = model(year, u_id, age, sex, month, day, dow, pos_item, extra_ids, True)
            loss = crit(u, p, item_ids=pos_item, logq=lq, extra=x, extra_ids=extra_ids, extra_logq=xlq)

    Not done: masking a user's OTHER seen items, a symmetric item-to-user term, the loss inside `GraphedTrainStep`."""

    def __init__(self, weight_decay, batch_size, temperature=1.0):
        super().__init__()
        self.temperature = _require_temperature("InBatchSoftmax", temperature)
        self.weight_decay, self.batch_size, self._ws = weight_decay, batch_size, _eng.Workspace()

    def forward(self, u, pos, item_ids=None, logq=None, pos_logq=None, extra=None, extra_ids=None, extra_logq=None):
        inv_tau = 1.0 / self.temperature
        if extra is not None and extra.shape[0] == 0:
            extra = extra_ids = extra_logq = None
        if _needs_grad(u, pos, extra):
            return InBatchSoftmaxLoss.apply(u, pos, extra, item_ids, logq, pos_logq, extra_ids, extra_logq, inv_tau, self.weight_decay,
                                            self.batch_size, self._ws)
        return _eng.losses.inbatch_softmax_loss(u.detach(), pos.detach(), inv_tau, self.weight_decay, self.batch_size, self._ws,
                                                ids=item_ids, logq=logq, pos_logq=pos_logq, extra=None if extra is None else extra.detach(),
                                                extra_ids=extra_ids, extra_logq=extra_logq)[0]
