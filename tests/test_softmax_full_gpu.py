"""GPU tests of the softmax loss over the whole catalogue (csrc/softmax_full.hip, engine.losses, SoftmaxFull) against the float64
oracle tests/softmax_full_oracle.py.

Tolerance: measured, not fixed.  The same float32 inputs also go through the same loss in float32 torch ops on the device (`mm` with
TF32 off, `logsumexp`, autograd), and for the loss and for each of lse, dU, dI
    max |fused - oracle|  <=  2 * max |torch32 - oracle|  +  4 ulp32(max |oracle|)
- an "error" is the largest absolute error of the tensor, the unit in the last place is float32's at the tensor's largest value.
Both sides round the same float32 inputs and differ in the order of their sums only, hence the factor 2; the 4 ulp cover a
comparator that happens to be exact.  No case is excluded.  The largest ratios max|fused - oracle| / bound observed on the MI355X
are in MEASURED below (`pytest -s` prints one line per case).
"""
import numpy as np
import pytest
import torch

import softmax_full_oracle as orc
from loss_rig import (U, batch as _batch, dev, float64_leaves, finish, held as _held, lap, model as _model, pkg as _pkg,  # noqa: F401
                      step_grads, ulp32 as _ulp32)

pytestmark = pytest.mark.gpu

# MEASURED on the MI355X: the largest max|fused - oracle| / (2 max|torch32 - oracle| + 4 ulp32(max|oracle|)) per tensor over every case
# of this file that applies the rule; "model": the parameter gradients through the model
MEASURED = {"loss": 0.205, "lse": 0.432, "du": 0.641, "ditems": 0.583, "model": 0.529}

WD, GOUT = 0.025, 3.0
# B in (1, 31, 32, 33, 65) x n_items in (1, 31, 32, 33, 127, 128, 129) x D in (1, 31, 32, 33, 65, 260), crossed sparsely
EDGES = [(1, 1, 1), (31, 31, 31), (32, 32, 32), (33, 33, 33), (65, 127, 65), (1, 128, 260), (33, 129, 1), (65, 129, 260),
         (32, 127, 33), (31, 128, 65), (65, 1, 32), (1, 33, 31), (33, 31, 260), (32, 129, 31)]
# (B, n_items, D): forward and dU cut with a ragged last piece; dI cut; the first D past the slab width (tests/test_softmax_full_oracle.py
# holds the plan to these)
CUTS = [(1, 4097, 65), (4097, 33, 65), (33, 33, 513)]


def _inputs(B, n, D, seed, scale=None):
    """Rows at a scale that keeps the scores around +-3 at every width; positives at item 0, at the last item (the ragged last
    tile), repeated within the batch; the same user row twice."""
    rng = np.random.default_rng(seed)
    scale = np.sqrt(3.0) / D ** 0.25 if scale is None else scale
    u = (rng.standard_normal((B, D)) * scale).astype(np.float32)
    it = (rng.standard_normal((n, D)) * scale).astype(np.float32)
    pos = rng.integers(0, n, B)
    pos[0] = 0
    pos[-1] = n - 1
    if B >= 4:
        pos[1] = pos[2] = n - 1 - (n > 2)
        u[3] = u[2]
    return u, it, pos.astype(np.int64)


def _device_items(it, dev):
    """`items` as a row block of a wider, padded matrix whose padding is NaN: a read outside the block shows."""
    n, D = it.shape
    wide = torch.full((n + 5, D + 7), float("nan"), device=dev)
    wide[3:3 + n, :D] = torch.from_numpy(it).to(dev)
    return wide[3:3 + n, :D]


def _fused(pkg, dev, u, it, pos, tau, wd, bs, check=True, crit=None):
    """(loss, lse, du, ditems) through SoftmaxFull and autograd; lse from the engine call, whose loss has the same bits."""
    tu = torch.from_numpy(u).to(dev).requires_grad_(True)
    ti = _device_items(it, dev).requires_grad_(True)
    tp = torch.from_numpy(pos).to(dev)
    crit = crit or pkg.SoftmaxFull(wd, bs, temperature=tau, check_indices=check)
    loss = crit(tu, tp, ti)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda"
    (GOUT * loss).backward()
    loss2, lse = pkg.engine.losses.softmax_full_loss(tu.detach(), ti.detach(), tp, 1.0 / tau, wd, bs, pkg.engine.Workspace())
    assert torch.equal(loss2, loss.detach()) or (torch.isnan(loss2) and torch.isnan(loss))
    return loss.detach(), lse, tu.grad, ti.grad


def _torch32(dev, u, it, pos, tau, wd, bs):
    """The comparator: the same loss in float32 torch ops on the device, TF32 off (set and restored here)."""
    saved = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        tu = torch.from_numpy(u).to(dev).requires_grad_(True)
        ti = torch.from_numpy(it).to(dev).requires_grad_(True)
        tp = torch.from_numpy(pos).to(dev)
        s = torch.mm(tu, ti.t()) * (1.0 / tau)
        lse = torch.logsumexp(s, 1)
        loss = ((lse - s.gather(1, tp[:, None])[:, 0]).sum() + wd * (tu.pow(2).sum() + ti[tp].pow(2).sum())) / bs
        (GOUT * loss).backward()
        return loss.detach(), lse.detach(), tu.grad, ti.grad
    finally:
        torch.backends.cuda.matmul.allow_tf32 = saved


NAMES = ("loss", "lse", "du", "ditems")


def _check(pkg, dev, u, it, pos, tau, wd, bs, label):
    got = [x.cpu().numpy() for x in _fused(pkg, dev, u, it, pos, tau, wd, bs)]
    cmp_ = [x.cpu().numpy() for x in _torch32(dev, u, it, pos, tau, wd, bs)]
    w = orc.softmax_full(u, it, pos, 1.0 / tau, wd, bs, GOUT)
    ratios, bad = {}, []
    for name, a, b in zip(NAMES, got, cmp_):
        assert a.shape == b.shape == np.shape(w[name]), name
        bad.append(_held(name, a, b, w[name], ratios))
    print(f"\nsoftmax_full ratios {label}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert not any(bad), [x for x in bad if x]
    return got


@pytest.mark.parametrize("B,n,D", EDGES, ids=[f"{b}x{n}x{d}" for b, n, d in EDGES])
def test_tile_edges_match_the_oracle(B, n, D, dev):
    u, it, pos = _inputs(B, n, D, seed=B * 7 + n * 1000 + D)
    _check(_pkg(), dev, u, it, pos, 1.0, WD, B + 2, f"B={B} n={n} D={D}")
    _check(_pkg(), dev, u, it, pos, 0.5, 0.0, B, f"B={B} n={n} D={D} tau=0.5 wd=0")


@pytest.mark.parametrize("B,n,D", CUTS, ids=[f"{b}x{n}x{d}" for b, n, d in CUTS])
def test_pieces_and_slabs_match_the_oracle(B, n, D, dev):
    pkg = _pkg()
    plan = pkg.engine.losses.softmax_full_plan(B, n, D)
    assert max(plan["forward"][0], plan["du"][0], plan["ditems"][0], plan["du"][1]) >= 2
    u, it, pos = _inputs(B, n, D, seed=B + n + D)
    _check(pkg, dev, u, it, pos, 1.0, WD, B + 2, f"B={B} n={n} D={D}")


def test_scores_near_80_and_a_row_of_equal_scores(dev):
    """tau = 0.05 on unit-scale rows of width 16: scores of about +-80 and beyond, exp of which overflows float32 without the
    running maximum; user row 5 is zero, so all its scores are equal and its lse is log(n_items)."""
    B, n, D = 33, 129, 16
    u, it, pos = _inputs(B, n, D, seed=80, scale=1.0)
    u[5] = 0.0
    s = (u.astype(np.float64) @ it.astype(np.float64).T) / 0.05
    assert np.abs(s).max() > 150 and np.median(np.abs(s)) > 40
    got = _check(_pkg(), dev, u, it, pos, 0.05, WD, B, "scores +-80")
    assert all(np.isfinite(x).all() for x in got)
    assert abs(got[1][5] - np.log(n)) <= 2 * _ulp32(np.log(n))


def test_one_item_gives_exactly_zero(dev):
    pkg = _pkg()
    for B, D in ((1, 1), (33, 65), (65, 260)):
        u, it, pos = _inputs(B, 1, D, seed=B + D)
        loss, lse, du, di = _fused(pkg, dev, u, it, pos, 1.0, 0.0, B)
        assert float(loss) == 0.0 and bool((du == 0).all()) and bool((di == 0).all())
        s = torch.from_numpy(u.astype(np.float64) @ it[0].astype(np.float64))
        assert torch.allclose(lse.cpu().double(), s, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("B,n,D", [(65, 129, 260)] + CUTS, ids=lambda v: str(v))
def test_two_runs_give_equal_bits(B, n, D, dev):
    pkg = _pkg()
    u, it, pos = _inputs(B, n, D, seed=9)
    a, b = (_fused(pkg, dev, u, it, pos, 0.7, WD, B) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("B,n,D", [(33, 129, 65), (65, 100, 260), (5, 256, 33)])
def test_positive_score_has_the_bits_of_rank_topk(B, n, D, dev):
    pkg = _pkg()
    u, it, pos = _inputs(B, n, D, seed=B + 3 * n + D)
    tu, ti, tp = torch.from_numpy(u).to(dev), _device_items(it, dev), torch.from_numpy(pos).to(dev)
    spos = torch.empty(B, device=dev)
    _, lse = pkg.engine.losses.softmax_full_loss(tu, ti, tp, 1.0, 0.0, B, pkg.engine.Workspace(), spos=spos)
    val, idx = pkg.engine.ranking.rank_topk(tu, ti, n)
    at = (idx == tp[:, None]).nonzero()
    assert at.shape[0] == B and torch.equal(at[:, 0], torch.arange(B, device=dev))
    assert torch.equal(spos, val[at[:, 0], at[:, 1]])
    assert bool((spos <= val[:, 0]).all()) and bool((lse >= val[:, 0]).all())


def test_an_id_outside_the_catalogue(dev):
    pkg = _pkg()
    B, n, D = 33, 129, 65
    u, it, pos = _inputs(B, n, D, seed=21)
    good = _fused(pkg, dev, u, it, pos, 1.0, WD, B)
    for bad_id in (n, -1):
        bad = pos.copy()
        bad[7] = bad_id
        with pytest.raises(IndexError, match=str(bad_id)):
            _fused(pkg, dev, u, it, bad, 1.0, WD, B, check=True)
        crit = pkg.SoftmaxFull(WD, B, check_indices=False)
        loss, lse, du, di = _fused(pkg, dev, u, it, bad, 1.0, WD, B, crit=crit)
        assert int(crit.status.item()) == 1
        others = [b for b in range(B) if b != 7]
        assert torch.equal(lse, good[1]) and torch.equal(du[others], good[2][others])
        w = orc.softmax_full(u, it, bad, 1.0, WD, B, GOUT)
        assert abs(float(loss) - w["loss"]) <= 1e-5 * abs(w["loss"])
        np.testing.assert_allclose(di.cpu().numpy(), w["ditems"], atol=1e-7 + 1e-5 * np.abs(w["ditems"]).max(), rtol=1e-4)
        np.testing.assert_allclose(du.cpu().numpy(), w["du"], atol=1e-7 + 1e-5 * np.abs(w["du"]).max(), rtol=1e-4)
    crit = pkg.SoftmaxFull(WD, B, check_indices=False)                       # a clean batch leaves the word clear
    _fused(pkg, dev, u, it, pos, 1.0, WD, B, crit=crit)
    assert int(crit.status.item()) == 0


def test_a_nan_row_gives_a_nan_loss_and_the_process_goes_on(dev):
    pkg = _pkg()
    B, n, D = 33, 129, 65
    u, it, pos = _inputs(B, n, D, seed=22)
    u2 = u.copy()
    u2[2] = np.nan
    loss, lse, du, di = _fused(pkg, dev, u2, it, pos, 1.0, WD, B)
    assert bool(torch.isnan(loss)) and bool(torch.isnan(lse[2])) and bool(torch.isfinite(lse[[0, 1, 4]]).all())
    it2 = it.copy()
    it2[n - 1, 0] = -np.inf                                                  # a score of -inf (or NaN against a zero) faults nothing either
    _fused(pkg, dev, u, it2, pos, 1.0, WD, B)
    torch.cuda.synchronize()
    loss = _fused(pkg, dev, u, it, pos, 1.0, WD, B)[0]
    assert bool(torch.isfinite(loss))


def test_only_the_gradient_asked_for_is_computed(dev):
    pkg = _pkg()
    u, it, pos = _inputs(33, 129, 65, seed=23)
    full = _fused(pkg, dev, u, it, pos, 1.0, WD, 33)
    tp = torch.from_numpy(pos).to(dev)
    for need_u, need_i in ((True, False), (False, True)):
        tu = torch.from_numpy(u).to(dev).requires_grad_(need_u)
        ti = _device_items(it, dev).requires_grad_(need_i)
        # (the Function itself: the module refuses user rows that carry a gradient next to an item table that carries none)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        (GOUT * pkg.autograd.SoftmaxFullLoss.apply(tu, ti, tp, 1.0, WD, 33, pkg.engine.Workspace(), status)).backward()
        assert (tu.grad is not None) == need_u and (ti.grad is not None) == need_i
        assert torch.equal(tu.grad, full[2]) if need_u else torch.equal(ti.grad, full[3])
    with torch.no_grad():
        assert torch.equal(pkg.SoftmaxFull(WD, 33)(torch.from_numpy(u).to(dev), tp, _device_items(it, dev)), full[0])


# ---- through the model ---------------------------------------------------------------------------------------------------------
TAU = 0.5


def _torch_loss(u, pos, items, tau, wd, bs):
    s = torch.mm(u, items.t()) * (1.0 / tau)
    return ((torch.logsumexp(s, 1) - s.gather(1, pos[:, None])[:, 0]).sum() + wd * (u.pow(2).sum() + items[pos].pow(2).sum())) / bs


def _step_grads(model, loss_fn, batch, dev):
    def forward_and_loss(mdl):
        u, _, _ = mdl(node_flag=False, neg_item=torch.empty(0, dtype=torch.int64, device=dev), **batch)
        return loss_fn(u, batch["pos_item"], mdl.all_items_emb)
    return step_grads(model, forward_and_loss)


def _model_oracle(model, lap, batch, tau, wd, bs):
    """float64 autograd through the oracle's propagation and the loss in torch's float64 ops."""
    leaves, all_E = float64_leaves(model, lap)
    return finish(_torch_loss(all_E[batch["u_id"].cpu()], batch["pos_item"].cpu(), all_E[U:], tau, wd, bs), leaves)


def test_through_the_model_against_the_torch_composition(lap, dev):
    pkg = _pkg()
    B = 8
    batch = _batch(torch.Generator().manual_seed(8), B, dev)
    batch["pos_item"][1] = batch["pos_item"][0]                               # a duplicate positive
    crit = pkg.SoftmaxFull(WD, B, temperature=TAU)
    runs = [_step_grads(_model(pkg, lap, dev, B, False), crit, batch, dev) for _ in range(2)]
    model_x = _model(pkg, lap, dev, B, False)
    saved = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        ex_loss, ex = _step_grads(model_x, lambda u, p, items: _torch_loss(u, p, items, TAU, WD, B), batch, dev)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = saved
    want_loss, want = _model_oracle(model_x, lap, batch, TAU, WD, B)
    loss, grads = runs[0]
    ratios, bad = {}, []
    bad.append(_held("model", float(loss), float(ex_loss), want_loss, ratios))
    assert set(grads) == set(ex) == set(want) and "item_embedding.weight" in grads and "w2_list.2.bias" in grads
    for k in grads:
        bad.append(_held("model", grads[k].cpu().numpy(), ex[k].cpu().numpy(), want[k], ratios))
    print(f"\nsoftmax_full ratios through the model: {ratios['model']:.3f}")
    assert not any(bad), [x for x in bad if x]
    assert torch.equal(runs[0][0], runs[1][0])                               # two steps from equal state: the same bits
    for k in grads:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_a_replayed_forward_is_refused_by_name(lap, dev):
    """`auto_train_graph` at its default: the second call of a batch shape is the replayed one, whose item table is detached."""
    pkg = _pkg()
    B = 8
    batch = _batch(torch.Generator().manual_seed(8), B, dev)
    model = _model(pkg, lap, dev, B, None)
    assert model.auto_train_graph is True
    crit = pkg.SoftmaxFull(WD, B)
    _step_grads(model, crit, batch, dev)                                     # eager: fine
    with pytest.raises(RuntimeError, match="model.auto_train_graph = False"):
        _step_grads(model, crit, batch, dev)
