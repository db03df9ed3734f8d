"""GPU tests of the softmax loss with shared (in-batch) negatives (csrc/inbatch_softmax.hip, engine.losses, InBatchSoftmax) against
the float64 oracle tests/inbatch_softmax_oracle.py.

Tolerance: the rule of tests/test_softmax_full_gpu.py.  The same float32 inputs also go through the same loss in float32 torch ops
on the device (`mm` with TF32 off, a boolean mask, `logsumexp`, autograd), and for the loss and for each of lse, dU, dp, dx
    max |fused - oracle|  <=  2 * max |torch32 - oracle|  +  4 ulp32(max |oracle|)
- an "error" is the largest absolute error of the tensor, the unit in the last place is float32's at the tensor's largest value.
No case is excluded.  The largest ratios max|fused - oracle| / bound observed on the MI355X are in MEASURED below (`pytest -s` prints
one line per case).
"""
import functools

import numpy as np
import pytest
import torch

import inbatch_softmax_oracle as orc
from loss_rig import I, U, batch as _batch, dev, float64_leaves, finish, held as _held, lap, model as _model, pkg as _pkg, step_grads  # noqa: F401

pytestmark = pytest.mark.gpu

# MEASURED on the MI355X: the largest max|fused - oracle| / (2 max|torch32 - oracle| + 4 ulp32(max|oracle|)) per tensor over every case
# of this file that applies the rule; "model": the parameter gradients through the model
MEASURED = {"loss": 0.476, "lse": 0.327, "du": 0.829, "dp": 0.745, "dx": 0.559, "model": 0.867}

WD, GOUT = 0.025, 3.0
# B in (1, 2, 31, 32, 33, 64, 65, 129) x E in (0, 1, 31, 127, 128) x D in (1, 31, 32, 33, 65, 260), crossed sparsely; B + E = 128
# (1 + 127: the tile ends with the extras) and 129 (2 + 127, 1 + 128, 129 + 0); wherever E > 0 the positives end inside a tile
EDGES = [(1, 0, 1), (2, 0, 31), (31, 1, 32), (32, 31, 33), (33, 127, 65), (64, 128, 260), (65, 0, 260), (129, 0, 33), (1, 127, 65),
         (2, 127, 31), (1, 128, 32), (33, 31, 1), (65, 1, 31), (129, 31, 65), (31, 128, 260), (32, 0, 1), (64, 1, 33), (129, 127, 32)]
# (B, E, D): forward, dU and dC cut with a ragged last piece; the first D past the slab width; the walked side cut by the extras alone
# (tests/test_inbatch_softmax_oracle.py holds the plan to these)
CUTS = [(4097, 0, 33), (33, 0, 513), (33, 4064, 33)]
NAMES = ("loss", "lse", "du", "dp", "dx")


@functools.lru_cache(maxsize=None)
def _inputs(B, E, D, seed, scale=None, q_lo=-12.0, q_hi=0.0):
    """Rows at a scale that keeps the scores around +-3 at every width; ids from a catalogue of max(2, B // 4) items, so that rows
    share positives, and the first extra carries row 0's positive; corrections in [q_lo, q_hi]."""
    rng = np.random.default_rng(seed)
    scale = np.sqrt(3.0) / D ** 0.25 if scale is None else scale
    u, p, x = ((rng.standard_normal((n, D)) * scale).astype(np.float32) for n in (B, B, E))
    cat = max(2, B // 4)
    ids, xids = rng.integers(0, cat, B).astype(np.int64), rng.integers(0, cat, E).astype(np.int64)
    if E:
        xids[0] = ids[0]
    logq, xlogq, plq = (rng.uniform(q_lo, q_hi, n).astype(np.float32) for n in (B, E, B))
    return dict(u=u, p=p, x=x, ids=ids, xids=xids, logq=logq, xlogq=xlogq, pos_logq=plq)


def _padded(a, dev):
    """`a` as a row block of a wider, padded matrix whose padding is NaN: a read outside the block shows."""
    n, D = a.shape
    wide = torch.full((n + 5, D + 7), float("nan"), device=dev)
    wide[3:3 + n, :D] = torch.from_numpy(a).to(dev)
    return wide[3:3 + n, :D]


def _dev(v, dev):
    return None if v is None else torch.from_numpy(np.asarray(v)).to(dev)


def _fused(pkg, dev, c, tau, wd, bs, use=("ids", "q"), need=(True, True, True)):
    """(loss, lse, du, dp, dx) through InBatchSoftmax and autograd; lse from the engine call, whose loss has the same bits."""
    tu, tp, tx = (_padded(c[k], dev).requires_grad_(r) for k, r in zip(("u", "p", "x"), need))
    kw = dict(extra=tx)
    if "ids" in use:
        kw.update(item_ids=_dev(c["ids"], dev), extra_ids=_dev(c["xids"], dev))
    if "q" in use:
        kw.update(logq=_dev(c["logq"], dev), extra_logq=_dev(c["xlogq"], dev), pos_logq=_dev(c["pos_logq"], dev))
    loss = pkg.InBatchSoftmax(wd, bs, temperature=tau)(tu, tp, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda"
    (GOUT * loss).backward()
    kw["ids"] = kw.pop("item_ids", None)
    kw["extra"] = tx.detach() if tx.shape[0] else None
    loss2, lse = pkg.engine.losses.inbatch_softmax_loss(tu.detach(), tp.detach(), 1.0 / tau, wd, bs, pkg.engine.Workspace(), **kw)
    assert torch.equal(loss2, loss.detach())
    return loss.detach(), lse, tu.grad, tp.grad, tx.grad if tx.shape[0] else torch.zeros_like(tx)


def _torch32(dev, c, tau, wd, bs, use=("ids", "q")):
    """The comparator: the same loss in float32 torch ops on the device, TF32 off (set and restored here)."""
    saved = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        tu, tp, tx = (torch.from_numpy(c[k]).to(dev).requires_grad_(True) for k in ("u", "p", "x"))
        B, E = tu.shape[0], tx.shape[0]
        s = torch.mm(tu, torch.cat((tp, tx)).t()) * (1.0 / tau)
        eye = torch.eye(B, B + E, dtype=torch.bool, device=dev)
        if "q" in use:
            q = torch.cat((_dev(c["logq"], dev), _dev(c["xlogq"], dev)))
            s = torch.where(eye, s - _dev(c["pos_logq"], dev)[:, None], s - q[None, :])
        if "ids" in use:
            cid = torch.cat((_dev(c["ids"], dev), _dev(c["xids"], dev)))
            s = s.masked_fill((cid[None, :] == cid[:B, None]) & ~eye, float("-inf"))
        lse = torch.logsumexp(s, 1)
        loss = ((lse - s.diagonal()).sum() + wd * (tu.pow(2).sum() + tp.pow(2).sum())) / bs
        (GOUT * loss).backward()
        return loss.detach(), lse.detach(), tu.grad, tp.grad, tx.grad if E else torch.zeros_like(tx)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = saved


def _oracle(c, tau, wd, bs, use=("ids", "q")):
    kw = dict(x=c["x"])
    if "ids" in use:
        kw.update(ids=c["ids"], xids=c["xids"])
    if "q" in use:
        kw.update(logq=c["logq"], xlogq=c["xlogq"], pos_logq=c["pos_logq"])
    return orc.inbatch_softmax(c["u"], c["p"], 1.0 / tau, wd, bs, GOUT, **kw)


def _check(pkg, dev, c, tau, wd, bs, label, use=("ids", "q")):
    got = [t.cpu().numpy() for t in _fused(pkg, dev, c, tau, wd, bs, use)]
    cmp_ = [t.cpu().numpy() for t in _torch32(dev, c, tau, wd, bs, use)]
    w = _oracle(c, tau, wd, bs, use)
    ratios, bad = {}, []
    for name, a, b in zip(NAMES, got, cmp_):
        bad.append(_held(name, a, b, w[name], ratios))
    print(f"\ninbatch_softmax ratios {label}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert not any(bad), [t for t in bad if t]
    return got


def _mask_properties(c):
    B, E = c["u"].shape[0], c["x"].shape[0]
    hit = orc.mask(B, c["ids"], c["xids"])
    off = ~np.eye(B, B + E, dtype=bool)
    if B + E > 2:
        assert hit.any(), "no pair is masked"
        assert ((~hit) & off).any(axis=1).all(), "a row has no unmasked off-diagonal column"
    if E:
        assert hit[0, B], "the first extra is not row 0's positive"


@pytest.mark.parametrize("B,E,D", EDGES, ids=[f"{b}+{e}x{d}" for b, e, d in EDGES])
def test_tile_edges_with_masks_and_corrections_match_the_oracle(B, E, D, dev):
    c = _inputs(B, E, D, seed=B * 7 + E * 1000 + D)
    _mask_properties(c)
    _check(_pkg(), dev, c, 1.0, WD, B + 2, f"B={B} E={E} D={D}")
    _check(_pkg(), dev, c, 0.5, 0.0, B, f"B={B} E={E} D={D} tau=0.5 wd=0")


@pytest.mark.parametrize("B,E,D", CUTS, ids=[f"{b}+{e}x{d}" for b, e, d in CUTS])
def test_pieces_and_slabs_match_the_oracle(B, E, D, dev):
    pkg = _pkg()
    plan = pkg.engine.losses.inbatch_softmax_plan(B, E, D)
    assert max(plan["forward"][0], plan["du"][0], plan["dcolumns"][0], plan["du"][1]) >= 2
    c = _inputs(B, E, D, seed=B + E + D)
    _mask_properties(c)
    _check(pkg, dev, c, 1.0, WD, B + 2, f"B={B} E={E} D={D}")


def test_all_rows_share_one_id(dev):
    """Only the diagonals remain: L_b = 0 exactly, dU is the weight-decay term alone, the extras get nothing."""
    pkg = _pkg()
    B, E, D = 65, 31, 33
    c = dict(_inputs(B, E, D, seed=5))
    c["ids"], c["xids"] = np.full(B, 3, dtype=np.int64), np.full(E, 3, dtype=np.int64)
    loss, lse, du, dp, dx = _check(pkg, dev, c, 0.5, WD, B, "one id")
    assert not dx.any()
    loss0, _, du0, dp0, _ = (t.cpu().numpy() for t in _fused(pkg, dev, c, 0.5, 0.0, B))
    assert float(loss0) == 0.0 and not du0.any() and not dp0.any()
    g0 = np.float32(GOUT) / np.float32(B)
    assert np.array_equal(du, np.float32(2.0) * np.float32(WD) * g0 * c["u"])             # fmaf(2 wd g0, u, 0)


def test_scores_and_corrections_of_300_stay_finite(dev):
    B, E, D = 33, 31, 16
    c = _inputs(B, E, D, seed=300, scale=4.3, q_lo=-300.0, q_hi=300.0)
    s = c["u"].astype(np.float64) @ np.concatenate((c["p"], c["x"])).astype(np.float64).T
    assert np.abs(s).max() > 150 and max(np.abs(c["logq"]).max(), np.abs(c["pos_logq"]).max()) > 250
    got = _check(_pkg(), dev, c, 1.0, WD, B, "+-300")
    assert all(np.isfinite(t).all() for t in got)


def test_float64_corrections_give_the_bits_of_their_float32_cast(dev):
    pkg = _pkg()
    c = dict(_inputs(33, 31, 65, seed=64))
    rng = np.random.default_rng(1)
    wide = {k: rng.uniform(-12, 0, c[k].shape) for k in ("logq", "xlogq", "pos_logq")}               # float64, not float32 values
    assert any((v != v.astype(np.float32)).any() for v in wide.values())
    a = _fused(pkg, dev, {**c, **wide}, 0.5, WD, 33)
    b = _fused(pkg, dev, {**c, **{k: v.astype(np.float32) for k, v in wide.items()}}, 0.5, WD, 33)
    assert all(torch.equal(s, t) for s, t in zip(a, b))


PINS = [(1, 0, 1), (33, 127, 65), (1, 127, 65), (2, 127, 31), (129, 31, 65), (64, 128, 260), (65, 0, 260), (4097, 0, 33), (33, 4064, 33),
        (33, 0, 513)]


@pytest.mark.parametrize("B,E,D", PINS, ids=[f"{b}+{e}x{d}" for b, e, d in PINS])
def test_without_ids_and_corrections_it_has_the_bits_of_softmax_full(B, E, D, dev):
    """loss, lse, dU and cat(dp, dx) against `softmax_full_*` on cat(p, x) with pos = arange(B); all-zero corrections equal None."""
    pkg = _pkg()
    losses, ws = pkg.engine.losses, pkg.engine.Workspace()
    c = _inputs(B, E, D, seed=B + 3 * E + D)
    tau, bs = 0.7, B + 2
    got = _fused(pkg, dev, c, tau, WD, bs, use=())
    tu, items = _padded(c["u"], dev), _padded(np.concatenate((c["p"], c["x"])), dev)
    pos = torch.arange(B, device=dev)
    loss, lse = losses.softmax_full_loss(tu, items, pos, 1.0 / tau, WD, bs, ws)
    du, di = losses.softmax_full_backward(tu, items, pos, lse, 1.0 / tau, WD, bs, torch.tensor([GOUT], device=dev), ws)
    assert torch.equal(got[0], loss) and torch.equal(got[1], lse) and torch.equal(got[2], du)
    assert torch.equal(torch.cat((got[3], got[4])), di)
    zeros = {**c, **{k: np.zeros_like(c[k]) for k in ("logq", "xlogq", "pos_logq")}}
    assert all(torch.equal(s, t) for s, t in zip(got, _fused(pkg, dev, zeros, tau, WD, bs, use=("q",))))


@pytest.mark.parametrize("B,E,D", [(65, 127, 260)] + CUTS, ids=lambda v: str(v))
def test_two_runs_give_equal_bits(B, E, D, dev):
    pkg = _pkg()
    c = _inputs(B, E, D, seed=9)
    a, b = (_fused(pkg, dev, c, 0.7, WD, B) for _ in range(2))
    for s, t in zip(a, b):
        assert torch.equal(s, t)


@pytest.mark.parametrize("B,E,D", [(33, 31, 65), (4097, 0, 33)], ids=lambda v: str(v))
def test_only_the_gradients_asked_for_are_computed(B, E, D, dev):
    pkg = _pkg()
    c = _inputs(B, E, D, seed=23)
    full = _fused(pkg, dev, c, 1.0, WD, B)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        if need == (False, False, True) and E == 0:
            continue
        tu, tp, tx = (_padded(c[k], dev) for k in ("u", "p", "x"))
        lse = full[1]
        got = pkg.engine.losses.inbatch_softmax_backward(
            tu, tp, 1.0, WD, B, lse, torch.tensor([GOUT], device=dev), pkg.engine.Workspace(), *need, ids=_dev(c["ids"], dev),
            logq=_dev(c["logq"], dev), pos_logq=_dev(c["pos_logq"], dev), extra=tx if E else None,
            extra_ids=_dev(c["xids"], dev) if E else None, extra_logq=_dev(c["xlogq"], dev) if E else None)
        for k, (g, want) in enumerate(zip(got, full[2:])):
            if need[k] and (k < 2 or E):
                assert torch.equal(g, want), (need, k)
            else:
                assert g is None, (need, k)
    got = _fused(pkg, dev, c, 1.0, WD, B, need=(True, False, False))                      # autograd asks by needs_input_grad
    assert torch.equal(got[2], full[2]) and got[3] is None
    with torch.no_grad():
        crit = pkg.InBatchSoftmax(WD, B)
        kw = dict(item_ids=_dev(c["ids"], dev), logq=_dev(c["logq"], dev), pos_logq=_dev(c["pos_logq"], dev), extra=_padded(c["x"], dev),
                  extra_ids=_dev(c["xids"], dev), extra_logq=_dev(c["xlogq"], dev))
        assert torch.equal(crit(_padded(c["u"], dev), _padded(c["p"], dev), **kw), full[0])


def test_refusals_on_the_device(dev):
    pkg = _pkg()
    losses, ws = pkg.engine.losses, pkg.engine.Workspace()
    c = _inputs(5, 3, 4, seed=1)
    u, p, x = (_dev(c[k], dev) for k in ("u", "p", "x"))
    ids = _dev(c["ids"], dev)
    with pytest.raises(ValueError, match="extra_ids"):
        losses.inbatch_softmax_loss(u, p, 1.0, WD, 5, ws, ids=ids, extra=x)
    with pytest.raises(RuntimeError, match="logq is on cpu"):
        losses.inbatch_softmax_loss(u, p, 1.0, WD, 5, ws, logq=torch.zeros(5))
    with pytest.raises(ValueError, match="unit stride"):
        losses.inbatch_softmax_loss(u.t().contiguous().t(), p, 1.0, WD, 5, ws)
    loss, lse = losses.inbatch_softmax_loss(u, p, 1.0, WD, 5, ws, ids=ids)                # ids without extras: fine
    assert bool(torch.isfinite(loss)) and lse.shape == (5,)


# ---- through the model ---------------------------------------------------------------------------------------------------------
TAU = 0.5


def _rows(dev, T, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda hi: torch.randint(0, hi, (T,), generator=g).to(dev)  # noqa: E731
    users, items = r(U), r(I // 2)
    return users, items, (torch.full((T,), 18, device=dev), users, r(76), r(2), r(13), r(32), r(7))


def test_loader_steps_replayed_and_eager_give_equal_bits(lap, dev):
    """The loop of the InBatchSoftmax docstring, four Adam steps, with `auto_train_graph` on (the third call of the batch shape on is
    a replay) and off: losses and parameters bit for bit."""
    pkg = _pkg()
    B, E = 32, 5
    users, items, columns = _rows(dev, 4 * B, 12)
    table = pkg.sampling.item_logq(items, I)
    extra_ids = torch.tensor([29, 3, 17, 29, 0], device=dev)
    xlq = torch.full((E,), -float(np.log(I)), device=dev)
    runs = {}
    for auto in (True, False):
        loader = pkg.sampling.InBatchLoader(users, items, columns, batch_size=B, logq=table,
                                            generator=torch.Generator(device=dev).manual_seed(3))
        model = _model(pkg, lap, dev, B, auto)
        opt = pkg.optim.Adam(model.parameters(), lr=1e-2)
        crit = pkg.InBatchSoftmax(WD, B, temperature=TAU)
        seen = []
        for year, u_id, age, sex, month, day, dow, pos_item, lq in loader:
            u, p, x = model(year, u_id, age, sex, month, day, dow, pos_item, extra_ids, True)
            assert u.shape == p.shape == (B, 260) and x.shape == (E, 260) and lq.shape == (B,) and lq.dtype == torch.float32
            opt.zero_grad()
            loss = crit(u, p, item_ids=pos_item, logq=lq, pos_logq=lq, extra=x, extra_ids=extra_ids, extra_logq=xlq)
            loss.backward()
            opt.step()
            seen.append(loss.detach().clone())
        assert len(seen) == 4 and all(bool(torch.isfinite(t)) for t in seen)
        runs[auto] = (seen, {k: v.detach().clone() for k, v in model.named_parameters()})
    assert all(torch.equal(a, b) for a, b in zip(runs[True][0], runs[False][0]))
    for k, v in runs[False][1].items():
        assert torch.equal(runs[True][1][k], v), k


def _torch_loss(u, p, ids, lq, tau, wd, bs):
    B = u.shape[0]
    eye = torch.eye(B, dtype=torch.bool, device=u.device)
    s = torch.mm(u, p.t()) * (1.0 / tau)
    s = torch.where(eye, s - lq[:, None], s - lq[None, :])
    s = s.masked_fill((ids[None, :] == ids[:, None]) & ~eye, float("-inf"))
    return ((torch.logsumexp(s, 1) - s.diagonal()).sum() + wd * (u.pow(2).sum() + p.pow(2).sum())) / bs


def _step_grads(model, loss_fn, batch, dev):
    return step_grads(model, lambda mdl: loss_fn(*mdl(node_flag=False, neg_item=torch.empty(0, dtype=torch.int64, device=dev), **batch)[:2]))


def _model_oracle(model, lap, batch, lq, tau, wd, bs):
    """float64 autograd through the oracle's propagation and the loss in torch's float64 ops."""
    leaves, all_E = float64_leaves(model, lap)
    ids = batch["pos_item"].cpu()
    return finish(_torch_loss(all_E[batch["u_id"].cpu()], all_E[U:][ids], ids, lq.double().cpu(), tau, wd, bs), leaves)


def test_parameter_gradients_of_one_eager_step_against_the_float64_step(lap, dev):
    pkg = _pkg()
    B = 8
    g = torch.Generator().manual_seed(8)
    batch = _batch(g, B, dev)
    batch["pos_item"][1] = batch["pos_item"][0]                               # a shared positive: a masked pair
    lq = (-12.0 * torch.rand(B, generator=g)).to(dev)
    crit = pkg.InBatchSoftmax(WD, B, temperature=TAU)
    fused = lambda u, p: crit(u, p, item_ids=batch["pos_item"], logq=lq, pos_logq=lq)  # noqa: E731
    loss, grads = _step_grads(_model(pkg, lap, dev, B, False), fused, batch, dev)
    model_x = _model(pkg, lap, dev, B, False)
    saved = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        ex_loss, ex = _step_grads(model_x, lambda u, p: _torch_loss(u, p, batch["pos_item"], lq, TAU, WD, B), batch, dev)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = saved
    want_loss, want = _model_oracle(model_x, lap, batch, lq, TAU, WD, B)
    ratios, bad = {}, []
    bad.append(_held("model", float(loss), float(ex_loss), want_loss, ratios))
    assert set(grads) == set(ex) == set(want) and "item_embedding.weight" in grads and "w2_list.2.bias" in grads
    for k in grads:
        bad.append(_held("model", grads[k].cpu().numpy(), ex[k].cpu().numpy(), want[k], ratios))
    print(f"\ninbatch_softmax ratios through the model: {ratios['model']:.3f}")
    assert not any(bad), [t for t in bad if t]
