"""GPU tests of the BPR loss against m negatives per positive row (csrc/bpr_multi.hip, engine.losses, BPRMulti, sampling.train_negatives,
sampling.NegativesLoader) against the float64 oracle tests/bpr_multi_oracle.py and the two identities of include/ngcf_hip.h.

Tolerances.  `mean` is measured, not fixed: the same inputs also go through the existing single-negative kernels as the expanded
batch (u and p rows repeated m times, batch_size * m; the m gradient rows of a repeated row summed in float32, as the expanded
training step sums them), and for the loss and for each gradient tensor
    max |fused - oracle|  <=  2 * max |expanded - oracle|  +  4 ulp(max |oracle|)
- an "error" is the largest absolute error of the tensor, the unit in the last place is float32's at the tensor's largest value.
Only the order of the sums differs between the two, hence the factor 2.  `softmax` has no expanded counterpart and takes the
tolerances the single-negative kernels are held to against their oracle: the loss rtol 1e-5 (tests/test_parity_gpu.py), the
gradients atol 1e-7 + 1e-5 max|want|, rtol 1e-4 (tests/test_backward_gpu.py).

Largest ratios max|fused - oracle| / (2 max|expanded - oracle| + 4 ulp) observed on the MI355X: see MEASURED below (all below 1;
with du summed in one chain of m fmas instead of four the ratio of du was 1.14 at m = 63, B = 3 - the expanded rows are summed by
a tree).
"""
import numpy as np
import pytest
import torch

import bpr_multi_oracle as orc
import ngcf_oracle as model_orc
from loss_rig import I, U, batch as _batch, dev, float64_leaves, finish, held, lap, model as _model, pkg as _pkg, step_grads  # noqa: F401

pytestmark = pytest.mark.gpu

# MEASURED on the MI355X (`pytest -s` prints one line per case): the largest value of
# max|fused - oracle| / (2 max|expanded - oracle| + 4 ulp(max|oracle|)) over every `mean` case of this file; "model": through the model
MEASURED = {"loss": 0.447, "du": 0.464, "dp": 0.656, "dn": 0.403, "model": 0.593}

BS = (1, 3, 4, 5, 1025)
DS = (1, 63, 64, 65, 260)
MS = (2, 3, 24, 63, 64)
WD, GOUT = 0.025, 3.0


def _inputs(B, m, D, seed):
    """orc.cases at a scale that keeps the scores around +-3 at every width."""
    return orc.cases(B, m, D, seed, scale=np.sqrt(3.0) / D ** 0.25)


def _fused(pkg, dev, u, p, n, m, bs, reduction, wd=WD):
    t = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in (u, p, n)]
    loss = pkg.BPRMulti(wd, bs, m, reduction)(*t)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda"
    (GOUT * loss).backward()
    return [loss.detach()] + [x.grad for x in t]


def _existing(pkg, dev, u, p, n, bs, wd=WD):
    t = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in (u, p, n)]
    loss = pkg.BPR(wd, bs)(*t)
    (GOUT * loss).backward()
    return [loss.detach()] + [x.grad for x in t]


def _held_to_expanded(name, fused, expanded, want, ratios):
    """The rule of the module docstring (loss_rig.held) for one tensor (or the loss); the comparator is the expanded batch."""
    bad = held(name, fused, expanded, want, ratios)
    assert bad is None, bad


# ---- identity (a): m = 1, mean = the existing kernels, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("B", BS)
def test_one_negative_is_the_existing_loss_and_gradients_bit_for_bit(B, dev):
    """(B = 1 025: 257 workgroup partials, the strided loop of the second stage.)"""
    pkg = _pkg()
    for D in DS:
        u, p, n = _inputs(B, 1, D, seed=100 * B + D)
        got, want = _fused(pkg, dev, u, p, n, 1, B + 2, "mean"), _existing(pkg, dev, u, p, n, B + 2)
        for name, a, b in zip(("loss", "du", "dp", "dn"), got, want):
            assert a.shape == b.shape and torch.equal(a, b), (name, B, D)
        assert torch.isfinite(got[0])


# ---- values against the float64 oracle ------------------------------------------------------------------------------------------
def _check_values(pkg, dev, B, m, D, reduction, ratios):
    u, p, n = _inputs(B, m, D, seed=B * 7 + m * 1000 + D)
    bs = B + 2
    got = [x.cpu().numpy() for x in _fused(pkg, dev, u, p, n, m, bs, reduction)]
    want = (orc.loss(u, p, n, m, WD, bs, reduction),) + orc.grads(u, p, n, m, WD, bs, reduction, GOUT)
    names = ("loss", "du", "dp", "dn")
    # the rows cases() plants: a zero dot product passes nothing but the weight decay through its score
    g = GOUT / bs
    np.testing.assert_allclose(got[2][0], g * 2 * WD * p[0].astype(np.float64), rtol=1e-6, atol=1e-30)       # dp_0: sgn(u.p) = 0
    np.testing.assert_allclose(got[3][0], g * 2 * WD / m * n[0].astype(np.float64), rtol=1e-6, atol=1e-30)   # dn_00: sgn(u.n) = 0
    if reduction == "mean":
        ue, pe = orc.expand(u, p, m)
        ex = _existing(pkg, dev, ue, pe, n, bs * m)
        ex = [ex[0].cpu().numpy(), ex[1].reshape(B, m, D).sum(1).cpu().numpy(), ex[2].reshape(B, m, D).sum(1).cpu().numpy(),
              ex[3].cpu().numpy()]
        for name, a, b, w in zip(names, got, ex, want):
            _held_to_expanded(name, a, b, w, ratios)
    else:
        assert abs(float(got[0]) - want[0]) <= 1e-5 * abs(want[0])
        for name, a, w in zip(names[1:], got[1:], want[1:]):
            assert np.isfinite(a).all()
            np.testing.assert_allclose(a, w, atol=1e-7 + 1e-5 * np.abs(w).max(), rtol=1e-4, err_msg=f"{name} B={B} m={m} D={D}")


@pytest.mark.parametrize("reduction", ["mean", "softmax"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("m", MS)
def test_values_match_the_oracle(m, B, reduction, dev):
    pkg = _pkg()
    ratios = {}
    for D in DS:
        _check_values(pkg, dev, B, m, D, reduction, ratios)
    if ratios:
        print(f"\nbpr_multi ratios m={m} B={B}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("reduction", ["mean", "softmax"])
def test_values_at_the_widest_concatenation(reduction, dev):
    """D = 1 539 = 515 + 512 + 512: 25 registers of u per lane (the 32-register kernel); and beyond 2 048 the kernel without."""
    pkg = _pkg()
    ratios = {}
    _check_values(pkg, dev, 5, 3, 1539, reduction, ratios)
    _check_values(pkg, dev, 3, 2, 2049, reduction, ratios)
    if ratios:
        print("\nbpr_multi ratios wide: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("reduction", ["mean", "softmax"])
@pytest.mark.parametrize("D", (200, 600, 1539, 2049))
def test_every_register_width_and_row_batch(D, reduction, dev):
    """The widths the grid above leaves out: 4, 16 (the only one that walks two rows at a time) and 32 registers of u per lane and
    the kernel without, each at m = 1, 3, 5, 6 and 64 - a group of four negatives cut in the middle, cut at a batch of two, and
    complete.  B = 5: two workgroups, the second with one live wave."""
    pkg = _pkg()
    ratios = {}
    for m in (1, 3, 5, 6, 64):
        _check_values(pkg, dev, 5, m, D, reduction, ratios)
    if ratios:
        print(f"\nbpr_multi ratios D={D}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def test_softmax_near_300_is_finite_and_the_oracles(dev):
    """Scores of exactly 297 .. 303 (small integers: every product and partial sum is exact in float32, in any order), both signs
    of the dot products: exp of any of them overflows float32, the loss and the gradients do not."""
    pkg = _pkg()
    B, m, D = 4, 5, 12
    u = np.full((B, D), 5.0, dtype=np.float32)
    u[:, 0] = 1.0                                                            # a full row of +-5 scores 275 + the first column's value
    p = np.zeros((B, D), dtype=np.float32)
    n = np.zeros((B, m, D), dtype=np.float32)
    for b, sp in enumerate((300, -300, 297, 303)):
        p[b, :] = np.sign(sp) * 5.0
        p[b, 0] = np.sign(sp) * (abs(sp) - 275)
        for j, sn in enumerate((298, -301, 300, 303, 12)):
            n[b, j, :] = np.sign(sn) * 5.0 if abs(sn) > 275 else 0.0
            n[b, j, 0] = np.sign(sn) * (abs(sn) - 275) if abs(sn) > 275 else sn
    n = n.reshape(B * m, D)
    assert sorted(np.abs((u * p).sum(1)).tolist()) == [297.0, 300.0, 300.0, 303.0]
    assert sorted(set(np.abs((np.repeat(u, m, 0) * n).sum(1)).tolist())) == [12.0, 298.0, 300.0, 301.0, 303.0]
    got = [x.cpu().numpy() for x in _fused(pkg, dev, u, p, n, m, B, "softmax", wd=0.0)]
    want = (orc.loss(u, p, n, m, 0.0, B, "softmax"),) + orc.grads(u, p, n, m, 0.0, B, "softmax", GOUT)
    assert np.isfinite(got[0]) and abs(float(got[0]) - want[0]) <= 1e-5 * abs(want[0])
    for a, w in zip(got[1:], want[1:]):
        assert np.isfinite(a).all()
        np.testing.assert_allclose(a, w, atol=1e-7 + 1e-5 * np.abs(w).max(), rtol=1e-4)
    mean = _fused(pkg, dev, u, p, n, m, B, "mean", wd=0.0)
    assert all(bool(torch.isfinite(x).all()) for x in mean)
    assert abs(float(mean[0]) - orc.loss(u, p, n, m, 0.0, B, "mean")) <= 1e-5 * orc.loss(u, p, n, m, 0.0, B, "mean")


@pytest.mark.parametrize("reduction", ["mean", "softmax"])
def test_two_runs_give_equal_bits(reduction, dev):
    pkg = _pkg()
    u, p, n = _inputs(1025, 24, 65, seed=9)
    a, b = (_fused(pkg, dev, u, p, n, 24, 1024, reduction) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("reduction", ["mean", "softmax"])
def test_gradient_rows_follow_the_pairs(reduction, dev):
    """dn row b*m + j belongs to the pair (b, j): per row one negative (number (3 b + 1) % m) is a multiple of the row's u, the
    others are zero vectors - their dot product is 0, so with no weight decay nothing reaches them."""
    pkg = _pkg()
    B, m, D = 9, 7, 70
    rng = np.random.default_rng(5)
    u = rng.standard_normal((B, D)).astype(np.float32) / 4
    p = rng.standard_normal((B, D)).astype(np.float32) / 4
    n = np.zeros((B, m, D), dtype=np.float32)
    marked = [(3 * b + 1) % m for b in range(B)]
    for b, j in enumerate(marked):
        n[b, j] = (b + 1) * u[b]
    n = n.reshape(B * m, D)
    _, du, dp, dn = (x.cpu().numpy() for x in _fused(pkg, dev, u, p, n, m, B, reduction, wd=0.0))
    live = sorted(np.flatnonzero(np.abs(dn).max(1) > 0).tolist())
    assert live == [b * m + j for b, j in enumerate(marked)]
    want = orc.grads(u, p, n, m, 0.0, B, reduction, GOUT)
    for b, j in enumerate(marked):
        r = b * m + j
        coef = dn[r] / u[b]                                                  # a_j * g: one number per row, positive
        assert coef.min() > 0 and np.allclose(coef, coef[0], rtol=1e-5)
    for a, w in zip((du, dp, dn), want):
        np.testing.assert_allclose(a, w, atol=1e-7 + 1e-5 * np.abs(w).max(), rtol=1e-4)


def test_wrappers_take_and_return_what_they_document(dev):
    pkg = _pkg()
    losses = pkg.engine.losses
    u, p, n = (torch.from_numpy(x).to(dev) for x in _inputs(5, 3, 65, seed=2))
    ws = pkg.engine.Workspace()
    loss = losses.bpr_multi_loss(u, p, n, 3, WD, 7, ws)
    du, dp, dn = losses.bpr_multi_backward(u, p, n, 3, WD, 7, torch.full((), GOUT, device=dev))
    ref = _fused(pkg, dev, u.cpu().numpy(), p.cpu().numpy(), n.cpu().numpy(), 3, 7, "mean")
    for a, b in zip((loss, du, dp, dn), ref):
        assert torch.equal(a, b)
    with torch.no_grad():                                                    # the plain path of the module, and strided operands
        wide = torch.zeros((15, 96), device=dev)
        wide[:, :65] = n
        assert torch.equal(pkg.BPRMulti(WD, 7, 3)(u, p, wide[:, :65]), loss)
    with pytest.raises(ValueError):
        pkg.BPRMulti(WD, 7, 2)(u, p, n)                                      # 15 rows are not 5 * 2


# ---- through the model ---------------------------------------------------------------------------------------------------------
def _step_grads(model, crit, batch, neg_ids):
    return step_grads(model, lambda mdl: crit(*mdl(node_flag=False, neg_item=neg_ids, **batch)))


def _model_oracle(model, lap, batch, neg_ids, m, wd, bs):
    """float64 autograd through the oracle's propagation and a composition of the multi-negative definition."""
    leaves, all_E = float64_leaves(model, lap)
    u, p, n = model_orc.gather_torch(all_E, U, batch["u_id"].cpu(), batch["pos_item"].cpu(), neg_ids.cpu())
    B, D = u.shape
    sp = (u * p).sum(1).abs()
    sn = torch.einsum("bd,bjd->bj", u, n.reshape(B, m, D)).abs()
    rows = -torch.nn.functional.logsigmoid(sp[:, None] - sn).mean(1)
    return finish((rows.sum() + wd * (u.pow(2).sum() + p.pow(2).sum() + n.pow(2).sum() / m)) / bs, leaves)


def test_through_the_model_against_the_expanded_call(lap, dev):
    pkg = _pkg()
    B, m = 8, 3
    batch, neg = _batch(torch.Generator().manual_seed(8), B, dev, m)
    expanded = {k: v.repeat_interleave(m) for k, v in batch.items()}
    runs = {}
    for auto in (False, True):
        model = _model(pkg, lap, dev, B, auto)
        crit = pkg.BPRMulti(WD, B, m)
        runs[auto] = [_step_grads(model, crit, batch, neg.reshape(-1)) for _ in range(3)]      # (the 2nd call captures, 2nd and 3rd replay)
        if not auto:
            want_loss, want = _model_oracle(model, lap, batch, neg.reshape(-1), m, WD, B)
            model_x = _model(pkg, lap, dev, B, False)
            ex_loss, ex = _step_grads(model_x, pkg.BPR(WD, B * m), expanded, neg.reshape(-1))
    # no optimizer step in between: the three calls of a run see the same parameters
    loss, grads = runs[False][0]
    ratios = {}
    _held_to_expanded("model", float(loss), float(ex_loss), want_loss, ratios)
    assert set(grads) == set(ex) == set(want) and "user_embedding.weight" in grads and "w2_list.2.bias" in grads
    for k in grads:
        _held_to_expanded("model", grads[k].cpu().numpy(), ex[k].cpu().numpy(), want[k], ratios)
    print(f"\nbpr_multi ratios through the model: {ratios['model']:.3f}")
    for call in (1, 2):
        assert torch.equal(runs[True][call][0], runs[False][call][0])
        assert runs[True][call][1].keys() == runs[False][call][1].keys()
        for k in grads:
            assert torch.equal(runs[True][call][1][k], runs[False][call][1][k]), (call, k)


# ---- the sampler's side ---------------------------------------------------------------------------------------------------------
def _positives(dev, n_user=50, n_item=40, per_user=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    users = torch.arange(n_user).repeat_interleave(per_user)
    items = torch.cat([torch.randperm(n_item, generator=g)[:per_user] for _ in range(n_user)])
    return users.to(dev), items.to(dev), n_user, n_item


def test_train_negatives_is_sample_unseen_and_with_one_negative_train_triplets(dev):
    pkg = _pkg()
    s = pkg.sampling
    users, items, n_user, n_item = _positives(dev)
    seen = pkg.engine.ItemSets.from_pairs(users, items, n_user, n_item)
    for epoch in (0, 2):
        a = s.train_negatives(users, items, m=1, seed=17, epoch=epoch, n_user=n_user, n_item=n_item)
        b = s.train_triplets(users, items, seed=17, epoch=epoch, n_user=n_user, n_item=n_item)
        assert a[2].shape == (users.numel(), 1) and all(torch.equal(x, y) for x, y in zip((a[0], a[1], a[2][:, 0]), b))
        neg = s.train_negatives(users, items, m=5, seed=17, epoch=epoch, n_user=n_user, n_item=n_item)[2]
        assert neg.dtype == torch.int64 and torch.equal(neg, pkg.engine.sample_unseen(seen, users, 5, s.fmix(17 + epoch)))
    with pytest.raises(ValueError):
        s.train_negatives(users, items, m=n_item - 5, seed=1, n_user=n_user, n_item=n_item)       # 34 unseen items per user


def test_negatives_loader_batches(dev):
    pkg = _pkg()
    s = pkg.sampling
    users, items, n_user, n_item = _positives(dev)
    T, m, bs = int(users.numel()), 4, 64
    age = torch.arange(T, device=dev) % 76
    seen = pkg.engine.ItemSets.from_pairs(users, items, n_user, n_item)
    dense = torch.zeros((n_user, n_item), dtype=torch.bool, device=dev)
    dense[users, items] = True
    tag = users * n_item + items                                             # identifies a positive row (unique here)
    row_of = {int(t): i for i, t in enumerate(tag.cpu())}
    assert len(row_of) == T
    for columns, drop_last in (((), True), ((users, age), False)):
        loader = s.NegativesLoader(users, items, columns, batch_size=bs, m=m, seed=23, drop_last=drop_last,
                                   generator=torch.Generator(device=dev).manual_seed(1))
        assert len(loader) == (T // bs if drop_last else -(-T // bs))
        for epoch in (0, 1):
            assert loader.epoch == epoch
            want = pkg.engine.sample_unseen(seen, users, m, s.fmix(23 + epoch))
            rows_seen = []
            batches = list(loader)
            assert len(batches) == len(loader)
            for k, batch in enumerate(batches):
                n_rows = bs if (drop_last or k < len(batches) - 1) else T - bs * (len(batches) - 1)
                assert len(batch) == (len(columns) or 1) + 2
                assert all(c.shape == (n_rows,) and c.dtype == torch.int64 and c.is_contiguous() for c in batch[:-1])
                assert batch[-1].shape == (n_rows * m,) and batch[-1].is_contiguous()
                u, it, neg = batch[0], batch[-2], batch[-1].reshape(n_rows, m)
                rows = torch.tensor([row_of[int(t)] for t in (u * n_item + it).cpu()], device=dev)
                assert torch.equal(neg, want[rows])                          # the epoch's draw, under the epoch's permutation
                if columns:
                    assert torch.equal(batch[1], age[rows])
                assert not bool(dense[u[:, None].expand(-1, m), neg].any())  # unseen for the row's user
                assert bool((neg.sort(1).values.diff(dim=1) > 0).all())      # the m of a row are distinct
                rows_seen.append(rows)
            rows_seen = torch.cat(rows_seen)
            assert rows_seen.unique().numel() == rows_seen.numel() == (T // bs * bs if drop_last else T)
            assert not torch.equal(rows_seen, torch.arange(rows_seen.numel(), device=dev))       # shuffled
    plain = s.NegativesLoader(users, items, batch_size=bs, m=m, seed=23, shuffle=False)
    first = next(iter(plain))
    assert torch.equal(first[0], users[:bs]) and torch.equal(first[2].reshape(bs, m), pkg.engine.sample_unseen(seen, users, m, s.fmix(23))[:bs])


def test_two_optimizer_steps_on_the_standin(lap, dev):
    """The loop body of Experiment.train against a NegativesLoader batch, m = 4, with the package's Adam."""
    pkg = _pkg()
    B, m = 32, 4
    g = torch.Generator().manual_seed(12)
    T = 4 * B
    users, items = torch.randint(0, U, (T,), generator=g).to(dev), torch.randint(0, I // 2, (T,), generator=g).to(dev)
    r = lambda hi: torch.randint(0, hi, (T,), generator=g).to(dev)  # noqa: E731
    columns = (torch.full((T,), 18, device=dev), users, r(76), r(2), r(13), r(32), r(7))
    seen = pkg.engine.ItemSets.from_pairs(users, items, U, I)
    loader = pkg.sampling.NegativesLoader(users, items, columns, batch_size=B, m=m, seed=5, seen=seen)
    model = _model(pkg, lap, dev, B, True)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-2)
    for reduction in ("mean", "softmax"):
        crit = pkg.BPRMulti(WD, B, m, reduction)
        seen_losses = []
        for k, (year, u_id, age, sex, month, day, dow, pos_item, neg_item) in enumerate(loader):
            if k == 2:
                break
            u, p, n = model(year, u_id, age, sex, month, day, dow, pos_item, neg_item, True)
            assert u.shape == p.shape == (B, 260) and n.shape == (B * m, 260)
            opt.zero_grad()
            loss = crit(u, p, n)
            loss.backward()
            opt.step()
            seen_losses.append(loss)
        assert len(seen_losses) == 2 and all(bool(torch.isfinite(x)) for x in seen_losses)
