"""GPU tests of the sampled softmax loss with logQ correction (csrc/sampled_softmax.hip, engine.losses, SampledSoftmax,
sampling.LogQNegativesLoader) against the float64 oracle tests/sampled_softmax_oracle.py, against `BPRMulti(reduction="softmax")` bit
for bit where the two definitions meet, and against `SoftmaxFull` where the negatives are the whole rest of the catalogue.

Tolerances are the ones the project holds its softmax reduction to (tests/test_bpr_multi_gpu.py): the loss rtol 1e-5, the gradients
atol 1e-7 + 1e-5 max|want|, rtol 1e-4.  Through the model the float64 oracle of the whole step is met at what the whole backward is
held to (tests/test_backward_gpu.py): atol 2e-3 max|want| + 1e-9, rtol 2e-3, and the loss at rtol 1e-5.
"""
import functools

import numpy as np
import pytest
import torch

import bpr_multi_oracle as bpr_orc
import ngcf_oracle as model_orc
import sampled_softmax_oracle as orc
import softmax_full_oracle as full_orc
from loss_rig import I, U, batch as _batch, dev, float64_leaves, finish, lap, model as _model, pkg as _pkg, step_grads, ulp32 as _ulp32  # noqa: F401

pytestmark = pytest.mark.gpu

BS = (1, 3, 4, 5, 1025)
DS = (1, 63, 64, 65, 260)
MS = (1, 2, 3, 24, 63, 64)
TAUS = (1.0, 0.25)
WD, GOUT = 0.025, 3.0


def _inputs(B, m, D, seed):
    """bpr_multi_oracle.cases at the scale that keeps the scores around +-3 at every width; logq [B, m] and pos_logq [B] in [-12, 0)."""
    u, p, n = bpr_orc.cases(B, m, D, seed, scale=np.sqrt(3.0) / D ** 0.25)
    rng = np.random.default_rng(seed + 1)
    return u, p, n, rng.uniform(-12.0, 0.0, (B, m)).astype(np.float32), rng.uniform(-12.0, 0.0, B).astype(np.float32)


def _fused(pkg, dev, u, p, n, logq, m, bs, tau=1.0, pos_logq=None, wd=WD):
    t = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in (u, p, n)]
    lq = torch.from_numpy(np.asarray(logq)).to(dev)
    pq = None if pos_logq is None else torch.from_numpy(np.asarray(pos_logq)).to(dev)
    loss = pkg.SampledSoftmax(wd, bs, m, temperature=tau)(*t, lq, pq)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda"
    (GOUT * loss).backward()
    return [loss.detach()] + [x.grad for x in t]


def _multi(pkg, dev, u, p, n, m, bs, wd=WD):
    t = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in (u, p, n)]
    loss = pkg.BPRMulti(wd, bs, m, "softmax")(*t)
    (GOUT * loss).backward()
    return [loss.detach()] + [x.grad for x in t]


def _meets_the_oracle(got, u, p, n, logq, m, bs, tau, pos_logq, wd, what):
    got = [x.cpu().numpy() for x in got]
    want = (orc.loss(u, p, n, logq, m, 1 / tau, wd, bs, pos_logq),) + orc.grads(u, p, n, logq, m, 1 / tau, wd, bs, GOUT, pos_logq)
    assert np.isfinite(got[0]) and abs(float(got[0]) - want[0]) <= 1e-5 * abs(want[0]), (what, float(got[0]), want[0])
    for name, a, w in zip(("du", "dp", "dn"), got[1:], want[1:]):
        assert a.shape == w.shape and np.isfinite(a).all(), (what, name)
        np.testing.assert_allclose(a, w, atol=1e-7 + 1e-5 * np.abs(w).max(), rtol=1e-4, err_msg=f"{name} {what}")


# ---- values against the float64 oracle ------------------------------------------------------------------------------------------
def _check_values(pkg, dev, B, m, D):
    u, p, n, logq, pos_logq = _inputs(B, m, D, seed=B * 7 + m * 1000 + D)
    for tau in TAUS:
        for pq in (None, pos_logq):
            got = _fused(pkg, dev, u, p, n, logq, m, B + 2, tau, pq)
            _meets_the_oracle(got, u, p, n, logq, m, B + 2, tau, pq, WD, f"B={B} m={m} D={D} tau={tau} pos_logq={pq is not None}")


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("m", MS)
def test_values_match_the_oracle(m, B, dev):
    pkg = _pkg()
    for D in DS:
        _check_values(pkg, dev, B, m, D)


def test_values_at_the_widest_concatenation(dev):
    """D = 1 539 = 515 + 512 + 512: 25 registers of u per lane (the 32-register kernel); and beyond 2 048 the kernel without."""
    pkg = _pkg()
    _check_values(pkg, dev, 5, 3, 1539)
    _check_values(pkg, dev, 3, 2, 2049)


@pytest.mark.parametrize("D", (200, 600, 1539, 2049))
def test_every_register_width_and_row_batch(D, dev):
    """The widths the grid above leaves out: 4, 16 (the only one that walks two rows at a time) and 32 registers of u per lane and
    the kernel without, each at m = 1, 3, 5, 6 and 64 - a group of four negatives cut in the middle, cut at a batch of two, and
    complete.  B = 5: two workgroups, the second with one live wave."""
    pkg = _pkg()
    for m in (1, 3, 5, 6, 64):
        _check_values(pkg, dev, 5, m, D)


# ---- the identity with the multi-negative softmax ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 5, 1025))
def test_without_correction_it_is_the_multi_negative_softmax_bit_for_bit(B, dev):
    """inv_tau = 1, logq = 0, no pos_logq, every dot product positive: x * 1 - 0 is x and BPRMulti's sign factors are exactly 1.
    (D = 600, 1 539, 2 049 at m = 5: two rows at a time, 32 registers of u, and none.)"""
    pkg = _pkg()
    for D, ms in ((63, (1, 3, 64)), (65, (1, 3, 64)), (260, (1, 3, 64)), (600, (5,)), (1539, (5,)), (2049, (5,))):
        for m in ms:
            rng = np.random.default_rng(B * 1000 + D * 10 + m)
            u, p, n = (np.abs(rng.standard_normal(s)).astype(np.float32) / D ** 0.25 for s in ((B, D), (B, D), (B * m, D)))
            u64 = u.astype(np.float64)
            assert ((u64 * p).sum(1) > 0).all() and (np.einsum("bd,bjd->bj", u64, n.reshape(B, m, D).astype(np.float64)) > 0).all()
            want = _multi(pkg, dev, u, p, n, m, B + 2)
            for logq in (np.zeros((B, m), dtype=np.float32), np.zeros(B * m, dtype=np.float64)):
                got = _fused(pkg, dev, u, p, n, logq, m, B + 2)
                for name, a, b in zip(("loss", "du", "dp", "dn"), got, want):
                    assert a.shape == b.shape and torch.equal(a, b), (name, B, D, m)
            assert torch.isfinite(want[0])


# ---- agreement with the softmax over the whole catalogue ------------------------------------------------------------------------
@pytest.mark.parametrize("tau", (1.0, 0.5))
def test_all_other_items_as_negatives_is_the_full_softmax(tau, dev):
    """65 items, each row's negatives all items but its positive, no correction, no weight decay: both losses are the softmax over
    the catalogue.  Each meets the float64 oracle of the full softmax at this file's tolerances, hence the other at twice them."""
    pkg = _pkg()
    n_items, D, B, m = 65, 65, 5, 64
    rng = np.random.default_rng(65)
    u = (rng.standard_normal((B, D)) * np.sqrt(3.0) / D ** 0.25).astype(np.float32)
    items = (rng.standard_normal((n_items, D)) * np.sqrt(3.0) / D ** 0.25).astype(np.float32)
    pos = np.array([0, 64, 17, 17, 33])
    neg = np.stack([np.delete(np.arange(n_items), q) for q in pos])                       # [B, m]
    want = full_orc.softmax_full(u, items, pos, 1 / tau, 0.0, B, GOUT)
    sampled = [x.cpu().numpy().astype(np.float64) for x in
               _fused(pkg, dev, u, items[pos], items[neg.reshape(-1)], np.zeros((B, m), dtype=np.float32), m, B, tau, wd=0.0)]
    tu, ti = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (u, items))
    full_loss = pkg.SoftmaxFull(0.0, B, temperature=tau)(tu, torch.from_numpy(pos).to(dev), ti)
    (GOUT * full_loss).backward()
    table = np.zeros((n_items, D))
    np.add.at(table, pos, sampled[2])
    np.add.at(table, neg.reshape(-1), sampled[3])
    full = [float(full_loss.detach()), tu.grad.cpu().numpy().astype(np.float64), ti.grad.cpu().numpy().astype(np.float64)]
    for name, a, b, w in zip(("loss", "du", "ditems"), (sampled[0], sampled[1], table), full, (want["loss"], want["du"], want["ditems"])):
        w = np.asarray(w, dtype=np.float64)
        if name == "loss":
            assert abs(a - w) <= 1e-5 * abs(w) and abs(b - w) <= 1e-5 * abs(w) and abs(a - b) <= 2e-5 * abs(w)
            continue
        atol = 1e-7 + 1e-5 * np.abs(w).max()
        np.testing.assert_allclose(a, w, atol=atol, rtol=1e-4, err_msg=f"sampled {name}")
        np.testing.assert_allclose(b, w, atol=atol, rtol=1e-4, err_msg=f"full {name}")
        np.testing.assert_allclose(a, b, atol=2 * atol, rtol=2e-4, err_msg=f"sampled against full {name}")


# ---- overflow -------------------------------------------------------------------------------------------------------------------
def test_scores_and_corrections_near_300_stay_finite_and_meet_the_oracle(dev):
    """Scores of exactly +-297 .. +-303 and 12, corrections that are small integers up to +-300 (every product, partial sum and
    corrected score is exact in float32, in any order): exp of any of them overflows float32, the loss and the gradients do not."""
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
    assert (u * p).sum(1).tolist() == [300.0, -300.0, 297.0, 303.0]
    assert sorted(set((np.repeat(u, m, 0) * n).sum(1).tolist())) == [-301.0, 12.0, 298.0, 300.0, 303.0]
    logq = np.array([[0, -3, 300, -300, 2], [-300, 0, 1, 3, -299], [-2, -1, 0, 1, 2], [300, 300, 297, 299, -288]], dtype=np.float32)
    for pos_logq in (None, np.array([0, -300, 3, 300], dtype=np.float32)):
        for tau in (1.0, 0.5):
            got = _fused(pkg, dev, u, p, n, logq, m, B, tau, pos_logq, wd=0.0)
            _meets_the_oracle(got, u, p, n, logq, m, B, tau, pos_logq, 0.0, f"near 300 tau={tau} pos_logq={pos_logq is not None}")


# ---- the correction does something ----------------------------------------------------------------------------------------------
def test_a_rarely_proposed_negative_weighs_as_much_more_as_it_is_rarer(dev):
    """Two identical negative rows, proposed with probabilities 0.5 and 0.001: equal scores, so the softmax weights are as 1 : 500,
    and with no weight decay dn_j = g a_j inv_tau u - the second row is 500 times the first."""
    pkg = _pkg()
    B, m, D = 3, 2, 65
    rng = np.random.default_rng(500)
    u = rng.uniform(0.25, 1.0, (B, D)).astype(np.float32) / 4
    p = (rng.standard_normal((B, D)) / 4).astype(np.float32)
    n = np.repeat((rng.standard_normal((B, D)) / 4).astype(np.float32), m, axis=0)
    logq = np.tile(np.log(np.array([0.5, 0.001])), (B, 1))                    # float64: the wrapper casts it once
    for tau in TAUS:
        _, _, _, dn = _fused(pkg, dev, u, p, n, logq, m, B, tau, wd=0.0)
        dn = dn.cpu().numpy().astype(np.float64).reshape(B, m, D)
        assert (dn[:, 0] / u > 0).all()
        np.testing.assert_allclose(dn[:, 1] / dn[:, 0], 500.0, rtol=1e-5)
        a = orc.coefficients(u, p, n, logq, m, 1 / tau)
        np.testing.assert_allclose(a[:, 1] / a[:, 0], 500.0, rtol=1e-12)


def test_a_constant_per_row_in_both_corrections_changes_nothing(dev):
    """logq + k_b and pos_logq + k_b for an integer k_b per row (logq in multiples of 2^-10, so the shifted values are exact in
    float32): the loss moves by at most 4 ulp - only the roundings of the corrected scores differ - and the gradients stay within
    this file's tolerance of each other."""
    pkg = _pkg()
    B, m, D = 64, 24, 65
    u, p, n, _, _ = _inputs(B, m, D, seed=77)
    rng = np.random.default_rng(78)
    logq = (rng.integers(-4096, 0, (B, m)) / 1024.0).astype(np.float32)       # [-4, 0)
    pos_logq = (rng.integers(-4096, 0, B) / 1024.0).astype(np.float32)
    k = rng.integers(-2, 3, B).astype(np.float32)
    assert k.any() and ((logq + k[:, None]).astype(np.float64) == logq.astype(np.float64) + k[:, None]).all()
    for tau in TAUS:
        a = _fused(pkg, dev, u, p, n, logq, m, B, tau, pos_logq)
        b = _fused(pkg, dev, u, p, n, logq + k[:, None], m, B, tau, pos_logq + k)
        assert abs(float(a[0]) - float(b[0])) <= 4 * _ulp32(float(a[0])), (tau, float(a[0]), float(b[0]))
        for x, y in zip(a[1:], b[1:]):
            x, y = x.cpu().numpy(), y.cpu().numpy()
            np.testing.assert_allclose(y, x, atol=1e-7 + 1e-5 * np.abs(x).max(), rtol=1e-4)
        _meets_the_oracle(b, u, p, n, logq + k[:, None], m, B, tau, pos_logq + k, WD, f"shifted tau={tau}")


# ---- determinism and layout -----------------------------------------------------------------------------------------------------
def test_two_runs_give_equal_bits(dev):
    pkg = _pkg()
    u, p, n, logq, pos_logq = _inputs(1025, 24, 65, seed=9)
    a, b = (_fused(pkg, dev, u, p, n, logq, 24, 1024, 0.25, pos_logq) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_gradient_rows_and_corrections_follow_the_pairs(dev):
    """dn row b*m + j and logq[b, j] belong to the pair (b, j): per row one negative (number (3 b + 1) % m) is a multiple of the
    row's u with a correction in [-12, 0), the others are zero vectors whose correction of +200 puts their corrected score 200 below
    the positive's or lower - expf of that is exactly 0 in float32, so with no weight decay nothing reaches them."""
    pkg = _pkg()
    B, m, D = 9, 7, 70
    rng = np.random.default_rng(5)
    u = rng.standard_normal((B, D)).astype(np.float32) / 4
    p = np.abs(rng.standard_normal((B, D)).astype(np.float32) / 4) * np.sign(u + (u == 0))       # u.p > 0
    n = np.zeros((B, m, D), dtype=np.float32)
    logq = np.full((B, m), 200.0, dtype=np.float32)
    marked = [(3 * b + 1) % m for b in range(B)]
    for b, j in enumerate(marked):
        n[b, j] = (b + 1) / 4 * u[b]
        logq[b, j] = rng.uniform(-12.0, 0.0)
    n = n.reshape(B * m, D)
    got = _fused(pkg, dev, u, p, n, logq, m, B, wd=0.0)
    dn = got[3].cpu().numpy()
    live = sorted(np.flatnonzero(np.abs(dn).max(1) > 0).tolist())
    assert live == [b * m + j for b, j in enumerate(marked)]
    for b, j in enumerate(marked):
        coef = dn[b * m + j] / u[b]                                          # a_j * g: one number per row, positive
        assert coef.min() > 0 and np.allclose(coef, coef[0], rtol=1e-5)
    _meets_the_oracle(got, u, p, n, logq, m, B, 1.0, None, 0.0, "pairs")


def test_wrappers_take_and_return_what_they_document(dev):
    pkg = _pkg()
    losses = pkg.engine.losses
    un, pn, nn, lq, pq = _inputs(5, 3, 65, seed=2)
    u, p, n, logq, pos_logq = (torch.from_numpy(x).to(dev) for x in (un, pn, nn, lq, pq))
    ws = pkg.engine.Workspace()
    ref = _fused(pkg, dev, un, pn, nn, lq, 3, 7, 0.5, pq)
    for a, b in ((logq, pos_logq), (logq.reshape(-1), pos_logq), (logq.double(), pos_logq.double())):
        loss = losses.sampled_softmax_loss(u, p, n, a, 3, 2.0, WD, 7, ws, b)
        grads = losses.sampled_softmax_backward(u, p, n, a, 3, 2.0, WD, 7, torch.full((), GOUT, device=dev), pos_logq=b)
        for x, y in zip((loss,) + grads, ref):
            assert torch.equal(x, y)
    with torch.no_grad():                                                    # the plain path of the module, and strided operands
        wide = torch.zeros((15, 96), device=dev)
        wide[:, :65] = n
        assert torch.equal(pkg.SampledSoftmax(WD, 7, 3, 0.5)(u, p, wide[:, :65], logq, pos_logq), ref[0])
    assert torch.equal(losses.sampled_softmax_loss(u, p, n, logq, 3, 2.0, WD, 7, ws),           # no pos_logq is a correction of zero
                       losses.sampled_softmax_loss(u, p, n, logq, 3, 2.0, WD, 7, ws, torch.zeros(5, device=dev)))
    with pytest.raises(ValueError):
        pkg.SampledSoftmax(WD, 7, 2)(u, p, n, logq)                          # 15 rows are not 5 * 2
    with pytest.raises(RuntimeError, match="logq is on cpu"):
        losses.sampled_softmax_loss(u, p, n, logq.cpu(), 3, 2.0, WD, 7, ws)


# ---- through the model ---------------------------------------------------------------------------------------------------------
TAU = 0.5


def _step_grads(model, crit, batch, neg_ids, logq, pos_logq):
    return step_grads(model, lambda mdl: crit(*mdl(node_flag=False, neg_item=neg_ids, **batch), logq, pos_logq))


def _model_oracle(model, lap, batch, neg_ids, logq, pos_logq, m, tau, wd, bs):
    """float64 autograd through the oracle's propagation and a composition of the definition in torch's float64 ops."""
    leaves, all_E = float64_leaves(model, lap)
    u, p, n = model_orc.gather_torch(all_E, U, batch["u_id"].cpu(), batch["pos_item"].cpu(), neg_ids.cpu())
    B, D = u.shape
    z0 = (u * p).sum(1) / tau - pos_logq.double().cpu()
    zj = torch.einsum("bd,bjd->bj", u, n.reshape(B, m, D)) / tau - logq.double().cpu().reshape(B, m)
    rows = torch.logsumexp(torch.cat((z0[:, None], zj), 1), 1) - z0
    return finish((rows.sum() + wd * (u.pow(2).sum() + p.pow(2).sum() + n.pow(2).sum() / m)) / bs, leaves)


def test_through_the_model_against_the_float64_step(lap, dev):
    pkg = _pkg()
    B, m = 8, 3
    g = torch.Generator().manual_seed(8)
    batch, neg = _batch(g, B, dev, m)
    logq = (-12.0 * torch.rand((B, m), generator=g)).to(dev)
    pos_logq = (-12.0 * torch.rand(B, generator=g)).to(dev)
    runs = {}
    for auto in (False, True):
        model = _model(pkg, lap, dev, B, auto)
        crit = pkg.SampledSoftmax(WD, B, m, temperature=TAU)
        # (with auto_train_graph the 2nd call captures, the 2nd and 3rd replay; the loss itself is not part of the captured graphs)
        runs[auto] = [_step_grads(model, crit, batch, neg.reshape(-1), logq, pos_logq) for _ in range(3)]
        if not auto:
            want_loss, want = _model_oracle(model, lap, batch, neg.reshape(-1), logq, pos_logq, m, TAU, WD, B)
    # no optimizer step in between: the three calls of a run see the same parameters
    loss, grads = runs[False][0]
    assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)
    assert set(grads) == set(want) and "user_embedding.weight" in grads and "w2_list.2.bias" in grads
    for k, w in want.items():
        np.testing.assert_allclose(grads[k].cpu().numpy(), w, atol=2e-3 * np.abs(w).max() + 1e-9, rtol=2e-3, err_msg=k)
    for call in range(3):
        assert torch.equal(runs[True][call][0], runs[False][call][0])
        assert runs[True][call][1].keys() == runs[False][call][1].keys()
        for k in grads:
            assert torch.equal(runs[True][call][1][k], runs[False][call][1][k]), (call, k)


# ---- the loader -----------------------------------------------------------------------------------------------------------------
N_USER, N_ITEM, N_POS = 300, 100, 2000


@functools.lru_cache(maxsize=None)
def _positives():
    """Positives with a popular head: item ids are the squares of uniform draws, scaled."""
    g = torch.Generator().manual_seed(11)
    users = torch.randint(0, N_USER, (N_POS,), generator=g)
    items = (torch.rand(N_POS, generator=g) ** 2 * N_ITEM).long().clamp(max=N_ITEM - 1)
    return users.to("cuda:0"), items.to("cuda:0")


def test_logq_loader_batches(dev):
    """The negatives are `WeightedNegativesLoader`'s under the same seed, epoch and generator; `logq` is the epoch's
    `weighted_negatives(return_logq=True)[3].float()` under the epoch's permutation."""
    pkg = _pkg()
    sampling = pkg.sampling
    users, items = _positives()
    weights = sampling.popularity_weights(items, N_ITEM)
    m, bs = 4, 512
    used = N_POS // bs * bs
    cols = tuple(torch.arange(N_POS, device=dev) * 10 + q for q in range(7))           # year, u_id, age, sex, month, day, dow
    kw = dict(m=m, seed=99)
    gen = lambda: torch.Generator(device=dev).manual_seed(4)  # noqa: E731
    ordered = sampling.LogQNegativesLoader(users, items, weights, cols, batch_size=bs, shuffle=False, drop_last=False, **kw)
    shuffled = sampling.LogQNegativesLoader(users, items, weights, batch_size=bs, generator=gen(), **kw)
    existing = sampling.WeightedNegativesLoader(users, items, weights, batch_size=bs, generator=gen(), **kw)
    again = gen()
    assert len(ordered) == 4 and len(shuffled) == 3 and ordered.epoch == 0
    for e in range(2):
        drawn = sampling.weighted_negatives(users, items, weights, epoch=e, n_user=N_USER, n_item=N_ITEM, return_logq=True, **kw)
        want_neg, want_logq = drawn[2], drawn[3].float()
        batches = list(ordered)
        assert ordered.epoch == e + 1 and [len(b) for b in batches] == [10] * 4
        assert [int(b[0].numel()) for b in batches] == [bs, bs, bs, N_POS - used]
        for b in batches:
            rows = int(b[0].numel())
            assert all(c.shape == (rows,) and c.dtype == torch.int64 for c in b[:8])
            assert b[8].shape == b[9].shape == (rows * m,) and b[8].dtype == torch.int64 and b[9].dtype == torch.float32
            assert b[8].is_contiguous() and b[9].is_contiguous() and bool((b[9] < 0).all())
        for q in range(7):
            assert torch.equal(torch.cat([b[q] for b in batches]), cols[q])
        assert torch.equal(torch.cat([b[7] for b in batches]), items)
        assert torch.equal(torch.cat([b[8] for b in batches]).view(N_POS, m), want_neg)
        assert torch.equal(torch.cat([b[9] for b in batches]).view(N_POS, m), want_logq)
        # shuffled, without columns: (users, items, negatives, logq) at the rows the equally seeded generator gives
        rows = torch.randperm(N_POS, generator=again, device=dev)[:used]
        got, old = list(shuffled), list(existing)
        assert len(got) == len(old) == used // bs and all(len(b) == 4 for b in got) and all(len(b) == 3 for b in old)
        for b, o in zip(got, old):
            assert b[0].shape == (bs,) and b[2].shape == b[3].shape == (bs * m,)
            assert b[3].dtype == torch.float32 and b[3].is_contiguous() and bool((b[3] < 0).all())
            assert all(torch.equal(x, y) for x, y in zip(b[:3], o))
        assert torch.equal(torch.cat([b[0] for b in got]), users[rows]) and torch.equal(torch.cat([b[1] for b in got]), items[rows])
        assert torch.equal(torch.cat([b[2] for b in got]).view(used, m), want_neg[rows])
        assert torch.equal(torch.cat([b[3] for b in got]).view(used, m), want_logq[rows])
    assert not torch.equal(rows, torch.arange(used, device=dev))


def test_two_optimizer_steps_on_the_standin(lap, dev):
    """The loop body of Experiment.train against a LogQNegativesLoader batch, m = 4, with the package's Adam: one more argument."""
    pkg = _pkg()
    B, m = 32, 4
    g = torch.Generator().manual_seed(12)
    T = 4 * B
    users, items = torch.randint(0, U, (T,), generator=g).to(dev), torch.randint(0, I // 2, (T,), generator=g).to(dev)
    r = lambda hi: torch.randint(0, hi, (T,), generator=g).to(dev)  # noqa: E731
    columns = (torch.full((T,), 18, device=dev), users, r(76), r(2), r(13), r(32), r(7))
    seen = pkg.engine.ItemSets.from_pairs(users, items, U, I)
    weights = pkg.sampling.popularity_weights(items, I).clamp(min=1)        # the unseen half of the catalogue can be drawn too
    loader = pkg.sampling.LogQNegativesLoader(users, items, weights, columns, batch_size=B, m=m, seed=5, seen=seen)
    model = _model(pkg, lap, dev, B, True)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-2)
    crit = pkg.SampledSoftmax(WD, B, m, temperature=TAU)
    seen_losses = []
    for k, (year, u_id, age, sex, month, day, dow, pos_item, neg_item, logq) in enumerate(loader):
        if k == 2:
            break
        u, p, n = model(year, u_id, age, sex, month, day, dow, pos_item, neg_item, True)
        assert u.shape == p.shape == (B, 260) and n.shape == (B * m, 260) and logq.shape == (B * m,)
        opt.zero_grad()
        loss = crit(u, p, n, logq)
        loss.backward()
        opt.step()
        seen_losses.append(loss)
    assert len(seen_losses) == 2 and all(bool(torch.isfinite(x)) for x in seen_losses)
