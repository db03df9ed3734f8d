"""CPU: the float64 oracle of the in-batch softmax loss (tests/inbatch_softmax_oracle.py) against torch's float64 autograd of the
same loss written with a boolean mask and `logsumexp`, against the full-catalogue oracle and the sampled-softmax oracle where the
three losses coincide, and the launch plan (`ngcf_inbatch_softmax_plan`, host only) at the shapes tests/test_inbatch_softmax_gpu.py
uses for the multi-piece and multi-slab paths."""
import numpy as np
import pytest
import torch

import inbatch_softmax_oracle as orc
import sampled_softmax_oracle as ss_orc
import softmax_full_oracle as full_orc

CASES = [(1, 0, 1), (2, 0, 3), (5, 3, 3), (33, 0, 65), (33, 31, 65), (64, 128, 20)]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300) if b.size else 0.0


def _inputs(B, E, D, seed):
    rng = np.random.default_rng(seed)
    u, p, x = (rng.standard_normal((n, D)).astype(np.float32) for n in (B, B, E))
    ids = rng.integers(0, max(2, B // 4), B)
    xids = rng.integers(0, max(2, B // 4), E)
    logq, xlogq, plq = (rng.uniform(-12, 0, n).astype(np.float32) for n in (B, E, B))
    return u, p, x, ids, xids, logq, xlogq, plq


@pytest.mark.parametrize("B,E,D", CASES)
@pytest.mark.parametrize("tau,wd", [(1.0, 0.0), (0.5, 0.025)])
@pytest.mark.parametrize("with_ids,with_q", [(True, True), (False, True), (True, False)])
def test_oracle_is_torch_float64_autograd_of_the_masked_logsumexp(B, E, D, tau, wd, with_ids, with_q):
    u, p, x, ids, xids, logq, xlogq, plq = _inputs(B, E, D, B * 1000 + E * 10 + D)
    bs, gout = B + 2, 3.0
    kw = dict(x=x)
    if with_ids:
        kw.update(ids=ids, xids=xids)
    if with_q:
        kw.update(logq=logq, xlogq=xlogq, pos_logq=plq)
    got = orc.inbatch_softmax(u, p, 1.0 / tau, wd, bs, gout, **kw)
    tu, tp, tx = (torch.from_numpy(t).double().requires_grad_(True) for t in (u, p, x))
    s = tu @ torch.cat((tp, tx)).T / tau
    eye = torch.eye(B, B + E, dtype=torch.bool)
    if with_q:
        q = torch.from_numpy(np.concatenate((logq, xlogq))).double()
        s = torch.where(eye, s - torch.from_numpy(plq).double()[:, None], s - q[None, :])
    if with_ids:
        cid = torch.from_numpy(np.concatenate((ids, xids)))
        hit = (cid[None, :] == torch.from_numpy(ids)[:, None]) & ~eye
        s = s.masked_fill(hit, float("-inf"))
        assert np.array_equal(hit.numpy(), orc.mask(B, ids, xids))
    lse = torch.logsumexp(s, 1)
    loss = ((lse - s.diagonal()).sum() + wd * (tu.pow(2).sum() + tp.pow(2).sum())) / bs
    (gout * loss).backward()
    assert rel(got["loss"], float(loss.detach())) <= 1e-12 and rel(got["lse"], lse.detach().numpy()) <= 1e-12
    assert rel(got["du"], tu.grad.numpy()) <= 1e-12 and rel(got["dp"], tp.grad.numpy()) <= 1e-12
    assert got["dx"].shape == (E, D) and (E == 0 or rel(got["dx"], tx.grad.numpy()) <= 1e-12)


@pytest.mark.parametrize("B,E,D", CASES)
def test_without_ids_and_corrections_it_is_the_full_catalogue_oracle_over_the_columns(B, E, D):
    u, p, x = _inputs(B, E, D, 7 + B + E)[:3]
    got = orc.inbatch_softmax(u, p, 2.0, 0.025, B + 1, 3.0, x=x)
    want = full_orc.softmax_full(u, np.concatenate((p, x)), np.arange(B), 2.0, 0.025, B + 1, 3.0)       # regulariser: u and the p rows
    assert rel(got["loss"], want["loss"]) <= 1e-13 and rel(got["lse"], want["lse"]) <= 1e-13
    assert rel(got["du"], want["du"]) <= 1e-13 and rel(np.concatenate((got["dp"], got["dx"])), want["ditems"]) <= 1e-13


@pytest.mark.parametrize("B,D", [(2, 3), (33, 65), (65, 20)])
def test_without_extras_and_with_distinct_ids_it_is_the_sampled_softmax_over_the_other_rows(B, D):
    u, p, _, _, _, logq, _, plq = _inputs(B, 0, D, 11 + B)
    m = B - 1
    others = np.array([[j for j in range(B) if j != b] for b in range(B)])                               # [B, m]
    got = orc.inbatch_softmax(u, p, 0.5, 0.0, B, 3.0, ids=np.arange(B), logq=logq, pos_logq=plq)
    n = p[others.reshape(-1)]
    assert rel(got["loss"], ss_orc.loss(u, p, n, logq[others], m, 0.5, 0.0, B, plq)) <= 1e-12
    du, dp, dn = ss_orc.grads(u, p, n, logq[others], m, 0.5, 0.0, B, 3.0, plq)
    np.add.at(dp, others.reshape(-1), dn)                                                                # row j is a negative of the others
    assert rel(got["du"], du) <= 1e-12 and rel(got["dp"], dp) <= 1e-12


def test_a_batch_of_one_id_leaves_the_diagonals():
    u, p, x = _inputs(5, 2, 4, 3)[:3]
    got = orc.inbatch_softmax(u, p, 1.0, 0.025, 5, 3.0, x=x, ids=np.full(5, 9), xids=np.full(2, 9))
    assert np.array_equal(np.isfinite(got["z"]), np.eye(5, 7, dtype=bool))
    assert rel(got["loss"], 0.025 * ((u.astype(np.float64) ** 2).sum() + (p.astype(np.float64) ** 2).sum()) / 5) <= 1e-15
    assert np.allclose(got["du"], 2 * 0.025 * 3.0 / 5 * u.astype(np.float64), rtol=1e-14, atol=0) and not got["dx"].any()
    with pytest.raises(ValueError):
        orc.inbatch_softmax(u, p, 1.0, 0.0, 5, x=x, ids=np.arange(5))


def _plan(B, E, D):
    from seoul_tourism_recommendation_ngcf_amd.engine import losses
    return losses.inbatch_softmax_plan(B, E, D)


def test_plan_cuts_the_shapes_the_gpu_tests_rely_on():
    """(pieces, column slabs) of the forward, dU and the columns' gradient.  rank_item_split cuts n walked rows into `want` pieces of
    whole 128-row tiles, at least 16 tiles a piece: ceil(ceil(n / 128) / s) * 128 rows each, the last one ragged."""
    from seoul_tourism_recommendation_ngcf_amd.engine import losses
    p = _plan(4097, 0, 33)                                                            # 33 tiles, 2 pieces: 17 tiles + the rest
    assert p == {"forward": (2, 1), "du": (2, 1), "dcolumns": (2, 1)}
    split = -(-(-(-4097 // 128)) // 2) * 128
    assert (split, 4097 - split) == (2176, 1921)
    p = _plan(33, 0, 513)                                                             # the first width past one slab
    assert p == {"forward": (1, 1), "du": (1, 2), "dcolumns": (1, 2)} and _plan(33, 0, 512)["du"][1] == 1
    p = _plan(33, 4064, 33)                                                           # 4 097 columns by the extras alone
    assert p["forward"][0] == 2 and p["du"][0] == 2 and p["dcolumns"][0] == 1
    assert _plan(33, 4062, 33)["forward"][0] == 1                                     # 4 095 columns: under 2 x 16 tiles, one piece
    for B, E, D in ((4097, 0, 33), (33, 0, 513), (33, 4064, 33), (512, 0, 260), (8192, 1024, 512)):
        full = losses.softmax_full_plan(B, B + E, D)
        p = _plan(B, E, D)
        assert (p["forward"], p["du"], p["dcolumns"]) == (full["forward"], full["du"], full["ditems"])
    assert _plan(512, 0, 260) == {"forward": (1, 1), "du": (1, 1), "dcolumns": (1, 1)}


def test_plan_and_workspace_refuse_bad_shapes():
    import ctypes as C
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 6)()
    for B, E, D in ((0, 5, 5), (5, -1, 5), (5, 5, 0), (-1, 5, 5), (1 << 31, 0, 5), ((1 << 31) - 5, 5, 5), (5, 1 << 31, 5)):
        assert lib.ngcf_inbatch_softmax_plan(B, E, D, out) == _lib.ERR_ARG and "inbatch_softmax_plan" in _lib.last_error()
        assert lib.ngcf_inbatch_softmax_workspace_bytes(B, E, D) == -1
    assert lib.ngcf_inbatch_softmax_plan(5, 0, 5, None) == _lib.ERR_ARG
    assert lib.ngcf_inbatch_softmax_plan((1 << 31) - 6, 5, 5, out) == _lib.OK
    for B, E, D in ((4097, 0, 33), (33, 0, 513), (33, 4064, 33), (512, 0, 260)):
        need = lib.ngcf_inbatch_softmax_workspace_bytes(B, E, D)
        assert need == lib.ngcf_softmax_full_workspace_bytes(B, B + E, D) + (B * 4 + 255) // 256 * 256       # + the forward's z_bb
