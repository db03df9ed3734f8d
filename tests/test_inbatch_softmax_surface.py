"""CPU: the surface of the in-batch softmax loss - the exports and their prototypes, the refusals of the wrappers before anything
reaches the device, `sampling.item_logq` and `sampling.InBatchLoader` (plain torch: they run on the host)."""
import ctypes as C

import numpy as np
import pytest
import torch

import seoul_tourism_recommendation_ngcf_amd as pkg
from seoul_tourism_recommendation_ngcf_amd import _lib
from seoul_tourism_recommendation_ngcf_amd.engine import losses

WS = pkg.engine.Workspace()


def test_exports_and_abi():
    lib = _lib.load()
    for name in ("ngcf_inbatch_softmax_plan", "ngcf_inbatch_softmax_workspace_bytes", "ngcf_inbatch_softmax_f32",
                 "ngcf_inbatch_softmax_backward_f32"):
        assert name in _lib.PROTOTYPES and getattr(lib, name)
    assert _lib.ABI_VERSION == 11 and lib.ngcf_version() == 11
    assert "InBatchSoftmax" in pkg.__all__ and issubclass(pkg.InBatchSoftmax, torch.nn.Module)
    assert issubclass(pkg.autograd.InBatchSoftmaxLoss, torch.autograd.Function)
    for name in ("inbatch_softmax_plan", "inbatch_softmax_loss", "inbatch_softmax_backward"):
        assert callable(getattr(losses, name)) and not hasattr(pkg.engine, name)          # engine.losses, not the flat namespace
    assert callable(pkg.sampling.item_logq) and issubclass(pkg.sampling.InBatchLoader, pkg.sampling._EpochLoader)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Host pointers that are never dereferenced: every call returns NGCF_ERR_ARG from its checks."""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)

    def fwd(B=4, E=0, D=4, x=null, ids=null, xids=null, inv_tau=1.0, bs=4.0, ldu=4):
        return lib.ngcf_inbatch_softmax_f32(p, ldu, B, p, 4, x, 4, E, D, ids, xids, null, null, null, inv_tau, 0.0, bs, p, p, p, 1 << 20, null)

    def bwd(B=4, E=0, D=4, x=null, ids=null, xids=null, inv_tau=1.0, bs=4.0, du=p):
        return lib.ngcf_inbatch_softmax_backward_f32(p, 4, B, p, 4, x, 4, E, D, ids, xids, null, null, null, p, inv_tau, 0.0, bs, p, du, 4,
                                                     null, 4, null, 4, p, 1 << 20, null)

    for call in (fwd, bwd):
        for kw in (dict(B=0), dict(E=-1), dict(D=0), dict(B=(1 << 31) - 2, E=2), dict(inv_tau=0.0), dict(inv_tau=float("inf")),
                   dict(inv_tau=float("nan")), dict(bs=0.0), dict(bs=-1.0), dict(E=2, x=p, ids=p), dict(E=2)):
            assert call(**kw) == _lib.ERR_ARG, (call.__name__, kw)
            assert "inbatch_softmax" in _lib.last_error()
    assert fwd(ldu=3) == _lib.ERR_ARG and bwd(du=null) == _lib.ERR_ARG


def _rows(B=5, E=3, D=4):
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, D, generator=g), torch.randn(B, D, generator=g), torch.randn(E, D, generator=g)


@pytest.mark.parametrize("call", ["loss", "backward"])
def test_the_wrappers_refuse_before_anything_reaches_the_device(call):
    u, p, x = _rows()
    ids, xids = torch.arange(5), torch.arange(3)

    def run(u=u, p=p, inv_tau=1.0, **kw):
        if call == "loss":
            return losses.inbatch_softmax_loss(u, p, inv_tau, 0.025, 5, WS, **kw)
        return losses.inbatch_softmax_backward(u, p, inv_tau, 0.025, 5, torch.zeros(5), torch.ones(1), WS, **kw)

    # sizes: ValueError
    for kw in (dict(u=u[0]), dict(p=p[:4]), dict(p=p[:, :3]), dict(extra=x[:, :3]), dict(extra=x[0]), dict(u=u[:0], p=p[:0]),
               dict(ids=ids[:4]), dict(logq=torch.zeros(4)), dict(pos_logq=torch.zeros(5, 1)), dict(extra=x, extra_ids=xids[:2]),
               dict(extra=x, extra_logq=torch.zeros(5)), dict(extra_ids=xids), dict(ids=ids, extra=x)):
        with pytest.raises(ValueError):
            run(**kw)
    with pytest.raises(ValueError, match="extra_ids"):
        run(ids=ids, extra=x)
    # types: TypeError
    for kw in (dict(u=u.double()), dict(p=p.half()), dict(extra=x.double()), dict(ids=ids.int()), dict(extra=x, ids=ids, extra_ids=xids.int()),
               dict(logq=torch.zeros(5, dtype=torch.float16)), dict(pos_logq=torch.zeros(5, dtype=torch.int64)),
               dict(extra=x, extra_logq=torch.zeros(3, dtype=torch.bfloat16))):
        with pytest.raises(TypeError):
            run(**kw)
    # strides, then the temperature
    with pytest.raises(ValueError, match="unit stride"):
        run(u=u.t().contiguous().t())
    for t in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="inv_tau"):
            run(inv_tau=t)
    # last, the device: a size error on host tensors is reported first, a clean call on them ends at the device check
    with pytest.raises(RuntimeError, match="ROCm device"):
        run(ids=ids, logq=torch.zeros(5, dtype=torch.float64), extra=x, extra_ids=xids)


def test_the_module_refuses_a_bad_temperature_and_keeps_its_settings():
    for t in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            pkg.InBatchSoftmax(0.025, 8, temperature=t)
    crit = pkg.InBatchSoftmax(0.025, 8, temperature=0.5)
    assert (crit.weight_decay, crit.batch_size, crit.temperature) == (0.025, 8, 0.5)
    u, p, _ = _rows()
    with pytest.raises(ValueError, match="extra_ids"):                       # before the device check: host rows
        crit(u, p, item_ids=torch.arange(5), extra=torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):                   # an empty `extra` is no extra
        crit(u, p, item_ids=torch.arange(5), extra=torch.zeros(0, 4), extra_ids=torch.zeros(0, dtype=torch.int64))


def test_item_logq_is_numpy_on_a_small_column():
    items = torch.tensor([3, 1, 3, 3, 0, 1, 6])
    got = pkg.sampling.item_logq(items, 8)
    counts = np.bincount(items.numpy(), minlength=8)
    with np.errstate(divide="ignore"):
        want = np.log(counts.astype(np.float64) / 7.0).astype(np.float32)
    assert got.dtype == torch.float32 and got.shape == (8,) and np.array_equal(got.numpy(), want)
    assert np.isneginf(want[[2, 4, 5, 7]]).all() and np.isfinite(want[[0, 1, 3, 6]]).all()
    assert torch.equal(pkg.sampling.item_logq(items.int(), 8), got)
    for bad, exc in ((items.float(), ValueError), (items[:0], ValueError), (items.reshape(1, -1), ValueError)):
        with pytest.raises(exc):
            pkg.sampling.item_logq(bad, 8)
    with pytest.raises(IndexError):
        pkg.sampling.item_logq(items, 6)
    with pytest.raises(ValueError):
        pkg.sampling.item_logq(items, 0)


def test_inbatch_loader_batches():
    n, bs = 11, 4
    users, items = torch.arange(n) * 3 % 7, torch.arange(n) * 5 % 6
    cols = tuple(torch.arange(n) * 10 + q for q in range(7))                  # year, u_id, age, sex, month, day, dow
    table = pkg.sampling.item_logq(items, 6)
    ordered = pkg.sampling.InBatchLoader(users, items, cols, batch_size=bs, logq=table.double(), shuffle=False, drop_last=False)
    assert len(ordered) == 3 and ordered.epoch == 0
    for e in range(2):
        batches = list(ordered)
        assert ordered.epoch == e + 1 and [len(b) for b in batches] == [9] * 3 and [int(b[0].numel()) for b in batches] == [4, 4, 3]
        for q in range(7):
            assert torch.equal(torch.cat([b[q] for b in batches]), cols[q])
        assert torch.equal(torch.cat([b[7] for b in batches]), items) and batches[0][7].dtype == torch.int64
        lq = torch.cat([b[8] for b in batches])
        assert lq.dtype == torch.float32 and torch.equal(lq, table[items])
    plain = pkg.sampling.InBatchLoader(users, items, batch_size=bs, generator=torch.Generator().manual_seed(4))
    assert len(plain) == 2                                                    # drop_last by default
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(4))[:8]
    got = list(plain)
    assert [len(b) for b in got] == [2, 2] and plain.epoch == 1               # (users[b], items[b]) without columns and table
    assert torch.equal(torch.cat([b[0] for b in got]), users[rows]) and torch.equal(torch.cat([b[1] for b in got]), items[rows])
    with pytest.raises(ValueError):
        pkg.sampling.InBatchLoader(users, items[:5], batch_size=bs)
    with pytest.raises(ValueError):
        pkg.sampling.InBatchLoader(users, items, batch_size=0)
    with pytest.raises(ValueError):
        pkg.sampling.InBatchLoader(users, items, batch_size=bs, logq=torch.zeros(6, dtype=torch.int64))
