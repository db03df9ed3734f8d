"""CPU: the surface of the full-catalogue softmax loss - the C symbols and the header's text, the refusals of every layer (all
before any launch: they hold on a machine without a device), and where the new names live."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ("ngcf_softmax_full_plan", "ngcf_softmax_full_workspace_bytes", "ngcf_softmax_full_f32", "ngcf_softmax_full_backward_f32")


def _header():
    with open(os.path.join(ROOT, "include", "ngcf_hip.h")) as f:
        return f.read()


def test_symbols_are_declared_bound_and_exported():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    text = _header()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "#define NGCF_ABI_VERSION 11\n" in text and _lib.ABI_VERSION == 11 and lib.ngcf_version() == 11
    assert any(os.path.basename(s) == "softmax_full.hip" for s in _build.SOURCES)
    with open(_lib.lib_path(), "rb") as f:
        blob = f.read()
    for kernel in (b"softmax_full_fwd_kernel", b"softmax_full_rows_kernel", b"softmax_full_grad_kernel"):
        assert kernel in blob
    for words in ("Full-catalogue softmax", "fmaxf", "ascending piece order", "c_j"):
        assert words in text


GOOD = dict(ldu=8, B=4, ldi=8, n=6, D=8, inv_tau=1.0, bs=4.0, ws=1 << 20)
REFUSALS = [(dict(B=0), "B=0"), (dict(n=0), "n_items=0"), (dict(D=0), "D=0"), (dict(B=-2), "B=-2"), (dict(ldu=7), "leading"),
            (dict(ldi=7), "leading"), (dict(inv_tau=0.0), "inv_tau"), (dict(inv_tau=float("inf")), "inv_tau"),
            (dict(inv_tau=float("nan")), "inv_tau"), (dict(bs=0.0), "batch_size")]


@pytest.mark.parametrize("change,words", REFUSALS, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in REFUSALS])
def test_library_refuses_before_any_launch(change, words):
    """Without a device a launch would come back as NGCF_ERR_HIP: NGCF_ERR_ARG shows that the check came first."""
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    a = dict(GOOD, **change)
    fake = C.c_void_p(4096)
    rc = lib.ngcf_softmax_full_f32(fake, a["ldu"], a["B"], fake, a["ldi"], a["n"], a["D"], fake, a["inv_tau"], 0.1, a["bs"], fake, fake,
                                   fake, fake, fake, a["ws"], None)
    assert rc == _lib.ERR_ARG and "softmax_full:" in _lib.last_error() and words in _lib.last_error()
    rc = lib.ngcf_softmax_full_backward_f32(fake, a["ldu"], a["B"], fake, a["ldi"], a["n"], a["D"], fake, fake, a["inv_tau"], 0.1, a["bs"],
                                            fake, fake, a["D"], fake, a["D"], fake, a["ws"], None)
    assert rc == _lib.ERR_ARG and "softmax_full_backward:" in _lib.last_error() and words in _lib.last_error()


def test_library_refuses_null_pointers_and_a_short_workspace():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    fake, a = C.c_void_p(4096), GOOD
    need = lib.ngcf_softmax_full_workspace_bytes(a["B"], a["n"], a["D"])
    assert need > 0
    for ws, nbytes in ((fake, need - 1), (fake, 0), (None, need)):
        rc = lib.ngcf_softmax_full_f32(fake, 8, 4, fake, 8, 6, 8, fake, 1.0, 0.1, 4.0, fake, fake, fake, fake, ws, nbytes, None)
        assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
        rc = lib.ngcf_softmax_full_backward_f32(fake, 8, 4, fake, 8, 6, 8, fake, fake, 1.0, 0.1, 4.0, fake, fake, 8, fake, 8, ws, nbytes, None)
        assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    for hole in range(7):                                                    # users, items, pos, loss, lse, spos, status
        p = [None if i == hole else fake for i in range(7)]
        rc = lib.ngcf_softmax_full_f32(p[0], 8, 4, p[1], 8, 6, 8, p[2], 1.0, 0.1, 4.0, p[3], p[4], p[5], p[6], fake, need, None)
        assert rc == _lib.ERR_ARG and "null" in _lib.last_error()
    for hole in range(5):                                                    # users, items, pos, lse, grad_out
        p = [None if i == hole else fake for i in range(5)]
        rc = lib.ngcf_softmax_full_backward_f32(p[0], 8, 4, p[1], 8, 6, 8, p[2], p[3], 1.0, 0.1, 4.0, p[4], fake, 8, fake, 8, fake, need, None)
        assert rc == _lib.ERR_ARG and "null" in _lib.last_error()
    rc = lib.ngcf_softmax_full_backward_f32(fake, 8, 4, fake, 8, 6, 8, fake, fake, 1.0, 0.1, 4.0, fake, None, 8, None, 8, fake, need, None)
    assert rc == _lib.ERR_ARG and "null" in _lib.last_error()               # neither gradient asked for
    rc = lib.ngcf_softmax_full_backward_f32(fake, 8, 4, fake, 8, 6, 8, fake, fake, 1.0, 0.1, 4.0, fake, fake, 7, None, 8, fake, need, None)
    assert rc == _lib.ERR_ARG and "leading" in _lib.last_error()


def test_wrappers_refuse_before_the_device_is_asked_for():
    """Every refusal below is raised on CPU tensors: shapes, types and strides come first; CPU tensors themselves are refused last,
    the way `BPR` refuses them."""
    from seoul_tourism_recommendation_ngcf_amd import SoftmaxFull, engine
    losses = engine.losses
    ws = engine.Workspace()
    u, it, pos = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(4, dtype=torch.int64)
    lse, g = torch.zeros(4), torch.ones(())

    def both(u, it, pos, inv_tau=1.0):
        yield lambda: losses.softmax_full_loss(u, it, pos, inv_tau, 0.1, 4, ws)
        yield lambda: losses.softmax_full_backward(u, it, pos, lse, inv_tau, 0.1, 4, g, ws)

    for bad in ((u[0], it, pos), (u, it[0], pos), (u, it, pos[:, None]), (torch.zeros(0, 8), it, pos[:0]), (u, torch.zeros(0, 8), pos),
                (torch.zeros(4, 0), torch.zeros(6, 0), pos), (u, torch.zeros(6, 7), pos), (u, it, pos[:3])):
        for call in both(*bad):
            with pytest.raises(ValueError):
                call()
    for bad in ((u.double(), it, pos), (u, it.half(), pos), (u, it, pos.int()), (u, it, pos.float())):
        for call in both(*bad):
            with pytest.raises(TypeError):
                call()
    wide = torch.zeros(8, 16)
    for bad in ((wide[:4, ::2], it, pos), (u, torch.zeros(8, 6).t(), pos)):
        for call in both(*bad):
            with pytest.raises(ValueError, match="unit stride"):
                call()
    for inv_tau in (0.0, -1.0, float("inf"), float("nan")):
        for call in both(u, it, pos, inv_tau):
            with pytest.raises(ValueError, match="inv_tau"):
                call()
    for items in (it, wide[:6, :8]):                                         # nothing else wrong (a row block of a wider matrix is fine)
        for call in both(u, items, pos):
            with pytest.raises(RuntimeError, match="ROCm device only"):
                call()
    for req in (False, True):
        with pytest.raises(RuntimeError, match="ROCm device only"):
            SoftmaxFull(0.1, 4)(u.clone().requires_grad_(req), pos, it.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="auto_train_graph = False"):      # the replayed forward's detached item table
        SoftmaxFull(0.1, 4)(u.clone().requires_grad_(True), pos, it)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm device only"):
        SoftmaxFull(0.1, 4)(u.clone().requires_grad_(True), pos, it)
    for t in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            SoftmaxFull(0.1, 4, temperature=t)


def test_package_names():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    from seoul_tourism_recommendation_ngcf_amd import autograd, engine
    assert "SoftmaxFull" in pkg.__all__ and "BPRMulti" in pkg.__all__ and issubclass(pkg.SoftmaxFull, torch.nn.Module)
    assert str(inspect.signature(pkg.SoftmaxFull.__init__)) == "(self, weight_decay, batch_size, temperature=1.0, check_indices=True)"
    assert list(inspect.signature(pkg.SoftmaxFull.forward).parameters) == ["self", "u_embeds", "pos_item", "item_table"]
    crit = pkg.SoftmaxFull(0.025, 512, temperature=0.5, check_indices=False)
    assert (crit.weight_decay, crit.batch_size, crit.temperature, crit.check_indices) == (0.025, 512, 0.5, False)
    assert not list(crit.parameters()) and crit.status is None
    assert "auto_train_graph = False" in pkg.SoftmaxFull.__doc__ and "model.all_items_emb" in pkg.SoftmaxFull.__doc__
    assert issubclass(autograd.SoftmaxFullLoss, torch.autograd.Function)
    for name in ("softmax_full_loss", "softmax_full_backward"):
        assert callable(getattr(engine.losses, name)) and not hasattr(engine, name)
    assert list(inspect.signature(engine.losses.softmax_full_loss).parameters)[:8] == [
        "u", "items", "pos", "inv_tau", "weight_decay", "batch_size", "ws", "status"]
    assert list(inspect.signature(engine.losses.softmax_full_backward).parameters)[:9] == [
        "u", "items", "pos", "lse", "inv_tau", "weight_decay", "batch_size", "grad_out", "ws"]
