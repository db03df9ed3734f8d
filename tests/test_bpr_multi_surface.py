"""CPU: the surface of the multi-negative BPR loss - the C symbols, the header's text, the refusals of every layer (all before any
launch: they hold on a machine without a device), and the package's new names."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ("ngcf_bpr_multi_workspace_bytes", "ngcf_bpr_multi_f32", "ngcf_bpr_multi_backward_f32")


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
    from seoul_tourism_recommendation_ngcf_amd.engine import losses, negatives
    assert re.search(r"^#define\s+NGCF_BPR_MULTI_M_MAX\s+%d\s*$" % losses.M_MAX, text, flags=re.M)
    assert losses.M_MAX == negatives.HARD_M_MAX == 64
    for name, code in losses.REDUCTIONS.items():
        assert re.search(r"^#define\s+NGCF_BPR_MULTI_%s\s+%d\s*$" % (name.upper(), code), text, flags=re.M)
    assert any(os.path.basename(s) == "bpr_multi.hip" for s in _build.SOURCES)
    with open(_lib.lib_path(), "rb") as f:
        blob = f.read()
    assert b"bpr_multi_rows_kernel" in blob and b"bpr_multi_backward_kernel" in blob


def test_workspace_is_the_two_float_partials_of_four_rows():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    assert lib.ngcf_bpr_multi_workspace_bytes(-1) == -1
    for B in (0, 1, 4, 5, 1025, 1 << 20):
        assert lib.ngcf_bpr_multi_workspace_bytes(B) >= (B + 3) // 4 * 8
        assert lib.ngcf_bpr_multi_workspace_bytes(B) == lib.ngcf_bpr_workspace_bytes(B)     # the same partials as the single-negative loss


# B, B, B*m, m, D, reduction, workspace bytes -> what the library says; the pointers are never followed
GOOD = dict(Bu=4, Bp=4, Bn=12, m=3, D=8, red=0, ws=1 << 12)
REFUSALS = [
    (dict(m=0, Bn=0), "m=0"), (dict(m=65, Bn=4 * 65), "m=65"), (dict(m=-1), "m=-1"),
    (dict(Bn=11), "4/4/11"), (dict(Bn=4), "4/4/4"), (dict(Bp=1), "4/1/12"), (dict(Bp=5), "4/5/12"), (dict(Bu=1), "1/4/12"),
    (dict(Bu=0, Bp=0, Bn=0), "0/0/0"), (dict(D=0), "D=0"), (dict(D=-3), "D=-3"), (dict(red=2), "reduction=2"), (dict(red=-1), "reduction=-1"),
]


@pytest.mark.parametrize("change,words", REFUSALS, ids=[w for _, w in REFUSALS])
def test_library_refuses_before_any_launch(change, words):
    """Without a device a launch would come back as NGCF_ERR_HIP: NGCF_ERR_ARG shows that the check came first."""
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    a = dict(GOOD, **change)
    fake = C.c_void_p(4096)
    rc = lib.ngcf_bpr_multi_f32(fake, a["Bu"], fake, a["Bp"], fake, a["Bn"], a["m"], a["D"], a["red"], 0.1, 4.0, fake, fake, a["ws"], None)
    assert rc == _lib.ERR_ARG and "bpr_multi:" in _lib.last_error() and words in _lib.last_error()
    rc = lib.ngcf_bpr_multi_backward_f32(fake, a["Bu"], fake, a["Bp"], fake, a["Bn"], a["m"], a["D"], a["red"], 0.1, 4.0, fake, fake, fake,
                                         fake, None)
    assert rc == _lib.ERR_ARG and "bpr_multi_backward:" in _lib.last_error() and words in _lib.last_error()


def test_library_refuses_null_pointers_and_a_short_workspace():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    fake, a = C.c_void_p(4096), GOOD
    need = lib.ngcf_bpr_multi_workspace_bytes(a["Bu"])
    for ws, nbytes in ((fake, need - 1), (fake, 0), (None, need)):
        rc = lib.ngcf_bpr_multi_f32(fake, a["Bu"], fake, a["Bp"], fake, a["Bn"], a["m"], a["D"], 0, 0.1, 4.0, fake, ws, nbytes, None)
        assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    for hole in range(4):
        ptrs = [None if i == hole else fake for i in range(4)]
        rc = lib.ngcf_bpr_multi_f32(ptrs[0], 4, ptrs[1], 4, ptrs[2], 12, 3, 8, 0, 0.1, 4.0, ptrs[3], fake, 1 << 12, None)
        assert rc == _lib.ERR_ARG and "null" in _lib.last_error()
    for hole in range(7):
        ptrs = [None if i == hole else fake for i in range(7)]
        rc = lib.ngcf_bpr_multi_backward_f32(ptrs[0], 4, ptrs[1], 4, ptrs[2], 12, 3, 8, 0, 0.1, 4.0, *ptrs[3:], None)
        assert rc == _lib.ERR_ARG and "null" in _lib.last_error()


def test_wrappers_refuse_before_the_device_is_asked_for():
    """Every refusal below is raised on CPU tensors: shapes, types, limits come first; CPU tensors themselves are refused last, the
    way `BPR` refuses them."""
    from seoul_tourism_recommendation_ngcf_amd import BPR, BPRMulti, engine
    losses = engine.losses
    ws = engine.Workspace()
    u, p, n = torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(12, 8)
    g = torch.ones(())

    def both(u, p, n, m, reduction="mean"):
        yield lambda: losses.bpr_multi_loss(u, p, n, m, 0.1, 4, ws, reduction)
        yield lambda: losses.bpr_multi_backward(u, p, n, m, 0.1, 4, g, reduction)

    for m in (0, 65, -1, 2.5):
        for call in both(u, p, torch.zeros(max(int(4 * m), 0), 8), m):
            with pytest.raises(ValueError, match="outside"):
                call()
    for bad in ((u, p, torch.zeros(11, 8)), (u, p, torch.zeros(4, 8)), (u, torch.zeros(1, 8), n), (torch.zeros(1, 8), p, n),
                (u, torch.zeros(4, 7), n), (u, p, torch.zeros(12, 9)), (torch.zeros(4, 0), torch.zeros(4, 0), torch.zeros(12, 0)),
                (torch.zeros(0, 8), torch.zeros(0, 8), torch.zeros(0, 8)), (u[0], p, n)):
        for call in both(*bad, 3):
            with pytest.raises(ValueError):
                call()
    for call in both(u, p, n, 3, "max"):
        with pytest.raises(ValueError, match="reduction"):
            call()
    for bad in ((u.double(), p, n), (u, p.half(), n), (u, p, n.to(torch.bfloat16))):
        for call in both(*bad, 3):
            with pytest.raises(TypeError, match="float32"):
                call()
    wide = torch.zeros(12, 16)
    for bad in ((wide[:4, :8], p, n), (u, wide[:4, :8], n), (u, p, wide[:, :8]), (u, p, torch.zeros(8, 12).t())):
        for call in both(*bad, 3):
            with pytest.raises(ValueError, match="contiguous"):
                call()
    for call in both(u, p, n, 3):                              # nothing else wrong: no CPU path, in `BPR`'s words
        with pytest.raises(RuntimeError, match="ROCm device only"):
            call()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        BPR(0.1, 4)(u, p, torch.zeros(4, 8))
    for req in (False, True):
        with pytest.raises(RuntimeError, match="ROCm device only"):
            BPRMulti(0.1, 4, 3)(u.clone().requires_grad_(req), p, n)
    for kw in (dict(m=0), dict(m=65), dict(m=3, reduction="max")):
        with pytest.raises(ValueError):
            BPRMulti(0.1, 4, **kw)


def test_package_names():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    from seoul_tourism_recommendation_ngcf_amd import autograd, engine, sampling
    assert "BPRMulti" in pkg.__all__ and "BPR" in pkg.__all__ and issubclass(pkg.BPRMulti, torch.nn.Module)
    assert str(inspect.signature(pkg.BPRMulti.__init__)) == "(self, weight_decay, batch_size, m, reduction='mean')"
    assert str(inspect.signature(pkg.BPRMulti.forward)) == str(inspect.signature(pkg.BPR.forward))
    assert str(inspect.signature(pkg.BPR.__init__)) == "(self, weight_decay, batch_size)"
    crit = pkg.BPRMulti(0.025, 512, 8, reduction="softmax")
    assert (crit.weight_decay, crit.batch_size, crit.m, crit.reduction) == (0.025, 512, 8, "softmax") and not list(crit.parameters())
    assert issubclass(autograd.BPRMultiLoss, torch.autograd.Function)
    # the flat `engine` namespace is pinned (tests/test_engine_surface.py): the new wrappers live in a submodule of their own
    assert not hasattr(engine, "bpr_multi_loss") and not hasattr(engine, "bpr_multi_backward")
    assert inspect.ismodule(engine.losses) and engine.losses.__name__.endswith("engine.losses")
    assert list(inspect.signature(engine.losses.bpr_multi_loss).parameters) == ["u", "p", "n", "m", "weight_decay", "batch_size", "ws",
                                                                                "reduction"]
    assert inspect.signature(engine.losses.bpr_multi_loss).parameters["reduction"].default == "mean"
    assert list(inspect.signature(sampling.train_negatives).parameters) == ["users", "items", "seen", "m", "seed", "epoch", "n_user", "n_item"]
    lp = inspect.signature(sampling.NegativesLoader.__init__).parameters
    assert list(lp)[:10] == ["self", "users", "items", "columns", "batch_size", "m", "seed", "shuffle", "drop_last", "generator"]
    assert all(lp[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(lp)[4:])
    for name in ("train_negatives", "NegativesLoader"):
        assert getattr(sampling, name).__doc__


def test_sampling_refusals_on_the_host():
    """(The draws themselves need the device: `train_negatives(m=1)` against `train_triplets` is in tests/test_bpr_multi_gpu.py.)"""
    from seoul_tourism_recommendation_ngcf_amd import sampling
    users, items = torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])
    with pytest.raises(ValueError, match="expected"):
        sampling.train_negatives(users, items[:2], m=2, seed=1, n_user=3, n_item=3)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        sampling.train_negatives(users, items, m=2, seed=1, n_user=3, n_item=3)
    for kw in (dict(m=0), dict(m=65), dict(batch_size=0)):
        with pytest.raises(ValueError):
            sampling.NegativesLoader(users, items, **dict(dict(batch_size=2, m=2, seed=1), **kw))
    with pytest.raises(ValueError, match="every column"):
        sampling.NegativesLoader(users, items, (users[:2],), batch_size=2, m=2, seed=1)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        sampling.NegativesLoader(users, items, batch_size=2, m=2, seed=1)
