"""CPU: the float64 oracle of the full-catalogue softmax loss (tests/softmax_full_oracle.py) against torch's own float64
cross-entropy and its autograd, and the launch plan (`ngcf_softmax_full_plan`, host only) at the shapes tests/test_softmax_full_gpu.py
uses for the multi-piece and multi-slab paths."""
import numpy as np
import pytest
import torch

import softmax_full_oracle as orc

CASES = [(1, 1, 1), (5, 7, 3), (33, 129, 65), (64, 100, 260)]


@pytest.mark.parametrize("B,n,D", CASES)
@pytest.mark.parametrize("tau,wd", [(1.0, 0.0), (0.05, 0.025), (2.0, 0.5)])
def test_oracle_is_torch_float64_cross_entropy_and_its_autograd(B, n, D, tau, wd):
    rng = np.random.default_rng(B * 1000 + n + D)
    u = rng.standard_normal((B, D)).astype(np.float32)
    it = rng.standard_normal((n, D)).astype(np.float32)
    pos = rng.integers(0, n, B)
    pos[: B // 2] = pos[0]                                                   # duplicate positives
    bs, gout = B + 2, 3.0
    got = orc.softmax_full(u, it, pos, 1.0 / tau, wd, bs, gout)
    tu = torch.from_numpy(u).double().requires_grad_(True)
    ti = torch.from_numpy(it).double().requires_grad_(True)
    tp = torch.from_numpy(pos)
    s = tu @ ti.T / tau
    loss = (torch.nn.functional.cross_entropy(s, tp, reduction="sum") + wd * (tu.pow(2).sum() + ti[tp].pow(2).sum())) / bs
    (gout * loss).backward()
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)  # noqa: E731
    assert rel(got["loss"], float(loss.detach())) <= 1e-12
    assert rel(got["lse"], torch.logsumexp(s, 1).detach().numpy()) <= 1e-12
    assert rel(got["du"], tu.grad.numpy()) <= 1e-12 and rel(got["ditems"], ti.grad.numpy()) <= 1e-12
    assert rel(got["spos"], s.detach().numpy()[np.arange(B), pos]) <= 1e-12


def test_oracle_gives_a_row_with_an_id_outside_the_catalogue_no_positive_term():
    rng = np.random.default_rng(3)
    u, it = rng.standard_normal((4, 5)).astype(np.float32), rng.standard_normal((6, 5)).astype(np.float32)
    good = orc.softmax_full(u, it, [1, 2, 3, 4], 1.0, 0.0, 4)
    bad = orc.softmax_full(u, it, [1, 6, 3, -1], 1.0, 0.0, 4)
    assert np.array_equal(good["lse"], bad["lse"]) and bad["spos"][1] == 0 and bad["spos"][3] == 0
    assert np.array_equal(good["du"][[0, 2]], bad["du"][[0, 2]])


def _plan(B, n, D):
    from seoul_tourism_recommendation_ngcf_amd.engine import losses
    return losses.softmax_full_plan(B, n, D)


def test_plan_cuts_the_shapes_the_gpu_tests_rely_on():
    """(pieces, column slabs) of the forward, dU and dI: the shapes the issue names do take the cut paths."""
    p = _plan(1, 4097, 65)
    assert p["forward"][0] >= 2 and p["du"][0] >= 2 and p["ditems"][0] == 1          # the item side is cut, ragged last piece
    p = _plan(4097, 33, 65)
    assert p["ditems"][0] >= 2 and p["forward"][0] == 1 and p["du"][0] == 1          # the user side is cut for dI
    p = _plan(33, 33, 513)                                                           # the first width past one slab
    assert p["du"][1] == 2 and p["ditems"][1] == 2 and p["forward"][1] == 1
    assert _plan(33, 33, 512)["du"][1] == 1
    p = _plan(8192, 100000, 512)                                                     # the workload's rows: no item piece is empty
    assert p["forward"][0] >= 2 and p["du"][0] >= 2 and p["ditems"] == (1, 1)
    assert _plan(512, 100, 260) == {"forward": (1, 1), "du": (1, 1), "ditems": (1, 1)}


def test_plan_and_workspace_refuse_bad_shapes():
    import ctypes as C
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 6)()
    for B, n, D in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (1 << 31, 5, 5)):
        assert lib.ngcf_softmax_full_plan(B, n, D, out) == _lib.ERR_ARG and "softmax_full_plan" in _lib.last_error()
        assert lib.ngcf_softmax_full_workspace_bytes(B, n, D) == -1
    assert lib.ngcf_softmax_full_plan(5, 5, 5, None) == _lib.ERR_ARG
    # the bound of the header: the (max, sum) partials and, where a gradient is cut, pieces x rows x D floats
    for B, n, D in ((1, 4097, 65), (4097, 33, 65), (512, 100, 260), (33, 33, 513)):
        p = _plan(B, n, D)
        pieces = max(p["forward"][0], p["du"][0], p["ditems"][0])
        need = lib.ngcf_softmax_full_workspace_bytes(B, n, D)
        assert 0 < need <= pieces * (B + n) * D * 4 + 2 * pieces * B * 4 + (B + 3) // 4 * 16 + 8 * 256
