"""CPU: the surface of the sampled softmax loss with logQ correction - the C symbols, the header's text, the refusals of every layer
(all before any launch: they hold on a machine without a device), and the package's new names."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ("ngcf_sampled_softmax_workspace_bytes", "ngcf_sampled_softmax_f32", "ngcf_sampled_softmax_backward_f32")


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
    from seoul_tourism_recommendation_ngcf_amd.engine import losses
    assert re.search(r"^#define\s+NGCF_SAMPLED_SOFTMAX_M_MAX\s+%d\s*$" % losses.M_MAX, text, flags=re.M) and losses.M_MAX == 64
    assert text.index("BPR, m negatives per positive") < text.index("Sampled softmax with logQ correction")
    assert any(os.path.basename(s) == "sampled_softmax.hip" for s in _build.SOURCES)
    assert any(os.path.basename(s) == "loss_rows_device.h" for s in _build.HEADERS)
    with open(_lib.lib_path(), "rb") as f:
        blob = f.read()
    assert b"sampled_softmax_rows_kernel" in blob and b"sampled_softmax_backward_kernel" in blob


def test_the_row_machinery_is_defined_once():
    """URow, RowBatch, the score pass, wave_max and lane_value, the softmax over the lanes, the backward's walk over the negatives,
    the operand check, the workspace and the finish launch live in csrc/loss_rows_device.h, which both loss files include; the
    forward's partials tail in csrc/common.h, next to the second stage."""
    from seoul_tourism_recommendation_ngcf_amd import _build
    text = {}
    for name in ("loss_rows_device.h", "bpr_multi.hip", "sampled_softmax.hip", "common.h"):
        with open(os.path.join(_build.CSRC, name)) as f:
            text[name] = f.read()
    for definition in ("struct URow {", "struct RowBatch {", "Scores score_row(", "float wave_max(float", "float lane_value(float",
                       "void gradient_walk(", "float lanes_lse(float", "float softmax_weight(float", "int check_rows(const char",
                       "int64_t partials_workspace_bytes(int64_t", "int partials_in(const char", "int finish_loss(const float",
                       "void loss_rows_finish_kernel(", "#define LOSS_ROWS_LAUNCH("):
        assert text["loss_rows_device.h"].count(definition) == 1, definition
        assert definition not in text["bpr_multi.hip"] and definition not in text["sampled_softmax.hip"], definition
    assert text["common.h"].count("void bpr_block_partials(") == 1
    for name in ("bpr_multi.hip", "sampled_softmax.hip"):
        assert '#include "loss_rows_device.h"' in text[name]
        assert "bpr_block_partials(wave, lane, nl, sq, part);" in text[name] and "gradient_walk<KU>(" in text[name]
        # what the shared definitions replaced: no partials array, walk, finish kernel, size formula, dispatch layer or log-sum-exp
        # of the file's own
        for gone in ("__shared__", "acc[", "_finish_kernel", "align_up(", "launch_forward", "launch_backward", "logf(", "wave_max("):
            assert gone not in text[name], (name, gone)


def test_workspace_is_the_two_float_partials_of_four_rows():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    assert lib.ngcf_sampled_softmax_workspace_bytes(-1) == -1
    for B in (0, 1, 4, 5, 1025, 1 << 20):
        assert lib.ngcf_sampled_softmax_workspace_bytes(B) >= (B + 3) // 4 * 8
        assert lib.ngcf_sampled_softmax_workspace_bytes(B) == lib.ngcf_bpr_multi_workspace_bytes(B)


# B, B, B*m, m, D, inv_tau, workspace bytes -> what the library says; the pointers are never followed
GOOD = dict(Bu=4, Bp=4, Bn=12, m=3, D=8, it=1.0, ws=1 << 12)
REFUSALS = [
    (dict(m=0, Bn=0), "m=0"), (dict(m=65, Bn=4 * 65), "m=65"), (dict(m=-1), "m=-1"),
    (dict(Bn=11), "4/4/11"), (dict(Bn=4), "4/4/4"), (dict(Bp=1), "4/1/12"), (dict(Bp=5), "4/5/12"), (dict(Bu=1), "1/4/12"),
    (dict(Bu=0, Bp=0, Bn=0), "0/0/0"), (dict(D=0), "D=0"), (dict(D=-3), "D=-3"),
    (dict(it=0.0), "inv_tau=0"), (dict(it=-2.0), "inv_tau=-2"), (dict(it=float("inf")), "inv_tau=inf"), (dict(it=float("nan")), "inv_tau="),
]


def _forward(lib, a, ptrs=None, pos=None, ws=None):
    fake = C.c_void_p(4096)
    u, p, n, logq, loss = ptrs or [fake] * 5
    return lib.ngcf_sampled_softmax_f32(u, a["Bu"], p, a["Bp"], n, a["Bn"], a["m"], a["D"], logq, pos, a["it"], 0.1, 4.0, loss,
                                        *(ws or (fake, a["ws"])), None)


def _backward(lib, a, ptrs=None, pos=None):
    fake = C.c_void_p(4096)
    u, p, n, logq, gout, du, dp, dn = ptrs or [fake] * 8
    return lib.ngcf_sampled_softmax_backward_f32(u, a["Bu"], p, a["Bp"], n, a["Bn"], a["m"], a["D"], logq, pos, a["it"], 0.1, 4.0, gout, du,
                                                 dp, dn, None)


@pytest.mark.parametrize("change,words", REFUSALS, ids=[w for _, w in REFUSALS])
def test_library_refuses_before_any_launch(change, words):
    """Without a device a launch would come back as NGCF_ERR_HIP: NGCF_ERR_ARG shows that the check came first."""
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    a = dict(GOOD, **change)
    for pos in (None, C.c_void_p(4096)):
        assert _forward(lib, a, pos=pos) == _lib.ERR_ARG and "sampled_softmax:" in _lib.last_error() and words in _lib.last_error()
        assert _backward(lib, a, pos=pos) == _lib.ERR_ARG
        assert "sampled_softmax_backward:" in _lib.last_error() and words in _lib.last_error()


def test_library_refuses_null_pointers_and_a_short_workspace():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    fake, a = C.c_void_p(4096), GOOD
    need = lib.ngcf_sampled_softmax_workspace_bytes(a["Bu"])
    for ws in ((fake, need - 1), (fake, 0), (None, need)):
        assert _forward(lib, a, ws=ws) == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    for hole in range(5):                                      # u, p, n, logq, loss (pos_logq may be null: no correction of the positive)
        assert _forward(lib, a, ptrs=[None if i == hole else fake for i in range(5)]) == _lib.ERR_ARG and "null" in _lib.last_error()
    for hole in range(8):
        assert _backward(lib, a, ptrs=[None if i == hole else fake for i in range(8)]) == _lib.ERR_ARG and "null" in _lib.last_error()


def test_wrappers_refuse_before_the_device_is_asked_for():
    """Every refusal below is raised on CPU tensors: sizes, types, limits come first; CPU tensors themselves are refused last."""
    from seoul_tourism_recommendation_ngcf_amd import SampledSoftmax, engine
    losses = engine.losses
    ws = engine.Workspace()
    u, p, n = torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(12, 8)
    logq, pos = torch.zeros(4, 3), torch.zeros(4)
    g = torch.ones(())

    def both(u, p, n, logq, m, inv_tau=1.0, pos_logq=None):
        yield lambda: losses.sampled_softmax_loss(u, p, n, logq, m, inv_tau, 0.1, 4, ws, pos_logq)
        yield lambda: losses.sampled_softmax_backward(u, p, n, logq, m, inv_tau, 0.1, 4, g, pos_logq)

    for m in (0, 65, -1, 2.5):
        for call in both(u, p, torch.zeros(max(int(4 * m), 0), 8), torch.zeros(max(int(4 * m), 0)), m):
            with pytest.raises(ValueError, match="outside"):
                call()
    for bad in ((u, p, torch.zeros(11, 8)), (u, p, torch.zeros(4, 8)), (u, torch.zeros(1, 8), n), (torch.zeros(1, 8), p, n),
                (u, torch.zeros(4, 7), n), (u, p, torch.zeros(12, 9)), (torch.zeros(4, 0), torch.zeros(4, 0), torch.zeros(12, 0)),
                (torch.zeros(0, 8), torch.zeros(0, 8), torch.zeros(0, 8)), (u[0], p, n)):
        for lq in (logq, torch.zeros(int(bad[0].shape[0]) * 3 if bad[0].dim() == 2 else 3)):
            for call in both(*bad, lq, 3):
                with pytest.raises(ValueError):
                    call()
    for lq in (torch.zeros(11), torch.zeros(3, 4), torch.zeros(4), torch.zeros(4, 3, 1), torch.zeros(())):
        for call in both(u, p, n, lq, 3):
            with pytest.raises(ValueError, match="logq must be"):
                call()
    for bad_pos in (torch.zeros(3), torch.zeros(4, 1), torch.zeros(12)):
        for call in both(u, p, n, logq, 3, pos_logq=bad_pos):
            with pytest.raises(ValueError, match="pos_logq must be"):
                call()
    for lq, ps in ((logq.half(), None), (logq.long(), None), (logq, pos.to(torch.bfloat16)), (logq, pos.int())):
        for call in both(u, p, n, lq, 3, pos_logq=ps):
            with pytest.raises(TypeError, match="float32 or float64"):
                call()
    for inv_tau in (0.0, -1.0, float("inf"), float("nan")):
        for call in both(u, p, n, logq, 3, inv_tau):
            with pytest.raises(ValueError, match="inv_tau"):
                call()
    for bad in ((u.double(), p, n), (u, p.half(), n), (u, p, n.to(torch.bfloat16))):
        for call in both(*bad, logq, 3):
            with pytest.raises(TypeError, match="float32"):
                call()
    wide = torch.zeros(12, 16)
    for bad in ((wide[:4, :8], p, n), (u, wide[:4, :8], n), (u, p, wide[:, :8]), (u, p, torch.zeros(8, 12).t())):
        for call in both(*bad, logq, 3):
            with pytest.raises(ValueError, match="contiguous"):
                call()
    # nothing else wrong: no CPU path, in `BPR`'s words - with either shape and either type of the corrections
    for lq, ps in ((logq, None), (logq.reshape(-1), pos), (logq.double(), pos.double())):
        for call in both(u, p, n, lq, 3, 2.0, ps):
            with pytest.raises(RuntimeError, match="ROCm device only"):
                call()
    for req in (False, True):
        with pytest.raises(RuntimeError, match="ROCm device only"):
            SampledSoftmax(0.1, 4, 3)(u.clone().requires_grad_(req), p, n, logq)
        with pytest.raises(ValueError, match="logq must be"):
            SampledSoftmax(0.1, 4, 3)(u.clone().requires_grad_(req), p, n, torch.zeros(11))
        with pytest.raises(TypeError, match="float32 or float64"):
            SampledSoftmax(0.1, 4, 3)(u.clone().requires_grad_(req), p, n, logq.long())
    for kw in (dict(m=0), dict(m=65), dict(m=3, temperature=0.0), dict(m=3, temperature=-1.0), dict(m=3, temperature=float("inf")),
               dict(m=3, temperature=float("nan"))):
        with pytest.raises(ValueError):
            SampledSoftmax(0.1, 4, **kw)


def test_package_names():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    from seoul_tourism_recommendation_ngcf_amd import autograd, engine, sampling
    assert "SampledSoftmax" in pkg.__all__ and issubclass(pkg.SampledSoftmax, torch.nn.Module)
    assert str(inspect.signature(pkg.SampledSoftmax.__init__)) == "(self, weight_decay, batch_size, m, temperature=1.0)"
    assert str(inspect.signature(pkg.SampledSoftmax.forward)) == "(self, u_idx, pos_idx, neg_idx, logq, pos_logq=None)"
    crit = pkg.SampledSoftmax(0.025, 512, 8, temperature=0.25)
    assert (crit.weight_decay, crit.batch_size, crit.m, crit.temperature) == (0.025, 512, 8, 0.25) and not list(crit.parameters())
    assert issubclass(autograd.SampledSoftmaxLoss, torch.autograd.Function)
    # the flat `engine` namespace is pinned (tests/test_engine_surface.py): the new wrappers live in engine.losses
    assert not hasattr(engine, "sampled_softmax_loss") and not hasattr(engine, "sampled_softmax_backward")
    assert list(inspect.signature(engine.losses.sampled_softmax_loss).parameters) == [
        "u", "p", "n", "logq", "m", "inv_tau", "weight_decay", "batch_size", "ws", "pos_logq"]
    assert list(inspect.signature(engine.losses.sampled_softmax_backward).parameters) == [
        "u", "p", "n", "logq", "m", "inv_tau", "weight_decay", "batch_size", "grad_out", "pos_logq"]
    for fn in (engine.losses.sampled_softmax_loss, engine.losses.sampled_softmax_backward):
        assert inspect.signature(fn).parameters["pos_logq"].default is None and fn.__doc__
    lp = inspect.signature(sampling.LogQNegativesLoader.__init__).parameters
    assert list(lp) == ["self", "users", "items", "weights", "columns", "batch_size", "m", "seed", "shuffle", "drop_last", "generator", "seen"]
    assert str(inspect.signature(sampling.LogQNegativesLoader.__init__)) == str(inspect.signature(sampling.WeightedNegativesLoader.__init__))
    assert all(lp[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(lp)[5:])
    assert (lp["columns"].default, lp["shuffle"].default, lp["drop_last"].default, lp["generator"].default, lp["seen"].default) == (
        (), True, True, None, None)
    assert sampling.LogQNegativesLoader.__doc__ and pkg.SampledSoftmax.__doc__
    assert "not part of this package yet" not in sampling.weighted_negatives.__doc__


def test_loader_refusals_on_the_host():
    from seoul_tourism_recommendation_ngcf_amd import sampling
    rows, ones = torch.tensor([0, 1, 2]), torch.ones(3, dtype=torch.int64)
    for bad in (dict(m=0), dict(m=65), dict(batch_size=0)):
        with pytest.raises(ValueError, match="LogQNegativesLoader"):
            sampling.LogQNegativesLoader(rows, rows, ones, **{**dict(batch_size=2, m=4, seed=1), **bad})
    with pytest.raises(TypeError, match="LogQNegativesLoader: weights must be an int64"):
        sampling.LogQNegativesLoader(rows, rows, ones.float(), batch_size=2, m=4, seed=1)
    with pytest.raises(ValueError, match="every column"):
        sampling.LogQNegativesLoader(rows, rows[:-1], ones, batch_size=2, m=4, seed=1)
    with pytest.raises(ValueError, match="every column"):
        sampling.LogQNegativesLoader(rows, rows, ones, (rows[:2],), batch_size=2, m=4, seed=1)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        sampling.LogQNegativesLoader(rows, rows, ones, batch_size=2, m=4, seed=1)
    with pytest.raises(TypeError, match="^WeightedNegativesLoader: weights must be an int64"):      # the existing loader keeps its own name
        sampling.WeightedNegativesLoader(rows, rows, ones.float(), batch_size=2, m=4, seed=1)
