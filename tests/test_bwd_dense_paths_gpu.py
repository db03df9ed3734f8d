"""Every kernel path of ngcf_layer_bwd_weight_f32 and ngcf_layer_bwd_input_f32 (csrc/bwd_dense.hip) against the host oracle of
tests/bwd_dense_oracle.py - the layer's definition, not another kernel - through the C ABI, so that leading dimensions, alignment,
guards and workspace size are the test's own.

Exact form: integer operands in -3..3 whose every partial sum stays below 2^24, so each kernel - bwd_weight_kernel<ALIGNED> with
1, 2, 3, 512, 513 and 514 row blocks, bwd_weight_narrow_kernel around its 65 536-row threshold, bwd_weight_reduce_kernel with and
without either bias output, layer_bwd_input_kernel<4,true> / <4,false> / <5,false> with reductions d_out that are no multiple of 4
and below 4, layer_bwd_input_resident_kernel and layer_bwd_input_narrow_kernel from 131 072 rows - must produce the oracle bit for
bit (`torch.equal`).  Each case names the path it expects and asserts it through ngcf_layer_bwd_weight_path /
ngcf_layer_bwd_input_path after setting the options from DEFAULTS, so a case fails when the dispatch stops sending it there.
Inputs are views of NaN-filled buffers with guard rows (LE and E with different leading dimensions, dM of the input gradient with
NaN in its padding columns up to a multiple of 4 or 32); outputs are column slices of sentinel-filled buffers with guard rows; the
workspace is exactly ngcf_*_workspace_bytes inside a larger sentinel-filled allocation.  Nothing outside an output slice, no input
and neither end of the workspace allocation may change; a second call must reproduce the first.

fp64 form: one real-valued case of mixed magnitudes per path name, every element held to k 2^-24 S (k counted in
tests/bwd_dense_oracle.py); the observed maxima are printed.

Observed on an MI355X, the largest error of an element in units of 2^-24 S against its bound k (the 68 tests of this file took 26 s,
the slowest case, 131 072 x 260, 2.3 s):
    mfma_aligned    16 423 x 65 -> 100:  gW 1.90 (k 111),  gb2 0.12 (k 41)
    mfma_unaligned   1 000 x 33 -> 65:   gW 6.09 (k 72),   gb2 0.43 (k 26)
    narrow          70 001 x 3 -> 100:   gW 0.67 (k 95),   gb2 0.08 (k 95)
    staged_small       333 x 100 <- 65:  dLE 7.83,  dE 7.94  (k 66)
    staged_wide        261 x 130 <- 100: dLE 10.93, dE 10.07 (k 101)
    staged_tall     16 517 x 128 <- 33:  dLE 10.48, dE 9.70  (k 34)
    resident       131 105 x 130 <- 65:  dLE 14.51, dE 14.18 (k 66);  its narrow columns: dLE 3.66, dE 4.03 (k 9)
"""
import ctypes

import numpy as np
import pytest
import torch

import bwd_dense_oracle as bo
from test_row_kernels_gpu import Guard

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = 7.0                  # around the outputs
G = bo.GUARD_ROWS
# the library's defaults (csrc/common.h), set before a case's own options: the cases do not depend on NGCF_* in the environment
DEFAULTS = dict(bwd_input_resident=1)
WS_HEAD, WS_TAIL, WS_BYTE = 192, 4096, 0x5A     # the workspace starts 192 bytes into its allocation (not 256-byte aligned)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    return _lib.load()


def _L():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    return _lib


class Input(Guard):
    """An operand the kernel only reads: NaN in its padding columns and guard rows (compared as bits)."""

    def __init__(self, data, ld, dev, col0=0, guard=G):
        data = torch.as_tensor(np.asarray(data, dtype=np.float32))
        super().__init__(data.shape[0], data.shape[1], ld, dev, data, col0=col0, guard=guard, sentinel=NAN)

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))


class Workspace:
    """Exactly `need` bytes, WS_HEAD bytes into an allocation of WS_HEAD + need + WS_TAIL bytes filled with WS_BYTE."""

    def __init__(self, need, dev):
        self.need = int(need)
        self.buf = torch.full((WS_HEAD + self.need + WS_TAIL,), WS_BYTE, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + WS_HEAD

    def ends_intact(self):
        return bool((self.buf[:WS_HEAD] == WS_BYTE).all()) and bool((self.buf[WS_HEAD + self.need:] == WS_BYTE).all())


def _mismatch(what, path, got, want):
    """None, or the message of a failed exact comparison: the count and the first (row, column) that differs."""
    got, want = torch.as_tensor(got), torch.as_tensor(want).to(got.device)
    assert got.dim() == 2 and got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return None
    bad = torch.nonzero(got != want)                          # NaN compares unequal too
    r, c = (int(v) for v in bad[0])
    return (f"{path}: {len(bad)} elements of {what} differ from the exact oracle, first at row {r} column {c}: "
            f"{float(got[r, c])!r} for {float(want[r, c])!r}")


# ---- weight gradient -----------------------------------------------------------------------------------------------------------------
class _WeightCall:
    """The device operands of one weight-gradient case, laid out by bwd_dense_oracle.weight_layout, and its call."""

    def __init__(self, c, ins, dev, lib):
        self.c, self.lib = c, lib
        lay = bo.weight_layout(c)
        dM, LE, E = ins
        self.dM, self.LE, self.E = (Input(a, lay[k][0], dev, col0=lay[k][1]) for a, k in ((dM, "dM"), (LE, "LE"), (E, "E")))
        for src, k in ((self.dM, "dM"), (self.LE, "LE"), (self.E, "E")):
            assert src.ptr % 16 == bo.address(*lay[k]) % 16           # the alignment the host-only path test assumed
        self.gW1 = Guard(c.d_out, c.d_in, c.d_in + 5, dev, col0=2, guard=4)
        self.gW2 = Guard(c.d_out, c.d_in, c.d_in + 3, dev, col0=1, guard=4)
        self.gb1 = Guard(1, c.d_out, c.d_out + 7, dev, col0=3, guard=2)
        self.gb2 = Guard(1, c.d_out, c.d_out + 4, dev, col0=1, guard=2)
        self.ws = Workspace(lib.ngcf_bwd_weight_workspace_bytes(), dev)

    def path(self):
        n_wg = ctypes.c_int(-1)
        got = self.lib.ngcf_layer_bwd_weight_path(self.c.n, self.c.d_in, self.c.d_out, self.dM.ptr, self.dM.ld, self.LE.ptr, self.LE.ld,
                                                  self.E.ptr, self.E.ld, ctypes.byref(n_wg))
        return (None if got is None else got.decode()), n_wg.value

    def run(self, d_in=None, ws_bytes=None):
        c = self.c
        rc = self.lib.ngcf_layer_bwd_weight_f32(self.dM.ptr, self.dM.ld, self.LE.ptr, self.LE.ld, self.E.ptr, self.E.ld, c.n,
                                                c.d_in if d_in is None else d_in, c.d_out, self.gW1.ptr, self.gW1.ld, self.gW2.ptr,
                                                self.gW2.ld, self.gb1.ptr if c.bias in ("both", "gb1") else None,
                                                self.gb2.ptr if c.bias in ("both", "gb2") else None, self.ws.ptr,
                                                self.ws.need if ws_bytes is None else ws_bytes, None)
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return [g.view.clone() for g in (self.gW1, self.gW2, self.gb1, self.gb2)]

    def assert_nothing_else_changed(self):
        c = self.c
        assert self.dM.untouched() and self.LE.untouched() and self.E.untouched(), f"{c.path}: an input changed"
        assert self.gW1.guard_intact() and self.gW2.guard_intact(), f"{c.path}: a store outside gW1 / gW2"
        assert (self.gb1.guard_intact() if c.bias in ("both", "gb1") else self.gb1.untouched()), f"{c.path}: a store outside gb1"
        assert (self.gb2.guard_intact() if c.bias in ("both", "gb2") else self.gb2.untouched()), f"{c.path}: a store outside gb2"
        assert self.ws.ends_intact(), f"{c.path}: a store outside the workspace"


def _weight_call(c, ins, dev, lib, lib_options):
    lib_options(**DEFAULTS)
    call = _WeightCall(c, ins, dev, lib)
    name, n_wg = call.path()
    assert name == c.path and n_wg == bo.weight_workgroups(c.n, c.d_in), f"the dispatch sends this case to {name} on {n_wg} workgroups, not to {c.path}"
    _L().check(call.run())
    first = call.outputs()
    call.assert_nothing_else_changed()
    _L().check(call.run())
    for a, b, what in zip(call.outputs(), first, ("gW1", "gW2", "gb1", "gb2")):
        assert torch.equal(a, b), f"{c.path}: the second call's {what} differs from the first"
    return call, first


@pytest.mark.parametrize("c", bo.WEIGHT_CASES, ids=bo.wcase_id)
def test_weight_gradient_is_exact_on_every_path(c, dev, lib, lib_options):
    ins = bo.weight_inputs(c.n, c.d_in, c.d_out, c.seed)
    want = bo.exact_weight(*ins)
    call, (gW1, gW2, gb1, gb2) = _weight_call(c, ins, dev, lib, lib_options)
    errs = [_mismatch("gW1", c.path, gW1, want[0]), _mismatch("gW2", c.path, gW2, want[1])]
    if c.bias in ("both", "gb1"):
        errs.append(_mismatch("gb1", c.path, gb1, want[2][None]))
    if c.bias in ("both", "gb2"):
        errs.append(_mismatch("gb2", c.path, gb2, want[3][None]))
    assert not any(errs), "; ".join(e for e in errs if e)


@pytest.mark.parametrize("n,d_in,d_out,seed", bo.WRAPPER_CASES)
def test_weight_gradient_wrapper_cuts_a_wide_layer_into_exact_blocks(n, d_in, d_out, seed, dev, lib_options):
    """engine.backward.bwd_weight at 515 -> 200: 2 x 5 calls of at most 128 x 128 (the last input block 3 columns wide), the bias from the
    first column block only."""
    from seoul_tourism_recommendation_ngcf_amd import engine
    lib_options(**DEFAULTS)
    ins = bo.weight_inputs(n, d_in, d_out, seed)
    want = bo.exact_weight(*ins)
    dM, LE, E = (torch.as_tensor(a.astype(np.float32)).to(dev) for a in ins)
    got = engine.backward.bwd_weight(dM, LE, E, engine.Workspace())
    torch.cuda.synchronize()
    errs = [_mismatch(what, "wrapper", g.reshape(w.shape if w.ndim > 1 else (1, -1)), w if w.ndim > 1 else w[None])
            for what, g, w in zip(("gW1", "gb1", "gW2", "gb2"), got, (want[0], want[2], want[1], want[3]))]
    assert not any(errs), "; ".join(e for e in errs if e)


@pytest.mark.parametrize("c", bo.WEIGHT_FP64, ids=bo.wcase_id)
def test_weight_gradient_is_within_the_fp64_bound_per_element(c, dev, lib, lib_options):
    dM, LE, E = bo.mixed_weight_inputs(c.n, c.d_in, c.d_out, c.seed)
    gW, S_W, gb, S_b = bo.fp64_weight(dM, LE, E)
    call, (gW1, gW2, gb1, gb2) = _weight_call(c, (dM.numpy(), LE.numpy(), E.numpy()), dev, lib, lib_options)
    got = torch.cat((gW1, gW2), 1).cpu().double()
    kw, kb = bo.weight_k(c.path, c.n, c.d_in), bo.bias_k(c.path, c.n, c.d_in)
    assert bool(torch.isfinite(got).all()) and bool((S_W > 0).all())
    e_w = float(((got - gW).abs() / S_W).max()) / bo.U32
    e_b = float(((gb2.cpu().double()[0] - gb).abs() / S_b).max()) / bo.U32
    print(f"\n{c.path}: {c.n} x {c.d_in} -> {c.d_out}: gW error {e_w:.2f} (k {kw}), gb2 error {e_b:.2f} (k {kb}), in units of 2^-24 S")
    assert bool(((got - gW).abs() <= bo.bound(kw, S_W)).all()), (c.path, e_w, kw)
    assert bool(((gb2.cpu().double()[0] - gb).abs() <= bo.bound(kb, S_b)).all()), (c.path, e_b, kb)
    assert torch.equal(gb1, 2.0 * gb2)


def test_weight_gradient_error_returns_leave_the_outputs_untouched(dev, lib, lib_options):
    lib_options(**DEFAULTS)
    c = bo.WCase("mfma_aligned", 33, 128, 64, "padded", "both", 7)
    call = _WeightCall(c, bo.weight_inputs(c.n, c.d_in + 4, c.d_out, c.seed), dev, lib)        # LE, E hold 132 columns
    for kw, code, text in ((dict(d_in=129), _L().ERR_ARG, "not in 1..128"), (dict(ws_bytes=call.ws.need - 1), _L().ERR_WORKSPACE, "workspace")):
        assert call.run(**kw) == code and text in _L().last_error() and "layer_bwd_weight" in _L().last_error()
        for g in (call.gW1, call.gW2, call.gb1, call.gb2, call.dM, call.LE, call.E):
            assert g.untouched()
        assert bool((call.ws.buf == WS_BYTE).all())


# ---- input gradient ------------------------------------------------------------------------------------------------------------------
class _InputCall:
    def __init__(self, c, ins, dev, lib, ldm=None):
        self.c, self.lib = c, lib
        dM, W1, W2, LE, E = ins
        self.dM = Input(dM, bo.input_ldm(c) if ldm is None else ldm, dev)
        self.W1, self.W2 = Input(W1, c.d_in, dev, guard=8), Input(W2, c.d_in, dev, guard=8)        # contiguous, NaN rows around
        self.LE, self.E = Input(LE, c.d_in + 3, dev, col0=1), Input(E, c.d_in + 6, dev, col0=2)
        self.dLE = Guard(c.n, c.d_in, c.d_in + 6, dev, col0=2, guard=G)
        self.dE = Guard(c.n, c.d_in, c.d_in + 9, dev, col0=5, guard=G)
        self.ws = Workspace(lib.ngcf_layer_bwd_input_workspace_bytes(c.d_out), dev)

    def run(self, n=None):
        c = self.c
        rc = self.lib.ngcf_layer_bwd_input_f32(self.dM.ptr, self.dM.ld, c.n if n is None else n, c.d_out, self.W1.ptr, self.W2.ptr, c.d_in,
                                               self.LE.ptr, self.LE.ld, self.E.ptr, self.E.ld, self.dLE.ptr, self.dLE.ld, self.dE.ptr,
                                               self.dE.ld, self.ws.ptr, self.ws.need, None)
        torch.cuda.synchronize()
        return rc

    def inputs(self):
        return (self.dM, self.W1, self.W2, self.LE, self.E)

    def assert_nothing_else_changed(self, path):
        assert all(s.untouched() for s in self.inputs()), f"{path}: an input changed"
        assert self.dLE.guard_intact() and self.dE.guard_intact(), f"{path}: a store outside dLE / dE"
        assert self.ws.ends_intact(), f"{path}: a store outside the workspace"


def _input_call(c, ins, dev, lib, lib_options):
    lib_options(**{**DEFAULTS, **c.opts})
    path = "+".join(c.panels)
    got = bo.query_input_panels(lib, c.n, c.d_in, c.d_out)
    assert got == bo.expected_panels(c), f"the dispatch sends this case to {got}, not to {path}"
    call = _InputCall(c, ins, dev, lib)
    if bo.input_ldm(c) > c.d_out:
        assert bool(torch.isnan(call.dM.buf[G:G + c.n, c.d_out:]).all())
    _L().check(call.run())
    first = (call.dLE.view.clone(), call.dE.view.clone())
    call.assert_nothing_else_changed(path)
    _L().check(call.run())
    assert torch.equal(call.dLE.view, first[0]) and torch.equal(call.dE.view, first[1]), f"{path}: the second call differs from the first"
    return first


@pytest.mark.parametrize("c", bo.INPUT_CASES, ids=bo.icase_id)
def test_input_gradient_is_exact_on_every_path(c, dev, lib, lib_options):
    ins = bo.input_inputs(c.n, c.d_in, c.d_out, c.seed)
    want = bo.exact_input(*ins)
    dLE, dE = _input_call(c, ins, dev, lib, lib_options)
    path = "+".join(c.panels)
    errs = [_mismatch("dLE", path, dLE, want[0]), _mismatch("dE", path, dE, want[1])]
    assert not any(errs), "; ".join(e for e in errs if e)


@pytest.mark.parametrize("c", bo.INPUT_FP64, ids=bo.icase_id)
def test_input_gradient_is_within_the_fp64_bound_per_element(c, dev, lib, lib_options):
    ins = bo.mixed_input_inputs(c.n, c.d_in, c.d_out, c.seed)
    rL, S_L, rE, S_E = bo.fp64_input(*ins)
    dLE, dE = _input_call(c, tuple(t.numpy() for t in ins), dev, lib, lib_options)
    panel = bo.panel_of_column(c)
    k = torch.tensor([bo.input_k(p, c.d_out) for p in panel], dtype=torch.float64)
    live = torch.ones(c.n, dtype=torch.bool)
    live[::97] = False                                                  # zero rows of dM: S = 0, the result must be an exact zero
    for what, got, ref, S in (("dLE", dLE, rL, S_L), ("dE", dE, rE, S_E)):
        got = got.cpu().double()
        assert bool(torch.isfinite(got).all()) and not got[~live].any() and bool((S[live] > 0).all())
        err = (got - ref).abs()[live] / S[live] / bo.U32
        for name in sorted(set(panel)):
            cols = torch.tensor([p == name for p in panel])
            print(f"\n{name}: {c.n} x {c.d_in} <- {c.d_out}: {what} error {float(err[:, cols].max()):.2f} (k {bo.input_k(name, c.d_out)}), in units of 2^-24 S")
        assert bool(((got - ref).abs() <= bo.bound(k, S)).all()), (what, "+".join(c.panels), float((err / k).max()))


def test_input_gradient_error_returns_leave_the_outputs_untouched(dev, lib, lib_options):
    lib_options(**DEFAULTS)
    c = bo.ICase(("staged_small",), 33, 65, 66, "pad4", {}, 9)
    ins = bo.input_inputs(c.n, c.d_in, c.d_out, c.seed)
    for ldm, n, code in ((70, None, _L().ERR_ARG), (68, 0, _L().OK)):                           # ldM % 4 != 0; nothing to do
        call = _InputCall(c, ins, dev, lib, ldm=ldm)
        assert call.run(n=n) == code
        if code:
            assert "layer_bwd_input" in _L().last_error() and "multiple of 4" in _L().last_error()
        assert all(g.untouched() for g in call.inputs() + (call.dLE, call.dE)) and bool((call.ws.buf == WS_BYTE).all())
