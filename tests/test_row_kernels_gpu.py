"""The row kernels every training step runs between the SpMM and dense kernels, called directly through the C ABI at the shapes
where they branch, against references the kernels had no part in (tests/row_oracle.py: float32 emulation of a documented order,
float64 autograd, exact torch copies and sums).  Every device operand lives inside a wider buffer filled with a sentinel; after
every call the rows around it and its padding columns must be unchanged."""
import functools

import numpy as np
import pytest
import torch

import ngcf_oracle as orc
import row_oracle as ro

pytestmark = pytest.mark.gpu

SENT, SENT_IN, GUARD = 7.0, -3.0, 32   # sentinels around outputs and around inputs (a copy of input padding onto output padding shows);
                                       # guard rows before and after an operand


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    return _lib.load()


def _check(rc):
    from seoul_tourism_recommendation_ngcf_amd import _lib
    _lib.check(rc)


class Guard:
    """rows x d floats at column col0 of a [guard + rows + guard, ld] buffer full of the sentinel (rows x d of `data` copied in)."""

    def __init__(self, rows, d, ld, dev, data=None, col0=0, guard=GUARD, sentinel=SENT):
        assert col0 + d <= ld
        self.buf = torch.full((rows + 2 * guard, ld), sentinel, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.inside = (slice(guard, guard + rows), slice(col0, col0 + d))
        self.view = self.buf[self.inside]
        if data is not None:
            self.view.copy_(torch.as_tensor(data))
        self.before = self.buf.clone()
        self.ptr, self.ld = self.buf.data_ptr() + 4 * (guard * ld + col0), ld

    def untouched(self):
        """An input: nothing was written."""
        return torch.equal(self.buf, self.before)

    def guard_intact(self):
        """An output: nothing outside the rows x d view was written."""
        probe = self.buf.clone()
        probe[self.inside] = self.before[self.inside]
        return torch.equal(probe, self.before)


def Source(*args, **kw):
    """An operand the kernel only reads."""
    return Guard(*args, sentinel=SENT_IN, **kw)


def _i64(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)


# ---- 1. ngcf_segment_sum_rows_f32 ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segment_reference(d):
    g, order, segptr = ro.segment_case(d, seed=d)
    return g, order, segptr, ro.segment_sum_chains(g, order, segptr), ro.segment_sum_f64(g, order, segptr)


@pytest.mark.parametrize("form", ["dense", "scatter"])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 320, 321, 358, 700])
def test_segment_sum_rows_has_the_documented_bits(d, form, dev, lib):
    """Segments of 0 .. 200 entries in one call (the jb loop's second to fourth pass, idle lanes, a tail after a full block),
    positions in a random order, ldg = d + 3, ldo = d + 5; 321 columns and more take the second column pass.  The result has the
    bits of the four-chain order the kernel documents, and lies within len * 2^-24 * sum|g| of the float64 sum.  Scatter form:
    the two longest segments go to rows -1 and n_out_rows (skipped), the last two segments are cut off by the device-side count;
    their rows, and the rows no segment names, keep the sentinel."""
    g, order, segptr, want, (total, bound) = _segment_reference(d)
    n_seg = len(segptr) - 1
    G = Source(len(g), d, d + 3, dev, g)
    order_d, segptr_d = _i64(order, dev), _i64(segptr, dev)
    if form == "dense":
        O = Guard(n_seg, d, d + 5, dev)
        _check(lib.ngcf_segment_sum_rows_f32(G.ptr, G.ld, d, order_d.data_ptr(), segptr_d.data_ptr(), n_seg, None, None, O.ptr, O.ld, 0, None))
        expect, written, seg_of_row = want, np.arange(n_seg), np.arange(n_seg)
    else:
        n_out, live = 40, n_seg - 2
        rng = np.random.default_rng(d)
        dst = rng.permutation(n_out)[:n_seg].astype(np.int64)
        lengths = np.diff(segptr)
        longest = np.argsort(lengths[:live])[-2:]
        assert lengths[longest].min() > 64 and lengths[live:].max() > 0
        dst[longest[0]], dst[longest[1]] = -1, n_out            # the guard rows right before and right after `out`
        O = Guard(n_out, d, d + 5, dev)
        dst_d, cnt_d = _i64(dst, dev), _i64([live], dev)
        _check(lib.ngcf_segment_sum_rows_f32(G.ptr, G.ld, d, order_d.data_ptr(), segptr_d.data_ptr(), n_seg, dst_d.data_ptr(),
                                             cnt_d.data_ptr(), O.ptr, O.ld, n_out, None))
        expect = np.full((n_out, d), SENT, dtype=np.float32)
        ok = [r for r in range(live) if 0 <= dst[r] < n_out]
        assert len(ok) == live - 2
        expect[dst[ok]] = want[ok]
        written, seg_of_row = dst[ok], np.asarray(ok)
    torch.cuda.synchronize()
    got = O.view.cpu().numpy()
    assert G.untouched() and O.guard_intact()
    assert np.array_equal(got, expect), f"{int((got != expect).sum())} elements differ from the four-chain order"
    err = np.abs(got[written].astype(np.float64) - total[seg_of_row])
    assert np.all(err <= bound[seg_of_row]), float((err - bound[seg_of_row]).max())


def test_segment_sum_rows_rejects_a_leading_dimension_below_d(dev, lib):
    from seoul_tourism_recommendation_ngcf_amd import _lib
    g, order, segptr, _, _ = _segment_reference(65)
    G, O = Source(len(g), 65, 68, dev, g), Guard(len(segptr) - 1, 65, 70, dev)
    order_d, segptr_d = _i64(order, dev), _i64(segptr, dev)
    for ldg, ldo in ((64, 70), (68, 64)):
        rc = lib.ngcf_segment_sum_rows_f32(G.ptr, ldg, 65, order_d.data_ptr(), segptr_d.data_ptr(), len(segptr) - 1, None, None, O.ptr, ldo, 0, None)
        assert rc != 0 and "segment_sum_rows" in _lib.last_error()
    torch.cuda.synchronize()
    assert O.untouched()


# ---- 2. BPR loss and gradient ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,D,broadcast", [(R, D, "") for R, D in ro.BPR_SHAPES] + [(1029, 65, b) for b in ro.BPR_BROADCAST])
def test_bpr_loss_and_gradients_match_fp64_autograd_in_every_score_regime(R, D, broadcast, dev):
    """pkg.BPR (ngcf_bpr_fused_f32 + ngcf_bpr_backward_f32) against float64 autograd of the oracle's loss, upstream gradient 3:
    scores from -120 to 120 in one batch (saturated logsigmoid and expf on both sides, and around 0), a zero u row (both signs 0),
    a zero p row, D below and off the wave width, R around the 1 024 rows one pass of the finishing kernel covers.  The inputs keep
    every dot product at 0 or at least 1e-3 of its magnitude sum, so the reference does not depend on rounding at the kink of |t|.
    Tolerances: the project's own for these kernels (loss 1e-5 relative; gradients atol 1e-7 + 2e-5 max|want|, rtol 1e-4)."""
    import seoul_tourism_recommendation_ngcf_amd as pkg
    wd, bs, upstream = 0.025, 64, 3.0
    cpu = ro.bpr_inputs(R, D, seed=R + D, broadcast=broadcast)
    assert ro.bpr_scores(*cpu)[2] >= 1e-3
    ref = [t.double().requires_grad_(True) for t in cpu]
    want_loss = orc.bpr_torch(*ref, wd, bs)
    (upstream * want_loss).backward()
    want_loss = float(want_loss.detach())
    runs = []
    for _ in range(2):
        guards = [Source(t.shape[0], D, D, dev, t) for t in cpu]
        leaves = [g.view.requires_grad_(True) for g in guards]
        assert all(t.is_contiguous() for t in leaves)
        loss = pkg.BPR(wd, bs)(*leaves)
        (upstream * loss).backward()
        torch.cuda.synchronize()
        assert all(g.untouched() for g in guards)
        runs.append((loss.detach().cpu(), [t.grad.cpu() for t in leaves]))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    got_loss, got = float(runs[0][0]), runs[0][1]
    print(f"loss {got_loss!r} want {want_loss!r} rel {abs(got_loss - want_loss) / abs(want_loss):.2e}")
    for k, a, r in zip("upn", got, ref):
        w = r.grad
        print(f"d{k}: max|err| {float((a.double() - w).abs().max()):.3e} max|want| {float(w.abs().max()):.3e}")
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss)
    for k, a, r in zip("upn", got, ref):
        w = r.grad.numpy()
        assert a.shape == r.shape
        np.testing.assert_allclose(a.numpy(), w, atol=1e-7 + 2e-5 * np.abs(w).max(), rtol=1e-4, err_msg=k)


# ---- 3. ngcf_layer_bwd_pre_f32 ---------------------------------------------------------------------------------------------------
LEAKY = 0.2


def _pre_call(lib, n_rows, d, dN, dC, C, mask, dM, drop_p=0.0, seed=0, row_ids=None):
    """Each operand a Guard or None."""
    a = lambda g: (None, 0) if g is None else (g.ptr, g.ld)  # noqa: E731
    _check(lib.ngcf_layer_bwd_pre_f32(*a(dN), *a(dC), *a(C), n_rows, d, LEAKY, drop_p, seed, *a(mask),
                                      None if row_ids is None else row_ids.data_ptr(), *a(dM), None))
    torch.cuda.synchronize()
    assert all(g.untouched() for g in (dN, dC, C, mask) if g is not None) and dM.guard_intact()
    return dM.view.cpu()


def _pre_vec(d, *guards):
    """The kernel's vector width: 2 when d and every given operand's leading dimension are even and its pointer 8-byte aligned."""
    return 2 if d % 2 == 0 and all(g.ld % 2 == 0 and g.ptr % 8 == 0 for g in guards if g is not None) else 1


def _pre_assert(got, want, zero_row, what):
    assert bool(torch.isfinite(got).all()), what
    rows = torch.ones(len(want), dtype=torch.bool)
    if zero_row is not None:                          # the clamped row: N = C / 1e-12, tolerance relative to the row's scale
        rows[zero_row] = False
        w = want[zero_row].numpy()
        np.testing.assert_allclose(got[zero_row].numpy(), w, atol=2e-5 * np.abs(w).max(), rtol=2e-3, err_msg=what + " (clamped row)")
    np.testing.assert_allclose(got[rows].numpy(), want[rows].numpy(), atol=2e-5, rtol=2e-3, err_msg=what)


@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "mask"])
@pytest.mark.parametrize("d", ro.PRE_D)
def test_layer_bwd_pre_matches_fp64_autograd(d, dropout, dev, lib):
    """dM against float64 autograd through leaky_relu -> * mask -> normalize, fed the float32 C and the same noise tensor: dN only, dC
    only and both; 1, 5 and 1 001 rows; one all-zero row of C (the clamped norm).  Every even d runs twice: all operands 8-byte
    aligned with even leading dimensions (VEC = 2), and as views from column 1 of wider buffers (VEC = 1).  Tolerance: the project's
    atol 2e-5, rtol 2e-3."""
    for n_rows in ro.PRE_ROWS:
        zero_row = None if n_rows == 1 else n_rows // 2
        M, dN, dC, mask = ro.pre_inputs(n_rows, d, seed=d + n_rows, drop_p=0.3 if dropout else 0.0, zero_row=zero_row)
        for grads in ("N", "C", "NC"):
            C64, want = ro.pre_reference(M, mask, dN if "N" in grads else None, dC if "C" in grads else None, LEAKY)
            assert not bool(((C64 != 0) & (C64.abs() < 1e-6)).any())
            for col0 in (0, 1) if d % 2 == 0 else (0,):
                pad = 2 if d % 2 == 0 else 3
                mk = lambda i, data=None: (Guard if data is None else Source)(n_rows, d, d + pad + 2 * i, dev, data, col0)  # noqa: E731
                ops = dict(dN=mk(0, dN) if "N" in grads else None, dC=mk(1, dC) if "C" in grads else None, C=mk(2, C64.float()),
                           mask=mk(3, mask) if dropout else None, dM=mk(4))
                assert _pre_vec(d, *ops.values()) == (2 if d % 2 == 0 and col0 == 0 else 1)
                got = _pre_call(lib, n_rows, d, **ops)
                _pre_assert(got, want.float(), zero_row, f"n_rows={n_rows} d={d} grads={grads} col0={col0}")


@pytest.mark.parametrize("which", ["dN", "dC", "C", "mask", "dM"])
def test_layer_bwd_pre_takes_the_scalar_path_when_one_operand_is_odd(which, dev, lib):
    """Even d, four operands aligned: the fifth alone has an odd leading dimension, then a pointer at 4 modulo 8."""
    n_rows, d = 5, 64
    M, dN, dC, mask = ro.pre_inputs(n_rows, d, seed=3, drop_p=0.3, zero_row=2)
    C64, want = ro.pre_reference(M, mask, dN, dC, LEAKY)
    data = dict(dN=dN, dC=dC, C=C64.float(), mask=mask, dM=None)
    for ld, col0 in ((d + 3, 0), (d + 2, 1)):
        ops = {k: (Guard if v is None else Source)(n_rows, d, ld if k == which else d + 2, dev, v, col0 if k == which else 0)
               for k, v in data.items()}
        assert _pre_vec(d, *ops.values()) == 1 and _pre_vec(d, *(g for k, g in ops.items() if k != which)) == 2
        _pre_assert(_pre_call(lib, n_rows, d, **ops), want.float(), 2, f"{which} ld={ld} col0={col0}")


@pytest.mark.parametrize("d", [64, 65])
def test_layer_bwd_pre_hash_dropout_is_a_function_of_seed_row_and_column(d, dev, lib):
    """drop_p > 0 without a mask tensor: two calls give the same bits; the compacted rows S with row_ids = S give the bits of rows S
    of the full call (the mask is indexed by the row of the matrix, not by the position in the call).  From the documented meaning
    alone: every element is 0 or the no-dropout value over 1 - p, and about p of them are 0 (65 000 draws: 0.3 +- 0.05 is 27 sigma)."""
    n_rows, p, seed = 1001, 0.3, 99
    M, dN, dC, _ = ro.pre_inputs(n_rows, d, seed=d, zero_row=None)
    C = torch.nn.functional.leaky_relu(M, LEAKY)
    mk = lambda rows, i, data=None: (Guard if data is None else Source)(rows, d, d + 2 + 2 * i, dev, data)  # noqa: E731
    full = [_pre_call(lib, n_rows, d, mk(n_rows, 0, dN), mk(n_rows, 1, dC), mk(n_rows, 2, C), None, mk(n_rows, 4), p, seed) for _ in range(2)]
    assert torch.equal(full[0], full[1])
    S = torch.randperm(n_rows, generator=torch.Generator().manual_seed(1))[:300]
    part = _pre_call(lib, 300, d, mk(300, 0, dN[S]), mk(300, 1, dC[S]), mk(300, 2, C[S]), None, mk(300, 4), p, seed, row_ids=S.to(dev))
    assert torch.equal(part, full[0][S])
    other = _pre_call(lib, 300, d, mk(300, 0, dN[S]), mk(300, 1, dC[S]), mk(300, 2, C[S]), None, mk(300, 4), p, seed)
    assert not torch.equal(other, part)                       # without row_ids the positions 0 .. 299 index the stream
    plain = _pre_call(lib, n_rows, d, mk(n_rows, 0, dN), mk(n_rows, 1, dC), mk(n_rows, 2, C), None, mk(n_rows, 4))
    dropped = full[0] == 0
    assert 0.25 < float(dropped.float().mean()) < 0.35
    torch.testing.assert_close(full[0][~dropped], (plain / (1 - p))[~dropped], rtol=1e-6, atol=0.0)


# ---- 4. exact movers ---------------------------------------------------------------------------------------------------------------
def _width(d, widths, *operands):
    """The widest vector (in floats) of `widths` such that d and every operand's leading dimension are multiples of it and every
    operand's pointer is aligned to it: the dispatch rule the movers state."""
    for v in widths:
        if d % v == 0 and all(g.ld % v == 0 and g.ptr % (4 * v) == 0 for g in operands):
            return v
    return 1


def _rand(rows, d, seed):
    return torch.randn((rows, d), generator=torch.Generator().manual_seed(seed))


# (n_rows, d, ld of out, col0 of out, ld of add, col0 of add, vector width)
ADD_ROWS = [(37, 8, 12, 0, 16, 0, 4), (37, 260, 264, 0, 260, 0, 4),
            (37, 7, 12, 0, 16, 0, 1), (37, 8, 13, 0, 16, 0, 1), (37, 8, 12, 0, 18, 0, 1), (37, 8, 12, 1, 16, 0, 1), (37, 8, 12, 0, 16, 2, 1),
            (1, 1, 1, 0, 1, 0, 1),
            (4099, 257, 257, 0, 260, 0, 1), (4099, 1028, 1032, 0, 1028, 0, 4)]     # past the grid cap: the stride loop iterates


@pytest.mark.parametrize("n_rows,d,ldo,co,lda,ca,vec", ADD_ROWS)
def test_add_rows_is_an_exact_float32_sum(n_rows, d, ldo, co, lda, ca, vec, dev, lib):
    if n_rows > 4096:
        assert n_rows * (d // vec) > 4096 * 256
    out0, add = _rand(n_rows, d, 1), _rand(n_rows, d, 2)
    O, A = Guard(n_rows, d, ldo, dev, out0, co), Source(n_rows, d, lda, dev, add, ca)
    assert _width(d, (4,), O, A) == vec
    _check(lib.ngcf_add_rows_f32(O.ptr, O.ld, A.ptr, A.ld, n_rows, d, None))
    torch.cuda.synchronize()
    assert A.untouched() and O.guard_intact()
    assert torch.equal(O.view.cpu(), out0 + add)
    _check(lib.ngcf_add_rows_f32(O.ptr, O.ld, A.ptr, A.ld, 0, d, None))           # no rows: nothing happens
    torch.cuda.synchronize()
    assert torch.equal(O.view.cpu(), out0 + add)


# (n_rows, d, ld of src, col0 of src, ld of dst, col0 of dst, vector width)
COPY_ROWS = [(37, 8, 12, 0, 16, 0, 4), (37, 260, 260, 0, 264, 0, 4),
             (37, 8, 12, 2, 16, 0, 2), (37, 8, 12, 0, 16, 2, 2), (37, 6, 8, 0, 8, 0, 2), (37, 8, 10, 0, 12, 0, 2), (37, 8, 12, 0, 14, 0, 2),
             (37, 8, 12, 1, 16, 0, 1), (37, 8, 12, 0, 16, 1, 1), (37, 7, 8, 0, 8, 0, 1), (37, 8, 9, 0, 12, 0, 1), (37, 8, 12, 0, 13, 0, 1),
             (1, 1, 1, 0, 1, 0, 1),
             (4099, 257, 260, 0, 257, 0, 1), (4099, 514, 514, 0, 516, 0, 2), (4099, 1028, 1028, 0, 1032, 0, 4)]


@pytest.mark.parametrize("n_rows,d,lds,cs,ldd,cd,vec", COPY_ROWS)
def test_copy_rows_copies_the_bits(n_rows, d, lds, cs, ldd, cd, vec, dev, lib):
    if n_rows > 4096:
        assert n_rows * (d // vec) > 4096 * 256
    src = _rand(n_rows, d, 3)
    S, D = Source(n_rows, d, lds, dev, src, cs), Guard(n_rows, d, ldd, dev, None, cd)
    assert _width(d, (4, 2), S, D) == vec
    _check(lib.ngcf_copy_rows_f32(S.ptr, S.ld, D.ptr, D.ld, 0, d, None))          # no rows: nothing happens
    torch.cuda.synchronize()
    assert D.untouched()
    _check(lib.ngcf_copy_rows_f32(S.ptr, S.ld, D.ptr, D.ld, n_rows, d, None))
    torch.cuda.synchronize()
    assert S.untouched() and D.guard_intact()
    assert torch.equal(D.view.cpu(), src)


# (n_rows, d, ld of src, ld of dst, ld of dst2, col0 of dst2, vector width): src and dst allow 4 floats; the last four: dst2 alone narrows
COPY_ROWS2 = [(37, 8, 12, 16, 20, 0, 4), (37, 8, 12, 16, 18, 0, 2), (37, 8, 12, 16, 20, 2, 2), (37, 8, 12, 16, 19, 0, 1), (37, 8, 12, 16, 20, 1, 1),
              (37, 65, 65, 68, 96, 0, 1),
              (4099, 257, 257, 260, 288, 0, 1), (4099, 1028, 1028, 1032, 1036, 0, 4)]


@pytest.mark.parametrize("n_rows,d,lds,ldd,ldd2,c2,vec", COPY_ROWS2)
def test_copy_rows2_copies_the_bits_to_both_destinations(n_rows, d, lds, ldd, ldd2, c2, vec, dev, lib):
    if n_rows > 4096:
        assert n_rows * (d // vec) > 4096 * 256
    src = _rand(n_rows, d, 4)
    S, D, D2 = Source(n_rows, d, lds, dev, src), Guard(n_rows, d, ldd, dev), Guard(n_rows, d, ldd2, dev, None, c2)
    assert _width(d, (4, 2), S, D, D2) == vec
    _check(lib.ngcf_copy_rows2_f32(S.ptr, S.ld, D.ptr, D.ld, D2.ptr, D2.ld, 0, d, None))
    torch.cuda.synchronize()
    assert D.untouched() and D2.untouched()
    _check(lib.ngcf_copy_rows2_f32(S.ptr, S.ld, D.ptr, D.ld, D2.ptr, D2.ld, n_rows, d, None))
    torch.cuda.synchronize()
    assert S.untouched() and D.guard_intact() and D2.guard_intact()
    assert torch.equal(D.view.cpu(), src) and torch.equal(D2.view.cpu(), src)


@pytest.mark.parametrize("n_idx", [0, 1, 5, 1025])
@pytest.mark.parametrize("d", [1, 65, 260])
def test_copy_rows_indexed_copies_the_named_rows_and_skips_bad_ids(d, n_idx, dev, lib):
    """Duplicates, ids below 0 and from n_rows on (skipped: -1, n_rows and n_rows + 7 would copy src's guard rows, which hold another
    sentinel, over dst's; +-2^40 lie far outside), rows nobody names keep what dst held."""
    n_rows = 300
    src, dst0 = _rand(n_rows, d, 5), _rand(n_rows, d, 6)
    idx = torch.randint(0, n_rows, (n_idx,), generator=torch.Generator().manual_seed(n_idx))
    if n_idx == 1:
        idx[0] = 17
    if n_idx >= 5:
        idx[1], idx[2], idx[4] = -1, n_rows, idx[0]
    if n_idx > 5:
        idx[700], idx[701], idx[1024] = 2 ** 40, -(2 ** 40), n_rows + 7
        assert len(idx.unique()) < n_idx - 300
    S, D = Source(n_rows, d, d + 3, dev, src), Guard(n_rows, d, d + 5, dev, dst0)
    idx_d = idx.to(dev)
    _check(lib.ngcf_copy_rows_indexed_f32(S.ptr, S.ld, D.ptr, D.ld, idx_d.data_ptr() if n_idx else None, n_idx, n_rows, d, None))
    torch.cuda.synchronize()
    good = idx[(idx >= 0) & (idx < n_rows)]
    want = dst0.clone()
    want[good] = src[good]
    assert S.untouched() and D.guard_intact()
    assert torch.equal(D.view.cpu(), want)


# (n, n_slots, slot_stride)
SUM_SLOTS = [(4, 1, 8), (4, 2, 8), (1028, 8, 1036), (1028, 2, 1028), (260, 8, 4096), (4099 * 1028, 2, 4099 * 1028 + 4)]


@pytest.mark.parametrize("n,n_slots,stride", SUM_SLOTS)
def test_sum_slots_adds_in_slot_order(n, n_slots, stride, dev, lib):
    if n > 10 ** 6:
        assert n // 4 > 4096 * 256                                                  # past the grid cap: the stride loop iterates
    slots = _rand(n_slots, n, 7) * 10.0 ** torch.arange(n_slots).view(-1, 1)       # slots of different scale: the order shows in the bits
    S = Source(n_slots, n, stride, dev, slots, guard=4)
    O = Guard(1, n, n, dev, guard=4)
    _check(lib.ngcf_sum_slots_f32(S.ptr, stride, n_slots, n, O.ptr, None))
    torch.cuda.synchronize()
    want = slots[0].clone()
    for q in range(1, n_slots):
        want = want + slots[q]
    assert S.untouched() and O.guard_intact()
    assert torch.equal(O.view.cpu()[0], want)
    _check(lib.ngcf_sum_slots_f32(S.ptr, stride, n_slots, 0, O.ptr, None))         # nothing to add: nothing happens
    torch.cuda.synchronize()
    assert torch.equal(O.view.cpu()[0], want)


def test_argument_errors_are_reported_and_launch_nothing(dev, lib):
    """A count that is no multiple of 4 floats for sum_slots, a leading dimension below d, a null second destination: a non-zero
    status, the routine's name in ngcf_last_error, and not a byte written."""
    from seoul_tourism_recommendation_ngcf_amd import _lib
    n_rows, d = 5, 8
    S, D, D2 = Source(n_rows, d, 12, dev, _rand(n_rows, d, 8)), Guard(n_rows, d, 12, dev), Guard(n_rows, d, 12, dev)
    idx = _i64([0, 1, 2], dev)
    calls = [
        ("sum_slots", lambda: lib.ngcf_sum_slots_f32(S.ptr, 12, 2, 7, D.ptr, None)),
        ("sum_slots", lambda: lib.ngcf_sum_slots_f32(S.ptr, 12, 2, 6, D.ptr, None)),
        ("sum_slots", lambda: lib.ngcf_sum_slots_f32(S.ptr, 10, 2, 8, D.ptr, None)),
        ("copy_rows", lambda: lib.ngcf_copy_rows_f32(S.ptr, 7, D.ptr, 12, n_rows, d, None)),
        ("copy_rows", lambda: lib.ngcf_copy_rows_f32(S.ptr, 12, D.ptr, 7, n_rows, d, None)),
        ("copy_rows", lambda: lib.ngcf_copy_rows2_f32(S.ptr, 12, D.ptr, 12, D2.ptr, 7, n_rows, d, None)),
        ("copy_rows2", lambda: lib.ngcf_copy_rows2_f32(S.ptr, 12, D.ptr, 12, None, 12, n_rows, d, None)),
        ("copy_rows_indexed", lambda: lib.ngcf_copy_rows_indexed_f32(S.ptr, 7, D.ptr, 12, idx.data_ptr(), 3, n_rows, d, None)),
        ("copy_rows_indexed", lambda: lib.ngcf_copy_rows_indexed_f32(S.ptr, 12, D.ptr, 7, idx.data_ptr(), 3, n_rows, d, None)),
        ("add_rows", lambda: lib.ngcf_add_rows_f32(D.ptr, 7, S.ptr, 12, n_rows, d, None)),
        ("add_rows", lambda: lib.ngcf_add_rows_f32(D.ptr, 12, S.ptr, 7, n_rows, d, None)),
    ]
    for name, call in calls:
        rc = call()
        assert rc != 0 and name in _lib.last_error(), (name, rc, _lib.last_error())
    torch.cuda.synchronize()
    assert S.untouched() and D.untouched() and D2.untouched()
