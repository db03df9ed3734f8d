"""layer_dense_split_kernel (dense_resident = 4, the default): the large-row dense layer on the bf16 matrix cores with an exact
three-way split of every fp32 operand.  Not bit-identical to the fp32 kernels, so it is held to their accuracy instead: on sampled
rows its error against an fp64 restatement of the layer is at most twice that of layer_dense_resident_kernel (dense_resident = 1)
on the same inputs, and within an absolute bound derived from its accumulation chain (`carry_k`, `norm_k`); the dropout zero
pattern is the fp32 path's, bit for bit, and the rows of the normalised block are unit rows.

The kernel runs from dense_resident_min_rows rows on; the sweep lowers that option (`lib_options`) so that its whole shape range -
1..9 input chunks, full and partial last chunks, 97..128 output columns (and 32 / 64 on <= 16 384 rows, where the small-tile rule
pads them to 128), 1..131 073 rows - runs at small row counts, with poisoned padding around every operand and output."""
import numpy as np
import pytest
import torch

from dense_oracle import U32, carry_k, fp64_layer, norm_k      # the bounds and error measures live with the layer's host oracle

pytestmark = pytest.mark.gpu

N_ROWS = 140_001            # above dense_resident_min_rows; not a multiple of 32: a partial last tile
SENT = -3.25                # sentinel in the columns around the carry / norm slices


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a ROCm device")
    return torch.device("cuda:0")


def _pkg():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg


def _inputs(d_in, d_out, mode, mixed, dev):
    g = torch.Generator().manual_seed(1000 + d_in + d_out + len(mode) + (7 if mixed else 0))
    n = N_ROWS
    ld = (d_in + 31) // 32 * 32
    LE = torch.randn((n, ld), generator=g) * 0.5
    E = torch.randn((n, ld), generator=g) * 0.5
    W1, W2 = (torch.randn((d_out, d_in), generator=g) * 0.1 for _ in range(2))
    b1, b2 = (torch.randn((d_out,), generator=g) * 0.1 for _ in range(2))
    if mixed:
        # magnitudes from 1e-3 to 1e3 per row and per element, every 97th row zero; zero biases so that a zero row of the
        # operands gives a zero output row (normalised to zeros)
        LE *= 10.0 ** (torch.rand((n, 1), generator=g) * 6 - 3)
        E *= 10.0 ** (torch.rand((n, ld), generator=g) * 6 - 3)
        W1 *= 10.0 ** (torch.rand((d_out, d_in), generator=g) * 2 - 1)
        LE[::97] = 0.0
        E[::97] = 0.0
        b1.zero_()
        b2.zero_()
    mask = (torch.rand((n, d_out), generator=g) > 0.3).float() / 0.7 if mode == "mask" else None
    return LE, E, W1, b1, W2, b2, mask


def _run(eng, dev, resident, lib_options, LE, E, W1, b1, W2, b2, mask, mode, d_out):
    if resident is not None:
        lib_options(dense_resident=resident)
    n = LE.shape[0]
    carry = None if mode == "last" else torch.full((n, d_out), 5.0, device=dev)
    norm = torch.full((n, d_out + 3), 7.0, device=dev)[:, :d_out]
    kw = dict(drop_p=0.3 if mode in ("hash", "mask") else 0.0, drop_seed=77 if mode == "hash" else 0, drop_mask=mask)
    eng.layer_dense(LE, E, W1, b1, W2, b2, carry, norm, eng.Workspace(), **kw)
    torch.cuda.synchronize()
    assert bool((norm.as_strided((n, 3), (d_out + 3, 1), d_out) == 7.0).all())      # nothing written past the slice
    return (None if carry is None else carry.cpu()), norm.cpu()


def _check_against_fp64(le, e, W1, b1, W2, b2, mode, keep, c32, n32, csp, nsp):
    """Errors of both kernels on the sampled rows (CPU tensors: le, e [R, d_in]; the outputs' rows [R, d_out], carries None in
    mode "last"; keep the dropout keep pattern or None) against fp64; asserts the split kernel's bounds."""
    d_in, d_out = le.shape[1], W1.shape[0]
    ref = fp64_layer(le, e, W1, b1, W2, b2, keep)
    err_carry, err_norm = ref.err_carry, ref.err_norm

    out = {}
    # the fp32 kernel is the yardstick, so it is held to the same bounds (its chain is shorter: 2 d_in fp32 products and sums)
    if mode != "last":
        e32, esp = err_carry(c32), err_carry(csp)
        out["carry"] = (esp, e32)
        assert e32 <= carry_k(d_in) * U32, ("fp32 kernel", e32 / U32, carry_k(d_in))
        assert esp <= 2 * e32 + U32, (esp, e32)
        assert esp <= carry_k(d_in) * U32, (esp / U32, carry_k(d_in))
    e32, esp = err_norm(n32), err_norm(nsp)
    out["norm"] = (esp, e32)
    assert e32 <= norm_k(d_in, d_out) * U32, ("fp32 kernel", e32 / U32, norm_k(d_in, d_out))
    assert esp <= 2 * e32 + U32, (esp, e32)
    assert esp <= norm_k(d_in, d_out) * U32, (esp / U32, norm_k(d_in, d_out))
    print("errors / 2^-24 (split, fp32):", {k: (round(a / U32, 2), round(b / U32, 2)) for k, (a, b) in out.items()})
    return out


@pytest.mark.parametrize("mixed", [False, True], ids=["normal", "mixed"])
@pytest.mark.parametrize("mode", ["eval", "hash", "mask", "last"])
@pytest.mark.parametrize("d_in", [128, 130])
def test_split_dense_kernel_error_is_within_twice_the_fp32_kernels(d_in, mode, mixed, dev, lib_options):
    eng = _pkg().engine
    d_out = 128
    LE, E, W1, b1, W2, b2, mask = _inputs(d_in, d_out, mode, mixed, dev)
    args = [t.to(dev) for t in (LE, E, W1, b1, W2, b2)]
    args[0], args[1] = args[0][:, :d_in], args[1][:, :d_in]
    mask_d = None if mask is None else mask.to(dev)
    c32, n32 = _run(eng, dev, 1, lib_options, *args, mask_d, mode, d_out)
    csp, nsp = _run(eng, dev, 4, lib_options, *args, mask_d, mode, d_out)

    # sampled rows: a spread over the matrix, the partial last tile, and (mixed) zero rows
    rng = np.random.default_rng(d_in)
    rows = np.unique(np.concatenate([rng.choice(N_ROWS, 2048, replace=False), np.arange(N_ROWS - 17, N_ROWS),
                                     np.arange(0, 97 * 8, 97)]))
    r = torch.from_numpy(rows)
    keep = None
    if mode in ("hash", "mask"):
        keep = c32[r] != 0 if mode == "hash" else mask[r] != 0
        assert torch.equal(csp == 0, c32 == 0)        # the dropout zero pattern of the fp32 path
        if mode == "hash" and not mixed:
            assert abs(float((csp == 0).float().mean()) - 0.3) < 0.01
    sel = (lambda c: None) if mode == "last" else (lambda c: c[r])
    _check_against_fp64(LE[r, :d_in], E[r, :d_in], W1, b1, W2, b2, mode, keep, sel(c32), n32[r], sel(csp), nsp[r])
    if mode in ("hash", "mask"):
        assert torch.equal(nsp == 0, n32 == 0)
    norms = nsp.double().norm(dim=1)
    if mixed:
        zero = torch.zeros(N_ROWS, dtype=torch.bool)
        zero[::97] = True
        assert bool((nsp[zero] == 0).all())             # a zero row stays zeros
        norms = norms[~zero]
    assert float((norms - 1).abs().max()) < 1e-5


def test_split_dense_kernel_is_the_default_and_fp32_values_select_fp32_kernels(dev, lib_options):
    """The default option takes the split kernel at C3-sized shapes, and dense_resident = 1 / 0 keep the fp32 kernels, which agree
    bit for bit with each other (same k order) but not with the split kernel."""
    eng = _pkg().engine
    d_in = d_out = 128
    LE, E, W1, b1, W2, b2, _ = _inputs(d_in, d_out, "eval", False, dev)
    args = [t.to(dev) for t in (LE, E, W1, b1, W2, b2)]
    import os
    default = None if "NGCF_DENSE_RESIDENT" in os.environ else _run(eng, dev, None, lib_options, *args, None, "eval", d_out)
    outs = {res: _run(eng, dev, res, lib_options, *args, None, "eval", d_out) for res in (1, 0, 4)}
    if default is not None:
        assert torch.equal(default[0], outs[4][0]) and torch.equal(default[1], outs[4][1])
    assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])
    assert not torch.equal(outs[4][0], outs[1][0])
    torch.testing.assert_close(outs[4][0], outs[1][0], rtol=1e-4, atol=1e-5)


# ---- the whole shape range at small row counts ------------------------------------------------------------------------------

def _poisoned(n, d, ld, poison, data):
    """`data` [n, d] as the column slice of an [n, ld] device matrix whose other columns hold `poison`."""
    big = torch.full((n, ld), poison, device=data.device)
    big[:, :d] = data
    return big[:, :d]


def _sweep_inputs(n, d_in, d_out, mode, mixed, poison, seed, dev):
    """Device inputs of one sweep case: LE and E as column slices of wider 16-byte aligned matrices (different leading dimensions,
    `poison` in the padding), the host mask [n, d_out] as a slice of a matrix with NaN past d_out."""
    g = torch.Generator(device=dev).manual_seed(seed)
    r4 = (d_in + 3) // 4 * 4
    LE = torch.randn((n, d_in), generator=g, device=dev) * 0.5
    E = torch.randn((n, d_in), generator=g, device=dev) * 0.5
    W1, W2 = (torch.randn((d_out, d_in), generator=g, device=dev) * 0.1 for _ in range(2))
    b1, b2 = (torch.randn((d_out,), generator=g, device=dev) * 0.1 for _ in range(2))
    if mixed:       # as _inputs: 1e-3..1e3 per row and per element, every 97th row zero, zero biases
        LE *= 10.0 ** (torch.rand((n, 1), generator=g, device=dev) * 6 - 3)
        E *= 10.0 ** (torch.rand((n, d_in), generator=g, device=dev) * 6 - 3)
        W1 *= 10.0 ** (torch.rand((d_out, d_in), generator=g, device=dev) * 2 - 1)
        LE[::97] = 0.0
        E[::97] = 0.0
        b1.zero_()
        b2.zero_()
    LE = _poisoned(n, d_in, r4 + 4 * (1 + seed % 3), poison, LE)
    E = _poisoned(n, d_in, r4 + 4 * (1 + (seed + 1) % 3), poison, E)
    mask = None
    if mode == "mask":
        mask = _poisoned(n, d_out, d_out + 5, float("nan"), (torch.rand((n, d_out), generator=g, device=dev) > 0.3).float() / 0.7)
    return LE, E, W1, b1, W2, b2, mask


def _run_sliced(eng, lib_options, resident, LE, E, W1, b1, W2, b2, mask, mode, c_off, n_off):
    """One call with carry and norm as column slices (at column offsets c_off / n_off) of wider matrices filled with SENT; asserts
    that every column outside the slices still holds SENT and returns the slices (carry None in mode "last")."""
    lib_options(dense_resident=resident)
    n, d_out = LE.shape[0], W1.shape[0]
    cbig = None if mode == "last" else torch.full((n, d_out + 6), SENT, device=LE.device)
    nbig = torch.full((n, d_out + 5), SENT, device=LE.device)
    carry = None if cbig is None else cbig[:, c_off:c_off + d_out]
    norm = nbig[:, n_off:n_off + d_out]
    kw = dict(drop_p=0.3 if mode in ("hash", "mask") else 0.0, drop_seed=1234 if mode == "hash" else 0, drop_mask=mask)
    eng.layer_dense(LE, E, W1, b1, W2, b2, carry, norm, eng.Workspace(), **kw)
    torch.cuda.synchronize()
    for big, off in ((cbig, c_off), (nbig, n_off)):
        if big is not None:
            outside = torch.ones(big.shape[1], dtype=torch.bool, device=big.device)
            outside[off:off + d_out] = False
            assert bool((big[:, outside] == SENT).all()), "a store outside the output slice"
    return (None if carry is None else carry.clone()), norm.clone()


def _sweep_cases():
    d_ins = [4, 5, 16, 17, 33, 48, 64, 100, 113, 127, 128, 129, 130, 143, 144]     # 1..9 chunks, full / partial last chunk
    d_outs = [97, 100, 127, 128]
    rows = [1, 31, 32, 33, 4099, 65535, 65536, 65537, 131073]                      # 65 536 rows: 2 048 tiles, one per wave
    modes = ["eval", "hash", "mask", "last"]
    cases = []
    for i in range(60):             # every (d_in, d_out) pair once; rows, modes and data cycled against them
        cases.append((d_ins[i % 15], d_outs[i % 4], rows[i % 9], modes[(i + i // 4) % 4], (i // 15) % 2 == 1,
                      "nan" if i % 2 else "inf", i))
    # <= 16 384 rows: narrow layers are padded to 128 output columns (small_rows), so with a lowered dense_resident_min_rows the
    # split kernel runs them too
    for j, (d_in, d_out, n, mode, mixed) in enumerate([(64, 32, 4099, "eval", False), (130, 64, 16384, "hash", True),
                                                        (17, 32, 33, "mask", False), (144, 64, 1, "last", True),
                                                        (100, 64, 16384, "mask", True), (5, 32, 16383, "eval", True)]):
        cases.append((d_in, d_out, n, mode, mixed, "inf" if j % 2 else "nan", 60 + j))
    return cases


@pytest.mark.parametrize("d_in,d_out,n,mode,mixed,poison,seed", _sweep_cases(),
                         ids=lambda v: str(v) if not isinstance(v, bool) else ("mixed" if v else "normal"))
def test_split_dense_kernel_shape_sweep_against_fp64(d_in, d_out, n, mode, mixed, poison, seed, dev, lib_options):
    """The split kernel against fp64 (absolute bound) and against the fp32 resident kernel (at most twice its error) across its
    shape range, with NaN / +Inf in the padding columns of LE and E (selected away, never multiplied by zero), NaN past d_out in the
    host mask, and carry / norm as column slices of sentinel-filled matrices (nothing stored outside them)."""
    eng = _pkg().engine
    lib_options(dense_resident_min_rows=1)
    LE, E, W1, b1, W2, b2, mask = _sweep_inputs(n, d_in, d_out, mode, mixed, float(poison), seed, dev)
    c_off, n_off = seed % 5, (seed + 2) % 4
    c32, n32 = _run_sliced(eng, lib_options, 1, LE, E, W1, b1, W2, b2, mask, mode, c_off, n_off)
    csp, nsp = _run_sliced(eng, lib_options, 4, LE, E, W1, b1, W2, b2, mask, mode, c_off, n_off)
    assert bool(torch.isfinite(nsp).all()) and (csp is None or bool(torch.isfinite(csp).all()))
    if mode in ("hash", "mask"):
        ref = c32 if c32 is not None else n32
        assert torch.equal(nsp == 0, n32 == 0) and torch.equal(csp == 0, ref == 0)

    rng = np.random.default_rng(seed)
    rows = np.unique(np.concatenate([rng.choice(n, min(n, 1024), replace=False), np.arange(min(n, 40)),
                                     np.arange(max(0, n - 40), n), np.arange(0, min(n, 97 * 6), 97)]))
    r = torch.from_numpy(rows).to(dev)
    keep = None
    if mode == "hash":
        keep = (c32[r] != 0).cpu()
    elif mode == "mask":
        keep = (mask[r] != 0).cpu()
    cpu = lambda t: None if t is None else t[r].cpu()          # noqa: E731
    _check_against_fp64(LE[r].cpu(), E[r].cpu(), W1.cpu(), b1.cpu(), W2.cpu(), b2.cpu(), mode, keep,
                        cpu(c32), cpu(n32), cpu(csp), cpu(nsp))
    norms = nsp.double().norm(dim=1)
    if mixed:
        zero = torch.zeros(n, dtype=torch.bool, device=dev)
        zero[::97] = True
        assert bool((nsp[zero] == 0).all())
        norms = norms[~zero]
    if norms.numel():
        assert float((norms - 1).abs().max()) < 1e-5


def _layer(eng, LE, E, W1, b1, W2, b2, mask=None, drop_p=0.0, drop_seed=0):
    n, d_out = LE.shape[0], W1.shape[0]
    carry = torch.full((n, d_out), SENT, device=LE.device)
    norm = torch.full((n, d_out), SENT, device=LE.device)
    eng.layer_dense(LE, E, W1, b1, W2, b2, carry, norm, eng.Workspace(), drop_p=drop_p, drop_seed=drop_seed, drop_mask=mask)
    torch.cuda.synchronize()
    return carry, norm


@pytest.mark.parametrize("mode", ["eval", "mask"])
def test_split_dense_kernel_rows_are_independent_and_runs_repeat(mode, dev, lib_options):
    """A row's result does not depend on which other rows are in the call or where its tile starts: the rows of LE[a:b] (a, b off
    tile boundaries) equal the same rows of the full call bit for bit; a second call repeats the first bit for bit."""
    eng = _pkg().engine
    lib_options(dense_resident=4, dense_resident_min_rows=1)
    n, d_in, d_out = 70_001, 130, 100
    LE, E, W1, b1, W2, b2, mask = _sweep_inputs(n, d_in, d_out, mode, False, float("nan"), 5, dev)
    kw = dict(mask=mask, drop_p=0.3) if mode == "mask" else {}
    full = _layer(eng, LE, E, W1, b1, W2, b2, **kw)
    again = _layer(eng, LE, E, W1, b1, W2, b2, **kw)
    assert torch.equal(full[0], again[0]) and torch.equal(full[1], again[1])
    for a, b in ((12_345, 60_001), (0, 17), (69_990, n), (31, 33)):
        kw_s = dict(mask=mask[a:b], drop_p=0.3) if mode == "mask" else {}
        part = _layer(eng, LE[a:b], E[a:b], W1, b1, W2, b2, **kw_s)
        assert torch.equal(part[0], full[0][a:b]) and torch.equal(part[1], full[1][a:b]), (a, b)
    lib_options(dense_resident=0)
    staged = _layer(eng, LE, E, W1, b1, W2, b2, **kw)
    assert not torch.equal(staged[0], full[0])                 # the split kernel did run


MIN_ROWS = 17_000           # a lowered threshold above the small-tile limit (16 384 rows)


@pytest.mark.parametrize("d_in,d_out,n,ld_pad,split", [
    (144, 128, MIN_ROWS, 0, True), (145, 128, MIN_ROWS, 0, False),              # at most 9 chunks of weights in LDS
    (128, 96, MIN_ROWS + 1, 0, False), (128, 97, MIN_ROWS + 1, 0, True),       # 97..128 output columns
    (128, 128, MIN_ROWS + 1, 0, True), (128, 129, MIN_ROWS + 1, 0, False),
    (100, 128, MIN_ROWS - 1, 0, False), (100, 128, MIN_ROWS, 0, True),         # from dense_resident_min_rows rows
    (128, 128, MIN_ROWS + 5, 1, False), (130, 100, MIN_ROWS + 5, 3, False),    # LE rows not 16-byte aligned
    (130, 100, MIN_ROWS + 5, 4, True)])                                         # aligned again
def test_split_dense_kernel_dispatch_boundaries(d_in, d_out, n, ld_pad, split, dev, lib_options):
    """Which kernel ran, told by the bits: the split kernel never matches the fp32 kernels bit for bit on generic data, the fp32
    kernels match each other (dense_resident = 0 keeps the staged kernel).  Just inside and just outside every limit of the split
    kernel's dispatch: d_in <= 144, 97 <= d_out <= 128, n_rows >= dense_resident_min_rows, 16-byte aligned rows of LE."""
    eng = _pkg().engine
    lib_options(dense_resident_min_rows=MIN_ROWS)
    g = torch.Generator(device=dev).manual_seed(d_in * 1000 + d_out + n)
    LE = _poisoned(n, d_in, (d_in + 3) // 4 * 4 + ld_pad, float("nan"), torch.randn((n, d_in), generator=g, device=dev) * 0.5)
    E = _poisoned(n, d_in, (d_in + 3) // 4 * 4 + 4, float("nan"), torch.randn((n, d_in), generator=g, device=dev) * 0.5)
    W1, W2 = (torch.randn((d_out, d_in), generator=g, device=dev) * 0.1 for _ in range(2))
    b1, b2 = (torch.randn((d_out,), generator=g, device=dev) * 0.1 for _ in range(2))
    lib_options(dense_resident=4)
    got = _layer(eng, LE, E, W1, b1, W2, b2)
    lib_options(dense_resident=0)
    want = _layer(eng, LE, E, W1, b1, W2, b2)
    assert bool(torch.isfinite(got[1]).all())
    same = torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert same != split, "split kernel expected" if split else "fall-back to the fp32 kernels expected"
    if split:
        torch.testing.assert_close(got[0], want[0], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("d_in,d_out", [(128, 128), (130, 100), (64, 32), (256, 256), (515, 512)])
@pytest.mark.parametrize("resident", [4, 1, 0])
def test_layer_dense_with_no_rows_is_a_no_op(d_in, d_out, resident, dev, lib_options):
    """n_rows = 0 returns OK and writes nothing, also with dense_resident_min_rows = 0 (which would otherwise send the empty call
    to a persistent kernel whose rows clamp to row -1).  Called through the C entry point: an empty torch tensor has no data
    pointer to pass."""
    from seoul_tourism_recommendation_ngcf_amd import _lib
    eng = _pkg().engine
    lib = _lib.load()
    lib_options(dense_resident=resident, dense_resident_min_rows=0, dense_tall=2, dense_direct=2)
    LE, E = (torch.full((4, d_in), float("nan"), device=dev) for _ in range(2))
    W1, W2 = torch.ones((d_out, d_in), device=dev), torch.ones((d_out, d_in), device=dev)
    b1, b2 = torch.zeros(d_out, device=dev), torch.zeros(d_out, device=dev)
    carry, norm = (torch.full((4, d_out), SENT, device=dev) for _ in range(2))
    ws = eng.Workspace().get(int(lib.ngcf_dense_workspace_bytes(d_in, d_out)), dev)
    p = eng._ptr
    for drop_p, c in ((0.0, carry), (0.3, None)):
        rc = lib.ngcf_layer_dense_f32(p(LE), d_in, p(E), d_in, 0, d_in, p(W1), p(b1), p(W2), p(b2), d_out, eng.LEAKY_SLOPE, drop_p,
                                      5, None, 0, p(c), d_out, p(norm), d_out, p(ws), ws.numel(), eng._stream())
        assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((carry == SENT).all()) and bool((norm == SENT).all())
