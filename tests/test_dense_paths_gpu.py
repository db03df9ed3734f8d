"""Every forward kernel path of ngcf_layer_dense_f32 (csrc/dense.hip) against the host oracle of tests/dense_oracle.py - the layer's
definition, not another kernel.

Exact form: integer-valued operands whose every partial sum stays below 2^24, so each kernel - the seven tile configurations of
the staged kernel in their three row layouts, direct<2,4> / <4,4>, tall + row_scale, resident, and the bf16 three-way split - must
produce `carry` bit for bit (`torch.equal`), drop exactly the elements the host's restatement of the hash drops (or the host mask's
zeros), and normalise within norm_k of the fp64 normalisation of that carry.  Each case names the path it expects and asserts it
through ngcf_dense_path after setting the options, so a case fails when the dispatch stops sending it there.  Per path: 1, T-1, T,
T+1 and 2T+5 rows of its row tile T (the full-tile and the guarded epilogue arm), the padded output width, one below it and one
above the previous step, input widths that are a multiple of 16, of 4 only, and of neither, and the modes eval, hash dropout
(p = 0.3, seed 0 and a seed >= 2^63), host mask and no carry (tests/dense_oracle.py: PADDED_PATHS, CASES).  LE and E have NaN in
their padding columns and in guard rows around them; carry and norm are column slices of sentinel-filled buffers with guard rows
before and after, none of which may change.

fp64 form: one real-valued case of mixed magnitudes per path, every row held to carry_k / norm_k; the observed maxima are printed.

The backward's layer_bwd_pre_kernel draws the same mask: with and without row_ids it must zero exactly the host's set."""
import functools

import numpy as np
import pytest
import torch

import dense_oracle as do
from test_row_kernels_gpu import Guard, Source, _pre_call

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -3.25                # in the columns and rows around the carry / norm slices
GUARD = 136                 # guard rows on either side of an operand: more than the tallest row tile (128)
# the library's defaults (csrc/common.h), set before a case's own options: the cases do not depend on NGCF_* in the environment
DEFAULTS = dict(dense_small_tiles=1, dense_tall=1, dense_direct=1, dense_resident=4, dense_resident_min_rows=106496)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _pkg():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg


def _operand(data, layout, which, dev):
    """`data` [n, d] (CPU float32) as a view of a NaN-filled device buffer with GUARD rows of NaN before and after.  padded: rows
    of a multiple of 4 floats beyond d (LE and E differ), 16-byte aligned; odd: an odd leading dimension, the view starts at column
    1; tight: d < 4 in rows of 4 floats."""
    n, d = data.shape
    if layout == "padded":
        ld, c0 = (d + 3) // 4 * 4 + 4 * (1 + which), 0
    elif layout == "odd":
        ld, c0 = d + 2 + (d + 1) % 2 + 2 * which, 1
        assert ld % 2 == 1
    else:
        assert layout == "tight" and d < 4
        ld, c0 = 4, 0
    buf = torch.full((n + 2 * GUARD, ld), NAN, device=dev)
    view = buf[GUARD:GUARD + n, c0:c0 + d]
    view.copy_(data)
    assert (view.data_ptr() % 16 == 0 and ld % 4 == 0) == (layout != "odd")
    return view


class _Output:
    """[n, d] at column `off` of a [GUARD + n + GUARD, d + extra] buffer full of SENT."""

    def __init__(self, n, d, off, extra, dev):
        self.buf = torch.full((n + 2 * GUARD, d + extra), SENT, device=dev)
        self.inside = (slice(GUARD, GUARD + n), slice(off, off + d))
        self.view = self.buf[self.inside]

    def take(self):
        """The slice as a CPU array, after asserting that nothing outside it was written."""
        got = self.view.cpu().numpy().copy()
        probe = self.buf.clone()
        probe[self.inside] = SENT
        assert bool((probe == SENT).all()), "a store outside the output slice"
        return got


def _run(lib_options, dev, path, opts, ins, layout, mode, mask, seed):
    """One call of the layer under `opts`; asserts the path by name; returns (carry or None, norm) as CPU float32 arrays."""
    pkg = _pkg()
    eng, lib = pkg.engine, pkg._lib.load()
    lib_options(**{**DEFAULTS, **opts})
    LE, E, W1, b1, W2, b2 = (torch.as_tensor(np.asarray(a, dtype=np.float32)) for a in ins)
    n, d_in, d_out = LE.shape[0], LE.shape[1], W1.shape[0]
    LEd, Ed = _operand(LE, layout, 0, dev), _operand(E, layout, 1, dev)
    got = lib.ngcf_dense_path(n, d_in, d_out, LEd.data_ptr(), LEd.stride(0), Ed.data_ptr(), Ed.stride(0))
    assert got is not None and got.decode() == path, f"the dispatch sends this case to {got}, not to {path}"
    carry = None if mode == "last" else _Output(n, d_out, seed % 5, 6, dev)
    norm = _Output(n, d_out, (seed + 2) % 4, 5, dev)
    mask_d = None
    if mask is not None:                # a slice of a wider matrix with NaN past d_out
        mask_d = torch.full((n, d_out + 5), NAN, device=dev)[:, :d_out]
        mask_d.copy_(torch.as_tensor(mask))
    kw = dict(drop_p=do.DROP_P if mode in do.HASH_SEED or mode == "mask" else 0.0, drop_seed=do.HASH_SEED.get(mode, 0), drop_mask=mask_d)
    eng.layer_dense(LEd, Ed, *(t.to(dev) for t in (W1, b1, W2, b2)), None if carry is None else carry.view, norm.view,
                    eng.Workspace(), **kw)
    torch.cuda.synchronize()
    return (None if carry is None else carry.take()), norm.take()


def _check_exact(c, lib_options, dev):
    ins, keep, mask, want, M, scale = do.case_expected(c)
    carry, norm = _run(lib_options, dev, c.path, c.opts, ins, c.layout, c.mode, mask, c.seed)
    zeros = want == 0
    if carry is not None:
        bad = carry != want            # NaN compares unequal too
        assert not bad.any(), (f"{int(bad.sum())} elements of carry differ from the exact layer, first at {tuple(np.argwhere(bad)[0])}: "
                               f"{carry[bad][0]!r} for {want[bad][0]!r}")
        assert torch.equal(torch.from_numpy(carry), torch.from_numpy(want))
    # the dropped set: zeros exactly where the host's mask drops (or where the integer M is 0)
    dropped = ~keep if keep is not None else (mask == 0 if mask is not None else np.zeros_like(zeros))
    assert np.array_equal(zeros, dropped | (M == 0))
    assert np.array_equal(norm == 0, zeros), "the zeros of norm are not the dropped set"
    if carry is not None:
        assert np.array_equal(carry == 0, zeros)
    err, zero_row = do.norm_error(norm, want, scale)
    assert err <= do.norm_k(c.d_in, c.d_out), (err, do.norm_k(c.d_in, c.d_out))
    lengths = np.linalg.norm(norm.astype(np.float64), axis=1)
    assert not lengths[zero_row].any()                                     # a zero row normalises to zeros
    assert all(zero_row[r] for r in do.zero_rows_of(c))
    if (~zero_row).any():
        assert np.abs(lengths[~zero_row] - 1).max() < 1e-5                 # every other row is a unit row


def _exact(family):
    return pytest.mark.parametrize("c", do.CASES[family], ids=do.case_id)


@_exact("staged")
def test_staged_kernel_every_tile_configuration_and_row_layout_is_exact(c, lib_options, dev):
    _check_exact(c, lib_options, dev)


@_exact("direct")
def test_direct_kernel_is_exact(c, lib_options, dev):
    _check_exact(c, lib_options, dev)


@_exact("tall")
def test_tall_kernel_and_row_scale_are_exact(c, lib_options, dev):
    _check_exact(c, lib_options, dev)


@_exact("resident")
def test_resident_kernel_is_exact(c, lib_options, dev):
    _check_exact(c, lib_options, dev)


@_exact("split")
def test_split_kernel_is_exact_on_integers(c, lib_options, dev):
    _check_exact(c, lib_options, dev)


@pytest.mark.parametrize("path,opts,n,d_in,d_out,mode,layout", do.FP64_CASES, ids=[f"{c[0]}-{c[2]}x{c[3]}to{c[4]}-{c[5]}" for c in do.FP64_CASES])
def test_every_path_is_within_the_fp64_bounds_on_mixed_magnitudes(path, opts, n, d_in, d_out, mode, layout, lib_options, dev):
    """Real-valued operands from 1e-3 to 1e3 (dense_oracle.mixed_inputs), every row against fp64: |carry - act| <= carry_k 2^-24 scale
    and ||act|| |norm - act / ||act||| <= norm_k 2^-24 S; the rows 0, 97, 194 are zero rows."""
    seed = 7 + n + d_in + d_out
    ins = do.mixed_inputs(n, d_in, d_out, seed)
    keep = mask = None
    rows, cols = np.arange(n), np.arange(d_out)
    if mode in do.HASH_SEED:
        keep = do.msg_keep(do.HASH_SEED[mode], rows, cols, do.DROP_P)
    elif mode == "mask":
        mask = ((torch.rand((n, d_out), generator=torch.Generator().manual_seed(seed)) > do.DROP_P).float() / 0.7).numpy()
        keep = mask != 0
    carry, norm = _run(lib_options, dev, path, opts, [t.numpy() for t in ins], layout, mode, mask, seed)
    ref = do.fp64_layer(*ins, keep=None if keep is None else torch.from_numpy(keep))
    zero_row = np.zeros(n, dtype=bool)
    zero_row[::97] = True
    dropped = zero_row[:, None] | (~keep if keep is not None else False)
    assert np.isfinite(norm).all() and np.array_equal(norm == 0, np.broadcast_to(dropped, norm.shape))
    e_carry = None
    if carry is not None:
        assert np.array_equal(carry == 0, norm == 0)
        e_carry = ref.err_carry(torch.from_numpy(carry)) / do.U32
    e_norm = ref.err_norm(torch.from_numpy(norm)) / do.U32
    print(f"\n{path}: {n} x {d_in} -> {d_out} {mode}: carry error {'-' if e_carry is None else round(e_carry, 2)} "
          f"(carry_k {do.carry_k(d_in)}), norm error {e_norm:.2f} (norm_k {do.norm_k(d_in, d_out):.0f}), in units of 2^-24")
    assert e_carry is None or e_carry <= do.carry_k(d_in)
    assert e_norm <= do.norm_k(d_in, d_out)
    lengths = np.linalg.norm(norm.astype(np.float64), axis=1)
    all_zero = dropped.all(axis=1) if keep is not None else zero_row
    assert not lengths[all_zero].any() and np.abs(lengths[~all_zero] - 1).max() < 1e-5


# ---- the backward draws the forward's mask -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pre_case(d):
    rng = np.random.default_rng(d)
    n = 133
    dC = (rng.integers(1, 4, (n, d)) * rng.choice(np.array([-1, 1]), (n, d))).astype(np.float32)
    C = (rng.integers(1, 3, (n, d)) * rng.choice(np.array([-1, 1]), (n, d))).astype(np.float32)
    ids = np.sort(rng.choice(3_000_000_000, n - 3, replace=False))
    ids = np.concatenate((ids, [2 ** 31, 2 ** 32 + 5, 2 ** 40 + 1])).astype(np.int64)      # matrix rows past 2^31 and 2^32
    return dC, C, ids


@pytest.mark.parametrize("seed", [do.SEED_HI, 0], ids=["seed_hi", "seed0"])
@pytest.mark.parametrize("d", [64, 65])
def test_layer_bwd_pre_hash_dropout_zeroes_exactly_the_forwards_set(d, seed, dev):
    """ngcf_layer_bwd_pre_f32 with drop_p = 0.3 and no mask tensor, dC only (non-zero integers): dM = msg_drop(dC) * (C > 0 ? 1 : 0.2f)
    restated in float32, zero exactly where msg_keep drops - for rows 0 .. n-1, and with row_ids for those matrix rows.  d = 64
    takes the two-column kernel, 65 the scalar one."""
    lib = _pkg()._lib.load()
    dC, C, ids = _pre_case(d)
    n = len(dC)
    slope = np.where(C > 0, np.float32(1.0), do.LEAKY).astype(np.float32)
    for rows, row_ids in ((np.arange(n), None), (ids, torch.from_numpy(ids).to(dev))):
        keep = do.msg_keep(seed, rows, np.arange(d), do.DROP_P)
        want = (np.where(keep, (dC * do.keep_scale(do.DROP_P)).astype(np.float32), np.float32(0.0)).astype(np.float32) * slope).astype(np.float32)
        ld = d + 2
        got = _pre_call(lib, n, d, None, Source(n, d, ld, dev, dC), Source(n, d, ld, dev, C), None, Guard(n, d, ld, dev), do.DROP_P, seed,
                        row_ids=row_ids).numpy()
        assert np.array_equal(got == 0, ~keep), "the backward zeroes another set than the forward's mask"
        assert np.array_equal(got, want)
        assert 0.25 < (~keep).mean() < 0.35
