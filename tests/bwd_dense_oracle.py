"""Host oracle of a layer's dense half in the backward pass as include/ngcf_hip.h defines it (ngcf_layer_bwd_weight_f32,
ngcf_layer_bwd_input_f32), in numpy / CPU torch, written from the header and the comments of csrc/bwd_dense.hip - no code shared
with the product, nothing here runs on a GPU.  tests/test_bwd_dense_oracle.py checks it on the CPU against float64 autograd of
the layer's definition; tests/test_bwd_dense_paths_gpu.py holds every backward dense kernel to it.

    gW1 = dM^T (LE + E)     gW2 = dM^T (LE * E)     gb2 = column sums of dM     gb1 = 2 gb2
    dS = dM W1              dP = dM W2              dLE = dS + dP * E           dE = dS + dP * LE

EXACT form (`exact_weight`, `exact_input`).  dM, LE, E, W1, W2 hold integers in -3..3, every value present in every operand of
seven elements or more.  LE + E and LE * E are then integers of magnitude <= 6 and <= 9, and every product and every partial sum of
an output element is an integer of magnitude at most
    weight gradient:  n_rows * max|dM| * max(max|LE| + max|E|, max|LE| max|E|)
    input gradient:   d_out * max|dM| * max(max|W1|, max|W2|) * (1 + max(max|E|, max|LE|))
asserted to be below 2^24 for each case: such a sum is the same in any order, with or without fma, through
v_mfma_f32_32x32x2_f32, in per-workgroup partials or a butterfly.  The products are formed in float64 BLAS (exact here) and cast to
float32.  No tolerance: every output must equal this bit for bit.

fp64 form (`fp64_weight`, `fp64_input`): real-valued operands of mixed magnitudes, the error of every ELEMENT held to
k * 2^-24 * S with S the same product formed from absolute values.  The operand [LE+E | LE*E] is formed in float32 as the kernels
form it (one fp32 add, one fp32 multiply per element, no contraction possible), so it carries no error against the reference, which
forms it the same way and continues in float64.  Every fp32 addition counts as one rounding of relative size 2^-24 of a partial sum
that is at most S; nothing is assumed about the order or the width of the MFMA's internal adder; a product counts as rounded before
it is added.  An element that passes through n additions and one product rounding is then off by at most (n + 1) 2^-24 S to first
order; the second order is covered by the factor (1 + k 2^-24) (`bound`).

  weight gradient, matrix-core kernel (`weight_k`): a workgroup adds the rows of its ceil(n_blocks / n_wg) blocks of 32 rows into
  one accumulator per output element: R = ceil(n_blocks / n_wg) * 32 additions (rows past the end add exact zeros), 1 for the
  products' own roundings.  bwd_weight_reduce_kernel then adds the n_wg partials: a quarter of them, per = ceil(n_wg / 4), per
  wave, on eight chains of ceil(per / 8) additions, three levels to combine the chains, three additions for the four quarters:
  D = ceil(ceil(n_wg / 4) / 8) + 6.                                        k = R + 1 + D.
  weight gradient, narrow kernel: a workgroup owns per = ceil(n_rows / 2048) rows, its two halves alternate groups of 8 rows:
  a chain of 8 ceil(per / 16) fmaf (one rounding each, the product is not rounded), one addition of the two halves, then the same
  reduction over 2 048 partials (D = 70).                                  k = 8 ceil(per / 16) + 1 + D.
  bias gradient gb2 (`bias_k`; S = column sums of |dM|; gb1 = 2 gb2 is exact): matrix-core kernel: a thread adds 8 rows of each of
  the workgroup's blocks (R / 4 additions), three additions for the four row quarters, then D.  Narrow kernel: as its weights.
  input gradient, staged and resident kernels (`input_k`): one accumulator per element of dS and of dP walks k = 0 .. d_out - 1:
  d_out - 1 additions (the first product meets a zero accumulator; the zero padding adds exact zeros), 1 for the products'
  roundings; the epilogue's fmaf(dP, E, dS) rounds once:                   k = d_out + 1.
  input gradient, narrow kernel: a lane holds k = lane and lane + 64: m0 * w (1 rounding), fmaf (1), the halving butterfly over
  lane bits 5..0 (6 additions), the epilogue's fmaf (1):                   k = 9 at any d_out <= 128.
"""
from collections import namedtuple

import numpy as np
import torch

U32 = 2.0 ** -24
GUARD_ROWS = 136            # guard rows around a row operand on the device: more than the tallest row tile (128)
A0 = 0x7F0000000000         # a 256-byte aligned address for the host-only path queries (never dereferenced)


# ---- the dispatch rules, restated from include/ngcf_hip.h ------------------------------------------------------------------------
def weight_workgroups(n_rows, d_in):
    if d_in <= 4 and n_rows >= 65536:
        return 2048
    return min(256, max(1, ((n_rows + 31) // 32 + 1) // 2))


def reduce_depth(n_wg):
    return -(-(-(-n_wg // 4)) // 8) + 6


def weight_k(path, n_rows, d_in):
    n_wg = weight_workgroups(n_rows, d_in)
    if path == "narrow":
        per = -(-n_rows // n_wg)
        return 8 * -(-per // 16) + 1 + reduce_depth(n_wg)
    n_blocks = (n_rows + 31) // 32
    return -(-n_blocks // n_wg) * 32 + 1 + reduce_depth(n_wg)


def bias_k(path, n_rows, d_in):
    n_wg = weight_workgroups(n_rows, d_in)
    if path == "narrow":
        return weight_k(path, n_rows, d_in)
    n_blocks = (n_rows + 31) // 32
    return -(-n_blocks // n_wg) * 8 + 3 + reduce_depth(n_wg)


def input_k(panel, d_out):
    return 9 if panel == "narrow" else d_out + 1


def bound(k, S):
    """k roundings of relative size 2^-24 each, with the second order: (1 + u)^k - 1 <= k u (1 + k u) while k u < 1."""
    return k * U32 * (1 + k * U32) * S


# ---- operands --------------------------------------------------------------------------------------------------------------------
def _ints(rng, shape):
    a = rng.integers(-3, 4, shape, dtype=np.int8)
    if a.size >= 7:
        a.reshape(-1)[rng.permutation(a.size)[:7]] = np.arange(-3, 4)          # every value present
    return a


def weight_inputs(n, d_in, d_out, seed):
    rng = np.random.default_rng(seed)
    return _ints(rng, (n, d_out)), _ints(rng, (n, d_in)), _ints(rng, (n, d_in))          # dM, LE, E


def input_inputs(n, d_in, d_out, seed):
    rng = np.random.default_rng(seed)
    return (_ints(rng, (n, d_out)), _ints(rng, (d_out, d_in)), _ints(rng, (d_out, d_in)), _ints(rng, (n, d_in)),
            _ints(rng, (n, d_in)))                                                                  # dM, W1, W2, LE, E


def _amax(a):
    return max(int(a.max()), -int(a.min())) if a.size else 0


def every_value_present(a):
    """Each of -3 .. 3 occurs (operands of fewer than seven elements excepted)."""
    return a.size < 7 or bool(np.bincount(a.reshape(-1).astype(np.int64) + 3, minlength=7).all())


def weight_bound(dM, LE, E):
    return dM.shape[0] * _amax(dM) * max(_amax(LE) + _amax(E), _amax(LE) * _amax(E))


def input_bound(dM, W1, W2, LE, E):
    return dM.shape[1] * _amax(dM) * max(_amax(W1), _amax(W2)) * (1 + max(_amax(E), _amax(LE)))


def _integral(*arrs):
    assert all(np.asarray(a).dtype.kind == "i" for a in arrs), "integer-valued data only"
    return [np.asarray(a).astype(np.float64) for a in arrs]


def exact_weight(dM, LE, E):
    """(gW1, gW2, gb1, gb2) float32 as every kernel must produce them bit for bit.  Asserts the 2^24 condition."""
    assert weight_bound(dM, LE, E) < 2 ** 24, f"{weight_bound(dM, LE, E)} is not below 2^24"
    m, le, e = _integral(dM, LE, E)
    gW1, gW2, gb2 = m.T @ (le + e), m.T @ (le * e), m.sum(0)
    return tuple(a.astype(np.float32) for a in (gW1, gW2, 2 * gb2, gb2))


def exact_input(dM, W1, W2, LE, E):
    """(dLE, dE) float32 as every kernel must produce them bit for bit.  Asserts the 2^24 condition."""
    assert input_bound(dM, W1, W2, LE, E) < 2 ** 24, f"{input_bound(dM, W1, W2, LE, E)} is not below 2^24"
    m, w1, w2, le, e = _integral(dM, W1, W2, LE, E)
    dS, dP = m @ w1, m @ w2
    return (dS + dP * e).astype(np.float32), (dS + dP * le).astype(np.float32)


def mixed_weight_inputs(n, d_in, d_out, seed):
    """Real-valued float32 CPU tensors: dM 1e-2..1e2 per element, LE per row and E per element 1e-2..1e2; every 97th row of dM zero."""
    g = torch.Generator().manual_seed(seed)
    dM = torch.randn((n, d_out), generator=g) * 0.3 * 10.0 ** (torch.rand((n, d_out), generator=g) * 4 - 2)
    LE = torch.randn((n, d_in), generator=g) * 0.5 * 10.0 ** (torch.rand((n, 1), generator=g) * 4 - 2)
    E = torch.randn((n, d_in), generator=g) * 0.5 * 10.0 ** (torch.rand((n, d_in), generator=g) * 4 - 2)
    dM[::97] = 0.0
    return dM, LE, E


def mixed_input_inputs(n, d_in, d_out, seed):
    g = torch.Generator().manual_seed(seed)
    dM, LE, E = mixed_weight_inputs(n, d_in, d_out, seed + 1)
    W1, W2 = (torch.randn((d_out, d_in), generator=g) * 0.1 * 10.0 ** (torch.rand((d_out, d_in), generator=g) * 2 - 1) for _ in range(2))
    return dM, W1, W2, LE, E


def fp64_weight(dM, LE, E):
    """float32 CPU tensors -> (gW [d_out, 2 d_in], S_W, gb2, S_b) in float64: the values and what their rounding error is measured
    against.  [LE+E | LE*E] is formed in float32, as the kernels form it."""
    SP = torch.cat((LE + E, LE * E), 1).double()
    m = dM.double()
    return m.T @ SP, m.abs().T @ SP.abs(), m.sum(0), m.abs().sum(0)


def fp64_input(dM, W1, W2, LE, E):
    """float32 CPU tensors -> (dLE, S_dLE, dE, S_dE) in float64."""
    m, w1, w2, le, e = (t.double() for t in (dM, W1, W2, LE, E))
    dS, dP = m @ w1, m @ w2
    aS, aP = m.abs() @ w1.abs(), m.abs() @ w2.abs()
    return dS + dP * e, aS + aP * e.abs(), dS + dP * le, aS + aP * le.abs()


# ---- layouts: where an operand lies in its guarded buffer (shared by the CPU test's path query and the GPU test) ------------------------
def weight_layout(c):
    """name -> (ld, col0) of dM, LE, E for a weight-gradient case.  padded: 16-byte aligned rows, leading dimensions multiples of 4
    beyond the width (all three differ), the padding holds NaN; odd_X: an odd leading dimension on X alone; offset: every leading
    dimension a multiple of 4, LE starts one float into its row."""
    def pad(d, extra):
        return (d + 3) // 4 * 4 + extra
    lay = {"dM": (pad(c.d_out, 4), 0), "LE": (pad(c.d_in, 8), 0), "E": (pad(c.d_in, 12), 0)}
    if c.layout.startswith("odd_"):
        name = c.layout[4:]
        ld = lay[name][0] + 1
        assert ld % 2 == 1
        lay[name] = (ld, 0)
    elif c.layout == "offset":
        lay["LE"] = (lay["LE"][0], 1)
    else:
        assert c.layout == "padded"
    return lay


def address(ld, col0, guard=GUARD_ROWS, base=A0):
    """The address of element (0, col0) of the view behind `guard` guard rows in a 256-byte aligned buffer."""
    return base + 4 * (guard * ld + col0)


def input_ldm(c):
    """dM of an input-gradient case: 16-byte aligned rows padded to a multiple of 4 floats (pad4) or of 32 as engine.backward.bwd_pre makes them."""
    q = 4 if c.ldm == "pad4" else 32
    return (c.d_out + q - 1) // q * q


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# weight gradient.  bias: which of gb1 / gb2 are passed (both | none | gb1 | gb2)
WCase = namedtuple("WCase", "path n d_in d_out layout bias seed")
_W = [
    # rows on the matrix-core kernel: one block; 33: two blocks, one workgroup (the buffer toggles once); 69, 96: three blocks on two
    # workgroups (uneven); 16 384: 256 workgroups x 2 blocks; 16 400: a third block for workgroup 0 only; 16 423: for 0 and 1, ragged
    ("mfma_aligned", 0, 5, 4, "padded", "both"),
    ("mfma_aligned", 1, 1, 1, "padded", "none"),
    ("mfma_aligned", 31, 3, 3, "padded", "gb1"),
    ("mfma_aligned", 32, 32, 33, "padded", "gb2"),
    ("mfma_aligned", 33, 31, 100, "padded", "both"),
    ("mfma_aligned", 33, 5, 1, "padded", "both"),
    ("mfma_aligned", 69, 33, 127, "padded", "both"),
    ("mfma_aligned", 69, 128, 4, "padded", "gb2"),
    ("mfma_aligned", 96, 65, 128, "padded", "none"),
    ("mfma_aligned", 16384, 127, 100, "padded", "gb1"),
    ("mfma_aligned", 16400, 32, 33, "padded", "both"),
    ("mfma_aligned", 16423, 128, 128, "padded", "both"),
    ("mfma_unaligned", 33, 33, 33, "odd_dM", "both"),
    ("mfma_unaligned", 69, 5, 100, "odd_LE", "gb2"),
    ("mfma_unaligned", 96, 128, 127, "odd_E", "both"),
    ("mfma_unaligned", 31, 65, 4, "offset", "none"),
    # the narrow kernel from 65 536 rows (32 rows per workgroup) up; one row below it the matrix cores
    ("narrow", 65536, 1, 1, "padded", "both"),
    ("narrow", 65536, 4, 128, "padded", "gb1"),
    ("narrow", 65536, 2, 100, "odd_dM", "both"),
    ("narrow", 65537, 2, 100, "padded", "none"),
    ("narrow", 65537, 3, 128, "padded", "both"),
    ("narrow", 65537, 1, 128, "odd_LE", "gb2"),
    ("narrow", 70001, 3, 100, "padded", "both"),
    ("narrow", 70001, 4, 1, "offset", "both"),
    ("mfma_aligned", 65535, 2, 100, "padded", "both"),
    ("mfma_unaligned", 65535, 2, 128, "odd_E", "gb2"),
]
WEIGHT_CASES = [WCase(*row, seed=100 + i) for i, row in enumerate(_W)]
WEIGHT_FP64 = [WCase("mfma_aligned", 16423, 65, 100, "padded", "both", 901), WCase("mfma_unaligned", 1000, 33, 65, "odd_LE", "both", 902),
               WCase("narrow", 70001, 3, 100, "padded", "both", 903)]
WRAPPER_CASES = [(300, 515, 200, 951), (333, 515, 200, 952)]          # engine.backward.bwd_weight: 2 x 5 blocks of at most 128 x 128

# input gradient.  panels: the kernel of every panel, in column order; ldm: pad4 | pad32; opts on top of DEFAULTS
ICase = namedtuple("ICase", "panels n d_in d_out ldm opts seed")
OFF = dict(bwd_input_resident=0)
_S, _T, _WD, _R, _N = "staged_small", "staged_tall", "staged_wide", "resident", "narrow"
_I = [
    ((_S,), 1, 1, 1, "pad4"), ((_S,), 31, 4, 3, "pad32"), ((_S,), 32, 100, 4, "pad4"), ((_S,), 33, 128, 5, "pad4"),
    ((_S, _WD), 69, 288, 31, "pad4"), ((_S,), 16384, 100, 32, "pad32"), ((_S, _WD), 33, 288, 200, "pad4"), ((_S,), 69, 128, 129, "pad32"),
    ((_S,), 33, 4, 2, "pad4"),
    ((_WD,), 1, 129, 33, "pad4"), ((_WD,), 127, 130, 65, "pad32"), ((_WD,), 128, 160, 100, "pad4"), ((_WD,), 129, 129, 128, "pad4"),
    ((_WD,), 261, 160, 129, "pad4"), ((_WD,), 16385, 130, 1, "pad32"),
    ((_T,), 16385, 1, 200, "pad4"), ((_T,), 16511, 100, 5, "pad32"), ((_T,), 16512, 128, 33, "pad4"), ((_T, _WD), 16517, 288, 4, "pad4"),
    ((_T,), 131071, 4, 32, "pad4"), ((_T,), 131072, 100, 3, "pad32"), ((_T,), 131072, 4, 129, "pad4"),
    ((_T,), 131073, 128, 65, "pad32", OFF),
    ((_N,), 131072, 4, 65, "pad32"), ((_R,), 131105, 128, 4, "pad4"), ((_R, _N), 131072, 129, 5, "pad32"),
    ((_R, _N), 131105, 130, 64, "pad4"), ((_R, _N), 131072, 131, 128, "pad4"), ((_R, _N), 196609, 132, 4, "pad32"),
    ((_R, _R), 131072, 133, 65, "pad4"), ((_R, _R, _N), 131072, 260, 5, "pad4"),
]
INPUT_CASES = [ICase(*(row if len(row) == 6 else row + ({},)), seed=500 + i) for i, row in enumerate(_I)]
INPUT_FP64 = [ICase((_S,), 333, 100, 65, "pad32", {}, 911), ICase((_WD,), 261, 130, 100, "pad4", {}, 912),
              ICase((_T,), 16517, 128, 33, "pad4", {}, 913), ICase((_R, _N), 131105, 130, 65, "pad32", {}, 914)]
WEIGHT_PATHS = ("mfma_aligned", "mfma_unaligned", "narrow")
INPUT_PATHS = (_S, _T, _WD, _R, _N)
PANEL_COLS = {_S: 128, _T: 128, _WD: 160, _R: 128}                       # narrow: the 1..4 columns left


def wcase_id(c):
    return f"{c.path}-{c.n}x{c.d_in}to{c.d_out}-{c.layout}-{c.bias}"


def icase_id(c):
    return f"{'+'.join(c.panels)}-{c.n}x{c.d_in}to{c.d_out}-{c.ldm}" + ("-resident_off" if c.opts else "")


def panel_of_column(c):
    """The kernel name of every input column of a case: [d_in] list."""
    out, col0 = [], 0
    for p in c.panels:
        w = min(PANEL_COLS.get(p, 4), c.d_in - col0)
        out += [p] * w
        col0 += PANEL_COLS.get(p, w)
    assert len(out) == c.d_in, (c, len(out))
    return out


def query_weight_path(lib, c):
    """(name, n_workgroups) from ngcf_layer_bwd_weight_path for the case's sizes and the alignment of its layout (host code)."""
    import ctypes
    lay = weight_layout(c)
    n_wg = ctypes.c_int(-1)
    got = lib.ngcf_layer_bwd_weight_path(c.n, c.d_in, c.d_out, address(*lay["dM"]), lay["dM"][0], address(*lay["LE"], base=A0 + (1 << 32)),
                                         lay["LE"][0], address(*lay["E"], base=A0 + (2 << 32)), lay["E"][0], ctypes.byref(n_wg))
    return (None if got is None else got.decode()), n_wg.value


def query_input_panels(lib, n, d_in, d_out):
    """The names and widths of the panels ngcf_layer_bwd_input_path walks from column 0 (host code)."""
    import ctypes
    names, col0 = [], 0
    while col0 < d_in:
        w = ctypes.c_int(-1)
        got = lib.ngcf_layer_bwd_input_path(n, d_in, d_out, col0, ctypes.byref(w))
        assert got is not None and w.value > 0, (n, d_in, d_out, col0)
        names.append((got.decode(), w.value))
        col0 += w.value
    return names


def expected_panels(c):
    out, col0 = [], 0
    for p in c.panels:
        w = PANEL_COLS.get(p, c.d_in - col0)
        out.append((p, w))
        col0 += w
    return out
