"""Host oracle of the dense half of a layer (NGCF.py:131-146) as include/ngcf_hip.h defines it, in numpy / CPU torch, written from the
header and the comments of csrc/dense*.hip, csrc/dense_device.h and csrc/common.h - no code shared with the product, nothing here runs on a GPU.
tests/test_dense_oracle.py checks it on the CPU; tests/test_dense_paths_gpu.py holds every forward kernel to it and
tests/test_dense_split_gpu.py imports the fp64 form's bounds.

    A = [LE+E | LE*E],  B = [W1^T ; W2^T],  M = A.B + ((b1 + b1) + b2)
    carry = dropout(leaky_relu(M, 0.2)),  norm = carry / max(||carry||, 1e-12)

EXACT form (`exact_layer`).  All of LE, E, W1, W2, b1, b2 hold small integers, so every product and every partial sum of an output
element is an integer of magnitude at most |A|.|B| + |bias|, asserted to be below 2^24 for each case: such a sum is the same in
any order, with or without fma, in fp32 or through the three bf16 parts of the split kernel (an integer up to 255 is one bf16, the
other two parts are zero).  Every kernel must therefore produce the integer M exactly, and what follows is restated operation by
operation in float32: v >= 0 ? v : 0.2f * v (one rounding), then the keep scale float32(1) / (float32(1) - float32(p)) (the
subtraction is exact for p = 0.3, the division correctly rounded) or the host mask's own value, multiplied in (one rounding).  No
tolerance: `carry` must equal this bit for bit.

fp64 form (`fp64_layer`, `carry_k`, `norm_k`): for real-valued inputs and for the normalised block; errors are measured against
scale = |A|.|B| + |bias| in units of 2^-24.

Hash mask (`msg_keep`): element (row, col) is dropped iff uint32(fmix64(seed ^ (row * 0x9E3779B97F4A7C15 + col))) is below
uint32(double(float32(p)) * 2^32)."""
import math
from collections import namedtuple

import numpy as np
import torch

from dropout_oracle import GOLDEN, M64, _fmix64, drop_threshold

U32 = 2.0 ** -24            # fp32 unit roundoff (round to nearest)
LEAKY = np.float32(0.2)     # the slope the wrappers pass (a C float)
DROP_P = 0.3


# ---- fp64 form: bounds and error measures ----------------------------------------------------------------------------------------
def carry_k(d_in):
    """Bound on |carry - act| in units of 2^-24 * scale, scale = |A|.|B| + |bias| (A = [LE+E | LE*E] formed in fp32 as the kernel
    forms it, so A itself carries no error; B = [W1^T ; W2^T]).

    - Split: x = h + m + l EXACTLY for every fp32 operand (h = bf16(x) leaves a residual of at most 16 significant bits, m = bf16 of
      that one of at most 8, which l holds exactly), |h| + |m| + |l| <= (1 + 2^-7)|x|.
    - Dropped cross terms m.l, l.m, l.l: |m| <= 2^-8 (1 + 2^-8)|x|, |l| <= 2^-16 |x|, so at most (2 (1 + 2^-8) + 2^-8) 2^-24 |a||b|
      per product: 2.01 in all.
    - Accumulation: one fp32 accumulator per output element, six exact bf16 x bf16 products per real k (2 d_in of them: d_in sums
      against W1, d_in products against W2; the zero columns past d_in add exact zeros).  Nothing is assumed about the order or
      width of the MFMA's internal adder: every addition counts as one rounding, at most 12 d_in of them, each <= 2^-24 times a
      partial sum <= (1 + 2^-7)^2 scale: 12.2 d_in, 12.5 d_in with the second-order terms.
    - Epilogue: bias2 = (b1 + b1) + b2 (1 rounding, <= |bias|), acc + bias2 (1), LeakyReLU 0.2f * v (0.2f is 0.2 (1 + 2^-26),
      + 1 rounding: 1.25), dropout keep scale fp32(1 / (1 - 0.3f)) or the host mask's fp32 1/0.7 (<= 2.3) times v (1): 3.3; the
      dropout's 1/0.7 also scales `scale`.  7.6 in all.
    k = 12.5 d_in + 2.01 + 7.6 <= 12.5 d_in + 10."""
    return 12.5 * d_in + 10


def norm_k(d_in, d_out):
    """Bound on ||act|| * |norm - act/||act||| in units of 2^-24 * S, S = max over the row of scale.  The kernel's 1/||v||: sum of
    squares in 9 roundings of non-negative terms (4 fmaf per lane, 5 shuffle adds), sqrtf (halves that, + 1), 1/x (1), v * inv
    (1): 7.5 (+ 0.5 second order).  To first order ||act|| |n_j - a_j/||act||| <= |v_j - act_j| + |a_j/||act||| ||v - act|| +
    8 u |act_j|, with |v_j - act_j| <= carry_k u scale_j, ||v - act|| <= carry_k u sqrt(d_out) S and |act_j| <= S:
    k = carry_k (1 + sqrt(d_out)) + 8."""
    return carry_k(d_in) * (1 + math.sqrt(d_out)) + 8


class Fp64Layer:
    """The layer in float64 from CPU tensors and the error measures against it: `act` the activated (and dropped) values, `scale`
    what the rounding error of the product is measured against, `nrm` the normalised rows."""

    def __init__(self, act, scale):
        self.act, self.scale = act, scale
        self.rn = act.norm(dim=1, keepdim=True)
        self.nrm = act / self.rn.clamp_min(1e-12)
        self.S = scale.amax(dim=1, keepdim=True)

    def err_carry(self, c):
        """max |c - act| / scale."""
        return float(((c.double() - self.act).abs() / (self.scale + 1e-300)).max())

    def err_norm(self, nb):
        """max ||act|| |nb - act / ||act||| / S."""
        return float(((nb.double() - self.nrm).abs() * self.rn.clamp_min(1e-12) / (self.S + 1e-300)).max())


def fp64_layer(le, e, W1, b1, W2, b2, keep=None, keep_div=0.7):
    """le, e [R, d_in], W1, W2 [d_out, d_in], b1, b2 [d_out] float32 CPU tensors; keep: the keep pattern [R, d_out] (bool or 0 / 1)
    or None; a kept element is divided by keep_div = 1 - p."""
    A = torch.cat((le + e, le * e), 1).double()          # the operands as the kernels form them (fp32 sums and products)
    B = torch.cat((W1.T, W2.T), 0).double()
    bias = (b1 + b1 + b2).double()
    pre = A @ B + bias
    scale = A.abs() @ B.abs() + bias.abs()               # what the rounding error of the product is measured against
    act = torch.where(pre >= 0, pre, 0.2 * pre)
    if keep is not None:
        act = act * keep.double() / keep_div
        scale = scale * keep.double() / keep_div
    return Fp64Layer(act, scale)


# ---- hash mask -------------------------------------------------------------------------------------------------------------------
def msg_hash(seed, rows, cols):
    """uint32(fmix64(seed ^ (row * golden + col))) for every (row, col) pair: [len(rows), len(cols)] uint64 values below 2^32."""
    r = np.atleast_1d(np.asarray(rows)).astype(np.uint64)[:, None]
    c = np.atleast_1d(np.asarray(cols)).astype(np.uint64)[None, :]
    s = np.full((1, 1), int(seed) & M64, dtype=np.uint64)
    return _fmix64(s ^ (r * GOLDEN + c)) & np.uint64(0xFFFFFFFF)


def msg_keep(seed, rows, cols, p):
    """Which elements message dropout keeps: [len(rows), len(cols)] bool, kept iff the hash is >= uint32(double(float32(p)) * 2^32)."""
    return msg_hash(seed, rows, cols) >= np.uint64(drop_threshold(p))


def keep_scale(p):
    """1 / (1 - p) as the kernels form it: in float32 from the float32 p."""
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p) if p > 0 else np.float32(1.0)


# ---- exact form ------------------------------------------------------------------------------------------------------------------
def exact_inputs(n, d_in, d_out, seed, zero_bias=False, zero_rows=()):
    """Integer-valued inputs (int64 arrays): LE, E in -3..3, W1, W2 in -2..2, b1, b2 in -4..4 (zeros with zero_bias); the rows
    `zero_rows` of LE and E are zero."""
    rng = np.random.default_rng(seed)
    LE, E = rng.integers(-3, 4, (n, d_in)), rng.integers(-3, 4, (n, d_in))
    W1, W2 = rng.integers(-2, 3, (d_out, d_in)), rng.integers(-2, 3, (d_out, d_in))
    b1, b2 = rng.integers(-4, 5, d_out), rng.integers(-4, 5, d_out)
    if zero_bias:
        b1, b2 = np.zeros_like(b1), np.zeros_like(b2)
    for r in zero_rows:
        LE[r], E[r] = 0, 0
    return LE, E, W1, b1, W2, b2


def exact_layer(LE, E, W1, b1, W2, b2, p=0.0, keep=None, mask=None):
    """(carry, M, scale): carry float32 [n, d_out] as every kernel must produce it bit for bit, M the int64 pre-activation and
    scale = |A|.|B| + |bias| (float64; times the keep factor).  keep [n, d_out] bool with p: hash dropout; mask [n, d_out] float32:
    the host noise tensor, whose own value is multiplied in.  Asserts the 2^24 condition."""
    arrs = [np.asarray(a) for a in (LE, E, W1, b1, W2, b2)]
    assert all(np.array_equal(a, np.rint(a)) for a in arrs), "integer-valued data only"
    LE, E, W1, b1, W2, b2 = (a.astype(np.int64) for a in arrs)
    A = np.concatenate((LE + E, LE * E), 1).astype(np.float64)        # float64 products of integers this small are exact
    B = np.concatenate((W1.T, W2.T), 0).astype(np.float64)
    bias = (2 * b1 + b2).astype(np.float64)
    bound = np.abs(A) @ np.abs(B) + np.abs(bias)
    assert bound.max() < 2 ** 24, f"|A|.|B| + |bias| = {bound.max()} is not below 2^24"
    M = A @ B + bias
    assert np.array_equal(M, np.rint(M))
    v = M.astype(np.float32)
    v = np.where(v >= 0, v, LEAKY * v).astype(np.float32)
    scale = bound
    if mask is not None:
        mask = np.asarray(mask, dtype=np.float32)
        v = (v * mask).astype(np.float32)
        scale = bound * mask.astype(np.float64)
    elif keep is not None and p > 0:
        ks = keep_scale(p)
        v = np.where(keep, (v * ks).astype(np.float32), np.float32(0.0)).astype(np.float32)
        scale = bound * np.where(keep, float(ks), 0.0)
    assert v.dtype == np.float32
    return v, M.astype(np.int64), scale


def norm_error(norm, carry, scale):
    """max ||act|| |norm - act / ||act||| / S in units of 2^-24 (act = the exact carry in float64), and the rows of act that are
    all zero."""
    ref = Fp64Layer(torch.from_numpy(np.asarray(carry, dtype=np.float64)), torch.from_numpy(np.asarray(scale, dtype=np.float64)))
    return ref.err_norm(torch.as_tensor(norm)) / U32, (ref.rn[:, 0] == 0).numpy()


# ---- real-valued inputs of the fp64 cases ----------------------------------------------------------------------------------------
def mixed_inputs(n, d_in, d_out, seed):
    """Random real-valued inputs with mixed magnitudes (float32 CPU tensors): 1e-3..1e3 per row of LE and per element of E, 0.1..10
    per element of W1, every 97th row of LE and E zero, zero biases (a zero row gives a zero output row, normalised to zeros)."""
    g = torch.Generator().manual_seed(seed)
    LE = torch.randn((n, d_in), generator=g) * 0.5
    E = torch.randn((n, d_in), generator=g) * 0.5
    W1, W2 = (torch.randn((d_out, d_in), generator=g) * 0.1 for _ in range(2))
    LE *= 10.0 ** (torch.rand((n, 1), generator=g) * 6 - 3)
    E *= 10.0 ** (torch.rand((n, d_in), generator=g) * 6 - 3)
    W1 *= 10.0 ** (torch.rand((d_out, d_in), generator=g) * 2 - 1)
    LE[::97] = 0.0
    E[::97] = 0.0
    return LE, E, W1, torch.zeros(d_out), W2, torch.zeros(d_out)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# mode: eval | hash_hi (p = 0.3, a seed >= 2^63) | hash0 (p = 0.3, seed 0) | mask (host noise tensor) | last (eval, no carry)
# layout: padded (16-byte aligned rows, leading dimension a multiple of 4 beyond d_in, NaN in the padding) | odd (odd leading
#         dimension, the view starts at column 1) | tight (d_in < 4 in 16-byte aligned rows of 4 floats)
# special: zero biases and a few all-zero rows of LE and E
Case = namedtuple("Case", "path opts n d_in d_out mode layout special seed")
MODES = ("eval", "hash_hi", "hash0", "mask", "last")
SEED_HI = 0xC2B2AE3D27D4EB4F          # >= 2^63; its top 16 bits are not the tag of a seed behind a pointer
HASH_SEED = {"hash_hi": SEED_HI, "hash0": 0}

SMALL_OFF = dict(dense_small_tiles=0)
WIDE_STAGED = dict(dense_direct=0, dense_tall=0)
DIRECT = dict(dense_direct=2, dense_tall=0)
TALL = dict(dense_tall=2)
RESIDENT = dict(dense_resident=1, dense_resident_min_rows=1)
SPLIT = dict(dense_resident=4, dense_resident_min_rows=1)

# path -> (options, row tile T, d_out: (padded width, one below, one above the previous step, extras..),
#          d_in: (a multiple of 16, a multiple of 4 that is none of 16, neither, extras..))
PADDED_PATHS = {
    "staged<1,4,1>/padded": ({}, 32, (128, 127, 1, 33, 65), (16, 4, 17)),
    "staged<4,1,1>/padded": (SMALL_OFF, 128, (32, 31, 1), (16, 4, 15)),
    "staged<4,1,2>/padded": (SMALL_OFF, 128, (64, 63, 33), (16, 20, 65)),
    "staged<4,1,3>/padded": (SMALL_OFF, 128, (96, 95, 65), (48, 12, 130)),
    "staged<4,1,4>/padded": (SMALL_OFF, 128, (128, 127, 97), (144, 4, 130)),
    "staged<2,2,4>/padded": (WIDE_STAGED, 64, (256, 255, 129, 200), (16, 20, 130)),
    "staged<1,4,4>/padded": (WIDE_STAGED, 32, (512, 511, 257), (16, 4, 515)),
    "direct<2,4>": (DIRECT, 32, (256, 255, 129, 200), (16, 132, 65)),
    "direct<4,4>": (DIRECT, 32, (512, 511, 257), (16, 4, 515)),
    "tall256": (TALL, 96, (256, 255, 129, 200), (32, 20, 130)),
    "tall512": (TALL, 96, (512, 511, 257), (16, 4, 515)),
    "resident": (RESIDENT, 32, (128, 127, 97, 1), (144, 4, 17, 130)),
    "split": (SPLIT, 32, (128, 127, 97, 1), (16, 132, 65, 144)),
}
STAGED_CONFIGS = [p[:-len("/padded")] for p in PADDED_PATHS if p.startswith("staged")]


def _padded_cases(path, k):
    """Seven cases and one per extra width: every row count 1, T-1, T, T+1, 2T+5, every mode, the three d_out and the three d_in;
    the full-tile epilogue arm (d_out = the padded width on T rows or more) in eval, hash, mask and no-carry mode, the guarded
    arm (a partial last tile, or d_out below the padded width) in eval, hash and mask mode."""
    opts, T, do, di = PADDED_PATHS[path]
    P, P1, Q = do[:3]
    a, b, c = di[:3]
    rows = [(1, P1, c, "eval", False), (T - 1, Q, a, "hash_hi", False), (T, P, b, "mask", False), (T + 1, P, c, "hash0", False),
            (2 * T + 5, P, a, "last", False), (2 * T + 5, P1, b, "mask", False), (T, P, a, "eval", True)]
    for j, d_out in enumerate(do[3:]):
        rows.append((T + 1, d_out, di[j % 3], MODES[(j + 1) % 4], False))
    for j, d_in in enumerate(di[3:]):
        rows.append((T + 1, P, d_in, MODES[(j + 2) % 4], False))
    return [Case(path, opts, n, d_in, d_out, mode, "padded", special, 1000 * k + i)
            for i, (n, d_out, d_in, mode, special) in enumerate(rows)]


def _staged_layout_cases(cfg, k):
    """The unaligned and the aligned-but-narrower-than-4 instantiations of one staged tile configuration."""
    opts, T, do, di = PADDED_PATHS[cfg + "/padded"]
    P, P1, Q = do[:3]
    a, b, c = di[:3]
    un, al = cfg + "/unaligned", cfg + "/aligned"
    narrow = 1 if k % 2 else 3                      # d_in = 1 and 3 alternate between the configurations
    rows = [(un, T + 1, P, c, "hash_hi", "odd"), (un, 1, P1, a, "mask", "odd"), (un, 2 * T + 5, Q, 4 - narrow, "eval", "odd"),
            (un, T - 1, P, b, "last", "odd"), (un, T, P, a, "hash0", "odd"),
            (al, T + 1, P, 3, "hash0", "tight"), (al, 2 * T + 5, P1, narrow, "mask", "tight")]
    return [Case(path, opts, n, d_in, d_out, mode, layout, False, 1000 * k + 500 + i)
            for i, (path, n, d_out, d_in, mode, layout) in enumerate(rows)]


def _cases():
    out = {"staged": [], "direct": [], "tall": [], "resident": [], "split": []}
    for k, path in enumerate(PADDED_PATHS):
        out[path.split("<")[0].rstrip("0123456789")] += _padded_cases(path, k)
        if path.startswith("staged"):
            out["staged"] += _staged_layout_cases(path[:-len("/padded")], k)
    # 145 input columns are ten chunks of weights, more than the resident and split kernels hold in LDS: the staged kernel runs
    for j, opts in enumerate((RESIDENT, SPLIT)):
        out["staged"].append(Case("staged<1,4,1>/padded", opts, 33, 145, 128, ("hash_hi", "eval")[j], "padded", False, 90000 + j))
    return out


CASES = _cases()
ALL_CASES = [c for fam in CASES.values() for c in fam]
# one real-valued case per path: (path, options, rows, d_in, d_out, mode, layout); rows 0, 97, .. are zero rows
FP64_CASES = ([(p, o, 2 * T + 5, di[2], do[i % 2], MODES[i % 4], "padded") for i, (p, (o, T, do, di)) in enumerate(PADDED_PATHS.items())]
              + [(cfg + "/unaligned", PADDED_PATHS[cfg + "/padded"][0], PADDED_PATHS[cfg + "/padded"][1] + 1,
                  PADDED_PATHS[cfg + "/padded"][3][2], PADDED_PATHS[cfg + "/padded"][2][1], MODES[i % 4], "odd")
                 for i, cfg in enumerate(STAGED_CONFIGS)]
              + [(cfg + "/aligned", PADDED_PATHS[cfg + "/padded"][0], PADDED_PATHS[cfg + "/padded"][1] + 1, 3,
                  PADDED_PATHS[cfg + "/padded"][2][0], MODES[(i + 2) % 4], "tight") for i, cfg in enumerate(STAGED_CONFIGS)])


def case_id(c):
    return f"{c.path}-{c.n}x{c.d_in}to{c.d_out}-{c.mode}-{c.layout}" + ("-zeros" if getattr(c, "special", False) else "") + (
        "-" + "+".join(f"{k.replace('dense_', '')}{v}" for k, v in c.opts.items()) if c.path.startswith("staged<1,4,1>") and c.opts else "")


def zero_rows_of(c):
    """The all-zero rows of LE and E in a special case: the first, the last and one in the middle of the first tile."""
    return tuple(sorted({0, min(5, c.n - 1), c.n - 1})) if c.special else ()


def case_inputs(c):
    """(LE, E, W1, b1, W2, b2) int64 arrays, keep [n, d_out] bool or None, mask [n, d_out] float32 or None."""
    ins = exact_inputs(c.n, c.d_in, c.d_out, c.seed, zero_bias=c.special, zero_rows=zero_rows_of(c))
    keep = mask = None
    if c.mode in HASH_SEED:
        keep = msg_keep(HASH_SEED[c.mode], np.arange(c.n), np.arange(c.d_out), DROP_P)
    elif c.mode == "mask":
        g = torch.Generator().manual_seed(c.seed)
        mask = ((torch.rand((c.n, c.d_out), generator=g) > DROP_P).float() / 0.7).numpy()     # nn.Dropout's noise: 0 or fp32 1 / 0.7
    return ins, keep, mask


def case_expected(c):
    """(inputs, keep, mask, carry float32, M int64, scale float64) of an exact case."""
    ins, keep, mask = case_inputs(c)
    carry, M, scale = exact_layer(*ins, p=DROP_P if keep is not None else 0.0, keep=keep, mask=mask)
    return ins, keep, mask, carry, M, scale
