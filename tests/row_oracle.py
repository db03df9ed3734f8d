"""References and input builders for the direct tests of the backward's row kernels (tests/test_row_kernels_gpu.py), in plain numpy /
CPU torch, written from the statements in include/ngcf_hip.h and the kernels' comments - no code shared with the product, and
nothing here runs on a GPU.  tests/test_row_oracle.py checks these helpers, and the inputs they build, on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

# ---- ngcf_segment_sum_rows_f32 ---------------------------------------------------------------------------------------------------
# one call must hold all of these segment lengths (below / at / above 4, 16 and 64, a tail after full blocks, several blocks)
SEG_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 19, 20, 63, 64, 65, 67, 68, 70, 83, 128, 131, 200)


def segment_sum_chains(g, order, segptr):
    """The documented order of the gather backward, emulated in float32: position k of a segment (counted from its start) goes to
    chain k % 4 while k < n4 = len // 4 * 4, in ascending k; the positions from n4 on go to chain 0; the result is
    (s0 + s1) + (s2 + s3).  An empty segment gives zeros.  Only float32 additions: the kernel must give the same bits."""
    g = np.asarray(g, dtype=np.float32)
    order, segptr = np.asarray(order, dtype=np.int64), np.asarray(segptr, dtype=np.int64)
    out = np.zeros((len(segptr) - 1, g.shape[1]), dtype=np.float32)
    for r in range(len(segptr) - 1):
        rows = g[order[segptr[r]:segptr[r + 1]]]
        n4 = len(rows) // 4 * 4
        s = np.zeros((4, g.shape[1]), dtype=np.float32)
        for k in range(n4):
            s[k % 4] = s[k % 4] + rows[k]
        for k in range(n4, len(rows)):
            s[0] = s[0] + rows[k]
        out[r] = (s[0] + s[1]) + (s[2] + s[3])
    return out


def segment_sum_f64(g, order, segptr):
    """(sum, bound) per segment and column in float64: the exact sum of the float32 inputs and the bound len * 2^-24 * sum|g| that any
    order of len - 1 rounded float32 additions stays within (each addition errs by at most 2^-24 of a partial sum <= sum|g|)."""
    g = np.asarray(g, dtype=np.float64)
    n_seg = len(segptr) - 1
    total, bound = np.zeros((n_seg, g.shape[1])), np.zeros((n_seg, g.shape[1]))
    for r in range(n_seg):
        rows = g[np.asarray(order[segptr[r]:segptr[r + 1]], dtype=np.int64)]
        total[r] = rows.sum(0)
        bound[r] = len(rows) * 2.0 ** -24 * np.abs(rows).sum(0)
    return total, bound


def segment_case(d, seed):
    """g [M, d] float32, order (a random permutation of the M gradient rows) and segptr for SEG_LENGTHS in a shuffled order."""
    rng = np.random.default_rng(seed)
    lengths = rng.permutation(np.asarray(SEG_LENGTHS, dtype=np.int64))
    segptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    M = int(segptr[-1])
    g = rng.standard_normal((M, d)).astype(np.float32)
    return g, rng.permutation(M).astype(np.int64), segptr


# ---- BPR (bprloss.py:15-22) ------------------------------------------------------------------------------------------------------
BPR_R = (1, 3, 4, 5, 1023, 1025, 1029)
BPR_D = (1, 63, 64, 65, 260)
# every R at D = 65, every D at R = 5 and R = 1029
BPR_SHAPES = sorted({(R, 65) for R in BPR_R} | {(R, D) for R in (5, 1029) for D in BPR_D})
BPR_BROADCAST = ("u", "p", "n", "pn")          # the operands with ONE row, at R = 1029, D = 65


def bpr_inputs(R, D, seed, broadcast=""):
    """float32 u, p, n ([R, D], or [1, D] for the operands named in `broadcast`) whose scores x = |u.p| - |u.n| are spread over
    [-120, 120] in one batch: beyond +-90 (expf over- and underflows), and near 0.  Random rows are corrected along the other operand
    so that u.p and u.n hit their targets: the dot products keep cancelling terms but stay far from 0, where d|t|/dt jumps.  With
    all operands full and R >= 3, row 1 of u is all zero (both signs 0) and row 2 of p is all zero against a non-zero n."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-120.0, 120.0, R) if R > 1 else np.array([-120.0])
    x = x[rng.permutation(R)]
    base = rng.uniform(0.5, 3.0, R)
    tp = (base + np.maximum(x, 0.0)) * rng.choice([-1.0, 1.0], R)          # targets of u.p and u.n, either sign
    tn = (base + np.maximum(-x, 0.0)) * rng.choice([-1.0, 1.0], R)

    def draw(rows, scale):     # no entry near zero: at D = 1 the correction divides by it
        z = rng.standard_normal((rows, D))
        return np.sign(z) * (0.5 + np.abs(z)) * scale / np.sqrt(D)
    u = draw(1 if "u" in broadcast else R, 3.0)
    p = draw(1 if "p" in broadcast else R, 1.5)
    n = draw(1 if "n" in broadcast else R, 1.5)
    dot = lambda a, b: (a * b).sum(1)  # noqa: E731
    if "p" in broadcast and "n" in broadcast:                               # u.p = tp and u.n = tn: a step inside span(p, n)
        gram = np.array([[dot(p, p)[0], dot(p, n)[0]], [dot(p, n)[0], dot(n, n)[0]]])
        ab = np.linalg.solve(gram, np.stack([tp - dot(u, p), tn - dot(u, n)]))
        u = u + ab[0][:, None] * p + ab[1][:, None] * n
    elif "p" in broadcast:
        u = u + ((tp - dot(u, p)) / dot(p, p))[:, None] * p
    elif "n" in broadcast:
        u = u + ((tn - dot(u, n)) / dot(n, n))[:, None] * n
    if "p" not in broadcast:
        p = p + ((tp - dot(u, p)) / dot(u, u))[:, None] * u
    if "n" not in broadcast:
        n = n + ((tn - dot(u, n)) / dot(u, u))[:, None] * u
    if not broadcast and R >= 3:
        u[1] = 0.0
        p[2] = 0.0
    return tuple(torch.from_numpy(t.astype(np.float32)) for t in (u, p, n))


def bpr_scores(u, p, n):
    """(u.p, u.n, margin) in float64 of the float32 inputs; margin = the smallest |dot| / sum_j |a_j b_j| over the dot products that
    are not exactly 0.  The reference is unambiguous (no score at the kink of |t|) when margin >= 1e-3."""
    u, p, n = (t.double() for t in (u, p, n))
    margin = np.inf
    dots = []
    for b in (p, n):
        prod = u * b
        dot, mag = prod.sum(1), prod.abs().sum(1)
        nz = dot != 0
        if bool(nz.any()):
            margin = min(margin, float((dot[nz].abs() / mag[nz]).min()))
        dots.append(dot)
    return dots[0], dots[1], margin


# ---- ngcf_layer_bwd_pre_f32 (NGCF.py:140-144) ------------------------------------------------------------------------------------
PRE_ROWS = (1, 5, 1001)
PRE_D = (1, 2, 63, 64, 65, 128, 130, 258, 515)


def pre_inputs(n_rows, d, seed, drop_p=0.0, zero_row=None):
    """float32 M (no entry within 1e-2 of the kink of LeakyReLU; row `zero_row` all zero), dN, dC and the dropout noise tensor
    (0 or 1/(1-p); all ones at drop_p = 0)."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn((n_rows, d), generator=gen)
    M = torch.where(z < 0, -1.0, 1.0) * (0.01 + 0.4 * z.abs())
    if zero_row is not None:
        M[zero_row] = 0.0
    dN, dC = torch.randn((n_rows, d), generator=gen), torch.randn((n_rows, d), generator=gen)
    mask = torch.ones((n_rows, d))
    if drop_p > 0:
        mask = (torch.rand((n_rows, d), generator=gen) >= drop_p).float() / (1.0 - drop_p)
    return M, dN, dC, mask


def pre_reference(M, mask, dN, dC, leaky):
    """(C, dM) in float64: C = leaky_relu(M) * mask, N = normalize(C), dM = d/dM of (N.dN).sum() + (C.dC).sum() by autograd;
    dN or dC may be None."""
    M = M.double().requires_grad_(True)
    C = F.leaky_relu(M, leaky) * mask.double()
    N = F.normalize(C, p=2, dim=1, eps=1e-12)
    loss = 0.0
    if dN is not None:
        loss = loss + (N * dN.double()).sum()
    if dC is not None:
        loss = loss + (C * dC.double()).sum()
    loss.backward()
    return C.detach(), M.grad
