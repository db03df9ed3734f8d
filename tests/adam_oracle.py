"""The Adam step of csrc/adam.hip restated on the host, operation by operation (the recipe is in include/ngcf_hip.h, section "Adam
step"): float32 arrays, float64 scalars, the same double-double square-and-multiply for beta^t.  numpy rounds every float32 operation
once and contracts nothing, and Python's floats are IEEE doubles, so this file computes the bits the kernel must give."""
import numpy as np

F = np.float32
SPLIT = 134217729.0        # 2^27 + 1


def dd_mul(a, b):
    """(hi, lo) * (hi, lo) in double-double; the product's rounding error by Veltkamp's split, as in the header."""
    a_hi, a_lo = a
    b_hi, b_lo = b
    p = a_hi * b_hi
    c = SPLIT * a_hi
    ah = c - (c - a_hi)
    al = a_hi - ah
    c = SPLIT * b_hi
    bh = c - (c - b_hi)
    bl = b_hi - bh
    e = (((ah * bh - p) + ah * bl) + al * bh) + al * bl
    e = e + (a_hi * b_lo + a_lo * b_hi)
    hi = p + e
    return hi, e - (hi - p)


def beta_pow(beta: float, t: int) -> float:
    """beta^t by square-and-multiply on the integer t."""
    r, b, e = (1.0, 0.0), (float(beta), 0.0), int(t)
    while e > 0:
        if e & 1:
            r = dd_mul(r, b)
        e >>= 1
        if e > 0:
            b = dd_mul(b, b)
    return r[0]


def scalars(step: float, lr, beta1, beta2, eps, weight_decay):
    """(step_size, bc2s, c1, beta2, c2, eps, wd), each rounded to float32 once, for the step that follows `step` steps."""
    t = int(F(step) + F(1.0))
    with np.errstate(divide="ignore"):
        bc1 = 1.0 - beta_pow(beta1, t)
        step_size = -(np.float64(lr) / np.float64(bc1))
    bc2s = np.sqrt(np.float64(1.0 - beta_pow(beta2, t)))
    return F(step_size), F(bc2s), F(1.0 - beta1), F(beta2), F(1.0 - beta2), F(eps), F(weight_decay)


def adam_step(p, g, m, v, step, *, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False):
    """(p, g, m, v, step) -> (p, m, v, step): new arrays, the inputs are left alone.  `step` is the float32 count of steps so far."""
    p, g, m, v = (np.array(x, dtype=F, copy=True) for x in (p, g, m, v))
    step_size, bc2s, c1, b2, c2, eps32, wd = scalars(step, lr, betas[0], betas[1], eps, weight_decay)
    with np.errstate(all="ignore"):
        if maximize:
            g = -g
        if wd != 0:
            g = g + wd * p
        m = m + c1 * (g - m)
        v = v * b2 + (c2 * g) * g
        d = np.sqrt(v) / bc2s + eps32
        p = p + step_size * (m / d)
    assert p.dtype == F and m.dtype == F and v.dtype == F
    return p, m, v, F(step) + F(1.0)


def ulp_distance(a, b):
    """Element-wise distance of two float32 arrays in units in the last place: the difference of their positions on the ordered line
    of float32 values (so +0 and -0 are 0 apart).  NaN against NaN is 0, NaN against a number 2^32."""
    def line(x):
        i = np.ascontiguousarray(x, dtype=F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    d = np.abs(line(a) - line(b))
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.where(nan_a & nan_b, 0, np.where(nan_a | nan_b, 2 ** 32, d))


# ---- the one-step distance to torch's Adam on the device (tests/test_adam_gpu.py holds it, tools/adam_lab.py measures it) ----------
HELD_SHAPES = ((65, 65), (600, 65))
HELD_STEPS = 50
HELD_KW = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False)


def ulp_distance_torch(a, b):
    """`ulp_distance` for float32 tensors on any device (int64 result; NaN against NaN 0, NaN against a number 2^32)."""
    import torch

    def line(x):
        i = x.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = (line(a) - line(b)).abs()
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    return torch.where(nan_a & nan_b, torch.zeros_like(d), torch.where(nan_a | nan_b, torch.full_like(d, 2 ** 32), d))


def distance_to_torch(adam_step, new_ticket, dev, capturable, steps=HELD_STEPS, seed=2024):
    """Max distance in ulps of torch's result, {"m", "v", "p"}, of ONE step from equal state, over `steps` steps of a run of
    torch.optim.Adam(capturable=...) on the HELD_SHAPES tensors with N(0, 1) * 1e-2 gradients: before every step torch's (p, m, v)
    are copied into a second set of tensors, `adam_step` (the signature of engine.optim.adam_step) steps that set and torch its own
    on the same gradients.  The two step counters advance in lockstep.  Not a statement about trajectories: over a run the
    differences compound."""
    import torch
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in HELD_SHAPES]
    ref = torch.optim.Adam(ps, lr=HELD_KW["lr"], betas=HELD_KW["betas"], eps=HELD_KW["eps"], capturable=capturable)
    mine = [[torch.zeros_like(p) for p in ps] for _ in range(3)]              # p, m, v
    counters = [torch.zeros((), device=dev) for _ in ps]
    ticket = new_ticket(dev)
    worst = {"m": 0, "v": 0, "p": 0}
    for k in range(steps):
        grads = [(torch.randn(s, generator=g) * 1e-2).to(dev) for s in HELD_SHAPES]
        for i, p in enumerate(ps):
            st = ref.state.get(p, {})
            mine[0][i].copy_(p.detach())
            for j, key in ((1, "exp_avg"), (2, "exp_avg_sq")):
                mine[j][i].copy_(st[key]) if st else mine[j][i].zero_()
            p.grad = grads[i].clone()
        adam_step(mine[0], grads, mine[1], mine[2], counters, ticket, **HELD_KW)
        ref.step()
        for i, p in enumerate(ps):
            st = ref.state[p]
            assert float(counters[i]) == float(st["step"]) == k + 1
            for name, got, want in (("p", mine[0][i], p.detach()), ("m", mine[1][i], st["exp_avg"]), ("v", mine[2][i], st["exp_avg_sq"])):
                worst[name] = max(worst[name], int(ulp_distance_torch(got, want).max()))
    return worst
