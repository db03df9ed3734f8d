"""CPU tests of tests/adam_oracle.py, the host restatement that csrc/adam.hip is pinned to bit for bit (tests/test_adam_gpu.py): the
restatement itself is held against an fp64 evaluation of the textbook update, against torch.optim.Adam on CPU tensors, and its
beta^t against Python's."""
import math

import numpy as np
import pytest
import torch

import adam_oracle as orc

U32 = 2.0 ** -24          # unit roundoff of float32, round to nearest: one operation is off by at most U32, relatively
U64 = 2.0 ** -53


def gamma(k, u=U32):
    """k roundings in a row: the product of k factors (1 + d), |d| <= u, is off from 1 by at most this."""
    return (1.0 + u) ** k - 1.0


def _state(seed, n, steps):
    """(p, g, m, v, step) after `steps` oracle steps on N(0, 1) * 1e-2 gradients: moments of a run, not zeros."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    m, v, step = np.zeros(n, np.float32), np.zeros(n, np.float32), np.float32(0)
    for _ in range(steps):
        g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        p, m, v, step = orc.adam_step(p, g, m, v, step, lr=1e-2)
    return p, (rng.standard_normal(n) * 1e-2).astype(np.float32), m, v, step


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("steps", [0, 1, 7])
def test_oracle_against_the_textbook_update_in_fp64(steps, maximize, weight_decay):
    """Kingma & Ba's update, evaluated in fp64 from the same float32 state, against the oracle's float32 chain.  Every bound is a
    forward error bound counted from the operations: a term that passes through k float32 roundings is off by at most gamma(k) of
    its magnitude, and a sum by that much of the sum of its terms' magnitudes.  The fp64 evaluation's own roundings (fewer than 32
    per quantity) are added as 32 * 2^-53 of the same magnitudes.  No constant is fitted."""
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    p, g, m, v, step = _state(5 + steps, 4099, steps)
    got_p, got_m, got_v, got_step = orc.adam_step(p, g, m, v, step, lr=lr, betas=(b1, b2), eps=eps, weight_decay=weight_decay,
                                                 maximize=maximize)
    assert got_step == step + 1
    P, G, M, V = (x.astype(np.float64) for x in (p, g, m, v))
    t = int(step) + 1
    if maximize:
        G = -G
    G = G + weight_decay * P
    m_x = b1 * M + (1 - b1) * G
    v_x = b2 * V + (1 - b2) * G * G
    d_x = np.sqrt(v_x / (1 - b2 ** t)) + eps
    q_x = m_x / d_x
    s_x = lr / (1 - b1 ** t)
    p_x = P - s_x * q_x
    f64 = 32 * U64

    # g' = g + wd * p: wd to float32, the product, the sum - 3 roundings (none without weight decay); magnitude |g| + wd |p|
    kg = 3 if weight_decay else 0
    g_mag = np.abs(g.astype(np.float64)) + weight_decay * np.abs(P)
    # m' = m + c1 * (g' - m): c1 to float32, the difference, the product, the sum - 4 roundings on top of g's
    m_mag = np.abs(M) + (1 - b1) * (g_mag + np.abs(M))
    e_m = (gamma(kg + 4) + f64) * m_mag
    assert np.all(np.abs(got_m - m_x) <= e_m)
    # v' = v * beta2 + (c2 * g') * g': beta2 / c2 to float32, one / two products, the sum - at most 4 roundings, g' twice
    v_mag = b2 * V + (1 - b2) * g_mag * g_mag
    e_v = (gamma(2 * kg + 4) + f64) * v_mag
    assert np.all(np.abs(got_v - v_x) <= e_v)
    # d = sqrt(v') / bc2s + eps: the root of a value within e_v of v', then the root, bc2s to float32, the quotient, eps to
    # float32 and the sum - 5 roundings of positive terms
    bc2s = math.sqrt(1 - b2 ** t)
    e_root = np.sqrt(v_x + e_v) - np.sqrt(np.maximum(v_x - e_v, 0.0))
    e_d = e_root / bc2s * (1 + gamma(4)) + (gamma(5) + f64) * d_x
    # q = m' / d: (m' + dm) / (d + dd) - m' / d = (dm * d - m' * dd) / (d * (d + dd)), and the quotient's rounding.  Where g + wd * p
    # cancels on the first step, v' and so d are known to no digit (e_d >= d) and m' / d is +-1 by the sign of a rounding error: the
    # update is ill-conditioned there, no finite bound exists, and those few elements are held through m' and v' alone
    sound = e_d < d_x
    assert sound.mean() > 0.99
    with np.errstate(divide="ignore", invalid="ignore"):
        e_q = np.where(sound, (e_m + np.abs(q_x) * e_d) / (d_x - e_d), np.inf)
    e_q = e_q + gamma(1) * (np.abs(q_x) + e_q)
    # p' = p + step_size * q: step_size to float32, the product, the sum - 3 roundings
    e_p = s_x * e_q * (1 + gamma(2)) + (gamma(3) + f64) * (np.abs(P) + s_x * np.abs(q_x))
    assert np.all(np.abs(got_p - p_x) <= e_p)
    # and the bounds are tight enough to mean something: a few units in the last place of the magnitudes
    assert np.all(e_m <= 8 * U32 * m_mag) and np.all(e_v <= 11 * U32 * v_mag)


# Measured here with torch 2.10 on CPU tensors (its single-tensor path: lerp_, mul_ + addcmul_, sqrt / div / add_, addcdiv_), over
# the cases of the test below, in units in the last place of torch's result: max distance without weight decay m 18218, v 1, p 1024 and with it m 25945, v 12647, p 2048.  The large figures
# are cancellation, not another formula: m + c1 * (g - m), g + wd * p and p + step_size * q subtract, and where the result is a small
# fraction of its operands one rounding of an operand is many units of the result (v, a sum of positive terms, is 1 unit off without
# weight decay).  The bound is the measurement plus one: one more operation contracted differently moves a result by one unit.
TORCH_CPU_ULP = {False: {"m": 18218 + 1, "v": 1 + 1, "p": 1024 + 1}, True: {"m": 25945 + 1, "v": 12647 + 1, "p": 2048 + 1}}     # by weight decay


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("maximize", [False, True])
def test_oracle_against_torch_adam_on_cpu_tensors(maximize, weight_decay):
    """One step from identical state, 20 times along a run of torch's: torch's (p, m, v, step) before its step go through the
    oracle, and the oracle's result is compared with torch's after its step."""
    rng = np.random.default_rng(11 + 2 * int(maximize) + int(weight_decay > 0))
    worst = {"m": 0, "v": 0, "p": 0}
    for n in (65 * 65, 4097):
        prm = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)))
        opt = torch.optim.Adam([prm], lr=1e-2, weight_decay=weight_decay, maximize=maximize)
        for k in range(20):
            g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
            st = opt.state[prm]
            before = (prm.detach().numpy().copy(), g, st["exp_avg"].numpy().copy() if st else np.zeros(n, np.float32),
                      st["exp_avg_sq"].numpy().copy() if st else np.zeros(n, np.float32), np.float32(float(st["step"])) if st else np.float32(0))
            prm.grad = torch.from_numpy(g.copy())
            opt.step()
            got_p, got_m, got_v, got_step = orc.adam_step(*before, lr=1e-2, weight_decay=weight_decay, maximize=maximize)
            st = opt.state[prm]
            assert float(got_step) == float(st["step"]) == k + 1
            for name, got, want in (("m", got_m, st["exp_avg"]), ("v", got_v, st["exp_avg_sq"]), ("p", got_p, prm.detach())):
                worst[name] = max(worst[name], int(orc.ulp_distance(got, want.numpy()).max()))
    print("oracle against torch.optim.Adam on CPU, max ulp:", worst)
    for name in worst:
        assert worst[name] <= TORCH_CPU_ULP[weight_decay > 0][name], worst


def test_beta_pow_against_pythons_power():
    """Square-and-multiply takes at most log2(t) squarings and log2(t) + 1 products; held to 2 * log2(t) * 2^-53 of Python's
    `beta ** t`.  In plain fp64 a squaring doubles the error it inherits and the chain ends about
    t * 2^-53 off; the products are therefore kept in double-double.  Where the power underflows both sides give 0.0."""
    betas = (0.9, 0.999, 0.99, 0.8, 0.5, 0.95)
    ts = list(range(1, 1001)) + [2 ** k for k in range(10, 25)]
    for beta in betas:
        for t in ts:
            got, want = orc.beta_pow(beta, t), beta ** t
            bound = 2 * math.log2(t) * U64            # 0 at t = 1: the power is beta itself
            assert abs(got - want) <= bound * abs(want), (beta, t, got, want)
    assert orc.beta_pow(0.9, 0) == 1.0 and orc.beta_pow(0.999, 1) == 0.999
