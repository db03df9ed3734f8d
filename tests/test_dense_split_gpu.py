"""layer_dense_split_kernel (dense_resident = 4, the default): the large-row dense layer on the bf16 matrix cores with an exact
three-way split of every fp32 operand.  Not bit-identical to the fp32 kernels, so it is held to their accuracy instead: on sampled
rows its error against an fp64 restatement of the layer is at most twice that of layer_dense_resident_kernel (dense_resident = 1)
on the same inputs; the dropout zero pattern is the fp32 path's, bit for bit, and the rows of the normalised block are unit rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROWS = 140_001            # above dense_resident_min_rows; not a multiple of 32: a partial last tile


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
    le, e = LE[r, :d_in], E[r, :d_in]
    A = torch.cat((le + e, le * e), 1).double()          # the operands as both kernels form them (fp32 sums and products)
    B = torch.cat((W1.T, W2.T), 0).double()
    bias = (b1 + b1 + b2).double()
    pre = A @ B + bias
    scale = A.abs() @ B.abs() + bias.abs()               # what the rounding error of the product is measured against
    act = torch.where(pre >= 0, pre, 0.2 * pre)
    if mode in ("hash", "mask"):
        keep = c32[r] != 0 if mode == "hash" else mask[r] != 0
        act = act * keep.double() / 0.7
        scale = scale * keep.double() / 0.7
    nrm = act / act.norm(dim=1, keepdim=True).clamp_min(1e-12)
    tiny = 2.0 ** -24

    def err_carry(c):
        return float(((c[r].double() - act).abs() / (scale + 1e-300)).max())

    def err_norm(nb):
        rn = act.norm(dim=1, keepdim=True).clamp_min(1e-12)
        return float(((nb[r].double() - nrm).abs() * rn / (scale.amax(dim=1, keepdim=True) + 1e-300)).max())

    if mode != "last":
        e32, esp = err_carry(c32), err_carry(csp)
        assert esp <= 2 * e32 + tiny, (esp, e32)
        if mode in ("hash", "mask"):
            assert torch.equal(csp == 0, c32 == 0)        # the dropout zero pattern of the fp32 path
            if mode == "hash" and not mixed:
                assert abs(float((csp == 0).float().mean()) - 0.3) < 0.01
    e32, esp = err_norm(n32), err_norm(nsp)
    assert esp <= 2 * e32 + tiny, (esp, e32)
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
