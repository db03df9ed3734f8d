"""BASELINE.json configs[4] (C5: 10 M users x 1 M items, 500 M interactions, d = 256) on the one GPU a box has: the slabs that
ranks 0, 3 and 7 of the 8-GPU row partition hold - each (1.25 M user rows + ~1/8 of the item rows by stored entries, ~125 M stored entries
of the 1 G, gathered from the full 11 M-row replica), built exactly as `dist.ShardedPropagation.from_interactions` builds
it.  Size-independent properties: linearity, fp64 spot rows from the definition (incl. the heaviest rows), agreement of the
kernel variants; and the whole dense half on the slab's rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ATOL, RTOL = 2e-5, 2e-3            # forward tolerance


def test_c5_rank_slabs_of_eight():
    """Ranks 0, 3 and 7 of eight (the two boundary ranks and a middle one): SpMM properties on both slabs and the whole dense half
    (NGCF.py:131-146) on both slabs' rows."""
    import seoul_tourism_recommendation_ngcf_amd as pkg
    from seoul_tourism_recommendation_ngcf_amd import dist as nd
    eng = pkg.engine
    dev = torch.device("cuda:0")
    U, I, W, d = 10_000_000, 1_000_000, 8, 256
    u, i, w = pkg.graphs.synthetic_interactions(U, I, 500_000_000, seed=2605, device=dev)
    n_inter = int(u.numel())
    assert n_inter > 490_000_000
    v, deg_u, deg_i = nd.laplacian_values(u, i, w, U, I)
    del w
    cnt = torch.cat([deg_u, deg_i]).cpu()
    ub, ib = nd.balanced_bounds(cnt, 0, U, W), nd.balanced_bounds(cnt, U, U + I, W)
    lay = nd.ShardLayout(U, I, ub, ib)
    g = torch.Generator(device=dev).manual_seed(5)
    X = torch.randn((lay.P, d), generator=g, device=dev)
    Y = torch.randn((lay.P, d), generator=g, device=dev)
    gw = torch.Generator().manual_seed(7)
    W1, W2 = ((torch.rand((d, d), generator=gw) - 0.5) * 0.2 for _ in range(2))
    b1, b2 = ((torch.rand((d,), generator=gw) - 0.5) * 0.1 for _ in range(2))
    W1, W2, b1, b2 = (t.to(dev) for t in (W1, W2, b1, b2))
    ws = eng.Workspace()
    for rank in (0, 3, 7):
        (ur, uc, uv), (ir, ic, iv) = nd.cut_slabs(u, i, v, U, ub[rank], ub[rank + 1], ib[rank] - U, ib[rank + 1] - U)
        torch.cuda.empty_cache()
        nu, ni = lay.n_users_of(rank), lay.n_items_of(rank)
        slabs = {"user": (ur - ub[rank], lay.to_padded(uc), uv, nu, lay.user_pos(rank)),
                 "item": (ir - ib[rank], lay.to_padded(ic), iv, ni, lay.item_pos(rank))}
        stored = sum(int(s[0].numel()) for s in slabs.values())
        assert abs(stored - 2 * n_inter / W) < 0.02 * 2 * n_inter / W        # the rank holds 1/8 of the stored entries
        for name, (r, c, vals, n_rows, pos0) in slabs.items():
            tag = f"rank {rank} {name}"
            csr = eng.LaplacianCSR.from_coo(r, c, vals, n_rows, lay.P)
            csr.set_mode(3)
            # expected re-use of a fetched table row inside an XCD is ~0.9 at this shape: the plan declines on the
            # middle rank; rank 0 holds the most popular items (15 K rows of ~4 000 entries: re-use above 3, a plan is built), but
            # the 12 GB table is beyond the plan's 32-bit offsets, so its products run on the row-wise kernels all the same
            if rank == 3:
                assert csr.swept_rows == 0, tag
            LX = eng.spmm(csr, X, ws=ws)
            LY = eng.spmm(csr, Y, ws=ws)
            LZ = eng.spmm(csr, 2.0 * X - 0.5 * Y, ws=ws)
            scale = float(LX.abs().max())
            assert float((LZ - (2.0 * LX - 0.5 * LY)).abs().max()) <= 2e-5 * max(scale, 1.0), tag
            if rank == 3:
                csr.set_mode(1)                                               # row-wise kernels without d-slicing: same product
                assert float((eng.spmm(csr, X, ws=ws) - LX).abs().max()) <= 2e-6 * max(scale, 1.0), tag
            deg = torch.bincount(r, minlength=n_rows)
            rows = torch.cat([torch.randint(0, n_rows, (24,), device=dev), torch.topk(deg, 4).indices, torch.tensor([0, n_rows - 1], device=dev)])
            rp = torch.searchsorted(r, torch.stack([rows, rows + 1]))
            for row, (lo, hi) in zip(rows.tolist(), rp.T.tolist()):
                want = (vals[lo:hi].double()[:, None] * X[c[lo:hi]].double()).sum(0)
                np.testing.assert_allclose(LX[row].cpu().numpy(), want.cpu().numpy(), atol=ATOL, rtol=RTOL, err_msg=f"{tag} row {row}")
            # one whole layer (NGCF.py:130-146) on the slab: unit-norm rows, sample rows against fp64 from the definition
            e_self = X[pos0:pos0 + n_rows]
            carry = torch.empty((n_rows, d), device=dev)
            nrm = torch.empty((n_rows, d), device=dev)
            eng.layer_fused(csr, X, e_self, W1, b1, W2, b2, carry, nrm, ws)
            assert float((nrm.norm(dim=1) - 1).abs().max()) < 1e-5, tag
            for row in rows[:6].tolist() + rows[-2:].tolist():
                le, e = LX[row].double(), e_self[row].double()
                m = (le + e) @ W1.double().T + 2 * b1.double() + (le * e) @ W2.double().T + b2.double()
                m = torch.where(m >= 0, m, 0.2 * m)
                np.testing.assert_allclose(carry[row].cpu().numpy(), m.cpu().numpy(), atol=2e-4, rtol=RTOL, err_msg=f"{tag} row {row}")
                # ... and the block that goes into all_E (F.normalize, NGCF.py:144) at the forward tolerance itself: the carry's entries
                # are O(1..30) here (random unit-variance operands, K = 256), its normalised row is what SURVEY 8c's atol is stated on
                np.testing.assert_allclose(nrm[row].cpu().numpy(), (m / m.norm().clamp_min(1e-12)).cpu().numpy(), atol=ATOL, rtol=RTOL,
                                           err_msg=f"{tag} normalised row {row}")
            del csr, LX, LY, LZ, carry, nrm
        del ur, uc, uv, ir, ic, iv, slabs
        if rank == 3:
            # the same rank's slabs in the DEFAULT exchange scheme (bipartite, sharded.py): user rows x item replica in the
            # owner-major padded numbering, and the transposed slab that forms the item partial sums over the local users
            ob = nd.even_bounds(0, I, W)
            mi = max(ob[q + 1] - ob[q] for q in range(W))
            PI = W * mi
            eb = nd.balanced_bounds(cnt, 0, U, W)
            lo, hi = eb[rank], eb[rank + 1]
            (bur, buc, buv), _ = nd.cut_slabs(u, i, v, U, lo, hi, 0, 0)
            pos = nd.padded_item_pos(buc - U, ob, mi)
            csr_u = eng.LaplacianCSR.from_coo(bur - lo, pos, buv, hi - lo, PI)
            order = torch.sort(pos, stable=True).indices
            csr_it = eng.LaplacianCSR.from_coo(pos[order], bur[order] - lo, buv[order], PI, hi - lo)
            assert csr_u.nnz == csr_it.nnz and abs(csr_u.nnz - n_inter / W) < 0.02 * n_inter / W
            Xi, Xu = X[:PI], X[:hi - lo]
            for name, csr, tab, (rr, cc, vv) in (("bipartite user rows", csr_u, Xi, (bur - lo, pos, buv)),
                                                  ("bipartite item partial sums", csr_it, Xu, (pos[order], bur[order] - lo, buv[order]))):
                out = eng.spmm(csr, tab, ws=ws)
                out2 = eng.spmm(csr, 3.0 * tab, ws=ws)
                scale = float(out.abs().max())
                assert float((out2 - 3.0 * out).abs().max()) <= 2e-5 * max(scale, 1.0), name
                rows = torch.cat([torch.randint(0, csr.n_rows, (16,), device=dev), torch.topk(torch.bincount(rr, minlength=csr.n_rows), 3).indices])
                rp = torch.searchsorted(rr, torch.stack([rows, rows + 1]))
                for row, (a, b) in zip(rows.tolist(), rp.T.tolist()):
                    want = (vv[a:b].double()[:, None] * tab[cc[a:b]].double()).sum(0)
                    np.testing.assert_allclose(out[row].cpu().numpy(), want.cpu().numpy(), atol=ATOL, rtol=RTOL, err_msg=f"{name} row {row}")
            del csr_u, csr_it, bur, buc, buv, pos, order
