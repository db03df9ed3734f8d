"""The HIP builder of the year-slice Laplacians (csrc/laplacian.hip, matrix.laplacian_csr_slices, Matrix(builder="device")) against
the torch builder on the CPU, which tests/test_matrix.py pins to the reference bit for bit.  Nothing in the recipe may differ by a
bit, so every comparison is exact: rows, columns and the values' bits."""
import numpy as np
import pandas as pd
import pytest
import torch

import laplacian_cases as lc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _build(year, userid, itemid, rating, n_user, n_item):
    from seoul_tourism_recommendation_ngcf_amd.matrix import laplacian_csr_slices
    return laplacian_csr_slices(year, userid, itemid, rating, n_user, n_item, torch.device(DEV))


def _frame(g, tag):
    return pd.DataFrame({k: g[f"{tag}_in_{k}"] for k in ("year", "userid", "itemid", "visitor")})


def _matrix(g, tag, builder, **kw):
    from seoul_tourism_recommendation_ngcf_amd.matrix import Matrix
    U, I = (int(x) for x in g[f"{tag}_dims"])
    return Matrix(_frame(g, tag), ["year", "userid", "itemid", "visitor"], "visitor", {"user": U, "item": I}, device=torch.device(DEV),
                  builder=builder, **kw)


@pytest.fixture(scope="module")
def branch_points():
    """The branch-point graph, its oracle slices (checked to hold the rows it was built for) and one device build, shared."""
    from seoul_tourism_recommendation_ngcf_amd import engine
    wave_limit, group_limit = engine.laplacian_limits()
    year, userid, itemid, rating, n_user, n_item, plan = lc.branch_point_input(wave_limit, group_limit)
    want = lc.oracle_slices(year, userid, itemid, rating, n_user, n_item)
    lc.check_branch_point_plan(want, year, userid, plan, n_user, n_item, wave_limit, group_limit)
    got = _build(year, userid, itemid, rating, n_user, n_item)
    return (year, userid, itemid, rating, n_user, n_item), want, got


@pytest.mark.parametrize("tag", ["toy", "mid"])
def test_golden_slices_through_matrix(tag, tmp_path):
    """The reference's own output, through the public class - and `save_data` writes a file `load_lap_list` reads back."""
    from seoul_tourism_recommendation_ngcf_amd.matrix import load_lap_list
    g = load_golden("matrix")
    U, I = (int(x) for x in g[f"{tag}_dims"])
    m = _matrix(g, tag, "device", folder_path=str(tmp_path), save_data=True)
    laps = m.create_matrix()
    assert len(laps) == 2
    back = load_lap_list(m.saved_path)
    for yi, L in enumerate(laps):
        assert L.is_sparse and L.is_cuda and tuple(L.shape) == (U + I, U + I) and L.dtype == torch.float32 and not L.is_coalesced()
        for T in (L, back[yi]):
            idx, val = T._indices().cpu().numpy(), T._values().cpu().numpy()
            assert np.array_equal(idx[0], g[f"{tag}_lap{yi}_rows"]) and np.array_equal(idx[1], g[f"{tag}_lap{yi}_cols"])
            assert np.array_equal(val, g[f"{tag}_lap{yi}_vals"])


def test_semantics_case_equals_the_oracle():
    year, userid, itemid, rating = lc.semantics_input()
    U, I = lc.SEMANTICS_DIMS
    assert year[0] == 19 and sorted(set(year.tolist())) == [18, 19, 20] and 38 <= len(year) <= 42
    assert 5 not in userid and 6 not in itemid                                   # a user and an item that never appear
    want = lc.oracle_slices(year, userid, itemid, rating, U, I)
    got = _build(year, userid, itemid, rating, U, I)
    lc.assert_slices_equal(got, want)
    # the 1.4e-45 entry (user 4, item 5): gone from year 19's slice, where it underflows, back in year 18's, which is built next
    # from the carried-over state with smaller degrees
    def has(sl):
        rows, cols, _ = sl.coo()
        return bool(((rows == 4) & (cols == U + 5)).any()), bool(((rows == U + 5) & (cols == 4)).any())
    assert has(got[19 % 18]) == (False, False) and has(got[18 % 18]) == (True, True)
    rows, cols, vals = got[0].coo()
    assert float(vals[(rows == 4) & (cols == U + 5)]) == np.float32(lc.UNDERFLOW)
    # user 3 lost every edge in year 18 and user 5 never appears: empty rows
    assert int(got[0].rowptr[4] - got[0].rowptr[3]) == 0 and int(got[0].rowptr[6] - got[0].rowptr[5]) == 0


def test_branch_points_equal_the_oracle(branch_points):
    _, want, got = branch_points
    lc.assert_slices_equal(got, want)
    for k, sl in got.items():                                                    # and the CSR is well formed
        n = sl.n
        assert sl.rowptr.dtype == torch.int64 and sl.colidx.dtype == torch.int32 and tuple(sl.rowptr.shape) == (n + 1,)
        assert int(sl.rowptr[0]) == 0 and int(sl.rowptr[-1]) == sl.nnz == int(want[k][0].numel())


def test_two_builds_give_identical_bytes(branch_points):
    inp, _, got = branch_points
    again = _build(*inp)
    for k in got:
        for a, b in ((got[k].rowptr, again[k].rowptr), (got[k].colidx, again[k].colidx), (got[k].vals.view(torch.int32), again[k].vals.view(torch.int32))):
            assert torch.equal(a, b), k


def test_record_order_does_not_matter_without_repeats():
    year, userid, itemid, rating, n_user, n_item = lc.unique_pairs_input()
    want = lc.oracle_slices(year, userid, itemid, rating, n_user, n_item)
    lc.assert_slices_equal(_build(year, userid, itemid, rating, n_user, n_item), want)
    order = lc.permutation_first_year_first(year, np.random.default_rng(5))
    assert year[order][0] == year[0] and not np.array_equal(order, np.arange(order.size))
    lc.assert_slices_equal(_build(year[order], userid[order], itemid[order], rating[order], n_user, n_item), want)


def test_bad_ids_raise_and_the_next_build_is_right():
    """A refusal, not a fault: the kernels leave flagged records out of the buckets and never read through them."""
    year, userid, itemid, rating = lc.semantics_input()
    U, I = lc.SEMANTICS_DIMS
    for col, value in (("userid", U), ("itemid", -1), ("itemid", I)):
        u, i = userid.copy(), itemid.copy()
        (u if col == "userid" else i)[17] = value
        with pytest.raises(IndexError, match="outside"):
            _build(year, u, i, rating, U, I)
    lc.assert_slices_equal(_build(year, userid, itemid, rating, U, I), lc.oracle_slices(year, userid, itemid, rating, U, I))
    with pytest.raises(RuntimeError, match="ROCm device"):
        from seoul_tourism_recommendation_ngcf_amd.matrix import laplacian_csr_slices
        laplacian_csr_slices(year, userid, itemid, rating, U, I, "cpu")


def test_slices_feed_the_engine():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    from seoul_tourism_recommendation_ngcf_amd import engine
    g = load_golden("matrix")
    U, I = (int(x) for x in g["mid_dims"])
    dev = torch.device(DEV)
    cols = [g[f"mid_in_{k}"] for k in ("year", "userid", "itemid", "visitor")]
    want = lc.oracle_slices(*cols, U, I)
    got = _build(*cols, U, I)
    gen = torch.Generator().manual_seed(3)
    for k in sorted(want):
        direct = got[k].csr()
        via_coo = engine.LaplacianCSR.from_coo(*(t.to(dev) for t in want[k]), U + I, U + I)
        assert direct.nnz == via_coo.nnz
        for d in (64, 65):
            E = torch.randn(U + I, d, generator=gen).to(dev)
            assert torch.equal(engine.spmm(direct, E), engine.spmm(via_coo, E)), (k, d)
    num_dict = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    outs = []
    for builder in ("device", "torch"):
        laps = _matrix(g, "mid", builder).create_matrix()
        torch.manual_seed(11)
        model = pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, laps, num_dict, 8, dev).to(dev).eval()
        with torch.no_grad():
            outs.append(model.propagate(1).clone())
    assert outs[0].shape == (U + I, 65 + 128) and torch.equal(outs[0], outs[1])
