"""The trip context on the device against tests/context_oracle.py: the Kahan sums, the float pivot and the congestion table bit for bit
(the oracle is pinned to pd.pivot_table on these very inputs in tests/test_context_oracle.py), the haversine table within 4x the
spread of two host evaluations of the same formula, and `recommend.blended_ranking` fed from raw rows against the same call fed
with tables and rows built on the host."""
import functools

import numpy as np
import pytest
import torch

import context_oracle as orc
import groupby_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DAYS3 = ((7, 30, 2), (7, 31, 3), (8, 1, 4))
DAYS5 = DAYS3 + ((8, 2, 5), (8, 3, 6))


def _pkg():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.cpu().contiguous().view(torch.int64)


# ---- Kahan sums ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_order", [False, True])
@pytest.mark.parametrize("n_values", [1, 2])
def test_kahan_sums_equal_the_oracle_bit_for_bit_on_both_tiers(n_values, with_order):
    rowptr, order, _, columns, want, plain = orc.kahan_case(n_values, with_order)
    lengths = np.diff(rowptr)
    long = lengths >= 64
    assert long.any() and all((w[long].view(np.int64) != p[long].view(np.int64)).any() for w, p in zip(want, plain))   # on the host, first
    ctx = _pkg().engine.context
    values = tuple(_dev(c) for c in columns)
    for wave_min in (1, int(lengths.max()) + 1, 0):                # all on the wave tier, all on the lane tier, the default
        runs = [ctx.segment_kahan_sum(_dev(rowptr), values if n_values > 1 else values[0], order=_dev(order), wave_min=wave_min)
                for _ in range(2)]
        assert len(runs[0]) == n_values
        for k in range(n_values):
            assert runs[0][k].dtype == torch.float64 and torch.equal(_bits(runs[0][k]), torch.from_numpy(want[k].view(np.int64))), (wave_min, k)
            assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), (wave_min, k)
    got = runs[0][0].cpu().numpy()
    assert (got[lengths == 0] == 0).all() and np.isposinf(got).sum() >= 1          # empty and all-NaN: 0.0; the +inf segment


@pytest.mark.parametrize("wave_min", [1, 100000])
def test_out_of_range_order_and_rowptr_raise_and_fault_nothing(wave_min):
    rowptr, order, _, columns, _, _ = orc.kahan_case(1, True)
    ctx = _pkg().engine.context
    x = _dev(columns[0])
    for bad in (len(order), -1, 2 ** 40):
        o = order.copy()
        o[len(o) // 2] = bad
        with pytest.raises(IndexError):
            ctx.segment_kahan_sum(_dev(rowptr), x, order=_dev(o), wave_min=wave_min)
    for u, v in ((-1, len(order) + 1), (3, -2)):
        r = rowptr.copy()
        r[u] = v
        with pytest.raises(IndexError):
            ctx.segment_kahan_sum(_dev(r), x, order=_dev(order), wave_min=wave_min)
    torch.cuda.synchronize()                                       # every entry was checked before use


# ---- group_sum_float and congestion_table ------------------------------------------------------------------------------------------
def test_float_pivot_and_congestion_table_equal_the_oracle_bit_for_bit():
    pkg = _pkg()
    n_item = 130
    log = orc.congestion_log(DAYS3, n_item)
    index = ("month", "day", "dayofweek", "item")
    keys, sums, inverse = orc.pivot_float([log[c] for c in index], [log["congestion_1"], log["congestion_2"]])
    cols = [_dev(log[c]) for c in index]
    cols[1] = cols[1].to(torch.int32)
    vals = (_dev(log["congestion_1"]), _dev(log["congestion_2"]))
    for wave_min in (0, 1, 8):
        g = pkg.engine.context.group_sum_float(cols, vals, wave_min=wave_min)
        assert len(g.keys) == 4 and len(g.sums) == 2
        for k in range(4):
            assert g.keys[k].dtype == torch.int64 and np.array_equal(g.keys[k].cpu().numpy(), keys[k])
        for v in range(2):
            assert g.sums[v].dtype == torch.float64 and orc.same_bits(g.sums[v].cpu().numpy(), sums[v]), (wave_min, v)
        assert np.array_equal(g.inverse.cpu().numpy(), inverse)
    for by in (0, 1):
        want_table, want_days = orc.congestion_table(log, n_item, by=by)
        table, days = pkg.recommend.congestion_table(*cols, vals, n_item=n_item, by=by)
        assert table.dtype == torch.float64 and days.dtype == torch.int64 and np.array_equal(days.cpu().numpy(), want_days)
        assert orc.same_bits(table.cpu().numpy(), want_table)
        assert 0 < int(torch.isposinf(table).sum()) == 3 * n_item - len(keys[0])            # absent pairs are +inf
    one, _ = pkg.recommend.congestion_table(*cols, vals[1], n_item=n_item)
    assert torch.equal(_bits(one), _bits(table))
    with pytest.raises(IndexError, match="outside \\[0, 129\\)"):
        pkg.recommend.congestion_table(*cols, vals, n_item=n_item - 1)


# ---- haversine -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _haversine(kind, S, n_item):
    dep, item = orc.points(kind, S, n_item)
    want = orc.haversine_numpy(dep, item)
    spread = float(orc.ulps(orc.haversine_math(dep, item), want).max())
    got = _pkg().recommend.distance_table(_dev(dep), _dev(item)).cpu().numpy()
    return dep, item, want, spread, got


@pytest.mark.parametrize("kind,S,n_item", [("seoul", 3, 130), ("globe", 3, 130), ("seoul", 17, 257)])
def test_haversine_table_within_four_times_the_spread_of_two_host_evaluations(kind, S, n_item):
    """The yardstick is recomputed: the largest difference, in ulps of numpy's value, between numpy's and `math`'s evaluation of the
    formula on these inputs; the device gets 4x it (three transcendental calls from another library through the same conditioning).

    On these inputs numpy's sin and cos are the host libm's, as `math`'s are, and the two arcsin agree at the small arguments of a
    city: the spread of the Seoul 3 x 130 set is 0 and its bound asks for the host's bits.  The kernel meets it because its sin,
    cos and asin are correctly rounded (csrc/dd_math.h, tests/test_dd_math.py) and so, on these arguments, are glibc's.
    The same text compiled for the host gives Python's bits on all three sets, so against numpy the expected maxima are the spreads
    themselves: 0, 2 and 1 ulp."""
    dep, item, want, spread, got = _haversine(kind, S, n_item)
    err = orc.ulps(got, want)
    print(f"haversine {kind} {S}x{n_item}: host spread {spread} ulp, device max {err.max()} ulp, bound {4 * spread} ulp")
    assert got.shape == (S, n_item) and got.dtype == np.float64
    assert got[0, 1] == 0.0 and not np.signbit(got[0, 1])                          # coincident points: exactly 0.0
    assert np.array_equal(got[:, 2], got[:, 3])                                    # the same coordinates, the same bits
    assert err.max() <= 4 * spread, (kind, float(err.max()), spread)
    bound = 4 * spread * np.spacing(want)
    for s in range(S):                                                             # the row's item order, where the oracle's is decided
        idx = np.argsort(want[s], kind="stable")
        a, b = idx[:-1], idx[1:]
        apart = want[s][b] - want[s][a] > bound[s][b]
        assert (got[s][a][apart] < got[s][b][apart]).all(), (kind, s)


def test_haversine_nan_coordinates_give_inf_and_out_is_written_in_place():
    pkg = _pkg()
    dep, item = (x.copy() for x in orc.points("seoul", 3, 130))
    dep[1, 0], item[7, 1], item[9, 0] = np.nan, np.nan, np.nan
    out = torch.full((3, 130), -1.0, dtype=torch.float64, device=DEV)
    got = pkg.engine.context.haversine_table(_dev(dep), _dev(item), out=out)
    assert got is out
    got = got.cpu().numpy()
    missing = np.zeros((3, 130), dtype=bool)
    missing[1, :], missing[:, 7], missing[:, 9] = True, True, True
    assert np.isposinf(got[missing]).all() and np.isfinite(got[~missing]).all() and (got[~missing] >= 0).all()
    assert np.array_equal(got[~missing], _haversine("seoul", 3, 130)[4][~missing])
    assert pkg.recommend.distance_table(_dev(dep[:0]), _dev(item)).shape == (0, 130)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
N_USER, N_ITEM, TOP, POINTS = 5840, 100, 10, 100
WEIGHTS = (0.5, 0.25, 0.25)                                        # exact in binary: the blend's rounding note does not apply


def _model():
    pkg = _pkg()
    laps = [pkg.graphs.to_sparse_coo(s) for s in pkg.graphs.seoul_standin(DEV)]
    num_dict = {"user": N_USER, "item": N_ITEM, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}
    torch.manual_seed(1801)
    return pkg.NGCF(65, [64, 64], 0.3, [0.1, 0.1], 1.0, laps, num_dict, 25, DEV).to(DEV)


def test_blended_ranking_from_raw_rows_equals_the_host_built_context():
    pkg = _pkg()
    rec = pkg.recommend
    # the reference's 5 840 users: the sorted strings are the dictionary, their codes what preprocess.map_ids keeps
    strings = sorted(groupby_oracle.user_strings(*groupby_oracle.reference_users()).tolist())
    user_dict = {s: i for i, s in enumerate(strings)}
    user_codes = torch.tensor([groupby_oracle.code_of_string(s) for s in strings], dtype=torch.int64, device=DEV)
    assert len(strings) == N_USER and bool((user_codes[1:] > user_codes[:-1]).all())
    parties = [dict(ages=[27, 61], sexes=[0, 1], month=7, day=30, dow=2, duration=3),           # crosses the end of July
               dict(ages=[33, 38], sexes=[1, 1], month=8, day=1, dow=4, duration=3)]           # one age bucket and sex: one id per day
    log = orc.congestion_log(DAYS5, N_ITEM)
    dep, item = orc.points("seoul", 2, N_ITEM)                     # a departure point per party; items 2 and 3 coincide

    # on the host, by the oracle
    rows = [r + [p] for p, q in enumerate(parties)
            for r in orc.party_loop(q["ages"], q["sexes"], q["month"], q["day"], q["dow"], q["duration"], user_dict)]
    want_uid, want_feats = [r[0] for r in rows], [[r[c] for r in rows] for c in range(1, 6)]
    table, days = orc.congestion_table(log, N_ITEM)
    day_index = {tuple(d): s for s, d in enumerate(days.tolist())}
    want_con_slot = [day_index[(r[3], r[4], r[5])] for r in rows]
    want_dis_slot = [r[6] for r in rows]
    host_con, host_dis = orc.dense_ranks(table), orc.dense_ranks(orc.haversine_numpy(dep, item))
    assert np.isinf(host_con).any() and (host_dis[:, 2] == host_dis[:, 3]).all()               # absent pairs and a tie are in play

    # on the device, from raw rows
    got = rec.party_rows(torch.tensor([0, 0, 1, 1], device=DEV), torch.tensor([27, 61, 33, 38], device=DEV),
                         torch.tensor([0, 1, 1, 1], device=DEV), start_month=[7, 8], start_day=[30, 1], start_dow=[2, 4], duration=3,
                         user_codes=user_codes)
    assert got.user_ids.tolist() == want_uid and [t.tolist() for t in got.features] == want_feats
    assert got.party.tolist() == want_dis_slot
    con, con_days = rec.congestion_table(*(_dev(log[c]) for c in ("month", "day", "dayofweek", "item")),
                                         (_dev(log["congestion_1"]), _dev(log["congestion_2"])), n_item=N_ITEM)
    con_slot = rec.context_slots(con_days, got.month, got.day, got.dow)
    assert con_slot.tolist() == want_con_slot
    dev_con, dev_dis = rec.order_table(con), rec.order_table(rec.distance_table(_dev(dep), _dev(item)))
    assert np.array_equal(dev_con.cpu().numpy(), host_con) and np.array_equal(dev_dis.cpu().numpy(), host_dis)

    model = _model()
    mask = torch.rand(N_ITEM, generator=torch.Generator().manual_seed(7)) < 0.5
    kw = dict(year=[0], weights=WEIGHTS, item_mask=mask.to(DEV), top=TOP, points=POINTS, return_table=True)
    raw = rec.blended_ranking(model, got.user_ids, features=got.features, congestion=dev_con, congestion_slot=con_slot, distance=dev_dis,
                              distance_slot=got.party, **kw)
    host = rec.blended_ranking(model, torch.tensor(want_uid), features=tuple(torch.tensor(f) for f in want_feats),
                               congestion=torch.from_numpy(host_con), congestion_slot=torch.tensor(want_con_slot),
                               distance=torch.from_numpy(host_dis), distance_slot=torch.tensor(want_dis_slot), **kw)
    assert len(raw) == len(host) == 4
    for a, b in zip(raw, host):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert raw[0].shape == (len(set(want_uid)), TOP) and bool((raw[0] >= 0).all())
    # the lookup's refusals: a string the dictionary does not hold, named by its first row
    with pytest.raises(IndexError, match="request row 1: '2501231'"):
        rec.party_rows(torch.tensor([0], device=DEV), torch.tensor([27], device=DEV), torch.tensor([0], device=DEV), start_month=12,
                       start_day=30, start_dow=0, duration=2,
                       user_codes=torch.cat((user_codes[:user_dict["2501231"]], user_codes[user_dict["2501231"] + 1:])))
