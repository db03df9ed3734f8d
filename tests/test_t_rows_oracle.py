"""CPU checks of tests/t_rows_oracle.py: every named case reaches, by the walk model, the branches of spmm_t_rows_bm_kernel it was built
for (a case that misses its branch is repaired in t_rows_oracle.py, never here); the exact and the order oracle equal a brute-force
Python loop on a tiny matrix; the order oracle's fma is `math.fma` where the interpreter has it; its data makes fp32 round."""
import math

import numpy as np
import pytest

import dropout_oracle as orc
import t_rows_oracle as tro

WALKED = [c for c in tro.CASES if not c.startswith("lds_")]


def _walk(name):
    c = tro.case(name)
    return tro.walk(c["rowptr"], c["colidx"], c["slot"], c["seg_len"])


@pytest.mark.parametrize("name", WALKED)
def test_every_case_reaches_the_branches_it_was_built_for(name):
    c, ev = tro.case(name), _walk(name)
    missing = [k for k in c["built_for"] if ev[k] <= 0]
    assert not missing, (name, missing, dict(ev))
    assert ev["units"] == -(-c["n"] // 16) and ev["chunks"] == -(-ev["units"] // 32)
    assert c["sel"].size > 0 and c["slot"][c["sel"]].tolist() == list(range(c["sel"].size))


def test_row_counts_put_the_units_and_chunks_on_their_edges():
    got = {n: _walk(f"rows_{n}") for n in tro.ROWS_N}
    assert [(got[n]["units"], got[n]["short_units"], got[n]["chunks"]) for n in tro.ROWS_N] == [
        (1, 1, 1), (1, 1, 1), (1, 0, 1), (2, 1, 1), (32, 0, 1), (33, 1, 2)]
    ev = _walk("rows_refill")
    assert ev["units"] > 2 * tro.WORKGROUPS * tro.CHUNK and ev["chunks"] > 2 * tro.WORKGROUPS     # a second chunk with units in it for every workgroup
    lens = np.diff(tro.case("rows_refill")["rowptr"])
    assert lens.min() == 1 and lens.max() == 2


def test_window_case_details():
    c, ev = tro.case("windows"), _walk("windows")
    assert np.diff(c["rowptr"]).max() <= c["seg_len"] == 2048 and ev["cut_rows"] == 0
    # the unit of 1 024 entries: row boundary on entry 512, hits on 511 and 512, in different rows
    assert ev["hit_row_change_on_window_boundary"] >= 1 and ev["row_starts_on_window_boundary"] >= 1
    # the unit of 513 entries: 511 | 512 are hits of one row (a window boundary inside a row)
    assert ev["hit_last_of_window"] >= 2 and ev["hit_first_of_window"] >= 2


def test_hits_case_details():
    ev = _walk("hits")
    assert ev["forced_at=85"] >= 2 and ev["forced_at=130"] >= 1 and ev["forced_at=168"] >= 1
    assert ev["list_exactly_full"] >= 4           # [84], 40 + 44, and [84, 84] twice
    assert ev["windows_one_by_one"] >= 3 and ev["one_by_one_after_parked"] >= 1
    assert tro.case("hits")["seg_len"] == 2048 and ev["cut_rows"] == 0


def test_runs_and_init_case_details():
    c, ev = tro.case("runs"), _walk("runs")
    lens = np.diff(c["rowptr"])
    assert c["seg_len"] == 64 and c["n"] % 16 == 5 and ev["cut_rows"] == (lens > 64).sum() == 25
    assert ev["segments"] == int((-(-lens[lens > 64] // 64)).sum()) and ev["cut_row_in_R"] >= 5
    cut_out_of_R = [r for r in np.flatnonzero(lens > 64) if c["slot"][r] < 0]
    assert cut_out_of_R, "a cut row outside R is needed as well"
    ev = _walk("init")
    assert ev["init_no_hit_rows"] >= 8 and ev["empty_rows_between_hits"] >= 14


def test_lds_limit():
    assert tro.lds_bytes(tro.LDS_MAX_N) <= tro.LDS_BYTES < tro.lds_bytes(tro.LDS_MAX_N + 1)
    assert tro.fits(tro.LDS_MAX_N, 4096) and not tro.fits(tro.LDS_MAX_N + 1, 4) and not tro.fits(512, 4100)
    assert tro.LDS_ODD_N % 32 and tro.LDS_ODD_N % 128
    assert [tro.panels(d) for d in (1, 512, 513, 600, 4096)] == [1, 1, 2, 2, 8]
    c = tro.case(f"lds_{tro.LDS_MAX_N}")
    assert c["n"] == tro.LDS_MAX_N and c["slot"][0] >= 0 and c["slot"][-1] >= 0 and 1.5 < c["colidx"].size / c["n"] < 2.5
    assert (c["colidx"] == c["n"] - 1).any() and (c["colidx"] == 0).any()


# ---- the oracles against brute force ---------------------------------------------------------------------------------------------
def _fma(v, x, acc):
    if hasattr(math, "fma"):
        return np.float32(math.fma(float(v), float(x), float(acc)))
    return np.float32(np.float64(v) * np.float64(x) + np.float64(acc))            # exact, then one rounding (see fma32)


def _brute_order(c, vals, X, init, keep):
    rp, col, slot, L = c["rowptr"], c["colidx"], c["slot"], c["seg_len"]
    out = np.zeros((c["n"], X.shape[1]), np.float32)
    for r in range(c["n"]):
        b, e = int(rp[r]), int(rp[r + 1])
        pieces = [(b, e)] if e - b <= L else [(s, min(s + L, e)) for s in range(b, e, L)]
        parts = []
        for i, (pb, pe) in enumerate(pieces):
            acc = init[slot[r]].copy() if (i == 0 and init is not None and slot[r] >= 0) else np.zeros(X.shape[1], np.float32)
            for j in range(pb, pe):
                if slot[col[j]] >= 0 and (keep is None or keep[j]):
                    for q in range(X.shape[1]):
                        acc[q] = _fma(vals[j], X[slot[col[j]], q], acc[q])
            parts.append(acc)
        if len(pieces) == 1:
            out[r] = parts[0]
        else:
            tot = np.zeros(X.shape[1], np.float32)
            for p in parts:
                tot = (tot + p).astype(np.float32)
            out[r] = tot
    return out


def _tiny():
    rng = np.random.default_rng(3)
    pats = {0: rng.random(150) < 0.5, 1: np.zeros(0, bool), 2: rng.random(64) < 0.5, 3: rng.random(65) < 0.5, 7: np.zeros(5, bool)}
    return tro._from_patterns("tiny", 20, pats, [0, 1, 3, 7, 9, 19], 64, 3, [])


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("drop", [False, True])
def test_exact_oracle_against_a_python_loop(with_init, drop):
    c = _tiny()
    X, init = tro.int_inputs(c, 3)
    seeds, p = ((5, 6), 0.3) if drop else ((), 0.0)
    got = tro.exact_product(c, X, init if with_init else None, seeds, p)
    want = np.zeros((c["n"], 3), np.int64)
    n_dropped = 0
    for r in range(c["n"]):
        if with_init and c["slot"][r] >= 0:
            want[r] += init[c["slot"][r]]
        for j in range(int(c["rowptr"][r]), int(c["rowptr"][r + 1])):
            col = int(c["colidx"][j])
            if c["slot"][col] < 0:
                continue
            if drop and not orc.keep_mask([col], [r], seeds, p)[0]:            # the key is the entry (col, r) of L
                n_dropped += 1
                continue
            want[r] += c["vals"][j] * X[c["slot"][col]]
    assert np.array_equal(got, want) and (n_dropped > 0) == drop


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("drop", [False, True])
def test_order_oracle_against_a_python_loop_with_fma(with_init, drop):
    c = _tiny()
    vals, X, init = tro.float_inputs(c, 3)
    keep = orc.keep_mask(tro.entry_rows(c), c["colidx"], (5, 6), 0.3, transposed=True) if drop else None
    got = tro.order_product(c, vals, X, init if with_init else None, keep)
    want = _brute_order(c, vals, X, init if with_init else None, keep)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert (np.diff(c["rowptr"]) > c["seg_len"]).sum() == 2                      # cut rows took part


@pytest.mark.parametrize("name", ["hits", "runs", "windows"])
def test_order_oracle_data_rounds_so_that_the_order_matters(name):
    c = tro.case(name)
    vals, X, init = tro.float_inputs(c, 8)
    fwd, rev = tro.order_product(c, vals, X, init), tro.order_product(c, vals, X, init, reverse=True)
    differs = (fwd != rev).any(1)
    n_hits = np.add.reduceat(np.r_[tro.kept_hits(c), False].astype(np.int64), c["rowptr"][:-1]) * (np.diff(c["rowptr"]) > 0)
    assert differs.sum() >= (n_hits >= 8).sum() // 2, (int(differs.sum()), int((n_hits >= 8).sum()))


def test_fma32_refuses_data_outside_its_range():
    one = np.ones((1, 1), np.float32)
    assert tro.fma32(one, one, one)[0, 0] == 2
    with pytest.raises(AssertionError):
        tro.fma32(one, one, np.full((1, 1), 2.0 ** -60, np.float32))
    if hasattr(math, "fma"):
        rng = np.random.default_rng(0)
        v, x, a = (tro.float_inputs(tro.case("hits"), 64)[k].reshape(-1)[:40] for k in (0, 1, 2))
        a = (a * rng.integers(1, 200, a.size)).astype(np.float32)
        got = tro.fma32(v, x, a)
        assert [float(g) for g in got] == [float(np.float32(math.fma(float(p), float(q), float(r)))) for p, q, r in zip(v, x, a)]
