"""Host-side surface of the rank-point blending: the C ABI symbols, argument errors before any launch, the public module, and the
column builder of the reference's four views."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_blend_points():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib, engine
    text = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ngcf_blend_points\s*\(", text) and re.search(r"\bint64_t\s+ngcf_blend_workspace_bytes\s*\(", text)
    lib = _lib.load()
    for name in ("ngcf_blend_points", "ngcf_blend_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert any(p.endswith("blend.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    assert b"blend_points_kernel" in blob and b"blend_merge_kernel" in blob       # gfx950 kernels of its own
    assert int(lib.ngcf_version()) == _lib.ABI_VERSION == 11
    assert engine.BLEND_TOP_MAX == 256


def test_workspace_bytes():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    assert lib.ngcf_blend_workspace_bytes(7, 100, 10, 0) == 0                      # one tile: the result is written directly
    assert lib.ngcf_blend_workspace_bytes(7, 300, 10, 128) == 7 * 3 * 10 * 16      # three tiles: [G, tiles, top] items and ratings
    assert lib.ngcf_blend_workspace_bytes(7, 100000, 10, 0) == 7 * 25 * 10 * 16    # the default tile: 4 096 items
    assert lib.ngcf_blend_workspace_bytes(7, 300, 0, 0) == -1 and lib.ngcf_blend_workspace_bytes(7, 300, 10, 4097) == -1


def test_c_abi_limits_are_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()

    def call(R=6, Pl=100, P=100, n_items=100, top=10, tile=0, G=2, ld=None):
        ld = Pl if ld is None else ld
        return lib.ngcf_blend_points(None, ld, R, Pl, None, ld, 3, None, None, ld, 1, None, None, None, 12, G, P, n_items,
                                     0.5, 0.3, 0.2, None, top, tile, None, None, None, None, None, 0, None)
    assert call() == _lib.ERR_ARG and "null argument" in _lib.last_error()       # everything else in range: only the pointers are missing
    assert call(G=0) == _lib.OK                                                   # no columns: nothing to do
    cases = ((dict(top=0), "top outside [1, 256]"), (dict(top=257), "top outside [1, 256]"),
             (dict(P=0, Pl=1), "outside [1, 1024]"), (dict(P=1025), "outside [1, 1024]"),
             (dict(R=(2 ** 31 + 99) // 100), ">= 2^31"), (dict(R=2 ** 31, P=1, Pl=1), ">= 2^31"),
             (dict(Pl=101), "bad argument"), (dict(Pl=0), "bad argument"), (dict(ld=99), "bad argument"),
             (dict(tile=4097), "tile_items"), (dict(tile=-1), "tile_items"), (dict(n_items=0), "n_items"),
             (dict(n_items=2 ** 31), "n_items"))
    for kw, msg in cases:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert call(R=(2 ** 31 - 1) // 100) == _lib.ERR_ARG and "null argument" in _lib.last_error()   # the largest R that passes
    with pytest.raises(RuntimeError):
        _lib.check(call(top=257))


def test_blend_points_argument_checks():
    from seoul_tourism_recommendation_ngcf_amd import engine
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)  # noqa: E731
    pref, rowptr, rows = i64(6, 100), i64(3), i64(4)
    ok = dict(points=100, top=10)
    with pytest.raises(RuntimeError, match="ROCm device"):                       # CPU tensors: no fallback, and no launch
        engine.blend_points(pref, rowptr, rows, 100, **ok)
    for kw, exc, msg in ((dict(top=0), ValueError, "top=0"), (dict(top=257), ValueError, "top=257"),
                         (dict(points=0), ValueError, "points=0"), (dict(points=1025), ValueError, "points=1025"),
                         (dict(weights=(1.0, 0.0)), ValueError, "weights"), (dict(tile_items=4097), ValueError, "tile_items"),
                         (dict(con=i64(3, 100)), ValueError, "come together"), (dict(dis_slot=i64(6)), ValueError, "come together"),
                         (dict(con=i64(3, 99), con_slot=i64(6)), ValueError, r"con must be \[S, Pl = 100\]"),
                         (dict(con=i64(3, 100), con_slot=i64(5)), ValueError, r"con_slot must be \[R = 6\]"),
                         (dict(dis=i64(100), dis_slot=i64(6)), ValueError, r"dis must be \[S, Pl = 100\]"),
                         (dict(dis=i64(1, 100), dis_slot=i64(6, 1)), ValueError, r"dis_slot must be \[R = 6\]"),
                         (dict(item_mask=torch.ones(99, dtype=torch.uint8)), ValueError, "item_mask must be"),
                         (dict(item_mask=torch.ones(100)), TypeError, "uint8 or bool"),
                         (dict(con=i64(3, 100).int(), con_slot=i64(6)), TypeError, "con must be int64"),
                         (dict(con=i64(3, 100), con_slot=i64(6).int()), TypeError, "con_slot must be int64")):
        with pytest.raises(exc, match=msg):
            engine.blend_points(pref, rowptr, rows, 100, **{**ok, **kw})
    with pytest.raises(TypeError, match="pref must be int64"):
        engine.blend_points(pref.int(), rowptr, rows, 100, **ok)
    with pytest.raises(TypeError, match="col_rows must be int64"):
        engine.blend_points(pref, rowptr, rows.int(), 100, **ok)
    with pytest.raises(ValueError, match="pref must be"):                        # lists longer than the point ranks
        engine.blend_points(pref, rowptr, rows, 100, points=99)
    with pytest.raises(ValueError, match="pref must be"):
        engine.blend_points(pref[0], rowptr, rows, 100, **ok)
    with pytest.raises(ValueError, match="col_rowptr"):
        engine.blend_points(pref, rowptr[:0], rows, 100, **ok)
    with pytest.raises(ValueError, match="n_items"):
        engine.blend_points(pref, rowptr, rows, 2 ** 31, **ok)
    big = torch.zeros((1, 1), dtype=torch.int64).expand(2 ** 31, 1)              # R * P = 2^31 without the memory
    with pytest.raises(ValueError, match="2\\^31"):
        engine.blend_points(big, rowptr, rows, 100, points=1)


def test_recommend_is_exported():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    assert "recommend" in pkg.__all__ and pkg.recommend.blended_ranking and pkg.recommend.demo_views
    sig = inspect.signature(pkg.recommend.blended_ranking)
    assert list(sig.parameters) == ["model", "user_ids", "features", "year", "columns", "weights", "congestion", "congestion_slot",
                                    "distance", "distance_slot", "item_mask", "top", "points", "exclude", "row_chunk", "return_table"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["weights"] == (1.0, 0.0, 0.0) and d["top"] == 10 and d["points"] == 100 and d["row_chunk"] == 65536
    assert d["return_table"] is False and sig.parameters["features"].kind is inspect.Parameter.KEYWORD_ONLY


def test_demo_views_on_a_hand_written_party():
    """2 members x 3 days, request rows in the order the demo builds them (day by day, member by member).  The reference gives an id
    per (age, sex, month, day) (user_dict, demo.py:384-388): on day 2 both members have the same age and sex, so rows 2 and 3 share
    an id."""
    from seoul_tourism_recommendation_ngcf_amd import recommend
    #                       d1 A  d1 B  d2 A  d2 B  d3 A  d3 B
    uid = torch.tensor([40, 17, 23, 23, 5, 31])
    age = torch.tensor([25, 35, 30, 30, 25, 35])
    sex = torch.tensor([0, 1, 1, 1, 0, 1])
    month = torch.tensor([7, 7, 7, 7, 8, 8])
    day = torch.tensor([30, 30, 31, 31, 1, 1])
    rowptr, rows, labels = recommend.demo_views(uid, age, sex, month, day)
    assert labels == [("user", 5), ("user", 17), ("user", 23), ("user", 31), ("user", 40),
                      ("day", 7, 30), ("day", 7, 31), ("day", 8, 1),
                      ("person", 25, 0), ("person", 30, 1), ("person", 35, 1),
                      ("all",)]
    assert rowptr.dtype == torch.int64 and rows.dtype == torch.int64
    assert rowptr.tolist() == [0, 1, 2, 4, 5, 6, 8, 10, 12, 14, 16, 18, 24]
    assert rows.tolist() == [4, 1, 2, 3, 5, 0,
                             0, 1, 2, 3, 4, 5,
                             0, 4, 2, 3, 1, 5,
                             0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError, match="entries of a feature"):
        recommend.demo_views(uid, age[:5], sex, month, day)
    e = torch.zeros(0, dtype=torch.int64)
    rowptr, rows, labels = recommend.demo_views(e, e, e, e, e)
    assert rowptr.tolist() == [0] and rows.numel() == 0 and labels == []
