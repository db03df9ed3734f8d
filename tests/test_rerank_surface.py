"""CPU tests of the diversifying re-rank's surface: `engine.lists.mmr_rerank` and `recommend.diversified_ranking` exist where they
belong, their argument checks raise before the device is touched (every tensor here lives on the CPU), and the entry point is
declared, bound, compiled and refuses bad arguments before any launch."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT


def _lists_module():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.lists


def test_names_live_in_engine_lists_and_recommend_not_in_the_flat_namespace():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    from seoul_tourism_recommendation_ngcf_amd import engine
    lists = _lists_module()
    assert callable(lists.mmr_rerank) and not hasattr(engine, "mmr_rerank") and not hasattr(engine, "MMR_POOL_MAX")
    sig = inspect.signature(lists.mmr_rerank)
    assert list(sig.parameters) == ["pool_idx", "relevance", "item_emb", "top", "lam", "normalize", "return_slots", "return_keys", "status"]
    assert [sig.parameters[p].default for p in ("lam", "normalize", "return_slots", "return_keys", "status")] == [0.7, True, False, False, None]
    sig = inspect.signature(pkg.recommend.diversified_ranking)
    assert list(sig.parameters) == ["model", "user_ids", "train", "lam", "pool", "top", "year_idx", "normalize", "user_chunk"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for name, p in sig.parameters.items() if name not in ("model", "user_ids"))
    assert {n: sig.parameters[n].default for n in ("train", "lam", "pool", "top", "year_idx", "normalize", "user_chunk")} == {
        "train": None, "lam": 0.7, "pool": 64, "top": 10, "year_idx": 0, "normalize": True, "user_chunk": 65536}
    assert "mmr_rerank(out_items, out_ratings, model.all_items_emb, top)" in pkg.recommend.diversified_ranking.__doc__
    # the neighbours keep their signatures
    assert list(inspect.signature(pkg.evaluate.list_quality).parameters) == ["model", "train", "ks", "year_idx", "user_ids", "user_chunk",
                                                                             "lists"]
    assert list(inspect.signature(pkg.recommend.blended_ranking).parameters)[:2] == ["model", "user_ids"]


def test_the_constant_equals_the_header():
    header = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert _lists_module().MMR_POOL_MAX == int(re.search(r"^#define\s+NGCF_LIST_MMR_POOL_MAX\s+(\d+)\b", header, flags=re.M).group(1)) == 64
    for words in ("diversified top lists", "1.0 - lam is formed once", "A NaN key ranks below every other key, -inf included",
                  "among equal keys, and among NaN keys, the lowest slot wins", "never used as an index"):
        assert words in header, words


def _call(lib, **kw):
    """ngcf_list_mmr_f32 with small valid scalars and non-null host addresses that are never dereferenced: every case below is
    refused before anything is launched."""
    a = dict(pool=0x10000, ld=8, rel=0x20000, rel_f64=0, ldr=8, B=1, n=8, top=4, items=0x30000, ldi=16, n_items=10, D=16, lam=0.5,
             normalize=1, out_items=0x40000, out_slots=None, out_keys=None, status=0x50000)
    a.update(kw)
    return lib.ngcf_list_mmr_f32(a["pool"], a["ld"], a["rel"], a["rel_f64"], a["ldr"], a["B"], a["n"], a["top"], a["items"], a["ldi"],
                                 a["n_items"], a["D"], a["lam"], a["normalize"], a["out_items"], a["out_slots"], a["out_keys"], a["status"],
                                 None)


def test_entry_point_is_declared_bound_exported_and_checks_its_arguments():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert re.search(r"\bint ngcf_list_mmr_f32\(", header) and header.index("ngcf_list_diversity_f32(") < header.index("ngcf_list_mmr_f32(")
    assert _lib.PROTOTYPES["ngcf_list_mmr_f32"] == (C.c_int, [
        C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
        C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    assert any(p.endswith("list_rerank.hip") for p in _build.SOURCES)
    lib = _lib.load()
    assert hasattr(lib, "ngcf_list_mmr_f32") and int(lib.ngcf_version()) == _lib.ABI_VERSION == 11
    assert b"list_mmr_kernel" in open(_lib.lib_path(), "rb").read()
    bad = [dict(pool=None), dict(rel=None), dict(items=None), dict(out_items=None), dict(status=None),
           dict(n=0), dict(n=65, ld=65, ldr=65), dict(top=0), dict(top=9), dict(lam=float("nan")), dict(lam=-0.001), dict(lam=1.001),
           dict(D=0), dict(D=17), dict(n_items=0), dict(n_items=2 ** 31), dict(B=-1), dict(ld=7), dict(ldr=7)]
    for kw in bad:
        assert _call(lib, **kw) == _lib.ERR_ARG and "list_mmr" in _lib.last_error(), kw
    with pytest.raises(RuntimeError, match="list_mmr"):
        _lib.check(_call(lib, top=9))
    assert _call(lib, B=0) == _lib.OK                              # nothing to do: nothing is launched, no pointer is read


def test_mmr_rerank_checks_raise_on_the_host():
    lists = _lists_module()
    pool = torch.zeros((4, 8), dtype=torch.int64)
    rel = torch.zeros((4, 8))
    emb = torch.zeros((10, 16))
    with pytest.raises(TypeError, match="pool_idx must be int64"):
        lists.mmr_rerank(pool.int(), rel, emb, 4)
    with pytest.raises(TypeError, match="relevance must be float32 or float64"):
        lists.mmr_rerank(pool, rel.half(), emb, 4)
    with pytest.raises(TypeError, match="item_emb must be float32"):
        lists.mmr_rerank(pool, rel, emb.double(), 4)
    with pytest.raises(ValueError, match=r"pool_idx must be \[B, n\]"):
        lists.mmr_rerank(pool[0], rel[0], emb, 4)
    with pytest.raises(ValueError, match="relevance must be"):
        lists.mmr_rerank(pool, rel[:, :7], emb, 4)
    with pytest.raises(ValueError, match="item_emb must be"):
        lists.mmr_rerank(pool, rel, emb[0], 4)
    wide = torch.zeros((2, 65), dtype=torch.int64)
    with pytest.raises(ValueError, match="n=65"):
        lists.mmr_rerank(wide, torch.zeros((2, 65)), emb, 4)
    for top in (0, 9):
        with pytest.raises(ValueError, match="top="):
            lists.mmr_rerank(pool, rel, emb, top)
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam="):
            lists.mmr_rerank(pool, rel, emb, 4, lam=lam)
    for relevance in (rel, rel.double()):                           # everything else in order: only the device is missing
        with pytest.raises(RuntimeError, match="ROCm device"):
            lists.mmr_rerank(pool, relevance, emb, 4)


def test_diversified_ranking_checks_raise_before_the_model_is_touched():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    users = torch.arange(3)
    for kw, words in ((dict(pool=0), "pool=0"), (dict(pool=65), "pool=65"), (dict(top=0), "top=0"), (dict(pool=8, top=9), "top=9"),
                      (dict(lam=-0.5), "lam="), (dict(lam=float("nan")), "lam="), (dict(user_chunk=0), "user_chunk=0")):
        with pytest.raises(ValueError, match=words):
            pkg.recommend.diversified_ranking(None, users, **kw)
    with pytest.raises(TypeError, match="user_ids"):
        pkg.recommend.diversified_ranking(None, users.float())
