"""Host side of the certified two-stage ranking: `engine.shortlist` beside an unchanged flat `engine`, its signatures and defaults, the
refusals that come before any launch, the C exports and their gfx950 kernels."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT


def _mod():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.shortlist


def test_the_module_sits_beside_the_flat_namespace():
    from seoul_tourism_recommendation_ngcf_amd import engine
    sl = _mod()
    for name in ("pack_items", "rank_topk_certified", "shortlist_scores", "PackedItems", "default_pool", "beta"):
        assert hasattr(sl, name) and not hasattr(engine, name)
    assert sl.PackedItems._fields == ("bf16", "norm_up", "flags", "n_items", "D")
    assert (sl.POOL_MAX, sl.D_MAX, sl.K_STEP) == (256, 4096, 16) and sl.RANK_K_MAX == engine.RANK_K_MAX
    assert [sl.default_pool(k) for k in (1, 32, 33, 256)] == [128, 128, 256, 256]
    assert sl.beta(512) == 2.0 ** -7 + 2.0 ** -16 + 2050 * 2.0 ** -24


def test_signatures_and_defaults():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    sl = _mod()
    assert str(inspect.signature(sl.pack_items)) == "(item_emb: 'torch.Tensor') -> 'PackedItems'"
    p = inspect.signature(sl.rank_topk_certified).parameters
    assert list(p) == ["user_emb", "item_emb", "k", "user_ids", "exclude", "status", "packed", "pool", "fallback", "return_certified"]
    assert [p[n].default for n in list(p)[3:]] == [None, None, None, None, None, True, False]
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("packed", "pool", "fallback", "return_certified"))
    assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(p)[:6])
    assert "read-back" in sl.rank_topk_certified.__doc__ and "fallback=False" in sl.rank_topk_certified.__doc__
    f = inspect.signature(pkg.evaluate.full_ranking).parameters
    assert list(f)[-2:] == ["prefilter", "pool"] and all(f[n].kind is inspect.Parameter.KEYWORD_ONLY and f[n].default is None
                                                         for n in ("prefilter", "pool"))
    assert list(f)[:7] == ["model", "train", "test", "ks", "year_idx", "users", "user_chunk"] and "read-back per chunk" in pkg.evaluate.full_ranking.__doc__


def test_refusals_come_before_any_launch():
    """On host tensors: whatever is wrong with the sizes is said before the device is asked for."""
    import seoul_tourism_recommendation_ngcf_amd as pkg
    sl = _mod()
    u, items = torch.zeros(5, 16), torch.zeros(300, 16)
    for bad_k in (0, 301):
        with pytest.raises(RuntimeError, match="out of range"):
            sl.rank_topk_certified(u, items, bad_k)
    with pytest.raises(RuntimeError, match="recommend_topk"):
        sl.rank_topk_certified(u, items, 257)
    with pytest.raises(RuntimeError, match="cannot be multiplied"):
        sl.rank_topk_certified(u, items[:, :15], 1)
    for bad_pool in (19, 257, 0):
        with pytest.raises(ValueError, match="pool="):
            sl.rank_topk_certified(u, items, 20, pool=bad_pool)
    with pytest.raises(RuntimeError, match="expected float32"):
        sl.rank_topk_certified(u.double(), items.double(), 5)
    with pytest.raises(RuntimeError, match="expected float32"):
        sl.pack_items(items.half())
    with pytest.raises(RuntimeError, match="D=4097"):
        sl.pack_items(torch.zeros(2, 4097))
    packed = sl.PackedItems(torch.zeros(300, 32, dtype=torch.bfloat16), torch.zeros(300), torch.zeros(1, dtype=torch.int32), 300, 17)
    with pytest.raises(ValueError, match="packed"):
        sl.rank_topk_certified(u, items, 5, packed=packed)
    with pytest.raises(ValueError, match="packed"):
        sl.rank_topk_certified(u, items, 5, packed=packed._replace(D=16, n_items=299))
    with pytest.raises(RuntimeError, match="ROCm device"):                        # sizes in order: only now the device
        sl.rank_topk_certified(u, items, 5, packed=packed._replace(D=16))
    with pytest.raises(ValueError, match="prefilter"):
        pkg.evaluate.full_ranking(None, None, None, prefilter="fp8")


def test_header_declares_and_library_exports_the_family():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    names = ("ngcf_rank_pack_items", "ngcf_rank_prefilter_workspace_bytes", "ngcf_rank_shortlist_bf16", "ngcf_rank_rescore")
    lib = _lib.load()
    for name in names:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert header.index("ngcf_rank_topk_f32(") < header.index("ngcf_rank_pack_items(") < header.index("ngcf_rank_positions_f32(")
    for words in ("beta = 2^-7 + 2^-16 + (4 D + 2) 2^-24", "ub = fmaf(bu, ni, s~)", "[2^-40, 2^40]", "#define NGCF_RANK_POOL_MAX 256",
                  "#define NGCF_RANK_PREFILTER_KSTEP 16", "#define NGCF_RANK_PREFILTER_DMAX 4096"):
        assert words in header, words
    assert _lib.PROTOTYPES["ngcf_rank_prefilter_workspace_bytes"] == (C.c_int64, [C.c_int64, C.c_int64, C.c_int, C.c_int])
    assert any(p.endswith("rank_prefilter.hip") for p in _build.SOURCES)
    blob = open(_lib.lib_path(), "rb").read()
    for kernel in (b"rank_pack_items_kernel", b"rank_shortlist_kernel", b"rank_rescore_kernel", b"rank_user_bounds_kernel"):
        assert kernel in blob
    # host-side answers: sizes out of range have no workspace; one split needs the bounds alone, two splits their lists too
    ws = lib.ngcf_rank_prefilter_workspace_bytes
    assert ws(40, 700, 64, 257) == ws(40, 700, 4097, 64) == ws(-1, 700, 64, 64) == ws(40, 0, 64, 64) == -1
    assert ws(40, 700, 64, 128) == 256 and ws(40, 4500, 64, 64) == 256 + 2 * 2 * 40 * 64 * 4
    # argument errors of the entry points, before any launch
    for rc in (lib.ngcf_rank_pack_items(None, 16, 10, 16, None, None, None, None),
               lib.ngcf_rank_shortlist_bf16(None, 16, None, 5, 5, None, None, 300, 16, 300, None, None, 0, None, None, None, None, None, None, 0, None),
               lib.ngcf_rank_rescore(None, 16, None, 5, 5, None, 16, 300, 16, 65, 64, None, None, None, None, None, None, None, None)):
        assert rc == _lib.ERR_ARG and b"rank_" in lib.ngcf_last_error()


def test_the_selection_scheme_stands_once():
    """By reading the sources: compaction, row lookup and the merge of the split lists are rank_device.h's, used by both kernels."""
    csrc = os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("rank.hip", "rank_prefilter.hip", "rank_device.h")}
    for words in ("void rank_compact(", "int64_t rank_user(", "void rank_merge_kernel("):
        assert [f for f, t in sorted(text.items()) if words in t] == ["rank_device.h"], words
    for f in ("rank.hip", "rank_prefilter.hip"):
        assert "rank_compact<CAPP>(" in text[f] and "rank_merge_kernel<<<" in text[f] and "rank_item_split(" in text[f]
    assert "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in text["rank_prefilter.hip"]
