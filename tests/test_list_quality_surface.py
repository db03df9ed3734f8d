"""CPU tests of the beyond-accuracy list figures' surface: `engine.lists` exists beside the flat namespace, its argument checks
raise before the device is touched (every tensor here lives on the CPU), and the three entry points are declared, bound and
compiled."""
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

NAMES = ("ngcf_list_exposure", "ngcf_exposure_summary", "ngcf_list_diversity_f32")


def _lists_module():
    from seoul_tourism_recommendation_ngcf_amd import engine
    return engine.lists


def test_module_is_reached_by_its_name_and_stays_out_of_the_flat_namespace():
    from seoul_tourism_recommendation_ngcf_amd import engine, evaluate
    lists = _lists_module()
    for name in ("exposure_counts", "exposure_summary", "exposure_summary_launch", "exposure_figures", "list_diversity",
                 "diversity_from_sums"):
        assert callable(getattr(lists, name)) and not hasattr(engine, name)
    assert "engine.lists" in engine.__doc__
    assert list(inspect.signature(lists.exposure_counts).parameters)[:4] == ["top_idx", "n_items", "k", "out"]
    assert list(inspect.signature(lists.exposure_summary).parameters) == ["counts", "popularity", "n_user"]
    assert list(inspect.signature(lists.list_diversity).parameters)[:5] == ["top_idx", "item_emb", "ks", "per_user", "sums"]
    assert list(inspect.signature(evaluate.list_quality).parameters) == ["model", "train", "ks", "year_idx", "user_ids", "user_chunk",
                                                                         "lists"]


def test_constants_equal_the_sources():
    lists = _lists_module()
    src = open(os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc", "list_quality.hip")).read()
    header = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert lists.EXPOSURE_LDS_ITEMS == int(re.search(r"^#define\s+NGCF_EXPOSURE_LDS_ITEMS\s+(\d+)\b", src, flags=re.M).group(1))
    assert lists.DIVERSITY_K_MAX == int(re.search(r"^#define\s+NGCF_LIST_DIV_K_MAX\s+(\d+)\b", header, flags=re.M).group(1)) == 64
    assert lists.DIVERSITY_KS_MAX == int(re.search(r"^#define\s+NGCF_LIST_DIV_KS_MAX\s+(\d+)\b", src, flags=re.M).group(1)) == 8
    assert lists.EXPOSURE_LDS_ITEMS * 4 * 2 <= 160 * 1024       # two workgroups' tables in a CU's LDS


def test_entry_points_are_declared_bound_and_exported():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.PROTOTYPES
    assert any(p.endswith("list_quality.hip") for p in _build.SOURCES)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NAMES)
    blob = open(_lib.lib_path(), "rb").read()
    assert b"list_diversity_kernel" in blob and b"list_exposure_kernel" in blob and b"exposure_summary_kernel" in blob
    # host-side argument errors of the C entry points: nothing is launched
    assert lib.ngcf_list_exposure(None, 4, 1, 8, 10, None, None, None) == _lib.ERR_ARG and "list_exposure" in _lib.last_error()
    assert lib.ngcf_exposure_summary(None, None, None, 10, 0, None, None) == _lib.ERR_ARG and "exposure_summary" in _lib.last_error()
    assert lib.ngcf_list_diversity_f32(None, 4, 1, 4, None, 4, 10, 4, None, 0, None, None, None, None) == _lib.ERR_ARG
    assert "list_diversity" in _lib.last_error()


def test_the_header_states_the_order_the_oracle_restates():
    header = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    for words in ("ONE ascending-k fmaf chain from 0", "added in ascending a from 0.0", "added in ascending b from 0.0",
                  "every fp64 operation rounded once, no FMA", "never used as an index"):
        assert words in header, words


def test_an_entry_is_compared_with_n_items_before_it_is_an_index():
    """By reading the code, not by a run: in each kernel that takes list entries the comparison `>= n_items` stands before the first
    expression that indexes with the entry."""
    src = open(os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc", "list_quality.hip")).read()
    expo = src[src.index("void list_exposure_kernel"):src.index('extern "C" int ngcf_list_exposure')]
    assert expo.index("if (id >= n_items)") < expo.index("expo_tab[id]") < expo.index("counts[id]")
    assert expo.index("if (id < 0) continue;") < expo.index("if (id >= n_items)")
    div = src[src.index("void list_diversity_kernel"):src.index('extern "C" int ngcf_list_diversity_f32')]
    assert div.index("if (v >= n_items)") < div.index("id = (int32_t)v") < div.index("sid[lane] = id") < div.index("(int64_t)it * ldi")
    assert div.count("(int64_t)it * ldi") == 2 and div.count("if (it >= 0 && kk < D)") + div.count("(it >= 0 && kk < D) ?") == 2


def test_exposure_checks_raise_on_the_host():
    lists = _lists_module()
    top = torch.zeros((4, 8), dtype=torch.int64)
    with pytest.raises(TypeError, match="int64"):
        lists.exposure_counts(top.int(), 10)
    with pytest.raises(ValueError, match=r"\[B, k\]"):
        lists.exposure_counts(top[0], 10)
    for k in (0, 9):
        with pytest.raises(ValueError, match="k="):
            lists.exposure_counts(top, 10, k=k)
    for n in (0, 2 ** 31):
        with pytest.raises(ValueError, match="n_items"):
            lists.exposure_counts(top, n)
    for bad in (torch.zeros(10, dtype=torch.int32), torch.zeros(9, dtype=torch.int64), torch.zeros((10, 1), dtype=torch.int64)):
        with pytest.raises(ValueError, match="out must be"):
            lists.exposure_counts(top, 10, out=bad)
    with pytest.raises(RuntimeError, match="ROCm device"):
        lists.exposure_counts(top, 10)


def test_summary_checks_raise_on_the_host():
    lists = _lists_module()
    counts = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(TypeError, match="counts must be int64"):
        lists.exposure_summary(counts.int())
    with pytest.raises(TypeError, match="popularity must be int64"):
        lists.exposure_summary(counts, counts.double(), 5)
    with pytest.raises(ValueError, match="n_items"):
        lists.exposure_summary(counts[:0])
    with pytest.raises(ValueError, match="popularity must be"):
        lists.exposure_summary(counts, counts[:9], 5)
    for n_user in (None, 0):
        with pytest.raises(ValueError, match="n_user"):
            lists.exposure_summary(counts, counts, n_user)
    with pytest.raises(RuntimeError, match="ROCm device"):
        lists.exposure_summary(counts)


def test_diversity_checks_raise_on_the_host():
    lists = _lists_module()
    top = torch.zeros((4, 80), dtype=torch.int64)
    emb = torch.zeros((10, 16))
    with pytest.raises(ValueError, match="K=65"):
        lists.list_diversity(top, emb, (20, 65))                # above the kernel's limit although the list is longer
    with pytest.raises(ValueError, match="K=21 above the list length k=20"):
        lists.list_diversity(top[:, :20], emb, (21,))
    with pytest.raises(ValueError, match="K=1 "):
        lists.list_diversity(top, emb, (1,))
    with pytest.raises(ValueError, match="cut-offs, got 9"):
        lists.list_diversity(top, emb, range(2, 11))
    with pytest.raises(ValueError, match="cut-offs, got 0"):
        lists.list_diversity(top, emb, ())
    with pytest.raises(TypeError, match="top_idx must be int64"):
        lists.list_diversity(top.int(), emb, (20,))
    with pytest.raises(TypeError, match="item_emb must be float32"):
        lists.list_diversity(top, emb.double(), (20,))
    with pytest.raises(ValueError, match="item_emb must be"):
        lists.list_diversity(top, emb[0], (20,))
    with pytest.raises(RuntimeError, match="ROCm device"):
        lists.list_diversity(top, emb, (20,))
    with pytest.raises(ValueError, match="3 slots for 1 cut-offs"):
        lists.diversity_from_sums(torch.zeros(3, dtype=torch.float64), (20,))


def test_figures_from_six_words():
    """The host half: Gini as one rounding of the exact fraction, NaN figures for an empty histogram, the status bits as exceptions."""
    import math
    import struct
    from fractions import Fraction
    lists = _lists_module()
    bits = lambda x: struct.unpack("<q", struct.pack("<d", x))[0]          # noqa: E731
    fig = lists.exposure_figures([2, 10, 3 * 1 + 4 * 9, 0, bits(9 * math.log2(9)), bits(12.5)], 4)
    assert fig["coverage"] == 0.5 and fig["gini"] == float(Fraction(2 * 39, 40) - Fraction(5, 4))
    assert fig["entropy"] == math.log2(10) - 9 * math.log2(9) / 10 and fig["novelty"] == 1.25
    empty = lists.exposure_figures([0, 0, 0, 0, 0, 0], 4)
    assert empty["covered"] == 0 and all(math.isnan(empty[n]) for n in ("coverage", "gini", "entropy", "novelty"))
    with pytest.raises(OverflowError):
        lists.exposure_figures([1, 2 ** 60, 0, lists.SUMMARY_OVERFLOW, 0, 0], 4)
    with pytest.raises(RuntimeError, match="negative"):
        lists.exposure_figures([1, 1, 1, lists.SUMMARY_NEGATIVE, 0, 0], 4)
