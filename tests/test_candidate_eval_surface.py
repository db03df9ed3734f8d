"""Host-side surface of the candidate-list evaluation: the C ABI symbol, argument checks before any launch, the means of a sums vector."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_eval_candidates():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ngcf_eval_candidates_f32\s*\(", text)
    lib = _lib.load()
    assert hasattr(lib, "ngcf_eval_candidates_f32") and "ngcf_eval_candidates_f32" in _lib.PROTOTYPES
    assert any(p.endswith("eval_candidates.hip") for p in _build.SOURCES)
    assert b"eval_candidates_kernel" in open(_lib.lib_path(), "rb").read()       # a gfx950 kernel of its own, not a library call
    assert int(lib.ngcf_version()) == _lib.ABI_VERSION


def test_c_abi_limits_are_errors_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()

    def call(C_=20, ks=(10,), hit_k=3, repeat=None, D=8):
        arr = (C.c_int32 * max(len(ks), 1))(*ks)
        return lib.ngcf_eval_candidates_f32(None, D, 4, None, D, 9, D, None, None, C_, 5, C_, None, arr, len(ks), hit_k, 0.025, 25.0,
                                            C_ if repeat is None else repeat, None, None, None, None, None)
    assert call() == _lib.ERR_ARG and "null argument" in _lib.last_error()       # everything else in range: only the pointers are missing
    for kw, msg in ((dict(C_=1025), "outside [1, 1024]"), (dict(C_=0), "outside [1, 1024]"), (dict(ks=(21,)), "out of range"),
                    (dict(ks=(0,)), "out of range"), (dict(hit_k=21), "out of range"), (dict(hit_k=0), "out of range"),
                    (dict(ks=tuple(range(1, 10))), "cut-offs"), (dict(repeat=2), "user_repeat"), (dict(D=0), "bad argument")):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    with pytest.raises(RuntimeError):
        _lib.check(call(C_=1025))


def test_eval_candidates_argument_checks():
    from seoul_tourism_recommendation_ngcf_amd import engine
    u, items = torch.zeros(4, 8), torch.zeros(9, 8)
    ids, cand = torch.zeros(3, dtype=torch.int64), torch.zeros((3, 5), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device"):                       # CPU tensors: no fallback
        engine.eval_candidates(u, items, ids, cand, ks=(5,))
    for bad in (dict(ks=(6,)), dict(ks=(0,)), dict(ks=(3,), hit_k=6)):           # k > C: what torch.topk raises there
        with pytest.raises(RuntimeError, match="out of range"):
            engine.eval_candidates(u, items, ids, cand, **{"ks": (5,), **bad})
    with pytest.raises(ValueError, match="1024"):
        engine.eval_candidates(u, items, ids, torch.zeros((3, 1025), dtype=torch.int64), ks=(5,))
    with pytest.raises(TypeError, match="int64"):
        engine.eval_candidates(u, items, ids.int(), cand, ks=(5,))
    with pytest.raises(TypeError, match="int64"):
        engine.eval_candidates(u, items, ids, cand.int(), ks=(5,))
    with pytest.raises(ValueError, match="ratings"):
        engine.eval_candidates(u, items, ids, cand, ratings=torch.zeros(4), ks=(5,))
    with pytest.raises(ValueError, match="user_repeat"):
        engine.eval_candidates(u, items, ids, cand, ks=(5,), user_repeat=2)
    with pytest.raises(ValueError, match="cut-offs"):
        engine.eval_candidates(u, items, ids, cand, ks=(1,) * 9)
    with pytest.raises(ValueError, match="candidates"):
        engine.eval_candidates(u, items, ids, cand[:2], ks=(5,))
    with pytest.raises(RuntimeError, match="cannot be multiplied"):
        engine.eval_candidates(u, items[:, :7], ids, cand, ks=(5,))


def test_candidate_metrics_from_sums_by_hand():
    from seoul_tourism_recommendation_ngcf_amd import engine
    # [hits@3, ndcg@5, ndcg@10, bpr, abs_err, cases]
    got = engine.candidate_metrics_from_sums(torch.tensor([3.0, 1.5, 2.5, 8.0, 2.0, 4.0], dtype=torch.float64), (5, 10), 3)
    assert got == {"bpr": 2.0, "hr@3": 0.75, "ndcg@5": 0.375, "ndcg@10": 0.625, "rmse": 0.5, "cases": 4}
    assert list(got) == ["bpr", "hr@3", "ndcg@5", "ndcg@10", "rmse", "cases"]
    empty = engine.candidate_metrics_from_sums([0.0] * 5, (10,), 1)
    assert empty == {"bpr": 0.0, "hr@1": 0.0, "ndcg@10": 0.0, "rmse": 0.0, "cases": 0}
    with pytest.raises(ValueError, match="slots"):
        engine.candidate_metrics_from_sums([0.0] * 5, (5, 10), 3)


def test_candidate_ranking_is_exported():
    import inspect
    import seoul_tourism_recommendation_ngcf_amd as pkg
    sig = inspect.signature(pkg.evaluate.candidate_ranking)
    assert list(sig.parameters) == ["model", "user_ids", "candidates", "year", "features", "ratings", "criterion", "ks", "hit_k",
                                    "user_repeat", "case_chunk", "return_scores"]
    assert sig.parameters["ks"].default == (10,) and sig.parameters["hit_k"].default == 3
    assert sig.parameters["case_chunk"].default == 65536 and sig.parameters["year"].kind is inspect.Parameter.KEYWORD_ONLY
